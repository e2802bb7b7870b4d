// Spectral distances at one short-time resolution (include/vtts_spectral.h): spectral convergence, log-magnitude L1 and log-spectral distance
// of a signal under test against its reference, and optionally both magnitude spectrograms; batched and ragged.
//
// Two launches per VTTS_SPECTRAL_ROWS_PER_LAUNCH rows, each anchored at the row's own first sample:
//
//   spectral_frames_k<NFFT>  workgroup = F consecutive frames of one row, one wave per frame (F: vtts_spectral.h).
//     1. stage: the (F - 1) hop + NFFT samples the frames cover, of x and of y, once, into LDS (PCM16 scaled by 2^-15 on the way),
//        reflected at the ROW'S OWN ends.  The frames' overlap (NFFT / hop: 8.5x at the default resolutions) is served from LDS.
//     2. per signal, x then y, through the same code: the windowed frame as H = NFFT / 2 complex points z[n] = v[2n] + i v[2n+1], a Stockham
//        autosort transform in radix-8 and radix-4 passes (128 = 8.4.4, 256 = 8.8.4, 512 = 8.8.8, 1024 = 8.8.4.4).  Pass with radix R after
//        Ns = the product of the radices before it, butterfly j = 0 .. H / R - 1:
//            v[q] = in[j + q H / R] W_(Ns R)^(q (j mod Ns)),  V = DFT_R(v),  out[(j / Ns) Ns R + (j mod Ns) + q Ns] = V[q].
//        A lane owns butterflies j = lane + 64 m and keeps their points in registers, so a pass runs in place: every read of the wave's
//        exchange buffer comes before any write, separated by a compiler-only wave fence (the LDS keeps one wave's accesses in order:
//        mel.hip).  The first pass reads the staged span and multiplies by the window; the last leaves Z in natural order.
//        Entry i of the exchange buffer lives at i + i / 8 (mel.hip's XROW = 72 in one formula): the radix-8 first pass writes
//        out[8 j + q], which would put a half-wave's 32 ds_write_b64 on 4 bank pairs; at stride 9 they take 32 distinct ones.  The second
//        pass (Ns = 8) writes 8 consecutive entries per group of 72: 16 dwords apart, distinct again.  Later passes and every read run
//        over consecutive entries.
//     3. split step to bins 0 .. H (lane pairs bin k with bin H - k), P = max(re^2 + im^2, 1e-7); x's powers wait in registers for y's.
//        The terms and their sums are fp64 in the header's order; with mags_dev the square roots are stored on the way.
//     4. the F frames' sums meet in LDS; threads 0 .. 3 add those below T in ascending order, one sum each: four fp64 partials.
//   spectral_finish_k        one wave per row: the partials in the header's order, the three figures and T.
//
// Twiddles and window come from the packed blob (computed in double on the host, rounded once); there is no sin / cos in the kernels.
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>
#include <vector>

#include "../../include/vtts_audio.h"
#include "../../include/vtts_hifigan.h"
#include "../../include/vtts_spectral.h"
#include "vtts_internal.h"

// x and y must come out of the same arithmetic whichever kernel instance (fp32 or PCM16 input) and whichever turn of the signal loop runs it:
// every operation of this file is rounded on its own, no a * b + c becomes an FMA (as in stoi.hip).
#pragma clang fp contract(off)

using vtts::check_blob;
using vtts::failf;
using vtts::upload_blob;

namespace {

constexpr int ROWS_PER_LAUNCH = 128;
static_assert(ROWS_PER_LAUNCH == VTTS_SPECTRAL_ROWS_PER_LAUNCH, "the header states the split");
constexpr int MAX_F = VTTS_SPECTRAL_MAX_FRAMES_PER_BLOCK;
constexpr float P_FLOOR = 1e-7f;

__host__ __device__ constexpr int pad8(int i) { return i + (i >> 3); }  // where entry i of an exchange buffer lives
constexpr int even(int n) { return (n + 1) & ~1; }

// LDS of one workgroup of F frames, in bytes, in the order of the header's table (and of the kernel's carve-up)
size_t lds_bytes(int n_fft, int hop, int F) {
    const int H = n_fft / 2;
    return (size_t)32 * F + (size_t)8 * H + (size_t)8 * (H / 2 + 2) + (size_t)2 * 4 * even((F - 1) * hop + n_fft) + (size_t)8 * F * pad8(H);
}
int frames_per_block(int n_fft, int hop) {
    int F = n_fft == 2048 ? VTTS_SPECTRAL_MAX_FRAMES_PER_BLOCK_2048 : MAX_F;
    while (F > 1 && lds_bytes(n_fft, hop, F) > VTTS_SPECTRAL_LDS_BUDGET) --F;
    return F;
}

struct SpecRows {
    int len[ROWS_PER_LAUNCH];  // samples of each row of this launch
};

struct SpecArgs {            // every pointer at the launch's first row
    const void* x;           // reference
    const void* y;           // under test
    const float* blob;       // window [n_fft] | exp(-2 pi i m / H) [H] | exp(-2 pi i k / n_fft) [H / 2 + 1]
    long long s_stride;      // samples between rows
    long long t_stride;      // frames between the two planes of mags: [rows][2][t_stride][H + 1]
    long long g_stride;      // workgroups between rows of part
    double* part;            // [rows][g_stride][4]
    float* mags;             // or nullptr
    double* sc;
    double* logmag;
    double* lsd;
    int* n_frames;
    int hop, F, span;        // span = even((F - 1) hop + n_fft): floats of one staged signal
};

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 mul_mi(float2 a) { return make_float2(a.y, -a.x); }  // -i a

// A[k] = sum_j a_j (-i)^(j k)
__device__ __forceinline__ void dft4(float2 a0, float2 a1, float2 a2, float2 a3, float2& A0, float2& A1, float2& A2, float2& A3) {
    const float2 s0 = cadd(a0, a2), d0 = csub(a0, a2), s1 = cadd(a1, a3), d1 = mul_mi(csub(a1, a3));
    A0 = cadd(s0, s1);
    A1 = cadd(d0, d1);
    A2 = csub(s0, s1);
    A3 = csub(d0, d1);
}
// in place: v[k] = sum_a v[a] exp(-2 pi i a k / R)
__device__ __forceinline__ void radix(float2 (&v)[4]) { dft4(v[0], v[1], v[2], v[3], v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ void radix(float2 (&v)[8]) {
    float2 e0, e1, e2, e3, o0, o1, o2, o3;
    dft4(v[0], v[2], v[4], v[6], e0, e1, e2, e3);
    dft4(v[1], v[3], v[5], v[7], o0, o1, o2, o3);
    const float c = 0.70710678118654752440f;
    o1 = make_float2(c * (o1.x + o1.y), c * (o1.y - o1.x));   // times W8   = (c, -c)
    o2 = mul_mi(o2);                                          // times W8^2 = -i
    o3 = make_float2(c * (o3.y - o3.x), -c * (o3.x + o3.y));  // times W8^3 = (-c, -c)
    v[0] = cadd(e0, o0), v[4] = csub(e0, o0);
    v[1] = cadd(e1, o1), v[5] = csub(e1, o1);
    v[2] = cadd(e2, o2), v[6] = csub(e2, o2);
    v[3] = cadd(e3, o3), v[7] = csub(e3, o3);
}

// A sample as fp32.  PCM16 is scaled by 2^-15 with an exponent add, not with the multiply of sample_convert.h (the same bits): staging converts x
// and y side by side, and the compiler pairs two such multiplies into a v_pk_mul_f32, which no kernel of this library may hold (build.py).
__device__ __forceinline__ float sample(const float* x, long long g) { return x[g]; }
__device__ __forceinline__ float sample(const short* x, long long g) { return ldexpf((float)x[g], -15); }

// Orders a wave's LDS writes before its later LDS reads of other lanes' data: no instruction, it only holds the compiler (mel.hip).
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the header's halvings h = 32 .. 1 (every lane ends with lane 0's bits: each step adds the same two numbers on both sides)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Butterflies a lane owns in a pass of radix R over H points
template <int H, int R>
struct Own {
    static constexpr int BF = H / R;                   // butterflies of the pass
    static constexpr int PER = BF >= 64 ? BF / 64 : 1; // ... of one lane
    static __device__ __forceinline__ bool active(int lane) { return BF >= 64 || lane < BF; }
};

// One Stockham pass in place over the wave's exchange buffer (see the head of the file).  FIRST: the input is the staged frame `fr` times the
// window values `wv` the lane holds (its own points' windows, loaded once per wave).
template <int H, int R, int NS, bool FIRST>
__device__ __forceinline__ void fft_pass(float2* xb, const float2* twH, int lane, const float* fr, const float2 (&wv)[Own<H, 8>::PER][8]) {
    using O = Own<H, R>;
    float2 v[O::PER][R];
    if (O::active(lane)) {
#pragma unroll
        for (int m = 0; m < O::PER; ++m) {
            const int j = lane + 64 * m;
#pragma unroll
            for (int q = 0; q < R; ++q) {
                const int i = j + q * O::BF;
                if constexpr (FIRST)
                    v[m][q] = make_float2(fr[2 * i] * wv[m][q].x, fr[2 * i + 1] * wv[m][q].y);
                else
                    v[m][q] = xb[pad8(i)];
            }
            if constexpr (NS > 1) {
                const int k = j & (NS - 1);
#pragma unroll
                for (int q = 1; q < R; ++q) v[m][q] = cmul(v[m][q], twH[k * q * (H / (NS * R))]);
            }
            radix(v[m]);
        }
    }
    wave_sync();
    if (O::active(lane)) {
#pragma unroll
        for (int m = 0; m < O::PER; ++m) {
            const int j = lane + 64 * m;
            const int j0 = (j / NS) * NS * R + (j & (NS - 1));
#pragma unroll
            for (int q = 0; q < R; ++q) xb[pad8(j0 + q * NS)] = v[m][q];
        }
    }
    wave_sync();
}

template <int H>
__device__ __forceinline__ void fft(float2* xb, const float2* twH, int lane, const float* fr, const float2 (&wv)[Own<H, 8>::PER][8]) {
    fft_pass<H, 8, 1, true>(xb, twH, lane, fr, wv);
    if constexpr (H == 128) {
        fft_pass<H, 4, 8, false>(xb, twH, lane, fr, wv);
        fft_pass<H, 4, 32, false>(xb, twH, lane, fr, wv);
    } else if constexpr (H == 256) {
        fft_pass<H, 8, 8, false>(xb, twH, lane, fr, wv);
        fft_pass<H, 4, 64, false>(xb, twH, lane, fr, wv);
    } else if constexpr (H == 512) {
        fft_pass<H, 8, 8, false>(xb, twH, lane, fr, wv);
        fft_pass<H, 8, 64, false>(xb, twH, lane, fr, wv);
    } else {
        static_assert(H == 1024, "n_fft is 256, 512, 1024 or 2048");
        fft_pass<H, 8, 8, false>(xb, twH, lane, fr, wv);
        fft_pass<H, 4, 64, false>(xb, twH, lane, fr, wv);
        fft_pass<H, 4, 256, false>(xb, twH, lane, fr, wv);
    }
}

template <int NFFT, typename TI>
__global__ __launch_bounds__(64 * MAX_F) void spectral_frames_k(const SpecArgs a, const SpecRows rows) {
    constexpr int H = NFFT / 2, NB = H + 1, XB = pad8(H);
    constexpr int J = (H / 2) / 64 + 1;  // bins k = lane + 64 j <= H / 2 of a lane
    extern __shared__ double lds8[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int F = a.F;
    double* red = lds8;                                          // [F][4]
    float2* twH = reinterpret_cast<float2*>(red + 4 * F);        // [H]
    float2* twN = twH + H;                                       // [H / 2 + 2]
    float* span = reinterpret_cast<float*>(twN + H / 2 + 2);     // [2][a.span]
    float2* xb = reinterpret_cast<float2*>(span + 2 * a.span) + wave * XB;

    const int b = blockIdx.y;
    const long long S = rows.len[b];  // >= H + 1 (checked on the host)
    const long long T = 1 + S / a.hop;
    const long long t0 = (long long)blockIdx.x * F;
    if (t0 >= T) return;  // block-uniform

    // this lane's window values of the first pass: issued now, so that their latency hides behind the staging
    using O1 = Own<H, 8>;
    float2 wv[O1::PER][8];
    {
        const float2* win2 = reinterpret_cast<const float2*>(a.blob);
#pragma unroll
        for (int m = 0; m < O1::PER; ++m)
#pragma unroll
            for (int q = 0; q < 8; ++q) wv[m][q] = O1::active(lane) ? win2[lane + 64 * m + q * O1::BF] : make_float2(0.0f, 0.0f);
    }
    {
        const float2* t2 = reinterpret_cast<const float2*>(a.blob + NFFT);
        for (int i = tid; i < H + H / 2 + 1; i += 64 * F) (i < H ? twH[i] : twN[i - H]) = t2[i];
    }
    // ---- 1. stage: span[sig][i] = padded sample hop t0 + i = row sample hop t0 - H + i, reflected at the row's ends
#pragma unroll
    for (int sig = 0; sig < 2; ++sig) {
        const TI* x = static_cast<const TI*>(sig ? a.y : a.x) + (long long)b * a.s_stride;
        float* sp = span + sig * a.span;
        const long long g0 = t0 * a.hop - H;
        for (int i = tid; i < a.span; i += 64 * F) {
            long long g = g0 + i;
            if (g < 0) g = -g;
            if (g >= S) g = 2 * (S - 1) - g;
            g = g < 0 ? 0 : g >= S ? S - 1 : g;  // frames past the row's last (never used) stay inside the row
            sp[i] = sample(x, g);
        }
    }
    __syncthreads();

    // ---- 2./3. From here on a wave touches only its own exchange buffer.
    const long long t = t0 + wave;
    double A = 0.0, B = 0.0, C = 0.0, E = 0.0;
    if (t < T) {
        float pk[J], pn[J];  // x's powers at bins k and H - k
        const double K10 = 4.34294481903251827651;  // 10 / ln 10
#pragma unroll 1
        for (int sig = 0; sig < 2; ++sig) {  // one body for both signals
            fft<H>(xb, twH, lane, span + sig * a.span + wave * a.hop, wv);
            float* mg = a.mags ? a.mags + ((((long long)b * 2 + sig) * a.t_stride + t) * NB) : nullptr;
            float2 zk[J], zn[J];
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const int k = min(lane + 64 * j, H / 2);
                zk[j] = xb[pad8(k)];
                zn[j] = xb[pad8((H - k) & (H - 1))];
            }
            wave_sync();  // the next signal's first pass writes the buffer
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const int k = lane + 64 * j;
                if (k <= H / 2) {
                    const float2 e = make_float2(0.5f * (zk[j].x + zn[j].x), 0.5f * (zk[j].y - zn[j].y));
                    const float2 o = make_float2(0.5f * (zk[j].y + zn[j].y), -0.5f * (zk[j].x - zn[j].x));
                    const float2 w = cmul(twN[k], o);
                    const float2 p = cadd(e, w), m = csub(e, w);
                    const float Pk = fmaxf(p.x * p.x + p.y * p.y, P_FLOOR), Pn = fmaxf(m.x * m.x + m.y * m.y, P_FLOOR);
                    const bool two = k != H / 2;
                    if (mg) {
                        mg[k] = sqrtf(Pk);
                        if (two) mg[H - k] = sqrtf(Pn);
                    }
                    if (sig == 0) {
                        pk[j] = Pk, pn[j] = Pn;
                    } else {
#pragma unroll
                        for (int s = 0; s < 2; ++s) {
                            if (s == 1 && !two) break;
                            const float Px = s ? pn[j] : pk[j], Py = s ? Pn : Pk;
                            const double Mx = (double)sqrtf(Px), My = (double)sqrtf(Py);
                            const double d = My - Mx, L = log((double)Py / (double)Px), l10 = K10 * L;
                            A += d * d, B += Mx * Mx, C += 0.5 * fabs(L), E += l10 * l10;
                        }
                    }
                }
            }
        }
    }
    A = wave_sum(A), B = wave_sum(B), C = wave_sum(C), E = wave_sum(E);
    if (lane == 0) {
        red[4 * wave + 0] = A, red[4 * wave + 1] = B, red[4 * wave + 2] = C;
        red[4 * wave + 3] = sqrt(E / (double)NB);
    }
    __syncthreads();
    // ---- 4. the workgroup's partials: its frames below T in ascending order
    if (tid < 4) {
        double s = 0.0;
        for (int w = 0; w < F && t0 + w < T; ++w) s += red[4 * w + tid];
        a.part[((long long)b * a.g_stride + blockIdx.x) * 4 + tid] = s;
    }
}

template <int NB>
__global__ __launch_bounds__(64) void spectral_finish_k(const SpecArgs a, const SpecRows rows) {
    const int lane = threadIdx.x, b = blockIdx.x;
    const long long T = 1 + (long long)rows.len[b] / a.hop, G = (T + a.F - 1) / a.F;
    const double* p = a.part + (long long)b * a.g_stride * 4;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long g = lane; g < G; g += 64)
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] += p[g * 4 + i];
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = wave_sum(s[i]);
    if (lane == 0) {
        a.sc[b] = sqrt(s[0]) / sqrt(s[1]);
        a.logmag[b] = s[2] / ((double)T * (double)NB);
        a.lsd[b] = s[3] / (double)T;
        a.n_frames[b] = (int)T;
    }
}

template <int NFFT>
hipError_t launch(bool pcm, dim3 grid, int F, size_t lds, hipStream_t s, const SpecArgs& a, const SpecRows& rows, vtts::DynLdsOnce& once) {
    const void* fn = pcm ? reinterpret_cast<const void*>(&spectral_frames_k<NFFT, short>) : reinterpret_cast<const void*>(&spectral_frames_k<NFFT, float>);
    const hipError_t e = vtts::set_max_dynamic_lds(fn, VTTS_SPECTRAL_LDS_BUDGET, once);
    if (e != hipSuccess) return e;
    if (pcm)
        hipLaunchKernelGGL((spectral_frames_k<NFFT, short>), grid, dim3(64 * F), lds, s, a, rows);
    else
        hipLaunchKernelGGL((spectral_frames_k<NFFT, float>), grid, dim3(64 * F), lds, s, a, rows);
    hipLaunchKernelGGL((spectral_finish_k<NFFT / 2 + 1>), dim3(grid.y), dim3(64), 0, s, a, rows);
    return hipGetLastError();
}

}  // namespace

struct vtts_spectral {
    vtts_spectral_cfg cfg;
    int device = 0;
    int F = 1;
    std::vector<float> img;  // the packed blob's host image: window | twH | twN
    const float* blob = nullptr;
    vtts::DynLdsOnce lds_f32, lds_pcm;
};

namespace {
int64_t num_frames(const vtts_spectral* h, int64_t S) { return 1 + S / h->cfg.hop; }
int check_len(const vtts_spectral* h, const char* what, int64_t S) {
    if (S < h->cfg.n_fft / 2 + 1 || S > VTTS_SPECTRAL_MAX_SAMPLES)
        return failf(VTTS_ERR_SHAPE, "%s must be in n_fft / 2 + 1 = %d .. %d samples for the reflection padding (got %lld)", what, h->cfg.n_fft / 2 + 1,
                     VTTS_SPECTRAL_MAX_SAMPLES, (long long)S);
    return VTTS_OK;
}
}  // namespace

VTTS_API int vtts_spectral_create(const vtts_spectral_cfg* cfg, int device, vtts_spectral** out) {
    if (!cfg || !out) return failf(VTTS_ERR_INVALID, "null argument");
    const vtts_spectral_cfg& c = *cfg;
    if (c.n_fft != 256 && c.n_fft != 512 && c.n_fft != 1024 && c.n_fft != 2048)
        return failf(VTTS_ERR_INVALID, "n_fft must be 256, 512, 1024 or 2048 (got %d)", c.n_fft);
    if (c.hop < 1 || c.win < c.hop || c.win > c.n_fft)
        return failf(VTTS_ERR_INVALID, "need 1 <= hop <= win <= n_fft (got hop %d, win %d, n_fft %d)", c.hop, c.win, c.n_fft);
    auto* h = new (std::nothrow) vtts_spectral();
    if (!h) return failf(VTTS_ERR_NOMEM, "host allocation failed");
    h->cfg = c;
    h->device = device;
    h->F = frames_per_block(c.n_fft, c.hop);
    const int H = c.n_fft / 2;
    h->img.assign((size_t)c.n_fft + 2 * H + 2 * (H / 2 + 2), 0.0f);
    const double pi = 3.14159265358979323846;
    float* win = h->img.data();
    float* twH = win + c.n_fft;
    float* twN = twH + 2 * H;
    const int lead = (c.n_fft - c.win) / 2;
    for (int r = 0; r < c.win; ++r) win[lead + r] = (float)(0.5 - 0.5 * std::cos(2.0 * pi * r / c.win));
    for (int m = 0; m < H; ++m) {
        twH[2 * m] = (float)std::cos(2.0 * pi * m / H);
        twH[2 * m + 1] = (float)-std::sin(2.0 * pi * m / H);
    }
    for (int k = 0; k <= H / 2; ++k) {
        twN[2 * k] = (float)std::cos(2.0 * pi * k / c.n_fft);
        twN[2 * k + 1] = (float)-std::sin(2.0 * pi * k / c.n_fft);
    }
    *out = h;
    return VTTS_OK;
}

VTTS_API void vtts_spectral_destroy(vtts_spectral* h) { delete h; }

VTTS_API int vtts_spectral_window(const vtts_spectral* h, float* host_out) {
    if (!h || !host_out) return failf(VTTS_ERR_INVALID, "null argument");
    memcpy(host_out, h->img.data(), (size_t)h->cfg.n_fft * sizeof(float));
    return VTTS_OK;
}

VTTS_API int vtts_spectral_frames_per_block(const vtts_spectral* h, int* frames) {
    if (!h || !frames) return failf(VTTS_ERR_INVALID, "null argument");
    *frames = h->F;
    return VTTS_OK;
}

VTTS_API int vtts_spectral_num_frames(const vtts_spectral* h, int64_t n_samples, int64_t* frames) {
    if (!h || !frames) return failf(VTTS_ERR_INVALID, "null argument");
    if (int rc = check_len(h, "n_samples", n_samples)) return rc;
    *frames = num_frames(h, n_samples);
    return VTTS_OK;
}

VTTS_API int vtts_spectral_packed_bytes(const vtts_spectral* h, size_t* bytes) {
    if (!h || !bytes) return failf(VTTS_ERR_INVALID, "null argument");
    *bytes = h->img.size() * sizeof(float);
    return VTTS_OK;
}

VTTS_API int vtts_spectral_pack(vtts_spectral* h, void* dev_blob, size_t blob_bytes, void* stream) {
    if (!h) return failf(VTTS_ERR_INVALID, "null argument");
    const size_t need = h->img.size() * sizeof(float);
    if (int rc = check_blob(dev_blob, blob_bytes, need)) return rc;
    if (int rc = upload_blob(dev_blob, h->img.data(), need, static_cast<hipStream_t>(stream), "the spectral tables")) return rc;
    h->blob = static_cast<const float*>(dev_blob);
    return VTTS_OK;
}

VTTS_API int vtts_spectral_bind_packed(vtts_spectral* h, void* dev_blob, size_t blob_bytes) {
    if (!h) return failf(VTTS_ERR_INVALID, "null argument");
    if (int rc = check_blob(dev_blob, blob_bytes, h->img.size() * sizeof(float))) return rc;
    h->blob = static_cast<const float*>(dev_blob);
    return VTTS_OK;
}

VTTS_API int vtts_spectral_workspace_bytes(const vtts_spectral* h, int N, int64_t S, size_t* bytes) {
    if (!h || !bytes) return failf(VTTS_ERR_INVALID, "null argument");
    if (N <= 0) return failf(VTTS_ERR_INVALID, "N must be positive (got %d)", N);
    if (int rc = check_len(h, "S", S)) return rc;
    *bytes = (size_t)N * (size_t)((num_frames(h, S) + h->F - 1) / h->F) * 4 * sizeof(double);
    return VTTS_OK;
}

VTTS_API int vtts_spectral_forward(vtts_spectral* h, const void* ref_dev, const void* test_dev, int dtype, int N, int64_t S_stride,
                                   const int32_t* lengths, double* sc_dev, double* logmag_dev, double* lsd_dev, int32_t* n_frames_dev,
                                   float* mags_dev, int64_t T_stride, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h || !ref_dev || !test_dev || !sc_dev || !logmag_dev || !lsd_dev || !n_frames_dev || !workspace) return failf(VTTS_ERR_INVALID, "null argument");
    if (dtype != VTTS_AUDIO_F32 && dtype != VTTS_AUDIO_PCM16) return failf(VTTS_ERR_INVALID, "dtype must be VTTS_AUDIO_F32 or VTTS_AUDIO_PCM16 (got %d)", dtype);
    if (!h->blob) return failf(VTTS_ERR_STATE, "forward() before pack()/bind_packed()");
    if (N <= 0) return failf(VTTS_ERR_INVALID, "N must be positive (got %d)", N);
    if (S_stride < 0 || S_stride > 0x7fffffff) return failf(VTTS_ERR_SHAPE, "S_stride must be in 0 .. 2^31 - 1 (got %lld)", (long long)S_stride);
    int64_t longest = 0;
    for (int b = 0; b < N; ++b) {
        const int64_t len = lengths ? lengths[b] : S_stride;
        if (len > S_stride) return failf(VTTS_ERR_SHAPE, "lengths[%d] = %lld is above S_stride = %lld", b, (long long)len, (long long)S_stride);
        if (int rc = check_len(h, "every row", len)) return rc;
        if (len > longest) longest = len;
    }
    const int F = h->F, n_fft = h->cfg.n_fft, hop = h->cfg.hop;
    const int64_t tmax = num_frames(h, longest), gmax = (tmax + F - 1) / F;
    if (mags_dev && T_stride < tmax)
        return failf(VTTS_ERR_SHAPE, "T_stride = %lld is below the longest row's %lld frames", (long long)T_stride, (long long)tmax);
    const size_t need = (size_t)N * (size_t)gmax * 4 * sizeof(double);
    if (workspace_bytes < need) return failf(VTTS_ERR_NOMEM, "workspace too small: %zu < %zu bytes", workspace_bytes, need);
    if (reinterpret_cast<uintptr_t>(workspace) % 8) return failf(VTTS_ERR_INVALID, "workspace must be 8-byte aligned");

    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool pcm = dtype == VTTS_AUDIO_PCM16;
    const size_t esz = pcm ? 2 : 4, lds = lds_bytes(n_fft, hop, F);
    const size_t nb = (size_t)n_fft / 2 + 1;
    for (int r0 = 0; r0 < N; r0 += ROWS_PER_LAUNCH) {  // the rows' lengths travel as kernel arguments
        const int nr = N - r0 < ROWS_PER_LAUNCH ? N - r0 : ROWS_PER_LAUNCH;
        SpecRows rows;
        for (int b = 0; b < ROWS_PER_LAUNCH; ++b) rows.len[b] = b < nr ? (lengths ? lengths[r0 + b] : (int)S_stride) : 0;
        SpecArgs a;
        a.x = static_cast<const char*>(ref_dev) + (size_t)r0 * S_stride * esz;
        a.y = static_cast<const char*>(test_dev) + (size_t)r0 * S_stride * esz;
        a.blob = h->blob;
        a.s_stride = S_stride;
        a.t_stride = T_stride;
        a.g_stride = gmax;
        a.part = static_cast<double*>(workspace) + (size_t)r0 * gmax * 4;
        a.mags = mags_dev ? mags_dev + (size_t)r0 * 2 * T_stride * nb : nullptr;
        a.sc = sc_dev + r0;
        a.logmag = logmag_dev + r0;
        a.lsd = lsd_dev + r0;
        a.n_frames = n_frames_dev + r0;
        a.hop = hop, a.F = F, a.span = even((F - 1) * hop + n_fft);
        const dim3 grid((unsigned)gmax, (unsigned)nr);
        vtts::DynLdsOnce& once = pcm ? h->lds_pcm : h->lds_f32;
        const hipError_t e = n_fft == 256    ? launch<256>(pcm, grid, F, lds, s, a, rows, once)
                             : n_fft == 512  ? launch<512>(pcm, grid, F, lds, s, a, rows, once)
                             : n_fft == 1024 ? launch<1024>(pcm, grid, F, lds, s, a, rows, once)
                                             : launch<2048>(pcm, grid, F, lds, s, a, rows, once);
        if (e != hipSuccess) return failf(VTTS_ERR_HIP, "spectral kernel launch failed: %s", hipGetErrorString(e));
    }
    return VTTS_OK;
}
