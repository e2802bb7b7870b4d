// Spectral distances at one short-time resolution (include/vtts_spectral.h): spectral convergence, log-magnitude L1 and log-spectral distance
// of a signal under test against its reference, and optionally both magnitude spectrograms; batched and ragged.
//
// Two launches per VTTS_SPECTRAL_ROWS_PER_LAUNCH rows, each anchored at the row's own first sample:
//
//   spectral_frames_k<NFFT>  workgroup = F consecutive frames of one row, one wave per frame (F: vtts_spectral.h).
//     1. stage: the (F - 1) hop + NFFT samples the frames cover, of x and of y, once, into LDS (PCM16 scaled by 2^-15 on the way),
//        reflected at the ROW'S OWN ends.  The frames' overlap (NFFT / hop: 8.5x at the default resolutions) is served from LDS.
//     2. per signal, x then y, through the same code: the windowed frame as H = NFFT / 2 complex points z[n] = v[2n] + i v[2n+1] through
//        stockham.h's forward transform in the wave's own exchange buffer.  Steps 1 and 2 and the split step are stft_front.h's, which
//        stft.hip's forward kernel runs as well: the magnitudes stored here are that kernel's spectrum under this file's floor, bit for bit.
//     3. split step to bins 0 .. H (lane pairs bin k with bin H - k), P = max(re^2 + im^2, 1e-7); x's powers wait in registers for y's.
//        The terms and their sums are fp64 in the header's order; with mags_dev the square roots are stored on the way.
//     4. the F frames' sums meet in LDS; threads 0 .. 3 add those below T in ascending order, one sum each: four fp64 partials.
//   spectral_finish_k        one wave per row: the partials in the header's order, the three figures and T.
//
// Twiddles and window come from the packed blob (computed in double on the host, rounded once); there is no sin / cos in the kernels.
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>

#include "../../include/vtts_audio.h"
#include "../../include/vtts_hifigan.h"
#include "../../include/vtts_spectral.h"
#include "launch_rows.h"
#include "vtts_internal.h"

// x and y must come out of the same arithmetic whichever kernel instance (fp32 or PCM16 input) and whichever turn of the signal loop runs it:
// every operation of this file is rounded on its own, no a * b + c becomes an FMA (as in stoi.hip).
#pragma clang fp contract(off)

#include "stft_front.h"
#include "stft_host.h"

using vtts::failf;
using namespace vtts_stft_front;
namespace sh = vtts_stft_host;

namespace {

constexpr int ROWS_PER_LAUNCH = 128;
static_assert(ROWS_PER_LAUNCH == VTTS_SPECTRAL_ROWS_PER_LAUNCH, "the header states the split");
using Rows = vtts_rows::Lens<ROWS_PER_LAUNCH>;  // samples of each row of this launch
constexpr int MAX_F = sh::MAX_F;
constexpr float P_FLOOR = 1e-7f;
constexpr int SIGNALS = 2, REDUCE = 32;  // of sh::frames_lds_bytes: x and y are staged, and a frame leaves four fp64 sums

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

template <int NFFT, typename TI>
__global__ __launch_bounds__(64 * MAX_F) void spectral_frames_k(const SpecArgs a, const Rows rows) {
    constexpr int H = NFFT / 2, NB = H + 1, XB = pad8(H), J = Bins<H>::J;
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

    Window<H> wv;
    load_window<H>(wv, a.blob, lane);
    stage_twiddles<H>(twH, twN, a.blob, tid, 64 * F);
    // ---- 1. stage: span[sig][i] = padded sample hop t0 + i = row sample hop t0 - H + i, reflected at the row's ends
#pragma unroll
    for (int sig = 0; sig < 2; ++sig)
        stage_reflected(span + sig * a.span, static_cast<const TI*>(sig ? a.y : a.x) + (long long)b * a.s_stride, S, t0 * a.hop - H, a.span, tid, 64 * F);
    __syncthreads();

    // ---- 2./3. From here on a wave touches only its own exchange buffer.
    const long long t = t0 + wave;
    double A = 0.0, B = 0.0, C = 0.0, E = 0.0;
    if (t < T) {
        float pk[J], pn[J];  // x's powers at bins k and H - k
        const double K10 = 4.34294481903251827651;  // 10 / ln 10
#pragma unroll 1
        for (int sig = 0; sig < 2; ++sig) {  // one body for both signals
            transform_frame<H>(xb, twH, lane, span + sig * a.span + wave * a.hop, wv);
            float* mg = a.mags ? a.mags + ((((long long)b * 2 + sig) * a.t_stride + t) * NB) : nullptr;
            Bins<H> z;
            gather_bins(z, xb, lane);
            wave_sync();  // the next signal's first pass writes the buffer
            split_bins(z, twN, lane, [&](int j, int k, float2 p, float2 m) {
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
            });
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
__global__ __launch_bounds__(64) void spectral_finish_k(const SpecArgs a, const Rows rows) {
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
hipError_t launch(bool pcm, dim3 grid, int F, size_t lds, hipStream_t s, const SpecArgs& a, const Rows& rows, vtts::DynLdsOnce& once) {
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

struct vtts_spectral : sh::Tables {
    vtts_spectral_cfg cfg;
    int device = 0;
    int F = 1;
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
    if (int rc = sh::check_resolution(c.n_fft, c.hop, c.win)) return rc;
    auto* h = new (std::nothrow) vtts_spectral();
    if (!h) return failf(VTTS_ERR_NOMEM, "host allocation failed");
    h->cfg = c;
    h->device = device;
    h->F = sh::frames_per_block(c.n_fft, c.hop, SIGNALS, REDUCE);
    h->build(c.n_fft, c.win);
    *out = h;
    return VTTS_OK;
}

VTTS_API void vtts_spectral_destroy(vtts_spectral* h) { delete h; }

VTTS_API int vtts_spectral_window(const vtts_spectral* h, float* host_out) { return sh::window(h, h ? h->cfg.n_fft : 0, host_out); }

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

VTTS_API int vtts_spectral_packed_bytes(const vtts_spectral* h, size_t* bytes) { return sh::packed_bytes(h, bytes); }

VTTS_API int vtts_spectral_pack(vtts_spectral* h, void* dev_blob, size_t blob_bytes, void* stream) {
    return sh::pack(h, dev_blob, blob_bytes, stream, "the spectral tables");
}

VTTS_API int vtts_spectral_bind_packed(vtts_spectral* h, void* dev_blob, size_t blob_bytes) { return sh::bind_packed(h, dev_blob, blob_bytes); }

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
    const size_t esz = pcm ? 2 : 4, lds = sh::frames_lds_bytes(n_fft, hop, F, SIGNALS, REDUCE);
    const size_t nb = (size_t)n_fft / 2 + 1;
    return vtts_rows::for_each_launch<ROWS_PER_LAUNCH>(N, lengths, S_stride, [&](int r0, int nr, const Rows& rows) -> int {
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
        a.hop = hop, a.F = F, a.span = sh::even((F - 1) * hop + n_fft);
        const dim3 grid((unsigned)gmax, (unsigned)nr);
        vtts::DynLdsOnce& once = pcm ? h->lds_pcm : h->lds_f32;
        const hipError_t e = sh::by_nfft(n_fft, [&](auto n) { return launch<decltype(n)::value>(pcm, grid, F, lds, s, a, rows, once); });
        if (e != hipSuccess) return failf(VTTS_ERR_HIP, "spectral kernel launch failed: %s", hipGetErrorString(e));
        return VTTS_OK;
    });
}
