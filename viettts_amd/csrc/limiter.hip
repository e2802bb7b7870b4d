// The true-peak meter and look-ahead limiter (include/vtts_limiter.h): a 4x oversampled envelope, its row maximum, and a per-sample gain
// (sliding minimum, then a sliding mean, of the gain each sample asks for) into fp32 or PCM16.
//
//   lim_env_k, one workgroup (256 lanes) per VTTS_LIMITER_TILE = 4096 samples of one row:
//     1. stage the tile and its FIR halo (27 samples before, 24 after; zeros outside the row) in LDS, PCM16 scaled by 2^-15.
//     2. each lane takes 4 consecutive samples at a time: 56 staged values in registers feed the 16 fmaf chains of their 4 x 4 oversampled
//        points (audio.hip's chain for L = 4, M = 1: 52 taps a phase, ascending n, the zero padding first), 14 16-byte LDS reads for 832 FMAs.
//        The 208 taps are a kernel argument and reach the FMAs as scalar operands.
//     3. p[n] = max(|x[n]|, |u[4 n .. 4 n + 3]|) goes to the workspace (unless only the peak is wanted) and, if asked for, to the caller's
//        envelope; the tile's maximum goes to its slot.
//   lim_reduce_k, one wave per row: the row's true peak from its tiles' slots in tile order (and, behind the limiter, its smallest gain).
//   lim_apply_k, same tiling.  A row with fl(g true_peak) <= c takes the plain multiply.  Otherwise:
//     1. req over the tile and 2 W samples either side (indices clamped to the row) into LDS.
//     2. sliding minimum over 2 W + 1 by doubling: min over windows of 2, 4, .. 2^q <= 2 W + 1 samples between two LDS buffers, and the two
//        overlapping windows of 2^q that cover 2 W + 1.  A minimum is exact, so the scheme does not show in the bits.
//     3. the mean in the contract's fixed order: a lane owns VTTS_LIMITER_RUN = 16 consecutive samples, sums the first one's window in fp64
//        and slides it along the other 15.  held is kept at word j + j / 16 so that 64 lanes walking 16 words apart meet 64 banks.
//     4. a = min(req, mean), y = (g x) a, the store, and the tile's smallest a to its slot: coalesced again.
//   lim_pregain_k: one thread per row.
//
// Passes over HBM: the meter reads the samples once.  The limiter reads them twice, writes and reads the envelope (fp32) once each, and writes
// the output once.  Tiles are anchored at a row's own first sample, so nothing depends on the batch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>

#include "../../include/vtts_audio.h"
#include "../../include/vtts_hifigan.h"
#include "../../include/vtts_limiter.h"
#include "audio_design.h"
#include "limiter_common.h"
#include "vtts_internal.h"

using vtts::failf;
namespace ad = vtts_audio_design;
using vtts_limiter_dev::from_float;
using vtts_limiter_dev::KP;
using vtts_limiter_dev::LEAD;
using vtts_limiter_dev::LimTaps;
using vtts_limiter_dev::OS;
using vtts_limiter_dev::padded;
using vtts_limiter_dev::req_of;
using vtts_limiter_dev::to_float;

namespace {

constexpr int TILE = VTTS_LIMITER_TILE;
constexpr int RUN = VTTS_LIMITER_RUN;
constexpr int THREADS = 256;
constexpr int ROWS_PER_LAUNCH = 128;
constexpr int SPAN = TILE + KP + 4;   // staged samples of a tile: x[t0 - LEAD .. t0 + TILE + 28]
constexpr int MAX_W = 960;
static_assert(THREADS * RUN == TILE, "one lane per run of the mean");
static_assert(TILE % (4 * THREADS) == 0, "whole passes of 4 samples a lane");

// floats of one of lim_apply_k's two LDS buffers: req over TILE + 4 W, or held over TILE + 2 W at word j + j / 16
constexpr int apply_buf_floats(int W) { return (TILE + 4 * W + (TILE + 2 * W) / RUN + 4 + 3) / 4 * 4; }
constexpr int MAX_APPLY_LDS = 2 * apply_buf_floats(MAX_W) * (int)sizeof(float);

struct LimLens {
    int len[ROWS_PER_LAUNCH];  // samples of each row of this launch
};

struct LimRows {
    long long off[ROWS_PER_LAUNCH];  // first output element of each row of this launch, from the call's out
    int len[ROWS_PER_LAUNCH];
};

struct EnvArgs {
    const void* wav;     // first row of this launch, as every pointer below
    long long s_stride;  // samples between rows
    float* env;          // NULL, or [rows][e_stride]: the workspace's envelope
    long long e_stride;
    float* envout;       // NULL, or [rows][s_stride]: the caller's
    float* tmax;         // [rows][nt]
    long long nt;
};

struct ReduceArgs {
    const float* slots;  // [rows][nt]
    long long nt;
    float* result;       // [rows]
    const float* gains;  // NULL, or [rows]
    float* gains_used;   // NULL, or [rows]
};

struct ApplyArgs {
    const void* wav;
    void* out;  // the call's output
    const float* env;
    long long e_stride;
    const float* gains;  // NULL = 1
    const float* true_peak;
    float* tmin;  // [rows][nt]
    long long nt;
    long long s_stride;
    long long o_stride;  // 0 = packed
    float c;
    int W;
    int nb;  // floats of one LDS buffer
};

template <typename TI>
__global__ __launch_bounds__(THREADS) void lim_env_k(const EnvArgs a, const LimTaps tp, const LimLens rows) {
    __shared__ float4 span4[SPAN / 4];
    __shared__ float wmax[THREADS / 64];
    float* span = reinterpret_cast<float*>(span4);
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const long long len = rows.len[b];
    const long long t0 = (long long)blockIdx.x * TILE;
    const long long cap = a.envout ? a.s_stride : len;
    if (t0 >= cap) return;  // block-uniform
    const int cnt = (int)min((long long)TILE, cap - t0);
    float* eo = a.envout ? a.envout + (long long)b * a.s_stride + t0 : nullptr;
    if (t0 >= len) {  // past the row: the caller's envelope is zero there
        for (int i = tid; i < cnt; i += THREADS) eo[i] = 0.0f;
        return;
    }
    const int live = (int)min((long long)TILE, len - t0);
    const TI* x = static_cast<const TI*>(a.wav) + (long long)b * a.s_stride;

    // ---- 1. span[k] = x[t0 - LEAD + k], zero outside [0, len)
#pragma clang loop vectorize(disable)  // (the loop vectoriser would pair the multiplies into v_pk_mul_f32: build.py)
    for (int k = tid; k < SPAN; k += THREADS) {
        const long long g = t0 - LEAD + k;
        span[k] = (g >= 0 && g < len) ? to_float(x[g]) : 0.0f;
    }
    __syncthreads();

    // ---- 2./3. four samples a lane and pass
    float* ew = a.env ? a.env + (long long)b * a.e_stride + t0 : nullptr;
    float mx = 0.0f;
    for (int it = 0; it < TILE / (4 * THREADS); ++it) {
        const int i = 4 * (tid + THREADS * it);
        if (i >= live) break;
        float xv[KP + 4];
#pragma unroll
        for (int c = 0; c < (KP + 4) / 4; ++c) {
            const float4 v = span4[(i >> 2) + c];
            xv[4 * c + 0] = v.x, xv[4 * c + 1] = v.y, xv[4 * c + 2] = v.z, xv[4 * c + 3] = v.w;
        }
        float pk[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            float p = fabsf(xv[s + LEAD]);
#pragma unroll
            for (int r = 0; r < OS; ++r) {
                float acc = 0.0f;
#pragma unroll
                for (int k = 0; k < KP; ++k) acc = fmaf(xv[s + k], tp.t[r][k], acc);
                p = fmaxf(p, fabsf(acc));
            }
            pk[s] = p;
            if (i + s < live) mx = fmaxf(mx, p);
        }
        if (ew) *reinterpret_cast<float4*>(ew + i) = make_float4(pk[0], pk[1], pk[2], pk[3]);  // (past the row inside its last tile: never read)
        if (eo) {
#pragma unroll
            for (int s = 0; s < 4; ++s)
                if (i + s < live) eo[i + s] = pk[s];
        }
    }
    if (eo)
        for (int i = live + tid; i < cnt; i += THREADS) eo[i] = 0.0f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((tid & 63) == 0) wmax[tid >> 6] = mx;
    __syncthreads();
    if (tid == 0) a.tmax[(long long)b * a.nt + blockIdx.x] = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
}

// MIN = false: result = max over the row's tile slots, from 0.  MIN = true: min, from 1.
template <bool MIN>
__global__ __launch_bounds__(64) void lim_reduce_k(const ReduceArgs a, const LimLens rows) {
    const int lane = threadIdx.x;
    const int b = blockIdx.x;
    const long long ntr = ((long long)rows.len[b] + TILE - 1) / TILE;
    float v = MIN ? 1.0f : 0.0f;
    for (long long t = lane; t < ntr; t += 64) {
        const float s = a.slots[(long long)b * a.nt + t];
        v = MIN ? fminf(v, s) : fmaxf(v, s);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float w = __shfl_xor(v, o);
        v = MIN ? fminf(v, w) : fmaxf(v, w);
    }
    if (lane == 0) {
        a.result[b] = v;
        if (a.gains_used) a.gains_used[b] = a.gains ? a.gains[b] : 1.0f;
    }
}

__global__ __launch_bounds__(THREADS) void lim_pregain_k(const float* integrated, float target, float max_gain, float* gains, int N) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= N) return;
    const float I = integrated[i];
    float g = 1.0f;
    if (I == I && I != -INFINITY && I != INFINITY) {
        const float g1 = (float)pow(10.0, ((double)target - (double)I) / 20.0);
        const float g2 = (float)pow(10.0, (double)max_gain / 20.0);
        g = fminf(g1, g2);
    }
    gains[i] = g;
}

template <typename TI, typename TO>
__global__ __launch_bounds__(THREADS) void lim_apply_k(const ApplyArgs a, const LimRows rows) {
    extern __shared__ float4 lds4[];
    __shared__ float wmin[THREADS / 64];
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const long long len = rows.len[b];
    const long long cap = a.o_stride ? a.o_stride : len;
    const long long t0 = (long long)blockIdx.x * TILE;
    if (t0 >= cap) return;  // block-uniform, as every branch before the last barrier
    const int cnt = (int)min((long long)TILE, cap - t0);
    const int live = (int)max(0LL, min((long long)TILE, len - t0));
    const TI* x = static_cast<const TI*>(a.wav) + (long long)b * a.s_stride + t0;
    TO* out = static_cast<TO*>(a.out) + rows.off[b] + t0;
    if (live == 0) {
        for (int i = tid; i < cnt; i += THREADS) out[i] = TO(0);
        return;
    }
    const float g = a.gains ? a.gains[b] : 1.0f;
    const float c = a.c;
    if (!(g * a.true_peak[b] > c)) {  // no sample of the row asks for a reduction: a = 1 exactly
#pragma clang loop vectorize(disable)  // (the loop vectoriser would pair the multiplies into v_pk_mul_f32: build.py)
        for (int i = tid; i < cnt; i += THREADS) out[i] = i < live ? from_float<TO>(to_float(x[i]) * g) : TO(0);
        if (tid == 0) a.tmin[(long long)b * a.nt + blockIdx.x] = 1.0f;
        return;
    }

    const int W = a.W, Lw = 2 * W + 1, nR = TILE + 4 * W, nH = TILE + 2 * W;
    const float* e = a.env + (long long)b * a.e_stride;
    const long long last = len - 1;
    float* cur = reinterpret_cast<float*>(lds4);
    float* nxt = cur + a.nb;

    // ---- 1. req[t0 - 2 W + k], k < TILE + 4 W
#pragma clang loop vectorize(disable)  // (the loop vectoriser would pair the multiplies into v_pk_mul_f32: build.py)
    for (int k = tid; k < nR; k += THREADS) {
        const long long n = min(max(t0 - 2 * W + k, 0LL), last);
        cur[k] = req_of(e[n], g, c);
    }
    __syncthreads();

    // ---- 2. cur[k] = min req over `win` samples from k, win = 1, 2, 4, .. while 2 win <= Lw
    int win = 1, ncur = nR;
    while (2 * win <= Lw) {
        ncur -= win;
        for (int k = tid; k < ncur; k += THREADS) nxt[k] = fminf(cur[k], cur[k + win]);
        __syncthreads();
        float* t = cur;
        cur = nxt;
        nxt = t;
        win *= 2;
    }
    // held[t0 - W + j] at nxt[padded(j)], j < TILE + 2 W: the window of the CLAMPED sample
    for (int j = tid; j < nH; j += THREADS) {
        const long long m = min(max(t0 - W + j, 0LL), last);
        const int jc = (int)(m - (t0 - W));  // 0 .. nH - 1; its window is req[jc .. jc + 2 W] of the staged span
        nxt[padded(j)] = fminf(cur[jc], cur[jc + Lw - win]);
    }
    __syncthreads();

    // ---- 3. the mean of held[n - W .. n + W]: fp64, the first sample of a run from scratch, the others by sliding
    {
        const float* H = nxt;
        const int i0 = RUN * tid;
        if (i0 < live) {
            double s = 0.0;
            for (int k = 0; k < Lw; ++k) s += (double)H[padded(i0 + k)];
            const double dl = (double)Lw;
            cur[i0] = (float)(s / dl);
            for (int t = 1; t < RUN; ++t) {
                const int n = i0 + t;
                s = (s + (double)H[padded(n + 2 * W)]) - (double)H[padded(n - 1)];
                cur[n] = (float)(s / dl);
            }
        }
    }
    __syncthreads();

    // ---- 4. a, y, the store
    float amin = 1.0f;
#pragma clang loop vectorize(disable)  // (the loop vectoriser would pair the multiplies into v_pk_mul_f32: build.py)
    for (int i = tid; i < cnt; i += THREADS) {
        if (i < live) {
            const float av = fminf(req_of(e[t0 + i], g, c), cur[i]);
            amin = fminf(amin, av);
            out[i] = from_float<TO>((to_float(x[i]) * g) * av);
        } else {
            out[i] = TO(0);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amin = fminf(amin, __shfl_xor(amin, o));
    if ((tid & 63) == 0) wmin[tid >> 6] = amin;
    __syncthreads();
    if (tid == 0) a.tmin[(long long)b * a.nt + blockIdx.x] = fminf(fminf(wmin[0], wmin[1]), fminf(wmin[2], wmin[3]));
}

// ------------------------------------------------------------ host side ------------------------------------------------------------
constexpr int64_t MAX_S = 0x7fffffff - TILE;

struct Layout {
    int64_t nt = 0;        // tiles of the longest row: the per-row pitch of the slots, and e_stride = nt * TILE
    size_t env = 0, tmax = 0, tmin = 0, bytes = 0;
};
Layout layout(int N, int64_t S) {
    Layout l;
    l.nt = (S + TILE - 1) / TILE;
    const size_t slots = (size_t)N * (size_t)l.nt * sizeof(float);
    l.env = 0;
    l.tmax = (size_t)N * (size_t)l.nt * TILE * sizeof(float);
    l.tmin = l.tmax + slots;
    l.bytes = (l.tmin + slots + 15) / 16 * 16;
    if (l.bytes == 0) l.bytes = 16;
    return l;
}

int check_rows(const char* what, const void* wav, int dtype, int N, int64_t S_stride, const int32_t* lengths, int64_t* longest) {
    if (!wav) return failf(VTTS_ERR_INVALID, "null argument");
    if (dtype != VTTS_AUDIO_F32 && dtype != VTTS_AUDIO_PCM16) return failf(VTTS_ERR_INVALID, "%s: dtype must be VTTS_AUDIO_F32 or VTTS_AUDIO_PCM16 (got %d)", what, dtype);
    if (N <= 0) return failf(VTTS_ERR_INVALID, "%s: N must be positive (got %d)", what, N);
    if (S_stride < 0 || S_stride > MAX_S) return failf(VTTS_ERR_SHAPE, "%s: S_stride must be in 0 .. 2^31 - 1 - %d (got %lld)", what, TILE, (long long)S_stride);
    int64_t m = 0;
    for (int b = 0; b < N; ++b) {
        const int64_t len = lengths ? lengths[b] : S_stride;
        if (len < 0 || len > S_stride) return failf(VTTS_ERR_SHAPE, "%s: lengths[%d] = %lld is outside 0 .. S_stride = %lld", what, b, (long long)len, (long long)S_stride);
        if (len > m) m = len;
    }
    *longest = m;
    return VTTS_OK;
}

int check_workspace(const void* workspace, size_t workspace_bytes, const Layout& l) {
    if (!workspace) return failf(VTTS_ERR_INVALID, "null argument");
    if (workspace_bytes < l.bytes) return failf(VTTS_ERR_NOMEM, "workspace too small: %zu < %zu bytes", workspace_bytes, l.bytes);
    if (reinterpret_cast<uintptr_t>(workspace) % 16) return failf(VTTS_ERR_INVALID, "workspace must be 16-byte aligned");
    return VTTS_OK;
}

}  // namespace

struct vtts_limiter {
    int rate = 0;
    int W = 0;
    int device = 0;
    LimTaps taps;
    vtts::DynLdsOnce lds[4];
};

namespace {

// The envelope pass of true_peak() and apply(): lim_env_k over every row, then the rows' maxima.
int run_envelope(vtts_limiter* h, const void* wav_dev, int dtype, int N, int64_t S_stride, const int32_t* lengths, int64_t longest, const Layout& l,
                 char* ws, bool keep_env, float* envelope_dev, float* true_peak_dev, const float* gains_dev, float* gains_used_dev, hipStream_t s) {
    const bool pcm = dtype == VTTS_AUDIO_PCM16;
    const size_t esz = pcm ? 2 : 4;
    const int64_t cover = envelope_dev ? S_stride : longest;
    const unsigned tiles = (unsigned)((cover + TILE - 1) / TILE);
    for (int r0 = 0; r0 < N; r0 += ROWS_PER_LAUNCH) {  // the rows' lengths travel as kernel arguments
        const int nr = N - r0 < ROWS_PER_LAUNCH ? N - r0 : ROWS_PER_LAUNCH;
        LimLens rows;
        for (int b = 0; b < ROWS_PER_LAUNCH; ++b) rows.len[b] = b < nr ? (lengths ? lengths[r0 + b] : (int)S_stride) : 0;
        EnvArgs a;
        a.wav = static_cast<const char*>(wav_dev) + (size_t)r0 * S_stride * esz;
        a.s_stride = S_stride;
        a.env = keep_env ? reinterpret_cast<float*>(ws + l.env) + (size_t)r0 * l.nt * TILE : nullptr;
        a.e_stride = l.nt * TILE;
        a.envout = envelope_dev ? envelope_dev + (size_t)r0 * S_stride : nullptr;
        a.tmax = reinterpret_cast<float*>(ws + l.tmax) + (size_t)r0 * l.nt;
        a.nt = l.nt;
        if (tiles > 0) {
            const dim3 grid(tiles, (unsigned)nr);
            if (pcm)
                hipLaunchKernelGGL((lim_env_k<short>), grid, dim3(THREADS), 0, s, a, h->taps, rows);
            else
                hipLaunchKernelGGL((lim_env_k<float>), grid, dim3(THREADS), 0, s, a, h->taps, rows);
        }
        ReduceArgs r;
        r.slots = a.tmax;
        r.nt = l.nt;
        r.result = true_peak_dev + r0;
        r.gains = gains_dev ? gains_dev + r0 : nullptr;
        r.gains_used = gains_used_dev ? gains_used_dev + r0 : nullptr;
        hipLaunchKernelGGL((lim_reduce_k<false>), dim3((unsigned)nr), dim3(64), 0, s, r, rows);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return failf(VTTS_ERR_HIP, "limiter kernel launch failed: %s", hipGetErrorString(e));
    }
    return VTTS_OK;
}

template <typename TI, typename TO>
hipError_t launch_apply(const ApplyArgs& a, const LimRows& rows, dim3 grid, hipStream_t s, vtts::DynLdsOnce& once) {
    const void* fn = reinterpret_cast<const void*>(&lim_apply_k<TI, TO>);
    hipError_t e = vtts::set_max_dynamic_lds(fn, MAX_APPLY_LDS, once);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((lim_apply_k<TI, TO>), grid, dim3(THREADS), 2 * (size_t)a.nb * sizeof(float), s, a, rows);
    return hipGetLastError();
}

}  // namespace

VTTS_API int vtts_limiter_create(const vtts_limiter_cfg* cfg, int device, vtts_limiter** out) {
    if (!cfg || !out) return failf(VTTS_ERR_INVALID, "null argument");
    if (cfg->sample_rate < VTTS_LIMITER_MIN_RATE || cfg->sample_rate > VTTS_LIMITER_MAX_RATE)
        return failf(VTTS_ERR_INVALID, "sample_rate must be in %d .. %d (got %d)", VTTS_LIMITER_MIN_RATE, VTTS_LIMITER_MAX_RATE, cfg->sample_rate);
    if (!(cfg->lookahead_ms > 0.0f) || !(cfg->lookahead_ms <= (float)VTTS_LIMITER_MAX_LOOKAHEAD_MS))
        return failf(VTTS_ERR_INVALID, "lookahead_ms must be above 0 and at most %g (got %g)", VTTS_LIMITER_MAX_LOOKAHEAD_MS, (double)cfg->lookahead_ms);
    auto* h = new (std::nothrow) vtts_limiter();
    if (!h) return failf(VTTS_ERR_NOMEM, "host allocation failed");
    ad::Design d;
    char why[160];
    if (ad::design(cfg->sample_rate, OS * cfg->sample_rate, d, why) != 0 || d.L != OS || d.M != 1 || d.kp4 != KP) {
        delete h;
        return failf(VTTS_ERR_INVALID, "%s", why[0] ? why : "the 4x design does not have the shape the kernel expects");
    }
    for (int p = 0; p < OS; ++p)
        for (int i = 0; i < KP; ++i) h->taps.t[p][i] = ad::table_at(d, p, i);
    const int W = (int)std::floor((double)cfg->sample_rate * (double)cfg->lookahead_ms / 1000.0 + 0.5);
    h->W = W < 1 ? 1 : W;
    h->rate = cfg->sample_rate;
    h->device = device;
    *out = h;
    return VTTS_OK;
}

VTTS_API void vtts_limiter_destroy(vtts_limiter* h) { delete h; }

VTTS_API int vtts_limiter_lookahead(const vtts_limiter* h, int32_t* W) {
    if (!h || !W) return failf(VTTS_ERR_INVALID, "null argument");
    *W = h->W;
    return VTTS_OK;
}

VTTS_API int vtts_limiter_taps(const vtts_limiter* h, float* host_out) {
    if (!h || !host_out) return failf(VTTS_ERR_INVALID, "null argument");
    for (int p = 0; p < OS; ++p)
        for (int i = 0; i < KP; ++i) host_out[p * KP + i] = h->taps.t[p][i];
    return VTTS_OK;
}

VTTS_API int vtts_limiter_workspace_bytes(const vtts_limiter* h, int N, int64_t S, size_t* bytes) {
    if (!h || !bytes) return failf(VTTS_ERR_INVALID, "null argument");
    if (N <= 0) return failf(VTTS_ERR_INVALID, "N must be positive (got %d)", N);
    if (S < 0 || S > MAX_S) return failf(VTTS_ERR_SHAPE, "S must be in 0 .. 2^31 - 1 - %d (got %lld)", TILE, (long long)S);
    *bytes = layout(N, S).bytes;
    return VTTS_OK;
}

VTTS_API int vtts_limiter_true_peak(vtts_limiter* h, const void* wav_dev, int dtype, int N, int64_t S_stride, const int32_t* lengths,
                                    float* true_peak_dev, float* envelope_dev, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h || !true_peak_dev) return failf(VTTS_ERR_INVALID, "null argument");
    int64_t longest = 0;
    if (int rc = check_rows("true_peak", wav_dev, dtype, N, S_stride, lengths, &longest)) return rc;
    const Layout l = layout(N, longest);
    if (int rc = check_workspace(workspace, workspace_bytes, l)) return rc;
    return run_envelope(h, wav_dev, dtype, N, S_stride, lengths, longest, l, static_cast<char*>(workspace), false, envelope_dev, true_peak_dev, nullptr,
                        nullptr, static_cast<hipStream_t>(stream));
}

VTTS_API int vtts_limiter_pregain(vtts_limiter* h, const float* integrated_dev, int N, float target_lufs, float max_gain_db, float* gains_dev,
                                  void* stream) {
    if (!h || !integrated_dev || !gains_dev) return failf(VTTS_ERR_INVALID, "null argument");
    if (N <= 0) return failf(VTTS_ERR_INVALID, "pregain: N must be positive (got %d)", N);
    if (!std::isfinite(target_lufs) || !std::isfinite(max_gain_db))
        return failf(VTTS_ERR_INVALID, "pregain: target_lufs and max_gain_db must be finite (got %g, %g)", target_lufs, max_gain_db);
    hipLaunchKernelGGL(lim_pregain_k, dim3((unsigned)((N + THREADS - 1) / THREADS)), dim3(THREADS), 0, static_cast<hipStream_t>(stream), integrated_dev,
                       target_lufs, max_gain_db, gains_dev, N);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return failf(VTTS_ERR_HIP, "limiter kernel launch failed: %s", hipGetErrorString(e));
    return VTTS_OK;
}

VTTS_API int vtts_limiter_apply(vtts_limiter* h, const void* wav_dev, int dtype, int N, int64_t S_stride, const int32_t* lengths,
                                const float* gains_dev, float ceiling_dbtp, void* out_dev, int out_dtype, int64_t O_stride, float* true_peak_dev,
                                float* min_gain_dev, float* gains_used_dev, float* envelope_dev, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h || !out_dev || !true_peak_dev || !min_gain_dev || !gains_used_dev) return failf(VTTS_ERR_INVALID, "null argument");
    if (out_dtype != VTTS_AUDIO_F32 && out_dtype != VTTS_AUDIO_PCM16)
        return failf(VTTS_ERR_INVALID, "apply: out_dtype must be VTTS_AUDIO_F32 or VTTS_AUDIO_PCM16 (got %d)", out_dtype);
    int64_t longest = 0;
    if (int rc = check_rows("apply", wav_dev, dtype, N, S_stride, lengths, &longest)) return rc;
    if (!std::isfinite(ceiling_dbtp)) return failf(VTTS_ERR_INVALID, "apply: ceiling_dbtp must be finite (got %g)", ceiling_dbtp);
    if (O_stride < 0 || (O_stride > 0 && O_stride < longest))
        return failf(VTTS_ERR_SHAPE, "O_stride = %lld is below the longest row's %lld samples", (long long)O_stride, (long long)longest);
    const Layout l = layout(N, longest);
    if (int rc = check_workspace(workspace, workspace_bytes, l)) return rc;

    hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    if (int rc = run_envelope(h, wav_dev, dtype, N, S_stride, lengths, longest, l, ws, true, envelope_dev, true_peak_dev, gains_dev, gains_used_dev, s)) return rc;

    const bool pin = dtype == VTTS_AUDIO_PCM16, pout = out_dtype == VTTS_AUDIO_PCM16;
    const size_t esz = pin ? 2 : 4;
    const int64_t cover = O_stride ? O_stride : longest;
    const unsigned tiles = (unsigned)((cover + TILE - 1) / TILE);
    long long packed = 0;
    for (int r0 = 0; r0 < N; r0 += ROWS_PER_LAUNCH) {
        const int nr = N - r0 < ROWS_PER_LAUNCH ? N - r0 : ROWS_PER_LAUNCH;
        LimRows rows;
        LimLens lens;
        for (int b = 0; b < ROWS_PER_LAUNCH; ++b) {
            const int len = b < nr ? (lengths ? lengths[r0 + b] : (int)S_stride) : 0;
            rows.len[b] = lens.len[b] = len;
            rows.off[b] = O_stride ? (long long)(r0 + b) * O_stride : packed;
            packed += len;
        }
        ApplyArgs a;
        a.wav = static_cast<const char*>(wav_dev) + (size_t)r0 * S_stride * esz;
        a.out = out_dev;
        a.env = reinterpret_cast<const float*>(ws + l.env) + (size_t)r0 * l.nt * TILE;
        a.e_stride = l.nt * TILE;
        a.gains = gains_dev ? gains_dev + r0 : nullptr;
        a.true_peak = true_peak_dev + r0;
        a.tmin = reinterpret_cast<float*>(ws + l.tmin) + (size_t)r0 * l.nt;
        a.nt = l.nt;
        a.s_stride = S_stride;
        a.o_stride = O_stride;
        a.c = (float)std::pow(10.0, (double)ceiling_dbtp / 20.0);
        a.W = h->W;
        a.nb = apply_buf_floats(h->W);
        if (tiles > 0) {
            const dim3 grid(tiles, (unsigned)nr);
            hipError_t e;
            if (pin)
                e = pout ? launch_apply<short, short>(a, rows, grid, s, h->lds[3]) : launch_apply<short, float>(a, rows, grid, s, h->lds[2]);
            else
                e = pout ? launch_apply<float, short>(a, rows, grid, s, h->lds[1]) : launch_apply<float, float>(a, rows, grid, s, h->lds[0]);
            if (e != hipSuccess) return failf(VTTS_ERR_HIP, "limiter kernel launch failed: %s", hipGetErrorString(e));
        }
        ReduceArgs r;
        r.slots = a.tmin;
        r.nt = l.nt;
        r.result = min_gain_dev + r0;
        r.gains = nullptr;
        r.gains_used = nullptr;
        hipLaunchKernelGGL((lim_reduce_k<true>), dim3((unsigned)nr), dim3(64), 0, s, r, lens);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return failf(VTTS_ERR_HIP, "limiter kernel launch failed: %s", hipGetErrorString(e));
    }
    return VTTS_OK;
}
