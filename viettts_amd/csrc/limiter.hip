// The true-peak meter and look-ahead limiter (include/vtts_limiter.h): a 4x oversampled envelope, its row maximum, and a per-sample gain
// (sliding minimum, then a sliding mean, of the gain each sample asks for) into fp32 or PCM16.
//
//   lim_env_k, one workgroup (256 lanes) per VTTS_LIMITER_TILE = 4096 samples of one row:
//     1. stage the tile and its FIR halo (27 samples before, 24 after; zeros outside the row) in LDS, PCM16 scaled by 2^-15.
//     2. each lane takes 4 consecutive samples at a time through limiter_common.h's true_peak4: their 4 x 4 oversampled points.  The 208
//        taps are a kernel argument.
//     3. p[n] = max(|x[n]|, |u[4 n .. 4 n + 3]|) goes to the workspace (unless only the peak is wanted) and, if asked for, to the caller's
//        envelope; the tile's maximum goes to its slot.
//   lim_reduce_k, one wave per row: the row's true peak from its tiles' slots in tile order (and, behind the limiter, its smallest gain).
//   lim_apply_k, same tiling.  A row with fl(g true_peak) <= c takes the plain multiply.  Otherwise:
//     1. req over the tile and 2 W samples either side (indices clamped to the row) into LDS.
//     2./3. limiter_common.h's smooth_gains: the sliding minimum over 2 W + 1, then its mean in the contract's fixed order, between two
//        LDS buffers.
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
#include "launch_rows.h"
#include "limiter_common.h"
#include "vtts_internal.h"

using vtts::failf;
using vtts::check_rows;
using namespace vtts_limiter_dev;  // (the tiling constants among them)

namespace {

constexpr int ROWS_PER_LAUNCH = 128;
constexpr int SPAN = TILE + KP + 4;   // staged samples of a tile: x[t0 - LEAD .. t0 + TILE + 28]
constexpr int MAX_APPLY_LDS = 2 * gain_buf_floats(MAX_W) * (int)sizeof(float);  // lim_apply_k's two gain buffers

using LimLens = vtts_rows::Lens<ROWS_PER_LAUNCH>;     // samples of each row of this launch
using LimRows = vtts_rows::OffLens<ROWS_PER_LAUNCH>;  // ... and each row's first output element, from the call's out

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
        float pk[4];
        true_peak4(span4, i, tp, pk);
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (i + s < live) mx = fmaxf(mx, pk[s]);
        if (ew) *reinterpret_cast<float4*>(ew + i) = make_float4(pk[0], pk[1], pk[2], pk[3]);  // (past the row inside its last tile: never read)
        if (eo) {
#pragma unroll
            for (int s = 0; s < 4; ++s)
                if (i + s < live) eo[i + s] = pk[s];
        }
    }
    if (eo)
        for (int i = live + tid; i < cnt; i += THREADS) eo[i] = 0.0f;
    mx = wave_extreme<false>(mx);
    if ((tid & 63) == 0) wmax[tid >> 6] = mx;
    __syncthreads();
    if (tid == 0) a.tmax[(long long)b * a.nt + blockIdx.x] = extreme4<false>(wmax);
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
    v = wave_extreme<MIN>(v);
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

    const int W = a.W, nR = TILE + 4 * W;
    const float* e = a.env + (long long)b * a.e_stride;
    const long long last = len - 1;
    float* cur = reinterpret_cast<float*>(lds4);

    // ---- 1. req[t0 - 2 W + k], k < TILE + 4 W
#pragma clang loop vectorize(disable)  // (the loop vectoriser would pair the multiplies into v_pk_mul_f32: build.py)
    for (int k = tid; k < nR; k += THREADS) {
        const long long n = min(max(t0 - 2 * W + k, 0LL), last);
        cur[k] = req_of(e[n], g, c);
    }
    __syncthreads();

    // ---- 2./3. the mean of the sliding minimum, for the tile's samples
    const float* mean = smooth_gains(cur, cur + a.nb, nR, W, t0, last, TILE + 2 * W, live, tid);

    // ---- 4. a, y, the store
    float amin = 1.0f;
#pragma clang loop vectorize(disable)  // (the loop vectoriser would pair the multiplies into v_pk_mul_f32: build.py)
    for (int i = tid; i < cnt; i += THREADS) {
        if (i < live) {
            const float av = fminf(req_of(e[t0 + i], g, c), mean[i]);
            amin = fminf(amin, av);
            out[i] = from_float<TO>((to_float(x[i]) * g) * av);
        } else {
            out[i] = TO(0);
        }
    }
    amin = wave_extreme<true>(amin);
    if ((tid & 63) == 0) wmin[tid >> 6] = amin;
    __syncthreads();
    if (tid == 0) a.tmin[(long long)b * a.nt + blockIdx.x] = extreme4<true>(wmin);
}

// ------------------------------------------------------------ host side ------------------------------------------------------------
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
    return vtts_rows::for_each_launch<ROWS_PER_LAUNCH>(N, lengths, S_stride, [&](int r0, int nr, const LimLens& rows) -> int {
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
        return VTTS_OK;
    });
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
    auto* h = new (std::nothrow) vtts_limiter();
    if (!h) return failf(VTTS_ERR_NOMEM, "host allocation failed");
    if (int rc = configure(cfg, h->taps, h->W)) {
        delete h;
        return rc;
    }
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
    if (int rc = check_rows("true_peak", wav_dev, dtype, N, S_stride, lengths, TILE, &longest)) return rc;
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
    if (int rc = check_rows("apply", wav_dev, dtype, N, S_stride, lengths, TILE, &longest)) return rc;
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
    return vtts_rows::for_each_launch_off<ROWS_PER_LAUNCH>(N, lengths, S_stride, O_stride, [&](int r0, int nr, const LimRows& rows) -> int {
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
        a.nb = gain_buf_floats(h->W);
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
        LimLens lens;  // lim_reduce_k takes the lengths alone
        for (int b = 0; b < ROWS_PER_LAUNCH; ++b) lens.len[b] = rows.len[b];
        hipLaunchKernelGGL((lim_reduce_k<true>), dim3((unsigned)nr), dim3(64), 0, s, r, lens);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return failf(VTTS_ERR_HIP, "limiter kernel launch failed: %s", hipGetErrorString(e));
        return VTTS_OK;
    });
}
