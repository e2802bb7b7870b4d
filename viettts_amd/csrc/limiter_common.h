// What the limiter's two files share (limiter.hip, limiter_stream.hip), each stated once: the tiling constants and the size of a gain buffer,
// the taps' argument and the set-up both create()s run, the 4x oversampled peak of four samples, the gain a sample asks for, the gain
// smoothing (sliding minimum, then the fp64 sliding mean at its padded LDS layout) and the butterflies that end the kernels.  The streamed
// limiter owes "the un-streamed bits": it gets them by running this arithmetic, not a copy of it.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/vtts_limiter.h"
#include "audio_design.h"
#include "sample_convert.h"
#include "vtts_internal.h"

namespace vtts_limiter_dev {

using vtts_sample::from_float;
using vtts_sample::to_float;

constexpr int KP = VTTS_LIMITER_PHASE_TAPS;
constexpr int OS = VTTS_LIMITER_OVERSAMPLE;
constexpr int LEAD = 27;  // x[n - LEAD] meets a phase's first tap
constexpr int TILE = VTTS_LIMITER_TILE;
constexpr int RUN = VTTS_LIMITER_RUN;
constexpr int THREADS = 256;
constexpr int MAX_W = 960;                      // VTTS_LIMITER_MAX_RATE at VTTS_LIMITER_MAX_LOOKAHEAD_MS
constexpr int64_t MAX_S = 0x7fffffff - TILE;    // the longest row
static_assert(THREADS * RUN == TILE, "one lane per run of the mean");
static_assert(TILE % (4 * THREADS) == 0, "whole passes of 4 samples a lane");
static_assert(VTTS_LIMITER_MAX_RATE / 1000 * VTTS_LIMITER_MAX_LOOKAHEAD_MS == MAX_W, "the widest look-ahead create() hands out");

// floats of one of the two gain buffers: req over TILE + 4 W, or held over TILE + 2 W at word j + j / 16
constexpr int gain_buf_floats(int W) { return (TILE + 4 * W + (TILE + 2 * W) / RUN + 4 + 3) / 4 * 4; }

struct LimTaps {
    float t[OS][KP];
};

// What both create()s do with a configuration: the rate and look-ahead ranges, audio_design.h's 4x design into `taps`, and W.
inline int configure(const vtts_limiter_cfg* cfg, LimTaps& taps, int& W) {
    using vtts::failf;
    namespace ad = vtts_audio_design;
    if (cfg->sample_rate < VTTS_LIMITER_MIN_RATE || cfg->sample_rate > VTTS_LIMITER_MAX_RATE)
        return failf(VTTS_ERR_INVALID, "sample_rate must be in %d .. %d (got %d)", VTTS_LIMITER_MIN_RATE, VTTS_LIMITER_MAX_RATE, cfg->sample_rate);
    if (!(cfg->lookahead_ms > 0.0f) || !(cfg->lookahead_ms <= (float)VTTS_LIMITER_MAX_LOOKAHEAD_MS))
        return failf(VTTS_ERR_INVALID, "lookahead_ms must be above 0 and at most %g (got %g)", VTTS_LIMITER_MAX_LOOKAHEAD_MS, (double)cfg->lookahead_ms);
    ad::Design d;
    char why[160];
    if (ad::design(cfg->sample_rate, OS * cfg->sample_rate, d, why) != 0 || d.L != OS || d.M != 1 || d.kp4 != KP)
        return failf(VTTS_ERR_INVALID, "%s", why[0] ? why : "the 4x design does not have the shape the kernel expects");
    for (int p = 0; p < OS; ++p)
        for (int i = 0; i < KP; ++i) taps.t[p][i] = ad::table_at(d, p, i);
    const int w = (int)std::floor((double)cfg->sample_rate * (double)cfg->lookahead_ms / 1000.0 + 0.5);
    W = w < 1 ? 1 : w;
    return VTTS_OK;
}

// pk[s] = max(|x[n]|, |u[4 n .. 4 n + 3]|) of the four samples n = i + s (i a multiple of 4) of a span staged so that span[n + k] meets tap k
// of sample n: 56 staged values in registers feed the 16 fmaf chains of the 4 x 4 oversampled points (audio_common.h's chain for L = 4,
// M = 1: 52 taps a phase, ascending k, the zero padding first), 14 16-byte LDS reads for 832 FMAs.  The taps reach them as scalar operands;
// they are passed by value because by reference the compiler spills more of them into VGPR lanes inside the pass (16 more lane reads).
__device__ __forceinline__ void true_peak4(const float4* span4, int i, const LimTaps tp, float (&pk)[4]) {
    float xv[KP + 4];
#pragma unroll
    for (int c = 0; c < (KP + 4) / 4; ++c) {
        const float4 v = span4[(i >> 2) + c];
        xv[4 * c + 0] = v.x, xv[4 * c + 1] = v.y, xv[4 * c + 2] = v.z, xv[4 * c + 3] = v.w;
    }
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
    }
}

__device__ __forceinline__ float req_of(float p, float g, float c) {
    const float gp = g * p;
    return gp <= c ? 1.0f : c / gp;
}

// held[j] lives at word j + j / 16, so that 64 lanes walking 16 words apart meet 64 banks
__device__ __forceinline__ int padded(int j) { return j + (j >> 4); }

// The gain smoothing of one tile, called by the whole workgroup (it holds barriers, the first after the caller's own that published cur).
// In: cur[k] = req[t0 - 2 W + k], k < nR; nH = nR - 2 W; sample indices clamp to 0 .. top.  Out: the buffer (cur or nxt) whose words
// 0 .. live - 1 hold the mean of held[n - W .. n + W] for the tile's samples n = t0 ...
//   1. sliding minimum over 2 W + 1 by doubling: min over windows of 2, 4, .. 2^q <= 2 W + 1 samples between the two buffers, and the two
//      overlapping windows of 2^q that cover 2 W + 1.  A minimum is exact, so the scheme does not show in the bits.
//   2. the mean in the contract's fixed order: a lane owns RUN = 16 consecutive samples, sums the first one's window in fp64 and slides it
//      along the other 15.
__device__ __forceinline__ float* smooth_gains(float* cur, float* nxt, int nR, int W, long long t0, long long top, int nH, int live, int tid) {
    const int Lw = 2 * W + 1;
    // cur[k] = min req over `win` samples from k, win = 1, 2, 4, .. while 2 win <= Lw
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
    // held[t0 - W + j] at nxt[padded(j)], j < nH: the window of the CLAMPED sample
    for (int j = tid; j < nH; j += THREADS) {
        const long long m = min(max(t0 - W + j, 0LL), top);
        const int jc = (int)(m - (t0 - W));  // 0 .. nH - 1; its window is req[jc .. jc + 2 W] of the staged span
        nxt[padded(j)] = fminf(cur[jc], cur[jc + Lw - win]);
    }
    __syncthreads();
    // the mean of held[n - W .. n + W]: fp64, the first sample of a run from scratch, the others by sliding
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
    __syncthreads();
    return cur;
}

// A wave's maximum (MIN = false) or minimum in every lane, and that of the four waves' values a workgroup left in LDS.
template <bool MIN>
__device__ __forceinline__ float wave_extreme(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = MIN ? fminf(v, __shfl_xor(v, o)) : fmaxf(v, __shfl_xor(v, o));
    return v;
}
template <bool MIN>
__device__ __forceinline__ float extreme4(const float* w) {
    return MIN ? fminf(fminf(w[0], w[1]), fminf(w[2], w[3])) : fmaxf(fmaxf(w[0], w[1]), fmaxf(w[2], w[3]));
}
static_assert(THREADS == 4 * 64, "extreme4 reads four waves' values");

}  // namespace vtts_limiter_dev
