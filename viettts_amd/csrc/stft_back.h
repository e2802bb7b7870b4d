// The back of the inverse short-time transform, stated once for stft.hip's inverse kernel and denoise.hip's fused pass: a workgroup of W waves
// owns a run of consecutive output samples of one row, thread i samples i, i + 64 W, ..., and keeps their overlap-add sum y and envelope e in
// registers.  It walks the frames whose window covers the run in ascending t, W per round: each wave builds Z from its frame's bins (the inverse
// split step) in its own exchange buffer and inverse-transforms it there; after a workgroup barrier every thread adds the round's frames to its
// samples in ascending t.  Where the bins come from is the caller's.
//
// Include under the caller's `#pragma clang fp contract(off)`: both callers must produce the same bits (tests/test_gpu_denoise.py).
#pragma once

#include "stockham.h"

namespace vtts_stft_back {

using namespace vtts_stockham;

constexpr int inv_waves(int n_fft) { return n_fft == 2048 ? 4 : 8; }
constexpr int inv_per_thread(int n_fft) { return n_fft == 256 ? 2 : n_fft == 512 ? 4 : n_fft == 1024 ? 8 : 16; }
constexpr int inv_run(int n_fft) { return 64 * inv_waves(n_fft) * inv_per_thread(n_fft); }

// The frames t_lo .. t_hi (of T) whose window [hop t + lead, hop t + lead + win) meets the padded samples [p0, p1]; p1 >= lead.
__device__ __forceinline__ void covering_frames(int p0, int p1, int T, int hop, int lead, int win, int& t_lo, int& t_hi) {
    const int below = p0 - (lead + win - 1);
    t_lo = below <= 0 ? 0 : (below + hop - 1) / hop;
    t_hi = min(T - 1, (p1 - lead) / hop);
}

// The inverse split step for bin k <= H / 2 with X[k] = xk and X[H - k] = xn: Z[k] and Z[H - k] into the wave's exchange buffer.  The
// imaginary parts of bins 0 and H are no part of the signal.
template <int H>
__device__ __forceinline__ void put_bin_pair(float2* xb, const float2* twN, int k, float2 xk, float2 xn) {
    if (k == 0) xk.y = 0.0f, xn.y = 0.0f;
    const float2 A = make_float2(xk.x + xn.x, xk.y - xn.y);
    const float2 D = make_float2(xk.x - xn.x, xk.y + xn.y);
    const float2 B = cmul(conj(twN[k]), D);
    xb[pad8(k)] = make_float2(A.x - B.y, A.y + B.x);
    if (k != 0 && k != H / 2) xb[pad8(H - k)] = make_float2(A.x + B.y, B.x - A.y);
}

// y += v w, e += w w (each rounded) for the n frames tb .. tb + n - 1 of a round, in ascending t; xall holds their inverse transforms, one
// exchange buffer of XB entries each.  Thread tid of NT owns padded samples p0 + tid + NT r.
template <int R, int NT, int XB>
__device__ __forceinline__ void add_round(float (&y)[R], float (&e)[R], const float2* xall, const float* winl, int p0, int tid, int hop, int tb, int n,
                                          int lead, int win) {
    for (int u = 0; u < n; ++u) {
        const float* v = reinterpret_cast<const float*>(xall + u * XB);
        const int base = p0 + tid - hop * (tb + u);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int o = base + NT * r;
            if (o >= lead && o < lead + win) {
                const float w = winl[o];
                y[r] += v[2 * pad8(o >> 1) + (o & 1)] * w;
                e[r] += w * w;
            }
        }
    }
}

}  // namespace vtts_stft_back
