// The front of the forward short-time transform, stated once for spectral.hip's meter and stft.hip's forward and projection kernels (denoise.hip's
// fused pass runs its transform_frame-like first pass straight from global memory, and its gather_bins and split_bins): a
// workgroup of F waves stages the samples its F consecutive frames cover, reflected at the row's own ends; each wave then runs its windowed
// frame, as H = NFFT / 2 complex points z[n] = v[2n] + i v[2n+1], through stockham.h's forward transform in its own exchange buffer and
// splits the result into bins 0 .. H, a lane pairing bin k with bin H - k.  What becomes of the bins is the caller's.
//
// The tables come from the packed blob (stft_host.h): window [NFFT] | twH = exp(-2 pi i m / H) [H] | twN = exp(-2 pi i k / NFFT) [H / 2 + 1].
// Include under the caller's `#pragma clang fp contract(off)`: both callers must produce the same bits (tests/test_gpu_stft.py).
#pragma once

#include "sample_convert.h"
#include "stockham.h"

namespace vtts_stft_front {

using namespace vtts_stockham;

// this lane's window values of the first pass, [m][q] for point q of its m-th butterfly: loaded before the staging, so that their latency
// hides behind it
template <int H>
using Window = float2[Own<H, 8>::PER][8];

template <int H>
__device__ __forceinline__ void load_window(Window<H>& wv, const float* blob, int lane) {
    using O1 = Own<H, 8>;
    const float2* win2 = reinterpret_cast<const float2*>(blob);
#pragma unroll
    for (int m = 0; m < O1::PER; ++m)
#pragma unroll
        for (int q = 0; q < 8; ++q) wv[m][q] = O1::active(lane) ? win2[lane + 64 * m + q * O1::BF] : make_float2(0.0f, 0.0f);
}

// twH [H] and twN [H / 2 + 1] into LDS, by the whole workgroup
template <int H>
__device__ __forceinline__ void stage_twiddles(float2* twH, float2* twN, const float* blob, int tid, int nthreads) {
    const float2* t2 = reinterpret_cast<const float2*>(blob + 2 * H);
    for (int i = tid; i < H + H / 2 + 1; i += nthreads) (i < H ? twH[i] : twN[i - H]) = t2[i];
}

// row sample g of a row of S samples, reflected at the row's ends
__device__ __forceinline__ long long reflect_index(long long g, long long S) {
    if (g < 0) g = -g;
    if (g >= S) g = 2 * (S - 1) - g;
    return g < 0 ? 0 : g >= S ? S - 1 : g;  // frames past the row's last (never used) stay inside the row
}

// dst[i] = row sample g0 + i, i < n, reflected at the row's ends (S samples), PCM16 scaled by 2^-15 on the way; by the whole workgroup
template <typename TI>
__device__ __forceinline__ void stage_reflected(float* dst, const TI* x, long long S, long long g0, int n, int tid, int nthreads) {
    for (int i = tid; i < n; i += nthreads) dst[i] = vtts_sample::to_float_exact_shift(x[reflect_index(g0 + i, S)]);
}

// the transform of the frame that starts at fr[0], times the window; Z lies in xb in natural order
template <int H>
__device__ __forceinline__ void transform_frame(float2* xb, const float2* twH, int lane, const float* fr, const Window<H>& wv) {
    transform<H, false>(xb, twH, lane, [&](int m, int q, int i) { return make_float2(fr[2 * i] * wv[m][q].x, fr[2 * i + 1] * wv[m][q].y); });
}

// Z at the bins k = lane + 64 j <= H / 2 of a lane, and at their partners H - k
template <int H>
struct Bins {
    static constexpr int J = (H / 2) / 64 + 1;
    float2 zk[J], zn[J];
};

template <int H>
__device__ __forceinline__ void gather_bins(Bins<H>& z, const float2* xb, int lane) {
#pragma unroll
    for (int j = 0; j < Bins<H>::J; ++j) {
        const int k = min(lane + 64 * j, H / 2);
        z.zk[j] = xb[pad8(k)];
        z.zn[j] = xb[pad8((H - k) & (H - 1))];
    }
}

// The split step: use(j, k, p, m) for every bin k = lane + 64 j <= H / 2 of the lane, with X[k] = p and X[H - k] = conj(m).
template <int H, typename Use>
__device__ __forceinline__ void split_bins(const Bins<H>& z, const float2* twN, int lane, const Use& use) {
#pragma unroll
    for (int j = 0; j < Bins<H>::J; ++j) {
        const int k = lane + 64 * j;
        if (k <= H / 2) {
            const float2 e = make_float2(0.5f * (z.zk[j].x + z.zn[j].x), 0.5f * (z.zk[j].y - z.zn[j].y));
            const float2 o = make_float2(0.5f * (z.zk[j].y + z.zn[j].y), -0.5f * (z.zk[j].x - z.zn[j].x));
            const float2 w = cmul(twN[k], o);
            use(j, k, cadd(e, w), csub(e, w));
        }
    }
}

}  // namespace vtts_stft_front
