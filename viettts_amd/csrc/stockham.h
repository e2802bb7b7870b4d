// The H-point complex Stockham autosort transform of the short-time stages, stated once with the direction as a template parameter
// (INV = false: exp(-2 pi i ..), the analysis; INV = true: exp(+2 pi i ..), unscaled, the synthesis).  One wave transforms one frame in its own
// exchange buffer in LDS; H = 128, 256, 512 or 1024 (n_fft = 2 H) in radix-8 and radix-4 passes, 8 first: 128 = 8.4.4, 256 = 8.8.4,
// 512 = 8.8.8, 1024 = 8.8.4.4.  Pass with radix R after Ns = the product of the radices before it, butterfly j = 0 .. H / R - 1:
//     v[q] = in[j + q H / R] W^(q (j mod Ns)),  V = DFT_R(v),  out[(j / Ns) Ns R + (j mod Ns) + q Ns] = V[q],
// with W = exp(-+ 2 pi i / (Ns R)) read from ONE table exp(-2 pi i m / H) and conjugated for INV (a sign flip: exact).  A lane owns
// butterflies j = lane + 64 m and keeps their points in registers, so a pass runs in place: every read of the exchange buffer comes before any
// write, separated by a compiler-only wave fence (the LDS keeps one wave's accesses in order).  Entry i of the buffer lives at pad8(i) = i + i / 8:
// the radix-8 first pass writes out[8 j + q], which at stride 8 would put a half-wave's stores on 4 bank pairs and at stride 9 takes distinct ones.
//
// spectral.hip and stft.hip run it under `#pragma clang fp contract(off)`, every operation rounded on its own: a header's inline functions
// take the contraction mode of the file that includes them, so those files include this one AFTER their pragma.
//
// fft512_888 at the end is the other transform of the library, the fixed 512-point one of mel.hip and stoi.hip: twiddles AFTER the
// butterflies, so its bits are not the Stockham schedule's.  The two share the butterflies and nothing else.
#pragma once

#include <hip/hip_runtime.h>

#include "wave_common.h"

namespace vtts_stockham {

using vtts_wave::wave_sum;
using vtts_wave::wave_sync;

__host__ __device__ constexpr int pad8(int i) { return i + (i >> 3); }  // where entry i of an exchange buffer lives

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 conj(float2 a) { return make_float2(a.x, -a.y); }
// a times -i (the analysis) or +i (the synthesis)
template <bool INV>
__device__ __forceinline__ float2 mul_i(float2 a) {
    return INV ? make_float2(-a.y, a.x) : make_float2(a.y, -a.x);
}

// A[k] = sum_j a_j (-+ i)^(j k)
template <bool INV>
__device__ __forceinline__ void dft4(float2 a0, float2 a1, float2 a2, float2 a3, float2& A0, float2& A1, float2& A2, float2& A3) {
    const float2 s0 = cadd(a0, a2), d0 = csub(a0, a2), s1 = cadd(a1, a3), d1 = mul_i<INV>(csub(a1, a3));
    A0 = cadd(s0, s1);
    A1 = cadd(d0, d1);
    A2 = csub(s0, s1);
    A3 = csub(d0, d1);
}
// in place: v[k] = sum_a v[a] exp(-+ 2 pi i a k / R)
template <bool INV>
__device__ __forceinline__ void radix(float2 (&v)[4]) {
    dft4<INV>(v[0], v[1], v[2], v[3], v[0], v[1], v[2], v[3]);
}
template <bool INV>
__device__ __forceinline__ void radix(float2 (&v)[8]) {
    float2 e0, e1, e2, e3, o0, o1, o2, o3;
    dft4<INV>(v[0], v[2], v[4], v[6], e0, e1, e2, e3);
    dft4<INV>(v[1], v[3], v[5], v[7], o0, o1, o2, o3);
    const float c = 0.70710678118654752440f;
    if constexpr (INV) {
        o1 = make_float2(c * (o1.x - o1.y), c * (o1.x + o1.y));   // times conj W8   = (c, c)
        o2 = mul_i<true>(o2);                                     // times conj W8^2 = i
        o3 = make_float2(-c * (o3.x + o3.y), c * (o3.x - o3.y));  // times conj W8^3 = (-c, c)
    } else {
        o1 = make_float2(c * (o1.x + o1.y), c * (o1.y - o1.x));   // times W8   = (c, -c)
        o2 = mul_i<false>(o2);                                    // times W8^2 = -i
        o3 = make_float2(c * (o3.y - o3.x), -c * (o3.x + o3.y));  // times W8^3 = (-c, -c)
    }
    v[0] = cadd(e0, o0), v[4] = csub(e0, o0);
    v[1] = cadd(e1, o1), v[5] = csub(e1, o1);
    v[2] = cadd(e2, o2), v[6] = csub(e2, o2);
    v[3] = cadd(e3, o3), v[7] = csub(e3, o3);
}

// Butterflies a lane owns in a pass of radix R over H points
template <int H, int R>
struct Own {
    static constexpr int BF = H / R;                    // butterflies of the pass
    static constexpr int PER = BF >= 64 ? BF / 64 : 1;  // ... of one lane
    static __device__ __forceinline__ bool active(int lane) { return BF >= 64 || lane < BF; }
};

// One pass in place over the wave's exchange buffer.  load(m, q, i) gives input point i = j + q H / R of the lane's m-th butterfly: the
// buffer's entry (FromBuffer) or, in a first pass, whatever the caller computes it from.
struct FromBuffer {
    const float2* xb;
    __device__ __forceinline__ float2 operator()(int, int, int i) const { return xb[pad8(i)]; }
};

template <int H, int R, int NS, bool INV, typename Load>
__device__ __forceinline__ void pass(float2* xb, const float2* twH, int lane, const Load& load) {
    using O = Own<H, R>;
    float2 v[O::PER][R];
    if (O::active(lane)) {
#pragma unroll
        for (int m = 0; m < O::PER; ++m) {
            const int j = lane + 64 * m;
#pragma unroll
            for (int q = 0; q < R; ++q) v[m][q] = load(m, q, j + q * O::BF);
            if constexpr (NS > 1) {
                const int k = j & (NS - 1);
#pragma unroll
                for (int q = 1; q < R; ++q) {
                    const float2 w = twH[k * q * (H / (NS * R))];
                    v[m][q] = cmul(v[m][q], INV ? conj(w) : w);
                }
            }
            radix<INV>(v[m]);
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

// The whole transform: `first` feeds the radix-8 first pass, the result lies in xb in natural order.
template <int H, bool INV, typename Load>
__device__ __forceinline__ void transform(float2* xb, const float2* twH, int lane, const Load& first) {
    const FromBuffer buf{xb};
    pass<H, 8, 1, INV>(xb, twH, lane, first);
    if constexpr (H == 128) {
        pass<H, 4, 8, INV>(xb, twH, lane, buf);
        pass<H, 4, 32, INV>(xb, twH, lane, buf);
    } else if constexpr (H == 256) {
        pass<H, 8, 8, INV>(xb, twH, lane, buf);
        pass<H, 4, 64, INV>(xb, twH, lane, buf);
    } else if constexpr (H == 512) {
        pass<H, 8, 8, INV>(xb, twH, lane, buf);
        pass<H, 8, 64, INV>(xb, twH, lane, buf);
    } else {
        static_assert(H == 1024, "n_fft is 256, 512, 1024 or 2048");
        pass<H, 8, 8, INV>(xb, twH, lane, buf);
        pass<H, 4, 64, INV>(xb, twH, lane, buf);
        pass<H, 4, 256, INV>(xb, twH, lane, buf);
    }
}

// ---- 512 = 8 x 8 x 8 in one wave: 64 lanes x 8 points, three radix-8 passes in registers, two exchanges through the wave's buffer xb[XBUF]
//     n = 64 a + 8 b + c,  k = k0 + 8 k1 + 64 k2
//     X[k] = sum_c W8^(c k2) W64^(c k1) W512^(c k0)  sum_b W8^(b k1) W64^(b k0)  sum_a W8^(a k0) z[n]
// pass 1: lane = 8 b + c, registers a -> k0, times W512^(lane k0) = tw1(k0);   pass 2: lane = 8 k0 + c, registers b -> k1, times
// W512^(8 c k1);   pass 3: lane = 8 k0 + k1, registers c -> k2.  On entry v[a] = z[64 a + lane]; on return xb[k] = X[k] in natural order for
// k < 64 K2 (K2 = 8: all of them; a caller that needs the lower bins only stores fewer rows).  The rows of the exchanges are padded (72 complex
// per k0, and 9 per k1 in the second) so that every ds_write_b64 / ds_read_b64 of a 32-lane half touches 32 distinct bank pairs: stride-64 and
// stride-8 columns would be 4- and 8-way conflicts otherwise.  tw512[j] = exp(-2 pi i j / 512), in global memory or in LDS.
constexpr int XROW = 72;        // complex entries per k0 row of the exchange buffer (64 + 8 pad)
constexpr int XBUF = 8 * XROW;  // complex entries of one wave's exchange buffer (>= 512)

template <int K2, typename Tw1>
__device__ __forceinline__ void fft512_888(float2 (&v)[8], float2* xb, const float2* tw512, int lane, const Tw1& tw1) {
    const int hi = lane >> 3, lo = lane & 7;
    radix<false>(v);
#pragma unroll
    for (int k0 = 1; k0 < 8; ++k0) v[k0] = cmul(v[k0], tw1(k0));
#pragma unroll
    for (int k0 = 0; k0 < 8; ++k0) xb[k0 * XROW + lane] = v[k0];
    wave_sync();
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = xb[hi * XROW + q * 8 + lo];
    wave_sync();
    radix<false>(v);
#pragma unroll
    for (int k1 = 1; k1 < 8; ++k1) v[k1] = cmul(v[k1], tw512[8 * lo * k1]);
#pragma unroll
    for (int k1 = 0; k1 < 8; ++k1) xb[hi * XROW + k1 * 9 + lo] = v[k1];
    wave_sync();
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = xb[hi * XROW + lo * 9 + q];
    wave_sync();
    radix<false>(v);
#pragma unroll
    for (int k2 = 0; k2 < K2; ++k2) xb[hi + 8 * lo + 64 * k2] = v[k2];  // Z[k0 + 8 k1 + 64 k2], natural order
    wave_sync();
}

}  // namespace vtts_stockham
