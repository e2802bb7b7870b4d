// Host side of the loudness meter (include/vtts_loudness.h): the K-weighting coefficients in double, the filter's 4 x 4 state
// transition matrix, its powers and the homogeneous-response table the kernel's scan uses, and the row arithmetic of measure().
// Plain C++ with no HIP in it, so that a stand-alone program can run it under the host sanitizers (tools/loudness_design_check.cpp);
// loudness.hip is its only other user.
//
// Both biquads run in transposed direct form II, so the state is s = (s1, s2, s3, s4) and one sample x does
//     y1 = b0 x + s1;   s1' = b1 x - a1 y1 + s2;   s2' = b2 x - a2 y1                     (shelf)
//     z  = y1 + s3;     s3' = -2 y1 - c1 z + s4;   s4' = y1 - c2 z                        (high-pass, b = [1, -2, 1])
// With x = 0 this is s' = A s and z = s1 + s3: the homogeneous response to an incoming state s is z[i] = (1, 0, 1, 0) A^i s.
//
// The high-pass has both poles within 0.015 (16 kHz) to 0.0025 (96 kHz) of 1, and in these coordinates its block of A is close to a Jordan
// block: the entries of A^n grow to 136 at 96 kHz before they decay, s3 and s4 are large and cancel, and carrying s across chunks in fp32
// lost 0.025 dB on a DC step (tools/loudness_design_check.cpp measured it).  So the state is CARRIED as q = T s,
//     q1 = s1, q2 = s2, q3 = s3 + s4, q4 = kappa s4,   kappa = sqrt(1 + c1 + c2)   ((1 - pole)^2 up to a factor near 1)
// in which the high-pass block is near a rotation and no power of it exceeds a few units.  Every table below is in these coordinates
// (T A^n T^-1, and the response row times T^-1); the kernel applies T once to each chunk's end state.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/vtts_loudness.h"

namespace vtts_loudness_design {

constexpr int CHUNK = VTTS_LOUDNESS_CHUNK;
constexpr int SEGMENT = VTTS_LOUDNESS_SEGMENT;
constexpr int LANES = 64;                        // chunks per wave
constexpr int WAVES = SEGMENT / (CHUNK * LANES);  // waves per workgroup
constexpr int SLOTS = VTTS_LOUDNESS_SEGMENT_HOPS;
static_assert(WAVES * LANES * CHUNK == SEGMENT && WAVES == 4, "a workgroup of 256 lanes covers one segment");
static_assert((SEGMENT - 1) / (VTTS_LOUDNESS_MIN_RATE / 10) + 2 <= SLOTS, "a segment's hops fit its partial-sum slots");
static_assert(CHUNK <= VTTS_LOUDNESS_MIN_RATE / 10, "a chunk meets at most one hop boundary");

// What the kernels take by value: everything derived from the rate.
struct Tables {
    float cf[10];           // the coefficients, rounded once: shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2
    float kappa;            // q4 = kappa s4
    float htab[CHUNK * 4];  // htab[i] = (1, 0, 1, 0) A^i T^-1: sample i of a chunk adds htab[i] . (the chunk's incoming q)
    float lo[8 * 16];       // lo[k] = T A^(CHUNK k) T^-1, row-major: lane l's incoming q is excl + lo[l & 7] hi[l >> 3] (the wave's)
    float hi[8 * 16];       // hi[k] = T A^(8 CHUNK k) T^-1
    float wave[16];         // T A^(64 CHUNK) T^-1: from one wave's incoming q to the next's
    float seg[16];          // T A^SEGMENT T^-1
};

struct Design {
    int fs = 0, H = 0;
    double coef[10] = {};
    Tables t = {};
};

using Mat = double[16];

inline void mat_mul(const Mat a, const Mat b, Mat out) {
    Mat r;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += a[4 * i + k] * b[4 * k + j];
            r[4 * i + j] = s;
        }
    std::memcpy(out, r, sizeof(Mat));
}

// a^n by squaring, n >= 0
inline void mat_pow(const Mat a, int64_t n, Mat out) {
    Mat r = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, p;
    std::memcpy(p, a, sizeof(Mat));
    while (n > 0) {
        if (n & 1) mat_mul(r, p, r);
        n >>= 1;
        if (n) mat_mul(p, p, p);
    }
    std::memcpy(out, r, sizeof(Mat));
}

// (float)(T m T^-1), T = [1 0 0 0; 0 1 0 0; 0 0 1 1; 0 0 0 k]
inline void to_f32(const Mat m, double k, float* out) {
    const Mat T = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1, 0, 0, 0, k}, Ti = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -1.0 / k, 0, 0, 0, 1.0 / k};
    Mat r;
    mat_mul(T, m, r);
    mat_mul(r, Ti, r);
    for (int i = 0; i < 16; ++i) out[i] = (float)r[i];
}

// The ten coefficients of the header at rate fs, in double.
inline void coefficients(int fs, double* c) {
    const double pi = 3.14159265358979323846;
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(pi * f0 / fs), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        c[0] = (Vh + Vb * K / Q + K * K) / a0;
        c[1] = 2.0 * (K * K - Vh) / a0;
        c[2] = (Vh - Vb * K / Q + K * K) / a0;
        c[3] = 2.0 * (K * K - 1.0) / a0;
        c[4] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(pi * f0 / fs);
        const double a0 = 1.0 + K / Q + K * K;
        c[5] = 1.0;
        c[6] = -2.0;
        c[7] = 1.0;
        c[8] = 2.0 * (K * K - 1.0) / a0;
        c[9] = (1.0 - K / Q + K * K) / a0;
    }
}

// 0, or -1 with a message in why[160].
inline int design(int fs, Design& d, char* why) {
    if (fs < VTTS_LOUDNESS_MIN_RATE || fs > VTTS_LOUDNESS_MAX_RATE) {
        std::snprintf(why, 160, "sample_rate must be in %d .. %d (got %d)", VTTS_LOUDNESS_MIN_RATE, VTTS_LOUDNESS_MAX_RATE, fs);
        return -1;
    }
    if (fs % 10 != 0) {
        std::snprintf(why, 160, "sample_rate must be divisible by 10, so that a 100 ms hop is a whole number of samples (got %d)", fs);
        return -1;
    }
    d.fs = fs;
    d.H = fs / 10;
    coefficients(fs, d.coef);
    for (int i = 0; i < 10; ++i) d.t.cf[i] = (float)d.coef[i];
    // the transition matrix of the filter the kernel runs: from the ROUNDED coefficients
    const double a1 = d.t.cf[3], a2 = d.t.cf[4], c1 = d.t.cf[8], c2 = d.t.cf[9];
    const Mat A = {-a1, 1.0, 0.0, 0.0,          //
                   -a2, 0.0, 0.0, 0.0,          //
                   -2.0 - c1, 0.0, -c1, 1.0,    //
                   1.0 - c2, 0.0, -c2, 0.0};
    d.t.kappa = (float)std::sqrt(1.0 + c1 + c2);  // 1 + c1 + c2 = 4 K^2 / a0 > 0, and 50 or more ulps of c1 wide at 96 kHz
    const double kp = d.t.kappa;                  // the tables use the rounded value, as the kernel does
    Mat p = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    for (int i = 0; i < CHUNK; ++i) {  // (1, 0, 1, 0) A^i = row 0 + row 2 = h; h T^-1 = (h0, h1, h2, (h3 - h2) / kappa)
        const double h[4] = {p[0] + p[8], p[1] + p[9], p[2] + p[10], p[3] + p[11]};
        d.t.htab[4 * i + 0] = (float)h[0];
        d.t.htab[4 * i + 1] = (float)h[1];
        d.t.htab[4 * i + 2] = (float)h[2];
        d.t.htab[4 * i + 3] = (float)((h[3] - h[2]) / kp);
        mat_mul(A, p, p);
    }
    Mat m;
    for (int k = 0; k < 8; ++k) {
        mat_pow(A, (int64_t)CHUNK * k, m);
        to_f32(m, kp, d.t.lo + 16 * k);
        mat_pow(A, (int64_t)CHUNK * 8 * k, m);
        to_f32(m, kp, d.t.hi + 16 * k);
    }
    mat_pow(A, (int64_t)CHUNK * LANES, m);
    to_f32(m, kp, d.t.wave);
    mat_pow(A, (int64_t)SEGMENT, m);
    to_f32(m, kp, d.t.seg);
    return 0;
}

inline int64_t num_hops(const Design& d, int64_t n) { return n / d.H; }
inline int64_t num_blocks(const Design& d, int64_t n) { return n / d.H >= 3 ? n / d.H - 3 : 0; }
inline int64_t num_segments(int64_t n) { return (n + SEGMENT - 1) / SEGMENT; }

// The workspace of measure() for N rows whose longest has S samples, as byte offsets: the doubles first.
struct Layout {
    int64_t nseg = 0, nhop = 0;  // per-row strides of the arrays below (at least 1 each)
    size_t partial = 0;          // double [N][nseg][SLOTS]: a segment's share of the hops it meets, slot = hop - (segment's first hop)
    size_t hops = 0;             // double [N][nhop]: e_j
    size_t state = 0;            // float  [N][nseg][4]: a segment's end state from a zero incoming state
    size_t peak = 0;             // float  [N][nseg]
    size_t bytes = 0;
};

inline Layout layout(const Design& d, int N, int64_t S) {
    Layout l;
    l.nseg = num_segments(S) > 0 ? num_segments(S) : 1;
    l.nhop = num_hops(d, S) > 0 ? num_hops(d, S) : 1;
    const size_t n = (size_t)N;
    l.partial = 0;
    l.hops = l.partial + n * (size_t)l.nseg * SLOTS * sizeof(double);
    l.state = l.hops + n * (size_t)l.nhop * sizeof(double);
    l.peak = l.state + n * (size_t)l.nseg * 4 * sizeof(float);
    l.bytes = l.peak + n * (size_t)l.nseg * sizeof(float);
    l.bytes = (l.bytes + 255) / 256 * 256;
    return l;
}

// The slot of hop j in segment s's partial sums, and the segments hop j meets: what the two kernels must agree on.
inline int64_t first_hop(const Design& d, int64_t s) { return s * SEGMENT / d.H; }
inline int64_t hop_first_segment(const Design& d, int64_t j) { return j * d.H / SEGMENT; }
inline int64_t hop_last_segment(const Design& d, int64_t j) { return ((j + 1) * d.H - 1) / SEGMENT; }

}  // namespace vtts_loudness_design
