// Host side of the audio stage (include/vtts_audio.h): the prototype filter in double, the phase-major fp32 tap table, the size of a
// workgroup's input span and the row arithmetic of forward().  Plain C++ with no HIP in it, so that a stand-alone program can run
// it under the host sanitizers (tools/audio_design_check.cpp); audio.hip is its only other user.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/vtts_audio.h"

namespace vtts_audio_design {

constexpr int OPB = VTTS_AUDIO_OUT_PER_BLOCK;

struct Design {
    int in_rate = 0, out_rate = 0;
    int L = 1, M = 1, half = 0;
    int kp4 = 0;                 // taps per phase in the table: ceil((2 half + 1) / L), rounded up to a multiple of 4
    std::vector<double> proto;   // h[-half .. half]
    int minv = 0;                // M^-1 mod L (0 for L = 1): output i = s minv mod L of a run of L outputs has phase p0 + s
    // Phase p's taps reversed and right-aligned, row[p][kp4 - 1 - j] = (float)h[p + j L - half] with zeros where p + j L > 2 half, stored
    // four taps at a time with the phase running fastest: table[(c L + p) 4 + e] = row[p][4 c + e].
    std::vector<float> table;
    int span_floats = 0;         // LDS floats a workgroup's staged span needs at most
    bool identity = false;       // in_rate == out_rate: no filter
};

inline int64_t gcd64(int64_t a, int64_t b) {
    while (b) {
        const int64_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// modified Bessel function of the first kind, order 0: sum_k ((x / 2)^k / k!)^2, every term positive
inline double bessel_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-20 * sum) break;
    }
    return sum;
}

// floor(a / b) for b > 0
inline int64_t floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// The span of a workgroup: inputs floor8(q0 - (kp4 - 1)) .. q0 + (p0 + (OPB - 1) M) / L, staged in chunks of 8.
inline int64_t span_floats_for(int L, int M, int kp4) {
    const int64_t reach = ((int64_t)(L - 1) + (int64_t)(OPB - 1) * M) / L;  // largest q - q0 inside a block
    const int64_t n = reach + (kp4 - 1) + 7 + 1;
    return (n + 7) / 8 * 8;
}

// 0, or a negative value with `why` filled in (printf-ready text, at most 159 characters)
inline int design(int in_rate, int out_rate, Design& d, char (&why)[160]) {
    why[0] = 0;
    if (in_rate <= 0 || out_rate <= 0) {
        snprintf(why, sizeof why, "rates must be positive (got in_rate %d, out_rate %d)", in_rate, out_rate);
        return -1;
    }
    const int64_t g = gcd64(in_rate, out_rate);
    const int64_t L = out_rate / g, M = in_rate / g, R = L > M ? L : M;
    if (R > VTTS_AUDIO_MAX_R) {
        snprintf(why, sizeof why, "%d -> %d Hz is %lld / %lld: max(L, M) must not pass %d", in_rate, out_rate, (long long)L, (long long)M, VTTS_AUDIO_MAX_R);
        return -1;
    }
    d.in_rate = in_rate;
    d.out_rate = out_rate;
    d.L = (int)L;
    d.M = (int)M;
    d.half = (int)(VTTS_AUDIO_ZEROS * R);
    d.identity = in_rate == out_rate;
    const int ntaps = 2 * d.half + 1;
    const int kp = (ntaps + d.L - 1) / d.L;
    d.kp4 = (kp + 3) / 4 * 4;
    const int64_t span = span_floats_for(d.L, d.M, d.kp4);
    if (span * (int64_t)sizeof(float) > VTTS_AUDIO_MAX_SPAN_BYTES) {
        snprintf(why, sizeof why, "%d -> %d Hz decimates by %lld / %lld: a workgroup's input span of %lld bytes passes %d", in_rate, out_rate,
                 (long long)M, (long long)L, (long long)(span * 4), VTTS_AUDIO_MAX_SPAN_BYTES);
        return -1;
    }
    d.span_floats = (int)span;

    const double pi = 3.14159265358979323846;
    const double i0b = bessel_i0(VTTS_AUDIO_BETA);
    d.proto.assign(ntaps, 0.0);
    double sum = 0.0;
    for (int n = -d.half; n <= d.half; ++n) {
        const double x = (double)n / (double)R;
        const double sinc = n == 0 ? 1.0 : std::sin(pi * x) / (pi * x);
        const double r = (double)n / (double)d.half;
        const double arg = 1.0 - r * r;
        const double win = bessel_i0(VTTS_AUDIO_BETA * std::sqrt(arg > 0.0 ? arg : 0.0)) / i0b;
        d.proto[n + d.half] = sinc / (double)R * win;
        sum += d.proto[n + d.half];
    }
    for (double& v : d.proto) v = (double)L * v / sum;
    d.table.assign((size_t)d.L * d.kp4, 0.0f);
    for (int p = 0; p < d.L; ++p)
        for (int j = 0; j < d.kp4; ++j) {
            const int64_t k = (int64_t)p + (int64_t)j * d.L;
            const int i = d.kp4 - 1 - j;
            if (k < ntaps) d.table[((size_t)(i >> 2) * d.L + p) * 4 + (i & 3)] = (float)d.proto[k];  // rounded once
        }
    d.minv = 0;
    for (int v = 1; v < d.L; ++v)
        if ((int64_t)v * d.M % d.L == 1) d.minv = v;
    return 0;
}

// row[p][i] of the table
inline float table_at(const Design& d, int p, int i) { return d.table[((size_t)(i >> 2) * d.L + p) * 4 + (i & 3)]; }

inline int64_t out_samples(const Design& d, int64_t n_in) { return d.identity ? n_in : (n_in * d.L + d.M - 1) / d.M; }

// forward()'s rows: every length checked, each row's first output element (strided: b O_stride; packed: the running sum) and the
// output count the launch grid has to cover.  0, or a negative value: -1 = invalid argument, -6 = shape.
struct Rows {
    std::vector<int32_t> len;
    std::vector<int64_t> off;
    int64_t cover = 0;  // outputs per row the grid covers: O_stride, or the longest row's So when packed
    int64_t total = 0;  // elements of the output the call writes
};
inline int plan_rows(const Design& d, int N, int64_t S_stride, const int32_t* lengths, int64_t O_stride, Rows& r, char (&why)[160]) {
    why[0] = 0;
    if (N <= 0) {
        snprintf(why, sizeof why, "N must be positive (got %d)", N);
        return -1;
    }
    if (S_stride < 1 || S_stride > 0x7fffffff) {
        snprintf(why, sizeof why, "S_stride must be in 1 .. 2^31 - 1 (got %lld)", (long long)S_stride);
        return -6;
    }
    if (O_stride < 0) {
        snprintf(why, sizeof why, "O_stride must be 0 (packed) or the output rows' pitch (got %lld)", (long long)O_stride);
        return -6;
    }
    r.len.assign(N, 0);
    r.off.assign(N, 0);
    int64_t longest = 0, run = 0;
    for (int b = 0; b < N; ++b) {
        const int64_t len = lengths ? lengths[b] : S_stride;
        if (len < 0 || len > S_stride) {
            snprintf(why, sizeof why, "lengths[%d] = %lld is outside 0 .. S_stride = %lld", b, (long long)len, (long long)S_stride);
            return -6;
        }
        const int64_t so = out_samples(d, len);
        r.len[b] = (int32_t)len;
        r.off[b] = O_stride ? (int64_t)b * O_stride : run;
        run += so;
        if (so > longest) longest = so;
    }
    if (O_stride && O_stride < longest) {
        snprintf(why, sizeof why, "O_stride = %lld is below the longest row's %lld output samples", (long long)O_stride, (long long)longest);
        return -6;
    }
    r.cover = O_stride ? O_stride : longest;
    r.total = O_stride ? (int64_t)N * O_stride : run;
    if ((r.cover + OPB - 1) / OPB > 0x7fffffff) {
        snprintf(why, sizeof why, "rows of %lld output samples are too long", (long long)r.cover);
        return -6;
    }
    return 0;
}

}  // namespace vtts_audio_design
