// Stand-alone run of the loudness meter's host code (viettts_amd/csrc/loudness_design.h: the K-weighting coefficients, the transition
// matrix's powers, the homogeneous-response table, the workspace layout and the hop / segment arithmetic the two kernels share) under
// the host sanitizers.  No HIP, no GPU, not loaded into Python:
//
//     clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/loudness_design_check.cpp -o loudness_design_check
//     ./loudness_design_check
//
// For every rate the tests use and the range's ends it designs the tables, checks them against each other, and replays loud_scan_k
// and loud_gate_k on the host, lane by lane with the kernel's own index arithmetic (every LDS word, partial-sum slot and workspace
// element checked against the allocated sizes), against the plain sequential filter in double: the hop sums of the fp32 scheme have to
// stay within a quarter of the 0.1 LU meter tolerance.  Prints the distances it measured and "ok", or aborts.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../viettts_amd/csrc/loudness_design.h"

namespace ld = vtts_loudness_design;

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            abort();                                                   \
        }                                                              \
    } while (0)

static void matvec(const float* m, const float* s, float* r) {
    for (int i = 0; i < 4; ++i) r[i] = fmaf(m[4 * i + 3], s[3], fmaf(m[4 * i + 2], s[2], fmaf(m[4 * i + 1], s[1], m[4 * i] * s[0])));
}

// The plain filter in double with the ROUNDED coefficients: hop sums of a row.
static std::vector<double> sequential_hops(const ld::Design& d, const std::vector<float>& x) {
    const float* c = d.t.cf;
    double s1 = 0, s2 = 0, s3 = 0, s4 = 0;
    std::vector<double> e((size_t)ld::num_hops(d, (int64_t)x.size()), 0.0);
    for (size_t n = 0; n < x.size(); ++n) {
        const double v = x[n];
        const double y1 = c[0] * v + s1;
        s1 = c[1] * v - c[3] * y1 + s2;
        s2 = c[2] * v - c[4] * y1;
        const double z = y1 + s3;
        s3 = -2.0 * y1 - c[8] * z + s4;
        s4 = y1 - c[9] * z;
        const size_t j = n / (size_t)d.H;
        if (j < e.size()) e[j] += z * z;
    }
    return e;
}

// loud_scan_k (both launches) and the hop assembly of loud_gate_k for one row, on the host.
static std::vector<double> replay(const ld::Design& d, const std::vector<float>& x) {
    const int64_t len = (int64_t)x.size(), H = d.H;
    const ld::Layout l = ld::layout(d, 1, len);
    CHECK(l.partial % 8 == 0 && l.hops % 8 == 0 && l.state % 4 == 0 && l.peak % 4 == 0 && l.bytes >= l.peak + (size_t)l.nseg * 4);
    std::vector<double> partial((size_t)l.nseg * ld::SLOTS, -1.0), hops((size_t)l.nhop, -1.0);
    std::vector<float> state((size_t)l.nseg * 4, 0.0f);
    const int64_t nseg = ld::num_segments(len);
    CHECK(nseg <= l.nseg);
    const ld::Tables& t = d.t;
    for (int full = 0; full < 2; ++full)
        for (int64_t seg = 0; seg < nseg; ++seg) {
            const int64_t g0 = seg * ld::SEGMENT;
            if (!full && g0 + ld::SEGMENT >= len) continue;
            std::vector<float> xs((size_t)(ld::SEGMENT + ld::SEGMENT / ld::CHUNK), 0.0f);
            for (int i = 0; i < ld::CHUNK; ++i)
                for (int tid = 0; tid < 256; ++tid) {
                    const int pos = i * 256 + tid;
                    const int64_t g = g0 + pos;
                    xs.at((size_t)(pos + (pos >> 5))) = g < len ? x[(size_t)g] : 0.0f;
                }
            float p[256][4], e[256][4];
            for (int tid = 0; tid < 256; ++tid) {
                float* c = &xs.at((size_t)tid * (ld::CHUNK + 1));
                float s1 = 0, s2 = 0, s3 = 0, s4 = 0;
                for (int i = 0; i < ld::CHUNK; ++i) {
                    const float xi = c[i];
                    const float y1 = fmaf(t.cf[0], xi, s1);
                    s1 = fmaf(t.cf[1], xi, fmaf(-t.cf[3], y1, s2));
                    s2 = fmaf(t.cf[2], xi, -t.cf[4] * y1);
                    const float z = y1 + s3;
                    s3 = fmaf(-t.cf[8], z, s4 - 2.0f * y1);
                    s4 = fmaf(-t.cf[9], z, y1);
                    c[i] = z;
                }
                p[tid][0] = s1, p[tid][1] = s2, p[tid][2] = s3 + s4, p[tid][3] = t.kappa * s4;
            }
            for (int st = 0; st < 6; ++st) {  // the waves' scans
                const int dd = 1 << st;
                const float* m = st < 3 ? t.lo + (16 << st) : t.hi + (16 << (st - 3));
                float q[256][4];
                for (int tid = 0; tid < 256; ++tid)
                    for (int k = 0; k < 4; ++k) q[tid][k] = (tid & 63) >= dd ? p[tid - dd][k] : 0.0f;
                for (int tid = 0; tid < 256; ++tid)
                    if ((tid & 63) >= dd) {
                        float r[4];
                        matvec(m, q[tid], r);
                        for (int k = 0; k < 4; ++k) p[tid][k] += r[k];
                    }
            }
            for (int tid = 0; tid < 256; ++tid)
                for (int k = 0; k < 4; ++k) e[tid][k] = (tid & 63) ? p[tid - 1][k] : 0.0f;
            float sg[4] = {0, 0, 0, 0};
            if (full)
                for (int64_t j = 0; j < seg; ++j) {
                    float r[4];
                    matvec(t.seg, sg, r);
                    for (int k = 0; k < 4; ++k) sg[k] = r[k] + state.at((size_t)(4 * j + k));
                }
            float sw[ld::WAVES + 1][4];
            for (int k = 0; k < 4; ++k) sw[0][k] = sg[k];
            for (int w = 0; w < ld::WAVES; ++w) {
                float r[4];
                matvec(t.wave, sw[w], r);
                for (int k = 0; k < 4; ++k) sw[w + 1][k] = r[k] + p[64 * w + 63][k];
            }
            if (!full) {
                for (int k = 0; k < 4; ++k) state.at((size_t)(4 * seg + k)) = sw[ld::WAVES][k];
                continue;
            }
            const int64_t hS = g0 / H;
            double part[ld::WAVES * ld::SLOTS] = {};
            for (int tid = 0; tid < 256; ++tid) {
                const int lane = tid & 63, w = tid >> 6;
                float r[4], r2[4], sin_[4];
                matvec(t.hi + 16 * (lane >> 3), sw[w], r);
                matvec(t.lo + 16 * (lane & 7), r, r2);
                for (int k = 0; k < 4; ++k) sin_[k] = e[tid][k] + r2[k];
                const int64_t cg = g0 + (int64_t)tid * ld::CHUNK, hop0 = cg / H, left = (hop0 + 1) * H - cg;
                const int bnd = left < ld::CHUNK ? (int)left : ld::CHUNK;
                const int64_t wg = g0 + (int64_t)w * ld::CHUNK * 64, hA = wg / H, hB = (wg + ld::CHUNK * 64 - 1) / H;
                const float* c = &xs.at((size_t)tid * (ld::CHUNK + 1));
                for (int i = 0; i < ld::CHUNK; ++i) {
                    const float* h = t.htab + 4 * i;
                    const float z = fmaf(h[0], sin_[0], fmaf(h[1], sin_[1], fmaf(h[2], sin_[2], fmaf(h[3], sin_[3], c[i]))));
                    const int64_t hop = i < bnd ? hop0 : hop0 + 1;
                    CHECK(hop >= hA && hop <= hB && hop - hS >= 0 && hop - hS < ld::SLOTS);  // the slot the wave's butterfly writes
                    CHECK(hop == (cg + i) / H);
                    part[w * ld::SLOTS + (int)(hop - hS)] += (double)z * (double)z;
                }
            }
            for (int s = 0; s < ld::SLOTS; ++s)
                partial.at((size_t)(seg * ld::SLOTS + s)) = ((part[s] + part[ld::SLOTS + s]) + part[2 * ld::SLOTS + s]) + part[3 * ld::SLOTS + s];
        }
    const int64_t nH = ld::num_hops(d, len);
    CHECK(nH <= l.nhop);
    for (int64_t j = 0; j < nH; ++j) {
        const int64_t sA = ld::hop_first_segment(d, j), sB = ld::hop_last_segment(d, j);
        double acc = 0.0;
        for (int64_t s = sA; s <= sB; ++s) {
            const int64_t slot = j - ld::first_hop(d, s);
            CHECK(s < nseg && slot >= 0 && slot < ld::SLOTS);
            const double v = partial.at((size_t)(s * ld::SLOTS + slot));
            CHECK(v >= 0.0);  // written
            acc += v;
        }
        hops.at((size_t)j) = acc;
    }
    hops.resize((size_t)nH);
    return hops;
}

int main() {
    const int rates[] = {8000, 11020, 16000, 22050, 44100, 48000, 96000};
    for (int fs : rates) {
        ld::Design d;
        char why[160];
        CHECK(ld::design(fs, d, why) == 0 && d.H * 10 == fs);
        if (fs == 48000) {  // BS.1770-4, tables 1 and 2
            const double want[10] = {1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
                                     1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621};
            for (int i = 0; i < 10; ++i) CHECK(std::fabs(d.coef[i] - want[i]) <= 1e-12);
        }
        // lo[0] = hi[0] = I; lo[k] hi[j] = A^(CHUNK (k + 8 j)): lo[1]^8 = hi[1] up to the tables' rounding
        for (int i = 0; i < 16; ++i) CHECK(d.t.lo[i] == (i % 5 == 0 ? 1.0f : 0.0f) && d.t.hi[i] == d.t.lo[i]);
        {
            ld::Mat a, b;
            for (int i = 0; i < 16; ++i) a[i] = d.t.lo[16 + i];
            ld::mat_pow(a, 8, b);
            double scale = 0.0, worst = 0.0;
            for (int i = 0; i < 16; ++i) {
                scale = std::fmax(scale, std::fabs(b[i]));
                worst = std::fmax(worst, std::fabs(b[i] - d.t.hi[16 + i]));
            }
            printf("%d Hz: |lo[1]^8 - hi[1]| <= %.2e of %.2e\n", fs, worst, scale);
            CHECK(worst <= 1e-5 * scale);  // (in the carried coordinates: 1e-3 and worse in the filter's own)
        }
        CHECK(d.t.htab[0] == 1.0f && d.t.htab[1] == 0.0f && d.t.htab[2] == 1.0f && d.t.htab[3] == (float)(-1.0 / (double)d.t.kappa));  // (1, 0, 1, 0) T^-1
        CHECK(d.t.kappa > 0.0f && d.t.kappa < 0.1f);
        // rows at the grid's edges: a state carry over three segments, with a DC step the high-pass has to forget and a low tone
        const int64_t lens[] = {4 * d.H - 1, ld::SEGMENT, ld::SEGMENT + 1, 2 * ld::SEGMENT + 1, 3 * ld::SEGMENT + 5 * d.H + 7};
        double worst = 0.0;
        for (int64_t len : lens) {
            std::vector<float> x((size_t)len);
            for (int64_t n = 0; n < len; ++n)
                x[(size_t)n] = (float)(0.25 + 0.25 * std::sin(2.0 * 3.14159265358979323846 * 30.0 * (double)n / fs) + 0.01 * std::sin(2.0 * 3.14159265358979323846 * 1000.0 * (double)n / fs));
            const std::vector<double> want = sequential_hops(d, x), got = replay(d, x);
            CHECK(want.size() == got.size() && (int64_t)got.size() == len / d.H);
            for (size_t j = 0; j < got.size(); ++j) {
                const double err = std::fabs(got[j] - want[j]) / want[j];
                if (err > worst) worst = err;
                // a quarter of the 0.1 LU the meter may be off by (EBU Tech 3341): 10^(0.025 / 10) - 1
                if (!(err <= 5.7e-3)) fprintf(stderr, "%d Hz, %lld samples, hop %zu: %.9g against %.9g\n", fs, (long long)len, j, got[j], want[j]);
                CHECK(err <= 5.7e-3);
            }
        }
        printf("%d Hz: hop sums of the chunked float scheme within %.2e (relative) of the sequential filter in double\n", fs, worst);
    }
    ld::Design d;
    char why[160];
    CHECK(ld::design(7990, d, why) != 0 && ld::design(96010, d, why) != 0 && ld::design(16005, d, why) != 0 && ld::design(0, d, why) != 0);
    CHECK(ld::design(16000, d, why) == 0 && ld::num_blocks(d, 0) == 0 && ld::num_blocks(d, 6399) == 0 && ld::num_blocks(d, 6400) == 1 && ld::num_blocks(d, 8000) == 2);
    printf("ok\n");
    return 0;
}
