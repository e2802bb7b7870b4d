// Stand-alone run of the audio stage's host code (viettts_amd/csrc/audio_design.h: the prototype, the phase-major tap table, the span
// bound and forward()'s row arithmetic) under the host sanitizers.  No HIP, no GPU, not loaded into Python:
//
//     clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/audio_design_check.cpp -o audio_design_check
//     ./audio_design_check
//
// It designs every ratio the tests use and the table's extremes, replays the kernel's indexing over each design on the host (every
// span and table index a workgroup forms, checked against the allocated sizes) and walks the argument checks.  Prints "ok" or aborts.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../viettts_amd/csrc/audio_design.h"

namespace ad = vtts_audio_design;

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            abort();                                                   \
        }                                                              \
    } while (0)

// The kernel's index arithmetic for the block that starts at output m0 of a row of S samples: the largest span index staged or read
// and every table index, against span_floats and the table's size.  Returns the block's first output by the table against the
// definition's sum, to tie the table's layout to the contract.
static void replay_block(const ad::Design& d, int64_t S, int64_t m0) {
    const int64_t So = ad::out_samples(d, S);
    if (m0 >= So) return;
    const int64_t live = So - m0 < ad::OPB ? So - m0 : ad::OPB;
    const int64_t t0 = m0 * d.M + d.half, q0 = t0 / d.L, p0 = t0 - q0 * d.L;
    const int64_t nb = ad::floor_div(q0 - (d.kp4 - 1), 8) * 8;
    const int64_t nspan = q0 + (p0 + (live - 1) * d.M) / d.L - nb + 1;
    CHECK(nspan >= 1 && (nspan + 7) / 8 * 8 <= d.span_floats);
    const int64_t sbase = (q0 - nb) - (d.kp4 - 1);
    CHECK(sbase >= 0);
    std::vector<float> x((size_t)S);
    for (int64_t i = 0; i < S; ++i) x[(size_t)i] = (float)((i * 2654435761u % 2001) / 1000.0 - 1.0);
    // the kernel's slots: slot g = chunk L + s computes output i = chunk L + (s minv mod L), whose phase is p0 + s: every output once
    const int64_t nslots = (live + d.L - 1) / d.L * d.L;
    std::vector<char> seen((size_t)live, 0);
    for (int64_t g = 0; g < nslots; ++g) {
        const int64_t chunk = g / d.L, s = g - chunk * d.L;
        CHECK(s * d.minv <= 0x7fffffff);
        const int64_t i = chunk * d.L + s * d.minv % d.L;
        if (i >= live) continue;
        CHECK(!seen[(size_t)i]);
        seen[(size_t)i] = 1;
        CHECK((p0 + i * d.M) % d.L == (p0 + s) % d.L && p0 + s < 2 * (int64_t)d.L);
    }
    for (int64_t i = 0; i < live; ++i) CHECK(seen[(size_t)i]);
    for (int64_t i = 0; i < live; i += (live > 64 ? live / 7 : 1)) {
        const int64_t u = p0 + i * d.M;
        CHECK(u <= 0x7fffffff);
        const int64_t dq = u / d.L, p = u - dq * d.L;
        CHECK(sbase + dq + d.kp4 - 1 < nspan);
        CHECK((((size_t)(d.kp4 / 4 - 1) * d.L + p) * 4 + 3) < d.table.size());
        // the table's chain against the definition, in double
        double by_table = 0.0, by_def = 0.0;
        for (int c = 0; c < d.kp4; ++c) {
            const int64_t n = nb + sbase + dq + c;
            const double xv = (n >= 0 && n < S) ? x[(size_t)n] : 0.0;
            by_table += xv * ad::table_at(d, (int)p, c);
        }
        const int64_t m = m0 + i;
        for (int64_t n = 0; n < S; ++n) {
            const int64_t k = m * d.M - n * d.L + d.half;
            if (k >= 0 && k <= 2 * (int64_t)d.half) by_def += (double)x[(size_t)n] * (double)(float)d.proto[(size_t)k];
        }
        CHECK(std::fabs(by_table - by_def) <= 1e-9);
    }
}

int main() {
    char why[160];
    const int pairs[][2] = {{16000, 48000}, {16000, 8000}, {16000, 24000}, {16000, 44100}, {44100, 16000}, {44100, 32000}, {48000, 16000},
                            {16000, 16000}, {2048, 2047}, {2047, 2048}, {1, 2048}, {30, 1}, {8000, 44100}, {44100, 8000}};
    for (const auto& pr : pairs) {
        ad::Design d;
        CHECK(ad::design(pr[0], pr[1], d, why) == 0);
        CHECK((int64_t)d.L * pr[0] == (int64_t)d.M * pr[1]);
        CHECK((int)d.proto.size() == 2 * d.half + 1 && d.table.size() == (size_t)d.L * d.kp4 && d.kp4 % 4 == 0);
        double sum = 0.0;
        for (size_t i = 0; i < d.proto.size(); ++i) {
            sum += d.proto[i];
            CHECK(std::fabs(d.proto[i] - d.proto[d.proto.size() - 1 - i]) <= 1e-15 * d.L);
        }
        CHECK(std::fabs(sum - d.L) <= 1e-11 * d.L);
        double tsum = 0.0;
        for (float v : d.table) tsum += v;
        CHECK(std::fabs(tsum - d.L) <= 1e-4 * d.L);  // every tap is in the table once (fp32 roundings apart)
        for (int64_t S : {1, 2, 17, 385, 1024, 4097, 6000})
            for (int64_t m0 = 0; m0 < ad::out_samples(d, S); m0 += ad::OPB) replay_block(d, S, m0);
        // a block far into a long row: m M and n L beyond 2^31
        const int64_t S = 2000000000;
        const int64_t So = ad::out_samples(d, S);
        {
            const int64_t m0 = (So - 1) / ad::OPB * ad::OPB;
            const int64_t live = So - m0;
            const int64_t t0 = m0 * d.M + d.half, q0 = t0 / d.L, p0 = t0 - q0 * d.L;
            const int64_t nb = ad::floor_div(q0 - (d.kp4 - 1), 8) * 8;
            const int64_t nspan = q0 + (p0 + (live - 1) * d.M) / d.L - nb + 1;
            CHECK(nspan >= 1 && (nspan + 7) / 8 * 8 <= d.span_floats);
            CHECK(q0 + (p0 + (live - 1) * d.M) / d.L <= S - 1 + d.kp4);  // the last output's window ends near the row's end
        }
        // forward()'s rows
        ad::Rows r;
        const int32_t lens[4] = {6000, 1, 385, 4097};
        CHECK(ad::plan_rows(d, 4, 6000, lens, 0, r, why) == 0);
        int64_t run = 0;
        for (int b = 0; b < 4; ++b) {
            CHECK(r.off[b] == run);
            run += ad::out_samples(d, lens[b]);
        }
        CHECK(r.total == run && r.cover == ad::out_samples(d, 6000));
        const int64_t pitch = ad::out_samples(d, 6000) + 3;
        CHECK(ad::plan_rows(d, 4, 6000, lens, pitch, r, why) == 0 && r.off[3] == 3 * pitch && r.total == 4 * pitch && r.cover == pitch);
        CHECK(ad::plan_rows(d, 4, 6000, lens, pitch - 4, r, why) == -6 && strstr(why, "O_stride"));
        CHECK(ad::plan_rows(d, 4, 5999, lens, 0, r, why) == -6 && strstr(why, "lengths[0]"));
        const int32_t neg[2] = {5, -1};
        CHECK(ad::plan_rows(d, 2, 6000, neg, 0, r, why) == -6 && strstr(why, "lengths[1]"));
        CHECK(ad::plan_rows(d, 0, 6000, nullptr, 0, r, why) == -1);
        CHECK(ad::plan_rows(d, 1, 0, nullptr, 0, r, why) == -6);
        CHECK(ad::plan_rows(d, 1, (int64_t)1 << 31, nullptr, 0, r, why) == -6);
        CHECK(ad::plan_rows(d, 1, 6000, nullptr, -1, r, why) == -6);
        const int64_t so_max = ad::out_samples(d, 0x7fffffff);  // the longest row there is: refused only where the grid cannot cover it
        if ((so_max + ad::OPB - 1) / ad::OPB > 0x7fffffff)
            CHECK(ad::plan_rows(d, 3, 0x7fffffff, nullptr, 0, r, why) == -6 && strstr(why, "too long"));
        else
            CHECK(ad::plan_rows(d, 3, 0x7fffffff, nullptr, 0, r, why) == 0 && r.total == 3 * so_max);
    }
    ad::Design d;
    CHECK(ad::design(0, 16000, d, why) == -1 && strstr(why, "positive"));
    CHECK(ad::design(16000, -5, d, why) == -1);
    CHECK(ad::design(16000, 16001, d, why) == -1 && strstr(why, "2048"));
    CHECK(ad::design(2049, 1, d, why) == -1);
    CHECK(ad::design(2147483647, 2147483646, d, why) == -1);
    CHECK(ad::design(44100, 1000, d, why) == -1 && strstr(why, "span"));  // 441 / 10: within the table, beyond the staged span
    CHECK(ad::floor_div(-1, 8) == -1 && ad::floor_div(-8, 8) == -1 && ad::floor_div(-9, 8) == -2 && ad::floor_div(7, 8) == 0);
    printf("ok\n");
    return 0;
}
