// Host-only check of the streamed resampler's index arithmetic (viettts_amd/csrc/rsstream_host.h, with audio_design.h for the ratios) against
// a brute-force restatement, under the address and undefined-behaviour sanitizers.  It links nothing of the HIP runtime and needs no GPU:
//
//   clang++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tools/check_rsstream_host.cpp -o /tmp/check_rsstream_host \
//       && /tmp/check_rsstream_host
//
// For every rate pair of the tests and random chunkings of random rows (zero counts, single samples and chunks of several tiles among them):
// F' is monotone and is the count of outputs whose newest input has arrived (by search); F' on `last` equals out_samples; the history never
// passes kp4 - 1 samples; every tile's span stays within span_floats; and the model replays the kernel's reads: it keeps the history and the
// chunk as vectors of ABSOLUTE sample indices, so an index that where_is() gets wrong reads the wrong sample's number, and one out of bounds
// is the sanitizer's.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../viettts_amd/csrc/audio_design.h"
#include "../viettts_amd/csrc/rsstream_host.h"

namespace ad = vtts_audio_design;
namespace rh = vtts_rsstream_host;

static long failures = 0;
#define EXPECT(cond, ...)                     \
    do {                                      \
        if (!(cond)) {                        \
            if (failures < 20) {              \
                printf("WRONG: %s: ", #cond); \
                printf(__VA_ARGS__);          \
                printf("\n");                 \
            }                                 \
            ++failures;                       \
        }                                     \
    } while (0)

// the rule by search: the outputs whose newest input q(m) <= R' - 1
static int64_t emit_brute(const rh::Ratio& r, int64_t R, int64_t F, int64_t count, bool last) {
    const int64_t n = R + count;
    if (r.identity) return n;
    if (last) {
        int64_t m = 0;
        while (m * r.M < n * r.L) ++m;  // ceil(n L / M)
        return m;
    }
    int64_t m = 0;
    while ((m * r.M + r.half) / r.L <= n - 1) ++m;
    return m > F ? m : F;
}

static void one_row(const ad::Design& d, const rh::Ratio& r, int64_t S, std::mt19937& rng, int max_chunk) {
    std::vector<int64_t> hist[2];  // absolute indices, as the two device buffers hold samples
    hist[0].assign(rh::hist_floats(r), -7);
    hist[1].assign(rh::hist_floats(r), -7);
    int par = 0;
    int64_t R = 0, F = 0, emitted_total = 0;
    bool closed = false;
    while (!closed) {
        int64_t cnt = 0;
        switch (rng() % 4) {
            case 0: cnt = 0; break;
            case 1: cnt = 1; break;
            default: cnt = (int64_t)(rng() % (unsigned)max_chunk) + 1;
        }
        if (cnt > S - R) cnt = S - R;
        const bool last = R + cnt == S && (rng() % 2 || cnt == 0);
        const int64_t Rn = R + cnt, Fn = rh::emit_rule(r, R, F, cnt, last);
        EXPECT(Fn >= F, "F' %lld < F %lld", (long long)Fn, (long long)F);
        EXPECT(Fn == emit_brute(r, R, F, cnt, last), "R %lld count %lld last %d: F' %lld", (long long)R, (long long)cnt, (int)last, (long long)Fn);
        EXPECT(F == rh::emitted_of(r, R), "F %lld is not a function of R %lld", (long long)F, (long long)R);
        EXPECT(Fn - F <= rh::max_emit(r, cnt), "emit %lld passes max_emit %lld", (long long)(Fn - F), (long long)rh::max_emit(r, cnt));
        if (last) EXPECT(Fn == ad::out_samples(d, Rn), "last: F' %lld, out_samples %lld", (long long)Fn, (long long)ad::out_samples(d, Rn));
        std::vector<int64_t> chunk((size_t)cnt);
        for (int64_t i = 0; i < cnt; ++i) chunk[(size_t)i] = R + i;
        auto fetch = [&](int64_t g) -> int64_t {  // the kernel's lookup; -1 stands for a zero
            const rh::Where w = rh::where_is(R, cnt, rh::hist_base(r, F), g);
            if (w.src == rh::SRC_CHUNK) return chunk.at((size_t)w.index);
            if (w.src == rh::SRC_HIST) return hist[par].at((size_t)w.index);
            return -1;
        };
        if (!r.identity) {
            // tile 0: the next history into the other buffer
            if (!last) {
                const int64_t Bn = rh::hist_base(r, Fn);
                EXPECT(Rn - Bn <= r.kp4 - 1, "history of %lld samples passes kp4 - 1 = %d", (long long)(Rn - Bn), r.kp4 - 1);
                EXPECT(rh::newest_of(r, Fn) >= Rn, "q(F') %lld < R' %lld", (long long)rh::newest_of(r, Fn), (long long)Rn);
                for (int64_t g = Bn; g < Rn; ++g) {
                    const int64_t v = fetch(g);
                    EXPECT(v == g, "history: x[%lld] read as %lld", (long long)g, (long long)v);
                    hist[par ^ 1].at((size_t)(g - Bn)) = v;
                }
            }
            // every tile: its span, and what each output's chain reads through it
            for (int64_t m0 = F; m0 < Fn; m0 += rh::OPB) {
                const int live = (int)(Fn - m0 < rh::OPB ? Fn - m0 : rh::OPB);
                const rh::Span sp = rh::span_of(r, m0, live);
                EXPECT(sp.count >= 1 && (sp.count + 7) / 8 * 8 <= d.span_floats, "span of %d floats passes %d", sp.count, d.span_floats);
                EXPECT(sp.sbase >= 0 && sp.sbase < 8, "sbase %d", sp.sbase);
                std::vector<int64_t> span((size_t)sp.count);
                for (int k = 0; k < sp.count; ++k) span[(size_t)k] = fetch(sp.first + k);
                for (int i = 0; i < live; i += (live > 64 ? 37 : 1)) {
                    const int dq = (int)((sp.p0 + (int64_t)i * r.M) / r.L);
                    const int64_t q = rh::newest_of(r, m0 + i);
                    EXPECT(sp.q0 + dq == q, "output %lld: newest %lld, the block says %lld", (long long)(m0 + i), (long long)q, (long long)(sp.q0 + dq));
                    EXPECT((sp.p0 + (int64_t)i * r.M) % r.L == ((m0 + i) * r.M + r.half) % r.L, "phase of output %lld", (long long)(m0 + i));
                    for (int t = 0; t < r.kp4; ++t) {
                        const int64_t g = q - (r.kp4 - 1) + t;
                        const int64_t v = span.at((size_t)(sp.sbase + dq + t));
                        const int64_t want = g < 0 || g >= Rn ? -1 : g;
                        EXPECT(v == want, "output %lld tap %d: x[%lld] read as %lld", (long long)(m0 + i), t, (long long)g, (long long)v);
                        if (!last) EXPECT(g < Rn, "output %lld reads x[%lld] before it arrived (R' %lld)", (long long)(m0 + i), (long long)g, (long long)Rn);
                    }
                }
            }
        }
        emitted_total += Fn - F;
        R = Rn;
        F = Fn;
        if (last)
            closed = true;
        else
            par ^= 1;
    }
    EXPECT(emitted_total == ad::out_samples(d, S), "a row of %lld samples emitted %lld", (long long)S, (long long)emitted_total);
}

int main() {
    const int rates[][2] = {{16000, 48000}, {16000, 8000}, {16000, 24000}, {16000, 44100}, {16000, 22050}, {44100, 16000}, {16000, 16000}, {48000, 1600}};
    std::mt19937 rng(12345);
    long rows = 0;
    for (const auto& io : rates) {
        ad::Design d;
        char why[160];
        if (ad::design(io[0], io[1], d, why) != 0) {
            printf("design %d -> %d: %s\n", io[0], io[1], why);
            return 2;
        }
        const rh::Ratio r = {d.L, d.M, d.half, d.kp4, d.identity ? 1 : 0};
        const int delay = (d.half + d.L - 1) / d.L;
        const int64_t lens[] = {0, 1, delay - 1, delay, delay + 1, 300, 3001, 20000};
        for (int64_t S : lens)
            for (int rep = 0; rep < 6; ++rep) {
                one_row(d, r, S, rng, rep < 3 ? 700 : 9000);
                ++rows;
            }
        // the cursors near the end of the range: 64-bit products, no overflow for the sanitizer to find
        const int64_t big = 0x7fffffff;
        const int64_t Fb = rh::emitted_of(r, big - 5);
        EXPECT(rh::emit_rule(r, big - 5, Fb, 5, 1) == ad::out_samples(d, big), "%d -> %d at 2^31 - 1", io[0], io[1]);
        EXPECT(big - rh::hist_base(r, rh::emit_rule(r, big - 5, Fb, 5, 0)) <= (r.identity ? big : r.kp4 - 1), "history at 2^31 - 1");
    }
    if (failures) {
        printf("check_rsstream_host: %ld FAILURES\n", failures);
        return 1;
    }
    printf("check_rsstream_host: %ld rows, all checks passed\n", rows);
    return 0;
}
