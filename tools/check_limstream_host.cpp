// Host-only check of the streamed limiter's index arithmetic (viettts_amd/csrc/limstream_host.h) against a brute-force restatement, under
// the address and undefined-behaviour sanitizers.  It links nothing of the HIP runtime and needs no GPU:
//
//   clang++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tools/check_limstream_host.cpp -o /tmp/check_limstream_host \
//       && /tmp/check_limstream_host
//
// For W in {1, 80, 960}, every count 0 .. 3 TILE, last and not last, a row is pushed twice (a first push of one of several sizes, then the
// count under test).  The model keeps the state as a vector of ABSOLUTE sample indices and the chunk likewise, so an index that where_is()
// gets wrong reads the wrong sample's number, and one out of bounds is the sanitizer's.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../viettts_amd/csrc/limstream_host.h"

namespace lh = vtts_limstream_host;

static long failures = 0;
#define EXPECT(cond, ...)                   \
    do {                                    \
        if (!(cond)) {                      \
            if (failures < 20) {            \
                printf("WRONG: %s: ", #cond); \
                printf(__VA_ARGS__);        \
                printf("\n");               \
            }                               \
            ++failures;                     \
        }                                   \
    } while (0)

// the rule by search: the largest multiple of 16 whose samples all have 2 W + 24 samples after them
static int64_t emit_brute(int W, int64_t R, int64_t F, int64_t count, bool last) {
    const int64_t r = R + count;
    if (last) return r;
    int64_t f = F;
    for (int64_t t = 0; t <= r; t += 16)
        if (t == 0 || (t - 1) + 2 * W + 24 <= r - 1) f = t > f ? t : f;
    return f;
}

struct Model {
    int W;
    int64_t R = 0, F = 0;
    std::vector<int64_t> state;  // absolute indices of the samples the state holds

    // one push: checks every tile's span (every sample of it when `full`, else its ends and the seams), then moves the state
    void push(int64_t count, bool last, bool full) {
        const int64_t Rn = R + count, Fn = lh::emit_rule(W, R, F, count, last);
        EXPECT(Fn == emit_brute(W, R, F, count, last), "W %d R %lld F %lld count %lld last %d: %lld", W, (long long)R, (long long)F, (long long)count, (int)last, (long long)Fn);
        EXPECT(F == lh::emitted_of(W, R), "an open row's F follows from R: W %d R %lld F %lld", W, (long long)R, (long long)F);
        EXPECT(Fn >= F && Fn <= Rn && (last || Fn % 16 == 0), "W %d", W);
        std::vector<int64_t> chunk((size_t)count);
        for (int64_t i = 0; i < count; ++i) chunk[(size_t)i] = R + i;
        const int64_t emit = Fn - F;
        const int nt = lh::tiles_of(emit);
        EXPECT(nt >= 1 && (int64_t)nt * lh::TILE >= emit && ((int64_t)nt - 1) * lh::TILE < (emit > 0 ? emit : 1), "tiles");
        EXPECT(nt <= lh::max_tiles(W, count < 1 ? 1 : (int)count), "a push of %lld samples takes %d tiles", (long long)count, nt);
        auto look = [&](int64_t g) {
            const lh::Where w = lh::where_is(W, R, F, count, g);
            const bool inside = g >= 0 && g < Rn;
            if (!inside) {
                EXPECT(w.src == lh::SRC_ZERO, "g %lld outside the row", (long long)g);
            } else if (g >= R) {
                EXPECT(w.src == lh::SRC_CHUNK && w.index >= 0 && w.index < count, "chunk index");
                if (w.src == lh::SRC_CHUNK && w.index >= 0 && w.index < count) EXPECT(chunk[(size_t)w.index] == g, "chunk sample");
            } else {
                EXPECT(w.src == lh::SRC_STATE && w.index >= 0 && w.index < (int64_t)state.size(), "state index %lld of %zu (g %lld R %lld F %lld W %d)",
                       (long long)w.index, state.size(), (long long)g, (long long)R, (long long)F, W);
                if (w.src == lh::SRC_STATE && w.index >= 0 && w.index < (int64_t)state.size()) EXPECT(state[(size_t)w.index] == g, "state sample");
            }
        };
        for (int t = 0; t < nt && emit > 0; ++t) {
            const int64_t t0 = F + (int64_t)t * lh::TILE, t1 = t0 + lh::TILE < Fn ? t0 + lh::TILE : Fn;
            const int64_t lo = t0 - lh::back(W), hi = t1 - 1 + lh::ahead(W);  // what y[t0 .. t1 - 1] depends on
            EXPECT(last || hi <= Rn - 1, "a tile before last reads past what has arrived: hi %lld Rn %lld", (long long)hi, (long long)Rn);
            if (full) {
                for (int64_t g = lo; g <= hi + 4; ++g) look(g);
            } else {
                const int64_t pts[] = {lo, lo + 1, -1, 0, R - 1, R, Rn - 1, Rn, hi, hi + 4, lh::state_base(W, F)};
                for (int64_t g : pts)
                    if (g >= lo && g <= hi + 4) look(g);
            }
        }
        // the next state: x[state_base(Fn) .. Rn), through the same lookup
        std::vector<int64_t> next;
        if (!last) {
            const int64_t Bn = lh::state_base(W, Fn);
            EXPECT(Rn - Bn <= lh::state_floats(W), "the state holds %lld of %d floats", (long long)(Rn - Bn), lh::state_floats(W));
            EXPECT(Bn >= lh::state_base(W, F), "the state never moves back");
            for (int64_t g = Bn; g < Rn; ++g) {
                const lh::Where w = lh::where_is(W, R, F, count, g);
                int64_t v = -1;
                if (w.src == lh::SRC_CHUNK && w.index >= 0 && w.index < count) v = chunk[(size_t)w.index];
                if (w.src == lh::SRC_STATE && w.index >= 0 && w.index < (int64_t)state.size()) v = state[(size_t)w.index];
                EXPECT(v == g, "the next state's sample %lld", (long long)g);
                next.push_back(v);
            }
        }
        state.swap(next);
        R = Rn;
        F = Fn;
    }
};

int main() {
    long pushes = 0;
    for (int W : {1, 80, 960}) {
        EXPECT(lh::back(W) == 2 * W + 27 && lh::ahead(W) == 2 * W + 24 && lh::state_floats(W) >= 4 * W + 66 && lh::state_floats(W) % 4 == 0, "W %d", W);
        const int firsts[] = {0, 1, 2 * W + 24, 2 * W + 25, 2 * W + 40, 4 * W + 100, lh::TILE + 3};
        for (int count = 0; count <= 3 * lh::TILE; ++count)
            for (int last = 0; last < 2; ++last) {
                const int first = firsts[count % 7];
                Model m{W};
                m.push(first, false, false);
                m.push(count, last != 0, count % 97 == 0 || count < 64);
                if (!last) m.push(count % 5 == 0 ? 0 : 33, true, false);  // and the row's end: a flush, or a short tail
                pushes += 3 - last;
            }
        const lh::Layout l = lh::layout(W, 3, 8192);
        EXPECT(l.row_floats % 4 == 0 && l.row_floats >= 2 * l.state_floats + l.slot_floats && l.bytes == 3 * l.row_floats * 4, "layout");
        EXPECT(l.slot_floats == 2 * (size_t)((8192 + 2 * W + 39 + lh::TILE - 1) / lh::TILE), "slots");
    }
    printf("%ld pushes checked, %ld wrong\n", pushes, failures);
    return failures ? 1 : 0;
}
