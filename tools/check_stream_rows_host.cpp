// Host-only check of the streamed sessions' shared bookkeeping (viettts_amd/csrc/stream_rows_host.h) against a brute-force model of the
// cursors, under the address and undefined-behaviour sanitizers.  It links nothing of the HIP runtime and needs no GPU:
//
//   clang++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tools/check_stream_rows_host.cpp -o /tmp/check_stream_rows_host \
//       && /tmp/check_stream_rows_host
//
// Random pushes (rows out of range, rows named twice, closed rows, zero counts, counts past max_chunk or c_stride, rows at the length
// ceiling, a stage's own per-row refusal) go to Cursors::check_push and to a model that walks the same rows with its own copy of the rules
// and its own texts.  Every answer must match in code and text; a refused push must leave R, F, closed and parity as they were; an
// accepted one is advanced on both sides and compared again.  Both ceilings are driven (2^31 - 1 - 4096 with the limiter's wording,
// 2^31 - 1 with the resampler's), and the wrap of the push counter with marks left over from before it.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../viettts_amd/csrc/stream_rows_host.h"

namespace sr = vtts_stream_rows;

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

struct Model {
    int rows, max_chunk;
    std::vector<int64_t> R, F;
    std::vector<int> closed, parity;
};

struct Push {
    std::vector<int32_t> rows, counts, last, emitted;
    int64_t c_stride;
};

// The stage's own refusal in this check: a row may not take exactly 7 samples onto an odd received count.
static bool hook_refuses(int64_t R, int64_t cnt) { return (R & 1) && cnt == 7; }

// The first refusal of a push, by walking it: code, and the text in `why`
static int model_check(const Model& m, const Push& p, int margin, bool hooked, std::string& why) {
    char buf[256];
    buf[0] = 0;
    int code = 0;
    for (size_t i = 0; i < p.rows.size() && !code; ++i) {
        const int r = p.rows[i];
        const long long cnt = p.counts[i];
        bool twice = false;
        for (size_t j = 0; j < i; ++j) twice |= p.rows[j] == r;
        if (r < 0 || r >= m.rows)
            code = -1, snprintf(buf, sizeof buf, "push: rows[%d] = %d is outside 0 .. %d", (int)i, r, m.rows - 1);
        else if (twice)
            code = -1, snprintf(buf, sizeof buf, "push: row %d is named twice", r);
        else if (m.closed[r])
            code = -2, snprintf(buf, sizeof buf, "push: row %d ended with its last push; reset() it first", r);
        else if (cnt < 0 || cnt > m.max_chunk)
            code = -1, snprintf(buf, sizeof buf, "push: counts[%d] = %lld is outside 0 .. max_chunk = %d", (int)i, cnt, m.max_chunk);
        else if (p.c_stride && cnt > p.c_stride)
            code = -1, snprintf(buf, sizeof buf, "push: counts[%d] = %lld is above c_stride = %lld", (int)i, cnt, (long long)p.c_stride);
        else if (m.R[r] + cnt > 2147483647LL - margin)
            code = -6, margin ? snprintf(buf, sizeof buf, "push: row %d would pass 2^31 - 1 - %d samples", r, margin)
                              : snprintf(buf, sizeof buf, "push: row %d would pass 2^31 - 1 samples", r);
        else if (hooked && hook_refuses(m.R[r], cnt))
            code = -2, snprintf(buf, sizeof buf, "hook: row %d at %lld", r, (long long)m.R[r]);
    }
    why = buf;
    return code;
}

static void same_cursors(const sr::Cursors& c, const Model& m, const char* when) {
    for (int r = 0; r < m.rows; ++r)
        EXPECT(c.R[r] == m.R[r] && c.F[r] == m.F[r] && c.closed[r] == m.closed[r] && c.parity[r] == m.parity[r],
               "%s: row %d is R %lld F %lld closed %d parity %d, the model R %lld F %lld closed %d parity %d", when, r, (long long)c.R[r], (long long)c.F[r],
               (int)c.closed[r], (int)c.parity[r], (long long)m.R[r], (long long)m.F[r], m.closed[r], m.parity[r]);
}

static long session(std::mt19937& rng, int rows, int max_chunk, int margin, bool hooked, unsigned pushes_at_start, int n_pushes) {
    sr::Cursors c;
    EXPECT(c.init(rows, max_chunk), "init(%d, %d)", rows, max_chunk);
    EXPECT(c.rows == rows && c.max_chunk == max_chunk && c.has(0) && c.has(rows - 1) && !c.has(-1) && !c.has(rows), "init / has");
    c.pushes = pushes_at_start;  // near the wrap, with the marks 1, 2, 3 of pushes long past: they must not read as the marks of the pushes after it
    if (pushes_at_start)
        for (int r = 0; r < rows; ++r) c.seen[(size_t)r] = 1u + (unsigned)r % 3u;
    Model m{rows, max_chunk, std::vector<int64_t>(rows, 0), std::vector<int64_t>(rows, 0), std::vector<int>(rows, 0), std::vector<int>(rows, 0)};
    const int64_t ceiling = 2147483647LL - margin;
    long refused = 0;
    for (int it = 0; it < n_pushes; ++it) {
        if (rng() % 3 == 0) {  // a row starts over; now and then just below its ceiling, as a long session would leave it
            const int r = (int)(rng() % (unsigned)rows);
            c.reset(r);
            m.R[r] = m.F[r] = 0, m.closed[r] = 0;
            if (rng() % 5 == 0) c.R[r] = m.R[r] = ceiling - (int64_t)(rng() % (unsigned)(2 * max_chunk)), c.F[r] = m.F[r] = m.R[r] / 2;
        }
        Push p;
        const int n = 1 + (int)(rng() % (unsigned)rows);
        p.c_stride = rng() % 3 == 0 ? 1 + (int64_t)(rng() % (unsigned)max_chunk) : 0;
        std::vector<int> order((size_t)rows);
        for (int r = 0; r < rows; ++r) order[(size_t)r] = r;
        std::shuffle(order.begin(), order.end(), rng);
        for (int i = 0; i < n; ++i) {
            int r = order[(size_t)i];
            if (i > 0 && rng() % 25 == 0) r = p.rows[rng() % (unsigned)i];  // named twice
            if (rng() % 40 == 0) r = rng() % 2 ? -1 - (int)(rng() % 3) : rows + (int)(rng() % 3);
            int cnt = 0;
            switch (rng() % 6) {
                case 0: cnt = 0; break;
                case 1: cnt = 7; break;
                case 2: cnt = max_chunk; break;
                case 3: cnt = rng() % 2 ? -1 : max_chunk + 1; break;
                default: cnt = (int)(rng() % (unsigned)(max_chunk + 1));
            }
            if (rng() % 4) cnt = p.c_stride && cnt > p.c_stride ? (int)p.c_stride : cnt < 0 || cnt > max_chunk ? 1 : cnt;  // mostly acceptable
            p.rows.push_back(r);
            p.counts.push_back(cnt);
            p.last.push_back(rng() % 12 == 0);
            p.emitted.push_back(cnt > 0 ? (int32_t)(rng() % (unsigned)(cnt + 1)) : 0);
        }
        std::string want;
        const int code = model_check(m, p, margin, hooked, want);
        char why[160];
        memset(why, 'x', sizeof why);
        const unsigned before = c.pushes;
        const int got = hooked ? c.check_push(n, p.rows.data(), p.counts.data(), p.c_stride, margin,
                                              [&](int i, int r, int64_t cnt, char (&w)[160]) {
                                                  EXPECT(r == p.rows[(size_t)i] && cnt == p.counts[(size_t)i], "the hook's arguments at %d", i);
                                                  if (!hook_refuses(c.R[r], cnt)) return 0;
                                                  snprintf(w, sizeof w, "hook: row %d at %lld", r, (long long)c.R[r]);
                                                  return -2;
                                              },
                                              why)
                           : c.check_push(n, p.rows.data(), p.counts.data(), p.c_stride, margin, why);
        EXPECT(got == code && want == why, "push %d: got %d \"%s\", the model %d \"%s\"", it, got, why, code, want.c_str());
        EXPECT(c.pushes != 0 && (before == 0xffffffffu ? c.pushes == 1 : c.pushes == before + 1), "the counter went %u -> %u", before, c.pushes);
        same_cursors(c, m, "after check_push");  // accepted or refused, nothing has moved yet
        if (code) {
            ++refused;
            continue;
        }
        // the launches: a few rows at a time, as the kernels' row tables split a push
        for (int r0 = 0; r0 < n; r0 += 3) {
            const int nr = n - r0 < 3 ? n - r0 : 3;
            bool any_last = false;
            for (int i = 0; i < nr; ++i) any_last |= p.last[(size_t)(r0 + i)] != 0;
            c.advance(nr, p.rows.data() + r0, p.counts.data() + r0, any_last || rng() % 2 ? p.last.data() + r0 : nullptr, p.emitted.data() + r0);  // NULL = no row ends
        }
        for (int i = 0; i < n; ++i) {
            const int r = p.rows[(size_t)i];
            m.R[r] += p.counts[(size_t)i];
            m.F[r] += p.emitted[(size_t)i];
            if (p.last[(size_t)i])
                m.closed[r] = 1;
            else
                m.parity[r] ^= 1;
        }
        same_cursors(c, m, "after advance");
    }
    return refused;
}

int main() {
    std::mt19937 rng(4321);
    long refused = 0, sessions = 0;
    for (int rep = 0; rep < 40; ++rep) {
        const int rows = 1 + (int)(rng() % 9), max_chunk = rep % 2 ? 8 + (int)(rng() % 5000) : 1 << 20;
        for (int margin : {4096, 0})
            for (unsigned start : {0u, 0xfffffff0u}) {
                refused += session(rng, rows, max_chunk, margin, margin == 0, start, 120);
                ++sessions;
            }
    }
    if (failures) {
        printf("check_stream_rows_host: %ld FAILURES\n", failures);
        return 1;
    }
    printf("check_stream_rows_host: %ld sessions, %ld refused pushes, all checks passed\n", sessions, refused);
    return 0;
}
