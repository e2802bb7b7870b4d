// Host-only check of the batched stages' shared launch loop (viettts_amd/csrc/launch_rows.h) against a brute-force model, under the address
// and undefined-behaviour sanitizers.  It links nothing of the HIP runtime and needs no GPU:
//
//   clang++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tools/check_launch_rows_host.cpp -o /tmp/check_launch_rows_host \
//       && /tmp/check_launch_rows_host
//
// Both loop forms, at R = 128 and 256, for every N in 1 .. 2R + 2 and 3R, with lengths NULL and given (zeros among them, the last row of a
// launch and the first of the next included), strided and packed, with a row's own count and a caller's: every row must be handed over
// once and in order with its length and its first output element (packed: the sum of the counts of all rows of the call before it, by the
// model's own walk over the call), r0 and nr must be right, the slots past a launch's last row must hold length 0 (and an offset that
// keeps counting), and a non-zero return must end the loop at that launch and come back.  A packed sum past 2^31 must stay exact.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../viettts_amd/csrc/launch_rows.h"

namespace vr = vtts_rows;

static long failures = 0, launches = 0;
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

// a caller's count rule, as audio.hip's out_samples at 3 : 2 (0 for an empty row)
static long long resampled(int len) { return ((long long)len * 3 + 1) / 2; }

// the model: row i's length, and the first output element of every row (and, at [N], of a row behind the last) by one walk over the call
static int model_len(const int32_t* lengths, int64_t full, int i) { return lengths ? lengths[i] : (int)full; }
static std::vector<long long> model_offsets(int N, const int32_t* lengths, int64_t full, int64_t O_stride, bool own_rule) {
    std::vector<long long> off((size_t)N + 1, 0);
    for (int i = 1; i <= N; ++i) {
        const int before = model_len(lengths, full, i - 1);
        off[(size_t)i] = O_stride ? (long long)i * O_stride : off[(size_t)i - 1] + (own_rule ? resampled(before) : (long long)before);
    }
    return off;
}

// one call through both forms; stop_at >= 0: the launch whose fn refuses with 7 + stop_at
template <int R>
static void one_call(int N, const int32_t* lengths, int64_t full, int64_t O_stride, bool own_rule, int stop_at) {
    const int n_launches = (N + R - 1) / R, want_calls = stop_at >= 0 && stop_at < n_launches ? stop_at + 1 : n_launches;
    const int want_rc = stop_at >= 0 && stop_at < n_launches ? 7 + stop_at : VTTS_OK;
    int calls = 0, next = 0;
    int rc = vr::for_each_launch<R>(N, lengths, full, [&](int r0, int nr, const vr::Lens<R>& rows) -> int {
        EXPECT(r0 == calls * R && r0 == next && nr == (N - r0 < R ? N - r0 : R) && nr >= 1, "N %d: launch %d has r0 %d, nr %d", N, calls, r0, nr);
        for (int b = 0; b < R; ++b)
            EXPECT(rows.len[b] == (b < nr ? model_len(lengths, full, r0 + b) : 0), "N %d r0 %d: len[%d] = %d", N, r0, b, rows.len[b]);
        next += nr;
        ++launches;
        return calls++ == stop_at ? 7 + stop_at : 0;
    });
    EXPECT(rc == want_rc && calls == want_calls && (stop_at >= 0 || next == N), "N %d: rc %d after %d launches and %d rows", N, rc, calls, next);

    calls = next = 0;
    const std::vector<long long> off = model_offsets(N, lengths, full, O_stride, own_rule);
    auto fn = [&](int r0, int nr, const vr::OffLens<R>& rows) -> int {
        EXPECT(r0 == calls * R && r0 == next && nr == (N - r0 < R ? N - r0 : R) && nr >= 1, "N %d: launch %d has r0 %d, nr %d", N, calls, r0, nr);
        for (int b = 0; b < R; ++b) {
            EXPECT(rows.len[b] == (b < nr ? model_len(lengths, full, r0 + b) : 0), "N %d r0 %d: len[%d] = %d", N, r0, b, rows.len[b]);
            const long long want = b < nr ? off[(size_t)(r0 + b)] : O_stride ? (long long)(r0 + b) * O_stride : off[(size_t)N];
            EXPECT(rows.off[b] == want, "N %d r0 %d O_stride %lld: off[%d] = %lld, the model %lld", N, r0, (long long)O_stride, b, rows.off[b], want);
        }
        next += nr;
        ++launches;
        return calls++ == stop_at ? 7 + stop_at : 0;
    };
    rc = own_rule ? vr::for_each_launch_off<R>(N, lengths, full, O_stride, resampled, fn) : vr::for_each_launch_off<R>(N, lengths, full, O_stride, fn);
    EXPECT(rc == want_rc && calls == want_calls && (stop_at >= 0 || next == N), "N %d: rc %d after %d launches and %d rows (offsets)", N, rc, calls, next);
}

template <int R>
static void all_calls() {
    std::vector<int> sizes;
    for (int N = 1; N <= 2 * R + 2; ++N) sizes.push_back(N);
    sizes.push_back(3 * R);
    for (int N : sizes) {
        // lengths of a few hundred samples; zeros at every seventh row and on both sides of each split
        std::vector<int32_t> lens((size_t)N);
        for (int i = 0; i < N; ++i) lens[(size_t)i] = i % 7 == 3 || i % R == R - 1 || i % R == 0 ? 0 : 385 + (i * 37) % 613;
        for (const int32_t* lengths : {(const int32_t*)nullptr, (const int32_t*)lens.data()})
            for (int64_t O_stride : {(int64_t)0, (int64_t)1024})
                for (bool own_rule : {false, true}) one_call<R>(N, lengths, 1000, O_stride, own_rule, -1);
        for (int stop_at : {0, 1, 2}) one_call<R>(N, lens.data(), 1000, 0, false, stop_at);
    }
    // a packed sum past 2^31: full-length rows and rows just below, on both sides of a split
    {
        const int N = R + 3;
        std::vector<int32_t> lens((size_t)N, 0x7fffffff);
        for (int i = 0; i < N; i += 3) lens[(size_t)i] = 0x7fffffff - i;
        one_call<R>(N, lens.data(), 0x7fffffff, 0, false, -1);
        one_call<R>(N, lens.data(), 0x7fffffff, 0, true, -1);
        one_call<R>(N, nullptr, 0x7fffffff, 0, false, -1);
        one_call<R>(5, nullptr, 0x7fffffff, 0x7fffffff, false, -1);
        long long last = -1;
        vr::for_each_launch_off<R>(N, nullptr, 0x7fffffff, 0, [&](int r0, int nr, const vr::OffLens<R>& rows) -> int {
            (void)r0;
            last = rows.off[nr - 1];
            return 0;
        });
        EXPECT(last == (long long)(N - 1) * 0x7fffffffLL && last > (1LL << 31), "the last row of %d starts at %lld", N, last);
    }
}

int main() {
    static_assert(sizeof(vr::Lens<128>) == 128 * 4 && sizeof(vr::OffLens<128>) == 128 * 12, "the tables are the kernels' arguments: no padding");
    static_assert(offsetof(vr::OffLens<128>, off) == 0 && offsetof(vr::OffLens<128>, len) == 128 * 8, "off before len");
    all_calls<128>();
    all_calls<256>();
    if (failures) {
        printf("check_launch_rows_host: %ld FAILURES\n", failures);
        return 1;
    }
    printf("check_launch_rows_host: %ld launches, all checks passed\n", launches);
    return 0;
}
