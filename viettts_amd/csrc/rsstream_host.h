// The index arithmetic of the streamed resampler (include/vtts_rsstream.h), in plain C++ without HIP types: the emit rule, the newest input
// of an output, the history a row keeps between pushes, where a sample of a workgroup's span lives (the row's history, the new chunk, or
// nowhere), tile counts and the state's layout.  resample_stream.hip uses it on the host and in its kernel; tools/check_rsstream_host.cpp
// sweeps it against a brute-force restatement, stand-alone and under the sanitizers.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/vtts_audio.h"

#if defined(__HIPCC__)
#define VTTS_RS_HD __host__ __device__ inline
#else
#define VTTS_RS_HD inline
#endif

namespace vtts_rsstream_host {

constexpr int OPB = VTTS_AUDIO_OUT_PER_BLOCK;

// vtts_audio.h's L, M, half and the table's taps per phase (a multiple of 4); identity = in_rate == out_rate: no filter, no state
struct Ratio {
    int L, M, half, kp4, identity;
};

// ceil(a / b) for b > 0, a of either sign
VTTS_RS_HD int64_t ceil_div(int64_t a, int64_t b) { return a >= 0 ? (a + b - 1) / b : -((-a) / b); }

// q(m): the newest input sample output m reads; its chain runs over x[q - (kp4 - 1) .. q]
VTTS_RS_HD int64_t newest_of(const Ratio& r, int64_t m) { return (m * r.M + r.half) / r.L; }

// The emitted count after a push of `count` samples onto `received`: the outputs whose newest input has arrived, every output of the
// row on `last`.
VTTS_RS_HD int64_t emit_rule(const Ratio& r, int64_t received, int64_t emitted, int64_t count, int last) {
    const int64_t n = received + count;
    if (r.identity) return n;
    if (last) return ceil_div(n * r.L, r.M);
    const int64_t f = ceil_div(n * r.L - r.half, r.M);  // the first m with q(m) >= n
    const int64_t g = f > 0 ? f : 0;
    return g > emitted ? g : emitted;
}

// An open row's emitted count is a function of its received count alone (the rule is monotone): what the kernel derives F from.
VTTS_RS_HD int64_t emitted_of(const Ratio& r, int64_t received) { return emit_rule(r, received, 0, 0, 0); }

// The history after a push holds x[hist_base(F') .. R').  q(F') >= R' (F' M + half >= R' L by the rule, and R' L < half where the rule
// floors F' at 0), so it is at most kp4 - 1 samples: hist_floats(), rounded up to whole 16-byte groups.
VTTS_RS_HD int64_t hist_base(const Ratio& r, int64_t emitted) {
    const int64_t b = newest_of(r, emitted) - (r.kp4 - 1);
    return b > 0 ? b : 0;
}
VTTS_RS_HD int hist_floats(const Ratio& r) { return r.identity ? 0 : (r.kp4 - 1 + 3) / 4 * 4; }

// Workgroups a row takes in a push that emits `emit` samples: one per tile, and one for a push that only moves the history.
VTTS_RS_HD int64_t tiles_of(int64_t emit) { return emit <= 0 ? 1 : (emit + OPB - 1) / OPB; }

// A push of `count` samples emits at most this many, whatever the cursors: F >= (R L - half) / M and F' < R' L / M + 1.
VTTS_RS_HD int64_t max_emit(const Ratio& r, int64_t count) { return r.identity ? count : (count * r.L + r.half) / r.M + 2; }

// A workgroup's staged span: the outputs m0 .. m0 + live - 1 (live >= 1) read x[first + sbase .. first + count - 1]; `first` is a
// multiple of 8 as in audio.hip, and count never passes audio_design.h's span_floats.
struct Span {
    int64_t first;  // absolute index of span[0]
    int64_t q0;     // q(m0)
    int p0;         // the phase of output m0
    int count;      // staged samples
    int sbase;      // span index of x[q0 - (kp4 - 1)]
};
VTTS_RS_HD Span span_of(const Ratio& r, int64_t m0, int live) {
    Span s;
    const int64_t t0 = m0 * r.M + r.half;
    s.q0 = t0 / r.L;
    s.p0 = (int)(t0 - s.q0 * r.L);
    s.first = (s.q0 - (r.kp4 - 1)) & ~(int64_t)7;  // floor to a multiple of 8, also below zero
    s.count = (int)(s.q0 + (s.p0 + (int64_t)(live - 1) * r.M) / r.L - s.first) + 1;
    s.sbase = (int)(s.q0 - s.first) - (r.kp4 - 1);
    return s;
}

// Where sample g of a row lives during a push of `count` samples onto `received`, the history (the one the previous push wrote) starting
// at hist_first = hist_base(F): nowhere (zero extension, or a sample no output of this push may read), hist[index] or chunk[index].
enum Source : int { SRC_ZERO = 0, SRC_HIST = 1, SRC_CHUNK = 2 };
struct Where {
    int src;
    int64_t index;
};
VTTS_RS_HD Where where_is(int64_t received, int64_t count, int64_t hist_first, int64_t g) {
    Where w = {SRC_ZERO, 0};
    if (g < 0 || g >= received + count) return w;
    if (g >= received) {
        w.src = SRC_CHUNK;
        w.index = g - received;
        return w;
    }
    const int64_t b = hist_first;
    if (g < b) return w;  // (below the history: only the span's rounding down to 8 reaches here, no chain does)
    w.src = SRC_HIST;
    w.index = g - b;
    return w;
}

// Device memory of a session: per row two history buffers.
struct Layout {
    size_t hist_floats = 0;  // of one buffer
    size_t row_floats = 0;   // 2 * hist_floats
    size_t bytes = 0;
};
inline Layout layout(const Ratio& r, int rows) {
    Layout l;
    l.hist_floats = (size_t)hist_floats(r);
    l.row_floats = 2 * l.hist_floats;
    l.bytes = (size_t)rows * l.row_floats * sizeof(float);
    return l;
}

}  // namespace vtts_rsstream_host
