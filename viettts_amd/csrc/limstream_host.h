// The index arithmetic of the streamed limiter (include/vtts_limstream.h), in plain C++ without HIP types: the emit rule, where a sample of a
// workgroup's span lives (the row's state, the new chunk, or nowhere), tile counts and the state's layout.  limiter_stream.hip uses it on
// the host and in its kernels; tools/check_limstream_host.cpp sweeps it against a brute-force restatement, stand-alone and under the
// sanitizers.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/vtts_limiter.h"

#if defined(__HIPCC__)
#define VTTS_LS_HD __host__ __device__ inline
#else
#define VTTS_LS_HD inline
#endif

namespace vtts_limstream_host {

constexpr int TILE = VTTS_LIMITER_TILE;
constexpr int RUN = VTTS_LIMITER_RUN;
constexpr int LEAD = 27;   // x[n - LEAD] meets a phase's first tap
constexpr int TRAIL = 24;  // x[n + TRAIL] its last

// y[n] needs x[n - back(W) .. n + ahead(W)]
VTTS_LS_HD int back(int W) { return 2 * W + LEAD; }
VTTS_LS_HD int ahead(int W) { return 2 * W + TRAIL; }

// The emitted count after a push of `count` samples onto `received`: whole runs of 16 whose look-ahead has arrived, everything on `last`.
VTTS_LS_HD int64_t emit_rule(int W, int64_t received, int64_t emitted, int64_t count, int last) {
    const int64_t r = received + count;
    if (last) return r;
    const int64_t d = r - ahead(W);
    const int64_t f = d <= 0 ? 0 : d / RUN * RUN;
    return f > emitted ? f : emitted;
}

// An open row's emitted count is a function of its received count alone (the rule is monotone): what the kernels derive F from.
VTTS_LS_HD int64_t emitted_of(int W, int64_t received) { return emit_rule(W, received, 0, 0, 0); }

// The state after a push holds x[state_base(W, F') .. R'), at most state_floats(W) of them, fp32.
VTTS_LS_HD int64_t state_base(int W, int64_t emitted) { return emitted > back(W) ? emitted - back(W) : 0; }
VTTS_LS_HD int state_floats(int W) { return (back(W) + ahead(W) + RUN - 1 + 3) / 4 * 4; }

// Workgroups a row takes in a push that emits `emit` samples: one per tile, and one for a push that only moves the state.
VTTS_LS_HD int tiles_of(int64_t emit) { return emit <= 0 ? 1 : (int)((emit + TILE - 1) / TILE); }
// ... at most, in a session of this max_chunk (a push emits fewer than count + ahead(W) + RUN samples)
VTTS_LS_HD int max_tiles(int W, int max_chunk) { return tiles_of((int64_t)max_chunk + ahead(W) + RUN - 1); }

// Where sample g of a row lives during a push onto `received` samples of which `emitted` had left (the state read is the one the previous
// push wrote): nowhere (zero extension), state[index] or chunk[index].
enum Source : int { SRC_ZERO = 0, SRC_STATE = 1, SRC_CHUNK = 2 };
struct Where {
    int src;
    int64_t index;
};
VTTS_LS_HD Where where_is(int W, int64_t received, int64_t emitted, int64_t count, int64_t g) {
    Where w = {SRC_ZERO, 0};
    if (g < 0 || g >= received + count) return w;
    if (g >= received) {
        w.src = SRC_CHUNK;
        w.index = g - received;
    } else {
        w.src = SRC_STATE;
        w.index = g - state_base(W, emitted);
    }
    return w;
}

// Device memory of a session: per row two state buffers, then two result slots (max p, min a) per tile of the largest push.
struct Layout {
    size_t state_floats = 0;  // of one buffer
    size_t slot_floats = 0;   // 2 * max_tiles
    size_t row_floats = 0;    // 2 * state_floats + slot_floats
    size_t bytes = 0;
};
inline Layout layout(int W, int rows, int max_chunk) {
    Layout l;
    l.state_floats = (size_t)state_floats(W);
    l.slot_floats = 2 * (size_t)max_tiles(W, max_chunk);
    l.row_floats = (2 * l.state_floats + l.slot_floats + 3) / 4 * 4;
    l.bytes = (size_t)rows * l.row_floats * sizeof(float);
    return l;
}

}  // namespace vtts_limstream_host
