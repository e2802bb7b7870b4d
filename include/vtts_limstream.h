/*
 * vtts_limstream.h — C ABI of the streamed true-peak limiter: vtts_limiter.h's look-ahead limiter fed chunk by chunk, for audio that leaves
 * while its sentence is still being decoded.  A session holds `rows` independent row slots of one vtts_limiter_cfg (rate, look-ahead -> W)
 * and one ceiling.  The reference has no such stage.
 *
 * The contract is vtts_limiter.h's, and the guarantee is about bits: for every row, the concatenation of what its pushes emit equals
 * vtts_limiter_apply() on the whole row with gains[b] = g, the same ceiling and the same input and output dtype, bit for bit, as fp32 and
 * as PCM16; and the row's three results after its `last` push equal apply()'s true_peak, min_gain and gains_used.  That holds whatever the
 * chunking, the slot, the other rows of a push, their cursors, and strided or packed input.  It can hold because, by vtts_limiter.h,
 * y[n] depends on x[n - 2 W - 27 .. n + 2 W + 24] and on nothing else of the row, and the fp64 window sums are anchored at multiples of
 * VTTS_LIMITER_RUN = 16 from the row's first sample, not at tiles or at the row's length.
 *
 * Per slot the HOST keeps four numbers, all deterministic (the device is never asked for them): the received count R, the emitted count F,
 * the pre-gain g (fp32) and whether the row is closed.
 *
 *   emit rule     a push of `count` samples gives R' = R + count and
 *                     not last:  F' = max(F, floor((R' - 2 W - 24) / 16) * 16), floored at 0
 *                     last:      F' = R'                                          (the row is then closed until reset())
 *                 and emits y[F .. F' - 1].  The delay is 2 W + 24 samples (184 at 16 kHz with the 5 ms look-ahead), plus up to 15.
 *   edges         edge replication (vtts_limiter.h: every index clamped to the row) happens at the row's absolute sample 0, never at a
 *                 window's start, and at the row's end only on the `last` push.  Before `last`, no value that depends on the zero
 *                 extension past R' is used: no p[n] with n + 24 >= R' enters an output or a result.
 *   state         fp32, per row x[max(0, F' - 2 W - 27) .. R'): at most 4 W + 66 samples (PCM16 input is kept times 2^-15, exact).  It is
 *                 double-buffered: a push reads one buffer and writes the other, because several workgroups of a row read the old tail
 *                 while one of them writes the new one; the host flips the parity of the rows of a push.
 *   results       [rows, 3] fp32, per slot: the running true_peak (max p[n] over the samples emitted so far), the running min_gain (min a[n]
 *                 over them; 1 before any) and g.  The first push of a row after reset() overwrites them.
 *   device memory state_bytes() bytes, owned by the caller, 16-byte aligned; its contents need not be initialised: reset() is host
 *                 bookkeeping only, and no history is read before a row's sample 0.
 *
 * Launches: one kernel per push does the whole chain for every row of the push (one workgroup per VTTS_LIMITER_TILE emitted samples of a
 * row), and one small kernel merges the tiles' maxima and minima into the results: two launches for up to 128 rows, whatever the counts;
 * more rows mean more launches of the same two kernels.  Nothing synchronises with the host.
 *
 * Out of scope: streamed loudness normalisation or any gain that depends on the utterance's own level, and everything vtts_limiter.h
 * leaves out.  A streamed resampler is vtts_rsstream.h's: it takes this session's fp32 output chunk by chunk.
 *
 * Same conventions as vtts_limiter.h: plain pointers and sizes, 0 or a negative vtts_status (vtts_last_error() of vtts_hifigan.h), device
 * memory owned by the caller, asynchronous on the given stream.  The handle owns nothing on the device.
 */
#ifndef VTTS_LIMSTREAM_H
#define VTTS_LIMSTREAM_H

#include <stddef.h>
#include <stdint.h>

#include "vtts_limiter.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vtts_limstream vtts_limstream; /* opaque */

#define VTTS_LIMSTREAM_MAX_CHUNK (1 << 20)
/* Rows whose cursors one launch carries. */
#define VTTS_LIMSTREAM_ROWS_PER_LAUNCH 128

/* Touches no HIP call.  1 <= rows <= 2^24, 1 <= max_chunk <= VTTS_LIMSTREAM_MAX_CHUNK, a finite ceiling, and vtts_limiter_create()'s ranges, else
 * VTTS_ERR_INVALID.  Every slot starts open with R = F = 0 and g = 1. */
int vtts_limstream_create(const vtts_limiter_cfg* cfg, int device, int rows, int32_t max_chunk, float ceiling_dbtp, vtts_limstream** out);
void vtts_limstream_destroy(vtts_limstream* h);

/* W in samples; the delay is 2 W + 24. */
int vtts_limstream_lookahead(const vtts_limstream* h, int32_t* W);

/* Bytes of device state push() needs: per row two buffers of (4 W + 66 rounded up to 4) floats and two floats per tile of the largest
 * push, ceil((max_chunk + 2 W + 39) / VTTS_LIMITER_TILE) tiles, the row's floats rounded up to 4. */
int vtts_limstream_state_bytes(const vtts_limstream* h, size_t* bytes);

/* Host bookkeeping only: R = F = 0, open, g = gain (finite). */
int vtts_limstream_reset(vtts_limstream* h, int row, float gain);

/* The emit rule alone: *new_emitted = F' for a push of `count` samples (0 <= count) onto `received` of which `emitted` have left. */
int vtts_limstream_emit(const vtts_limstream* h, int64_t received, int64_t emitted, int32_t count, int last, int64_t* new_emitted);

/*
 *   state_dev          state_bytes() bytes, 16-byte aligned; the same pointer for every push of the session
 *   chunk_dev, dtype   samples of `dtype` (VTTS_AUDIO_F32 | VTTS_AUDIO_PCM16): [n, c_stride], or PACKED with c_stride == 0 (row i of the
 *                      call starts at the sum of the counts before it)
 *   n, rows_host       the call's rows: n slots, 1 <= n <= rows, each named once, none closed.  HOST memory, as the three arrays below.
 *   counts_host        [n] new samples per row, 0 <= counts[i] <= max_chunk (and <= c_stride when strided).  A zero count is legal, also
 *                      with last: a flush.
 *   last_host          [n] non-zero = the row ends with this push; NULL = none does
 *   out_dev, out_dtype the emitted samples of every row back to back in the call's row order (always packed); the caller sizes it for
 *                      sum(counts[i] + 2 W + 39) at most, or calls emit() first
 *   out_counts_host    [n] F' - F per row, filled before the call returns
 *   results_dev        [rows, 3] fp32: true_peak, min_gain, g per SLOT
 * A refused call (VTTS_ERR_INVALID: a bad argument, a row out of range or named twice, a count out of range; VTTS_ERR_STATE: a closed row;
 * VTTS_ERR_SHAPE: a row past 2^31 - 1 - VTTS_LIMITER_TILE samples) enqueues nothing and changes no slot's bookkeeping.
 * chunk_dev, out_dev and state_dev must not overlap.
 */
int vtts_limstream_push(vtts_limstream* h, void* state_dev, const void* chunk_dev, int dtype, int n, const int32_t* rows_host, int64_t c_stride,
                        const int32_t* counts_host, const int32_t* last_host, void* out_dev, int out_dtype, int32_t* out_counts_host,
                        float* results_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTTS_LIMSTREAM_H */
