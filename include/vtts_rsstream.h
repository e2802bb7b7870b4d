/*
 * vtts_rsstream.h — C ABI of the streamed resampler: vtts_audio.h's sample-rate conversion fed chunk by chunk, for audio that leaves at
 * another rate while its sentence is still being decoded.  A session holds `rows` independent row slots of one vtts_audio_cfg.  The
 * reference has no such stage.
 *
 * The contract is vtts_audio.h's, and the guarantee is about bits: for every row, the concatenation of what its pushes emit equals
 * vtts_audio_forward() on the whole row with the same input and output dtype, bit for bit, as fp32 and as PCM16.  That holds whatever the
 * chunking, the slot, the other rows of a push, their cursors, and strided or packed input.  It can hold because, by vtts_audio.h, y[m] is
 * one fp32 fmaf chain over x[q - (kp4 - 1) .. q], q = q(m) = (m M + half) div L (kp4 = the table's taps per phase, ceil((2 half + 1) / L)
 * rounded up to 4), and depends on nothing else of the row, on no tile and on no row length.
 *
 * Per slot the HOST keeps three numbers, all deterministic (the device is never asked for them): the received count R, the emitted count
 * F and whether the row is closed.
 *
 *   emit rule     a push of `count` samples gives R' = R + count and
 *                     not last:  F' = max(F, max(0, ceil((R' L - half) / M))): the outputs whose newest input q(m) <= R' - 1 has arrived
 *                     last:      F' = ceil(R' L / M) = vtts_audio_out_samples(R')          (the row is then closed until reset())
 *                     in_rate == out_rate:  F' = R', no filter and no state
 *                 and emits y[F .. F' - 1].  The delay is ceil(half / L) input samples: 24 (1.5 ms at 16 kHz) when upsampling, 24 M / L when
 *                 downsampling.
 *   edges         zero extension happens at the row's absolute sample 0, never at a chunk's start, and at the row's end only on the
 *                 `last` push.  Before `last`, no sample at index >= R' enters an output.
 *   state         fp32, per row x[max(0, q(F') - (kp4 - 1)) .. R') (PCM16 input is kept times 2^-15, exact).  That is at most kp4 - 1
 *                 samples: the rule gives F' M + half >= R' L, so q(F') >= R'; and where it floors F' at 0, R' L < half gives
 *                 R' <= half div L = q(0).  push() asserts the bound.  The padding taps' samples (up to 4, vtts_audio.h) are inside
 *                 it, so an Inf or NaN reaches exactly the outputs it reaches un-streamed.  The state is double-buffered: a push reads one
 *                 buffer and writes the other, because several workgroups of a row read the old tail while one of them writes the new
 *                 one; the host flips the parity of the rows of a push.
 *   device memory state_bytes() bytes, owned by the caller, 16-byte aligned; its contents need not be initialised: reset() is host
 *                 bookkeeping only, and no history is read before a row's sample 0.
 *   tap table     vtts_audio.h's packed blob.  The session computes no second table: it binds the blob a vtts_audio handle of the same
 *                 configuration packed (vtts_audio_pack), and push() before bind_packed() is VTTS_ERR_STATE (not when in_rate == out_rate).
 *
 * Launches: one kernel per push does everything for every row of the push (one workgroup per VTTS_AUDIO_OUT_PER_BLOCK emitted samples of
 * a row, tiles anchored at the row's F; the first workgroup of a row also writes the row's next history): one launch for up to 128 rows,
 * whatever the counts; more rows mean more launches of the same kernel.  Nothing synchronises with the host.
 *
 * Out of scope: an input-side streamed resampler for the analysis direction, a streamed loudness normaliser, and everything
 * vtts_audio.h leaves out.
 *
 * Same conventions as vtts_audio.h: plain pointers and sizes, 0 or a negative vtts_status (vtts_last_error() of vtts_hifigan.h), device
 * memory owned by the caller, asynchronous on the given stream.  The handle owns nothing on the device.
 */
#ifndef VTTS_RSSTREAM_H
#define VTTS_RSSTREAM_H

#include <stddef.h>
#include <stdint.h>

#include "vtts_audio.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vtts_rsstream vtts_rsstream; /* opaque */

#define VTTS_RSSTREAM_MAX_CHUNK (1 << 20)
/* Rows whose cursors one launch carries. */
#define VTTS_RSSTREAM_ROWS_PER_LAUNCH 128

/* Touches no HIP call.  1 <= rows <= 2^24, 1 <= max_chunk <= VTTS_RSSTREAM_MAX_CHUNK, and vtts_audio_create()'s ranges, else
 * VTTS_ERR_INVALID.  Every slot starts open with R = F = 0. */
int vtts_rsstream_create(const vtts_audio_cfg* cfg, int device, int rows, int32_t max_chunk, vtts_rsstream** out);
void vtts_rsstream_destroy(vtts_rsstream* h);

/* L, M and half of vtts_audio.h (any of the three pointers may be NULL). */
int vtts_rsstream_ratio(const vtts_rsstream* h, int32_t* L, int32_t* M, int32_t* half);

/* Bytes of device state push() needs: per row two buffers of (kp4 - 1 rounded up to 4) floats; 0 when in_rate == out_rate. */
int vtts_rsstream_state_bytes(const vtts_rsstream* h, size_t* bytes);

/* The tap table: vtts_audio_packed_bytes() of the same configuration, and the blob such a handle packed. */
int vtts_rsstream_packed_bytes(const vtts_rsstream* h, size_t* bytes);
int vtts_rsstream_bind_packed(vtts_rsstream* h, void* dev_blob, size_t blob_bytes);

/* Host bookkeeping only: R = F = 0, open. */
int vtts_rsstream_reset(vtts_rsstream* h, int row);

/* A slot's bookkeeping as the host holds it (any of the three pointers may be NULL). */
int vtts_rsstream_cursor(const vtts_rsstream* h, int row, int64_t* received, int64_t* emitted, int* closed);

/* The emit rule alone: *new_emitted = F' for a push of `count` samples (0 <= count) onto `received` of which `emitted` have left. */
int vtts_rsstream_emit(const vtts_rsstream* h, int64_t received, int64_t emitted, int32_t count, int last, int64_t* new_emitted);

/*
 *   state_dev          state_bytes() bytes, 16-byte aligned; the same pointer for every push of the session (may be NULL when
 *                      state_bytes() is 0)
 *   chunk_dev, dtype   samples of `dtype` (VTTS_AUDIO_F32 | VTTS_AUDIO_PCM16): [n, c_stride], or PACKED with c_stride == 0 (row i of the
 *                      call starts at the sum of the counts before it)
 *   n, rows_host       the call's rows: n slots, 1 <= n <= rows, each named once, none closed.  HOST memory, as the three arrays below.
 *   counts_host        [n] new samples per row, 0 <= counts[i] <= max_chunk (and <= c_stride when strided).  A zero count is legal, also
 *                      with last: a flush.
 *   last_host          [n] non-zero = the row ends with this push; NULL = none does
 *   out_dev, out_dtype the emitted samples of every row back to back in the call's row order (always packed); the caller sizes it for
 *                      sum((counts[i] L + half) div M + 2) at most, or calls emit() first
 *   out_counts_host    [n] F' - F per row, filled before the call returns
 * A refused call (VTTS_ERR_INVALID: a bad argument, a row out of range or named twice, a count out of range; VTTS_ERR_STATE: a closed row,
 * or no tap table bound; VTTS_ERR_SHAPE: a row past 2^31 - 1 input samples) enqueues nothing and changes no slot's bookkeeping.
 * chunk_dev, out_dev and state_dev must not overlap.
 */
int vtts_rsstream_push(vtts_rsstream* h, void* state_dev, const void* chunk_dev, int dtype, int n, const int32_t* rows_host, int64_t c_stride,
                       const int32_t* counts_host, const int32_t* last_host, void* out_dev, int out_dtype, int32_t* out_counts_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTTS_RSSTREAM_H */
