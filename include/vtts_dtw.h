/*
 * vtts_dtw.h — C ABI of batched dynamic time warping between two feature sequences of different lengths (log-mels: the
 * output layout of vtts_mel_forward and of the acoustic model).  The reference has no such stage; it is what carries the
 * model's own token boundaries onto a recording (alignment by synthesis -> the durations ground-truth-aligned mels need)
 * and what gives the DTW log-mel distance between a synthesised sentence and the recording of it.
 *
 * For pair n: query a[la, D] and reference b[lb, D], fp32, rows contiguous, 1 <= D <= VTTS_DTW_MAX_FEAT.
 *
 *   local cost   c(i, j) = ONE fp32 chain in ascending d:  s = 0;  s = s + fabsf(a[i, d] - b[j, d])
 *                (subtract, absolute value, add, each rounded to fp32; never reassociated or split)
 *   recurrence   D(0, 0) = c(0, 0);  otherwise D(i, j) = c(i, j) + min over the allowed predecessors (one fp32 add).
 *                Predecessors are tried in the order  diagonal (i-1, j-1),  up (i-1, j),  left (i, j-1);  a later one replaces
 *                an earlier one only if it is strictly smaller.  A predecessor outside the matrix or outside the band counts
 *                as +inf, so row 0 only has `left` and column 0 only has `up`.  The chosen move is kept as a 2-bit code per
 *                cell: 0 diagonal, 1 up, 2 left.
 *   band         band = r >= 0.  r = 0: every cell is allowed.  r >= 1: cell (i, j) is allowed iff
 *                    | i (lb - 1) - j (la - 1) |  <=  r max(la - 1, lb - 1)                (int64)
 *                Cells outside hold +inf and are never computed; whole tiles outside are skipped.  The corner (la-1, lb-1) is
 *                reachable for every r >= 1 (tests/test_dtw_cpu.py sweeps r = 1, 2; a larger r contains them).
 *   results      total = D(la-1, lb-1);  path_len = cells on the optimal path;  span[i] = {first j, last j} of the path in row i.
 *                The path is monotone, so span is the path: row i+1 starts at last[i] (up) or last[i] + 1 (diagonal).
 *   backtrace    follows the stored codes only, from the corner; at most la + lb - 1 cells, indices clamped into the matrix (on row 0
 *                it moves left, on column 0 up, whatever the code), so non-finite inputs give a meaningless path but never an
 *                out-of-range access.  Inputs are documented as finite.
 *
 * Every operation above is an IEEE fp32 operation in a fixed order: tests/_dtw_oracle.py restates it in numpy float32 and the
 * results are compared with ==.
 *
 * Same conventions as vtts_mel.h / vtts_audio.h (vtts_status and vtts_last_error() of vtts_hifigan.h): plain pointers and sizes, 0 or
 * a negative vtts_status, device memory owned by the caller, asynchronous on the given stream.  The handle owns nothing on the device.
 */
#ifndef VTTS_DTW_H
#define VTTS_DTW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vtts_dtw_cfg {
    int32_t n_feat;      /* D, 1 .. VTTS_DTW_MAX_FEAT */
    int32_t band;        /* r >= 0, 0 = no band */
    int32_t max_frames;  /* 1 .. VTTS_DTW_MAX_FRAMES: the longest la or lb forward() accepts */
} vtts_dtw_cfg;

typedef struct vtts_dtw vtts_dtw; /* opaque */

#define VTTS_DTW_MAX_FEAT 128
/* The wavefront kernel keeps one row of D (the previous strip's last row) in LDS: 4 bytes per column, 16 KB at 4096.  One pair at
 * 4096 x 4096 needs 76 MB of workspace (below), so a single pair of the longest kind still fits the Python owner's 1 GiB budget;
 * 4096 frames are 65 s of speech at the reference's hop. */
#define VTTS_DTW_MAX_FRAMES 4096

/* Rows one workgroup of the wavefront kernel advances together: thread l owns row i0 + l of the strip and is at column step - l. */
#define VTTS_DTW_STRIP 256
/* The cost kernel's tile: VTTS_DTW_TILE rows by VTTS_DTW_TILE anti-diagonal steps (below). */
#define VTTS_DTW_TILE 64
/* 2-bit move codes of consecutive columns of one row per 32-bit word. */
#define VTTS_DTW_CODES_PER_WORD 16
/* The backtrace's prefetched window of code words: VTTS_DTW_BT_ROWS rows up from the current cell by VTTS_DTW_BT_WORDS words left. */
#define VTTS_DTW_BT_ROWS 16
#define VTTS_DTW_BT_WORDS 4

/* Touches no HIP call: works on a host without a GPU.  VTTS_ERR_INVALID outside the ranges above. */
int vtts_dtw_create(const vtts_dtw_cfg* cfg, int device, vtts_dtw** out);
void vtts_dtw_destroy(vtts_dtw* h);

/*
 * Scratch bytes forward() needs for N pairs with row strides Ta_stride, Tb_stride (both 1 .. max_frames).  Per pair:
 *     strips     = ceil(Ta_stride / VTTS_DTW_STRIP)
 *     steps      = round_up(Tb_stride + VTTS_DTW_STRIP - 1, VTTS_DTW_TILE)
 *     cost       = strips * steps * VTTS_DTW_STRIP            fp32: c(i, j) at [strip i / STRIP][step j + i % STRIP][i % STRIP],
 *                                                             the order the wavefront reads it in (one contiguous kilobyte per step)
 *     codes      = Ta_stride * ceil(Tb_stride / VTTS_DTW_CODES_PER_WORD)      32-bit words, row-major
 *     pair_bytes = round_up(4 * (cost + codes), 256)
 * and bytes = N * pair_bytes (size_t: N * la * lb passes 2^31 long before one pair does; every per-pair offset is 64-bit).
 */
int vtts_dtw_workspace_bytes(const vtts_dtw* h, int N, int64_t Ta_stride, int64_t Tb_stride, size_t* bytes);

/*
 *   a_dev        [N, Ta_stride, D] fp32, device memory; pair n's query is its first la[n] rows, the rest is never read
 *   b_dev        [N, Tb_stride, D] fp32; first lb[n] rows
 *   la, lb       [N] HOST int32, 1 <= la[n] <= Ta_stride, 1 <= lb[n] <= Tb_stride, both <= max_frames (else VTTS_ERR_INVALID, before
 *                any launch); read before the call returns
 *   total_dev    [N] fp32       D(la-1, lb-1)
 *   path_len_dev [N] int32
 *   span_dev     [N, Ta_stride, 2] int32; rows la[n] .. Ta_stride - 1 are set to -1
 *   workspace    256-byte aligned, at least workspace_bytes(N, Ta_stride, Tb_stride) (else VTTS_ERR_NOMEM)
 * Every pair's results are bit for bit what the pair gives alone.
 */
int vtts_dtw_forward(vtts_dtw* h, const float* a_dev, const float* b_dev, int N, int64_t Ta_stride, int64_t Tb_stride, const int32_t* la,
                     const int32_t* lb, float* total_dev, int32_t* path_len_dev, int32_t* span_dev, void* workspace, size_t workspace_bytes,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTTS_DTW_H */
