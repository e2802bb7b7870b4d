/*
 * vtts_mcd.h — C ABI of mel-cepstral distortion between log-mels (the output layout of vtts_mel_forward and of the acoustic model): MCD in dB
 * of a time-aligned pair, and MCD-DTW of two sequences of different lengths.  The reference has no such stage.  This is the one local metric
 * of the DTW besides vtts_dtw.h's L1: the recurrence, the band, the codes and the backtrace are those of vtts_dtw.h, run by the same kernels.
 *
 *   input        natural-log mels x[t, m], fp32, [N, T, M] with rows contiguous, M = n_mels, 1 <= M <= VTTS_MCD_MAX_MELS.
 *   basis        rows k = 1 .. K of the orthonormal DCT-II (row 0, the energy term, is left out):
 *                    dct[k][m] = sqrt(2 / M) cos(pi k (2 m + 1) / (2 M)),        K = n_ceps, 1 <= K <= min(M - 1, VTTS_MCD_MAX_CEPS)
 *                computed on the host in double (pi k (2 m + 1) / (2 M) as written, left to right) and rounded once to fp32; basis() gives
 *                the table the kernels use, row k - 1 of it is dct[k].
 *   cepstrum     c[t, k] = ONE fp32 chain in ascending m:  s = 0;  s = s + dct[k][m] * x[t, m]
 *                (the multiply and the add each rounded to fp32; never contracted into an fma, reassociated or split)
 *   distance     d(i, j) = sqrt(s),  s = ONE fp32 chain in ascending k:  e = ca[i, k] - cb[j, k];  s = s + e * e
 *                (subtract, multiply, add each rounded, no fma; the square root correctly rounded)
 *   scale        alpha = 10 sqrt(2) / ln 10, applied by the caller in float64 (VTTS_MCD_ALPHA below; viettts_amd/mcd.py does it).
 *   aligned      of a row of L frames:  sum = the float64 sum of the fp32 values d(t, t), t < L, in this order: the frames are cut into
 *                blocks of VTTS_MCD_FRAMES_PER_BLOCK from the row's first frame; a block's values are added in ascending t starting from
 *                0.0; the blocks' sums are added in ascending order starting from 0.0.  The order depends on nothing but L, so a row gives
 *                the same bits alone, in a ragged batch and at any stride.  MCD = alpha sum / L.  L = 0 gives sum = 0.
 *   dtw          total, path_len and span of vtts_dtw.h's contract with its local cost c(i, j) replaced by d(i, j) over the cepstra
 *                (D = K): the same recurrence, tie rule (diagonal / up / left, a later one replaces only if strictly smaller), band
 *                predicate, 2-bit codes, backtrace and clamping.  MCD-DTW = alpha total / path_len.
 *
 * Every operation above is an IEEE operation in a fixed order: tests/_mcd_oracle.py restates it in numpy and the results are compared with ==.
 *
 * Not here: SPTK / WORLD mel-generalised (frequency-warped all-pole) cepstra (this is the log-mel-cepstrum MCD), c0-inclusive variants,
 * voiced-only or silence masks, other DTW step patterns or slope weights, soft-DTW, gradients, streamed inputs.
 *
 * Same conventions as vtts_dtw.h / vtts_stft.h (vtts_status and vtts_last_error() of vtts_hifigan.h): plain pointers and sizes, 0 or a negative
 * vtts_status, inputs, outputs and workspaces in device memory owned by the caller, asynchronous on the given stream.  The one thing the handle
 * keeps on the device is its copy of the basis (K M floats), made at the first call that launches and freed by destroy().
 */
#ifndef VTTS_MCD_H
#define VTTS_MCD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vtts_mcd_cfg {
    int32_t n_mels;      /* M, 1 .. VTTS_MCD_MAX_MELS */
    int32_t n_ceps;      /* K, 1 .. min(M - 1, VTTS_MCD_MAX_CEPS) */
    int32_t band;        /* r >= 0 of vtts_dtw.h, 0 = no band; dtw() only */
    int32_t max_frames;  /* 1 .. VTTS_DTW_MAX_FRAMES (4096): the longest la or lb dtw() accepts */
} vtts_mcd_cfg;

typedef struct vtts_mcd vtts_mcd; /* opaque */

#define VTTS_MCD_MAX_MELS 128
#define VTTS_MCD_MAX_CEPS 64
/* Frames one workgroup of the cepstrum and aligned kernels takes, and the block of the aligned sum's order (above). */
#define VTTS_MCD_FRAMES_PER_BLOCK 64
/* 10 sqrt(2) / ln 10 */
#define VTTS_MCD_ALPHA 6.141851463713754

/* Touches no HIP call: works on a host without a GPU.  VTTS_ERR_INVALID outside the ranges above. */
int vtts_mcd_create(const vtts_mcd_cfg* cfg, int device, vtts_mcd** out);
void vtts_mcd_destroy(vtts_mcd* h);

/* host_out [K][M] fp32: the table the kernels use.  Host only. */
int vtts_mcd_basis(const vtts_mcd* h, float* host_out);

/*
 *   logmel_dev   [N, T_stride, M] fp32; row n's first lens[n] frames, the rest is never read
 *   lens         [N] HOST int32, 0 <= lens[n] <= T_stride (else VTTS_ERR_INVALID, before any launch), or NULL: every row holds T_stride frames
 *   ceps_dev     [N, T_stride, K] fp32: c[t, k]; frames lens[n] .. T_stride - 1 are written as zeros
 */
int vtts_mcd_cepstra(vtts_mcd* h, const float* logmel_dev, int N, int64_t T_stride, const int32_t* lens, float* ceps_dev, void* stream);

/*
 * Scratch bytes aligned() needs for N rows of at most T frames (T = min(Ta_stride, Tb_stride)): the blocks' float64 sums,
 *     blocks = ceil(T / VTTS_MCD_FRAMES_PER_BLOCK),   bytes = round_up(8 * N * blocks, 256),   row n's block q at double index n * blocks + q.
 */
int vtts_mcd_aligned_workspace_bytes(const vtts_mcd* h, int N, int64_t T, size_t* bytes);

/*
 * One fused launch per VTTS_MCD_ROWS_PER_LAUNCH rows forms both cepstra in LDS (they are never written to memory), the distances and the
 * blocks' sums; a second, small one adds each row's blocks.
 *   logmel_a_dev [N, Ta_stride, M], logmel_b_dev [N, Tb_stride, M]
 *   lens         [N] HOST int32, one length for both inputs, 0 <= lens[n] <= min(Ta_stride, Tb_stride) (and <= F_stride with frame_dev), or
 *                NULL: min(Ta_stride, Tb_stride) for every row
 *   sum_dev      [N] float64: the sum above (the caller scales it by alpha / lens[n])
 *   frame_dev    [N, F_stride] fp32 or NULL: d(t, t), zeros from lens[n] on
 *   workspace    256-byte aligned, at least aligned_workspace_bytes(N, min(Ta_stride, Tb_stride)) (else VTTS_ERR_NOMEM)
 */
#define VTTS_MCD_ROWS_PER_LAUNCH 128
int vtts_mcd_aligned(vtts_mcd* h, const float* logmel_a_dev, const float* logmel_b_dev, int N, int64_t Ta_stride, int64_t Tb_stride,
                     const int32_t* lens, double* sum_dev, float* frame_dev, int64_t F_stride, void* workspace, size_t workspace_bytes, void* stream);

/* vtts_dtw_workspace_bytes' formula (vtts_dtw.h), strides 1 .. max_frames. */
int vtts_mcd_dtw_workspace_bytes(const vtts_mcd* h, int N, int64_t Ta_stride, int64_t Tb_stride, size_t* bytes);

/*
 * vtts_dtw_forward (vtts_dtw.h) with D = K and the local cost d(i, j): the same arguments, refusals and workspace layout.
 *   ceps_a_dev   [N, Ta_stride, K] fp32 (cepstra() writes it), first la[n] rows; ceps_b_dev [N, Tb_stride, K], first lb[n] rows
 *   la, lb       [N] HOST int32, 1 <= la[n] <= Ta_stride, 1 <= lb[n] <= Tb_stride
 *   total_dev    [N] fp32; path_len_dev [N] int32; span_dev [N, Ta_stride, 2] int32, rows la[n] .. Ta_stride - 1 set to -1
 * Every pair's results are bit for bit what the pair gives alone.
 */
int vtts_mcd_dtw(vtts_mcd* h, const float* ceps_a_dev, const float* ceps_b_dev, int N, int64_t Ta_stride, int64_t Tb_stride, const int32_t* la,
                 const int32_t* lb, float* total_dev, int32_t* path_len_dev, int32_t* span_dev, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTTS_MCD_H */
