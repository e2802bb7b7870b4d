/*
 * vtts_denoise.h — C ABI of STFT-domain spectral subtraction in ONE pass: forward transform, magnitude subtraction with the phase kept, inverse
 * transform and overlap-add, with no spectrum in device memory.  With a bias measured from a vocoder's output for an empty mel it is the
 * "denoising strength" of published HiFi-GAN / WaveGlow inference scripts; with one measured from room tone it is plain spectral subtraction.
 * Batched and ragged.  The reference project has no such stage.
 *
 * One handle = a vtts_stft_cfg {n_fft, win, hop, framing}: the transform lengths, framings, window, tables, row lengths and refusals are
 * vtts_stft.h's, and so is the packed blob: bind_packed() adopts what a vtts_stft of the same n_fft and win packed.  H = n_fft / 2.
 *
 *   contract     every operation fp32 and rounded on its own (fl), no FMA contraction.  For row b, frame t < T_b, bin f = 0 .. H:
 *                    c  = forward(wav)[t, f]                                  vtts_stft.h's forward, bit for bit
 *                    r  = sqrt(fl(fl(c.re^2) + fl(c.im^2)))                   correctly rounded root
 *                    sb = fl(strength bias[f])
 *                    m  = max(fl(r - sb), 0)
 *                    d  = fl(r + 1e-16f)
 *                    c' = (fl(m fl(c.re / d)), fl(m fl(c.im / d)))            IEEE divides
 *                    out = inverse(c')                                        vtts_stft.h's inverse, steps 1 to 4: ascending-t sums, IEEE divide
 *                                                                             by the envelope, 1 / n_fft, the one PCM16 rule
 *                VTTS_AUDIO_PCM16 input is multiplied by 2^-15 on load (exact).  bias[f] >= 0 and strength >= 0, both finite.
 *   hence        apply() equals vtts_stft_inverse(gain(vtts_stft_forward(wav))) bit for bit, gain being the five lines above in IEEE float32
 *                (numpy's on the host); and a row gives the same bits alone, in a ragged batch, at any stride, whatever lies past its S_b
 *                samples, and on either side of the VTTS_DENOISE_ROWS_PER_LAUNCH split.  Nothing is written past lengths[b].
 *   NOLA         apply() refuses a row whose vtts_stft_min_envelope() is below VTTS_DENOISE_NOLA_FLOOR with VTTS_ERR_INVALID, as
 *                vtts_stft_inverse() does.
 *
 * Choices the kernel makes (viettts_amd/csrc/denoise.hip: denoise_k; csrc/stft_front.h, stft_back.h, stockham.h); no result depends on them:
 *   blocking     vtts_stft_inverse()'s: a workgroup of W = 8 (4 at n_fft = 2048) waves owns a run of 1024, 2048, 4096, 4096
 *                (n_fft = 256 .. 2048) consecutive output samples of a row, thread i samples i, i + 64 W, ...: their y and e stay in registers.
 *                It walks the frames whose window covers the run in ascending t, W per round.  In a round each wave reads its frame's n_fft
 *                samples STRAIGHT FROM GLOBAL MEMORY (reflected at the row's own ends) into the first pass of the forward transform in its
 *                own exchange buffer (no staged span), splits the result into bins, scales each pair of bins in registers, applies the
 *                inverse split step and inverse-transforms in the same buffer.  After a workgroup barrier every thread adds the round's
 *                frames to its samples in ascending t.  No atomics; no spectrum leaves the workgroup.
 *   LDS          8 H + 8 (H / 2 + 2)  the tables  + 4 n_fft  the window  + 4 (H + 2)  fl(strength bias[f])  + 8 W (H + H / 8)  the exchange buffers
 *                (60.0 KB at 2048, 48.0 KB at 1024), within VTTS_SPECTRAL_LDS_BUDGET.
 *   cost         neighbouring workgroups both transform, in both directions, the frames that straddle their border: (run + n_fft) / run =
 *                1.25x the frames at 1024, 1.5x at 2048.
 *
 * Same conventions as vtts_stft.h: plain pointers and sizes, 0 or a negative vtts_status (vtts_last_error()), host lengths[N] (NULL = the
 * stride), 64-bit row offsets, device memory owned by the caller, asynchronous on the given stream.  No gradients, no streamed state.
 */
#ifndef VTTS_DENOISE_H
#define VTTS_DENOISE_H

#include <stddef.h>
#include <stdint.h>

#include "vtts_stft.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vtts_denoise vtts_denoise; /* opaque */

/* The longest row, in samples (VTTS_STFT_MAX_SAMPLES). */
#define VTTS_DENOISE_MAX_SAMPLES 16777216
/* Rows whose lengths one launch carries as kernel arguments. */
#define VTTS_DENOISE_ROWS_PER_LAUNCH 128
/* The least overlap-add envelope apply() accepts (VTTS_STFT_NOLA_FLOOR). */
#define VTTS_DENOISE_NOLA_FLOOR 1e-11

/* Accepts and refuses what vtts_stft_create() does.  Touches no HIP call: works on a host without a GPU. */
int vtts_denoise_create(const vtts_stft_cfg* cfg, int device, vtts_denoise** out);
void vtts_denoise_destroy(vtts_denoise* h);

/* The waves and the run of output samples of one workgroup. */
int vtts_denoise_blocking(const vtts_denoise* h, int* waves, int* run);

/* vtts_stft.h's blob: pack() uploads the tables into the caller's blob (256-byte aligned, >= packed_bytes) and waits; bind_packed() adopts a
 * blob that a vtts_denoise or a vtts_stft of the same n_fft and win packed. */
int vtts_denoise_packed_bytes(const vtts_denoise* h, size_t* bytes);
int vtts_denoise_pack(vtts_denoise* h, void* dev_blob, size_t blob_bytes, void* stream);
int vtts_denoise_bind_packed(vtts_denoise* h, void* dev_blob, size_t blob_bytes);

/*
 *   wav_dev    [N, S_stride] samples of `in_dtype` (VTTS_AUDIO_F32 = 0 | VTTS_AUDIO_PCM16 = 1 of vtts_audio.h), device memory
 *   lengths    [N] HOST int32 sample counts, at most S_stride and out_stride; NULL = every row has S_stride.  Read before the call returns.
 *   bias_dev   [n_fft / 2 + 1] fp32, >= 0, device memory
 *   strength   >= 0, finite
 *   out_dev    [N, out_stride] of `out_dtype`; samples past lengths[b] are not written.  Must not overlap wav_dev (VTTS_ERR_INVALID).
 * VTTS_ERR_STATE before pack() / bind_packed().
 */
int vtts_denoise_apply(vtts_denoise* h, const void* wav_dev, int in_dtype, int N, int64_t S_stride, const int32_t* lengths,
                       const float* bias_dev /* [n_fft/2+1], >= 0 */, float strength /* >= 0, finite */,
                       void* out_dev, int out_dtype, int64_t out_stride, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTTS_DENOISE_H */
