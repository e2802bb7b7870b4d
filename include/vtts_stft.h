/*
 * vtts_stft.h — C ABI of the complex short-time Fourier transform at ONE resolution and framing, in both directions, and of the projection
 * step a phase-retrieval loop (Griffin-Lim) repeats: what vtts_spectral.h leaves out.  Batched and ragged.  The reference project has no such
 * stage.
 *
 * One handle = {n_fft, win, hop, framing}: n_fft in {256, 512, 1024, 2048}, 1 <= hop <= win <= n_fft; anything else is VTTS_ERR_INVALID at
 * create().  H = n_fft / 2, NB = H + 1 bins.  Window and tables are vtts_spectral.h's: w[r + (n_fft - win) / 2] = 0.5 - 0.5 cos(2 pi r / win)
 * (periodic Hann, centred, zeros around it), exp(-2 pi i m / H) and exp(-2 pi i k / n_fft), computed in double and rounded ONCE.
 *
 *   framing      padded sample p is row sample g = p - P; g < 0 reads -g, g >= S reads 2 (S - 1) - g.  Frame t covers padded samples
 *                [hop t, hop t + n_fft); T = (S + 2 P - n_fft) / hop + 1 (integer division).
 *                  VTTS_STFT_CENTER  P = n_fft / 2: torch.stft(center=True, pad_mode="reflect"), vtts_spectral.h's.  T = 1 + S / hop.
 *                  VTTS_STFT_MEL     P = (n_fft - hop) / 2: vtts_mel.h's; create() requires n_fft - hop even.  T = S / hop, so a mel of T
 *                                    frames inverts to exactly hop T samples, aligned with the generator's output for that mel.
 *                A row needs max(P + 1, the S of one frame) <= S <= VTTS_STFT_MAX_SAMPLES; anything else is VTTS_ERR_SHAPE.
 *                num_samples(T) is the smallest S with T frames: hop (T - 1) for CENTER, hop T for MEL.
 *   forward      spec[t, f] = sum_n fl32(sample[n] w[n]) exp(-2 pi i f n / n_fft), f = 0 .. H, in fp32: the transform of vtts_spectral.h
 *                (H-point complex Stockham transform of z[n] = v[2 n] + i v[2 n + 1], radix 8 first, and the split step), stored BEFORE that
 *                header's floor: with CENTER framing sqrt(max(re^2 + im^2, 1e-7)) in separately rounded fp32 operations is vtts_spectral.h's M
 *                bit for bit.  VTTS_AUDIO_PCM16 samples are multiplied by 2^-15 on load (exact).
 *   inverse      torch.istft's contract per row:
 *                  1. v_t[n] = sum over the Hermitian extension of spec[t, .] of X[f] exp(+2 pi i f n / n_fft), unscaled; the imaginary
 *                     parts of bins 0 and H are ignored.  Computed as the inverse split step
 *                         A = X[k] + conj X[H - k], B = conj(W^k) (X[k] - conj X[H - k]), Z[k] = A + i B, Z[H - k] = conj(A) + i conj(B)
 *                     and the H-point inverse transform (same radix order, the same tables conjugated): v[2 n] + i v[2 n + 1] = z[n].
 *                  2. with o = p - hop t:  y[p] = sum_t fl32(v_t[o] w[o]),  e[p] = sum_t fl32(w[o] w[o]),  both fp32 sums from 0 in
 *                     ascending t over the frames t < T_b whose window covers p (lead <= o < lead + win).
 *                  3. out[g] = (y[p] / e[p]) (1 / n_fft), p = g + P, g < S_b: an IEEE divide and an exact power of two.
 *                  4. VTTS_AUDIO_PCM16 output is the fp32 value through the library's one rounding rule (rint(clip(x, -1, 1) 32767)).
 *                  5. NOLA: inverse() refuses a row whose min_envelope() is below 1e-11 (torch's rule) with VTTS_ERR_INVALID.  Hann with
 *                     hop == win is such a case.
 *   project      torchaudio's griffinlim update, fused into the forward transform's store so that a spectrum is written once per iteration:
 *                  c = forward(wav)[t, f];  a = c - alpha tprev (alpha = fl32(momentum / fl32(1 + momentum)), per component);
 *                  r = sqrt(fl32(fl32(a.re^2) + fl32(a.im^2))) (correctly rounded);  d = fl32(r + 1e-16f);
 *                  spec = (mag (a.re / d), mag (a.im / d));  tprev = c.  Every operation fp32, rounded on its own.
 *   invariance   every grid is anchored at the row's own first sample and depends on no other row: a row gives the same bits alone or in a
 *                ragged batch, at any stride, whatever lies past its S_b samples or its T_b frames.  Nothing is written past S_b / T_b.
 *
 * Choices the kernels make (viettts_amd/csrc/stft.hip, csrc/stockham.h); no result depends on them:
 *   forward,     one wave per frame, F consecutive frames of a row per workgroup from one staged span of samples in LDS; F = the largest
 *   project      count <= 8 (4 at n_fft = 2048) whose LDS fits VTTS_SPECTRAL_LDS_BUDGET:
 *                    8 H + 8 (H / 2 + 2)  the tables  + 4 even((F - 1) hop + n_fft)  the span  + 8 F (H + H / 8)  the exchange buffers.
 *   inverse      a workgroup of W = 8 (4 at 2048) waves owns a run of 1024, 2048, 4096, 4096 (n_fft = 256 .. 2048) consecutive output samples of a
 *                row, thread i samples i, i + 64 W, ...: their y and e stay in registers.  It walks the frames whose window covers the run
 *                in ascending t, W per round: each wave inverse-transforms one frame in its own exchange buffer, and after a workgroup
 *                barrier every thread adds the round's frames to its samples in ascending t.  No atomics.  LDS:
 *                    8 H + 8 (H / 2 + 2)  the tables  + 4 n_fft  the window  + 8 W (H + H / 8)  the exchange buffers   (56.0 KB at 2048).
 *                Neighbouring workgroups both transform the n_fft / hop frames that straddle their border: (run + n_fft) / run = 1.25x the
 *                frames at 1024, 1.5x at 2048.
 *
 * Same conventions as vtts_spectral.h: plain pointers and sizes, 0 or a negative vtts_status (vtts_last_error()), host lengths[N] (NULL = the
 * stride), 64-bit row offsets, device memory owned by the caller, asynchronous on the given stream.  No gradients.
 */
#ifndef VTTS_STFT_H
#define VTTS_STFT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vtts_stft vtts_stft; /* opaque */

#define VTTS_STFT_CENTER 0
#define VTTS_STFT_MEL 1

typedef struct vtts_stft_cfg {
    int32_t n_fft;   /* 256, 512, 1024 or 2048 */
    int32_t win;     /* hop <= win <= n_fft */
    int32_t hop;     /* >= 1 */
    int32_t framing; /* VTTS_STFT_CENTER | VTTS_STFT_MEL */
} vtts_stft_cfg;

/* The longest row, in samples. */
#define VTTS_STFT_MAX_SAMPLES 16777216
/* Rows whose lengths one launch carries as kernel arguments. */
#define VTTS_STFT_ROWS_PER_LAUNCH 128
/* The least overlap-add envelope inverse() accepts (torch.istft's). */
#define VTTS_STFT_NOLA_FLOOR 1e-11

/* Touches no HIP call: works on a host without a GPU. */
int vtts_stft_create(const vtts_stft_cfg* cfg, int device, vtts_stft** out);
void vtts_stft_destroy(vtts_stft* h);

/* The n_fft window values the kernels use, to host memory. */
int vtts_stft_window(const vtts_stft* h, float* host_out);

/* F of forward() and project(); the waves W and the run of inverse(). */
int vtts_stft_blocking(const vtts_stft* h, int* forward_frames, int* inverse_waves, int* inverse_run);

/* T of a row of n_samples, and the smallest n_samples with `frames` frames (what inverse() writes for a caller who has only T). */
int vtts_stft_num_frames(const vtts_stft* h, int64_t n_samples, int64_t* frames);
int vtts_stft_num_samples(const vtts_stft* h, int64_t frames, int64_t* n_samples);

/* min over g < n_samples of e[g + P] = sum_t w[o]^2, in double from the fp32 window (host arithmetic: the interior is periodic in hop, so one
 * period and both ends are visited). */
int vtts_stft_min_envelope(const vtts_stft* h, int64_t n_samples, double* envelope);

/* The tables, vtts_spectral.h's layout: pack() uploads them into the caller's blob (256-byte aligned, >= packed_bytes) and waits;
 * bind_packed() adopts a blob that another handle of the same n_fft and win packed. */
int vtts_stft_packed_bytes(const vtts_stft* h, size_t* bytes);
int vtts_stft_pack(vtts_stft* h, void* dev_blob, size_t blob_bytes, void* stream);
int vtts_stft_bind_packed(vtts_stft* h, void* dev_blob, size_t blob_bytes);

/*
 *   wav_dev    [N, S_stride] samples of `dtype` (VTTS_AUDIO_F32 = 0 | VTTS_AUDIO_PCM16 = 1 of vtts_audio.h), device memory
 *   lengths    [N] HOST int32 sample counts; NULL = every row has S_stride.  Read before the call returns.
 *   spec_dev   [N, T_stride, n_fft / 2 + 1] float2 (re, im), T_stride >= num_frames(longest row); frames past T_b are not written
 * VTTS_ERR_STATE before pack() / bind_packed().
 */
int vtts_stft_forward(vtts_stft* h, const void* wav_dev, int dtype, int N, int64_t S_stride, const int32_t* lengths, void* spec_dev,
                      int64_t T_stride, void* stream);

/*
 *   spec_dev   [N, T_stride, n_fft / 2 + 1] float2; row b's first num_frames(lengths[b]) frames are read
 *   lengths    [N] HOST int32 SAMPLE counts of the output rows; NULL = every row has S_stride
 *   out_dev    [N, S_stride] of `dtype`; samples past lengths[b] are not written
 */
int vtts_stft_inverse(vtts_stft* h, const void* spec_dev, int N, int64_t T_stride, const int32_t* lengths, void* out_dev, int dtype,
                      int64_t S_stride, void* stream);

/*
 *   mag_dev    [N, T_stride, n_fft / 2 + 1] fp32: the magnitudes the spectrum is projected onto
 *   tprev_dev  [N, T_stride, n_fft / 2 + 1] float2, read and overwritten (zeros before the first iteration)
 *   spec_dev   [N, T_stride, n_fft / 2 + 1] float2, written; must not overlap tprev_dev
 */
int vtts_stft_project(vtts_stft* h, const void* wav_dev, int dtype, int N, int64_t S_stride, const int32_t* lengths, const float* mag_dev,
                      void* tprev_dev, void* spec_dev, int64_t T_stride, float momentum, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTTS_STFT_H */
