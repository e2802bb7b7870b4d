/*
 * vtts_limiter.h — C ABI of the true-peak meter and the look-ahead limiter: the inter-sample ("true") peak of mono waveforms from a 4x
 * oversampled reconstruction, and a per-sample gain that holds the reconstruction's peaks under a ceiling in dBTP, written out as fp32 or
 * PCM16.  vtts_loudness.h brings a row to a level with ONE gain and a ceiling on its sample values; this stage owns the ceiling instead, so
 * that a single plosive no longer backs a whole sentence off its target.  The reference has no such stage.
 *
 * Everything is mono.  fs = sample_rate, 8000 <= fs <= 96000, else VTTS_ERR_INVALID.  For row b of wav[N, S_stride] with S = lengths[b]
 * samples x[0 .. S - 1] (VTTS_AUDIO_PCM16 samples are multiplied by 2^-15 on load, exact):
 *
 *   oversampling  u[m], m = 0 .. 4 S - 1, is vtts_audio.h's sum for fs -> 4 fs (L = 4, M = 1, half = 96): the same prototype rounded once to
 *                 fp32, zero extension at the row's own ends, and each u[m] ONE fp32 fmaf chain in ascending n that starts with the audio
 *                 kernel's leading zero-pad taps (52 taps a phase, x[n - 27 .. n + 24] for u[4 n + r]).  u is what vtts_audio_forward() gives
 *                 for (fs, 4 fs), bit for bit.  The factor is 4 at EVERY rate.
 *   envelope      p[n] = max(|x[n]|, |u[4 n]|, |u[4 n + 1]|, |u[4 n + 2]|, |u[4 n + 3]|);  true_peak = max_n p[n], 0 for an empty row.  Both
 *                 are exact functions of u.  This is a true-peak meter in the sense of ITU-R BS.1770-4 Annex 2, with this project's
 *                 193-tap Kaiser-windowed sinc in place of the Annex's 48-tap table.  At 4x the reading of a component at the input's
 *                 Nyquist frequency falls short by at most -20 log10 cos(pi / 8) = 0.69 dB, at half of it by 0.17 dB.
 *   look-ahead    W = max(1, floor(fs * lookahead_ms / 1000 + 0.5)) computed in double, 0 < lookahead_ms <= 10: W <= 960.
 *   gain          with the row's pre-gain g (fp32; 1 without one) and c = fp32(10^(ceiling_dbtp / 20)), every index clamped to [0, S - 1]
 *                 at both stages (edge replication), fl() one fp32 rounding:
 *                     req[n]  = 1 where fl(g p[n]) <= c, else fl(c / fl(g p[n]))
 *                     held[n] = min(req[n - W .. n + W])                         (a minimum is exact: any algorithm gives the same bits)
 *                     a[n]    = min(req[n], fp32(sum(held[n - W .. n + W]) / (2 W + 1)))
 *                 The sum and the division are fp64 in a fixed order anchored at the row's own first sample: for n divisible by
 *                 VTTS_LIMITER_RUN the 2 W + 1 terms are added in ascending index from 0.0; every other n takes its predecessor's sum,
 *                 s[n] = (s[n - 1] + held[n + W]) - held[n - W - 1].  So a row gives the same bits alone, in a ragged batch, at any
 *                 S_stride, and as fp32 or as the PCM16 of the same values.
 *   output        y[n] = fl(fl(g x[n]) a[n]), stored as fp32 or as PCM16 by vtts_audio.h's rule (clip to [-1, 1], times 32767 in double,
 *                 round half to even, NaN -> 0).
 *   results       per row: true_peak of the INPUT, min_gain = min_n a[n] (1 for an empty row), the gain g that was used, and optionally the
 *                 envelope p.
 *   pre-gain      g = min(10^((target_lufs - I) / 20), 10^(max_gain_db / 20)), each term computed in double and rounded to fp32; g = 1 for
 *                 a non-finite I.  I is read where vtts_loudness.h's meter left it on the device.  There is no peak term: the limiter owns
 *                 the ceiling.
 *   non-finite    the results for a row with Inf or NaN samples are unspecified; nothing is read or written out of bounds.
 *
 * What the construction guarantees: a[n] <= req[n] always.  Every held[k] the mean reads is the minimum of a window that contains n, the
 * clamped ones at the ends included, so none of them exceeds req[n]: the mean ramps down ahead of a peak, meets req at it and ramps back
 * over 2 W samples.  From the rounding order the output's SAMPLE peak is at most c (1 + 2^-23)^2.  The output's TRUE peak is not bounded by
 * construction, since the gain varies between samples; measured on speech-like rows 3 .. 12 dB over a -1 dBTP ceiling it passes the ceiling
 * by 0.0001 .. 0.0004 dB, on clicks and a plateau by up to 0.0035 dB.  Rows with fl(g true_peak) <= c come back as
 * fl(g x[n]) exactly, with min_gain = 1.
 * tests/_limiter_oracle.py restates the contract in float64 and, for the error scale, in float32.
 *
 * Out of scope: loudness range (LRA), release shaping other than the symmetric window, multiband or soft-knee compression, re-metering or
 * iterating until the limited row lands exactly on the target, stereo, gradients.
 *
 * Same conventions as vtts_loudness.h (vtts_status and vtts_last_error() of vtts_hifigan.h): plain pointers and sizes, 0 or a negative
 * vtts_status, device memory owned by the caller, asynchronous on the given stream.  The handle owns nothing on the device: the 208 taps
 * travel as kernel arguments.
 */
#ifndef VTTS_LIMITER_H
#define VTTS_LIMITER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vtts_limiter_cfg {
    int32_t sample_rate; /* Hz: 8000 .. 96000 */
    float lookahead_ms;  /* 0 < lookahead_ms <= 10; 5.0 is the usual value */
} vtts_limiter_cfg;

typedef struct vtts_limiter vtts_limiter; /* opaque */

#define VTTS_LIMITER_MIN_RATE 8000
#define VTTS_LIMITER_MAX_RATE 96000
#define VTTS_LIMITER_OVERSAMPLE 4
#define VTTS_LIMITER_MAX_LOOKAHEAD_MS 10.0
/* Consecutive samples of one row one workgroup covers, in both kernels. */
#define VTTS_LIMITER_TILE 4096
/* Consecutive samples whose window sums are derived from the first one's (the contract's fixed order). */
#define VTTS_LIMITER_RUN 16
/* Taps of one phase, the zero padding included. */
#define VTTS_LIMITER_PHASE_TAPS 52

/* Touches no HIP call: works on a host without a GPU.  VTTS_ERR_INVALID for a rate or a look-ahead outside the ranges above. */
int vtts_limiter_create(const vtts_limiter_cfg* cfg, int device, vtts_limiter** out);
void vtts_limiter_destroy(vtts_limiter* h);

/* W in samples. */
int vtts_limiter_lookahead(const vtts_limiter* h, int32_t* W);
/* The taps the kernels use, [4][VTTS_LIMITER_PHASE_TAPS] fp32 to host memory: row r is phase r in ascending n, zero padding first. */
int vtts_limiter_taps(const vtts_limiter* h, float* host_out);

/* Scratch bytes true_peak() and apply() need for N rows whose longest has S samples: the envelope and two slots per tile. */
int vtts_limiter_workspace_bytes(const vtts_limiter* h, int N, int64_t S, size_t* bytes);

/*
 *   wav_dev            [N, S_stride] samples of `dtype` (VTTS_AUDIO_F32 = 0 | VTTS_AUDIO_PCM16 = 1 of vtts_audio.h), device memory
 *   lengths            [N] HOST int32 sample counts, 0 <= lengths[b] <= S_stride; NULL = every row has S_stride.  Read before the call returns.
 *   true_peak_dev      [N] fp32
 *   envelope_dev       NULL, or [N, S_stride] fp32: p[n], and 0 from lengths[b] to S_stride - 1
 *   workspace          >= workspace_bytes(N, longest row) bytes, 16-byte aligned; its contents need not survive the call
 * Every per-row offset is 64-bit.
 */
int vtts_limiter_true_peak(vtts_limiter* h, const void* wav_dev, int dtype, int N, int64_t S_stride, const int32_t* lengths, float* true_peak_dev,
                           float* envelope_dev, void* workspace, size_t workspace_bytes, void* stream);

/* gains_dev[b] = the pre-gain of the contract from integrated_dev[b], N rows, both [N] fp32 on the device. */
int vtts_limiter_pregain(vtts_limiter* h, const float* integrated_dev, int N, float target_lufs, float max_gain_db, float* gains_dev, void* stream);

/*
 *   wav_dev, dtype, N, S_stride, lengths, envelope_dev, workspace     as true_peak()
 *   gains_dev          NULL (g = 1 for every row), or [N] fp32 pre-gains on the device (pregain()'s, or the caller's)
 *   out_dev            samples of `out_dtype`; row b has lengths[b] samples.
 *                      O_stride > 0: [N, O_stride], O_stride >= the longest row; samples lengths[b] .. O_stride - 1 of row b are set to 0.
 *                      O_stride == 0: PACKED, row b starts at the sum of the lengths before it.
 *   true_peak_dev, min_gain_dev, gains_used_dev     [N] fp32 each: the results of the contract
 * wav_dev and out_dev must not overlap.
 */
int vtts_limiter_apply(vtts_limiter* h, const void* wav_dev, int dtype, int N, int64_t S_stride, const int32_t* lengths, const float* gains_dev,
                       float ceiling_dbtp, void* out_dev, int out_dtype, int64_t O_stride, float* true_peak_dev, float* min_gain_dev,
                       float* gains_used_dev, float* envelope_dev, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTTS_LIMITER_H */
