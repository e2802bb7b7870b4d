/*
 * vtts_pitch.h — C ABI of the batched F0 tracker: YIN (de Cheveigné & Kawahara 2002, steps 2-5) on the mel front end's framing, so
 * that f0[N, T] lines up with vtts_mel_forward's mel[N, T, n_mels] frame for frame.  The reference has no pitch stage; this is what
 * gives the F0 error and the voicing error between a recording and its resynthesis (viettts_amd/pitch.py).
 *
 * For row b of wav[N, S_stride], with n_fft = VTTS_PITCH_NFFT, hop = VTTS_PITCH_HOP, pad = VTTS_PITCH_PAD, W = VTTS_PITCH_WINDOW:
 *
 *   lags         tau_max = floor(sample_rate / fmin),  tau_min = ceil(sample_rate / fmax)   (the quotients in double precision)
 *                2 <= tau_min <= tau_max <= VTTS_PITCH_MAX_LAG and 0 < threshold < 1, else VTTS_ERR_INVALID.
 *   framing      the row's first lengths[b] samples are reflect-padded by pad at the row's OWN ends (vtts_mel.h); frame t = padded
 *                samples [hop t, hop t + n_fft); T_b = (lengths[b] + 2 pad - n_fft) / hop + 1, the rule of vtts_mel_num_frames.
 *                VTTS_MEL_PCM16 samples are multiplied by 2^-15 on load (exact).  With x the frame and
 *                    base = (n_fft - W - tau_max) / 2                                   (integer division)
 *                the analysed span is x[base .. base + W - 1 + tau_max], centred in the frame; tau_max = 512 uses the whole frame.
 *   difference   for tau = 0 .. tau_max, d[tau] is ONE fp32 chain in ascending j = 0 .. W - 1:
 *                    s = 0;   e = x[base + j] - x[base + j + tau];   s = s + e * e
 *                (subtract, multiply, add, each rounded to fp32; never fused into an FMA, split or reassociated)
 *   normalise    c[0] = 1, run = 0; for tau = 1 .. tau_max in order:
 *                    run = run + d[tau];   c[tau] = run > 0 ? (d[tau] * (float)tau) / run : 1
 *                (one sequential fp32 chain for run; the multiply is rounded, the divide is IEEE.  run > 0 keeps digital silence,
 *                d = 0 everywhere, out of 0 / 0.)
 *   pick         tau* = the smallest tau in [tau_min, tau_max] with c[tau] < threshold and (tau == tau_max or c[tau + 1] >= c[tau]):
 *                the first dip below the threshold, walked down to its local minimum.  If it exists the frame is voiced.  Otherwise
 *                it is unvoiced and tau* = the first position of the minimum of c over [tau_min, tau_max].
 *   refine       if tau* + 1 <= tau_max:  a = c[tau* - 1], b = c[tau*], g = c[tau* + 1]  (c[tau_min - 1] is used although it is outside the
 *                search range);  den = (a + g) - (b + b);  if den > 0:  delta = (0.5f * (a - g)) / den, clamped to [-1, 1], and
 *                tau_f = (float)tau* + delta.  In every other case tau_f = (float)tau*.
 *   results      candidate = (float)sample_rate / tau_f;   aperiodicity = c[tau*];   f0 = voiced ? candidate : 0.
 *
 * Every operation above is an IEEE fp32 operation in a fixed order: tests/_pitch_oracle.py restates it in numpy float32 and the
 * results are compared with ==.  Inputs are documented as finite (PCM, or floats of a few units at most: d must not overflow).
 *
 * Same conventions as vtts_mel.h / vtts_dtw.h (vtts_status and vtts_last_error() of vtts_hifigan.h): plain pointers and sizes, 0 or
 * a negative vtts_status, device memory owned by the caller, asynchronous on the given stream.  The handle owns nothing on the device.
 */
#ifndef VTTS_PITCH_H
#define VTTS_PITCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vtts_pitch_cfg {
    int32_t sample_rate;
    float fmin;       /* lowest F0 searched: tau_max = floor(sample_rate / fmin) */
    float fmax;       /* highest F0 searched: tau_min = ceil(sample_rate / fmax) */
    float threshold;  /* YIN's absolute threshold on c, 0 < threshold < 1 */
} vtts_pitch_cfg;

typedef struct vtts_pitch vtts_pitch; /* opaque */

/* The mel front end's framing (vtts_mel.h at its only supported n_fft) and YIN's integration window. */
#define VTTS_PITCH_NFFT 1024
#define VTTS_PITCH_HOP 256
#define VTTS_PITCH_PAD 384
#define VTTS_PITCH_WINDOW 512
/* The longest lag: W + tau_max samples must fit in one frame. */
#define VTTS_PITCH_MAX_LAG 512
/* Consecutive frames of one row that one workgroup computes (one wave each) from one staged span of samples. */
#define VTTS_PITCH_FRAMES_PER_BLOCK 8
/* Shortest row, as VTTS_MEL_MIN_SAMPLES: a single reflection must suffice. */
#define VTTS_PITCH_MIN_SAMPLES 385

/* Touches no HIP call: works on a host without a GPU.  VTTS_ERR_INVALID outside the ranges above. */
int vtts_pitch_create(const vtts_pitch_cfg* cfg, int device, vtts_pitch** out);
void vtts_pitch_destroy(vtts_pitch* h);

/* T = (n_samples + 2 pad - n_fft) / hop + 1 = vtts_mel_num_frames; VTTS_ERR_SHAPE below VTTS_PITCH_MIN_SAMPLES. */
int vtts_pitch_num_frames(const vtts_pitch* h, int64_t n_samples, int64_t* frames);

/* Scratch bytes forward() needs for N rows of S samples (0: one frame's d and c live in LDS). */
int vtts_pitch_workspace_bytes(const vtts_pitch* h, int N, int64_t S, size_t* bytes);

/*
 *   wav_dev            [N, S_stride] samples of `dtype` (VTTS_MEL_F32 = 0 | VTTS_MEL_PCM16 = 1 of vtts_mel.h), device memory
 *   lengths            [N] HOST int32 sample counts, VTTS_PITCH_MIN_SAMPLES <= lengths[b] <= S_stride; NULL = every row has S_stride.
 *                      Read before the call returns.
 *   f0_dev, aperiodicity_dev, candidate_dev
 *                      [N, T_stride] fp32 each, T_stride >= the longest row's frame count.  Row b's first T_b frames are bit for bit what
 *                      the row gives alone; frames T_b .. T_stride - 1 hold 0 / 1 / 0 (f0 / aperiodicity / candidate).
 *   workspace          unused (workspace_bytes is 0); may be NULL
 * Every per-row offset is 64-bit.
 */
int vtts_pitch_forward(vtts_pitch* h, const void* wav_dev, int dtype, int N, int64_t S_stride, const int32_t* lengths, float* f0_dev,
                       float* aperiodicity_dev, float* candidate_dev, int64_t T_stride, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTTS_PITCH_H */
