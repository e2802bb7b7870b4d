/*
 * vtts_loudness.h — C ABI of the batched loudness meter: ITU-R BS.1770-4 integrated loudness (the "LUFS" figure of EBU R 128) of mono
 * waveforms, and a per-row gain to a target level written out as fp32 or PCM16.  The reference has no loudness stage; this is what lets
 * either end of the project (vtts_audio.h's PCM16 out, vtts_mel.h's recordings in) say how loud a row is without a host round trip.
 *
 * Everything is mono.  fs = sample_rate, 8000 <= fs <= 96000 and fs divisible by 10, else VTTS_ERR_INVALID.  For row b of
 * wav[N, S_stride] with S = lengths[b] samples x[0 .. S - 1] (VTTS_AUDIO_PCM16 samples are multiplied by 2^-15 on load, exact):
 *
 *   K-weighting  two biquads in cascade, y1 = shelf(x), z = highpass(y1), each a0 = 1:
 *                    y[n] = b0 x[n] + b1 x[n-1] + b2 x[n-2] - a1 y[n-1] - a2 y[n-2]
 *                computed by the handle in double from the analogue prototypes and rounded ONCE to fp32.  With K = tan(pi f0 / fs),
 *                a0 = 1 + K / Q + K^2:
 *                  shelf      f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196,
 *                             Vh = 10^(G / 20), Vb = Vh^0.4996667741545416
 *                             b = [(Vh + Vb K / Q + K^2) / a0, 2 (K^2 - Vh) / a0, (Vh - Vb K / Q + K^2) / a0]
 *                             a = [1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0]
 *                  high-pass  f0 = 38.13547087602444, Q = 0.5003270373238773
 *                             b = [1, -2, 1],   a = [1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0]
 *                At 48 kHz these are the table of BS.1770-4 to 9e-16.  The filter starts from zero state at the row's own first sample.
 *   blocks       H = fs / 10.  Hop sum e_j = sum of z^2 over filtered samples [j H, (j + 1) H), j < floor(S / H); a trailing partial hop
 *                is not used.  Block energy z_j = (((e_j + e_{j+1}) + e_{j+2}) + e_{j+3}) / (4 H): 400 ms at 75 % overlap,
 *                J = max(0, floor(S / H) - 3) blocks.  Momentary loudness l_j = -0.691 + 10 log10 z_j.
 *   gating       absolute gate -70 LUFS; relative gate = -0.691 + 10 log10(mean of z_j over blocks with l_j > -70) - 10;
 *                integrated loudness I = -0.691 + 10 log10(mean of z_j over the blocks with l_j above BOTH gates), -inf when no block
 *                passes: a row shorter than 0.4 s, or a silent one, gives -inf.
 *   outputs      integrated = I and momentary_max = max_j l_j (-inf without a block), rounded to fp32; sample_peak = max |x|, exact;
 *                n_blocks = J; n_gated = the blocks above both gates; optionally the series l_j [N, J_stride], -inf past J_b.
 *   precision    the filter runs in fp32; z^2, the hop sums and everything after them are fp64, accumulated in a fixed order.  The time
 *                grid of the kernel's scan (VTTS_LOUDNESS_CHUNK, VTTS_LOUDNESS_SEGMENT) is anchored at the row's own first sample, so a row
 *                gives the same bits alone, in a ragged batch, at any S_stride, and as fp32 or as the PCM16 of the same values.
 *                tests/_loudness_oracle.py restates the contract in float64 and, for the error scale, in float32.
 *   normalise    g = min(10^((target_lufs - I) / 20), 10^(max_gain_db / 20), 10^(ceiling_dbfs / 20) / sample_peak), each term computed
 *                in double and rounded to fp32 before the min; g = 1 when I = -inf (or NaN).  Output sample = x * g, one fp32 multiply,
 *                stored as fp32 or as PCM16 by vtts_audio.h's rule (clip to [-1, 1], times 32767 in double, round half to even, NaN -> 0).
 *                ceiling_dbfs acts on the SAMPLE peak, and the gain is one number per row: the true-peak (4x oversampled) measurement and
 *                the look-ahead limiter are a separate component, vtts_limiter.h, which takes `integrated` from here.
 *
 * Same conventions as vtts_audio.h (vtts_status and vtts_last_error() of vtts_hifigan.h): plain pointers and sizes, 0 or a negative
 * vtts_status, device memory owned by the caller, asynchronous on the given stream.  The handle owns nothing on the device: the filter's
 * tables (a few hundred floats, computed in double on the host) travel as kernel arguments.
 */
#ifndef VTTS_LOUDNESS_H
#define VTTS_LOUDNESS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vtts_loudness_cfg {
    int32_t sample_rate; /* Hz: 8000 .. 96000, divisible by 10 */
} vtts_loudness_cfg;

typedef struct vtts_loudness vtts_loudness; /* opaque */

#define VTTS_LOUDNESS_MIN_RATE 8000
#define VTTS_LOUDNESS_MAX_RATE 96000
/* Consecutive samples one lane filters from zero state before the lanes' end states are combined. */
#define VTTS_LOUDNESS_CHUNK 32
/* Consecutive samples of one row one workgroup covers (256 lanes x VTTS_LOUDNESS_CHUNK); a wave spans 64 x VTTS_LOUDNESS_CHUNK. */
#define VTTS_LOUDNESS_SEGMENT 8192
/* Hops a segment can meet at most: floor((SEGMENT - 1) / (MIN_RATE / 10)) + 2. */
#define VTTS_LOUDNESS_SEGMENT_HOPS 12

/* Touches no HIP call: works on a host without a GPU.  VTTS_ERR_INVALID for a rate outside the range or not divisible by 10. */
int vtts_loudness_create(const vtts_loudness_cfg* cfg, int device, vtts_loudness** out);
void vtts_loudness_destroy(vtts_loudness* h);

/* The ten coefficients in double, to host memory: shelf b0 b1 b2 a1 a2, then high-pass b0 b1 b2 a1 a2 (for oracles; the kernel uses
 * their fp32 roundings). */
int vtts_loudness_coefficients(const vtts_loudness* h, double* host_out);

/* J = max(0, floor(n_samples / H) - 3); 0 <= n_samples < 2^31. */
int vtts_loudness_num_blocks(const vtts_loudness* h, int64_t n_samples, int64_t* blocks);

/* Scratch bytes measure() needs for N rows whose longest has S samples: every segment's end state, peak and hop partial sums, and the
 * rows' hop sums. */
int vtts_loudness_workspace_bytes(const vtts_loudness* h, int N, int64_t S, size_t* bytes);

/*
 *   wav_dev            [N, S_stride] samples of `dtype` (VTTS_AUDIO_F32 = 0 | VTTS_AUDIO_PCM16 = 1 of vtts_audio.h), device memory
 *   lengths            [N] HOST int32 sample counts, 0 <= lengths[b] <= S_stride; NULL = every row has S_stride.  Read before the call returns.
 *   integrated_dev, momentary_max_dev, sample_peak_dev     [N] fp32 each
 *   n_blocks_dev, n_gated_dev                              [N] int32 each
 *   momentary_dev      NULL, or [N, J_stride] fp32 with J_stride >= the longest row's block count: l_j, and -inf from J_b to J_stride - 1
 *   workspace          >= workspace_bytes(N, longest row) bytes, 8-byte aligned; its contents need not survive the call
 * Every per-row offset is 64-bit.
 */
int vtts_loudness_measure(vtts_loudness* h, const void* wav_dev, int dtype, int N, int64_t S_stride, const int32_t* lengths,
                          float* integrated_dev, float* momentary_max_dev, float* sample_peak_dev, int32_t* n_blocks_dev, int32_t* n_gated_dev,
                          float* momentary_dev, int64_t J_stride, void* workspace, size_t workspace_bytes, void* stream);

/*
 *   wav_dev, dtype, N, S_stride, lengths     as measure()
 *   integrated_dev, sample_peak_dev          [N] fp32 each, as measure() left them on the device (no host round trip)
 *   out_dev            samples of `out_dtype`; row b has lengths[b] samples.
 *                      O_stride > 0: [N, O_stride], O_stride >= the longest row; samples lengths[b] .. O_stride - 1 of row b are set to 0.
 *                      O_stride == 0: PACKED, row b starts at the sum of the lengths before it.
 *   gains_dev          [N] fp32: the gain each row was multiplied by
 * wav_dev and out_dev must not overlap.
 */
int vtts_loudness_normalize(vtts_loudness* h, const void* wav_dev, int dtype, int N, int64_t S_stride, const int32_t* lengths,
                            const float* integrated_dev, const float* sample_peak_dev, float target_lufs, float ceiling_dbfs, float max_gain_db,
                            void* out_dev, int out_dtype, int64_t O_stride, float* gains_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTTS_LOUDNESS_H */
