/*
 * vtts_audio.h — C ABI of the audio stage either side of the models: rational sample-rate conversion and PCM16 in and out.
 * The synthesis direction ends in fp32 samples at 16 kHz and a WAV file holds PCM16 at whatever rate its user needs; the
 * analysis direction (vtts_mel.h) begins at 16 kHz.  One fused kernel: samples of one format and rate in, samples of another out.
 *
 * The arithmetic (the contract; tests/_audio_oracle.py restates it in fp64):
 *     g = gcd(in_rate, out_rate), L = out_rate / g, M = in_rate / g, R = max(L, M), Z = 24, half = Z R
 *     prototype  h[n] = L w[n] / sum(w),  w[n] = sinc(n / R) / R * kaiser(2 half + 1, beta = 10)[n + half],  n = -half .. half
 *                (sinc(x) = sin(pi x) / (pi x); kaiser(N, beta)[k] = I0(beta sqrt(1 - (2 k / (N - 1) - 1)^2)) / I0(beta))
 *     a row of S samples gives So = ceil(S L / M) samples,
 *     y[m] = sum_n x[n] h[m M - n L + half],  n = max(0, ceil((m M - half) / L)) .. min(S - 1, floor((m M + half) / L)):
 *     zero extension at the row's OWN ends.  With scipy: resample_poly(x, L, M, window=h / L).
 * Z = 24 and beta = 10 give, at the worst of 3/1, 1/2, 3/2, 441/160, 160/441, 320/441, a passband within 1e-4 dB up to 0.85 of the
 * narrower Nyquist frequency and a stopband of -100 dB from 1.15 of it: below one PCM16 step.
 * The taps are rounded once to fp32; one output is ONE fp32 fmaf chain in ascending n, whatever the batch, the layout or the tile:
 * a row gives the same bits alone, in a ragged batch, strided or packed.  (The chain starts with up to 4 zero taps of the
 * table's padding, on the samples just before the window: they leave a finite sum as it is, but an Inf or NaN sample reaches the
 * outputs that far past its window as well.)
 * in_rate == out_rate: no filter at all; forward() converts the format and packs, f32 -> f32 is a copy.
 *
 * PCM16 in: divided by 2^15 on load, as vtts_mel.h.  PCM16 out is libsndfile's rule (viettts_amd/wavio.py float_to_pcm16): clip to
 * [-1, 1], times 32767 without intermediate rounding (computed in double), round half to even; NaN gives 0.
 *
 * Same conventions as vtts_mel.h and vtts_hifigan.h (whose vtts_status / vtts_last_error() this header uses): plain pointers and
 * sizes, 0 or a negative vtts_status, device memory owned by the caller, asynchronous on the given stream.  The handle owns only
 * the host-side tap table, which it computes itself in double precision.
 */
#ifndef VTTS_AUDIO_H
#define VTTS_AUDIO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vtts_audio_cfg {
    int32_t in_rate;  /* Hz, > 0 */
    int32_t out_rate; /* Hz, > 0; max(L, M) <= VTTS_AUDIO_MAX_R */
} vtts_audio_cfg;

typedef struct vtts_audio vtts_audio; /* opaque */

/* sample formats of forward(), on either side */
#define VTTS_AUDIO_F32 0   /* float */
#define VTTS_AUDIO_PCM16 1 /* int16 PCM */

#define VTTS_AUDIO_ZEROS 24     /* Z: zero crossings of the sinc on each side of the prototype's centre */
#define VTTS_AUDIO_BETA 10.0    /* the Kaiser window's beta */
#define VTTS_AUDIO_MAX_R 2048   /* largest max(L, M): the tap table's size */
/* Consecutive outputs of one row that one workgroup computes from one staged span of input samples. */
#define VTTS_AUDIO_OUT_PER_BLOCK 1024
/* The span of VTTS_AUDIO_OUT_PER_BLOCK outputs is staged in LDS, so the decimation M / L is bounded too: a configuration whose span
 * passes this many bytes (M / L above about 30) is VTTS_ERR_INVALID. */
#define VTTS_AUDIO_MAX_SPAN_BYTES 131072

/* Touches no HIP call: works on a host without a GPU.  Rates <= 0 and max(L, M) > VTTS_AUDIO_MAX_R are VTTS_ERR_INVALID. */
int vtts_audio_create(const vtts_audio_cfg* cfg, int device, vtts_audio** out);
void vtts_audio_destroy(vtts_audio* h);

/* L, M and half of the contract above (any of the three pointers may be NULL). */
int vtts_audio_ratio(const vtts_audio* h, int32_t* L, int32_t* M, int32_t* half);
/* ceil(n_in L / M); n_in >= 0. */
int vtts_audio_out_samples(const vtts_audio* h, int64_t n_in, int64_t* n_out);
/* The 2 half + 1 taps h[-half .. half] in double, to host memory (for oracles; the kernel uses their fp32 roundings). */
int vtts_audio_prototype(const vtts_audio* h, double* host_out);

/* The tap table (L phases x taps per phase, fp32, zero-padded to a multiple of 4 taps; four taps of every phase side by side) as one
 * packed device blob, caller-owned and 256-B aligned, as in vtts_mel.h: pack() fills it on the stream and waits; bind_packed() adopts a
 * blob another handle of the same configuration packed. */
int vtts_audio_packed_bytes(const vtts_audio* h, size_t* bytes);
int vtts_audio_pack(vtts_audio* h, void* dev_blob, size_t blob_bytes, void* stream);
int vtts_audio_bind_packed(vtts_audio* h, void* dev_blob, size_t blob_bytes);

/*
 *   in_dev    [N, S_stride] samples of `in_dtype`, device memory
 *   lengths   [N] HOST int32 sample counts, 0 <= lengths[b] <= S_stride; NULL = every row has S_stride.  Read before the call returns.
 *   out_dev   samples of `out_dtype`.  Row b has So_b = out_samples(lengths[b]) samples.
 *             O_stride > 0: [N, O_stride], O_stride >= the longest row's So; samples So_b .. O_stride - 1 of row b are set to 0.
 *             O_stride == 0: PACKED, row b starts at the sum of So of the rows before it; sum(So) samples are written.
 * in_dev and out_dev must not overlap.
 */
int vtts_audio_forward(vtts_audio* h, const void* in_dev, int in_dtype, int N, int64_t S_stride, const int32_t* lengths, void* out_dev,
                       int out_dtype, int64_t O_stride, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTTS_AUDIO_H */
