/*
 * vtts_mel.h — C ABI of the waveform -> log-mel front end (the analysis direction of NTT123/vietTTS):
 *     vietTTS/nat/dsp.py            MelFilter.__call__(y)                      (JAX)
 *     vietTTS/hifigan/create_mel.py mel_spectrogram(y, ..., center=False)     (torch)
 * Both compute, for y[N, S]:
 *     reflect-pad each row by p = (n_fft - hop) / 2; frame t = padded samples [hop t, hop t + n_fft) times the periodic
 *     Hann window; DFT bins 0 .. n_fft / 2; mag = sqrt(re^2 + im^2 + 1e-9); mel = melfb @ mag (librosa.filters.mel
 *     defaults: Slaney scale, Slaney area normalisation); out[N, T, n_mels] = log(max(mel, 1e-5)).
 * The output layout is vtts_hifigan_forward's input layout.  One fused kernel: the spectrum never reaches HBM.
 *
 * Same conventions as vtts_hifigan.h (whose vtts_status / vtts_last_error() this header uses): plain pointers and sizes,
 * 0 or a negative vtts_status, device memory owned by the caller, asynchronous on the given stream.  The handle owns
 * only host-side tables (window, twiddles, filter bank), which it computes itself in double precision.
 */
#ifndef VTTS_MEL_H
#define VTTS_MEL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* vietTTS/nat/config.py:43-47 (assets/hifigan/config.json agrees): 16000, 1024, 256, 80, 0, 8000. */
typedef struct vtts_mel_cfg {
    int32_t sample_rate;
    int32_t n_fft;   /* window = transform length; the kernel is built for 1024, anything else is VTTS_ERR_INVALID */
    int32_t hop;     /* must be n_fft / 4, the only relation the reference uses */
    int32_t n_mels;  /* 1 .. 128 */
    float fmin;      /* 0 <= fmin < fmax <= sample_rate / 2 */
    float fmax;
} vtts_mel_cfg;

typedef struct vtts_mel vtts_mel; /* opaque */

/* input sample formats of forward() */
#define VTTS_MEL_F32 0   /* float, as is */
#define VTTS_MEL_PCM16 1 /* int16 PCM, divided by 2^15 on load (vietTTS/nat/gta.py:31) */

/* Consecutive frames of one row that one workgroup computes (one wave each) from one staged span of samples. */
#define VTTS_MEL_FRAMES_PER_BLOCK 8
/* Shortest row: a single reflection must suffice, lengths[b] >= (n_fft - hop) / 2 + 1 (torch's rule for reflect padding). */
#define VTTS_MEL_MIN_SAMPLES 385

/* Touches no HIP call: works on a host without a GPU. */
int vtts_mel_create(const vtts_mel_cfg* cfg, int device, vtts_mel** out);
void vtts_mel_destroy(vtts_mel* h);

/* T = (n_samples + 2 p - n_fft) / hop + 1 (= n_samples / 256 for the default configuration); VTTS_ERR_SHAPE below
 * VTTS_MEL_MIN_SAMPLES. */
int vtts_mel_num_frames(const vtts_mel* h, int64_t n_samples, int64_t* frames);

/* The [n_mels, n_fft / 2 + 1] basis rounded to fp32, to host memory. */
int vtts_mel_filterbank(const vtts_mel* h, float* host_out);

/* The tables (window, twiddles, the basis's non-zeros) as one packed device blob, caller-owned and 256-B aligned, as in
 * vtts_hifigan.h: pack() fills it on the stream and waits; bind_packed() adopts a blob another handle of the same
 * configuration packed. */
int vtts_mel_packed_bytes(const vtts_mel* h, size_t* bytes);
int vtts_mel_pack(vtts_mel* h, void* dev_blob, size_t blob_bytes, void* stream);
int vtts_mel_bind_packed(vtts_mel* h, void* dev_blob, size_t blob_bytes);

/* Scratch bytes forward() needs for N rows of S samples (0: the pass keeps everything on chip). */
int vtts_mel_workspace_bytes(const vtts_mel* h, int N, int64_t S, size_t* bytes);

/*
 *   wav_dev   [N, S_stride] samples of `dtype` (VTTS_MEL_F32 | VTTS_MEL_PCM16), device memory
 *   lengths   [N] HOST int32 sample counts, VTTS_MEL_MIN_SAMPLES <= lengths[b] <= S_stride; NULL = every row has S_stride
 *   mel_dev   [N, T_stride, n_mels] fp32, T_stride >= the longest row's frame count.  Row b's first
 *             T_b = num_frames(lengths[b]) frames are bit for bit what the row gives alone (it is reflected at its OWN end);
 *             frames T_b .. T_stride - 1 are set to logf(1e-5f), the value of a silent frame.
 * The lengths are read before the call returns.
 */
int vtts_mel_forward(vtts_mel* h, const void* wav_dev, int dtype, int N, int64_t S_stride, const int32_t* lengths,
                     float* mel_dev, int64_t T_stride, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTTS_MEL_H */
