/*
 * vtts_spectral.h — C ABI of the batched spectral distances at ONE short-time resolution: spectral convergence and log-magnitude L1 (the two
 * parts of the multi-resolution STFT distance of Yamamoto, Song, Kim: Parallel WaveGAN, 2020) and log-spectral distance of a signal under
 * test y against the reference signal x it is sample-aligned with, and, optionally, both magnitude spectrograms: the forward magnitude STFT
 * at any of four transform lengths.  Magnitudes only: the complex spectrum, the inverse transform and the phase are vtts_stft.h's.  The reference
 * project has no such stage.
 *
 * One handle = one resolution {n_fft, win, hop}: n_fft in {256, 512, 1024, 2048}, 1 <= hop <= win <= n_fft; anything else is
 * VTTS_ERR_INVALID at create().  With H = n_fft / 2 and NB = H + 1 bins, for row b of x[N, S_stride] and y[N, S_stride] with S = lengths[b]
 * samples each (VTTS_AUDIO_PCM16 samples are multiplied by 2^-15 on load, exact):
 *
 *   framing      torch.stft(center=True, pad_mode="reflect"): padded sample p is row sample g = p - H, g < 0 reads -g, g >= S reads
 *                2 (S - 1) - g.  Frame t covers padded samples [hop t, hop t + n_fft); T = 1 + S / hop (integer division).
 *                A row needs H + 1 <= S <= VTTS_SPECTRAL_MAX_SAMPLES; anything else is VTTS_ERR_SHAPE.
 *   window       w[r + (n_fft - win) / 2] = 0.5 - 0.5 cos(2 pi r / win), r = 0 .. win - 1 (periodic Hann, centred, zeros around it; the
 *                offset is an integer division), computed by the handle in double and rounded ONCE to fp32 (vtts_spectral_window()).
 *   transform    v[n] = fl32(sample[n] * w[n]); X[f] = sum_n v[n] exp(-2 pi i f n / n_fft), f = 0 .. H, in fp32: an H-point complex
 *                transform of z[n] = v[2 n] + i v[2 n + 1] (radix-8 and radix-4 Stockham passes, 8 first) and the split step
 *                    E = (Z[k] + conj Z[H - k]) / 2, O = -i (Z[k] - conj Z[H - k]) / 2, X[k] = E + W^k O, X[H - k] = conj(E - W^k O),
 *                with twiddles computed in double on the host and rounded once.  x and y go through the SAME code one after the other
 *                (never packed into one complex transform): each signal's error is relative to its own level, and x == y gives equal bits.
 *   bins         P = max(re^2 + im^2, 1e-7) and M = sqrt(P), both fp32 (the square root correctly rounded).
 *   terms        per bin, in fp64 from the fp32 values: d = My - Mx; a = d^2; b = Mx^2; L = ln(Py / Px) (one fp64 quotient, one fp64
 *                logarithm); c = |L| / 2 (= |ln My - ln Mx|); e = (10 L / ln 10)^2 (= (10 log10(Py / Px))^2).
 *   order        every sum is fp64, in THIS order.  Within frame t, lane l = 0 .. 63 adds, for j = 0, 1, ... while k = l + 64 j <= H / 2,
 *                bin k and then bin H - k (the second only where it is another bin: k != H / 2; k = 0 pairs with the Nyquist bin H);
 *                the 64 lane sums are combined by six halvings s_l <- s_l + s_(l + h) for l < h, h = 32, 16, 8, 4, 2, 1.  That gives
 *                A_t = sum a, B_t = sum b, C_t = sum c, E_t = sum e; D_t = sqrt(E_t / NB).
 *                Workgroup g owns frames F g .. F g + F - 1 (F = vtts_spectral_frames_per_block()) and adds its frames below T in
 *                ascending t from 0.0: four partials (A, B, C, D) per (row, workgroup).  A second kernel gives lane l the partials of
 *                workgroups l, l + 64, ... in ascending order and combines the lanes by the same six halvings.
 *   figures      sc = sqrt(A) / sqrt(B); logmag = C / (T NB); lsd = D / T (dB); n_frames = T.  fp64 outputs: the figures are means over up
 *                to 10^7 bins, and an fp32 store would be coarser than their error.
 *   mags         optional [N, 2, T_stride, NB] fp32: Mx, then My; entries past T_b are not written.  When it is NULL no spectrum reaches
 *                HBM and the figures are the same bits.
 *   invariance   every grid is anchored at the row's own first sample: a row gives the same bits alone or in a ragged batch, at any
 *                S_stride, whatever lies past its length, and as fp32 or as the PCM16 of the same values.  x == y gives
 *                sc = logmag = lsd = 0 exactly.
 *
 * Choices the kernel makes (viettts_amd/csrc/spectral.hip), stated here because results depend on F alone:
 *   tables       a packed blob (packed_bytes / pack / bind_packed as in vtts_mel.h): the window [n_fft], exp(-2 pi i m / H) for m < H and
 *                exp(-2 pi i k / n_fft) for k <= H / 2.  At n_fft = 2048 they are 20 KB: too large for kernel arguments.
 *   frames per   one wave per frame.  F = the largest count <= VTTS_SPECTRAL_MAX_FRAMES_PER_BLOCK(n_fft) = 8, 8, 8, 4 (n_fft = 256, 512, 1024,
 *   workgroup    2048) whose LDS fits VTTS_SPECTRAL_LDS_BUDGET = 80 KB, so that two workgroups share a CU's 160 KB:
 *                    32 F                                   the frames' four sums, fp64
 *                  + 8 H + 8 (H / 2 + 2)                    the two twiddle tables
 *                  + 2 * 4 * even((F - 1) hop + n_fft)      the staged span of x and of y
 *                  + 8 F (H + H / 8)                        one exchange buffer per wave, a pad entry after every 8
 *                n_fft = 2048 keeps F = 4 up to hop 676 and F >= 2 at every hop; n_fft = 1024 keeps F = 8 up to hop 543; 512 and 256 keep
 *                F = 8 at every hop.
 *
 * Same conventions as vtts_stoi.h (vtts_status and vtts_last_error() of vtts_hifigan.h): plain pointers and sizes, 0 or a negative
 * vtts_status, device memory owned by the caller, asynchronous on the given stream.
 */
#ifndef VTTS_SPECTRAL_H
#define VTTS_SPECTRAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vtts_spectral vtts_spectral; /* opaque */

typedef struct vtts_spectral_cfg {
    int32_t n_fft; /* 256, 512, 1024 or 2048 */
    int32_t win;   /* hop <= win <= n_fft */
    int32_t hop;   /* >= 1 */
} vtts_spectral_cfg;

/* The longest row, in samples (17 minutes at 16 kHz). */
#define VTTS_SPECTRAL_MAX_SAMPLES 16777216
/* The most frames (= waves) one workgroup covers at n_fft = 2048, and at the shorter lengths. */
#define VTTS_SPECTRAL_MAX_FRAMES_PER_BLOCK_2048 4
#define VTTS_SPECTRAL_MAX_FRAMES_PER_BLOCK 8
/* LDS one workgroup may take, in bytes. */
#define VTTS_SPECTRAL_LDS_BUDGET 81920
/* Rows whose lengths one launch carries as kernel arguments. */
#define VTTS_SPECTRAL_ROWS_PER_LAUNCH 128

/* Touches no HIP call: works on a host without a GPU. */
int vtts_spectral_create(const vtts_spectral_cfg* cfg, int device, vtts_spectral** out);
void vtts_spectral_destroy(vtts_spectral* h);

/* The n_fft window values the kernels use (zeros around the centred Hann), to host memory (for oracles). */
int vtts_spectral_window(const vtts_spectral* h, float* host_out);

/* F of this resolution. */
int vtts_spectral_frames_per_block(const vtts_spectral* h, int* frames);

/* T = 1 + n_samples / hop; n_fft / 2 + 1 <= n_samples <= VTTS_SPECTRAL_MAX_SAMPLES, else VTTS_ERR_SHAPE. */
int vtts_spectral_num_frames(const vtts_spectral* h, int64_t n_samples, int64_t* frames);

/* The tables: pack() uploads them into the caller's blob (256-byte aligned, >= packed_bytes) and waits; bind_packed() adopts a blob that
 * another handle of the same configuration packed. */
int vtts_spectral_packed_bytes(const vtts_spectral* h, size_t* bytes);
int vtts_spectral_pack(vtts_spectral* h, void* dev_blob, size_t blob_bytes, void* stream);
int vtts_spectral_bind_packed(vtts_spectral* h, void* dev_blob, size_t blob_bytes);

/* Scratch bytes forward() needs for N rows whose longest has S samples: double [N][ceil(num_frames(S) / F)][4], the partials (A, B, C, D). */
int vtts_spectral_workspace_bytes(const vtts_spectral* h, int N, int64_t S, size_t* bytes);

/*
 *   ref_dev, test_dev  [N, S_stride] samples of `dtype` (VTTS_AUDIO_F32 = 0 | VTTS_AUDIO_PCM16 = 1 of vtts_audio.h), device memory: x and y
 *   lengths            [N] HOST int32 sample counts of both, n_fft / 2 + 1 <= lengths[b] <= S_stride; NULL = every row has S_stride.  Read
 *                      before the call returns.
 *   sc_dev, logmag_dev, lsd_dev   [N] fp64 each
 *   n_frames_dev       [N] int32
 *   mags_dev           NULL, or [N, 2, T_stride, n_fft / 2 + 1] fp32 with T_stride >= num_frames(longest row)
 *   workspace          >= workspace_bytes(N, longest row) bytes, 8-byte aligned
 * Every per-row offset is 64-bit.  VTTS_ERR_STATE before pack() / bind_packed().
 */
int vtts_spectral_forward(vtts_spectral* h, const void* ref_dev, const void* test_dev, int dtype, int N, int64_t S_stride, const int32_t* lengths,
                          double* sc_dev, double* logmag_dev, double* lsd_dev, int32_t* n_frames_dev, float* mags_dev, int64_t T_stride,
                          void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTTS_SPECTRAL_H */
