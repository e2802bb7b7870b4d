/*
 * vtts_stoi.h — C ABI of the batched intelligibility meter: STOI (Taal, Hendriks, Heusdens, Jensen 2011) and its extended form ESTOI
 * (Jensen, Taal 2016) of a processed waveform y against the clean waveform x it is sample-aligned with.  The reference has no such stage;
 * the project has exactly the pair the figure needs: generator(MelFilter(y))[:, :S] against y.
 *
 * The algorithm is defined at 10 kHz.  This side is rate-agnostic and counts samples (viettts_amd/stoi.py converts to 10 kHz first).  For row
 * b of x[N, S_stride] and y[N, S_stride] with S = lengths[b] samples each (VTTS_AUDIO_PCM16 samples are multiplied by 2^-15 on load, exact):
 *
 *   constants    FRAME = 256, HOP = 128, NFFT = 512, BANDS = 15, SEG = 30, clip factor c = 1 + 10^(15 / 20), eps = 2^-52.
 *                Window w[r] = 0.5 - 0.5 cos(2 pi (r + 1) / 257), r = 0 .. 255 (hanning(258)[1:-1]), computed by the handle in double and
 *                rounded ONCE to fp32 (vtts_stoi_window()).
 *                Band j sums bins lo[j] .. lo[j + 1] - 1 of the 512-point DFT,
 *                    lo = 7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219:
 *                the nearest bins to 150 * 2^((2 j -+ 1) / 6) Hz on the grid f = 10000 k / 512 (third octaves from 150 Hz).
 *   A. candidate frames
 *                K = ceil((S - 256) / 128) for S > 256, else 0; frame k starts at 128 k (the last <= 128 samples may go unused).
 *                p_k[r] = fl32(x[128 k + r] * w[r]), q_k[r] likewise from y.  Energy e_k = sum_r p_k[r]^2 in fp64 (each square is exact) in
 *                THIS order: s_l = ((p[l]^2 + p[l + 64]^2) + p[l + 128]^2) + p[l + 192]^2 for l = 0 .. 63, then five halvings
 *                s_l <- s_l + s_(l + h) for l < h, h = 32, 16, 8, 4, 2, 1; e_k = s_0.
 *                Frame k is KEPT iff e_k > 1e-4 * e_max (one fp64 multiply; e_max = the row's largest e_k): the 40 dB silent-frame rule,
 *                decided on the clean signal alone.  A row with e_max = 0 keeps nothing.  Kept frames k_0 < ... < k_(Kk - 1).
 *   B. analysis frames, straight from the kept list (the overlap-added "silence-removed signal" is never materialised)
 *                T = max(0, Kk - 1).  u_t[r] = p_(k_t)[r] + p_(k_(t-1))[r + 128] for r < 128 (the second term absent at t = 0) and
 *                u_t[r] = p_(k_t)[r] + p_(k_(t+1))[r - 128] for r >= 128; v_t = fl32(u_t * w), zero-padded to 512; P[f] = re^2 + im^2 of
 *                its DFT; X[j, t] = sqrt(sum of P over band j).  Y[j, t] the same from q, with the SAME kept list.  This equals windowing,
 *                overlap-adding at hop 128 and re-framing with range(0, len - 256, 128).
 *   C. segments  M = max(0, T - 29); segment m covers frames m .. m + 29 (n = 0 .. 29).
 *                STOI   per band j: alpha = ||X_j|| / (||Y_j|| + eps); Y' = min(alpha Y_j, c X_j); from X_j and from Y' subtract the mean
 *                       and divide by (the norm + eps); d_m = (1 / 15) sum_j sum_n Xn Y'n.
 *                ESTOI  mean- and norm-normalise the rows (a band over its 30 frames), then the columns (a frame over its 15 bands) of both
 *                       the same way (each division by norm + eps); d_m = (1 / 30) sum_j sum_n Xn Yn.
 *                d = mean_m d_m.
 *   outputs      stoi[N], estoi[N] fp32: NaN where M = 0 (never the 1e-5 placeholder some host packages return); n_frames = K, n_kept = Kk,
 *                n_segments = M as int32; optionally the per-segment series [N, M_stride] of each figure, NaN past M_b; optionally the band
 *                magnitudes [N, 2, 15, T_stride] fp32 (X then Y; entries past T_b are not written).
 *   precision    the window products, the overlap sums and the DFT are fp32; P is summed over a band in fp64 in ascending bin order, and X, Y
 *                are the fp64 square roots rounded to fp32.  Stage C is fp64 throughout and every sum of it is sequential in ascending index
 *                from 0: over the 30 frames of a band, over the 15 bands of a frame, over the 15 band terms and the 30 frame terms of a
 *                segment.  A normalised product is formed as one quotient, sum(a b) / ((||a|| + eps) (||b|| + eps)), which differs from the
 *                product of the two normalised vectors by fp64 rounding alone.
 *                d = (sum over lanes l of (d_l + d_(l + 64) + ... in ascending m), by the six halvings h = 32 .. 1) / M.
 *   invariance   every grid of the kernels is anchored at the row's own first sample: a row gives the same bits alone, in a ragged batch,
 *                at any S_stride, and as fp32 or as the PCM16 of the same values.
 *
 * Same conventions as vtts_loudness.h (vtts_status and vtts_last_error() of vtts_hifigan.h): plain pointers and sizes, 0 or a negative
 * vtts_status, device memory owned by the caller, asynchronous on the given stream.  The handle owns nothing on the device: its tables (the
 * window and a quarter turn of twiddles, 512 floats, computed in double on the host) travel as kernel arguments.
 */
#ifndef VTTS_STOI_H
#define VTTS_STOI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vtts_stoi vtts_stoi; /* opaque */

#define VTTS_STOI_FRAME 256
#define VTTS_STOI_HOP 128
#define VTTS_STOI_BANDS 15
#define VTTS_STOI_SEG 30
/* The longest row, in samples (28 minutes at 10 kHz). */
#define VTTS_STOI_MAX_SAMPLES 16777216
/* Frames (= waves) one workgroup of the energy and the spectrum kernels covers. */
#define VTTS_STOI_FRAMES_PER_BLOCK 8

/* Touches no HIP call: works on a host without a GPU. */
int vtts_stoi_create(int device, vtts_stoi** out);
void vtts_stoi_destroy(vtts_stoi* h);

/* The 256 window values the kernels use, to host memory (for oracles). */
int vtts_stoi_window(const vtts_stoi* h, float* host_out);

/* K = n_samples > 256 ? ceil((n_samples - 256) / 128) : 0; 0 <= n_samples <= VTTS_STOI_MAX_SAMPLES. */
int vtts_stoi_num_frames(const vtts_stoi* h, int64_t n_samples, int64_t* frames);

/*
 * Scratch bytes forward() needs for N rows whose longest has S samples.  With Kmax = num_frames(S), Tmax = max(0, Kmax - 1),
 * Mmax = max(0, Tmax - 29) and every part's size rounded up to 8 bytes, the workspace holds, in this order:
 *     kept   int32  [N][Kmax]             the kept frames' indices k_0 .. k_(Kk - 1) of each row in ascending order, then -1 up to Kmax
 *     energy double [N][Kmax]             e_k
 *     dseg   double [N][2][Mmax]          d_m of STOI, then of ESTOI
 *     mags   float  [N][2][15][Tmax]      X, then Y (used when forward() is given no mags_dev)
 * `kept` and `energy` are valid once forward()'s work on the stream has finished: that is how a caller reads the keep mask.
 */
int vtts_stoi_workspace_bytes(const vtts_stoi* h, int N, int64_t S, size_t* bytes);

/*
 *   clean_dev, processed_dev   [N, S_stride] samples of `dtype` (VTTS_AUDIO_F32 = 0 | VTTS_AUDIO_PCM16 = 1 of vtts_audio.h), device memory
 *   lengths            [N] HOST int32 sample counts of both, 0 <= lengths[b] <= S_stride; NULL = every row has S_stride.  Read before the call
 *                      returns.
 *   stoi_dev, estoi_dev                        [N] fp32 each
 *   n_frames_dev, n_kept_dev, n_segments_dev   [N] int32 each
 *   stoi_series_dev, estoi_series_dev   both NULL, or both [N, M_stride] fp32 with M_stride >= max(0, num_frames(longest row) - 30)
 *   mags_dev           NULL, or [N, 2, 15, T_stride] fp32 with T_stride >= max(0, num_frames(longest row) - 1)
 *   workspace          >= workspace_bytes(N, longest row) bytes, 8-byte aligned
 * Every per-row offset is 64-bit.
 */
int vtts_stoi_forward(vtts_stoi* h, const void* clean_dev, const void* processed_dev, int dtype, int N, int64_t S_stride, const int32_t* lengths,
                      float* stoi_dev, float* estoi_dev, int32_t* n_frames_dev, int32_t* n_kept_dev, int32_t* n_segments_dev,
                      float* stoi_series_dev, float* estoi_series_dev, int64_t M_stride, float* mags_dev, int64_t T_stride, void* workspace,
                      size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTTS_STOI_H */
