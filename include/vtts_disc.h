/*
 * vtts_disc.h — C ABI of the HiFi-GAN discriminators and losses as a forward-only scoring pass
 * (NTT123/vietTTS vietTTS/hifigan/torch_model.py: MultiPeriodDiscriminator, MultiScaleDiscriminator, feature_loss,
 * generator_loss, discriminator_loss).  No gradients, no optimiser.
 *
 * The architecture is the reference's, which hard-codes it:
 *   MPD  periods 2, 3, 5, 7, 11: reflect-pad T up to a multiple of p, view as [N, 1, T/p, p]; Conv2d (5,1) stride (3,1) pad (2,0)
 *        1 -> 32 -> 128 -> 512 -> 1024, Conv2d (5,1) stride 1 1024 -> 1024, conv_post (3,1) 1024 -> 1; LeakyReLU 0.1 after all but conv_post.
 *   MSD  three scales, scale i > 0 on AvgPool1d(4, 2, padding=2) of the previous scale's input (L -> L/2 + 1); Conv1d
 *        1 -> 128 k15 | 128 -> 128 k41 s2 g4 | 128 -> 256 k41 s2 g16 | 256 -> 512 k41 s4 g16 | 512 -> 1024 k41 s4 g16 |
 *        1024 -> 1024 k41 g16 | 1024 -> 1024 k5 | conv_post 1024 -> 1 k3.
 * 54 convolutions, 54 feature maps (5 x 6 + 3 x 8), 8 discriminators.  Discriminator d = 0..4 is MPD period 2..11, d = 5..7 is MSD
 * scale 0..2.  Feature map indices run discriminator by discriminator, layer by layer, conv_post's output last.
 *
 * Same conventions as vtts_hifigan.h (whose vtts_status / vtts_last_error() this header uses): plain pointers and sizes, 0 or a
 * negative vtts_status, device memory owned by the caller, asynchronous on the given stream.  All arithmetic is fp32
 * (v_mfma_f32_32x32x2_f32, v_mfma_f32_16x16x4_f32 for the 16-channel groups).  Every row's results are bit for bit what the row gives
 * alone, whatever the batch.
 */
#ifndef VTTS_DISC_H
#define VTTS_DISC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vtts_disc vtts_disc; /* opaque */

#define VTTS_DISC_NUM_CONVS 54
#define VTTS_DISC_NUM_FMAPS 54
#define VTTS_DISC_NUM_DISCS 8
#define VTTS_DISC_MIN_SAMPLES 11 /* the reflect pad of period 11 needs T >= 11 */

/*
 * Layout of losses()'s output, in floats.  Entries 0 .. VTTS_DISC_LOSS_RESULTS - 1 are results; the rest of the
 * VTTS_DISC_LOSS_FLOATS-float buffer is the first reduction stage's scratch (fixed-size, so the same inputs give the same bits).
 *   [  0 ..  53]  mean |r - g| of feature map i
 *   [ 54 ..  61]  mean (1 - d_r)^2 of discriminator d                (discriminator_loss's r_losses)
 *   [ 62 ..  69]  mean d_g^2                                         (discriminator_loss's g_losses)
 *   [ 70 ..  77]  mean (1 - d_g)^2                                   (generator_loss's gen_losses)
 *   [ 78 ] feature_loss(MPD) = 2 * sum of entries 0 .. 29    [ 79 ] feature_loss(MSD) = 2 * sum of entries 30 .. 53
 *   [ 80 ] discriminator_loss(MPD) = sum over d < 5 of (r + g)       [ 81 ] discriminator_loss(MSD), d = 5 .. 7
 *   [ 82 ] generator_loss(MPD)                                       [ 83 ] generator_loss(MSD)
 *   [ 84 ] = [78] + [79]     [ 85 ] = [80] + [81]     [ 86 ] = [82] + [83]
 * Sums run in ascending index order, as the reference's loops do.
 */
#define VTTS_DISC_LOSS_FMAP 0
#define VTTS_DISC_LOSS_REAL 54
#define VTTS_DISC_LOSS_FAKE 62
#define VTTS_DISC_LOSS_GEN 70
#define VTTS_DISC_LOSS_TOTALS 78
#define VTTS_DISC_LOSS_RESULTS 128
#define VTTS_DISC_LOSS_PARTIALS 64 /* first-stage workgroups per reduced tensor */
#define VTTS_DISC_LOSS_FLOATS (VTTS_DISC_LOSS_RESULTS + 2 * (VTTS_DISC_NUM_FMAPS + 3 * VTTS_DISC_NUM_DISCS) * VTTS_DISC_LOSS_PARTIALS)

/* Touches no HIP call: works on a host without a GPU. */
int vtts_disc_create(int device, vtts_disc** out);
void vtts_disc_destroy(vtts_disc* h);

/*
 * 108 parameters: for convolution c = 0 .. 53 (in feature-map order) parameter 2c is its EFFECTIVE weight (weight norm or
 * spectral norm already folded) in torch layout [Cout, Cin / groups, k] (a Conv2d's trailing 1 dropped), which = "w", and 2c + 1
 * its bias [Cout], which = "b".  Keys are the torch module paths: "mpd.discriminators.0.convs.3", "msd.discriminators.2.conv_post".
 */
int vtts_disc_num_params(const vtts_disc* h, int* n);
int vtts_disc_param_info(const vtts_disc* h, int i, const char** key, const char** which, int64_t shape[3], int* ndim);
int vtts_disc_set_param(vtts_disc* h, const char* key, const char* which, const float* host, const int64_t* shape, int ndim);

/* The weights in MFMA A-fragment order plus biases as one device blob, caller-owned and 256-B aligned: pack() copies it on the
 * stream and waits (VTTS_ERR_MISSING while a parameter was never set); bind_packed() adopts a blob another handle packed.
 * blob_bytes may exceed packed_bytes(), as for every other handle; a smaller blob is VTTS_ERR_NOMEM. */
int vtts_disc_packed_bytes(const vtts_disc* h, size_t* bytes);
int vtts_disc_pack(vtts_disc* h, void* dev_blob, size_t blob_bytes, void* stream);
int vtts_disc_bind_packed(vtts_disc* h, void* dev_blob, size_t blob_bytes);

/* Scratch bytes forward() needs for N rows of T samples (0: every intermediate is a feature map). */
int vtts_disc_workspace_bytes(const vtts_disc* h, int N, int64_t T, size_t* bytes);

/*
 * Feature map i of a call with N rows of T samples is the contiguous array [N, C, L, columns] starting `offset` floats into the
 * feature-map buffer (columns = the period for MPD, 1 for MSD).  offset + N * C * L * columns of the last map is the buffer's size.
 * The offsets are multiples of 64 floats.
 */
int vtts_disc_num_fmaps(const vtts_disc* h, int* n);
int vtts_disc_fmap_info(const vtts_disc* h, int i, int N, int64_t T, int64_t* C_, int64_t* L, int64_t* columns, int64_t* offset);

/*
 *   y_dev      [N, T] fp32 waveforms, all rows of length T >= VTTS_DISC_MIN_SAMPLES (VTTS_ERR_SHAPE below)
 *   fmaps_dev  the feature-map buffer (fmap_info); every map is written once and read by the next layer
 *   scores_dev the eight discriminators' flattened outputs one after the other: discriminator d's [N, L_d * columns_d] block starts
 *              at the sum of N * L_e * columns_e over e < d, where L, columns are those of its conv_post feature map
 */
int vtts_disc_forward(vtts_disc* h, const float* y_dev, int N, int64_t T, float* fmaps_dev, float* scores_dev, void* workspace, void* stream);

/*
 * Every loss of a forward() call with N = 2 B rows, rows 0 .. B - 1 real and rows B .. 2 B - 1 generated, in one reduction pass:
 * out_dev [VTTS_DISC_LOSS_FLOATS], layout above.  Two fixed-order stages, no float atomics.
 */
int vtts_disc_losses(vtts_disc* h, const float* fmaps_dev, const float* scores_dev, int B, int64_t T, float* out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTTS_DISC_H */
