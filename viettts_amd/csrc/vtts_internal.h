// Internal declarations shared by the engine and the kernel translation units.
// gfx950 only: wave64, MFMA, 160 KiB LDS.  No portability layer on purpose.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/vtts_audio.h"
#include "../../include/vtts_hifigan.h"

#define VTTS_API extern "C" __attribute__((visibility("default")))

namespace vtts {

// engine.hip: record the calling thread's last error message (vtts_last_error(); printf-style, 511 characters at most) and return `code`
int failf(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                                          \
    do {                                                                                                       \
        hipError_t _e = (expr);                                                                                \
        if (_e != hipSuccess)                                                                                  \
            return vtts::failf(VTTS_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// The one rule for a caller's packed blob, behind every handle's pack() and bind_packed(): `bytes` at `dev_blob` must hold the handle's `need`
// packed bytes (more is fine) and start on a 256-byte boundary (the kernels read it as float4 / uint4).  Host arithmetic only.
inline int check_blob(const void* dev_blob, size_t bytes, size_t need) {
    if (!dev_blob) return failf(VTTS_ERR_INVALID, "null argument");
    if (bytes < need) return failf(VTTS_ERR_NOMEM, "blob too small: %zu < %zu bytes", bytes, need);
    if (reinterpret_cast<uintptr_t>(dev_blob) % 256) return failf(VTTS_ERR_INVALID, "blob must be 256-byte aligned");
    return VTTS_OK;
}
// pack()'s upload: `bytes` of `host` into the checked blob on `s`, waited for (the host image may die at the caller's return)
inline int upload_blob(void* dev_blob, const void* host, size_t bytes, hipStream_t s, const char* what) {
    hipError_t e = hipMemcpyAsync(dev_blob, host, bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return failf(VTTS_ERR_HIP, "copying %s failed: %s", what, hipGetErrorString(e));
    return VTTS_OK;
}

// The one rule for a batch of waveform rows (the limiter's and the loudness meter's calls): fp32 or PCM16, N >= 1, a pitch that leaves `margin`
// samples (the stage's tile) below 2^31, every length within the pitch.  *longest = the longest row.  Host only; launch_rows.h cuts the call up.
inline int check_rows(const char* what, const void* wav, int dtype, int N, int64_t S_stride, const int32_t* lengths, int margin, int64_t* longest) {
    if (!wav) return failf(VTTS_ERR_INVALID, "null argument");
    if (dtype != VTTS_AUDIO_F32 && dtype != VTTS_AUDIO_PCM16) return failf(VTTS_ERR_INVALID, "%s: dtype must be VTTS_AUDIO_F32 or VTTS_AUDIO_PCM16 (got %d)", what, dtype);
    if (N <= 0) return failf(VTTS_ERR_INVALID, "%s: N must be positive (got %d)", what, N);
    if (S_stride < 0 || S_stride > 0x7fffffff - margin)
        return failf(VTTS_ERR_SHAPE, "%s: S_stride must be in 0 .. 2^31 - 1 - %d (got %lld)", what, margin, (long long)S_stride);
    int64_t m = 0;
    for (int b = 0; b < N; ++b) {
        const int64_t len = lengths ? lengths[b] : S_stride;
        if (len < 0 || len > S_stride)
            return failf(VTTS_ERR_SHAPE, "%s: lengths[%d] = %lld is outside 0 .. S_stride = %lld", what, b, (long long)len, (long long)S_stride);
        if (len > m) m = len;
    }
    *longest = m;
    return VTTS_OK;
}

// fp32 -> bf16 bits, round-to-nearest-even (what v_cvt_pk_bf16_f32 gives), and back
inline unsigned short f32_to_bf16_rne(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);  // NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}
inline float bf16_to_f32(unsigned short h) {
    const uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
// The split-operand engine's two bf16 terms of a weight, w = hi + lo to 16 significand bits: the host form of bf16_common.h: split2
// (w - float(hi) is exact in fp32)
inline void split_bf16(float w, unsigned short& hi, unsigned short& lo) {
    hi = f32_to_bf16_rne(w);
    lo = f32_to_bf16_rne(w - bf16_to_f32(hi));
}

// hipFuncAttributeMaxDynamicSharedMemorySize is a property of the function ON A DEVICE: a process that drives several GPUs (a
// second Generator on cuda:1 after cuda:0) must set it once per device, not once per process.  `done` = the caller's static
// per-kernel table; devices beyond it just set the attribute on every launch (cheap next to a launch).
struct DynLdsOnce {
    bool done[32] = {};
};
inline hipError_t set_max_dynamic_lds(const void* fn, int bytes, DynLdsOnce& once) {
    int dev = -1;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const bool tracked = dev >= 0 && dev < 32;
    if (tracked && once.done[dev]) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess && tracked) once.done[dev] = true;
    return e;
}

// How a convolution's result is combined with what is already in memory.  This is where
// ResBlock1's residual (model.py:50 `x = xt + x`) and the MRF mean (model.py:115-121
// `xs = rb0; xs += rb1; xs += rb2; x = xs / 3`) are fused into the producing kernel.
//   v = acc + bias;  if (res) v = v + res[i];
//   ACC_STORE : out[i] = v
//   ACC_ADD   : out[i] = out[i] + v
//   ACC_MEAN  : out[i] = (out[i] + v) / div      (true division, as the reference)
enum AccMode : int { ACC_STORE = 0, ACC_ADD = 1, ACC_MEAN = 2 };

struct ConvArgs {
    const float* x;      // input activations
    long x_sb, x_sc, x_st;  // element strides of x: batch, channel, time  (NCW: C*L, L, 1)
    const float* w;      // plain weights, Haiku layout [K][Cin][Cout]  (convT: [K][Cout][Cin])
    const void* wp;      // MFMA-packed weights (or nullptr)
    const float* bias;   // [Cout]
    const float* res;    // optional residual [B][Cout][L] (may alias y) or nullptr
    float* y;            // output [B][Cout][Lout]
    int B, Cin, Cout, K;
    int dil, pad;        // convolution: rate and symmetric zero pad
    int stride, pad_a;   // transposed convolution: stride and left pad of the zero-stuffed input
    int L;               // input length (time)
    int Lout;            // output length
    float slope_in;      // LeakyReLU slope applied to x on load (1.0f = identity)
    int acc_mode;        // AccMode
    float div;           // divisor for ACC_MEAN
    int tanh_out;        // apply tanh to the result (conv_post)
    float* pre_act;      // optional copy of the pre-tanh value (same indexing as y) or nullptr
    int tile_pref;       // MFMA time-tile choice: 0 = by problem size, 1 = wide, 2 = narrow (tests)
    int zrev;            // MFMA kernels: 1 = utterance = gridDim.z - 1 - blockIdx.z (engine.hip: next_zrev)
    // ragged batch (vtts_hifigan_forward_ragged on the fp32 / bf16x3 engines): utterance b's valid INPUT length is lens[b] * len_mul of the L
    // allocated (L stays the row pitch); everything past it reads as the reference's zero padding (model.py:8-10, lax "SAME"), nothing past
    // it is stored, tiles past it exit at once.  nullptr = all L columns valid.  device_common.h: valid_len
    const int* lens;     // [B] mel frames per utterance (device memory)
    int len_mul;         // input columns of this layer per mel frame
};

// ---- generic (any shape) fp32 kernels: kernels_generic.hip -------------------------------
hipError_t launch_conv1d_generic(const ConvArgs& a, hipStream_t s);
hipError_t launch_convT1d_generic(const ConvArgs& a, hipStream_t s);

// ---- fp32 MFMA implicit-GEMM convolution: kernels_f32_mfma.hip ------------------------------
// ResBlock shapes (Cin == Cout in {32,64,128,256}, K in {3,7,11}, channel-major input) and conv_pre
// (80 -> 512, K = 7, time-major input: nwc = true).
bool conv1d_f32_mfma_supported(int Cin, int Cout, int K, int dil, int L, bool nwc);
size_t conv1d_f32_mfma_packed_floats(int Cin, int Cout, int K);
// host-side re-layout: Haiku [K][Cin][Cout] -> MFMA A-fragment order
void conv1d_f32_mfma_pack(const float* w_hk, int Cin, int Cout, int K, float* out);
hipError_t launch_conv1d_f32_mfma(const ConvArgs& a, hipStream_t s);
const char* conv1d_f32_mfma_kernel_name(int C, int K);

// ---- fp32 fused ResBlock1 pair  x' = c2(lrelu(c1(lrelu(x)))) + x  (kernels_f32_pair.hip) ----
// a = c1's ConvArgs (x, wp = c1's packed weights, bias = b1, dil, slope_in, B, L, zrev) with the OUTPUT side filled in (y, res = x,
// acc_mode, div); wp2 / bias2 = c2's.  Bit-identical to launching the two convolutions one after the other.
bool pair_f32_supported(int C, int K, int dil, int L);
hipError_t launch_pair_f32(const ConvArgs& a, const void* wp2, const float* bias2, hipStream_t s);

// ---- split-operand ("bf16x3") fused ResBlock1 pair on the bf16 matrix pipe, fp32 channel-major activations (kernels_x3.hip) ----
// a as for launch_pair_f32 (a.wp unused); w1 / w2 = the two convolutions' packed weights, each [hi fragments][lo fragments] (pair_x3_pack)
bool pair_x3_supported(int C, int K, int dil, int L);
size_t pair_x3_conv_bytes(int C, int K);
void pair_x3_pack(const float* w_hk, int C, int K, unsigned short* out);
hipError_t launch_pair_x3(const ConvArgs& a, const void* w1, const void* w2, const float* bias2, hipStream_t s);
// ... and the four transposed convolutions (polyphase, k = 2 * stride): a.x [B][Cin][L] -> a.y [B][Cout][stride * L], a.wp = convt_x3_pack's output
bool convt_x3_supported(int Cin, int Cout, int K, int stride, int pad_a, int L);
size_t convt_x3_bytes(int Cin, int Cout, int stride);
void convt_x3_pack(const float* w_hk, int Cin, int Cout, int K, int stride, int pad_a, unsigned short* out);
hipError_t launch_convt_x3(const ConvArgs& a, hipStream_t s);
// ... and conv_pre (80 -> 512, k = 7, mel NWC in): a.x [B][L][80] (a.x_sb = the batch stride), a.y [B][512][L], a.wp = conv_pre_x3_pack's output
bool conv_pre_x3_supported(int Cin, int Cout, int K, int dil);
size_t conv_pre_x3_bytes();
void conv_pre_x3_pack(const float* w_hk, unsigned short* out);
hipError_t launch_conv_pre_x3(const ConvArgs& a, hipStream_t s);

// ---- whole ResBlock1 with split operands (kernels_x3_rb.hip): three pairs + the MRF bookkeeping in one launch, bit-identical to three launch_pair_x3 ----
// a = ConvArgs of the ResBlock (x = stage input [B][C][L], y = output with acc_mode / div, Cin = C, K, B, L, lens / len_mul, slope_in, zrev);
// dils = the three rates; w[q] / bias[q] = the six convolutions (c1_0, c2_0, c1_1, ...), weights as pair_x3_pack lays them out
bool resblock_x3_supported(int C, int K, const int* dils, int L);
bool resblock_x3_preferred(int C, int K);
hipError_t launch_resblock_x3(const ConvArgs& a, const int* dils, const void* const* w, const float* const* bias, hipStream_t s);

// ---- fp32 polyphase transposed convolution on MFMA (k == 2*stride) -------------------------
bool convT1d_f32_mfma_supported(int Cin, int Cout, int K, int stride, int pad_a, int L);
size_t convT1d_f32_mfma_packed_floats(int Cin, int Cout, int K);
void convT1d_f32_mfma_pack(const float* w_hk, int Cin, int Cout, int K, int stride, int pad_a, float* out);
hipError_t launch_convT1d_f32_mfma(const ConvArgs& a, hipStream_t s);

// ---- streaming conv_post (32 -> 1, K = 7, fused LeakyReLU + tanh) ----------------------------
bool conv_post_fast_supported(int Cin, int Cout, int K, int L);
hipError_t launch_conv_post_fast(const ConvArgs& a, hipStream_t s);

// =================================================================================================
// bf16 path: kernels_bf16.hip  (channels-last activations, v_mfma_f32_32x32x16_bf16)
// =================================================================================================
enum BClass : int { BCLS_NONE = -1, BCLS_RES256 = 0, BCLS_RES128, BCLS_RES64, BCLS_RES32, BCLS_PRE, BCLS_UP0, BCLS_UP1, BCLS_UP2, BCLS_UP3 };

struct BConvArgs {
    const void* x;        // input activations: bf16 [B][L][x_pitch]  (fp32 for conv_pre)
    const void* wp;       // packed bf16 weights (A-fragment-ordered slabs)
    const float* wf;      // plain fp32 weights (conv_post only)
    const float* bias;    // fp32 [COUTP]
    const void* res;      // optional residual, bf16 [B][L][COUTP], or nullptr
    void* y;              // output bf16 [B][L][COUTP]
    int B, L;             // utterances; rows (time steps) ALLOCATED per utterance in x / y
    const int* lens;      // ragged batch: valid mel frames per utterance (device, [B]) or nullptr = all L rows valid
    int len_mul;          // rows of this layer per mel frame (valid rows of utterance b = lens[b] * len_mul)
    int x_pitch;          // elements per input row in global memory
    int cin_real;         // valid input channels (conv_pre: 80)
    int dil, pad;
    int convt_halves;     // conv_bf16_k on a transposed convolution's 3-tap form: skip each row half's all-zero tap
    int dils[3];          // whole-ResBlock kernel: the three pairs' rates
    float slope_in;       // LeakyReLU applied to the input while staging (1 = producer already did it)
    float slope_out;      // LeakyReLU applied to the stored output (the consumer's activation), 1 = none
    int acc_add;          // y = y + v   (MRF accumulate)
    int tile_pref;        // fused-pair tile width: 0 = by launch size, 1 = wide, 2 = narrow (option "tiles"; tests run both on short inputs)
    float div;            // then the MRF mean v / div as v * (1 / div) (bf16_common.h: mrf_recip), 1 = none
    int zrev;             // 1 = utterance = gridDim.z - 1 - blockIdx.z: the launch walks the batch backwards (engine.hip: next_zrev)
    unsigned long long* dbg;  // kernel-development builds only (-DVTTS_TIMELINE): per-workgroup s_memtime stamps; else unused
    // stage-4 tail fused into the last pair launch (kernels_bf16_rbg.hip: GTail): conv_post's plain fp32 weights [7][32] and bias, the waveform
    // [B][L] fp32 (pitch = this layer's L); nullptr = a plain pair launch
    float* tail_wav;
    const float* tail_wf;
    const float* tail_bias;
    // the next stage's transposed convolution fused into the stage-ending pair launch (kernels_bf16_rbg.hip: GUp): its weights in convt_g_pack_geom's
    // order, its bias [C] and its output [B][L][C] (= the next stage's [B][2 L][C / 2]); nullptr = a plain pair launch.  y is then only read.
    const void* up_wp;
    const float* up_bias;
    void* up_y;
};

struct BPackGeom { int cinp, ckc, coutp, ks, mt, tg; };

hipError_t launch_conv_bf16(int cls, int K, const BConvArgs& a, hipStream_t s);
BPackGeom bf16_pack_geom(int cls, int K);
const char* bf16_kernel_name(int cls, int K);
inline size_t bf16_packed_bytes(const BPackGeom& g) {
    const int ncc = g.cinp / g.ckc, nsl = (g.ks + g.tg - 1) / g.tg;
    return (size_t)(g.coutp / g.mt) * ncc * nsl * ((size_t)g.mt * g.tg * g.ckc * 2);
}
void bf16_pack(const float* Wc, int cin_real, const BPackGeom& g, unsigned short* out);
// fused ResBlock1 pair (c1 -> lrelu -> c2 -> + x): kernels_bf16_rbg.hip, weights straight from L2 into register rings, no workgroup
// sync in the main loops.  a.wp = [c1 fragments][c2 fragments] (each packed with pair_g_pack_geom), a.bias = [b1 (C)][b2 (C)],
// a.x = raw pair input (also the residual), a.dil/a.pad = c1's rate / pad.
bool pair_bf16_supported(int C, int K, int dil);
bool pair_tail_bf16_supported(int C, int K, int post_cin, int post_cout, int post_k);
// where a pair launch (accumulate, mean, LeakyReLU epilogue) can carry the stride-2 transposed convolution that follows its stage (a.up_y): BCLS_UP2 / BCLS_UP3
bool pair_up_bf16_supported(int C, int K, int up_cls, int up_cin, int up_cout, int up_k, int up_stride);
hipError_t launch_pair_g_bf16(int C, int K, const BConvArgs& a, hipStream_t s);
BPackGeom pair_g_pack_geom(int C, int K);
// resblock_pair_g_bf16_k's own weights: pair_g_pack_geom's order on the classes whose loops run 32 x 32 x 16 blocks, the 16 x 16 x 32 fragment order
// (pair_g_pack16, same byte count) on those that run 16-blocks (pair_g_mfma_blk).  The split-operand kernels and the whole-ResBlock blob keep pair_g_pack_geom.
int pair_g_mfma_blk(int C, int K);
// The 16 x 16 x 32 fragment order of one convolution: [q = tap*(C/32) + ks][mblk16][lane][8] bf16 with  co = 16 mblk + (lane & 15),
// ci = 32 ks + 8 (lane >> 4) + e.  Wc: [K][C][C] fp32 (Haiku layout: tap, input channel, output channel).  K * C * C * 2 bytes, as pair_g_pack_geom's
// order (tools/check_pair_pack16_host.cpp checks both, stand-alone and under the sanitizers).
inline size_t pair_g_pack16_bytes(int C, int K) { return (size_t)K * (C / 32) * (C / 16) * 64 * 8 * sizeof(unsigned short); }
inline void pair_g_pack16(const float* Wc, int C, int K, unsigned short* out) {
    size_t o = 0;
    for (int tap = 0; tap < K; ++tap)
        for (int ks = 0; ks < C / 32; ++ks)
            for (int mblk = 0; mblk < C / 16; ++mblk)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 8; ++e) {
                        const int ci = 32 * ks + 8 * (lane >> 4) + e, co = 16 * mblk + (lane & 15);
                        out[o++] = f32_to_bf16_rne(Wc[((size_t)tap * C + ci) * C + co]);
                    }
}
void pair_g_pack(const float* Wc, int C, int K, unsigned short* out);
const char* pair_g_kernel_name(int C, int K);
// whole ResBlock1 in one kernel (kernels_bf16_rbk.hip): C = 32 (k = 3, 7, 11), C = 64 / 128 (k = 3)
bool resblock_bf16_supported(int C, int K, const int* dils);
bool resblock_bf16_preferred(int C, int K);
hipError_t launch_resblock_bf16(int C, int K, const BConvArgs& a, hipStream_t s);
// the four transposed convolutions on the register-streamed structure (kernels_bf16_up.hip): cls = BCLS_UP0..3,
// a.wp = the 3-tap polyphase form's weights packed with convt_g_pack_geom(cls) (bf16_pack)
hipError_t launch_convt_g_bf16(int cls, const BConvArgs& a, hipStream_t s);
BPackGeom convt_g_pack_geom(int cls);
hipError_t launch_conv_post_bf16(const BConvArgs& a, float* wav, float* pre_act, hipStream_t s);
hipError_t launch_bf16_to_f32(const void* in, float* out, size_t n, hipStream_t s);
hipError_t launch_f32_to_bf16(const float* in, void* out, size_t n, hipStream_t s);


// ---- the NAT acoustic decoder's frame loop as one resident kernel for 1 <= B <= 4 sentences (nat_resident.hip; option "resident" of vtts_nat.h) ----
// Built for the reference's decoder (decoder_dim 512, prenet_dim 256: the recurrent weights' share per thread is a compile-time register array).
constexpr int NAT_RES_H = 512, NAT_RES_PN = 256, NAT_RES_MELMAX = 128;
constexpr int NAT_RES_XCH_ELEMS = NAT_RES_MELMAX + 2 * NAT_RES_PN + 2 * NAT_RES_H;  // [mel | p1 | p | h1 | h2], 4 sentences per element
struct NatResidentArgs {
    const float* w1;   // "lstm/linear" w from Haiku row E on: [PN + H][4H]
    const float* w2;   // "lstm_1/linear" w from Haiku row E on: [PN + 2H][4H]
    const float* wp;   // "linear" w [2H][MEL], bp its bias
    const float* bp;
    const float* f1;   // "linear_1" w [MEL][PN]
    const float* f2;   // "linear_2" w [PN][PN]
    const float* G1;   // hoisted gates [B][Fmax][4H] in the step kernel's accumulator order, all frames
    const float* G2;
    const int* nframes;
    const unsigned char* keep;  // [B][Fmax][2][PN] or nullptr
    float* mel0;       // [B][Fmax][MEL], cleared by the caller
    float* xch;        // [NAT_RES_XCH_ELEMS][4] exchange buffer
    unsigned* sync;    // [0] arrivals, [1] abort word; 8-byte aligned, zeroed on the stream before the launch
    unsigned long long* timeline;  // -DVTTS_TIMELINE builds: 10 phase clocks of workgroup 0 (wall_clock64 ticks); unused otherwise
    int Fmax, MEL;
};
// cooperative launch on `grid` in {64, 128, 256} workgroups; the runtime's error (hipErrorCooperativeLaunchTooLarge ...) is returned as it is
hipError_t launch_nat_dec_resident(const NatResidentArgs& a, int B, int grid, hipStream_t s);

}  // namespace vtts
