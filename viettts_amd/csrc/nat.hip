// NAT duration and acoustic models on MI355X behind the C ABI of include/vtts_nat.h.
//
// Reference: vietTTS/nat/model.py — TokenEncoder (:9-50: Embed, 3 x [Conv1D(k=3, SAME) + BatchNorm(eval) + ReLU],
// forward LSTM, backward LSTM) and DurationModel (:53-70: Linear -> gelu -> Linear(1) -> softplus), called with batch 1
// by text2mel.py:22-34.  All arithmetic fp32 (the reference's dtype); one sentence per workgroup row, rows independent.
//
// This is a latency path (a sentence is ~100 tokens x 256 channels), not an MFMA path: the recurrence is sequential in
// time and each step is a [1 x 512] x [512 x 1024] product.  Mapping:
//   * front end: one kernel per layer; a workgroup owns TL time steps x all D output channels of one sentence, the
//     (TL + 2) input rows staged in LDS, weights read coalesced along the output channel;
//   * LSTM: one persistent workgroup per (sentence, direction), one thread per gate column (4D = 1024 threads); per
//     step every thread walks its column of the [2D x 4D] weight matrix (coalesced across threads, L2-resident: all
//     workgroups read the same 2 MB), [x_t ; h] broadcast from LDS, cell state in registers of the first D threads;
//   * head: Linear(2D -> D) + tanh-form gelu + Linear(D -> 1) + softplus per token, block reduction for the last dot.
// Acoustic model (model.py:73-151, inference path): the same TokenEncoder, Gaussian upsampling to frames (one block per
// frame), the autoregressive decoder as one launch per layer per frame over ALL sentences of the batch (two LSTM-512 with
// skip connections on the fp32 matrix cores, cell update in registers; mel projection + next frame's prenet), then the
// 5-layer postnet as fp32 MFMA convolutions.
// The prenet's always-on dropout (model.py:95-100) takes explicit keep masks, which vtts_nat_acoustic_keep_masks can draw on
// the device with jax.random's cipher (Threefry-2x32-20) from per-sentence seeds, and vtts_nat_acoustic_keep_masks_haiku as the
// reference itself draws them from the checkpoint's rng (classic jax.random layout + Haiku's key chain, restated in round 2).
#include "../../include/vtts_nat.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/vtts_hifigan.h"
#include "bf16_common.h"
#include "nat_model.h"
#include "vtts_internal.h"

using namespace vtts;

struct vtts_nat_duration : NatModel {
    vtts_nat_duration_cfg cfg;
};
struct vtts_nat_acoustic : NatModel {
    vtts_nat_acoustic_cfg cfg;
    int x3 = 0;  // option "bf16x3": LSTM steps, gate GEMM and postnet as three bf16 x bf16 terms per product on the bf16 matrix pipe
    // forward_groups(): the postnet of a group of rows runs on `side` as soon as the decoder has produced the group's last frame
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_gates = nullptr;
    std::vector<hipEvent_t> ev_dec, ev_done;  // per group: decoder frames complete (recorded on the caller's stream) / mel rows complete (on `side`)
    int groups_valid = 0;
    // option "resident": the decoder's frame loop of a call with 1 <= B <= 4 as one resident kernel (nat_resident.hip)
    int resident = 0, resident_grid = 0, resident_used = 0;
    int cu_count = 0;               // of the device the first forward() ran on
    unsigned* res_sync = nullptr;   // [arrivals | abort word] of the last resident launch, in that call's workspace
    // option "stage_times": timing events on the caller's stream in front of the gate GEMM, the decoder loop, the postnet, and behind it
    int stage_times = 0, stage_valid = 0;
    hipEvent_t ev_stage[4] = {nullptr, nullptr, nullptr, nullptr};
    // stream_begin() .. stream_end(): the caller's arrays and dimensions, how far the decoder has run (cursor) and how far the mel is final (finished)
    struct Session {
        bool open = false;
        const int32_t *lengths = nullptr, *nframes = nullptr;
        const float* durations = nullptr;
        const uint8_t* keep = nullptr;
        float* mel = nullptr;
        void* workspace = nullptr;
        size_t workspace_bytes = 0;
        int B = 0, Lmax = 0, Fmax = 0, max_window = 0, x3 = 0, cursor = 0, finished = 0;
    } ss;
    // pool_open() .. pool_close(): the caller's arrays and dimensions, the tick the next pool_decode() starts at, and the host's mirror of every slot
    struct Pool {
        bool open = false;
        const uint8_t* keep = nullptr;
        float* mel = nullptr;
        void* workspace = nullptr;
        size_t workspace_bytes = 0;
        int slots = 0, Lmax = 0, Fmax = 0, max_window = 0, x3 = 0, tick = 0;
        struct Slot {
            bool busy = false;
            int start = 0, nframes = 0, finished = 0;  // admitted at tick `start`; the mel is final below `finished`
        };
        std::vector<Slot> slot;
        int cursor(int i) const { return std::clamp(tick - slot[i].start, 0, slot[i].nframes); }  // frames of slot i the enqueued ticks decode
    } pool;
    ~vtts_nat_acoustic() {
        for (hipEvent_t e : ev_dec) (void)hipEventDestroy(e);
        for (hipEvent_t e : ev_done) (void)hipEventDestroy(e);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_gates) (void)hipEventDestroy(ev_gates);
        if (side) (void)hipStreamDestroy(side);
        for (hipEvent_t e : ev_stage)
            if (e) (void)hipEventDestroy(e);
    }
};

// ================================================ kernels ================================================
namespace {

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// x0[b][t][:] = embeddings[tokens[b][t]][:]   (model.py:27); rows past the sentence's length are zero
__global__ void nat_embed_k(const int* __restrict__ tokens, const int* __restrict__ lengths, const float* __restrict__ emb,
                            float* __restrict__ out, int Lmax, int D, int V) {
    const int b = blockIdx.y, t = blockIdx.x;
    const int len = lengths[b];
    int tok = tokens[(size_t)b * Lmax + t];
    tok = tok < 0 ? 0 : (tok >= V ? V - 1 : tok);
    for (int c = threadIdx.x; c < D; c += blockDim.x) out[((size_t)b * Lmax + t) * D + c] = t < len ? emb[(size_t)tok * D + c] : 0.0f;
}

// y = act(batchnorm_eval(conv1d_same(x))) [+ res]   hk.Conv1D(Cout, K, padding="SAME"): w[K][Cin][Cout], cross-correlation,
// pads ((K-1)/2, K/2).  Token encoder: K = 3, BatchNorm + ReLU (model.py:28-34); postnet: K = 5, BatchNorm + tanh, the
// last layer plain and added to its input's source (model.py:113-121, :151).  inv = scale * rsqrt(var + eps) comes from
// pack time (nullptr = no BatchNorm).  Rows at or past the sequence's length read as zero (the reference runs each
// sequence alone, so its SAME padding sees zeros there) and are written as zero.
enum { NAT_ACT_NONE = 0, NAT_ACT_RELU = 1, NAT_ACT_TANH = 2 };
template <int K, int TL>
__global__ __launch_bounds__(256) void nat_conv_bn_act_k(const float* __restrict__ x, const int* __restrict__ lengths, const float* __restrict__ w,
                                                         const float* __restrict__ bias, const float* __restrict__ inv,
                                                         const float* __restrict__ mean, const float* __restrict__ offset,
                                                         const float* __restrict__ res, float* __restrict__ y, int Lmax, int Cin, int Cout,
                                                         int act) {
    extern __shared__ float xs[];  // (TL + K - 1) x Cin
    constexpr int PL = (K - 1) / 2;
    const int b = blockIdx.y, t0 = blockIdx.x * TL;
    const int len = lengths[b];
    for (int i = threadIdx.x; i < (TL + K - 1) * Cin; i += blockDim.x) {
        const int r = i / Cin, c = i % Cin;
        const int t = t0 - PL + r;
        xs[i] = (t >= 0 && t < len) ? x[((size_t)b * Lmax + t) * Cin + c] : 0.0f;
    }
    __syncthreads();
    for (int co = threadIdx.x; co < Cout; co += blockDim.x) {
        float acc[TL];
        const float bv = bias[co];
#pragma unroll
        for (int i = 0; i < TL; ++i) acc[i] = bv;
        for (int j = 0; j < K; ++j) {
            const float* __restrict__ wj = w + (size_t)j * Cin * Cout + co;
            for (int ci = 0; ci < Cin; ++ci) {
                const float wv = wj[(size_t)ci * Cout];
#pragma unroll
                for (int i = 0; i < TL; ++i) acc[i] = fmaf(xs[(i + j) * Cin + ci], wv, acc[i]);
            }
        }
        const bool bn = inv != nullptr;
        const float iv = bn ? inv[co] : 1.0f, mv = bn ? mean[co] : 0.0f, ov = bn ? offset[co] : 0.0f;
#pragma unroll
        for (int i = 0; i < TL; ++i) {
            const int t = t0 + i;
            if (t < Lmax) {
                float v = bn ? (acc[i] - mv) * iv + ov : acc[i];
                if (act == NAT_ACT_RELU) v = fmaxf(v, 0.0f);
                else if (act == NAT_ACT_TANH) v = tanhf(v);
                const size_t o = ((size_t)b * Lmax + t) * Cout + co;
                if (res) v = res[o] + v;
                y[o] = t < len ? v : 0.0f;
            }
        }
    }
}

// Postnet convolutions (model.py:113-121) and the hoisted gate GEMMs on the fp32 matrix cores: y = act(batchnorm_eval(conv1d_same(x))) [+ res],
// channels-last fp32 rows, same zero-beyond-the-length semantics as nat_conv_bn_act_k.  GEMM view: M = cout (A = weights, host-packed
// by pack_conv_frag_f32, nat_model.h), N = frame,
// k = (32-channel step, tap, channel).  A workgroup = 64 frames x (4 waves x MR m-blocks); a wave owns MR x 2 accumulator blocks.
// Round 4: the B operand goes through LDS.  Round 1-3 had every lane read 64 contiguous bytes of ITS frame's row per step and tap straight
// from L1 (no LDS, no barrier): 64 lanes x 16 bytes from 32 different rows per instruction, five times over for the five taps — the kernel
// sat at 64-80 TF/s, bound by the vector-memory pipeline (software-pipelining those loads changed nothing: profiles/r04_c_kernel_structure_findings.md).
// Now the 64 + K - 1 rows x 32 channels of a step are staged ONCE (coalesced float4 loads along the channels, next step's in flight under this
// step's MFMAs, two LDS buffers, one barrier per step), the taps are shifted views of the tile, and a fragment is one ds_read_b32 per lane
// (row stride 33 floats: 32 consecutive frames of one channel hit 32 banks).  The fmaf chains are the old ones, in the old order: same bits.
// TF (the teacher-forced pass's GEMMs, compile-time, 0 everywhere else): NAT_TF_SHIFT = row t reads x[t - 1], a zero row first (the target mels become
// the decoder's inputs without a shifted copy); NAT_TF_KEEP = hk.dropout(0.5) after the activation, v = keep[b][t][co] ? 2 v : 0 with keep rows 2 * Cout
// bytes apart (the prenet's [B][F][2][PN] masks, the pointer already at the layer's half); NAT_TF_ACC = y += the result, the previous value read
// through y itself (res is not used: y is the only pointer to that array).
enum : int { NAT_TF_SHIFT = 1, NAT_TF_KEEP = 2, NAT_TF_ACC = 4 };
// FOLD (compile-time, the postnet's layers with more than 512 input channels): the running sums are set aside every 8 steps (8 x 32 x K terms) and the
// parts added at the end, in step order.  One fp32 chain over all of 5 x 1024 terms carries four to five times the rounding error of a blocked sum
// (tools/restate_nat_conv_order.py); chains of 1280 terms stay where the narrower layers' are.  Up to 512 channels nothing changes, bit for bit.
template <int K, int MR, int TF = 0, int FOLD = 0>
__global__ __launch_bounds__(256, 2) void nat_conv_mfma_k(const float* __restrict__ x, const int* __restrict__ lengths, const float4* __restrict__ wpk,
                                                       const float* __restrict__ bias, const float* __restrict__ inv, const float* __restrict__ mean,
                                                       const float* __restrict__ offset, const float* __restrict__ res, float* __restrict__ y, int Lmax,
                                                       int Cin, int Cout, int act, int tile0, const unsigned char* __restrict__ keep = nullptr) {
    typedef float f32x16 __attribute__((ext_vector_type(16)));
    constexpr int NR = 2, PL = (K - 1) / 2 + ((TF & NAT_TF_SHIFT) ? 1 : 0), ROWS = 64 + K - 1, RS = 33, UNITS = ROWS * 8, UPT = (UNITS + 255) / 256;
    __shared__ float xs[2][ROWS * RS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int b = blockIdx.z, t0 = (blockIdx.x + tile0) * 64;  // tile0: a launch may cover the 64-frame tiles [tile0, tile0 + gridDim.x) only
    const int len = lengths[b];
    const int MB = (Cout + 31) / 32, NCS = (Cin + 31) / 32;
    const int mb0 = (blockIdx.y * 4 + wave) * MR;
    if (t0 >= len) return;               // rows at or past the length: zero by the caller's memset (last layer) or masked by the reader (uniform per workgroup)
    const bool mine = mb0 < MB;          // a wave without an m-block still helps staging and meets the barriers
    const bool two = len - t0 > 32;      // a sentence's last tile with <= 32 frames left: the second 32-frame block is skipped (uniform)
    f32x16 acc[MR][NR];
#pragma unroll
    for (int mr = 0; mr < MR; ++mr)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int co = 32 * (mb0 + mr) + 8 * rq + 4 * lh + i;
                const float bv = (mb0 + mr < MB && co < Cout) ? bias[co] : 0.0f;
#pragma unroll
                for (int nr = 0; nr < NR; ++nr) acc[mr][nr][4 * rq + i] = bv;
            }
    const float* __restrict__ xb = x + (size_t)b * Lmax * Cin;
    // staging of step cs: unit u = (row, 4-channel group); unconditional loads from clamped addresses, masked afterwards
    float4 sv[UPT];
    auto stage_load = [&](int cs) {
#pragma unroll
        for (int q = 0; q < UPT; ++q) {
            const int u = tid + q * 256, uc = u < UNITS ? u : UNITS - 1;
            const int row = uc >> 3, c = cs * 32 + 4 * (uc & 7);
            const int t = t0 + row - PL;
            const int tc = t < 0 ? 0 : (t >= len ? len - 1 : t);
            const int cc = c + 4 <= Cin ? c : Cin - 4;
            float4 v = *reinterpret_cast<const float4*>(xb + (size_t)tc * Cin + cc);
            if (t != tc || c != cc) v = make_float4(0.f, 0.f, 0.f, 0.f);
            sv[q] = v;
        }
    };
    auto stage_store = [&](int buf) {
#pragma unroll
        for (int q = 0; q < UPT; ++q) {
            const int u = tid + q * 256;
            if (u >= UNITS) continue;
            float* d = &xs[buf][(u >> 3) * RS + 4 * (u & 7)];
            d[0] = sv[q].x; d[1] = sv[q].y; d[2] = sv[q].z; d[3] = sv[q].w;
        }
    };
    // A operands (weights, L2-resident) one (step, tap) ahead in a second register set: with two workgroups per CU nothing else covers their round trip
    auto load_a = [&](int cs, int j, float4 (&av)[MR][4]) {
#pragma unroll
        for (int mr = 0; mr < MR; ++mr) {
            const int mb = mb0 + mr < MB ? mb0 + mr : MB - 1;  // a wave's spare block re-reads the last one; never stored
            const float4* __restrict__ ap = wpk + ((((size_t)mb * NCS + cs) * K + j) * 64 + lane) * 4;
#pragma unroll
            for (int q = 0; q < 4; ++q) av[mr][q] = ap[q];
        }
    };
    auto mfma_tap = [&](int buf, int j, const float4 (&av)[MR][4]) {
        const float* xr = &xs[buf][(l31 + j) * RS + 16 * lh];  // tile row of frame t0 + l31 + j - PL, this half-wave's 16 channels
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float bv[NR];
#pragma unroll
                for (int nr = 0; nr < NR; ++nr) bv[nr] = (nr == 0 || two) ? xr[nr * 32 * RS + 4 * q + e] : 0.0f;
#pragma unroll
                for (int mr = 0; mr < MR; ++mr) {
                    const float a1 = e == 0 ? av[mr][q].x : e == 1 ? av[mr][q].y : e == 2 ? av[mr][q].z : av[mr][q].w;
#pragma unroll
                    for (int nr = 0; nr < NR; ++nr)
                        if (nr == 0 || two) acc[mr][nr] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv[nr], acc[mr][nr], 0, 0, 0);
                }
            }
        }
    };
    float4 avA[MR][4], avB[MR][4];
    f32x16 tot[FOLD ? MR : 1][NR];  // FOLD: the sums of the steps set aside so far
    if constexpr (FOLD != 0) {
#pragma unroll
        for (int mr = 0; mr < MR; ++mr)
#pragma unroll
            for (int nr = 0; nr < NR; ++nr)
#pragma unroll
                for (int r = 0; r < 16; ++r) tot[mr][nr][r] = 0.0f;
    }
    stage_load(0);
    if (mine) load_a(0, 0, avA);
    stage_store(0);
    __syncthreads();
    // steps in pairs (cs0, cs0 + 1) so that LDS buffer and register-set parities are compile-time positions (K is odd: the parity of the first tap flips from
    // one step to the next)
#pragma unroll 1
    for (int cs0 = 0; cs0 < NCS; cs0 += 2) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int cs = cs0 + u;
            if (cs >= NCS) break;  // uniform
            if (cs + 1 < NCS) stage_load(cs + 1);  // in flight under this step's MFMAs
            if (mine) {
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    const bool last = j + 1 == K;
                    const int ncs = last ? cs + 1 : cs, nj = last ? 0 : j + 1;
                    const bool more = ncs < NCS;
                    if (((u * K + j) & 1) == 0) {
                        if (more) load_a(ncs, nj, avB);
                        __builtin_amdgcn_sched_barrier(0);
                        mfma_tap(u, j, avA);
                    } else {
                        if (more) load_a(ncs, nj, avA);
                        __builtin_amdgcn_sched_barrier(0);
                        mfma_tap(u, j, avB);
                    }
                }
            }
            if (cs + 1 < NCS) {
                stage_store(u ^ 1);  // nobody reads that buffer any more: its last readers passed the barrier that ended step cs - 1
                __syncthreads();
            }
        }
        if constexpr (FOLD != 0) {
            if (((cs0 + 2) & 7) == 0 && cs0 + 2 < NCS) {  // 8 steps done and more to come (uniform)
#pragma unroll
                for (int mr = 0; mr < MR; ++mr)
#pragma unroll
                    for (int nr = 0; nr < NR; ++nr)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            tot[mr][nr][r] += acc[mr][nr][r];
                            acc[mr][nr][r] = 0.0f;
                        }
            }
        }
    }
    if (!mine) return;
    if constexpr (FOLD != 0) {
#pragma unroll
        for (int mr = 0; mr < MR; ++mr)
#pragma unroll
            for (int nr = 0; nr < NR; ++nr)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mr][nr][r] = tot[mr][nr][r] + acc[mr][nr][r];
    }
    const bool bn = inv != nullptr;
#pragma unroll
    for (int mr = 0; mr < MR; ++mr)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
            const int co = 32 * (mb0 + mr) + 8 * rq + 4 * lh;
            if (mb0 + mr >= MB || co >= Cout) continue;  // Cout is a multiple of 4: a lane's 4 channels are in or out together
            float iv[4] = {1.f, 1.f, 1.f, 1.f}, mv[4] = {0.f, 0.f, 0.f, 0.f}, ov[4] = {0.f, 0.f, 0.f, 0.f};
            if (bn) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    iv[i] = inv[co + i];
                    mv[i] = mean[co + i];
                    ov[i] = offset[co + i];
                }
            }
#pragma unroll
            for (int nr = 0; nr < NR; ++nr) {
                const int t = t0 + nr * 32 + l31;
                if (t >= Lmax || (nr == 1 && !two)) continue;
                const size_t o = ((size_t)b * Lmax + t) * Cout + co;
                float v[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    v[i] = acc[mr][nr][4 * rq + i];
                    if (bn) v[i] = (v[i] - mv[i]) * iv[i] + ov[i];
                    if (act == NAT_ACT_RELU) v[i] = fmaxf(v[i], 0.0f);
                    else if (act == NAT_ACT_TANH) v[i] = tanhf(v[i]);
                }
                if constexpr ((TF & NAT_TF_KEEP) != 0) {
                    const uchar4 k4 = *reinterpret_cast<const uchar4*>(keep + ((size_t)b * Lmax + t) * 2 * Cout + co);
                    v[0] = k4.x ? v[0] * 2.0f : 0.0f; v[1] = k4.y ? v[1] * 2.0f : 0.0f; v[2] = k4.z ? v[2] * 2.0f : 0.0f; v[3] = k4.w ? v[3] * 2.0f : 0.0f;
                }
                if constexpr ((TF & NAT_TF_ACC) != 0) {
                    const float4 r = *reinterpret_cast<const float4*>(y + o);
                    v[0] = r.x + v[0]; v[1] = r.y + v[1]; v[2] = r.z + v[2]; v[3] = r.w + v[3];
                } else if (res) {
                    const float4 r = *reinterpret_cast<const float4*>(res + o);
                    v[0] += r.x; v[1] += r.y; v[2] += r.z; v[3] += r.w;
                }
                if (t >= len) v[0] = v[1] = v[2] = v[3] = 0.0f;
                *reinterpret_cast<float4*>(y + o) = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
}

// The same convolution with every product as three bf16 x bf16 terms on the bf16 matrix pipe (v_mfma_f32_32x32x16_bf16, fp32 accumulation):
// v = v0 + v1 with v0 = bf16(v), v1 = bf16(v - v0) (16 mantissa bits), x * w ~ x1 w0 + x0 w1 + x0 w0 (the dropped x1 w1 is 2^-18 of the
// product) — the split of the vocoder's bf16x3 engine (kernels_x3.hip; profiles/r04_b_split_findings.md).  An OPTION of the acoustic model
// (vtts_nat_acoustic_set_option "bf16x3"), not its default: the fp32 kernel above is what the parity tests against the reference pin at 5e-5;
// this one is for callers whose vocoder is bf16-class anyway (the text -> waveform pipeline).  Same tile, same epilogue; per 32-channel step
// and tap 6 matrix instructions of 32 cycles instead of 16 of 64.  Weights pre-split at pack time ("…#x3": [mblk][step][tap][16-channel
// half][hi | lo][lane][8] bf16, as many bytes as the fp32 fragments); the activations are split while they are staged: two bf16 LDS planes,
// rows of 32 channels padded to 80 bytes (eight lanes' 16-byte reads cover the 32 banks).
template <int K, int MR>
__global__ __launch_bounds__(256, 2) void nat_conv_x3_k(const float* __restrict__ x, const int* __restrict__ lengths, const uint4* __restrict__ wpk,
                                                     const float* __restrict__ bias, const float* __restrict__ inv, const float* __restrict__ mean,
                                                     const float* __restrict__ offset, const float* __restrict__ res, float* __restrict__ y, int Lmax,
                                                     int Cin, int Cout, int act, int tile0) {
    typedef float f32x16 __attribute__((ext_vector_type(16)));
    using vtts::bf16x8;
    constexpr int NR = 2, PL = (K - 1) / 2, ROWS = 64 + K - 1, RSB = 40, UNITS = ROWS * 8, UPT = (UNITS + 255) / 256;
    __shared__ __attribute__((aligned(16))) unsigned short xs[2][2][ROWS * RSB];  // [buffer][hi | lo][row][32 channels + 8 pad] bf16
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int b = blockIdx.z, t0 = (blockIdx.x + tile0) * 64;
    const int len = lengths[b];
    const int MB = (Cout + 31) / 32, NCS = (Cin + 31) / 32;
    const int mb0 = (blockIdx.y * 4 + wave) * MR;
    if (t0 >= len) return;
    const bool mine = mb0 < MB;
    const bool two = len - t0 > 32;
    f32x16 acc[MR][NR];
#pragma unroll
    for (int mr = 0; mr < MR; ++mr)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int co = 32 * (mb0 + mr) + 8 * rq + 4 * lh + i;
                const float bv = (mb0 + mr < MB && co < Cout) ? bias[co] : 0.0f;
#pragma unroll
                for (int nr = 0; nr < NR; ++nr) acc[mr][nr][4 * rq + i] = bv;
            }
    const float* __restrict__ xb = x + (size_t)b * Lmax * Cin;
    float4 sv[UPT];
    auto stage_load = [&](int cs) {
#pragma unroll
        for (int q = 0; q < UPT; ++q) {
            const int u = tid + q * 256, uc = u < UNITS ? u : UNITS - 1;
            const int row = uc >> 3, c = cs * 32 + 4 * (uc & 7);
            const int t = t0 + row - PL;
            const int tc = t < 0 ? 0 : (t >= len ? len - 1 : t);
            const int cc = c + 4 <= Cin ? c : Cin - 4;
            float4 v = *reinterpret_cast<const float4*>(xb + (size_t)tc * Cin + cc);
            if (t != tc || c != cc) v = make_float4(0.f, 0.f, 0.f, 0.f);
            sv[q] = v;
        }
    };
    auto stage_store = [&](int buf) {
#pragma unroll
        for (int q = 0; q < UPT; ++q) {
            const int u = tid + q * 256;
            if (u >= UNITS) continue;
            const unsigned h0 = vtts::pack_bf16x2(sv[q].x, sv[q].y), h1 = vtts::pack_bf16x2(sv[q].z, sv[q].w);
            const unsigned l0 = vtts::pack_bf16x2(sv[q].x - vtts::bf16_lo(h0), sv[q].y - vtts::bf16_hi(h0));
            const unsigned l1 = vtts::pack_bf16x2(sv[q].z - vtts::bf16_lo(h1), sv[q].w - vtts::bf16_hi(h1));
            const int o = (u >> 3) * RSB + 4 * (u & 7);
            *reinterpret_cast<uint2*>(&xs[buf][0][o]) = make_uint2(h0, h1);
            *reinterpret_cast<uint2*>(&xs[buf][1][o]) = make_uint2(l0, l1);
        }
    };
    // A fragments of one (step, tap): [16-channel half][hi | lo] per m-block, a (step, tap) ahead in a second register set
    auto load_a = [&](int cs, int j, bf16x8 (&av)[MR][2][2]) {
#pragma unroll
        for (int mr = 0; mr < MR; ++mr) {
            const int mb = mb0 + mr < MB ? mb0 + mr : MB - 1;
            const uint4* __restrict__ ap = wpk + ((((size_t)mb * NCS + cs) * K + j) * 4) * 64 + lane;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int pl = 0; pl < 2; ++pl) av[mr][ks][pl] = __builtin_bit_cast(bf16x8, ap[(ks * 2 + pl) * 64]);
        }
    };
    auto mfma_tap = [&](int buf, int j, const bf16x8 (&av)[MR][2][2]) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 bh[NR], bl[NR];
#pragma unroll
            for (int nr = 0; nr < NR; ++nr) {
                const int o = (l31 + j + 32 * nr) * RSB + 16 * ks + 8 * lh;  // frame t0 + 32 nr + l31 + j - PL, channels 16 ks + 8 lh .. + 7 of the step
                bh[nr] = *reinterpret_cast<const bf16x8*>(&xs[buf][0][o]);
                bl[nr] = *reinterpret_cast<const bf16x8*>(&xs[buf][1][o]);
            }
            // the small terms first
#pragma unroll
            for (int mr = 0; mr < MR; ++mr)
#pragma unroll
                for (int nr = 0; nr < NR; ++nr)
                    if (nr == 0 || two) acc[mr][nr] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[mr][ks][1], bh[nr], acc[mr][nr], 0, 0, 0);
#pragma unroll
            for (int mr = 0; mr < MR; ++mr)
#pragma unroll
                for (int nr = 0; nr < NR; ++nr)
                    if (nr == 0 || two) acc[mr][nr] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[mr][ks][0], bl[nr], acc[mr][nr], 0, 0, 0);
#pragma unroll
            for (int mr = 0; mr < MR; ++mr)
#pragma unroll
                for (int nr = 0; nr < NR; ++nr)
                    if (nr == 0 || two) acc[mr][nr] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[mr][ks][0], bh[nr], acc[mr][nr], 0, 0, 0);
        }
    };
    bf16x8 avA[MR][2][2], avB[MR][2][2];
    stage_load(0);
    if (mine) load_a(0, 0, avA);
    stage_store(0);
    __syncthreads();
#pragma unroll 1
    for (int cs0 = 0; cs0 < NCS; cs0 += 2) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int cs = cs0 + u;
            if (cs >= NCS) break;  // uniform
            if (cs + 1 < NCS) stage_load(cs + 1);
            if (mine) {
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    const bool last = j + 1 == K;
                    const int ncs = last ? cs + 1 : cs, nj = last ? 0 : j + 1;
                    const bool more = ncs < NCS;
                    if (((u * K + j) & 1) == 0) {
                        if (more) load_a(ncs, nj, avB);
                        __builtin_amdgcn_sched_barrier(0);
                        mfma_tap(u, j, avA);
                    } else {
                        if (more) load_a(ncs, nj, avA);
                        __builtin_amdgcn_sched_barrier(0);
                        mfma_tap(u, j, avB);
                    }
                }
            }
            if (cs + 1 < NCS) {
                stage_store(u ^ 1);
                __syncthreads();
            }
        }
    }
    if (!mine) return;
    const bool bn = inv != nullptr;
#pragma unroll
    for (int mr = 0; mr < MR; ++mr)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
            const int co = 32 * (mb0 + mr) + 8 * rq + 4 * lh;
            if (mb0 + mr >= MB || co >= Cout) continue;
            float iv[4] = {1.f, 1.f, 1.f, 1.f}, mv[4] = {0.f, 0.f, 0.f, 0.f}, ov[4] = {0.f, 0.f, 0.f, 0.f};
            if (bn) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    iv[i] = inv[co + i];
                    mv[i] = mean[co + i];
                    ov[i] = offset[co + i];
                }
            }
#pragma unroll
            for (int nr = 0; nr < NR; ++nr) {
                const int t = t0 + nr * 32 + l31;
                if (t >= Lmax || (nr == 1 && !two)) continue;
                const size_t o = ((size_t)b * Lmax + t) * Cout + co;
                float v[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    v[i] = acc[mr][nr][4 * rq + i];
                    if (bn) v[i] = (v[i] - mv[i]) * iv[i] + ov[i];
                    if (act == NAT_ACT_RELU) v[i] = fmaxf(v[i], 0.0f);
                    else if (act == NAT_ACT_TANH) v[i] = tanhf(v[i]);
                }
                if (res) {
                    const float4 r = *reinterpret_cast<const float4*>(res + o);
                    v[0] += r.x; v[1] += r.y; v[2] += r.z; v[3] += r.w;
                }
                if (t >= len) v[0] = v[1] = v[2] = v[3] = 0.0f;
                *reinterpret_cast<float4*>(y + o) = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
}

// durations = softplus(Linear(D->1)(gelu(Linear(2D->D)(enc))))   (model.py:64-70); blockDim = D, one token per block
__global__ void nat_duration_head_k(const float* __restrict__ enc, const int* __restrict__ lengths, const float* __restrict__ w1,
                                    const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
                                    float* __restrict__ dur, int Lmax, int D) {
    extern __shared__ float sh[];  // enc row [2D], partial sums [blockDim/64]
    float* e = sh;
    float* part = sh + 2 * D;
    const int b = blockIdx.y, t = blockIdx.x, j = threadIdx.x;
    const int len = lengths[b];
    if (t >= len) {
        if (j == 0) dur[(size_t)b * Lmax + t] = 0.0f;
        return;
    }
    for (int i = j; i < 2 * D; i += blockDim.x) e[i] = enc[((size_t)b * Lmax + t) * (2 * D) + i];
    __syncthreads();
    float acc = b1[j];
    for (int k = 0; k < 2 * D; ++k) acc = fmaf(e[k], w1[(size_t)k * D + j], acc);
    // jax.nn.gelu(approximate=True)
    const float u = 0.7978845608028654f * (acc + 0.044715f * acc * acc * acc);
    float v = 0.5f * acc * (1.0f + tanhf(u)) * w2[j];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((j & 63) == 0) part[j >> 6] = v;
    __syncthreads();
    if (j == 0) {
        float s = b2[0];
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += part[i];
        // jax.nn.softplus = logaddexp(s, 0) = max(s, 0) + log1p(exp(-|s|))
        dur[(size_t)b * Lmax + t] = fmaxf(s, 0.0f) + log1pf(expf(-fabsf(s)));
    }
}

// AcousticModel.upsample (model.py:102-111): cond[b][f][:] = sum_j softmax_j(-(mid_j - f)^2 / 10) * enc[b][j][:], with
// mid = cumsum(d) - d/2, d in frames; E = 2D encoder channels.
// The conditioning's share of the LSTM gates WITHOUT materialising the conditioning (round 4).  cond[b][f] = sum_k a[b][f][k] enc[b][k]
// only ever meets the first E rows of the two LSTMs' input matrices (x = [cond_f ; p], model.py:134-141), so
//   G_l[b][f] = b_l + cond[b][f] @ W_l[0:E] = b_l + sum_k a[b][f][k] (enc[b][k] @ W_l[0:E]):
// the GEMM runs over TOKENS (EG_l = enc @ W_l[0:E], nat_conv_mfma_k with one tap; a sixth of the frames' rows: 302 -> 37 GFLOP for 256 sentences)
// and this kernel mixes its rows into the frames' rows with the upsampling weights a = softmax_k(-(mid_k - f)^2 / 10), mid = cumsum(d) - d/2.
// A workgroup = NAT_MIX_FT frames x 1024 gate columns of one sentence and one layer: the weights of its frames in LDS ([token][frame]: four
// 16-byte broadcast reads per token), a thread's 4 columns x NAT_MIX_FT frames in registers, EG rows streamed from L2 (coalesced float4).
// Sums in token order, weights from the sentence's own durations: a row does not depend on its batch.
constexpr int NAT_MIX_FT = 16;
constexpr int NAT_RES_DEFAULT_GRID = 128;  // workgroups of the resident decoder (64, 128 or 256): DESIGN.md section 6g
__global__ __launch_bounds__(256) void nat_gates_mix_k(const float* __restrict__ eg1, const float* __restrict__ eg2, const float* __restrict__ bias1,
                                                       const float* __restrict__ bias2, const int* __restrict__ lengths, const float* __restrict__ dur,
                                                       const int* __restrict__ nframes, float* __restrict__ G1, float* __restrict__ G2, int Lmax, int Fmax,
                                                       int G4, int tile0) {
    constexpr int FT = NAT_MIX_FT;
    extern __shared__ float sw[];
    float* mid = sw;                       // [Lmax rounded up to 4]
    float* wn = sw + (Lmax + 3) / 4 * 4;   // [Lmax][FT]
    const int b = blockIdx.z, f0 = (blockIdx.x + tile0) * FT, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int len = lengths[b], nf = nframes[b];
    if (f0 >= nf) return;  // rows at or past the sentence's frames are never used (the step kernel masks them)
    const int chunks = G4 / 1024, layer = blockIdx.y / chunks, col = (blockIdx.y % chunks) * 1024 + 4 * t;
    if (t == 0) {  // jnp.cumsum: sequential fp32 prefix sum
        float end = 0.0f;
        for (int k = 0; k < len; ++k) {
            const float d = dur[(size_t)b * Lmax + k];
            end += d;
            mid[k] = end - d / 2.0f;
        }
    }
    __syncthreads();
    // a wave takes FT / 4 of the tile's frames, one after the other: max and sum over the tokens in a fixed butterfly order
    for (int q = 0; q < FT / 4; ++q) {
        const int fi = wave * (FT / 4) + q;
        const float ff = (float)(f0 + fi);
        float mx = -INFINITY;
#pragma clang loop vectorize(disable)  // the loop vectoriser would pair these into v_pk_*_f32 (build.py: no packed-f32 VALU code)
        for (int k = lane; k < len; k += 64) {
            const float z = mid[k] - ff;
            mx = fmaxf(mx, -(z * z) / 10.0f);
        }
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        float sum = 0.0f;
#pragma clang loop vectorize(disable)  // the loop vectoriser would pair these into v_pk_*_f32 (build.py: no packed-f32 VALU code)
        for (int k = lane; k < len; k += 64) {
            const float z = mid[k] - ff;
            const float e = expf(-(z * z) / 10.0f - mx);
            wn[k * FT + fi] = e;
            sum += e;
        }
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
#pragma clang loop vectorize(disable)
        for (int k = lane; k < len; k += 64) wn[k * FT + fi] = wn[k * FT + fi] / sum;
    }
    __syncthreads();
    const float* __restrict__ eg = (layer ? eg2 : eg1) + (size_t)b * Lmax * G4 + col;
    const float4 bv = *reinterpret_cast<const float4*>((layer ? bias2 : bias1) + col);
    float4 acc[FT];
#pragma unroll
    for (int i = 0; i < FT; ++i) acc[i] = bv;
#pragma unroll 4
    for (int k = 0; k < len; ++k) {
        const float4 e = *reinterpret_cast<const float4*>(eg + (size_t)k * G4);
        const float4* __restrict__ w4 = reinterpret_cast<const float4*>(wn + k * FT);
#pragma unroll
        for (int q = 0; q < FT / 4; ++q) {
            const float4 w = w4[q];
            const float ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float4& a = acc[4 * q + i];
                a.x = fmaf(ws[i], e.x, a.x);
                a.y = fmaf(ws[i], e.y, a.y);
                a.z = fmaf(ws[i], e.z, a.z);
                a.w = fmaf(ws[i], e.w, a.w);
            }
        }
    }
    float* __restrict__ G = (layer ? G2 : G1) + ((size_t)b * Fmax + f0) * G4 + col;
#pragma unroll
    for (int i = 0; i < FT; ++i)
        if (f0 + i < nf) *reinterpret_cast<float4*>(G + (size_t)i * G4) = acc[i];
}

// AcousticModel.inference's scan body (model.py:134-141) for ALL sentences of the batch at once, one launch per layer per
// frame (the recurrence is sequential in frames; sentences are independent):
//   p = dropout(relu(dropout(relu(prev @ f1)) @ f2))           prenet, no bias, rate 0.5, ALWAYS on (model.py:95-100);
//                                                               keep[b][f][0|1][PN] bytes (1 = keep, value * 2), nullptr = none
//   x = [cond_f ; p];  h1 = LSTM1([x ; h1]);  h2 = LSTM2([[x ; h1] ; h2])      hk.deep_rnn_with_skip_connections
//       (dm-haiku recurrent.py, _DeepRNN.__call__: current_inputs = tree_map(concat, inputs, current_inputs), i.e. the
//        NETWORK INPUT first, then the previous layer's output; hk.LSTM then appends its own hidden state)
//   mel_f = [h1 ; h2] @ wp + bp;  prev = mel_f
// Decoder state in HBM, k-major in groups of four rows with the sentences contiguous (Bp = B rounded up to 64 columns),
// ping-pong by frame parity:
//   Z[parity][row / 4][Bp][row % 4]  (one 16-byte load per lane = 4 consecutive rows of its sentence: the LSTM step is bound
//   by the number of vector-memory instructions a CU can issue, and dword loads of the state were 8 of its 9 per iteration),
//   rows [ p (PN) | h1 (H) | h2 (H) ]:  LSTM1 reads p of the current parity then h1 of the previous one; LSTM2 reads
//   [p ; h1] of the current parity then h2 of the previous one.  Haiku's matrices are [cond ; p ; h1] and
//   [cond ; p ; h1 ; h2] (x = [cond ; p] first): the state order is Haiku's order minus the cond rows.
//   **The conditioning's share of the gates is hoisted out of the frame loop (round 4):** cond_f is known for every frame
//   before the loop starts, so G_l[b][f][:] = b_l + cond[b][f] @ W_l[0:E] is ONE fp32-MFMA GEMM per layer ahead of the loop
//   (nat_conv_mfma_k with one tap, output columns in the step kernel's accumulator order) and a step starts its sums from
//   G_l[b][f] instead of from the bias: per-frame K 1280 -> 768 (layer 1) and 1792 -> 1280 (layer 2), a third less of the
//   L2 -> CU weight stream that bounds the step.  Only the first 64 frames' G is computed in front of the loop; the rest runs on
//   a side stream beside the (latency-bound) first 64 steps.  Cell states c1, c2 as [H][Bp].
//
// nat_dec_lstm_k: gates[32 sentences x (8 units x 4 gates)] per wave on the fp32 matrix cores (v_mfma_f32_32x32x2_f32:
// M = the slice's 32 gate columns ordered 4*unit + gate, N = 32 sentences, K = 2 per instruction).  With that row order a
// lane's 16 accumulators are the i, g, f, o pre-activations of 4 (unit, sentence) pairs: the LSTM cell update
// (hk.LSTM: gates i, g, f, o; forget bias +1) happens in registers, no exchange.  Weights host-packed per slice so that one
// 16-byte load per lane feeds 4 MFMAs ([slice][K/8][lane][4]: element i = W[8*kb + 4*(lane/32) + i][col(lane%32)]);
// activations straight from Z (128-byte rows, L2-resident); both PD iterations (8 k each) ahead in registers.
// Every output element depends on its own sentence's column only: rows are bit-identical alone or batched.
__device__ __forceinline__ size_t nat_zidx(int row, int b, int Bp) { return ((size_t)(row >> 2) * Bp + b) * 4 + (row & 3); }
#ifndef VTTS_NAT_PD
#define VTTS_NAT_PD 4
#endif
constexpr int NAT_DEC_PD = VTTS_NAT_PD;   // iterations (8 k each) a wave keeps in flight (7 measured no faster: the step is L2-bandwidth-bound)

// Which frame a step is for.  A call's rows all stand at the same frame `f`; a slot pool's rows (vtts_nat_acoustic_pool_*) each stand at their own,
// f_b = tick - start[b], and a row is idle while f_b < 0 or f_b >= nframes[b].  POOL selects the second form in the three step kernels; whatever a
// step indexes by its frame (the hoisted gates, the mel row, the keep bytes, the guards) goes through these two functions, so the sums are the
// same chains in both forms.
template <bool POOL>
struct NatFrameArg {
    int f;
};
template <>
struct NatFrameArg<true> {
    int tick;
    const int* start;  // [slots]
};
template <bool POOL>
__device__ __forceinline__ int nat_row_frame(const NatFrameArg<POOL>& a, int b) {
    if constexpr (POOL) return a.tick - a.start[b];
    else return a.f;
}
// the row decodes a frame in this step
template <bool POOL>
__device__ __forceinline__ bool nat_row_live(int fb, int nf) {
    if constexpr (POOL) return fb >= 0 && fb < nf;
    else return fb < nf;
}
// the hoisted gates of row b at its frame: a call's host has moved ops.gin to frame f already, a pool's rows move it themselves (idle rows read frame 0)
template <bool POOL>
__device__ __forceinline__ const float* nat_row_gin(const float* gin, size_t gpitch, int b, int fb, int nf, int G4) {
    if constexpr (POOL) return gin + (size_t)b * gpitch + (size_t)(nat_row_live<true>(fb, nf) ? fb : 0) * G4;
    else return gin + (size_t)b * gpitch;
}

// NT = 32-sentence tiles per wave (one weight fragment feeds NT MFMAs: L2 traffic for the weights / NT), KW = waves per
// workgroup, each with a contiguous share of K; their partial sums meet in LDS in a fixed tree order.
// One LSTM's operands; blockIdx.z picks one of two sets (the token encoder steps its forward and backward LSTMs in one launch).
struct NatLstmOps {
    const float* inA;    // KA state rows, then
    const float* inB;    // KB state rows (the LSTM's own previous hidden state)
    const float4* wpk;   // [slice][K/8][lane][4]
    const float* bias;   // [4H], gates i, g, f, o
    float* cst;          // cell state [H][Bp]
    float* hout;         // new hidden state, state layout
    const float* gin;    // optional: this step's gate pre-activations computed ahead of the loop (bias + the contribution of inputs known in
                         // advance), [sentence][gpitch floats] with the step's 4H values in the order ((slice * 2 + lane / 32) * 4 + unit pair) * 4 + gate:
                         // a lane's 16 accumulators are 64 contiguous bytes.  nullptr = start from the bias.
    size_t gpitch;
};
template <int NT, int KW, int SL = 1, bool POOL = false>
__global__ __launch_bounds__(64 * KW) void nat_dec_lstm_k(NatLstmOps ops0, NatLstmOps ops1, int KA, int KB, const int* __restrict__ nframes, NatFrameArg<POOL> fa,
                                                          int B, int Bp, int H) {
    // SL = slices (8 units each) per workgroup: a wave's state fragments feed SL weight fragments, so the state's share of the L2 -> CU stream
    // (2/3 of it at SL = 1, NT = 2: every slice's workgroup reads the whole state of its sentences) falls by SL.  Each output element's sum is
    // the same chain in the same order whatever SL is.  MEASURED (round 4, 256 sentences): SL = 2 makes the step 19.3 -> 28.9 us — the step is not
    // bound by that stream but by what ONE workgroup has to do (its fp32 MFMAs: 2 waves per SIMD x K/64 iterations x 8 x 64 cycles = 6-10 us, and
    // a cold L2 at every launch: 17.5 MB of misses per step, PMC passes in profiles/r04_e_nat_decoder_findings.md); the launches use SL = 1.
    typedef float f32x16 __attribute__((ext_vector_type(16)));
    static_assert(KW == 1 || KW == 2 || KW == 4 || KW == 8, "tree reduction");
    __shared__ float red[KW][SL][NT][16][64];  // every wave's share of the gate sums
    const NatLstmOps& ops = blockIdx.z ? ops1 : ops0;
    const float* __restrict__ inA = ops.inA;
    const float* __restrict__ inB = ops.inB;
    const float4* __restrict__ wpk = ops.wpk;
    const float* __restrict__ bias = ops.bias;
    float* __restrict__ cst = ops.cst;
    float* __restrict__ hout = ops.hout;
    const int lane = threadIdx.x & 63, kw = threadIdx.x >> 6, l31 = lane & 31, lh = lane >> 5;
    const int slice0 = blockIdx.x * SL, b0 = blockIdx.y * 32 * NT;
    const int NIT = (KA + KB) / 8, NWMAX = (NIT + KW - 1) / KW, it_lo = kw * NWMAX;
    const int NW = it_lo >= NIT ? 0 : (NIT - it_lo < NWMAX ? NIT - it_lo : NWMAX);  // this wave's iterations [it_lo, it_lo + NW)
    // this wave's cell-update blocks ((slice, sentence tile, unit pair) kw, kw + KW, ...): their cell states are requested now, a kernel's length
    // before they are needed (round 4: loaded after the reduction they were ~1 us of every step)
    constexpr int NBLK = (SL * NT * 4 + KW - 1) / KW;
    float cold[NBLK];
#pragma unroll
    for (int q = 0; q < NBLK; ++q) {
        const int blk = kw + q * KW, sl = blk / (NT * 4), nt = (blk / 4) % NT, rq = blk % 4;
        cold[q] = blk < SL * NT * 4 ? cst[(size_t)(8 * (slice0 + sl) + 2 * rq + lh) * Bp + b0 + 32 * nt + l31] : 0.0f;
    }
    // a pool's rows look their frame up first: the hoisted gates' address depends on it (one 4-byte load per row in front of the gate loads)
    int fb[NT], nfb[NT];
    if constexpr (POOL) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int b = b0 + 32 * nt + l31, bc = b < B ? b : B - 1;
            fb[nt] = nat_row_frame(fa, bc), nfb[nt] = nframes[bc];
        }
    }
    f32x16 acc[SL][NT][2];
    if (ops.gin != nullptr && kw == 0) {
        // the sum starts from the hoisted part (bias + the inputs known ahead of the loop, themselves an MFMA chain in k order)
#pragma unroll
        for (int sl = 0; sl < SL; ++sl)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int b = b0 + 32 * nt + l31;
                const float4* __restrict__ gp = reinterpret_cast<const float4*>(
                    nat_row_gin<POOL>(ops.gin, ops.gpitch, b < B ? b : B - 1, POOL ? fb[nt] : 0, POOL ? nfb[nt] : 0, 4 * H) + (size_t)(2 * (slice0 + sl) + lh) * 16);
#pragma unroll
                for (int rq = 0; rq < 4; ++rq) {
                    const float4 g4 = gp[rq];
                    acc[sl][nt][0][4 * rq + 0] = g4.x;
                    acc[sl][nt][0][4 * rq + 1] = g4.y;
                    acc[sl][nt][0][4 * rq + 2] = g4.z;
                    acc[sl][nt][0][4 * rq + 3] = g4.w;
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[sl][nt][1][4 * rq + i] = 0.0f;
                }
            }
    } else {
#pragma unroll
        for (int sl = 0; sl < SL; ++sl)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float bv = (kw == 0 && ops.gin == nullptr) ? bias[i * H + 8 * (slice0 + sl) + 2 * rq + lh] : 0.0f;
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        acc[sl][nt][0][4 * rq + i] = bv;
                        acc[sl][nt][1][4 * rq + i] = 0.0f;
                    }
                }
    }
    float4 wv[NAT_DEC_PD][SL];
    float4 xv[NAT_DEC_PD][NT];
    const float4* __restrict__ wsl = wpk + (size_t)slice0 * NIT * 64 + lane;
    auto load_it = [&](int it, int slot) {
        if (it >= NIT) it = NIT - 1;  // tail: an in-bounds re-read, never used
#pragma unroll
        for (int sl = 0; sl < SL; ++sl) wv[slot][sl] = wsl[((size_t)sl * NIT + it) * 64];
        const int k0 = it * 8;
        // rows k0 + 4*lh .. + 3 of this lane's sentences: MFMA j of the iteration takes k = k0 + 4*(lane/32) + j on both operands
        const float* __restrict__ xr = (k0 < KA ? inA + (size_t)k0 * Bp : inB + (size_t)(k0 - KA) * Bp) + ((size_t)lh * Bp + b0 + l31) * 4;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) xv[slot][nt] = *reinterpret_cast<const float4*>(xr + (size_t)(32 * nt) * 4);
    };
#pragma unroll
    for (int j = 0; j < NAT_DEC_PD; ++j) load_it(it_lo + j, j);
    // which sentences still decode is looked up only now, behind the first operands' loads (the early exit of a finished tile waits for an L2
    // round trip; in front of everything it was that much of EVERY step: 0.18 ms of the bf16x3 acoustic model)
    bool live[NT];
    bool any = false;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int b = b0 + 32 * nt + l31;
        if constexpr (POOL) live[nt] = b < B && nat_row_live<true>(fb[nt], nfb[nt]);
        else live[nt] = b < B && nat_row_live<false>(nat_row_frame(fa, b), nframes[b < B ? b : B - 1]);
        any = any || live[nt];
    }
    if (__ballot(any) == 0ull) return;  // every sentence of these tiles has all its frames (same for all waves)
#pragma nounroll
    for (int it0 = 0; it0 < NW; it0 += NAT_DEC_PD) {
#pragma unroll
        for (int j = 0; j < NAT_DEC_PD; ++j) {
            if (it0 + j >= NW) break;  // wave-uniform
#pragma unroll
            for (int sl = 0; sl < SL; ++sl)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[sl][nt][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[j][sl].x, xv[j][nt].x, acc[sl][nt][0], 0, 0, 0);
#pragma unroll
            for (int sl = 0; sl < SL; ++sl)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[sl][nt][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[j][sl].y, xv[j][nt].y, acc[sl][nt][1], 0, 0, 0);
#pragma unroll
            for (int sl = 0; sl < SL; ++sl)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[sl][nt][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[j][sl].z, xv[j][nt].z, acc[sl][nt][0], 0, 0, 0);
#pragma unroll
            for (int sl = 0; sl < SL; ++sl)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[sl][nt][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[j][sl].w, xv[j][nt].w, acc[sl][nt][1], 0, 0, 0);
            const int nx = it0 + j + NAT_DEC_PD;
            load_it(nx < NW ? it_lo + nx : NIT, j);
        }
    }
#pragma unroll
    for (int sl = 0; sl < SL; ++sl)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[sl][nt][0][r] += acc[sl][nt][1][r];
    // every wave leaves its share of the sums in LDS; after ONE barrier a wave adds the KW shares of its own cell-update blocks in wave order
    // (round 4: a three-level tree with a barrier per level cost ~0.5 us of every step)
    if constexpr (KW > 1) {
#pragma unroll
        for (int sl = 0; sl < SL; ++sl)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) red[kw][sl][nt][r][lane] = acc[sl][nt][0][r];
        __syncthreads();
    }
    // The cell update (3 sigmoids + 2 tanh per (unit, sentence): ~1000 VALU instructions per lane for a wave's 8 pairs) is shared out: wave w takes
    // the (slice, sentence tile, unit pair) blocks w, w + KW, ... (round 2 left it to wave 0 alone while the other seven idled: ~2.5 us of a step).
    auto cell_update = [&](int sl, int nt, int rq, float c, float gi, float gg, float gf, float go) {
        if (!live[nt]) return;
        const int b = b0 + 32 * nt + l31;
        const int u = 8 * (slice0 + sl) + 2 * rq + lh;
        c = sigmoidf_(gf + 1.0f) * c + sigmoidf_(gi) * tanhf(gg);
        cst[(size_t)u * Bp + b] = c;
        hout[nat_zidx(u, b, Bp)] = sigmoidf_(go) * tanhf(c);
    };
    if constexpr (KW == 1) {
#pragma unroll
        for (int blk = 0; blk < SL * NT * 4; ++blk) {
            const int sl = blk / (NT * 4), nt = (blk / 4) % NT, rq = blk % 4;
            cell_update(sl, nt, rq, cold[blk], acc[sl][nt][0][4 * rq + 0], acc[sl][nt][0][4 * rq + 1], acc[sl][nt][0][4 * rq + 2], acc[sl][nt][0][4 * rq + 3]);
        }
    } else {
#pragma unroll
        for (int blk = 0; blk < SL * NT * 4; ++blk) {
            if (blk % KW != kw) continue;  // wave-uniform
            const int sl = blk / (NT * 4), nt = (blk / 4) % NT, rq = blk % 4;
            float gs[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float v = red[0][sl][nt][4 * rq + i][lane];
#pragma unroll
                for (int w = 1; w < KW; ++w) v += red[w][sl][nt][4 * rq + i][lane];
                gs[i] = v;
            }
            cell_update(sl, nt, rq, cold[blk / KW], gs[0], gs[1], gs[2], gs[3]);
        }
    }
}

// (Round 4 built the decoder as ONE resident kernel per run of frames — bit-identical, 26.7 ms against 22.4 with the per-frame launches; the L2s of the 8 XCDs
//  are not coherent, so every barrier costs the workgroups their cached state — and did not ship it: profiles/r04_e_nat_decoder_findings.md.)

// ---- the decoder step with the option "bf16x3": the gate sums as three bf16 x bf16 terms per product on the bf16 matrix pipe ----------------
// The state lives in HBM already split: Zx[parity][hi | lo][row / 8][Bp][8] bf16 (rows [p | h1 | h2]; h = hi + lo to 16 mantissa bits), so that a
// lane's B fragment of v_mfma_f32_32x32x16_bf16 (sentence lane % 32, rows 16 step + 8 (lane / 32) .. + 7) is one 16-byte load per plane; the
// weights are split at pack time ("…#x3": [slice][K / 16][hi | lo][lane][8] bf16, the fp32 fragments' bytes).  Per 16 rows and 32-sentence tile
// three matrix instructions of 32 cycles instead of eight of 64; everything around them (the hoisted gates G in fp32, the tree over the K
// shares, the cell update in fp32 registers, c in fp32) is the fp32 step's.  Every output element still depends on its own sentence only.
__device__ __forceinline__ size_t nat_zxidx(int row, int b, int Bp) { return ((size_t)(row >> 3) * Bp + b) * 8 + (row & 7); }
struct NatLstmX3Ops {
    const unsigned short* zc;  // this frame's parity (rows [0, KA) are read from it), plane 0; plane 1 at + plane
    const unsigned short* zp;  // the previous frame's (rows [KA, K))
    size_t plane;              // bf16 elements between the hi and the lo plane
    const uint4* wpk;          // [slice][K / 16][2][64] x 16 bytes
    const float* gin;          // this step's hoisted gate pre-activations (NatLstmOps::gin)
    size_t gpitch;
    float* cst;                // [H][Bp] fp32
    unsigned short* hout;      // zc, plane 0: the new hidden state goes to rows out_row0 + unit
    int out_row0;
};
template <int NT, int KW, bool POOL = false>
__global__ __launch_bounds__(64 * KW) void nat_dec_lstm_x3_k(NatLstmX3Ops ops, int KA, int K, const int* __restrict__ nframes, NatFrameArg<POOL> fa, int B, int Bp,
                                                             int H) {
    typedef float f32x16 __attribute__((ext_vector_type(16)));
    using vtts::bf16x8;
    constexpr int PD = 3;
    __shared__ float red[KW][NT][16][64];
    const int lane = threadIdx.x & 63, kw = threadIdx.x >> 6, l31 = lane & 31, lh = lane >> 5;
    const int slice = blockIdx.x, b0 = blockIdx.y * 32 * NT;
    const int NST = K / 16, NWMAX = (NST + KW - 1) / KW, st_lo = kw * NWMAX;
    const int NW = st_lo >= NST ? 0 : (NST - st_lo < NWMAX ? NST - st_lo : NWMAX);
    int fb[NT], nfb[NT];  // (a pool's rows look their frame up first, as in nat_dec_lstm_k)
    if constexpr (POOL) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int b = b0 + 32 * nt + l31, bc = b < B ? b : B - 1;
            fb[nt] = nat_row_frame(fa, bc), nfb[nt] = nframes[bc];
        }
    }
    f32x16 acc[NT];
    if (kw == 0) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int b = b0 + 32 * nt + l31;
            const float4* __restrict__ gp = reinterpret_cast<const float4*>(
                nat_row_gin<POOL>(ops.gin, ops.gpitch, b < B ? b : B - 1, POOL ? fb[nt] : 0, POOL ? nfb[nt] : 0, 4 * H) + (size_t)(2 * slice + lh) * 16);
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                const float4 g4 = gp[rq];
                acc[nt][4 * rq + 0] = g4.x;
                acc[nt][4 * rq + 1] = g4.y;
                acc[nt][4 * rq + 2] = g4.z;
                acc[nt][4 * rq + 3] = g4.w;
            }
        }
    } else {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[nt][r] = 0.0f;
    }
    // this wave's cell-update block(s): the cell state is requested now, a kernel's length before it is needed
    constexpr int NBLK = (NT * 4 + KW - 1) / KW;
    float cold[NBLK];
#pragma unroll
    for (int q = 0; q < NBLK; ++q) {
        const int blk = kw + q * KW, nt = blk / 4, rq = blk % 4;
        cold[q] = blk < NT * 4 ? ops.cst[(size_t)(8 * slice + 2 * rq + lh) * Bp + b0 + 32 * nt + l31] : 0.0f;
    }
    uint4 wv[PD][2], xv[PD][NT][2];
    const uint4* __restrict__ wsl = ops.wpk + (size_t)slice * NST * 2 * 64 + lane;
    auto load_st = [&](int st, int slot) {
        if (st >= NST) st = NST - 1;  // tail: an in-bounds re-read, never used
        wv[slot][0] = wsl[(size_t)(2 * st) * 64];
        wv[slot][1] = wsl[(size_t)(2 * st + 1) * 64];
        const unsigned short* __restrict__ zs = (16 * st < KA ? ops.zc : ops.zp) + ((size_t)(2 * st + lh) * Bp + b0 + l31) * 8;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            xv[slot][nt][0] = *reinterpret_cast<const uint4*>(zs + (size_t)(32 * nt) * 8);
            xv[slot][nt][1] = *reinterpret_cast<const uint4*>(zs + ops.plane + (size_t)(32 * nt) * 8);
        }
    };
#pragma unroll
    for (int j = 0; j < PD; ++j) load_st(st_lo + j, j);
    // (the frame counts behind the first operands' loads, as in nat_dec_lstm_k)
    bool live[NT];
    bool any = false;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int b = b0 + 32 * nt + l31;
        if constexpr (POOL) live[nt] = b < B && nat_row_live<true>(fb[nt], nfb[nt]);
        else live[nt] = b < B && nat_row_live<false>(nat_row_frame(fa, b), nframes[b < B ? b : B - 1]);
        any = any || live[nt];
    }
    if (__ballot(any) == 0ull) return;
#pragma nounroll
    for (int i0 = 0; i0 < NW; i0 += PD) {
#pragma unroll
        for (int j = 0; j < PD; ++j) {
            if (i0 + j >= NW) break;  // wave-uniform
            const bf16x8 whi = __builtin_bit_cast(bf16x8, wv[j][0]), wlo = __builtin_bit_cast(bf16x8, wv[j][1]);
            // the small terms first
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wlo, __builtin_bit_cast(bf16x8, xv[j][nt][0]), acc[nt], 0, 0, 0);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(whi, __builtin_bit_cast(bf16x8, xv[j][nt][1]), acc[nt], 0, 0, 0);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(whi, __builtin_bit_cast(bf16x8, xv[j][nt][0]), acc[nt], 0, 0, 0);
            const int nx = i0 + j + PD;
            load_st(nx < NW ? st_lo + nx : NST, j);
        }
    }
    // every wave leaves its share of the sums in LDS; after ONE barrier a wave adds the KW shares of its own cell-update block in wave order
    // (round 4: a three-level tree with a barrier per level, and the cell state loaded only after it, cost 1.1 us of every step)
    {
        float* redf = &red[0][0][0][0];  // [KW][NT][16][64] (the kernel's LDS is sized for it under this switch)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) redf[((kw * NT + nt) * 16 + r) * 64 + lane] = acc[nt][r];
    }
    __syncthreads();
#pragma unroll
    for (int blk = 0; blk < NT * 4; ++blk) {
        if (blk % KW != kw) continue;  // wave-uniform
        const int nt = blk / 4, rq = blk % 4;
        if (!live[nt]) continue;
        float gs[4];
        {
            const float* redf = &red[0][0][0][0];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float v = redf[((0 * NT + nt) * 16 + 4 * rq + i) * 64 + lane];
#pragma unroll
                for (int w = 1; w < KW; ++w) v += redf[((w * NT + nt) * 16 + 4 * rq + i) * 64 + lane];
                gs[i] = v;
            }
        }
        const float gi = gs[0], gg = gs[1], gf = gs[2], go = gs[3];
        const int b = b0 + 32 * nt + l31, u = 8 * slice + 2 * rq + lh;
        float c = cold[blk / KW];
        c = sigmoidf_(gf + 1.0f) * c + sigmoidf_(gi) * tanhf(gg);
        ops.cst[(size_t)u * Bp + b] = c;
        const float hv = sigmoidf_(go) * tanhf(c);
        const unsigned hp = vtts::pack_bf16x2(hv, 0.0f);
        const unsigned lp = vtts::pack_bf16x2(hv - vtts::bf16_lo(hp), 0.0f);
        const size_t o = nat_zxidx(ops.out_row0 + u, b, Bp);
        ops.hout[o] = (unsigned short)(hp & 0xffffu);
        ops.hout[o + ops.plane] = (unsigned short)(lp & 0xffffu);
    }
}

// TokenEncoder's two LSTMs (model.py:39-46) on the same batched step kernel: hk.LSTM over [x_t ; h] is the decoder step with
// KA = D input rows and KB = D hidden rows, and all sentences advance together (one launch per token position steps BOTH
// directions: blockIdx.z).  The step kernel wants its operands k-major with the sentences contiguous, so
//   nat_enc_scatter_k : x [B][Lmax][D] -> XT[dir][s][D/4][Bp][4]; step s of the backward LSTM reads token len-1-s, which IS
//                       hk.dynamic_unroll over the length-reversed sequence (jnp.flip with the ResetCore reset falling on the
//                       padding steps, where the state still is the initial state);
//   step s            : reads XT[dir][s] and HS[dir][s] (slab 0 = zeros = the initial state), writes HS[dir][s + 1] for the
//                       sentences with s < len (the others' columns are never read again);
//   nat_enc_gather_k  : enc[b][t][dir * D + j] = HS[dir][1 + (dir ? len-1-t : t)][j][b], zero at and beyond the length.
__global__ __launch_bounds__(256) void nat_enc_scatter_k(const float* __restrict__ x, const int* __restrict__ lengths, float* __restrict__ xt, int B, int Bp,
                                                         int Lmax, int D) {
    const int s = blockIdx.x, dir = blockIdx.z, D4 = D / 4;
    const size_t slab = (size_t)D * Bp;
    float4* __restrict__ dst = reinterpret_cast<float4*>(xt + ((size_t)dir * Lmax + s) * slab);
    for (int i = blockIdx.y * 256 + threadIdx.x; i < D4 * Bp; i += gridDim.y * 256) {
        const int k4 = i / Bp, b = i - k4 * Bp;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (b < B) {
            const int len = lengths[b];
            if (s < len) v = *reinterpret_cast<const float4*>(x + ((size_t)b * Lmax + (dir ? len - 1 - s : s)) * D + 4 * k4);
        }
        dst[i] = v;
    }
}
__global__ __launch_bounds__(256) void nat_enc_gather_k(const float* __restrict__ hs, const int* __restrict__ lengths, float* __restrict__ enc, int Bp,
                                                        int Lmax, int D) {
    const int t = blockIdx.x, b = blockIdx.y;
    const int len = lengths[b];
    const size_t slab = (size_t)D * Bp;
    for (int c = threadIdx.x; c < 2 * D; c += 256) {
        const int dir = c >= D, j = c - dir * D;
        float v = 0.0f;
        if (t < len) v = hs[((size_t)dir * (Lmax + 1) + 1 + (dir ? len - 1 - t : t)) * slab + nat_zidx(j, b, Bp)];
        enc[((size_t)b * Lmax + t) * 2 * D + c] = v;
    }
}

// Keep masks for the prenet's dropout drawn on the device: Threefry-2x32 with 20 rounds (Salmon et al., SC'11 — the
// block cipher jax.random is built on), key = the sentence's 64-bit seed, counter = (2 * frame + layer, 64-column block);
// the 64 output bits are the keep flags of 64 consecutive prenet columns (P(keep) = 1/2 = 1 - rate, model.py:97,99).
// This is a stream of our own (one seed per sentence, for batches of unrelated sentences); the reference's schedule from the
// checkpoint's rng is nat_keep_masks_haiku_k below.
__host__ __device__ __forceinline__ void threefry2x32_20(unsigned k0, unsigned k1, unsigned& x0, unsigned& x1) {
    const unsigned ks[3] = {k0, k1, 0x1BD11BDAu ^ k0 ^ k1};
    const int R[8] = {13, 15, 26, 6, 17, 29, 16, 24};
    x0 += ks[0];
    x1 += ks[1];
#pragma unroll
    for (int g = 0; g < 5; ++g) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int rot = R[(g & 1) * 4 + r];
            x0 += x1;
            x1 = (x1 << rot) | (x1 >> (32 - rot));
            x1 ^= x0;
        }
        x0 += ks[(g + 1) % 3];
        x1 += ks[(g + 2) % 3] + (unsigned)(g + 1);
    }
}
__global__ void nat_keep_masks_k(const unsigned long long* __restrict__ seeds, unsigned char* __restrict__ keep, int B, int Fmax, int PN) {
    const int nblk = (PN + 63) / 64;
    const size_t n = (size_t)B * Fmax * 2 * nblk;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int blk = (int)(i % nblk);
        const size_t fl = i / nblk;  // (b * Fmax + f) * 2 + layer
        const int b = (int)(fl / (2 * (size_t)Fmax));
        const unsigned ctr0 = (unsigned)(fl % (2 * (size_t)Fmax));
        const unsigned long long sd = seeds[b];
        unsigned x0 = ctr0, x1 = (unsigned)blk;
        threefry2x32_20((unsigned)sd, (unsigned)(sd >> 32), x0, x1);
        unsigned char* dst = keep + fl * PN + (size_t)blk * 64;
        for (int j = 0; j < 64 && blk * 64 + j < PN; ++j) dst[j] = (unsigned char)(((j < 32 ? x0 >> j : x1 >> (j - 32)) & 1u));
    }
}

// The REFERENCE's mask stream (jax.random's classic threefry layout under dm-haiku's PRNGSequence; restated in
// oracle/nat_oracle.py::haiku_prenet_keep_masks, which carries the derivation): K_0 = the checkpoint's rng,
// (K_n, S_n) = jax.random.split(K_{n-1}) = the cipher on counters (0, 2) and (1, 3), frame f takes S_{2f+1} / S_{2f+2}, and a mask of
// PN columns is uniform(S, (1, PN)) < 0.5: column c < half takes word x0 of counter (c, c + half), column half + c word x1
// (half = ceil(PN / 2)); keep <=> the word's top bit is clear.  Every sentence of a batch gets the same masks (the reference runs
// every sentence from the same checkpoint key).  One block per frame: its threads walk the key chain to frame f together (wave-
// uniform, <= 4 * (f + 1) ciphers), then thread (layer, c) draws its word and writes it to all B sentences.
// mode 1 = the layout of jax_threefry_partitionable=True (JAX >= 0.5's default; oracle/nat_oracle.py::jax_partitionable_*, restated from
// recollection of jax/_src/prng.py and NOT pinned by any known answer): split(key, 2)[i] = cipher(key, (0, i)) as the pair
// (y0, y1); a 32-bit draw of element c = y0 ^ y1 of cipher(S, (0, c)).
// Only the block's first wave walks the key chain (2 f + 2 splits, wave-uniform) and hands the frame's two subkeys to the others
// through LDS (round 2: every thread of the block walked it).
__global__ void nat_keep_masks_haiku_k(unsigned k0, unsigned k1, int mode, unsigned char* __restrict__ keep, int B, int Fmax, int PN) {
    __shared__ unsigned sub[4];  // s0[0], s1[0], s0[1], s1[1]
    const int f = blockIdx.x;
    if (threadIdx.x < 64) {
        unsigned ka = k0, kb = k1;
        for (int n = 0; n < 2 * f + 2; ++n) {
            unsigned a0, b0, a1, b1;
            if (mode == 0) {
                a0 = 0u, b0 = 2u, a1 = 1u, b1 = 3u;  // counts iota(4) in halves: pairs (0, 2), (1, 3)
                threefry2x32_20(ka, kb, a0, b0);
                threefry2x32_20(ka, kb, a1, b1);
                if (n >= 2 * f && threadIdx.x == 0) {  // [1] = (y1[0], y1[1]) is handed out
                    sub[2 * (n - 2 * f)] = b0;
                    sub[2 * (n - 2 * f) + 1] = b1;
                }
                ka = a0;  // split(key, 2)[0] = (y0[0], y0[1]) stays the sequence's key
                kb = a1;
            } else {
                a0 = 0u, b0 = 0u, a1 = 0u, b1 = 1u;  // subkey i = cipher(key, (0, i))
                threefry2x32_20(ka, kb, a0, b0);
                threefry2x32_20(ka, kb, a1, b1);
                if (n >= 2 * f && threadIdx.x == 0) {
                    sub[2 * (n - 2 * f)] = a1;
                    sub[2 * (n - 2 * f) + 1] = b1;
                }
                ka = a0;
                kb = b0;
            }
        }
    }
    __syncthreads();
    const int half = (PN + 1) / 2;
    for (int u = threadIdx.x; u < 2 * PN; u += blockDim.x) {
        const int layer = u / PN, c = u % PN;
        unsigned word;
        if (mode == 0) {
            const int i = c < half ? c : c - half;
            unsigned x0 = (unsigned)i, x1 = i + half < PN ? (unsigned)(i + half) : 0u;  // counters iota(PN) in two halves; an odd count is padded with one 0
            threefry2x32_20(sub[2 * layer], sub[2 * layer + 1], x0, x1);
            word = c < half ? x0 : x1;
        } else {
            unsigned x0 = 0u, x1 = (unsigned)c;
            threefry2x32_20(sub[2 * layer], sub[2 * layer + 1], x0, x1);
            word = x0 ^ x1;
        }
        const unsigned char kp = (word >> 31) ? 0 : 1;  // uniform = (word >> 9 | 1.0f) - 1 < 0.5  <=>  top bit clear
        for (int b = 0; b < B; ++b) keep[(((size_t)b * Fmax + f) * 2 + layer) * PN + c] = kp;
    }
}

// (Round 4 measured two restructurings of this kernel and kept neither: every weight fragment loaded ahead of its use, 16.3-18.7 -> 19.4 us, and
// 4-5 adjacent columns per thread to cut the LDS operand reads by four, 16.0 -> 20.0 us — the step is bound by one CU streaming the three
// matrices' 670 KB through its vector-memory path, ~5 us, plus three dependent phases: profiles/r04_e_nat_decoder_findings.md.)
// mel_f = [h1 ; h2] @ wp + bp, then the prenet of frame f + 1 into the other parity's state.  One
// 1024-thread workgroup per 4 sentences (weights read once per k for the four).  Every product is split over k into
// 1024 / width partial sums that are added in chunk order: a frame step is latency-bound, short dependent chains matter.
// POOL: every row at its own frame (NatFrameArg); an idle row of a live group is carried through the sums and stores nothing, so a slot's
// state stays what its reset made it until the row's first frame.
template <bool X3, bool POOL = false>  // X3: the state is the bf16x3 step's (two bf16 planes, nat_zxidx; `plane` elements apart); h = hi + lo exactly, p is split on its way out
__global__ __launch_bounds__(1024) void nat_dec_proj_prenet_k(const float* __restrict__ zcur, float* __restrict__ znext,
                                                              const int* __restrict__ nframes, const float4* __restrict__ f1, const float4* __restrict__ f2,
                                                              const float4* __restrict__ wp, const float* __restrict__ bp,
                                                              const unsigned char* __restrict__ keep, float* __restrict__ mel, NatFrameArg<POOL> fa, int B, int Bp,
                                                              int Fmax, int PN, int H, int MEL, size_t plane) {
    extern __shared__ float4 sq[];
    float4* hs = sq;              // [2H]   h1 ; h2 of the 4 sentences
    float4* part = hs + 2 * H;    // [1024] partial sums of the product in flight
    float4* prev = part + 1024;   // [MEL]
    float4* p1 = prev + MEL;      // [PN]
    const int g = threadIdx.x, b0 = blockIdx.x * 4;
    int nf[4], fs[4];  // the rows' frame counts and the frame each stands at
    bool live[4];
    bool any = false;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        nf[s] = b0 + s < B ? nframes[b0 + s] : 0;
        fs[s] = nat_row_frame(fa, b0 + s < B ? b0 + s : B - 1);
        live[s] = nat_row_live<POOL>(fs[s], nf[s]);
        any = any || live[s];
    }
    if (!any) return;
    // the projection's bias and the keep bytes of frame f + 1, requested before anything else (each was a cold load behind a barrier: 0.7 us of a step)
    const float bb_h = g < MEL ? bp[g] : 0.0f;
    unsigned char kp[2][4];
#pragma unroll
    for (int which = 0; which < 2; ++which)
#pragma unroll
        for (int s = 0; s < 4; ++s)
            kp[which][s] = (keep && g < PN && b0 + s < B && (!POOL || live[s]) && fs[s] + 1 < Fmax) ? keep[(((size_t)(b0 + s) * Fmax + fs[s] + 1) * 2 + which) * PN + g]
                                                                                                    : (unsigned char)1;
#pragma clang loop vectorize(disable)  // (it would pair the hi + lo additions of two rows into v_pk_add_f32: build.py)
    for (int k = g; k < 2 * H; k += 1024) {
        if constexpr (X3) {
            const unsigned short* __restrict__ zr = reinterpret_cast<const unsigned short*>(zcur) + nat_zxidx(PN + k, b0, Bp);  // sentences 8 elements apart
            float v[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) v[s] = __builtin_bit_cast(float, (unsigned)zr[8 * s] << 16) + __builtin_bit_cast(float, (unsigned)zr[plane + 8 * s] << 16);
            hs[k] = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            const float* __restrict__ zr = zcur + nat_zidx(PN + k, b0, Bp);  // state rows [p | h1 | h2]; the 4 sentences of a row are 16 bytes apart
            hs[k] = make_float4(zr[0], zr[4], zr[8], zr[12]);
        }
    }
    __syncthreads();
    // out[col] (4 sentences) = sum over chunk `ch` of rows [ch*per, (ch+1)*per) of src[row] * w[row][col]
    // weights in [row / 4][col][4] order (pack-time copies "…#k4"): one 16-byte load per lane = 4 consecutive rows of its
    // column, a wave's loads 1 KiB contiguous — dword loads made the step wait on the number of vector-memory instructions
    // a CU can issue (2 700 per workgroup and frame)
    auto partial = [&](const float4* __restrict__ src, const float4* __restrict__ w4, int rows, int width, int col, int ch, int per) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        const int k1 = (ch + 1) * per < rows ? (ch + 1) * per : rows;  // per and rows are multiples of 4
#pragma unroll 4
        for (int k = ch * per; k < k1; k += 4) {
            const float4 wv = w4[(size_t)(k >> 2) * width + col];
            const float4 x0 = src[k], x1 = src[k + 1], x2 = src[k + 2], x3 = src[k + 3];
            a.x = fmaf(x0.x, wv.x, a.x); a.y = fmaf(x0.y, wv.x, a.y); a.z = fmaf(x0.z, wv.x, a.z); a.w = fmaf(x0.w, wv.x, a.w);
            a.x = fmaf(x1.x, wv.y, a.x); a.y = fmaf(x1.y, wv.y, a.y); a.z = fmaf(x1.z, wv.y, a.z); a.w = fmaf(x1.w, wv.y, a.w);
            a.x = fmaf(x2.x, wv.z, a.x); a.y = fmaf(x2.y, wv.z, a.y); a.z = fmaf(x2.z, wv.z, a.z); a.w = fmaf(x2.w, wv.z, a.w);
            a.x = fmaf(x3.x, wv.w, a.x); a.y = fmaf(x3.y, wv.w, a.y); a.z = fmaf(x3.z, wv.w, a.z); a.w = fmaf(x3.w, wv.w, a.w);
        }
        return a;
    };
    auto gather = [&](float4 a, int width, int col, int nch) {
        for (int ch = 0; ch < nch; ++ch) {
            const float4 q = part[ch * width + col];
            a.x += q.x; a.y += q.y; a.z += q.z; a.w += q.w;
        }
        return a;
    };
    const int nchP = 1024 / MEL, perP = ((2 * H + nchP - 1) / nchP + 3) / 4 * 4;
    if (g < nchP * MEL) part[g] = partial(hs, wp, 2 * H, MEL, g % MEL, g / MEL, perP);
    __syncthreads();
    if (g < MEL) {
        const float bb = bb_h;
        const float4 a = gather(make_float4(bb, bb, bb, bb), MEL, g, nchP);
        prev[g] = a;
        const float v[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (live[s]) mel[((size_t)(b0 + s) * Fmax + fs[s]) * MEL + g] = v[s];
    }
    __syncthreads();
    if constexpr (POOL) {  // the next frame's prenet for the rows that have a next frame
        bool more = false;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            live[s] = live[s] && fs[s] + 1 < Fmax;
            more = more || live[s];
        }
        if (!more) return;
    } else {
        if (fs[0] + 1 >= Fmax) return;
    }
    auto masked = [&](float4 a, int which, int col) {  // relu, then hk.dropout(rate 0.5) with the given keep bytes of frame f + 1
        float v[4] = {fmaxf(a.x, 0.0f), fmaxf(a.y, 0.0f), fmaxf(a.z, 0.0f), fmaxf(a.w, 0.0f)};
        if (keep) {
#pragma unroll
            for (int s = 0; s < 4; ++s)
                if (b0 + s < B) v[s] = kp[which][s] ? v[s] * 2.0f : 0.0f;  // (col == g for both callers)
        }
        return make_float4(v[0], v[1], v[2], v[3]);
    };
    const int nchN = 1024 / PN;
    if (g < nchN * PN) part[g] = partial(prev, f1, MEL, PN, g % PN, g / PN, ((MEL + nchN - 1) / nchN + 3) / 4 * 4);
    __syncthreads();
    if (g < PN) p1[g] = masked(gather(make_float4(0.f, 0.f, 0.f, 0.f), PN, g, nchN), 0, g);
    __syncthreads();
    if (g < nchN * PN) part[g] = partial(p1, f2, PN, PN, g % PN, g / PN, ((PN + nchN - 1) / nchN + 3) / 4 * 4);
    __syncthreads();
    if (g < PN) {
        const float4 r = masked(gather(make_float4(0.f, 0.f, 0.f, 0.f), PN, g, nchN), 1, g);
        if constexpr (X3) {
            unsigned short* __restrict__ zw = reinterpret_cast<unsigned short*>(znext) + nat_zxidx(g, b0, Bp);
            const float v[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if (POOL && !live[s]) continue;
                const unsigned hp = vtts::pack_bf16x2(v[s], 0.0f);
                const unsigned lp = vtts::pack_bf16x2(v[s] - vtts::bf16_lo(hp), 0.0f);
                zw[8 * s] = (unsigned short)(hp & 0xffffu);
                zw[plane + 8 * s] = (unsigned short)(lp & 0xffffu);
            }
        } else {
            float* __restrict__ zw = znext + nat_zidx(g, b0, Bp);
            if constexpr (POOL) {
                const float v[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    if (live[s]) zw[4 * s] = v[s];
            } else {
                zw[0] = r.x; zw[4] = r.y; zw[8] = r.z; zw[12] = r.w;
            }
        }
    }
}

// (Round 6 cut the projection + prenet step along its WEIGHTS — a workgroup = a 32-sentence tile x a slice of a matrix, two launches per frame over 64-workgroup
//  grids, every load requested before the first wait — and measured it SLOWER: 6.7 + 24.0 us per frame against this kernel's 15.2, the acoustic model 17.0 ms against
//  12.5 (profiles/r06_c_nat_proj_prenet_findings.md).)
// ---- the TEACHER-FORCED pass: AcousticModel.__call__ (model.py:146-169), the forward vietTTS/nat/gta.py:28-40 runs to dump ground-truth-aligned mels ----
// The previous mel of every frame is the (shifted) TARGET mel, known before the loop.  So besides the conditioning's share of the gates, the prenet
// (two bias-free GEMMs over all B x F rows), the prenet's share of both LSTMs' gates (G_l += p @ W_l[E : E + PN]) and the mel projection leave the
// frame loop — all on nat_conv_mfma_k with one tap — and a frame is TWO launches of the step kernel below: K = H for layer 1 (its own state) and
// 2H for layer 2 (layer 1's fresh output, then its own state); the inference loop has PN + H and PN + 2H there, plus the projection / prenet launch.
// New in the step is zoneout, applied by the reference with is_training=False too (model.py:154-166): state = m * prev + (1 - m) * new for h and c of
// both layers (m in {0, 1}: a select), while the decoder OUTPUT [h1_new ; h2_new] — what layer 2 and the projection see — is not zoned out.
//
// nat_tf_lstm_k: nat_dec_lstm_k's tiling, operand order, K split and in-register cell update (the sums are the same chains in the same order: see the
// comments there), one operand set, SL = 1.  Its epilogue writes the un-zoned h to hseq [B][Fmax][2H] (the projection GEMM's input) and, for layer 1,
// to `hfresh` in state layout (layer 2's first H rows of this frame), and the zoned h / c to the recurrent state (h ping-pong by frame parity: the
// other workgroups of this launch still read the previous one).  Hidden state buffers are [H / 4][Bp][4] (nat_zidx), cell states [H][Bp].
// zone [B][Fmax][4][H] bytes (l0.h, l0.c, l1.h, l1.c; 1 = keep the previous state), nullptr = no zoneout.
struct NatTfOps {
    const float* inA;           // KA state rows (layer 2: layer 1's un-zoned output of this frame), then
    const float* inB;           // KB = H rows: the layer's own zoned hidden state of the previous frame
    const float4* wpk;          // [slice][K/8][lane][4]
    float* cst;                 // zoned cell state [H][Bp]
    float* hstate;              // zoned hidden state of this frame
    float* hfresh;              // un-zoned hidden state in state layout, or nullptr (layer 2: nobody reads it)
    float* hseq;                // un-zoned hidden state, [B][Fmax][2H] + layer * H
    const float* gin;           // this frame's hoisted gate pre-activations, accumulator order (NatLstmOps::gin)
    size_t gpitch;
    const unsigned char* zone;  // [B][Fmax][4][H] + 2 * layer * H, or nullptr
};
template <int NT, int KW>
__global__ __launch_bounds__(64 * KW) void nat_tf_lstm_k(NatTfOps ops, int KA, int KB, const int* __restrict__ nframes, int f, int B, int Bp, int H, int Fmax) {
    typedef float f32x16 __attribute__((ext_vector_type(16)));
    static_assert(KW == 2 || KW == 4 || KW == 8, "the K shares meet in LDS");
    __shared__ float red[KW][NT][16][64];
    const float* __restrict__ inA = ops.inA;
    const float* __restrict__ inB = ops.inB;
    const float4* __restrict__ wpk = ops.wpk;
    float* __restrict__ cst = ops.cst;
    const int lane = threadIdx.x & 63, kw = threadIdx.x >> 6, l31 = lane & 31, lh = lane >> 5;
    const int slice0 = blockIdx.x, b0 = blockIdx.y * 32 * NT;
    const int NIT = (KA + KB) / 8, NWMAX = (NIT + KW - 1) / KW, it_lo = kw * NWMAX;
    const int NW = it_lo >= NIT ? 0 : (NIT - it_lo < NWMAX ? NIT - it_lo : NWMAX);
    // this wave's cell-update blocks: previous cell and hidden state and the zoneout bytes are requested a kernel's length before they are needed
    constexpr int NBLK = (NT * 4 + KW - 1) / KW;
    float cold[NBLK], hold[NBLK];
    unsigned char zh[NBLK], zc[NBLK];
#pragma unroll
    for (int q = 0; q < NBLK; ++q) {
        const int blk = kw + q * KW, nt = (blk / 4) % NT, rq = blk % 4;
        const bool in = blk < NT * 4;
        const int u = 8 * slice0 + 2 * rq + lh, b = b0 + 32 * nt + l31;
        cold[q] = in ? cst[(size_t)u * Bp + b] : 0.0f;
        hold[q] = in ? inB[nat_zidx(u, b, Bp)] : 0.0f;
        const unsigned char* __restrict__ zp = ops.zone ? ops.zone + ((size_t)(b < B ? b : B - 1) * Fmax + f) * 4 * H + u : nullptr;
        zh[q] = (in && zp) ? zp[0] : (unsigned char)0;
        zc[q] = (in && zp) ? zp[H] : (unsigned char)0;
    }
    f32x16 acc[NT][2];
    if (kw == 0) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int b = b0 + 32 * nt + l31;
            const float4* __restrict__ gp = reinterpret_cast<const float4*>(ops.gin + (size_t)(b < B ? b : B - 1) * ops.gpitch + (size_t)(2 * slice0 + lh) * 16);
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                const float4 g4 = gp[rq];
                acc[nt][0][4 * rq + 0] = g4.x;
                acc[nt][0][4 * rq + 1] = g4.y;
                acc[nt][0][4 * rq + 2] = g4.z;
                acc[nt][0][4 * rq + 3] = g4.w;
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[nt][1][4 * rq + i] = 0.0f;
            }
        }
    } else {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc[nt][0][r] = 0.0f;
                acc[nt][1][r] = 0.0f;
            }
    }
    float4 wv[NAT_DEC_PD];
    float4 xv[NAT_DEC_PD][NT];
    const float4* __restrict__ wsl = wpk + (size_t)slice0 * NIT * 64 + lane;
    auto load_it = [&](int it, int slot) {
        if (it >= NIT) it = NIT - 1;  // tail: an in-bounds re-read, never used
        wv[slot] = wsl[(size_t)it * 64];
        const int k0 = it * 8;
        const float* __restrict__ xr = (k0 < KA ? inA + (size_t)k0 * Bp : inB + (size_t)(k0 - KA) * Bp) + ((size_t)lh * Bp + b0 + l31) * 4;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) xv[slot][nt] = *reinterpret_cast<const float4*>(xr + (size_t)(32 * nt) * 4);
    };
#pragma unroll
    for (int j = 0; j < NAT_DEC_PD; ++j) load_it(it_lo + j, j);
    bool live[NT];
    bool any = false;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int b = b0 + 32 * nt + l31;
        live[nt] = b < B && f < nframes[b < B ? b : B - 1];
        any = any || live[nt];
    }
    if (__ballot(any) == 0ull) return;  // every sentence of these tiles has all its frames (same for all waves)
#pragma nounroll
    for (int it0 = 0; it0 < NW; it0 += NAT_DEC_PD) {
#pragma unroll
        for (int j = 0; j < NAT_DEC_PD; ++j) {
            if (it0 + j >= NW) break;  // wave-uniform
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[j].x, xv[j][nt].x, acc[nt][0], 0, 0, 0);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[j].y, xv[j][nt].y, acc[nt][1], 0, 0, 0);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[j].z, xv[j][nt].z, acc[nt][0], 0, 0, 0);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[j].w, xv[j][nt].w, acc[nt][1], 0, 0, 0);
            const int nx = it0 + j + NAT_DEC_PD;
            load_it(nx < NW ? it_lo + nx : NIT, j);
        }
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) red[kw][nt][r][lane] = acc[nt][0][r] + acc[nt][1][r];
    __syncthreads();
#pragma unroll
    for (int blk = 0; blk < NT * 4; ++blk) {
        if (blk % KW != kw) continue;  // wave-uniform
        const int nt = (blk / 4) % NT, rq = blk % 4, q = blk / KW;
        float gs[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float v = red[0][nt][4 * rq + i][lane];
#pragma unroll
            for (int w = 1; w < KW; ++w) v += red[w][nt][4 * rq + i][lane];
            gs[i] = v;
        }
        if (!live[nt]) continue;  // frames past the sentence's last: neither state nor output is touched
        const int b = b0 + 32 * nt + l31, u = 8 * slice0 + 2 * rq + lh;
        const float cn = sigmoidf_(gs[2] + 1.0f) * cold[q] + sigmoidf_(gs[0]) * tanhf(gs[1]);
        const float hn = sigmoidf_(gs[3]) * tanhf(cn);
        ops.hseq[((size_t)b * Fmax + f) * 2 * H + u] = hn;
        if (ops.hfresh) ops.hfresh[nat_zidx(u, b, Bp)] = hn;
        cst[(size_t)u * Bp + b] = zc[q] ? cold[q] : cn;
        ops.hstate[nat_zidx(u, b, Bp)] = zh[q] ? hold[q] : hn;
    }
}

// The masks of the teacher-forced pass as the REFERENCE draws them (model.py:149 -> :95-100, :162-165): six subkeys S_1 .. S_6 of the chain
// (K_n, S_n) = split(K_{n-1}) from the checkpoint's rng (walked on the host: 12 ciphers), each ONE draw over a whole [B][F][D] tensor — S_1, S_2
// the prenet's keep masks (uniform < 0.5, D = PN), S_3 .. S_6 bernoulli(0.1) for l0.h, l0.c, l1.h, l1.c (D = H).  Element i of n = B F D (row-major)
// in jax.random's classic layout: word x0 of the counter pair (i, i + half) for i < half = n / 2, else word x1 of (i - half, i); jax pads an odd n
// with one zero count, which cannot occur here (PN and H are multiples of 32).  uniform = bitcast((word >> 9) | 0x3F800000) - 1.0f, compared in fp32 as jax does.  A row's masks therefore depend
// on B, F and its row index.  mode 1 = jax_threefry_partitionable (word = y0 ^ y1 of the cipher on the 64-bit index; unpinned, as in
// nat_keep_masks_haiku_k).  One thread per mask byte.
struct NatTeacherKeys {
    unsigned k[6][2];
};
__global__ void nat_teacher_masks_k(NatTeacherKeys keys, int mode, unsigned char* __restrict__ keep, unsigned char* __restrict__ zone, int B, int F, int PN, int H) {
    const size_t rows = (size_t)B * F, per = 2 * (size_t)PN + 4 * (size_t)H, total = rows * per;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const size_t row = idx / per;
        int r = (int)(idx % per), d, c, D;
        unsigned char* dst;
        if (r < 2 * PN) {
            d = r / PN, c = r % PN, D = PN;
            dst = keep + row * 2 * PN + r;
        } else {
            r -= 2 * PN;
            d = 2 + r / H, c = r % H, D = H;
            dst = zone + row * 4 * H + r;
        }
        const size_t n = rows * D, i = row * D + c;
        unsigned word;
        if (mode == 0) {
            const size_t half = n / 2, j = i < half ? i : i - half;  // n is even (D is a multiple of 32: create()), so jax's zero pad of an odd count never occurs
            unsigned x0 = (unsigned)j, x1 = (unsigned)(j + half);
            threefry2x32_20(keys.k[d][0], keys.k[d][1], x0, x1);
            word = i < half ? x0 : x1;
        } else {
            unsigned x0 = (unsigned)(i >> 32), x1 = (unsigned)i;
            threefry2x32_20(keys.k[d][0], keys.k[d][1], x0, x1);
            word = x0 ^ x1;
        }
        const float u = __builtin_bit_cast(float, (word >> 9) | 0x3F800000u) - 1.0f;
        *dst = (unsigned char)(u < (d < 2 ? 0.5f : 0.1f) ? 1 : 0);
    }
}

// ---- shared host-side sequence: TokenEncoder of `m` under module prefix `te` -> enc [B][Lmax][2D] ------------------
// scratch of the two encoder LSTMs: XT[2][Lmax], HS[2][Lmax + 1] slabs of [D][Bp] and the two cell states
size_t nat_enc_lstm_floats(int D, int B, int Lmax) {
    const size_t Bp = (size_t)(B + 63) / 64 * 64;
    return ((size_t)2 * Lmax + 2 * ((size_t)Lmax + 1) + 2) * D * Bp;
}
// A streaming session's frame window (vtts_nat_acoustic_stream_finish), in units of 4 channels.  Gather: win[b][p] = full[b][lo + p] for p < n, zeros for
// n <= p < W, and wl[b] = clamp(nframes[b] - lo, 0, n), the row's length inside the window.  Scatter: full[b][lo + p] = win[b][p] for k0 <= p < k1 where
// lo + p < nframes[b] (a row's frames past its end stay what the session's memset made them).
template <bool SCATTER>
__global__ __launch_bounds__(256) void nat_window_k(const float4* __restrict__ src, float4* __restrict__ dst, const int* __restrict__ nframes, int* __restrict__ wl,
                                                    int B, int Fmax, int W, int C4, int lo, int n, int k0, int k1) {
    const size_t gtid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    const int span = SCATTER ? k1 - k0 : W;
    const size_t total = (size_t)B * span * C4;
    for (size_t i = gtid; i < total; i += stride) {
        const int c = (int)(i % C4), p = k0 + (int)((i / C4) % span), b = (int)(i / ((size_t)C4 * span));
        const size_t fi = ((size_t)b * Fmax + lo + p) * C4 + c, wi = ((size_t)b * W + p) * C4 + c;
        if constexpr (SCATTER) {
            if (lo + p < nframes[b]) dst[fi] = src[wi];
        } else {
            dst[wi] = p < n ? src[fi] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    if constexpr (!SCATTER) {
        for (size_t b = gtid; b < (size_t)B; b += stride) {
            const int r = nframes[b] - lo;
            wl[b] = r < 0 ? 0 : (r > n ? n : r);
        }
    }
}

// ---- slot pool (vtts_nat_acoustic_pool_*): rows that start at any tick ----
// The pool's per-slot words, written on the device in stream order: the tick a slot's row was admitted at, its frame count (0 = idle) and its token count.
struct NatPoolMeta {
    int *start, *nframes, *lengths;  // [slots] each
};
// A slot as pool_admit() needs it, behind every tick enqueued so far: the slot's columns of both state parities and of both cell states zero (X3: the
// step's two bf16 planes per parity, nat_zxidx), its rows of the decoder's mel and of the caller's mel zero (C4 = Fmax * MEL / 4), its words set.
template <bool X3>
__global__ __launch_bounds__(256) void nat_pool_reset_k(float* __restrict__ dstate, float4* __restrict__ mel0, float4* __restrict__ mel, NatPoolMeta meta, int slot,
                                                        int start, int nframes, int length, int Bp, int ZW, int H, int C4) {
    const int gtid = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    const size_t zfloats = (size_t)ZW * Bp;
    for (int i = gtid; i < 2 * ZW; i += stride) {
        const int par = i / ZW, row = i % ZW;
        if constexpr (X3) {
            unsigned short* __restrict__ zx = reinterpret_cast<unsigned short*>(dstate + par * zfloats);
            zx[nat_zxidx(row, slot, Bp)] = 0;
            zx[zfloats + nat_zxidx(row, slot, Bp)] = 0;  // the lo plane: ZW * Bp bf16 elements behind the hi plane
        } else {
            dstate[par * zfloats + nat_zidx(row, slot, Bp)] = 0.0f;
        }
    }
    float* __restrict__ cst = dstate + 2 * zfloats;  // c1 [H][Bp], c2 [H][Bp]
    for (int i = gtid; i < 2 * H; i += stride) cst[(size_t)i * Bp + slot] = 0.0f;
    for (int i = gtid; i < C4; i += stride) {
        mel0[(size_t)slot * C4 + i] = make_float4(0.f, 0.f, 0.f, 0.f);
        mel[(size_t)slot * C4 + i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (gtid == 0) meta.start[slot] = start, meta.nframes[slot] = nframes, meta.lengths[slot] = length;
}
// pool_retire(): the slot's row decodes no further frame
__global__ void nat_pool_idle_k(NatPoolMeta meta, int slot) {
    if (blockIdx.x == 0 && threadIdx.x == 0) meta.nframes[slot] = 0;
}
// nat_window_k with a window per row (pool_finish()): list entry j is compact row r0 + j, the frames [lo, lo + n) of slot `slot`.  Gather: win[r0 + j][p] =
// full[slot][lo + p] for p < n, zeros for n <= p < W, and wl[r0 + j] = n.  Scatter: full[slot][lo + p] = win[r0 + j][p] for k0 <= p < k1 (the host has cut
// k1 at the row's last frame).  The list travels in the kernel's arguments, NAT_POOL_LIST rows a launch: no host memory is read in stream order.
constexpr int NAT_POOL_LIST = 48;
struct NatPoolWindows {
    int count, r0;
    int slot[NAT_POOL_LIST], lo[NAT_POOL_LIST], n[NAT_POOL_LIST], k0[NAT_POOL_LIST], k1[NAT_POOL_LIST];
};
template <bool SCATTER>
__global__ __launch_bounds__(256) void nat_pool_window_k(const float4* __restrict__ src, float4* __restrict__ dst, int* __restrict__ wl, NatPoolWindows L, int Fmax, int W,
                                                         int C4) {
    const size_t gtid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    const size_t total = (size_t)L.count * W * C4;
    for (size_t i = gtid; i < total; i += stride) {
        const int c = (int)(i % C4), p = (int)((i / C4) % W), j = (int)(i / ((size_t)C4 * W));
        const size_t fi = ((size_t)L.slot[j] * Fmax + L.lo[j] + p) * C4 + c, wi = ((size_t)(L.r0 + j) * W + p) * C4 + c;
        if constexpr (SCATTER) {
            if (p >= L.k0[j] && p < L.k1[j]) dst[fi] = src[wi];
        } else {
            dst[wi] = p < L.n[j] ? src[fi] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    if constexpr (!SCATTER) {
        for (size_t j = gtid; j < (size_t)L.count; j += stride) wl[L.r0 + j] = L.n[j];
    }
}

int run_token_encoder(const NatModel& m, const std::string& te, int V, int D, const int32_t* tokens, const int32_t* lengths, int B, int Lmax,
                      float* bufA, float* bufB, float* lstm_ws, float* enc, hipStream_t s) {
    hipLaunchKernelGGL(nat_embed_k, dim3(Lmax, B), dim3(256), 0, s, tokens, lengths, m.dev(te + "embed", "embeddings"), bufA, Lmax, D, V);
    constexpr int TL = 8;
    float* cur = bufA;
    float* nxt = bufB;
    for (int i = 0; i < 3; ++i) {
        const std::string sfx = i ? "_" + std::to_string(i) : "";
        const std::string cv = te + "conv1_d" + sfx, bn = te + "batch_norm" + sfx;
        hipLaunchKernelGGL((nat_conv_bn_act_k<3, TL>), dim3((Lmax + TL - 1) / TL, B), dim3(256), (TL + 2) * D * sizeof(float), s, cur, lengths,
                           m.dev(cv, "w"), m.dev(cv, "b"), m.inv(bn), m.dev(bn + "/~/mean_ema", "average"), m.dev(bn, "offset"), nullptr, nxt, Lmax,
                           D, D, (int)NAT_ACT_RELU);
        std::swap(cur, nxt);
    }
    {  // forward + backward hk.LSTM (model.py:39-46), every sentence and both directions per launch
        const int Bp = (B + 63) / 64 * 64;
        const size_t slab = (size_t)D * Bp;
        float* xt = lstm_ws;                                   // [2][Lmax] slabs
        float* hs = xt + 2 * (size_t)Lmax * slab;              // [2][Lmax + 1] slabs
        float* cs = hs + 2 * ((size_t)Lmax + 1) * slab;        // [2] slabs
        HIP_TRY(hipMemsetAsync(hs, 0, slab * 4, s));
        HIP_TRY(hipMemsetAsync(hs + ((size_t)Lmax + 1) * slab, 0, slab * 4, s));
        HIP_TRY(hipMemsetAsync(cs, 0, 2 * slab * 4, s));
        const int gy = (int)std::min<size_t>((slab / 4 + 255) / 256, 64);
        hipLaunchKernelGGL(nat_enc_scatter_k, dim3(Lmax, gy, 2), dim3(256), 0, s, cur, lengths, xt, B, Bp, Lmax, D);
        const bool wide = B > 32;  // two 32-sentence tiles per wave once there are that many sentences
        const dim3 lgrid(D / 8, wide ? Bp / 64 : 1, 2);
        NatLstmOps o[2];
        for (int dir = 0; dir < 2; ++dir) {
            const std::string mod = te + (dir ? "lstm_1/linear" : "lstm/linear");
            o[dir].wpk = m.extra<float4>(mod + "#mfma");
            o[dir].bias = m.dev(mod, "b");
            o[dir].cst = cs + dir * slab;
            o[dir].gin = nullptr;
            o[dir].gpitch = 0;
        }
        for (int st = 0; st < Lmax; ++st) {
            for (int dir = 0; dir < 2; ++dir) {
                o[dir].inA = xt + ((size_t)dir * Lmax + st) * slab;
                o[dir].inB = hs + ((size_t)dir * (Lmax + 1) + st) * slab;
                o[dir].hout = hs + ((size_t)dir * (Lmax + 1) + st + 1) * slab;
            }
            if (wide) hipLaunchKernelGGL((nat_dec_lstm_k<2, 8>), lgrid, dim3(512), 0, s, o[0], o[1], D, D, lengths, NatFrameArg<false>{st}, B, Bp, D);
            else hipLaunchKernelGGL((nat_dec_lstm_k<1, 8>), lgrid, dim3(512), 0, s, o[0], o[1], D, D, lengths, NatFrameArg<false>{st}, B, Bp, D);
        }
        hipLaunchKernelGGL(nat_enc_gather_k, dim3(Lmax, B), dim3(256), 0, s, hs, lengths, enc, Bp, Lmax, D);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return failf(VTTS_ERR_HIP, "token encoder launch failed: %s", hipGetErrorString(e));
    return VTTS_OK;
}

int check_encoder_dims(const char* what, int D, int V) {
    if (D < 64 || D > 256 || D % 64 != 0 || V < 1)
        return failf(VTTS_ERR_INVALID, "%s: encoder width must be 64, 128, 192 or 256 (one thread per channel in the convolutions) and vocab_size >= 1 (got %d, %d)",
                     what, D, V);
    return VTTS_OK;
}

// ---- workspaces: a layout is one walk over its buffers, each 256-byte aligned.  Over the caller's base pointer the walk yields the buffers, over
// nullptr only `bytes`, so the *_workspace_bytes entry points and the passes read the same statement. ----
struct NatCarver {
    char* base = nullptr;
    size_t bytes = 0;
    float* take(size_t n) {
        float* r = base ? reinterpret_cast<float*>(base + bytes) : nullptr;
        bytes += align_up(n, 256);
        return r;
    }
};
struct NatDurationWs : NatCarver {
    float *bufA, *bufB, *enc, *lstm_ws;
    NatDurationWs(const vtts_nat_duration_cfg& c, int B, int Lmax, void* ws) : NatCarver{static_cast<char*>(ws)} {
        const size_t BLD = (size_t)B * Lmax * c.lstm_dim * 4;
        bufA = take(BLD), bufB = take(BLD), enc = take(2 * BLD);  // two ping-pong [B][Lmax][D] buffers + the encoder output [B][Lmax][2D]
        lstm_ws = take(nat_enc_lstm_floats(c.lstm_dim, B, Lmax) * 4);
    }
};
// the resident decoder's share of the workspace (whether the option is set or not: a workspace sized once serves both paths): 256 bytes of polled
// words (arrival counter, abort word; development builds' phase clocks) in front, then the exchange buffer
constexpr size_t NAT_RES_WS_BYTES = 256 + (size_t)NAT_RES_XCH_ELEMS * 4 * sizeof(float);
static_assert(NAT_RES_WS_BYTES % 256 == 0, "workspace blocks are 256-byte aligned");
size_t nat_dec_state_floats(const vtts_nat_acoustic_cfg& c, int B) {
    const size_t Bp = (size_t)(B + 63) / 64 * 64, H = c.decoder_dim, ZW = 2 * H + c.prenet_dim;  // rows [p | h1 | h2]
    return (2 * ZW + 2 * H) * Bp;
}
struct NatAcousticWs : NatCarver {
    float *bufA, *bufB, *enc, *EG1, *EG2, *mel0, *pA, *pB, *dstate, *G1, *G2, *lstm_ws;
    unsigned* res_sync;
    NatAcousticWs() = default;
    NatAcousticWs(const vtts_nat_acoustic_cfg& c, int B, int Lmax, int Fmax, void* ws) : NatCarver{static_cast<char*>(ws)} {
        const size_t BLD = (size_t)B * Lmax * c.encoder_dim * 4, BF = (size_t)B * Fmax * 4, G = (size_t)4 * c.decoder_dim;
        bufA = take(BLD), bufB = take(BLD), enc = take(2 * BLD);           // encoder ping-pong + output
        EG1 = take((size_t)B * Lmax * G * 4), EG2 = take((size_t)B * Lmax * G * 4);  // enc @ W_l[0:E] per token
        mel0 = take(BF * c.mel_dim);                                       // decoder mel
        pA = take(BF * c.postnet_dim), pB = take(BF * c.postnet_dim);      // postnet ping-pong
        dstate = take(nat_dec_state_floats(c, B) * 4);                     // decoder state Z[2], c1, c2
        G1 = take(BF * G), G2 = take(BF * G);                              // hoisted gate pre-activations
        lstm_ws = take(nat_enc_lstm_floats(c.encoder_dim, B, Lmax) * 4);   // encoder LSTMs' scratch
        res_sync = reinterpret_cast<unsigned*>(take(NAT_RES_WS_BYTES));    // resident decoder: counters, exchange buffer
    }
};
// what the teacher-forced pass needs behind forward()'s layout `a`: the prenet's two layers, the hidden sequence, the recurrent state
struct NatTeacherWs : NatCarver {
    float *P1, *P2, *hseq, *tstate;
    NatTeacherWs(const NatAcousticWs& a, const vtts_nat_acoustic_cfg& c, int B, int Fmax) : NatCarver{a.base, a.bytes} {
        const size_t Bp = (size_t)(B + 63) / 64 * 64, H = c.decoder_dim, BF = (size_t)B * Fmax * 4;
        P1 = take(BF * c.prenet_dim), P2 = take(BF * c.prenet_dim), hseq = take(BF * 2 * H), tstate = take(7 * H * Bp * 4);
    }
};

// what a streaming session needs behind forward()'s layout `a`: the compact window [B][W][.] of the decoder's mel, of the postnet's ping-pong buffers and of
// its result, W = the widest window plus a halo per side, rounded up to the convolutions' 64-frame tiles, and the rows' lengths inside the window
struct NatStreamWs : NatCarver {
    float *wmel, *wpA, *wpB, *wout;
    int32_t* wl;
    int W;
    NatStreamWs(const NatAcousticWs& a, const vtts_nat_acoustic_cfg& c, int B, int Fmax, int max_window) : NatCarver{a.base, a.bytes} {
        W = (std::min(max_window, Fmax) + 2 * VTTS_NAT_POSTNET_HALO + 63) / 64 * 64;
        const size_t BW = (size_t)B * W * 4;
        wmel = take(BW * c.mel_dim), wpA = take(BW * c.postnet_dim), wpB = take(BW * c.postnet_dim), wout = take(BW * c.mel_dim);
        wl = reinterpret_cast<int32_t*>(take((size_t)B * 4));
    }
};

// what a slot pool needs behind a session's layout `s`: the per-slot words
struct NatPoolWs : NatCarver {
    NatPoolMeta meta;
    NatPoolWs(const NatStreamWs& s, int slots) : NatCarver{s.base, s.bytes} {
        int* w = reinterpret_cast<int*>(take((size_t)3 * slots * 4));
        meta = NatPoolMeta{w, w ? w + slots : nullptr, w ? w + 2 * slots : nullptr};
    }
};

}  // namespace

// ================================================ C ABI: duration model ================================================
VTTS_API int vtts_nat_duration_create(const vtts_nat_duration_cfg* cfg, int device, vtts_nat_duration** out) {
    if (!cfg || !out) return failf(VTTS_ERR_INVALID, "null argument");
    const int D = cfg->lstm_dim, V = cfg->vocab_size;
    if (int rc = check_encoder_dims("duration model", D, V)) return rc;
    auto* h = new (std::nothrow) vtts_nat_duration();
    if (!h) return failf(VTTS_ERR_NOMEM, "host allocation failed");
    h->what = "duration model";
    h->cfg = *cfg;
    h->device = device;
    h->add_token_encoder("token_encoder/~/", V, D);
    h->add("linear", "w", {2 * D, D});
    h->add("linear", "b", {D});
    h->add("linear_1", "w", {D, 1});
    h->add("linear_1", "b", {1});
    h->layout();
    *out = h;
    return VTTS_OK;
}
VTTS_API void vtts_nat_duration_destroy(vtts_nat_duration* h) { delete h; }
VTTS_API int vtts_nat_duration_num_params(const vtts_nat_duration* h, int* n) {
    if (!h || !n) return failf(VTTS_ERR_INVALID, "null argument");
    *n = (int)h->arrs.size();
    return VTTS_OK;
}
VTTS_API int vtts_nat_duration_param_info(const vtts_nat_duration* h, int i, const char** module, const char** name, int64_t shape[3], int* ndim) {
    if (!h) return failf(VTTS_ERR_INVALID, "null argument");
    return h->param_info(i, module, name, shape, ndim);
}
VTTS_API int vtts_nat_duration_set_param(vtts_nat_duration* h, const char* module, const char* name, const float* host, const int64_t* shape, int ndim) {
    if (!h) return failf(VTTS_ERR_INVALID, "null argument");
    return h->set_param(module, name, host, shape, ndim);
}
VTTS_API int vtts_nat_duration_packed_bytes(const vtts_nat_duration* h, size_t* bytes) {
    if (!h || !bytes) return failf(VTTS_ERR_INVALID, "null argument");
    *bytes = h->blob_bytes;
    return VTTS_OK;
}
VTTS_API int vtts_nat_duration_pack(vtts_nat_duration* h, void* dev_blob, size_t blob_bytes, void* stream) {
    if (!h) return failf(VTTS_ERR_INVALID, "null argument");
    return h->pack(dev_blob, blob_bytes, stream);
}
VTTS_API int vtts_nat_duration_bind_packed(vtts_nat_duration* h, void* dev_blob, size_t blob_bytes) {
    if (!h) return failf(VTTS_ERR_INVALID, "null argument");
    return h->bind(dev_blob, blob_bytes);
}
VTTS_API int vtts_nat_duration_workspace_bytes(const vtts_nat_duration* h, int B, int Lmax, size_t* bytes) {
    if (!h || !bytes) return failf(VTTS_ERR_INVALID, "null argument");
    if (B <= 0 || Lmax <= 0) return failf(VTTS_ERR_INVALID, "B and Lmax must be positive (got %d, %d)", B, Lmax);
    *bytes = NatDurationWs(h->cfg, B, Lmax, nullptr).bytes;
    return VTTS_OK;
}
VTTS_API int vtts_nat_duration_forward(vtts_nat_duration* h, const int32_t* tokens_dev, const int32_t* lengths_dev, int B, int Lmax,
                                       float* durations_dev, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h || !tokens_dev || !lengths_dev || !durations_dev) return failf(VTTS_ERR_INVALID, "null argument");
    if (!h->blob) return failf(VTTS_ERR_STATE, "forward() before pack()/bind_packed()");
    size_t need = 0;
    int rc = vtts_nat_duration_workspace_bytes(h, B, Lmax, &need);
    if (rc) return rc;
    if (!workspace || workspace_bytes < need) return failf(VTTS_ERR_NOMEM, "workspace too small: %zu < %zu bytes", workspace_bytes, need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int D = h->cfg.lstm_dim, V = h->cfg.vocab_size;
    const NatDurationWs ws(h->cfg, B, Lmax, workspace);
    rc = run_token_encoder(*h, "token_encoder/~/", V, D, tokens_dev, lengths_dev, B, Lmax, ws.bufA, ws.bufB, ws.lstm_ws, ws.enc, s);
    if (rc) return rc;
    hipLaunchKernelGGL(nat_duration_head_k, dim3(Lmax, B), dim3(D), (2 * D + 16) * sizeof(float), s, ws.enc, lengths_dev, h->dev("linear", "w"),
                       h->dev("linear", "b"), h->dev("linear_1", "w"), h->dev("linear_1", "b"), durations_dev, Lmax, D);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return failf(VTTS_ERR_HIP, "duration model launch failed: %s", hipGetErrorString(e));
    return VTTS_OK;
}

// ================================================ C ABI: acoustic model ================================================
VTTS_API int vtts_nat_acoustic_create(const vtts_nat_acoustic_cfg* cfg, int device, vtts_nat_acoustic** out) {
    if (!cfg || !out) return failf(VTTS_ERR_INVALID, "null argument");
    const int D = cfg->encoder_dim, V = cfg->vocab_size, H = cfg->decoder_dim, PN = cfg->prenet_dim, MEL = cfg->mel_dim, PD = cfg->postnet_dim;
    if (int rc = check_encoder_dims("acoustic model", D, V)) return rc;
    // decoder_dim in multiples of 256: nat_gates_mix_k takes the 4 * decoder_dim gate columns in chunks of 1024 (256 threads x 4 columns)
    if (H < 256 || H > 1024 || H % 256 != 0)
        return failf(VTTS_ERR_INVALID, "acoustic model: decoder_dim must be 256, 512, 768 or 1024 (the gate mix takes 4 * decoder_dim columns in chunks of 1024; got %d)", H);
    if (PN < 32 || PN % 32 != 0 || 2 * D + PN > 1024)
        return failf(VTTS_ERR_INVALID, "acoustic model: prenet_dim must be a multiple of 32 (matrix-core k-steps) with 2 * encoder_dim + prenet_dim <= 1024 (got %d, encoder_dim %d)", PN, D);
    if (MEL < 4 || MEL > 128 || MEL % 4 != 0) return failf(VTTS_ERR_INVALID, "acoustic model: mel_dim must be a multiple of 4 in 4 .. 128 (16-byte rows; got %d)", MEL);
    if (PD < 4 || PD > 1024 || PD % 4 != 0) return failf(VTTS_ERR_INVALID, "acoustic model: postnet_dim must be a multiple of 4 in 4 .. 1024 (16-byte rows; got %d)", PD);
    auto* h = new (std::nothrow) vtts_nat_acoustic();
    if (!h) return failf(VTTS_ERR_NOMEM, "host allocation failed");
    h->what = "acoustic model";
    h->cfg = *cfg;
    h->device = device;
    const int E = 2 * D, X = E + PN, G4 = 4 * H;
    h->add_token_encoder("token_encoder/~/", V, D);
    h->add("lstm/linear", "w", {X + H, 4 * H});          // decoder layer 1: [x ; h1]
    h->add("lstm/linear", "b", {4 * H});
    h->add("lstm_1/linear", "w", {X + H + H, 4 * H});    // decoder layer 2: [[x ; h1] ; h2]   (skip connection: input first)
    h->add("lstm_1/linear", "b", {4 * H});
    h->add("linear", "w", {2 * H, MEL});                 // projection of concat(h1, h2)
    h->add("linear", "b", {MEL});
    h->add("linear_1", "w", {MEL, PN});                  // prenet_fc1 (no bias)
    h->add("linear_2", "w", {PN, PN});                   // prenet_fc2 (no bias)
    for (int i = 0; i < 5; ++i) {
        const std::string sfx = i ? "_" + std::to_string(i) : "";
        const int cin = i == 0 ? MEL : PD, cout = i == 4 ? MEL : PD;
        h->add("conv1_d" + sfx, "w", {5, cin, cout});
        h->add("conv1_d" + sfx, "b", {cout});
        if (i < 4) h->add_bn("batch_norm" + sfx, PD);
    }
    // The kernels' private layouts behind the plain arrays (nat_model.h states each one at its packer), in the blob's order.
    // The postnet's convolutions for nat_conv_mfma_k, then their bf16 split for nat_conv_x3_k
    for (int x3 = 0; x3 < 2; ++x3)
        for (int i = 0; i < 5; ++i) {
            const std::string mod = "conv1_d" + (i ? "_" + std::to_string(i) : std::string());
            const int cin = i == 0 ? MEL : PD, cout = i == 4 ? MEL : PD;
            h->add_conv_frag(mod + (x3 ? "#x3" : "#mfma"), mod, x3, 5, 0, cin, cout, cout);
        }
    // projection and prenet matrices in [row / 4][col][4] order (nat_dec_proj_prenet_k: one 16-byte load = 4 rows of a column)
    for (const char* l : {"linear", "linear_1", "linear_2"}) {
        const std::string mod = l;
        const int rows = mod == "linear" ? 2 * H : (mod == "linear_1" ? MEL : PN), cols = mod == "linear" ? MEL : PN;
        h->add_extra(mod + "#k4", (size_t)rows * cols * sizeof(float), [mod, rows, cols](const NatModel& m, void* outv) {
            const float* W = m.host(mod, "w");
            float* out = static_cast<float*>(outv);
            for (int k = 0; k < rows; ++k)
                for (int c = 0; c < cols; ++c) out[((size_t)(k >> 2) * cols + c) * 4 + (k & 3)] = W[(size_t)k * cols + c];
        });
    }
    // The decoder's LSTMs.  Haiku's matrices are [cond ; p ; h1] (layer 1) and [cond ; p ; h1 ; h2] (layer 2: hk.deep_rnn_with_skip_connections puts the
    // network input first); the per-frame step multiplies the state rows [p ; h1] / [p ; h1 ; h2] = Haiku rows E + r ("#mfma", "#x3"), and the cond rows
    // [0, E) go into the GEMM ahead of the loop: "#cond" / "#cond#x3" = those rows as a one-tap convolution with the output columns in the step kernel's
    // accumulator order (nat_hcol), "#condb" = the bias in that order, "#zerob" = the zero bias of that GEMM (the mix adds the real one).
    const char* const lstm[2] = {"lstm/linear", "lstm_1/linear"};
    const std::vector<int> hcol = nat_hcol(H);
    for (int x3 = 0; x3 < 2; ++x3)
        for (int l = 0; l < 2; ++l) h->add_lstm_frag(std::string(lstm[l]) + (x3 ? "#x3" : "#mfma"), lstm[l], x3, PN + H + l * H, H, E);
    for (const std::string mod : lstm) {
        h->add_conv_frag(mod + "#cond", mod, false, 1, 0, E, G4, G4, hcol);
        h->add_extra(mod + "#condb", (size_t)G4 * sizeof(float), [mod, hcol](const NatModel& m, void* out) {
            const float* bv = m.host(mod, "b");
            for (size_t cp = 0; cp < hcol.size(); ++cp) static_cast<float*>(out)[cp] = bv[hcol[cp]];
        });
        h->add_conv_frag(mod + "#cond#x3", mod, true, 1, 0, E, G4, G4, hcol);
        h->add_zeros(mod + "#zerob", G4);
    }
    // The teacher-forced pass (nat_teacher_decoder): the step multiplies the recurrent rows only — "#tf" = Haiku rows E + PN + r, [h1] for layer 1 and
    // [h1 ; h2] for layer 2 — and everything known ahead of the loop is a one-tap nat_conv_mfma_k GEMM: "#pre" = the prenet's rows [E, E + PN) of the LSTM
    // matrices with the columns in accumulator order (as "#cond"), "linear_1#mfma" / "linear_2#mfma" the prenet's own matrices and "linear#mfma" the mel
    // projection, columns as they are.
    for (int l = 0; l < 2; ++l) h->add_lstm_frag(std::string(lstm[l]) + "#tf", lstm[l], false, H + l * H, H, E + PN);
    for (const std::string mod : lstm) h->add_conv_frag(mod + "#pre", mod, false, 1, E, PN, G4, G4, hcol);
    h->add_conv_frag("linear_1#mfma", "linear_1", false, 1, 0, MEL, PN, PN);
    h->add_conv_frag("linear_2#mfma", "linear_2", false, 1, 0, PN, PN, PN);
    h->add_conv_frag("linear#mfma", "linear", false, 1, 0, 2 * H, MEL, MEL);
    h->add_zeros("prenet#zerob", PN);
    h->layout();
    *out = h;
    return VTTS_OK;
}
VTTS_API void vtts_nat_acoustic_destroy(vtts_nat_acoustic* h) { delete h; }
static const char* const NAT_ACOUSTIC_OPTIONS = "bf16x3, resident, resident_grid, resident_used, stage_times, stage_gates_us, stage_decoder_us, stage_postnet_us";
VTTS_API int vtts_nat_acoustic_set_option(vtts_nat_acoustic* h, const char* key, int value) {
    if (!h || !key) return failf(VTTS_ERR_INVALID, "null argument");
    if (!strcmp(key, "bf16x3")) {
        if (value != 0 && value != 1) return failf(VTTS_ERR_INVALID, "bf16x3 must be 0 or 1 (got %d)", value);
        h->x3 = value;
        return VTTS_OK;
    }
    if (!strcmp(key, "resident")) {
        if (value != 0 && value != 1) return failf(VTTS_ERR_INVALID, "resident must be 0 or 1 (got %d)", value);
        h->resident = value;
        return VTTS_OK;
    }
    if (!strcmp(key, "resident_grid")) {
        if (value != 0 && value != 64 && value != 128 && value != 256) return failf(VTTS_ERR_INVALID, "resident_grid must be 0, 64, 128 or 256 (got %d)", value);
        h->resident_grid = value;
        return VTTS_OK;
    }
    if (!strcmp(key, "stage_times")) {
        if (value != 0 && value != 1) return failf(VTTS_ERR_INVALID, "stage_times must be 0 or 1 (got %d)", value);
        h->stage_times = value;
        h->stage_valid = 0;
        return VTTS_OK;
    }
    if (!strcmp(key, "resident_used") || !strncmp(key, "stage_", 6)) return failf(VTTS_ERR_INVALID, "%s is read-only", key);
    return failf(VTTS_ERR_INVALID, "unknown option '%s' (known: %s)", key, NAT_ACOUSTIC_OPTIONS);
}
VTTS_API int vtts_nat_acoustic_get_option(const vtts_nat_acoustic* h, const char* key, int* value) {
    if (!h || !key || !value) return failf(VTTS_ERR_INVALID, "null argument");
    if (!strcmp(key, "bf16x3")) {
        *value = h->x3;
        return VTTS_OK;
    }
    if (!strcmp(key, "resident") || !strcmp(key, "resident_grid") || !strcmp(key, "resident_used")) {
        *value = !strcmp(key, "resident") ? h->resident : !strcmp(key, "resident_grid") ? h->resident_grid : h->resident_used;
        return VTTS_OK;
    }
    if (!strcmp(key, "stage_times")) {
        *value = h->stage_times;
        return VTTS_OK;
    }
    const int stage = !strcmp(key, "stage_gates_us") ? 0 : !strcmp(key, "stage_decoder_us") ? 1 : !strcmp(key, "stage_postnet_us") ? 2 : -1;
    if (stage >= 0) {
        if (!h->stage_valid) return failf(VTTS_ERR_STATE, "%s: no forward() with the option stage_times set has run", key);
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, h->ev_stage[stage], h->ev_stage[stage + 1]));  // (hipErrorNotReady before the caller has synchronised)
        *value = (int)(ms * 1000.0f + 0.5f);
        return VTTS_OK;
    }
    return failf(VTTS_ERR_INVALID, "unknown option '%s' (known: %s)", key, NAT_ACOUSTIC_OPTIONS);
}
VTTS_API int vtts_nat_acoustic_resident_status(vtts_nat_acoustic* h, int* timed_out) {
    if (!h || !timed_out) return failf(VTTS_ERR_INVALID, "null argument");
    if (!h->res_sync) return failf(VTTS_ERR_STATE, "resident_status(): this handle has not launched the resident decoder");
    unsigned words[2 + 2 * 10] = {};
    HIP_TRY(hipMemcpy(words, h->res_sync, VTTS_TIMELINE ? sizeof(words) : 2 * sizeof(unsigned), hipMemcpyDeviceToHost));
    *timed_out = words[1] != 0u;
#if VTTS_TIMELINE  // kernel-development builds: the phase clocks of workgroup 0 (10 ns ticks, summed over the frames)
    unsigned long long tl[10];
    memcpy(tl, words + 2, sizeof(tl));
    fprintf(stderr, "nat_dec_resident_k timeline [wait1 lstm1 wait2 lstm2 wait3 proj wait4 prenet1 wait5 prenet2] x 10 ns:");
    for (int i = 0; i < 10; ++i) fprintf(stderr, " %llu", tl[i]);
    fprintf(stderr, "\n");
#endif
    return VTTS_OK;
}
VTTS_API int vtts_nat_acoustic_num_params(const vtts_nat_acoustic* h, int* n) {
    if (!h || !n) return failf(VTTS_ERR_INVALID, "null argument");
    *n = (int)h->arrs.size();
    return VTTS_OK;
}
VTTS_API int vtts_nat_acoustic_param_info(const vtts_nat_acoustic* h, int i, const char** module, const char** name, int64_t shape[3], int* ndim) {
    if (!h) return failf(VTTS_ERR_INVALID, "null argument");
    return h->param_info(i, module, name, shape, ndim);
}
VTTS_API int vtts_nat_acoustic_set_param(vtts_nat_acoustic* h, const char* module, const char* name, const float* host, const int64_t* shape, int ndim) {
    if (!h) return failf(VTTS_ERR_INVALID, "null argument");
    return h->set_param(module, name, host, shape, ndim);
}
VTTS_API int vtts_nat_acoustic_packed_bytes(const vtts_nat_acoustic* h, size_t* bytes) {
    if (!h || !bytes) return failf(VTTS_ERR_INVALID, "null argument");
    *bytes = h->blob_bytes;
    return VTTS_OK;
}
VTTS_API int vtts_nat_acoustic_pack(vtts_nat_acoustic* h, void* dev_blob, size_t blob_bytes, void* stream) {
    if (!h) return failf(VTTS_ERR_INVALID, "null argument");
    return h->pack(dev_blob, blob_bytes, stream);
}
VTTS_API int vtts_nat_acoustic_bind_packed(vtts_nat_acoustic* h, void* dev_blob, size_t blob_bytes) {
    if (!h) return failf(VTTS_ERR_INVALID, "null argument");
    return h->bind(dev_blob, blob_bytes);
}
VTTS_API int vtts_nat_acoustic_workspace_bytes(const vtts_nat_acoustic* h, int B, int Lmax, int Fmax, size_t* bytes) {
    if (!h || !bytes) return failf(VTTS_ERR_INVALID, "null argument");
    if (B <= 0 || Lmax <= 0 || Fmax <= 0) return failf(VTTS_ERR_INVALID, "B, Lmax and Fmax must be positive (got %d, %d, %d)", B, Lmax, Fmax);
    *bytes = NatAcousticWs(h->cfg, B, Lmax, Fmax, nullptr).bytes;
    return VTTS_OK;
}
VTTS_API int vtts_nat_acoustic_forward_teacher_workspace_bytes(const vtts_nat_acoustic* h, int B, int Lmax, int Fmax, size_t* bytes) {
    if (int rc = vtts_nat_acoustic_workspace_bytes(h, B, Lmax, Fmax, bytes)) return rc;
    *bytes = NatTeacherWs(NatAcousticWs(h->cfg, B, Lmax, Fmax, nullptr), h->cfg, B, Fmax).bytes;
    return VTTS_OK;
}
VTTS_API int vtts_nat_acoustic_keep_masks(const vtts_nat_acoustic* h, const uint64_t* seeds_dev, int B, int Fmax, uint8_t* keep_dev, void* stream) {
    if (!h || !seeds_dev || !keep_dev) return failf(VTTS_ERR_INVALID, "null argument");
    if (B <= 0 || Fmax <= 0) return failf(VTTS_ERR_INVALID, "B and Fmax must be positive (got %d, %d)", B, Fmax);
    const int PN = h->cfg.prenet_dim;
    const size_t n = (size_t)B * Fmax * 2 * ((PN + 63) / 64);
    const int blocks = (int)((n + 255) / 256 < 65535 ? (n + 255) / 256 : 65535);
    hipLaunchKernelGGL(nat_keep_masks_k, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), reinterpret_cast<const unsigned long long*>(seeds_dev),
                       keep_dev, B, Fmax, PN);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return failf(VTTS_ERR_HIP, "keep-mask launch failed: %s", hipGetErrorString(e));
    return VTTS_OK;
}
VTTS_API int vtts_nat_acoustic_keep_masks_haiku_mode(const vtts_nat_acoustic* h, uint32_t rng_key0, uint32_t rng_key1, int threefry_partitionable, int B, int Fmax,
                                                     uint8_t* keep_dev, void* stream) {
    if (!h || !keep_dev) return failf(VTTS_ERR_INVALID, "null argument");
    if (B <= 0 || Fmax <= 0) return failf(VTTS_ERR_INVALID, "B and Fmax must be positive (got %d, %d)", B, Fmax);
    if (threefry_partitionable != 0 && threefry_partitionable != 1) return failf(VTTS_ERR_INVALID, "threefry_partitionable must be 0 (classic layout) or 1");
    const int PN = h->cfg.prenet_dim;
    const int threads = 2 * PN < 1024 ? (2 * PN < 64 ? 64 : 2 * PN) : 1024;
    hipLaunchKernelGGL(nat_keep_masks_haiku_k, dim3(Fmax), dim3(threads), 0, static_cast<hipStream_t>(stream), rng_key0, rng_key1, threefry_partitionable,
                       keep_dev, B, Fmax, PN);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return failf(VTTS_ERR_HIP, "keep-mask launch failed: %s", hipGetErrorString(e));
    return VTTS_OK;
}
VTTS_API int vtts_nat_acoustic_keep_masks_haiku(const vtts_nat_acoustic* h, uint32_t rng_key0, uint32_t rng_key1, int B, int Fmax, uint8_t* keep_dev,
                                                void* stream) {
    return vtts_nat_acoustic_keep_masks_haiku_mode(h, rng_key0, rng_key1, 0, B, Fmax, keep_dev, stream);
}
VTTS_API int vtts_nat_acoustic_teacher_masks_haiku(const vtts_nat_acoustic* h, uint32_t rng_key0, uint32_t rng_key1, int threefry_partitionable, int B, int F,
                                                   uint8_t* keep_dev, uint8_t* zone_dev, void* stream) {
    if (!h || !keep_dev || !zone_dev) return failf(VTTS_ERR_INVALID, "null argument");
    if (B <= 0 || F <= 0) return failf(VTTS_ERR_INVALID, "B and F must be positive (got %d, %d)", B, F);
    if (threefry_partitionable != 0 && threefry_partitionable != 1) return failf(VTTS_ERR_INVALID, "threefry_partitionable must be 0 (classic layout) or 1");
    const int PN = h->cfg.prenet_dim, H = h->cfg.decoder_dim;
    if ((size_t)B * F * (size_t)(PN > H ? PN : H) >= ((size_t)1 << 31)) return failf(VTTS_ERR_INVALID, "a mask draw of %d x %d frames exceeds 2^31 elements", B, F);
    NatTeacherKeys keys;
    unsigned ka = rng_key0, kb = rng_key1;
    for (int n = 0; n < 6; ++n) {  // (K_n, S_n) = jax.random.split(K_{n-1}): as nat_keep_masks_haiku_k walks it
        unsigned a0, b0, a1, b1;
        if (threefry_partitionable == 0) {
            a0 = 0u, b0 = 2u, a1 = 1u, b1 = 3u;
            threefry2x32_20(ka, kb, a0, b0);
            threefry2x32_20(ka, kb, a1, b1);
            keys.k[n][0] = b0, keys.k[n][1] = b1;
            ka = a0, kb = a1;
        } else {
            a0 = 0u, b0 = 0u, a1 = 0u, b1 = 1u;
            threefry2x32_20(ka, kb, a0, b0);
            threefry2x32_20(ka, kb, a1, b1);
            keys.k[n][0] = a1, keys.k[n][1] = b1;
            ka = a0, kb = b0;
        }
    }
    const size_t total = (size_t)B * F * (2 * (size_t)PN + 4 * (size_t)H);
    const int blocks = (int)((total + 255) / 256 < 65535 ? (total + 255) / 256 : 65535);
    hipLaunchKernelGGL(nat_teacher_masks_k, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), keys, threefry_partitionable, keep_dev, zone_dev, B, F, PN, H);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return failf(VTTS_ERR_HIP, "teacher-mask launch failed: %s", hipGetErrorString(e));
    return VTTS_OK;
}
namespace {

// One call of the acoustic model: the entry point's arguments, then what nat_validate() derives from them.
struct NatCall {
    vtts_nat_acoustic* h;
    const int32_t *tokens, *lengths;
    const float* durations;
    const int32_t* nframes;
    int B, Lmax, Fmax;
    const uint8_t* keep;
    float* mel;
    void* workspace;
    size_t workspace_bytes;
    hipStream_t s;
    int ngroups = 0;  // forward_groups(); 0 is the plain call (the postnet on the caller's stream after the last frame)
    const int32_t *group_row0 = nullptr, *group_frames = nullptr;
    const float* enc_pre = nullptr;    // the token encoder's output [B][Lmax][2D] computed ahead by vtts_nat_acoustic_encode() (tokens is not read then)
    // forward_teacher(): [B][Fmax][MEL] target mels (the one-frame shift happens here), zone masks [B][Fmax][4][H] or nullptr, and optionally where the
    // decoder's mel before the postnet residual goes
    const float* mels = nullptr;
    const uint8_t* zone = nullptr;
    float* mel_pre = nullptr;
    int H = 0, PN = 0, MEL = 0, PD = 0, E = 0, G4 = 0, Bp = 0, mtiles = 0;  // mtiles: the gate mix's tiles of NAT_MIX_FT frames
    NatAcousticWs ws;
};

// what a call's dimensions and workspace pointer give: the model's widths, the padded batch, the mix's tiles and the workspace's buffers
void nat_derive(NatCall& c) {
    const vtts_nat_acoustic* h = c.h;
    c.H = h->cfg.decoder_dim, c.PN = h->cfg.prenet_dim, c.MEL = h->cfg.mel_dim, c.PD = h->cfg.postnet_dim;
    c.E = 2 * h->cfg.encoder_dim, c.G4 = 4 * c.H, c.Bp = (c.B + 63) / 64 * 64, c.mtiles = (c.Fmax + NAT_MIX_FT - 1) / NAT_MIX_FT;
    c.ws = NatAcousticWs(h->cfg, c.B, c.Lmax, c.Fmax, c.workspace);
}

int nat_validate(NatCall& c) {
    vtts_nat_acoustic* h = c.h;
    if (!h || (!c.tokens && !c.enc_pre) || !c.lengths || !c.durations || !c.nframes || !c.mel) return failf(VTTS_ERR_INVALID, "null argument");
    if (!h->blob) return failf(VTTS_ERR_STATE, "forward() before pack()/bind_packed()");
    size_t need = 0;
    int rc = c.mels ? vtts_nat_acoustic_forward_teacher_workspace_bytes(h, c.B, c.Lmax, c.Fmax, &need) : vtts_nat_acoustic_workspace_bytes(h, c.B, c.Lmax, c.Fmax, &need);
    if (rc) return rc;
    if (!c.workspace || c.workspace_bytes < need) return failf(VTTS_ERR_NOMEM, "workspace too small: %zu < %zu bytes", c.workspace_bytes, need);
    if (c.mels && h->x3) return failf(VTTS_ERR_INVALID, "forward_teacher() has fp32 products only: clear the option bf16x3 (there is no split-operand teacher-forced step)");
    if (c.Lmax > 2048) return failf(VTTS_ERR_INVALID, "at most 2048 tokens per sentence (upsampling weights live in LDS)");
    h->groups_valid = 0;
    if (c.ngroups > 0) {
        if (!c.group_row0 || !c.group_frames) return failf(VTTS_ERR_INVALID, "null argument");
        if (c.ngroups > 64) return failf(VTTS_ERR_INVALID, "at most 64 groups (got %d)", c.ngroups);
        if (c.group_row0[0] != 0 || c.group_row0[c.ngroups] != c.B) return failf(VTTS_ERR_INVALID, "the groups must cover rows [0, %d)", c.B);
        for (int g = 0; g < c.ngroups; ++g)
            if (c.group_row0[g + 1] <= c.group_row0[g] || c.group_frames[g] < 1 || c.group_frames[g] > c.Fmax)
                return failf(VTTS_ERR_INVALID, "group %d: rows [%d, %d), %d frames (every group needs at least one row and 1 <= frames <= Fmax = %d)", g,
                             c.group_row0[g], c.group_row0[g + 1], c.group_frames[g], c.Fmax);
    }
    nat_derive(c);
    return VTTS_OK;
}

// the side stream and the events of the hand-over (created once per handle, on the device the caller made current)
int nat_side_stream(vtts_nat_acoustic* h, int ngroups) {
    if (!h->side) {
        HIP_TRY(hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&h->ev_gates, hipEventDisableTiming));
    }
    while ((int)h->ev_dec.size() < ngroups) {
        hipEvent_t a, b;
        HIP_TRY(hipEventCreateWithFlags(&a, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&b, hipEventDisableTiming));
        h->ev_dec.push_back(a);
        h->ev_done.push_back(b);
    }
    return VTTS_OK;
}

// One launch of nat_conv_mfma_k, or with x3 of nat_conv_x3_k (w = the "#x3" fragments then), over `nrows` sentences and the first `npos` of their
// `pitch` positions: y[b][t] = epilogue(act(conv(x[b])[t] + bias)) for t < rows[b], epilogue TF as described at the kernel.  A workgroup takes 64 positions
// x 4 waves x MR blocks of 32 output channels, MR = 2 from 8 blocks on.  One tap makes it a GEMM over a sentence's positions.
// The split-operand kernel has no TF epilogue, and of its one-tap form only MR = 2 is built: its one user, the gate GEMM, has 4H / 32 >= 32 blocks.
struct NatConv {
    int nrows, npos, pitch;
    const int32_t* rows;
    const float* x;
    float* y;
    const float *w, *bias;
    int cin, cout, act;
    const uint8_t* keep = nullptr;
    const float *inv = nullptr, *mean = nullptr, *offset = nullptr, *res = nullptr;
};
template <int K, int TF = 0>
void nat_conv(const NatConv& o, bool x3, hipStream_t s) {
    const int MB = (o.cout + 31) / 32;
    auto launch = [&](auto mr) {
        constexpr int MR = decltype(mr)::value;
        const dim3 grid((o.npos + 63) / 64, (MB + 4 * MR - 1) / (4 * MR), o.nrows);
        if constexpr (TF == 0 && (K == 5 || MR == 2)) {
            if (x3) {
                hipLaunchKernelGGL((nat_conv_x3_k<K, MR>), grid, dim3(256), 0, s, o.x, o.rows, reinterpret_cast<const uint4*>(o.w), o.bias, o.inv, o.mean, o.offset,
                                   o.res, o.y, o.pitch, o.cin, o.cout, o.act, 0);
                return;
            }
        }
        if constexpr (K == 5 && TF == 0) {
            if (o.cin > 512) {  // chains of more than 5 x 512 terms: folded every 8 steps (FOLD at the kernel)
                hipLaunchKernelGGL((nat_conv_mfma_k<K, MR, TF, 1>), grid, dim3(256), 0, s, o.x, o.rows, reinterpret_cast<const float4*>(o.w), o.bias, o.inv, o.mean,
                                   o.offset, o.res, o.y, o.pitch, o.cin, o.cout, o.act, 0, o.keep);
                return;
            }
        }
        hipLaunchKernelGGL((nat_conv_mfma_k<K, MR, TF>), grid, dim3(256), 0, s, o.x, o.rows, reinterpret_cast<const float4*>(o.w), o.bias, o.inv, o.mean, o.offset,
                           o.res, o.y, o.pitch, o.cin, o.cout, o.act, 0, o.keep);
    };
    if (MB >= 8) launch(std::integral_constant<int, 2>{});
    else launch(std::integral_constant<int, 1>{});
}

// The conditioning's share of both layers' gates for every frame, G_l = b_l + cond @ W_l[0:E]: the GEMM over the tokens' rows, then the mix over the
// frames (:132, the upsampling, lives inside it: cond is never materialised).  The first `mfirst` of its tiles run on the
// caller's stream, the rest beside it on the side stream, ev_gates behind them.
int nat_cond_gates(const NatCall& c, int mfirst) {
    vtts_nat_acoustic* h = c.h;
    if (c.G4 % 1024 != 0) return failf(VTTS_ERR_INVALID, "decoder_dim %d: create() admits multiples of 256 only (the gate mix takes 4 * decoder_dim in chunks of 1024)", c.H);
    for (int l = 0; l < 2; ++l) {
        const std::string mod = l ? "lstm_1/linear" : "lstm/linear";
        nat_conv<1>(NatConv{c.B, c.Lmax, c.Lmax, c.lengths, c.ws.enc, l ? c.ws.EG2 : c.ws.EG1, h->extra(mod + (h->x3 ? "#cond#x3" : "#cond")), h->extra(mod + "#zerob"),
                            c.E, c.G4, (int)NAT_ACT_NONE}, h->x3, c.s);
    }
    const size_t mlds = ((size_t)(c.Lmax + 3) / 4 * 4 + (size_t)c.Lmax * NAT_MIX_FT) * sizeof(float);
    if (mlds > 48 * 1024)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&nat_gates_mix_k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)mlds));
    const float *b1 = h->extra("lstm/linear#condb"), *b2 = h->extra("lstm_1/linear#condb");
    auto mix = [&](int tile0, int ntiles, hipStream_t gs) {
        hipLaunchKernelGGL(nat_gates_mix_k, dim3(ntiles, 2 * (c.G4 / 1024), c.B), dim3(256), mlds, gs, c.ws.EG1, c.ws.EG2, b1, b2, c.lengths, c.durations,
                           c.nframes, c.ws.G1, c.ws.G2, c.Lmax, c.Fmax, c.G4, tile0);
    };
    mix(0, mfirst, c.s);
    if (c.mtiles > mfirst) {
        HIP_TRY(hipEventRecord(h->ev_fork, c.s));
        HIP_TRY(hipStreamWaitEvent(h->side, h->ev_fork, 0));
        mix(mfirst, c.mtiles - mfirst, h->side);
        HIP_TRY(hipEventRecord(h->ev_gates, h->side));
    }
    return VTTS_OK;
}

// postnet (:113-121) + residual (:151) of rows [r0, r1) over their first `frames` frames: 4 x (Conv1D(PD, 5) + BatchNorm + tanh),
// Conv1D(MEL, 5), mel + .   A row's result does not depend on the launch it is part of.
// The five launches over `nrows` rows of `pitch` positions, the first `npos` of them computed and rows[b] of them real: in = the decoder's mel (the first
// layer's input and the residual), pp = the ping-pong buffers, out = the result.
struct NatPostnetBufs {
    int nrows, npos, pitch;
    const int32_t* rows;
    const float* in;
    float* pp[2];
    float* out;
};
void nat_postnet_run(const NatCall& c, const NatPostnetBufs& p, hipStream_t ps) {
    const vtts_nat_acoustic* h = c.h;
    const float* cur = p.in;
    for (int i = 0; i < 5; ++i) {
        const std::string sfx = i ? "_" + std::to_string(i) : "";
        const std::string cv = "conv1_d" + sfx, bn = "batch_norm" + sfx;
        const bool last = i == 4;
        NatConv o{p.nrows, p.npos, p.pitch, p.rows, cur, last ? p.out : p.pp[i & 1], h->extra(cv + (h->x3 ? "#x3" : "#mfma")), h->dev(cv, "b"),
                  i == 0 ? c.MEL : c.PD, last ? c.MEL : c.PD, last ? (int)NAT_ACT_NONE : (int)NAT_ACT_TANH};
        if (last) o.res = p.in;
        else o.inv = h->inv(bn), o.mean = h->dev(bn + "/~/mean_ema", "average"), o.offset = h->dev(bn, "offset");
        nat_conv<5>(o, h->x3, ps);
        cur = o.y;
    }
}
void nat_postnet(const NatCall& c, int r0, int r1, int frames, hipStream_t ps) {
    const size_t m0 = (size_t)r0 * c.Fmax * c.MEL, p0 = (size_t)r0 * c.Fmax * c.PD;
    nat_postnet_run(c, NatPostnetBufs{r1 - r0, frames, c.Fmax, c.nframes + r0, c.ws.mel0 + m0, {c.ws.pA + p0, c.ws.pB + p0}, c.mel + m0}, ps);
}

// teacher-forced decoder (model.py:146-167): everything but the two LSTMs' recurrent products ahead of the frame loop
int nat_teacher_decoder(const NatCall& c) {
    const vtts_nat_acoustic* h = c.h;
    const NatAcousticWs& ws = c.ws;
    const NatTeacherWs tw(ws, h->cfg, c.B, c.Fmax);
    const int B = c.B, Bp = c.Bp, Fmax = c.Fmax, H = c.H, PN = c.PN, MEL = c.MEL, G4 = c.G4;
    hipStream_t s = c.s;
    const size_t BF = (size_t)B * Fmax, HB = (size_t)H * Bp;
    float* hz1[2] = {tw.tstate, tw.tstate + HB};  // zoned h1, ping-pong by frame parity
    float* hz2[2] = {tw.tstate + 2 * HB, tw.tstate + 3 * HB};
    float* hf1 = tw.tstate + 4 * HB;              // layer 1's un-zoned output of the frame in flight
    float* c1 = tw.tstate + 5 * HB;
    float* c2 = tw.tstate + 6 * HB;
    HIP_TRY(hipMemsetAsync(tw.tstate, 0, 7 * HB * 4, s));
    HIP_TRY(hipMemsetAsync(ws.mel0, 0, BF * MEL * 4, s));
    if (int rc = nat_cond_gates(c, c.mtiles)) return rc;
    // a GEMM over every sentence's frames (nat_conv's one-tap form); rows past nframes are not computed
    auto gemm = [&](const float* x, const char* key, const float* bias, float* y, int cin, int cout, int act, const uint8_t* kp = nullptr) {
        return NatConv{B, Fmax, Fmax, c.nframes, x, y, h->extra(key), bias, cin, cout, act, kp};
    };
    // prenet(inp_mels) over all frames (:149, :95-100), the one-frame shift of the target mels (gta.py:34-36) in the first GEMM's staging, relu and the
    // dropout's keep x 2 in both epilogues
    const float* zb = h->extra("prenet#zerob");
    if (c.keep) {
        nat_conv<1, NAT_TF_SHIFT | NAT_TF_KEEP>(gemm(c.mels, "linear_1#mfma", zb, tw.P1, MEL, PN, (int)NAT_ACT_RELU, c.keep), false, s);
        nat_conv<1, NAT_TF_KEEP>(gemm(tw.P1, "linear_2#mfma", zb, tw.P2, PN, PN, (int)NAT_ACT_RELU, c.keep + PN), false, s);
    } else {
        nat_conv<1, NAT_TF_SHIFT>(gemm(c.mels, "linear_1#mfma", zb, tw.P1, MEL, PN, (int)NAT_ACT_RELU), false, s);
        nat_conv<1>(gemm(tw.P1, "linear_2#mfma", zb, tw.P2, PN, PN, (int)NAT_ACT_RELU), false, s);
    }
    // G_l += p @ W_l[E : E + PN], onto the mix's output
    nat_conv<1, NAT_TF_ACC>(gemm(tw.P2, "lstm/linear#pre", h->extra("lstm/linear#zerob"), ws.G1, PN, G4, (int)NAT_ACT_NONE), false, s);
    nat_conv<1, NAT_TF_ACC>(gemm(tw.P2, "lstm_1/linear#pre", h->extra("lstm_1/linear#zerob"), ws.G2, PN, G4, (int)NAT_ACT_NONE), false, s);
    const float4 *w1 = h->extra<float4>("lstm/linear#tf"), *w2 = h->extra<float4>("lstm_1/linear#tf");
    const bool wide = B > 32;
    const dim3 lgrid(H / 8, wide ? Bp / 64 : 1);
    auto step = [&](const NatTfOps& o, int KA, int f) {
        if (wide) hipLaunchKernelGGL((nat_tf_lstm_k<2, 8>), lgrid, dim3(512), 0, s, o, KA, H, c.nframes, f, B, Bp, H, Fmax);
        else hipLaunchKernelGGL((nat_tf_lstm_k<1, 8>), lgrid, dim3(512), 0, s, o, KA, H, c.nframes, f, B, Bp, H, Fmax);
    };
    const size_t gp = (size_t)Fmax * G4;
    for (int f = 0; f < Fmax; ++f) {
        const int cur = f & 1, prv = cur ^ 1;
        step(NatTfOps{hz1[prv], hz1[prv], w1, c1, hz1[cur], hf1, tw.hseq, ws.G1 + (size_t)f * G4, gp, c.zone}, 0, f);
        step(NatTfOps{hf1, hz2[prv], w2, c2, hz2[cur], nullptr, tw.hseq + H, ws.G2 + (size_t)f * G4, gp, c.zone ? c.zone + 2 * (size_t)H : nullptr}, H, f);
    }
    nat_conv<1>(gemm(tw.hseq, "linear#mfma", h->dev("linear", "b"), ws.mel0, 2 * H, MEL, (int)NAT_ACT_NONE), false, s);  // :167
    if (c.mel_pre) HIP_TRY(hipMemcpyAsync(c.mel_pre, ws.mel0, BF * MEL * 4, hipMemcpyDeviceToDevice, s));
    return VTTS_OK;
}

// option "resident": 1 <= B <= 4, fp32 products, the reference's decoder dimensions, no hand-over, a stream that is not being captured
// and a grid the device can hold; in every other case *grid = 0 and the call takes the per-frame launches
int nat_resident_grid(const NatCall& c, int* grid) {
    vtts_nat_acoustic* h = c.h;
    *grid = 0;
    if (!h->resident || c.ngroups != 0 || c.B > 4 || h->x3 || c.H != NAT_RES_H || c.PN != NAT_RES_PN || c.MEL > NAT_RES_MELMAX) return VTTS_OK;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIP_TRY(hipStreamIsCapturing(c.s, &cap));
    if (!h->cu_count) {
        int dev = 0;
        HIP_TRY(hipGetDevice(&dev));
        HIP_TRY(hipDeviceGetAttribute(&h->cu_count, hipDeviceAttributeMultiprocessorCount, dev));
    }
    // at most one workgroup per CU: the default grid where the device has that many CUs, else the next smaller one
    int g = h->resident_grid ? h->resident_grid : NAT_RES_DEFAULT_GRID;
    while (g > h->cu_count && g > 64) g /= 2;
    if (cap == hipStreamCaptureStatusNone && g <= h->cu_count) *grid = g;
    return VTTS_OK;
}
// the frame loop as one resident kernel; h->resident_used stays 0 where the runtime cannot hold the grid resident
int nat_resident_launch(const NatCall& c, int grid) {
    vtts_nat_acoustic* h = c.h;
    const NatAcousticWs& ws = c.ws;
    HIP_TRY(hipMemsetAsync(ws.res_sync, 0, 256, c.s));
    const size_t e4 = (size_t)c.E * c.G4;  // Haiku rows [E, ...): the state's rows
    const NatResidentArgs ra{h->dev("lstm/linear", "w") + e4, h->dev("lstm_1/linear", "w") + e4, h->dev("linear", "w"), h->dev("linear", "b"),
                             h->dev("linear_1", "w"), h->dev("linear_2", "w"), ws.G1, ws.G2, c.nframes, c.keep, ws.mel0, reinterpret_cast<float*>(ws.res_sync + 64), ws.res_sync,
                             reinterpret_cast<unsigned long long*>(ws.res_sync + 2), c.Fmax, c.MEL};
    const hipError_t le = launch_nat_dec_resident(ra, c.B, grid, c.s);
    if (le == hipSuccess) {
        h->resident_used = 1;
        h->res_sync = ws.res_sync;
    } else if (le == hipErrorCooperativeLaunchTooLarge) {
        (void)hipGetLastError();  // the per-frame launches take over
    } else {
        return failf(VTTS_ERR_HIP, "resident decoder launch failed: %s", hipGetErrorString(le));
    }
    return VTTS_OK;
}

// frame 0's state: h1 = h2 = 0, c = 0, prenet(0) = 0 (no biases); and a zero decoder mel: rows past a sentence's last frame stay zero
int nat_dec_reset(const NatCall& c) {
    HIP_TRY(hipMemsetAsync(c.ws.dstate, 0, nat_dec_state_floats(c.h->cfg, c.B) * 4, c.s));
    HIP_TRY(hipMemsetAsync(c.ws.mel0, 0, (size_t)c.B * c.Fmax * c.MEL * 4, c.s));
    return VTTS_OK;
}

// autoregressive decoder (:134-150), frames [fa, fb): per frame LSTM1, LSTM2, projection + next frame's prenet, all sentences at once.  The state lives in
// the workspace between launches, its ping-pong indexed by the absolute frame's parity, so a range may start at any frame the previous one ended at.
// gates_wait: the mix of the frames from 64 on runs on the side stream (nat_cond_gates with mfirst < mtiles) and frame 64 waits for it.
int nat_dec_frames(const NatCall& c, int fa, int fb, bool gates_wait) {
    vtts_nat_acoustic* h = c.h;
    const NatAcousticWs& ws = c.ws;
    const int B = c.B, Bp = c.Bp, Fmax = c.Fmax, H = c.H, PN = c.PN, MEL = c.MEL, G4 = c.G4, ZW = PN + 2 * H;
    hipStream_t s = c.s;
    float* Z[2] = {ws.dstate, ws.dstate + (size_t)ZW * Bp};
    float* c1 = ws.dstate + 2 * (size_t)ZW * Bp;
    float* c2 = c1 + (size_t)H * Bp;
    const float4 *w1 = h->extra<float4>("lstm/linear#mfma"), *w2 = h->extra<float4>("lstm_1/linear#mfma");
    const float4 *f1 = h->extra<float4>("linear_1#k4"), *f2 = h->extra<float4>("linear_2#k4"), *wp = h->extra<float4>("linear#k4");
    const float* bp = h->dev("linear", "b");
    const bool wide = B > 32;  // two 32-sentence tiles per wave once there are that many sentences
    const dim3 lgrid(H / 8, wide ? Bp / 64 : 1);
    auto lstm = [&](const float* inA, int KA, const float* inB, const float4* w, const float* gin, float* cst, float* hout, int f) {
        const NatLstmOps o{inA, inB, w, nullptr, cst, hout, gin + (size_t)f * G4, (size_t)Fmax * G4};
        if (wide) hipLaunchKernelGGL((nat_dec_lstm_k<2, 8>), lgrid, dim3(512), 0, s, o, o, KA, H, c.nframes, NatFrameArg<false>{f}, B, Bp, H);
        else hipLaunchKernelGGL((nat_dec_lstm_k<1, 8>), lgrid, dim3(512), 0, s, o, o, KA, H, c.nframes, NatFrameArg<false>{f}, B, Bp, H);
    };
    const size_t plds = ((size_t)2 * H + 1024 + MEL + PN) * sizeof(float4);  // at most 64 KiB: create()'s limits at once (H = 1024, PN = 896, MEL = 128)
    if (plds > 48 * 1024) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&nat_dec_proj_prenet_k<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)plds));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&nat_dec_proj_prenet_k<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)plds));
    }
    auto group_handover = [&](int frames_done) -> int {  // a group whose last frame was frames_done - 1: its postnet starts now, on the side stream
        for (int g = 0; g < c.ngroups; ++g) {
            if (c.group_frames[g] != frames_done) continue;
            HIP_TRY(hipEventRecord(h->ev_dec[g], s));
            HIP_TRY(hipStreamWaitEvent(h->side, h->ev_dec[g], 0));
            nat_postnet(c, c.group_row0[g], c.group_row0[g + 1], c.group_frames[g], h->side);
            HIP_TRY(hipEventRecord(h->ev_done[g], h->side));
        }
        return VTTS_OK;
    };
    // option "bf16x3": the split-state step (nat_dec_lstm_x3_k) where its 16-row steps divide the row blocks; the state's two parities hold
    // two bf16 planes each (the same bytes as the fp32 rows)
    const bool dx3 = h->x3 && PN % 16 == 0 && H % 16 == 0 && ((PN + H) / 16) % 8 == 0 && ((PN + 2 * H) / 16) % 8 == 0;
    const size_t zplane = (size_t)ZW * Bp;  // bf16 elements per plane
    const uint4 *w1x = h->extra<uint4>("lstm/linear#x3"), *w2x = h->extra<uint4>("lstm_1/linear#x3");
    auto lstm_x3 = [&](unsigned short* zcx, const unsigned short* zpx, int KA, int K, const uint4* w, const float* gin, float* cst, int out_row0, int f) {
        const NatLstmX3Ops o{zcx, zpx, zplane, w, gin + (size_t)f * G4, (size_t)Fmax * G4, cst, zcx, out_row0};
        if (wide) hipLaunchKernelGGL((nat_dec_lstm_x3_k<2, 8>), lgrid, dim3(512), 0, s, o, KA, K, c.nframes, NatFrameArg<false>{f}, B, Bp, H);
        else hipLaunchKernelGGL((nat_dec_lstm_x3_k<1, 8>), lgrid, dim3(512), 0, s, o, KA, K, c.nframes, NatFrameArg<false>{f}, B, Bp, H);
    };
    for (int f = fa; f < fb; ++f) {
        if (f == 64 && gates_wait) HIP_TRY(hipStreamWaitEvent(s, h->ev_gates, 0));
        float* zc = Z[f & 1];
        float* zp = Z[(f + 1) & 1];
        if (dx3) {
            unsigned short* zcx = reinterpret_cast<unsigned short*>(zc);
            const unsigned short* zpx = reinterpret_cast<const unsigned short*>(zp);
            lstm_x3(zcx, zpx, PN, PN + H, w1x, ws.G1, c1, PN, f);
            lstm_x3(zcx, zpx, PN + H, PN + 2 * H, w2x, ws.G2, c2, PN + H, f);
            hipLaunchKernelGGL(nat_dec_proj_prenet_k<true>, dim3((B + 3) / 4), dim3(1024), plds, s, zc, zp, c.nframes, f1, f2, wp, bp, c.keep, ws.mel0, NatFrameArg<false>{f}, B, Bp,
                               Fmax, PN, H, MEL, zplane);
        } else {
            lstm(zc, PN, zp + (size_t)PN * Bp, w1, ws.G1, c1, zc + (size_t)PN * Bp, f);
            lstm(zc, PN + H, zp + (size_t)(PN + H) * Bp, w2, ws.G2, c2, zc + (size_t)(PN + H) * Bp, f);
            hipLaunchKernelGGL(nat_dec_proj_prenet_k<false>, dim3((B + 3) / 4), dim3(1024), plds, s, zc, zp, c.nframes, f1, f2, wp, bp, c.keep, ws.mel0, NatFrameArg<false>{f}, B, Bp,
                               Fmax, PN, H, MEL, (size_t)0);
        }
        if (int rc = group_handover(f + 1)) return rc;  // under the remaining decoder steps
    }
    return VTTS_OK;
}

// forward()'s decoder: every frame, as the resident kernel where the option asks for it and the call allows it
int nat_ar_decoder(const NatCall& c) {
    vtts_nat_acoustic* h = c.h;
    hipStream_t s = c.s;
    if (int rc = nat_dec_reset(c)) return rc;
    const bool stamps = h->stage_times && c.ngroups == 0;
    h->stage_valid = 0;
    if (stamps) {
        for (hipEvent_t& e : h->ev_stage)
            if (!e) HIP_TRY(hipEventCreate(&e));
        HIP_TRY(hipEventRecord(h->ev_stage[0], s));
    }
    // the gates' mix for frames [0, 64) here and for the rest beside the first 64 steps; all of it here when the resident kernel will run
    int res_grid = 0;
    if (int rc = nat_resident_grid(c, &res_grid)) return rc;
    const int mfirst = res_grid ? c.mtiles : std::min(64 / NAT_MIX_FT, c.mtiles);
    if (int rc = nat_cond_gates(c, mfirst)) return rc;
    if (stamps) HIP_TRY(hipEventRecord(h->ev_stage[1], s));
    if (res_grid)  // every frame's gates are on `s` already (mfirst = mtiles)
        if (int rc = nat_resident_launch(c, res_grid)) return rc;
    if (h->resident_used) return VTTS_OK;
    return nat_dec_frames(c, 0, c.Fmax, c.mtiles > mfirst);
}

// forward(), forward_groups(), forward_from_encoder() and forward_teacher()
int nat_acoustic_run(NatCall& c) {
    if (c.h) c.h->ss.open = c.h->pool.open = false;  // any forward*() ends an open streaming session or slot pool
    if (int rc = nat_validate(c)) return rc;
    vtts_nat_acoustic* h = c.h;
    if (int rc = nat_side_stream(h, c.ngroups)) return rc;
    h->resident_used = 0;
    if (c.enc_pre) c.ws.enc = const_cast<float*>(c.enc_pre);  // read only from here on
    else if (int rc = run_token_encoder(*h, "token_encoder/~/", h->cfg.vocab_size, h->cfg.encoder_dim, c.tokens, c.lengths, c.B, c.Lmax, c.ws.bufA, c.ws.bufB, c.ws.lstm_ws, c.ws.enc, c.s)) return rc;  // model.py:131
    HIP_TRY(hipMemsetAsync(c.mel, 0, (size_t)c.B * c.Fmax * c.MEL * 4, c.s));  // rows past a sentence's last frame
    if (int rc = c.mels ? nat_teacher_decoder(c) : nat_ar_decoder(c)) return rc;
    if (c.ngroups > 0) {
        for (int g = 0; g < c.ngroups; ++g) HIP_TRY(hipStreamWaitEvent(c.s, h->ev_done[g], 0));  // stream order for the caller: mel is complete after this call on `s`
        h->groups_valid = c.ngroups;
    } else {
        const bool stamps = !c.mels && h->stage_times;
        if (stamps) HIP_TRY(hipEventRecord(h->ev_stage[2], c.s));
        nat_postnet(c, 0, c.B, c.Fmax, c.s);
        if (stamps) {
            HIP_TRY(hipEventRecord(h->ev_stage[3], c.s));
            h->stage_valid = 1;
        }
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return failf(VTTS_ERR_HIP, "acoustic model launch failed: %s", hipGetErrorString(e));
    return VTTS_OK;
}

}  // namespace

VTTS_API int vtts_nat_acoustic_forward(vtts_nat_acoustic* h, const int32_t* tokens_dev, const int32_t* lengths_dev, const float* durations_dev,
                                       const int32_t* nframes_dev, int B, int Lmax, int Fmax, const uint8_t* keep_dev, float* mel_dev,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    NatCall c{h, tokens_dev, lengths_dev, durations_dev, nframes_dev, B, Lmax, Fmax, keep_dev, mel_dev, workspace, workspace_bytes, static_cast<hipStream_t>(stream)};
    return nat_acoustic_run(c);
}

VTTS_API int vtts_nat_acoustic_forward_groups(vtts_nat_acoustic* h, const int32_t* tokens_dev, const int32_t* lengths_dev, const float* durations_dev,
                                              const int32_t* nframes_dev, int B, int Lmax, int Fmax, const uint8_t* keep_dev, float* mel_dev,
                                              void* workspace, size_t workspace_bytes, void* stream, int ngroups, const int32_t* group_row0,
                                              const int32_t* group_frames) {
    if (ngroups < 1) return failf(VTTS_ERR_INVALID, "forward_groups() needs at least one group (got %d)", ngroups);
    NatCall c{h, tokens_dev, lengths_dev, durations_dev, nframes_dev, B, Lmax, Fmax, keep_dev, mel_dev, workspace, workspace_bytes, static_cast<hipStream_t>(stream),
              ngroups, group_row0, group_frames};
    return nat_acoustic_run(c);
}

// The teacher-forced pass (AcousticModel.__call__, model.py:146-169): the token encoder, forward()'s postnet, and the decoder fed with the target mels
VTTS_API int vtts_nat_acoustic_forward_teacher(vtts_nat_acoustic* h, const int32_t* tokens_dev, const int32_t* lengths_dev, const float* durations_dev,
                                               const int32_t* nframes_dev, int B, int Lmax, int Fmax, const float* mels_dev, const uint8_t* keep_dev,
                                               const uint8_t* zone_dev, float* mel_dev, float* mel_pre_dev, void* workspace, size_t workspace_bytes, void* stream) {
    if (!tokens_dev || !mels_dev) return failf(VTTS_ERR_INVALID, "null argument");
    if ((uintptr_t)mels_dev % 16 != 0 || (uintptr_t)keep_dev % 4 != 0)
        return failf(VTTS_ERR_INVALID, "forward_teacher() reads mels_dev in 16-byte and keep_dev in 4-byte units: align them so");
    NatCall c{h, tokens_dev, lengths_dev, durations_dev, nframes_dev, B, Lmax, Fmax, keep_dev, mel_dev, workspace, workspace_bytes, static_cast<hipStream_t>(stream)};
    c.mels = mels_dev, c.zone = zone_dev, c.mel_pre = mel_pre_dev;
    return nat_acoustic_run(c);
}

// The token encoder alone, ahead of forward_from_encoder(): it needs the tokens only, so a pipeline can run it while the host still turns the
// duration model's output into frame counts.  A row's output does not depend on its batch: rows may be re-ordered / dropped before
// forward_from_encoder() (whose B and row order are its own; Lmax must be this call's).  Workspace: workspace_bytes(h, B, Lmax, 1) suffice.
VTTS_API int vtts_nat_acoustic_encode(vtts_nat_acoustic* h, const int32_t* tokens_dev, const int32_t* lengths_dev, int B, int Lmax, float* enc_dev,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    if (!h || !tokens_dev || !lengths_dev || !enc_dev) return failf(VTTS_ERR_INVALID, "null argument");
    h->ss.open = h->pool.open = false;  // (its buffers are a session's and a pool's too)
    if (!h->blob) return failf(VTTS_ERR_STATE, "encode() before pack()/bind_packed()");
    size_t need = 0;
    int rc = vtts_nat_acoustic_workspace_bytes(h, B, Lmax, 1, &need);
    if (rc) return rc;
    if (!workspace || workspace_bytes < need) return failf(VTTS_ERR_NOMEM, "workspace too small: %zu < %zu bytes", workspace_bytes, need);
    const int D = h->cfg.encoder_dim, V = h->cfg.vocab_size;
    NatCarver w{static_cast<char*>(workspace)};  // its own three-buffer prefix (fits: the full layout holds the same three buffers and more)
    float* bufA = w.take((size_t)B * Lmax * D * 4);
    float* bufB = w.take((size_t)B * Lmax * D * 4);
    float* lstm_ws = w.take(nat_enc_lstm_floats(D, B, Lmax) * 4);
    rc = run_token_encoder(*h, "token_encoder/~/", V, D, tokens_dev, lengths_dev, B, Lmax, bufA, bufB, lstm_ws, enc_dev, static_cast<hipStream_t>(stream));
    if (rc) return rc;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return failf(VTTS_ERR_HIP, "token encoder launch failed: %s", hipGetErrorString(e));
    return VTTS_OK;
}
// forward() / forward_groups() (ngroups = 0: no hand-over) from an encoder output computed by vtts_nat_acoustic_encode(): the same mel, bit for bit
VTTS_API int vtts_nat_acoustic_forward_from_encoder(vtts_nat_acoustic* h, const float* enc_dev, const int32_t* lengths_dev, const float* durations_dev,
                                                    const int32_t* nframes_dev, int B, int Lmax, int Fmax, const uint8_t* keep_dev, float* mel_dev,
                                                    void* workspace, size_t workspace_bytes, void* stream, int ngroups, const int32_t* group_row0,
                                                    const int32_t* group_frames) {
    if (!enc_dev) return failf(VTTS_ERR_INVALID, "null argument");
    if (ngroups < 0) return failf(VTTS_ERR_INVALID, "ngroups must be >= 0 (got %d)", ngroups);
    NatCall c{h, nullptr, lengths_dev, durations_dev, nframes_dev, B, Lmax, Fmax, keep_dev, mel_dev, workspace, workspace_bytes, static_cast<hipStream_t>(stream),
              ngroups, group_row0, group_frames, enc_dev};
    return nat_acoustic_run(c);
}

VTTS_API int vtts_nat_acoustic_wait_group(vtts_nat_acoustic* h, int group, void* stream) {
    if (!h) return failf(VTTS_ERR_INVALID, "null argument");
    if (group < 0 || group >= h->groups_valid) return failf(VTTS_ERR_STATE, "wait_group(%d): the last forward_groups() call had %d groups", group, h->groups_valid);
    HIP_TRY(hipStreamWaitEvent(static_cast<hipStream_t>(stream), h->ev_done[group], 0));
    return VTTS_OK;
}

// ------------------------------------------------ streaming session ------------------------------------------------
// forward() cut along time (include/vtts_nat.h): begin = everything ahead of the frame loop, decode = a range of the loop's frames, finish = postnet +
// residual of a frame window on a compact copy of it.  The launches and their arithmetic are forward()'s; only the postnet's tiles sit elsewhere.
namespace {

// the session's call on `stream`, or a status: no handle, no session, or the option "bf16x3" changed under it
int nat_session_call(vtts_nat_acoustic* h, const char* what, void* stream, NatCall* c) {
    if (!h) return failf(VTTS_ERR_INVALID, "null argument");
    const vtts_nat_acoustic::Session& ss = h->ss;
    if (!ss.open) return failf(VTTS_ERR_STATE, "%s: no open session (stream_begin() first; any forward*(), encode() or stream_end() closes it)", what);
    if (h->x3 != ss.x3) return failf(VTTS_ERR_STATE, "%s: the option bf16x3 changed since stream_begin()", what);
    *c = NatCall{h, nullptr, ss.lengths, ss.durations, ss.nframes, ss.B, ss.Lmax, ss.Fmax, ss.keep, ss.mel, ss.workspace, ss.workspace_bytes, static_cast<hipStream_t>(stream)};
    nat_derive(*c);
    return VTTS_OK;
}

}  // namespace

VTTS_API int vtts_nat_acoustic_stream_workspace_bytes(const vtts_nat_acoustic* h, int B, int Lmax, int Fmax, int max_window, size_t* bytes) {
    if (int rc = vtts_nat_acoustic_workspace_bytes(h, B, Lmax, Fmax, bytes)) return rc;
    if (max_window < 1) return failf(VTTS_ERR_INVALID, "max_window must be positive (got %d)", max_window);
    *bytes = NatStreamWs(NatAcousticWs(h->cfg, B, Lmax, Fmax, nullptr), h->cfg, B, Fmax, max_window).bytes;
    return VTTS_OK;
}

VTTS_API int vtts_nat_acoustic_stream_begin(vtts_nat_acoustic* h, const int32_t* tokens_dev, const int32_t* lengths_dev, const float* durations_dev,
                                            const int32_t* nframes_dev, int B, int Lmax, int Fmax, const uint8_t* keep_dev, float* mel_dev, void* workspace,
                                            size_t workspace_bytes, int max_window, void* stream) {
    if (h) h->ss.open = h->pool.open = false;
    if (!tokens_dev) return failf(VTTS_ERR_INVALID, "null argument");
    NatCall c{h, tokens_dev, lengths_dev, durations_dev, nframes_dev, B, Lmax, Fmax, keep_dev, mel_dev, workspace, workspace_bytes, static_cast<hipStream_t>(stream)};
    if (int rc = nat_validate(c)) return rc;
    size_t need = 0;
    if (int rc = vtts_nat_acoustic_stream_workspace_bytes(h, B, Lmax, Fmax, max_window, &need)) return rc;
    if (workspace_bytes < need) return failf(VTTS_ERR_NOMEM, "workspace too small: %zu < %zu bytes (stream_workspace_bytes())", workspace_bytes, need);
    if ((uintptr_t)mel_dev % 16 != 0) return failf(VTTS_ERR_INVALID, "stream_begin(): mel_dev is written in 16-byte units: align it so");
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIP_TRY(hipStreamIsCapturing(c.s, &cap));
    if (cap != hipStreamCaptureStatusNone) return failf(VTTS_ERR_INVALID, "stream_begin(): the stream is being captured (a session's launches depend on host state)");
    h->resident_used = 0;
    h->stage_valid = 0;
    if (int rc = run_token_encoder(*h, "token_encoder/~/", h->cfg.vocab_size, h->cfg.encoder_dim, c.tokens, c.lengths, c.B, c.Lmax, c.ws.bufA, c.ws.bufB, c.ws.lstm_ws, c.ws.enc, c.s)) return rc;
    HIP_TRY(hipMemsetAsync(c.mel, 0, (size_t)c.B * c.Fmax * c.MEL * 4, c.s));  // rows past a sentence's last frame
    if (int rc = nat_dec_reset(c)) return rc;
    if (int rc = nat_cond_gates(c, c.mtiles)) return rc;  // every frame's mix on the caller's stream: nothing of a session runs on the side stream
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return failf(VTTS_ERR_HIP, "acoustic model launch failed: %s", hipGetErrorString(e));
    h->ss = vtts_nat_acoustic::Session{true, lengths_dev, nframes_dev, durations_dev, keep_dev, mel_dev, workspace, workspace_bytes, B, Lmax, Fmax, max_window, h->x3, 0, 0};
    return VTTS_OK;
}

VTTS_API int vtts_nat_acoustic_stream_decode(vtts_nat_acoustic* h, int upto, void* stream) {
    NatCall c;
    if (int rc = nat_session_call(h, "stream_decode()", stream, &c)) return rc;
    const int to = std::min(upto, c.Fmax);
    if (to <= h->ss.cursor) return VTTS_OK;
    if (int rc = nat_dec_frames(c, h->ss.cursor, to, false)) return rc;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return failf(VTTS_ERR_HIP, "decoder launch failed: %s", hipGetErrorString(e));
    h->ss.cursor = to;
    return VTTS_OK;
}

VTTS_API int vtts_nat_acoustic_stream_finish(vtts_nat_acoustic* h, int f0, int f1, void* stream) {
    NatCall c;
    if (int rc = nat_session_call(h, "stream_finish()", stream, &c)) return rc;
    vtts_nat_acoustic::Session& ss = h->ss;
    if (f0 != ss.finished || f1 <= f0 || f0 >= c.Fmax)
        return failf(VTTS_ERR_INVALID, "stream_finish(%d, %d): windows are issued in order, contiguous and not empty; the next one starts at frame %d of %d", f0, f1, ss.finished, c.Fmax);
    if (f1 - f0 > ss.max_window) return failf(VTTS_ERR_INVALID, "stream_finish(%d, %d): the session was opened for windows of at most %d frames", f0, f1, ss.max_window);
    f1 = std::min(f1, c.Fmax);
    const int lo = std::max(0, f0 - VTTS_NAT_POSTNET_HALO), hi = std::min(c.Fmax, f1 + VTTS_NAT_POSTNET_HALO), n = hi - lo;
    if (ss.cursor < hi) return failf(VTTS_ERR_STATE, "stream_finish(%d, %d) reads the decoder's frames up to %d: stream_decode() has reached %d", f0, f1, hi, ss.cursor);
    const NatStreamWs w(c.ws, h->cfg, c.B, c.Fmax, ss.max_window);
    const int C4 = c.MEL / 4;
    auto blocks = [](size_t elems) { return (int)std::min<size_t>((elems + 255) / 256, 65535); };
    hipLaunchKernelGGL(nat_window_k<false>, dim3(blocks((size_t)c.B * w.W * C4)), dim3(256), 0, c.s, reinterpret_cast<const float4*>(c.ws.mel0), reinterpret_cast<float4*>(w.wmel),
                       c.nframes, w.wl, c.B, c.Fmax, w.W, C4, lo, n, 0, 0);
    nat_postnet_run(c, NatPostnetBufs{c.B, n, w.W, w.wl, w.wmel, {w.wpA, w.wpB}, w.wout}, c.s);
    hipLaunchKernelGGL(nat_window_k<true>, dim3(blocks((size_t)c.B * (f1 - f0) * C4)), dim3(256), 0, c.s, reinterpret_cast<const float4*>(w.wout), reinterpret_cast<float4*>(c.mel),
                       c.nframes, static_cast<int*>(nullptr), c.B, c.Fmax, w.W, C4, lo, n, f0 - lo, f1 - lo);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return failf(VTTS_ERR_HIP, "postnet window launch failed: %s", hipGetErrorString(e));
    ss.finished = f1;
    return VTTS_OK;
}

VTTS_API int vtts_nat_acoustic_stream_end(vtts_nat_acoustic* h) {
    if (!h) return failf(VTTS_ERR_INVALID, "null argument");
    h->ss.open = false;
    return VTTS_OK;
}

// ------------------------------------------------ slot pool ------------------------------------------------
// The session's cut along time with a frame cursor PER ROW (include/vtts_nat.h): a tick is one frame step of every slot, the three launches of
// nat_dec_frames() in their POOL form, row b at frame tick - start[b].  The state ping-pong goes by the TICK's parity: a row admitted at an odd
// tick reads as "previous" what the tick before it left, which for its frame 0 is the zeros of its reset, in both parities.
namespace {

int nat_not_capturing(const char* what, hipStream_t s) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIP_TRY(hipStreamIsCapturing(s, &cap));
    if (cap != hipStreamCaptureStatusNone) return failf(VTTS_ERR_INVALID, "%s: the stream is being captured (a pool's launches depend on host state)", what);
    return VTTS_OK;
}

// the pool's call on `stream` (B = every slot), or a status: no handle, no pool, the option "bf16x3" changed under it, a stream that is being captured
int nat_pool_call(vtts_nat_acoustic* h, const char* what, void* stream, NatCall* c) {
    if (!h) return failf(VTTS_ERR_INVALID, "null argument");
    const vtts_nat_acoustic::Pool& p = h->pool;
    if (!p.open) return failf(VTTS_ERR_STATE, "%s: no open pool (pool_open() first; any forward*(), encode(), stream_begin() or pool_close() closes it)", what);
    if (h->x3 != p.x3) return failf(VTTS_ERR_STATE, "%s: the option bf16x3 changed since pool_open()", what);
    if (int rc = nat_not_capturing(what, static_cast<hipStream_t>(stream))) return rc;
    *c = NatCall{h, nullptr, nullptr, nullptr, nullptr, p.slots, p.Lmax, p.Fmax, p.keep, p.mel, p.workspace, p.workspace_bytes, static_cast<hipStream_t>(stream)};
    nat_derive(*c);
    return VTTS_OK;
}
NatPoolWs nat_pool_ws(const NatCall& c) {
    return NatPoolWs(NatStreamWs(c.ws, c.h->cfg, c.B, c.Fmax, c.h->pool.max_window), c.B);
}
int nat_pool_slot(const NatCall& c, const char* what, int slot, bool busy) {
    if (slot < 0 || slot >= c.B) return failf(VTTS_ERR_INVALID, "%s: slot %d of a pool of %d", what, slot, c.B);
    if (c.h->pool.slot[slot].busy != busy) return failf(VTTS_ERR_STATE, "%s: slot %d is %s", what, slot, busy ? "free" : "busy (pool_retire() frees it)");
    return VTTS_OK;
}
// whether the decoder runs the split-state step (nat_dec_frames: dx3)
bool nat_dec_x3(const NatCall& c) {
    return c.h->x3 && c.PN % 16 == 0 && c.H % 16 == 0 && ((c.PN + c.H) / 16) % 8 == 0 && ((c.PN + 2 * c.H) / 16) % 8 == 0;
}

// ticks [ta, tb) for every slot: nat_dec_frames()'s operands and launches, the frame argument per row
int nat_pool_ticks(const NatCall& c, const NatPoolMeta& meta, int ta, int tb) {
    vtts_nat_acoustic* h = c.h;
    const NatAcousticWs& ws = c.ws;
    const int B = c.B, Bp = c.Bp, Fmax = c.Fmax, H = c.H, PN = c.PN, MEL = c.MEL, G4 = c.G4, ZW = PN + 2 * H;
    hipStream_t s = c.s;
    float* Z[2] = {ws.dstate, ws.dstate + (size_t)ZW * Bp};
    float* c1 = ws.dstate + 2 * (size_t)ZW * Bp;
    float* c2 = c1 + (size_t)H * Bp;
    const float4 *w1 = h->extra<float4>("lstm/linear#mfma"), *w2 = h->extra<float4>("lstm_1/linear#mfma");
    const float4 *f1 = h->extra<float4>("linear_1#k4"), *f2 = h->extra<float4>("linear_2#k4"), *wp = h->extra<float4>("linear#k4");
    const uint4 *w1x = h->extra<uint4>("lstm/linear#x3"), *w2x = h->extra<uint4>("lstm_1/linear#x3");
    const float* bp = h->dev("linear", "b");
    const bool wide = B > 32, dx3 = nat_dec_x3(c);
    const dim3 lgrid(H / 8, wide ? Bp / 64 : 1), pgrid((B + 3) / 4);
    const size_t gp = (size_t)Fmax * G4, zplane = (size_t)ZW * Bp;
    const size_t plds = ((size_t)2 * H + 1024 + MEL + PN) * sizeof(float4);
    if (plds > 48 * 1024) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&nat_dec_proj_prenet_k<false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)plds));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&nat_dec_proj_prenet_k<true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)plds));
    }
    for (int t = ta; t < tb; ++t) {
        const NatFrameArg<true> fa{t, meta.start};
        float* zc = Z[t & 1];
        float* zp = Z[(t + 1) & 1];
        if (dx3) {
            unsigned short* zcx = reinterpret_cast<unsigned short*>(zc);
            const unsigned short* zpx = reinterpret_cast<const unsigned short*>(zp);
            const NatLstmX3Ops o1{zcx, zpx, zplane, w1x, ws.G1, gp, c1, zcx, PN}, o2{zcx, zpx, zplane, w2x, ws.G2, gp, c2, zcx, PN + H};
            if (wide) {
                hipLaunchKernelGGL((nat_dec_lstm_x3_k<2, 8, true>), lgrid, dim3(512), 0, s, o1, PN, PN + H, meta.nframes, fa, B, Bp, H);
                hipLaunchKernelGGL((nat_dec_lstm_x3_k<2, 8, true>), lgrid, dim3(512), 0, s, o2, PN + H, PN + 2 * H, meta.nframes, fa, B, Bp, H);
            } else {
                hipLaunchKernelGGL((nat_dec_lstm_x3_k<1, 8, true>), lgrid, dim3(512), 0, s, o1, PN, PN + H, meta.nframes, fa, B, Bp, H);
                hipLaunchKernelGGL((nat_dec_lstm_x3_k<1, 8, true>), lgrid, dim3(512), 0, s, o2, PN + H, PN + 2 * H, meta.nframes, fa, B, Bp, H);
            }
            hipLaunchKernelGGL((nat_dec_proj_prenet_k<true, true>), pgrid, dim3(1024), plds, s, zc, zp, meta.nframes, f1, f2, wp, bp, c.keep, ws.mel0, fa, B, Bp, Fmax, PN, H,
                               MEL, zplane);
        } else {
            const NatLstmOps o1{zc, zp + (size_t)PN * Bp, w1, nullptr, c1, zc + (size_t)PN * Bp, ws.G1, gp};
            const NatLstmOps o2{zc, zp + (size_t)(PN + H) * Bp, w2, nullptr, c2, zc + (size_t)(PN + H) * Bp, ws.G2, gp};
            if (wide) {
                hipLaunchKernelGGL((nat_dec_lstm_k<2, 8, 1, true>), lgrid, dim3(512), 0, s, o1, o1, PN, H, meta.nframes, fa, B, Bp, H);
                hipLaunchKernelGGL((nat_dec_lstm_k<2, 8, 1, true>), lgrid, dim3(512), 0, s, o2, o2, PN + H, H, meta.nframes, fa, B, Bp, H);
            } else {
                hipLaunchKernelGGL((nat_dec_lstm_k<1, 8, 1, true>), lgrid, dim3(512), 0, s, o1, o1, PN, H, meta.nframes, fa, B, Bp, H);
                hipLaunchKernelGGL((nat_dec_lstm_k<1, 8, 1, true>), lgrid, dim3(512), 0, s, o2, o2, PN + H, H, meta.nframes, fa, B, Bp, H);
            }
            hipLaunchKernelGGL((nat_dec_proj_prenet_k<false, true>), pgrid, dim3(1024), plds, s, zc, zp, meta.nframes, f1, f2, wp, bp, c.keep, ws.mel0, fa, B, Bp, Fmax, PN, H,
                               MEL, (size_t)0);
        }
    }
    return VTTS_OK;
}

}  // namespace

VTTS_API int vtts_nat_acoustic_pool_workspace_bytes(const vtts_nat_acoustic* h, int slots, int Lmax, int Fmax, int max_window, size_t* bytes) {
    if (int rc = vtts_nat_acoustic_stream_workspace_bytes(h, slots, Lmax, Fmax, max_window, bytes)) return rc;
    *bytes = NatPoolWs(NatStreamWs(NatAcousticWs(h->cfg, slots, Lmax, Fmax, nullptr), h->cfg, slots, Fmax, max_window), slots).bytes;
    return VTTS_OK;
}

VTTS_API int vtts_nat_acoustic_pool_open(vtts_nat_acoustic* h, int slots, int Lmax, int Fmax, int max_window, const uint8_t* keep_dev, float* mel_dev, void* workspace,
                                         size_t workspace_bytes, void* stream) {
    if (h) h->ss.open = h->pool.open = false;
    if (!h || !mel_dev) return failf(VTTS_ERR_INVALID, "null argument");
    if (!h->blob) return failf(VTTS_ERR_STATE, "pool_open() before pack()/bind_packed()");
    size_t need = 0;
    if (int rc = vtts_nat_acoustic_pool_workspace_bytes(h, slots, Lmax, Fmax, max_window, &need)) return rc;
    if (!workspace || workspace_bytes < need) return failf(VTTS_ERR_NOMEM, "workspace too small: %zu < %zu bytes (pool_workspace_bytes())", workspace_bytes, need);
    if (Lmax > 2048) return failf(VTTS_ERR_INVALID, "at most 2048 tokens per sentence (upsampling weights live in LDS)");
    if ((uintptr_t)mel_dev % 16 != 0) return failf(VTTS_ERR_INVALID, "pool_open(): mel_dev is written in 16-byte units: align it so");
    if (int rc = nat_not_capturing("pool_open()", static_cast<hipStream_t>(stream))) return rc;
    NatCall c{h, nullptr, nullptr, nullptr, nullptr, slots, Lmax, Fmax, keep_dev, mel_dev, workspace, workspace_bytes, static_cast<hipStream_t>(stream)};
    nat_derive(c);
    h->resident_used = 0;
    h->stage_valid = 0;
    h->pool.max_window = max_window;
    const NatPoolWs pw = nat_pool_ws(c);
    // every slot idle (nframes 0) over a zero state, a zero decoder mel and a zero mel
    HIP_TRY(hipMemsetAsync(pw.meta.start, 0, (size_t)3 * slots * 4, c.s));
    HIP_TRY(hipMemsetAsync(c.mel, 0, (size_t)slots * Fmax * c.MEL * 4, c.s));
    if (int rc = nat_dec_reset(c)) return rc;
    vtts_nat_acoustic::Pool& p = h->pool;
    p.keep = keep_dev, p.mel = mel_dev, p.workspace = workspace, p.workspace_bytes = workspace_bytes;
    p.slots = slots, p.Lmax = Lmax, p.Fmax = Fmax, p.x3 = h->x3, p.tick = 0;
    p.slot.assign(slots, vtts_nat_acoustic::Pool::Slot{});
    p.open = true;
    return VTTS_OK;
}

VTTS_API int vtts_nat_acoustic_pool_admit(vtts_nat_acoustic* h, int slot, const int32_t* tokens_dev, int length, const float* durations_dev, int nframes, void* stream) {
    NatCall c;
    if (int rc = nat_pool_call(h, "pool_admit()", stream, &c)) return rc;
    if (!tokens_dev || !durations_dev) return failf(VTTS_ERR_INVALID, "null argument");
    if (length < 1 || length > c.Lmax) return failf(VTTS_ERR_INVALID, "pool_admit(): %d tokens; the pool was opened for 1 .. %d", length, c.Lmax);
    if (nframes < 1 || nframes > c.Fmax) return failf(VTTS_ERR_INVALID, "pool_admit(): %d frames; the pool was opened for 1 .. %d", nframes, c.Fmax);
    if (int rc = nat_pool_slot(c, "pool_admit()", slot, false)) return rc;
    vtts_nat_acoustic::Pool& p = h->pool;
    const NatPoolWs pw = nat_pool_ws(c);
    // the reset goes first: it writes the slot's token and frame counts, which the row's encoder and gate mix read
    const int ZW = c.PN + 2 * c.H, C4 = c.Fmax * c.MEL / 4;
    const dim3 rgrid(std::max(1, std::min(64, (std::max(2 * ZW, C4) + 255) / 256)));
    float4* mel0 = reinterpret_cast<float4*>(c.ws.mel0);
    float4* mel = reinterpret_cast<float4*>(c.mel);
    if (nat_dec_x3(c)) hipLaunchKernelGGL(nat_pool_reset_k<true>, rgrid, dim3(256), 0, c.s, c.ws.dstate, mel0, mel, pw.meta, slot, p.tick, nframes, length, c.Bp, ZW, c.H, C4);
    else hipLaunchKernelGGL(nat_pool_reset_k<false>, rgrid, dim3(256), 0, c.s, c.ws.dstate, mel0, mel, pw.meta, slot, p.tick, nframes, length, c.Bp, ZW, c.H, C4);
    // a one-row call on the slot's rows of the pool's buffers ([B][...] row-major: offset pointers); the encoder LSTMs' scratch is the pool's, one admission at a time
    NatCall r = c;
    const size_t LD = (size_t)slot * c.Lmax * h->cfg.encoder_dim, LG = (size_t)slot * c.Lmax * c.G4, FG = (size_t)slot * c.Fmax * c.G4;
    r.tokens = tokens_dev, r.durations = durations_dev, r.lengths = pw.meta.lengths + slot, r.nframes = pw.meta.nframes + slot;
    r.B = 1, r.Bp = 64;
    r.ws.bufA += LD, r.ws.bufB += LD, r.ws.enc += 2 * LD, r.ws.EG1 += LG, r.ws.EG2 += LG, r.ws.G1 += FG, r.ws.G2 += FG;
    if (int rc = run_token_encoder(*h, "token_encoder/~/", h->cfg.vocab_size, h->cfg.encoder_dim, r.tokens, r.lengths, 1, r.Lmax, r.ws.bufA, r.ws.bufB, r.ws.lstm_ws, r.ws.enc, r.s)) return rc;
    if (int rc = nat_cond_gates(r, r.mtiles)) return rc;  // every frame's mix on the caller's stream, as stream_begin()
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return failf(VTTS_ERR_HIP, "pool admission launch failed: %s", hipGetErrorString(e));
    p.slot[slot] = vtts_nat_acoustic::Pool::Slot{true, p.tick, nframes, 0};
    return VTTS_OK;
}

VTTS_API int vtts_nat_acoustic_pool_decode(vtts_nat_acoustic* h, int nticks, void* stream) {
    NatCall c;
    if (int rc = nat_pool_call(h, "pool_decode()", stream, &c)) return rc;
    vtts_nat_acoustic::Pool& p = h->pool;
    if (nticks < 0 || nticks > INT32_MAX - p.tick) return failf(VTTS_ERR_INVALID, "pool_decode(%d): the pool stands at tick %d; ticks are counted in 31 bits", nticks, p.tick);
    if (int rc = nat_pool_ticks(c, nat_pool_ws(c).meta, p.tick, p.tick + nticks)) return rc;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return failf(VTTS_ERR_HIP, "decoder launch failed: %s", hipGetErrorString(e));
    p.tick += nticks;
    return VTTS_OK;
}

VTTS_API int vtts_nat_acoustic_pool_finish(vtts_nat_acoustic* h, int n, const int32_t* slots, const int32_t* f0, const int32_t* f1, void* stream) {
    NatCall c;
    if (int rc = nat_pool_call(h, "pool_finish()", stream, &c)) return rc;
    vtts_nat_acoustic::Pool& p = h->pool;
    if (n < 1 || n > c.B || !slots || !f0 || !f1) return failf(VTTS_ERR_INVALID, "pool_finish(): 1 .. %d rows and their windows (got %d)", c.B, n);
    // every row is checked before anything is enqueued
    std::vector<int> end(n);
    std::vector<char> seen(c.B, 0);
    for (int j = 0; j < n; ++j) {
        if (int rc = nat_pool_slot(c, "pool_finish()", slots[j], true)) return rc;
        const vtts_nat_acoustic::Pool::Slot& sl = p.slot[slots[j]];
        if (seen[slots[j]]) return failf(VTTS_ERR_INVALID, "pool_finish(): slot %d is listed twice", slots[j]);
        seen[slots[j]] = 1;
        if (f0[j] != sl.finished || f1[j] <= f0[j] || f0[j] >= sl.nframes)
            return failf(VTTS_ERR_INVALID, "pool_finish(): slot %d, [%d, %d): windows are issued in order, contiguous and not empty; the next one starts at frame %d of %d",
                         slots[j], f0[j], f1[j], sl.finished, sl.nframes);
        if (f1[j] - f0[j] > p.max_window) return failf(VTTS_ERR_INVALID, "pool_finish(): slot %d, [%d, %d): the pool was opened for windows of at most %d frames", slots[j], f0[j], f1[j], p.max_window);
        end[j] = std::min(f1[j], sl.nframes);
        const int hi = std::min(sl.nframes, end[j] + VTTS_NAT_POSTNET_HALO);
        if (p.cursor(slots[j]) < hi)
            return failf(VTTS_ERR_STATE, "pool_finish(): slot %d, [%d, %d) reads the decoder's frames up to %d: the slot's row has reached %d", slots[j], f0[j], f1[j], hi, p.cursor(slots[j]));
    }
    const NatStreamWs w(c.ws, h->cfg, c.B, c.Fmax, p.max_window);
    const int C4 = c.MEL / 4;
    auto blocks = [](size_t elems) { return (int)std::min<size_t>((elems + 255) / 256, 65535); };
    // the list in launches of NAT_POOL_LIST rows; one postnet pass over all of them in between
    int npos = 0;
    auto windows = [&](bool scatter) {
        for (int j0 = 0; j0 < n; j0 += NAT_POOL_LIST) {
            NatPoolWindows L{};
            L.count = std::min(NAT_POOL_LIST, n - j0), L.r0 = j0;
            for (int q = 0; q < L.count; ++q) {
                const int j = j0 + q, nf = p.slot[slots[j]].nframes;
                const int lo = std::max(0, f0[j] - VTTS_NAT_POSTNET_HALO), hi = std::min(nf, end[j] + VTTS_NAT_POSTNET_HALO);
                L.slot[q] = slots[j], L.lo[q] = lo, L.n[q] = hi - lo, L.k0[q] = f0[j] - lo, L.k1[q] = end[j] - lo;
                npos = std::max(npos, hi - lo);
            }
            const dim3 grid(blocks((size_t)L.count * w.W * C4));
            if (scatter) hipLaunchKernelGGL(nat_pool_window_k<true>, grid, dim3(256), 0, c.s, reinterpret_cast<const float4*>(w.wout), reinterpret_cast<float4*>(c.mel), static_cast<int*>(nullptr), L, c.Fmax, w.W, C4);
            else hipLaunchKernelGGL(nat_pool_window_k<false>, grid, dim3(256), 0, c.s, reinterpret_cast<const float4*>(c.ws.mel0), reinterpret_cast<float4*>(w.wmel), w.wl, L, c.Fmax, w.W, C4);
        }
    };
    windows(false);
    nat_postnet_run(c, NatPostnetBufs{n, npos, w.W, w.wl, w.wmel, {w.wpA, w.wpB}, w.wout}, c.s);
    windows(true);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return failf(VTTS_ERR_HIP, "postnet window launch failed: %s", hipGetErrorString(e));
    for (int j = 0; j < n; ++j) p.slot[slots[j]].finished = end[j];
    return VTTS_OK;
}

VTTS_API int vtts_nat_acoustic_pool_retire(vtts_nat_acoustic* h, int slot, void* stream) {
    NatCall c;
    if (int rc = nat_pool_call(h, "pool_retire()", stream, &c)) return rc;
    if (int rc = nat_pool_slot(c, "pool_retire()", slot, true)) return rc;
    hipLaunchKernelGGL(nat_pool_idle_k, dim3(1), dim3(64), 0, c.s, nat_pool_ws(c).meta, slot);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return failf(VTTS_ERR_HIP, "pool_retire() launch failed: %s", hipGetErrorString(e));
    h->pool.slot[slot].busy = false;
    return VTTS_OK;
}

VTTS_API int vtts_nat_acoustic_pool_close(vtts_nat_acoustic* h) {
    if (!h) return failf(VTTS_ERR_INVALID, "null argument");
    h->pool.open = false;
    return VTTS_OK;
}
