// HiFi-GAN discriminators and losses, forward only (include/vtts_disc.h): vietTTS/hifigan/torch_model.py MultiPeriodDiscriminator,
// MultiScaleDiscriminator, feature_loss, generator_loss, discriminator_loss.
//
// Activations are [N][C][L][p] (p = the period's columns for MPD, 1 for MSD): exactly the reference's feature-map shapes, so every
// layer's output is written once and is both the next layer's input and a feature map.
//
//   disc_conv_k    the strided, grouped implicit GEMM of the 36 middle layers.  M = a group's output channels, K = (tap, input channel
//                  of the group), N = output positions n = h' p + w of one row.  A workgroup owns BM channels x NT positions.  The input
//                  it needs is, per channel, ONE contiguous span of the flat [L][p] axis: rows stride h0 - pad ... of all p columns.
//                  It is staged 16 channels at a time into LDS with the `stride` phases of the row index de-interleaved,
//                      row r = stride q + ph  ->  LDS row ph PH + q,
//                  so that tap t of output position j sits at  off(t) + j  with  off(t) = ((t % stride) PH + t / stride) p :
//                  every B-fragment read of a wave is 32 (16) consecutive floats whatever the stride and the period, no bank conflict.
//                  The weights never touch LDS: the host packs them in A-fragment order ([group][m tile][chunk][tap][lane][k step]), so
//                  a lane reads the taps' fragments as 16-byte loads from a linear stream, one tap ahead of the MFMAs.
//                  v_mfma_f32_32x32x2_f32, and v_mfma_f32_16x16x4_f32 for the 16-channel groups (MSD 128 -> 256).
//                  Bias and LeakyReLU are fused.  The K order of an output element does not depend on the tile or the batch, so a
//                  row's results are bit-identical alone and in any batch.
//   mpd_first_k / msd_first_k   Cin = 1 on the VALU, the reflect pad / the average pools applied while loading.
//   disc_post_k    conv_post (Cout = 1, k = 3): lanes = positions, four waves split the channels, double accumulators, fixed-order combine.
//   loss_stage1_k / loss_stage2_k   every loss in one fixed-order two-stage reduction (double accumulators, no atomics).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/vtts_disc.h"
#include "../../include/vtts_hifigan.h"
#include "vtts_internal.h"

using vtts::check_blob;
using vtts::failf;
using vtts::upload_blob;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr float SLOPE = 0.1f;
constexpr int NDISC = VTTS_DISC_NUM_DISCS, NCONV = VTTS_DISC_NUM_CONVS, NPART = VTTS_DISC_LOSS_PARTIALS;
constexpr int NRED = VTTS_DISC_NUM_FMAPS + 3 * NDISC;  // tensors the loss pass reduces
constexpr int PERIODS[5] = {2, 3, 5, 7, 11};
constexpr int64_t MAX_T = 1 << 23;  // keeps one row of any feature map (128 T floats at most) inside 32-bit indexing

enum Kind : int { K_MPD_FIRST, K_MSD_FIRST, K_GEMM, K_POST };

struct ConvSpec {
    std::string key;
    int disc, kind, cin, cout, k, stride, pad, groups;
    size_t w_off, b_off;  // floats into the blob
};

// ---- the middle layers ------------------------------------------------------------------------------------------------------------
struct GArgs {
    const float* x;
    float* y;
    const float* wp;    // this layer's packed weights
    const float* bias;  // [Cout]
    long x_row, y_row;  // floats per batch row of x / y
    int cin_g, cout_g, k, stride, pad, p;
    int Lin, Nout;      // flat input length Hin p and output positions Hout p, per channel
    int nch;            // cin_g / CK
    int PH, spanp;      // staged rows per phase; floats per staged channel (>= stride PH p)
    int mblocks;        // workgroups along M per group
    int flush;          // taps after which the MFMA accumulator is added to the running total and cleared
};

template <int WM, int WN, int MW, int NW, bool M16>
__global__ __launch_bounds__(256) void disc_conv_k(const GArgs a) {
    constexpr int CK = M16 ? 8 : 16;       // input channels per staged chunk
    constexpr int MTILE = M16 ? 16 : 32;
    constexpr int SPT = M16 ? CK / 4 : CK / 2;  // MFMA k steps per tap of a chunk
    constexpr int NT = WN * NW * 32;
    constexpr int NACC = M16 ? 2 * NW : NW;
    static_assert(WM * WN == 4, "four waves");
    static_assert(!M16 || (WM == 1 && MW == 1), "the 16-row form has one m tile");
    extern __shared__ float lds[];
    int* tab = reinterpret_cast<int*>(lds);
    float* xs = lds + a.spanp;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int g = blockIdx.y / a.mblocks, mb = blockIdx.y - g * a.mblocks;
    const int p = a.p, s = a.stride, PH = a.PH, spanp = a.spanp;
    const int n0 = blockIdx.x * NT, h0 = n0 / p, jrel0 = n0 - h0 * p;
    const int flat0 = (s * h0 - a.pad) * p;  // flat input index of the span's first element (may be negative: zero padding)
    const int span = s * PH * p;
    for (int e = tid; e < span; e += 256) {
        const int r = e / p, w = e - r * p, q = r / s, ph = r - q * s;
        tab[e] = (ph * PH + q) * p + w;
    }
    const float* xb = a.x + (long)blockIdx.z * a.x_row + (long)g * a.cin_g * a.Lin;
    const int mt_total = a.cout_g / MTILE;
    const int mt0 = mb * (WM * MW) + wm * MW;
    const int steps = a.nch * a.k;  // taps of all chunks: the weight stream's length per m tile
    const long mt_stride = (long)steps * 64 * SPT;
    const float* wq = a.wp + ((long)g * mt_total + mt0) * mt_stride + lane * SPT;

    typedef typename std::conditional<M16, f32x4, f32x16>::type acc_t;
    // Two-level sum: the MFMAs accumulate `flush` taps of a chunk (64 - 128 terms), then the partial goes into `tot` on the VALU.  One fp32
    // chain over all K (5120 terms in the 1024 -> 1024 layers) alone uses up the parity bound of 4 x the reference's fp32 error; with
    // partials of ~sqrt(K) terms the error is 6 - 10 x smaller (measured in a CPU restatement of this order).
    acc_t acc[MW][NACC], tot[MW][NACC];
#pragma unroll
    for (int i = 0; i < MW; ++i)
#pragma unroll
        for (int j = 0; j < NACC; ++j)
#pragma unroll
            for (int r = 0; r < (M16 ? 4 : 16); ++r) acc[i][j][r] = 0.0f, tot[i][j][r] = 0.0f;
    auto flush_acc = [&]() {
#pragma unroll
        for (int i = 0; i < MW; ++i)
#pragma unroll
            for (int j = 0; j < NACC; ++j)
#pragma unroll
                for (int r = 0; r < (M16 ? 4 : 16); ++r) tot[i][j][r] += acc[i][j][r], acc[i][j][r] = 0.0f;
    };

    float av[MW][SPT], an[MW][SPT];
    auto load_a = [&](int step, float (&dst)[MW][SPT]) {
#pragma unroll
        for (int mw = 0; mw < MW; ++mw) {
            const float* src = wq + mw * mt_stride + (long)step * 64 * SPT;
            if constexpr (SPT == 8) {
                const float4 u = *reinterpret_cast<const float4*>(src), v = *reinterpret_cast<const float4*>(src + 4);
                dst[mw][0] = u.x, dst[mw][1] = u.y, dst[mw][2] = u.z, dst[mw][3] = u.w;
                dst[mw][4] = v.x, dst[mw][5] = v.y, dst[mw][6] = v.z, dst[mw][7] = v.w;
            } else {
                const float2 u = *reinterpret_cast<const float2*>(src);
                dst[mw][0] = u.x, dst[mw][1] = u.y;
            }
        }
    };
    load_a(0, an);

    const int ksel = M16 ? lane >> 4 : lane >> 5;   // which k of the step this lane supplies
    const int col = M16 ? lane & 15 : lane & 31;
    const float* bq = xs + ksel * spanp + jrel0 + wn * NW * 32 + col;
    int step = 0, since = 0;
    for (int ch = 0; ch < a.nch; ++ch) {
        __syncthreads();  // the table is complete / every wave is done with the previous chunk
        for (int c = wave; c < CK; c += 4) {
            const float* xc = xb + (long)(ch * CK + c) * a.Lin;
            float* dst = xs + c * spanp;
            for (int e = lane; e < span; e += 64) {
                const int f = flat0 + e;
                dst[tab[e]] = (f >= 0 && f < a.Lin) ? xc[f] : 0.0f;
            }
        }
        __syncthreads();
        int ph = 0, q = 0;
        for (int t = 0; t < a.k; ++t, ++step) {
#pragma unroll
            for (int mw = 0; mw < MW; ++mw)
#pragma unroll
                for (int j = 0; j < SPT; ++j) av[mw][j] = an[mw][j];
            load_a(step + 1 < steps ? step + 1 : step, an);  // one tap ahead; the last one re-reads itself
            const float* bt = bq + (ph * PH + q) * p;
            if (++ph == s) ph = 0, ++q;
#pragma unroll
            for (int j = 0; j < SPT; ++j) {
                float b[NACC];
                if constexpr (M16) {
#pragma unroll
                    for (int nt = 0; nt < NACC; ++nt) b[nt] = bt[4 * j * spanp + 16 * nt];
#pragma unroll
                    for (int nt = 0; nt < NACC; ++nt) acc[0][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[0][j], b[nt], acc[0][nt], 0, 0, 0);
                } else {
#pragma unroll
                    for (int nt = 0; nt < NACC; ++nt) b[nt] = bt[2 * j * spanp + 32 * nt];
#pragma unroll
                    for (int mw = 0; mw < MW; ++mw)
#pragma unroll
                        for (int nt = 0; nt < NACC; ++nt) acc[mw][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mw][j], b[nt], acc[mw][nt], 0, 0, 0);
                }
            }
            if (++since == a.flush) {
                flush_acc();
                since = 0;
            }
        }
    }
    flush_acc();

    // ---- epilogue: bias, LeakyReLU, store.  C/D: 32x32 col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5); 16x16 col = lane & 15, row = 4 (lane >> 4) + r
    float* yb = a.y + (long)blockIdx.z * a.y_row + (long)g * a.cout_g * a.Nout;
    const float* bias = a.bias + g * a.cout_g;
#pragma unroll
    for (int mw = 0; mw < MW; ++mw)
#pragma unroll
        for (int nt = 0; nt < NACC; ++nt) {
            const int n = n0 + wn * NW * 32 + nt * MTILE + col;
#pragma unroll
            for (int r = 0; r < (M16 ? 4 : 16); ++r) {
                const int m = (mt0 + mw) * MTILE + (M16 ? 4 * ksel + r : (r & 3) + 8 * (r >> 2) + 4 * ksel);
                float v = tot[mw][nt][r] + bias[m];
                v = v > 0.0f ? v : SLOPE * v;
                if (n < a.Nout) yb[(long)m * a.Nout + n] = v;
            }
        }
}

// ---- first layers (Cin = 1) -------------------------------------------------------------------------------------------------------
// MPD: out[n][c][h'][w] = lrelu(b[c] + sum_t w[c][t] x[3 h' + t - 2][w]),  x[h][w] = y[h p + w] reflected once at the row's end
__global__ __launch_bounds__(256) void mpd_first_k(const float* __restrict__ y, int T, int p, int H0, int Hout, const float* __restrict__ w,
                                                   const float* __restrict__ bias, float* __restrict__ out) {
    const int n = blockIdx.x * 256 + threadIdx.x, Nout = Hout * p;
    if (n >= Nout) return;
    const int h = n / p, col = n - h * p;
    const float* yr = y + (long)blockIdx.y * T;
    float x[5];
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        const int r = 3 * h + t - 2;
        float v = 0.0f;
        if (r >= 0 && r < H0) {
            int i = r * p + col;
            if (i >= T) i = 2 * (T - 1) - i;
            v = yr[i];
        }
        x[t] = v;
    }
    float* o = out + (long)blockIdx.y * 32 * Nout + n;
#pragma clang loop vectorize(disable)  // no packed-f32 VALU in this library (build.py)
    for (int c = 0; c < 32; ++c) {
        float acc = 0.0f;
#pragma unroll
        for (int t = 0; t < 5; ++t) acc = fmaf(w[c * 5 + t], x[t], acc);
        acc += bias[c];
        o[(long)c * Nout] = acc > 0.0f ? acc : SLOPE * acc;
    }
}

// AvgPool1d(4, 2, padding = 2), padding counted: pooled[j] = (x[2j - 2] + x[2j - 1] + x[2j] + x[2j + 1]) / 4, zeros outside
__device__ __forceinline__ float at0(const float* y, int T, int i) { return (i >= 0 && i < T) ? y[i] : 0.0f; }
__device__ __forceinline__ float pool1(const float* y, int T, int L1, int j) {
    if (j < 0 || j >= L1) return 0.0f;
    return ((at0(y, T, 2 * j - 2) + at0(y, T, 2 * j - 1)) + (at0(y, T, 2 * j) + at0(y, T, 2 * j + 1))) * 0.25f;
}
__device__ __forceinline__ float pool2(const float* y, int T, int L1, int L2, int j) {
    if (j < 0 || j >= L2) return 0.0f;
    return ((pool1(y, T, L1, 2 * j - 2) + pool1(y, T, L1, 2 * j - 1)) + (pool1(y, T, L1, 2 * j) + pool1(y, T, L1, 2 * j + 1))) * 0.25f;
}

// MSD: out[n][c][l] = lrelu(b[c] + sum_t w[c][t] x[l + t - 7]), x = the scale's pooled input
__global__ __launch_bounds__(256) void msd_first_k(const float* __restrict__ y, int T, int scale, int L, const float* __restrict__ w,
                                                   const float* __restrict__ bias, float* __restrict__ out) {
    __shared__ float xs[256 + 14];
    const float* yr = y + (long)blockIdx.y * T;
    const int l0 = blockIdx.x * 256, L1 = T / 2 + 1;
    for (int i = threadIdx.x; i < 256 + 14; i += 256) {
        const int j = l0 + i - 7;
        xs[i] = scale == 0 ? at0(yr, T, j) : scale == 1 ? pool1(yr, T, L, j) : pool2(yr, T, L1, L, j);
    }
    __syncthreads();
    const int l = l0 + threadIdx.x;
    if (l >= L) return;
    float x[15];
#pragma unroll
    for (int t = 0; t < 15; ++t) x[t] = xs[threadIdx.x + t];
    float* o = out + (long)blockIdx.y * 128 * L + l;
#pragma clang loop vectorize(disable)
    for (int c = 0; c < 128; ++c) {
        float acc = 0.0f;
#pragma unroll
        for (int t = 0; t < 15; ++t) acc = fmaf(w[c * 15 + t], x[t], acc);
        acc += bias[c];
        o[(long)c * L] = acc > 0.0f ? acc : SLOPE * acc;
    }
}

// ---- conv_post: out[n][pos] = b + sum_c sum_t w[c][t] x[c][pos + (t - 1) p] ----------------------------------------------------------
__global__ __launch_bounds__(256) void disc_post_k(const float* __restrict__ x, int C, int Npos, int p, const float* __restrict__ w,
                                                   const float* __restrict__ bias, float* __restrict__ fmap, float* __restrict__ score) {
    __shared__ double part[4][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pos = blockIdx.x * 64 + lane;
    const float* xr = x + (long)blockIdx.y * C * Npos;
    const bool ok0 = pos - p >= 0 && pos - p < Npos, ok1 = pos < Npos, ok2 = pos + p < Npos;
    // double accumulators: 3072 terms whose sum is small against the terms; the layer is 0.02 % of the pass's arithmetic
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const int cw = C / 4;
    for (int c = wave * cw; c < (wave + 1) * cw; c += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float* xc = xr + (long)(c + u) * Npos + pos;
            const float* wc = w + (c + u) * 3;
            const float x0 = ok0 ? xc[-p] : 0.0f, x1 = ok1 ? xc[0] : 0.0f, x2 = ok2 ? xc[p] : 0.0f;
            acc[u] = fma((double)wc[2], (double)x2, fma((double)wc[1], (double)x1, fma((double)wc[0], (double)x0, acc[u])));
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) part[wave][u][lane] = acc[u];
    __syncthreads();
    if (wave == 0 && ok1) {
        double v = 0.0;
#pragma unroll
        for (int wv = 0; wv < 4; ++wv) v += (part[wv][0][lane] + part[wv][1][lane]) + (part[wv][2][lane] + part[wv][3][lane]);
        const float r = (float)(v + (double)bias[0]);
        fmap[(long)blockIdx.y * Npos + pos] = r;
        score[(long)blockIdx.y * Npos + pos] = r;
    }
}

// ---- losses -----------------------------------------------------------------------------------------------------------------------
struct LossArgs {
    long off[NRED];  // feature maps: float offset of the real half in the feature-map buffer; scores: of the real half in the score buffer
    long cnt[NRED];  // elements of one half (B rows)
};

__device__ __forceinline__ double block_sum(double v, double* sh) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) sh[tid] += sh[tid + w];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// grid (NPART, NRED): workgroup (b, i) reduces slice b of tensor i.  i < 54: |r - g| of a feature map; then per discriminator d the three
// score sums (1 - d_r)^2, d_g^2, (1 - d_g)^2 as tensors 54 + 3 d + {0, 1, 2}.
__global__ __launch_bounds__(256) void loss_stage1_k(const float* __restrict__ fmaps, const float* __restrict__ scores, const LossArgs a,
                                                     double* __restrict__ partial) {
    __shared__ double sh[256];
    const int i = blockIdx.y, b = blockIdx.x;
    const long cnt = a.cnt[i], chunk = (cnt + NPART - 1) / NPART;
    const long lo = b * chunk, hi = lo + chunk < cnt ? lo + chunk : cnt;
    double acc = 0.0;
    if (i < VTTS_DISC_NUM_FMAPS) {
        const float* r = fmaps + a.off[i];
        const float* g = r + cnt;
        for (long e = lo + threadIdx.x; e < hi; e += 256) acc += (double)fabsf(r[e] - g[e]);
    } else {
        const int which = (i - VTTS_DISC_NUM_FMAPS) % 3;
        const float* r = scores + a.off[i];
        const float* g = r + cnt;
        for (long e = lo + threadIdx.x; e < hi; e += 256) {
            const float v = which == 0 ? 1.0f - r[e] : which == 1 ? g[e] : 1.0f - g[e];
            acc += (double)(v * v);
        }
    }
    const double tot = block_sum(acc, sh);
    if (threadIdx.x == 0) partial[(long)i * NPART + b] = tot;
}

__global__ __launch_bounds__(128) void loss_stage2_k(const LossArgs a, const double* __restrict__ partial, float* __restrict__ out) {
    __shared__ double mean[NRED];
    const int i = threadIdx.x;
    if (i < NRED) {
        double s = 0.0;
        for (int b = 0; b < NPART; ++b) s += partial[(long)i * NPART + b];
        mean[i] = s / (double)a.cnt[i];
    }
    __syncthreads();
    if (i < VTTS_DISC_NUM_FMAPS) out[VTTS_DISC_LOSS_FMAP + i] = (float)mean[i];
    if (i < NDISC) {
        out[VTTS_DISC_LOSS_REAL + i] = (float)mean[VTTS_DISC_NUM_FMAPS + 3 * i];
        out[VTTS_DISC_LOSS_FAKE + i] = (float)mean[VTTS_DISC_NUM_FMAPS + 3 * i + 1];
        out[VTTS_DISC_LOSS_GEN + i] = (float)mean[VTTS_DISC_NUM_FMAPS + 3 * i + 2];
    }
    if (i == 0) {
        double fm[2] = {0, 0}, dl[2] = {0, 0}, gl[2] = {0, 0};
        for (int f = 0; f < VTTS_DISC_NUM_FMAPS; ++f) fm[f >= 30] += mean[f];
        for (int d = 0; d < NDISC; ++d) {
            dl[d >= 5] += mean[VTTS_DISC_NUM_FMAPS + 3 * d] + mean[VTTS_DISC_NUM_FMAPS + 3 * d + 1];
            gl[d >= 5] += mean[VTTS_DISC_NUM_FMAPS + 3 * d + 2];
        }
        float* t = out + VTTS_DISC_LOSS_TOTALS;
        t[0] = (float)(2.0 * fm[0]), t[1] = (float)(2.0 * fm[1]);
        t[2] = (float)dl[0], t[3] = (float)dl[1];
        t[4] = (float)gl[0], t[5] = (float)gl[1];
        t[6] = (float)(2.0 * fm[0] + 2.0 * fm[1]), t[7] = (float)(dl[0] + dl[1]), t[8] = (float)(gl[0] + gl[1]);
        for (int z = VTTS_DISC_LOSS_TOTALS + 9; z < VTTS_DISC_LOSS_RESULTS; ++z) out[z] = 0.0f;
    }
}

// ---- host: the layer table and the geometry ----------------------------------------------------------------------------------------
std::vector<ConvSpec> make_specs() {
    std::vector<ConvSpec> v;
    auto add = [&](const std::string& key, int disc, int kind, int cin, int cout, int k, int stride, int pad, int groups) {
        v.push_back(ConvSpec{key, disc, kind, cin, cout, k, stride, pad, groups, 0, 0});
    };
    for (int d = 0; d < 5; ++d) {
        const std::string base = "mpd.discriminators." + std::to_string(d);
        const int ch[5] = {1, 32, 128, 512, 1024};
        for (int l = 0; l < 4; ++l) add(base + ".convs." + std::to_string(l), d, l == 0 ? K_MPD_FIRST : K_GEMM, ch[l], ch[l + 1], 5, 3, 2, 1);
        add(base + ".convs.4", d, K_GEMM, 1024, 1024, 5, 1, 2, 1);
        add(base + ".conv_post", d, K_POST, 1024, 1, 3, 1, 1, 1);
    }
    for (int sc = 0; sc < 3; ++sc) {
        const std::string base = "msd.discriminators." + std::to_string(sc);
        const int d = 5 + sc;
        add(base + ".convs.0", d, K_MSD_FIRST, 1, 128, 15, 1, 7, 1);
        add(base + ".convs.1", d, K_GEMM, 128, 128, 41, 2, 20, 4);
        add(base + ".convs.2", d, K_GEMM, 128, 256, 41, 2, 20, 16);
        add(base + ".convs.3", d, K_GEMM, 256, 512, 41, 4, 20, 16);
        add(base + ".convs.4", d, K_GEMM, 512, 1024, 41, 4, 20, 16);
        add(base + ".convs.5", d, K_GEMM, 1024, 1024, 41, 1, 20, 16);
        add(base + ".convs.6", d, K_GEMM, 1024, 1024, 5, 1, 2, 1);
        add(base + ".conv_post", d, K_POST, 1024, 1, 3, 1, 1, 1);
    }
    size_t off = 0;
    for (auto& c : v) {
        c.w_off = off;
        off += ((size_t)c.cout * (c.cin / c.groups) * c.k + 63) / 64 * 64;
        c.b_off = off;
        off += ((size_t)c.cout + 63) / 64 * 64;
    }
    return v;
}

struct FmapGeom {
    int64_t C, L, cols, offset;  // [N][C][L][cols] at `offset` floats
};

// the 54 maps of N rows of T samples; returns the buffer's size in floats
int64_t fmap_geometry(const std::vector<ConvSpec>& specs, int N, int64_t T, FmapGeom* out) {
    int64_t off = 0, L = 0;
    for (int i = 0; i < NCONV; ++i) {
        const ConvSpec& c = specs[i];
        int64_t cols = 1;
        if (c.disc < 5) {
            cols = PERIODS[c.disc];
            if (c.kind == K_MPD_FIRST) L = (T + cols - 1) / cols;
        } else if (c.kind == K_MSD_FIRST) {
            L = T;
            for (int sc = 5; sc < c.disc; ++sc) L = L / 2 + 1;
        }
        L = (L + 2 * c.pad - c.k) / c.stride + 1;
        out[i] = FmapGeom{c.cout, L, cols, off};
        off += ((int64_t)N * c.cout * L * cols + 63) / 64 * 64;
    }
    return off;
}

vtts::DynLdsOnce g_lds_once[8];

template <int WM, int WN, int MW, int NW, bool M16>
hipError_t launch_gemm(GArgs a, int N, int slot, hipStream_t s) {
    constexpr int CK = M16 ? 8 : 16, MTILE = M16 ? 16 : 32, BM = WM * MW * MTILE, NT = WN * NW * 32;
    const int HH = (NT + a.p - 2) / a.p + 1;  // output rows a tile of NT flat positions can touch
    a.PH = HH + (a.k - 1) / a.stride;
    a.spanp = a.stride * a.PH * a.p;
    a.spanp = M16 ? (a.spanp + 31) / 32 * 32 + 16 : (a.spanp + 3) / 4 * 4;  // 16-row form: a half's two channels 16 banks apart
    a.nch = a.cin_g / CK;
    a.mblocks = a.cout_g / BM;
    a.flush = a.k <= 8 ? a.k : 8;
    const size_t lds = (size_t)(CK + 1) * a.spanp * sizeof(float);
    const void* fn = reinterpret_cast<const void*>(&disc_conv_k<WM, WN, MW, NW, M16>);
    hipError_t e = vtts::set_max_dynamic_lds(fn, 96 * 1024, g_lds_once[slot]);
    if (e != hipSuccess) return e;
    if (lds > 96 * 1024) return hipErrorInvalidValue;
    const int groups_y = a.mblocks * (int)(a.x_row / ((long)a.cin_g * a.Lin));
    const dim3 grid((unsigned)((a.Nout + NT - 1) / NT), (unsigned)groups_y, (unsigned)N);
    hipLaunchKernelGGL((disc_conv_k<WM, WN, MW, NW, M16>), grid, dim3(256), lds, s, a);
    return hipGetLastError();
}

}  // namespace

struct vtts_disc {
    int device = 0;
    std::vector<ConvSpec> specs;
    std::vector<float> img;  // the blob's host image, allocated at the first set_param
    size_t blob_floats = 0;
    bool have[2 * NCONV] = {};
    const float* blob = nullptr;
};

VTTS_API int vtts_disc_create(int device, vtts_disc** out) {
    if (!out) return failf(VTTS_ERR_INVALID, "null argument");
    auto* h = new (std::nothrow) vtts_disc();
    if (!h) return failf(VTTS_ERR_NOMEM, "host allocation failed");
    h->device = device;
    h->specs = make_specs();
    h->blob_floats = h->specs.back().b_off + 64;
    *out = h;
    return VTTS_OK;
}

VTTS_API void vtts_disc_destroy(vtts_disc* h) { delete h; }

VTTS_API int vtts_disc_num_params(const vtts_disc* h, int* n) {
    if (!h || !n) return failf(VTTS_ERR_INVALID, "null argument");
    *n = 2 * NCONV;
    return VTTS_OK;
}

VTTS_API int vtts_disc_param_info(const vtts_disc* h, int i, const char** key, const char** which, int64_t shape[3], int* ndim) {
    if (!h || !key || !which || !shape || !ndim) return failf(VTTS_ERR_INVALID, "null argument");
    if (i < 0 || i >= 2 * NCONV) return failf(VTTS_ERR_INVALID, "parameter index %d is outside 0 .. %d", i, 2 * NCONV - 1);
    const ConvSpec& c = h->specs[i / 2];
    *key = c.key.c_str();
    if (i % 2 == 0) {
        *which = "w";
        shape[0] = c.cout, shape[1] = c.cin / c.groups, shape[2] = c.k;
        *ndim = 3;
    } else {
        *which = "b";
        shape[0] = c.cout, shape[1] = shape[2] = 0;
        *ndim = 1;
    }
    return VTTS_OK;
}

VTTS_API int vtts_disc_set_param(vtts_disc* h, const char* key, const char* which, const float* host, const int64_t* shape, int ndim) {
    if (!h || !key || !which || !host || !shape) return failf(VTTS_ERR_INVALID, "null argument");
    int ci = -1;
    for (int i = 0; i < NCONV; ++i)
        if (h->specs[i].key == key) ci = i;
    if (ci < 0) return failf(VTTS_ERR_INVALID, "unknown module '%s'", key);
    const ConvSpec& c = h->specs[ci];
    const bool is_w = !strcmp(which, "w");
    if (!is_w && strcmp(which, "b")) return failf(VTTS_ERR_INVALID, "which must be \"w\" or \"b\" (got '%s')", which);
    const int cin_g = c.cin / c.groups;
    if (is_w) {
        const bool ok = (ndim == 3 || (ndim == 4 && shape[3] == 1)) && shape[0] == c.cout && shape[1] == cin_g && shape[2] == c.k;
        if (!ok) return failf(VTTS_ERR_SHAPE, "%s: weight must be [%d, %d, %d]", key, c.cout, cin_g, c.k);
    } else if (ndim != 1 || shape[0] != c.cout) {
        return failf(VTTS_ERR_SHAPE, "%s: bias must be [%d]", key, c.cout);
    }
    if (h->img.empty()) {
        try {
            h->img.assign(h->blob_floats, 0.0f);
        } catch (const std::bad_alloc&) {
            return failf(VTTS_ERR_NOMEM, "host allocation of the %zu-byte weight image failed", h->blob_floats * sizeof(float));
        }
    }
    if (!is_w) {
        memcpy(h->img.data() + c.b_off, host, (size_t)c.cout * sizeof(float));
    } else if (c.kind != K_GEMM) {
        memcpy(h->img.data() + c.w_off, host, (size_t)c.cout * cin_g * c.k * sizeof(float));
    } else {
        // A-fragment order [group][m tile][chunk][tap][lane][k step]: lane l of step j supplies W[m0 + (l & 31)][chunk CK + 2 j + (l >> 5)][tap]
        // (16-row form: W[m0 + (l & 15)][chunk CK + 4 j + (l >> 4)][tap])
        const int cout_g = c.cout / c.groups;
        const bool m16 = cout_g == 16;
        const int CK = m16 ? 8 : 16, MT = m16 ? 16 : 32, SPT = m16 ? 2 : 8, KS = m16 ? 4 : 2;
        const int nch = cin_g / CK, mtiles = cout_g / MT;
        float* dst = h->img.data() + c.w_off;
        for (int g = 0; g < c.groups; ++g)
            for (int mt = 0; mt < mtiles; ++mt)
                for (int ch = 0; ch < nch; ++ch)
                    for (int t = 0; t < c.k; ++t)
                        for (int l = 0; l < 64; ++l) {
                            const int m = g * cout_g + mt * MT + (m16 ? l & 15 : l & 31), ksel = m16 ? l >> 4 : l >> 5;
                            for (int j = 0; j < SPT; ++j) *dst++ = host[((size_t)m * cin_g + ch * CK + KS * j + ksel) * c.k + t];
                        }
    }
    h->have[2 * ci + (is_w ? 0 : 1)] = true;
    return VTTS_OK;
}

VTTS_API int vtts_disc_packed_bytes(const vtts_disc* h, size_t* bytes) {
    if (!h || !bytes) return failf(VTTS_ERR_INVALID, "null argument");
    *bytes = h->blob_floats * sizeof(float);
    return VTTS_OK;
}

VTTS_API int vtts_disc_pack(vtts_disc* h, void* dev_blob, size_t blob_bytes, void* stream) {
    if (!h) return failf(VTTS_ERR_INVALID, "null argument");
    const size_t need = h->blob_floats * sizeof(float);
    if (int rc = check_blob(dev_blob, blob_bytes, need)) return rc;
    for (int i = 0; i < 2 * NCONV; ++i)
        if (!h->have[i]) return failf(VTTS_ERR_MISSING, "parameter %s/%s was never set", h->specs[i / 2].key.c_str(), i % 2 ? "b" : "w");
    if (int rc = upload_blob(dev_blob, h->img.data(), need, static_cast<hipStream_t>(stream), "the discriminator weights")) return rc;
    h->blob = static_cast<const float*>(dev_blob);
    std::vector<float>().swap(h->img);  // 283 MB of host memory; a later set_param starts a new image
    memset(h->have, 0, sizeof(h->have));
    return VTTS_OK;
}

VTTS_API int vtts_disc_bind_packed(vtts_disc* h, void* dev_blob, size_t blob_bytes) {
    if (!h) return failf(VTTS_ERR_INVALID, "null argument");
    if (int rc = check_blob(dev_blob, blob_bytes, h->blob_floats * sizeof(float))) return rc;
    h->blob = static_cast<const float*>(dev_blob);
    return VTTS_OK;
}

static int check_shape(int N, int64_t T) {
    if (N < 1) return failf(VTTS_ERR_INVALID, "N must be positive (got %d)", N);
    if (N > 65535) return failf(VTTS_ERR_INVALID, "at most 65535 rows per call (got %d)", N);
    if (T < VTTS_DISC_MIN_SAMPLES)
        return failf(VTTS_ERR_SHAPE, "a row needs at least %d samples for period 11's reflection padding (got %lld)", VTTS_DISC_MIN_SAMPLES, (long long)T);
    if (T > MAX_T) return failf(VTTS_ERR_SHAPE, "rows longer than %lld samples are not supported (got %lld)", (long long)MAX_T, (long long)T);
    return VTTS_OK;
}

VTTS_API int vtts_disc_workspace_bytes(const vtts_disc* h, int N, int64_t T, size_t* bytes) {
    if (!h || !bytes) return failf(VTTS_ERR_INVALID, "null argument");
    if (int rc = check_shape(N, T)) return rc;
    *bytes = 0;
    return VTTS_OK;
}

VTTS_API int vtts_disc_num_fmaps(const vtts_disc* h, int* n) {
    if (!h || !n) return failf(VTTS_ERR_INVALID, "null argument");
    *n = VTTS_DISC_NUM_FMAPS;
    return VTTS_OK;
}

VTTS_API int vtts_disc_fmap_info(const vtts_disc* h, int i, int N, int64_t T, int64_t* C_, int64_t* L, int64_t* columns, int64_t* offset) {
    if (!h || !C_ || !L || !columns || !offset) return failf(VTTS_ERR_INVALID, "null argument");
    if (i < 0 || i >= VTTS_DISC_NUM_FMAPS) return failf(VTTS_ERR_INVALID, "feature map index %d is outside 0 .. %d", i, VTTS_DISC_NUM_FMAPS - 1);
    if (int rc = check_shape(N, T)) return rc;
    FmapGeom g[NCONV];
    fmap_geometry(h->specs, N, T, g);
    *C_ = g[i].C, *L = g[i].L, *columns = g[i].cols, *offset = g[i].offset;
    return VTTS_OK;
}

VTTS_API int vtts_disc_forward(vtts_disc* h, const float* y_dev, int N, int64_t T64, float* fmaps_dev, float* scores_dev, void* workspace,
                               void* stream) {
    (void)workspace;
    if (!h || !y_dev || !fmaps_dev || !scores_dev) return failf(VTTS_ERR_INVALID, "null argument");
    if (!h->blob) return failf(VTTS_ERR_STATE, "forward() before pack()/bind_packed()");
    if (int rc = check_shape(N, T64)) return rc;
    const int T = (int)T64;
    hipStream_t s = static_cast<hipStream_t>(stream);
    FmapGeom geo[NCONV];
    fmap_geometry(h->specs, N, T, geo);
    int64_t score_off = 0;
    hipError_t e = hipSuccess;
    for (int i = 0; i < NCONV && e == hipSuccess; ++i) {
        const ConvSpec& c = h->specs[i];
        const FmapGeom& o = geo[i];
        const float* w = h->blob + c.w_off;
        const float* b = h->blob + c.b_off;
        float* out = fmaps_dev + o.offset;
        const int p = (int)o.cols, Nout = (int)(o.L * o.cols);
        if (c.kind == K_MPD_FIRST) {
            const int H0 = (T + p - 1) / p;
            hipLaunchKernelGGL(mpd_first_k, dim3((Nout + 255) / 256, N), dim3(256), 0, s, y_dev, T, p, H0, (int)o.L, w, b, out);
            e = hipGetLastError();
        } else if (c.kind == K_MSD_FIRST) {
            hipLaunchKernelGGL(msd_first_k, dim3((Nout + 255) / 256, N), dim3(256), 0, s, y_dev, T, c.disc - 5, (int)o.L, w, b, out);
            e = hipGetLastError();
        } else if (c.kind == K_POST) {
            const FmapGeom& in = geo[i - 1];
            hipLaunchKernelGGL(disc_post_k, dim3((Nout + 63) / 64, N), dim3(256), 0, s, fmaps_dev + in.offset, c.cin, Nout, p, w, b, out,
                               scores_dev + score_off);
            e = hipGetLastError();
            score_off += (int64_t)N * Nout;
        } else {
            const FmapGeom& in = geo[i - 1];
            GArgs a{};
            a.x = fmaps_dev + in.offset, a.y = out, a.wp = w, a.bias = b;
            a.cin_g = c.cin / c.groups, a.cout_g = c.cout / c.groups, a.k = c.k, a.stride = c.stride, a.pad = c.pad, a.p = p;
            a.Lin = (int)(in.L * in.cols), a.Nout = Nout;
            a.x_row = (long)c.cin * a.Lin, a.y_row = (long)c.cout * Nout;
            const bool wide = Nout > 64;  // one 128-position tile instead of two 64-position ones: half the weight traffic
            if (a.cout_g >= 512)
                e = wide ? launch_gemm<4, 1, 2, 4, false>(a, N, 0, s) : launch_gemm<4, 1, 2, 2, false>(a, N, 1, s);
            else if (a.cout_g == 128)
                e = wide ? launch_gemm<4, 1, 1, 4, false>(a, N, 2, s) : launch_gemm<4, 1, 1, 2, false>(a, N, 3, s);
            else if (a.cout_g == 64)
                e = launch_gemm<2, 2, 1, 2, false>(a, N, 4, s);
            else if (a.cout_g == 32)
                e = launch_gemm<1, 4, 1, 2, false>(a, N, 5, s);
            else
                e = launch_gemm<1, 4, 1, 2, true>(a, N, 6, s);
        }
    }
    if (e != hipSuccess) return failf(VTTS_ERR_HIP, "discriminator kernel launch failed: %s", hipGetErrorString(e));
    return VTTS_OK;
}

VTTS_API int vtts_disc_losses(vtts_disc* h, const float* fmaps_dev, const float* scores_dev, int B, int64_t T, float* out_dev, void* stream) {
    if (!h || !fmaps_dev || !scores_dev || !out_dev) return failf(VTTS_ERR_INVALID, "null argument");
    if (B < 1) return failf(VTTS_ERR_INVALID, "B must be positive (got %d)", B);
    if (int rc = check_shape(2 * B, T)) return rc;
    if (reinterpret_cast<uintptr_t>(out_dev) % 8) return failf(VTTS_ERR_INVALID, "the loss buffer must be 8-byte aligned");
    FmapGeom geo[NCONV];
    fmap_geometry(h->specs, 2 * B, T, geo);
    LossArgs a;
    int64_t score_off = 0;
    int d = 0;
    for (int i = 0; i < NCONV; ++i) {
        a.off[i] = geo[i].offset;
        a.cnt[i] = (int64_t)B * geo[i].C * geo[i].L * geo[i].cols;
        if (h->specs[i].kind == K_POST) {
            for (int q = 0; q < 3; ++q) a.off[NCONV + 3 * d + q] = score_off, a.cnt[NCONV + 3 * d + q] = a.cnt[i];
            score_off += 2 * a.cnt[i];
            ++d;
        }
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* partial = reinterpret_cast<double*>(out_dev + VTTS_DISC_LOSS_RESULTS);
    hipLaunchKernelGGL(loss_stage1_k, dim3(NPART, NRED), dim3(256), 0, s, fmaps_dev, scores_dev, a, partial);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        hipLaunchKernelGGL(loss_stage2_k, dim3(1), dim3(128), 0, s, a, static_cast<const double*>(partial), out_dev);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return failf(VTTS_ERR_HIP, "loss kernel launch failed: %s", hipGetErrorString(e));
    return VTTS_OK;
}
