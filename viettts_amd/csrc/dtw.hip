// Batched dynamic time warping (include/vtts_dtw.h): L1 local cost, the three-predecessor recurrence with a fixed tie rule, an optional
// band, and the backtrace to per-row spans.  Three kernels per call, all plain fp32 VALU (L1 is not a GEMM, and the bit-exact chain is
// the point):
//
//   1. dtw_cost_k      one workgroup per (pair, TILE rows x TILE anti-diagonal steps).  The rows of a and the 2 TILE - 1 rows of b the tile
//                      meets are staged in LDS (row pitch D | 1: the lanes of a wave read consecutive rows, an odd pitch spreads them
//                      over the 64 banks); a thread runs 16 whole chains for one row.  The tile is written in the SKEWED order
//                      [strip][step = j + l][l], l = i % STRIP, which is the order the wavefront reads: a step of a strip is one
//                      contiguous kilobyte, and the wave's store here is a contiguous 256 bytes.  Tiles outside the lengths or the band return
//                      at once.
//   2. dtw_wavefront_k one workgroup of STRIP threads per pair.  Thread l owns row i0 + l and is at column step - l; its `up` neighbour's
//                      value goes through a double-buffered LDS array (the diagonal one is last step's `up`, kept in a register; thread 0 feeds the boundary
//                      row into the same array, so every thread runs the same code), one
//                      __syncthreads() per anti-diagonal.  The strip's last row stays in LDS as the next strip's boundary (in place: its
//                      writer trails its reader by STRIP - 1 columns).  Costs are fetched sixteen steps ahead, so no load sits on the
//                      dependent chain.  Sixteen 2-bit codes of a row are collected in a register and stored as one dword.  With a band
//                      each row's allowed columns [jlo, jhi] are computed once per strip in int64 and the strip only runs the steps
//                      that meet them.
//   3. dtw_backtrace_k one wave per pair.  The lanes fetch a window of code words (BT_ROWS rows up, BT_WORDS words left of the current
//                      cell) into LDS, lane 0 walks while the path stays inside: one HBM round trip per >= 16 moves.
// Barriers inside a workgroup are the only synchronisation; the kernels of one call are ordered by the stream.
// The launch arguments, the band, the workspace layout, the host checks and the cost kernel's tile map (with the local metric as a parameter) are
// dtw_common.h's, shared with mcd.hip (include/vtts_mcd.h: the L2 cost over mel cepstra), which runs kernels 2 and 3 through vtts::dtw_path_launch.
#include <hip/hip_runtime.h>

#include <new>

#include "dtw_common.h"

using vtts::failf;
using vtts::band_range;
using vtts::DtwArgs;
using vtts::DtwPairs;

namespace {

constexpr int PAIRS_PER_LAUNCH = 128;
constexpr int STRIP = vtts::DTW_STRIP;
constexpr int CPW = vtts::DTW_CPW;
constexpr int BT_ROWS = VTTS_DTW_BT_ROWS;
constexpr int BT_WORDS = VTTS_DTW_BT_WORDS;
constexpr int MAXF = vtts::DTW_MAXF;
constexpr int AHEAD = 16;  // steps the wavefront fetches its costs ahead

static_assert(BT_ROWS * BT_WORDS == 64, "one code word per lane of the backtrace's wave");
static_assert(PAIRS_PER_LAUNCH == vtts::DTW_PAIRS_PER_LAUNCH, "DtwPairs (dtw_common.h) holds one launch's lengths");

// vtts_dtw.h: local cost, one link of the chain and what is stored
struct L1Metric {
    static __device__ __forceinline__ float term(float acc, float a, float b) { return acc + fabsf(a - b); }
    static __device__ __forceinline__ float finish(float acc) { return acc; }
};

// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(vtts::DTW_COST_THREADS) void dtw_cost_k(DtwArgs g, DtwPairs p) {
    extern __shared__ float lds[];
    vtts::dtw_cost_tile<L1Metric>(g, p, lds);
}

// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(STRIP) void dtw_wavefront_k(DtwArgs g, DtwPairs p) {
    __shared__ float nb[2][STRIP + 1];  // nb[step & 1][l + 1]: thread l's value of that step; slot 0: the boundary row, fed by thread 0
    __shared__ float bound[MAXF];       // the previous strip's last row
    const int n = blockIdx.x, la = p.la[n], lb = p.lb[n];
    const int l = threadIdx.x;
    const float INF = __builtin_inff();
    const float* cost = reinterpret_cast<const float*>(g.ws + (size_t)n * g.pair_bytes);
    unsigned* codes = reinterpret_cast<unsigned*>(g.ws + (size_t)n * g.pair_bytes) + g.cost_floats;

    for (int i0 = 0; i0 < la; i0 += STRIP) {
        const int i = i0 + l;
        const int last_l = (la - i0 < STRIP ? la - i0 : STRIP) - 1;
        int jlo = 1, jhi = 0, plo = 1, phi = 0, s_begin, s_end, t;
        if (i < la) band_range(i, la, lb, g.band, jlo, jhi);
        if (i0 > 0) band_range(i0 - 1, la, lb, g.band, plo, phi);  // the boundary row's allowed columns
        band_range(i0, la, lb, g.band, s_begin, t);
        band_range(i0 + last_l, la, lb, g.band, t, s_end);
        s_end += last_l;
        // the cell is allowed iff (unsigned)(j - jlo) <= width; a thread without a row or without allowed columns never is
        const unsigned width = jhi >= jlo ? (unsigned)(jhi - jlo) : 0u;
        if (jhi < jlo) jlo = 0x40000000;
        // D(i0 - 1, q), +inf outside that row's allowed columns; above row 0 the one finite value is the 0 that D(0, 0) = c(0, 0) + 0 starts from
        auto feed = [&](int q) -> float { return (q >= plo && q <= phi) ? bound[q] : (i0 == 0 && q == -1 ? 0.0f : INF); };
        nb[0][l + 1] = INF;
        nb[1][l + 1] = INF;
        float left = INF, diag = INF;
        if (l == 0) {
            nb[s_begin & 1][0] = INF;
            nb[(s_begin - 1) & 1][0] = feed(s_begin);
            diag = feed(s_begin - 1);
        }
        __syncthreads();
        const float* cs = cost + (size_t)(i0 / STRIP) * g.steps * STRIP + l;
        unsigned* crow = codes + (size_t)(i < la ? i : 0) * g.code_words;
        const bool last_row = i == la - 1;
        const unsigned s_max = (unsigned)g.steps - 1u;
        unsigned word = 0;
        float cur[AHEAD], nxt[AHEAD];
#pragma unroll
        for (int k = 0; k < AHEAD; ++k) {
            const unsigned s = (unsigned)(s_begin + k);
            cur[k] = cs[(s < s_max ? s : s_max) * (unsigned)STRIP];
        }
        for (int sb = s_begin; sb <= s_end; sb += AHEAD) {
#pragma unroll
            for (int k = 0; k < AHEAD; ++k) {
                const unsigned s = (unsigned)(sb + AHEAD + k);
                nxt[k] = cs[(s < s_max ? s : s_max) * (unsigned)STRIP];
            }
#pragma unroll
            for (int k = 0; k < AHEAD; ++k) {
                const int s = sb + k;
                if (s <= s_end) {  // uniform
                    const int j = s - l;
                    const bool active = (unsigned)(j - jlo) <= width;
                    const float up = nb[(s - 1) & 1][l];
                    float best = diag;
                    unsigned code = 0;
                    if (up < best) {
                        best = up;
                        code = 1;
                    }
                    if (left < best) {
                        best = left;
                        code = 2;
                    }
                    const float val = active ? cur[k] + best : INF;
                    diag = up;
                    left = val;
                    nb[s & 1][l + 1] = val;
                    if (l == 0) nb[s & 1][0] = feed(s + 1);
                    word |= (active ? code : 0u) << (2 * (j & (CPW - 1)));
                    if (active && ((j & (CPW - 1)) == CPW - 1 || j == jhi)) {
                        crow[j / CPW] = word;
                        word = 0;
                        if (last_row && j == jhi) g.total[n] = val;  // the corner: row la - 1 ends at column lb - 1 under every band
                    }
                    if (active && l == STRIP - 1) bound[j] = val;
                    __syncthreads();
                }
            }
#pragma unroll
            for (int k = 0; k < AHEAD; ++k) cur[k] = nxt[k];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void dtw_backtrace_k(DtwArgs g, DtwPairs p) {
    __shared__ unsigned win[BT_ROWS][BT_WORDS];
    __shared__ int pos[3];  // i, j, done
    const int n = blockIdx.x, la = p.la[n], lb = p.lb[n];
    const int lane = threadIdx.x;
    const unsigned* codes = reinterpret_cast<const unsigned*>(g.ws + (size_t)n * g.pair_bytes) + g.cost_floats;
    int* span = g.span + (size_t)n * g.ta_stride * 2;
    for (long long r = la + lane; r < g.ta_stride; r += 64) {
        span[2 * r] = -1;
        span[2 * r + 1] = -1;
    }
    int i = la - 1, j = lb - 1, len = 1, moves = la + lb - 2;  // lane 0's walk
    if (lane == 0) span[2 * i + 1] = j;
    const int wr = lane / BT_WORDS, wc = lane % BT_WORDS;
    for (int round = 0; round < la + lb; ++round) {  // every round makes at least one move
        const int wi = i, wj = j / CPW;              // the window's corner: rows wi - BT_ROWS + 1 .. wi, words wj - BT_WORDS + 1 .. wj
        const int row = wi - wr, wd = wj - wc;
        win[wr][wc] = (row >= 0 && wd >= 0) ? codes[(size_t)row * g.code_words + wd] : 0u;
        __syncthreads();
        if (lane == 0) {
            bool done = false;
            for (;;) {
                if ((i == 0 && j == 0) || moves <= 0) {
                    done = true;
                    break;
                }
                const int r = wi - i, c = wj - j / CPW;
                if (r >= BT_ROWS || c >= BT_WORDS) break;
                unsigned code = (win[r][c] >> (2 * (j & (CPW - 1)))) & 3u;
                if (i == 0)
                    code = 2;
                else if (j == 0)
                    code = 1;
                else if (code == 3)
                    code = 0;
                if (code == 2) {
                    --j;
                } else {
                    span[2 * i] = j;
                    --i;
                    if (code == 0) --j;
                    span[2 * i + 1] = j;
                }
                ++len;
                --moves;
            }
            if (done) {
                span[2 * i] = j;
                g.path_len[n] = len;
            }
            pos[0] = i;
            pos[1] = j;
            pos[2] = done;
        }
        __syncthreads();
        i = pos[0];
        j = pos[1];
        const int done = pos[2];
        __syncthreads();
        if (done) break;
    }
}

}  // namespace

void vtts::dtw_path_launch(const DtwArgs& g, const DtwPairs& pairs, int np, hipStream_t s) {
    hipLaunchKernelGGL(dtw_wavefront_k, dim3(np), dim3(STRIP), 0, s, g, pairs);
    hipLaunchKernelGGL(dtw_backtrace_k, dim3(np), dim3(64), 0, s, g, pairs);
}

struct vtts_dtw {
    vtts_dtw_cfg cfg;
    int device;
    vtts::DynLdsOnce lds_cost;
};

VTTS_API int vtts_dtw_create(const vtts_dtw_cfg* cfg, int device, vtts_dtw** out) {
    if (!cfg || !out) return failf(VTTS_ERR_INVALID, "null argument");
    if (cfg->n_feat < 1 || cfg->n_feat > VTTS_DTW_MAX_FEAT) return failf(VTTS_ERR_INVALID, "n_feat must be in 1 .. %d (got %d)", VTTS_DTW_MAX_FEAT, cfg->n_feat);
    if (cfg->band < 0) return failf(VTTS_ERR_INVALID, "band must be >= 0 (got %d)", cfg->band);
    if (cfg->max_frames < 1 || cfg->max_frames > MAXF) return failf(VTTS_ERR_INVALID, "max_frames must be in 1 .. %d (got %d)", MAXF, cfg->max_frames);
    auto* h = new (std::nothrow) vtts_dtw();
    if (!h) return failf(VTTS_ERR_NOMEM, "host allocation failed");
    h->cfg = *cfg;
    h->device = device;
    *out = h;
    return VTTS_OK;
}

VTTS_API void vtts_dtw_destroy(vtts_dtw* h) { delete h; }

VTTS_API int vtts_dtw_workspace_bytes(const vtts_dtw* h, int N, int64_t Ta_stride, int64_t Tb_stride, size_t* bytes) {
    if (!h || !bytes) return failf(VTTS_ERR_INVALID, "null argument");
    if (int rc = vtts::dtw_check_shape(h->cfg.max_frames, N, Ta_stride, Tb_stride)) return rc;
    *bytes = (size_t)N * (size_t)vtts::dtw_layout(Ta_stride, Tb_stride).pair_bytes;
    return VTTS_OK;
}

VTTS_API int vtts_dtw_forward(vtts_dtw* h, const float* a_dev, const float* b_dev, int N, int64_t Ta_stride, int64_t Tb_stride, const int32_t* la,
                              const int32_t* lb, float* total_dev, int32_t* path_len_dev, int32_t* span_dev, void* workspace, size_t workspace_bytes,
                              void* stream) {
    if (!h || !a_dev || !b_dev || !la || !lb || !total_dev || !path_len_dev || !span_dev) return failf(VTTS_ERR_INVALID, "null argument");
    DtwArgs call;
    if (int rc = vtts::dtw_check_call(h->cfg.max_frames, h->cfg.n_feat, h->cfg.band, N, Ta_stride, Tb_stride, la, lb, workspace, workspace_bytes, &call)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t lds = vtts::dtw_cost_lds_bytes(call.D);
    hipError_t e = vtts::set_max_dynamic_lds(reinterpret_cast<const void*>(&dtw_cost_k), (int)lds, h->lds_cost);
    if (e != hipSuccess) return failf(VTTS_ERR_HIP, "hipFuncSetAttribute failed: %s", hipGetErrorString(e));
    for (int n0 = 0; n0 < N; n0 += PAIRS_PER_LAUNCH) {
        const vtts::DtwSlice sl = vtts::dtw_slice(call, a_dev, b_dev, la, lb, total_dev, path_len_dev, span_dev, workspace, N, n0);
        hipLaunchKernelGGL(dtw_cost_k, sl.cost_grid, dim3(vtts::DTW_COST_THREADS), lds, s, sl.g, sl.pairs);
        vtts::dtw_path_launch(sl.g, sl.pairs, sl.np, s);
        e = hipGetLastError();
        if (e != hipSuccess) return failf(VTTS_ERR_HIP, "dtw kernel launch failed: %s", hipGetErrorString(e));
    }
    return VTTS_OK;
}
