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
#include <hip/hip_runtime.h>

#include <new>

#include "../../include/vtts_dtw.h"
#include "../../include/vtts_hifigan.h"
#include "vtts_internal.h"

using vtts::failf;

namespace {

constexpr int STRIP = VTTS_DTW_STRIP;
constexpr int TILE = VTTS_DTW_TILE;
constexpr int CPW = VTTS_DTW_CODES_PER_WORD;
constexpr int BT_ROWS = VTTS_DTW_BT_ROWS;
constexpr int BT_WORDS = VTTS_DTW_BT_WORDS;
constexpr int MAXF = VTTS_DTW_MAX_FRAMES;
constexpr int PAIRS_PER_LAUNCH = 128;
constexpr int COST_THREADS = 256;
constexpr int CELLS = TILE * TILE / COST_THREADS;  // chains per thread of the cost kernel: consecutive steps of one row
constexpr int AHEAD = 16;                          // steps the wavefront fetches its costs ahead

static_assert(STRIP % TILE == 0, "a cost tile lies in one strip");
static_assert(CELLS == 16 && COST_THREADS / TILE * CELLS == TILE, "the cost kernel's thread map");
static_assert(BT_ROWS * BT_WORDS == 64, "one code word per lane of the backtrace's wave");

struct DtwPairs {
    int la[PAIRS_PER_LAUNCH];
    int lb[PAIRS_PER_LAUNCH];
};

struct DtwArgs {
    const float* a;      // first pair of this launch
    const float* b;
    char* ws;            // first pair's workspace
    float* total;
    int* path_len;
    int* span;
    long long ta_stride, tb_stride;
    long long pair_bytes;   // workspace bytes per pair
    long long cost_floats;  // of which the cost matrix; the code words follow
    int steps;              // skewed columns per strip (vtts_dtw.h: steps)
    int code_words;         // code words per row
    int D, band;
};

__host__ __device__ inline long long floor_div(long long a, long long b) {  // b > 0
    long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// Row i's allowed columns [jlo, jhi] (vtts_dtw.h: band), exactly: j (la - 1) within R of i (lb - 1).
__device__ __forceinline__ void band_range(int i, int la, int lb, int band, int& jlo, int& jhi) {
    jlo = 0;
    jhi = lb - 1;
    if (band > 0 && la > 1) {
        const long long m = la - 1, c = (long long)i * (lb - 1), R = (long long)band * (la > lb ? la - 1 : lb - 1);
        const long long lo = -floor_div(-(c - R), m), hi = floor_div(c + R, m);  // ceil, floor
        if (lo > jlo) jlo = (int)(lo < lb ? lo : lb);
        if (hi < jhi) jhi = (int)hi;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(COST_THREADS) void dtw_cost_k(DtwArgs g, DtwPairs p) {
    extern __shared__ float lds[];
    const int n = blockIdx.z, la = p.la[n], lb = p.lb[n];
    const int i0 = blockIdx.y * TILE, s0 = blockIdx.x * TILE;
    if (i0 >= la) return;
    const int strip = i0 / STRIP, l0 = i0 % STRIP;
    const int jmin = s0 - (l0 + TILE - 1), jmax = s0 + TILE - 1 - l0;  // columns the tile's cells have
    if (jmax < 0 || jmin >= lb) return;
    const int ilast = (i0 + TILE - 1 < la ? i0 + TILE - 1 : la - 1);
    {
        int lo, hi, lo2, hi2;
        band_range(i0, la, lb, g.band, lo, hi);
        band_range(ilast, la, lb, g.band, lo2, hi2);
        if (hi2 < jmin || lo > jmax) return;  // jlo and jhi grow with i: no row of the tile has an allowed column in it
    }
    const int D = g.D, P = D | 1;
    float* A = lds;             // [TILE][P]
    float* B = lds + TILE * P;  // [2 TILE - 1][P]
    const float* a = g.a + (size_t)n * g.ta_stride * D;
    const float* b = g.b + (size_t)n * g.tb_stride * D;
    for (int idx = threadIdx.x; idx < TILE * D; idx += COST_THREADS) {
        const int r = idx / D, d = idx - r * D, i = i0 + r;
        A[r * P + d] = i < la ? a[(size_t)i * D + d] : 0.0f;
    }
    for (int idx = threadIdx.x; idx < (2 * TILE - 1) * D; idx += COST_THREADS) {
        const int r = idx / D, d = idx - r * D, j = jmin + r;
        B[r * P + d] = (j >= 0 && j < lb) ? b[(size_t)j * D + d] : 0.0f;
    }
    __syncthreads();
    const int r = threadIdx.x & (TILE - 1), k0 = (threadIdx.x / TILE) * CELLS;  // row of the tile; first of the thread's steps
    const float* ar = A + r * P;
    const float* br = B + (k0 - r + TILE - 1) * P;  // column s0 + k0 - (l0 + r), as a row of B
    float acc[CELLS];
#pragma unroll
    for (int k = 0; k < CELLS; ++k) acc[k] = 0.0f;
    for (int d = 0; d < D; ++d) {
        const float av = ar[d];
#pragma unroll
        for (int k = 0; k < CELLS; ++k) acc[k] = acc[k] + fabsf(av - br[k * P + d]);
    }
    if (i0 + r >= la) return;
    float* cost = reinterpret_cast<float*>(g.ws + (size_t)n * g.pair_bytes);
    const int l = l0 + r;
#pragma unroll
    for (int k = 0; k < CELLS; ++k) {
        const int s = s0 + k0 + k, j = s - l;
        if (j >= 0 && j < lb) cost[((size_t)strip * g.steps + s) * STRIP + l] = acc[k];
    }
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

struct vtts_dtw {
    vtts_dtw_cfg cfg;
    int device;
    vtts::DynLdsOnce lds_cost;
};

namespace {

struct Layout {
    long long steps, code_words, cost_floats, pair_bytes;
};

Layout layout(int64_t ta, int64_t tb) {
    Layout L;
    const long long strips = (ta + STRIP - 1) / STRIP;
    L.steps = (tb + STRIP - 1 + TILE - 1) / TILE * TILE;
    L.cost_floats = strips * L.steps * STRIP;
    L.code_words = (tb + CPW - 1) / CPW;
    L.pair_bytes = (4 * (L.cost_floats + ta * L.code_words) + 255) / 256 * 256;
    return L;
}

int check_shape(const vtts_dtw* h, int N, int64_t ta, int64_t tb) {
    if (N <= 0) return failf(VTTS_ERR_INVALID, "N must be positive (got %d)", N);
    if (ta < 1 || tb < 1 || ta > h->cfg.max_frames || tb > h->cfg.max_frames)
        return failf(VTTS_ERR_INVALID, "Ta_stride and Tb_stride must be in 1 .. max_frames = %d (got %lld, %lld)", h->cfg.max_frames, (long long)ta, (long long)tb);
    return VTTS_OK;
}

}  // namespace

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
    if (int rc = check_shape(h, N, Ta_stride, Tb_stride)) return rc;
    *bytes = (size_t)N * (size_t)layout(Ta_stride, Tb_stride).pair_bytes;
    return VTTS_OK;
}

VTTS_API int vtts_dtw_forward(vtts_dtw* h, const float* a_dev, const float* b_dev, int N, int64_t Ta_stride, int64_t Tb_stride, const int32_t* la,
                              const int32_t* lb, float* total_dev, int32_t* path_len_dev, int32_t* span_dev, void* workspace, size_t workspace_bytes,
                              void* stream) {
    if (!h || !a_dev || !b_dev || !la || !lb || !total_dev || !path_len_dev || !span_dev) return failf(VTTS_ERR_INVALID, "null argument");
    if (int rc = check_shape(h, N, Ta_stride, Tb_stride)) return rc;
    for (int n = 0; n < N; ++n)
        if (la[n] < 1 || la[n] > Ta_stride || lb[n] < 1 || lb[n] > Tb_stride)
            return failf(VTTS_ERR_INVALID, "pair %d: la = %d, lb = %d are outside 1 .. Ta_stride = %lld, 1 .. Tb_stride = %lld", n, la[n], lb[n],
                         (long long)Ta_stride, (long long)Tb_stride);
    const Layout L = layout(Ta_stride, Tb_stride);
    const size_t need = (size_t)N * (size_t)L.pair_bytes;
    if (!workspace || workspace_bytes < need) return failf(VTTS_ERR_NOMEM, "workspace too small: %zu < %zu bytes", workspace_bytes, need);
    if (reinterpret_cast<uintptr_t>(workspace) % 256) return failf(VTTS_ERR_INVALID, "workspace must be 256-byte aligned");

    hipStream_t s = static_cast<hipStream_t>(stream);
    const int D = h->cfg.n_feat;
    const size_t lds = (size_t)(3 * TILE - 1) * (D | 1) * sizeof(float);
    hipError_t e = vtts::set_max_dynamic_lds(reinterpret_cast<const void*>(&dtw_cost_k), (int)lds, h->lds_cost);
    if (e != hipSuccess) return failf(VTTS_ERR_HIP, "hipFuncSetAttribute failed: %s", hipGetErrorString(e));
    DtwArgs g;
    g.ta_stride = Ta_stride;
    g.tb_stride = Tb_stride;
    g.pair_bytes = L.pair_bytes;
    g.cost_floats = L.cost_floats;
    g.steps = (int)L.steps;
    g.code_words = (int)L.code_words;
    g.D = D;
    g.band = h->cfg.band;
    for (int n0 = 0; n0 < N; n0 += PAIRS_PER_LAUNCH) {  // the lengths travel as kernel arguments
        const int np = N - n0 < PAIRS_PER_LAUNCH ? N - n0 : PAIRS_PER_LAUNCH;
        DtwPairs pairs;
        int la_max = 1, lb_max = 1;
        for (int k = 0; k < PAIRS_PER_LAUNCH; ++k) {
            pairs.la[k] = k < np ? la[n0 + k] : 1;
            pairs.lb[k] = k < np ? lb[n0 + k] : 1;
            if (pairs.la[k] > la_max) la_max = pairs.la[k];
            if (pairs.lb[k] > lb_max) lb_max = pairs.lb[k];
        }
        g.a = a_dev + (size_t)n0 * Ta_stride * D;
        g.b = b_dev + (size_t)n0 * Tb_stride * D;
        g.ws = static_cast<char*>(workspace) + (size_t)n0 * L.pair_bytes;
        g.total = total_dev + n0;
        g.path_len = path_len_dev + n0;
        g.span = span_dev + (size_t)n0 * Ta_stride * 2;
        const int row_tiles = (la_max + TILE - 1) / TILE;
        const int rows_in_strip = la_max < STRIP ? la_max : STRIP;
        const int step_tiles = (lb_max + rows_in_strip - 1 + TILE - 1) / TILE;
        hipLaunchKernelGGL(dtw_cost_k, dim3(step_tiles, row_tiles, np), dim3(COST_THREADS), lds, s, g, pairs);
        hipLaunchKernelGGL(dtw_wavefront_k, dim3(np), dim3(STRIP), 0, s, g, pairs);
        hipLaunchKernelGGL(dtw_backtrace_k, dim3(np), dim3(64), 0, s, g, pairs);
        e = hipGetLastError();
        if (e != hipSuccess) return failf(VTTS_ERR_HIP, "dtw kernel launch failed: %s", hipGetErrorString(e));
    }
    return VTTS_OK;
}
