// What the two DTW front ends share (dtw.hip: include/vtts_dtw.h, the L1 cost over log-mels; mcd.hip: include/vtts_mcd.h, the L2 cost over
// mel cepstra): the workspace layout, the launch arguments, the band, the cost kernel's tile map with the local metric as a parameter, the
// host checks of a forward() call and the slicing of a batch into launches.  The wavefront and backtrace kernels live in dtw.hip alone;
// vtts::dtw_path_launch runs them over a cost matrix that is already in the workspace.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/vtts_dtw.h"
#include "../../include/vtts_hifigan.h"
#include "vtts_internal.h"

namespace vtts {

constexpr int DTW_STRIP = VTTS_DTW_STRIP;
constexpr int DTW_TILE = VTTS_DTW_TILE;
constexpr int DTW_CPW = VTTS_DTW_CODES_PER_WORD;
constexpr int DTW_MAXF = VTTS_DTW_MAX_FRAMES;
constexpr int DTW_PAIRS_PER_LAUNCH = 128;
constexpr int DTW_COST_THREADS = 256;
constexpr int DTW_CELLS = DTW_TILE * DTW_TILE / DTW_COST_THREADS;  // chains per thread of the cost kernel: consecutive steps of one row

static_assert(DTW_STRIP % DTW_TILE == 0, "a cost tile lies in one strip");
static_assert(DTW_CELLS == 16 && DTW_COST_THREADS / DTW_TILE * DTW_CELLS == DTW_TILE, "the cost kernel's thread map");

struct DtwPairs {
    int la[DTW_PAIRS_PER_LAUNCH];
    int lb[DTW_PAIRS_PER_LAUNCH];
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

// The cost kernel's body: one workgroup per (pair, TILE rows x TILE anti-diagonal steps), DTW_COST_THREADS threads, (3 TILE - 1) (D | 1)
// floats of dynamic LDS.  Metric::term(acc, a, b) is one link of the local cost's chain in ascending d, Metric::finish(acc) what is stored.
template <class Metric>
__device__ __forceinline__ void dtw_cost_tile(const DtwArgs& g, const DtwPairs& p, float* lds) {
    constexpr int STRIP = DTW_STRIP, TILE = DTW_TILE, CELLS = DTW_CELLS;
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
    for (int idx = threadIdx.x; idx < TILE * D; idx += DTW_COST_THREADS) {
        const int r = idx / D, d = idx - r * D, i = i0 + r;
        A[r * P + d] = i < la ? a[(size_t)i * D + d] : 0.0f;
    }
    for (int idx = threadIdx.x; idx < (2 * TILE - 1) * D; idx += DTW_COST_THREADS) {
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
        for (int k = 0; k < CELLS; ++k) acc[k] = Metric::term(acc[k], av, br[k * P + d]);
    }
    if (i0 + r >= la) return;
    float* cost = reinterpret_cast<float*>(g.ws + (size_t)n * g.pair_bytes);
    const int l = l0 + r;
#pragma unroll
    for (int k = 0; k < CELLS; ++k) {
        const int s = s0 + k0 + k, j = s - l;
        if (j >= 0 && j < lb) cost[((size_t)strip * g.steps + s) * STRIP + l] = Metric::finish(acc[k]);
    }
}

inline size_t dtw_cost_lds_bytes(int D) { return (size_t)(3 * DTW_TILE - 1) * (D | 1) * sizeof(float); }

struct DtwLayout {
    long long steps, code_words, cost_floats, pair_bytes;
};

inline DtwLayout dtw_layout(int64_t ta, int64_t tb) {  // vtts_dtw.h: workspace_bytes
    DtwLayout L;
    const long long strips = (ta + DTW_STRIP - 1) / DTW_STRIP;
    L.steps = (tb + DTW_STRIP - 1 + DTW_TILE - 1) / DTW_TILE * DTW_TILE;
    L.cost_floats = strips * L.steps * DTW_STRIP;
    L.code_words = (tb + DTW_CPW - 1) / DTW_CPW;
    L.pair_bytes = (4 * (L.cost_floats + ta * L.code_words) + 255) / 256 * 256;
    return L;
}

inline int dtw_check_shape(int max_frames, int N, int64_t ta, int64_t tb) {
    if (N <= 0) return failf(VTTS_ERR_INVALID, "N must be positive (got %d)", N);
    if (ta < 1 || tb < 1 || ta > max_frames || tb > max_frames)
        return failf(VTTS_ERR_INVALID, "Ta_stride and Tb_stride must be in 1 .. max_frames = %d (got %lld, %lld)", max_frames, (long long)ta, (long long)tb);
    return VTTS_OK;
}

// The refusals of a forward() call (vtts_dtw.h: forward), all host arithmetic, and the call's DtwArgs: everything but a, b, ws and the three
// results, which dtw_slice points at a launch's first pair.
inline int dtw_check_call(int max_frames, int D, int band, int N, int64_t Ta_stride, int64_t Tb_stride, const int32_t* la, const int32_t* lb,
                          const void* workspace, size_t workspace_bytes, DtwArgs* g) {
    if (int rc = dtw_check_shape(max_frames, N, Ta_stride, Tb_stride)) return rc;
    for (int n = 0; n < N; ++n)
        if (la[n] < 1 || la[n] > Ta_stride || lb[n] < 1 || lb[n] > Tb_stride)
            return failf(VTTS_ERR_INVALID, "pair %d: la = %d, lb = %d are outside 1 .. Ta_stride = %lld, 1 .. Tb_stride = %lld", n, la[n], lb[n],
                         (long long)Ta_stride, (long long)Tb_stride);
    const DtwLayout L = dtw_layout(Ta_stride, Tb_stride);
    const size_t need = (size_t)N * (size_t)L.pair_bytes;
    if (!workspace || workspace_bytes < need) return failf(VTTS_ERR_NOMEM, "workspace too small: %zu < %zu bytes", workspace_bytes, need);
    if (reinterpret_cast<uintptr_t>(workspace) % 256) return failf(VTTS_ERR_INVALID, "workspace must be 256-byte aligned");
    *g = DtwArgs{};
    g->ta_stride = Ta_stride;
    g->tb_stride = Tb_stride;
    g->pair_bytes = L.pair_bytes;
    g->cost_floats = L.cost_floats;
    g->steps = (int)L.steps;
    g->code_words = (int)L.code_words;
    g->D = D;
    g->band = band;
    return VTTS_OK;
}

// One launch's share of a call: pairs n0 .. n0 + np - 1 (the lengths travel as kernel arguments), every pointer re-based, the cost grid.
struct DtwSlice {
    DtwArgs g;
    DtwPairs pairs;
    int np;
    dim3 cost_grid;
};

inline DtwSlice dtw_slice(const DtwArgs& call, const float* a_dev, const float* b_dev, const int32_t* la, const int32_t* lb, float* total_dev,
                          int32_t* path_len_dev, int32_t* span_dev, void* workspace, int N, int n0) {
    DtwSlice sl;
    sl.g = call;
    sl.np = N - n0 < DTW_PAIRS_PER_LAUNCH ? N - n0 : DTW_PAIRS_PER_LAUNCH;
    int la_max = 1, lb_max = 1;
    for (int k = 0; k < DTW_PAIRS_PER_LAUNCH; ++k) {
        sl.pairs.la[k] = k < sl.np ? la[n0 + k] : 1;
        sl.pairs.lb[k] = k < sl.np ? lb[n0 + k] : 1;
        if (sl.pairs.la[k] > la_max) la_max = sl.pairs.la[k];
        if (sl.pairs.lb[k] > lb_max) lb_max = sl.pairs.lb[k];
    }
    sl.g.a = a_dev + (size_t)n0 * call.ta_stride * call.D;
    sl.g.b = b_dev + (size_t)n0 * call.tb_stride * call.D;
    sl.g.ws = static_cast<char*>(workspace) + (size_t)n0 * call.pair_bytes;
    sl.g.total = total_dev + n0;
    sl.g.path_len = path_len_dev + n0;
    sl.g.span = span_dev + (size_t)n0 * call.ta_stride * 2;
    const int row_tiles = (la_max + DTW_TILE - 1) / DTW_TILE;
    const int rows_in_strip = la_max < DTW_STRIP ? la_max : DTW_STRIP;
    const int step_tiles = (lb_max + rows_in_strip - 1 + DTW_TILE - 1) / DTW_TILE;
    sl.cost_grid = dim3(step_tiles, row_tiles, sl.np);
    return sl;
}

// dtw.hip: dtw_wavefront_k and dtw_backtrace_k for the np pairs of one launch, over the cost matrix a cost kernel has written to g.ws on the
// same stream.  Not exported.
void dtw_path_launch(const DtwArgs& g, const DtwPairs& pairs, int np, hipStream_t s);

}  // namespace vtts
