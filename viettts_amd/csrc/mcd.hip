// Mel-cepstral distortion (include/vtts_mcd.h): DCT-II cepstra of log-mels, the aligned distance with its float64 sum, and the L2 local cost
// of the DTW.  Plain fp32 VALU in the header's fixed order; the file is built with -ffp-contract=off (viettts_amd/csrc/build.py), so no
// multiply below is contracted into an fma, and sqrtf is hipcc's correctly rounded one.
//
//   1. mcd_cepstra_k   one workgroup per (row, FRAMES frames).  The frames are staged in LDS (row pitch M | 1: the lanes of a wave own
//                      consecutive frames, an odd pitch spreads them over the banks), the K x M basis beside them (a wave reads one element
//                      of it at a time: a broadcast).  Wave w owns the coefficients k = w, w + 4, ..., four chains at a time per lane.  The
//                      tile of cepstra goes through LDS once more, so that the store to memory is contiguous.
//   2. mcd_aligned_k   the same tile for both inputs, then lane t of wave 0 runs frame t's distance chain over the two cepstra in LDS, and
//                      thread 0 adds the block's distances in float64 in ascending t into the block's slot of the workspace.
//      mcd_rowsum_k    adds a row's block sums in ascending order.
//   3. mcd_cost_k      dtw_common.h's cost tile (the tile map, early returns and skewed store of dtw_cost_k) with the L2 metric over
//                      D = K cepstra: a sixth of the L1 kernel's arithmetic and LDS at K = 13 against 80 bands.
// The wavefront and the backtrace are dtw.hip's (vtts::dtw_path_launch).
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>
#include <vector>

#include "../../include/vtts_mcd.h"
#include "dtw_common.h"
#include "launch_rows.h"

using vtts::DtwArgs;
using vtts::DtwPairs;
using vtts::failf;

namespace {

constexpr int ROWS_PER_LAUNCH = 128;
constexpr int FRAMES = VTTS_MCD_FRAMES_PER_BLOCK;
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int CHAINS = 4;  // coefficients a lane carries at once

static_assert(ROWS_PER_LAUNCH == VTTS_MCD_ROWS_PER_LAUNCH, "the header names the split");
static_assert(FRAMES == 64, "a wave's lanes own the frames of a block");
static_assert(VTTS_MCD_MAX_CEPS <= VTTS_DTW_MAX_FEAT, "the cepstra are the DTW's features");

using McdRows = vtts_rows::Lens<ROWS_PER_LAUNCH>;  // frames of each row of this launch

struct McdArgs {
    const float* xa;     // first row of this launch
    const float* xb;     // aligned only
    const float* basis;  // [K][M]
    float* ceps;         // cepstra only
    float* frame;        // aligned only, or nullptr
    double* part;        // aligned only: [rows][blocks]
    double* sum;
    long long ta_stride, tb_stride, f_stride;
    int blocks;
    int M, K;
};

// Frames t0 .. t0 + FRAMES - 1 of a row (those below len; the others as zeros, never read) into X[FRAMES][M | 1].
__device__ __forceinline__ void stage_frames(const float* row, int t0, int len, int M, float* X) {
    const int P = M | 1, valid = (len - t0 < FRAMES ? len - t0 : FRAMES) * M;
    const float* src = row + (size_t)t0 * M;
    for (int idx = threadIdx.x; idx < FRAMES * M; idx += THREADS) {
        const int r = idx / M, m = idx - r * M;
        X[r * P + m] = idx < valid ? src[idx] : 0.0f;
    }
}

// C[FRAMES][K] = the cepstra of the staged frames X: c[t, k] = one chain in ascending m (vtts_mcd.h: cepstrum).
__device__ __forceinline__ void cepstra_tile(const float* X, const float* T, int M, int K, float* C) {
    const int P = M | 1, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float* x = X + lane * P;
    for (int kb = w; kb < K; kb += WAVES * CHAINS) {
        const float* t[CHAINS];
        float acc[CHAINS];
#pragma unroll
        for (int q = 0; q < CHAINS; ++q) {
            const int k = kb + WAVES * q;
            t[q] = T + (k < K ? k : kb) * M;
            acc[q] = 0.0f;
        }
        for (int m = 0; m < M; ++m) {
            const float xv = x[m];
#pragma unroll
            for (int q = 0; q < CHAINS; ++q) acc[q] = acc[q] + t[q][m] * xv;
        }
#pragma unroll
        for (int q = 0; q < CHAINS; ++q) {
            const int k = kb + WAVES * q;
            if (k < K) C[lane * K + k] = acc[q];
        }
    }
}

__device__ __forceinline__ void stage_basis(const float* basis, int n, float* T) {
    for (int idx = threadIdx.x; idx < n; idx += THREADS) T[idx] = basis[idx];
}

// dynamic LDS: T [K M] | X [FRAMES (M | 1)] | C [FRAMES K]
__global__ __launch_bounds__(THREADS) void mcd_cepstra_k(McdArgs g, McdRows p) {
    extern __shared__ float lds[];
    const int n = blockIdx.y, len = p.len[n], t0 = blockIdx.x * FRAMES, M = g.M, K = g.K;
    float* out = g.ceps + ((size_t)n * g.ta_stride + t0) * K;
    const long long left = g.ta_stride - t0;
    const int rows = (int)(left < FRAMES ? left : FRAMES);  // frames of this block inside the stride
    if (t0 >= len) {
        for (int idx = threadIdx.x; idx < rows * K; idx += THREADS) out[idx] = 0.0f;
        return;
    }
    float* T = lds;
    float* X = T + K * M;
    float* C = X + FRAMES * (M | 1);
    stage_basis(g.basis, K * M, T);
    stage_frames(g.xa + (size_t)n * g.ta_stride * M, t0, len, M, X);
    __syncthreads();
    cepstra_tile(X, T, M, K, C);
    __syncthreads();
    const int valid = (len - t0 < FRAMES ? len - t0 : FRAMES) * K;
    for (int idx = threadIdx.x; idx < rows * K; idx += THREADS) out[idx] = idx < valid ? C[idx] : 0.0f;
}

// dynamic LDS: T [K M] | XA [FRAMES (M | 1)] | XB [FRAMES (M | 1)] | CA [FRAMES K] | CB [FRAMES K] | D [FRAMES]
__global__ __launch_bounds__(THREADS) void mcd_aligned_k(McdArgs g, McdRows p) {
    extern __shared__ float lds[];
    const int n = blockIdx.y, len = p.len[n], t0 = blockIdx.x * FRAMES, M = g.M, K = g.K;
    float* frame = g.frame ? g.frame + (size_t)n * g.f_stride : nullptr;
    if (frame && blockIdx.x == gridDim.x - 1)  // what of the row's stride lies behind the grid
        for (long long t = (long long)gridDim.x * FRAMES + threadIdx.x; t < g.f_stride; t += THREADS) frame[t] = 0.0f;
    if (t0 >= len) {
        if (threadIdx.x == 0) g.part[(size_t)n * g.blocks + blockIdx.x] = 0.0;
        if (frame && threadIdx.x < FRAMES && t0 + (long long)threadIdx.x < g.f_stride) frame[t0 + threadIdx.x] = 0.0f;
        return;
    }
    float* T = lds;
    float* XA = T + K * M;
    float* XB = XA + FRAMES * (M | 1);
    float* CA = XB + FRAMES * (M | 1);
    float* CB = CA + FRAMES * K;
    float* Dv = CB + FRAMES * K;
    stage_basis(g.basis, K * M, T);
    stage_frames(g.xa + (size_t)n * g.ta_stride * M, t0, len, M, XA);
    stage_frames(g.xb + (size_t)n * g.tb_stride * M, t0, len, M, XB);
    __syncthreads();
    cepstra_tile(XA, T, M, K, CA);
    cepstra_tile(XB, T, M, K, CB);
    __syncthreads();
    const int count = len - t0 < FRAMES ? len - t0 : FRAMES;
    if (threadIdx.x < FRAMES) {
        const int t = threadIdx.x;
        float s = 0.0f;
        for (int k = 0; k < K; ++k) {
            const float e = CA[t * K + k] - CB[t * K + k];
            s = s + e * e;
        }
        const float d = t < count ? sqrtf(s) : 0.0f;
        Dv[t] = d;
        if (frame && t0 + (long long)t < g.f_stride) frame[t0 + t] = d;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int t = 0; t < count; ++t) s = s + (double)Dv[t];
        g.part[(size_t)n * g.blocks + blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(64) void mcd_rowsum_k(McdArgs g, int rows) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= rows) return;
    double s = 0.0;
    for (int q = 0; q < g.blocks; ++q) s = s + g.part[(size_t)n * g.blocks + q];
    g.sum[n] = s;
}

// vtts_mcd.h: distance, one link of the chain and what is stored
struct L2Metric {
    static __device__ __forceinline__ float term(float acc, float a, float b) {
        const float e = a - b;
        return acc + e * e;
    }
    static __device__ __forceinline__ float finish(float acc) { return sqrtf(acc); }
};

__global__ __launch_bounds__(vtts::DTW_COST_THREADS) void mcd_cost_k(DtwArgs g, DtwPairs p) {
    extern __shared__ float lds[];
    vtts::dtw_cost_tile<L2Metric>(g, p, lds);
}

}  // namespace

struct vtts_mcd {
    vtts_mcd_cfg cfg;
    int device;
    std::vector<float> basis;     // [K][M]
    float* basis_dev = nullptr;   // the same on the device, from the first launching call on
    vtts::DynLdsOnce lds_ceps, lds_aligned, lds_cost;
};

namespace {

int upload_basis(vtts_mcd* h, hipStream_t s) {
    if (h->basis_dev) return VTTS_OK;
    void* p = nullptr;
    const size_t bytes = h->basis.size() * sizeof(float);
    HIP_TRY(hipMalloc(&p, bytes));
    hipError_t e = hipMemcpyAsync(p, h->basis.data(), bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        (void)hipFree(p);
        return failf(VTTS_ERR_HIP, "copying the basis failed: %s", hipGetErrorString(e));
    }
    h->basis_dev = static_cast<float*>(p);
    return VTTS_OK;
}

// lens (or T for every row when it is null) within 0 .. limit
int check_lens(const int32_t* lens, int N, int64_t limit) {
    if (lens)
        for (int n = 0; n < N; ++n)
            if (lens[n] < 0 || lens[n] > limit) return failf(VTTS_ERR_INVALID, "lens[%d] = %d is outside 0 .. %lld", n, lens[n], (long long)limit);
    return VTTS_OK;
}

int check_batch(int N, int64_t T) {
    if (N <= 0) return failf(VTTS_ERR_INVALID, "N must be positive (got %d)", N);
    if (T < 1 || T > 0x7fffffff - FRAMES) return failf(VTTS_ERR_INVALID, "a stride must be in 1 .. 2^31 - 1 - %d frames (got %lld)", FRAMES, (long long)T);
    return VTTS_OK;
}

size_t aligned_bytes(int N, int64_t T) { return vtts::align_up(sizeof(double) * (size_t)N * (size_t)((T + FRAMES - 1) / FRAMES), 256); }

}  // namespace

VTTS_API int vtts_mcd_create(const vtts_mcd_cfg* cfg, int device, vtts_mcd** out) {
    if (!cfg || !out) return failf(VTTS_ERR_INVALID, "null argument");
    if (cfg->n_mels < 1 || cfg->n_mels > VTTS_MCD_MAX_MELS) return failf(VTTS_ERR_INVALID, "n_mels must be in 1 .. %d (got %d)", VTTS_MCD_MAX_MELS, cfg->n_mels);
    const int kmax = cfg->n_mels - 1 < VTTS_MCD_MAX_CEPS ? cfg->n_mels - 1 : VTTS_MCD_MAX_CEPS;
    if (cfg->n_ceps < 1 || cfg->n_ceps > kmax) return failf(VTTS_ERR_INVALID, "n_ceps must be in 1 .. min(n_mels - 1, %d) = %d (got %d)", VTTS_MCD_MAX_CEPS, kmax, cfg->n_ceps);
    if (cfg->band < 0) return failf(VTTS_ERR_INVALID, "band must be >= 0 (got %d)", cfg->band);
    if (cfg->max_frames < 1 || cfg->max_frames > vtts::DTW_MAXF) return failf(VTTS_ERR_INVALID, "max_frames must be in 1 .. %d (got %d)", vtts::DTW_MAXF, cfg->max_frames);
    auto* h = new (std::nothrow) vtts_mcd();
    if (!h) return failf(VTTS_ERR_NOMEM, "host allocation failed");
    h->cfg = *cfg;
    h->device = device;
    const int M = cfg->n_mels, K = cfg->n_ceps;
    const double pi = 3.14159265358979323846, scale = std::sqrt(2.0 / M);
    h->basis.resize((size_t)K * M);
    for (int k = 1; k <= K; ++k)
        for (int m = 0; m < M; ++m) h->basis[(size_t)(k - 1) * M + m] = (float)(scale * std::cos(pi * k * (2 * m + 1) / (2.0 * M)));
    *out = h;
    return VTTS_OK;
}

VTTS_API void vtts_mcd_destroy(vtts_mcd* h) {
    if (h && h->basis_dev) (void)hipFree(h->basis_dev);
    delete h;
}

VTTS_API int vtts_mcd_basis(const vtts_mcd* h, float* host_out) {
    if (!h || !host_out) return failf(VTTS_ERR_INVALID, "null argument");
    memcpy(host_out, h->basis.data(), h->basis.size() * sizeof(float));
    return VTTS_OK;
}

VTTS_API int vtts_mcd_cepstra(vtts_mcd* h, const float* logmel_dev, int N, int64_t T_stride, const int32_t* lens, float* ceps_dev, void* stream) {
    if (!h || !logmel_dev || !ceps_dev) return failf(VTTS_ERR_INVALID, "null argument");
    if (int rc = check_batch(N, T_stride)) return rc;
    if (int rc = check_lens(lens, N, T_stride)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = upload_basis(h, s)) return rc;
    const int M = h->cfg.n_mels, K = h->cfg.n_ceps;
    const size_t lds = sizeof(float) * ((size_t)K * M + (size_t)FRAMES * (M | 1) + (size_t)FRAMES * K);
    hipError_t e = vtts::set_max_dynamic_lds(reinterpret_cast<const void*>(&mcd_cepstra_k), (int)lds, h->lds_ceps);
    if (e != hipSuccess) return failf(VTTS_ERR_HIP, "hipFuncSetAttribute failed: %s", hipGetErrorString(e));
    McdArgs g{};
    g.basis = h->basis_dev;
    g.ta_stride = T_stride;
    g.M = M;
    g.K = K;
    const int blocks = (int)((T_stride + FRAMES - 1) / FRAMES);
    return vtts_rows::for_each_launch<ROWS_PER_LAUNCH>(N, lens, T_stride, [&](int n0, int np, const McdRows& rows) -> int {
        g.xa = logmel_dev + (size_t)n0 * T_stride * M;
        g.ceps = ceps_dev + (size_t)n0 * T_stride * K;
        hipLaunchKernelGGL(mcd_cepstra_k, dim3(blocks, np), dim3(THREADS), lds, s, g, rows);
        e = hipGetLastError();
        if (e != hipSuccess) return failf(VTTS_ERR_HIP, "mcd_cepstra_k launch failed: %s", hipGetErrorString(e));
        return VTTS_OK;
    });
}

VTTS_API int vtts_mcd_aligned_workspace_bytes(const vtts_mcd* h, int N, int64_t T, size_t* bytes) {
    if (!h || !bytes) return failf(VTTS_ERR_INVALID, "null argument");
    if (int rc = check_batch(N, T)) return rc;
    *bytes = aligned_bytes(N, T);
    return VTTS_OK;
}

VTTS_API int vtts_mcd_aligned(vtts_mcd* h, const float* logmel_a_dev, const float* logmel_b_dev, int N, int64_t Ta_stride, int64_t Tb_stride,
                              const int32_t* lens, double* sum_dev, float* frame_dev, int64_t F_stride, void* workspace, size_t workspace_bytes,
                              void* stream) {
    if (!h || !logmel_a_dev || !logmel_b_dev || !sum_dev) return failf(VTTS_ERR_INVALID, "null argument");
    if (int rc = check_batch(N, Ta_stride)) return rc;
    if (int rc = check_batch(N, Tb_stride)) return rc;
    const int64_t T = Ta_stride < Tb_stride ? Ta_stride : Tb_stride;
    int64_t limit = T;
    if (frame_dev && F_stride < T) {  // then every row has to say that it is shorter
        if (F_stride < 1 || !lens) return failf(VTTS_ERR_INVALID, "F_stride = %lld does not hold the rows' frames", (long long)F_stride);
        limit = F_stride;
    }
    if (int rc = check_lens(lens, N, limit)) return rc;
    const size_t need = aligned_bytes(N, T);
    if (!workspace || workspace_bytes < need) return failf(VTTS_ERR_NOMEM, "workspace too small: %zu < %zu bytes", workspace_bytes, need);
    if (reinterpret_cast<uintptr_t>(workspace) % 256) return failf(VTTS_ERR_INVALID, "workspace must be 256-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = upload_basis(h, s)) return rc;
    const int M = h->cfg.n_mels, K = h->cfg.n_ceps;
    const size_t lds = sizeof(float) * ((size_t)K * M + 2 * (size_t)FRAMES * (M | 1) + 2 * (size_t)FRAMES * K + FRAMES);
    hipError_t e = vtts::set_max_dynamic_lds(reinterpret_cast<const void*>(&mcd_aligned_k), (int)lds, h->lds_aligned);
    if (e != hipSuccess) return failf(VTTS_ERR_HIP, "hipFuncSetAttribute failed: %s", hipGetErrorString(e));
    McdArgs g{};
    g.basis = h->basis_dev;
    g.ta_stride = Ta_stride;
    g.tb_stride = Tb_stride;
    g.f_stride = F_stride;
    g.blocks = (int)((T + FRAMES - 1) / FRAMES);
    g.M = M;
    g.K = K;
    return vtts_rows::for_each_launch<ROWS_PER_LAUNCH>(N, lens, T, [&](int n0, int np, const McdRows& rows) -> int {
        g.xa = logmel_a_dev + (size_t)n0 * Ta_stride * M;
        g.xb = logmel_b_dev + (size_t)n0 * Tb_stride * M;
        g.frame = frame_dev ? frame_dev + (size_t)n0 * F_stride : nullptr;
        g.part = static_cast<double*>(workspace) + (size_t)n0 * g.blocks;
        g.sum = sum_dev + n0;
        hipLaunchKernelGGL(mcd_aligned_k, dim3(g.blocks, np), dim3(THREADS), lds, s, g, rows);
        hipLaunchKernelGGL(mcd_rowsum_k, dim3((np + 63) / 64), dim3(64), 0, s, g, np);
        e = hipGetLastError();
        if (e != hipSuccess) return failf(VTTS_ERR_HIP, "mcd_aligned_k launch failed: %s", hipGetErrorString(e));
        return VTTS_OK;
    });
}

VTTS_API int vtts_mcd_dtw_workspace_bytes(const vtts_mcd* h, int N, int64_t Ta_stride, int64_t Tb_stride, size_t* bytes) {
    if (!h || !bytes) return failf(VTTS_ERR_INVALID, "null argument");
    if (int rc = vtts::dtw_check_shape(h->cfg.max_frames, N, Ta_stride, Tb_stride)) return rc;
    *bytes = (size_t)N * (size_t)vtts::dtw_layout(Ta_stride, Tb_stride).pair_bytes;
    return VTTS_OK;
}

VTTS_API int vtts_mcd_dtw(vtts_mcd* h, const float* ceps_a_dev, const float* ceps_b_dev, int N, int64_t Ta_stride, int64_t Tb_stride, const int32_t* la,
                          const int32_t* lb, float* total_dev, int32_t* path_len_dev, int32_t* span_dev, void* workspace, size_t workspace_bytes,
                          void* stream) {
    if (!h || !ceps_a_dev || !ceps_b_dev || !la || !lb || !total_dev || !path_len_dev || !span_dev) return failf(VTTS_ERR_INVALID, "null argument");
    DtwArgs call;
    if (int rc = vtts::dtw_check_call(h->cfg.max_frames, h->cfg.n_ceps, h->cfg.band, N, Ta_stride, Tb_stride, la, lb, workspace, workspace_bytes, &call)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t lds = vtts::dtw_cost_lds_bytes(call.D);
    hipError_t e = vtts::set_max_dynamic_lds(reinterpret_cast<const void*>(&mcd_cost_k), (int)lds, h->lds_cost);
    if (e != hipSuccess) return failf(VTTS_ERR_HIP, "hipFuncSetAttribute failed: %s", hipGetErrorString(e));
    for (int n0 = 0; n0 < N; n0 += vtts::DTW_PAIRS_PER_LAUNCH) {
        const vtts::DtwSlice sl = vtts::dtw_slice(call, ceps_a_dev, ceps_b_dev, la, lb, total_dev, path_len_dev, span_dev, workspace, N, n0);
        hipLaunchKernelGGL(mcd_cost_k, sl.cost_grid, dim3(vtts::DTW_COST_THREADS), lds, s, sl.g, sl.pairs);
        vtts::dtw_path_launch(sl.g, sl.pairs, sl.np, s);
        e = hipGetLastError();
        if (e != hipSuccess) return failf(VTTS_ERR_HIP, "mcd dtw kernel launch failed: %s", hipGetErrorString(e));
    }
    return VTTS_OK;
}
