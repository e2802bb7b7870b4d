// The streamed true-peak limiter (include/vtts_limstream.h): limiter.hip's chain fed chunk by chunk, one fused launch per push.
//
//   lim_stream_k, one workgroup (256 lanes) per VTTS_LIMITER_TILE emitted samples of one row; tiles start at the row's emitted count F, a
//   multiple of 16, so the runs of the mean are whole and anchored at the row's first sample:
//     0. tile 0 of a row writes the row's next state x[max(0, F' - 2 W - 27) .. R') into the OTHER state buffer (the row's other tiles
//        still read this one), from the old state below R and the chunk from R on.
//     1. stage x over the tile and 2 W + 27 before, 2 W + 24 after, by absolute index: the old state below R, the chunk from R on, zero
//        before sample 0 and past R'.
//     2. p over the tile and 2 W either side: lim_env_k's 52-tap fmaf chains in its order, four samples a lane and pass.
//     3. req (indices clamped to sample 0, and to the row's last sample on its `last` push only), then lim_apply_k's doubling sliding
//        minimum, its fp64 run sums at the same padded LDS layout, a = min(req, mean), the product and a coalesced store.  A tile whose
//        req are all 1 takes the plain multiply: a mean of ones is exactly 1.
//     4. the tile's max p and min a over its emitted samples go to the row's slots.
//   lim_stream_merge_k, one wave per row: the slots into the row's running results.
//
// Per-row cursors travel as kernel arguments (128 rows a launch); the index arithmetic is limstream_host.h's, on both sides.
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>
#include <vector>

#include "../../include/vtts_audio.h"
#include "../../include/vtts_hifigan.h"
#include "../../include/vtts_limstream.h"
#include "limiter_common.h"
#include "limstream_host.h"
#include "stream_rows_host.h"
#include "vtts_internal.h"

using vtts::failf;
namespace lh = vtts_limstream_host;
using namespace vtts_limiter_dev;  // (the tiling constants among them)

namespace {

constexpr int ROWS_PER_LAUNCH = VTTS_LIMSTREAM_ROWS_PER_LAUNCH;
static_assert(LEAD == lh::LEAD && KP == lh::LEAD + lh::TRAIL + 1, "a phase reads x[n - 27 .. n + 24]");

// staged samples: x[t0 - 2 W - 27 .. t0 + TILE + 2 W + 24], and what the last group of four reads past it
constexpr int span_floats(int W) { return TILE + 4 * W + KP + 4; }
constexpr int lds_bytes(int W) { return (span_floats(W) + 2 * gain_buf_floats(W) + TILE) * (int)sizeof(float); }
constexpr int MAX_LDS = lds_bytes(MAX_W);
static_assert(MAX_LDS <= 160 * 1024, "one workgroup's LDS");

struct LsRow {
    int in_off;     // packed input: first element of the row's chunk, from the launch's chunk pointer
    int out_off;    // first emitted element of the row, from the launch's out pointer
    int R;          // samples received before this push
    int cnt_flags;  // count << 2 | state buffer to read << 1 | last
    int slot;
    float g;
};
struct LsRows {
    LsRow r[ROWS_PER_LAUNCH];
};

struct LsArgs {
    float* state;        // the session's
    const void* chunk;   // first row of this launch
    void* out;           // first emitted sample of this launch
    float* results;      // the session's [rows][3]
    long long c_stride;  // 0 = packed
    float c;
    int W;
    int nb;    // floats of one gain buffer
    int sf;    // floats of one state buffer
    int rowf;  // floats of one row's device memory
};
static_assert(sizeof(LsArgs) + sizeof(LimTaps) + sizeof(LsRows) <= 4096, "the kernel arguments stay within 4 KB");

template <typename TI, typename TO>
__global__ __launch_bounds__(THREADS) void lim_stream_k(const LsArgs a, const LimTaps tp, const LsRows rows) {
    extern __shared__ float4 lds4[];
    __shared__ float wred[2][THREADS / 64];
    __shared__ int any_less;
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const LsRow row = rows.r[b];
    const int W = a.W;
    const int cnt = row.cnt_flags >> 2, last = row.cnt_flags & 1, par = (row.cnt_flags >> 1) & 1;
    const long long R = row.R, Rn = R + cnt;
    const long long F = lh::emitted_of(W, R), Fn = lh::emit_rule(W, R, F, cnt, last);
    if ((int)blockIdx.x >= lh::tiles_of(Fn - F)) return;  // block-uniform, as every branch before the last barrier
    const long long t0 = F + (long long)blockIdx.x * TILE;
    const int live = (int)min((long long)TILE, Fn - t0);  // 0: a push that emits nothing

    float* rowmem = a.state + (size_t)row.slot * a.rowf;
    const float* old = rowmem + (size_t)par * a.sf;
    float* slots = rowmem + 2 * (size_t)a.sf;
    const TI* ch = static_cast<const TI*>(a.chunk) + (a.c_stride ? (long long)b * a.c_stride : (long long)row.in_off);
    auto fetch = [&](long long g) -> float {  // x[g] of the row, zero outside [0, R'): limstream_host.h's lookup
        const lh::Where w = lh::where_is(W, R, F, cnt, g);
        return w.src == lh::SRC_CHUNK ? to_float(ch[w.index]) : w.src == lh::SRC_STATE ? old[w.index] : 0.0f;
    };

    // ---- 0. the row's next state
    if (blockIdx.x == 0 && !last) {
        float* neu = rowmem + (size_t)(par ^ 1) * a.sf;
        const long long Bn = lh::state_base(W, Fn);
        for (long long g = Bn + tid; g < Rn; g += THREADS) neu[g - Bn] = fetch(g);
    }
    if (live == 0) {
        if (tid == 0) slots[0] = 0.0f, slots[1] = 1.0f;
        return;
    }

    float* span = reinterpret_cast<float*>(lds4);
    float* cur = span + span_floats(W);
    float* nxt = cur + a.nb;
    float* rq = nxt + a.nb;
    const int liveR = (live + RUN - 1) / RUN * RUN;  // whole runs: past the row's end (its last push only) they repeat its last sample
    const int nR = liveR + 4 * W;
    const int nP = (live + 4 * W + 3) / 4 * 4;  // p[t0 - 2 W + k], k < nP
    const float g = row.g, c = a.c;
    const long long top = last ? Rn - 1 : 0x7fffffffffffLL;  // the row's last sample, once it is known

    // ---- 1. span[k] = x[t0 - 2 W - LEAD + k]
    {
        const long long s0 = t0 - 2 * W - LEAD;
        const int ns = nP + KP;
#pragma clang loop vectorize(disable)  // (the loop vectoriser would pair the multiplies into v_pk_mul_f32: build.py)
        for (int k = tid; k < ns; k += THREADS) span[k] = fetch(s0 + k);
    }
    if (tid == 0) any_less = 0;
    __syncthreads();

    // ---- 2. p into nxt, four samples a lane and pass: lim_env_k's chains
    float mx = 0.0f;
    for (int i = 4 * tid; i < nP; i += 4 * THREADS) {
        float pk[4];
        true_peak4(lds4, i, tp, pk);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int e = i + s - 2 * W;  // the tile's own samples are final by the emit rule
            if (e >= 0 && e < live) mx = fmaxf(mx, pk[s]);
        }
        *reinterpret_cast<float4*>(nxt + i) = make_float4(pk[0], pk[1], pk[2], pk[3]);
    }
    __syncthreads();

    // ---- 3a. req[t0 - 2 W + k], k < nR: clamped at sample 0, and at the row's last sample once it is known
    {
        const long long r0 = t0 - 2 * W;
        bool less = false;
#pragma clang loop vectorize(disable)  // (the loop vectoriser would pair the multiplies into v_pk_mul_f32: build.py)
        for (int k = tid; k < nR; k += THREADS) {
            const long long n = min(max(r0 + k, 0LL), top);
            const float v = req_of(nxt[(int)(n - r0)], g, c);
            cur[k] = v;
            less |= v < 1.0f;
            const int e = k - 2 * W;
            if (e >= 0 && e < live) rq[e] = v;
        }
        if (less) any_less = 1;
    }
    __syncthreads();

    TO* out = static_cast<TO*>(a.out) + row.out_off + (t0 - F);
    const float* xc = span + 2 * W + LEAD;  // the tile's own samples
    float amin = 1.0f;
    if (!any_less) {  // no sample in reach asks for a reduction: a = 1 exactly
#pragma clang loop vectorize(disable)  // (the loop vectoriser would pair the multiplies into v_pk_mul_f32: build.py)
        for (int i = tid; i < live; i += THREADS) out[i] = from_float<TO>(xc[i] * g);
    } else {
        // ---- 3b./3c. the mean of the sliding minimum, for the tile's samples: lim_apply_k's
        const float* mean = smooth_gains(cur, nxt, nR, W, t0, top, liveR + 2 * W, live, tid);
        // ---- 3d. a, y, the store
#pragma clang loop vectorize(disable)  // (the loop vectoriser would pair the multiplies into v_pk_mul_f32: build.py)
        for (int i = tid; i < live; i += THREADS) {
            const float av = fminf(rq[i], mean[i]);
            amin = fminf(amin, av);
            out[i] = from_float<TO>((xc[i] * g) * av);
        }
    }

    // ---- 4. the tile's max p and min a
    mx = wave_extreme<false>(mx), amin = wave_extreme<true>(amin);
    if ((tid & 63) == 0) wred[0][tid >> 6] = mx, wred[1][tid >> 6] = amin;
    __syncthreads();
    if (tid == 0) slots[2 * blockIdx.x] = extreme4<false>(wred[0]), slots[2 * blockIdx.x + 1] = extreme4<true>(wred[1]);
}

// One wave per row of the push: the tiles' slots into the slot's running results.  A row's first push (R = 0) starts them over.
__global__ __launch_bounds__(64) void lim_stream_merge_k(const LsArgs a, const LsRows rows) {
    const int lane = threadIdx.x;
    const LsRow row = rows.r[blockIdx.x];
    const int cnt = row.cnt_flags >> 2, last = row.cnt_flags & 1;
    const long long F = lh::emitted_of(a.W, row.R);
    const int nt = lh::tiles_of(lh::emit_rule(a.W, row.R, F, cnt, last) - F);
    const float* slots = a.state + (size_t)row.slot * a.rowf + 2 * (size_t)a.sf;
    float vmax = 0.0f, vmin = 1.0f;
    for (int t = lane; t < nt; t += 64) {
        vmax = fmaxf(vmax, slots[2 * t]);
        vmin = fminf(vmin, slots[2 * t + 1]);
    }
    vmax = wave_extreme<false>(vmax), vmin = wave_extreme<true>(vmin);
    if (lane == 0) {
        float* res = a.results + 3 * (size_t)row.slot;
        if (row.R > 0) {
            vmax = fmaxf(vmax, res[0]);
            vmin = fminf(vmin, res[1]);
        }
        res[0] = vmax;
        res[1] = vmin;
        res[2] = row.g;
    }
}

template <typename TI, typename TO>
hipError_t launch_stream(const LsArgs& a, const LimTaps& taps, const LsRows& rows, dim3 grid, hipStream_t s, vtts::DynLdsOnce& once) {
    const void* fn = reinterpret_cast<const void*>(&lim_stream_k<TI, TO>);
    hipError_t e = vtts::set_max_dynamic_lds(fn, MAX_LDS, once);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((lim_stream_k<TI, TO>), grid, dim3(THREADS), (size_t)lds_bytes(a.W), s, a, taps, rows);
    return hipGetLastError();
}

}  // namespace

struct vtts_limstream {
    int rate = 0, W = 0;
    float c = 0.0f;
    lh::Layout lay;
    LimTaps taps;
    vtts_stream_rows::Cursors cur;
    std::vector<float> g;
    vtts::DynLdsOnce lds[4];
};

VTTS_API int vtts_limstream_create(const vtts_limiter_cfg* cfg, int device, int rows, int32_t max_chunk, float ceiling_dbtp, vtts_limstream** out) {
    (void)device;  // (the handle owns nothing on a device: the calls run on the caller's current one)
    if (!cfg || !out) return failf(VTTS_ERR_INVALID, "null argument");
    LimTaps taps;
    int W = 0;
    if (int rc = configure(cfg, taps, W)) return rc;
    if (rows < 1 || rows > (1 << 24)) return failf(VTTS_ERR_INVALID, "rows must be in 1 .. 2^24 (got %d)", rows);
    if (max_chunk < 1 || max_chunk > VTTS_LIMSTREAM_MAX_CHUNK)
        return failf(VTTS_ERR_INVALID, "max_chunk must be in 1 .. %d (got %d)", VTTS_LIMSTREAM_MAX_CHUNK, max_chunk);
    if (!std::isfinite(ceiling_dbtp)) return failf(VTTS_ERR_INVALID, "ceiling_dbtp must be finite (got %g)", ceiling_dbtp);
    auto* h = new (std::nothrow) vtts_limstream();
    if (!h) return failf(VTTS_ERR_NOMEM, "host allocation failed");
    h->taps = taps;
    h->W = W;
    h->rate = cfg->sample_rate;
    h->c = (float)std::pow(10.0, (double)ceiling_dbtp / 20.0);
    h->lay = lh::layout(h->W, rows, max_chunk);
    bool ok = h->cur.init(rows, max_chunk);
    try {
        h->g.assign(rows, 1.0f);
    } catch (const std::bad_alloc&) {
        ok = false;
    }
    if (!ok) {
        delete h;
        return failf(VTTS_ERR_NOMEM, "host allocation failed");
    }
    *out = h;
    return VTTS_OK;
}

VTTS_API void vtts_limstream_destroy(vtts_limstream* h) { delete h; }

VTTS_API int vtts_limstream_lookahead(const vtts_limstream* h, int32_t* W) {
    if (!h || !W) return failf(VTTS_ERR_INVALID, "null argument");
    *W = h->W;
    return VTTS_OK;
}

VTTS_API int vtts_limstream_state_bytes(const vtts_limstream* h, size_t* bytes) {
    if (!h || !bytes) return failf(VTTS_ERR_INVALID, "null argument");
    *bytes = h->lay.bytes;
    return VTTS_OK;
}

VTTS_API int vtts_limstream_reset(vtts_limstream* h, int row, float gain) {
    if (!h) return failf(VTTS_ERR_INVALID, "null argument");
    if (!h->cur.has(row)) return failf(VTTS_ERR_INVALID, "reset: row %d is outside 0 .. %d", row, h->cur.rows - 1);
    if (!std::isfinite(gain)) return failf(VTTS_ERR_INVALID, "reset: the gain must be finite (got %g)", gain);
    h->cur.reset(row);
    h->g[row] = gain;
    return VTTS_OK;
}

VTTS_API int vtts_limstream_emit(const vtts_limstream* h, int64_t received, int64_t emitted, int32_t count, int last, int64_t* new_emitted) {
    if (!h || !new_emitted) return failf(VTTS_ERR_INVALID, "null argument");
    if (received < 0 || emitted < 0 || emitted > received || count < 0)
        return failf(VTTS_ERR_INVALID, "emit: need 0 <= emitted <= received and count >= 0 (got %lld, %lld, %d)", (long long)emitted, (long long)received, count);
    *new_emitted = lh::emit_rule(h->W, received, emitted, count, last != 0);
    return VTTS_OK;
}

VTTS_API int vtts_limstream_push(vtts_limstream* h, void* state_dev, const void* chunk_dev, int dtype, int n, const int32_t* rows_host, int64_t c_stride,
                                 const int32_t* counts_host, const int32_t* last_host, void* out_dev, int out_dtype, int32_t* out_counts_host,
                                 float* results_dev, void* stream) {
    if (!h || !state_dev || !chunk_dev || !rows_host || !counts_host || !out_dev || !out_counts_host || !results_dev)
        return failf(VTTS_ERR_INVALID, "null argument");
    if (dtype != VTTS_AUDIO_F32 && dtype != VTTS_AUDIO_PCM16) return failf(VTTS_ERR_INVALID, "push: dtype must be VTTS_AUDIO_F32 or VTTS_AUDIO_PCM16 (got %d)", dtype);
    if (out_dtype != VTTS_AUDIO_F32 && out_dtype != VTTS_AUDIO_PCM16)
        return failf(VTTS_ERR_INVALID, "push: out_dtype must be VTTS_AUDIO_F32 or VTTS_AUDIO_PCM16 (got %d)", out_dtype);
    vtts_stream_rows::Cursors& cu = h->cur;
    if (n < 1 || n > cu.rows) return failf(VTTS_ERR_INVALID, "push: n must be in 1 .. rows = %d (got %d)", cu.rows, n);
    if (c_stride < 0) return failf(VTTS_ERR_INVALID, "push: c_stride must not be negative (got %lld)", (long long)c_stride);
    if (reinterpret_cast<uintptr_t>(state_dev) % 16) return failf(VTTS_ERR_INVALID, "push: the state must be 16-byte aligned");
    // ---- every refusal before any bookkeeping changes; a row stays within MAX_S = 2^31 - 1 - TILE samples
    char why[160];
    if (int rc = cu.check_push(n, rows_host, counts_host, c_stride, TILE, why)) return failf(rc, "%s", why);

    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool pin = dtype == VTTS_AUDIO_PCM16, pout = out_dtype == VTTS_AUDIO_PCM16;
    const size_t isz = pin ? 2 : 4, osz = pout ? 2 : 4;
    LsArgs a;
    a.state = static_cast<float*>(state_dev);
    a.results = results_dev;
    a.c_stride = c_stride;
    a.c = h->c;
    a.W = h->W;
    a.nb = gain_buf_floats(h->W);
    a.sf = (int)h->lay.state_floats;
    a.rowf = (int)h->lay.row_floats;
    size_t in_total = 0, out_total = 0;
    for (int r0 = 0; r0 < n; r0 += ROWS_PER_LAUNCH) {
        const int nr = n - r0 < ROWS_PER_LAUNCH ? n - r0 : ROWS_PER_LAUNCH;
        LsRows rows = {};
        a.chunk = static_cast<const char*>(chunk_dev) + (c_stride ? (size_t)r0 * (size_t)c_stride : in_total) * isz;
        a.out = static_cast<char*>(out_dev) + out_total * osz;
        int in_off = 0, out_off = 0, tiles = 1;
        for (int b = 0; b < nr; ++b) {
            const int r = rows_host[r0 + b], cnt = counts_host[r0 + b], last = last_host && last_host[r0 + b] ? 1 : 0;
            const int64_t Fn = lh::emit_rule(h->W, cu.R[r], cu.F[r], cnt, last);
            const int emit = (int)(Fn - cu.F[r]);
            LsRow& q = rows.r[b];
            q.in_off = in_off;
            q.out_off = out_off;
            q.R = (int)cu.R[r];
            q.cnt_flags = cnt << 2 | (int)cu.parity[r] << 1 | last;
            q.slot = r;
            q.g = h->g[r];
            in_off += cnt;
            out_off += emit;
            out_counts_host[r0 + b] = emit;
            if (lh::tiles_of(emit) > tiles) tiles = lh::tiles_of(emit);
        }
        in_total += (size_t)in_off;
        out_total += (size_t)out_off;
        const dim3 grid((unsigned)tiles, (unsigned)nr);
        hipError_t e;
        if (pin)
            e = pout ? launch_stream<short, short>(a, h->taps, rows, grid, s, h->lds[3]) : launch_stream<short, float>(a, h->taps, rows, grid, s, h->lds[2]);
        else
            e = pout ? launch_stream<float, short>(a, h->taps, rows, grid, s, h->lds[1]) : launch_stream<float, float>(a, h->taps, rows, grid, s, h->lds[0]);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(lim_stream_merge_k, dim3((unsigned)nr), dim3(64), 0, s, a, rows);
            e = hipGetLastError();
        }
        if (e != hipSuccess) return failf(VTTS_ERR_HIP, "limiter kernel launch failed: %s", hipGetErrorString(e));
        cu.advance(nr, rows_host + r0, counts_host + r0, last_host ? last_host + r0 : nullptr, out_counts_host + r0);  // the launch's rows have moved
    }
    return VTTS_OK;
}
