// The streamed resampler (include/vtts_rsstream.h): audio.hip's conversion fed chunk by chunk, one fused launch per push.
//
//   rs_stream_k, one workgroup (256 lanes) per VTTS_AUDIO_OUT_PER_BLOCK emitted outputs of one row; tiles start at the row's emitted count
//   F, and an output's bits do not depend on its tile:
//     0. tile 0 of a row writes the row's next history x[max(0, q(F') - (kp4 - 1)) .. R') into the OTHER history buffer (the row's other
//        tiles still read this one), from the old history below R and the chunk from R on.  Also where the row emits nothing.
//     1. stage the span the tile's outputs meet into LDS by absolute index: the old history below R, the chunk from R on (16-byte loads
//        where the chunk's address allows: a packed push puts a row at any offset), zero before sample 0 and past R'.  The span starts
//        at a multiple of 8 samples as audio.hip's does; what that rounding reaches below the history is zero and meets no chain.
//     2. audio_common.h's outputs: the same chains on consecutive phases, the table in global memory.
//   in_rate == out_rate skips 0. to 2.: the kernel converts and packs only.
//
// Per-row cursors travel as kernel arguments (128 rows a launch); the index arithmetic is rsstream_host.h's, on both sides.  Block bases
// are 64-bit, everything inside a block is a 32-bit offset.
#include <hip/hip_runtime.h>

#include <new>
#include <type_traits>
#include <vector>

#include "../../include/vtts_audio.h"
#include "../../include/vtts_hifigan.h"
#include "../../include/vtts_rsstream.h"
#include "audio_common.h"
#include "audio_design.h"
#include "rsstream_host.h"
#include "stream_rows_host.h"
#include "vtts_internal.h"

using vtts::check_blob;
using vtts::failf;
namespace ad = vtts_audio_design;
namespace rh = vtts_rsstream_host;
using vtts_audio_dev::from_float;
using vtts_audio_dev::Phases;
using vtts_audio_dev::span_outputs;
using vtts_audio_dev::to_float;

namespace {

constexpr int OPB = VTTS_AUDIO_OUT_PER_BLOCK;
constexpr int THREADS = 256;
constexpr int ROWS_PER_LAUNCH = VTTS_RSSTREAM_ROWS_PER_LAUNCH;

struct RsRow {
    long long out_off;  // first emitted element of the row, from the launch's out pointer
    int in_off;         // packed input: first element of the row's chunk, from the launch's chunk pointer
    int R;              // samples received before this push
    int cnt_flags;      // count << 2 | history buffer to read << 1 | last
    int slot;
};
struct RsRows {
    RsRow r[ROWS_PER_LAUNCH];
};

struct RsArgs {
    float* state;        // the session's
    const void* chunk;   // first row of this launch
    void* out;           // first emitted sample of this launch
    const float* table;  // [kp4 / 4][L][4]
    long long c_stride;  // 0 = packed
    rh::Ratio ratio;
    int minv;  // M^-1 mod L
    int hf;    // floats of one history buffer
};
static_assert(sizeof(RsArgs) + sizeof(RsRows) <= 4096, "the kernel arguments stay within 4 KB");

template <typename TI, typename TO>
__global__ __launch_bounds__(THREADS) void rs_stream_k(const RsArgs a, const RsRows rows) {
    extern __shared__ float4 lds4[];
    float* span = reinterpret_cast<float*>(lds4);
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const RsRow row = rows.r[b];
    const rh::Ratio rt = a.ratio;
    const int cnt = row.cnt_flags >> 2, last = row.cnt_flags & 1, par = (row.cnt_flags >> 1) & 1;
    const long long R = row.R, Rn = R + cnt;
    const long long F = rh::emitted_of(rt, R), Fn = rh::emit_rule(rt, R, F, cnt, last);
    if ((long long)blockIdx.x >= rh::tiles_of(Fn - F)) return;  // block-uniform, as every branch before the barrier
    const long long m0 = F + (long long)blockIdx.x * OPB;
    const int live = (int)min((long long)OPB, Fn - m0);  // 0: a push that emits nothing
    const TI* ch = static_cast<const TI*>(a.chunk) + (a.c_stride ? (long long)b * a.c_stride : (long long)row.in_off);
    TO* out = static_cast<TO*>(a.out) + row.out_off + (m0 - F);

    if (rt.identity) {  // F = R: output m is sample m
        const TI* x = ch + (m0 - R);
#pragma clang loop vectorize(disable)  // (the loop vectoriser would pair the PCM16 scalings into v_pk_mul_f32: build.py)
        for (int i = tid; i < live; i += THREADS) {
            if constexpr (std::is_same<TI, TO>::value)
                out[i] = x[i];  // the same format on both sides is a copy
            else
                out[i] = from_float<TO>(to_float(x[i]));
        }
        return;
    }

    const float* old = a.state + ((size_t)row.slot * 2 + par) * a.hf;
    const long long B = rh::hist_base(rt, F);  // the old history's first sample
    auto fetch = [&](long long g) -> float {  // x[g] of the row, zero outside [0, R'): rsstream_host.h's lookup
        const rh::Where w = rh::where_is(R, cnt, B, g);
        return w.src == rh::SRC_CHUNK ? to_float(ch[w.index]) : w.src == rh::SRC_HIST ? old[w.index] : 0.0f;
    };

    // ---- 0. the row's next history
    if (blockIdx.x == 0 && !last) {
        float* neu = a.state + ((size_t)row.slot * 2 + (par ^ 1)) * a.hf;
        const long long Bn = rh::hist_base(rt, Fn);
#pragma clang loop vectorize(disable)  // (likewise)
        for (long long g = Bn + tid; g < Rn && g - Bn < a.hf; g += THREADS) neu[g - Bn] = fetch(g);
    }
    if (live == 0) return;

    // ---- 1. stage the span: span[k] = x[sp.first + k]
    const rh::Span sp = rh::span_of(rt, m0, live);  // sp.count <= span_floats (audio_design.h: span_floats_for)
    {
        constexpr int CH = 16 / sizeof(TI);
        // chunk c of the span starts at the row's sample sp.first + c CH, i.e. at ch + (sp.first - R) + c CH: 16-byte aligned for every c or none
        const bool vec_ok = (((long long)reinterpret_cast<uintptr_t>(ch) + (sp.first - R) * (long long)sizeof(TI)) & 15) == 0;
        for (int c = tid; c < (sp.count + CH - 1) / CH; c += THREADS) {
            const long long i0 = sp.first + (long long)c * CH;
            if (vec_ok && i0 >= R && i0 + CH <= Rn) {
                const float4 raw = *reinterpret_cast<const float4*>(ch + (i0 - R));
                TI e[CH];
                __builtin_memcpy(e, &raw, 16);
#pragma unroll
                for (int j = 0; j < CH; ++j) span[c * CH + j] = to_float(e[j]);
            } else {
#pragma unroll
                for (int j = 0; j < CH; ++j) span[c * CH + j] = fetch(i0 + j);
            }
        }
    }
    __syncthreads();

    // ---- 2. one fmaf chain per output, ascending n
    const Phases ph = {a.table, rt.L, rt.M, rt.kp4, a.minv};
    span_outputs<TO>(ph, span, sp.sbase, sp.p0, live, live, out, tid, THREADS);
}

template <typename TI, typename TO>
hipError_t launch_stream(const RsArgs& a, const RsRows& rows, dim3 grid, size_t lds, hipStream_t s, vtts::DynLdsOnce& once) {
    const void* fn = reinterpret_cast<const void*>(&rs_stream_k<TI, TO>);
    hipError_t e = vtts::set_max_dynamic_lds(fn, VTTS_AUDIO_MAX_SPAN_BYTES, once);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((rs_stream_k<TI, TO>), grid, dim3(THREADS), lds, s, a, rows);
    return hipGetLastError();
}

constexpr int64_t MAX_S = 0x7fffffff;

}  // namespace

struct vtts_rsstream {
    rh::Ratio ratio = {};
    int minv = 0, span_floats = 0;
    size_t table_bytes = 0;
    rh::Layout lay;
    const float* blob = nullptr;
    vtts_stream_rows::Cursors cur;
    vtts::DynLdsOnce lds[4];
};

VTTS_API int vtts_rsstream_create(const vtts_audio_cfg* cfg, int device, int rows, int32_t max_chunk, vtts_rsstream** out) {
    (void)device;  // (the handle owns nothing on a device: the calls run on the caller's current one)
    if (!cfg || !out) return failf(VTTS_ERR_INVALID, "null argument");
    if (rows < 1 || rows > (1 << 24)) return failf(VTTS_ERR_INVALID, "rows must be in 1 .. 2^24 (got %d)", rows);
    if (max_chunk < 1 || max_chunk > VTTS_RSSTREAM_MAX_CHUNK)
        return failf(VTTS_ERR_INVALID, "max_chunk must be in 1 .. %d (got %d)", VTTS_RSSTREAM_MAX_CHUNK, max_chunk);
    ad::Design d;  // (for the ratio and the table's shape; the table itself is the Resampler's)
    char why[160];
    if (ad::design(cfg->in_rate, cfg->out_rate, d, why) != 0) return failf(VTTS_ERR_INVALID, "%s", why);
    auto* h = new (std::nothrow) vtts_rsstream();
    if (!h) return failf(VTTS_ERR_NOMEM, "host allocation failed");
    h->ratio = {d.L, d.M, d.half, d.kp4, d.identity ? 1 : 0};
    h->minv = d.minv;
    h->span_floats = d.span_floats;
    h->table_bytes = d.table.size() * sizeof(float);
    h->lay = rh::layout(h->ratio, rows);
    if (!h->cur.init(rows, max_chunk)) {
        delete h;
        return failf(VTTS_ERR_NOMEM, "host allocation failed");
    }
    *out = h;
    return VTTS_OK;
}

VTTS_API void vtts_rsstream_destroy(vtts_rsstream* h) { delete h; }

VTTS_API int vtts_rsstream_ratio(const vtts_rsstream* h, int32_t* L, int32_t* M, int32_t* half) {
    if (!h) return failf(VTTS_ERR_INVALID, "null argument");
    if (L) *L = h->ratio.L;
    if (M) *M = h->ratio.M;
    if (half) *half = h->ratio.half;
    return VTTS_OK;
}

VTTS_API int vtts_rsstream_state_bytes(const vtts_rsstream* h, size_t* bytes) {
    if (!h || !bytes) return failf(VTTS_ERR_INVALID, "null argument");
    *bytes = h->lay.bytes;
    return VTTS_OK;
}

VTTS_API int vtts_rsstream_packed_bytes(const vtts_rsstream* h, size_t* bytes) {
    if (!h || !bytes) return failf(VTTS_ERR_INVALID, "null argument");
    *bytes = h->table_bytes;
    return VTTS_OK;
}

VTTS_API int vtts_rsstream_bind_packed(vtts_rsstream* h, void* dev_blob, size_t blob_bytes) {
    if (!h) return failf(VTTS_ERR_INVALID, "null argument");
    if (int rc = check_blob(dev_blob, blob_bytes, h->table_bytes)) return rc;
    h->blob = static_cast<const float*>(dev_blob);
    return VTTS_OK;
}

VTTS_API int vtts_rsstream_reset(vtts_rsstream* h, int row) {
    if (!h) return failf(VTTS_ERR_INVALID, "null argument");
    if (!h->cur.has(row)) return failf(VTTS_ERR_INVALID, "reset: row %d is outside 0 .. %d", row, h->cur.rows - 1);
    h->cur.reset(row);
    return VTTS_OK;
}

VTTS_API int vtts_rsstream_cursor(const vtts_rsstream* h, int row, int64_t* received, int64_t* emitted, int* closed) {
    if (!h) return failf(VTTS_ERR_INVALID, "null argument");
    if (!h->cur.has(row)) return failf(VTTS_ERR_INVALID, "cursor: row %d is outside 0 .. %d", row, h->cur.rows - 1);
    if (received) *received = h->cur.R[row];
    if (emitted) *emitted = h->cur.F[row];
    if (closed) *closed = h->cur.closed[row];
    return VTTS_OK;
}

VTTS_API int vtts_rsstream_emit(const vtts_rsstream* h, int64_t received, int64_t emitted, int32_t count, int last, int64_t* new_emitted) {
    if (!h || !new_emitted) return failf(VTTS_ERR_INVALID, "null argument");
    if (received < 0 || emitted < 0 || count < 0 || received > MAX_S - count)
        return failf(VTTS_ERR_INVALID, "emit: need 0 <= emitted, 0 <= count and 0 <= received <= 2^31 - 1 - count (got %lld, %lld, %d)", (long long)emitted,
                     (long long)received, count);
    *new_emitted = rh::emit_rule(h->ratio, received, emitted, count, last != 0);
    return VTTS_OK;
}

VTTS_API int vtts_rsstream_push(vtts_rsstream* h, void* state_dev, const void* chunk_dev, int dtype, int n, const int32_t* rows_host, int64_t c_stride,
                                const int32_t* counts_host, const int32_t* last_host, void* out_dev, int out_dtype, int32_t* out_counts_host,
                                void* stream) {
    if (!h || !chunk_dev || !rows_host || !counts_host || !out_dev || !out_counts_host) return failf(VTTS_ERR_INVALID, "null argument");
    if (!state_dev && h->lay.bytes) return failf(VTTS_ERR_INVALID, "null argument");
    if (dtype != VTTS_AUDIO_F32 && dtype != VTTS_AUDIO_PCM16) return failf(VTTS_ERR_INVALID, "push: dtype must be VTTS_AUDIO_F32 or VTTS_AUDIO_PCM16 (got %d)", dtype);
    if (out_dtype != VTTS_AUDIO_F32 && out_dtype != VTTS_AUDIO_PCM16)
        return failf(VTTS_ERR_INVALID, "push: out_dtype must be VTTS_AUDIO_F32 or VTTS_AUDIO_PCM16 (got %d)", out_dtype);
    vtts_stream_rows::Cursors& cu = h->cur;
    if (n < 1 || n > cu.rows) return failf(VTTS_ERR_INVALID, "push: n must be in 1 .. rows = %d (got %d)", cu.rows, n);
    if (c_stride < 0) return failf(VTTS_ERR_INVALID, "push: c_stride must not be negative (got %lld)", (long long)c_stride);
    if (reinterpret_cast<uintptr_t>(state_dev) % 16) return failf(VTTS_ERR_INVALID, "push: the state must be 16-byte aligned");
    const rh::Ratio& rt = h->ratio;
    if (!rt.identity && !h->blob) return failf(VTTS_ERR_STATE, "push() before bind_packed()");

    // ---- every refusal before any bookkeeping changes; a row may reach MAX_S = 2^31 - 1 samples
    // the contract's bounds, row by row: F is the function of R the kernel derives, and the next history fits its buffer
    auto history_bound = [&](int i, int r, int64_t cnt, char (&why)[160]) {
        const int last = last_host && last_host[i] ? 1 : 0;
        const int64_t Rn = cu.R[r] + cnt, Fn = rh::emit_rule(rt, cu.R[r], cu.F[r], cnt, last);
        if (cu.F[r] == rh::emitted_of(rt, cu.R[r]) && (rt.identity || last || Rn - rh::hist_base(rt, Fn) <= rt.kp4 - 1)) return (int)VTTS_OK;
        snprintf(why, sizeof why, "push: row %d's cursors break the history bound (R %lld, F %lld)", r, (long long)cu.R[r], (long long)cu.F[r]);
        return (int)VTTS_ERR_STATE;
    };
    char why[160];
    if (int rc = cu.check_push(n, rows_host, counts_host, c_stride, 0, history_bound, why)) return failf(rc, "%s", why);

    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool pin = dtype == VTTS_AUDIO_PCM16, pout = out_dtype == VTTS_AUDIO_PCM16;
    const size_t isz = pin ? 2 : 4, osz = pout ? 2 : 4;
    RsArgs a;
    a.state = static_cast<float*>(state_dev);
    a.table = h->blob;
    a.c_stride = c_stride;
    a.ratio = rt;
    a.minv = h->minv;
    a.hf = (int)h->lay.hist_floats;
    const size_t lds = rt.identity ? 0 : (size_t)h->span_floats * sizeof(float);
    size_t in_total = 0, out_total = 0;
    for (int r0 = 0; r0 < n; r0 += ROWS_PER_LAUNCH) {
        const int nr = n - r0 < ROWS_PER_LAUNCH ? n - r0 : ROWS_PER_LAUNCH;
        RsRows rows = {};
        a.chunk = static_cast<const char*>(chunk_dev) + (c_stride ? (size_t)r0 * (size_t)c_stride : in_total) * isz;
        a.out = static_cast<char*>(out_dev) + out_total * osz;
        int in_off = 0;
        int64_t out_off = 0, tiles = 1;
        for (int b = 0; b < nr; ++b) {
            const int r = rows_host[r0 + b], cnt = counts_host[r0 + b], last = last_host && last_host[r0 + b] ? 1 : 0;
            const int64_t emit = rh::emit_rule(rt, cu.R[r], cu.F[r], cnt, last) - cu.F[r];  // < max_emit(): fits int32 by max_chunk and MAX_R
            RsRow& q = rows.r[b];
            q.out_off = out_off;
            q.in_off = in_off;
            q.R = (int)cu.R[r];
            q.cnt_flags = cnt << 2 | (int)cu.parity[r] << 1 | last;
            q.slot = r;
            in_off += cnt;
            out_off += emit;
            out_counts_host[r0 + b] = (int32_t)emit;
            if (rh::tiles_of(emit) > tiles) tiles = rh::tiles_of(emit);
        }
        in_total += (size_t)in_off;
        out_total += (size_t)out_off;
        const dim3 grid((unsigned)tiles, (unsigned)nr);
        hipError_t e;
        if (pin)
            e = pout ? launch_stream<short, short>(a, rows, grid, lds, s, h->lds[3]) : launch_stream<short, float>(a, rows, grid, lds, s, h->lds[2]);
        else
            e = pout ? launch_stream<float, short>(a, rows, grid, lds, s, h->lds[1]) : launch_stream<float, float>(a, rows, grid, lds, s, h->lds[0]);
        if (e != hipSuccess) return failf(VTTS_ERR_HIP, "resampler kernel launch failed: %s", hipGetErrorString(e));
        cu.advance(nr, rows_host + r0, counts_host + r0, last_host ? last_host + r0 : nullptr, out_counts_host + r0);  // the launch's rows have moved
    }
    return VTTS_OK;
}
