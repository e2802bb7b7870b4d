// The audio stage (include/vtts_audio.h): rational sample-rate conversion by L / M with a Kaiser-windowed sinc, and PCM16 <-> fp32 on
// either side, one fused kernel.  Samples of one format and rate in, samples of another out, strided or packed.
//
//   y[m] = sum_n x[n] h[m M - n L + half]          (zero extension at the row's own ends)
// With t = m M + half, q = t div L, p = t mod L the taps an output meets are h[p + j L], j = 0 .. , on x[q - j]: one row of the
// phase-major table.  The table's rows are reversed and right-aligned (row[L][kp4], kp4 = taps per phase rounded up to 4, the
// padding zeros first), so that walking a row forwards walks n upwards:
//   y[m] = sum_{i = 0 .. kp4 - 1} x[q - (kp4 - 1) + i] * row[p][i]          one fp32 fmaf chain in ascending n
//
//   workgroup = VTTS_AUDIO_OUT_PER_BLOCK (1024) consecutive outputs of one row, 256 threads.
//   1. stage: the input span the 1024 outputs meet, once, into LDS (16-byte loads where the row allows; PCM16 scaled by 2^-15 on
//      the way), zeros outside the row.  The span starts at a multiple of 8 samples, so its 16-byte chunks are the row's.
//      m M and n L pass 2^31 on long rows: the block's base (t0, q0, the span's first sample) is 64-bit, everything inside the block
//      is a 32-bit offset from it.
//   2. each output walks its phase's row with 16-byte loads.  The table stays in global memory: 86 KB at 441 / 160 does not fit LDS
//      beside the span with more than one workgroup per CU, and under 1 KB at 3 / 1 lives in the L1 either way.  Consecutive OUTPUTS have
//      phases M apart (mod L), and 64 lanes on 64 scattered rows cost 64 cache lines per load (measured: DESIGN.md section 6i).  So the
//      lanes take consecutive PHASES: inside each run of L outputs, slot s computes output s M^-1 mod L, whose phase is p0 + s, and the
//      table keeps four taps of every phase side by side ([kp4 / 4][L] float4): a wave's load is one contiguous kilobyte.  Which lane
//      computes an output changes nothing in its chain.
//   3. store fp32, or PCM16 by libsndfile's rule computed in double (clip, times 32767 exactly, round half to even; NaN -> 0).
// in_rate == out_rate skips 1. and 2.: the kernel converts and packs only.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <type_traits>

#include "../../include/vtts_audio.h"
#include "../../include/vtts_hifigan.h"
#include "audio_common.h"
#include "audio_design.h"
#include "launch_rows.h"
#include "vtts_internal.h"

using vtts::check_blob;
using vtts::failf;
using vtts::upload_blob;
namespace ad = vtts_audio_design;
using vtts_audio_dev::floor8;
using vtts_audio_dev::from_float;
using vtts_audio_dev::Phases;
using vtts_audio_dev::span_outputs;
using vtts_audio_dev::to_float;

namespace {

constexpr int OPB = VTTS_AUDIO_OUT_PER_BLOCK;
constexpr int THREADS = 256;
constexpr int ROWS_PER_LAUNCH = 128;

using AudioRows = vtts_rows::OffLens<ROWS_PER_LAUNCH>;  // input samples and first output element (from a.out) of each row of this launch

struct AudioArgs {
    const void* in;      // first row of this launch
    void* out;           // the call's output
    const float* table;  // [kp4 / 4][L][4]
    long long s_stride;  // input samples between rows
    long long o_stride;  // output samples to write per row (the rest of a row past its own count is zeroed); 0 = packed: the row's own count
    int L, M, half, kp4;
    int minv;            // M^-1 mod L
    int vec_ok;          // input rows are 16-byte aligned: interior chunks take one 16-byte load
    int identity;        // in_rate == out_rate
};

template <typename TI, typename TO>
__global__ __launch_bounds__(THREADS) void audio_resample_k(const AudioArgs a, const AudioRows rows) {
    extern __shared__ float4 lds4[];
    float* span = reinterpret_cast<float*>(lds4);
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const int S = rows.len[b];
    const long long So = a.identity ? (long long)S : ((long long)S * a.L + a.M - 1) / a.M;
    const long long cap = a.o_stride ? a.o_stride : So;
    const long long m0 = (long long)blockIdx.x * OPB;
    if (m0 >= cap) return;  // block-uniform
    const int cnt = (int)min((long long)OPB, cap - m0);                   // outputs this block writes
    const int live = (int)max(0LL, min((long long)OPB, So - m0));        // ... of which the row has this many; the rest are zero
    TO* out = static_cast<TO*>(a.out) + rows.off[b] + m0;
    const TI* x = static_cast<const TI*>(a.in) + (long long)b * a.s_stride;

    if (a.identity || live == 0) {
        for (int i = tid; i < cnt; i += THREADS) {
            if constexpr (std::is_same<TI, TO>::value)
                out[i] = i < live ? x[m0 + i] : TO(0);  // the same format on both sides is a copy
            else
                out[i] = from_float<TO>(i < live ? to_float(x[m0 + i]) : 0.0f);
        }
        return;
    }

    // ---- 1. stage the span: span[k] = x[nb + k], zero outside [0, S)
    const long long t0 = m0 * a.M + a.half;
    const long long q0 = t0 / a.L;
    const int p0 = (int)(t0 - q0 * a.L);
    const long long nb = floor8(q0 - (a.kp4 - 1));
    const int nspan = (int)(q0 + (p0 + (long long)(live - 1) * a.M) / a.L - nb) + 1;  // <= span_floats (audio_design.h: span_floats_for)
    {
        constexpr int CH = 16 / sizeof(TI);
        for (int c = tid; c < (nspan + CH - 1) / CH; c += THREADS) {
            const long long i0 = nb + (long long)c * CH;
            if (a.vec_ok && i0 >= 0 && i0 + CH <= S) {
                const float4 raw = *reinterpret_cast<const float4*>(x + i0);
                TI e[CH];
                __builtin_memcpy(e, &raw, 16);
#pragma unroll
                for (int j = 0; j < CH; ++j) span[c * CH + j] = to_float(e[j]);
            } else {
#pragma unroll
                for (int j = 0; j < CH; ++j) {
                    const long long i = i0 + j;
                    span[c * CH + j] = (i >= 0 && i < S) ? to_float(x[i]) : 0.0f;
                }
            }
        }
    }
    __syncthreads();

    // ---- 2./3. one fmaf chain per output, ascending n
    const int sbase = (int)(q0 - nb) - (a.kp4 - 1);  // >= 0: span index of x[q0 - (kp4 - 1)]
    const Phases ph = {a.table, a.L, a.M, a.kp4, a.minv};
    span_outputs<TO>(ph, span, sbase, p0, cnt, live, out, tid, THREADS);
}

template <typename TI, typename TO>
hipError_t launch(const AudioArgs& a, const AudioRows& rows, dim3 grid, size_t lds, hipStream_t s, vtts::DynLdsOnce& once) {
    const void* fn = reinterpret_cast<const void*>(&audio_resample_k<TI, TO>);
    hipError_t e = vtts::set_max_dynamic_lds(fn, VTTS_AUDIO_MAX_SPAN_BYTES, once);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((audio_resample_k<TI, TO>), grid, dim3(THREADS), lds, s, a, rows);
    return hipGetLastError();
}

}  // namespace

struct vtts_audio {
    ad::Design d;
    int device = 0;
    const float* blob = nullptr;
    vtts::DynLdsOnce lds[4];
};

VTTS_API int vtts_audio_create(const vtts_audio_cfg* cfg, int device, vtts_audio** out) {
    if (!cfg || !out) return failf(VTTS_ERR_INVALID, "null argument");
    auto* h = new (std::nothrow) vtts_audio();
    if (!h) return failf(VTTS_ERR_NOMEM, "host allocation failed");
    char why[160];
    if (ad::design(cfg->in_rate, cfg->out_rate, h->d, why) != 0) {
        delete h;
        return failf(VTTS_ERR_INVALID, "%s", why);
    }
    h->device = device;
    *out = h;
    return VTTS_OK;
}

VTTS_API void vtts_audio_destroy(vtts_audio* h) { delete h; }

VTTS_API int vtts_audio_ratio(const vtts_audio* h, int32_t* L, int32_t* M, int32_t* half) {
    if (!h) return failf(VTTS_ERR_INVALID, "null argument");
    if (L) *L = h->d.L;
    if (M) *M = h->d.M;
    if (half) *half = h->d.half;
    return VTTS_OK;
}

VTTS_API int vtts_audio_out_samples(const vtts_audio* h, int64_t n_in, int64_t* n_out) {
    if (!h || !n_out) return failf(VTTS_ERR_INVALID, "null argument");
    if (n_in < 0 || n_in > 0x7fffffff) return failf(VTTS_ERR_SHAPE, "n_in must be in 0 .. 2^31 - 1 (got %lld)", (long long)n_in);
    *n_out = ad::out_samples(h->d, n_in);
    return VTTS_OK;
}

VTTS_API int vtts_audio_prototype(const vtts_audio* h, double* host_out) {
    if (!h || !host_out) return failf(VTTS_ERR_INVALID, "null argument");
    memcpy(host_out, h->d.proto.data(), h->d.proto.size() * sizeof(double));
    return VTTS_OK;
}

VTTS_API int vtts_audio_packed_bytes(const vtts_audio* h, size_t* bytes) {
    if (!h || !bytes) return failf(VTTS_ERR_INVALID, "null argument");
    *bytes = h->d.table.size() * sizeof(float);
    return VTTS_OK;
}

VTTS_API int vtts_audio_pack(vtts_audio* h, void* dev_blob, size_t blob_bytes, void* stream) {
    if (!h) return failf(VTTS_ERR_INVALID, "null argument");
    const size_t need = h->d.table.size() * sizeof(float);
    if (int rc = check_blob(dev_blob, blob_bytes, need)) return rc;
    if (int rc = upload_blob(dev_blob, h->d.table.data(), need, static_cast<hipStream_t>(stream), "the tap table")) return rc;
    h->blob = static_cast<const float*>(dev_blob);
    return VTTS_OK;
}

VTTS_API int vtts_audio_bind_packed(vtts_audio* h, void* dev_blob, size_t blob_bytes) {
    if (!h) return failf(VTTS_ERR_INVALID, "null argument");
    const size_t need = h->d.table.size() * sizeof(float);
    if (int rc = check_blob(dev_blob, blob_bytes, need)) return rc;
    h->blob = static_cast<const float*>(dev_blob);
    return VTTS_OK;
}

VTTS_API int vtts_audio_forward(vtts_audio* h, const void* in_dev, int in_dtype, int N, int64_t S_stride, const int32_t* lengths, void* out_dev,
                                int out_dtype, int64_t O_stride, void* stream) {
    if (!h || !in_dev || !out_dev) return failf(VTTS_ERR_INVALID, "null argument");
    if ((in_dtype != VTTS_AUDIO_F32 && in_dtype != VTTS_AUDIO_PCM16) || (out_dtype != VTTS_AUDIO_F32 && out_dtype != VTTS_AUDIO_PCM16))
        return failf(VTTS_ERR_INVALID, "dtype must be VTTS_AUDIO_F32 or VTTS_AUDIO_PCM16 (got in %d, out %d)", in_dtype, out_dtype);
    const ad::Design& d = h->d;
    if (!d.identity && !h->blob) return failf(VTTS_ERR_STATE, "forward() before pack()/bind_packed()");
    ad::Rows plan;
    char why[160];
    const int rc = ad::plan_rows(d, N, S_stride, lengths, O_stride, plan, why);
    if (rc != 0) return failf(rc, "%s", why);
    if (plan.cover == 0) return VTTS_OK;  // packed, and every row is empty

    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool pin = in_dtype == VTTS_AUDIO_PCM16, pout = out_dtype == VTTS_AUDIO_PCM16;
    const size_t esz = pin ? 2 : 4;
    AudioArgs a;
    a.out = out_dev;
    a.table = h->blob;
    a.s_stride = S_stride;
    a.o_stride = O_stride;
    a.L = d.L;
    a.M = d.M;
    a.half = d.half;
    a.kp4 = d.kp4;
    a.minv = d.minv;
    a.vec_ok = reinterpret_cast<uintptr_t>(in_dev) % 16 == 0 && ((size_t)S_stride * esz) % 16 == 0;
    a.identity = d.identity ? 1 : 0;
    const size_t lds = d.identity ? 0 : (size_t)d.span_floats * sizeof(float);
    const unsigned tiles = (unsigned)((plan.cover + OPB - 1) / OPB);
    // the rows' lengths and offsets travel as kernel arguments: plan_rows() has checked them, a row of len samples writes out_samples(d, len)
    const auto count = [&](int len) { return (long long)ad::out_samples(d, len); };
    return vtts_rows::for_each_launch_off<ROWS_PER_LAUNCH>(N, lengths, S_stride, O_stride, count, [&](int r0, int nr, const AudioRows& rows) -> int {
        a.in = static_cast<const char*>(in_dev) + (size_t)r0 * S_stride * esz;
        const dim3 grid(tiles, (unsigned)nr);
        hipError_t e;
        if (pin)
            e = pout ? launch<short, short>(a, rows, grid, lds, s, h->lds[3]) : launch<short, float>(a, rows, grid, lds, s, h->lds[2]);
        else
            e = pout ? launch<float, short>(a, rows, grid, lds, s, h->lds[1]) : launch<float, float>(a, rows, grid, lds, s, h->lds[0]);
        if (e != hipSuccess) return failf(VTTS_ERR_HIP, "audio kernel launch failed: %s", hipGetErrorString(e));
        return VTTS_OK;
    });
}
