// Batched YIN F0 tracker (include/vtts_pitch.h), one fused kernel on the mel front end's framing.  Samples in, three floats per frame
// out; the difference function d, the normalised c and the running sum never reach HBM.
//
//   workgroup = VTTS_PITCH_FRAMES_PER_BLOCK (8) consecutive frames of one row, one wave per frame.
//   1. stage: the (8 + 3) * 256 samples the eight frames cover, once, into LDS (16-byte loads; PCM16 scaled by 2^-15 on the way),
//      mirrored at the ROW'S OWN ends, as mel.hip does.  The image is shifted by sh = (-base) & 3 floats so that x[base] of every
//      frame sits on a 16-byte boundary (frames are 1024 bytes apart).
//   2. difference function.  Lane l owns the lags l, l + 64, ..., one chain each.  With u = j + 64 k, chain k of lane l needs
//          x[base + j]          the same value in every lane: one broadcast ds_read_b128 per four steps
//          x[base + l + u]      the lane's own stream: the SAME value for every k at the same u
//      so the kernel walks u in blocks of 64.  Block c loads the lane's 64 stream values once (conflict-free ds_read_b32: consecutive
//      lanes, consecutive words) and advances every chain that is inside its j range there: chain k = c - r is at j = 64 r + i,
//      r = 0 .. 7.  Each chain is still one fp32 chain in ascending j.  The eight accumulators are indexed by r, so the code is
//      static: at the end of a block they move up one place, the chain at r = 7 is complete and goes to LDS, r = 0 starts a new
//      lag block at 0.  Blocks of lags past tau_max are skipped by wave-uniform branches.  Per step: subtract, multiply, add, each
//      rounded (the file is built without contraction and tests/test_pitch_cpu.py reads the ISA for FMAs); per 192 VALU
//      operations 16 broadcast reads, and 64 stream reads per block of up to 1536.
//      Lanes whose lag is past tau_max run chains nobody reads; their stream reads go past the frame, into the next frames or the
//      zeroed 128-float tail of the image (at most word 2880 of 2948: static_assert below), never out of the array.
//   3. running sum: lane 0, one sequential chain over d[0 .. tau_max] (d[0] = +0 exactly, so starting at 0 changes nothing), read
//      and written as float4 through LDS.  At most 516 dependent adds per frame, the price of the == contract.
//   4. c[tau] = run > 0 ? (d * tau) / run : 1, every lane its own lags, IEEE divide, in place over d.
//   5. pick: per lag block, ballot of (c < threshold and at a local minimum), first set bit of the first non-empty block.  Unvoiced:
//      wave minimum of c over the search range, then the first lag that holds it, by the same ballot.
//   6. refinement and the three stores by lane 0.
//   A wave touches only its own d / run buffers after the staging barrier; the LDS keeps one wave's accesses in order, so the phases are
//   separated by a compiler-only wave fence (wave_sync), as in mel.hip.  49 KB of LDS per workgroup: three per CU.
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>

#include "../../include/vtts_hifigan.h"
#include "../../include/vtts_mel.h"
#include "../../include/vtts_pitch.h"
#include "launch_rows.h"
#include "mel_framing.h"
#include "sample_convert.h"
#include "vtts_internal.h"
#include "wave_common.h"

// The contract's operations are single fp32 operations: nothing in this file may be fused into an FMA.  The pragma covers this file's own
// operators; __fsub_rn / __fmul_rn / __fadd_rn / __fdiv_rn are plain operators of a header that precedes it, which hipcc contracts all the
// same, so build.py compiles this file with -ffp-contract=off as well (FILE_FLAGS).  Division is hipcc's default correctly rounded one.
#pragma clang fp contract(off)

using vtts::failf;
using vtts_sample::to_float;
using vtts_wave::wave_sync;
namespace mf = vtts_mel_framing;

namespace {

constexpr int NFFT = VTTS_PITCH_NFFT, HOP = VTTS_PITCH_HOP, PADL = VTTS_PITCH_PAD, W = VTTS_PITCH_WINDOW, MAX_LAG = VTTS_PITCH_MAX_LAG;
constexpr int FPB = VTTS_PITCH_FRAMES_PER_BLOCK;          // frames (= waves) per workgroup
constexpr int THREADS = 64 * FPB;
constexpr int SPAN = (FPB + 3) * HOP;                     // samples the FPB frames cover
constexpr int TAIL = 128;                                 // zeroed floats behind the span: where unowned lags' stream reads end up
constexpr int IMG = 4 + SPAN + TAIL;                      // the staged image: shift (< 4), span, tail
constexpr int RUNS = W / 64;                              // 8: chains in flight per lane = 64-blocks of j
constexpr int MAX_LAG_BLOCKS = MAX_LAG / 64 + 1;          // 9: lags 0 .. 512
constexpr int LAGBUF = 64 * MAX_LAG_BLOCKS;               // floats of one wave's d (then c) buffer, and of its running-sum buffer
constexpr int ROWS_PER_LAUNCH = 256;
// the last word any lane reads from the image: shift 3, last frame, base + lane 63 + the last block's last step (tau_max = 512: base 0)
static_assert(3 + (FPB - 1) * HOP + 63 + 64 * (MAX_LAG_BLOCKS - 1 + RUNS - 1) + 63 < IMG, "stream reads stay inside the staged image");
static_assert(NFFT == mf::NFFT && HOP == mf::HOP && PADL == mf::PADL && W == 512 && W + MAX_LAG == NFFT, "the kernel is built for the mel framing");
static_assert(VTTS_PITCH_MIN_SAMPLES == VTTS_MEL_MIN_SAMPLES, "one rule for the shortest row");
static_assert((size_t)(IMG + FPB * 2 * LAGBUF) * sizeof(float) <= 64 * 1024, "static LDS");

using Rows = vtts_rows::Lens<ROWS_PER_LAUNCH>;  // samples of each row of this launch

struct PitchArgs {
    const void* wav;   // first row of this launch
    float* f0;         // first row of this launch, as the two below
    float* ap;
    float* cand;
    long s_stride;     // samples between rows
    long t_stride;     // frames between output rows = frames to write per row
    int tau_min, tau_max;
    int vec_ok;        // rows are 16-byte aligned: interior chunks take one 16-byte load
    float threshold;
    float rate;        // (float)sample_rate
};

// one step of a chain: s + (a - y)^2, three rounded operations
__device__ __forceinline__ float step(float s, float a, float y) {
    const float e = __fsub_rn(a, y);
    return __fadd_rn(s, __fmul_rn(e, e));
}

template <typename T>
__global__ __launch_bounds__(THREADS) void pitch_yin_k(const PitchArgs a, const Rows rows) {
    __shared__ float4 lds4[(IMG + FPB * 2 * LAGBUF) / 4];
    float* lds = reinterpret_cast<float*>(lds4);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* dbuf = lds + IMG + wave * 2 * LAGBUF;  // d[tau], then c[tau]
    float* rbuf = dbuf + LAGBUF;                  // run[tau]

    const int b = blockIdx.y;
    const int L = rows.len[b];                 // >= 385 (checked on the host)
    const int Tb = (L + 2 * PADL - NFFT) / HOP + 1;
    const int t0 = blockIdx.x * FPB;
    const int t = t0 + wave;
    const long o = (long)b * a.t_stride + t;
    if (t0 >= Tb) {  // the whole tile lies past this row's frames (block-uniform): fill only
        if (lane == 0 && t < a.t_stride) a.f0[o] = 0.0f, a.ap[o] = 1.0f, a.cand[o] = 0.0f;
        return;
    }
    const int tau_max = a.tau_max, tau_min = a.tau_min;
    const int base = (NFFT - W - tau_max) / 2;
    const int sh = (4 - (base & 3)) & 3;

    // ---- 1. stage the span: img[sh + j] = padded sample 256 t0 + j = row sample 256 t0 - 384 + j, reflected at the row's ends
    {
        const T* x = static_cast<const T*>(a.wav) + (long)b * a.s_stride;
        const long q0 = (long)t0 * HOP - PADL;
        constexpr int CH = 16 / sizeof(T);
        float* span = lds + sh;
        for (int c = tid; c < SPAN / CH; c += THREADS) {
            const long i0 = q0 + (long)c * CH;
            if (a.vec_ok && i0 >= 0 && i0 + CH <= L) {
                const float4 raw = *reinterpret_cast<const float4*>(x + i0);
                T e[CH];
                __builtin_memcpy(e, &raw, 16);
#pragma unroll
                for (int j = 0; j < CH; ++j) span[c * CH + j] = to_float(e[j]);
            } else {
#pragma unroll
                for (int j = 0; j < CH; ++j) {
                    long i = i0 + j;
                    if (i < 0) i = -i;
                    if (i >= L) i = 2 * ((long)L - 1) - i;
                    i = min(max(i, 0L), (long)L - 1);  // frames past the row's end (never stored) stay inside the row
                    span[c * CH + j] = to_float(x[i]);
                }
            }
        }
        if (tid < sh) lds[tid] = 0.0f;
        for (int i = sh + SPAN + tid; i < IMG; i += THREADS) lds[i] = 0.0f;
    }
    __syncthreads();
    if (t >= Tb) {  // a frame past the row's own count (wave-uniform); no barrier follows
        if (lane == 0 && t < a.t_stride) a.f0[o] = 0.0f, a.ap[o] = 1.0f, a.cand[o] = 0.0f;
        return;
    }

    // ---- 2. difference function
    const int nblk = tau_max / 64 + 1;  // lag blocks: lags 0 .. tau_max
    {
        const float* xa = lds + sh + wave * HOP + base;  // x[base + j], 16-byte aligned
        const float* xs = xa + lane;                     // the lane's stream
        float acc[RUNS];
#pragma unroll
        for (int r = 0; r < RUNS; ++r) acc[r] = 0.0f;
#pragma unroll 1
        for (int c = 0; c < nblk + RUNS - 1; ++c) {
            float y[64];
#pragma unroll
            for (int i = 0; i < 64; ++i) y[i] = xs[64 * c + i];
#pragma unroll
            for (int r = 0; r < RUNS; ++r) {
                const int k = c - r;
                if (k >= 0 && k < nblk) {  // wave-uniform
                    const float4* a4 = reinterpret_cast<const float4*>(xa + 64 * r);
                    float s = acc[r];
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const float4 v = a4[q];
                        s = step(s, v.x, y[4 * q]);
                        s = step(s, v.y, y[4 * q + 1]);
                        s = step(s, v.z, y[4 * q + 2]);
                        s = step(s, v.w, y[4 * q + 3]);
                    }
                    acc[r] = s;
                }
            }
            if (c >= RUNS - 1) dbuf[64 * (c - (RUNS - 1)) + lane] = acc[RUNS - 1];  // c - 7 < nblk by the loop's bound
#pragma unroll
            for (int r = RUNS - 1; r > 0; --r) acc[r] = acc[r - 1];
            acc[0] = 0.0f;
        }
    }
    wave_sync();

    // ---- 3. the running sum, one chain
    if (lane == 0) {
        const float4* d4 = reinterpret_cast<const float4*>(dbuf);
        float4* r4 = reinterpret_cast<float4*>(rbuf);
        float run = 0.0f;
#pragma unroll 4
        for (int g = 0; g <= tau_max / 4; ++g) {
            const float4 d = d4[g];
            float4 r;
            r.x = run = __fadd_rn(run, d.x);
            r.y = run = __fadd_rn(run, d.y);
            r.z = run = __fadd_rn(run, d.z);
            r.w = run = __fadd_rn(run, d.w);
            r4[g] = r;
        }
    }
    wave_sync();

    // ---- 4. c, in place over d (not vectorised: the loop vectoriser pairs two blocks' multiplies into v_pk_mul_f32, which this library bans)
#pragma clang loop vectorize(disable)
    for (int k = 0; k < nblk; ++k) {
        const int tau = 64 * k + lane;
        const float d = dbuf[tau], run = rbuf[tau];
        float c = 1.0f;
        if (tau >= 1 && run > 0.0f) c = __fdiv_rn(__fmul_rn(d, (float)tau), run);
        dbuf[tau] = c;
    }
    wave_sync();

    // ---- 5. pick
    const float* c = dbuf;
    int pick = -1;
    for (int k = 0; k < nblk; ++k) {
        const int tau = 64 * k + lane;
        const float cv = c[min(tau, tau_max)], cn = c[min(tau + 1, tau_max)];
        const bool hit = tau >= tau_min && tau <= tau_max && cv < a.threshold && (tau == tau_max || cn >= cv);
        const unsigned long long m = __ballot(hit);
        if (m) {
            pick = 64 * k + __ffsll(m) - 1;
            break;
        }
    }
    const bool voiced = pick >= 0;
    if (!voiced) {
        float vmin = INFINITY;
        for (int k = 0; k < nblk; ++k) {
            const int tau = 64 * k + lane;
            if (tau >= tau_min && tau <= tau_max) vmin = fminf(vmin, c[tau]);
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) vmin = fminf(vmin, __shfl_xor(vmin, s));
        pick = tau_min;  // (kept if nothing compares equal: non-finite input)
        for (int k = 0; k < nblk; ++k) {
            const int tau = 64 * k + lane;
            const unsigned long long m = __ballot(tau >= tau_min && tau <= tau_max && c[tau] == vmin);
            if (m) {
                pick = 64 * k + __ffsll(m) - 1;
                break;
            }
        }
    }

    // ---- 6. refinement and stores
    if (lane == 0) {
        const float bq = c[pick];
        float tau_f = (float)pick;
        if (pick + 1 <= tau_max) {
            const float aq = c[pick - 1], gq = c[pick + 1];
            const float den = __fsub_rn(__fadd_rn(aq, gq), __fadd_rn(bq, bq));
            if (den > 0.0f) {
                float delta = __fdiv_rn(__fmul_rn(0.5f, __fsub_rn(aq, gq)), den);
                delta = fminf(fmaxf(delta, -1.0f), 1.0f);
                tau_f = __fadd_rn(tau_f, delta);
            }
        }
        const float cand = __fdiv_rn(a.rate, tau_f);
        a.f0[o] = voiced ? cand : 0.0f;
        a.ap[o] = bq;
        a.cand[o] = cand;
    }
}

}  // namespace

struct vtts_pitch {
    vtts_pitch_cfg cfg;
    int device = 0;
    int tau_min = 0, tau_max = 0;
};

VTTS_API int vtts_pitch_create(const vtts_pitch_cfg* cfg, int device, vtts_pitch** out) {
    if (!cfg || !out) return failf(VTTS_ERR_INVALID, "null argument");
    const vtts_pitch_cfg& c = *cfg;
    if (c.sample_rate <= 0 || c.sample_rate > (1 << 24)) return failf(VTTS_ERR_INVALID, "sample_rate must be in 1 .. 2^24 (got %d)", c.sample_rate);
    if (!(c.fmin > 0.0f) || !(c.fmax > 0.0f) || !std::isfinite(c.fmin) || !std::isfinite(c.fmax))
        return failf(VTTS_ERR_INVALID, "fmin and fmax must be positive and finite (got %g, %g)", c.fmin, c.fmax);
    if (!(c.threshold > 0.0f) || !(c.threshold < 1.0f)) return failf(VTTS_ERR_INVALID, "need 0 < threshold < 1 (got %g)", c.threshold);
    const double lo = std::ceil((double)c.sample_rate / (double)c.fmax), hi = std::floor((double)c.sample_rate / (double)c.fmin);
    if (!(lo >= 2.0) || !(lo <= hi) || !(hi <= (double)MAX_LAG))
        return failf(VTTS_ERR_INVALID, "need 2 <= tau_min = ceil(sample_rate / fmax) <= tau_max = floor(sample_rate / fmin) <= %d (got tau_min %.0f, tau_max %.0f)",
                     MAX_LAG, lo, hi);
    auto* h = new (std::nothrow) vtts_pitch();
    if (!h) return failf(VTTS_ERR_NOMEM, "host allocation failed");
    h->cfg = c;
    h->device = device;
    h->tau_min = (int)lo;
    h->tau_max = (int)hi;
    *out = h;
    return VTTS_OK;
}

VTTS_API void vtts_pitch_destroy(vtts_pitch* h) { delete h; }

VTTS_API int vtts_pitch_num_frames(const vtts_pitch* h, int64_t n_samples, int64_t* frames) {
    if (!h || !frames) return failf(VTTS_ERR_INVALID, "null argument");
    if (int rc = mf::check_shortest(n_samples)) return rc;
    *frames = mf::num_frames(n_samples);
    return VTTS_OK;
}

VTTS_API int vtts_pitch_workspace_bytes(const vtts_pitch* h, int N, int64_t S, size_t* bytes) {
    if (!h || !bytes) return failf(VTTS_ERR_INVALID, "null argument");
    if (N <= 0) return failf(VTTS_ERR_INVALID, "N must be positive (got %d)", N);
    if (int rc = mf::check_shortest(S)) return rc;
    *bytes = 0;  // d, c and the running sum live in LDS; the row lengths travel as kernel arguments
    return VTTS_OK;
}

VTTS_API int vtts_pitch_forward(vtts_pitch* h, const void* wav_dev, int dtype, int N, int64_t S_stride, const int32_t* lengths, float* f0_dev,
                                float* aperiodicity_dev, float* candidate_dev, int64_t T_stride, void* workspace, void* stream) {
    (void)workspace;
    if (!h || !wav_dev || !f0_dev || !aperiodicity_dev || !candidate_dev) return failf(VTTS_ERR_INVALID, "null argument");
    if (dtype != VTTS_MEL_F32 && dtype != VTTS_MEL_PCM16) return failf(VTTS_ERR_INVALID, "dtype must be VTTS_MEL_F32 or VTTS_MEL_PCM16 (got %d)", dtype);
    if (N <= 0) return failf(VTTS_ERR_INVALID, "N must be positive (got %d)", N);
    if (int rc = mf::check_batch(N, S_stride, lengths, T_stride)) return rc;
    const int64_t tiles = (T_stride + FPB - 1) / FPB;
    if (tiles > 0x7fffffff) return failf(VTTS_ERR_SHAPE, "T_stride = %lld is too large", (long long)T_stride);

    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool pcm = dtype == VTTS_MEL_PCM16;
    const size_t esz = pcm ? 2 : 4;
    PitchArgs a;
    a.s_stride = S_stride;
    a.t_stride = T_stride;
    a.tau_min = h->tau_min;
    a.tau_max = h->tau_max;
    a.vec_ok = reinterpret_cast<uintptr_t>(wav_dev) % 16 == 0 && (S_stride * esz) % 16 == 0;
    a.threshold = h->cfg.threshold;
    a.rate = (float)h->cfg.sample_rate;
    return vtts_rows::for_each_launch<ROWS_PER_LAUNCH>(N, lengths, S_stride, [&](int r0, int nr, const Rows& rows) -> int {
        a.wav = static_cast<const char*>(wav_dev) + (size_t)r0 * S_stride * esz;
        a.f0 = f0_dev + (size_t)r0 * T_stride;
        a.ap = aperiodicity_dev + (size_t)r0 * T_stride;
        a.cand = candidate_dev + (size_t)r0 * T_stride;
        const dim3 grid((unsigned)tiles, (unsigned)nr);
        if (pcm)
            hipLaunchKernelGGL(pitch_yin_k<short>, grid, dim3(THREADS), 0, s, a, rows);
        else
            hipLaunchKernelGGL(pitch_yin_k<float>, grid, dim3(THREADS), 0, s, a, rows);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return failf(VTTS_ERR_HIP, "pitch kernel launch failed: %s", hipGetErrorString(e));
        return VTTS_OK;
    });
}
