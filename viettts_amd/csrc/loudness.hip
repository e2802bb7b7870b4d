// The loudness meter (include/vtts_loudness.h): BS.1770 K-weighting, 400 ms blocks, the two gates, and a per-row gain into fp32 or PCM16.
//
// K-weighting is a 4th-order IIR along up to hundreds of thousands of samples per row, and 64 rows do not fill 256 CUs, so the filter
// is cut along time.  One sample maps the filter's state s -> A s + B x (loudness_design.h); a run of n samples maps s -> A^n s + p
// with p the state the run leaves from a ZERO incoming state.  These affine maps compose, so:
//
//   loud_scan_k, one workgroup (256 lanes) per VTTS_LOUDNESS_SEGMENT = 8192 samples of one row:
//     1. stage the segment in LDS with coalesced loads (PCM16 scaled by 2^-15), zeros past the row's end.  Lane c's chunk of
//        VTTS_LOUDNESS_CHUNK = 32 samples starts at word 33 c: the padding keeps 64 lanes walking their chunks off one bank.
//     2. each lane filters its chunk from zero state, in place (the particular solution), and keeps its end state p and max |x|.
//     3. an inclusive scan over the wave's 64 lanes (6 steps, p += A^(32 d) p[lane - d]), the four waves' totals through LDS, and the
//        segment's incoming state: a prefix over the earlier segments' end states (s = A^8192 s + p_j, at most S / 8192 steps).
//        Those come from a first launch of the same kernel that stops here and leaves each segment's end state in the workspace.
//     4. each lane adds the homogeneous response htab[i] . s_in of its incoming state to its 32 samples, squares in double, and sums
//        into the (at most two) hops its chunk meets; a butterfly per hop over the wave, the four waves in order, and the segment's share
//        of each hop it meets goes to the workspace.
//   loud_gate_k, one wave per row: hop sums from the segments' shares in segment order, block energies, both gates, every sum a lane's
//     sequential partial in ascending j followed by a butterfly: a fixed order.
//   loud_gain_k / loud_apply_k: the gain rule on the device, then one streaming multiply and store.
//
// Passes over HBM: measure reads the samples twice (end states, then hop sums) and writes a few bytes per segment; normalise reads them once
// and writes the output once.  The filter's tables (427 floats) travel as kernel arguments, as do the rows' lengths, 128 rows per launch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>
#include <type_traits>

#include "../../include/vtts_audio.h"
#include "../../include/vtts_hifigan.h"
#include "../../include/vtts_loudness.h"
#include "launch_rows.h"
#include "loudness_design.h"
#include "sample_convert.h"
#include "vtts_internal.h"
#include "wave_common.h"

using vtts::check_rows;
using vtts::failf;
using vtts_sample::from_float;
using vtts_sample::to_float;
using vtts_wave::wave_sum;
namespace ld = vtts_loudness_design;

namespace {

constexpr int CHUNK = ld::CHUNK;
constexpr int SEGMENT = ld::SEGMENT;
constexpr int SLOTS = ld::SLOTS;
constexpr int WAVES = ld::WAVES;
constexpr int THREADS = 256;
constexpr int WAVE_SPAN = CHUNK * 64;
constexpr int ROWS_PER_LAUNCH = 128;
constexpr int APPLY_TILE = 4096;
static_assert(THREADS == WAVES * 64 && THREADS * CHUNK == SEGMENT, "one lane per chunk");

using LoudLens = vtts_rows::Lens<ROWS_PER_LAUNCH>;     // samples of each row of this launch
using LoudRows = vtts_rows::OffLens<ROWS_PER_LAUNCH>;  // normalise: and each row's first output element, from the call's out

struct ScanArgs {
    const void* wav;      // first row of this launch
    long long s_stride;   // samples between rows
    long long nseg;       // segments between rows in the three arrays below
    double* partial;      // [rows][nseg][SLOTS]   (the launch's first row, as the next two)
    float* state;         // [rows][nseg][4]
    float* peak;          // [rows][nseg]
    int H;
};

struct GateArgs {
    long long nseg, nhop;  // per-row strides
    const double* partial;
    double* hops;          // [rows][nhop]
    const float* peak;
    float* integrated;     // [rows], the launch's first row, as the four below
    float* momentary_max;
    float* sample_peak;
    int* n_blocks;
    int* n_gated;
    float* momentary;      // NULL, or [rows][j_stride]
    long long j_stride;
    int H;
};

struct ApplyArgs {
    const void* wav;  // first row of this launch
    void* out;        // the call's output
    const float* gains;
    long long s_stride;
    long long o_stride;  // 0 = packed
};

// r = m s, m row-major 4 x 4
__device__ __forceinline__ void matvec(const float* m, const float (&s)[4], float (&r)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = fmaf(m[4 * i + 3], s[3], fmaf(m[4 * i + 2], s[2], fmaf(m[4 * i + 1], s[1], m[4 * i] * s[0])));
}

// FULL = false: stop after the scan and leave the segment's end state (from a zero incoming state) in a.state; the row's last segment is
// skipped, nobody needs its end state.  FULL = true: the whole of the file comment.
template <typename TI, bool FULL>
__global__ __launch_bounds__(THREADS) void loud_scan_k(const ScanArgs a, const ld::Tables t, const LoudLens rows) {
    __shared__ float xs[SEGMENT + SEGMENT / CHUNK];  // chunk c at word (CHUNK + 1) c
    __shared__ float pw[256];                        // t.lo, t.hi: indexed by lane
    __shared__ float wtot[WAVES][4];
    __shared__ double part[WAVES * SLOTS];
    __shared__ float pkw[WAVES];

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b = blockIdx.y;
    const int len = rows.len[b];
    const long long seg = blockIdx.x;
    const long long g0 = seg * SEGMENT;
    if (g0 >= len) return;                      // block-uniform
    if (!FULL && g0 + SEGMENT >= len) return;   // the row's last segment
    const TI* x = static_cast<const TI*>(a.wav) + (long long)b * a.s_stride;

    // ---- 1. stage
    pw[tid] = tid < 128 ? t.lo[tid] : t.hi[tid - 128];
    if (FULL && tid < WAVES * SLOTS) part[tid] = 0.0;
#pragma clang loop vectorize(disable) unroll_count(4)  // (the loop vectoriser would pair the PCM16 scalings into v_pk_mul_f32: build.py)
    for (int i = 0; i < CHUNK; ++i) {
        const int pos = i * THREADS + tid;
        const long long g = g0 + pos;
        xs[pos + (pos >> 5)] = g < len ? to_float(x[g]) : 0.0f;
    }
    __syncthreads();

    // ---- 2. the lane's chunk from zero state, in place
    float* c = xs + tid * (CHUNK + 1);
    float p[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float pk = 0.0f;
    {
        const float b0 = t.cf[0], b1 = t.cf[1], b2 = t.cf[2], a1 = t.cf[3], a2 = t.cf[4], c1 = t.cf[8], c2 = t.cf[9];
        float s1 = 0.0f, s2 = 0.0f, s3 = 0.0f, s4 = 0.0f;
#pragma unroll 8
        for (int i = 0; i < CHUNK; ++i) {
            const float xi = c[i];
            pk = fmaxf(pk, fabsf(xi));
            const float y1 = fmaf(b0, xi, s1);
            s1 = fmaf(b1, xi, fmaf(-a1, y1, s2));
            s2 = fmaf(b2, xi, -a2 * y1);
            const float z = y1 + s3;
            s3 = fmaf(-c1, z, s4 - 2.0f * y1);
            s4 = fmaf(-c2, z, y1);
            if (FULL) c[i] = z;
        }
        p[0] = s1, p[1] = s2, p[2] = s3 + s4, p[3] = t.kappa * s4;  // carried as q = T s (loudness_design.h)
    }

    // ---- 3. scan: p becomes the end state of lanes 0 .. lane of this wave from a zero incoming state
#pragma unroll
    for (int st = 0; st < 6; ++st) {
        const int d = 1 << st;
        const float* m = st < 3 ? pw + (16 << st) : pw + 128 + (16 << (st - 3));  // A^(CHUNK d)
        float q[4], r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = __shfl_up(p[k], d);
        matvec(m, q, r);
        if (lane >= d) {
#pragma unroll
            for (int k = 0; k < 4; ++k) p[k] += r[k];
        }
    }
    float e[4];  // the lanes before this one
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        e[k] = __shfl_up(p[k], 1);
        if (lane == 0) e[k] = 0.0f;
    }
    if (lane == 63) {
#pragma unroll
        for (int k = 0; k < 4; ++k) wtot[w][k] = p[k];
    }
    __syncthreads();

    float sw[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // the wave's incoming state
    if (FULL) {                               // ... starting from the segment's: the earlier segments' end states, in order
        const float* st = a.state + (long long)b * a.nseg * 4;
        for (long long j = 0; j < seg; ++j) {
            float r[4];
            matvec(t.seg, sw, r);
#pragma unroll
            for (int k = 0; k < 4; ++k) sw[k] = r[k] + st[4 * j + k];
        }
    }
    for (int j = 0; j < w; ++j) {
        float r[4];
        matvec(t.wave, sw, r);
#pragma unroll
        for (int k = 0; k < 4; ++k) sw[k] = r[k] + wtot[j][k];
    }
    if (!FULL) {
        if (tid == THREADS - 1) {  // the last wave's incoming state, through that wave
            float r[4];
            matvec(t.wave, sw, r);
            float* o = a.state + ((long long)b * a.nseg + seg) * 4;
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = r[k] + wtot[WAVES - 1][k];
        }
        return;
    }

    // ---- 4. the lane's incoming state, the full response, hop sums
    float sin_[4];
    {
        float r[4], r2[4];
        matvec(pw + 128 + 16 * (lane >> 3), sw, r);
        matvec(pw + 16 * (lane & 7), r, r2);
#pragma unroll
        for (int k = 0; k < 4; ++k) sin_[k] = e[k] + r2[k];
    }
    const long long cg = g0 + (long long)tid * CHUNK;  // the chunk's first sample
    const long long hop0 = cg / a.H;
    const long long left = (hop0 + 1) * a.H - cg;      // samples of the chunk in hop0 (a chunk meets at most one hop boundary)
    const int bnd = left < CHUNK ? (int)left : CHUNK;
    double acc0 = 0.0, acc1 = 0.0;
#pragma unroll 8
    for (int i = 0; i < CHUNK; ++i) {
        const float z = fmaf(t.htab[4 * i], sin_[0], fmaf(t.htab[4 * i + 1], sin_[1], fmaf(t.htab[4 * i + 2], sin_[2], fmaf(t.htab[4 * i + 3], sin_[3], c[i]))));
        const double zz = (double)z * (double)z;
        if (i < bnd)
            acc0 += zz;
        else
            acc1 += zz;
    }
    const long long wg = g0 + (long long)w * WAVE_SPAN;
    const long long hS = g0 / a.H, hA = wg / a.H, hB = (wg + WAVE_SPAN - 1) / a.H;  // hB - hS <= SLOTS - 1 (loudness_design.h)
    for (long long h = hA; h <= hB; ++h) {                                           // wave-uniform
        const double v = wave_sum((hop0 == h ? acc0 : 0.0) + (hop0 + 1 == h ? acc1 : 0.0));
        if (lane == 0) part[w * SLOTS + (int)(h - hS)] = v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pk = fmaxf(pk, __shfl_xor(pk, o));
    if (lane == 0) pkw[w] = pk;
    __syncthreads();
    if (tid < SLOTS)
        a.partial[((long long)b * a.nseg + seg) * SLOTS + tid] = ((part[tid] + part[SLOTS + tid]) + part[2 * SLOTS + tid]) + part[3 * SLOTS + tid];
    if (tid == 0) a.peak[(long long)b * a.nseg + seg] = fmaxf(fmaxf(pkw[0], pkw[1]), fmaxf(pkw[2], pkw[3]));
}

__device__ __forceinline__ double lufs(double z) { return -0.691 + 10.0 * log10(z); }

__global__ __launch_bounds__(64) void loud_gate_k(const GateArgs a, const LoudLens rows) {
    const int lane = threadIdx.x;
    const int b = blockIdx.x;
    const long long len = rows.len[b];
    const long long H = a.H;
    const long long nH = len / H, J = nH >= 3 ? nH - 3 : 0, nseg = (len + SEGMENT - 1) / SEGMENT;
    const double ninf = -(double)INFINITY;

    float pk = 0.0f;
    for (long long s = lane; s < nseg; s += 64) pk = fmaxf(pk, a.peak[b * a.nseg + s]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pk = fmaxf(pk, __shfl_xor(pk, o));

    double* e = a.hops + b * a.nhop;
    for (long long j = lane; j < nH; j += 64) {  // hop j from the segments it meets, in segment order
        const long long sA = j * H / SEGMENT, sB = ((j + 1) * H - 1) / SEGMENT;
        double acc = 0.0;
        for (long long s = sA; s <= sB; ++s) acc += a.partial[(b * a.nseg + s) * SLOTS + (j - s * SEGMENT / H)];
        e[j] = acc;
    }
    __syncthreads();  // one wave: the hop sums are visible to every lane

    const double d4h = 4.0 * (double)H;
    double sum = 0.0, mx = ninf;
    int cnt = 0;
    for (long long j = lane; j < J; j += 64) {
        const double z = (((e[j] + e[j + 1]) + e[j + 2]) + e[j + 3]) / d4h;
        const double l = lufs(z);
        mx = fmax(mx, l);
        if (l > -70.0) {
            sum += z;
            ++cnt;
        }
        if (a.momentary) a.momentary[b * a.j_stride + j] = (float)l;
    }
    if (a.momentary)
        for (long long j = J + lane; j < a.j_stride; j += 64) a.momentary[b * a.j_stride + j] = -INFINITY;
    sum = wave_sum(sum);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o);
        mx = fmax(mx, __shfl_xor(mx, o));
    }
    const double rel = cnt ? lufs(sum / (double)cnt) - 10.0 : ninf;
    double sum2 = 0.0;
    int cnt2 = 0;
    for (long long j = lane; j < J; j += 64) {
        const double z = (((e[j] + e[j + 1]) + e[j + 2]) + e[j + 3]) / d4h;
        const double l = lufs(z);
        if (l > -70.0 && l > rel) {
            sum2 += z;
            ++cnt2;
        }
    }
    sum2 = wave_sum(sum2);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt2 += __shfl_xor(cnt2, o);
    if (lane == 0) {
        a.integrated[b] = cnt2 ? (float)lufs(sum2 / (double)cnt2) : -INFINITY;
        a.momentary_max[b] = (float)mx;
        a.sample_peak[b] = pk;
        a.n_blocks[b] = (int)J;
        a.n_gated[b] = cnt2;
    }
}

__global__ __launch_bounds__(THREADS) void loud_gain_k(const float* integrated, const float* peak, float target, float ceiling, float max_gain,
                                                        float* gains, int N) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= N) return;
    const float I = integrated[i];
    float g = 1.0f;
    if (I == I && I != -INFINITY) {
        const float g1 = (float)pow(10.0, ((double)target - (double)I) / 20.0);
        const float g2 = (float)pow(10.0, (double)max_gain / 20.0);
        const float g3 = (float)(pow(10.0, (double)ceiling / 20.0) / (double)peak[i]);
        g = fminf(g1, fminf(g2, g3));
    }
    gains[i] = g;
}

template <typename TI, typename TO>
__global__ __launch_bounds__(THREADS) void loud_apply_k(const ApplyArgs a, const LoudRows rows) {
    const int b = blockIdx.y;
    const long long len = rows.len[b];
    const long long cap = a.o_stride ? a.o_stride : len;
    const long long m0 = (long long)blockIdx.x * APPLY_TILE;
    if (m0 >= cap) return;
    const int cnt = (int)min((long long)APPLY_TILE, cap - m0);
    const float g = a.gains[b];
    const TI* x = static_cast<const TI*>(a.wav) + (long long)b * a.s_stride;
    TO* out = static_cast<TO*>(a.out) + rows.off[b];
    for (int i = threadIdx.x; i < cnt; i += THREADS) {
        const long long m = m0 + i;
        out[m] = m < len ? from_float<TO>(to_float(x[m]) * g) : TO(0);
    }
}

}  // namespace

struct vtts_loudness {
    ld::Design d;
    int device = 0;
};

VTTS_API int vtts_loudness_create(const vtts_loudness_cfg* cfg, int device, vtts_loudness** out) {
    if (!cfg || !out) return failf(VTTS_ERR_INVALID, "null argument");
    auto* h = new (std::nothrow) vtts_loudness();
    if (!h) return failf(VTTS_ERR_NOMEM, "host allocation failed");
    char why[160];
    if (ld::design(cfg->sample_rate, h->d, why) != 0) {
        delete h;
        return failf(VTTS_ERR_INVALID, "%s", why);
    }
    h->device = device;
    *out = h;
    return VTTS_OK;
}

VTTS_API void vtts_loudness_destroy(vtts_loudness* h) { delete h; }

VTTS_API int vtts_loudness_coefficients(const vtts_loudness* h, double* host_out) {
    if (!h || !host_out) return failf(VTTS_ERR_INVALID, "null argument");
    for (int i = 0; i < 10; ++i) host_out[i] = h->d.coef[i];
    return VTTS_OK;
}

VTTS_API int vtts_loudness_num_blocks(const vtts_loudness* h, int64_t n_samples, int64_t* blocks) {
    if (!h || !blocks) return failf(VTTS_ERR_INVALID, "null argument");
    if (n_samples < 0 || n_samples > 0x7fffffff) return failf(VTTS_ERR_SHAPE, "n_samples must be in 0 .. 2^31 - 1 (got %lld)", (long long)n_samples);
    *blocks = ld::num_blocks(h->d, n_samples);
    return VTTS_OK;
}

VTTS_API int vtts_loudness_workspace_bytes(const vtts_loudness* h, int N, int64_t S, size_t* bytes) {
    if (!h || !bytes) return failf(VTTS_ERR_INVALID, "null argument");
    if (N <= 0) return failf(VTTS_ERR_INVALID, "N must be positive (got %d)", N);
    if (S < 0 || S > 0x7fffffff - SEGMENT) return failf(VTTS_ERR_SHAPE, "S must be in 0 .. 2^31 - 1 - %d (got %lld)", SEGMENT, (long long)S);
    *bytes = ld::layout(h->d, N, S).bytes;
    return VTTS_OK;
}

VTTS_API int vtts_loudness_measure(vtts_loudness* h, const void* wav_dev, int dtype, int N, int64_t S_stride, const int32_t* lengths,
                                   float* integrated_dev, float* momentary_max_dev, float* sample_peak_dev, int32_t* n_blocks_dev, int32_t* n_gated_dev,
                                   float* momentary_dev, int64_t J_stride, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h || !integrated_dev || !momentary_max_dev || !sample_peak_dev || !n_blocks_dev || !n_gated_dev || !workspace)
        return failf(VTTS_ERR_INVALID, "null argument");
    int64_t longest = 0;
    if (int rc = check_rows("measure", wav_dev, dtype, N, S_stride, lengths, SEGMENT, &longest)) return rc;
    if (momentary_dev && J_stride < ld::num_blocks(h->d, longest))
        return failf(VTTS_ERR_SHAPE, "J_stride = %lld is below the longest row's %lld blocks", (long long)J_stride, (long long)ld::num_blocks(h->d, longest));
    const ld::Layout l = ld::layout(h->d, N, longest);
    if (workspace_bytes < l.bytes) return failf(VTTS_ERR_NOMEM, "workspace too small: %zu < %zu bytes", workspace_bytes, l.bytes);
    if (reinterpret_cast<uintptr_t>(workspace) % 8) return failf(VTTS_ERR_INVALID, "workspace must be 8-byte aligned");

    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool pcm = dtype == VTTS_AUDIO_PCM16;
    const size_t esz = pcm ? 2 : 4;
    char* ws = static_cast<char*>(workspace);
    const unsigned nseg = (unsigned)ld::num_segments(longest);
    return vtts_rows::for_each_launch<ROWS_PER_LAUNCH>(N, lengths, S_stride, [&](int r0, int nr, const LoudLens& rows) -> int {
        ScanArgs a;
        a.wav = static_cast<const char*>(wav_dev) + (size_t)r0 * S_stride * esz;
        a.s_stride = S_stride;
        a.nseg = l.nseg;
        a.partial = reinterpret_cast<double*>(ws + l.partial) + (size_t)r0 * l.nseg * SLOTS;
        a.state = reinterpret_cast<float*>(ws + l.state) + (size_t)r0 * l.nseg * 4;
        a.peak = reinterpret_cast<float*>(ws + l.peak) + (size_t)r0 * l.nseg;
        a.H = h->d.H;
        if (nseg > 1) {
            const dim3 grid(nseg - 1, (unsigned)nr);
            if (pcm)
                hipLaunchKernelGGL((loud_scan_k<short, false>), grid, dim3(THREADS), 0, s, a, h->d.t, rows);
            else
                hipLaunchKernelGGL((loud_scan_k<float, false>), grid, dim3(THREADS), 0, s, a, h->d.t, rows);
        }
        if (nseg > 0) {
            const dim3 grid(nseg, (unsigned)nr);
            if (pcm)
                hipLaunchKernelGGL((loud_scan_k<short, true>), grid, dim3(THREADS), 0, s, a, h->d.t, rows);
            else
                hipLaunchKernelGGL((loud_scan_k<float, true>), grid, dim3(THREADS), 0, s, a, h->d.t, rows);
        }
        GateArgs g;
        g.nseg = l.nseg;
        g.nhop = l.nhop;
        g.partial = a.partial;
        g.hops = reinterpret_cast<double*>(ws + l.hops) + (size_t)r0 * l.nhop;
        g.peak = a.peak;
        g.integrated = integrated_dev + r0;
        g.momentary_max = momentary_max_dev + r0;
        g.sample_peak = sample_peak_dev + r0;
        g.n_blocks = n_blocks_dev + r0;
        g.n_gated = n_gated_dev + r0;
        g.momentary = momentary_dev ? momentary_dev + (size_t)r0 * J_stride : nullptr;
        g.j_stride = J_stride;
        g.H = h->d.H;
        hipLaunchKernelGGL(loud_gate_k, dim3((unsigned)nr), dim3(64), 0, s, g, rows);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return failf(VTTS_ERR_HIP, "loudness kernel launch failed: %s", hipGetErrorString(e));
        return VTTS_OK;
    });
}

VTTS_API int vtts_loudness_normalize(vtts_loudness* h, const void* wav_dev, int dtype, int N, int64_t S_stride, const int32_t* lengths,
                                     const float* integrated_dev, const float* sample_peak_dev, float target_lufs, float ceiling_dbfs, float max_gain_db,
                                     void* out_dev, int out_dtype, int64_t O_stride, float* gains_dev, void* stream) {
    if (!h || !integrated_dev || !sample_peak_dev || !out_dev || !gains_dev) return failf(VTTS_ERR_INVALID, "null argument");
    if (out_dtype != VTTS_AUDIO_F32 && out_dtype != VTTS_AUDIO_PCM16)
        return failf(VTTS_ERR_INVALID, "normalize: out_dtype must be VTTS_AUDIO_F32 or VTTS_AUDIO_PCM16 (got %d)", out_dtype);
    int64_t longest = 0;
    if (int rc = check_rows("normalize", wav_dev, dtype, N, S_stride, lengths, SEGMENT, &longest)) return rc;
    if (!std::isfinite(target_lufs) || !std::isfinite(ceiling_dbfs) || !std::isfinite(max_gain_db))
        return failf(VTTS_ERR_INVALID, "normalize: target_lufs, ceiling_dbfs and max_gain_db must be finite (got %g, %g, %g)", target_lufs, ceiling_dbfs, max_gain_db);
    if (O_stride < 0 || (O_stride > 0 && O_stride < longest))
        return failf(VTTS_ERR_SHAPE, "O_stride = %lld is below the longest row's %lld samples", (long long)O_stride, (long long)longest);

    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(loud_gain_k, dim3((unsigned)((N + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, integrated_dev, sample_peak_dev, target_lufs, ceiling_dbfs,
                       max_gain_db, gains_dev, N);
    const bool pin = dtype == VTTS_AUDIO_PCM16, pout = out_dtype == VTTS_AUDIO_PCM16;
    const size_t esz = pin ? 2 : 4;
    const int64_t cover = O_stride ? O_stride : longest;
    const unsigned tiles = (unsigned)((cover + APPLY_TILE - 1) / APPLY_TILE);
    vtts_rows::for_each_launch_off<ROWS_PER_LAUNCH>(N, lengths, S_stride, O_stride, [&](int r0, int nr, const LoudRows& rows) -> int {
        if (tiles == 0) return VTTS_OK;  // packed, and every row is empty
        ApplyArgs a;
        a.wav = static_cast<const char*>(wav_dev) + (size_t)r0 * S_stride * esz;
        a.out = out_dev;
        a.gains = gains_dev + r0;
        a.s_stride = S_stride;
        a.o_stride = O_stride;
        const dim3 grid(tiles, (unsigned)nr);
        if (pin) {
            if (pout)
                hipLaunchKernelGGL((loud_apply_k<short, short>), grid, dim3(THREADS), 0, s, a, rows);
            else
                hipLaunchKernelGGL((loud_apply_k<short, float>), grid, dim3(THREADS), 0, s, a, rows);
        } else {
            if (pout)
                hipLaunchKernelGGL((loud_apply_k<float, short>), grid, dim3(THREADS), 0, s, a, rows);
            else
                hipLaunchKernelGGL((loud_apply_k<float, float>), grid, dim3(THREADS), 0, s, a, rows);
        }
        return VTTS_OK;
    });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return failf(VTTS_ERR_HIP, "loudness kernel launch failed: %s", hipGetErrorString(e));
    return VTTS_OK;
}
