// The intelligibility meter (include/vtts_stoi.h): STOI and ESTOI of a processed waveform against the clean one, batched and ragged.
//
// Five launches per 128 rows, each anchored at the row's own first sample:
//
//   stoi_energy_k    workgroup = VTTS_STOI_FRAMES_PER_BLOCK (8) candidate frames of the CLEAN row, one wave per frame, from one staged span of
//                    (8 + 1) * 128 samples: the 2x overlap of the frames is served from LDS.  e_k in fp64 in the header's order.
//   stoi_keep_k      one workgroup per row: the largest e_k, the keep mask e_k > 1e-4 e_max, and an exclusive scan (ballot + popcount per wave,
//                    the four waves' counts through LDS, a running base) into the kept list.
//   stoi_spectra_k   workgroup = 8 analysis frames, one wave per frame, x then y.  A frame gathers its three kept candidate frames straight
//                    from the row (the overlap-added signal is never written; both signals' loads are issued first), and runs the zero-padded 512-point transform that mel.hip
//                    runs (stockham.h: fft512_888): 64 lanes x 8 points, three radix-8 passes in registers, two exchanges through the wave's
//                    own padded LDS buffer behind compiler-only wave fences.  x and y are NOT packed as the real and imaginary parts of one transform: that
//                    would tie y's absolute error to x's magnitude, and a resynthesis 40 dB below its input would lose 40 dB of precision.
//                    Bins 7 .. 218 become 15 band magnitudes: 60 B per frame and signal.
//   stoi_segments_k  workgroup = 16 consecutive segments from one staged tile of 45 frames' magnitudes; fp64.  One lane per (segment, band),
//                    then one lane per (segment, frame), then one per segment: every sum is sequential in a lane, nothing is shuffled.
//                    (A first version held a frame per lane and summed along the bands' rows by butterflies of fp64 shuffles, with every
//                    lane redoing the row's square roots and divisions: 1.23 ms of the 1.43 ms the meter took on 64 x 163 840 samples.)
//   stoi_mean_k      one wave per row: the fixed-order means, the NaN of a row without a segment, and the NaN tails of the series.
//
// The tables (the window and a quarter turn of twiddles: 512 floats, computed in double on the host) and the rows' lengths travel as kernel
// arguments.  Passes over HBM: x once for the energies, x and y once for the spectra (the frames' 4x overlap is served by the L2).
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>

#include "../../include/vtts_audio.h"
#include "../../include/vtts_hifigan.h"
#include "../../include/vtts_stoi.h"
#include "launch_rows.h"
#include "sample_convert.h"
#include "vtts_internal.h"

// include/vtts_stoi.h states single rounded fp32 products (p = fl32(x w)) that the keep mask is compared on with ==: no a * b + c of this
// file may become an FMA.
#pragma clang fp contract(off)

#include "stockham.h"

using vtts::failf;
using vtts_sample::to_float;
using namespace vtts_stockham;

namespace {

constexpr int FRAME = VTTS_STOI_FRAME, HOP = VTTS_STOI_HOP, NFFT = 512, BANDS = VTTS_STOI_BANDS, SEG = VTTS_STOI_SEG;
constexpr int FPB = VTTS_STOI_FRAMES_PER_BLOCK;
constexpr int THREADS = 64 * FPB;
constexpr int SPAN = (FPB + 1) * HOP;   // samples the FPB candidate frames of a workgroup cover
constexpr int ROWS_PER_LAUNCH = 128;
constexpr int SEG_THREADS = 256, SEGS_PER_BLOCK = SEG_THREADS / 16;  // 16 lanes per segment in phase 1: 15 bands and an idle one
constexpr int TILE_FRAMES = SEGS_PER_BLOCK + SEG - 1;                 // frames the segments of a workgroup cover
constexpr int TILE_ROW = TILE_FRAMES + 2;
constexpr int KEEP_THREADS = 256;
static_assert(FRAME == 2 * HOP && NFFT == 2 * FRAME && FRAME == 4 * 64, "a lane holds four samples of a frame");

__constant__ int BAND_LO[BANDS + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

struct StoiTables {
    float win[FRAME];   // w[r]
    float tw[FRAME];    // exp(-2 pi i j / 512), j = 0 .. 127, as (re, im) pairs
};

using Rows = vtts_rows::Lens<ROWS_PER_LAUNCH>;  // samples of each row of this launch

struct StoiArgs {               // every pointer at the launch's first row
    const void* x;              // clean
    const void* y;              // processed
    long long s_stride;         // samples between rows
    long long k_stride;         // candidate frames between rows of energy / kept
    long long t_stride;         // frames between the band rows of mags: [rows][2][15][t_stride]
    long long m_stride;         // segments between rows of dseg: [rows][2][m_stride]
    long long series_stride;    // ... and of the two series
    double* energy;
    int* kept;
    float* mags;
    double* dseg;
    float* stoi;
    float* estoi;
    int* n_frames;
    int* n_kept;
    int* n_segments;
    float* stoi_series;         // NULL, or [rows][series_stride]
    float* estoi_series;
    double clip;                // 1 + 10^(15 / 20)
};

__host__ __device__ __forceinline__ long long num_frames(long long S) { return S > FRAME ? (S - FRAME + HOP - 1) / HOP : 0; }

// ---- A. candidate frame energies of the clean row ----------------------------------------------------------------------------------
template <typename TI>
__global__ __launch_bounds__(THREADS) void stoi_energy_k(const StoiArgs a, const StoiTables t, const Rows rows) {
    __shared__ float span[SPAN];
    __shared__ float win[FRAME];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    const long long len = rows.len[b];
    const long long K = num_frames(len);
    const long long k0 = (long long)blockIdx.x * FPB;
    if (k0 >= K) return;  // block-uniform
    const TI* x = static_cast<const TI*>(a.x) + (long long)b * a.s_stride;
    if (tid < FRAME) win[tid] = t.win[tid];
    for (int i = tid; i < SPAN; i += THREADS) {
        const long long g = k0 * HOP + i;
        span[i] = g < len ? to_float(x[g]) : 0.0f;
    }
    __syncthreads();
    const long long k = k0 + wave;
    if (k >= K) return;
    const float* f = span + wave * HOP;
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float p = f[lane + 64 * q] * win[lane + 64 * q];
        s += (double)p * (double)p;
    }
    s = wave_sum(s);
    if (lane == 0) a.energy[(long long)b * a.k_stride + k] = s;
}

// ---- A. the keep mask and the kept list ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KEEP_THREADS) void stoi_keep_k(const StoiArgs a, const Rows rows) {
    __shared__ double wmax[KEEP_THREADS / 64];
    __shared__ int wcnt[KEEP_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b = blockIdx.x;
    const long long K = num_frames(rows.len[b]);
    const double* e = a.energy + (long long)b * a.k_stride;
    int* kept = a.kept + (long long)b * a.k_stride;

    double mx = 0.0;
    for (long long k = tid; k < K; k += KEEP_THREADS) mx = fmax(mx, e[k]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
    if (lane == 0) wmax[w] = mx;
    __syncthreads();
    mx = fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3]));
    const double thr = 1e-4 * mx;

    long long run = 0;  // kept frames before this round's
    for (long long base = 0; base < K; base += KEEP_THREADS) {  // block-uniform trip count
        const long long k = base + tid;
        const bool keep = k < K && e[k] > thr;
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wcnt[w] = __popcll(m);
        __syncthreads();
        long long off = run;
        for (int j = 0; j < w; ++j) off += wcnt[j];
        if (keep) kept[off + __popcll(m & ((1ull << lane) - 1ull))] = (int)k;
        run += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
    for (long long j = run + tid; j < a.k_stride; j += KEEP_THREADS) kept[j] = -1;
    if (tid == 0) {
        a.n_frames[b] = (int)K;
        a.n_kept[b] = (int)run;
    }
}

// ---- B. band magnitudes of the analysis frames --------------------------------------------------------------------------------------
template <typename TI>
__global__ __launch_bounds__(THREADS) void stoi_spectra_k(const StoiArgs a, const StoiTables t) {
    __shared__ float2 xbuf[FPB * XBUF];
    __shared__ float2 tw[NFFT];
    __shared__ float win[FRAME];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    const int Kk = a.n_kept[b];
    const long long T = Kk > 0 ? Kk - 1 : 0;
    const long long t0 = (long long)blockIdx.x * FPB;
    if (t0 >= T) return;  // block-uniform

    for (int j = tid; j < NFFT; j += THREADS) {  // the full turn from its first quarter: W^(i + 128 q) = W^i (-i)^q
        const int i = j & 127, q = j >> 7;
        const float c = t.tw[2 * i], s = t.tw[2 * i + 1];
        tw[j] = q == 0 ? make_float2(c, s) : q == 1 ? make_float2(s, -c) : q == 2 ? make_float2(-c, -s) : make_float2(-s, c);
    }
    if (tid < FRAME) win[tid] = t.win[tid];
    __syncthreads();

    // From here on a wave touches only its own exchange buffer.
    const long long tt = t0 + wave;
    if (tt >= T) return;
    const int* kept = a.kept + (long long)b * a.k_stride;
    const long long oc = (long long)kept[tt] * HOP, on = (long long)kept[tt + 1] * HOP;  // tt + 1 <= Kk - 1
    const long long op = tt > 0 ? (long long)kept[tt - 1] * HOP : -1;
    float2* xb = xbuf + wave * XBUF;

    // both signals' samples are requested before either transform runs: the second's latency hides behind the first's arithmetic
    float vin[2][4];
#pragma unroll
    for (int sig = 0; sig < 2; ++sig) {
        const TI* x = static_cast<const TI*>(sig ? a.y : a.x) + (long long)b * a.s_stride;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = lane + 64 * q;
            float u = to_float(x[oc + r]) * win[r];
            if (q < 2) {
                if (op >= 0) u += to_float(x[op + r + HOP]) * win[r + HOP];
            } else {
                u += to_float(x[on + r - HOP]) * win[r - HOP];
            }
            vin[sig][q] = u * win[r];
        }
    }

#pragma unroll
    for (int sig = 0; sig < 2; ++sig) {
        float2 v[8];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = make_float2(vin[sig][q], 0.0f);
#pragma unroll
        for (int q = 4; q < 8; ++q) v[q] = make_float2(0.0f, 0.0f);  // the zero padding to 512

        fft512_888<4>(v, xb, tw, lane, [&](int k0) { return tw[lane * k0]; });  // bins below 256 only

        float pw[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float2 z = xb[lane + 64 * i];
            pw[i] = z.x * z.x + z.y * z.y;
        }
        wave_sync();
        float* pb = reinterpret_cast<float*>(xb);  // the powers, over the wave's exchange buffer
#pragma unroll
        for (int i = 0; i < 4; ++i) pb[lane + 64 * i] = pw[i];
        wave_sync();
        if (lane < BANDS) {
            double acc = 0.0;
            for (int f = BAND_LO[lane]; f < BAND_LO[lane + 1]; ++f) acc += (double)pb[f];
            a.mags[(((long long)b * 2 + sig) * BANDS + lane) * a.t_stride + tt] = (float)sqrt(acc);
        }
        wave_sync();
    }
}

// ---- C. the segments ----------------------------------------------------------------------------------------------------------------
// One workgroup per SEGS_PER_BLOCK consecutive segments of one row: their 45 frames' magnitudes are staged once.  Phase 1, one lane per
// (segment, band): the band's STOI term and the row normalisation's mean and divisor, every sum sequential over the 30 frames.  Phase 2, one
// lane per (segment, frame): the frame's column of row-normalised values over the 15 bands, normalised again and correlated in the lane.
// Phase 3, one lane per segment: the 15 band terms and the 30 column terms in ascending order.
__global__ __launch_bounds__(SEG_THREADS) void stoi_segments_k(const StoiArgs a) {
    __shared__ float tile[2][BANDS][TILE_ROW];
    __shared__ double stat[SEGS_PER_BLOCK][BANDS][4];  // mean and divisor of X's row, then of Y's
    __shared__ double term[SEGS_PER_BLOCK][BANDS];
    __shared__ double cdot[SEGS_PER_BLOCK][SEG];
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const int Kk = a.n_kept[b];
    const long long T = Kk > 0 ? Kk - 1 : 0, M = T > SEG - 1 ? T - (SEG - 1) : 0;
    const long long m0 = (long long)blockIdx.x * SEGS_PER_BLOCK;
    if (m0 >= M) return;  // block-uniform
    const int nseg = M - m0 < SEGS_PER_BLOCK ? (int)(M - m0) : SEGS_PER_BLOCK;
    const int nfr = nseg + SEG - 1;  // frames m0 .. m0 + nfr - 1 <= T - 1
    const double EPS = 2.220446049250313e-16;  // 2^-52
    const float* mags = a.mags + (long long)b * 2 * BANDS * a.t_stride + m0;
    for (int i = tid; i < 2 * BANDS * TILE_FRAMES; i += SEG_THREADS) {
        const int row = i / TILE_FRAMES, f = i - row * TILE_FRAMES;
        (&tile[0][0][0])[row * TILE_ROW + f] = f < nfr ? mags[(long long)row * a.t_stride + f] : 0.0f;
    }
    __syncthreads();

    {
        const int s = tid >> 4, j = tid & 15;
        if (j < BANDS && s < nseg) {
            const float* xp = &tile[0][j][s];
            const float* yp = &tile[1][j][s];
            double sx = 0.0, sy = 0.0, qx = 0.0, qy = 0.0;
#pragma unroll 2
            for (int n = 0; n < SEG; ++n) {
                const double x = xp[n], y = yp[n];
                sx += x, sy += y, qx += x * x, qy += y * y;
            }
            const double alpha = sqrt(qx) / (sqrt(qy) + EPS);
            double sp = 0.0;
#pragma unroll 2
            for (int n = 0; n < SEG; ++n) sp += fmin(alpha * (double)yp[n], a.clip * (double)xp[n]);
            const double mx = sx / SEG, my = sy / SEG, mp = sp / SEG;
            double cxx = 0.0, cyy = 0.0, cpp = 0.0, cxp = 0.0;
#pragma unroll 2
            for (int n = 0; n < SEG; ++n) {
                const double x = xp[n], y = yp[n];
                const double xc = x - mx, yc = y - my, pc = fmin(alpha * y, a.clip * x) - mp;
                cxx += xc * xc, cyy += yc * yc, cpp += pc * pc, cxp += xc * pc;
            }
            const double dx = sqrt(cxx) + EPS, dy = sqrt(cyy) + EPS, dp = sqrt(cpp) + EPS;
            term[s][j] = cxp / (dx * dp);
            stat[s][j][0] = mx, stat[s][j][1] = dx, stat[s][j][2] = my, stat[s][j][3] = dy;
        }
    }
    __syncthreads();

    for (int c = tid; c < nseg * SEG; c += SEG_THREADS) {
        const int s = c / SEG, n = c - s * SEG;
        double xr[BANDS], yr[BANDS], sx = 0.0, sy = 0.0;
#pragma unroll
        for (int j = 0; j < BANDS; ++j) {
            xr[j] = ((double)tile[0][j][s + n] - stat[s][j][0]) / stat[s][j][1];
            yr[j] = ((double)tile[1][j][s + n] - stat[s][j][2]) / stat[s][j][3];
            sx += xr[j], sy += yr[j];
        }
        const double cx = sx / BANDS, cy = sy / BANDS;
        double qx = 0.0, qy = 0.0, qxy = 0.0;
#pragma unroll
        for (int j = 0; j < BANDS; ++j) {
            const double u = xr[j] - cx, v = yr[j] - cy;
            qx += u * u, qy += v * v, qxy += u * v;
        }
        cdot[s][n] = qxy / ((sqrt(qx) + EPS) * (sqrt(qy) + EPS));
    }
    __syncthreads();

    if (tid < nseg) {
        double ds = 0.0, de = 0.0;
        for (int j = 0; j < BANDS; ++j) ds += term[tid][j];
        for (int n = 0; n < SEG; ++n) de += cdot[tid][n];
        const double d_stoi = ds / BANDS, d_estoi = de / SEG;
        const long long m = m0 + tid;
        double* d = a.dseg + (long long)b * 2 * a.m_stride;
        d[m] = d_stoi;
        d[a.m_stride + m] = d_estoi;
        if (a.stoi_series) {
            a.stoi_series[(long long)b * a.series_stride + m] = (float)d_stoi;
            a.estoi_series[(long long)b * a.series_stride + m] = (float)d_estoi;
        }
    }
}

// ---- the means ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void stoi_mean_k(const StoiArgs a) {
    const int lane = threadIdx.x;
    const int b = blockIdx.x;
    const int Kk = a.n_kept[b];
    const long long T = Kk > 0 ? Kk - 1 : 0, M = T > SEG - 1 ? T - (SEG - 1) : 0;
    const double* d = a.dseg + (long long)b * 2 * a.m_stride;
    double s0 = 0.0, s1 = 0.0;
    for (long long m = lane; m < M; m += 64) s0 += d[m], s1 += d[a.m_stride + m];
    s0 = wave_sum(s0), s1 = wave_sum(s1);
    const float nan = __builtin_nanf("");
    if (lane == 0) {
        a.stoi[b] = M ? (float)(s0 / (double)M) : nan;
        a.estoi[b] = M ? (float)(s1 / (double)M) : nan;
        a.n_segments[b] = (int)M;
    }
    if (a.stoi_series)
        for (long long m = M + lane; m < a.series_stride; m += 64)
            a.stoi_series[(long long)b * a.series_stride + m] = a.estoi_series[(long long)b * a.series_stride + m] = nan;
}

struct Layout {
    long long kmax, tmax, mmax;
    size_t kept, energy, dseg, mags, bytes;
};

Layout layout(int N, int64_t S) {
    Layout l;
    l.kmax = num_frames(S);
    l.tmax = l.kmax > 0 ? l.kmax - 1 : 0;
    l.mmax = l.tmax > SEG - 1 ? l.tmax - (SEG - 1) : 0;
    size_t o = 0;
    l.kept = o, o += vtts::align_up((size_t)N * l.kmax * sizeof(int), 8);
    l.energy = o, o += (size_t)N * l.kmax * sizeof(double);
    l.dseg = o, o += (size_t)N * 2 * l.mmax * sizeof(double);
    l.mags = o, o += vtts::align_up((size_t)N * 2 * BANDS * l.tmax * sizeof(float), 8);
    l.bytes = o > 8 ? o : 8;
    return l;
}

}  // namespace

struct vtts_stoi {
    StoiTables t;
    double clip = 0.0;
    int device = 0;
};

VTTS_API int vtts_stoi_create(int device, vtts_stoi** out) {
    if (!out) return failf(VTTS_ERR_INVALID, "null argument");
    auto* h = new (std::nothrow) vtts_stoi();
    if (!h) return failf(VTTS_ERR_NOMEM, "host allocation failed");
    const double pi = 3.14159265358979323846;
    for (int r = 0; r < FRAME; ++r) h->t.win[r] = (float)(0.5 - 0.5 * std::cos(2.0 * pi * (r + 1) / (FRAME + 1)));
    for (int j = 0; j < 128; ++j) {
        h->t.tw[2 * j] = (float)std::cos(2.0 * pi * j / NFFT);
        h->t.tw[2 * j + 1] = (float)-std::sin(2.0 * pi * j / NFFT);
    }
    h->clip = 1.0 + std::pow(10.0, 15.0 / 20.0);
    h->device = device;
    *out = h;
    return VTTS_OK;
}

VTTS_API void vtts_stoi_destroy(vtts_stoi* h) { delete h; }

VTTS_API int vtts_stoi_window(const vtts_stoi* h, float* host_out) {
    if (!h || !host_out) return failf(VTTS_ERR_INVALID, "null argument");
    memcpy(host_out, h->t.win, sizeof(h->t.win));
    return VTTS_OK;
}

VTTS_API int vtts_stoi_num_frames(const vtts_stoi* h, int64_t n_samples, int64_t* frames) {
    if (!h || !frames) return failf(VTTS_ERR_INVALID, "null argument");
    if (n_samples < 0 || n_samples > VTTS_STOI_MAX_SAMPLES)
        return failf(VTTS_ERR_SHAPE, "n_samples must be in 0 .. %d (got %lld)", VTTS_STOI_MAX_SAMPLES, (long long)n_samples);
    *frames = num_frames(n_samples);
    return VTTS_OK;
}

VTTS_API int vtts_stoi_workspace_bytes(const vtts_stoi* h, int N, int64_t S, size_t* bytes) {
    if (!h || !bytes) return failf(VTTS_ERR_INVALID, "null argument");
    if (N <= 0) return failf(VTTS_ERR_INVALID, "N must be positive (got %d)", N);
    if (S < 0 || S > VTTS_STOI_MAX_SAMPLES) return failf(VTTS_ERR_SHAPE, "S must be in 0 .. %d (got %lld)", VTTS_STOI_MAX_SAMPLES, (long long)S);
    *bytes = layout(N, S).bytes;
    return VTTS_OK;
}

VTTS_API int vtts_stoi_forward(vtts_stoi* h, const void* clean_dev, const void* processed_dev, int dtype, int N, int64_t S_stride,
                               const int32_t* lengths, float* stoi_dev, float* estoi_dev, int32_t* n_frames_dev, int32_t* n_kept_dev,
                               int32_t* n_segments_dev, float* stoi_series_dev, float* estoi_series_dev, int64_t M_stride, float* mags_dev,
                               int64_t T_stride, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h || !clean_dev || !processed_dev || !stoi_dev || !estoi_dev || !n_frames_dev || !n_kept_dev || !n_segments_dev || !workspace)
        return failf(VTTS_ERR_INVALID, "null argument");
    if (dtype != VTTS_AUDIO_F32 && dtype != VTTS_AUDIO_PCM16) return failf(VTTS_ERR_INVALID, "dtype must be VTTS_AUDIO_F32 or VTTS_AUDIO_PCM16 (got %d)", dtype);
    if (N <= 0) return failf(VTTS_ERR_INVALID, "N must be positive (got %d)", N);
    if (S_stride < 0 || S_stride > 0x7fffffff) return failf(VTTS_ERR_SHAPE, "S_stride must be in 0 .. 2^31 - 1 (got %lld)", (long long)S_stride);
    if ((stoi_series_dev == nullptr) != (estoi_series_dev == nullptr)) return failf(VTTS_ERR_INVALID, "give both series or neither");
    int64_t longest = 0;
    for (int b = 0; b < N; ++b) {
        const int64_t len = lengths ? lengths[b] : S_stride;
        if (len < 0 || len > S_stride || len > VTTS_STOI_MAX_SAMPLES)
            return failf(VTTS_ERR_SHAPE, "lengths[%d] = %lld is outside 0 .. min(S_stride = %lld, %d)", b, (long long)len, (long long)S_stride, VTTS_STOI_MAX_SAMPLES);
        if (len > longest) longest = len;
    }
    const Layout l = layout(N, longest);
    if (stoi_series_dev && M_stride < l.mmax)
        return failf(VTTS_ERR_SHAPE, "M_stride = %lld is below the longest row's %lld possible segments", (long long)M_stride, l.mmax);
    if (mags_dev && T_stride < l.tmax)
        return failf(VTTS_ERR_SHAPE, "T_stride = %lld is below the longest row's %lld possible frames", (long long)T_stride, l.tmax);
    if (workspace_bytes < l.bytes) return failf(VTTS_ERR_NOMEM, "workspace too small: %zu < %zu bytes", workspace_bytes, l.bytes);
    if (reinterpret_cast<uintptr_t>(workspace) % 8) return failf(VTTS_ERR_INVALID, "workspace must be 8-byte aligned");

    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool pcm = dtype == VTTS_AUDIO_PCM16;
    const size_t esz = pcm ? 2 : 4;
    char* ws = static_cast<char*>(workspace);
    const long long t_stride = mags_dev ? T_stride : l.tmax;
    float* mags = mags_dev ? mags_dev : reinterpret_cast<float*>(ws + l.mags);
    return vtts_rows::for_each_launch<ROWS_PER_LAUNCH>(N, lengths, S_stride, [&](int r0, int nr, const Rows& rows) -> int {
        StoiArgs a;
        a.x = static_cast<const char*>(clean_dev) + (size_t)r0 * S_stride * esz;
        a.y = static_cast<const char*>(processed_dev) + (size_t)r0 * S_stride * esz;
        a.s_stride = S_stride;
        a.k_stride = l.kmax;
        a.t_stride = t_stride;
        a.m_stride = l.mmax;
        a.series_stride = M_stride;
        a.kept = reinterpret_cast<int*>(ws + l.kept) + (size_t)r0 * l.kmax;
        a.energy = reinterpret_cast<double*>(ws + l.energy) + (size_t)r0 * l.kmax;
        a.dseg = reinterpret_cast<double*>(ws + l.dseg) + (size_t)r0 * 2 * l.mmax;
        a.mags = mags + (size_t)r0 * 2 * BANDS * t_stride;
        a.stoi = stoi_dev + r0;
        a.estoi = estoi_dev + r0;
        a.n_frames = n_frames_dev + r0;
        a.n_kept = n_kept_dev + r0;
        a.n_segments = n_segments_dev + r0;
        a.stoi_series = stoi_series_dev ? stoi_series_dev + (size_t)r0 * M_stride : nullptr;
        a.estoi_series = estoi_series_dev ? estoi_series_dev + (size_t)r0 * M_stride : nullptr;
        a.clip = h->clip;
        const unsigned ktiles = (unsigned)((l.kmax + FPB - 1) / FPB), ttiles = (unsigned)((l.tmax + FPB - 1) / FPB);
        const unsigned mtiles = (unsigned)((l.mmax + SEGS_PER_BLOCK - 1) / SEGS_PER_BLOCK);
        if (ktiles) {
            if (pcm)
                hipLaunchKernelGGL(stoi_energy_k<short>, dim3(ktiles, (unsigned)nr), dim3(THREADS), 0, s, a, h->t, rows);
            else
                hipLaunchKernelGGL(stoi_energy_k<float>, dim3(ktiles, (unsigned)nr), dim3(THREADS), 0, s, a, h->t, rows);
        }
        hipLaunchKernelGGL(stoi_keep_k, dim3((unsigned)nr), dim3(KEEP_THREADS), 0, s, a, rows);
        if (ttiles) {
            if (pcm)
                hipLaunchKernelGGL(stoi_spectra_k<short>, dim3(ttiles, (unsigned)nr), dim3(THREADS), 0, s, a, h->t);
            else
                hipLaunchKernelGGL(stoi_spectra_k<float>, dim3(ttiles, (unsigned)nr), dim3(THREADS), 0, s, a, h->t);
        }
        if (mtiles) hipLaunchKernelGGL(stoi_segments_k, dim3(mtiles, (unsigned)nr), dim3(SEG_THREADS), 0, s, a);
        hipLaunchKernelGGL(stoi_mean_k, dim3((unsigned)nr), dim3(64), 0, s, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return failf(VTTS_ERR_HIP, "stoi kernel launch failed: %s", hipGetErrorString(e));
        return VTTS_OK;
    });
}
