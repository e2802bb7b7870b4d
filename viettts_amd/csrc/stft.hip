// The complex short-time Fourier transform in both directions and Griffin-Lim's projection step (include/vtts_stft.h); batched and ragged.
//
//   stft_forward_k<NFFT, TI, PROJ>  workgroup = F consecutive frames of one row, one wave per frame (spectral.hip's shape for one signal):
//     1. stage the (F - 1) hop + NFFT samples the frames cover into LDS, reflected at the ROW'S OWN ends;
//     2. per wave: the windowed frame as H = NFFT / 2 complex points through stockham.h's forward transform in its own exchange buffer;
//     3. the split step to bins 0 .. H (a lane pairs bin k with bin H - k), stored as they are (PROJ = false) or through the projection
//        c -> mag a / (|a| + 1e-16), a = c - alpha tprev, with tprev <- c (PROJ = true): one spectrum written per iteration.
//   stft_inverse_k<NFFT, TO>        workgroup = RUN consecutive output samples of one row, W waves; thread i owns samples i, i + 64 W, ...
//     and keeps their overlap-add sum y and envelope e in registers.  The frames whose window covers the run are walked in ascending t,
//     W per round:
//     1. each wave builds Z from its frame's bins (the inverse split step) in its own exchange buffer and inverse-transforms it there;
//     2. after a workgroup barrier every thread adds the round's frames to its samples in ascending t (y += v w, e += w w, each rounded);
//     3. a second barrier frees the buffers for the next round.
//     At the end out = (y / e) / NFFT.  A sample's sums run over the same frames in the same order whichever workgroup owns it, so no result
//     depends on RUN or W.  Reads of v for consecutive samples are consecutive LDS dwords (a pad dword pair after every 16).  The blocking, the
//     inverse split step and the add-to-samples loop live in stft_back.h, shared with denoise.hip.
//
// Twiddles and window come from the packed blob (computed in double on the host, rounded once); there is no sin / cos and no atomic here.
#include <hip/hip_runtime.h>

#include <cmath>
#include <map>
#include <new>
#include <vector>

#include "../../include/vtts_audio.h"
#include "../../include/vtts_hifigan.h"
#include "../../include/vtts_spectral.h"
#include "../../include/vtts_stft.h"
#include "launch_rows.h"
#include "sample_convert.h"
#include "vtts_internal.h"

// Every operation of this file is rounded on its own: no a * b + c becomes an FMA (the header states single roundings, the forward
// transform's bits are spectral.hip's, and a sample's sums must not depend on how the compiler schedules a workgroup's run).
#pragma clang fp contract(off)

#include "stft_back.h"
#include "stft_front.h"
#include "stft_host.h"
#include "stockham.h"

using vtts::failf;
using namespace vtts_stft_front;
using namespace vtts_stft_back;
namespace sh = vtts_stft_host;

namespace {

constexpr int ROWS_PER_LAUNCH = 128;
static_assert(ROWS_PER_LAUNCH == VTTS_STFT_ROWS_PER_LAUNCH, "the header states the split");
using Rows = vtts_rows::Lens<ROWS_PER_LAUNCH>;  // samples of each row of this launch
constexpr int MAX_F = sh::MAX_F;
constexpr int SIGNALS = 1, REDUCE = 0;  // of sh::frames_lds_bytes: one staged signal, nothing to reduce

size_t inv_lds_bytes(int n_fft) {
    const int H = n_fft / 2;
    return (size_t)8 * H + (size_t)8 * (H / 2 + 2) + (size_t)4 * n_fft + (size_t)8 * inv_waves(n_fft) * pad8(H);
}

struct FwdArgs {             // every pointer at the launch's first row
    const void* x;
    const float* blob;       // window [n_fft] | exp(-2 pi i m / H) [H] | exp(-2 pi i k / n_fft) [H / 2 + 1]
    long long s_stride;      // samples between rows
    long long t_stride;      // frames between rows of spec, mag and tprev
    float2* spec;
    const float* mag;        // PROJ only
    float2* tprev;           // PROJ only
    float alpha;             // PROJ only: momentum / (1 + momentum)
    int hop, F, span, P;     // span = even((F - 1) hop + n_fft): floats of the staged signal; P = the framing's pad
};

struct InvArgs {
    const float2* spec;
    const float* blob;
    void* out;
    long long s_stride, t_stride;
    int hop, P, lead, win;   // the window's support is [lead, lead + win) of a frame
    float scale;             // 1 / n_fft
};

__device__ __forceinline__ long long num_frames_dev(long long S, int P, int n_fft, int hop) { return (S + 2 * P - n_fft) / hop + 1; }

template <int NFFT, typename TI, bool PROJ>
__global__ __launch_bounds__(64 * MAX_F) void stft_forward_k(const FwdArgs a, const Rows rows) {
    constexpr int H = NFFT / 2, NB = H + 1, XB = pad8(H);
    extern __shared__ float2 lds2[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int F = a.F;
    float2* twH = lds2;                                       // [H]
    float2* twN = twH + H;                                    // [H / 2 + 2]
    float* span = reinterpret_cast<float*>(twN + H / 2 + 2);  // [a.span]
    float2* xb = reinterpret_cast<float2*>(span + a.span) + wave * XB;

    const int b = blockIdx.y;
    const long long S = rows.len[b];  // >= P + 1, and one frame at least (checked on the host)
    const long long T = num_frames_dev(S, a.P, NFFT, a.hop);
    const long long t0 = (long long)blockIdx.x * F;
    if (t0 >= T) return;  // block-uniform

    Window<H> wv;
    load_window<H>(wv, a.blob, lane);
    stage_twiddles<H>(twH, twN, a.blob, tid, 64 * F);
    // ---- 1. stage: span[i] = padded sample hop t0 + i = row sample hop t0 - P + i, reflected at the row's ends
    stage_reflected(span, static_cast<const TI*>(a.x) + (long long)b * a.s_stride, S, t0 * a.hop - a.P, a.span, tid, 64 * F);
    __syncthreads();

    // ---- 2./3. From here on a wave touches only its own exchange buffer.
    const long long t = t0 + wave;
    if (t >= T) return;
    transform_frame<H>(xb, twH, lane, span + wave * a.hop, wv);
    Bins<H> z;
    gather_bins(z, xb, lane);
    const long long row = ((long long)b * a.t_stride + t) * NB;
    auto store = [&](int f, float2 c) {
        if constexpr (PROJ) {
            const float2 tp = a.tprev[row + f];
            const float2 d = make_float2(c.x - a.alpha * tp.x, c.y - a.alpha * tp.y);
            const float den = sqrtf(d.x * d.x + d.y * d.y) + 1e-16f;
            const float mg = a.mag[row + f];
            a.spec[row + f] = make_float2(mg * (d.x / den), mg * (d.y / den));
            a.tprev[row + f] = c;
        } else {
            a.spec[row + f] = c;
        }
    };
    split_bins(z, twN, lane, [&](int, int k, float2 p, float2 m) {
        store(k, p);
        if (k != H / 2) store(H - k, conj(m));
    });
}

template <int NFFT, typename TO>
__global__ __launch_bounds__(64 * inv_waves(NFFT)) void stft_inverse_k(const InvArgs a, const Rows rows) {
    constexpr int H = NFFT / 2, NB = H + 1, XB = pad8(H), W = inv_waves(NFFT), R = inv_per_thread(NFFT), NT = 64 * W, RUN = NT * R;
    constexpr int J = (H / 2) / 64 + 1;
    extern __shared__ float2 lds2[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float2* twH = lds2;                                         // [H]
    float2* twN = twH + H;                                      // [H / 2 + 2]
    float* winl = reinterpret_cast<float*>(twN + H / 2 + 2);    // [NFFT]
    float2* xall = reinterpret_cast<float2*>(winl + NFFT);      // [W][XB]
    float2* xb = xall + wave * XB;

    const int b = blockIdx.y;
    const int S = rows.len[b];
    const int g0 = blockIdx.x * RUN;  // < 2^24 + RUN
    if (g0 >= S) return;              // block-uniform
    const int T = (int)num_frames_dev(S, a.P, NFFT, a.hop);
    stage_twiddles<H>(twH, twN, a.blob, tid, NT);
    for (int i = tid; i < NFFT; i += NT) winl[i] = a.blob[i];
    // the frames whose window [hop t + lead, hop t + lead + win) meets the run's padded samples [p0, p1]
    const int p0 = g0 + a.P, p1 = min(g0 + RUN, S) - 1 + a.P;
    int t_lo, t_hi;
    covering_frames(p0, p1, T, a.hop, a.lead, a.win, t_lo, t_hi);  // p1 >= P >= lead

    float y[R], e[R];
#pragma unroll
    for (int r = 0; r < R; ++r) y[r] = 0.0f, e[r] = 0.0f;
    __syncthreads();

    for (int tb = t_lo; tb <= t_hi; tb += W) {  // block-uniform bounds: every wave meets every barrier
        const int t = tb + wave;
        if (t <= t_hi) {
            const float2* X = a.spec + ((long long)b * a.t_stride + t) * NB;
            float2 xk[J], xn[J];
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const int k = min(lane + 64 * j, H / 2);
                xk[j] = X[k];
                xn[j] = X[H - k];
            }
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const int k = lane + 64 * j;
                if (k <= H / 2) put_bin_pair<H>(xb, twN, k, xk[j], xn[j]);
            }
            wave_sync();
            transform<H, true>(xb, twH, lane, FromBuffer{xb});
        }
        __syncthreads();
        add_round<R, NT, XB>(y, e, xall, winl, p0, tid, a.hop, tb, min(W, t_hi - tb + 1), a.lead, a.win);
        __syncthreads();
    }
    TO* out = static_cast<TO*>(a.out) + (long long)b * a.s_stride;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int g = g0 + tid + NT * r;
        if (g < S) out[g] = vtts_sample::from_float<TO>((y[r] / e[r]) * a.scale);
    }
}

template <int NFFT>
hipError_t launch_fwd(bool pcm, bool proj, dim3 grid, int F, size_t lds, hipStream_t s, const FwdArgs& a, const Rows& rows, vtts::DynLdsOnce* once) {
    const void* fn = pcm ? (proj ? reinterpret_cast<const void*>(&stft_forward_k<NFFT, short, true>) : reinterpret_cast<const void*>(&stft_forward_k<NFFT, short, false>))
                         : (proj ? reinterpret_cast<const void*>(&stft_forward_k<NFFT, float, true>) : reinterpret_cast<const void*>(&stft_forward_k<NFFT, float, false>));
    const hipError_t e = vtts::set_max_dynamic_lds(fn, VTTS_SPECTRAL_LDS_BUDGET, once[2 * pcm + proj]);
    if (e != hipSuccess) return e;
    if (pcm && proj)
        hipLaunchKernelGGL((stft_forward_k<NFFT, short, true>), grid, dim3(64 * F), lds, s, a, rows);
    else if (pcm)
        hipLaunchKernelGGL((stft_forward_k<NFFT, short, false>), grid, dim3(64 * F), lds, s, a, rows);
    else if (proj)
        hipLaunchKernelGGL((stft_forward_k<NFFT, float, true>), grid, dim3(64 * F), lds, s, a, rows);
    else
        hipLaunchKernelGGL((stft_forward_k<NFFT, float, false>), grid, dim3(64 * F), lds, s, a, rows);
    return hipGetLastError();
}

template <int NFFT>
hipError_t launch_inv(bool pcm, dim3 grid, hipStream_t s, const InvArgs& a, const Rows& rows, vtts::DynLdsOnce* once) {
    const void* fn = pcm ? reinterpret_cast<const void*>(&stft_inverse_k<NFFT, short>) : reinterpret_cast<const void*>(&stft_inverse_k<NFFT, float>);
    const hipError_t e = vtts::set_max_dynamic_lds(fn, VTTS_SPECTRAL_LDS_BUDGET, once[pcm]);
    if (e != hipSuccess) return e;
    const size_t lds = inv_lds_bytes(NFFT);
    if (pcm)
        hipLaunchKernelGGL((stft_inverse_k<NFFT, short>), grid, dim3(64 * inv_waves(NFFT)), lds, s, a, rows);
    else
        hipLaunchKernelGGL((stft_inverse_k<NFFT, float>), grid, dim3(64 * inv_waves(NFFT)), lds, s, a, rows);
    return hipGetLastError();
}

}  // namespace

struct vtts_stft : sh::Tables {
    vtts_stft_cfg cfg;
    int device = 0;
    int F = 1;
    int P = 0, lead = 0;
    std::map<int64_t, double> envelope;  // min_envelope() of the lengths seen so far
    vtts::DynLdsOnce lds_fwd[4], lds_inv[2];
};

namespace {
int64_t num_frames(const vtts_stft* h, int64_t S) { return (S + 2 * h->P - h->cfg.n_fft) / h->cfg.hop + 1; }
int64_t min_samples(const vtts_stft* h) {
    const int64_t one = (int64_t)h->cfg.n_fft - 2 * h->P;  // the S of one frame
    return h->P + 1 > one ? h->P + 1 : one;
}
int check_len(const vtts_stft* h, const char* what, int64_t S) {
    if (S < min_samples(h) || S > VTTS_STFT_MAX_SAMPLES)
        return failf(VTTS_ERR_SHAPE, "%s must be in %lld .. %d samples (the reflection padding needs pad + 1 = %d, one frame %d; got %lld)", what,
                     (long long)min_samples(h), VTTS_STFT_MAX_SAMPLES, h->P + 1, h->cfg.n_fft - 2 * h->P, (long long)S);
    return VTTS_OK;
}
// min over g < S of sum_t w[p - hop t]^2, p = g + P, t < T: in double from the fp32 window
double min_envelope(const vtts_stft* h, int64_t S) {
    const int n_fft = h->cfg.n_fft, hop = h->cfg.hop;
    const int64_t T = num_frames(h, S);
    const float* w = h->img.data();
    auto at = [&](int64_t g) {
        const int64_t p = g + h->P;
        int64_t t1 = p / hop;
        if (t1 > T - 1) t1 = T - 1;
        double e = 0.0;
        for (int64_t t = t1; t >= 0 && p - hop * t < n_fft; --t) e += (double)w[p - hop * t] * (double)w[p - hop * t];
        return e;
    };
    double m = INFINITY;
    const int64_t edge = (int64_t)n_fft + hop;
    for (int64_t g = 0; g < S && g < edge; ++g) m = fmin(m, at(g));
    for (int64_t g = S - edge > edge ? S - edge : edge; g < S; ++g) m = fmin(m, at(g));
    return m;
}
int check_batch(vtts_stft* h, int N, int64_t S_stride, const int32_t* lengths, int64_t T_stride, int64_t* longest) {
    if (N <= 0) return failf(VTTS_ERR_INVALID, "N must be positive (got %d)", N);
    if (S_stride < 0 || S_stride > 0x7fffffff) return failf(VTTS_ERR_SHAPE, "S_stride must be in 0 .. 2^31 - 1 (got %lld)", (long long)S_stride);
    int64_t m = 0;
    for (int b = 0; b < N; ++b) {
        const int64_t len = lengths ? lengths[b] : S_stride;
        if (len > S_stride) return failf(VTTS_ERR_SHAPE, "lengths[%d] = %lld is above S_stride = %lld", b, (long long)len, (long long)S_stride);
        if (int rc = check_len(h, "every row", len)) return rc;
        if (len > m) m = len;
    }
    if (T_stride < num_frames(h, m))
        return failf(VTTS_ERR_SHAPE, "T_stride = %lld is below the longest row's %lld frames", (long long)T_stride, (long long)num_frames(h, m));
    *longest = m;
    return VTTS_OK;
}

int forward_or_project(vtts_stft* h, const char* what, bool proj, const void* wav_dev, int dtype, int N, int64_t S_stride, const int32_t* lengths,
                       const float* mag_dev, void* tprev_dev, void* spec_dev, int64_t T_stride, float momentum, void* stream) {
    if (!h || !wav_dev || !spec_dev || (proj && (!mag_dev || !tprev_dev))) return failf(VTTS_ERR_INVALID, "null argument");
    if (dtype != VTTS_AUDIO_F32 && dtype != VTTS_AUDIO_PCM16) return failf(VTTS_ERR_INVALID, "dtype must be VTTS_AUDIO_F32 or VTTS_AUDIO_PCM16 (got %d)", dtype);
    if (proj && !(momentum >= 0.0f && momentum < 1.0f)) return failf(VTTS_ERR_INVALID, "momentum must be in [0, 1) (got %g)", (double)momentum);
    if (proj && tprev_dev == spec_dev) return failf(VTTS_ERR_INVALID, "spec_dev must not be tprev_dev");
    if (!h->blob) return failf(VTTS_ERR_STATE, "%s() before pack()/bind_packed()", what);
    int64_t longest = 0;
    if (int rc = check_batch(h, N, S_stride, lengths, T_stride, &longest)) return rc;
    const int F = h->F, n_fft = h->cfg.n_fft, hop = h->cfg.hop;
    const int64_t gmax = (num_frames(h, longest) + F - 1) / F;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool pcm = dtype == VTTS_AUDIO_PCM16;
    const size_t esz = pcm ? 2 : 4, lds = sh::frames_lds_bytes(n_fft, hop, F, SIGNALS, REDUCE), nb = (size_t)n_fft / 2 + 1;
    return vtts_rows::for_each_launch<ROWS_PER_LAUNCH>(N, lengths, S_stride, [&](int r0, int nr, const Rows& rows) -> int {
        FwdArgs a;
        a.x = static_cast<const char*>(wav_dev) + (size_t)r0 * S_stride * esz;
        a.blob = h->blob;
        a.s_stride = S_stride;
        a.t_stride = T_stride;
        a.spec = static_cast<float2*>(spec_dev) + (size_t)r0 * T_stride * nb;
        a.mag = proj ? mag_dev + (size_t)r0 * T_stride * nb : nullptr;
        a.tprev = proj ? static_cast<float2*>(tprev_dev) + (size_t)r0 * T_stride * nb : nullptr;
        a.alpha = proj ? momentum / (1.0f + momentum) : 0.0f;
        a.hop = hop, a.F = F, a.span = sh::even((F - 1) * hop + n_fft), a.P = h->P;
        const dim3 grid((unsigned)gmax, (unsigned)nr);
        const hipError_t e = sh::by_nfft(n_fft, [&](auto n) { return launch_fwd<decltype(n)::value>(pcm, proj, grid, F, lds, s, a, rows, h->lds_fwd); });
        if (e != hipSuccess) return failf(VTTS_ERR_HIP, "stft %s kernel launch failed: %s", what, hipGetErrorString(e));
        return VTTS_OK;
    });
}
}  // namespace

VTTS_API int vtts_stft_create(const vtts_stft_cfg* cfg, int device, vtts_stft** out) {
    if (!cfg || !out) return failf(VTTS_ERR_INVALID, "null argument");
    const vtts_stft_cfg& c = *cfg;
    if (int rc = sh::check_resolution(c.n_fft, c.hop, c.win)) return rc;
    if (c.framing != VTTS_STFT_CENTER && c.framing != VTTS_STFT_MEL)
        return failf(VTTS_ERR_INVALID, "framing must be VTTS_STFT_CENTER or VTTS_STFT_MEL (got %d)", c.framing);
    if (c.framing == VTTS_STFT_MEL && (c.n_fft - c.hop) % 2)
        return failf(VTTS_ERR_INVALID, "VTTS_STFT_MEL framing pads (n_fft - hop) / 2 on each side: n_fft - hop must be even (got n_fft %d, hop %d)", c.n_fft, c.hop);
    auto* h = new (std::nothrow) vtts_stft();
    if (!h) return failf(VTTS_ERR_NOMEM, "host allocation failed");
    h->cfg = c;
    h->device = device;
    h->F = sh::frames_per_block(c.n_fft, c.hop, SIGNALS, REDUCE);
    h->P = c.framing == VTTS_STFT_MEL ? (c.n_fft - c.hop) / 2 : c.n_fft / 2;
    h->lead = (c.n_fft - c.win) / 2;
    h->build(c.n_fft, c.win);
    *out = h;
    return VTTS_OK;
}

VTTS_API void vtts_stft_destroy(vtts_stft* h) { delete h; }

VTTS_API int vtts_stft_window(const vtts_stft* h, float* host_out) { return sh::window(h, h ? h->cfg.n_fft : 0, host_out); }

VTTS_API int vtts_stft_blocking(const vtts_stft* h, int* forward_frames, int* inverse_waves, int* inverse_run) {
    if (!h || !forward_frames || !inverse_waves || !inverse_run) return failf(VTTS_ERR_INVALID, "null argument");
    *forward_frames = h->F;
    *inverse_waves = inv_waves(h->cfg.n_fft);
    *inverse_run = inv_run(h->cfg.n_fft);
    return VTTS_OK;
}

VTTS_API int vtts_stft_num_frames(const vtts_stft* h, int64_t n_samples, int64_t* frames) {
    if (!h || !frames) return failf(VTTS_ERR_INVALID, "null argument");
    if (int rc = check_len(h, "n_samples", n_samples)) return rc;
    *frames = num_frames(h, n_samples);
    return VTTS_OK;
}

VTTS_API int vtts_stft_num_samples(const vtts_stft* h, int64_t frames, int64_t* n_samples) {
    if (!h || !n_samples) return failf(VTTS_ERR_INVALID, "null argument");
    if (frames < 1) return failf(VTTS_ERR_SHAPE, "frames must be positive (got %lld)", (long long)frames);
    const int64_t S = (frames - 1) * h->cfg.hop + h->cfg.n_fft - 2 * h->P;  // the smallest S with that many frames
    if (frames > VTTS_STFT_MAX_SAMPLES || S > VTTS_STFT_MAX_SAMPLES || S < min_samples(h))
        return failf(VTTS_ERR_SHAPE, "%lld frames are %lld samples, outside %lld .. %d (the reflection padding needs pad + 1 = %d)", (long long)frames, (long long)S,
                     (long long)min_samples(h), VTTS_STFT_MAX_SAMPLES, h->P + 1);
    *n_samples = S;
    return VTTS_OK;
}

VTTS_API int vtts_stft_min_envelope(const vtts_stft* h, int64_t n_samples, double* envelope) {
    if (!h || !envelope) return failf(VTTS_ERR_INVALID, "null argument");
    if (int rc = check_len(h, "n_samples", n_samples)) return rc;
    *envelope = min_envelope(h, n_samples);
    return VTTS_OK;
}

VTTS_API int vtts_stft_packed_bytes(const vtts_stft* h, size_t* bytes) { return sh::packed_bytes(h, bytes); }

VTTS_API int vtts_stft_pack(vtts_stft* h, void* dev_blob, size_t blob_bytes, void* stream) {
    return sh::pack(h, dev_blob, blob_bytes, stream, "the stft tables");
}

VTTS_API int vtts_stft_bind_packed(vtts_stft* h, void* dev_blob, size_t blob_bytes) { return sh::bind_packed(h, dev_blob, blob_bytes); }

VTTS_API int vtts_stft_forward(vtts_stft* h, const void* wav_dev, int dtype, int N, int64_t S_stride, const int32_t* lengths, void* spec_dev,
                               int64_t T_stride, void* stream) {
    return forward_or_project(h, "forward", false, wav_dev, dtype, N, S_stride, lengths, nullptr, nullptr, spec_dev, T_stride, 0.0f, stream);
}

VTTS_API int vtts_stft_project(vtts_stft* h, const void* wav_dev, int dtype, int N, int64_t S_stride, const int32_t* lengths, const float* mag_dev,
                               void* tprev_dev, void* spec_dev, int64_t T_stride, float momentum, void* stream) {
    return forward_or_project(h, "project", true, wav_dev, dtype, N, S_stride, lengths, mag_dev, tprev_dev, spec_dev, T_stride, momentum, stream);
}

VTTS_API int vtts_stft_inverse(vtts_stft* h, const void* spec_dev, int N, int64_t T_stride, const int32_t* lengths, void* out_dev, int dtype,
                               int64_t S_stride, void* stream) {
    if (!h || !spec_dev || !out_dev) return failf(VTTS_ERR_INVALID, "null argument");
    if (dtype != VTTS_AUDIO_F32 && dtype != VTTS_AUDIO_PCM16) return failf(VTTS_ERR_INVALID, "dtype must be VTTS_AUDIO_F32 or VTTS_AUDIO_PCM16 (got %d)", dtype);
    if (!h->blob) return failf(VTTS_ERR_STATE, "inverse() before pack()/bind_packed()");
    int64_t longest = 0;
    if (int rc = check_batch(h, N, S_stride, lengths, T_stride, &longest)) return rc;
    const int n_fft = h->cfg.n_fft;
    for (int b = 0; b < N; ++b) {  // NOLA, once per distinct length
        const int64_t len = lengths ? lengths[b] : S_stride;
        auto it = h->envelope.find(len);
        if (it == h->envelope.end()) {
            if (h->envelope.size() >= 4096) h->envelope.clear();
            it = h->envelope.emplace(len, min_envelope(h, len)).first;
        }
        if (!(it->second >= VTTS_STFT_NOLA_FLOOR))
            return failf(VTTS_ERR_INVALID, "the squared Hann window of %d samples overlap-added at hop %d falls to %.3g inside a row of %lld samples, below %g (NOLA): no inverse",
                         h->cfg.win, h->cfg.hop, it->second, (long long)len, VTTS_STFT_NOLA_FLOOR);
    }
    const int run = inv_run(n_fft);
    const int64_t gmax = (longest + run - 1) / run;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool pcm = dtype == VTTS_AUDIO_PCM16;
    const size_t esz = pcm ? 2 : 4, nb = (size_t)n_fft / 2 + 1;
    return vtts_rows::for_each_launch<ROWS_PER_LAUNCH>(N, lengths, S_stride, [&](int r0, int nr, const Rows& rows) -> int {
        InvArgs a;
        a.spec = static_cast<const float2*>(spec_dev) + (size_t)r0 * T_stride * nb;
        a.blob = h->blob;
        a.out = static_cast<char*>(out_dev) + (size_t)r0 * S_stride * esz;
        a.s_stride = S_stride;
        a.t_stride = T_stride;
        a.hop = h->cfg.hop, a.P = h->P, a.lead = h->lead, a.win = h->cfg.win;
        a.scale = 1.0f / (float)n_fft;
        const dim3 grid((unsigned)gmax, (unsigned)nr);
        const hipError_t e = sh::by_nfft(n_fft, [&](auto n) { return launch_inv<decltype(n)::value>(pcm, grid, s, a, rows, h->lds_inv); });
        if (e != hipSuccess) return failf(VTTS_ERR_HIP, "stft inverse kernel launch failed: %s", hipGetErrorString(e));
        return VTTS_OK;
    });
}
