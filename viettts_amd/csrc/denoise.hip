// STFT-domain spectral subtraction in one pass (include/vtts_denoise.h); batched and ragged.
//
//   denoise_k<NFFT, TI, TO>  workgroup = RUN consecutive output samples of one row, W waves (stft.hip's stft_inverse_k's shape); thread i owns
//     samples i, i + 64 W, ... and keeps their overlap-add sum y and envelope e in registers.  The frames whose window covers the run are walked
//     in ascending t, W per round.  In a round each wave, for its frame:
//     1. reads the frame's NFFT samples from global memory, reflected at the ROW'S OWN ends, times the window (from LDS), into the first pass of
//        stockham.h's forward transform in its own exchange buffer: stft_forward_k's products, so its bits;
//     2. gathers and splits the result into bins 0 .. H (stft_front.h: a lane pairs bin k with bin H - k);
//     3. scales both bins of each pair in registers: c -> max(|c| - strength bias, 0) c / (|c| + 1e-16), strength bias[f] from LDS;
//     4. applies the inverse split step (stft_back.h) and inverse-transforms in the same buffer.
//     After a workgroup barrier every thread adds the round's frames to its samples in ascending t; a second barrier frees the buffers.
//     At the end out = (y / e) / NFFT.  No spectrum reaches device memory and nothing here is atomic.
#include <hip/hip_runtime.h>

#include <cmath>
#include <map>
#include <new>

#include "../../include/vtts_audio.h"
#include "../../include/vtts_denoise.h"
#include "../../include/vtts_hifigan.h"
#include "../../include/vtts_spectral.h"
#include "../../include/vtts_stft.h"
#include "launch_rows.h"
#include "sample_convert.h"
#include "vtts_internal.h"

// Every operation of this file is rounded on its own, as in stft.hip: the header states single roundings and equality with that file's kernels.
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
static_assert(ROWS_PER_LAUNCH == VTTS_DENOISE_ROWS_PER_LAUNCH, "the header states the split");
using Rows = vtts_rows::Lens<ROWS_PER_LAUNCH>;  // samples of each row of this launch
static_assert(VTTS_DENOISE_MAX_SAMPLES == VTTS_STFT_MAX_SAMPLES, "the rows are vtts_stft.h's");

// the header's table: tables, window, strength x bias, W exchange buffers
size_t lds_bytes(int n_fft) {
    const int H = n_fft / 2;
    return (size_t)8 * H + (size_t)8 * (H / 2 + 2) + (size_t)4 * n_fft + (size_t)4 * (H + 2) + (size_t)8 * inv_waves(n_fft) * pad8(H);
}

struct Args {                // every pointer at the launch's first row
    const void* x;
    const float* blob;       // window [n_fft] | exp(-2 pi i m / H) [H] | exp(-2 pi i k / n_fft) [H / 2 + 1]
    const float* bias;       // [H + 1]
    void* out;
    long long s_stride, o_stride;
    int hop, P, lead, win;   // the window's support is [lead, lead + win) of a frame
    float strength;
    float scale;             // 1 / n_fft
};

// the header's five lines for one bin; sb = fl(strength bias[f])
__device__ __forceinline__ float2 subtract(float2 c, float sb) {
    const float r = sqrtf(c.x * c.x + c.y * c.y);
    const float m = fmaxf(r - sb, 0.0f);
    const float d = r + 1e-16f;
    return make_float2(m * (c.x / d), m * (c.y / d));
}

template <int NFFT, typename TI, typename TO>
__global__ __launch_bounds__(64 * inv_waves(NFFT)) void denoise_k(const Args a, const Rows rows) {
    constexpr int H = NFFT / 2, XB = pad8(H), W = inv_waves(NFFT), R = inv_per_thread(NFFT), NT = 64 * W, RUN = NT * R;
    extern __shared__ float2 lds2[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float2* twH = lds2;                                         // [H]
    float2* twN = twH + H;                                      // [H / 2 + 2]
    float* winl = reinterpret_cast<float*>(twN + H / 2 + 2);    // [NFFT]
    float* sbl = winl + NFFT;                                   // [H + 2]
    float2* xall = reinterpret_cast<float2*>(sbl + H + 2);      // [W][XB]
    float2* xb = xall + wave * XB;

    const int b = blockIdx.y;
    const int S = rows.len[b];  // >= P + 1, and one frame at least (checked on the host)
    const int g0 = blockIdx.x * RUN;  // < 2^24 + RUN
    if (g0 >= S) return;              // block-uniform
    const int T = (S + 2 * a.P - NFFT) / a.hop + 1;
    stage_twiddles<H>(twH, twN, a.blob, tid, NT);
    for (int i = tid; i < NFFT; i += NT) winl[i] = a.blob[i];
    for (int i = tid; i <= H; i += NT) sbl[i] = a.strength * a.bias[i];
    const int p0 = g0 + a.P, p1 = min(g0 + RUN, S) - 1 + a.P;
    int t_lo, t_hi;
    covering_frames(p0, p1, T, a.hop, a.lead, a.win, t_lo, t_hi);  // p1 >= P >= lead

    const TI* x = static_cast<const TI*>(a.x) + (long long)b * a.s_stride;
    const float2* win2 = reinterpret_cast<const float2*>(winl);
    float y[R], e[R];
#pragma unroll
    for (int r = 0; r < R; ++r) y[r] = 0.0f, e[r] = 0.0f;
    __syncthreads();

    for (int tb = t_lo; tb <= t_hi; tb += W) {  // block-uniform bounds: every wave meets every barrier
        const int t = tb + wave;
        if (t <= t_hi) {
            // ---- 1. frame t covers padded samples [hop t, hop t + NFFT): row samples from f0 on, reflected at the row's ends
            const int f0 = a.hop * t - a.P;
            if (f0 >= 0 && f0 + NFFT <= S) {  // wave-uniform: no end of the row in this frame
                const TI* fr = x + f0;
                transform<H, false>(xb, twH, lane, [&](int, int, int i) {
                    const float2 w = win2[i];
                    return make_float2(vtts_sample::to_float_exact_shift(fr[2 * i]) * w.x, vtts_sample::to_float_exact_shift(fr[2 * i + 1]) * w.y);
                });
            } else {
                transform<H, false>(xb, twH, lane, [&](int, int, int i) {
                    const float2 w = win2[i];
                    const float s0 = vtts_sample::to_float_exact_shift(x[reflect_index(f0 + 2 * i, S)]);
                    const float s1 = vtts_sample::to_float_exact_shift(x[reflect_index(f0 + 2 * i + 1, S)]);
                    return make_float2(s0 * w.x, s1 * w.y);
                });
            }
            // ---- 2. bins k and H - k of every lane, out of the buffer before anything is written back into it
            Bins<H> z;
            gather_bins(z, xb, lane);
            wave_sync();
            // ---- 3./4. X[k] = p, X[H - k] = conj(m), scaled, and the inverse split step
            split_bins(z, twN, lane, [&](int, int k, float2 p, float2 m) {
                const float2 xk = subtract(p, sbl[k]);
                const float2 xn = k == H / 2 ? xk : subtract(conj(m), sbl[H - k]);  // (bin H / 2 is its own partner: the spectrum holds p)
                put_bin_pair<H>(xb, twN, k, xk, xn);
            });
            wave_sync();
            transform<H, true>(xb, twH, lane, FromBuffer{xb});
        }
        __syncthreads();
        add_round<R, NT, XB>(y, e, xall, winl, p0, tid, a.hop, tb, min(W, t_hi - tb + 1), a.lead, a.win);
        __syncthreads();
    }
    TO* out = static_cast<TO*>(a.out) + (long long)b * a.o_stride;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int g = g0 + tid + NT * r;
        if (g < S) out[g] = vtts_sample::from_float<TO>((y[r] / e[r]) * a.scale);
    }
}

template <int NFFT, typename TI, typename TO>
hipError_t launch_one(dim3 grid, hipStream_t s, const Args& a, const Rows& rows, vtts::DynLdsOnce& once) {
    const hipError_t e = vtts::set_max_dynamic_lds(reinterpret_cast<const void*>(&denoise_k<NFFT, TI, TO>), VTTS_SPECTRAL_LDS_BUDGET, once);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((denoise_k<NFFT, TI, TO>), grid, dim3(64 * inv_waves(NFFT)), lds_bytes(NFFT), s, a, rows);
    return hipGetLastError();
}

template <int NFFT>
hipError_t launch(bool pcm_in, bool pcm_out, dim3 grid, hipStream_t s, const Args& a, const Rows& rows, vtts::DynLdsOnce* once) {
    vtts::DynLdsOnce& o = once[2 * pcm_in + pcm_out];
    if (pcm_in) return pcm_out ? launch_one<NFFT, short, short>(grid, s, a, rows, o) : launch_one<NFFT, short, float>(grid, s, a, rows, o);
    return pcm_out ? launch_one<NFFT, float, short>(grid, s, a, rows, o) : launch_one<NFFT, float, float>(grid, s, a, rows, o);
}

}  // namespace

struct vtts_denoise : sh::Tables {
    vtts_stft_cfg cfg;
    vtts_stft* stft = nullptr;           // the framing's arithmetic: row lengths and the overlap-add envelope are vtts_stft.h's
    int P = 0, lead = 0;
    std::map<int64_t, double> envelope;  // vtts_stft_min_envelope() of the lengths seen so far
    vtts::DynLdsOnce lds_once[4];
    ~vtts_denoise() { vtts_stft_destroy(stft); }
};

VTTS_API int vtts_denoise_create(const vtts_stft_cfg* cfg, int device, vtts_denoise** out) {
    if (!cfg || !out) return failf(VTTS_ERR_INVALID, "null argument");
    vtts_stft* st = nullptr;
    if (int rc = vtts_stft_create(cfg, device, &st)) return rc;  // the same four transform lengths, both framings, the same refusals
    auto* h = new (std::nothrow) vtts_denoise();
    if (!h) {
        vtts_stft_destroy(st);
        return failf(VTTS_ERR_NOMEM, "host allocation failed");
    }
    h->cfg = *cfg;
    h->stft = st;
    h->P = cfg->framing == VTTS_STFT_MEL ? (cfg->n_fft - cfg->hop) / 2 : cfg->n_fft / 2;
    h->lead = (cfg->n_fft - cfg->win) / 2;
    h->build(cfg->n_fft, cfg->win);
    static_assert(sizeof(float) == 4, "the blob is fp32");
    if (lds_bytes(cfg->n_fft) > VTTS_SPECTRAL_LDS_BUDGET) {
        delete h;
        return failf(VTTS_ERR_INVALID, "the denoiser's workgroup needs %zu bytes of LDS, above the budget of %d", lds_bytes(cfg->n_fft), VTTS_SPECTRAL_LDS_BUDGET);
    }
    *out = h;
    return VTTS_OK;
}

VTTS_API void vtts_denoise_destroy(vtts_denoise* h) { delete h; }

VTTS_API int vtts_denoise_blocking(const vtts_denoise* h, int* waves, int* run) {
    if (!h || !waves || !run) return failf(VTTS_ERR_INVALID, "null argument");
    *waves = inv_waves(h->cfg.n_fft);
    *run = inv_run(h->cfg.n_fft);
    return VTTS_OK;
}

VTTS_API int vtts_denoise_packed_bytes(const vtts_denoise* h, size_t* bytes) { return sh::packed_bytes(h, bytes); }

VTTS_API int vtts_denoise_pack(vtts_denoise* h, void* dev_blob, size_t blob_bytes, void* stream) {
    return sh::pack(h, dev_blob, blob_bytes, stream, "the denoiser's tables");
}

VTTS_API int vtts_denoise_bind_packed(vtts_denoise* h, void* dev_blob, size_t blob_bytes) { return sh::bind_packed(h, dev_blob, blob_bytes); }

VTTS_API int vtts_denoise_apply(vtts_denoise* h, const void* wav_dev, int in_dtype, int N, int64_t S_stride, const int32_t* lengths, const float* bias_dev,
                                float strength, void* out_dev, int out_dtype, int64_t out_stride, void* stream) {
    if (!h || !wav_dev || !bias_dev || !out_dev) return failf(VTTS_ERR_INVALID, "null argument");
    for (int dtype : {in_dtype, out_dtype})
        if (dtype != VTTS_AUDIO_F32 && dtype != VTTS_AUDIO_PCM16)
            return failf(VTTS_ERR_INVALID, "in_dtype and out_dtype must be VTTS_AUDIO_F32 or VTTS_AUDIO_PCM16 (got %d)", dtype);
    if (!(strength >= 0.0f) || !std::isfinite(strength)) return failf(VTTS_ERR_INVALID, "strength must be finite and not negative (got %g)", (double)strength);
    if (!h->blob) return failf(VTTS_ERR_STATE, "apply() before pack()/bind_packed()");
    if (N <= 0) return failf(VTTS_ERR_INVALID, "N must be positive (got %d)", N);
    if (S_stride < 0 || S_stride > 0x7fffffff) return failf(VTTS_ERR_SHAPE, "S_stride must be in 0 .. 2^31 - 1 (got %lld)", (long long)S_stride);
    if (out_stride < 0 || out_stride > 0x7fffffff) return failf(VTTS_ERR_SHAPE, "out_stride must be in 0 .. 2^31 - 1 (got %lld)", (long long)out_stride);
    int64_t longest = 0;
    for (int b = 0; b < N; ++b) {  // the row's length by vtts_stft.h's rule, and NOLA, once per distinct length
        const int64_t len = lengths ? lengths[b] : S_stride;
        if (len > S_stride) return failf(VTTS_ERR_SHAPE, "lengths[%d] = %lld is above S_stride = %lld", b, (long long)len, (long long)S_stride);
        if (len > out_stride) return failf(VTTS_ERR_SHAPE, "lengths[%d] = %lld is above out_stride = %lld", b, (long long)len, (long long)out_stride);
        auto it = h->envelope.find(len);
        if (it == h->envelope.end()) {
            double env = 0.0;
            if (int rc = vtts_stft_min_envelope(h->stft, len, &env)) return rc;  // VTTS_ERR_SHAPE for what no row may be
            if (h->envelope.size() >= 4096) h->envelope.clear();
            it = h->envelope.emplace(len, env).first;
        }
        if (!(it->second >= VTTS_DENOISE_NOLA_FLOOR))
            return failf(VTTS_ERR_INVALID, "the squared Hann window of %d samples overlap-added at hop %d falls to %.3g inside a row of %lld samples, below %g (NOLA): no inverse",
                         h->cfg.win, h->cfg.hop, it->second, (long long)len, VTTS_DENOISE_NOLA_FLOOR);
        if (len > longest) longest = len;
    }
    const bool pcm_in = in_dtype == VTTS_AUDIO_PCM16, pcm_out = out_dtype == VTTS_AUDIO_PCM16;
    const size_t isz = pcm_in ? 2 : 4, osz = pcm_out ? 2 : 4;
    {  // the kernel reads a frame's samples while a neighbouring workgroup writes its run: the two arrays may not share a byte
        const char* i0 = static_cast<const char*>(wav_dev);
        const char* o0 = static_cast<const char*>(out_dev);
        const char* i1 = i0 + ((size_t)(N - 1) * S_stride + longest) * isz;
        const char* o1 = o0 + ((size_t)(N - 1) * out_stride + longest) * osz;
        if (i0 < o1 && o0 < i1) return failf(VTTS_ERR_INVALID, "out_dev must not overlap wav_dev: a frame reads samples that another workgroup's run writes");
    }
    const int n_fft = h->cfg.n_fft, run = inv_run(n_fft);
    const int64_t gmax = (longest + run - 1) / run;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return vtts_rows::for_each_launch<ROWS_PER_LAUNCH>(N, lengths, S_stride, [&](int r0, int nr, const Rows& rows) -> int {
        Args a;
        a.x = static_cast<const char*>(wav_dev) + (size_t)r0 * S_stride * isz;
        a.blob = h->blob;
        a.bias = bias_dev;
        a.out = static_cast<char*>(out_dev) + (size_t)r0 * out_stride * osz;
        a.s_stride = S_stride, a.o_stride = out_stride;
        a.hop = h->cfg.hop, a.P = h->P, a.lead = h->lead, a.win = h->cfg.win;
        a.strength = strength;
        a.scale = 1.0f / (float)n_fft;
        const dim3 grid((unsigned)gmax, (unsigned)nr);
        const hipError_t e = sh::by_nfft(n_fft, [&](auto n) { return launch<decltype(n)::value>(pcm_in, pcm_out, grid, s, a, rows, h->lds_once); });
        if (e != hipSuccess) return failf(VTTS_ERR_HIP, "denoise kernel launch failed: %s", hipGetErrorString(e));
        return VTTS_OK;
    });
}
