// Waveform -> log-mel front end (include/vtts_mel.h): vietTTS/nat/dsp.py MelFilter.__call__ == vietTTS/hifigan/create_mel.py
// mel_spectrogram(center=False), one fused kernel.  Samples in, log-mel out; the [N, 513, T] spectrum never reaches HBM.
//
//   workgroup = VTTS_MEL_FRAMES_PER_BLOCK (8) consecutive frames of one row, one wave per frame.
//   1. stage: the (8 + 3) * 256 samples the eight frames cover, once, into LDS (16-byte loads; PCM16 scaled by 2^-15 on the way),
//      mirrored at the ROW'S OWN ends.  The 4x overlap of the frames is served from LDS: every sample is read from HBM once.
//   2. FFT: a real 1024-point transform = a 512-point complex FFT of z[n] = x[2n] + i x[2n+1] and a split step.
//      512 = 8 x 8 x 8: 64 lanes x 8 points, three radix-8 passes in registers, two exchanges through padded LDS rows (stockham.h:
//      fft512_888, shared with stoi.hip; the first pass's twiddles wait in registers here).  Window and twiddles come from tables computed
//      in double on the host and rounded once; there is no sin / cos in the kernel.
//      A wave touches only its own exchange buffer and the LDS keeps one wave's accesses in order, so the exchanges are separated
//      by a compiler-only wave fence (wave_sync), not by workgroup barriers.
//   3. split step: lane pairs bin k with bin 512 - k, X[k] = E + W1024^k O, X[512 - k] = conj(E - W1024^k O); magnitudes
//      sqrt(re^2 + im^2 + 1e-9) go to LDS, over the wave's exchange buffer.  52 KB of LDS per workgroup: three per CU.
//   4. mel projection: the basis has at most two non-zero bands per bin, so band m (one lane each) sums its own support
//      [start, start + count) in ascending bin order: ~1000 multiply-adds per frame instead of 41 040, all terms non-negative.
//      (The dense product over all 513 bins, one band per lane, made the whole pass 4x slower: DESIGN.md section 6e.)
//   5. out = mel > 1e-5 ? logf(mel) : (float)log(1e-5), coalesced [T][n_mels] stores.  Frames past a row's own count, up to the
//      output's T_stride, are set to that floor value.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/vtts_hifigan.h"
#include "../../include/vtts_mel.h"
#include "launch_rows.h"
#include "mel_framing.h"
#include "sample_convert.h"
#include "stockham.h"  // under this file's default contraction: the a * b + c of its complex products are FMAs here, as they always were
#include "vtts_internal.h"

using vtts::check_blob;
using vtts::failf;
using vtts::upload_blob;
using vtts_sample::to_float;
using namespace vtts_stockham;
namespace mf = vtts_mel_framing;

namespace {

constexpr int NFFT = mf::NFFT, HOP = mf::HOP, NBINS = NFFT / 2 + 1, HALF = NFFT / 2;
constexpr int PADL = mf::PADL;                            // 384 reflected samples on each side
constexpr int FPB = VTTS_MEL_FRAMES_PER_BLOCK;            // frames (= waves) per workgroup
constexpr int THREADS = 64 * FPB;
constexpr int SPAN = (FPB + 3) * HOP;                     // samples the FPB frames cover
constexpr int MAX_MELS = 128;
constexpr int ROWS_PER_LAUNCH = 256;
constexpr int MAX_NNZ = 2 * NBINS;                        // triangles overlap their neighbours only: two bands per bin

// blob layout, in floats
constexpr int OFF_WIN = 0;                                // [1024] periodic Hann
constexpr int OFF_TW512 = OFF_WIN + NFFT;                 // [512] complex exp(-2 pi i j / 512)
constexpr int OFF_TW1024 = OFF_TW512 + 2 * HALF;          // [257] complex exp(-2 pi i k / 1024), padded to 260
constexpr int OFF_BAND = OFF_TW1024 + 2 * 260;            // [3][128] int: first bin, bin count, offset into the non-zeros
constexpr int OFF_SPW = OFF_BAND + 3 * MAX_MELS;          // [MAX_NNZ] the bands' non-zero weights, band after band
constexpr int BLOB_FLOATS = OFF_SPW + MAX_NNZ + 2;

constexpr size_t LDS_BYTES = (size_t)(SPAN + FPB * 2 * XBUF + MAX_NNZ) * sizeof(float);

using Rows = vtts_rows::Lens<ROWS_PER_LAUNCH>;  // samples of each row of this launch

struct MelArgs {
    const void* wav;   // first row of this launch
    float* mel;        // first row of this launch
    const float* blob;
    long s_stride;     // samples between rows
    long t_stride;     // frames between output rows = frames to write per row
    int n_mels, nnz;
    int vec_ok;        // rows are 16-byte aligned: interior chunks take one 16-byte load
    float floor_log;   // (float)log(1e-5)
};

template <typename T>
__global__ __launch_bounds__(THREADS) void mel_fused_k(const MelArgs a, const Rows rows) {
    extern __shared__ float4 lds4[];
    float* lds = reinterpret_cast<float*>(lds4);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* span = lds;
    float2* xb = reinterpret_cast<float2*>(lds + SPAN) + wave * XBUF;
    float* spw = lds + SPAN + FPB * 2 * XBUF;

    const int b = blockIdx.y;
    const int L = rows.len[b];                 // >= 385 (checked on the host)
    const int Tb = (L + 2 * PADL - NFFT) / HOP + 1;
    const int t0 = blockIdx.x * FPB;
    float* out = a.mel + (long)b * a.t_stride * a.n_mels;
    if (t0 >= Tb) {  // the whole tile lies past this row's frames (block-uniform): floor only
        const long n = (long)min((long)FPB, a.t_stride - t0) * a.n_mels;
        for (long i = tid; i < n; i += THREADS) out[(long)t0 * a.n_mels + i] = a.floor_log;
        return;
    }

    // this lane's window and first-pass twiddles: issued now, so that their latency hides behind the staging
    const float2* win2 = reinterpret_cast<const float2*>(a.blob + OFF_WIN);
    const float2* tw512 = reinterpret_cast<const float2*>(a.blob + OFF_TW512);
    const float2* tw1024 = reinterpret_cast<const float2*>(a.blob + OFF_TW1024);
    float2 win[8], tw1[7];
#pragma unroll
    for (int q = 0; q < 8; ++q) win[q] = win2[64 * q + lane];
#pragma unroll
    for (int k0 = 1; k0 < 8; ++k0) tw1[k0 - 1] = tw512[lane * k0];
    for (int i = tid; i < a.nnz; i += THREADS) spw[i] = a.blob[OFF_SPW + i];
    // ---- 1. stage the span: span[j] = padded sample 256 t0 + j = row sample 256 t0 - 384 + j, reflected at the row's ends
    {
        const T* x = static_cast<const T*>(a.wav) + (long)b * a.s_stride;
        const long q0 = (long)t0 * HOP - PADL;
        constexpr int CH = 16 / sizeof(T);
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
    }
    __syncthreads();

    // ---- 2. windowed frame -> 512-point complex FFT.  From here on a wave touches only its own exchange buffer: LDS executes one
    // wave's accesses in order, so the exchanges need wave_sync() (which holds the compiler), not a workgroup barrier.
    float2 v[8];
    {
        const float2* fr = reinterpret_cast<const float2*>(span + wave * HOP);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float2 x = fr[64 * q + lane];
            v[q] = make_float2(x.x * win[q].x, x.y * win[q].y);
        }
    }
    fft512_888<8>(v, xb, tw512, lane, [&](int k0) { return tw1[k0 - 1]; });

    // ---- 3. split step and magnitudes; the magnitudes overwrite the wave's exchange buffer once every lane has read its bins
    float2 zk[5], zn[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int k = min(lane + 64 * j, HALF / 2);
        zk[j] = xb[k];
        zn[j] = xb[(HALF - k) & (HALF - 1)];
    }
    wave_sync();
    float* mag = reinterpret_cast<float*>(xb);
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int k = lane + 64 * j;
        if (k <= HALF / 2) {
            const float2 e = make_float2(0.5f * (zk[j].x + zn[j].x), 0.5f * (zk[j].y - zn[j].y));
            const float2 o = make_float2(0.5f * (zk[j].y + zn[j].y), -0.5f * (zk[j].x - zn[j].x));
            const float2 t = cmul(tw1024[k], o);
            const float2 p = cadd(e, t), m = csub(e, t);
            mag[k] = sqrtf(p.x * p.x + p.y * p.y + 1e-9f);
            if (k != HALF / 2) mag[NFFT / 2 - k] = sqrtf(m.x * m.x + m.y * m.y + 1e-9f);
        }
    }
    wave_sync();

    // ---- 4./5. mel projection, log, store
    const int t = t0 + wave;
    if (t >= a.t_stride) return;
    const int* band = reinterpret_cast<const int*>(a.blob + OFF_BAND);
    for (int m = lane; m < a.n_mels; m += 64) {
        float acc = 0.0f;
        const int s0 = band[m], n = band[MAX_MELS + m], off = band[2 * MAX_MELS + m];
        for (int i = 0; i < n; ++i) acc = fmaf(spw[off + i], mag[s0 + i], acc);
        const float val = acc > 1e-5f ? logf(acc) : a.floor_log;
        out[(long)t * a.n_mels + m] = t < Tb ? val : a.floor_log;
    }
}

// ---- host side: the tables, in double ------------------------------------------------------------------------------------------
constexpr double F_SP = 200.0 / 3.0, MIN_LOG_HZ = 1000.0, MIN_LOG_MEL = MIN_LOG_HZ / F_SP;
double logstep() { return std::log(6.4) / 27.0; }
double hz_to_mel(double f) { return f >= MIN_LOG_HZ ? MIN_LOG_MEL + std::log(f / MIN_LOG_HZ) / logstep() : f / F_SP; }
double mel_to_hz(double m) { return m >= MIN_LOG_MEL ? MIN_LOG_HZ * std::exp(logstep() * (m - MIN_LOG_MEL)) : F_SP * m; }

// librosa.filters.mel at its defaults (htk=False, norm="slaney"), as this project reads it: n_mels + 2 points equally spaced in
// mel between fmin and fmax, triangles between neighbouring points, each scaled by 2 / (hz[i + 2] - hz[i]).
std::vector<double> slaney_filterbank(const vtts_mel_cfg& c) {
    const int nb = c.n_fft / 2 + 1, nm = c.n_mels;
    std::vector<double> hz(nm + 2), fb((size_t)nm * nb, 0.0);
    const double m0 = hz_to_mel(c.fmin), m1 = hz_to_mel(c.fmax), step = (m1 - m0) / (nm + 1);
    for (int i = 0; i < nm + 2; ++i) hz[i] = mel_to_hz(i == nm + 1 ? m1 : m0 + i * step);  // np.linspace
    for (int i = 0; i < nm; ++i) {
        const double enorm = 2.0 / (hz[i + 2] - hz[i]);
        for (int s = 0; s < nb; ++s) {
            const double f = s * ((double)c.sample_rate / c.n_fft);
            const double lower = -(hz[i] - f) / (hz[i + 1] - hz[i]), upper = (hz[i + 2] - f) / (hz[i + 2] - hz[i + 1]);
            fb[(size_t)i * nb + s] = std::fmax(0.0, std::fmin(lower, upper)) * enorm;
        }
    }
    return fb;
}

}  // namespace

struct vtts_mel {
    vtts_mel_cfg cfg;
    int device = 0;
    std::vector<float> fb;    // [n_mels][513] fp32
    std::vector<float> img;   // the packed blob's host image
    int nnz = 0;
    const float* blob = nullptr;
    vtts::DynLdsOnce lds_f32, lds_pcm;
};

VTTS_API int vtts_mel_create(const vtts_mel_cfg* cfg, int device, vtts_mel** out) {
    if (!cfg || !out) return failf(VTTS_ERR_INVALID, "null argument");
    const vtts_mel_cfg& c = *cfg;
    if (c.n_fft < 8 || (c.n_fft & (c.n_fft - 1))) return failf(VTTS_ERR_INVALID, "n_fft must be a power of two (got %d)", c.n_fft);
    if (c.hop * 4 != c.n_fft) return failf(VTTS_ERR_INVALID, "hop must be n_fft / 4 (got hop %d, n_fft %d)", c.hop, c.n_fft);
    if (c.n_fft != NFFT) return failf(VTTS_ERR_INVALID, "the kernel is built for n_fft = %d, hop = %d (got n_fft %d)", NFFT, HOP, c.n_fft);
    if (c.n_mels < 1 || c.n_mels > MAX_MELS) return failf(VTTS_ERR_INVALID, "n_mels must be in 1 .. %d (got %d)", MAX_MELS, c.n_mels);
    if (c.sample_rate <= 0) return failf(VTTS_ERR_INVALID, "sample_rate must be positive (got %d)", c.sample_rate);
    if (!(c.fmin >= 0.0f) || !(c.fmax > c.fmin) || !(c.fmax <= 0.5f * c.sample_rate))
        return failf(VTTS_ERR_INVALID, "need 0 <= fmin < fmax <= sample_rate / 2 (got fmin %g, fmax %g, sample_rate %d)", c.fmin, c.fmax, c.sample_rate);
    auto* h = new (std::nothrow) vtts_mel();
    if (!h) return failf(VTTS_ERR_NOMEM, "host allocation failed");
    h->cfg = c;
    h->device = device;
    const std::vector<double> fb = slaney_filterbank(c);
    h->fb.assign(fb.begin(), fb.end());  // rounded once
    h->img.assign(BLOB_FLOATS, 0.0f);
    float* img = h->img.data();
    const double pi = 3.14159265358979323846;
    for (int n = 0; n < NFFT; ++n) img[OFF_WIN + n] = (float)(0.5 - 0.5 * std::cos(2.0 * pi * n / NFFT));  // np.hanning(1025)[:-1]
    for (int j = 0; j < HALF; ++j) {
        img[OFF_TW512 + 2 * j] = (float)std::cos(2.0 * pi * j / HALF);
        img[OFF_TW512 + 2 * j + 1] = (float)-std::sin(2.0 * pi * j / HALF);
    }
    for (int k = 0; k <= HALF / 2; ++k) {
        img[OFF_TW1024 + 2 * k] = (float)std::cos(2.0 * pi * k / NFFT);
        img[OFF_TW1024 + 2 * k + 1] = (float)-std::sin(2.0 * pi * k / NFFT);
    }
    int* band = reinterpret_cast<int*>(img + OFF_BAND);
    int nnz = 0;
    for (int m = 0; m < c.n_mels; ++m) {
        const float* row = h->fb.data() + (size_t)m * NBINS;
        int first = -1, last = -1;
        for (int s = 0; s < NBINS; ++s)
            if (row[s] != 0.0f) {
                if (first < 0) first = s;
                last = s;
            }
        const int cnt = first < 0 ? 0 : last - first + 1;
        if (nnz + cnt > MAX_NNZ) {
            delete h;
            return failf(VTTS_ERR_INVALID, "filter bank has more than %d non-zero weights", MAX_NNZ);
        }
        band[m] = first < 0 ? 0 : first;
        band[MAX_MELS + m] = cnt;
        band[2 * MAX_MELS + m] = nnz;
        for (int i = 0; i < cnt; ++i) img[OFF_SPW + nnz + i] = row[first + i];
        nnz += cnt;
    }
    h->nnz = nnz;
    *out = h;
    return VTTS_OK;
}

VTTS_API void vtts_mel_destroy(vtts_mel* h) { delete h; }

VTTS_API int vtts_mel_num_frames(const vtts_mel* h, int64_t n_samples, int64_t* frames) {
    if (!h || !frames) return failf(VTTS_ERR_INVALID, "null argument");
    if (int rc = mf::check_shortest(n_samples)) return rc;
    *frames = mf::num_frames(n_samples);
    return VTTS_OK;
}

VTTS_API int vtts_mel_filterbank(const vtts_mel* h, float* host_out) {
    if (!h || !host_out) return failf(VTTS_ERR_INVALID, "null argument");
    memcpy(host_out, h->fb.data(), h->fb.size() * sizeof(float));
    return VTTS_OK;
}

VTTS_API int vtts_mel_packed_bytes(const vtts_mel* h, size_t* bytes) {
    if (!h || !bytes) return failf(VTTS_ERR_INVALID, "null argument");
    *bytes = h->img.size() * sizeof(float);
    return VTTS_OK;
}

VTTS_API int vtts_mel_pack(vtts_mel* h, void* dev_blob, size_t blob_bytes, void* stream) {
    if (!h) return failf(VTTS_ERR_INVALID, "null argument");
    const size_t need = h->img.size() * sizeof(float);
    if (int rc = check_blob(dev_blob, blob_bytes, need)) return rc;
    if (int rc = upload_blob(dev_blob, h->img.data(), need, static_cast<hipStream_t>(stream), "the mel tables")) return rc;
    h->blob = static_cast<const float*>(dev_blob);
    return VTTS_OK;
}

VTTS_API int vtts_mel_bind_packed(vtts_mel* h, void* dev_blob, size_t blob_bytes) {
    if (!h) return failf(VTTS_ERR_INVALID, "null argument");
    const size_t need = h->img.size() * sizeof(float);
    if (int rc = check_blob(dev_blob, blob_bytes, need)) return rc;
    h->blob = static_cast<const float*>(dev_blob);
    return VTTS_OK;
}

VTTS_API int vtts_mel_workspace_bytes(const vtts_mel* h, int N, int64_t S, size_t* bytes) {
    if (!h || !bytes) return failf(VTTS_ERR_INVALID, "null argument");
    if (N <= 0) return failf(VTTS_ERR_INVALID, "N must be positive (got %d)", N);
    if (int rc = mf::check_shortest(S)) return rc;
    *bytes = 0;  // spectrum and magnitudes live in LDS; the row lengths travel as kernel arguments
    return VTTS_OK;
}

VTTS_API int vtts_mel_forward(vtts_mel* h, const void* wav_dev, int dtype, int N, int64_t S_stride, const int32_t* lengths, float* mel_dev,
                              int64_t T_stride, void* workspace, void* stream) {
    (void)workspace;
    if (!h || !wav_dev || !mel_dev) return failf(VTTS_ERR_INVALID, "null argument");
    if (dtype != VTTS_MEL_F32 && dtype != VTTS_MEL_PCM16) return failf(VTTS_ERR_INVALID, "dtype must be VTTS_MEL_F32 or VTTS_MEL_PCM16 (got %d)", dtype);
    if (!h->blob) return failf(VTTS_ERR_STATE, "forward() before pack()/bind_packed()");
    if (N <= 0) return failf(VTTS_ERR_INVALID, "N must be positive (got %d)", N);
    if (int rc = mf::check_batch(N, S_stride, lengths, T_stride)) return rc;
    const int64_t tiles = (T_stride + FPB - 1) / FPB;
    if (tiles > 0x7fffffff) return failf(VTTS_ERR_SHAPE, "T_stride = %lld is too large", (long long)T_stride);

    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool pcm = dtype == VTTS_MEL_PCM16;
    const size_t esz = pcm ? 2 : 4;
    const void* fn = pcm ? reinterpret_cast<const void*>(&mel_fused_k<short>) : reinterpret_cast<const void*>(&mel_fused_k<float>);
    hipError_t e = vtts::set_max_dynamic_lds(fn, (int)LDS_BYTES, pcm ? h->lds_pcm : h->lds_f32);
    if (e != hipSuccess) return failf(VTTS_ERR_HIP, "hipFuncSetAttribute failed: %s", hipGetErrorString(e));
    MelArgs a;
    a.blob = h->blob;
    a.s_stride = S_stride;
    a.t_stride = T_stride;
    a.n_mels = h->cfg.n_mels;
    a.nnz = h->nnz;
    a.vec_ok = reinterpret_cast<uintptr_t>(wav_dev) % 16 == 0 && (S_stride * esz) % 16 == 0;
    a.floor_log = (float)std::log(1e-5);
    return vtts_rows::for_each_launch<ROWS_PER_LAUNCH>(N, lengths, S_stride, [&](int r0, int nr, const Rows& rows) -> int {
        a.wav = static_cast<const char*>(wav_dev) + (size_t)r0 * S_stride * esz;
        a.mel = mel_dev + (size_t)r0 * T_stride * h->cfg.n_mels;
        const dim3 grid((unsigned)tiles, (unsigned)nr);
        if (pcm)
            hipLaunchKernelGGL(mel_fused_k<short>, grid, dim3(THREADS), LDS_BYTES, s, a, rows);
        else
            hipLaunchKernelGGL(mel_fused_k<float>, grid, dim3(THREADS), LDS_BYTES, s, a, rows);
        e = hipGetLastError();
        if (e != hipSuccess) return failf(VTTS_ERR_HIP, "mel kernel launch failed: %s", hipGetErrorString(e));
        return VTTS_OK;
    });
}
