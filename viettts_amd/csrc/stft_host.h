// The host side that the short-time stages with a free resolution share (spectral.hip, stft.hip, denoise.hip): what a resolution may be, the
// tables it needs and their packed blob, the LDS of a workgroup of F frames and the choice of a kernel instance by n_fft (launch_rows.h: the rows).
#pragma once

#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../include/vtts_hifigan.h"
#include "../../include/vtts_spectral.h"
#include "stockham.h"
#include "vtts_internal.h"

namespace vtts_stft_host {

using vtts::failf;
using vtts_stockham::pad8;

constexpr int MAX_F = VTTS_SPECTRAL_MAX_FRAMES_PER_BLOCK;
constexpr int even(int n) { return (n + 1) & ~1; }

// LDS of one forward workgroup of F frames, in bytes, in the order of vtts_spectral.h's table (and of the kernels' carve-up): `reduce` bytes
// per frame of reduction area, twH, twN, the staged span of each of `signals` signals, the F exchange buffers.
inline size_t frames_lds_bytes(int n_fft, int hop, int F, int signals, int reduce) {
    const int H = n_fft / 2;
    return (size_t)reduce * F + (size_t)8 * H + (size_t)8 * (H / 2 + 2) + (size_t)signals * 4 * even((F - 1) * hop + n_fft) + (size_t)8 * F * pad8(H);
}
// the largest count <= 8 (4 at n_fft = 2048) whose LDS fits the budget
inline int frames_per_block(int n_fft, int hop, int signals, int reduce) {
    int F = n_fft == 2048 ? VTTS_SPECTRAL_MAX_FRAMES_PER_BLOCK_2048 : MAX_F;
    while (F > 1 && frames_lds_bytes(n_fft, hop, F, signals, reduce) > VTTS_SPECTRAL_LDS_BUDGET) --F;
    return F;
}

inline int check_resolution(int n_fft, int hop, int win) {
    if (n_fft != 256 && n_fft != 512 && n_fft != 1024 && n_fft != 2048) return failf(VTTS_ERR_INVALID, "n_fft must be 256, 512, 1024 or 2048 (got %d)", n_fft);
    if (hop < 1 || win < hop || win > n_fft) return failf(VTTS_ERR_INVALID, "need 1 <= hop <= win <= n_fft (got hop %d, win %d, n_fft %d)", hop, win, n_fft);
    return VTTS_OK;
}

// fn(std::integral_constant<int, n_fft>) for the n_fft check_resolution() let through
template <typename Fn>
auto by_nfft(int n_fft, const Fn& fn) {
    return n_fft == 256    ? fn(std::integral_constant<int, 256>())
           : n_fft == 512  ? fn(std::integral_constant<int, 512>())
           : n_fft == 1024 ? fn(std::integral_constant<int, 1024>())
                           : fn(std::integral_constant<int, 2048>());
}

// The tables of one resolution and the device blob that holds them; a handle derives from it.
struct Tables {
    std::vector<float> img;  // the packed blob's host image: window [n_fft] | twH [H] complex | twN [H / 2 + 1] complex, padded to H / 2 + 2
    const float* blob = nullptr;

    // vtts_spectral.h's tables: computed in double, rounded once
    void build(int n, int win) {
        const int H = n / 2, lead = (n - win) / 2;
        img.assign((size_t)n + 2 * H + 2 * (H / 2 + 2), 0.0f);
        const double pi = 3.14159265358979323846;
        float* w = img.data();
        float* twH = w + n;
        float* twN = twH + 2 * H;
        for (int r = 0; r < win; ++r) w[lead + r] = (float)(0.5 - 0.5 * std::cos(2.0 * pi * r / win));
        for (int m = 0; m < H; ++m) {
            twH[2 * m] = (float)std::cos(2.0 * pi * m / H);
            twH[2 * m + 1] = (float)-std::sin(2.0 * pi * m / H);
        }
        for (int k = 0; k <= H / 2; ++k) {
            twN[2 * k] = (float)std::cos(2.0 * pi * k / n);
            twN[2 * k + 1] = (float)-std::sin(2.0 * pi * k / n);
        }
    }
    size_t bytes() const { return img.size() * sizeof(float); }
};

// the bodies of vtts_{spectral,stft}_{window,packed_bytes,pack,bind_packed}
inline int window(const Tables* t, int n_fft, float* host_out) {
    if (!t || !host_out) return failf(VTTS_ERR_INVALID, "null argument");
    memcpy(host_out, t->img.data(), (size_t)n_fft * sizeof(float));
    return VTTS_OK;
}
inline int packed_bytes(const Tables* t, size_t* bytes) {
    if (!t || !bytes) return failf(VTTS_ERR_INVALID, "null argument");
    *bytes = t->bytes();
    return VTTS_OK;
}
inline int bind_packed(Tables* t, void* dev_blob, size_t blob_bytes) {
    if (!t) return failf(VTTS_ERR_INVALID, "null argument");
    if (int rc = vtts::check_blob(dev_blob, blob_bytes, t->bytes())) return rc;
    t->blob = static_cast<const float*>(dev_blob);
    return VTTS_OK;
}
inline int pack(Tables* t, void* dev_blob, size_t blob_bytes, void* stream, const char* what) {
    if (!t) return failf(VTTS_ERR_INVALID, "null argument");
    if (int rc = vtts::check_blob(dev_blob, blob_bytes, t->bytes())) return rc;
    if (int rc = vtts::upload_blob(dev_blob, t->img.data(), t->bytes(), static_cast<hipStream_t>(stream), what)) return rc;
    t->blob = static_cast<const float*>(dev_blob);
    return VTTS_OK;
}

}  // namespace vtts_stft_host
