// The row rule of the mel framing (1024-point frames every 256 samples, 384 reflected samples on each side), stated once for mel.hip and
// pitch.hip: the shortest row, the frames of a row, and forward()'s check of the rows' pitch, lengths and output pitch.
#pragma once

#include "../../include/vtts_mel.h"
#include "vtts_internal.h"

namespace vtts_mel_framing {

constexpr int NFFT = 1024, HOP = 256, PADL = (NFFT - HOP) / 2, MIN_SAMPLES = VTTS_MEL_MIN_SAMPLES;

inline int64_t num_frames(int64_t n_samples) { return (n_samples + 2 * PADL - NFFT) / HOP + 1; }

// a row must hold its own reflection: `what` names the argument in forward()'s refusal ("S_stride "), "" elsewhere
inline int check_shortest(int64_t n_samples, const char* what = "") {
    if (n_samples >= MIN_SAMPLES) return VTTS_OK;
    return vtts::failf(VTTS_ERR_SHAPE, "a row needs at least %d samples for its reflection padding (got %s%lld)", MIN_SAMPLES, what, (long long)n_samples);
}

// forward(): S_stride, every row's length and T_stride against the longest row's frames (t_max)
inline int check_batch(int N, int64_t S_stride, const int32_t* lengths, int64_t T_stride) {
    if (int rc = check_shortest(S_stride, "S_stride ")) return rc;
    if (S_stride > 0x7fffffff - 2 * NFFT) return vtts::failf(VTTS_ERR_SHAPE, "rows of 2^31 samples are not supported (got S_stride %lld)", (long long)S_stride);
    int64_t t_max = 0;
    for (int b = 0; b < N; ++b) {
        const int64_t len = lengths ? lengths[b] : S_stride;
        if (len < MIN_SAMPLES || len > S_stride)
            return vtts::failf(VTTS_ERR_SHAPE, "lengths[%d] = %lld is outside %d .. S_stride = %lld", b, (long long)len, MIN_SAMPLES, (long long)S_stride);
        if (num_frames(len) > t_max) t_max = num_frames(len);
    }
    if (T_stride < t_max) return vtts::failf(VTTS_ERR_SHAPE, "T_stride = %lld is below the longest row's %lld frames", (long long)T_stride, (long long)t_max);
    return VTTS_OK;
}

}  // namespace vtts_mel_framing
