// Device helpers the limiter's kernels share (limiter.hip, limiter_stream.hip): the taps' argument, the sample conversions, the gain a
// sample asks for and the padded LDS index of the mean.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/vtts_limiter.h"

namespace vtts_limiter_dev {

constexpr int KP = VTTS_LIMITER_PHASE_TAPS;
constexpr int OS = VTTS_LIMITER_OVERSAMPLE;
constexpr int LEAD = 27;  // x[n - LEAD] meets a phase's first tap

struct LimTaps {
    float t[OS][KP];
};

__device__ __forceinline__ float to_float(float v) { return v; }
__device__ __forceinline__ float to_float(short v) { return (float)v * (1.0f / 32768.0f); }

template <typename TO>
__device__ __forceinline__ TO from_float(float v);
template <>
__device__ __forceinline__ float from_float<float>(float v) {
    return v;
}
// audio.hip's rule (viettts_amd/wavio.py float_to_pcm16): rint(clip(x, -1, 1) * 32767) in double, NaN -> 0
template <>
__device__ __forceinline__ short from_float<short>(float v) {
    if (!(v == v)) return 0;
    const float c = fminf(fmaxf(v, -1.0f), 1.0f);
    return (short)(int)rint((double)c * 32767.0);
}

__device__ __forceinline__ float req_of(float p, float g, float c) {
    const float gp = g * p;
    return gp <= c ? 1.0f : c / gp;
}

// held[j] lives at word j + j / 16, so that 64 lanes walking 16 words apart meet 64 banks
__device__ __forceinline__ int padded(int j) { return j + (j >> 4); }

}  // namespace vtts_limiter_dev
