// The sample formats of every waveform stage, stated once: PCM16 in is scaled by 2^-15 (exact), PCM16 out follows one rounding rule.
#pragma once

#include <hip/hip_runtime.h>

namespace vtts_sample {

__device__ __forceinline__ float to_float(float v) { return v; }
__device__ __forceinline__ float to_float(short v) { return (float)v * (1.0f / 32768.0f); }
// The same bits with an exponent add in place of the multiply, for the short-time stages (stft_front.h): their staging converts two samples
// side by side, and the compiler pairs two such multiplies into a v_pk_mul_f32, which no kernel of this library may hold (build.py).
__device__ __forceinline__ float to_float_exact_shift(float v) { return v; }
__device__ __forceinline__ float to_float_exact_shift(short v) { return ldexpf((float)v, -15); }

template <typename TO>
__device__ __forceinline__ TO from_float(float v);
template <>
__device__ __forceinline__ float from_float<float>(float v) {
    return v;
}
// viettts_amd/wavio.py float_to_pcm16: rint(clip(x, -1, 1) * 32767) in double, NaN -> 0.  The product of a 24-bit and a 15-bit significand
// is exact in double, so the only rounding is rint's (to nearest, ties to even).
template <>
__device__ __forceinline__ short from_float<short>(float v) {
    if (!(v == v)) return 0;
    const float c = fminf(fmaxf(v, -1.0f), 1.0f);
    return (short)(int)rint((double)c * 32767.0);
}

}  // namespace vtts_sample
