// What one wave does with its 64 lanes, stated once for every stage that keeps a frame (or a chunk of a row) in one wave.
#pragma once

#include <hip/hip_runtime.h>

namespace vtts_wave {

// Orders a wave's LDS writes before its later LDS reads of other lanes' data.  No instruction: the hardware keeps one wave's LDS
// accesses in order; this only keeps the compiler from moving them across.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the halvings h = 32 .. 1 of the public headers (every lane ends with lane 0's bits: each step adds the same two numbers on both sides)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

}  // namespace vtts_wave
