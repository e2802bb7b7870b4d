// Device helpers the resampler's kernels share (audio.hip, resample_stream.hip): the outputs of one staged span, i.e. the slot -> output
// -> phase arithmetic and the one fp32 fmaf chain per output (include/vtts_audio.h).  The sample conversions are sample_convert.h's.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/vtts_audio.h"
#include "sample_convert.h"

namespace vtts_audio_dev {

using vtts_sample::from_float;
using vtts_sample::to_float;

// floor(a / 8) * 8, a may be negative
__device__ __forceinline__ long long floor8(long long a) { return a & ~7LL; }

// The table's shape and the ratio, as the kernels carry them.
struct Phases {
    const float* table;  // [kp4 / 4][L][4]
    int L, M, kp4;
    int minv;  // M^-1 mod L
};

// out[0 .. cnt) of a block whose first output has phase p0 and reads span[sbase .. sbase + kp4): one fmaf chain per output, ascending n;
// outputs live .. cnt - 1 are zero.  The lanes take consecutive PHASES: inside each run of L outputs, slot s computes output
// s M^-1 mod L, whose phase is p0 + s.  Which lane computes an output changes nothing in its chain.
template <typename TO>
__device__ __forceinline__ void span_outputs(const Phases& a, const float* span, int sbase, int p0, int cnt, int live, TO* out, int tid,
                                             int threads) {
    const int nq = a.kp4 >> 2;
    const int nslots = (cnt + a.L - 1) / a.L * a.L;  // whole runs of L outputs: < OUT_PER_BLOCK + L
    for (int slot = tid; slot < nslots; slot += threads) {
        const int run = slot / a.L, sl = slot - run * a.L;
        const int i = run * a.L + sl * a.minv % a.L;  // sl * minv < 2048^2
        if (i >= cnt) continue;
        float acc = 0.0f;
        if (i < live) {
            const int p = p0 + sl < a.L ? p0 + sl : p0 + sl - a.L;  // = (p0 + i M) mod L
            const int dq = (p0 + i * a.M) / a.L;                     // p0 + i M < L + OUT_PER_BLOCK * M <= 2049 * 2048
            const float* s = span + sbase + dq;
            const float4* g = reinterpret_cast<const float4*>(a.table) + p;
            for (int c = 0; c < nq; ++c) {
                const float4 w = g[(size_t)c * a.L];
                acc = fmaf(s[4 * c + 0], w.x, acc);
                acc = fmaf(s[4 * c + 1], w.y, acc);
                acc = fmaf(s[4 * c + 2], w.z, acc);
                acc = fmaf(s[4 * c + 3], w.w, acc);
            }
        }
        out[i] = from_float<TO>(acc);
    }
}

}  // namespace vtts_audio_dev
