// Device-side helpers shared by all kernels (gfx950).
#pragma once

#include "vtts_internal.h"

namespace vtts {

__device__ __forceinline__ float lrelu(float v, float slope) {
    // jax.nn.leaky_relu / F.leaky_relu: where(x >= 0, x, slope * x)  (model.py:46,48,112,122)
    return v >= 0.0f ? v : v * slope;
}

// Valid input length of utterance b (ragged batches: ConvArgs::lens; clamped into the slot, so a bad count never leaves it) — a.L otherwise.
__device__ __forceinline__ int valid_len(const ConvArgs& a, int b) {
    return a.lens ? min(max(a.lens[b], 0) * a.len_mul, a.L) : a.L;
}
// Four consecutive columns t .. t + 3 loaded as one float4 from a row whose valid length L is not a multiple of 4 (a ragged utterance's
// conv_pre output): the columns past L read as zero (select, not multiply: the slot's tail holds whatever the last pass left there).
__device__ __forceinline__ float4 mask_tail4(float4 v, int t, int L) {
    if (t + 1 >= L) v.y = 0.0f;
    if (t + 2 >= L) v.z = 0.0f;
    if (t + 3 >= L) v.w = 0.0f;
    return v;
}

// C/D layout of the 32 x 32 MFMAs: accumulator register r of a lane in wave half lh = lane >> 5 is row (channel) base + (r & 3) + 8 * (r >> 2) + 4 * lh
// of the block whose first row is base; the column (time) is lane & 31.  (base is a parameter because the sum is formed in this order: the
// kernels' address arithmetic was compiled from it, and hipcc does not reassociate it to the same code.)
__device__ __forceinline__ constexpr int acc_row(int r, int lh, int base) { return base + (r & 3) + 8 * (r >> 2) + 4 * lh; }

// XCD-aware tile order of the kernels whose workgroup is a time tile of NT outputs: workgroups go to the 8 XCDs round-robin in launch order, so
// on launches of at least XCD_MIN_TILES tiles per grid row (xcd_grid_x pads gridDim.x to whole rounds of the 8 XCDs; workgroup (x, y, z) then runs
// on XCD x % 8) XCD blockIdx.x % 8 takes a contiguous, balanced eighth of the utterance's tiles: a tile's halo columns were staged by the same
// L2's previous tile.  False: this workgroup has no tile (the padding of its eighth).
constexpr int XCD_MIN_TILES = 64;
__device__ __forceinline__ bool xcd_tile(int L, int NT, int& tile) {
    tile = blockIdx.x;
    if (gridDim.x >= XCD_MIN_TILES) {
        const int nt = (L + NT - 1) / NT, r = (int)((blockIdx.x + blockIdx.z) & 7), lo = (r * nt) >> 3, hi = ((r + 1) * nt) >> 3;
        tile = lo + (int)(blockIdx.x >> 3);
        if (tile >= hi) return false;
    }
    return true;
}
inline unsigned xcd_grid_x(int tiles) { return tiles >= XCD_MIN_TILES ? (tiles + 7) / 8 * 8 : tiles; }

// Combine a finished convolution value with memory according to ConvArgs::acc_mode and store it.
// `v` already holds acc + bias.  Order of operations follows the reference:
//   residual   xt + x            (model.py:50)
//   MRF        xs += rb(x)       (model.py:118-120), x = xs / num_kernels (model.py:121)
//   tail       tanh(conv_post)   (model.py:123-124)
__device__ __forceinline__ void epilogue_store(const ConvArgs& a, long idx, float v) {
    if (a.res) v = v + a.res[idx];
    if (a.acc_mode == ACC_ADD) {
        v = a.y[idx] + v;
    } else if (a.acc_mode == ACC_MEAN) {
        v = (a.y[idx] + v) / a.div;
    }
    if (a.tanh_out) {
        if (a.pre_act) a.pre_act[idx] = v;
        v = tanhf(v);
    }
    a.y[idx] = v;
}

}  // namespace vtts
