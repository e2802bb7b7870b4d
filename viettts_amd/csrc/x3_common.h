// Device primitives shared by the split-operand ("bf16x3") kernels: kernels_x3.hip (ResBlock pair, transposed convolutions, conv_pre) and
// kernels_x3_rb.hip (whole ResBlock).
//
// The contract.  resblock_x3_k promises the BITS of three launches of resblock_pair_x3_k
// (tests/test_gpu_x3.py::test_x3_whole_resblock_equals_the_pair_path), and every parity test of the split engine leans on that.  fp32 sums are
// not associative, so the promise holds only while both kernels perform the same operations in the same order on every output element.  What
// they must agree on is defined once, here and in the two headers below, and both kernels call it:
//   * the split (bf16_common.h: split2): v = v0 + v1, v0 = bf16(v), v1 = bf16(v - v0), round-to-nearest-even; the host packers split the
//     weights the same way (vtts_internal.h: split_bf16);
//   * the term order (x3_mma): per k-step  a1 b0, then a0 b1, then a0 b0  ("small terms first"; the dropped a1 b1 is 2^-18 of the product),
//     each term over all of the wave's blocks before the next; a block's very first MFMA may take the bias as its C operand — the accumulators
//     start from the bias in both kernels, no epilogue adds one;
//   * the exchange layout (put_block_split, on bf16_common.h: swap_pair): how a lane's accumulator values become 16-byte slots of a
//     channels-last tile row, i.e. which channel a B fragment of the next convolution finds where;
//   * the accumulator-row-to-channel map (device_common.h: acc_row) and the MRF arithmetic of the stores (device_common.h: mrf_combine).
// What differs on purpose stays in the kernels: loops, rings, look-ahead depths, chunk orders, epilogue structure.  The k-step ORDER of a sum
// (tap-major; chunk-major for a c1 pass staged in channel chunks) is the kernels' own and must match too: RXTile::KSX1 mirrors XTile::XC.
#pragma once

#include "bf16_common.h"
#include "device_common.h"

namespace vtts {

// One k-step of a wave's MR x NR blocks: acc += a (*) b from three bf16 products, a / b = [block][plane: 0 = hi, 1 = lo] fragments.
// c0 (optional): MR blocks that replace the accumulators as the C operand of the first term — a sum's very first step.
// MR * NR independent accumulators lie between two MFMAs on the same one.
template <int MR, int NR>
__device__ __forceinline__ void x3_mma(f32x16 (&acc)[MR][NR], const bf16x8 (&a)[MR][2], const bf16x8 (&b)[NR][2], const f32x16* c0 = nullptr) {
#pragma unroll
    for (int mr = 0; mr < MR; ++mr)
#pragma unroll
        for (int nr = 0; nr < NR; ++nr) acc[mr][nr] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mr][1], b[nr][0], c0 ? c0[mr] : acc[mr][nr], 0, 0, 0);
#pragma unroll
    for (int mr = 0; mr < MR; ++mr)
#pragma unroll
        for (int nr = 0; nr < NR; ++nr) acc[mr][nr] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mr][0], b[nr][1], acc[mr][nr], 0, 0, 0);
#pragma unroll
    for (int mr = 0; mr < MR; ++mr)
#pragma unroll
        for (int nr = 0; nr < NR; ++nr) acc[mr][nr] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mr][0], b[nr][0], acc[mr][nr], 0, 0, 0);
}

// One 16-channel half p of a 32 x 32 accumulator block -> tile row `row` of the hi / lo planes: v = this lane's 8 values (registers 8p .. 8p+7 of
// the block: column l31, channels 16p + 8 rq' + 4 lh + i), already biased / activated / masked.  Split, exchange across the wave halves — then
// lh = 0 holds channels 16p .. 16p+7 and lh = 1 holds 16p+8 .. 16p+15 — and one 16-byte write per plane; slot = (first channel of the half >> 3) + lh.
template <int SPR>
__device__ __forceinline__ void put_block_split(unsigned char* thi, unsigned char* tlo, int row, int slot, const float* v) {
    unsigned hp0, hp1, hq0, hq1, lp0, lp1, lq0, lq1;
    split2(v[0], v[1], hp0, lp0);
    split2(v[2], v[3], hp1, lp1);
    split2(v[4], v[5], hq0, lq0);
    split2(v[6], v[7], hq1, lq1);
    swap_pair(hp0, hq0);
    swap_pair(hp1, hq1);
    swap_pair(lp0, lq0);
    swap_pair(lp1, lq1);
    const int off = tile_off<SPR>(row, slot);
    *reinterpret_cast<uint4*>(thi + off) = make_uint4(hp0, hp1, hq0, hq1);
    *reinterpret_cast<uint4*>(tlo + off) = make_uint4(lp0, lp1, lq0, lq1);
}

}  // namespace vtts
