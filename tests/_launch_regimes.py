"""Launch geometry of the HIP kernels, restated for tests/test_gpu_launch_regimes.py (no torch, no GPU).

Every kernel family switches code paths on the size of a launch: a wider time tile, an XCD-aware tile order with a padded grid, a staged
epilogue.  The module tests of the other files run at B = 2 and L <= 1203, where every launch takes the small-launch path.  The GPU tests compute
their lengths from the numbers below so that they sit inside, or exactly on the edges of, the large-launch paths.
tests/test_launch_regime_table_cpu.py reads the same numbers out of viettts_amd/csrc/*.hip and fails when a source moves one: a moved threshold
would otherwise leave the GPU tests quietly exercising the small-launch path again.
"""
from __future__ import annotations

XCDS = 8  # the launchers pad gridDim.x to a multiple of this when the XCD-aware order is on

# ---- thresholds (name -> value) -------------------------------------------------------------------------------------------
THRESHOLDS = {
    "G_MIN_WGS": 384,            # kernels_bf16_rbg.hip: wide bf16 pair tile from this many wide-tile workgroups (tiles per row * B)
    "XCD_MAP_MIN_TILES": 192,    # kernels_bf16_rbg.hip: XCD order of resblock_pair_g_bf16_k from this many tiles per utterance slot
    "RB_BF16_XCD_MIN": 192,      # kernels_bf16_rbk.hip: XCD order of resblock_bf16_k from this many windows (a literal there)
    # the next four: device_common.h's XCD_MIN_TILES, named here by the kernel that applies it
    "F32_XCD_MIN_TILES": 64,     # kernels_f32_mfma.hip: XCD order of conv1d_f32_mfma_k from this many time tiles per grid row
    "F32_MIN_WGS": 384,          # kernels_f32_mfma.hip: launch_conv1d_f32_mfma's MIN_WGS, wide tile from this many wide-tile workgroups
    "FP_XCD_MIN_TILES": 64,      # kernels_f32_pair.hip: XCD order of resblock_pair_f32_k
    "X3_XCD_MIN_TILES": 64,      # kernels_x3.hip: XCD order of resblock_pair_x3_k
    "RX_XCD_MIN_TILES": 64,      # kernels_x3_rb.hip: XCD order of resblock_x3_k
}

# ---- tile sizes ----------------------------------------------------------------------------------------------------------------------------
# bf16 pair (kernels_bf16_rbg.hip, GTile N1: time rows per workgroup; outputs per workgroup NT2 = N1 - (k - 1))
BF16_PAIR_N1_WIDE = {256: {3: 128, 7: 128, 11: 128}, 128: {3: 256, 7: 256, 11: 256}, 64: {3: 512, 7: 512, 11: 512}, 32: {3: 512, 7: 512, 11: 512}}
BF16_PAIR_N1_NARROW = {256: 64, 128: 128, 64: 256, 32: 256}
# fp32 convolution (kernels_f32_mfma.hip, ConvTile NT: time columns per workgroup, MT: output channels per workgroup)
F32_CONV_NT_WIDE = {256: 128, 128: 128, 64: 64, 32: 128}
F32_CONV_NT_NARROW = {256: 32, 128: 64, 64: 64, 32: 128}
F32_CONV_MT = {256: 128, 128: 128, 64: 64, 32: 32}
# launch_conv1d_f32_mfma's narrow(NT, mtiles): the wide/narrow decision counts workgroups with these, not with the tile's own NT
F32_CONV_DECISION = {256: (128, 2), 128: (128, 1), 64: (128, 1), 32: (256, 1)}
# fp32 pair (kernels_f32_pair.hip, F32PairTile N1)
F32_PAIR_N1 = {128: 128, 64: 256, 32: 256}
# bf16x3 pair (kernels_x3.hip, XTile N1; C = 128 and C = 32 pick a geometry by k)
X3_PAIR_N1 = {256: {3: 128, 7: 128, 11: 128}, 128: {3: 128, 7: 256, 11: 256}, 64: {3: 256, 7: 256, 11: 256}, 32: {3: 512, 7: 512, 11: 512}}
# whole-ResBlock windows W (kernels_bf16_rbk.hip RBTile, kernels_x3_rb.hip RXTile); outputs per window NT = W - 2 H (d0 + d1 + d2 + 3), H = (k - 1) / 2
BF16_RB_W = {32: {3: 256, 7: 512, 11: 512}, 64: {3: 256}, 128: {3: 128}}
X3_RB_W = {32: {3: 512, 7: 512, 11: 512}, 64: {3: 256, 7: 256}, 128: {3: 128}}
# bf16x3 transposed convolutions (kernels_x3.hip, UXTile N1: input frames per workgroup)
X3_UPS_N1 = {0: 64, 1: 128, 2: 256, 3: 512}


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


def bf16_pair_nt2(C: int, k: int, narrow: bool) -> int:
    return (BF16_PAIR_N1_NARROW[C] if narrow else BF16_PAIR_N1_WIDE[C][k]) - (k - 1)


def bf16_pair_wide(C: int, L: int, B: int, tiles: int = 0) -> bool:
    """launch_pair_g_bf16 (tiles: 1 forces the wide tile, 2 the narrow one).  The decision counts tiles of the k = 11 wide tile, whatever k is."""
    if tiles:
        return tiles == 1
    return cdiv(L, bf16_pair_nt2(C, 11, False)) * B >= THRESHOLDS["G_MIN_WGS"]


def bf16_pair_tiles(C: int, k: int, L: int, B: int, tiles: int = 0) -> int:
    """tiles per utterance slot of the launched tile (the XCD order is on from XCD_MAP_MIN_TILES of them)"""
    return cdiv(L, bf16_pair_nt2(C, k, not bf16_pair_wide(C, L, B, tiles)))


def f32_conv_wide(C: int, L: int, B: int, tiles: int = 0) -> bool:
    if tiles:
        return tiles == 1
    nt, mtiles = F32_CONV_DECISION[C]
    return cdiv(L, nt) * mtiles * B >= THRESHOLDS["F32_MIN_WGS"]


def f32_conv_tiles(C: int, L: int, B: int, tiles: int = 0) -> int:
    return cdiv(L, (F32_CONV_NT_WIDE if f32_conv_wide(C, L, B, tiles) else F32_CONV_NT_NARROW)[C])


def f32_pair_tiles(C: int, k: int, L: int) -> int:
    return cdiv(L, F32_PAIR_N1[C] - (k - 1))


def x3_pair_tiles(C: int, k: int, L: int) -> int:
    return cdiv(L, X3_PAIR_N1[C][k] - (k - 1))


def rb_margin(k: int, dils=(1, 3, 5)) -> int:
    """M = H (d0 + d1 + d2) + 3 H: the rows per window side whose dependency cone left the window after the three pairs (H = (k - 1) / 2)"""
    h = (k - 1) // 2
    return h * sum(dils) + 3 * h


def rb_window_nt(W: int, k: int, dils=(1, 3, 5)) -> int:
    return W - 2 * rb_margin(k, dils)


def length_for_tiles(n: int, nt: int, mult: int = 1) -> int:
    """A length of exactly n tiles of nt outputs whose last tile is partial (about half full), rounded down to a multiple of `mult`."""
    L = (n - 1) * nt + nt // 2
    L -= L % mult
    assert cdiv(L, nt) == n and L % nt != 0, (n, nt, mult, L)
    return L
