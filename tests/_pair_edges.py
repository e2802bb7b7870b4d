"""Tile-edge lengths, ragged cases, references and bars for the fp32 and bf16x3 pair kernels and the fp32 per-convolution launches (numpy only).

The kernels under test — resblock_pair_f32_k (kernels_f32_pair.hip), resblock_pair_x3_k (kernels_x3.hip), conv1d_f32_mfma_k
(kernels_f32_mfma.hip) and the generic fallback — mask and clamp in four places: a tile past the utterance's end exits (``t0 >= L``), the staging
zero-fills outside ``[0, L)`` (float4 loads with ``mask_tail4`` and a clamped address where the valid length is no multiple of 4), epilogue 1
zero-pads xt (``tt < 0 || tt >= L``) and epilogue 2 masks its stores (``n < NT2 && t < L``).  ``pair_edge_lengths`` / ``conv_edge_lengths`` are
the lengths at which those conditions flip in the first, the second and the last tile; ``*_conditions`` restate them so that
tests/test_pair_edges_cpu.py can show that the lengths reach every one of them, both ways.

Bars (nothing taken from a kernel):
  fp32    max|got - ref64| <= 4 e32 + 2^-22 max|ref64| per utterance, e32 = the class-wide largest error of numpy's float32 run of the same
          reference and of the single-chain fp32 restatement below (the rule of tests/test_gpu_gta.py::_bar and tests/_nat_dims.py: bar);
  bf16x3  max|got - ref64| / max|ref64| < 5e-5 over a launch (X3_BOUND of tests/test_gpu_x3.py).
"""
from __future__ import annotations

import numpy as np

import _bf16_rb_ref as RB
import _launch_regimes as R

SENTINEL = 1536.0
X3_BOUND = 5e-5
CLASSES = [(C, k) for C in (256, 128, 64, 32) for k in (3, 7, 11)]
F32_PAIR_CLASSES = [(C, k) for C, k in CLASSES if C in R.F32_PAIR_N1]
MAX_DIL = 5
RATES = (1, 3, 5)
PARAM_SEED = 4321


def roundup4(v: int) -> int:
    return (v + 3) & ~3


# ---- geometry -------------------------------------------------------------------------------------------------------------------------------
def pair_geometry(engine: str, C: int, k: int):
    """(N1, H, NT2, R, PA) of the pair kernel of ``engine`` ("f32": F32PairTile, "x3": XTile): N1 columns of c1 per workgroup, H = (k - 1) / 2,
    NT2 = N1 - 2 H outputs, R = 6 H a pair's reach at rate 5, PA = roundup4(5 H) the per-convolution kernel's staged halo"""
    N1 = R.F32_PAIR_N1[C] if engine == "f32" else R.X3_PAIR_N1[C][k]
    H = (k - 1) // 2
    return N1, H, N1 - 2 * H, 6 * H, roundup4(MAX_DIL * H)


def conv_nt(C: int, narrow: bool) -> int:
    return (R.F32_CONV_NT_NARROW if narrow else R.F32_CONV_NT_WIDE)[C]


def pair_edge_lengths(H: int, NT2: int):
    R_ = 6 * H
    out = [1, 2, 3, 4, 5, H + 1, 2 * H, 2 * H + 1, R_, R_ + 1, NT2 - R_, NT2 - H - 1, NT2 - H, NT2 - 1, NT2, NT2 + 1, NT2 + H, NT2 + H + 1, NT2 + R_,
           NT2 + R_ + 1, 2 * NT2 - 1, 2 * NT2, 2 * NT2 + 1, 2 * NT2 + R_, 3 * NT2 + 5]
    return sorted({v for v in out if v >= 1})


def conv_edge_lengths(H: int, NT: int):
    out = [1, 2, 3, 4, 5, 5 * H, 5 * H + 1, NT - 1, NT, NT + 1, NT + 5 * H, NT + 5 * H + 1, 2 * NT, 2 * NT + 1, 3 * NT + 5]
    return sorted({v for v in out if v >= 1})


def conv_route_lengths(C: int, k: int):
    """the per-convolution launches' lengths: the pair edges of the engines' pair tiles and the edges of the wide and the narrow ConvTile"""
    H = (k - 1) // 2
    out = set()
    for engine in ("f32", "x3"):
        if engine == "x3" or C in R.F32_PAIR_N1:
            out |= set(pair_edge_lengths(H, pair_geometry(engine, C, k)[2]))
    for narrow in (False, True):
        out |= set(conv_edge_lengths(H, conv_nt(C, narrow)))
    return sorted(out)


# ---- the kernels' conditions, restated --------------------------------------------------------------------------------------------------------
def _stage4(t, L, LP):
    """one float4 staging unit at time t (a multiple of 4): 'lo' / 'hi' = zero-filled whole, 'partial' = mask_tail4 zeroes 1 .. 3 lanes,
    'in' = all four lanes valid; and whether the load address is clamped (resblock_pair_f32_k: t >= LP ? LP - 4 : t)"""
    kind = "lo" if t < 0 else "hi" if t >= L else "partial" if t + 3 >= L else "in"
    return kind, t >= LP


def f32_pair_conditions(N1, H, L, LP, tile, dil):
    """resblock_pair_f32_k, one workgroup: (exits, staging kinds, {address clamped?} per unit, xt kinds, store kinds)"""
    NT2 = N1 - 2 * H
    t0 = tile * NT2
    if t0 >= L:
        return True, set(), set(), set(), set()
    tstart = t0 - H - H * dil
    tx0 = tstart - tstart % 4
    w4 = (N1 + 2 * H * dil + 3 + 3) // 4
    st = [_stage4(tx0 + 4 * c4, L, LP) for c4 in range(w4)]
    xt = {"lo" if t0 - H + n < 0 else "hi" if t0 - H + n >= L else "in" for n in range(N1)}
    store = {(n < NT2, t0 + n < L) for n in range(N1)}
    return False, {s[0] for s in st}, {s[1] for s in st}, xt, store


def x3_pair_conditions(N1, H, L, LP, tile, dil):
    """resblock_pair_x3_k: the staging is per row (no float4: no partial units; the address is clamped to L - 1)"""
    NT2 = N1 - 2 * H
    t0 = tile * NT2
    if t0 >= L:
        return True, set(), set(), set(), set()
    tx0 = t0 - H - H * dil
    ts = [tx0 + r for r in range(N1 + 2 * H * dil)]
    st = {"lo" if t < 0 else "hi" if t >= L else "in" for t in ts}
    xt = {"lo" if t0 - H + n < 0 else "hi" if t0 - H + n >= L else "in" for n in range(N1)}
    store = {(n < NT2, t0 + n < L) for n in range(N1)}
    return False, st, {t >= L for t in ts}, xt, store


def conv_conditions(NT, PA, L, LP, tile):
    """conv1d_f32_mfma_k: staging t = t0 - PA + 4 c4 (no clamp: a unit outside [0, L) is not loaded), no xt, stores t < L"""
    t0 = tile * NT
    if t0 >= L:
        return True, set(), set(), set(), set()
    st = {_stage4(t0 - PA + 4 * c4, L, LP)[0] for c4 in range((NT + 2 * PA) // 4)}
    store = {(True, t0 + n < L) for n in range(NT)}
    return False, st, {False}, set(), store


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------
def utterance(C: int, L: int, seed: int):
    """(x, acc0) of one utterance, [L, C] float32: x ~ 2 N(0, 1), acc0 ~ N(0, 1); a function of (C, L, seed) alone, so that every launch that
    holds this utterance shares its reference"""
    rng = np.random.default_rng([int(seed), C, L])
    return (rng.standard_normal((L, C)) * 2.0).astype(np.float32), rng.standard_normal((L, C)).astype(np.float32)


def ragged_case(C: int, lengths, seed: int):
    """One slot per length, pitch LP = roundup4(max length), channel-major as the fp32 engines take it.  Returns a dict:
    rows [B]; LP; x [B, C, LP]: ``utterance(C, L, seed)`` inside rows[b], past it NaN in even slots and 1e4 N(0, 1) in odd ones (the header's
    contract is that the rest "reads as zero padding"; the kernels select and do not multiply); acc0 [B, C, LP] likewise inside and the
    sentinel past rows[b]; y [B, C, LP] the sentinel everywhere."""
    rows = [int(v) for v in lengths]
    B, LP = len(rows), roundup4(max(rows))
    rng = np.random.default_rng([int(seed), C, 99])
    x = np.empty((B, C, LP), np.float32)
    acc0 = np.full((B, C, LP), SENTINEL, np.float32)
    for b, L in enumerate(rows):
        xb, ab = utterance(C, L, seed)
        x[b, :, :L], acc0[b, :, :L] = xb.T, ab.T
        x[b, :, L:] = np.nan if b % 2 == 0 else (rng.standard_normal((C, LP - L)) * 1e4).astype(np.float32)
    return {"rows": rows, "LP": LP, "x": x, "acc0": acc0, "y": np.full((B, C, LP), SENTINEL, np.float32)}


def plain_case(C: int, L: int, seed: int):
    """B = 2 at pitch L: utterance(C, L, seed) and utterance(C, L, seed + 1); (x, acc0) [2, C, L]"""
    u = [utterance(C, L, seed), utterance(C, L, seed + 1)]
    return np.stack([q[0].T for q in u]).copy(), np.stack([q[1].T for q in u]).copy()


# ---- references -------------------------------------------------------------------------------------------------------------------------------
MODES = {"store": (False, 1.0), "add": (True, 1.0), "mean": (True, 3.0)}  # name -> (acc_add, div)


def params():
    from viettts_amd.hifigan.config import V1

    return RB.params_visible_bias(V1, PARAM_SEED)


def reference(P, C, k, x, acc0=None, div=1.0, dtype=np.float64, _mut=(), b=None):
    """one utterance alone: x / acc0 [L, C] -> [L, C] in ``dtype`` (resblock_ref on unrounded operands)"""
    W, b0 = RB.resblock_wb(P, C, k)
    out, _ = RB.resblock_ref(x[None], W, b0 if b is None else b, k, RB.DILS, dtype, acc0=None if acc0 is None else acc0[None], div=div,
                             rounded=False, _mut=_mut)
    return out[0]


def chunk_of(C: int) -> int:
    """input channels per staged chunk (kernels_f32_mfma.hip: chunk_of; the fp32 pair kernel's CK)"""
    return 64 if C >= 64 else 32


def chain_conv(x, w, b, d):
    """One convolution as ONE fp32 chain per output, in the order conv1d_f32_mfma_k documents: channel chunk -> tap -> channel, one fma per term
    (fp32(fp64(acc) + fp64(w) fp64(x)): the product of two fp32 values is exact in fp64), the bias added to the finished sum.
    x [L, C] fp32 (already activated), w [k, C, Cout], b [Cout] -> [L, Cout] fp32; vectorised over the outputs."""
    L, C = x.shape
    k = w.shape[0]
    pad = (k - 1) // 2 * d
    xp = np.zeros((L + 2 * pad, C), np.float64)
    xp[pad:pad + L] = x
    w64 = np.asarray(w, np.float32).astype(np.float64)
    acc = np.zeros((L, w.shape[2]), np.float64)
    tmp = np.empty_like(acc)
    CK = chunk_of(C)
    for c0 in range(0, C, CK):
        for j in range(k):
            for c in range(c0, c0 + CK):
                np.multiply(xp[j * d:j * d + L, c:c + 1], w64[j, c][None, :], out=tmp)
                tmp += acc
                acc = tmp.astype(np.float32).astype(np.float64)
    return (acc.astype(np.float32) + np.asarray(b, np.float32)).astype(np.float32)


def _lrelu32(v):
    return np.where(v >= 0, v, v * np.float32(0.1)).astype(np.float32)


def chain_resblock(P, C, k, x, acc0=None, div=1.0):
    """the ResBlock on ``chain_conv``, every other operation one fp32 operation in the epilogues' order (device_common.h: epilogue_store)"""
    W, b = RB.resblock_wb(P, C, k)
    cur = np.asarray(x, np.float32)
    for z, d in enumerate(RB.DILS):
        xt = _lrelu32(chain_conv(_lrelu32(cur), W[2 * z], b[2 * z], d))
        cur = (chain_conv(xt, W[2 * z + 1], b[2 * z + 1], 1) + cur).astype(np.float32)
    if acc0 is not None:
        cur = (np.asarray(acc0, np.float32) + cur).astype(np.float32)
        if div != 1.0:
            cur = (cur / np.float32(div)).astype(np.float32)
    return cur


def chain_lengths(C: int, k: int):
    """the two lengths the (slow) single-chain restatement runs at: past a pair's reach, and one output into the second tile"""
    _, _, NT2, R_, _ = pair_geometry("f32" if C in R.F32_PAIR_N1 else "x3", C, k)
    return R_ + 1, NT2 + 1


CHAIN_SEED = 7


def chain_errors(P, C, k):
    """[(L, max|chain - ref64|, max|ref32 - ref64|, max|ref64|)] on the class's two chain lengths"""
    out = []
    for L in chain_lengths(C, k):
        x, _ = utterance(C, L, CHAIN_SEED)
        r64 = reference(P, C, k, x)
        r32 = reference(P, C, k, x, dtype=np.float32)
        out.append((L, float(np.abs(chain_resblock(P, C, k, x).astype(np.float64) - r64).max()), float(np.abs(r32.astype(np.float64) - r64).max()),
                    float(np.abs(r64).max())))
    return out


def bar_f32(e32: float, want) -> float:
    return 4.0 * e32 + 2.0 ** -22 * float(np.abs(want).max())
