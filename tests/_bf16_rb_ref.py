"""Reference of one bf16 ResBlock1 as the kernels round it, the bias-visible parameter set, the window-edge lengths and the two bars the
ResBlock tests hold the kernels to (numpy only; tests/test_bf16_rb_ref_cpu.py shows on the CPU that the comparison bites).

Why a parameter set of its own: ``synthetic_params`` draws ``b ~ N(0, 0.01^2)``.  The bf16 known-answer tests feed ``x ~ 2 N(0, 1)`` and accept
2^-7 (pairs) or 2^-8 (single convolutions) of the output's range, 0.07 to 0.09 absolute, while dropping, swapping or mis-indexing such a bias
moves the output by 0.016 to 0.067: every bf16 module test passes a kernel that gets the biases wrong.  ``params_visible_bias`` keeps the
weights and draws every bias from N(0, 0.5^2), where the same faults move the output by 0.8 to 4.4.
"""
from __future__ import annotations

import numpy as np

import _launch_regimes as R
from oracle import hifigan_oracle as orc

BIAS_SIGMA = 0.5
DILS = (1, 3, 5)  # every V1 ResBlock1's rates
# (C, k) of the whole-ResBlock kernels: resblock_bf16_k (kernels_bf16_rbk.hip) and resblock_x3_k (kernels_x3_rb.hip)
BF16_RB_CLASSES = [(C, k) for C in (32, 64, 128) for k in sorted(R.BF16_RB_W[C])]
X3_RB_CLASSES = [(C, k) for C in (32, 64, 128) for k in sorted(R.X3_RB_W[C])]


def bf(x):
    """round-to-nearest-even to bf16, returned as float64 (NaN stays NaN)"""
    x32 = np.ascontiguousarray(x, dtype=np.float32)
    u = x32.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    out = u.astype(np.uint32).view(np.float32).astype(np.float64)
    return np.where(np.isnan(x32), np.nan, out)


def params_visible_bias(cfg, seed: int):
    """``synthetic_params(cfg, seed, "scaled")`` with every bias redrawn from N(0, 0.5^2), each layer from a stream of its own."""
    from viettts_amd.hifigan.synth import synthetic_params

    params = synthetic_params(cfg, seed, "scaled")
    out = {}
    for i, key in enumerate(sorted(params)):
        b = np.random.default_rng([int(seed), i]).standard_normal(params[key]["b"].shape) * BIAS_SIGMA
        out[key] = {"w": params[key]["w"], "b": b.astype(np.float32)}
    return out


def resblock_key(C: int, k: int, z: int = 0, conv: int = 1) -> str:
    """V1's ResBlock1 of (C, k): stage i has 512 >> (i + 1) channels, its ResBlock j the kernel size (3, 7, 11)[j]"""
    i, j = {256: 0, 128: 1, 64: 2, 32: 3}[C], {3: 0, 7: 1, 11: 2}[k]
    return f"generator/~/res_block1_{3 * i + j}/~/convs{conv}_{z}"


def resblock_wb(params, C: int, k: int):
    """the six convolutions (c1_0, c2_0, c1_1, ...) of V1's (C, k) ResBlock: ([w], [b])"""
    keys = [resblock_key(C, k, z, conv) for z in range(3) for conv in (1, 2)]
    return [params[q]["w"] for q in keys], [params[q]["b"] for q in keys]


def resblock_ref(x, W, b, k, dils, dtype, acc0=None, div=1.0, slope_out=1.0, rounded=True, _mut=()):
    """One ResBlock1 (vietTTS/hifigan/model.py:44-51) and the MRF bookkeeping of its last epilogue (model.py:115-121), on
    ``oracle.hifigan_oracle.conv1d / leaky_relu``, rounding to bf16 exactly where the bf16 kernels round:

        x, acc0 on entry;  lrelu(x) (c1's operand);  xt = lrelu(c1 + b) (c2's operand);  x' after pairs 0 and 1 (the stored running x)

    and NOT after pair 2: ``v = x''' (+ acc0)``, then ``v / div``, then LeakyReLU(``slope_out``), returned unrounded.  The weights are rounded
    to bf16, the biases are fp32.  ``x`` / ``acc0``: ``[B, L, C]``; ``W[6]``, ``b[6]``: c1_0, c2_0, c1_1, c2_1, c1_2, c2_2 in Haiku layout.

    ``dtype=np.float64`` is the reference; ``dtype=np.float32`` the restatement of the kernels' arithmetic: fp32 accumulation, tap by tap.
    ``rounded=False`` rounds nothing (the fp32 / split-operand engines' reference).  Returns ``(result, [p0, p1, p2])``, the per-pair outputs
    unrounded too.

    The kernels multiply by ``1.0f / div`` instead of dividing (bf16_common.h: mrf_recip): at most one fp32 ulp from the quotient, 2^-16 of
    the bf16 ulp the value is rounded to right afterwards.  ``_mut``: faults the CPU test plants to show that the bars see them.
    """
    rnd = (lambda a: bf(a).astype(dtype)) if rounded else (lambda a: np.asarray(a, dtype=dtype))
    L = x.shape[1]
    cur = rnd(x)
    pairs = []
    for z, d in enumerate(dils):
        w1, w2 = rnd(W[2 * z]), rnd(W[2 * z + 1])
        b1, b2 = np.asarray(b[2 * z], dtype=dtype), np.asarray(b[2 * z + 1], dtype=dtype)
        xin = rnd(orc.leaky_relu(cur, orc.LRELU_SLOPE))
        if "xt_tail" in _mut:  # c1's value at the first row past the utterance reaches c2 instead of the zero padding
            xin = np.concatenate([xin, np.zeros_like(xin[:, :1])], axis=1)
        xt = orc.conv1d(xin, w1, b1, d, orc.get_padding(k, d))
        xt = rnd(orc.leaky_relu(xt, orc.LRELU_SLOPE))
        nxt = orc.conv1d(xt, w2, b2, 1, orc.get_padding(k, 1))[:, :L] + cur
        pairs.append(nxt)
        cur = rnd(nxt) if z < 2 else nxt
    v = cur
    if "div_first" in _mut:
        v = v / dtype(div)
    if acc0 is not None:
        v = v + rnd(acc0)
    if "div_first" not in _mut:
        v = v / dtype(div)
    return orc.leaky_relu(v, slope_out), pairs


# ---- the two bars ---------------------------------------------------------------------------------------------------------------------------
BAR_I_REL = 2.0 ** -7  # the pair bound of test_fused_pair_kat_bf16 ...
BAR_II_FACTOR = 4.0    # ... and the 4 x err_ref32 convention of the mel and audio tests


def _rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, dtype=np.float64)))))


def bars(got, ref64, pairs64, ref32):
    """(err_i, bar_i, err_ii, bar_ii) of ``got`` against the fp64 reference.
    (i)  max|got - ref64| <= 2^-7 (max|p0| + max|p1| + max|final|): each pair meets 2^-7 of its output's range (test_fused_pair_kat_bf16), a pair
         hands its error on through the residual path with gain ~1 and adds its own (tests/test_gpu_launch_regimes.py: BF16_MRF_REL);
    (ii) rms(got - ref64) / rms(ref64) <= 4 rms(bf16(ref32) - ref64) / rms(ref64): four times what the fp32 restatement, stored as bf16, is
         off by — recomputed per case, never taken from a kernel."""
    got = np.asarray(got, dtype=np.float64)
    scale = _rms(ref64)
    err_i = float(np.abs(got - ref64).max())
    bar_i = BAR_I_REL * (float(np.abs(pairs64[0]).max()) + float(np.abs(pairs64[1]).max()) + float(np.abs(ref64).max()))
    err_ii = _rms(got - ref64) / scale
    bar_ii = BAR_II_FACTOR * _rms(bf(ref32) - ref64) / scale
    return err_i, bar_i, err_ii, bar_ii


def passes(got, ref64, pairs64, ref32) -> bool:
    e1, b1, e2, b2 = bars(got, ref64, pairs64, ref32)
    return bool(e1 <= b1) and bool(e2 <= b2)  # (a NaN fails both)


# ---- window geometry ------------------------------------------------------------------------------------------------------------------------
def rb_geometry(table, C: int, k: int, dils=DILS):
    """(W, M, NT) of a whole-ResBlock kernel's window: ``table`` = _launch_regimes.BF16_RB_W or X3_RB_W"""
    W = table[C][k]
    return W, R.rb_margin(k, dils), R.rb_window_nt(W, k, dils)


def edge_lengths(W: int, M: int, NT: int):
    """The lengths at which a window kernel's conditions (``t0 >= L``, ``tw >= 0 && tw + W <= L``, ``n >= M && n < W - M``, ``t < L``) flip for
    its first windows, with their neighbours: one and two rows; around the margin; a full window's outputs and one row less / more; the last
    staged row of window 0 (t = NT + M - 1) outside / inside / passed; two full windows; window 1 turning interior; four windows."""
    out = [1, 2, M, M + 1, NT - 1, NT, NT + 1, NT + M - 1, NT + M, NT + M + 1, 2 * NT, 2 * NT + M - 1, 2 * NT + M, 3 * NT + 5]
    assert out == sorted(set(out)) and out[0] >= 1, (W, M, NT)
    return out


def xcd_seams(ntv: int):
    """first tile of each XCD's eighth of ntv tiles (resblock_bf16_k / device_common.h xcd_tile: lo = (rx * ntv) >> 3), rx = 1..7"""
    return [(rx * ntv) >> 3 for rx in range(1, R.XCDS)]
