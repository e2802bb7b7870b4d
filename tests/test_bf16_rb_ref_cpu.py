"""The bf16 ResBlock comparison of tests/test_gpu_bf16_resblock.py, shown to bite on the CPU: the fp32 restatement stored as bf16 passes both
bars of tests/_bf16_rb_ref.py on every whole-ResBlock class, and a reference with one planted fault — a bias dropped, swapped or read from the
wrong channel block, a missing zero-padding mask, a shifted row or window, a NaN, a wrong epilogue — fails at least one.  Under
``synthetic_params``' own biases (N(0, 0.01^2)) the bias faults pass the pair KAT's bound: that is why ``params_visible_bias`` exists."""
import numpy as np
import pytest

import _bf16_rb_ref as RB
import _launch_regimes as R
from oracle import hifigan_oracle as orc
from viettts_amd.hifigan.config import V1
from viettts_amd.hifigan.synth import synthetic_params

L_CPU = 500
CLASSES = RB.BF16_RB_CLASSES
_ids = lambda ck: f"C{ck[0]}k{ck[1]}"  # noqa: E731


@pytest.fixture(scope="module")
def params():
    return RB.params_visible_bias(V1, 4321)


@pytest.fixture(scope="module")
def cases(params):
    """per class: inputs, the fp64 reference and the fp32 restatement, in store mode and in the accumulate-divide-LeakyReLU mode; computed once"""
    out = {}
    for C, k in CLASSES:
        rng = np.random.default_rng(C * 100 + k)
        x = (rng.standard_normal((2, L_CPU, C)) * 2.0).astype(np.float32)
        acc0 = rng.standard_normal((2, L_CPU, C)).astype(np.float32)
        W, b = RB.resblock_wb(params, C, k)
        c = {"x": x, "acc0": acc0, "W": W, "b": b}
        for mode, kw in (("store", {}), ("mean", dict(acc0=acc0, div=3.0, slope_out=0.1))):
            ref64, pairs = RB.resblock_ref(x, W, b, k, RB.DILS, np.float64, **kw)
            ref32, _ = RB.resblock_ref(x, W, b, k, RB.DILS, np.float32, **kw)
            c[mode] = (ref64, pairs, ref32)
        out[(C, k)] = c
    return out


def test_visible_bias_parameter_set(params):
    base = synthetic_params(V1, 4321, "scaled")
    assert sorted(params) == sorted(base)
    sig = []
    for key in base:
        assert np.array_equal(params[key]["w"], base[key]["w"]) and params[key]["b"].shape == base[key]["b"].shape
        assert params[key]["b"].dtype == np.float32
        sig.append(params[key]["b"])
    allb = np.concatenate(sig)
    assert 0.45 < allb.std() < 0.55 and abs(allb.mean()) < 0.05
    k0, k1 = RB.resblock_key(32, 3, 0, 1), RB.resblock_key(32, 3, 0, 2)
    assert not np.array_equal(params[k0]["b"], params[k1]["b"])  # drawn separately per layer
    again = RB.params_visible_bias(V1, 4321)
    assert all(np.array_equal(again[q]["b"], params[q]["b"]) for q in params)


@pytest.mark.parametrize("ck", CLASSES, ids=_ids)
def test_restatement_passes_both_bars(cases, ck, capsys):
    c = cases[ck]
    for mode in ("store", "mean"):
        ref64, pairs, ref32 = c[mode]
        e1, b1, e2, b2 = RB.bars(RB.bf(ref32), ref64, pairs, ref32)
        with capsys.disabled():
            print(f"\n[bf16(ref32) vs ref64, C={ck[0]} k={ck[1]} {mode}] max-abs {e1:.4f} (bar {b1:.4f})  rel-rms {e2:.5f} (bar {b2:.5f})")
        assert RB.passes(RB.bf(ref32), ref64, pairs, ref32)
        # the restatement alone is off by a bf16 rounding of the result and the flipped roundings of the intermediates: 2^-9 .. 2^-8 in rms
        assert 2.0 ** -10 < e2 < 2.0 ** -8, e2
        # unrounded, the restatement is the reference up to the flipped bf16 roundings of the intermediates
        assert np.abs(ref32 - ref64).max() <= b1 / 4


def _mutants(c, ck):
    """name -> bf16 output of the restatement with one fault planted (store mode unless the fault is in the epilogue)"""
    C, k = ck
    x, W, b, acc0 = c["x"], c["W"], c["b"], c["acc0"]
    _, _, NT = RB.rb_geometry(R.BF16_RB_W, C, k)
    good = RB.bf(c["store"][2])

    def run(bb=b, mut=(), **kw):
        return RB.bf(RB.resblock_ref(x, W, bb, k, RB.DILS, np.float32, _mut=mut, **kw)[0])

    flat = np.concatenate(b)
    out = {
        "b of two convolutions swapped": ("store", run([b[1], b[0]] + list(b[2:]))),
        "one b zeroed": ("store", run(list(b[:3]) + [np.zeros_like(b[3])] + list(b[4:]))),
        "b shifted by one 32-channel block": ("store", run(list(np.roll(flat, -32).reshape(6, C)))),
        "xt not zeroed at the first row past L": ("store", run(mut=("xt_tail",))),
    }
    row = good.copy()
    row[:, 137] = good[:, 138]
    out["one output row replaced by its neighbour"] = ("store", row)
    t0 = (R.cdiv(L_CPU, NT) - 1) * NT  # first output row of the last window
    win = good.copy()
    win[:, max(t0, 1):] = good[:, max(t0, 1) - 1 : -1]
    out["the last window shifted by one row"] = ("store", win)
    nan = good.copy()
    nan[1, 311, C // 2] = np.nan
    out["a NaN"] = ("store", nan)
    out["slope_out omitted"] = ("mean", run(acc0=acc0, div=3.0, slope_out=1.0))
    out["div applied before the accumulator is added"] = ("mean", run(mut=("div_first",), acc0=acc0, div=3.0, slope_out=0.1))
    out["acc0 ignored"] = ("mean", run(div=3.0, slope_out=0.1))
    return out


@pytest.mark.parametrize("ck", CLASSES, ids=_ids)
def test_every_planted_fault_fails_a_bar(cases, ck, capsys):
    c = cases[ck]
    lines = []
    for name, (mode, got) in _mutants(c, ck).items():
        ref64, pairs, ref32 = c[mode]
        e1, b1, e2, b2 = RB.bars(got, ref64, pairs, ref32)
        lines.append(f"  {name}: max-abs {e1:.3f} / {b1:.3f}, rel-rms {e2:.5f} / {b2:.5f}")
        assert not RB.passes(got, ref64, pairs, ref32), (ck, name, e1, b1, e2, b2)
    with capsys.disabled():
        print(f"\n[planted faults, C={ck[0]} k={ck[1]}: error / bar]\n" + "\n".join(lines))


@pytest.mark.parametrize("ck", CLASSES, ids=_ids)
def test_bias_faults_are_large_against_bar_i(cases, ck):
    """what params_visible_bias buys: a swapped or dropped bias moves the output by more than twice bar (i)"""
    c = cases[ck]
    ref64, pairs, ref32 = c["store"]
    m = _mutants(c, ck)
    for name in ("b of two convolutions swapped", "one b zeroed"):
        e1, b1, _, _ = RB.bars(m[name][1], ref64, pairs, ref32)
        assert e1 > 2 * b1, (ck, name, e1, b1)


@pytest.mark.parametrize("C,k", [(32, 3), (32, 7), (32, 11), (128, 3), (128, 7), (128, 11)])
def test_old_bound_passes_a_dropped_or_swapped_bias(C, k):
    """test_fused_pair_kat_bf16's reference formula and bound (2^-7 of the range, x ~ 2 N(0,1), B = 2, L = 700) under synthetic_params' biases:
    zeroing b1, zeroing b2, zeroing both or swapping them stays inside the bound on every class.  The gap params_visible_bias closes."""
    params = synthetic_params(V1, 4321, "scaled")
    k1, k2 = RB.resblock_key(C, k, 0, 1), RB.resblock_key(C, k, 0, 2)
    w1, b1, w2, b2 = params[k1]["w"], params[k1]["b"].astype(np.float64), params[k2]["w"], params[k2]["b"].astype(np.float64)
    x = np.random.default_rng(C * 100 + k * 10 + 1).standard_normal((2, 700, C)).astype(np.float32) * 2.0

    def pair(ba, bb):
        xt = orc.conv1d(RB.bf(orc.leaky_relu(RB.bf(x), 0.1)), RB.bf(w1), ba, 1, orc.get_padding(k, 1))
        return orc.conv1d(RB.bf(orc.leaky_relu(xt, 0.1)), RB.bf(w2), bb, 1, orc.get_padding(k, 1)) + RB.bf(x)

    ref = pair(b1, b2)
    bound = 2.0 ** -7 * np.abs(ref).max()
    z = np.zeros_like(b1)
    for name, got in (("b1 zeroed", pair(z, b2)), ("b2 zeroed", pair(b1, z)), ("both zeroed", pair(z, z)), ("swapped", pair(b2, b1))):
        moved = float(np.abs(got - ref).max())
        assert 0.005 < moved <= bound, (C, k, name, moved, bound)


def _kernel_conditions(W, M, NT, L):
    """resblock_bf16_k / resblock_x3_k's own conditions at length L, for windows 0 and 1:
    runs = !(t0 >= L); interior = tw >= 0 && tw + W <= L; every staged row inside (no `t >= L` mask); the last centre row (n = W - M - 1) stored"""
    out = []
    for w in (0, 1):
        t0 = w * NT
        tw = t0 - M
        out += [not t0 >= L, tw >= 0 and tw + W <= L, tw + W - 1 < L, (W - M - 1 >= M) and tw + (W - M - 1) < L]
    return tuple(out)


@pytest.mark.parametrize("table,classes", [(R.BF16_RB_W, RB.BF16_RB_CLASSES), (R.X3_RB_W, RB.X3_RB_CLASSES)], ids=["RBTile", "RXTile"])
def test_edge_lengths_are_where_the_kernels_conditions_flip(table, classes):
    for C, k in classes:
        W, M, NT = RB.rb_geometry(table, C, k)
        assert NT >= 32 and M >= 3 and NT > M + 2, (C, k)
        edges = RB.edge_lengths(W, M, NT)
        flips = [L for L in range(2, 3 * NT + 6) if _kernel_conditions(W, M, NT, L) != _kernel_conditions(W, M, NT, L - 1)]
        # window 0's last centre row stored; window 1 runs; window 0 fully inside; window 1's last centre row stored; window 1 interior
        assert flips == [NT, NT + 1, NT + M, 2 * NT, 2 * NT + M], (C, k, flips)
        before = [NT + M - 1, 2 * NT + M - 1]  # the staging path's flips are tested from both sides
        assert set(flips) | set(before) <= set(edges)
        # the rest: the shortest utterances, the margin, one row short of a window, one row past window 0, four windows
        assert sorted(set(edges) - set(flips) - set(before)) == sorted({1, 2, M, M + 1, NT - 1, NT + M + 1, 3 * NT + 5}), (C, k)
        L4 = 3 * NT + 5
        assert R.cdiv(L4, NT) == 4 and NT - M >= 0 and NT - M + W <= L4  # four windows: window 1 interior, window 3 five rows


def test_geometry_table_of_the_bf16_windows():
    want = {(32, 3): (256, 12, 232), (32, 7): (512, 36, 440), (32, 11): (512, 60, 392), (64, 3): (256, 12, 232), (128, 3): (128, 12, 104)}
    assert {ck: RB.rb_geometry(R.BF16_RB_W, *ck) for ck in RB.BF16_RB_CLASSES} == want
    assert RB.edge_lengths(256, 12, 232) == [1, 2, 12, 13, 231, 232, 233, 243, 244, 245, 464, 475, 476, 701]
    assert RB.xcd_seams(197) == [24, 49, 73, 98, 123, 147, 172]
