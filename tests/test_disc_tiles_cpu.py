"""tests/_disc_tiles.py against viettts_amd/csrc/disc.hip, the tile-edge cover it computes, and the per-layer comparison of
tests/_disc_layer_ref.py against itself (CPU only).

tests/test_gpu_disc_layers.py takes its lengths from the table so that each layer's row of outputs sits exactly on a tile edge.  A pull request
that moves a tile width in the source and not in the table would leave those tests passing beside the edge; the first test here reads the numbers
out of the source and fails instead.  The last tests show that the comparison's bar passes torch's own fp32 result and fails a moved element, a
NaN and a shifted tile."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import _disc_layer_ref as ref
import _disc_oracle as oracle
import _disc_tiles as D

SRC = (Path(__file__).resolve().parents[1] / "viettts_amd" / "csrc" / "disc.hip").read_text()


def _instances(expr):
    return tuple(tuple(int(v) if v.strip().isdigit() else v.strip() == "true" for v in m.split(",")) for m in re.findall(r"launch_gemm<([^>]+)>", expr))


def test_the_table_matches_the_source():
    fwd = SRC[SRC.index("VTTS_API int vtts_disc_forward(") :]
    fwd = fwd[: fwd.index("\n}\n")]
    switch = re.findall(r"const bool wide = Nout > (\d+);", fwd)
    assert switch == [str(D.WIDE_SWITCH)], switch
    branches = re.findall(r"(?:else )?if \(a\.cout_g (>=|==) (\d+)\)\s*e = ([^;]+);", fwd)
    last = re.findall(r"else\s*e = (launch_gemm[^;]+);", fwd)
    assert len(last) == 1, last
    got = {}
    for op, val, expr in branches:
        assert (op == ">=") == (int(val) == 512), (op, val)
        inst = _instances(expr)
        assert (len(inst) == 2) == expr.strip().startswith("wide ?"), expr  # two instances: the wide one first
        got[int(val)] = inst
    # the closing else takes what is left of the model's classes: the 16-channel groups, in the 16-row MFMA form
    classes = {D.gemm_class(ly["spec"][1] // ly["spec"][5]) for ly in D.layers() if ly["kind"] == "gemm"}
    assert classes == set(D.GEMM_LAUNCH) and classes - set(got) == {16}, (classes, sorted(got))
    got[16] = _instances(last[0])
    assert re.search(r"const bool m16 = cout_g == 16;", SRC)
    assert got == D.GEMM_LAUNCH, got
    for inst in got.values():
        for wm, wn, mw, nw, m16 in inst:
            assert wm * wn == 4 and (not m16 or (wm == 1 and mw == 1))
    # NT in the kernel and in the launcher, and the grids
    assert len(re.findall(r"constexpr int (?:[^;]*, )?NT = WN \* NW \* 32;", SRC)) == 2
    assert re.search(r"const dim3 grid\(\(unsigned\)\(\(a\.Nout \+ NT - 1\) / NT\)", SRC) and re.search(r"n0 = blockIdx\.x \* NT\b", SRC)
    F, P = D.FIRST_BLOCK, D.POST_BLOCK
    for kern in ("mpd_first_k", "msd_first_k"):
        assert re.search(rf"hipLaunchKernelGGL\({kern}, dim3\(\(Nout \+ {F - 1}\) / {F}, N\), dim3\(256\)", fwd), kern
    assert re.search(rf"hipLaunchKernelGGL\(disc_post_k, dim3\(\(Nout \+ {P - 1}\) / {P}, N\), dim3\(256\)", fwd)
    assert re.search(rf"const int n = blockIdx\.x \* {F} \+ threadIdx\.x", SRC) and re.search(rf"l0 = blockIdx\.x \* {F}\b", SRC)
    assert re.search(rf"const int pos = blockIdx\.x \* {P} \+ lane;", SRC)
    assert [(len(r), len(r[0])) for r in (D.layers(),)] == [(54, 8)] and [ly["spec"] for ly in D.layers()] == [s for _, s in oracle.conv_keys()]


def test_tile_widths_per_class():
    assert {c: tuple(D.gemm_nt(a) for a in inst) for c, inst in D.GEMM_LAUNCH.items()} == {512: (128, 64), 128: (128, 64), 64: (128,), 32: (256,), 16: (256,)}
    by_cls = {}
    for ly in D.layers():
        by_cls.setdefault(ly["cls"], []).append(ly["index"])
    assert {k: len(v) for k, v in by_cls.items()} == {"first": 8, "gemm128": 5, "gemm512": 18, "post": 8, "gemm32": 6, "gemm16": 3, "gemm64": 6}
    ly = D.layers()[2]
    assert [D.launched_nt(ly, n) for n in (1, 64, 65, 128, 129)] == [64, 64, 128, 128, 128]


def test_every_target_is_covered():
    targets, cover = D.targets(), D.cover()
    assert len(targets) == 154 == 2 * sum(len(ly["widths"]) for ly in D.layers())
    shapes = {T: oracle.fmap_shapes(T) for T in cover}
    covered = set()
    for T, items in cover.items():
        assert T >= D.MIN_T and items
        for i, nt, side, nout in items:
            _, L, p = shapes[T][i]
            assert L * p == nout and p == D.layers()[i]["p"], (T, i, nt, side, nout, L, p)  # the length gives the layer exactly the target's row
            assert (nout <= nt) if side == "le" else (nout > nt), (T, i, nt, side, nout)
            covered.add((i, nt, side, nout))
    assert covered == {t[:4] for t in targets}
    # each target is the row length NEXT to the edge: no reachable row lies between it and NT
    for i, nt, side, nout, lo, hi in targets:
        p = D.layers()[i]["p"]
        assert nout % p == 0 and (nt - p < nout <= nt if side == "le" else nt < nout <= nt + p), (i, nt, side, nout)
        assert D.nout(i, lo) == D.nout(i, hi) == nout and D.nout(i, hi + 1) > nout and (lo == D.MIN_T or D.nout(i, lo - 1) < nout)
    assert len(cover) == 41 and min(cover) == 256 and max(cover) == 32766, (len(cover), min(cover), max(cover))


def test_a_second_tile_starts_in_mid_row_for_every_odd_period():
    """jrel0 != 0 needs Nout > NT and NT % p != 0: at least one covered MPD GEMM layer per period 3, 5, 7, 11, at the tile width it launches."""
    found = {}
    for T, items in D.cover().items():
        for i, nt, side, nout in items:
            ly = D.layers()[i]
            if ly["kind"] == "gemm" and ly["disc"] < 5 and nout > nt and nt % ly["p"] and D.launched_nt(ly, nout) == nt:
                found.setdefault(ly["p"], []).append((T, i, nt, nout))
    assert set(found) >= {3, 5, 7, 11}, sorted(found)


# ---- the per-layer reference and the comparison itself -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def params():
    from viettts_amd.hifigan.disc_synth import synthetic_disc_checkpoint
    from viettts_amd.hifigan.discriminators import fold_checkpoint

    return fold_checkpoint(synthetic_disc_checkpoint(8642))


def test_the_layers_chained_are_the_oracle(params):
    """layer_reference() of the oracle's own map i - 1 is the oracle's map i: same operators, same order."""
    y2 = oracle.make_inputs(1, 38, 5)
    _, fmaps = oracle.forward(params, y2, torch.float64)
    for ly in D.layers():
        i = ly["index"]
        x = y2.astype(np.float64) if ly["kind"].endswith("first") else fmaps[i - 1].numpy()
        got = ref.layer_reference(params, i, x, torch.float64)
        want = fmaps[i].numpy()
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-13 * np.abs(want).max(), i


@pytest.fixture(scope="module")
def one_layer(params):
    """MPD period 3, 512 -> 1024 (K = 2560) with a row of 129 positions: one 128-wide tile and one position of a second, which starts in mid-row (128 = 42 * 3 + 2)."""
    i, L = 6 + 3, 43
    rng = np.random.default_rng(77)
    x = rng.standard_normal((2, 512, 3 * L - 2, 3)).astype(np.float32)
    x = np.where(x > 0, x, np.float32(0.1) * x)
    r64, r32 = ref.layer_reference(params, i, x, torch.float64), ref.layer_reference(params, i, x, torch.float32)
    assert r64.shape == (2, 1024, L, 3)
    return D.layers()[i], r64, r32


def test_the_comparison_passes_fp32_and_fails_what_it_should(one_layer):
    ly, r64, r32 = one_layer
    ok, err, e32, bound = ref.compare_layer(r32, r64, r32)
    assert ok and err == e32 and bound == 4 * e32 + 2.0 ** -22
    assert e32 > 2.0 ** -24  # 8 e32 > 4 e32 + 2^-22 exactly then
    scale = np.abs(r64).max()
    # one element of a row's last position, moved by 8 e32 max|ref| away from the expectation
    moved = r32.astype(np.float64)
    sign = 1.0 if moved[1, 1023, -1, -1] >= r64[1, 1023, -1, -1] else -1.0
    moved[1, 1023, -1, -1] += sign * 8 * e32 * scale
    ok, err, _, bound = ref.compare_layer(moved, r64, r32)
    assert not ok and err >= 8 * e32 > bound
    # one NaN
    holed = r32.copy()
    holed[0, 517, -1, -1] = np.nan
    assert not ref.compare_layer(holed, r64, r32)[0]
    # the last tile's columns shifted by one
    nt = D.launched_nt(ly, 129)
    assert nt == 128
    last = r32.reshape(2, 1024, 129).copy()
    last[:, :, nt:] = r32.reshape(2, 1024, 129)[:, :, nt - 1 : 128]
    assert not ref.compare_layer(last.reshape(r32.shape), r64, r32)[0]
    # conv_post's bar is one rounding: the fp64 result rounded once passes, an element moved by 2^-21 of the scale does not
    once = r64.astype(np.float32)
    assert ref.compare_layer(once, r64, r32, post=True)[0]
    off = once.astype(np.float64)
    off[0, 0, 0, 0] += 2.0 ** -21 * scale
    assert not ref.compare_layer(off, r64, r32, post=True)[0]


def test_loss_yardstick_is_the_oracle_in_its_arithmetic_class():
    """On data that fp32 element arithmetic handles exactly (multiples of 1/64, |x| < 4) the yardstick is the fp64 oracle's losses."""
    rng = np.random.default_rng(3)
    B = 2
    fm = [(rng.integers(-255, 256, (2 * B, 3, 5)) / 64.0).astype(np.float32) for _ in range(54)]
    sc = [(rng.integers(-255, 256, (2 * B, 7)) / 64.0).astype(np.float32) for _ in range(8)]
    got = ref.loss_yardstick(fm, sc, B)
    L = oracle.losses([torch.from_numpy(s).double() for s in sc], [torch.from_numpy(f).double() for f in fm], B)
    want = np.concatenate([L["fmap_l1"], L["real"], L["fake"], L["gens"], np.array([L[k] for k in oracle.LOSS_NAMES])])
    assert got.shape == (87,) and np.abs(got / want - 1).max() <= 1e-14
