"""tests/_pair_edges.py shown to bite, on the CPU: the edge lengths reach every mask and clamp of the fp32 / bf16x3 pair kernels and of the fp32
per-convolution kernel, both ways, in the first, the second and the last tile; the bars admit a single-chain fp32 restatement in the
kernels' documented order; and a reference with one planted fault misses both bars by a wide margin."""
import numpy as np
import pytest

import _bf16_rb_ref as RB
import _launch_regimes as R
import _pair_edges as PE
from oracle import hifigan_oracle as orc

_ids = lambda ck: f"C{ck[0]}k{ck[1]}"  # noqa: E731


@pytest.fixture(scope="module")
def P():
    return PE.params()


def test_geometry_and_length_tables():
    assert PE.pair_geometry("f32", 128, 11) == (128, 5, 118, 30, 28)
    assert PE.pair_geometry("f32", 32, 3) == (256, 1, 254, 6, 8)
    assert PE.pair_geometry("x3", 32, 7) == (512, 3, 506, 18, 16)
    assert PE.pair_geometry("x3", 256, 3) == (128, 1, 126, 6, 8)
    assert PE.pair_edge_lengths(1, 254) == [1, 2, 3, 4, 5, 6, 7, 248, 252, 253, 254, 255, 256, 260, 261, 507, 508, 509, 514, 767]
    assert PE.pair_edge_lengths(5, 118) == [1, 2, 3, 4, 5, 6, 10, 11, 30, 31, 88, 112, 113, 117, 118, 119, 123, 124, 148, 149, 235, 236, 237, 266, 359]
    assert PE.conv_edge_lengths(3, 64) == [1, 2, 3, 4, 5, 15, 16, 63, 64, 65, 79, 80, 128, 129, 197]
    for C, k in PE.CLASSES:
        H = (k - 1) // 2
        assert PE.pair_geometry("x3", C, k)[4] == ((5 * H + 3) // 4) * 4
        assert set(PE.conv_edge_lengths(H, PE.conv_nt(C, True))) <= set(PE.conv_route_lengths(C, k))
        assert PE.F32_PAIR_CLASSES == [ck for ck in PE.CLASSES if ck[0] <= 128]


def _seen(cond, lengths, tiles_of):
    """per tile kind ('first', 'second', 'last'): exits seen, staging kinds, clamp seen, xt kinds, store kinds — over ``lengths`` in one ragged slot
    of pitch roundup4(max) and each alone at pitch roundup4(L) (the plain launches), at the rates 1, 3, 5.
    'last' is the utterance's own last tile for the masks and the slot's last tile for the exit."""
    seen = {kind: {"exit": set(), "stage": set(), "clamp": set(), "xt": set(), "store": set()} for kind in ("first", "second", "last")}
    for L, LP in [(L, PE.roundup4(max(lengths))) for L in lengths] + [(L, PE.roundup4(L)) for L in lengths]:
        own, slot = tiles_of(L), tiles_of(LP)
        for kind, tile in (("first", 0), ("second", 1), ("last", own - 1)):
            if kind == "second" and slot < 2:
                continue
            for dil in PE.RATES:
                ex, st, cl, xt, store = cond(L, LP, tile, dil)
                s = seen[kind]
                s["exit"].add(ex)
                if not ex:
                    s["stage"] |= st
                    s["clamp"] |= cl
                    s["xt"] |= xt
                    s["store"] |= store
        seen["last"]["exit"].add(cond(L, LP, slot - 1, 1)[0])
    return seen


@pytest.mark.parametrize("engine", ["f32", "x3"])
def test_pair_edge_lengths_reach_every_condition_both_ways(engine):
    for C, k in (PE.F32_PAIR_CLASSES if engine == "f32" else PE.CLASSES):
        N1, H, NT2, R_, _ = PE.pair_geometry(engine, C, k)
        lengths = PE.pair_edge_lengths(H, NT2)
        assert lengths == sorted(set(lengths)) and lengths[0] == 1 and NT2 - R_ > R_ + 1, (C, k)
        assert {L % 4 for L in lengths} == {0, 1, 2, 3}, (C, k)
        assert any(L - (R.cdiv(L, NT2) - 1) * NT2 == 1 and L > NT2 for L in lengths), (C, k)  # the last tile holds exactly one output
        fn = PE.f32_pair_conditions if engine == "f32" else PE.x3_pair_conditions
        seen = _seen(lambda L, LP, tile, dil: fn(N1, H, L, LP, tile, dil), lengths, lambda L: R.cdiv(L, NT2))
        partial = {"partial"} if engine == "f32" else set()  # (the split-operand kernel stages row by row)
        for kind in ("first", "second", "last"):
            s = seen[kind]
            # t0 >= L: tile 0 always runs (rows >= 1); tile 1 and the slot's last tile both exit and run
            assert s["exit"] == ({False} if kind == "first" else {False, True}), (C, k, kind)
            # staging: zero-filled past L, loaded whole, (float4) cut by mask_tail4; before 0 only where a tile starts inside the halo of the utterance's start
            assert {"in", "hi"} | partial <= s["stage"], (C, k, kind, s["stage"])
            assert s["clamp"] == {False, True}, (C, k, kind)
            # xt's zero padding: tt >= L both ways; tt < 0 in tile 0
            assert {"in", "hi"} <= s["xt"], (C, k, kind)
            # the store mask: a kept column inside and past L, a discarded column (n >= NT2) inside and past L (an utterance's last tile has no
            # discarded column inside L)
            want = {(True, True), (True, False), (False, True), (False, False)} - ({(False, True)} if kind == "last" else set())
            assert s["store"] == want, (C, k, kind, s["store"])
        assert "lo" in seen["first"]["stage"] and "lo" in seen["first"]["xt"]
        assert "lo" not in seen["second"]["xt"] and "lo" not in seen["second"]["stage"]


def test_conv_edge_lengths_reach_every_condition_both_ways():
    for C, k in PE.CLASSES:
        H = (k - 1) // 2
        PA = PE.pair_geometry("x3", C, k)[4]
        for narrow in (False, True):
            NT = PE.conv_nt(C, narrow)
            lengths = PE.conv_edge_lengths(H, NT)
            assert {L % 4 for L in lengths} == {0, 1, 2, 3}
            assert any(L - (R.cdiv(L, NT) - 1) * NT == 1 and L > NT for L in lengths)
            seen = _seen(lambda L, LP, tile, dil: PE.conv_conditions(NT, PA, L, LP, tile), lengths, lambda L: R.cdiv(L, NT))
            for kind in ("first", "second", "last"):
                s = seen[kind]
                assert s["exit"] == ({False} if kind == "first" else {False, True}), (C, k, NT, kind)
                assert {"in", "hi", "partial"} <= s["stage"], (C, k, NT, kind)
                assert s["store"] == {(True, True), (True, False)}, (C, k, NT, kind)
            assert "lo" in seen["first"]["stage"]
        # the route's union holds every one of them
        assert set(PE.conv_edge_lengths(H, PE.conv_nt(C, False))) | set(PE.conv_edge_lengths(H, PE.conv_nt(C, True))) <= set(PE.conv_route_lengths(C, k))


def test_ragged_case_layout():
    c = PE.ragged_case(32, [5, 1, 9, 8], 3)
    assert c["LP"] == 12 and c["x"].shape == (4, 32, 12) and c["rows"] == [5, 1, 9, 8]
    assert np.isnan(c["x"][0, :, 5:]).all() and np.isnan(c["x"][2, :, 9:]).all()
    assert np.isfinite(c["x"][1]).all() and np.abs(c["x"][1, :, 1:]).max() > 1e4 and np.abs(c["x"][3, :, 8:]).max() > 1e4
    for b, L in enumerate(c["rows"]):
        x, a = PE.utterance(32, L, 3)
        assert np.array_equal(c["x"][b, :, :L], x.T) and np.array_equal(c["acc0"][b, :, :L], a.T)
        assert (c["acc0"][b, :, L:] == PE.SENTINEL).all()
    assert (c["y"] == PE.SENTINEL).all()
    x2, a2 = PE.plain_case(32, 8, 3)
    assert np.array_equal(x2[0], c["x"][3, :, :8]) and not np.array_equal(x2[0], x2[1]) and a2.shape == (2, 32, 8)


def test_chain_conv_is_the_convolution():
    """the single-chain restatement against the oracle's convolution: the same sum up to fp32 summation error, at every rate"""
    rng = np.random.default_rng(5)
    for C, k in ((32, 3), (64, 7), (128, 11)):
        x = rng.standard_normal((40, C)).astype(np.float32)
        w = (rng.standard_normal((k, C, C)) * 0.05).astype(np.float32)
        b = rng.standard_normal(C).astype(np.float32)
        for d in PE.RATES:
            want = orc.conv1d(x[None].astype(np.float64), w.astype(np.float64), b.astype(np.float64), d, orc.get_padding(k, d))[0]
            got = PE.chain_conv(x, w, b, d)
            assert got.dtype == np.float32 and got.shape == want.shape
            assert np.abs(got - want).max() <= 2.0 ** -24 * (C * k) ** 0.5 * 8 * np.abs(want).max(), (C, k, d)


@pytest.mark.parametrize("ck", PE.CLASSES, ids=_ids)
def test_the_fp32_bar_admits_the_single_chain_restatement(P, ck, capsys):
    """4 e32 + 2^-22 max|want| with e32 = numpy's float32 run ALONE on the same input admits one fp32 chain per output in the kernels' order
    (the GPU tests' e32 also takes the chain's own error in, class-wide, so their bar is no tighter than this one)"""
    C, k = ck
    for L, e_chain, e_np, peak in PE.chain_errors(P, C, k):
        bar = PE.bar_f32(e_np, np.array([peak]))
        with capsys.disabled():
            print(f"\n[single chain C={C} k={k} L={L}] err {e_chain:.3e} / bar {bar:.3e} = {e_chain / bar:.2f}  (numpy fp32 run {e_np:.3e}, max|want| {peak:.2f})")
        assert e_chain <= bar, (ck, L, e_chain, bar)
        assert e_chain / peak < PE.X3_BOUND / 10  # and sits far inside the bf16x3 bound's scale


def _faults(P, C, k, L, NT2):
    """name -> (mode, faulty [L, C] float64) on utterance(C, L, 11)"""
    H = (k - 1) // 2
    x, acc0 = PE.utterance(C, L, 11)
    W, b = RB.resblock_wb(P, C, k)
    out = {}
    out["xt not zeroed past L"] = ("store", PE.reference(P, C, k, x, _mut=("xt_tail",)))
    out["div applied before the accumulator is added"] = ("mean", PE.reference(P, C, k, x, acc0=acc0, div=3.0, _mut=("div_first",)))
    out["b2 of pair 2 dropped"] = ("store", PE.reference(P, C, k, x, b=list(b[:5]) + [np.zeros_like(b[5])]))
    out["biases of pairs 1 and 2 swapped"] = ("store", PE.reference(P, C, k, x, b=[b[0], b[1], b[4], b[5], b[2], b[3]]))
    leak = np.concatenate([x, np.full((1, C), 1.5, np.float32)])  # x read one column past L: a finite value where zero padding belongs
    out["x read one column past L"] = ("store", PE.reference(P, C, k, leak)[:L])
    # the first output column of tile 1 taken from tile 0's discarded column n = NT2: its last tap reads the zero-filled xt column N1
    good, pairs = RB.resblock_ref(x[None], W, b, k, RB.DILS, np.float64, rounded=False)
    p1 = pairs[1]
    xt = orc.leaky_relu(orc.conv1d(orc.leaky_relu(p1, 0.1), W[4].astype(np.float64), b[4].astype(np.float64), 5, orc.get_padding(k, 5)), 0.1)
    xt[:, NT2 + H:] = 0.0
    bad = orc.conv1d(xt, W[5].astype(np.float64), b[5].astype(np.float64), 1, orc.get_padding(k, 1))[:, :L] + p1
    assert np.allclose(bad[0, :NT2], good[0, :NT2], rtol=0, atol=1e-12)
    seam = good[0].copy()
    seam[NT2] = bad[0, NT2]
    out["tile 1's first column from tile 0's discarded columns"] = ("store", seam)
    return x, acc0, out


@pytest.mark.parametrize("ck", PE.CLASSES, ids=_ids)
def test_every_planted_fault_misses_both_bars_by_a_wide_margin(P, ck, capsys):
    C, k = ck
    _, H, NT2, R_, _ = PE.pair_geometry("f32" if C <= 128 else "x3", C, k)
    L = NT2 + R_ + 1
    x, acc0, faults = _faults(P, C, k, L, NT2)
    e32 = max(max(c[1], c[2]) for c in PE.chain_errors(P, C, k))
    lines = []
    for name, (mode, got) in faults.items():
        acc_add, div = PE.MODES[mode]
        want = PE.reference(P, C, k, x, acc0=acc0 if acc_add else None, div=div)
        err = float(np.abs(got - want).max())
        bar, rel = PE.bar_f32(e32, want), err / float(np.abs(want).max())
        lines.append(f"  {name}: err {err:.3e} = {err / bar:.0f} x the fp32 bar, {rel / PE.X3_BOUND:.0f} x the bf16x3 bound")
        assert err > 20 * bar and rel > 20 * PE.X3_BOUND, (ck, name, err, bar, rel)
    with capsys.disabled():
        print(f"\n[planted faults C={C} k={k} L={L}]\n" + "\n".join(lines))
