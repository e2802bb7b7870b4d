"""The fp32 and bf16x3 pair kernels and the fp32 per-convolution launches alone, at every tile edge (tests/_pair_edges.py).

``Generator.run_resblock`` launches ONE ResBlock1 as the engine does — route 1: three fused-pair launches (resblock_pair_f32_k on an fp32 handle,
resblock_pair_x3_k on a bf16x3 one), route 2: the six convolutions one by one (conv1d_f32_mfma_k; option "kernels" = 1: the generic kernel),
route 0: resblock_x3_k — with per-utterance row counts and the epilogue mode of the caller's choice.  The lengths are the ones at which the
kernels' masks and clamps flip (tests/test_pair_edges_cpu.py shows that they reach each one both ways, and that the bars see planted faults);
the parameters are ``params_visible_bias``.  A ragged slot's tail holds NaN (even slots) or 1e4 N(0, 1) (odd slots) in x and a sentinel in y.

Bars: fp32  max|err| <= 4 e32 + 2^-22 max|want| per utterance (e32 class-wide: numpy's float32 run and a single-chain restatement, both on the
CPU);  bf16x3  max|err| / max|want| < 5e-5 per launch;  bit identities with torch.equal.

Measured on an MI355X, worst err / bar per launch kind over the twelve classes (test_report_worst_ratios prints them per class; DESIGN.md
§6l′ keeps the table): fp32 pairs 0.27 - 0.32, fp32 convolutions (tiles 1 and 2) 0.25 - 0.35, the generic kernel 0.25 - 0.35, bf16x3 pairs
0.10 - 0.14 of the 5e-5 bound; every bit identity held.  Not run: a build with a fault planted in a kernel.
"""
import numpy as np
import pytest
import torch

import _bf16_rb_ref as RB
import _launch_regimes as R
import _pair_edges as PE

pytestmark = pytest.mark.gpu

SEED = 20
MODES = ("store", "add", "mean")
_ids = lambda ck: f"C{ck[0]}k{ck[1]}"  # noqa: E731


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def P():
    return PE.params()


def _gen(dev, P, dtype):
    from viettts_amd.hifigan.config import V1
    from viettts_amd.hifigan.generator import Generator

    g = Generator(V1, device=dev, dtype=dtype)
    g.load_params(P)
    return g


@pytest.fixture(scope="module")
def gen_f32(dev, P):
    g = _gen(dev, P, "f32")
    yield g
    g.close()


@pytest.fixture(scope="module")
def gen_x3(dev, P):
    g = _gen(dev, P, "bf16x3")
    yield g
    g.close()


@pytest.fixture(scope="module")
def worst():
    """(engine / route, C, k) -> worst err / bar over the module's comparisons (test_report_worst_ratios prints it)"""
    return {}


# ---- references, cached per (class, length, seed, mode); e32 per class -----------------------------------------------------------------------
_REF, _E32 = {}, {}


def _want(P, C, k, L, seed, mode="store"):
    """fp64 reference [C, L] of utterance(C, L, seed) alone"""
    key = (C, k, L, seed, mode)
    if key not in _REF:
        x, acc0 = PE.utterance(C, L, seed)
        acc_add, div = PE.MODES[mode]
        _REF[key] = np.ascontiguousarray(PE.reference(P, C, k, x, acc0=acc0 if acc_add else None, div=div).T)
    return _REF[key]


def _e32(P, C, k):
    """the class's e32: numpy's float32 run against the fp64 reference over the class's edge utterances (store mode), and the single-chain
    restatement's error on its two lengths; CPU only"""
    if (C, k) not in _E32:
        e = max(max(c[1], c[2]) for c in PE.chain_errors(P, C, k))
        for L in PE.conv_route_lengths(C, k):
            x, _ = PE.utterance(C, L, SEED)
            e = max(e, float(np.abs(PE.reference(P, C, k, x, dtype=np.float32).T.astype(np.float64) - _want(P, C, k, L, SEED)).max()))
        _E32[(C, k)] = e
    return _E32[(C, k)]


def _launch(gen, dev, C, k, x, route, rows=None, mode="store", y0=None):
    """run_resblock on an fp32-layout handle: x / y0 numpy [B, C, LP] -> torch [B, C, LP] (y0 default: the sentinel everywhere)"""
    acc_add, div = PE.MODES[mode]
    y = torch.full(x.shape, PE.SENTINEL, device=dev) if y0 is None else torch.from_numpy(y0).to(dev)
    return gen.run_resblock(RB.resblock_key(C, k), torch.from_numpy(x).to(dev), route=route, rows=rows, acc_add=acc_add, div=div, out=y)


def _kept(got, y0, rows, what):
    """past rows[b] the in-out tensor holds what went in, bit for bit"""
    for b, L in enumerate(rows):
        assert np.array_equal(got[b, :, L:].view(np.uint32), y0[b, :, L:].view(np.uint32)), (what, b, L)


def _hold_f32(worst, label, P, C, k, got, want, what):
    """the fp32 bar on one utterance (or one window of it): got / want [C, n]"""
    err, bar = float(np.abs(got.astype(np.float64) - want).max()), PE.bar_f32(_e32(P, C, k), want)
    worst[(label, C, k)] = max(worst.get((label, C, k), 0.0), err / bar)
    assert np.isfinite(got).all(), what
    assert err <= bar, (what, err, bar, err / bar)


def _hold_x3(worst, label, C, k, gots, wants, what):
    """the bf16x3 bound on one launch: the scale is the launch's largest |want|"""
    scale = max(float(np.abs(w).max()) for w in wants)
    err = max(float(np.abs(g.astype(np.float64) - w).max()) for g, w in zip(gots, wants))
    worst[(label, C, k)] = max(worst.get((label, C, k), 0.0), err / scale / PE.X3_BOUND)
    assert all(np.isfinite(g).all() for g in gots), what
    assert err / scale < PE.X3_BOUND, (what, err, scale, err / scale)


def _ragged(gen, dev, C, k, lengths, route, mode="store", seed=SEED):
    """one ragged launch over ``lengths``: (case, y0, result as numpy)"""
    case = PE.ragged_case(C, lengths, seed)
    y0 = case["acc0"] if PE.MODES[mode][0] else case["y"]
    got = _launch(gen, dev, C, k, case["x"], route, rows=case["rows"], mode=mode, y0=y0).cpu().numpy()
    _kept(got, y0, case["rows"], (C, k, route, mode))
    return case, y0, got


# ---- 4a. fp32 pairs ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ck", PE.F32_PAIR_CLASSES, ids=_ids)
def test_fp32_pairs_at_every_tile_edge(gen_f32, dev, P, worst, ck):
    """resblock_pair_f32_k, route 1.  One ragged launch over pair_edge_lengths: every utterance against its own reference at the fp32 bar, the
    sentinel past rows[b].  Then plain launches (B = 2, rows of different content) at every edge length rounded up to a multiple of 4, both
    rows at the bar; where an edge length is a multiple of 4 the ragged utterance has the bits of the same utterance launched plain."""
    C, k = ck
    _, H, NT2, _, _ = PE.pair_geometry("f32", C, k)
    lengths = PE.pair_edge_lengths(H, NT2)
    case, _, got = _ragged(gen_f32, dev, C, k, lengths, 1)
    for b, L in enumerate(lengths):
        _hold_f32(worst, "f32 pairs", P, C, k, got[b, :, :L], _want(P, C, k, L, SEED), (ck, "ragged", L))
    same = 0
    for L4 in sorted({PE.roundup4(L) for L in lengths}):
        x, _ = PE.plain_case(C, L4, SEED)
        plain = _launch(gen_f32, dev, C, k, x, 1).cpu().numpy()
        for r in (0, 1):
            _hold_f32(worst, "f32 pairs", P, C, k, plain[r], _want(P, C, k, L4, SEED + r), (ck, "plain", L4, r))
        if L4 in lengths:
            same += 1
            assert np.array_equal(got[lengths.index(L4), :, :L4], plain[0]), (ck, L4)
    assert same >= 3, (ck, same)


# ---- 4b. bf16x3 pairs -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ck", PE.CLASSES, ids=_ids)
def test_x3_pairs_at_every_tile_edge(gen_x3, dev, P, worst, ck):
    """resblock_pair_x3_k, route 1.  The ragged launch at the bf16x3 bound, the sentinel past rows[b]; a plain launch (B = 2) at every edge length:
    the ragged utterance has the bits of the utterance launched plain, the second row meets the bound; where resblock_x3_k exists, route 0 has
    route 1's bits, ragged and plain, at these pair-tile lengths."""
    C, k = ck
    _, H, NT2, _, _ = PE.pair_geometry("x3", C, k)
    lengths = PE.pair_edge_lengths(H, NT2)
    has_rb = ck in RB.X3_RB_CLASSES
    case, _, got = _ragged(gen_x3, dev, C, k, lengths, 1)
    _hold_x3(worst, "x3 pairs", C, k, [got[b, :, :L] for b, L in enumerate(lengths)], [_want(P, C, k, L, SEED) for L in lengths], (ck, "ragged"))
    if has_rb:
        assert np.array_equal(_ragged(gen_x3, dev, C, k, lengths, 0)[2].view(np.uint32), got.view(np.uint32)), (ck, "route 0 ragged")
    for b, L in enumerate(lengths):
        x, _ = PE.plain_case(C, L, SEED)
        plain = _launch(gen_x3, dev, C, k, x, 1)
        if has_rb:
            assert torch.equal(_launch(gen_x3, dev, C, k, x, 0), plain), (ck, "route 0 plain", L)
        plain = plain.cpu().numpy()
        assert np.array_equal(got[b, :, :L], plain[0]), (ck, L)
        _hold_x3(worst, "x3 pairs", C, k, [plain[0], plain[1]], [_want(P, C, k, L, SEED), _want(P, C, k, L, SEED + 1)], (ck, "plain", L))


# ---- 4c. fp32 per-convolution launches ----------------------------------------------------------------------------------------------------
SETTINGS = [("tiles", 1), ("tiles", 2), ("kernels", 1)]


@pytest.mark.parametrize("ck", PE.CLASSES, ids=_ids)
def test_fp32_convolutions_one_by_one_at_every_tile_edge(gen_f32, dev, P, worst, ck):
    """route 2 on the fp32 handle (conv1d_f32_mfma_k wide and narrow, the generic kernel): a ragged launch over the pair edges and both ConvTiles'
    edges against the reference at the fp32 bar.  C <= 128 on the MFMA kernels: route 1 (the fused pairs) has route 2's bits in every epilogue
    mode, ragged and plain.  C = 256: route 1 is refused with VTTS_ERR_INVALID and the handle goes on working."""
    from viettts_amd import _lib

    C, k = ck
    lengths = PE.conv_route_lengths(C, k)
    _, H, NT2, R_, _ = PE.pair_geometry("f32" if C <= 128 else "x3", C, k)
    plain_lengths = [PE.roundup4(NT2 + 1), PE.roundup4(2 * NT2 + R_)]
    for name, value in SETTINGS:
        gen_f32.set_option(name, value)
        try:
            label = "f32 generic" if name == "kernels" else "f32 convs"
            case, _, got = _ragged(gen_f32, dev, C, k, lengths, 2)
            for b, L in enumerate(lengths):
                _hold_f32(worst, label, P, C, k, got[b, :, :L], _want(P, C, k, L, SEED), (ck, name, value, L))
            if name == "kernels":
                continue
            if C > 128:
                with pytest.raises(_lib.VttsError) as ei:
                    _launch(gen_f32, dev, C, k, case["x"], 1, rows=case["rows"])
                assert ei.value.status == -1
                assert np.array_equal(_ragged(gen_f32, dev, C, k, lengths, 2)[2].view(np.uint32), got.view(np.uint32)), (ck, "after the refusal")
                continue
            for mode in MODES:
                r2 = got if mode == "store" else _ragged(gen_f32, dev, C, k, lengths, 2, mode)[2]
                r1 = _ragged(gen_f32, dev, C, k, lengths, 1, mode)[2]
                assert np.array_equal(r1.view(np.uint32), r2.view(np.uint32)), (ck, name, value, mode, "ragged", float(np.nanmax(np.abs(r1 - r2))))
                for L4 in plain_lengths:
                    x, acc0 = PE.plain_case(C, L4, SEED)
                    y0 = acc0 if PE.MODES[mode][0] else None
                    assert torch.equal(_launch(gen_f32, dev, C, k, x, 1, mode=mode, y0=y0), _launch(gen_f32, dev, C, k, x, 2, mode=mode, y0=y0)), (
                        ck, name, value, mode, "plain", L4)
        finally:
            gen_f32.set_option(name, 0)


# ---- 4d. epilogue modes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ck", PE.CLASSES, ids=_ids)
def test_epilogue_modes_under_row_counts(gen_f32, gen_x3, dev, P, worst, ck):
    """store, accumulate (div 1) and accumulate-mean (div 3) on routes 1 and 2 of the fp32 handle and on route 1 of the bf16x3 handle at
    NT2 + 1 (one output in the second tile) and 2 NT2 + R, as one ragged launch and as plain launches (fp32: rounded up to a multiple of 4);
    past rows[b] the accumulator keeps its initial content."""
    C, k = ck
    routes = [("x3", gen_x3, 1, "x3 pairs")] + ([("f32", gen_f32, 1, "f32 pairs")] if C <= 128 else []) + [("f32" if C <= 128 else "x3", gen_f32, 2, "f32 convs")]
    for engine, gen, route, label in routes:
        _, H, NT2, R_, _ = PE.pair_geometry(engine, C, k)
        lengths = [NT2 + 1, 2 * NT2 + R_]
        x3 = gen is gen_x3
        for mode in MODES:
            _, _, got = _ragged(gen, dev, C, k, lengths, route, mode)
            gots, wants = [got[b, :, :L] for b, L in enumerate(lengths)], [_want(P, C, k, L, SEED, mode) for L in lengths]
            if x3:
                _hold_x3(worst, label, C, k, gots, wants, (ck, route, mode, "ragged"))
            else:
                for g, w, L in zip(gots, wants, lengths):
                    _hold_f32(worst, label, P, C, k, g, w, (ck, route, mode, "ragged", L))
            for L in lengths:
                Lp = L if x3 else PE.roundup4(L)
                x, acc0 = PE.plain_case(C, Lp, SEED)
                plain = _launch(gen, dev, C, k, x, route, mode=mode, y0=acc0 if PE.MODES[mode][0] else None).cpu().numpy()
                wants = [_want(P, C, k, Lp, SEED + r, mode) for r in (0, 1)]
                if x3:
                    _hold_x3(worst, label, C, k, [plain[0], plain[1]], wants, (ck, route, mode, "plain", Lp))
                else:
                    for r in (0, 1):
                        _hold_f32(worst, label, P, C, k, plain[r], wants[r], (ck, route, mode, "plain", Lp, r))


# ---- 4e. ragged slots in the XCD-aware tile order ---------------------------------------------------------------------------------------------
SLOT_TILES = 66


def _xcd_rows(NT2):
    return [66 * NT2 - 3, 64 * NT2, 63 * NT2 + 1, 9 * NT2 + 1, 7, 1]


def _windows(L, N1, NT2):
    """[a, e) of 2 N1 rows: the utterance's start, every seam (r nt) >> 3 of its own tile count, its end"""
    spans = [(0, min(2 * N1, L))] + [(max(s * NT2 - N1, 0), min(s * NT2 + N1, L)) for s in RB.xcd_seams(R.cdiv(L, NT2))] + [(max(L - 2 * N1, 0), L)]
    return sorted({s for s in spans if s[1] > s[0]})


def test_xcd_slot_shape():
    """66 tiles per slot take the XCD-aware order (from 64 tiles per grid row) on a grid padded to 72, while every utterance but the first has a
    tile count of its own"""
    for engine, key in (("f32", "FP_XCD_MIN_TILES"), ("x3", "X3_XCD_MIN_TILES")):
        for C, k in ((32, 3), (64, 7)):
            _, _, NT2, _, _ = PE.pair_geometry(engine, C, k)
            rows = _xcd_rows(NT2)
            LP = PE.roundup4(max(rows))
            assert R.cdiv(LP, NT2) == SLOT_TILES >= R.THRESHOLDS[key] and SLOT_TILES % R.XCDS != 0
            assert [R.cdiv(L, NT2) for L in rows] == [66, 64, 64, 10, 1, 1]


@pytest.mark.parametrize("engine", ["f32", "x3"])
@pytest.mark.parametrize("ck", [(32, 3), (64, 7)], ids=_ids)
def test_ragged_slot_in_the_xcd_order(gen_f32, gen_x3, dev, P, worst, ck, engine):
    """xcd_tile takes nt from the utterance and gridDim.x from the slot: each utterance against references computed on slices (halo 18 H + 4
    rows) on windows of 2 N1 rows at its start, at every seam of its own tile count and at its end; the sentinel past rows[b]; launched
    twice, because the batch direction alternates from launch to launch."""
    C, k = ck
    gen = gen_f32 if engine == "f32" else gen_x3
    N1, H, NT2, _, _ = PE.pair_geometry(engine, C, k)
    rows = _xcd_rows(NT2)
    halo = 18 * H + 4
    case = PE.ragged_case(C, rows, SEED + 5)
    outs = [_launch(gen, dev, C, k, case["x"], 1, rows=rows).cpu().numpy() for _ in range(2)]
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), (ck, engine)
    got = outs[0]
    _kept(got, case["y"], rows, (ck, engine))
    gots, wants = [], []
    for b, L in enumerate(rows):
        for a, e in _windows(L, N1, NT2):
            lo, hi = max(a - halo, 0), min(e + halo, L)
            xs = np.ascontiguousarray(case["x"][b, :, lo:hi].T)
            want = PE.reference(P, C, k, xs)[a - lo:e - lo].T
            if engine == "f32":
                _hold_f32(worst, "f32 pairs", P, C, k, got[b, :, a:e], want, (ck, "xcd", b, a, e))
            gots.append(got[b, :, a:e])
            wants.append(want)
    if engine == "x3":
        _hold_x3(worst, "x3 pairs", C, k, gots, wants, (ck, "xcd"))


# ---- 4f. the figures --------------------------------------------------------------------------------------------------------------------------
def test_report_worst_ratios(worst, capsys):
    """worst err / bar per launch kind and class over the comparisons above (fp32: the class's e32 too)"""
    with capsys.disabled():
        for label in sorted({q[0] for q in worst}):
            cells = [f"C{C}k{k} {worst[(lb, C, k)]:.2f}" for lb, C, k in sorted(worst, key=lambda q: (-q[1], q[2])) if lb == label]
            print(f"\n[{label}] worst err / bar: " + "  ".join(cells))
        print("\n[e32 per class] " + "  ".join(f"C{C}k{k} {v:.2e}" for (C, k), v in sorted(_E32.items(), key=lambda q: (-q[0][0], q[0][1]))))
    assert worst and all(v <= 1.0 for v in worst.values())
