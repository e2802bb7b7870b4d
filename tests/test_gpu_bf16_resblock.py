"""The bf16 ResBlock kernels alone, with biases the bounds can see (tests/_bf16_rb_ref.py).

``Generator.run_resblock`` (vtts_hifigan_run_resblock) launches ONE ResBlock1 the way the engine does — route 0: the whole-ResBlock kernel
(resblock_bf16_k, kernels_bf16_rbk.hip; on a bf16x3 handle resblock_x3_k), route 1: three fused-pair launches — with the epilogue mode and the
per-utterance row counts of the caller's choice.  The lengths are the window edges ``edge_lengths`` computes per class, which a whole forward
(lengths that are multiples of 8 .. 256 rows) never reaches; the parameters are ``params_visible_bias``, under which a dropped, swapped or
mis-indexed bias moves the output by several times the bars (tests/test_bf16_rb_ref_cpu.py shows both on the CPU).

Both bars against the fp64 reference that rounds where the kernels round (``_bf16_rb_ref.bars``):
  (i)  max|err| <= 2^-7 (max|p0| + max|p1| + max|final|);   (ii) rel-rms <= 4 x the fp32 restatement's own, recomputed per case.
"""
import numpy as np
import pytest
import torch

import _bf16_rb_ref as RB
import _launch_regimes as R
from oracle import hifigan_oracle as orc
from viettts_amd.hifigan.config import V1
from viettts_amd.hifigan.synth import synthetic_mel
from viettts_amd.hifigan.weights import conv_specs

pytestmark = pytest.mark.gpu

SENTINEL = 1536.0  # bf16-exact, far outside every output's range
MODES = [(0, 1.0, 1.0), (1, 1.0, 1.0), (1, 3.0, 0.1), (1, 3.0, 0.01)]  # (acc_add, div, slope_out): store, accumulate, accumulate-divide-LeakyReLU
X3_BOUND = 5e-5  # tests/test_gpu_x3.py: BOUND, relative to the output's range
_ids = lambda ck: f"C{ck[0]}k{ck[1]}"  # noqa: E731
bf = RB.bf


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def params():
    return RB.params_visible_bias(V1, 4321)


@pytest.fixture(scope="module")
def gen(dev, params):
    from viettts_amd.hifigan.generator import Generator

    g = Generator(V1, device=dev, dtype="bf16")
    g.load_params(params)
    yield g
    g.close()


@pytest.fixture(scope="module")
def gen_x3(dev, params):
    from viettts_amd.hifigan.generator import Generator

    g = Generator(V1, device=dev, dtype="bf16x3")
    g.load_params(params)
    yield g
    g.close()


@pytest.fixture(scope="module")
def worst():
    """worst err / bar per class over the module's bf16 comparisons: test_report_worst_ratios prints it (DESIGN.md records it)"""
    return {}


def _inputs(C, L, seed, B=2):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, L, C)) * 2.0).astype(np.float32)
    acc0 = rng.standard_normal((B, L, C)).astype(np.float32)
    return x, acc0


def _refs(params, C, k, x, acc0, mode):
    """(ref64, pairs64, ref32) of ``x`` [B', L', C] in epilogue mode (acc_add, div, slope_out)"""
    acc_add, div, slope = mode
    W, b = RB.resblock_wb(params, C, k)
    kw = dict(acc0=acc0 if acc_add else None, div=div, slope_out=slope)
    ref64, pairs = RB.resblock_ref(x, W, b, k, RB.DILS, np.float64, **kw)
    ref32, _ = RB.resblock_ref(x, W, b, k, RB.DILS, np.float32, **kw)
    return ref64, pairs, ref32


def _hold(worst, ck, got, refs, what):
    """both bars; the figures are kept for the module's printout"""
    ref64, pairs, ref32 = refs
    e1, b1, e2, b2 = RB.bars(got, ref64, pairs, ref32)
    w = worst.setdefault(ck, [0.0, 0.0, 0.0])
    w[0], w[1], w[2] = max(w[0], e1 / b1), max(w[1], e2 / b2), max(w[2], b2 / RB.BAR_II_FACTOR)
    assert np.isfinite(got).all(), what
    assert e1 <= b1, (what, "bar (i)", e1, b1)
    assert e2 <= b2, (what, "bar (ii)", e2, b2)


def _run(gen, dev, C, k, x, route=0, rows=None, mode=(0, 1.0, 1.0), y0=None):
    """run_resblock on a bf16 handle: numpy [B, L, C] in and out; y0 = the in-out tensor's initial content (default: the sentinel)"""
    acc_add, div, slope = mode
    y = torch.full(x.shape, SENTINEL, device=dev) if y0 is None else torch.from_numpy(y0).to(dev)
    out = gen.run_resblock(RB.resblock_key(C, k), torch.from_numpy(x).to(dev), route=route, rows=rows, slope_out=slope, acc_add=bool(acc_add),
                           div=div, out=y)
    return out.cpu().numpy()


# ---- 1. the whole-ResBlock kernel against the reference, at every window edge -----------------------------------------------------------
@pytest.mark.parametrize("ck", RB.BF16_RB_CLASSES, ids=_ids)
def test_whole_resblock_at_every_window_edge(gen, dev, params, worst, ck):
    """Store mode, B = 2, y pre-filled with a sentinel: every row written and inside both bars.  Then the same length as a row batch
    rows = [L, max(1, L - NT + 3)]: rows below rows[b] against the reference of that utterance ALONE (its zero padding starts at rows[b]),
    rows at and past rows[b] still the sentinel."""
    C, k = ck
    W, M, NT = RB.rb_geometry(R.BF16_RB_W, C, k)
    for L in RB.edge_lengths(W, M, NT):
        x, _ = _inputs(C, L, C * 10000 + k * 100 + L % 97)
        refs = _refs(params, C, k, x, None, MODES[0])
        got = _run(gen, dev, C, k, x)
        _hold(worst, ck, got, refs, (ck, L, "plain"))
        rows = [L, max(1, L - NT + 3)]
        got = _run(gen, dev, C, k, x, rows=rows)
        _hold(worst, ck, got[0:1], _refs(params, C, k, x[0:1], None, MODES[0]), (ck, L, "rows[0]"))
        n1 = rows[1]
        _hold(worst, ck, got[1:2, :n1], _refs(params, C, k, x[1:2, :n1], None, MODES[0]), (ck, L, "rows[1]", n1))
        assert (got[1, n1:] == SENTINEL).all(), (ck, L, n1)


def test_run_resblock_rejects_what_it_cannot_run(gen, gen_x3, dev):
    from viettts_amd import _lib

    x = torch.zeros((1, 64, 32), device=dev)
    for key, route, C in (("generator/~/res_block1_9/~/convs2_0", 0, 32), ("generator/~/res_block1_9/~/convs1_1", 1, 32), ("generator/~/ups_0", 0, 32),
                          ("generator/~/nope", 1, 32), (RB.resblock_key(32, 3), 2, 32), (RB.resblock_key(256, 3), 0, 256)):  # (no whole-ResBlock kernel at C = 256)
        with pytest.raises(_lib.VttsError):
            gen.run_resblock(key, torch.zeros((1, 64, C), device=dev), route=route)
    with pytest.raises(_lib.VttsError):
        gen.run_resblock(RB.resblock_key(32, 3), x, slope_out=1.5)
    with pytest.raises(_lib.VttsError):
        gen.run_resblock(RB.resblock_key(32, 3), x, div=0.0)
    with pytest.raises(_lib.VttsError):  # the fp32 engine's epilogues have no output activation
        gen_x3.run_resblock(RB.resblock_key(32, 3), torch.zeros((1, 32, 64), device=dev), slope_out=0.1)
    # the ragged state of a refused or finished call does not leak into the next forward
    mel = torch.from_numpy(synthetic_mel(1, 8, 3)).to(dev)
    base = gen(mel).clone()
    gen.run_resblock(RB.resblock_key(32, 3), x, rows=[5])
    assert torch.equal(gen(mel), base)


# ---- 2. the epilogue modes, on the whole-ResBlock kernel and on the pair kernel ------------------------------------------------------------
@pytest.mark.parametrize("ck", RB.BF16_RB_CLASSES, ids=_ids)
def test_epilogue_modes_on_both_routes(gen, dev, params, worst, ck):
    """store / accumulate / accumulate-divide-LeakyReLU(0.1 | 0.01) at L = NT + 1 (window 1 holds one row) and 2 NT + M (window 1 interior), the
    accumulator N(0, 1): route 0 and route 1 (the pair kernel's accumulate and divide epilogues had no test of their own) against the reference.
    Store mode: route 0 within bar (i) of three run_pair calls."""
    C, k = ck
    W, M, NT = RB.rb_geometry(R.BF16_RB_W, C, k)
    for L in (NT + 1, 2 * NT + M):
        x, acc0 = _inputs(C, L, C * 777 + k * 13 + L)
        for mode in MODES:
            refs = _refs(params, C, k, x, acc0, mode)
            for route in (0, 1):
                got = _run(gen, dev, C, k, x, route=route, mode=mode, y0=acc0 if mode[0] else None)
                _hold(worst, ck, got, refs, (ck, L, mode, "route", route))
        cur = torch.from_numpy(x).to(dev)
        for z in range(3):
            cur = gen.run_pair(RB.resblock_key(C, k, z), cur)
        ref64, pairs, _ = _refs(params, C, k, x, None, MODES[0])
        bar_i = RB.BAR_I_REL * sum(float(np.abs(p).max()) for p in (pairs[0], pairs[1], ref64))
        err = float(np.abs(_run(gen, dev, C, k, x) - cur.cpu().numpy()).max())
        assert err <= bar_i, (ck, L, err, bar_i)


# ---- 3. wide == narrow tiles on route 1 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ck", RB.BF16_RB_CLASSES, ids=_ids)
def test_pair_route_wide_and_narrow_tiles_give_the_same_bits(gen, dev, ck):
    """option "tiles" = 1 (wide) and 2 (narrow) on the three pair launches: the same bits at every window edge length (the wide == narrow
    contract of tests/test_gpu_bf16_mfma16*.py), in the accumulate-divide-LeakyReLU mode."""
    C, k = ck
    W, M, NT = RB.rb_geometry(R.BF16_RB_W, C, k)
    try:
        for L in RB.edge_lengths(W, M, NT):
            x, acc0 = _inputs(C, L, C * 31 + k + L)
            out = {}
            for tiles in (1, 2):
                gen.set_option("tiles", tiles)
                out[tiles] = _run(gen, dev, C, k, x, route=1, mode=MODES[2], y0=acc0)
            assert np.array_equal(out[1], out[2]), (ck, L, float(np.abs(out[1] - out[2]).max()))
    finally:
        gen.set_option("tiles", 0)


# ---- 4. the XCD order of resblock_bf16_k, exactly at its switch ---------------------------------------------------------------------------
def _windows(ntv, NT, W, Lb):
    """[a, e) of 2 W rows: the start, the seams between two XCDs' eighths of ntv windows, the utterance's end"""
    spans = [(0, min(2 * W, Lb))] + [(max(s * NT - W, 0), min(s * NT + W, Lb)) for s in RB.xcd_seams(ntv)] + [(max(Lb - 2 * W, 0), Lb)]
    return sorted(set(spans))


@pytest.mark.parametrize("windows,rows1", [(191, None), (192, None), (197, 100 * 232 + 7)], ids=["191-launch-order", "192-xcd-order", "197-ragged"])
def test_xcd_order_switch_of_the_whole_resblock_kernel(gen, dev, params, worst, windows, rows1):
    """C = 32, k = 3 (NT = 232): 191 windows keep the launch order, 192 take the XCD-aware one (a padded grid, each XCD a contiguous eighth of the
    utterance's own windows, rotated per utterance), and a 197-window slot whose second utterance holds 101.  Route 0 against the reference on
    windows of 2 W rows (the start, every seam (rx ntv) >> 3 of each utterance's own tile count, each utterance's end), route 0 within bar (i)
    of route 1 on every row, the sentinel past rows[b]."""
    C, k = 32, 3
    W, M, NT = RB.rb_geometry(R.BF16_RB_W, C, k)
    thr = R.THRESHOLDS["RB_BF16_XCD_MIN"]
    L = {191: 191 * NT, 192: 191 * NT + 1, 197: 196 * NT + 100}[windows]
    assert R.cdiv(L, NT) == windows and (windows >= thr) == (windows != 191) and thr == 192
    rows = [L, rows1] if rows1 else None
    lens = rows or [L, L]
    x, _ = _inputs(C, L, 4000 + windows)
    got0 = _run(gen, dev, C, k, x, route=0, rows=rows)
    got1 = _run(gen, dev, C, k, x, route=1, rows=rows)
    halo = 64  # > M: a row's dependency cone lies inside the slice (or ends at the utterance's own edge, where the slice ends too)
    peak = [0.0, 0.0, 0.0]
    for b, Lb in enumerate(lens):
        assert (got0[b, Lb:] == SENTINEL).all() and (got1[b, Lb:] == SENTINEL).all(), (windows, b)
        for a, e in _windows(R.cdiv(Lb, NT), NT, W, Lb):
            lo, hi = max(a - halo, 0), min(e + halo, Lb)
            ref64, pairs, ref32 = _refs(params, C, k, x[b : b + 1, lo:hi], None, MODES[0])
            cut = lambda r: r[:, a - lo : e - lo]  # noqa: E731
            _hold(worst, (C, k), got0[b : b + 1, a:e], (cut(ref64), [cut(p) for p in pairs], cut(ref32)), (windows, b, a, e))
            peak = [max(p, float(np.abs(cut(q)).max())) for p, q in zip(peak, (pairs[0], pairs[1], ref64))]
    for b, Lb in enumerate(lens):
        err = float(np.abs(got0[b, :Lb] - got1[b, :Lb]).max())
        assert err <= RB.BAR_I_REL * sum(peak), (windows, b, err, peak)


def test_report_worst_ratios(worst, capsys):
    """the figures of the comparisons above (sections 1, 2 and 4), per class: worst error / bar for both bars, and the largest rel-rms of the
    fp32 restatement itself (bar (ii) is four times it)"""
    with capsys.disabled():
        for ck in sorted(worst):
            w = worst[ck]
            print(f"\n[bf16 ResBlock C={ck[0]} k={ck[1]}] worst err / bar: (i) {w[0]:.3f}  (ii) {w[1]:.3f};  restatement rel-rms up to {w[2]:.5f}")
    assert all(w[0] <= 1.0 and w[1] <= 1.0 for w in worst.values())


# ---- 5. bias-visible known-answer tests for the rest of the bf16 engine -----------------------------------------------------------------
# The cases, references and bounds of tests/test_gpu_bf16.py (test_resblock_conv_kat_bf16, test_fused_pair_kat_bf16, test_upsample_kat_bf16, the
# conv_pre half of test_conv_pre_and_post_bf16) under params_visible_bias, at one short length each: two tiles and a ragged rest.
CONV_NT = {256: 256, 128: 128, 64: 256, 32: 256}                              # kernels_bf16.hip: BRes<C> NT
UPS_TILE = {3: {0: 64, 1: 128, 2: 256, 3: 512}, 0: {0: 128, 1: 128, 2: 128, 3: 256}}  # frames per tile: kernels_bf16_up.hip UT<i> / kernels_bf16.hip BUp<i>
REST = 37


def _res_conv_cases():
    seen, out = set(), []
    for s in conv_specs(V1):
        if s.kind == "conv" and s.cin == s.cout and (s.cin, s.k, s.dilation) not in seen:
            seen.add((s.cin, s.k, s.dilation))
            out.append(s)
    return out


def _pair_cases():
    by = {s.key: s for s in conv_specs(V1)}
    return [(s, by[s.key.replace("convs1_", "convs2_")]) for s in _res_conv_cases() if "convs1_" in s.key]


@pytest.mark.parametrize("spec", _res_conv_cases(), ids=lambda s: f"C{s.cin}k{s.k}d{s.dilation}")
def test_resblock_conv_kat_bf16_visible_bias(gen, params, dev, spec):
    rng = np.random.default_rng(spec.cin * 1000 + spec.k * 10 + spec.dilation)
    B, L = 2, 2 * CONV_NT[spec.cin] + REST
    x = rng.standard_normal((B, L, spec.cin)).astype(np.float32) * 2.0
    res = rng.standard_normal((B, L, spec.cin)).astype(np.float32)
    w, b = params[spec.key]["w"], params[spec.key]["b"]
    xin = bf(orc.leaky_relu(bf(x), 0.1))
    ref = orc.conv1d(xin, bf(w), b.astype(np.float64), spec.dilation, orc.get_padding(spec.k, spec.dilation)) + bf(res)
    y = gen.run_module(spec.key, torch.from_numpy(x).to(dev), 0.1, torch.from_numpy(res).to(dev)).cpu().numpy()
    assert np.abs(y - ref).max() <= 2.0 ** -8 * np.abs(ref).max(), (np.abs(y - ref).max(), np.abs(ref).max())
    assert np.abs(y - bf(ref)).max() <= 2.0 ** -7 * np.abs(ref).max()


@pytest.mark.parametrize("pair", _pair_cases(), ids=lambda p: f"C{p[0].cin}k{p[0].k}d{p[0].dilation}")
def test_fused_pair_kat_bf16_visible_bias(gen, params, dev, pair):
    c1, c2 = pair
    rng = np.random.default_rng(c1.cin * 100 + c1.k * 10 + c1.dilation)
    B = 2
    L = 2 * R.bf16_pair_nt2(c1.cin, c1.k, not R.bf16_pair_wide(c1.cin, 1100, B)) + REST
    x = rng.standard_normal((B, L, c1.cin)).astype(np.float32) * 2.0
    w1, b1 = params[c1.key]["w"], params[c1.key]["b"]
    w2, b2 = params[c2.key]["w"], params[c2.key]["b"]
    xin = bf(orc.leaky_relu(bf(x), 0.1))
    xt = orc.conv1d(xin, bf(w1), b1.astype(np.float64), c1.dilation, orc.get_padding(c1.k, c1.dilation))
    xt = bf(orc.leaky_relu(xt, 0.1))
    ref = orc.conv1d(xt, bf(w2), b2.astype(np.float64), 1, orc.get_padding(c2.k, 1)) + bf(x)
    y = gen.run_pair(c1.key, torch.from_numpy(x).to(dev)).cpu().numpy()
    err = np.abs(y - ref).max()
    assert err <= 2.0 ** -7 * np.abs(ref).max(), (err, np.abs(ref).max())


@pytest.mark.parametrize("fuse", [3, 0], ids=["register-streamed", "first-generation"])
@pytest.mark.parametrize("i", [0, 1, 2, 3])
def test_upsample_kat_bf16_visible_bias(gen, params, dev, i, fuse):
    spec = [s for s in conv_specs(V1) if s.key == f"generator/~/ups_{i}"][0]
    rng = np.random.default_rng(40 + i)
    B, L = 2, 2 * UPS_TILE[fuse][i] + REST
    x = rng.standard_normal((B, L, spec.cin)).astype(np.float32) * 2.0
    w, b = params[spec.key]["w"], params[spec.key]["b"]
    ref = orc.conv1d_transpose(bf(x), bf(w), b.astype(np.float64), spec.stride)
    gen.set_option("fuse", fuse)
    try:
        y = gen.run_module(spec.key, torch.from_numpy(x).to(dev), 1.0).cpu().numpy()
    finally:
        gen.set_option("fuse", 2)
    assert y.shape == (B, L * spec.stride, spec.cout)
    assert np.abs(y - ref).max() <= 2.0 ** -8 * np.abs(ref).max()


@pytest.mark.parametrize("fuse", [2, 0], ids=["register-streamed", "first-generation"])
def test_conv_pre_kat_bf16_visible_bias(gen, params, dev, fuse):
    mel = synthetic_mel(2, 2 * 128 + REST, 5)  # both conv_pre kernels' tiles are 128 frames (UTP, BPre)
    w, b = params["generator/~/conv1_d"]["w"], params["generator/~/conv1_d"]["b"]
    ref = orc.conv1d(bf(mel), bf(w), b.astype(np.float64), 1, 3)
    gen.set_option("fuse", fuse)
    try:
        y = gen.run_module("generator/~/conv1_d", torch.from_numpy(mel).to(dev), 1.0).cpu().numpy()
    finally:
        gen.set_option("fuse", 2)
    assert np.abs(y - ref).max() <= 2.0 ** -8 * np.abs(ref).max()


# ---- 6. bf16x3: the whole-ResBlock kernel promises the bits of three pair launches (x3_common.h) -----------------------------------------
@pytest.mark.parametrize("ck", RB.X3_RB_CLASSES, ids=_ids)
def test_x3_whole_resblock_equals_three_pair_launches_at_every_window_edge(gen_x3, dev, params, ck, capsys):
    """route 0 (resblock_x3_k) torch.equal route 1 (three resblock_pair_x3_k launches) at every window edge of its RXTile that both routes accept,
    in store mode and in accumulate-divide mode (acc 1, div 3; the fp32 engines' epilogues have no output activation: slope_out stays 1), with
    and without row counts; route 0 against the fp64 reference on unrounded operands at test_gpu_x3.py's bound relative to the range."""
    from viettts_amd import _lib

    C, k = ck
    W, M, NT = RB.rb_geometry(R.X3_RB_W, C, k)
    key = RB.resblock_key(C, k)
    Wt, b = RB.resblock_wb(params, C, k)
    ran, worst_rel = 0, 0.0
    for L in RB.edge_lengths(W, M, NT):
        x, acc0 = _inputs(C, L, C * 500 + k * 7 + L)
        xc = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).to(dev)  # [B, C, L]
        ac = torch.from_numpy(np.ascontiguousarray(acc0.transpose(0, 2, 1))).to(dev)
        try:
            outs = {}
            for acc_add, div in ((0, 1.0), (1, 3.0)):
                for rows in (None, [L, max(1, L - NT + 3)]):
                    pair = []
                    for route in (0, 1):
                        y = ac.clone() if acc_add else torch.full_like(xc, SENTINEL)
                        pair.append(gen_x3.run_resblock(key, xc, route=route, rows=rows, acc_add=bool(acc_add), div=div, out=y).clone())
                    torch.cuda.synchronize()
                    assert torch.equal(pair[0], pair[1]), (ck, L, acc_add, rows, float((pair[0] - pair[1]).abs().max()))
                    outs[(acc_add, rows is None)] = pair[0]
                    if rows is not None:
                        keep = ac if acc_add else torch.full_like(xc, SENTINEL)
                        assert torch.equal(pair[0][1, :, rows[1]:], keep[1, :, rows[1]:]), (ck, L, acc_add)
        except _lib.VttsError as e:
            if e.status != -1:  # VTTS_ERR_INVALID: a length one of the routes does not take
                raise
            continue
        ran += 1
        for acc_add, div in ((0, 1.0), (1, 3.0)):
            ref, _ = RB.resblock_ref(x, Wt, b, k, RB.DILS, np.float64, acc0=acc0 if acc_add else None, div=div, rounded=False)
            got = outs[(acc_add, True)].cpu().numpy().transpose(0, 2, 1)
            rel = float(np.abs(got - ref).max() / np.abs(ref).max())
            worst_rel = max(worst_rel, rel)
            assert rel < X3_BOUND, (ck, L, acc_add, rel)
    with capsys.disabled():
        print(f"\n[bf16x3 ResBlock C={C} k={k}] {ran} edge lengths, route 0 == route 1 bit for bit; worst max|err| / max|ref| vs fp64 {worst_rel:.2e}")
    assert ran >= 10, (ck, ran)


# ---- 7. the bf16 ragged forward in the XCD-aware tile order ---------------------------------------------------------------------------------
FRAMES, T_RAGGED = [400, 333, 1, 177], 400


def test_ragged_shape_reaches_the_xcd_order():
    """stage 4 of a 400-frame slot: >= 192 windows / tiles per slot for the whole-ResBlock kernel (k = 3, 7 at fuse 2; k = 11 too at fuse 3) and
    for the pair kernel's launched tile at every "tiles" setting, while utterance 3 (177 frames) has fewer of its own"""
    hop, B = V1.hop, len(FRAMES)
    L, L3 = hop * T_RAGGED, hop * FRAMES[3]
    for k in (3, 7, 11):
        NT = R.rb_window_nt(R.BF16_RB_W[32][k], k)
        assert R.cdiv(L, NT) >= R.THRESHOLDS["RB_BF16_XCD_MIN"] and R.cdiv(L3, NT) < R.cdiv(L, NT)
        for tiles in (0, 1, 2):
            nt2 = R.bf16_pair_nt2(32, k, not R.bf16_pair_wide(32, L, B, tiles))
            assert R.bf16_pair_tiles(32, k, L, B, tiles) == R.cdiv(L, nt2) >= R.THRESHOLDS["XCD_MAP_MIN_TILES"] and R.cdiv(L3, nt2) < R.cdiv(L, nt2)


@pytest.mark.parametrize("tiles", [0, 1, 2])
@pytest.mark.parametrize("fuse", [1, 2, 3])
def test_bf16_ragged_forward_in_the_xcd_order(gen, dev, fuse, tiles):
    """forward_ragged at a slot length whose stage-4 launches take the XCD-aware order (the kernels take the tile count from the utterance's own
    length, the order and the grid padding from the slot's): each utterance bit for bit the utterance alone, the rest of its slot zero; the
    un-ragged forward of the same batch agrees on the full-length utterance and is finite."""
    mel = torch.from_numpy(synthetic_mel(len(FRAMES), T_RAGGED, 77)).to(dev)
    hop = V1.hop
    gen.set_option("fuse", fuse)
    gen.set_option("tiles", tiles)
    try:
        got = gen.forward_ragged(mel, FRAMES).clone()
        plain = gen(mel).clone()
        for b, n in enumerate(FRAMES):
            alone = gen(mel[b : b + 1, :n].contiguous())
            assert torch.equal(got[b, : hop * n], alone[0]), (fuse, tiles, b, n)
            assert not bool(got[b, hop * n :].any()), (fuse, tiles, b)
        assert torch.equal(plain[0], got[0]) and bool(torch.isfinite(plain).all())
    finally:
        gen.set_option("fuse", 2)
        gen.set_option("tiles", 0)
