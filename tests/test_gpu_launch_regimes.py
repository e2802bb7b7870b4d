"""Every kernel family on its LARGE-launch paths, element by element against the fp64 oracle (oracle/hifigan_oracle.py).

The per-kernel tests of test_gpu_parity.py, test_gpu_bf16.py and test_gpu_x3.py run at B = 2 and L <= 1203, where every launch takes its kernel's
small-launch code.  The product runs long utterances and the benchmark's batch on other code: the wide time tiles, the XCD-aware tile order with its
padded grid (a workgroup past its eighth of the tiles exits at once), the bf16x3 upsamplers' staged row stores.  The lengths here are computed from
tests/_launch_regimes.py (checked against the sources by tests/test_launch_regime_table_cpu.py) so that each launch lands inside such a path, or
exactly on a threshold's edge (threshold - 1, threshold, threshold + 1 tiles, the last one partial).

Conventions are the existing KATs': fp32 / bf16x3 handles take channel-major [B, C, L], bf16 handles channels-last [B, L, C] with the operands
rounded to bf16 on the oracle's side; the bounds are the ones those tests assert (fp32 2e-5 absolute; bf16 convolution 2^-8 and bf16 pair 2^-7 of
max|ref|; bf16x3 3e-5 of max|ref|).  Every element of every launch is compared with the oracle of its own input.  Outputs of fp32 / bf16x3 launches
are pre-filled with NaN, so a tile that is never written cannot pass on stale memory.  Batches have B >= 3 rows of different content: consecutive
launches walk the batch in alternating directions (engine.hip: next_zrev), so a wrong row mapping shows."""
import numpy as np
import pytest
import torch

import _launch_regimes as R
from oracle import hifigan_oracle as orc
from viettts_amd.hifigan.config import V1
from viettts_amd.hifigan.synth import synthetic_mel, synthetic_params
from viettts_amd.hifigan.weights import conv_specs

pytestmark = pytest.mark.gpu

B = 3
TIGHT = 2e-5          # fp32 kernels (test_gpu_parity.py)
X3_REL = 3e-5         # bf16x3 kernels, relative to max|ref| (test_gpu_x3.py)
X3_BOUND = 5e-5       # bf16x3 whole generator / stage (test_gpu_x3.py: BOUND)
BF16_MAXABS, BF16_SNR_DB = 0.03, 38.0  # bf16 whole generator (test_gpu_bf16.py)
TH = R.THRESHOLDS
DEEP = 8              # "deep in the regime": this many tiles (one more round of the 8 XCDs) past a tile-count threshold


def bf(x):
    """round-to-nearest-even to bf16, returned as float64 (as tests/test_gpu_bf16.py)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def _nwc(x):
    return np.ascontiguousarray(np.transpose(x, (0, 2, 1)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def v1_params():
    return synthetic_params(V1, 4321, "scaled")


@pytest.fixture(scope="module")
def gens(dev, v1_params):
    from viettts_amd.hifigan.generator import Generator

    out = {}
    for dt in ("f32", "bf16", "bf16x3"):
        g = Generator(V1, device=dev, dtype=dt)
        g.load_params(v1_params)
        out[dt] = g
    yield out
    for g in out.values():
        g.close()


def _pair_specs(C, k):
    """(convs1, convs2) of the V1 ResBlock pair with C channels, kernel size k and the widest rate (5)"""
    specs = conv_specs(V1)
    for i, s in enumerate(specs):
        if s.kind == "conv" and "convs1_" in s.key and s.cin == C and s.k == k and s.dilation == 5:
            return s, specs[i + 1]
    raise AssertionError((C, k))


def _first(pred, start, step=1):
    L = start
    while not pred(L):
        L += step
    return L


def _partial(L, *nts):
    return all(L % nt for nt in nts)


def _seeded_x(shape, seed):
    """B rows of different content (standard normal x 2, as the existing KATs)"""
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32) * 2.0


def _nan_out(shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def _report(what, err, scale=None):
    msg = f"[{what}] max|err| {err:.3e}" + (f" ({err / scale:.2e} of max|ref| {scale:.2f})" if scale is not None else "")
    print("\n" + msg, flush=True)


# ================================================================================================================================================
# fp32-layout engines: conv1d_f32_mfma_k (fp32 per-convolution path), resblock_pair_f32_k, resblock_pair_x3_k — one length per (C, k) class that is
# deep in all three kernels' large-launch regimes; one fp64 oracle shared by the three (and by the tile variants of the convolution)
# ================================================================================================================================================
def _fx_length(C, k):
    def ok(L):
        if L % 4 or not R.f32_conv_wide(C, L, B) or R.cdiv(L, R.F32_CONV_DECISION[C][0]) * R.F32_CONV_DECISION[C][1] * B < TH["F32_MIN_WGS"] + DEEP * B:
            return False
        if R.f32_conv_tiles(C, L, B) < TH["F32_XCD_MIN_TILES"] + DEEP or R.x3_pair_tiles(C, k, L) < TH["X3_XCD_MIN_TILES"] + DEEP:
            return False
        if C in R.F32_PAIR_N1 and R.f32_pair_tiles(C, k, L) < TH["FP_XCD_MIN_TILES"] + DEEP:
            return False
        nts = [R.F32_CONV_NT_WIDE[C], R.F32_CONV_NT_NARROW[C], R.X3_PAIR_N1[C][k] - (k - 1)] + ([R.F32_PAIR_N1[C] - (k - 1)] if C in R.F32_PAIR_N1 else [])
        return _partial(L, *nts)

    return _first(ok, 4, 4)


def _fx_cases():
    out = []
    for C in (256, 128, 64, 32):
        for k in (3, 7, 11):
            L = _fx_length(C, k)
            rid = f"C{C}k{k}d5-L{L}-f32conv-wide-xcd-{R.f32_conv_tiles(C, L, B)}tiles"
            if C in R.F32_PAIR_N1:
                rid += f"-f32pair-xcd-{R.f32_pair_tiles(C, k, L)}tiles"
            rid += f"-x3pair-xcd-{R.x3_pair_tiles(C, k, L)}tiles"
            out.append(pytest.param(C, k, L, id=rid))
    return out


def _pair_ref64(params, c1, c2, xn):
    """oracle c2(lrelu(c1(lrelu(x)))) + x in fp64 (vietTTS/hifigan/model.py:45-50): (c1's output, the pair's output), NWC"""
    w1, b1 = params[c1.key]["w"].astype(np.float64), params[c1.key]["b"].astype(np.float64)
    w2, b2 = params[c2.key]["w"].astype(np.float64), params[c2.key]["b"].astype(np.float64)
    xt = orc.conv1d(orc.leaky_relu(xn, 0.1), w1, b1, c1.dilation, orc.get_padding(c1.k, c1.dilation))
    return xt, orc.conv1d(orc.leaky_relu(xt, 0.1), w2, b2, 1, orc.get_padding(c2.k, 1)) + xn


def _check_fx_pairs(gens, dev, c1, x, ref, what):
    """the fp32 pair (where it covers C) and the bf16x3 pair on x, twice each (both batch directions), into NaN-filled outputs"""
    xd = torch.from_numpy(x).to(dev)
    scale = float(np.abs(ref).max())
    engines = (["f32"] if c1.cin in R.F32_PAIR_N1 else []) + ["bf16x3"]
    for dt in engines:
        for rep in range(2):
            y = gens[dt].run_pair(c1.key, xd, out=_nan_out(x.shape, dev))
            torch.cuda.synchronize()
            assert bool(torch.isfinite(y).all()), (dt, what, rep, "elements left unwritten")
            err = float(np.abs(_nwc(y.cpu().numpy()) - ref).max())
            _report(f"{dt} pair {what} rep {rep}", err, scale)
            if dt == "f32":
                assert err < TIGHT, (what, err)
            else:
                assert err / scale < X3_REL, (what, err, scale)


@pytest.mark.parametrize("C,k,L", _fx_cases())
def test_fp32_layout_kernels_large_launch(gens, v1_params, dev, C, k, L):
    """conv1d_f32_mfma_k (convs1 of the class, rate 5) under tiles = 0 (auto: the wide tile here), 1 (wide) and 2 (narrow), every variant with the XCD
    order on; then resblock_pair_f32_k (C <= 128; L % 4 == 0) and resblock_pair_x3_k on the same input.  One fp64 oracle for all of them: c1's
    output is what the convolution computes, the pair's output what the pair kernels compute."""
    c1, c2 = _pair_specs(C, k)
    assert R.f32_conv_wide(C, L, B) and all(R.f32_conv_tiles(C, L, B, t) >= TH["F32_XCD_MIN_TILES"] for t in (0, 1, 2))
    x = _seeded_x((B, C, L), 7000 + C * 10 + k)
    xt_ref, ref = _pair_ref64(v1_params, c1, c2, _nwc(x).astype(np.float64))
    g = gens["f32"]
    xd = torch.from_numpy(x).to(dev)
    try:
        for tiles in (0, 1, 2):
            g.set_option("tiles", tiles)
            y = g.run_module(c1.key, xd, 0.1, out=_nan_out((B, C, L), dev))
            torch.cuda.synchronize()
            assert bool(torch.isfinite(y).all()), (tiles, "elements left unwritten")
            err = float(np.abs(_nwc(y.cpu().numpy()) - xt_ref).max())
            _report(f"f32 conv C={C} k={k} d=5 L={L} tiles={tiles} ({R.f32_conv_tiles(C, L, B, tiles)} tiles per row)", err)
            assert err < TIGHT, (tiles, err)
    finally:
        g.set_option("tiles", 0)
    _check_fx_pairs(gens, dev, c1, x, ref, f"C={C} k={k} d=5 L={L}")


def _fx_edge_cases():
    out = []
    # conv1d_f32_mfma_k, class C = 128, k = 3: the wide/narrow edge (workgroups of the decision tile = MIN_WGS - B, MIN_WGS, MIN_WGS + B at B = 3) ...
    nt, mt = R.F32_CONV_DECISION[128]
    n0 = R.cdiv(TH["F32_MIN_WGS"], mt * B)
    for n in (n0 - 1, n0, n0 + 1):
        L = R.length_for_tiles(n, nt, 4)
        out.append(pytest.param("conv", 128, 3, B, L, id=f"f32conv-C128k3d5-{'wide' if R.f32_conv_wide(128, L, B) else 'narrow'}-edge-{n * mt * B}wgs-L{L}"))
    # ... and the XCD edge of the WIDE tile (B = 8 keeps 63 tiles per row wide)
    for n in (TH["F32_XCD_MIN_TILES"] - 1, TH["F32_XCD_MIN_TILES"], TH["F32_XCD_MIN_TILES"] + 1):
        L = R.length_for_tiles(n, R.F32_CONV_NT_WIDE[128], 4)
        assert R.f32_conv_wide(128, L, 8)
        out.append(pytest.param("conv", 128, 3, 8, L, id=f"f32conv-C128k3d5-wide-xcd-edge-{n}tiles-B8-L{L}"))
    # the fp32 and bf16x3 pairs, class C = 64, k = 3: both have 254 outputs per tile and the XCD order from 64 tiles
    nt2 = R.F32_PAIR_N1[64] - 2
    assert nt2 == R.X3_PAIR_N1[64][3] - 2 and TH["FP_XCD_MIN_TILES"] == TH["X3_XCD_MIN_TILES"]
    for n in (TH["FP_XCD_MIN_TILES"] - 1, TH["FP_XCD_MIN_TILES"], TH["FP_XCD_MIN_TILES"] + 1):
        L = R.length_for_tiles(n, nt2, 4)
        out.append(pytest.param("pair", 64, 3, B, L, id=f"f32pair-x3pair-C64k3d5-xcd-edge-{n}tiles-L{L}"))
    return out


@pytest.mark.parametrize("what,C,k,nb,L", _fx_edge_cases())
def test_fp32_layout_threshold_edges(gens, v1_params, dev, what, C, k, nb, L):
    """Threshold - 1, threshold and threshold + 1 tiles per row, the last tile partial: the first padded grid, its exit-early workgroups, and the
    last launch order without them."""
    c1, c2 = _pair_specs(C, k)
    x = _seeded_x((nb, C, L), 8000 + L)
    xt_ref, ref = _pair_ref64(v1_params, c1, c2, _nwc(x).astype(np.float64)) if what == "pair" else (None, None)
    if what == "conv":
        w1, b1 = v1_params[c1.key]["w"].astype(np.float64), v1_params[c1.key]["b"].astype(np.float64)
        xt_ref = orc.conv1d(orc.leaky_relu(_nwc(x).astype(np.float64), 0.1), w1, b1, c1.dilation, orc.get_padding(c1.k, c1.dilation))
        for rep in range(2):
            y = gens["f32"].run_module(c1.key, torch.from_numpy(x).to(dev), 0.1, out=_nan_out((nb, C, L), dev))
            torch.cuda.synchronize()
            assert bool(torch.isfinite(y).all()), (rep, "elements left unwritten")
            err = float(np.abs(_nwc(y.cpu().numpy()) - xt_ref).max())
            _report(f"f32 conv edge C={C} k={k} B={nb} L={L} ({R.f32_conv_tiles(C, L, nb)} tiles per row) rep {rep}", err)
            assert err < TIGHT, (rep, err)
    else:
        _check_fx_pairs(gens, dev, c1, x, ref, f"edge C={C} k={k} L={L} ({R.x3_pair_tiles(C, k, L)} tiles per row)")


# ================================================================================================================================================
# bf16 engine: resblock_pair_g_bf16_k — wide and narrow tiles, the XCD order from 192 tiles per utterance slot
# ================================================================================================================================================
def _bf16_length(C, k):
    nw, nn = R.bf16_pair_nt2(C, k, False), R.bf16_pair_nt2(C, k, True)
    return _first(lambda L: R.bf16_pair_wide(C, L, B) and R.bf16_pair_tiles(C, k, L, B) >= TH["XCD_MAP_MIN_TILES"] + DEEP and _partial(L, nw, nn),
                  (TH["XCD_MAP_MIN_TILES"] + DEEP - 1) * nw)


def _bf16_cases():
    out = []
    for C in (256, 128, 64, 32):
        for k in (3, 7, 11):
            L = _bf16_length(C, k)
            out.append(pytest.param(C, k, L, id=f"C{C}k{k}d5-L{L}-wide-xcd-{R.bf16_pair_tiles(C, k, L, B)}tiles-narrow-xcd-{R.bf16_pair_tiles(C, k, L, B, 2)}tiles"))
    # one class at the edges: C = 32, k = 3.  Wide/narrow: the decision counts k = 11 wide tiles (NT2 502), workgroups = tiles x B around G_MIN_WGS ...
    n0 = R.cdiv(TH["G_MIN_WGS"], B)
    nt11 = R.bf16_pair_nt2(32, 11, False)
    for n in (n0 - 1, n0, n0 + 1):
        L = _first(lambda L: R.cdiv(L, nt11) == n and _partial(L, R.bf16_pair_nt2(32, 3, False), R.bf16_pair_nt2(32, 3, True)), R.length_for_tiles(n, nt11))
        out.append(pytest.param(32, 3, L, id=f"C32k3d5-L{L}-{'wide' if R.bf16_pair_wide(32, L, B) else 'narrow'}-edge-{n * B}wgs"))
    # ... and the XCD edge of the wide tile (NT2 510)
    nt = R.bf16_pair_nt2(32, 3, False)
    for n in (TH["XCD_MAP_MIN_TILES"] - 1, TH["XCD_MAP_MIN_TILES"], TH["XCD_MAP_MIN_TILES"] + 1):
        L = R.length_for_tiles(n, nt)
        assert R.bf16_pair_wide(32, L, B)
        out.append(pytest.param(32, 3, L, id=f"C32k3d5-L{L}-wide-xcd-edge-{n}tiles"))
    return out


@pytest.mark.parametrize("C,k,L", _bf16_cases())
def test_bf16_pair_large_launch(gens, v1_params, dev, C, k, L):
    """resblock_pair_g_bf16_k under tiles = 0 (auto), 1 (wide) and 2 (narrow) against the oracle on the same bf16-rounded operands (xt rounded where
    the kernel rounds it), 2^-7 of max|ref| as test_fused_pair_kat_bf16; and bit-identical across the three (kernels_bf16_rbg.hip: the narrow tile has
    the wide one's per-element accumulation order).  The bf16 handle converts from a bf16 buffer the engine allocates per call, which may be the
    memory of the call before: so every checked call follows a call on a decoy input (-x) of the same shape, and a repeat of tiles = 0 follows two
    decoys (the other batch direction)."""
    c1, c2 = _pair_specs(C, k)
    x = np.ascontiguousarray(_nwc(_seeded_x((B, C, L), 9000 + C * 10 + k)))
    w1, b1 = v1_params[c1.key]["w"], v1_params[c1.key]["b"]
    w2, b2 = v1_params[c2.key]["w"], v1_params[c2.key]["b"]
    xin = bf(orc.leaky_relu(bf(x), 0.1))
    xt = bf(orc.leaky_relu(orc.conv1d(xin, bf(w1), b1.astype(np.float64), c1.dilation, orc.get_padding(c1.k, c1.dilation)), 0.1))
    del xin
    ref = orc.conv1d(xt, bf(w2), b2.astype(np.float64), 1, orc.get_padding(c2.k, 1)) + bf(x)
    del xt
    scale = float(np.abs(ref).max())
    g = gens["bf16"]
    xd, decoy = torch.from_numpy(x).to(dev), torch.from_numpy(-x).to(dev)
    outs = {}
    try:
        for tiles, n_decoy in ((0, 1), (1, 1), (2, 1), (0, 2)):
            g.set_option("tiles", tiles)
            for _ in range(n_decoy):
                g.run_pair(c1.key, decoy)
            y = g.run_pair(c1.key, xd)
            torch.cuda.synchronize()
            err = float(np.abs(y.cpu().numpy() - ref).max())
            _report(f"bf16 pair C={C} k={k} d=5 L={L} tiles={tiles} ({R.bf16_pair_tiles(C, k, L, B, tiles)} tiles per row, "
                    f"{'wide' if R.bf16_pair_wide(C, L, B, tiles) else 'narrow'})", err, scale)
            assert err <= 2.0 ** -7 * scale, (tiles, err, scale)
            if tiles in outs:
                assert torch.equal(outs[tiles], y), "the same launch in the other batch direction differs"
            outs[tiles] = y
    finally:
        g.set_option("tiles", 0)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), float((outs[0] - outs[2]).abs().max())


# ================================================================================================================================================
# bf16x3 upsamplers ups_2 / ups_3 (convt_x3_k, UX2 / UX3): staged fp32 row stores, several tiles, a partial last tile, odd L (output rows of 2 L
# floats: a row pitch of 2 mod 4), one length of >= 64 tiles
# ================================================================================================================================================
def _ups_cases():
    out = []
    for i in (2, 3):
        n1 = R.X3_UPS_N1[i]
        for L, what in ((3 * n1 + 77, "odd-4tiles"), (5 * n1 + 130, "even-6tiles"), (64 * n1 + 33, "odd-65tiles"), (80 * n1 + 2, "even-81tiles")):
            out.append(pytest.param(i, L, id=f"ups{i}-staged-{what}-L{L}"))
    return out


@pytest.mark.parametrize("i,L", _ups_cases())
def test_x3_upsampler_staged_stores(gens, v1_params, dev, i, L):
    """convt_x3_k's staged epilogue writes whole output rows as 16-byte units, and the two-float tail unit where an odd L leaves half of one: every
    sample of a NaN-filled output must be written and equal the oracle's conv1d_transpose(lrelu(x, 0.1)) (vietTTS/hifigan/model.py:112-114)."""
    spec = [s for s in conv_specs(V1) if s.key == f"generator/~/ups_{i}"][0]
    x = _seeded_x((B, spec.cin, L), 600 + 10 * i + L % 7)
    w, b = v1_params[spec.key]["w"], v1_params[spec.key]["b"]
    ref = orc.conv1d_transpose(orc.leaky_relu(_nwc(x).astype(np.float64), 0.1), w.astype(np.float64), b.astype(np.float64), spec.stride)
    scale = float(np.abs(ref).max())
    shape = (B, spec.cout, L * spec.stride)
    for rep in range(2):
        y = gens["bf16x3"].run_module(spec.key, torch.from_numpy(x).to(dev), 0.1, out=_nan_out(shape, dev))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(y).all()), (rep, "elements left unwritten", int((~torch.isfinite(y)).sum()))
        err = float(np.abs(_nwc(y.cpu().numpy()) - ref).max())
        _report(f"bf16x3 ups_{i} L={L} ({R.cdiv(L, R.X3_UPS_N1[i])} tiles) rep {rep}", err, scale)
        assert err / scale < X3_REL, (rep, err, scale)


# ================================================================================================================================================
# whole-ResBlock kernels (resblock_bf16_k, resblock_x3_k), stage by stage: the MRF output of a stage against the oracle's three ResBlocks and their
# mean computed on the engine's OWN stage input (tap ups_i), so that the error of earlier stages does not enter
# ================================================================================================================================================
MRF_T = 360  # frames: every stage with a whole-ResBlock kernel runs it in its XCD order (asserted below from the window geometry)
WHOLE_RB = {  # (engine, fuse) -> the (C, k) classes that run as one whole-ResBlock launch (engine.hip: resblock_*_preferred / _supported)
    ("bf16", 2): [(32, 3), (32, 7), (64, 3)],
    ("bf16", 3): [(32, 3), (32, 7), (32, 11), (64, 3), (128, 3)],
    ("bf16x3", 2): [(32, 3), (32, 7), (32, 11), (64, 3), (64, 7), (128, 3)],
    ("bf16x3", 3): [(32, 3), (32, 7), (32, 11), (64, 3), (64, 7), (128, 3)],
}


def _mrf_windows(engine, C, k, T):
    L = T * {256: 8, 128: 64, 64: 128, 32: 256}[C]
    W = (R.BF16_RB_W if engine == "bf16" else R.X3_RB_W)[C][k]
    return R.cdiv(L, R.rb_window_nt(W, k))


@pytest.fixture(scope="module")
def mrf_oracle_cache():
    return {}


def _mrf_ref(params, i, x):
    """model.py:116-121: the mean of the stage's three ResBlocks, fp64, NWC"""
    ys = [orc.resblock1(params, 3 * i + j, x, int(V1.resblock_kernel_sizes[j]), V1.resblock_dilation_sizes[j]) for j in range(3)]
    return (ys[0] + ys[1] + ys[2]) / 3.0


# bf16: each of a ResBlock's three pairs meets 2^-7 of its output's range against the oracle on the same bf16 operands (test_fused_pair_kat_bf16);
# chained, a pair hands its error on to the next through the residual path (gain ~1) and adds its own: <= 3 x 2^-7 per ResBlock, unchanged by the
# mean of three.  The weights of the oracle are bf16-rounded, its intermediates are not: the bound allows the same again, 6 x 2^-7 of the stage's
# range (observed on the MI355X: 5.6-6.3e-3 of the range, printed).
BF16_MRF_REL = 6 * 2.0 ** -7


@pytest.mark.parametrize("engine,fuse", [("f32", 2), ("bf16x3", 1), ("bf16x3", 2), ("bf16x3", 3), ("bf16", 2), ("bf16", 3)],
                         ids=["f32-default", "bf16x3-fuse1-pairs", "bf16x3-fuse2-rbx3-xcd", "bf16x3-fuse3-rbx3-xcd", "bf16-fuse2-rbbf16-xcd",
                              "bf16-fuse3-rbbf16-xcd"])
def test_stage_mrf_vs_oracle_on_the_stage_input(gens, v1_params, dev, mrf_oracle_cache, engine, fuse):
    """Every stage i = 0..3 at B = 1 x T = 360: forward_tap(mel, "ups_i") is the stage input, forward_tap(mel, "mrf_i") its output; the oracle runs
    oracle.resblock1 over the stage's three ResBlocks and the mean on that input.  The whole-ResBlock kernels were only compared with the pair path
    before.  Bounds: fp32 2e-5; bf16x3 the 5e-5 of test_gpu_x3.py relative to the stage's range; bf16 BF16_MRF_REL (see above) relative to the range of
    the activated stage output the bf16 engine stores (LeakyReLU of the next layer applied: 0.1, 0.01 after the last stage)."""
    thr = TH["RB_BF16_XCD_MIN"] if engine == "bf16" else TH["RX_XCD_MIN_TILES"]
    for C, k in WHOLE_RB.get((engine, fuse), []):
        assert _mrf_windows(engine, C, k, MRF_T) >= thr, (C, k, _mrf_windows(engine, C, k, MRF_T), thr)
    g = gens[engine]
    params = v1_params
    if engine == "bf16":
        params = {key: {"w": bf(m["w"]), "b": m["b"].astype(np.float64)} for key, m in v1_params.items()}
    mel = torch.from_numpy(synthetic_mel(1, MRF_T, 4242)).to(dev)
    g.set_option("fuse", fuse)
    try:
        for i in range(4):
            C = V1.upsample_initial_channel >> (i + 1)
            L = MRF_T * int(np.prod(V1.upsample_rates[: i + 1]))
            _, xin = g.forward_tap(mel, f"ups_{i}")
            _, got = g.forward_tap(mel, f"mrf_{i}")
            torch.cuda.synchronize()
            xin, got = xin.cpu().numpy(), got.cpu().numpy()
            if engine == "bf16":
                xin, got = xin.reshape(1, L, C), got.reshape(1, L, C)
            else:
                xin, got = _nwc(xin.reshape(1, C, L)), _nwc(got.reshape(1, C, L))
            key = (engine == "bf16", i, xin.tobytes().__hash__())
            if key not in mrf_oracle_cache:
                mrf_oracle_cache[key] = _mrf_ref(params, i, xin.astype(np.float64))
            ref = mrf_oracle_cache[key]
            if engine == "bf16":
                ref = orc.leaky_relu(ref, 0.1 if i + 1 < len(V1.upsample_rates) else 0.01)
            err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
            wins = {ck: _mrf_windows(engine, *ck, MRF_T) for ck in WHOLE_RB.get((engine, fuse), []) if ck[0] == C}
            _report(f"{engine} fuse={fuse} mrf_{i} C={C} L={L} whole-ResBlock windows {wins}", err, scale)
            if engine == "f32":
                assert err < TIGHT, (i, err)
            elif engine == "bf16x3":
                assert err / scale < X3_BOUND, (i, err, scale)
            else:
                assert err / scale <= BF16_MRF_REL, (i, err, scale)
    finally:
        g.set_option("fuse", 2)


# ================================================================================================================================================
# one dense whole-generator check: all 131 072 samples of B = 1 x T = 512
# ================================================================================================================================================
@pytest.fixture(scope="module")
def dense_t512(golden_dir, v1_params):
    import json

    rec = json.load(open(golden_dir / "golden_meta.json"))["cases"]["v1_scaled_T512"]
    g = np.load(golden_dir / "v1_scaled_T512.npz")
    assert (rec["B"], rec["T"], rec["wseed"], rec["kind"]) == (1, 512, 4321, "scaled")
    mel = synthetic_mel(1, 512, rec["mseed"])
    y, pre = orc.generator_forward(v1_params, mel, V1, np.float64, return_pre_tanh=True)
    y, pre = y[0, :, 0], pre[0, :, 0]
    # pinned to the reference: the oracle equals the reference generator's fp64 output on the golden's strided samples
    e_golden = float(np.abs(y[g["idx"]] - g["y64"][0]).max())
    assert e_golden < 1e-12, e_golden
    return mel, y, pre


@pytest.mark.parametrize("engine", ["f32", "bf16x3", "bf16"])
def test_whole_generator_dense_T512(gens, dev, dense_t512, engine):
    """Every sample, not the golden's 1.6 %: fp32 2e-5, bf16x3 5e-5, bf16 the BF16_MAXABS / BF16_SNR_DB of test_gpu_bf16.py."""
    mel, want_y, want_pre = dense_t512
    g = gens[engine]
    if engine == "bf16":
        wav, pre = g.forward_tap(torch.from_numpy(mel).to(dev), "pre_tanh")
        wav, pre = wav.cpu().numpy()[0].astype(np.float64), pre.cpu().numpy()[0].astype(np.float64)
    else:
        out = _nan_out((1, 256 * 512), dev)
        wav = g(torch.from_numpy(mel).to(dev), out).cpu().numpy()[0].astype(np.float64)
    assert np.isfinite(wav).all()
    e_y = float(np.abs(wav - want_y).max())
    if engine == "bf16":
        snr = float(10 * np.log10((want_pre ** 2).mean() / ((pre - want_pre) ** 2).mean()))
        _report(f"bf16 whole generator B=1 T=512, all samples (pre-tanh SNR {snr:.1f} dB)", e_y)
        assert e_y < BF16_MAXABS and snr > BF16_SNR_DB, (e_y, snr)
    else:
        _report(f"{engine} whole generator B=1 T=512, all samples", e_y)
        assert e_y < (TIGHT if engine == "f32" else X3_BOUND), e_y


def test_out_argument_of_the_module_hooks(gens, dev):
    """run_module / run_pair write into a caller's tensor and check it as __call__ does"""
    c1, _ = _pair_specs(64, 3)
    x = torch.from_numpy(_seeded_x((1, 64, 100), 1)).to(dev)
    g = gens["f32"]
    out = _nan_out((1, 64, 100), dev)
    assert g.run_pair(c1.key, x, out=out) is out and torch.equal(out, g.run_pair(c1.key, x))
    assert g.run_module(c1.key, x, 0.1, out=out) is out and torch.equal(out, g.run_module(c1.key, x, 0.1))
    for bad in (torch.empty((1, 64, 99), device=dev), torch.empty((1, 64, 100), dtype=torch.float64, device=dev),
                torch.empty((1, 100, 64), device=dev).transpose(1, 2), torch.empty((1, 64, 100))):
        with pytest.raises(ValueError):
            g.run_pair(c1.key, x, out=bad)
        with pytest.raises(ValueError):
            g.run_module(c1.key, x, 0.1, out=bad)
