"""The generator on every kind of config ``vtts_hifigan_create()`` accepts (tests/_gen_configs.py): mixed routes — MFMA tiles,
fused pairs, the split-operand kernels and the generic kernels inside one generator or one ResBlock —, MRFs of 1, 2 and 4 ResBlocks, 1, 3 and 8
upsample stages, transposed convolutions off k == 2 * stride, other mel counts, ResBlock2 at MFMA channel counts.  Everything is compared with the
fp64 oracle (oracle/hifigan_oracle.py) at the bars the engines already answer to on V1:

  fp32    TIGHT = 2e-5 on the waveform (tests/test_gpu_parity.py)
  bf16x3  5e-5 on the waveform (tests/test_gpu_x3.py: BOUND)
  bf16    max|dy| < 0.03 and pre-tanh SNR > 38 dB (tests/test_gpu_bf16.py: _edge_check, restated here)

One handle per (entry, engine) for the whole module.  Shapes are tiny: B <= 3, T <= 13 frames."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import _gen_configs as gc
from oracle import hifigan_oracle as orc
from viettts_amd._handle import ptr
from viettts_amd.hifigan.synth import synthetic_mel
from viettts_amd.hifigan.weights import conv_specs

pytestmark = pytest.mark.gpu

TIGHT = gc.TIGHT
X3_BOUND = 5e-5  # tests/test_gpu_x3.py: BOUND, the split-operand engine's whole-generator bar
BF16_MAXABS, BF16_SNR_DB = 0.03, 38.0  # tests/test_gpu_bf16.py
WAVE_BAR = {"f32": TIGHT, "bf16x3": X3_BOUND}
DEFAULTS = {"kernels": 0, "tiles": 0, "fuse": 2, "chains": 1, "streams": 0, "microbatch": 0, "graph": 1}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def handles(dev):
    """handles(name, engine) -> the module's one Generator of that entry on that engine, weights loaded; all closed at the end."""
    from viettts_amd.hifigan.generator import Generator

    pool = {}

    def get(name, engine):
        if (name, engine) not in pool:
            g = Generator(gc.BY_NAME[name].cfg, device=dev, dtype=engine)
            pool[(name, engine)] = g
            g.load_params(gc.params(name))
        return pool[(name, engine)]

    try:
        yield get
    finally:
        for g in pool.values():
            g.close()


@contextlib.contextmanager
def options(gen, **kw):
    try:
        for k, v in kw.items():
            gen.set_option(k, v)
        yield gen
    finally:
        for k in kw:
            gen.set_option(k, DEFAULTS[k])


def _nwc(x_ncw):
    return np.ascontiguousarray(np.transpose(x_ncw, (0, 2, 1)))


def _ncw(x_nwc):
    return np.ascontiguousarray(np.transpose(x_nwc, (0, 2, 1)))


def _forward_tap(gen, mel, tap):
    """Generator.forward_tap with both outputs pre-filled with NaN: a sample no kernel writes is seen."""
    B, T, _ = mel.shape
    n = C.c_size_t(0)
    gen._call("tap_elems", tap.encode(), B, T, C.byref(n))
    tap_t = torch.full((int(n.value),), float("nan"), dtype=torch.float32, device=gen.device)
    out = torch.full((B, gen.hop * T), float("nan"), dtype=torch.float32, device=gen.device)
    ws = gen._workspace(gen.workspace_bytes(B, T))
    gen._on_stream("forward_tap", ptr(mel), B, T, ptr(out), ptr(ws), ws.numel(), tail=(tap.encode(), ptr(tap_t)))
    torch.cuda.synchronize()
    return out.cpu().numpy(), tap_t.cpu().numpy()


def _run(gen, mel):
    out = torch.full((mel.shape[0], gen.hop * mel.shape[1]), float("nan"), dtype=torch.float32, device=gen.device)
    return gen(mel, out)


def _dmel(name, T, dev, B=gc.BATCH):
    return torch.from_numpy(np.array(gc.mel(name, T, B))).to(dev)


# --------------------------------------------------------------------------------------------------------------------------------
# a. the whole generator against the fp64 oracle (f: DEEP8 at T = 5 and T = 6 on one handle is two of these runs — the receptive-field
#    comparison of the two lengths has no samples to compare, tests/test_gen_configs_cpu.py::test_deep8_five_frames_have_no_interior)
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", gc.cases(), ids=gc.case_id)
def test_generator_vs_oracle(handles, dev, case, capsys):
    entry, engine = case
    gen = handles(entry.name, engine)
    worst_y, worst_p, worst_snr = 0.0, 0.0, 1e9
    for T in entry.frames:
        want_y, want_pre, _ = gc.oracle(entry.name, T)
        wav, pre = _forward_tap(gen, _dmel(entry.name, T, dev), "pre_tanh")
        pre = pre.reshape(wav.shape)
        assert wav.shape == want_y.shape == (gc.BATCH, entry.cfg.hop * T)
        assert np.isfinite(wav).all() and np.isfinite(pre).all(), (entry.name, engine, T, "samples no kernel wrote")
        e_y = float(np.abs(wav - want_y).max())
        e_p = float(np.abs(pre - want_pre).max() / max(1.0, np.abs(want_pre).max()))
        snr = float(10 * np.log10((want_pre ** 2).mean() / max(((pre - want_pre) ** 2).mean(), 1e-300)))
        worst_y, worst_p, worst_snr = max(worst_y, e_y), max(worst_p, e_p), min(worst_snr, snr)
        with capsys.disabled():
            print(f"\n[{entry.name} {engine} T={T}] max|dy| {e_y:.3e}  max|d pre-tanh| / max(1, max|pre|) {e_p:.3e}  pre-tanh SNR {snr:.1f} dB")
        if engine == "bf16":
            assert e_y < BF16_MAXABS and snr > BF16_SNR_DB, (entry.name, T, e_y, snr)
        else:
            assert e_y < WAVE_BAR[engine] and e_p < WAVE_BAR[engine], (entry.name, engine, T, e_y, e_p)


# --------------------------------------------------------------------------------------------------------------------------------
# b. the taps localise: conv_pre, every ups_i and every mrf_i
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", gc.cases(("f32", "bf16x3")), ids=gc.case_id)
def test_every_tap_vs_oracle(handles, dev, case):
    entry, engine = case
    gen = handles(entry.name, engine)
    for T in entry.frames:
        want_y, _, taps = gc.oracle(entry.name, T)
        mel = _dmel(entry.name, T, dev)
        for tap in gc.tap_names(entry.cfg):
            want = taps[tap]  # [B, L, C]
            wav, got = _forward_tap(gen, mel, tap)
            got = _nwc(got.reshape(gc.BATCH, want.shape[2], want.shape[1]))
            assert np.isfinite(got).all(), (tap, T)
            rel = float(np.abs(got - want).max() / np.abs(want).max())
            assert rel < WAVE_BAR[engine], (entry.name, engine, T, tap, rel)
            assert np.abs(wav - want_y).max() < WAVE_BAR[engine], (tap, T)  # a tap changes nothing downstream


# --------------------------------------------------------------------------------------------------------------------------------
# c. per-module known answers on the layers only these configs have
# --------------------------------------------------------------------------------------------------------------------------------
KAT_LENGTHS = (268, 134, 37)  # L % 4 == 0 / == 2 / odd; more than one tile of every MFMA kernel (64 .. 256 columns)
NEW_LAYERS = gc.new_layers()


def _mfma_eligible(s):
    return s.kind == "conv" and s.cin == s.cout and s.cin in (32, 64, 128, 256) and s.k in (3, 7, 11) and s.dilation <= 5


def _role(s):
    return {"generator/~/conv1_d": "pre", "generator/~/conv1_d_1": "post"}.get(s.key, s.kind)


def _kat_case(entry, s, L):
    """(x as the fp32 handle takes it, res or None, slope_in, fp64 reference [B, Lout, Cout])"""
    p = gc.params(entry.name)[s.key]
    w, b = p["w"].astype(np.float64), p["b"].astype(np.float64)
    rng = np.random.default_rng([s.cin, s.cout, s.k, s.dilation, s.stride, L])
    role = _role(s)
    if role == "pre":
        x = synthetic_mel(2, L, 50 + L, s.cin)
        return x, None, 1.0, orc.conv1d(x.astype(np.float64), w, b, 1, 3)
    x = rng.standard_normal((2, s.cin, L)).astype(np.float32) * 2.0
    xn = _nwc(x).astype(np.float64)
    if role == "post":
        return x, None, 0.01, np.tanh(orc.conv1d(orc.leaky_relu(xn, 0.01), w, b, 1, 3))
    if role == "convT":
        return x, None, 0.1, orc.conv1d_transpose(orc.leaky_relu(xn, 0.1), w, b, s.stride)
    res = rng.standard_normal((2, s.cout, L)).astype(np.float32)
    return x, res, 0.1, orc.conv1d(orc.leaky_relu(xn, 0.1), w, b, s.dilation, orc.get_padding(s.k, s.dilation)) + _nwc(res)


@pytest.mark.parametrize("name", [e.name for e in gc.TABLE if NEW_LAYERS[e.name]])
def test_new_layer_kats_f32(handles, dev, name, capsys):
    """run_module on every module signature (kind, Cin, Cout, k, dilation, stride) that V1 / TINY / TINY2 do not have, with LeakyReLU on load and
    (ResBlock convolutions) a residual: the engine's own choice of kernel (at MFMA-eligible layers both tile widths) and the generic kernels, at a
    length the float4 kernels take, one they refuse at run time and an odd one.  Transposed convolutions: every output phase — those that own no
    tap are bias only — against the oracle's zero-stuffed definition.  max|err| < TIGHT as in tests/test_gpu_parity.py::test_resblock_conv_kat
    (unit-scale inputs); conv_pre reads log-mels of magnitude up to 11.5 and its outputs reach +-25, so its error is taken relative to the
    output's max-abs, as for the taps above (a chain of up to 896 fp32 additions at partial sums of that size rounds by ~1e-6 of it)."""
    entry = gc.BY_NAME[name]
    gen = handles(name, "f32")
    worst = (0.0, None)
    for s in NEW_LAYERS[name]:
        for L in KAT_LENGTHS:
            x, res, slope, ref = _kat_case(entry, s, L)
            xd = torch.from_numpy(x).to(dev)
            rd = torch.from_numpy(res).to(dev) if res is not None else None
            if s.kind == "convT":
                assert gen.run_module(s.key, xd, slope).shape == ref.transpose(0, 2, 1).shape == (2, s.cout, L * s.stride)
            for kernels, tiles in [(0, 0), (1, 0)] + ([(0, 1), (0, 2)] if _mfma_eligible(s) else []):
                y = torch.full((2, s.cout, L * s.stride), float("nan"), dtype=torch.float32, device=dev)
                with options(gen, kernels=kernels, tiles=tiles):
                    gen.run_module(s.key, xd, slope, rd, out=y)
                    torch.cuda.synchronize()
                err = float(np.abs(_nwc(y.cpu().numpy()) - ref).max())  # NaN where nothing was written
                if _role(s) == "pre":
                    err /= float(np.abs(ref).max())
                worst = max(worst, (err, (s.key, L, kernels, tiles)))
                assert err < TIGHT, (s.key, gc.signature(s), L, kernels, tiles, err)
    with capsys.disabled():
        print(f"\n[{name} fp32 KATs, {len(NEW_LAYERS[name])} new signatures x L in {KAT_LENGTHS}] worst max|err| {worst[0]:.3e} at {worst[1]}")


def _new_pairs(name):
    specs = conv_specs(gc.BY_NAME[name].cfg)
    by = {s.key: i for i, s in enumerate(specs)}
    return [(s, specs[by[s.key] + 1]) for s in NEW_LAYERS[name] if "convs1_" in s.key and _mfma_eligible(s)]


@pytest.mark.parametrize("name", [e.name for e in gc.TABLE if _new_pairs(e.name)])
def test_new_pair_kats(handles, dev, name):
    """The fused pair kernels on the (C, k, rate) only these configs have (rates 2 and 4): x' = c2(lrelu(c1(lrelu(x)))) + x (model.py:45-50) in fp64.
    fp32 pair (C <= 128, L % 4 == 0): TIGHT, and the same bits as the two convolution launches (tests/test_gpu_parity.py::test_fp32_fused_pair_kat);
    split-operand pair (every L): 3e-5 of the output's magnitude (tests/test_gpu_x3.py::test_x3_pair_kat)."""
    p = gc.params(name)
    f32, x3 = handles(name, "f32"), handles(name, "bf16x3")
    for c1, c2 in _new_pairs(name):
        assert c2.key == c1.key.replace("convs1_", "convs2_") and c2.dilation == 1 and c2.k == c1.k
        w1, b1, w2, b2 = (p[k][n].astype(np.float64) for k in (c1.key, c2.key) for n in ("w", "b"))
        for L in KAT_LENGTHS:
            rng = np.random.default_rng([c1.cin, c1.k, c1.dilation, L])
            x = rng.standard_normal((2, c1.cin, L)).astype(np.float32) * 2.0
            xn = _nwc(x).astype(np.float64)
            xt = orc.conv1d(orc.leaky_relu(xn, 0.1), w1, b1, c1.dilation, orc.get_padding(c1.k, c1.dilation))
            ref = orc.conv1d(orc.leaky_relu(xt, 0.1), w2, b2, 1, orc.get_padding(c2.k, 1)) + xn
            xd = torch.from_numpy(x).to(dev)
            y = x3.run_pair(c1.key, xd, out=torch.full_like(xd, float("nan")))
            torch.cuda.synchronize()
            rel = float(np.abs(_nwc(y.cpu().numpy()) - ref).max() / np.abs(ref).max())
            assert rel < 3e-5, (c1.key, L, rel)
            if c1.cin <= 128 and L % 4 == 0:
                y = f32.run_pair(c1.key, xd, out=torch.full_like(xd, float("nan")))
                two = f32.run_module(c2.key, f32.run_module(c1.key, xd, 0.1), 0.1, xd)
                torch.cuda.synchronize()
                err = float(np.abs(_nwc(y.cpu().numpy()) - ref).max())
                assert err < TIGHT, (c1.key, L, err)
                assert torch.equal(two, y), (c1.key, L, float((two - y).abs().max()))


def _bf(x):
    """round-to-nearest-even to bf16, as float64 (tests/test_gpu_bf16.py: bf)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


@pytest.mark.parametrize("name", [e.name for e in gc.TABLE if "bf16" in e.accepts and NEW_LAYERS[e.name]])
def test_new_layer_kats_bf16(handles, dev, name):
    """The bf16 engine's kernels on the new signatures it accepts — conv_pre from 8, 64 and 128 mels (the tile pads to 128 input channels; only 80
    has run so far) and the ResBlock convolutions at rates 2 and 4 — against the oracle on the SAME bf16-rounded operands, so that only the fp32
    summation order and the output's bf16 rounding differ: 2^-8 of the output's magnitude (tests/test_gpu_bf16.py::test_resblock_conv_kat_bf16,
    test_conv_pre_and_post_bf16), 2^-7 for a fused pair (test_fused_pair_kat_bf16)."""
    p = gc.params(name)
    gen = handles(name, "bf16")
    specs = conv_specs(gc.BY_NAME[name].cfg)
    by = {s.key: i for i, s in enumerate(specs)}
    for s in NEW_LAYERS[name]:
        w, b = p[s.key]["w"], p[s.key]["b"].astype(np.float64)
        for L in KAT_LENGTHS + (700,):
            if _role(s) == "pre":
                x = synthetic_mel(2, L, 50 + L, s.cin)
                ref = orc.conv1d(_bf(x), _bf(w), b, 1, 3)
                for fuse in (2, 0):
                    with options(gen, fuse=fuse):
                        y = gen.run_module(s.key, torch.from_numpy(x).to(dev), 1.0, out=torch.full((2, L, s.cout), float("nan"), device=dev)).cpu().numpy()
                    assert np.abs(y - ref).max() <= 2.0 ** -8 * np.abs(ref).max(), (s.key, L, fuse)
                continue
            assert _role(s) == "conv" and s.cin == s.cout
            rng = np.random.default_rng([s.cin, s.k, s.dilation, L])
            x = rng.standard_normal((2, L, s.cin)).astype(np.float32) * 2.0
            res = rng.standard_normal((2, L, s.cin)).astype(np.float32)
            xin = _bf(orc.leaky_relu(_bf(x), 0.1))
            xt = orc.conv1d(xin, _bf(w), b, s.dilation, orc.get_padding(s.k, s.dilation))
            y = gen.run_module(s.key, torch.from_numpy(x).to(dev), 0.1, torch.from_numpy(res).to(dev),
                               out=torch.full((2, L, s.cout), float("nan"), device=dev)).cpu().numpy()
            ref = xt + _bf(res)
            assert np.abs(y - ref).max() <= 2.0 ** -8 * np.abs(ref).max(), (s.key, L)
            if "convs1_" in s.key:
                c2 = specs[by[s.key] + 1]
                ref = orc.conv1d(_bf(orc.leaky_relu(xt, 0.1)), _bf(p[c2.key]["w"]), p[c2.key]["b"].astype(np.float64), 1, orc.get_padding(c2.k, 1)) + _bf(x)
                for tiles in (1, 2):
                    with options(gen, tiles=tiles):
                        y = gen.run_pair(s.key, torch.from_numpy(x).to(dev), out=torch.full((2, L, s.cin), float("nan"), device=dev)).cpu().numpy()
                    assert np.abs(y - ref).max() <= 2.0 ** -7 * np.abs(ref).max(), (s.key, L, tiles)


# --------------------------------------------------------------------------------------------------------------------------------
# d. the result does not depend on the route or the schedule
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", gc.TABLE, ids=lambda e: e.name)
def test_fp32_routes_agree(handles, dev, entry):
    """fp32 engine: fused pairs at C <= 64 (fuse = 1), + C = 128 at k = 3 (2, the default), wherever the kernel exists (3) and one launch per
    convolution (0) give the same BITS (the engine's contract, tests/test_gpu_parity.py::test_fp32_fused_pairs_are_bit_identical, so far shown on V1);
    the generic kernels (kernels = 1) agree with the engine's own choice within TIGHT."""
    gen = handles(entry.name, "f32")
    for T in entry.frames:
        mel = _dmel(entry.name, T, dev)
        outs = {}
        for fuse in (0, 2, 3, 1):
            with options(gen, fuse=fuse):
                outs[fuse] = _run(gen, mel).clone()
        for fuse in (2, 3, 1):
            assert torch.equal(outs[fuse], outs[0]), (entry.name, T, fuse, float((outs[fuse] - outs[0]).abs().max()))
        with options(gen, kernels=1):
            generic = _run(gen, mel).clone()
        assert bool(torch.isfinite(generic).all())
        assert float((generic - outs[2]).abs().max()) < TIGHT, (entry.name, T)
        assert float(np.abs(generic.cpu().numpy() - gc.oracle(entry.name, T)[0]).max()) < TIGHT, (entry.name, T)


SCHEDULE_ENTRIES = ("V1_NK1", "V1_NK2", "V1_NK4", "DEEP8")


@pytest.mark.parametrize("case", [c for c in gc.cases() if c[0].name in SCHEDULE_ENTRIES], ids=gc.case_id)
def test_schedules_are_bit_identical(handles, dev, case):
    """MRFs of 1, 2 and 4 ResBlocks (and DEEP8's two, over eight stages): the ResBlocks of a stage one after the other (chains = 0), side by side
    where the engine offers it (1: fp32 at 2 and 3 ResBlocks, bf16 at 3; 2: on every single-micro-batch launch), on one or two streams, the batch in
    one micro-batch or one utterance at a time — the same bits."""
    entry, engine = case
    gen = handles(entry.name, engine)
    mel = _dmel(entry.name, entry.frames[-1], dev, 3)
    with options(gen, chains=0, streams=1, microbatch=0):
        base = _run(gen, mel).clone()
    assert bool(torch.isfinite(base).all())
    for chains in (0, 1, 2):
        for streams in (1, 2):
            for mb in (0, 1):
                with options(gen, chains=chains, streams=streams, microbatch=mb):
                    got = _run(gen, mel)
                    again = _run(gen, mel)  # the side streams and events are reused
                    assert torch.equal(got, base) and torch.equal(again, base), (entry.name, engine, chains, streams, mb, float((got - base).abs().max()))


@pytest.mark.parametrize("engine", ["f32", "bf16x3"])
@pytest.mark.parametrize("name", ["V1_NK2", "HALF"])
def test_graph_replay_is_bit_identical(dev, name, engine):
    """Small launches with parallel chains — two of them on V1_NK2, three with generic and MFMA kernels mixed on HALF — replay a captured hipGraph once
    the same buffers came back GRAPH_AFTER = 8 times (engine.hip: forward_maybe_graphed; three calls do not capture yet, so the loop is longer than
    that): the same bits as the eager run, before, at and after the capture.  A handle of its own: the count of cached graphs is asserted."""
    from viettts_amd.hifigan.generator import Generator

    entry = gc.BY_NAME[name]
    gen = Generator(entry.cfg, device=dev, dtype=engine)
    try:
        gen.load_params(gc.params(name))
        mel = _dmel(name, entry.frames[-1], dev)
        out = torch.empty((gc.BATCH, entry.cfg.hop * entry.frames[-1]), dtype=torch.float32, device=dev)
        with options(gen, graph=0):
            ref = gen(mel, out).clone()
        assert gen.get_option("graph") == 1 and gen.get_option("graphs_cached") == 0
        cached = []
        for i in range(11):
            out.fill_(float("nan"))
            gen(mel, out)
            torch.cuda.synchronize()
            assert torch.equal(out, ref), (name, engine, i)
            cached.append(gen.get_option("graphs_cached"))
        assert cached[2] == 0 and cached[-3:] == [1, 1, 1], cached  # the last three calls at least were replays
    finally:
        gen.close()


# --------------------------------------------------------------------------------------------------------------------------------
# e. batch semantics
# --------------------------------------------------------------------------------------------------------------------------------
def _same_kernels(cfg, engine, n, T):
    """Whether an utterance of n frames alone and in a slot of T frames takes the same kernels.  The fp32 kernels with float4 staging need
    L % 4 == 0 and the engine asks again per call (engine.hip: run_layer, pair_f32_fusable), with L the slot's length; the bf16 engine has no
    such switch.  (Conservative for the split-operand engine, whose own kernels take every L.)"""
    if engine == "bf16":
        return True
    muls = [1]
    for r in cfg.upsample_rates:
        muls.append(muls[-1] * int(r))
    return all(((n * m) % 4 == 0) == ((T * m) % 4 == 0) for m in muls)


@pytest.mark.parametrize("case", gc.cases(), ids=gc.case_id)
def test_batch_rows_and_ragged_rows(handles, dev, case):
    """Row b of a batch is the utterance alone, bit for bit.  A ragged batch (frames T, 1, T - 2; DEEP8: an odd and an even count) with a large
    constant behind every utterance's end: each row is bit for bit the same utterance as a one-row ragged call in the same slot, zero behind its
    end, and equal to the plain call on the utterance alone — bit for bit where both take the same kernels; where the slot's length and the
    utterance's own choose different fp32 kernels (another summation order: generator.py, forward_ragged) within TIGHT / 2: each of the two is an
    fp32 evaluation, and an fp32 evaluation of these inputs is within TIGHT / 4 of the exact result in any order
    (tests/test_gen_configs_cpu.py::test_fp32_round_off_stays_inside_the_bar)."""
    entry, engine = case
    gen = handles(entry.name, engine)
    T, hop = entry.frames[-1], entry.cfg.hop
    mel = _dmel(entry.name, T, dev, 3)
    base = _run(gen, mel).clone()
    assert bool(torch.isfinite(base).all())
    alone = [_run(gen, mel[b : b + 1].contiguous()).clone() for b in range(3)]
    for b in range(3):
        assert torch.equal(alone[b][0], base[b]), (entry.name, engine, b)
    frames = [13, 6, 1] if entry.name == "DEEP8" else [T, 1, max(1, T - 2)]
    junk = mel.clone()
    for b, n in enumerate(frames):
        junk[b, n:] = 77.0
    got = gen.forward_ragged(junk, frames, out=torch.full((3, hop * T), float("nan"), dtype=torch.float32, device=dev)).clone()
    assert bool(torch.isfinite(got).all())
    for b, n in enumerate(frames):
        row = gen.forward_ragged(junk[b : b + 1].contiguous(), [n])[0]
        assert torch.equal(row, got[b]), (entry.name, engine, b, n)
        assert not bool(got[b, hop * n :].any()), (b, n)
        one = _run(gen, mel[b : b + 1, :n].contiguous())[0]
        if _same_kernels(entry.cfg, engine, n, T):
            assert torch.equal(one, got[b, : hop * n]), (entry.name, engine, b, n, float((one - got[b, : hop * n]).abs().max()))
        else:
            assert float((one - got[b, : hop * n]).abs().max()) < TIGHT / 2, (entry.name, engine, b, n)
