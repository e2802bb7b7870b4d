"""GPU parity tests proper: the HIP path (through the C ABI) against the oracle and the committed
golden vectors minted from the reference's own generator.  Tolerance: BASELINE.json's north_star
asks <= 1e-4 max-abs in fp32; the fp32 kernels sit at fp32 round-off (~1e-6), so the asserts are
an order tighter than the bar and say so."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import hifigan_oracle as orc
from viettts_amd.hifigan.config import TINY, TINY2, V1
from viettts_amd.hifigan.synth import params_digest, synthetic_mel, synthetic_params
from viettts_amd.hifigan.weights import conv_specs

pytestmark = pytest.mark.gpu

TOL = 1e-4  # north_star bar
TIGHT = 2e-5  # what fp32 kernels are expected to meet


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def v1_params():
    return synthetic_params(V1, 4321, "scaled")


@pytest.fixture(scope="module")
def gen_v1(dev, v1_params):
    from viettts_amd.hifigan.generator import Generator

    g = Generator(V1, device=dev)
    g.load_params(v1_params)
    yield g
    g.close()


def _nwc(x_ncw):  # [B,C,L] -> [B,L,C]
    return np.ascontiguousarray(np.transpose(x_ncw, (0, 2, 1)))


def _ncw(x_nwc):
    return np.ascontiguousarray(np.transpose(x_nwc, (0, 2, 1)))


# --------------------------------------------------------------------------------------------------
# per-layer known-answer tests: every distinct (C, k, d) ResBlock conv, both kernel families
# --------------------------------------------------------------------------------------------------
def _res_conv_cases():
    seen, out = set(), []
    for s in conv_specs(V1):
        if s.kind == "conv" and s.cin == s.cout:
            sig = (s.cin, s.k, s.dilation)
            if sig not in seen:
                seen.add(sig)
                out.append(s)
    return out


@pytest.mark.parametrize("kernels", [(0, 1), (0, 2), (1, 0)], ids=["mfma-wide", "mfma-narrow", "generic"])
@pytest.mark.parametrize("spec", _res_conv_cases(), ids=lambda s: f"C{s.cin}k{s.k}d{s.dilation}")
def test_resblock_conv_kat(gen_v1, v1_params, dev, spec, kernels):
    kernels, tiles = kernels
    rng = np.random.default_rng(spec.cin * 1000 + spec.k * 10 + spec.dilation)
    B, L = 2, 300 if spec.cin >= 128 else 1000  # ragged: not a multiple of any time tile
    x = rng.standard_normal((B, spec.cin, L)).astype(np.float32) * 2.0
    res = rng.standard_normal((B, spec.cin, L)).astype(np.float32)
    w, b = v1_params[spec.key]["w"], v1_params[spec.key]["b"]
    xt = orc.leaky_relu(_nwc(x).astype(np.float64), 0.1)
    ref = orc.conv1d(xt, w.astype(np.float64), b.astype(np.float64), spec.dilation, orc.get_padding(spec.k, spec.dilation)) + _nwc(res)
    gen_v1.set_option("kernels", kernels)
    gen_v1.set_option("tiles", tiles)
    try:
        y = gen_v1.run_module(spec.key, torch.from_numpy(x).to(dev), 0.1, torch.from_numpy(res).to(dev))
        torch.cuda.synchronize()
    finally:
        gen_v1.set_option("kernels", 0)
        gen_v1.set_option("tiles", 0)
    err = np.abs(_nwc(y.cpu().numpy()) - ref).max()
    assert err < TIGHT, f"{spec.key} ({'generic' if kernels else 'mfma'}): max|err| = {err}"


def _pair_cases_f32():
    seen, out = set(), []
    specs = conv_specs(V1)
    for i, s in enumerate(specs):
        if s.kind == "conv" and s.cin == s.cout and s.cin <= 128 and "convs1_" in s.key:
            sig = (s.cin, s.k, s.dilation)
            if sig not in seen:
                seen.add(sig)
                out.append((s, specs[i + 1]))
    return out


@pytest.mark.parametrize("pair", _pair_cases_f32(), ids=lambda p: f"C{p[0].cin}k{p[0].k}d{p[0].dilation}")
def test_fp32_fused_pair_kat(gen_v1, v1_params, dev, pair):
    """The fused fp32 pair kernel (kernels_f32_pair.hip) on every (C, k, rate) it covers against the oracle's
    ``c2(lrelu(c1(lrelu(x)))) + x`` (vietTTS/hifigan/model.py:45-50) in fp64, lengths that are no multiple of any tile (ragged first /
    last tiles, several tiles per utterance), AND bit for bit against the two separate convolution launches."""
    c1, c2 = pair
    assert c2.key == c1.key.replace("convs1_", "convs2_") and c2.dilation == 1
    rng = np.random.default_rng(c1.cin * 1000 + c1.k * 10 + c1.dilation)
    B, L = 2, 300 if c1.cin >= 128 else 1000
    x = rng.standard_normal((B, c1.cin, L)).astype(np.float32) * 2.0
    xn = _nwc(x).astype(np.float64)
    w1, b1 = v1_params[c1.key]["w"].astype(np.float64), v1_params[c1.key]["b"].astype(np.float64)
    w2, b2 = v1_params[c2.key]["w"].astype(np.float64), v1_params[c2.key]["b"].astype(np.float64)
    xt = orc.conv1d(orc.leaky_relu(xn, 0.1), w1, b1, c1.dilation, orc.get_padding(c1.k, c1.dilation))
    ref = orc.conv1d(orc.leaky_relu(xt, 0.1), w2, b2, 1, orc.get_padding(c2.k, 1)) + xn
    xd = torch.from_numpy(x).to(dev)
    y = gen_v1.run_pair(c1.key, xd)
    torch.cuda.synchronize()
    err = np.abs(_nwc(y.cpu().numpy()) - ref).max()
    assert err < TIGHT, f"{c1.key}: max|err| = {err}"
    # the same fmaf chains in the same order as the two launches: the same bits
    t = gen_v1.run_module(c1.key, xd, 0.1)
    two = gen_v1.run_module(c2.key, t, 0.1, xd)
    torch.cuda.synchronize()
    assert torch.equal(two, y), float((two - y).abs().max())
    with pytest.raises(Exception):
        gen_v1.run_pair(c2.key, xd)  # not the first convolution of a pair


@pytest.mark.parametrize("BT", [(1, 1), (2, 5), (1, 37), (3, 160)], ids=lambda v: f"B{v[0]}T{v[1]}")
def test_fp32_fused_pairs_are_bit_identical(gen_v1, dev, BT):
    """Whole generator, fp32 engine: fused pairs at C <= 64 (the default, option fuse = 2), at C <= 128 (fuse = 3) and one launch per
    convolution (fuse = 0) give the SAME samples, bit for bit — so every golden / oracle test of the fp32 engine covers the fused path."""
    B, T = BT
    mel = torch.from_numpy(synthetic_mel(B, T, 31 + T)).to(dev)
    outs = {}
    try:
        for fuse in (0, 2, 3, 1):
            gen_v1.set_option("fuse", fuse)
            outs[fuse] = gen_v1(mel).clone()
    finally:
        gen_v1.set_option("fuse", 2)
    for fuse in (2, 3, 1):
        assert torch.equal(outs[fuse], outs[0]), (fuse, float((outs[fuse] - outs[0]).abs().max()))


def test_residual_in_place(gen_v1, v1_params, dev):
    """The engine writes c2(xt)+x over x for the 2nd/3rd pair of a ResBlock (res aliases y)."""
    spec = [s for s in conv_specs(V1) if s.cin == 64 and s.k == 7 and s.dilation == 1][0]
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.standard_normal((1, 64, 512)).astype(np.float32)).to(dev)
    res = torch.from_numpy(rng.standard_normal((1, 64, 512)).astype(np.float32)).to(dev)
    want = gen_v1.run_module(spec.key, x, 0.1, res.clone())
    import ctypes as C
    from viettts_amd import _lib

    y = res.clone()
    _lib.check(gen_v1.lib, gen_v1.lib.vtts_hifigan_run_module(gen_v1._h, spec.key.encode(), C.c_void_p(x.data_ptr()), 1, 512, C.c_float(0.1),
                                                                C.c_void_p(y.data_ptr()), C.c_void_p(y.data_ptr()), C.c_void_p(0)))
    torch.cuda.synchronize()
    assert torch.equal(want, y)


@pytest.mark.parametrize("i", [0, 1, 2, 3])
def test_upsample_kat(gen_v1, v1_params, dev, i):
    spec = [s for s in conv_specs(V1) if s.key == f"generator/~/ups_{i}"][0]
    rng = np.random.default_rng(40 + i)
    B, L = 2, 37
    x = rng.standard_normal((B, spec.cin, L)).astype(np.float32) * 2.0
    w, b = v1_params[spec.key]["w"], v1_params[spec.key]["b"]
    ref = orc.conv1d_transpose(orc.leaky_relu(_nwc(x).astype(np.float64), 0.1), w.astype(np.float64), b.astype(np.float64), spec.stride)
    y = gen_v1.run_module(spec.key, torch.from_numpy(x).to(dev), 0.1)
    torch.cuda.synchronize()
    assert y.shape == (B, spec.cout, L * spec.stride)
    assert np.abs(_nwc(y.cpu().numpy()) - ref).max() < TIGHT


def test_conv_pre_and_post_kat(gen_v1, v1_params, dev):
    rng = np.random.default_rng(9)
    mel = synthetic_mel(2, 21, 5)
    w, b = v1_params["generator/~/conv1_d"]["w"], v1_params["generator/~/conv1_d"]["b"]
    ref = orc.conv1d(mel.astype(np.float64), w.astype(np.float64), b.astype(np.float64), 1, 3)
    y = gen_v1.run_module("generator/~/conv1_d", torch.from_numpy(mel).to(dev), 1.0)
    assert np.abs(_nwc(y.cpu().numpy()) - ref).max() < TIGHT
    x = rng.standard_normal((2, 32, 1000)).astype(np.float32)
    w, b = v1_params["generator/~/conv1_d_1"]["w"], v1_params["generator/~/conv1_d_1"]["b"]
    ref = np.tanh(orc.conv1d(orc.leaky_relu(_nwc(x).astype(np.float64), 0.01), w.astype(np.float64), b.astype(np.float64), 1, 3))
    y = gen_v1.run_module("generator/~/conv1_d_1", torch.from_numpy(x).to(dev), 0.01)
    assert np.abs(_nwc(y.cpu().numpy()) - ref).max() < TIGHT


# --------------------------------------------------------------------------------------------------
# whole generator vs the golden vectors minted from the reference (tests/golden)
# --------------------------------------------------------------------------------------------------
def _meta(golden_dir):
    with open(golden_dir / "golden_meta.json") as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("kernels", [0, 1], ids=["mfma", "generic"])
@pytest.mark.parametrize("case", ["v1_scaled_T8", "v1_scaled_T37", "v1_init_T16"])
def test_generator_matches_reference_golden(golden_dir, dev, case, kernels):
    from viettts_amd.hifigan.generator import Generator

    rec = _meta(golden_dir)[case]
    g = np.load(golden_dir / f"{case}.npz")
    params = synthetic_params(V1, rec["wseed"], rec["kind"])
    assert params_digest(params) == rec["params_sha256"]
    gen = Generator(V1, device=dev)
    gen.load_params(params)
    gen.set_option("kernels", kernels)
    mel = torch.from_numpy(synthetic_mel(rec["B"], rec["T"], rec["mseed"])).to(dev)
    wav, pre = gen.forward_tap(mel, "pre_tanh")
    torch.cuda.synchronize()
    wav, pre = wav.cpu().numpy(), pre.cpu().numpy()
    gen.close()
    assert wav.shape == g["y64"].shape
    e_y, e_p = np.abs(wav - g["y64"]).max(), np.abs(pre - g["pre64"]).max()
    e_ref32 = np.abs(wav - g["y32"]).max()
    assert e_y < TIGHT and e_p < TIGHT and e_ref32 < TIGHT, (e_y, e_p, e_ref32)
    assert e_y < TOL
    # north_star's own sentence — "outputs match the HAIKU generator on identical mel inputs within 1e-4 max-abs fp32" — against the
    # reference's Haiku mel2wave executed (oracle/make_golden.py::reference_haiku_mel2wave): squeezed as mel2wave.py:39 returns it
    e_hk = np.abs(np.squeeze(wav) - g["y64_haiku"]).max()
    assert e_hk < TIGHT and e_hk < 1e-4, e_hk


def test_tiny_architecture_rng_independent(golden_dir, dev):
    """TINY config (channels 16/8/4/2: no MFMA instantiation -> generic HIP kernels) with weights and
    mel read from the fixture itself."""
    from viettts_amd.hifigan.generator import Generator

    g = np.load(golden_dir / "tiny_scaled_T12.npz")
    params = {}
    for name in g.files:
        if name.startswith("W::"):
            _, key, which = name.split("::")
            params.setdefault(key, {})[which] = g[name]
    gen = Generator(TINY, device=dev)
    gen.load_params(params)
    wav, pre = gen.forward_tap(torch.from_numpy(g["mel"]).to(dev), "pre_tanh")
    torch.cuda.synchronize()
    gen.close()
    assert np.abs(wav.cpu().numpy() - g["y64"]).max() < TIGHT
    assert np.abs(pre.cpu().numpy() - g["pre64"]).max() < TIGHT


def test_resblock2_generator_vs_reference_golden(golden_dir, dev):
    """ResBlock2 generators (vietTTS/hifigan/model.py:54-74, selected by config "resblock": "2", model.py:86): the fp32 engine
    against the reference's own torch generator (torch_model.py:117-148) on fixture weights — kernel sizes 3 / 5 / 7, rates
    (1, 2) / (2, 6) / (3, 12), two residual convolutions per block, MRF mean over the three blocks.  Parameter names are the
    ones the Haiku MODEL creates (res_block1_N/~/conv1_d, conv1_d_1)."""
    from viettts_amd import _lib
    from viettts_amd.hifigan.generator import Generator

    g = np.load(golden_dir / "tiny2_scaled_T12.npz")
    params = {}
    for name in g.files:
        if name.startswith("W::"):
            _, key, which = name.split("::")
            params.setdefault(key, {})[which] = g[name]
    assert "generator/~/res_block1_0/~/conv1_d_1" in params and len(params) == 1 + 4 + 12 * 2 + 1
    gen = Generator(TINY2, device=dev)
    gen.load_params(params)
    wav, pre = gen.forward_tap(torch.from_numpy(g["mel"]).to(dev), "pre_tanh")
    torch.cuda.synchronize()
    assert np.abs(wav.cpu().numpy() - g["y64"]).max() < 2e-5
    assert np.abs(pre.cpu().numpy() - g["pre64"]).max() < 2e-5
    want = orc.generator_forward(params, g["mel"], TINY2, np.float64)[..., 0]
    assert np.abs(wav.cpu().numpy() - want).max() < 2e-5
    gen.close()
    with pytest.raises(_lib.VttsError):  # the bf16 kernels cover the V1 channel / kernel-size / rate shapes only (ResBlock2 of those
        Generator(TINY2, device=dev, dtype="bf16")  # shapes: tests/test_gpu_bf16.py::test_resblock2_generator_bf16_vs_oracle)


def test_parallel_resblocks_schedule_is_bit_identical(dev):
    """fp32 engine, small launches: the three ResBlocks of a stage run side by side on parallel streams into separate buffers and
    are combined afterwards (engine.hip: plan_pass / mrf_mean_k).  Same additions in the same order as the accumulating
    epilogues of the one-after-the-other schedule: the samples must be the same BITS, for ResBlock1 and ResBlock2 generators."""
    from viettts_amd.hifigan.generator import Generator

    for cfg, shapes in ((V1, ((1, 37), (2, 160), (1, 512))), (TINY2, ((2, 12), (1, 300)))):
        gen = Generator(cfg, device=dev)
        gen.load_params(synthetic_params(cfg, 4321, "scaled"))
        for B, T in shapes:
            mel = torch.from_numpy(synthetic_mel(B, T, 9, cfg.num_mels)).to(dev)
            gen.set_option("chains", 1)
            a = gen(mel).clone()
            a2 = gen(mel).clone()  # twice: the side streams / events are reused
            gen.set_option("chains", 0)
            b = gen(mel).clone()
            torch.cuda.synchronize()
            assert torch.equal(a, b) and torch.equal(a, a2), (cfg.resblock, B, T, float((a - b).abs().max()))
        gen.close()


def test_baseline_config2_shape(golden_dir, gen_v1, dev):
    """BASELINE config 2: B=1, T=512 fp32, parity <= 1e-4 vs the reference generator."""
    rec = _meta(golden_dir)["v1_scaled_T512"]
    g = np.load(golden_dir / "v1_scaled_T512.npz")
    mel = torch.from_numpy(synthetic_mel(1, 512, rec["mseed"])).to(dev)
    wav, pre = gen_v1.forward_tap(mel, "pre_tanh")
    torch.cuda.synchronize()
    wav, pre = wav.cpu().numpy(), pre.cpu().numpy()
    idx = g["idx"]
    e_y, e_p = np.abs(wav[:, idx] - g["y64"]).max(), np.abs(pre[:, idx] - g["pre64"]).max()
    assert e_y < TIGHT and e_p < TIGHT, (e_y, e_p)
    # ... and vs the reference's HAIKU mel2wave executed at this shape (BASELINE configs[1]: "parity vs Haiku ref <= 1e-4")
    e_hk = np.abs(wav[0, idx] - g["y64_haiku"]).max()
    print(f"[fp32 B=1 T=512 vs the reference's Haiku mel2wave executed] max|dy| {e_hk:.3e}")
    assert e_hk < TIGHT and e_hk < 1e-4
    s = g["sum_y64"]
    w64 = wav.astype(np.float64)
    assert abs(np.abs(w64).sum() - s[1]) / s[1] < 1e-5
    assert abs((w64 ** 2).sum() - s[2]) / s[2] < 1e-5
    assert np.all(np.abs(wav) < 1.0)


@pytest.mark.parametrize("tap", ["conv_pre", "ups_0", "mrf_0", "ups_2", "mrf_3"])
def test_intermediate_taps_vs_oracle(gen_v1, v1_params, dev, tap):
    mel = synthetic_mel(2, 9, 11)
    taps = []
    orc.generator_forward(v1_params, mel, V1, np.float64, taps=taps)
    want = dict(taps)[tap]  # NWC
    _, got = gen_v1.forward_tap(torch.from_numpy(mel).to(dev), tap)
    torch.cuda.synchronize()
    got = got.cpu().numpy().reshape(2, want.shape[2], want.shape[1])
    assert np.abs(_nwc(got) - want).max() < TIGHT


# --------------------------------------------------------------------------------------------------
# size-independent properties at full BASELINE sizes
# --------------------------------------------------------------------------------------------------
def test_batch_rows_are_independent_and_microbatch_invariant(gen_v1, dev):
    """Utterances never mix: row b of a batched call is bit-identical to the single-utterance call,
    whatever the micro-batch the engine walks the batch in."""
    T = 64
    mel = torch.from_numpy(synthetic_mel(5, T, 21)).to(dev)
    base = gen_v1(mel).clone()
    for mb in (1, 2, 5):
        gen_v1.set_option("microbatch", mb)
        assert torch.equal(gen_v1(mel), base), f"microbatch {mb}"
    gen_v1.set_option("microbatch", 0)
    for b in (0, 3):
        assert torch.equal(gen_v1(mel[b : b + 1]), base[b : b + 1])


def test_receptive_field_halo(gen_v1, dev):
    """an output sample depends on mel frames within +-12.71 frames, so a chunk cut
    with a 13-frame halo reproduces the un-chunked interior (fp32 reassociation only)."""
    T, t0, t1, halo = 160, 60, 100, 13
    mel = torch.from_numpy(synthetic_mel(1, T, 8)).to(dev)
    full = gen_v1(mel)
    chunk = gen_v1(mel[:, t0 - halo : t1 + halo].contiguous())
    a = full[:, 256 * t0 : 256 * t1]
    b = chunk[:, 256 * halo : 256 * (halo + t1 - t0)]
    assert (a - b).abs().max().item() < 5e-6  # different tile/stage shapes -> fp32 reassociation only
    # and a 12-frame halo is NOT enough (the field really is that wide)
    chunk12 = gen_v1(mel[:, t0 - 12 : t1 + 12].contiguous())
    b12 = chunk12[:, 256 * 12 : 256 * (12 + t1 - t0)]
    assert (a - b12).abs().max().item() > 0


def test_full_size_batch_config3_properties(gen_v1, dev):
    """BASELINE config 3 shape (T=1024 frames per utterance) at a batch the test can afford: equal
    utterances give equal rows; output is finite, in (-1,1); row 0 equals the golden-checked path."""
    mel1 = torch.from_numpy(synthetic_mel(1, 1024, 1234)).to(dev)
    mel = mel1.repeat(3, 1, 1).contiguous()
    wav = gen_v1(mel)
    torch.cuda.synchronize()
    assert wav.shape == (3, 262144)
    assert torch.isfinite(wav).all() and wav.abs().max().item() < 1.0
    assert torch.equal(wav[0], wav[1]) and torch.equal(wav[0], wav[2])
    assert torch.equal(gen_v1(mel1)[0], wav[0])


def test_fp32_headline_shape_B64_T1024_default_schedule(golden_dir, gen_v1, dev, capsys):
    """The fp32 engine at the shape bench.py's ``fp32_path`` leg times (64 x 1024 frames) under the engine's DEFAULT schedule there
    (two half-size passes of 32 utterances side by side on two streams, engine.hip: auto_streams / pass_frames) against rows 0, 37, 63 of the
    reference generator's own output on this batch (tests/golden/v1_scaled_B64_T1024.npz, minted by oracle/make_golden.py from
    vietTTS/hifigan/torch_model.py through the reference's converter): the <= 1e-4 of BASELINE.json at the size the throughput is
    quoted on, not only at B = 1 x T = 512.  A row is also bit-identical to the same utterance run alone (the two-stream schedule
    changes no arithmetic)."""
    rec = _meta(golden_dir)["v1_scaled_B64_T1024"]
    g = np.load(golden_dir / "v1_scaled_B64_T1024.npz")
    rows, idx = rec["rows"], g["idx"]
    assert gen_v1.get_option("microbatch") == 0 and gen_v1.get_option("streams") == 0  # the defaults are what is under test
    mel = torch.from_numpy(synthetic_mel(64, 1024, rec["mseed"])).to(dev)
    wav, pre = gen_v1.forward_tap(mel, "pre_tanh")
    torch.cuda.synchronize()
    y = wav[rows].cpu().numpy()[:, idx].astype(np.float64)
    p = pre[rows].cpu().numpy()[:, idx].astype(np.float64)
    e_y, e_p = float(np.abs(y - g["y64"]).max()), float(np.abs(p - g["pre64"]).max())
    e_y32 = float(np.abs(y - g["y32"]).max())
    with capsys.disabled():
        print(f"\n[fp32 B=64 T=1024 rows {rows}, default two-stream schedule] max|dy| vs fp64 reference {e_y:.3e}  (vs its fp32 run {e_y32:.3e})  max|dpre| {e_p:.3e}")
    assert e_y < TIGHT and e_p < TIGHT and e_y < TOL, (e_y, e_p)
    plain = gen_v1(mel)
    assert torch.equal(plain, wav)
    assert bool(torch.isfinite(plain).all()) and float(plain.abs().max()) < 1.0
    for b in (0, 37, 63):  # one utterance from each half-size pass and the last one
        assert torch.equal(gen_v1(mel[b : b + 1].contiguous())[0], plain[b]), b
    s = g["sum_y64"]  # sums over ALL samples of the golden rows, not only the strided ones
    w64 = plain[rows].double()
    assert abs(float(w64.abs().sum()) - s[1]) / s[1] < 1e-5 and abs(float((w64 ** 2).sum()) - s[2]) / s[2] < 1e-5
    del wav, pre, plain, mel, w64


def test_edge_lengths(gen_v1, v1_params, dev):
    """T as small as 1..4 frames: every stage is dominated by zero padding (get_padding edges)."""
    for T in (1, 2, 3, 4):
        mel = synthetic_mel(1, T, 100 + T)
        want = orc.generator_forward(v1_params, mel, V1, np.float64)[..., 0]
        got = gen_v1(torch.from_numpy(mel).to(dev)).cpu().numpy()
        assert got.shape == (1, 256 * T)
        assert np.abs(got - want).max() < TIGHT


# --------------------------------------------------------------------------------------------------
# the boundary: mel2wave() drop-in
# --------------------------------------------------------------------------------------------------
def test_mel2wave_dropin(tmp_path, monkeypatch, v1_params, dev):
    from viettts_amd.hifigan import mel2wave as m2w
    from viettts_amd.hifigan.weights import save_haiku_pickle

    (tmp_path / "assets/hifigan").mkdir(parents=True)
    (tmp_path / "assets/infore/hifigan").mkdir(parents=True)
    repo_cfg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "assets/hifigan/config.json")
    (tmp_path / "assets/hifigan/config.json").write_text(open(repo_cfg).read())
    monkeypatch.chdir(tmp_path)
    m2w.reload()
    with pytest.raises(FileNotFoundError):
        m2w.mel2wave(synthetic_mel(1, 4, 1))
    save_haiku_pickle(tmp_path / "assets/infore/hifigan/hk_hifi.pickle", v1_params)
    mel = synthetic_mel(1, 10, 2)
    wav = m2w.mel2wave(mel)
    assert isinstance(wav, np.ndarray) and wav.dtype == np.float32 and wav.shape == (2560,)
    want = orc.mel2wave_oracle(v1_params, mel, V1)
    assert np.abs(wav - want).max() < TIGHT
    wav2 = m2w.mel2wave(torch.from_numpy(synthetic_mel(2, 10, 2)))
    assert wav2.shape == (2, 2560)
    with pytest.raises(ValueError):
        m2w.mel2wave(np.zeros((10, 80), np.float32))
    # an utterance longer than one pass takes goes through the chunk scheduler (limit lowered for the test)
    from viettts_amd.hifigan.generator import Generator

    assert m2w._generator().max_frames_per_pass == 65536  # fp32 engine, V1: 2^31 bytes / (8192 * 4)
    long_mel = synthetic_mel(1, 9000, 3)
    one_shot = m2w.mel2wave(long_mel)
    monkeypatch.setattr(Generator, "max_frames_per_pass", property(lambda self: 8192))
    chunked = m2w.mel2wave(long_mel)
    assert chunked.shape == one_shot.shape == (256 * 9000,)
    assert np.abs(chunked - one_shot).max() < 5e-6
    m2w.reload()


def test_integration_md_stub_executes(tmp_path, monkeypatch, v1_params, dev):
    """The ctypes stub of INTEGRATION.md §3 — what a maintainer would put in place of vietTTS/hifigan/mel2wave.py:20-41 — run as
    written (library path made absolute, the reference's FLAGS import replaced: tests/_integration_stub.py) against a scratch
    assets/ tree; its waveform is the product's `mel2wave` output (same engine, same weights: bit for bit) and meets the fp32 bar
    against the oracle."""
    from _integration_stub import runnable_source
    from viettts_amd import _lib
    from viettts_amd.hifigan import mel2wave as m2w
    from viettts_amd.hifigan.weights import save_haiku_pickle

    (tmp_path / "assets/hifigan").mkdir(parents=True)
    (tmp_path / "assets/infore/hifigan").mkdir(parents=True)
    repo_cfg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "assets/hifigan/config.json")
    (tmp_path / "assets/hifigan/config.json").write_text(open(repo_cfg).read())
    save_haiku_pickle(tmp_path / "assets/infore/hifigan/hk_hifi.pickle", v1_params)
    monkeypatch.chdir(tmp_path)
    _lib.load()  # the process's HIP runtime is already global; the stub's own CDLL calls find the same objects
    ns = {"__name__": "integration_md_stub"}
    exec(compile(runnable_source(str(_lib.default_lib_path()), str(tmp_path / "assets/infore/hifigan")), "INTEGRATION.md", "exec"), ns)
    mel = synthetic_mel(2, 12, 5)
    got = ns["mel2wave"](mel)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (2, 12 * 256)
    m2w.reload()
    want = m2w.mel2wave(mel)
    m2w.reload()
    assert np.array_equal(got, want)
    assert np.abs(got - orc.mel2wave_oracle(v1_params, mel, V1)).max() < TIGHT
    one = ns["mel2wave"](synthetic_mel(1, 7, 6))
    assert one.shape == (7 * 256,)
