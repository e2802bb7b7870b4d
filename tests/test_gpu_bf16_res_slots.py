"""The 16-block pair kernel's peeled last blocks (kernels_bf16_rbg.hip, GTile's RS_ / g_res_slots): c2's last block requests residual rows of
epilogue 2 in its look-ahead slots past the pass's end, c1's requests nothing there.  The arithmetic is the parent's; what can go wrong is which
row lands in which accumulator, the rows left over behind the loop, the clamped rows of the first and the last tile, and the accumulate modes,
whose rows reuse the registers the residual rows have just left.

``Generator.run_resblock(..., route=1)`` (three pair launches) on every 16-block class, wide and narrow tiles, B = 2, at the lengths
L = 1, NT2 - 1, NT2, NT2 + 1, 2 NT2 + 3 of the launched tile (NT2 = N1 - (k - 1): the first tile with its clamped rows, the last partial tile, a
seam), the same lengths as a ragged batch rows = [L, max(1, L - NT2 + 3)], in all four epilogue modes, y pre-filled with the sentinel.  Both bars
of tests/_bf16_rb_ref.py against the fp64 reference that rounds where the kernels round; the sentinel untouched past rows[b].

C = 256 and the stage-ending launches that carry ups_2 / ups_3 (GUp) run in a whole V1 forward — the smallest configuration that reaches
them — of 1 and 3 utterances of 5 and 37 frames, against the oracle at the bf16 bounds of tests/test_gpu_bf16.py.
"""
import numpy as np
import pytest
import torch

import _bf16_rb_ref as RB
import _launch_regimes as R
from oracle import hifigan_oracle as orc
from viettts_amd.hifigan.config import V1
from viettts_amd.hifigan.synth import synthetic_mel, synthetic_params

pytestmark = pytest.mark.gpu

SENTINEL = 1536.0  # bf16-exact, far outside every output's range
MODES = [(0, 1.0, 1.0), (1, 1.0, 1.0), (1, 3.0, 0.1), (1, 3.0, 0.01)]  # (acc_add, div, slope_out), as tests/test_gpu_bf16_resblock.py
CLASSES16 = [(256, 3), (256, 11), (128, 3), (128, 7), (128, 11), (64, 7), (64, 11)]  # g_mfma_blk(C, k) == 16: the classes on conv_phase16
BF16_MAXABS, BF16_SNR_DB = 0.03, 38.0  # tests/test_gpu_bf16.py
FRAMES3 = [37, 5, 37]


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


def test_the_classes_are_the_16_block_classes():
    """CLASSES16 is what the library runs on conv_phase16 (vtts_hifigan's pair_g_mfma_blk is not exported: the packed layout is), so read the
    table out of the source the library was built from"""
    import re
    from pathlib import Path

    src = (Path(__file__).resolve().parents[1] / "viettts_amd" / "csrc" / "kernels_bf16_rbg.hip").read_text()
    body = src[src.index("constexpr int g_mfma_blk(int C, int KS) {"):]
    body = body[: body.index("}")]
    rows = dict((int(c), [int(x) for x in v]) for c, *v in re.findall(r"C == (\d+)\s*\? \(KS == 3 \? (\d+) : KS == 7 \? (\d+) : (\d+)\)", body))
    got = [(C, k) for C in (256, 128, 64) for k, blk in zip((3, 7, 11), rows[C]) if blk == 16]
    assert got == CLASSES16, got


def _lengths(C, k, tiles):
    nt2 = R.bf16_pair_nt2(C, k, tiles == 2)
    return nt2, [1, nt2 - 1, nt2, nt2 + 1, 2 * nt2 + 3]


def _refs_all_modes(params, C, k, x, acc0):
    """{mode: (ref64, pairs64, ref32)} of x [B', L', C]: the three pairs once per precision, the epilogue per mode (resblock_ref's last lines)"""
    W, b = RB.resblock_wb(params, C, k)
    base = {dt: RB.resblock_ref(x, W, b, k, RB.DILS, dt) for dt in (np.float64, np.float32)}
    out = {}
    for mode in MODES:
        acc_add, div, slope = mode
        fin = {}
        for dt, (_, pairs) in base.items():
            v = pairs[2]
            if acc_add:
                v = v + RB.bf(acc0).astype(dt)
            fin[dt] = orc.leaky_relu(v / dt(div), slope)
        out[mode] = (fin[np.float64], base[np.float64][1], fin[np.float32])
    return out


def _hold(got, refs, what):
    ref64, pairs, ref32 = refs
    e1, b1, e2, b2 = RB.bars(got, ref64, pairs, ref32)
    assert np.isfinite(got).all(), what
    assert e1 <= b1, (what, "bar (i)", e1, b1)
    assert e2 <= b2, (what, "bar (ii)", e2, b2)


def _run(gen, dev, C, k, x, rows, mode, y0):
    acc_add, div, slope = mode
    y = torch.from_numpy(y0).to(dev)
    out = gen.run_resblock(RB.resblock_key(C, k), torch.from_numpy(x).to(dev), route=1, rows=rows, slope_out=slope, acc_add=bool(acc_add), div=div, out=y)
    return out.cpu().numpy()


@pytest.mark.parametrize("tiles", [1, 2], ids=["wide-tiles", "narrow-tiles"])
@pytest.mark.parametrize("ck", CLASSES16, ids=lambda ck: f"C{ck[0]}k{ck[1]}")
def test_pair_route_at_the_tile_edges_in_every_epilogue_mode(gen, dev, params, ck, tiles):
    C, k = ck
    nt2, lengths = _lengths(C, k, tiles)
    gen.set_option("tiles", tiles)
    try:
        for L in lengths:
            rng = np.random.default_rng(C * 10000 + k * 100 + tiles * 7 + L % 97)
            x = (rng.standard_normal((2, L, C)) * 2.0).astype(np.float32)
            acc0 = rng.standard_normal((2, L, C)).astype(np.float32)
            n1 = max(1, L - nt2 + 3)
            whole = _refs_all_modes(params, C, k, x, acc0)
            alone = _refs_all_modes(params, C, k, x[1:2, :n1], acc0[1:2, :n1])  # row 1 of the ragged batch: that utterance alone
            for mode in MODES:
                y0 = acc0 if mode[0] else np.full(x.shape, SENTINEL, np.float32)
                got = _run(gen, dev, C, k, x, None, mode, y0)
                _hold(got, whole[mode], (ck, tiles, L, mode, "plain"))
                got = _run(gen, dev, C, k, x, [L, n1], mode, y0)
                r64, prs, r32 = whole[mode]
                _hold(got[0:1], (r64[0:1], [p[0:1] for p in prs], r32[0:1]), (ck, tiles, L, mode, "rows[0]"))
                _hold(got[1:2, :n1], alone[mode], (ck, tiles, L, mode, "rows[1]", n1))
                assert np.array_equal(got[1, n1:], RB.bf(y0[1, n1:])), (ck, tiles, L, mode, n1)  # untouched past rows[1]: the sentinel / the accumulator (as bf16)
    finally:
        gen.set_option("tiles", 0)


# ---- C = 256 and the carriers of ups_2 / ups_3 in a whole forward ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fwd_oracle():
    """(params, [(mel, waveform, pre-tanh)] of the three utterances of FRAMES3, each alone, in fp64)"""
    p = synthetic_params(V1, 4321, "scaled")
    out = []
    for i, T in enumerate(FRAMES3):
        mel = synthetic_mel(1, T, 300 + 10 * i + T)
        y, pre = orc.generator_forward(p, mel, V1, np.float64, return_pre_tanh=True)
        out.append((mel, y[0, :, 0], pre[0, :, 0]))
    return p, out


@pytest.fixture(scope="module")
def gen_fwd(dev, fwd_oracle):
    from viettts_amd.hifigan.generator import Generator

    g = Generator(V1, device=dev, dtype="bf16")
    g.load_params(fwd_oracle[0])
    yield g
    g.close()


@pytest.mark.parametrize("tiles", [1, 2], ids=["wide-tiles", "narrow-tiles"])
def test_forward_through_c256_and_the_upsampler_carriers(gen_fwd, dev, fwd_oracle, tiles):
    """one utterance (5 and 37 frames, waveform and pre-tanh) and three as a ragged batch (each row against the utterance alone)"""
    utts = fwd_oracle[1]
    gen_fwd.set_option("tiles", tiles)
    try:
        for mel, want_y, want_pre in utts[:2]:
            wav, pre = gen_fwd.forward_tap(torch.from_numpy(mel).to(dev), "pre_tanh")
            wav, pre = wav.cpu().numpy()[0].astype(np.float64), pre.cpu().numpy()[0].astype(np.float64)
            e_y = float(np.abs(wav - want_y).max())
            snr = float(10 * np.log10((want_pre ** 2).mean() / ((pre - want_pre) ** 2).mean()))
            assert np.isfinite(wav).all() and e_y < BF16_MAXABS and snr > BF16_SNR_DB, (tiles, mel.shape[1], e_y, snr)
            plain = gen_fwd(torch.from_numpy(mel).to(dev)).cpu().numpy()[0].astype(np.float64)  # no tap: the tail and the upsamplers ride
            assert float(np.abs(plain - want_y).max()) < BF16_MAXABS, (tiles, mel.shape[1])
        Tmax = max(FRAMES3)
        batch = np.full((len(FRAMES3), Tmax, V1.num_mels), 77.0, np.float32)  # whatever sits past an utterance's end must not matter
        for b, (mel, _, _) in enumerate(utts):
            batch[b, : mel.shape[1]] = mel[0]
        got = gen_fwd.forward_ragged(torch.from_numpy(batch).to(dev), FRAMES3).cpu().numpy()
        for b, (mel, want_y, _) in enumerate(utts):
            n = V1.hop * mel.shape[1]
            e_y = float(np.abs(got[b, :n].astype(np.float64) - want_y).max())
            assert e_y < BF16_MAXABS, ("ragged row", tiles, b, e_y)
            assert not got[b, n:].any(), (tiles, b)
    finally:
        gen_fwd.set_option("tiles", 0)
