"""Option "upfuse" of the bf16 engine: the last pair launch of stage 1 (C = 128, k = 11) and of stage 2 (C = 64, k = 11) also runs the NEXT stage's
transposed convolution (ups_2: 128 -> 2 x 64, ups_3: 64 -> 2 x 32; kernels_bf16_rbg.hip: GUp) on the rows its epilogue has just formed, so the stage
output is neither written nor read back and the upsampler is not launched.  The rows the fused GEMM reads are the bf16 values the un-fused path
stores, and every output element sees convt_g_bf16_k's chain (bias block, two taps ascending, k-steps ascending, v_mfma_f32_32x32x16_bf16), so the
samples are BIT-IDENTICAL with the option off.  Every comparison here is torch.equal between the two settings on one generator: no tolerance.

Lengths: a fused tile yields NT2 - 2 frames (the transposed convolution's neighbours q - 1 and q + 1 come out of the tile's own rows), i.e. 244 / 116
at C = 128 (wide / narrow tile) and 500 / 244 at C = 64.  Stage 1 has 64 T rows and stage 2 128 T: 64 * 61 and 128 * 61 are whole multiples of 244,
128 * 125 of 500, 64 * 29 of 116, so with rows of T, T - 1 and T - 2 frames each width gets an utterance that ends on a tile edge and
utterances that end one and two frames short of it.  T = 4 is 256 rows at C = 128 and 512 at C = 64: with the wide tiles 12 rows of each fall into a second
tile (24 into a third with the narrow ones); T = 5 ends well inside a tile.  T = 1 is one frame."""
import numpy as np
import pytest
import torch

from viettts_amd.hifigan.config import V1
from viettts_amd.hifigan.synth import synthetic_mel, synthetic_params

pytestmark = pytest.mark.gpu

ALL_BITS = 3  # bit 0: ups_2 rides on stage 1's last pair launch, bit 1: ups_3 on stage 2's
DEFAULT = 3   # the committed default (profiles/upfuse_findings.md)


@pytest.fixture(scope="module")
def gen():
    from viettts_amd.hifigan.generator import Generator

    g = Generator(V1, device="cuda:0", dtype="bf16")
    g.load_params(synthetic_params(V1, 4321, "scaled"))
    yield g
    g.close()


@pytest.fixture(autouse=True)
def _restore(gen):
    yield
    for name, v in (("upfuse", DEFAULT), ("tiles", 0), ("microbatch", 0), ("streams", 0)):
        gen.set_option(name, v)


def _both(gen, fn):
    """fn() with every boundary fused and with none"""
    gen.set_option("upfuse", ALL_BITS)
    on = fn()
    gen.set_option("upfuse", 0)
    off = fn()
    return on, off


@pytest.mark.parametrize("tiles", [0, 1, 2])
@pytest.mark.parametrize("T", [1, 4, 5, 29, 61, 125], ids=lambda t: f"T{t}")
def test_plain_and_ragged_forwards_are_bit_identical(gen, T, tiles):
    gen.set_option("tiles", tiles)
    B = 3
    mel = torch.from_numpy(synthetic_mel(B, T, 500 + T)).to("cuda:0")
    frames = [max(1, T - b) for b in range(B)]
    on, off = _both(gen, lambda: (gen(mel).clone(), gen.forward_ragged(mel, frames).clone()))
    assert torch.equal(on[0], off[0]), (T, tiles)
    assert torch.equal(on[1], off[1]), (T, tiles)
    for b, n in enumerate(frames):
        assert not bool(on[1][b, 256 * n :].any()), (T, tiles, b)
    # one boundary at a time
    for bit in (1, 2):
        gen.set_option("upfuse", bit)
        assert torch.equal(gen.forward_ragged(mel, frames), off[1]), (T, tiles, bit)


def test_xcd_ordered_padded_grid(gen):
    """202 / 197 tiles per utterance slot at C = 128 / C = 64 with the wide tile: above XCD_MAP_MIN_TILES = 192, so the grid is padded to whole rounds
    of the 8 XCDs and an XCD walks a contiguous eighth of each utterance's valid tiles."""
    gen.set_option("tiles", 1)
    mel = torch.from_numpy(synthetic_mel(2, 768, 77)).to("cuda:0")
    frames = [768, 745]
    on, off = _both(gen, lambda: gen.forward_ragged(mel, frames).clone())
    assert torch.equal(on, off)
    assert not bool(on[1, 256 * 745 :].any())


def test_micro_batches_and_streams(gen):
    rng = np.random.default_rng(5)
    frames = [int(v) for v in rng.integers(3, 97, size=37)]
    g = torch.Generator().manual_seed(7)
    mel = torch.clamp(-5 + 2 * torch.randn(len(frames), max(frames), 80, generator=g), -11.5129, 2.0).to("cuda:0")
    for mb, streams in ((0, 1), (8, 1), (16, 2)):
        gen.set_option("microbatch", mb)
        gen.set_option("streams", streams)
        on, off = _both(gen, lambda: gen.forward_ragged(mel, frames).clone())
        assert torch.equal(on, off), (mb, streams)
        for b, n in enumerate(frames):
            assert not bool(on[b, 256 * n :].any()), (mb, streams, b)


def test_taps_fall_back_and_match(gen):
    """pre_tanh needs no stage output; mrf_1 / mrf_2 ARE the stage outputs a fused boundary never writes, so they force the un-fused path there"""
    mel = torch.from_numpy(synthetic_mel(2, 61, 9)).to("cuda:0")
    gen.set_option("upfuse", 0)
    plain = gen(mel).clone()
    ref = {name: [t.clone() for t in gen.forward_tap(mel, name)] for name in ("pre_tanh", "mrf_1", "mrf_2", "ups_2", "ups_3", "mrf_3")}
    gen.set_option("upfuse", ALL_BITS)
    assert torch.equal(gen(mel), plain)
    for name, (wav, t) in ref.items():
        got_wav, got_t = gen.forward_tap(mel, name)
        assert torch.equal(got_wav, plain) and torch.equal(wav, plain), name
        assert torch.equal(got_t, t), name


def test_the_option(gen):
    from viettts_amd import _lib

    assert gen.get_option("upfuse") == DEFAULT
    for v in (0, 1, 2, 3, 0, 3):
        gen.set_option("upfuse", v)
        assert gen.get_option("upfuse") == v
    for bad in (-1, 4):
        with pytest.raises(_lib.VttsError):
            gen.set_option("upfuse", bad)
