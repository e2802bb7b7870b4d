"""The bf16 pair kernel's C = 64 classes on either MFMA block shape (kernels_bf16_rbg.hip: g_mfma_blk): the C = 64 peer of test_gpu_bf16_mfma16.py.

C = 64 has two k = 32 steps per tap, so a 16-block loop's unit of four steps spans two taps and the k = 7 / 11 passes end in a peeled half
unit; its tiles are the blocked 16-row LDS image.  Whatever the per-class table says: (1) a pair launch gives the same bits on the wide and
the narrow tile at every length around a wide-tile edge, and is within the fused-pair KAT's bound of the fp64 oracle on the same bf16-rounded
operands; (2) the whole forward gives the same bits on either tile, for a batch row and for the utterance alone, plain and ragged.
(The weight order itself is checked on the host, stand-alone and under the sanitizers: tools/check_pair_pack16_host.cpp.)"""
import numpy as np
import pytest
import torch

from _launch_regimes import bf16_pair_nt2
from oracle import hifigan_oracle as orc
from viettts_amd.hifigan.config import V1
from viettts_amd.hifigan.synth import synthetic_mel, synthetic_params
from viettts_amd.hifigan.weights import conv_specs

pytestmark = pytest.mark.gpu


def bf(x):
    """round-to-nearest-even to bf16, returned as float64"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def v1_params():
    return synthetic_params(V1, 4321, "scaled")


@pytest.fixture(scope="module")
def gen(dev, v1_params):
    from viettts_amd.hifigan.generator import Generator

    g = Generator(V1, device=dev, dtype="bf16")
    g.load_params(v1_params)
    yield g
    g.close()


def _pair_cases():
    by = {s.key: s for s in conv_specs(V1)}
    seen, out = set(), []
    for s in conv_specs(V1):
        if s.kind == "conv" and s.cin == s.cout and s.cin == 64 and "convs1_" in s.key and (s.k, s.dilation) not in seen:
            seen.add((s.k, s.dilation))
            out.append((s, by[s.key.replace("convs1_", "convs2_")]))
    return out


def test_every_c64_class_and_dilation_is_a_case():
    assert sorted((p[0].k, p[0].dilation) for p in _pair_cases()) == [(k, d) for k in (3, 7, 11) for d in (1, 3, 5)]


@pytest.mark.parametrize("pair", _pair_cases(), ids=lambda p: f"C{p[0].cin}k{p[0].k}d{p[0].dilation}")
def test_pair_kat_at_the_tile_edges_on_both_tiles(gen, v1_params, dev, pair):
    """x' = c2(lrelu(c1(lrelu(x)))) + x at L = 1, 37, one wide tile, one more, two and five, B = 2: wide tile == narrow tile bit for bit, and each
    within 2^-7 max|ref| of the oracle with xt rounded to bf16 where the kernel rounds it (test_fused_pair_kat_bf16's reference and bound)."""
    c1, c2 = pair
    nt2 = bf16_pair_nt2(c1.cin, c1.k, False)
    assert nt2 == 512 - (c1.k - 1)
    w1, b1 = v1_params[c1.key]["w"], v1_params[c1.key]["b"]
    w2, b2 = v1_params[c2.key]["w"], v1_params[c2.key]["b"]
    try:
        for L in (1, 37, nt2, nt2 + 1, 2 * nt2, 5 * nt2):
            rng = np.random.default_rng(c1.cin * 100 + c1.k * 10 + c1.dilation + 7919 * L)
            x = rng.standard_normal((2, L, c1.cin)).astype(np.float32) * 2.0
            xin = bf(orc.leaky_relu(bf(x), 0.1))
            xt = orc.conv1d(xin, bf(w1), b1.astype(np.float64), c1.dilation, orc.get_padding(c1.k, c1.dilation))
            xt = bf(orc.leaky_relu(xt, 0.1))
            ref = orc.conv1d(xt, bf(w2), b2.astype(np.float64), 1, orc.get_padding(c2.k, 1)) + bf(x)
            got = {}
            for tiles in (1, 2):
                gen.set_option("tiles", tiles)
                got[tiles] = gen.run_pair(c1.key, torch.from_numpy(x).to(dev)).clone()
                err = np.abs(got[tiles].cpu().numpy() - ref).max()
                print(f"[pair C{c1.cin} k{c1.k} d{c1.dilation} L{L} tiles{tiles}] err {err:.3e} bound {2.0 ** -7 * np.abs(ref).max():.3e}")
                assert err <= 2.0 ** -7 * np.abs(ref).max(), (L, tiles, err, np.abs(ref).max())
            assert torch.equal(got[1], got[2]), (L, (got[1] != got[2]).sum().item())
    finally:
        gen.set_option("tiles", 0)


@pytest.mark.parametrize("T", [1, 3, 37])
def test_forward_same_bits_on_either_tile_batched_alone_and_ragged(gen, dev, T):
    mel = torch.from_numpy(synthetic_mel(2, T, 5 + T)).to(dev)
    lens = [T, max(1, T - 2)]
    hop = gen.hop
    try:
        outs = {}
        for tiles in (1, 2):
            gen.set_option("tiles", tiles)
            outs[tiles] = gen(mel).clone()
            for b in range(2):
                assert torch.equal(gen(mel[b : b + 1].contiguous())[0], outs[tiles][b]), (tiles, b)
            rag = gen.forward_ragged(mel, lens).clone()
            for b, n in enumerate(lens):
                alone = gen(mel[b : b + 1, :n].contiguous())[0]
                assert torch.equal(rag[b, : n * hop], alone[: n * hop]), (tiles, b, n)
        assert torch.equal(outs[1], outs[2])
        assert torch.isfinite(outs[1]).all()
    finally:
        gen.set_option("tiles", 0)
