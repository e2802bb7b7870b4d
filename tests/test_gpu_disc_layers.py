"""The discriminator kernels (viettts_amd/csrc/disc.hip) layer by layer, each on its own input, at every tile edge; and the loss reduction on
buffers of the test's own making.

tests/test_gpu_disc.py compares whole passes: a deep layer's input there already carries every earlier layer's error.  Here layer i is compared
with torch's CPU operators run on the SAME fp32 input the kernel read (the GPU's own feature map i - 1, or the waveform) and the same fp32
weights, over every element of a real and a generated row:

    max|gpu_i - fp64_i| / max|fp64_i|  <=  4 e32_i + 2^-22,    e32_i = max|fp32_i - fp64_i| / max|fp64_i|

(tests/_disc_layer_ref.py; the formula of test_gpu_disc.py and test_gpu_mel.py, the yardstick computed at test time from torch's fp32 run, never
from the kernel).  conv_post accumulates in double and rounds once: 2^-22 alone, and its score-buffer copy is its feature map bit for bit.
The buffers start as NaN, so an element nobody wrote fails the case.  The lengths come from tests/_disc_tiles.py: for each of the 54 layers and
each tile width of its class, the row lengths on either side of the tile edge (154 targets, 41 lengths from 256 to 32 766 samples); at a length
only the layers it is there for are computed on the CPU.  All 54 layers run at the short lengths, which pin the reflection, the pools' ends and
the one-position rows.

The loss reduction: |got - want| <= 2^-23 |want| for each of the 87 results.  The kernel's element arithmetic is fp32 and the yardstick's is
the same (numpy float32); both sum in double; one rounding to fp32 remains (2^-24), doubled for the reassociation of the double sums.  The
64-float alignment gaps between the maps keep their NaN fill: a read outside a map makes a result NaN.

Figures of the first GPU run (MI355X, all 59 cases pass, 8 s in all).  Worst err / bound per tile class over the 432 layer checks:
first layers 0.29 (MSD scale 1, T = 2311), Cout/group 128: 0.23, >= 512: 0.30, 64: 0.17, 32: 0.36 (T = 11), 16: 0.19, conv_post 0.23 of 2^-22;
err 2.9e-8 - 4.8e-7 against e32 2.7e-8 - 8.4e-7.  At the tile edges themselves nothing stands out from the short lengths (0.10 - 0.27 on the
Cout/group >= 128 classes either side of 64 and 128).  Loss reduction: worst |got - want| / |want| 4.6e-8 - 5.9e-8 per case against 1.19e-7.
"""
import re
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest
import torch

import _disc_layer_ref as ref
import _disc_oracle as oracle
import _disc_tiles as tiles

pytestmark = pytest.mark.gpu

COVER = tiles.cover()
LAYERS = tiles.layers()
# all 54 layers: 11 is the minimum; at 12 period 11 reflects 10 of its 11 columns; 13; 37; 38 is even with an even first pool (12 is even with
# an odd one), for the pools' last element; 2311 = 2 * 3 * 5 * 7 * 11 + 1 leaves remainder 1 for every period and is odd for the pools
SMALL = (11, 12, 13, 37, 38, 2311)
WORST = {}  # tile class -> (err / bound, T, layer): printed as the cases run


@pytest.fixture(scope="module")
def setup():
    from viettts_amd.hifigan.disc_synth import synthetic_disc_checkpoint
    from viettts_amd.hifigan.discriminators import Discriminators, fold_checkpoint

    params = fold_checkpoint(synthetic_disc_checkpoint(8642))
    d = Discriminators("cuda:0").load_params(params)
    yield d, params
    d.close()


@lru_cache(maxsize=None)
def rows(T):
    """one real and one generated row"""
    return oracle.make_inputs(1, T, 200000 + T)


def run_nan_filled(d, y2):
    N, T = y2.shape
    nf, ns = d.buffer_sizes(N, T)
    fb = torch.full((nf,), float("nan"), dtype=torch.float32, device=d.device)
    sb = torch.full((ns,), float("nan"), dtype=torch.float32, device=d.device)
    d.forward_raw(torch.from_numpy(y2).to(d.device), fb, sb)
    torch.cuda.synchronize()
    return fb, sb


def check_layers(d, params, T, which):
    y2 = rows(T)
    fb, sb = run_nan_filled(d, y2)
    scores, fmaps = d.views(fb, sb, 2, T)
    flat = [m for maps in fmaps for m in maps]
    shapes = oracle.fmap_shapes(T)
    bad = []
    for i in which:
        ly = LAYERS[i]
        C, L, p = shapes[i]
        x = y2 if ly["kind"].endswith("first") else flat[i - 1].cpu().numpy()  # the input the kernel read
        got = flat[i].cpu().numpy()
        assert got.shape == ((2, C, L, p) if ly["disc"] < 5 else (2, C, L)), (i, got.shape)
        r64, r32 = ref.layer_reference(params, i, x, torch.float64), ref.layer_reference(params, i, x, torch.float32)
        post = ly["kind"] == "post"
        ok, err, e32, bound = ref.compare_layer(got, r64, r32, post)
        nt = tiles.launched_nt(ly, L * p)
        print(f"T={T} layer {i} ({ly['cls']}, p={p}, Nout={L * p}, NT={nt}): err {err:.3e} e32 {e32:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
        if not ok:
            bad.append((i, ly["cls"], L * p, err, e32, bound))
        elif err / bound > WORST.get(ly["cls"], (0.0,))[0]:
            WORST[ly["cls"]] = (err / bound, T, i)
        if post:
            s = scores[ly["disc"]]
            assert s.shape == (2, L * p) and torch.equal(s.view(torch.int32), flat[i].reshape(2, L * p).view(torch.int32)), i
    print("worst ratio per tile class so far:", {k: (round(v[0], 3),) + v[1:] for k, v in sorted(WORST.items())})
    assert not bad, bad


@pytest.mark.parametrize("T", list(COVER))
def test_each_layer_at_its_tile_edges(setup, T):
    d, params = setup
    shapes = oracle.fmap_shapes(T)
    for i, nt, side, nout in COVER[T]:
        assert shapes[i][1] * shapes[i][2] == nout and ((nout <= nt) if side == "le" else (nout > nt))  # the length still lands on its edge
    check_layers(d, params, T, sorted({i for i, _, _, _ in COVER[T]}))


@pytest.mark.parametrize("T", SMALL)
def test_all_layers_at_the_short_lengths(setup, T):
    d, params = setup
    check_layers(d, params, T, range(54))


def _placement_lengths():
    """the first edge length with a mid-row second tile of an MPD layer (period >= 3), and the first with an MSD GEMM layer past its edge"""
    def first(pred):
        return next(T for T, items in COVER.items() if any(pred(LAYERS[i], nt, nout) for i, nt, _, nout in items))

    return (first(lambda ly, nt, nout: ly["kind"] == "gemm" and ly["p"] >= 3 and nout > nt == tiles.launched_nt(ly, nout)),
            first(lambda ly, nt, nout: ly["kind"] == "gemm" and ly["disc"] >= 5 and nout > nt))


@pytest.mark.parametrize("T", _placement_lengths())
def test_the_second_row_is_the_row_alone_at_a_tile_edge(setup, T):
    d, _ = setup
    y2 = rows(T)
    fb, sb = run_nan_filled(d, y2)
    s_all, f_all = d.views(fb, sb, 2, T)
    fb1, sb1 = run_nan_filled(d, y2[1:2])
    s_one, f_one = d.views(fb1, sb1, 1, T)
    for k, (a, b) in enumerate(zip([m for maps in f_all for m in maps] + s_all, [m for maps in f_one for m in maps] + s_one)):
        assert torch.isfinite(b).all() and torch.equal(a[1:2].view(torch.int32), b.view(torch.int32)), k


# ---- the loss reduction -----------------------------------------------------------------------------------------------------------------
def loss_buffers(d, B, T, seed, identical=False):
    """Both buffers of a 2 B-row call, NaN everywhere except the 54 maps and the 8 scores, which hold seeded normal data (written through views);
    the generated half differs from the real one unless `identical`."""
    nf, ns = d.buffer_sizes(2 * B, T)
    fb = torch.full((nf,), float("nan"), dtype=torch.float32)
    sb = torch.full((ns,), float("nan"), dtype=torch.float32)
    scores, fmaps = d.views(fb, sb, 2 * B, T)
    flat = [m for maps in fmaps for m in maps]
    rng = np.random.default_rng(seed)
    for v in flat + scores:
        a = rng.standard_normal(tuple(v.shape)).astype(np.float32)
        if identical:
            a[B:] = a[:B]
        else:
            a[B:] = (a[B:] * np.float32(0.7) + np.float32(0.1)).astype(np.float32)
        v.copy_(torch.from_numpy(a))
    assert int(torch.isfinite(fb).sum()) == sum(v.numel() for v in flat) and int(torch.isfinite(sb).sum()) == ns
    return fb, sb, [v.numpy() for v in flat], [v.numpy() for v in scores]


def check_losses(d, B, T, seed, identical=False):
    fb, sb, flat, scores = loss_buffers(d, B, T, seed, identical)
    want = ref.loss_yardstick(flat, scores, B)
    raw = d.losses_raw(fb.to(d.device), sb.to(d.device), B, T)
    torch.cuda.synchronize()
    got = raw[:87].cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), np.nonzero(~np.isfinite(got))[0].tolist()  # a NaN: a read outside a map
    err = np.abs(got - want)
    rel = err / np.where(want == 0, 1.0, np.abs(want))
    print(f"B={B} T={T}: worst |got - want| / |want| = {rel.max():.3e} at entry {int(rel.argmax())} (bound {2.0 ** -23:.3e})")
    bad = np.nonzero(~(err <= 2.0 ** -23 * np.abs(want)))[0]
    assert bad.size == 0, [(int(i), float(got[i]), float(want[i])) for i in bad]
    return got, want, flat, scores


@pytest.mark.parametrize("T", [11, 37, 4099])
@pytest.mark.parametrize("B", [1, 2, 3])
def test_loss_reduction(setup, B, T):
    d, _ = setup
    _, _, flat, scores = check_losses(d, B, T, 7000 + 10 * T + B)
    if B == 1 and T == 11:
        # fewer elements than first-stage slices: one-position scores, and maps of fewer than VTTS_DISC_LOSS_PARTIALS elements per half
        header = (Path(__file__).resolve().parents[1] / "include" / "vtts_disc.h").read_text()
        partials = int(re.search(r"#define VTTS_DISC_LOSS_PARTIALS (\d+)", header).group(1))
        assert min(s[:B].size for s in scores) == 1 and min(f[:B].size for f in flat) < partials


def test_loss_reduction_of_identical_halves(setup):
    d, _ = setup
    got, want, _, _ = check_losses(d, 2, 37, 99, identical=True)
    assert (got[:54] == 0.0).all() and (want[:54] == 0.0).all() and got[78] == got[79] == got[84] == 0.0
    assert (got[54:62] == got[70:78]).all()  # (1 - d_r)^2 and (1 - d_g)^2 of the same scores
