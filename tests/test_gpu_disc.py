"""The discriminators' GPU scoring pass (viettts_amd/csrc/disc.hip) against tests/_disc_oracle.py in fp64, computed at test time.

Bounds, per feature map and score, over every element:  max|gpu - fp64| / max|fp64|  <=  4 * err_ref32 + 2^-22  and  <= 1e-4.
err_ref32 is the error of the REFERENCE'S OWN modules run in fp32 on the CPU against their fp64 run (tests/golden/disc_golden.npz,
minted by tools/make_disc_golden.py); the factor 4 and the 2^-22 are the margin tests/test_gpu_mel.py gives a different but equally
valid fp32 summation order; 1e-4 is the project's parity bar.  Losses: relative error <= 4 * err_ref32 of that loss + 2^-22.
Outputs are pre-filled with NaN, so anything the kernels leave unwritten shows.

Figures so far.  A CPU restatement of the kernels' summation order (fp32, partial sums flushed every 5 / 8 taps, conv_post in double) puts
every feature map and score at <= 0.26 of its bound at T = 37 and T = 11, and every loss inside its bound except one: the L1 of feature map 50
at T = 37 (MSD scale 2, 512 -> 1024, one position per row), 1.1e-6 against 6.5e-7.  That entry's err_ref32 is 1.0e-7, a lucky draw of the
reference's fp32 run for a mean over 2048 correlated differences, and the figure moves between 0.8e-6 and 1.3e-6 with the flush interval
without trend: it is the rounding of the stored fp32 feature maps, not the order of the sums.  An early GPU run was of the build
BEFORE the partial sums, T = 37 only: all 62 feature maps and scores inside their bounds (worst 0.85 of it), losses 5 and 48 outside
(2.14e-5 against 1.99e-5, 4.7e-7 against 2.7e-7).  The first complete GPU run, of the final build with the partial sums (MI355X): all 10
tests pass.  Worst feature map or score per length, as a fraction of its bound: 0.22 (T = 37, map 47), 0.29 (2310, map 16), 0.27 (4099, map 28),
0.25 (11, map 40), 0.24 (16411, map 3).  The predicted loss entry, the L1 of map 50 at T = 37, sits just inside: 6.19e-7 against 6.53e-7; every
other loss is at <= 0.62 of its bound.  tests/test_gpu_disc_layers.py holds each layer on its own input.  The bounds stay as the issue sets them.
"""
from pathlib import Path

import numpy as np
import pytest
import torch

import _disc_oracle as oracle

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "disc_golden.npz"
SHAPES = {11: (2, 111), 37: (2, 137), 2310: (2, 12310), 4099: (2, 14099), 16411: (1, 116411)}  # T: (B, input seed), the fixture's
EPS = 2.0 ** -22
_CACHE = {}


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def setup():
    from viettts_amd.hifigan.disc_synth import synthetic_disc_checkpoint
    from viettts_amd.hifigan.discriminators import Discriminators, fold_checkpoint

    params = fold_checkpoint(synthetic_disc_checkpoint(8642))
    d = Discriminators("cuda:0").load_params(params)
    yield d, params
    d.close()


def expected(params, T):
    """fp64 oracle of a fixture shape, computed once and shared."""
    if T not in _CACHE:
        B, seed = SHAPES[T]
        y2 = oracle.make_inputs(B, T, seed)
        scores, fmaps = oracle.forward(params, y2, torch.float64)
        _CACHE[T] = (y2, [s.numpy() for s in scores], [f.numpy() for f in fmaps], oracle.losses(scores, fmaps, B))
    return _CACHE[T]


def run_nan_filled(d, y2):
    N, T = y2.shape
    nf, ns = d.buffer_sizes(N, T)
    fb = torch.full((nf,), float("nan"), dtype=torch.float32, device=d.device)
    sb = torch.full((ns,), float("nan"), dtype=torch.float32, device=d.device)
    d.forward_raw(torch.from_numpy(y2).to(d.device), fb, sb)
    torch.cuda.synchronize()
    return fb, sb


def loss_vector(L):
    return np.concatenate([L["fmap_l1"], L["real"], L["fake"], L["gens"], np.array([L[k] for k in oracle.LOSS_NAMES])]).astype(np.float64)


@pytest.mark.parametrize("T", [37, 2310, 4099, 11, 16411])
def test_feature_maps_scores_and_losses(setup, golden, T):
    d, params = setup
    B, _ = SHAPES[T]
    y2, s_ref, f_ref, l_ref = expected(params, T)
    assert abs(float(y2.astype(np.float64).sum()) - float(golden[f"ysum_{T}"])) == 0.0  # the inputs the fixture's yardstick was measured on
    fb, sb = run_nan_filled(d, y2)
    scores, fmaps = d.views(fb, sb, 2 * B, T)
    flat = [m for maps in fmaps for m in maps]
    assert [len(m) for m in fmaps] == [6] * 5 + [8] * 3 and len(scores) == 8
    bad = []
    for kind, got_list, ref_list, e32 in (("fmap", flat, f_ref, golden[f"err_ref32_fmap_{T}"]), ("score", scores, s_ref, golden[f"err_ref32_score_{T}"])):
        for i, (got, ref) in enumerate(zip(got_list, ref_list)):
            got = got.cpu().numpy().astype(np.float64)
            assert got.shape == ref.shape, (kind, i, got.shape, ref.shape)
            assert np.isfinite(got).all(), f"{kind} {i}: unwritten or non-finite elements"
            err = float(np.abs(got - ref).max() / np.abs(ref).max())
            bound = min(4.0 * float(e32[i]) + EPS, 1e-4)
            print(f"T={T} {kind} {i}: err {err:.3e} bound {bound:.3e} (err_ref32 {float(e32[i]):.3e})")
            if not err <= bound:
                bad.append((kind, i, err, bound))
    assert not bad, bad
    # losses: one reduction pass over the buffers just checked
    raw = d.losses_raw(fb, sb, B, T)
    L = d.unpack_losses(raw)
    assert len(L.r_losses_mpd) == len(L.g_losses_mpd) == len(L.gen_losses_mpd) == 5
    assert len(L.r_losses_msd) == len(L.g_losses_msd) == len(L.gen_losses_msd) == 3
    got = np.array(L.fmap_l1 + L.r_losses_mpd + L.r_losses_msd + L.g_losses_mpd + L.g_losses_msd + L.gen_losses_mpd + L.gen_losses_msd
                   + [L.feature_mpd, L.feature_msd, L.disc_mpd, L.disc_msd, L.gen_mpd, L.gen_msd, L.feature, L.disc, L.gen], dtype=np.float64)
    ref = loss_vector(l_ref)
    e32 = golden[f"err_ref32_loss_{T}"]
    rel = np.abs(got / ref - 1.0)
    for i in np.argsort(-rel / (4.0 * e32 + EPS))[:5]:
        print(f"T={T} loss {i}: rel err {rel[i]:.3e} bound {4.0 * e32[i] + EPS:.3e}")
    assert np.isfinite(got).all()
    assert (rel <= 4.0 * e32 + EPS).all(), [(int(i), float(rel[i]), float(4.0 * e32[i] + EPS)) for i in np.nonzero(~(rel <= 4.0 * e32 + EPS))[0]]


@pytest.mark.parametrize("T", [37, 4099])
def test_rows_are_bit_identical_alone_and_in_any_batch(setup, T):
    d, params = setup
    B, _ = SHAPES[T]
    y2 = expected(params, T)[0]
    fb, sb = run_nan_filled(d, y2)
    s_all, f_all = d.views(fb, sb, 2 * B, T)
    # a row alone
    row = 2 * B - 1
    fb1, sb1 = run_nan_filled(d, y2[row : row + 1])
    s_one, f_one = d.views(fb1, sb1, 1, T)
    for a, b in zip([m for maps in f_all for m in maps] + s_all, [m for maps in f_one for m in maps] + s_one):
        assert torch.equal(a[row : row + 1], b)
    # one 2 B-row call == two B-row calls
    halves = [run_nan_filled(d, y2[:B]), run_nan_filled(d, y2[B:])]
    for h, (fbh, sbh) in enumerate(halves):
        s_h, f_h = d.views(fbh, sbh, B, T)
        for a, b in zip([m for maps in f_all for m in maps] + s_all, [m for maps in f_h for m in maps] + s_h):
            assert torch.equal(a[h * B : (h + 1) * B], b)
    # the reduction gives the same bits on every run
    r1 = d.losses_raw(fb, sb, B, T)[:128].clone()
    r2 = d.losses_raw(fb, sb, B, T)[:128].clone()
    assert torch.equal(r1.view(torch.int32), r2.view(torch.int32)) and torch.isfinite(r1).all()


@pytest.mark.parametrize("T", [11, 37])
def test_an_adopted_blob_gives_the_same_bits(setup, T):
    """A second owner that binds the first one's packed weights (cloned) instead of loading its own: the raw buffers, bit for bit."""
    from viettts_amd.hifigan.discriminators import Discriminators

    d, _ = setup
    y = oracle.make_inputs(1, T, SHAPES[T][1])[:1]
    fb, sb = run_nan_filled(d, y)
    other = Discriminators("cuda:0")
    try:
        other.adopt_packed(d.packed_blob().clone())
        fb2, sb2 = run_nan_filled(other, y)
        scores, fmaps = other.views(fb2, sb2, 1, T)
        assert all(torch.isfinite(v).all() for v in [m for maps in fmaps for m in maps] + scores)
        # the raw buffers as bits: the alignment gaps between the maps keep the NaN fill in both
        assert torch.equal(fb2.view(torch.int32), fb.view(torch.int32)) and torch.equal(sb2.view(torch.int32), sb.view(torch.int32))
    finally:
        other.close()


def test_reference_import_path(setup):
    """vietTTS.hifigan.torch_model's discriminators return the reference's four lists, and feature_loss of them is the kernel's number."""
    from vietTTS.hifigan import torch_model as tm

    d, params = setup
    T = 2310
    B, _ = SHAPES[T]
    y2, s_ref, f_ref, _ = expected(params, T)
    tm.use_discriminators(d)
    try:
        y = torch.from_numpy(y2[:B]).to(d.device)[:, None, :]
        y_hat = torch.from_numpy(y2[B:]).to(d.device)[:, None, :]
        want = d.losses(y, y_hat)
        for cls, lo, n_disc, n_maps, feat, disc, gen in ((tm.MultiPeriodDiscriminator, 0, 5, 6, want.feature_mpd, want.disc_mpd, want.gen_mpd),
                                                         (tm.MultiScaleDiscriminator, 30, 3, 8, want.feature_msd, want.disc_msd, want.gen_msd)):
            y_d_rs, y_d_gs, fmap_rs, fmap_gs = cls()(y, y_hat)
            assert len(y_d_rs) == len(y_d_gs) == len(fmap_rs) == len(fmap_gs) == n_disc
            for k in range(n_disc):
                assert len(fmap_rs[k]) == len(fmap_gs[k]) == n_maps
                for j in range(n_maps):
                    ref = f_ref[lo + n_maps * k + j]
                    assert tuple(fmap_rs[k][j].shape) == (B,) + ref.shape[1:] == tuple(fmap_gs[k][j].shape)
                assert tuple(y_d_rs[k].shape) == (B, int(np.prod(f_ref[lo + n_maps * k + n_maps - 1].shape[1:])))
            assert float(tm.feature_loss(fmap_rs, fmap_gs)) == feat
            loss, r_losses, g_losses = tm.discriminator_loss(y_d_rs, y_d_gs)
            assert float(loss) == disc and len(r_losses) == len(g_losses) == n_disc
            loss, gen_losses = tm.generator_loss(y_d_gs)
            assert float(loss) == gen and len(gen_losses) == n_disc
    finally:
        tm.use_discriminators(None)
