"""The teacher-forced acoustic pass (include/vtts_nat.h: vtts_nat_acoustic_forward_teacher, ..._teacher_masks_haiku) on the GPU.

Parity is against tests/golden/nat_gta_golden.npz: what the reference's own ``AcousticModel(is_training=False).__call__`` returns
in fp64 (tools/make_gta_golden.py executes it), over EVERY element of the valid frames of BOTH return values.  The bar is the rule
of tests/test_gpu_mel.py,

    max |gpu - fp64|  <=  4 * err_ref32 + 2^-22 * max |fp64|      and never more than 5e-5 (tests/test_gpu_nat.py's bar),

with ``err_ref32`` = the reference's own fp32 run against its fp64 run, read from the fixture, never from the code under test.
Every figure is printed before it is asserted (run with -s to see them).

A mask draw with an ODD element count does not exist on the device: prenet_dim and decoder_dim are multiples of 32 by
vtts_nat_acoustic_create's rules, so B * F * D is always even and the kernel has no branch for jax's one-count pad (the restatement in
tests/_gta_oracle.py has, and tests/test_gta_cpu.py checks it there).  The smallest draw, (1, 1), stands in its place here.
"""
import numpy as np
import pytest
import torch

import _gta_oracle as G
import _mel_oracle as M
from viettts_amd import _lib

pytestmark = pytest.mark.gpu
PN, H, MEL = 256, 512, 80


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(golden_dir / "nat_gta_golden.npz"))


@pytest.fixture(scope="module")
def acoustic():
    from viettts_amd.nat.acoustic import AcousticModel
    from viettts_amd.nat.synth import synthetic_acoustic_checkpoint

    assert torch.cuda.is_available()
    m = AcousticModel(device="cuda:0")
    P, S = synthetic_acoustic_checkpoint()
    m.load_params(P, S)
    yield m, P, S
    m.close()


def _bar(err_ref32, want):
    return min(4.0 * float(err_ref32) + 2.0 ** -22 * float(np.abs(want).max()), 5e-5)


def _case(golden, prefix):
    return {k[len(prefix):]: v for k, v in golden.items() if k.startswith(prefix)}


def _run_case(m, g, **kw):
    B = len(g["tokens"])
    sents = [g["tokens"][b, : g["lengths"][b]] for b in range(B)]
    durs = [g["durations_frames"][b, : g["lengths"][b]] for b in range(B)]
    pre, mel = m.teacher_forced(sents, durs, g["mels"], return_pre=True, to_host=False, **kw)
    torch.cuda.synchronize()
    return pre.cpu().numpy(), mel.cpu().numpy()


# ------------------------------------------------------------ masks ------------------------------------------------------------
@pytest.mark.parametrize("B,F", [(3, 40), (1, 1), (64, 768)])
def test_device_masks_equal_the_restatement_byte_for_byte(acoustic, golden, B, F):
    m, _, _ = acoustic
    keep_d, zone_d = m.device_teacher_masks_haiku(golden["rng_key"], B, F, partitionable=False)
    torch.cuda.synchronize()
    keep, zone = G.haiku_teacher_masks(golden["rng_key"], B, F, PN, H)
    assert keep_d.shape == (B, F, 2, PN) and zone_d.shape == (B, F, 4, H) and keep_d.dtype == torch.uint8
    assert np.array_equal(keep_d.cpu().numpy(), keep.astype(np.uint8))
    assert np.array_equal(zone_d.cpu().numpy(), zone.astype(np.uint8))


def test_device_masks_partitionable_layout_equals_its_unpinned_restatement(acoustic, golden):
    m, _, _ = acoustic
    keep_d, zone_d = m.device_teacher_masks_haiku(golden["rng_key"], 3, 40, partitionable=True)
    keep, zone = G.haiku_teacher_masks(golden["rng_key"], 3, 40, PN, H, partitionable=True)
    assert np.array_equal(keep_d.cpu().numpy(), keep.astype(np.uint8)) and np.array_equal(zone_d.cpu().numpy(), zone.astype(np.uint8))


# ------------------------------------------------------------ parity ------------------------------------------------------------
def _assert_parity(name, got_pre, got_mel, g):
    for what, got, want in (("mel1", got_pre, g["mel1"]), ("mel2", got_mel, g["mel2"])):
        assert got.shape == want.shape and got.dtype == np.float32
        err, bar = float(np.abs(got.astype(np.float64) - want).max()), _bar(g["err_ref32"], want)
        print(f"[gta parity] {name} {what}: max |gpu - fp64| {err:.3e}, bar {bar:.3e} (err_ref32 {float(g['err_ref32']):.3e}, max |want| {np.abs(want).max():.3f})")
    for what, got, want in (("mel1", got_pre, g["mel1"]), ("mel2", got_mel, g["mel2"])):
        assert float(np.abs(got.astype(np.float64) - want).max()) <= _bar(g["err_ref32"], want), (name, what)


def test_reference_padding_case_matches_the_executed_reference(acoustic, golden):
    """Case (a): B = 3, all 24 padded columns are tokens, 40 frames — once with the masks drawn on the device from the rng, once with the
    restatement's masks uploaded: the same bits, and within the bar of the reference's fp64 run."""
    m, _, _ = acoustic
    g = _case(golden, "a_")
    pre_r, mel_r = _run_case(m, g, rng=golden["rng_key"])
    keep, zone = G.haiku_teacher_masks(golden["rng_key"], 3, 40, PN, H)
    pre_m, mel_m = _run_case(m, g, masks=(keep, zone))
    assert np.array_equal(pre_r, pre_m) and np.array_equal(mel_r, mel_m)
    _assert_parity("a", pre_r, mel_r, g)


@pytest.mark.parametrize("prefix", ["b0_", "b1_", "b2_", "c_"])
def test_rows_run_alone_match_the_executed_reference(acoustic, golden, prefix):
    """Cases (b) and (c): an utterance alone, unpadded, masks drawn at (1, F_row); (c) has a single frame."""
    m, _, _ = acoustic
    g = _case(golden, prefix)
    pre, mel = _run_case(m, g, rng=golden["rng_key"])
    _assert_parity(prefix[:-1], pre, mel, g)


# ------------------------------------------------------------ rows alone ------------------------------------------------------------
def test_ragged_batch_equals_each_row_alone_bit_for_bit(acoustic, golden):
    m, _, _ = acoustic
    gs = [_case(golden, f"b{b}_") for b in range(3)]
    sents = [g["tokens"][0] for g in gs]
    durs = [g["durations_frames"][0] for g in gs]
    mels = [g["mels"][0] for g in gs]
    nfs = [x.shape[0] for x in mels]
    masks = [G.haiku_teacher_masks(golden["rng_key"], 1, nf, PN, H) for nf in nfs]
    keep, zone = [k[0] for k, _ in masks], [z[0] for _, z in masks]
    pre, mel = m.teacher_forced(sents, durs, mels, masks=(keep, zone), to_host=False, return_pre=True)
    pre, mel = pre.cpu().numpy(), mel.cpu().numpy()
    assert mel.shape == (3, max(nfs), MEL)
    for b in range(3):
        a_pre, a_mel = m.teacher_forced([sents[b]], [durs[b]], [mels[b]], masks=([keep[b]], [zone[b]]), to_host=False, return_pre=True)
        assert np.array_equal(a_mel.cpu().numpy()[0], mel[b, : nfs[b]]) and np.array_equal(a_pre.cpu().numpy()[0], pre[b, : nfs[b]])
        assert not mel[b, nfs[b]:].any() and not pre[b, nfs[b]:].any()  # rows past nframes are zero
        _assert_parity(f"b{b} in a ragged batch", pre[b : b + 1, : nfs[b]], mel[b : b + 1, : nfs[b]], gs[b])


# ------------------------------------------------------------ zoneout ------------------------------------------------------------
def test_zoneout_is_live(acoustic, golden):
    m, P, S = acoustic
    g = _case(golden, "b1_")
    F = g["mels"].shape[1]
    keep, _ = G.haiku_teacher_masks(golden["rng_key"], 1, F, PN, H)
    none = _run_case(m, g, masks=(keep, None))
    zeros = _run_case(m, g, masks=(keep, np.zeros((1, F, 4, H), bool)))
    assert np.array_equal(none[0], zeros[0]) and np.array_equal(none[1], zeros[1])  # NULL == an all-zero mask, bit for bit
    frozen = np.ones((1, F, 4, H), bool)
    frozen[:, 0] = False  # frame 0 sets the state, every later frame keeps it
    got = _run_case(m, g, masks=(keep, frozen))
    assert np.abs(got[0] - none[0])[0, 2:].max() > 1e-3  # the mask changes the result ...
    want = G.teacher_forced(P, S, g["tokens"], g["lengths"], g["durations_frames"], g["mels"], keep, frozen, np.float64)
    w32 = G.teacher_forced(P, S, g["tokens"], g["lengths"], g["durations_frames"], g["mels"], keep, frozen, np.float32)
    for i, what in enumerate(("mel1", "mel2")):  # ... to what the restatement computes with a frozen state (yardstick: ITS fp32 run, not ours)
        e32 = float(np.abs(w32[i].astype(np.float64) - want[i]).max())
        err, bar = float(np.abs(got[i].astype(np.float64) - want[i]).max()), _bar(e32, want[i])
        print(f"[gta zoneout] frozen state {what}: max |gpu - fp64| {err:.3e}, bar {bar:.3e} (oracle fp32 vs fp64 {e32:.3e})")
        assert err <= bar


# ------------------------------------------------------------ end to end ------------------------------------------------------------
def test_wav_to_gta_mel_end_to_end(acoustic, golden):
    """gta.forward_fn on the fixture's int16 wavs, reference padding: MelFilter's fp32 error now passes through a recurrent model.  The
    yardstick for that part is computed here, on the oracles alone: the fp64 teacher-forced pass on the mel oracle's fp32-class mel against the
    same on its fp64 mel; the bar is 4 x that plus the parity bar."""
    from viettts_amd.nat import gta
    from viettts_amd.nat.dsp import MelFilter

    m, P, S = acoustic
    g = _case(golden, "a_")
    mf = MelFilter(16000, 1024, 80, 0.0, 8000, device="cuda:0")
    batch = gta.AcousticInput(phonemes=g["tokens"], lengths=golden["true_lengths"], durations=g["durations_frames"] * np.float32(256) / np.float32(16000),
                              wavs=g["wavs"], wav_lengths=g["wav_lengths"])
    assert np.array_equal(np.asarray(batch.durations, np.float32) * np.float32(16000) / np.float32(256), g["durations_frames"])  # the fixture's frames, exactly
    got = gta.forward_fn(m, mf, golden["rng_key"], batch, reference_padding=True)
    mf.close()
    y = g["wavs"].astype(np.float64) / 32768.0
    mel64, mel32 = M.log_mel(y, dtype=np.float64), M.log_mel(y.astype(np.float32), dtype=np.float32)
    assert np.array_equal(mel64.astype(np.float32), g["mels"])
    keep, zone = G.haiku_teacher_masks(golden["rng_key"], 3, 40, PN, H)
    args = (P, S, g["tokens"], g["lengths"], g["durations_frames"])
    via64 = G.teacher_forced(*args, mel64, keep, zone, np.float64)[1]
    via32 = G.teacher_forced(*args, mel32.astype(np.float64), keep, zone, np.float64)[1]
    d_in, d_out = float(np.abs(mel32.astype(np.float64) - mel64).max()), float(np.abs(via32 - via64).max())
    err = float(np.abs(got.astype(np.float64) - g["mel2"]).max())
    bar = 4.0 * d_out + _bar(g["err_ref32"], g["mel2"])
    print(f"[gta e2e] target mel fp32-class vs fp64 {d_in:.3e} -> GTA mel {d_out:.3e} (amplification {d_out / d_in:.2f}); max |gpu - fp64| {err:.3e}, bar {bar:.3e}")
    assert got.shape == (3, 40, MEL) and err <= bar


def test_wav_to_gta_mel_rows_alone_is_the_default(acoustic, golden):
    """gta.forward_fn's default: a padded batch whose rows have their own token, sample and frame counts.  Row i must be that utterance alone
    (its own tokens, its wav reflected at its own end) under row i of the masks drawn at the batch's (B, F), and zero past its own frames.
    Yardsticks from the oracles alone, per row: the restatement's fp32 run against its fp64 run, and what the mel oracle's fp32-class target
    moves the fp64 result by (times 4, as in the end-to-end test above)."""
    from viettts_amd.nat import gta
    from viettts_amd.nat.dsp import MelFilter

    m, P, S = acoustic
    g = _case(golden, "a_")
    lens, wl = [int(v) for v in golden["true_lengths"]], [40 * 256, 7000, 5123]  # 40, 27 and 20 frames; the last two end inside a hop
    mf = MelFilter(16000, 1024, 80, 0.0, 8000, device="cuda:0")
    batch = gta.AcousticInput(phonemes=g["tokens"], lengths=np.asarray(lens), durations=g["durations_frames"] * np.float32(256) / np.float32(16000),
                              wavs=g["wavs"], wav_lengths=np.asarray(wl))
    got = gta.forward_fn(m, mf, golden["rng_key"], batch)
    mf.close()
    assert got.shape == (3, 40, MEL) and got.dtype == np.float32
    keep, zone = G.haiku_teacher_masks(golden["rng_key"], 3, 40, PN, H)
    for i in range(3):
        nf = wl[i] // 256
        y = g["wavs"][i : i + 1, : wl[i]].astype(np.float64) / 32768.0
        mel64, mel32 = M.log_mel(y, dtype=np.float64), M.log_mel(y.astype(np.float32), dtype=np.float32)
        assert mel64.shape[1] == nf
        args = (P, S, g["tokens"][i : i + 1, : lens[i]], [lens[i]], g["durations_frames"][i : i + 1, : lens[i]])
        k, z = keep[i : i + 1, :nf], zone[i : i + 1, :nf]
        want = G.teacher_forced(*args, mel64, k, z, np.float64)[1]
        via32 = G.teacher_forced(*args, mel32.astype(np.float64), k, z, np.float64)[1]
        w32 = G.teacher_forced(*args, mel64.astype(np.float32), k, z, np.float32)[1]
        d_out, e32 = float(np.abs(via32 - want).max()), float(np.abs(w32.astype(np.float64) - want).max())
        err, bar = float(np.abs(got[i : i + 1, :nf].astype(np.float64) - want).max()), 4.0 * d_out + _bar(e32, want)
        print(f"[gta e2e rows alone] row {i}, {nf} frames: max |gpu - fp64| {err:.3e}, bar {bar:.3e} (oracle fp32 vs fp64 {e32:.3e}, target-mel share {d_out:.3e})")
        assert err <= bar and not got[i, nf:].any()


# ------------------------------------------------------------ the reference's corpus shape ------------------------------------------------------------
def test_corpus_shape_is_finite_zero_padded_and_split_invariant(acoustic, golden):
    """64 rows x 256 tokens x 768 frames (vietTTS/nat/config.py: batch_size, max_phoneme_seq_len, max_wave_len / hop): finite, exact zeros past
    nframes, and equal to the same rows run as two half batches with the same explicit masks."""
    m, _, _ = acoustic
    B, L, F = 64, 256, 768
    rng = np.random.default_rng(31)
    sents = [rng.integers(0, 100, size=int(n)) for n in rng.integers(40, L + 1, size=B)]
    sents[0] = rng.integers(0, 100, size=L)
    nfs = [int(v) for v in rng.integers(1, F + 1, size=B)]
    nfs[0], nfs[1], nfs[40] = F, 1, F
    durs = [(w / w.sum() * nf).astype(np.float32) for w, nf in ((rng.uniform(0.2, 1.8, size=len(s)), nf) for s, nf in zip(sents, nfs))]
    mels = torch.from_numpy(rng.normal(-3.0, 1.5, size=(B, F, MEL)).astype(np.float32)).to(m.device)
    keep, zone = m.device_teacher_masks_haiku(golden["rng_key"], B, F, partitionable=False)
    pre, mel = m.teacher_forced(sents, durs, mels, n_frames=nfs, masks=(keep, zone), to_host=False, return_pre=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(mel).all()) and bool(torch.isfinite(pre).all())
    for b in range(B):
        assert not bool(mel[b, nfs[b]:].any()) and not bool(pre[b, nfs[b]:].any())
        assert bool(mel[b, : nfs[b]].abs().max() > 0)
    for r0 in (0, 32):
        sl = slice(r0, r0 + 32)
        Fh = max(nfs[sl])
        hp, hm = m.teacher_forced(sents[sl], durs[sl], mels[sl, :Fh].contiguous(), n_frames=nfs[sl], masks=(keep[sl, :Fh].contiguous(), zone[sl, :Fh].contiguous()),
                                  to_host=False, return_pre=True)
        assert torch.equal(hm, mel[sl, :Fh]) and torch.equal(hp, pre[sl, :Fh])


# ------------------------------------------------------------ option guard ------------------------------------------------------------
def test_bf16x3_option_is_refused_with_a_message(acoustic, golden):
    m, _, _ = acoustic
    g = _case(golden, "c_")
    m.set_option("bf16x3", 1)
    try:
        with pytest.raises(_lib.VttsError, match="bf16x3"):
            _run_case(m, g)
    finally:
        m.set_option("bf16x3", 0)
    pre, mel = _run_case(m, g)  # and the handle still works
    assert np.isfinite(mel).all()
