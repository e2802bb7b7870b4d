"""The teacher-forced acoustic pass without a GPU: the numpy restatement (tests/_gta_oracle.py) against the fixture minted from the
reference's own ``AcousticModel.__call__`` (tools/make_gta_golden.py), the restated mask stream, the C ABI's exports, and the file
naming / cropping of ``viettts_amd.nat.gta.generate_gta`` on a stub model."""
import re

import numpy as np
import pytest

import _gta_oracle as G
from oracle import nat_oracle as O
from viettts_amd.nat.synth import synthetic_acoustic_checkpoint

CASES = ("a_", "b0_", "b1_", "b2_", "c_")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(golden_dir / "nat_gta_golden.npz"))


@pytest.mark.parametrize("case", CASES)
def test_oracle_reproduces_the_executed_reference(golden, case):
    P, S = synthetic_acoustic_checkpoint()
    g = {k[len(case):]: v for k, v in golden.items() if k.startswith(case)}
    B, F = g["mels"].shape[:2]
    keep, zone = G.haiku_teacher_masks(golden["rng_key"], B, F)
    m1, m2 = G.teacher_forced(P, S, g["tokens"], g["lengths"], g["durations_frames"], g["mels"], keep, zone, np.float64)
    assert m1.shape == g["mel1"].shape == (B, F, 80)
    assert np.abs(m1 - g["mel1"]).max() <= 1e-12 and np.abs(m2 - g["mel2"]).max() <= 1e-12
    assert 0.0 < float(g["err_ref32"]) < 1e-5  # the reference's own fp32 run against its fp64 run: the GPU tests' yardstick


def test_fixture_cases_are_the_stated_ones(golden):
    assert golden["a_tokens"].shape == (3, 24) and (golden["a_lengths"] == 24).all() and golden["a_mels"].shape == (3, 40, 80)
    assert list(golden["true_lengths"]) == [24, 17, 11]
    for b, n in enumerate(golden["true_lengths"]):
        assert (golden["a_tokens"][b, n:] == 0).all() and (golden["a_durations_frames"][b, n:] == 0).all()
        Fb = int(golden["a_wav_lengths"][b]) // 256
        assert golden[f"b{b}_tokens"].shape == (1, n) and golden[f"b{b}_mels"].shape == (1, Fb, 80)
        assert np.array_equal(golden[f"b{b}_mels"][0], golden["a_mels"][b, :Fb])
        assert (golden["a_wavs"][b, golden["a_wav_lengths"][b]:] == 0).all()
    assert golden["c_mels"].shape == (1, 1, 80)
    assert golden["a_wavs"].shape == (3, 40 * 256) and golden["a_wavs"].dtype == np.int16
    # a true length instead of the padded one moves the row: the two padding semantics are different computations
    P, S = synthetic_acoustic_checkpoint()
    full = G.teacher_forced_row(P, S, golden["a_tokens"][2], 24, golden["a_durations_frames"][2], golden["a_mels"][2])[1]
    short = G.teacher_forced_row(P, S, golden["a_tokens"][2], 11, golden["a_durations_frames"][2], golden["a_mels"][2])[1]
    assert np.abs(full - short).max() > 1e-4


def test_mask_restatement_draws_six_times_in_the_stated_order_and_shapes():
    key = np.array([7, 11], np.uint32)
    B, F, PN, H = 2, 5, 256, 512
    keep, zone = G.haiku_teacher_masks(key, B, F, PN, H)
    assert keep.shape == (B, F, 2, PN) and zone.shape == (B, F, 4, H) and keep.dtype == bool and zone.dtype == bool
    k, subs = key, []
    for _ in range(6):
        ks = O.jax_legacy_split(k, 2)
        k, sub = ks[0], ks[1]
        subs.append(sub)
    for d in range(6):  # slice-wise recomputation: draw d, element i of the flattened (B, F, D) tensor
        D, p = (PN, 0.5) if d < 2 else (H, 0.1)
        got = (keep[:, :, d] if d < 2 else zone[:, :, d - 2]).reshape(-1)
        n = B * F * D
        half = (n + 1) // 2
        for i in (0, 1, half - 1, half, n - 1, 12345 % n):
            j = i if i < half else i - half
            x0, x1 = O.threefry2x32_20(subs[d][0], subs[d][1], np.uint32(j), np.uint32(j + half if j + half < n else 0))
            word = np.uint32(x0 if i < half else x1)
            u = ((word >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)
            assert bool(got[i]) == bool(u < np.float32(p)), (d, i)
    # a row's masks depend on the batch shape: the same key at (1, F) is another stream
    k1, z1 = G.haiku_teacher_masks(key, 1, F, PN, H)
    assert not np.array_equal(k1[0], keep[0]) and not np.array_equal(z1[0], zone[0])
    # an odd element count is padded with one zero count
    ko, zo = G.haiku_teacher_masks(key, 1, 3, 5, 7)
    assert ko.shape == (1, 3, 2, 5) and zo.shape == (1, 3, 4, 7)
    # the two threefry layouts differ
    kp, zp = G.haiku_teacher_masks(key, B, F, PN, H, partitionable=True)
    assert not np.array_equal(kp, keep) and not np.array_equal(zp, zone)


def test_zoneout_and_dropout_rates():
    keep, zone = G.haiku_teacher_masks(np.array([0x1234ABCD, 0x0F1E2D3C], np.uint32), 4, 64)
    assert zone.shape == (4, 64, 4, 512)
    for j in range(4):
        assert abs(zone[:, :, j].mean() - 0.1) <= 0.01
    for j in range(2):
        assert abs(keep[:, :, j].mean() - 0.5) <= 0.01


def test_zoneout_freezes_the_state_but_not_the_output():
    """All-ones zoneout after frame 0: h and c stay what frame 0 left, while the decoder's output keeps following its input."""
    P, S = synthetic_acoustic_checkpoint()
    rng = np.random.default_rng(5)
    tok, dur, mel = rng.integers(1, 90, size=6), np.full(6, 2.0, np.float32), rng.normal(0, 1, size=(12, 80)).astype(np.float32)
    zone = np.ones((12, 4, 512), bool)
    zone[0] = False
    m1, _, st = G.teacher_forced_row(P, S, tok, 6, dur, mel, None, zone, np.float64, return_states=True)
    assert all(np.array_equal(st[t], st[0]) for t in range(1, 12))
    assert np.abs(m1[5] - m1[6]).max() > 1e-3
    free = G.teacher_forced_row(P, S, tok, 6, dur, mel, None, None, np.float64)[0]
    assert np.array_equal(free[0], m1[0]) and np.abs(free[3] - m1[3]).max() > 1e-4


def test_every_declared_nat_symbol_is_exported():
    from viettts_amd.csrc import build

    lib = build.build()
    header = (build.ROOT / "include" / "vtts_nat.h").read_text()
    declared = set(re.findall(r"\b(vtts_nat_[a-z0-9_]+)\s*\(", header))
    assert {"vtts_nat_acoustic_forward_teacher", "vtts_nat_acoustic_forward_teacher_workspace_bytes", "vtts_nat_acoustic_teacher_masks_haiku"} <= declared
    from viettts_amd import _lib

    cdll = _lib.load(lib)  # declares every prototype of the binding: AttributeError if one is not exported
    missing = sorted(n for n in declared if not hasattr(cdll, n))
    assert not missing, missing


def test_generate_gta_crops_and_names_like_the_reference(tmp_path):
    """gta.py:72-76 on a stub model: NAME.npy = mel[idx, :wav_length // hop].T, float32 [80, l]; durations reach the model in frames, fp32."""
    from viettts_amd.nat import gta

    hop, Fp = 256, 9
    seen = {}

    class StubMel:
        hop, sample_rate = 256, 16000

        def __call__(self, wavs, lengths=None):
            seen["mel_lengths"] = lengths
            return np.zeros((len(wavs), Fp, 80), np.float32)

    class StubModel:
        checkpoint_rng = np.array([1, 2], np.uint32)
        device = "cpu"

        def teacher_forced(self, sentences, durations_frames, mels, n_frames=None, rng=None, masks=None, to_host=True, return_pre=False):
            seen.update(sentences=sentences, durations=durations_frames, n_frames=n_frames, rng=rng)
            out = np.arange(len(sentences) * Fp * 80, dtype=np.float32).reshape(len(sentences), Fp, 80)
            return type("Dev", (), {"cpu": lambda self: type("H", (), {"numpy": lambda self: out})()})()  # stands in for a device tensor: .cpu().numpy()

    batch = gta.AcousticInput(phonemes=np.array([[5, 6, 7, 0], [8, 9, 0, 0]], np.int32), lengths=np.array([3, 2], np.int32),
                              durations=np.array([[0.016, 0.032, 0.048, 0], [0.064, 0.016, 0, 0]], np.float32),
                              wavs=np.zeros((2, Fp * hop), np.int16), wav_lengths=np.array([Fp * hop, 5 * hop + 100], np.int32))
    files = gta.generate_gta(tmp_path / "gta", [(["utt_a", "utt_b"], batch)], model=StubModel(), melfilter=StubMel())
    assert [f.name for f in files] == ["utt_a.npy", "utt_b.npy"]
    a, b = np.load(files[0]), np.load(files[1])
    assert a.shape == (80, 9) and b.shape == (80, 5) and a.dtype == np.float32
    full = np.arange(2 * Fp * 80, dtype=np.float32).reshape(2, Fp, 80)
    assert np.array_equal(a, full[0].T) and np.array_equal(b, full[1, :5].T)
    # rows alone: each row's own tokens, own frames; durations in frames (seconds * 16000 / 256), fp32
    assert [len(s) for s in seen["sentences"]] == [3, 2] and seen["n_frames"] == [9, 5] and seen["mel_lengths"] == [Fp * hop, 5 * hop + 100]
    assert np.array_equal(seen["durations"][0], np.array([0.016, 0.032, 0.048], np.float32) * np.float32(16000) / np.float32(256))
    assert np.array_equal(seen["rng"], [1, 2])
    # reference padding: all padded columns are tokens, all frames of the padded wav are frames
    gta.generate_gta(tmp_path / "gta2", [(["utt_a", "utt_b"], batch)], model=StubModel(), melfilter=StubMel(), reference_padding=True)
    assert [len(s) for s in seen["sentences"]] == [4, 4] and seen["n_frames"] == [Fp, Fp] and seen["mel_lengths"] is None
    assert np.load(tmp_path / "gta2" / "utt_b.npy").shape == (80, 5)


def test_reference_import_path_resolves():
    import vietTTS.nat.gta as ref_path
    import viettts_amd.nat.gta as ours

    assert ref_path.forward_fn is ours.forward_fn and ref_path.generate_gta is ours.generate_gta
