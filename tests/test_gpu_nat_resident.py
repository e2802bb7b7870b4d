"""The acoustic decoder's frame loop as one resident kernel (option "resident" of include/vtts_nat.h; viettts_amd/csrc/nat_resident.hip), the low-latency
path for one to four sentences: against the fp64 oracle and the reference-executed golden with the bars of the per-frame launches, rows independent of their
batch, re-use of a handle, and every case that must fall back to the launches."""
import numpy as np
import pytest

from oracle import nat_oracle as no
from viettts_amd import _lib
from viettts_amd.nat import text2mel as t2m
from viettts_amd.nat.acoustic import AcousticModel, bernoulli_keep_masks
from viettts_amd.nat.synth import synthetic_acoustic_checkpoint

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def acoustic():
    m = AcousticModel(device="cuda:0")
    P, S = synthetic_acoustic_checkpoint()
    m.load_params(P, S)
    yield m, P, S
    m.close()


@pytest.fixture()
def resident(acoustic):
    m, P, S = acoustic
    m.set_option("resident", 1)
    try:
        yield m, P, S
    finally:
        m.set_option("resident", 0)
        m.set_option("bf16x3", 0)


def _case(seed, L):
    rng = np.random.default_rng(seed)
    tok = list(rng.integers(0, 100, size=L))
    dur = np.abs(rng.normal(3.0, 1.5, size=L)).astype(np.float32)  # frames per token
    dur[rng.integers(0, L)] = 0.0  # a word-end token (text2mel.py:95-97)
    nf = max(1, int(np.sum(dur, dtype=np.float32)))
    return tok, dur, nf


_ORACLE = {}


def _oracle(P, S, case, keep=None):
    """fp64 oracle mel of a case, computed once per (case, masks) and shared."""
    tok, dur, nf = case
    key = (tuple(tok), dur.tobytes(), nf, None if keep is None else keep.tobytes())
    if key not in _ORACLE:
        masks = None if keep is None else (lambda t: (keep[t, 0], keep[t, 1]))
        _ORACLE[key] = no.acoustic_inference(P, S, np.array(tok), dur, nf, prenet_masks=masks, dtype=np.float64)
    return _ORACLE[key]


def _run(m, cases, keeps=None, **kw):
    return m([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], keep_masks=keeps, **kw)


@pytest.mark.parametrize("dropout", [False, True], ids=["no-dropout", "explicit-masks"])
def test_resident_matches_oracle(resident, dropout):
    m, P, S = resident
    one, seven, thirty = _case(21, 1), _case(22, 7), _case(23, 30)
    assert 1 <= one[2] <= 3
    ragged = [_case(41, 28), _case(42, 2), _case(43, 12), _case(44, 1)]  # very different frame counts: rows stop early
    assert max(c[2] for c in ragged) > 8 * min(c[2] for c in ragged)
    for cases in ([one], [seven], [thirty], [one, seven, thirty], ragged):
        keeps = [bernoulli_keep_masks(c[2], seed=5 + i) for i, c in enumerate(cases)] if dropout else None
        got = _run(m, cases, keeps)
        assert m.resident_used == 1
        dev = _run(m, cases, keeps, to_host=False)
        assert m.resident_used == 1
        dev = dev.cpu().numpy()
        m.set_option("resident", 0)
        try:
            launches = _run(m, cases, keeps)
            assert m.resident_used == 0
        finally:
            m.set_option("resident", 1)
        for i, (c, g) in enumerate(zip(cases, got)):
            ref = _oracle(P, S, c, keeps[i] if dropout else None)
            assert g.shape == ref.shape == (c[2], 80)
            err = np.abs(g - ref).max()
            print(f"[resident, B = {len(cases)}, row {i}: {c[2]} frames, dropout {dropout}] max|g - oracle| {err:.2e}, max|g - launches| {np.abs(g - launches[i]).max():.2e}")
            assert err < 5e-4 * max(1.0, np.abs(ref).max()), err
            assert np.array_equal(dev[i, : c[2]], g)
            assert not dev[i, c[2] :].any()  # rows past nframes are zero


def test_resident_text2mel_equals_the_reference_code_executed(tmp_path, monkeypatch):
    """tests/test_gpu_nat.py::test_text2mel_equals_the_reference_code_executed with set_low_latency(True): the reference's own text2mel.py / model.py output
    (tests/golden/nat_text2mel_golden.npz: 174, 218 and 278 frames), the same frame counts, the same 5e-5 bar."""
    from pathlib import Path

    from oracle.make_nat_golden import write_checkpoints

    g = np.load(Path(__file__).parent / "golden" / "nat_text2mel_golden.npz")
    assert write_checkpoints(tmp_path) == str(g["params_sha256"])
    lexicon = Path(__file__).parent / "golden" / "text" / "lexicon.txt"
    monkeypatch.chdir(tmp_path)
    t2m.set_duration_model(None)
    t2m.set_acoustic_model(None)
    was = t2m.get_low_latency()
    t2m.set_low_latency(True)
    try:
        for ci in range(int(g["n_cases"])):
            p = f"c{ci}_"
            text, sil = str(g[p + "text"]), float(g[p + "silence_duration"])
            mel = t2m.text2mel(text, lexicon, sil)
            assert t2m._ACOUSTIC_MODEL.resident_used == 1
            want = g[p + "mel_full"][: int(g[p + "n_frames"]) - int(g[p + "trailing_frames"])]
            assert mel.shape == (1,) + want.shape, (mel.shape, want.shape)  # integer frame counts: bit-exact
            err = float(np.abs(mel[0].astype(np.float64) - want).max())
            print(f"[low-latency text2mel vs the reference's code, case {ci}: {want.shape[0]} frames] max|d mel| {err:.2e}")
            assert err < 5e-5
    finally:
        t2m.set_low_latency(was)
        t2m.set_duration_model(None)
        t2m.set_acoustic_model(None)


def test_resident_rows_do_not_depend_on_the_batch(resident):
    m, _, _ = resident
    cases = [_case(51, 9), _case(52, 25), _case(53, 3), _case(54, 16)]
    keeps = [bernoulli_keep_masks(c[2], seed=60 + i) for i, c in enumerate(cases)]
    both = _run(m, cases, keeps)
    assert m.resident_used == 1
    again = _run(m, cases, keeps)
    for i, c in enumerate(cases):
        assert np.array_equal(both[i], again[i])  # two identical calls: identical bits
        alone = _run(m, [c], [keeps[i]])[0]
        assert m.resident_used == 1
        assert np.array_equal(alone, both[i])


def test_resident_handle_reuse(resident):
    """A long call, a two-frame call, the long one again on ONE handle (the arrival counter and the exchange buffers start afresh every call) against a
    handle that runs each for the first time."""
    m, P, S = resident
    long_ = [_case(71, 30), _case(72, 11)]
    assert 75 <= max(c[2] for c in long_) <= 110
    tiny = ([5, 9], np.array([1.0, 1.0], np.float32), 2)
    first = _run(m, long_)
    short = _run(m, [tiny])
    assert m.resident_used == 1 and len(short[0]) == 2
    third = _run(m, long_)
    assert m.resident_status() is False
    fresh = AcousticModel(device="cuda:0")
    try:
        fresh.load_params(P, S)
        fresh.set_option("resident", 1)
        want_short = _run(fresh, [tiny])
        assert fresh.resident_used == 1
    finally:
        fresh.close()
    fresh = AcousticModel(device="cuda:0")
    try:
        fresh.load_params(P, S)
        fresh.set_option("resident", 1)
        want_long = _run(fresh, long_)
    finally:
        fresh.close()
    assert np.array_equal(short[0], want_short[0])
    for a, b, w in zip(first, third, want_long):
        assert np.array_equal(a, w) and np.array_equal(b, w)


def test_resident_fallbacks(acoustic):
    m, P, S = acoustic
    fresh = AcousticModel(device="cuda:0")
    try:
        fresh.load_params(P, S)
        with pytest.raises(_lib.VttsError):  # no resident launch yet: the state error
            fresh.resident_status()
        assert fresh.get_option("resident") == 0
        fresh.set_option("resident", 1)
        assert fresh.get_option("resident") == 1
        with pytest.raises(_lib.VttsError):
            fresh.set_option("resident", 2)
        assert fresh.get_option("resident") == 1
        fresh.set_option("resident", 0)
        assert fresh.get_option("resident") == 0
    finally:
        fresh.close()
    five = [_case(80 + i, 3 + 2 * i) for i in range(5)]
    two = five[:2]

    def both_modes(fn):
        m.set_option("resident", 0)
        want = fn()
        m.set_option("resident", 1)
        try:
            got = fn()
            used = m.resident_used
        finally:
            m.set_option("resident", 0)
        return want, got, used

    want, got, used = both_modes(lambda: _run(m, five))  # B = 5
    assert used == 0 and all(np.array_equal(a, b) for a, b in zip(want, got))
    m.set_option("bf16x3", 1)
    try:
        want, got, used = both_modes(lambda: _run(m, two))  # bf16x3 set
    finally:
        m.set_option("bf16x3", 0)
    assert used == 0 and all(np.array_equal(a, b) for a, b in zip(want, got))
    want, got, used = both_modes(lambda: _run(m, two, to_host=False, group_row0=[0, 1, 2]).cpu().numpy())  # a group hand-over
    assert used == 0 and np.array_equal(want, got)
    m.set_option("resident", 1)  # ... and the same two sentences without any of these do take it
    try:
        _run(m, two)
        assert m.resident_used == 1
    finally:
        m.set_option("resident", 0)


def test_resident_from_a_precomputed_encoder_output(resident):
    m, _, _ = resident
    cases = [_case(91, 12), _case(92, 5), _case(93, 20)]
    plain = _run(m, cases)
    assert m.resident_used == 1
    enc = m.encode([c[0] for c in cases])
    got = _run(m, cases, encoded=enc)
    assert m.resident_used == 1
    for a, b in zip(plain, got):
        assert np.array_equal(a, b)
