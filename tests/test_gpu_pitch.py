"""The fused YIN kernel (viettts_amd/csrc/pitch.hip, include/vtts_pitch.h) on the GPU against the float32 restatement of the contract
(tests/_pitch_oracle.py).  Every output word of every frame is compared with ==: there is no tolerance anywhere.  The outputs are
pre-filled with NaN through the C ABI, so whatever the kernel does not write shows.  tests/test_pitch_cpu.py shows that each deviation
from the contract one could plant changes an output bit on these very inputs."""
import ctypes as C

import numpy as np
import pytest
import torch

import _pitch_oracle as O
import _row_split as RS
from viettts_amd import _lib
from viettts_amd._handle import ptr

pytestmark = pytest.mark.gpu
FPB = O.K["VTTS_PITCH_FRAMES_PER_BLOCK"]
_TRACKERS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    yield torch.device("cuda:0")
    for t in _TRACKERS.values():
        t.close()
    _TRACKERS.clear()


def _tracker(cfg: O.Cfg, dev):
    from viettts_amd.pitch import PitchTracker

    if cfg not in _TRACKERS:
        _TRACKERS[cfg] = PitchTracker(cfg.sample_rate, cfg.fmin, cfg.fmax, cfg.threshold, device=dev)
        assert (_TRACKERS[cfg].tau_min, _TRACKERS[cfg].tau_max) == O.lags(cfg)
    return _TRACKERS[cfg]


def _run(trk, y, lengths=None, t_extra=0):
    """forward() through the C ABI into NaN-filled outputs of ``t_extra`` frames more than the longest row has: [3, N, T] f0 / aperiodicity / candidate."""
    yt = torch.from_numpy(np.array(y)).to(trk.device)  # (a copy: the shared rows are read-only)
    N, S = y.shape
    lens = [S] * N if lengths is None else [int(v) for v in lengths]
    T = max(O.num_frames(n) for n in lens) + t_extra
    out = torch.full((3, N, T), float("nan"), dtype=torch.float32, device=trk.device)
    lens_c = None if lengths is None else (C.c_int32 * N)(*lens)
    dtype = _lib.VTTS_MEL_PCM16 if y.dtype == np.int16 else _lib.VTTS_MEL_F32
    trk._on_stream("forward", ptr(yt), dtype, N, S, lens_c, ptr(out[0]), ptr(out[1]), ptr(out[2]), T, None)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _want(r: O.Yin, t_extra=0):
    w = np.stack([r.f0, r.aperiodicity, r.candidate])
    if t_extra:
        fill = np.broadcast_to(np.array([0, 1, 0], np.float32)[:, None, None], (3, w.shape[1], t_extra))
        w = np.concatenate([w, fill], axis=2)
    return w


def _same(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[bad][:5], want[bad][:5])


@pytest.mark.parametrize("name", list(O.LAG_EDGE_CFGS))
def test_lag_count_edges(dev, name):
    """tau_max at and around the 64-lag blocks a lane owns, the largest (the whole frame), tau_min 2, and a search range of one lag."""
    cfg = O.LAG_EDGE_CFGS[name]
    y, lengths = O.content_rows()
    _same(_run(_tracker(cfg, dev), y, lengths), _want(O.yin_f32(y, cfg, lengths)))


@pytest.mark.parametrize("pcm", [False, True], ids=["f32", "pcm16"])
def test_length_edges(dev, pcm):
    """Rows of 385, 511, 512, 513 samples and of one less, exactly and one more than F - 1, F, F + 1, 2 F, 2 F + 1 hops (F frames per workgroup)."""
    lengths = O.edge_lengths(FPB)
    assert len(lengths) <= 20 and 385 in lengths
    y = O.rows_of(lengths, pcm)
    assert y.dtype == (np.int16 if pcm else np.float32)
    _same(_run(_tracker(O.DEFAULT, dev), y, lengths), _want(O.yin_f32(y, O.DEFAULT, lengths)))


@pytest.mark.parametrize("pcm", [False, True], ids=["f32", "pcm16"])
def test_ragged_batch_rows_equal_the_rows_alone(dev, pcm):
    """8 rows in a stride longer than all of them, NaN (0x7FFF) behind every row; the output has three frames more than any row needs."""
    y, lengths = O.ragged_batch(FPB, pcm)
    assert y.shape[0] == 8 and y.shape[1] > max(lengths)
    assert np.all(y[:, -1] == 0x7FFF) if pcm else np.isnan(y[:, -1]).all()
    trk = _tracker(O.DEFAULT, dev)
    got = _run(trk, y, lengths, t_extra=3)
    _same(got, _want(O.yin_f32(y, O.DEFAULT, lengths), t_extra=3))
    for b, n in enumerate(lengths):
        alone = _run(trk, np.ascontiguousarray(y[b : b + 1, :n]))
        Tb = O.num_frames(n)
        assert alone.shape == (3, 1, Tb)
        assert np.array_equal(alone[:, 0].view(np.uint32), got[:, b, :Tb].view(np.uint32)), b  # bit for bit: the row is reflected at its own end
        assert np.all(got[0, b, Tb:] == 0) and np.all(got[1, b, Tb:] == 1) and np.all(got[2, b, Tb:] == 0), b


@pytest.mark.parametrize("pcm", [False, True], ids=["f32", "pcm16"])
def test_rows_behind_the_launch_split_against_the_oracle(dev, pcm):
    """PITCH_ROWS_PER_LAUNCH + 3 rows (tests/_row_split.py): the rows behind the split differ from the first rows in content and length and
    hold the longest and the shortest row, so a second launch without ``r0`` on its input, its lengths or an output computes something else
    than yin_f32 says.  NaN-filled outputs with two spare frames; the fill rule past every row's frames."""
    bt = RS.frames_batch(_lib.PITCH_ROWS_PER_LAUNCH, pcm)
    assert bt.N == _lib.PITCH_ROWS_PER_LAUNCH + 3 and bt.rows.dtype == (np.int16 if pcm else np.float32)
    want = RS.per_kind(bt, lambda r: _want(O.yin_f32(r.content[None], O.DEFAULT, [r.length])))
    got = _run(_tracker(O.DEFAULT, dev), bt.rows, bt.lengths, t_extra=2)
    assert got.shape[2] == O.num_frames(max(bt.lengths[bt.P :])) + 2
    for b, n in enumerate(bt.lengths):
        Tb = O.num_frames(n)
        assert np.array_equal(got[:, b, :Tb].view(np.uint32), want[b][:, 0, :Tb].view(np.uint32)), b
        assert np.all(got[0, b, Tb:] == 0) and np.all(got[1, b, Tb:] == 1) and np.all(got[2, b, Tb:] == 0), b
    print(f"\npitch rows behind the split: {bt.k} rows ==, worst error / bar 0 (the contract is ==)")


@pytest.mark.parametrize("pcm", [False, True], ids=["f32", "pcm16"])
def test_unaligned_batch_takes_the_scalar_loads_to_the_same_bits(dev, pcm):
    """Three ragged rows as a view into a flat buffer that starts one element in, at an odd row stride: neither the base nor any row is on
    16 bytes, so the staging takes the scalar loads.  Bit for bit the same rows in an aligned buffer at an aligned stride."""
    bt = RS.frames_batch(_lib.PITCH_ROWS_PER_LAUNCH, pcm)
    pick = [0, bt.P, bt.P + 1]  # with a fourth row, the f32 row 3 would sit on 16 bytes again
    y, lengths = bt.rows[pick], [bt.lengths[b] for b in pick]
    trk = _tracker(O.DEFAULT, dev)
    want = _run(trk, y, lengths, t_extra=1)
    _same(want, _want(O.yin_f32(y, O.DEFAULT, lengths), t_extra=1))
    N, S = y.shape
    odd = S + 1
    assert S % 8 == 0 and odd % 2 == 1
    flat = torch.full((1 + N * odd,), 0x7FFF if pcm else float("nan"), dtype=torch.int16 if pcm else torch.float32, device=trk.device)
    view = flat[1:].view(N, odd)
    view[:, :S] = torch.from_numpy(np.array(y)).to(trk.device)
    assert view.data_ptr() % 16 != 0 and all((view.data_ptr() + b * odd * view.element_size()) % 16 != 0 for b in range(N))
    T = want.shape[2]
    out = torch.full((3, N, T), float("nan"), dtype=torch.float32, device=trk.device)
    trk._on_stream("forward", ptr(view), _lib.VTTS_MEL_PCM16 if pcm else _lib.VTTS_MEL_F32, N, odd, (C.c_int32 * N)(*lengths), ptr(out[0]), ptr(out[1]), ptr(out[2]), T, None)
    torch.cuda.synchronize()
    _same(out.cpu().numpy(), want)


def test_content_voiced_noise_and_silence(dev):
    """The 1152 frames of the float64 agreement test: gliding voiced speech-like frames, noise, exact zeros."""
    want = O.agreement_f32()
    assert want.voiced.sum() > 0 and (want.aperiodicity == 1).sum() > 0
    _same(_run(_tracker(O.DEFAULT, dev), O.agreement_rows()), _want(want))


def test_content_zero_square_and_ties(dev):
    """An all-zero row (the run > 0 guard, a tie over the whole range), a full-scale square wave (d up to 2048) and the tie-rich grid row, at the
    default threshold and at one that sits exactly on a value c takes (< against <=)."""
    y, lengths = O.content_rows()
    for cfg in (O.DEFAULT, O.threshold_on_a_value()):
        got = _run(_tracker(cfg, dev), y, lengths)
        _same(got, _want(O.yin_f32(y, cfg, lengths)))
    T1 = O.num_frames(lengths[1])
    assert np.all(got[0, 1, :T1] == 0) and np.all(got[1, 1, :T1] == 1) and np.all(got[2, 1, :T1] == np.float32(16000.0) / np.float32(32.0))


def test_multi_block_rows(dev):
    """3 rows of up to 300 frames: 38 workgroups per row, the last one partial, and rows that end inside other tiles."""
    lengths = [300 * O.HOP, 299 * O.HOP + 255, 203 * O.HOP + 17]
    y = np.stack([np.concatenate([O.glide_row(s) for s in (b, b + 3, b + 6, b + 9)])[: lengths[0]] for b in range(3)])
    assert O.num_frames(lengths[0]) == 300 and 300 % FPB != 0
    _same(_run(_tracker(O.DEFAULT, dev), y, lengths), _want(O.yin_f32(y, O.DEFAULT, lengths)))


def test_python_surface(dev):
    from viettts_amd.nat.dsp import MelFilter
    from viettts_amd.pitch import PitchResult, PitchTracker, f0_metrics, wav_f0_metrics

    y, lengths = O.content_rows()
    y = y.copy()
    trk = _tracker(O.DEFAULT, dev)
    r = trk(y, lengths)  # a numpy array is copied up
    assert isinstance(r, PitchResult) and all(t.is_cuda and t.dtype == torch.float32 for t in r)
    mf = MelFilter(16000, 1024, 80, 0.0, 8000, device=dev)
    mel = mf(y, lengths=lengths)
    assert tuple(r.f0.shape) == tuple(mel.shape[:2]) == tuple(r.aperiodicity.shape) == tuple(r.candidate.shape)
    assert all(trk.num_frames(n) == mf.num_frames(n) for n in lengths)
    mf.close()
    torch.cuda.synchronize()
    _same(torch.stack(list(r)).cpu().numpy(), _want(O.yin_f32(y, O.DEFAULT, lengths)))
    yt = torch.from_numpy(y).to(dev)
    m = wav_f0_metrics(yt, yt, lengths)
    assert m["voicing_error"] == 0.0 and m["f0_rmse_cents"] == 0.0 and m["gross_error"] == 0.0 and m["voiced_frames"] == int(O.yin_f32(y, O.DEFAULT, lengths).voiced.sum())
    # a tracker named by "cuda" (the current device), and a resynthesis an octave up in a third of the frames
    other = PitchTracker(device="cuda")
    assert other.device == trk.device and torch.equal(other(yt, lengths).f0, r.f0)
    other.close()
    f = r.f0.clone()
    f[:, ::3] *= 2
    m = f0_metrics(f, r.f0, [trk.num_frames(n) for n in lengths])
    assert m["voicing_error"] == 0.0 and 0.2 < m["gross_error"] < 0.5
    with pytest.raises(_lib.VttsError):
        trk(yt[:, :384].contiguous())
    with pytest.raises(ValueError):
        trk(yt.double())


def test_score_segments_gains_the_f0_keys_only_with_a_tracker(dev):
    from viettts_amd import vocoder_eval
    from viettts_amd.hifigan.config import V1
    from viettts_amd.hifigan.disc_synth import synthetic_disc_checkpoint
    from viettts_amd.hifigan.discriminators import Discriminators, fold_checkpoint
    from viettts_amd.hifigan.generator import Generator
    from viettts_amd.hifigan.synth import synthetic_params

    gen = Generator(V1, device=dev)
    gen.load_params(synthetic_params(V1, 4321, "scaled"))
    disc = Discriminators(dev).load_params(fold_checkpoint(synthetic_disc_checkpoint(8642)))
    y = torch.from_numpy(np.stack([O.glide_row(0)[:8192], O.glide_row(1)[2048 : 2048 + 8192]])).to(dev)
    plain = vocoder_eval.score_segments(y, gen, disc)
    assert set(plain) == {"adv", "fm", "mel", "total", "disc"}
    scored = vocoder_eval.score_segments(y, gen, disc, tracker=_tracker(O.DEFAULT, dev))
    assert set(scored) == set(plain) | {"f0_rmse_cents", "voicing_error", "gross_error"} == set(plain) | set(vocoder_eval.F0_KEYS)
    assert all(scored[k] == pytest.approx(plain[k], rel=1e-6) for k in plain)  # the existing figures are what they were
    assert 0.0 <= scored["voicing_error"] <= 1.0
    gen.close()
    disc.close()


@pytest.mark.parametrize("rate", [16000, 22050])
def test_command_line(dev, tmp_path, capsys, rate):
    """``python -m viettts_amd.pitch``: a 200 Hz tone at the model's rate and at another one (converted on the GPU first)."""
    from viettts_amd import pitch, wavio

    t = np.arange(rate) / rate
    wavio.write_wav_pcm16(tmp_path / "tone.wav", O.to_pcm16(0.3 * np.sin(2 * np.pi * 200.0 * t) + 0.1 * np.sin(2 * np.pi * 400.0 * t)), rate)
    pitch.main(["--wav", str(tmp_path / "tone.wav"), "--output", str(tmp_path / "f0.npy")])
    line = capsys.readouterr().out
    got = np.load(tmp_path / "f0.npy")
    assert got.shape == (16000 // 256, 3) and got.dtype == np.float32 and f"{got.shape[0]} frames" in line and "F0 median" in line
    inner = got[3:-3]
    assert np.all(inner[:, 0] == inner[:, 2]) and np.all(np.abs(1200.0 * np.log2(inner[:, 0] / 200.0)) < 5.0) and np.all(inner[:, 1] < 0.15)
