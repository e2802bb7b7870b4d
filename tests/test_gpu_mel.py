"""The fused waveform -> log-mel kernel (viettts_amd/csrc/mel.hip, include/vtts_mel.h) on the GPU against the fp64 oracle.

The bar, for every input and over EVERY element of the output (nothing masked):

    max |gpu - fp64|  <=  4 * err_ref32 + 2^-22 * max |fp64|

``err_ref32`` is the error of the reference's own arithmetic class (fp32 with a complex64 FFT) against fp64 on that input: read from
the fixture (tests/golden/mel_golden.npz, minted by tools/make_mel_golden.py from the reference's programs) or recomputed by the fp32
restatement (tests/_mel_oracle.py) for inputs made here; it is never taken from the kernel under test.  The second term is two fp32
ulps at the largest output: logf's one ulp and the final rounding.  All inputs carry a noise floor: log of a band near the 1e-5 floor
amplifies any absolute error, and no fp32 transform meets fp64 there.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import _mel_oracle as oracle
import _row_split as RS
from viettts_amd import _lib
from viettts_amd._handle import ptr

pytestmark = pytest.mark.gpu
FLOOR32 = np.float32(math.log(1e-5))
FPB = _lib.MEL_FRAMES_PER_BLOCK


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(golden_dir / "mel_golden.npz"))


@pytest.fixture(scope="module")
def mf(dev):
    from viettts_amd.nat.dsp import MelFilter

    f = MelFilter(16000, 1024, 80, 0.0, 8000, device=dev)
    yield f
    f.close()


def _bar(err_ref32, want):
    return 4.0 * float(err_ref32) + 2.0 ** -22 * float(np.abs(want).max())


def _run(mf, y, lengths=None):
    """Output pre-filled with NaN: whatever the kernel does not write shows."""
    yt = torch.from_numpy(np.ascontiguousarray(y)).to(mf.device)
    lens = [y.shape[1]] * y.shape[0] if lengths is None else [int(v) for v in lengths]
    T = max(oracle.num_frames(n) for n in lens)
    out = torch.full((y.shape[0], T, 80), float("nan"), dtype=torch.float32, device=mf.device)
    got = mf(yt, lengths=lengths, out=out)
    assert got is out
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("name", ["speech", "pcm", "noise"])
def test_parity_with_the_reference(mf, golden, name):
    y, want = golden[name], golden["mel_" + name]
    got = _run(mf, y)
    assert got.shape == want.shape and got.dtype == np.float32
    assert not np.isnan(got).any()
    err, bar = float(np.abs(got.astype(np.float64) - want).max()), _bar(golden["err_ref32_" + name], want)
    print(f"\n{name}: max|gpu - fp64| = {err:.3e}, err_ref32 = {float(golden['err_ref32_' + name]):.3e}, ratio {err / float(golden['err_ref32_' + name]):.2f}, bar {bar:.3e}")
    assert err <= bar
    assert err <= 5e-5  # the project's mel bar (tests/test_gpu_nat.py) is the outer limit in any case


def test_numpy_input_is_copied_up(mf, golden):
    a = mf(golden["speech"])
    b = mf(torch.from_numpy(golden["speech"]).to(mf.device))
    assert a.is_cuda and torch.equal(a, b)


def test_silence_is_the_floor(mf):
    for y in (np.zeros((2, 4096), np.float32), np.zeros((2, 4096 + 77), np.int16)):
        got = _run(mf, y)
        assert got.shape == (2, 16, 80) and np.all(got == FLOOR32)


def test_ragged_rows_equal_the_rows_alone(mf, golden):
    y, lengths = golden["speech"], golden["lengths"].tolist()
    assert 385 in lengths and max(lengths) == y.shape[1]
    got = _run(mf, y, lengths)
    assert not np.isnan(got).any()
    for b, n in enumerate(lengths):
        alone = _run(mf, y[b : b + 1, :n])[0]
        Tb = oracle.num_frames(n)
        assert alone.shape[0] == Tb == n // 256 or n < 256
        assert np.array_equal(got[b, :Tb], alone), b  # bit for bit: the row is reflected at its own end
        assert np.all(got[b, Tb:] == FLOOR32), b
    # ... and the whole ragged batch against the oracle, at the bar
    want = oracle.log_mel_ragged(y.astype(np.float64), lengths, golden["melfb"])
    e32 = np.abs(oracle.log_mel_ragged(y, lengths, golden["melfb"], dtype=np.float32).astype(np.float64) - want).max()
    valid = np.arange(got.shape[1])[None, :] < np.array([oracle.num_frames(n) for n in lengths])[:, None]
    err = float(np.abs(got.astype(np.float64) - want)[valid].max())
    print(f"\nragged: max|gpu - fp64| = {err:.3e}, err_ref32 = {e32:.3e}, ratio {err / e32:.2f}")
    assert err <= _bar(e32, want)


@pytest.mark.parametrize("pcm", [False, True], ids=["f32", "pcm16"])
def test_rows_behind_the_launch_split_against_the_oracle(mf, golden, pcm):
    """MEL_ROWS_PER_LAUNCH + 3 rows (tests/_row_split.py): the rows behind the split differ from the first rows in content and length and
    hold the longest and the shortest row.  Every row against log_mel_ragged (once per distinct row) at the module's bar, taken over the
    batch as test_ragged_rows_equal_the_rows_alone and test_tile_edges take it: err_ref32 and max |fp64| are the batch's.  Every row behind
    the split and the first ones bit for bit the row alone, FLOOR32 past every row's frames; the output is NaN-filled."""
    bt = RS.frames_batch(_lib.MEL_ROWS_PER_LAUNCH, pcm)
    assert bt.N == _lib.MEL_ROWS_PER_LAUNCH + 3

    def ref(r):
        x = r.content.astype(np.float32) / np.float32(32768.0) if pcm else r.content
        want = oracle.log_mel_ragged(x[None].astype(np.float64), [r.length], golden["melfb"])[0]
        e32 = np.abs(oracle.log_mel_ragged(x[None], [r.length], golden["melfb"], dtype=np.float32)[0].astype(np.float64) - want).max()
        return want, float(e32)

    refs = RS.per_kind(bt, ref)
    got = _run(mf, np.array(bt.rows), bt.lengths)  # (a copy: the shared rows are read-only)
    assert got.shape == (bt.N, oracle.num_frames(max(bt.lengths[bt.P :])), 80) and not np.isnan(got).any()
    bar = _bar(max(e32 for _, e32 in refs), np.concatenate([want for want, _ in refs]))
    worst = {False: 0.0, True: 0.0}
    for b, (n, (want, _)) in enumerate(zip(bt.lengths, refs)):
        Tb = oracle.num_frames(n)
        assert want.shape[0] == Tb
        err = float(np.abs(got[b, :Tb].astype(np.float64) - want).max())
        worst[b >= bt.P] = max(worst[b >= bt.P], err / bar)
        assert err <= bar, (b, err, bar)
        assert np.all(got[b, Tb:] == FLOOR32), b
    for b in list(range(bt.k)) + list(bt.behind()):
        n = bt.lengths[b]
        assert np.array_equal(_run(mf, np.array(bt.rows[b : b + 1, :n]))[0], got[b, : oracle.num_frames(n)]), b
    print(f"\nmel rows across the split ({'pcm16' if pcm else 'f32'}): worst error / bar {worst[False]:.3f} before, {worst[True]:.3f} behind the split")


@pytest.mark.parametrize("pcm", [False, True], ids=["f32", "pcm16"])
def test_unaligned_batch_takes_the_scalar_loads_to_the_same_bits(mf, pcm):
    """Three ragged rows as a view into a flat buffer that starts one element in, at an odd row stride: neither the base nor any row is on
    16 bytes, so the staging takes the scalar loads.  Bit for bit the same rows in an aligned buffer at an aligned stride."""
    bt = RS.frames_batch(_lib.MEL_ROWS_PER_LAUNCH, pcm)
    pick = [0, bt.P, bt.P + 1]  # with a fourth row, the f32 row 3 would sit on 16 bytes again
    y, lengths = bt.rows[pick], [bt.lengths[b] for b in pick]  # (fancy indexing: a copy)
    want = _run(mf, y, lengths)
    assert not np.isnan(want).any()
    N, S = y.shape
    odd = S + 1
    assert S % 8 == 0 and odd % 2 == 1
    flat = torch.full((1 + N * odd,), 0x7FFF if pcm else float("nan"), dtype=torch.int16 if pcm else torch.float32, device=mf.device)
    view = flat[1:].view(N, odd)
    view[:, :S] = torch.from_numpy(np.array(y)).to(mf.device)
    assert view.data_ptr() % 16 != 0 and all((view.data_ptr() + b * odd * view.element_size()) % 16 != 0 for b in range(N))
    out = torch.full(want.shape, float("nan"), dtype=torch.float32, device=mf.device)
    mf._on_stream("forward", ptr(view), _lib.VTTS_MEL_PCM16 if pcm else _lib.VTTS_MEL_F32, N, odd, (C.c_int32 * N)(*lengths), ptr(out), want.shape[1], None)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_an_adopted_blob_gives_the_same_bits(mf, golden):
    """A second filter that binds the first one's tables (cloned) instead of packing its own.  It names its device "cuda", the current
    one, as a caller without an index in hand does."""
    from viettts_amd.nat.dsp import MelFilter

    lengths = [385, 1409]
    y = torch.from_numpy(np.ascontiguousarray(golden["speech"][:2, :1409])).to(mf.device)
    assert y.dtype == torch.float32
    want = mf(y, lengths=lengths)
    other = MelFilter(16000, 1024, 80, 0.0, 8000, device="cuda")
    try:
        assert other.device == mf.device
        other.adopt_packed(mf.packed_blob().clone())
        got = other(y, lengths=lengths)
        torch.cuda.synchronize()
        assert got.shape == (2, oracle.num_frames(1409), 80) and torch.isfinite(got).all()
        assert torch.equal(got, want)
    finally:
        other.close()


def _speechlike(rng, n_rows, S):
    t = np.arange(S) / 16000.0
    y = np.zeros((n_rows, S))
    for b in range(n_rows):
        f0 = rng.uniform(90.0, 250.0)
        x = sum(np.sin(2 * np.pi * f0 * h * t + rng.uniform(0, 2 * np.pi)) / h for h in range(1, 30))
        x *= 0.55 + 0.45 * np.sin(2 * np.pi * 3.0 * t + rng.uniform(0, 2 * np.pi))
        y[b] = 0.2 * x / np.abs(x).max() + rng.normal(0.0, 0.003, size=S)
    return y.astype(np.float32)


def test_tile_edges(mf, golden):
    """Rows of F - 1, F and F + 1 frames (F = frames per workgroup) and one of more than 20 tiles, none a multiple of the hop."""
    frames = [FPB - 1, FPB, FPB + 1, 20 * FPB + 3]
    lengths = [256 * f + r for f, r in zip(frames, (33, 0, 255, 77))]
    y = _speechlike(np.random.default_rng(77), len(lengths), max(lengths))
    got = _run(mf, y, lengths)
    assert got.shape == (4, frames[-1], 80) and not np.isnan(got).any()
    want = oracle.log_mel_ragged(y.astype(np.float64), lengths, golden["melfb"])
    e32 = np.abs(oracle.log_mel_ragged(y, lengths, golden["melfb"], dtype=np.float32).astype(np.float64) - want).max()
    errs = [float(np.abs(got[b, :f].astype(np.float64) - want[b, :f]).max()) for b, f in enumerate(frames)]
    print(f"\ntile edges: max|gpu - fp64| per row {['%.3e' % e for e in errs]}, err_ref32 = {e32:.3e}, ratio {max(errs) / e32:.2f}")
    assert max(errs) <= _bar(e32, want)
    for b, f in enumerate(frames):
        assert np.all(got[b, f:] == FLOOR32)
    # the long row alone, as a full (unragged) batch of one, is the same bits
    alone = _run(mf, y[3:4, : lengths[3]])
    assert np.array_equal(alone[0], got[3])


def test_out_is_checked_like_the_generators(mf, golden):
    y = torch.from_numpy(golden["noise"]).to(mf.device)
    for bad in (
        torch.empty((2, 31, 80), dtype=torch.float32, device=mf.device),  # shape
        torch.empty((2, 32, 80), dtype=torch.float64, device=mf.device),  # dtype
        torch.empty((2, 32, 80), dtype=torch.float32),  # device
        torch.empty((2, 80, 32), dtype=torch.float32, device=mf.device).transpose(1, 2),  # not contiguous
    ):
        with pytest.raises(ValueError):
            mf(y, out=bad)
    with pytest.raises(ValueError):
        mf(y.double())
    with pytest.raises(ValueError):
        mf(y.cpu())
    with pytest.raises(_lib.VttsError):
        mf(y[:, :384].contiguous())  # too short to reflect
    with pytest.raises(_lib.VttsError):
        mf(y, lengths=[8192, 384])


def test_resynthesis_wiring(dev, mf, golden):
    from viettts_amd.hifigan.config import V1
    from viettts_amd.hifigan.generator import Generator
    from viettts_amd.hifigan.synth import synthetic_params
    from viettts_amd.resynth import resynthesize, wav2mel

    gen = Generator(V1, device=dev)
    gen.load_params(synthetic_params(V1, 4321, "scaled"))
    y, lengths = golden["speech"], golden["lengths"].tolist()
    yt = torch.from_numpy(y).to(dev)
    frames = [oracle.num_frames(n) for n in lengths]
    got = resynthesize(yt, gen, lengths=lengths)
    mel = mf(yt, lengths=lengths)
    assert torch.equal(wav2mel(y, lengths), mel)
    want = gen.forward_ragged(mel, frames)
    torch.cuda.synchronize()
    assert got.shape == (4, 256 * max(frames)) and torch.equal(got, want)
    g = got.cpu().numpy()
    for b, f in enumerate(frames):
        assert np.all(g[b, 256 * f :] == 0) and np.abs(g[b, : 256 * f]).max() > 0 and np.isfinite(g[b]).all()
    full = resynthesize(yt, gen)
    assert full.shape == (4, 256 * 64) and torch.equal(full, gen(mf(yt)))
    gen.close()


def test_metric_orders_the_engines(dev):
    """log-mel L1 of the bf16x3 and the bf16 engines' waveforms against the fp32 engine's, one synthetic mel: the split-operand
    engine is the closer one.  The two values are recorded in DESIGN.md; no threshold on them."""
    from viettts_amd.hifigan.config import V1
    from viettts_amd.hifigan.generator import Generator
    from viettts_amd.hifigan.synth import synthetic_mel, synthetic_params
    from viettts_amd.resynth import log_mel_l1

    params = synthetic_params(V1, 4321, "scaled")
    mel = torch.from_numpy(synthetic_mel(2, 128, 7)).to(dev)
    wavs = {}
    for dt in ("f32", "bf16x3", "bf16"):
        g = Generator(V1, device=dev, dtype=dt)
        g.load_params(params)
        wavs[dt] = g(mel).clone()
        torch.cuda.synchronize()
        g.close()
    dx3, d16 = log_mel_l1(wavs["bf16x3"], wavs["f32"]), log_mel_l1(wavs["bf16"], wavs["f32"])
    print(f"\nlog_mel_l1 against the fp32 engine: bf16x3 {dx3:.3e}, bf16 {d16:.3e}")
    assert log_mel_l1(wavs["f32"], wavs["f32"]) == 0.0
    assert dx3 <= d16
    assert log_mel_l1(wavs["bf16"], wavs["f32"], lengths=[128 * 256, 64 * 256 + 5]) > 0
