"""The loudness kernels (viettts_amd/csrc/loudness.hip, include/vtts_loudness.h) on the GPU against the float64 restatement of the contract
(tests/_loudness_oracle.py).  Counts and the sample peak are compared with ==; the loudness figures within a bound the test derives
itself: 4 x the distance of the float32 restatement of the kernel's scheme from float64 over the same rows, at least 1e-3 LU, at most the
0.1 LU of EBU Tech 3341.  Every batch is ragged with junk past each row's end, the outputs are pre-filled with NaN through the C ABI, and
no row is compared before the float64 oracle has shown all its blocks 0.05 LU or more from either gate."""
import ctypes as C

import numpy as np
import pytest
import torch

import _loudness_oracle as O
import _row_split as RS
from viettts_amd import _lib, wavio
from viettts_amd._handle import ptr

pytestmark = pytest.mark.gpu
CASES = [(name, 16000) for name in O.SIGNALS] + [("low", 22050), ("gated", 48000)]
_METERS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    yield torch.device("cuda:0")
    for m in _METERS.values():
        m.close()
    _METERS.clear()


def _meter(rate, dev):
    from viettts_amd.loudness import LoudnessMeter

    if rate not in _METERS:
        _METERS[rate] = LoudnessMeter(rate, device=dev)
        assert np.abs(_METERS[rate].coefficients() - O.coefficients(rate)).max() <= 1e-14
    return _METERS[rate]


@pytest.fixture(scope="module")
def bound():
    b = O.bound(CASES)
    print(f"\nfloat32 restatement within {O.restatement_error(CASES):.2e} LU of float64: the bound is {b:.2e} LU")
    assert O.restatement_error(CASES) <= 0.1  # otherwise the arithmetic is wrong, not the bound
    return b


def _run(m, y, lengths=None, j_extra=2):
    """measure() through the C ABI into NaN-filled outputs and a series of ``j_extra`` blocks more than the longest row has."""
    yt = torch.from_numpy(np.array(y)).to(m.device)  # (a copy: the shared rows are read-only)
    N, S = y.shape
    lens = [S] * N if lengths is None else [int(v) for v in lengths]
    J = max(O.num_blocks(n, m.sample_rate) for n in lens) + j_extra
    need = C.c_size_t(0)
    m._call("workspace_bytes", N, max(lens), C.byref(need))
    ws = torch.full((need.value,), 0xFF, dtype=torch.uint8, device=m.device)  # NaNs: whatever is read unwritten shows
    f = torch.full((3, N), float("nan"), dtype=torch.float32, device=m.device)
    n = torch.full((2, N), -7, dtype=torch.int32, device=m.device)
    mom = torch.full((N, J), float("nan"), dtype=torch.float32, device=m.device)
    lens_c = None if lengths is None else (C.c_int32 * N)(*lens)
    dtype = _lib.VTTS_AUDIO_PCM16 if y.dtype == np.int16 else _lib.VTTS_AUDIO_F32
    m._on_stream("measure", ptr(yt), dtype, N, S, lens_c, ptr(f[0]), ptr(f[1]), ptr(f[2]), ptr(n[0]), ptr(n[1]), ptr(mom), J, ptr(ws), ws.numel())
    torch.cuda.synchronize()
    return f.cpu().numpy(), n.cpu().numpy(), mom.cpu().numpy()


def _bits(f, n, mom):
    return np.concatenate([f.view(np.uint32).T, n.view(np.uint32).T, mom.view(np.uint32)], axis=1)  # [N, 5 + J]


def _got(f, n, mom, b, rate, length) -> O.Loudness:
    J = O.num_blocks(length, rate)
    assert np.all(np.isneginf(mom[b, J:])), (b, mom[b, J:])  # past the row's own blocks
    return O.Loudness(float(f[0, b]), float(f[1, b]), f[2, b], int(n[0, b]), int(n[1, b]), mom[b, :J], np.inf)


@pytest.mark.parametrize("name,rate", CASES)
def test_ragged_batch_agrees_with_the_float64_oracle(dev, bound, name, rate):
    """Row lengths at the first block's edges, at a segment's and a wave's, with a state carry over three segments and one row of about 3 s
    (seven segments at 16 kHz), on inputs that expose a broken carry."""
    rows, lengths = O.batch(name, rate)
    refs, _ = O.batch_reference(name, rate)
    assert rows.shape[1] > max(lengths)
    f, n, mom = _run(_meter(rate, dev), rows, lengths)
    worst = 0.0
    for b, (length, ref) in enumerate(zip(lengths, refs)):
        assert ref.gate_room >= 0.05, (b, length, ref.gate_room)  # the guard: a gate decision is discrete
        got = _got(f, n, mom, b, rate, length)
        assert (got.n_blocks, got.n_gated) == (ref.n_blocks, ref.n_gated), (b, length)
        assert got.sample_peak.view(np.uint32) == ref.sample_peak.view(np.uint32), (b, length)
        d = O.distance(got, ref)
        worst = max(worst, d)
        assert d <= bound, (b, length, d, got.integrated, ref.integrated)
        silent = ~(ref.momentary > O.ABS_GATE)
        assert np.all(got.momentary[silent] <= O.ABS_GATE)
    print(f"\n{name} at {rate} Hz: within {worst:.2e} LU of float64 (bound {bound:.2e})")


@pytest.mark.parametrize("name", O.SIGNALS)
def test_a_row_alone_at_another_stride_and_as_float_gives_the_same_bits(dev, name):
    rows, lengths = O.batch(name)
    m = _meter(16000, dev)
    want = _bits(*_run(m, rows, lengths))
    for b in (1, 6, 7, len(lengths) - 1):  # one block; one sample into the second segment; three segments; the long row
        n = lengths[b]
        alone = _bits(*_run(m, rows[b : b + 1, :n], None))
        J = O.num_blocks(n, 16000) + 2
        assert np.array_equal(alone[0, : 5 + J], want[b, : 5 + J]), (b, n)
    wide = np.full((len(lengths), rows.shape[1] + 1003), rows[0, -1], dtype=rows.dtype)  # another S_stride, odd against every 16-byte line
    wide[:, : rows.shape[1]] = rows
    assert np.array_equal(_bits(*_run(m, wide, lengths)), want)
    if rows.dtype == np.int16:  # the float32 of PCM16 values
        assert np.array_equal(_bits(*_run(m, O.as_float32(rows), lengths)), want)
    else:
        pcm = wavio.float_to_pcm16(rows)
        assert np.array_equal(_bits(*_run(m, pcm, lengths)), _bits(*_run(m, O.as_float32(pcm), lengths)))


def test_more_rows_than_one_launch_takes(dev):
    """The rows' lengths travel as kernel arguments, 128 rows per launch: row 128 + b must be row b."""
    rows, lengths = O.batch("low")
    m = _meter(16000, dev)
    short = [i for i, n in enumerate(lengths) if n <= 2 * O.SEGMENT + 1]
    base = rows[short][:, : 2 * O.SEGMENT + 40]
    reps = -(-131 // len(short))
    y = np.concatenate([base] * reps)[:131]
    lens = ([lengths[i] for i in short] * reps)[:131]
    got = _bits(*_run(m, y, lens))
    want = _bits(*_run(m, base, [lengths[i] for i in short]))
    assert np.array_equal(got, np.concatenate([want] * reps)[:131])


def _normalize(m, y, lengths, out_dtype, packed, **kw):
    out, gains = m.normalize(torch.from_numpy(np.array(y)).to(m.device), lengths, out_dtype=out_dtype, packed=packed, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), gains.cpu().numpy()


@pytest.mark.parametrize("name", ["low", "noise"])
def test_normalize_is_one_multiply_and_to_pcm16s_rule(dev, bound, name):
    rows, lengths = O.batch(name)
    refs, _ = O.batch_reference(name)
    m = _meter(16000, dev)
    x = O.as_float32(rows)
    kw = dict(target=-23.0, ceiling_db=-1.0, max_gain_db=30.0)
    f32, gains = _normalize(m, rows, lengths, "f32", False, **kw)
    pcm, gains2 = _normalize(m, rows, lengths, "pcm16", False, **kw)
    assert np.array_equal(gains.view(np.uint32), gains2.view(np.uint32)) and f32.dtype == np.float32 and pcm.dtype == np.int16
    ratio = 10.0 ** (2.0 * bound / 20.0)
    for b, (n, ref) in enumerate(zip(lengths, refs)):
        want = float(O.gain(ref, **kw))
        assert want / ratio <= float(gains[b]) <= want * ratio, (b, n, gains[b], want)
        prod = x[b, :n] * gains[b]  # one float32 multiply, with the gain the GPU chose
        assert np.array_equal(f32[b, :n].view(np.uint32), prod.view(np.uint32)), (b, n)
        assert np.array_equal(pcm[b, :n], wavio.float_to_pcm16(prod)), (b, n)
        assert not f32[b, n:].any() and not pcm[b, n:].any()  # padding
    for dt, strided in (("f32", f32), ("pcm16", pcm)):
        packed, g = _normalize(m, rows, lengths, dt, True, **kw)
        assert packed.shape == (sum(lengths),) and np.array_equal(g.view(np.uint32), gains.view(np.uint32))
        assert np.array_equal(packed, np.concatenate([strided[b, :n] for b, n in enumerate(lengths)]))


@pytest.fixture(scope="module")
def split():
    """The batch that crosses the rows-per-launch split (tests/_row_split.py) and the float64 oracle of every row, once per distinct row."""
    bt = RS.loudness_batch(_lib.LOUDNESS_ROWS_PER_LAUNCH)
    assert bt.N == _lib.LOUDNESS_ROWS_PER_LAUNCH + 3 and bt.lengths[bt.P - 1] > 0 and 0 < bt.lengths[bt.P] < 4 * 1600
    return bt, RS.per_kind(bt, lambda r: O.measure(r.content[: r.length]))


def test_measure_rows_behind_the_launch_split_against_the_oracle(dev, bound, split):
    """The rows behind the split differ from the first rows in content, level and length and hold the longest row (three blocks, two
    segments: nseg and nhop are the second launch's), the row too short for a block and an empty one.  All five results and the momentary
    series of EVERY row against the float64 oracle, as the ragged test above does; outputs and workspace pre-filled."""
    bt, refs = split
    f, n, mom = _run(_meter(16000, dev), bt.rows, bt.lengths)
    assert mom.shape[1] == O.num_blocks(max(bt.lengths[bt.P :]), 16000) + 2 == 3 + 2
    worst = {False: 0.0, True: 0.0}
    for b, (length, ref) in enumerate(zip(bt.lengths, refs)):
        assert ref.gate_room >= 0.05, (b, length, ref.gate_room)
        got = _got(f, n, mom, b, 16000, length)
        assert (got.n_blocks, got.n_gated) == (ref.n_blocks, ref.n_gated), (b, length)
        assert got.sample_peak.view(np.uint32) == ref.sample_peak.view(np.uint32), (b, length)
        d = O.distance(got, ref)
        worst[b >= bt.P] = max(worst[b >= bt.P], d / bound)
        assert d <= bound, (b, length, d, got.integrated, ref.integrated)
    print(f"\nloudness rows across the split: worst distance / bound {worst[False]:.3f} before, {worst[True]:.3f} behind the split (bound {bound:.2e} LU)")


def _normalize_prefilled(m, y, lengths, out_dtype, packed):
    """normalize() through the C ABI into samples pre-filled with NaN (f32) or 12345 (PCM16) and NaN gains; a packed output carries eight
    spare elements, which must keep the fill."""
    yt = torch.from_numpy(np.array(y)).to(m.device)
    N, S = yt.shape
    r = m(yt, lengths)
    tdt, odt, fill = (torch.int16, _lib.VTTS_AUDIO_PCM16, 12345) if out_dtype == "pcm16" else (torch.float32, _lib.VTTS_AUDIO_F32, float("nan"))
    out = torch.full((sum(lengths) + 8,) if packed else (N, S), fill, dtype=tdt, device=m.device)
    gains = torch.full((N,), float("nan"), dtype=torch.float32, device=m.device)
    m._on_stream("normalize", ptr(yt), _lib.VTTS_AUDIO_F32, N, S, (C.c_int32 * N)(*lengths), ptr(r.integrated), ptr(r.sample_peak), -23.0, -1.0, 30.0,
                 ptr(out), odt, 0 if packed else S, ptr(gains))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    if packed:
        assert np.all(out[-8:] == 12345) if out_dtype == "pcm16" else np.isnan(out[-8:]).all()
        out = out[:-8]
    return out, gains.cpu().numpy()


def test_normalize_rows_behind_the_launch_split(dev, bound, split):
    """The same batch into strided f32, packed f32 and packed PCM16.  Row P - 1 is not empty and row P is the row too short for a block (gain
    exactly 1), so the packed offset of row P is the running sum over the whole first launch; the rows behind the split have gains of their
    own.  Every row: the oracle's gain within the bound, one float32 multiply, to_pcm16's rule, zeros past its samples."""
    bt, refs = split
    m = _meter(16000, dev)
    x = bt.rows
    f32, gains = _normalize_prefilled(m, x, bt.lengths, "f32", False)
    ratio = 10.0 ** (2.0 * bound / 20.0)
    assert gains[bt.P] == 1.0 and len({float(gains[b]) for b in list(range(bt.k)) + list(bt.behind())}) == 2 * bt.k - 1  # (the empty row's gain is 1 as well)
    for b, (n, ref) in enumerate(zip(bt.lengths, refs)):
        want = float(O.gain(ref))
        assert want / ratio <= float(gains[b]) <= want * ratio, (b, n, gains[b], want)
        prod = x[b, :n] * gains[b]
        assert np.array_equal(f32[b, :n].view(np.uint32), prod.view(np.uint32)), (b, n)
        assert not f32[b, n:].any(), b
    flat = np.concatenate([f32[b, :n] for b, n in enumerate(bt.lengths)])
    packed, g = _normalize_prefilled(m, x, bt.lengths, "f32", True)
    assert np.array_equal(g.view(np.uint32), gains.view(np.uint32)) and np.array_equal(packed.view(np.uint32), flat.view(np.uint32))
    pcm, g = _normalize_prefilled(m, x, bt.lengths, "pcm16", True)
    assert pcm.dtype == np.int16 and np.array_equal(g.view(np.uint32), gains.view(np.uint32)) and np.array_equal(pcm, wavio.float_to_pcm16(flat))


def test_each_cap_binds_and_a_gain_of_one_is_to_pcm16(dev, bound):
    """Rows made for the target, for max_gain_db, for the ceiling, one without a loudness (gain exactly 1) and one that clips."""
    m = _meter(16000, dev)
    n = 16000
    click = O.tone(440.0, 0.01, n, 16000).astype(np.float32)
    click[::1600] += 0.9
    rng = np.random.default_rng(3)
    rows = np.stack([O.tone(440.0, 0.05, n, 16000).astype(np.float32), O.tone(440.0, 1e-3, n, 16000).astype(np.float32), click,
                     (rng.uniform(-1.2, 1.2, n)).astype(np.float32), np.zeros(n, np.float32)])
    lengths = [n, n, n, 4 * 1600 - 1, n]  # row 3: too short for a block, and beyond [-1, 1]
    refs = [O.measure(rows[b, :k]) for b, k in enumerate(lengths)]
    assert all(r.gate_room >= 0.05 for r in refs)
    pcm, gains = _normalize(m, rows, lengths, "pcm16", False)
    want = [O.gain(r) for r in refs]
    ratio = 10.0 ** (2.0 * bound / 20.0)
    assert want[0] / ratio <= gains[0] <= want[0] * ratio and 1.0 < gains[0] < 10.0
    ulps = 2.0 ** -22  # the caps do not depend on the loudness: the device's pow against numpy's, rounded to float32
    assert want[1] == np.float32(10.0 ** 1.5) and abs(gains[1] / want[1] - 1.0) <= ulps
    assert want[2] == np.float32(10.0 ** (-1.0 / 20.0) / np.float64(refs[2].sample_peak)) and abs(gains[2] / want[2] - 1.0) <= ulps and gains[2] < 1.0
    assert gains[3] == 1.0 and gains[4] == 1.0
    assert np.array_equal(pcm[3, : lengths[3]], wavio.float_to_pcm16(rows[3, : lengths[3]])) and np.abs(pcm[3]).max() == 32767
    assert not pcm[3, lengths[3] :].any() and not pcm[4].any()
    for b in range(3):
        assert np.array_equal(pcm[b], wavio.float_to_pcm16(rows[b] * gains[b]))
    assert abs(int(np.abs(pcm[2]).max()) - 29204) <= 1  # the loudest sample sits at the -1 dBFS ceiling: 32767 * 10^(-1 / 20)


def test_public_call_returns_device_tensors_and_the_series(dev, bound):
    rows, lengths = O.batch("gated")
    refs, _ = O.batch_reference("gated")
    m = _meter(16000, dev)
    rows = np.array(rows)  # (a copy: the shared rows are read-only)
    r = m(rows, lengths, series=True)
    assert all(t.device == dev for t in (r.integrated, r.momentary_max, r.sample_peak, r.n_blocks, r.n_gated, r.momentary))
    assert r.momentary.shape == (len(lengths), max(x.n_blocks for x in refs)) and m(rows, lengths).momentary is None
    b = len(lengths) - 1
    assert refs[b].gate_room >= 0.05
    assert abs(float(r.integrated[b]) - refs[b].integrated) <= bound and (int(r.n_blocks[b]), int(r.n_gated[b])) == (28, 15)
    one = m(rows[b, : lengths[b]])  # [S]
    assert one.integrated.shape == (1,) and float(one.integrated[0]) == float(r.integrated[b])
    from viettts_amd.loudness import default_meter

    assert default_meter(dev, 16000) is default_meter("cuda:0", 16000) and default_meter(dev, 48000) is not default_meter(dev, 16000)


def test_pipeline_loudness_is_off_by_default_and_reaches_the_target(dev, bound):
    """Three sentences of the synthetic models the pipeline tests use.  ``loudness=None`` is the call without the argument, bit for bit;
    with ``loudness=-23`` every sentence, metered by the float64 oracle on the returned samples, is at the target, or its gain sits at the
    sample-peak ceiling or at max_gain_db (or it has no loudness at all and is returned as it was: the contract's gain of 1)."""
    from viettts_amd.hifigan.config import V1
    from viettts_amd.hifigan.generator import Generator
    from viettts_amd.hifigan.synth import synthetic_params
    from viettts_amd.nat.acoustic import AcousticModel
    from viettts_amd.nat.config import FLAGS
    from viettts_amd.nat.duration import DurationModel
    from viettts_amd.nat.synth import synthetic_acoustic_checkpoint, synthetic_duration_checkpoint
    from viettts_amd.pipeline import synthesize_sentences

    dm, am = DurationModel(device="cuda:0"), AcousticModel(device="cuda:0")
    dm.load_params(*synthetic_duration_checkpoint())
    am.load_params(*synthetic_acoustic_checkpoint())
    gen = Generator(V1, device="cuda:0", dtype="bf16")
    gen.load_params(synthetic_params(V1, 4321, "scaled"))
    try:
        rng = np.random.default_rng(41)
        sents = [[FLAGS.sil_index] + list(rng.integers(4, 90, size=n)) + [FLAGS.sil_index] for n in (24, 40, 33)]
        base = synthesize_sentences(sents, dm, am, gen, silence_duration=0.05)
        base = {i: base[i].copy() for i in base}
        off = synthesize_sentences(sents, dm, am, gen, silence_duration=0.05, loudness=None)
        assert sorted(off) == [0, 1, 2] and all(np.array_equal(off[i].view(np.uint32), base[i].view(np.uint32)) for i in base)
        on = synthesize_sentences(sents, dm, am, gen, silence_duration=0.05, loudness=-23.0)
        pcm = synthesize_sentences(sents, dm, am, gen, silence_duration=0.05, loudness=-23.0, out_dtype="pcm16")
        reached = 0
        for i in range(3):
            assert on[i].dtype == np.float32 and on[i].shape == base[i].shape
            assert np.array_equal(pcm[i], wavio.float_to_pcm16(on[i])), i
            before, after = O.measure(base[i]), O.measure(on[i])
            print(f"\nsentence {i}: {len(base[i])} samples, {before.integrated:.2f} LUFS -> {after.integrated:.2f} LUFS, peak {float(after.sample_peak):.4f}")
            assert before.gate_room >= 0.05 and after.gate_room >= 0.05, i
            if not np.isfinite(before.integrated):
                assert np.array_equal(on[i], base[i]), i
                continue
            reached += 1
            at_target = abs(after.integrated - (-23.0)) <= bound
            at_ceiling = abs(float(after.sample_peak) / 10.0 ** (-1.0 / 20.0) - 1.0) <= 1e-6
            at_max_gain = np.array_equal(on[i], base[i] * np.float32(10.0 ** 1.5))
            assert at_target or at_ceiling or at_max_gain, (i, after.integrated, float(after.sample_peak))
        assert reached >= 1
    finally:
        gen.close()
        dm.close()
        am.close()


def test_score_segments_gains_the_loudness_keys_only_with_a_meter(dev, bound):
    from viettts_amd import vocoder_eval
    from viettts_amd.hifigan.config import V1
    from viettts_amd.hifigan.disc_synth import synthetic_disc_checkpoint
    from viettts_amd.hifigan.discriminators import Discriminators, fold_checkpoint
    from viettts_amd.hifigan.generator import Generator
    from viettts_amd.hifigan.synth import synthetic_params

    gen = Generator(V1, device=dev)
    gen.load_params(synthetic_params(V1, 4321, "scaled"))
    disc = Discriminators(dev).load_params(fold_checkpoint(synthetic_disc_checkpoint(8642)))
    try:
        x = O.signal("low", 2 * 8192)
        y = torch.from_numpy(np.stack([x[:8192], x[8192:]])).to(dev)
        plain = vocoder_eval.score_segments(y, gen, disc)
        assert set(plain) == {"adv", "fm", "mel", "total", "disc"}
        scored = vocoder_eval.score_segments(y, gen, disc, meter=_meter(16000, dev))
        assert set(scored) == set(plain) | set(vocoder_eval.LOUDNESS_KEYS)
        assert all(scored[k] == pytest.approx(plain[k], rel=1e-6) for k in plain)  # the existing figures are what they were
        ref = O.measure(x)  # the pass's segments end to end
        assert ref.gate_room >= 0.05 and abs(scored["lufs_y"] - ref.integrated) <= bound
        assert np.isfinite(scored["lufs_y_hat"])
    finally:
        gen.close()
        disc.close()


@pytest.mark.parametrize("rate", [16000, 22050])
def test_command_line(dev, tmp_path, capsys, rate, bound):
    """``python -m viettts_amd.loudness``: a file is metered at its own rate and written at the target."""
    from viettts_amd import loudness

    x = wavio.float_to_pcm16(O.tone(440.0, 0.05, 2 * rate, rate))
    src, dst = tmp_path / "in.wav", tmp_path / "out.wav"
    wavio.write_wav_pcm16(src, x, rate)
    loudness.main(["--wav", str(src), "--target", "-20", "--output", str(dst)])
    out = capsys.readouterr().out
    ref = O.measure(x, rate)
    import re

    printed = float(re.search(r"integrated (-?[0-9.]+) LUFS", out).group(1))
    assert abs(printed - ref.integrated) <= bound + 0.005  # (two decimals are printed)
    assert "momentary max" in out and "sample peak -26.0" in out and "gain +" in out and "to -20.0 LUFS" in out
    sr, y = wavio.read_wav(dst)
    assert sr == rate and y.dtype == np.int16 and y.shape == x.shape
    after = O.measure(y, rate)
    assert ref.gate_room >= 0.05 and after.gate_room >= 0.05
    assert abs(after.integrated - (-20.0)) <= bound  # (the PCM16 rounding adds 8e-11 of noise power to 1.2e-2 of signal: nothing)
    with pytest.raises(SystemExit):
        loudness.main(["--wav", str(src), "--output", str(dst)])
