"""The intelligibility kernels (viettts_amd/csrc/stoi.hip, include/vtts_stoi.h) on the GPU against the float64 restatement of the contract
(tests/_stoi_oracle.py).  Counts and the keep mask are compared with ==; band magnitudes (relative to the row's largest), per-segment values and
the two figures within bounds the test derives itself: 8 x the distance of the oracle's float32 mode from its float64 mode over the same rows,
never above 1e-5 (tests/test_stoi_cpu.py holds both).  Every batch is ragged with junk past each row's end; the accuracy tests go through the C
ABI into NaN-filled outputs and a workspace of 0xFF bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

import _row_split as RS
import _stoi_oracle as O
from viettts_amd import _lib
from viettts_amd._handle import ptr

pytestmark = pytest.mark.gpu
_METER = []


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    yield torch.device("cuda:0")
    for m in _METER:
        m.close()
    _METER.clear()


@pytest.fixture(scope="module")
def meter(dev):
    from viettts_amd.stoi import StoiMeter

    if not _METER:
        _METER.append(StoiMeter(device=dev))
        assert np.array_equal(_METER[0].window().view(np.uint32), O.window().view(np.uint32))
    return _METER[0]


@pytest.fixture(scope="module")
def bounds():
    b = O.bounds()
    print(f"\nfloat32 restatement within {b.scale_mags:.2e} / {b.scale_series:.2e} / {b.scale_mean:.2e} of float64 (band magnitudes / segments / figures): "
          f"bounds {b.mags:.2e} / {b.series:.2e} / {b.mean:.2e}")
    assert max(b.series, b.mean) <= O.BOUND_CAP
    return b


def _batch(pairs, pad=37, seed=5):
    """Rows of different lengths as one [N, S] pair with junk past each row's own end."""
    lengths = [len(x) for x, _ in pairs]
    S = max(lengths) + pad
    rng = np.random.default_rng(seed)
    dt = pairs[0][0].dtype
    junk = (lambda: rng.integers(-30000, 30000, S).astype(np.int16)) if dt == np.int16 else (lambda: rng.uniform(-1, 1, S).astype(np.float32))
    xs, ys = np.stack([junk() for _ in pairs]), np.stack([junk() for _ in pairs])
    for b, (x, y) in enumerate(pairs):
        xs[b, : len(x)], ys[b, : len(y)] = x, y
    return xs, ys, lengths


class Got:
    pass


def _run(m, xs, ys, lengths=None, extra=2):
    """forward() through the C ABI into NaN-filled outputs, series and band magnitudes ``extra`` columns wider than the longest row needs."""
    xt, yt = torch.from_numpy(np.array(xs)).to(m.device), torch.from_numpy(np.array(ys)).to(m.device)
    N, S = xs.shape
    lens = [S] * N if lengths is None else [int(v) for v in lengths]
    K = O.num_frames(max(lens))
    T, M = max(0, K - 1) + extra, max(0, K - O.SEG) + extra
    need = C.c_size_t(0)
    m._call("workspace_bytes", N, max(lens), C.byref(need))
    ws = torch.full((need.value,), 0xFF, dtype=torch.uint8, device=m.device)  # NaNs and -1s: whatever is read unwritten shows
    f = torch.full((2, N), 7.0, dtype=torch.float32, device=m.device)
    n = torch.full((3, N), -7, dtype=torch.int32, device=m.device)
    ser = torch.full((2, N, M), 7.0, dtype=torch.float32, device=m.device)
    mags = torch.full((N, 2, O.BANDS, T), float("nan"), dtype=torch.float32, device=m.device)
    lens_c = None if lengths is None else (C.c_int32 * N)(*lens)
    dtype = _lib.VTTS_AUDIO_PCM16 if xs.dtype == np.int16 else _lib.VTTS_AUDIO_F32
    m._on_stream("forward", ptr(xt), ptr(yt), dtype, N, S, lens_c, ptr(f[0]), ptr(f[1]), ptr(n[0]), ptr(n[1]), ptr(n[2]), ptr(ser[0]), ptr(ser[1]), M,
                 ptr(mags), T, ptr(ws), ws.numel())
    torch.cuda.synchronize()
    g = Got()
    g.f, g.n, g.ser, g.mags = f.cpu().numpy(), n.cpu().numpy(), ser.cpu().numpy(), mags.cpu().numpy()
    g.kept = ws[: 4 * N * K].view(torch.int32).view(N, K).cpu().numpy()  # the header's layout: the kept lists lead the workspace
    g.energy = ws[(4 * N * K + 7) // 8 * 8 :][: 8 * N * K].view(torch.float64).view(N, K).cpu().numpy()
    return g


def _bits(g):
    N = g.f.shape[1]
    return np.concatenate([g.f.view(np.uint32).T, g.n.view(np.uint32).T, g.ser.view(np.uint32).transpose(1, 0, 2).reshape(N, -1),
                           g.mags.view(np.uint32).reshape(N, -1)], axis=1)


def _compare(g, b, ref: O.Stoi, bounds, worst):
    """Row ``b`` of ``g`` against ``ref``: counts, keep mask and energies with ==, the rest within the bounds; ``worst`` collects the errors."""
    K, Kk, M = ref.n_frames, ref.n_kept, ref.n_segments
    T = max(0, Kk - 1)
    assert tuple(g.n[:, b]) == (K, Kk, M), (b, g.n[:, b], (K, Kk, M))
    assert np.array_equal(g.kept[b, :Kk], ref.kept) and np.all(g.kept[b, Kk:] == -1), b
    assert np.array_equal(g.energy[b, :K].view(np.uint64), ref.energy.view(np.uint64)), b
    assert np.all(np.isnan(g.ser[:, b, M:])) and not np.any(np.isnan(g.ser[:, b, :M])), b
    assert np.all(np.isnan(g.mags[b, :, :, T:])), b  # nothing is written past the row's own frames
    if T:
        e = float(np.abs(g.mags[b, :, :, :T].astype(np.float64) - ref.mags).max() / ref.mags.max())
        worst["mags"] = max(worst.get("mags", 0.0), e)
        assert e <= bounds.mags, (b, e)
    if M:
        e = max(float(np.abs(g.ser[0, b, :M] - ref.stoi_series).max()), float(np.abs(g.ser[1, b, :M] - ref.estoi_series).max()))
        worst["series"] = max(worst.get("series", 0.0), e)
        assert e <= bounds.series, (b, e)
        e = max(abs(float(g.f[0, b]) - ref.stoi), abs(float(g.f[1, b]) - ref.estoi))
        worst["mean"] = max(worst.get("mean", 0.0), e)
        assert e <= bounds.mean, (b, e, float(g.f[0, b]), ref.stoi, float(g.f[1, b]), ref.estoi)
    else:
        assert np.isnan(g.f[0, b]) and np.isnan(g.f[1, b]), (b, g.f[:, b])


def _report(what, worst, bounds):
    print(f"\n{what}: kernel within " + "  ".join(f"{k} {v:.2e} (bound {getattr(bounds, k):.2e})" for k, v in worst.items()) + " of float64")


def test_ragged_batch_agrees_with_the_float64_oracle(meter, bounds):
    """Six speech-like rows of 4 700 .. 20 000 samples at two noise levels, each with a stretch 60 dB down: drops at the first frame (row 1),
    at the last (row 3) and across a workgroup's boundary of both framed kernels (row 4)."""
    n = len(O.CASES)
    refs = [O.case_reference(i)[0] for i in range(n)]
    dropped = [np.setdiff1d(np.arange(r.n_frames), r.kept) for r in refs]
    assert all(len(d) for d in dropped) and dropped[1][0] == 0 and dropped[3][-1] == refs[3].n_frames - 1
    assert dropped[4][0] % O.FPB > dropped[4][-1] % O.FPB and dropped[4][0] // O.FPB + 1 == dropped[4][-1] // O.FPB  # on both sides of one boundary
    xs, ys, lengths = _batch([O.case(i) for i in range(n)])
    g = _run(meter, xs, ys, lengths)
    worst = {}
    for b, ref in enumerate(refs):
        _compare(g, b, ref, bounds, worst)
    _report("six rows", worst, bounds)


def test_one_long_row_spans_many_workgroups(meter, bounds):
    """300 000 samples: 2 342 candidate frames over 293 workgroups, 2 109 kept; beside a short row, so that its tiles past the short row's end run."""
    i = len(O.CASES)
    xs, ys, lengths = _batch([O.case(i), O.case(0)])
    g = _run(meter, xs, ys, lengths)
    worst = {}
    ref = O.case_reference(i)[0]
    assert ref.n_frames > 2000 and ref.n_kept < ref.n_frames
    _compare(g, 0, ref, bounds, worst)
    _compare(g, 1, O.case_reference(0)[0], bounds, worst)
    _report("long row", worst, bounds)


def _plain(S, seed=11):
    x = O.make_speechlike(max(S, 1), seed)[:S]
    return x, O.degrade(x, seed, 0.5) if S else x


def test_length_edges_and_tile_edges(meter, bounds):
    """The counts' edges (0, 256, 257; 4096 -> K = 30, no segment; 4097 -> one; 4224, 4225) and T = K - 1 at the frames per workgroup and at
    five times it, each - 1, + 0, + 1."""
    lens = [0, 256, 257, 4096, 4097, 4224, 4225]
    for T in (O.FPB - 1, O.FPB, O.FPB + 1, 5 * O.FPB - 1, 5 * O.FPB, 5 * O.FPB + 1):
        lens.append(O.FRAME + O.HOP * (T + 1))  # K = T + 1 exactly
    pairs = [_plain(S) for S in lens]
    refs = [O.measure(x, y) for x, y in pairs]
    assert [r.n_kept - 1 for r in refs[7:]] == [7, 8, 9, 39, 40, 41] and [r.n_segments for r in refs[:7]] == [0, 0, 0, 0, 1, 1, 2]
    xs, ys, lengths = _batch(pairs)
    g = _run(meter, xs, ys, lengths)
    worst = {}
    for b, ref in enumerate(refs):
        _compare(g, b, ref, bounds, worst)
    _report("edges", worst, bounds)


def test_rows_without_a_segment_give_nan(meter, bounds):
    """35 candidate frames of which 30 are kept (T = 29: one frame short of a segment), an all-zero row, and a zero clean row with a loud y."""
    S, seed, level, quiet = O.T29
    x = O.make_speechlike(S, seed, quiet=quiet)
    y = O.degrade(x, seed, level)
    ref = O.measure(x, y)
    assert ref.n_frames >= 31 and ref.n_kept == 30 and ref.n_segments == 0
    z = np.zeros(S, np.float32)
    xs, ys, lengths = _batch([(x, y), (z, z), (z, y)])
    g = _run(meter, xs, ys, lengths)
    _compare(g, 0, ref, bounds, {})
    for b in (1, 2):
        assert tuple(g.n[:, b]) == (ref.n_frames, 0, 0) and np.isnan(g.f[0, b]) and np.isnan(g.f[1, b]) and np.all(g.kept[b] == -1)
        assert np.all(np.isnan(g.ser[:, b]))


def test_a_row_alone_equals_the_row_in_a_ragged_batch_bit_for_bit(meter):
    pairs = [O.case(i) for i in (2, 0, 4, 1, 3)]
    xs, ys, lengths = _batch(pairs, pad=517)
    g = _run(meter, xs, ys, lengths)
    for b in (0, 2, 4):
        x, y = pairs[b]
        a = _run(meter, x[None, :], y[None, :], None)  # alone, at its own stride, without lengths
        K, Kk = int(a.n[0, 0]), int(a.n[1, 0])
        T, M = max(0, Kk - 1), int(a.n[2, 0])
        assert np.array_equal(a.f.view(np.uint32)[:, 0], g.f.view(np.uint32)[:, b]) and np.array_equal(a.n[:, 0], g.n[:, b])
        assert np.array_equal(a.ser.view(np.uint32)[:, 0, :M], g.ser.view(np.uint32)[:, b, :M])
        assert np.array_equal(a.mags.view(np.uint32)[0, :, :, :T], g.mags.view(np.uint32)[b, :, :, :T])
        assert np.array_equal(a.kept[0, :K], g.kept[b, :K]) and np.array_equal(a.energy.view(np.uint64)[0, :K], g.energy.view(np.uint64)[b, :K])


def test_rows_behind_the_launch_split_against_the_oracle(meter, bounds):
    """STOI_ROWS_PER_LAUNCH + 3 rows (tests/_row_split.py): the rows behind the split differ from the first rows in both signals and in
    length, and hold the longest row (kmax, mmax and the strides of the four workspace slices are the second launch's), a row one sample
    short of a segment and an empty one.  Both figures, the three counts, the keep list, the energies, both series and the band magnitudes of
    EVERY row against the float64 oracle (once per distinct row), all requested in the one call; each row behind the split is the row alone."""
    bt = RS.stoi_batch(_lib.STOI_ROWS_PER_LAUNCH)
    assert bt.N == _lib.STOI_ROWS_PER_LAUNCH + 3
    xs, ys = np.ascontiguousarray(bt.rows[:, :, 0]), np.ascontiguousarray(bt.rows[:, :, 1])
    refs = RS.per_kind(bt, lambda r: O.measure(r.content[: r.length, 0], r.content[: r.length, 1]))
    assert [refs[b].n_segments > 0 for b in bt.behind()] == [False, True, False] and refs[bt.P + 1].n_frames == max(r.n_frames for r in refs)
    g = _run(meter, xs, ys, bt.lengths)
    before, behind = {}, {}
    for b, ref in enumerate(refs):
        _compare(g, b, ref, bounds, behind if b >= bt.P else before)
    _report("rows before the split", before, bounds)
    _report("rows behind the split", behind, bounds)
    print("worst error / bound behind the split: " + "  ".join(f"{k} {v / getattr(bounds, k):.3f}" for k, v in behind.items()))
    for b in bt.behind():
        n = bt.lengths[b]
        if n == 0:
            continue  # (a call needs a sample; the empty row is compared with the oracle above)
        a = _run(meter, xs[b : b + 1, :n], ys[b : b + 1, :n], None)
        K, Kk = int(a.n[0, 0]), int(a.n[1, 0])
        T, M = max(0, Kk - 1), int(a.n[2, 0])
        assert np.array_equal(a.f.view(np.uint32)[:, 0], g.f.view(np.uint32)[:, b]) and np.array_equal(a.n[:, 0], g.n[:, b]), b
        assert np.array_equal(a.ser.view(np.uint32)[:, 0, :M], g.ser.view(np.uint32)[:, b, :M]), b
        assert np.array_equal(a.mags.view(np.uint32)[0, :, :, :T], g.mags.view(np.uint32)[b, :, :, :T]), b
        assert np.array_equal(a.kept[0, :K], g.kept[b, :K]) and np.array_equal(a.energy.view(np.uint64)[0, :K], g.energy.view(np.uint64)[b, :K]), b


def test_float32_input_equals_pcm16_input_bit_for_bit(meter, bounds):
    pairs16 = []
    for i in (1, 2):
        x, y = O.case(i)
        pairs16.append((np.rint(x * 32767.0).astype(np.int16), np.rint(np.clip(y, -1, 1) * 32767.0).astype(np.int16)))
    pairs32 = [(O.as_float32(x), O.as_float32(y)) for x, y in pairs16]
    a = _run(meter, *_batch(pairs16))
    b = _run(meter, *_batch(pairs32))
    for r in range(2):
        K, Kk, M = (int(v) for v in a.n[:, r])
        assert M > 0 and np.array_equal(a.n[:, r], b.n[:, r]) and np.array_equal(a.f.view(np.uint32)[:, r], b.f.view(np.uint32)[:, r])
        assert np.array_equal(a.ser.view(np.uint32)[:, r, :M], b.ser.view(np.uint32)[:, r, :M])
        assert np.array_equal(a.mags.view(np.uint32)[r, :, :, : Kk - 1], b.mags.view(np.uint32)[r, :, :, : Kk - 1])
        assert np.array_equal(a.kept[r], b.kept[r])
    _compare(a, 0, O.measure(*pairs16[0]), bounds, {})  # ... and the oracle reads PCM16 the same way


def test_scaling_the_processed_row_changes_neither_figure(meter, bounds):
    """x and y are transformed apart, so y's error does not scale with x: y 40 dB down keeps both figures within the bound."""
    pairs = [O.case(i) for i in (1, 2, 5)]
    small = [(x, (np.float32(0.01) * y).astype(np.float32)) for x, y in pairs]
    a, b = _run(meter, *_batch(pairs)), _run(meter, *_batch(small))
    worst = {}
    for r, i in enumerate((1, 2, 5)):
        d = max(abs(float(a.f[0, r]) - float(b.f[0, r])), abs(float(a.f[1, r]) - float(b.f[1, r])))
        print(f"\nrow {i}: y -> 0.01 y moves the figures by {d:.2e} (bound {bounds.mean:.2e})")
        assert d <= bounds.mean
        _compare(b, r, O.measure(*small[r]), bounds, worst)
    _report("y 40 dB down", worst, bounds)


def test_python_meter_returns_what_the_c_abi_wrote(meter, bounds):
    pairs = [O.case(i) for i in (0, 3)]
    xs, ys, lengths = _batch(pairs)
    g = _run(meter, xs, ys, lengths, extra=0)
    xt, yt = torch.from_numpy(xs).to(meter.device), torch.from_numpy(ys).to(meter.device)
    r = meter(xt, yt, lengths, series=True)
    assert r.stoi_series.shape == (2, O.num_frames(max(lengths)) - O.SEG)
    for got, want in ((r.stoi, g.f[0]), (r.estoi, g.f[1]), (r.stoi_series, g.ser[0]), (r.estoi_series, g.ser[1])):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    for got, want in ((r.n_frames, g.n[0]), (r.n_kept, g.n[1]), (r.n_segments, g.n[2]), (meter.kept_frames(), g.kept)):
        assert np.array_equal(got.cpu().numpy(), want)
    plain = meter(xs, ys, lengths)  # numpy in, no series
    assert plain.stoi_series is None and torch.equal(plain.stoi, r.stoi) and torch.equal(plain.estoi, r.estoi)
    one, mg = meter(xt[0, : lengths[0]].contiguous(), yt[0, : lengths[0]].contiguous(), mags=True)  # one row, 1-D
    assert torch.equal(one.stoi, r.stoi[:1]) and mg.shape == (1, 2, O.BANDS, O.num_frames(lengths[0]) - 1)
    mixed = meter(np.rint(xs * 32767.0).astype(np.int16), O.as_float32(np.rint(np.clip(ys, -1, 1) * 32767.0).astype(np.int16)), lengths)  # PCM16 against float32
    assert np.isfinite(mixed.stoi.cpu().numpy()).all()
    with pytest.raises(ValueError):
        meter(xt, yt[:, :-1].contiguous(), lengths)
    with pytest.raises(_lib.VttsError):
        meter(xt, yt, [lengths[0], xs.shape[1] + 1])


def test_wav_stoi_at_16_khz_is_the_meter_on_the_resamplers_output(meter, dev):
    from viettts_amd.audio import resampler
    from viettts_amd.stoi import default_stoi_meter, format_result, wav_stoi

    pairs = [_plain(16000, 31), _plain(12345, 32)]
    xs, ys, lengths = _batch(pairs)
    xt, yt = torch.from_numpy(xs).to(dev), torch.from_numpy(ys).to(dev)
    got = wav_stoi(xt, yt, lengths, rate=16000, series=True)
    rs = resampler(16000, 10000, dev)
    assert (rs.L, rs.M) == (5, 8)
    want = meter(rs(xt, lengths=lengths), rs(yt, lengths=lengths), rs.out_lengths(lengths), series=True)
    for a, b in zip(got, want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert int(got.n_segments[0]) == O.num_frames(rs.out_samples(16000)) - O.SEG > 0 and float(got.stoi[0]) > float(got.estoi[0]) > 0.0
    same = wav_stoi(xt, yt, lengths, rate=10000)  # already at 10 kHz: nothing is converted
    ref = meter(xt, yt, lengths)
    assert torch.equal(same.stoi.view(torch.int32), ref.stoi.view(torch.int32))
    assert default_stoi_meter("cuda") is default_stoi_meter(dev) and format_result(got).startswith("STOI 0.")


def test_score_segments_gains_the_stoi_keys_only_with_a_stoi_meter(meter, dev):
    from viettts_amd import vocoder_eval
    from viettts_amd.audio import resampler
    from viettts_amd.hifigan.config import V1
    from viettts_amd.hifigan.disc_synth import synthetic_disc_checkpoint
    from viettts_amd.hifigan.discriminators import Discriminators, fold_checkpoint
    from viettts_amd.hifigan.generator import Generator
    from viettts_amd.hifigan.synth import synthetic_params

    gen = Generator(V1, device=dev)
    gen.load_params(synthetic_params(V1, 4321, "scaled"))
    disc = Discriminators(dev).load_params(fold_checkpoint(synthetic_disc_checkpoint(8642)))
    try:
        x = _plain(2 * 8192, 41)[0]
        y = torch.from_numpy(np.stack([x[:8192], x[8192:]])).to(dev)
        plain = vocoder_eval.score_segments(y, gen, disc)
        assert set(plain) == {"adv", "fm", "mel", "total", "disc"}
        scored = vocoder_eval.score_segments(y, gen, disc, stoi_meter=meter)
        assert set(scored) == set(plain) | set(vocoder_eval.STOI_KEYS)
        assert all(scored[k] == pytest.approx(plain[k], rel=1e-6) for k in plain)  # the existing figures are what they were
        assert -1.0 <= scored["estoi"] <= 1.0 and -1.0 <= scored["stoi"] <= 1.0
        rs = resampler(16000, 10000, dev)  # the clean side is the pass's segments end to end at 10 kHz
        assert int(meter(rs(y.reshape(1, -1)), rs(y.reshape(1, -1))).n_frames[0]) == O.num_frames(rs.out_samples(2 * 8192))
        short = vocoder_eval.score_segments(y[:1, :2048].contiguous(), gen, disc, stoi_meter=meter)  # 1 280 samples at 10 kHz: 8 frames
        assert short["stoi"] != short["stoi"] and short["estoi"] != short["estoi"]
    finally:
        gen.close()
        disc.close()
