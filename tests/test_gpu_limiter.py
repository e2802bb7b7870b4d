"""The true-peak meter and limiter kernels (viettts_amd/csrc/limiter.hip, include/vtts_limiter.h) on the GPU.  The meter is compared with ==
against the audio stage's own kernel (Resampler(fs, 4 fs)); the limiter against the float64 restatement of the contract
(tests/_limiter_oracle.py) within a bound the test derives itself: 4 x the distance of the float32 restatement from float64 over the same rows
(tests/test_limiter_cpu.py prints it).  Every batch is ragged with NaN past each row's end, and the outputs and the workspace are pre-filled
with NaN through the C ABI: whatever is read past a row, or left unwritten, shows."""
import ctypes as C

import numpy as np
import pytest
import torch

import _limiter_oracle as O
import _row_split as RS
from viettts_amd import _lib, wavio
from viettts_amd._handle import ptr

pytestmark = pytest.mark.gpu
FS, W, TILE = 16000, 80, O.TILE
EPS = 2.0 ** -23
_LIMS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    yield torch.device("cuda:0")
    for m in _LIMS.values():
        m.close()
    _LIMS.clear()


def _lim(dev, rate=FS, ms=5.0):
    from viettts_amd.limiter import TruePeakLimiter

    if (rate, ms) not in _LIMS:
        _LIMS[rate, ms] = TruePeakLimiter(rate, device=dev, lookahead_ms=ms)
        assert _LIMS[rate, ms].lookahead == O.lookahead(rate, ms)
    return _LIMS[rate, ms]


def _ragged(rows, extra=5, dtype=np.float32):
    """[N, longest + extra] with NaN (PCM16: -32768) past each row's end, and the lengths."""
    lens = [len(x) for x in rows]
    wav = np.full((len(rows), max(lens) + extra), np.nan if dtype == np.float32 else -32768, dtype)
    for i, x in enumerate(rows):
        wav[i, :len(x)] = x
    return wav, lens


def _workspace(m, N, longest):
    need = C.c_size_t(0)
    m._call("workspace_bytes", N, longest, C.byref(need))
    return torch.full((need.value,), 0xFF, dtype=torch.uint8, device=m.device)  # NaNs


def _meter(m, wav, lens, envelope=True):
    yt = torch.from_numpy(np.array(wav)).to(m.device)
    N, S = wav.shape
    ws = _workspace(m, N, max(lens))
    tp = torch.full((N,), float("nan"), dtype=torch.float32, device=m.device)
    env = torch.full((N, S), float("nan"), dtype=torch.float32, device=m.device) if envelope else None
    dtype = _lib.VTTS_AUDIO_PCM16 if wav.dtype == np.int16 else _lib.VTTS_AUDIO_F32
    m._on_stream("true_peak", ptr(yt), dtype, N, S, (C.c_int32 * N)(*lens), ptr(tp), ptr(env), ptr(ws), ws.numel())
    torch.cuda.synchronize()
    return tp, env


def _apply(m, wav, lens, gains=None, ceiling=-1.0, pcm_out=False, packed=False, envelope=False):
    """apply() through the C ABI into NaN-filled outputs -> (samples [N, S] or packed, true_peak, min_gain, gains_used, envelope) as numpy."""
    yt = torch.from_numpy(np.array(wav)).to(m.device)
    N, S = wav.shape
    ws = _workspace(m, N, max(lens))
    total = sum(lens) if packed else N * S
    out = torch.full((max(total, 1),), -12345, dtype=torch.int16, device=m.device) if pcm_out else torch.full((max(total, 1),), float("nan"), device=m.device)
    f = torch.full((3, N), float("nan"), dtype=torch.float32, device=m.device)
    env = torch.full((N, S), float("nan"), dtype=torch.float32, device=m.device) if envelope else None
    g = None if gains is None else torch.tensor(np.asarray(gains, np.float32), device=m.device)
    dtype = _lib.VTTS_AUDIO_PCM16 if wav.dtype == np.int16 else _lib.VTTS_AUDIO_F32
    m._on_stream("apply", ptr(yt), dtype, N, S, (C.c_int32 * N)(*lens), ptr(g), float(ceiling), ptr(out), int(pcm_out), 0 if packed else S, ptr(f[0]), ptr(f[1]),
                 ptr(f[2]), ptr(env), ptr(ws), ws.numel())
    torch.cuda.synchronize()
    y = out[:total].cpu().numpy()
    fr = f.cpu().numpy()
    return (y if packed else y.reshape(N, S)), fr[0], fr[1], fr[2], (None if env is None else env.cpu().numpy())


@pytest.fixture(scope="module")
def reference():
    f64, f32, d = O.gpu_reference()
    print(f"\nfloat32 restatement within {d:.3e} of float64: the bound is {4 * d:.3e}")
    assert 0 < d <= 4e-6  # otherwise the arithmetic is wrong, not the bound
    return f64, 4 * d


@pytest.fixture(scope="module")
def batch(dev):
    """The ragged batch of _limiter_oracle.gpu_rows() through apply(), once."""
    rows = O.gpu_rows()
    wav, lens = _ragged([x for _, x, _ in rows])
    gains = [g for _, _, g in rows]
    return wav, lens, gains, _apply(_lim(dev), wav, lens, gains, envelope=True)


# ------------------------------------------------------------ the meter ------------------------------------------------------------
@pytest.mark.parametrize("rate,pcm", [(16000, False), (16000, True), (22050, False), (48000, False)])
def test_true_peak_and_envelope_equal_the_resamplers_output(dev, rate, pcm):
    """true_peak == max(|x|.max(), |Resampler(fs, 4 fs)(x)|.max()) and the envelope == the per-sample maximum of the same, bit for bit, at every
    edge length in one ragged batch."""
    from viettts_amd.audio import Resampler

    m = _lim(dev, rate)
    rows = [O.speech(400 + i, S, rate) for i, S in enumerate(O.edge_lengths(rate))]
    if pcm:
        rows = [wavio.float_to_pcm16(x) for x in rows]
    wav, lens = _ragged(rows, dtype=np.int16 if pcm else np.float32)
    tp, env = _meter(m, wav, lens)
    tp_only, _ = _meter(m, wav, lens, envelope=False)
    assert torch.equal(tp, tp_only)
    rs = Resampler(rate, 4 * rate, device=dev)
    try:
        x = torch.from_numpy(wav).to(dev)
        u = rs(x if pcm else torch.nan_to_num(x), lens)
        xf = x.float() / 32768.0 if pcm else x
        for b, n in enumerate(lens):
            if n == 0:
                assert float(tp[b]) == 0.0 and bool((env[b] == 0).all())
                continue
            want = torch.maximum(xf[b, :n].abs(), u[b, :4 * n].abs().view(n, 4).max(dim=1).values)
            assert torch.equal(env[b, :n], want), (b, n)
            assert bool((env[b, n:] == 0).all()), (b, n)
            assert float(tp[b]) == float(want.max()), (b, n)
    finally:
        rs.close()


def test_quarter_rate_sine_reads_three_db_more_than_its_samples(dev):
    x = O.tone(FS / 4, 1.0, 4000, FS, np.pi / 4)
    tp, env = _meter(_lim(dev), x[None, :], [4000])
    inside = float(env[0, 200:-200].max())
    print(f"\nsample peak {np.abs(x).max():.6f}, true peak inside {inside:.7f}, with the ends {float(tp[0]):.6f}")
    assert abs(inside - 1.0) <= 1e-6 and float(tp[0]) == float(np.float32(O.true_peak(x, FS, np.float32)))


# ------------------------------------------------------------ the limiter ------------------------------------------------------------
def test_ragged_batch_agrees_with_the_float64_oracle(dev, reference, batch):
    """Edge lengths from 0 to two tiles and a 3 s row, speech 3 / 6 / 12 dB over the ceiling, clicks at samples 0, S - 1 and TILE - 1, TILE,
    TILE +- W, TILE +- 2 W, pairs 2 W and 4 W + 1 apart across tile edges, a plateau longer than the window."""
    f64, bound = reference
    wav, lens, gains, (y, tp, mg, gu, env) = batch
    worst, over_max = 0.0, -np.inf
    for b, ((name, x, g), r) in enumerate(zip(O.gpu_rows(), f64)):
        n = lens[b]
        assert np.all(y[b, n:] == 0), name  # zeros past the row's end, and no NaN from the halo inside it
        assert gu[b] == np.float32(g), name
        if n == 0:
            assert tp[b] == 0.0 and mg[b] == 1.0
            continue
        err = float(np.abs(y[b, :n] - r.y).max())
        worst = max(worst, err)
        assert err <= bound, (name, err)
        assert abs(float(mg[b]) - r.min_gain) <= bound / float(r.c), name
        # (the bits of the meter are test_true_peak_and_envelope_equal_the_resamplers_output's; against float64, a chain of 52 fmaf and fp32 taps
        # is within 53 x 2^-24 of the sum of |x h|, itself under 3 max |x| for this filter)
        tol = 53 * 2.0 ** -24 * 3 * r.true_peak
        assert abs(float(tp[b]) - r.true_peak) <= tol, name
        assert np.abs(env[b, :n] - r.p).max() <= tol and np.all(env[b, n:] == 0), name
        assert float(np.abs(y[b, :n]).max()) <= float(r.c) * (1 + EPS) ** 2, name
        got, ora = O.true_peak(y[b, :n], FS), O.true_peak(r.y.astype(np.float32), FS)
        over = 20 * np.log10(got / float(r.c))
        over_max = max(over_max, over)
        print(f"\n{name}: {n} samples, error {err:.2e}, min gain {mg[b]:.4f}, true peak of the output {over:+.5f} dB from the ceiling (oracle {20 * np.log10(ora / float(r.c)):+.5f})")
        assert got <= max(ora, float(r.c)) + bound, name
    print(f"\nlargest error {worst:.3e} of {bound:.3e}; largest true-peak overshoot {over_max:.4f} dB")


def test_a_row_gives_the_same_bits_however_it_arrives(dev, batch):
    """Alone, in the ragged batch, at another S_stride, as the fp32 of its PCM16 values; packed equals strided; PCM16 out is float_to_pcm16 of
    the fp32 out; a row under the ceiling is fl(g x) and nothing else."""
    m = _lim(dev)
    wav, lens, gains, (y, tp, mg, gu, env) = batch
    names = [n for n, _, _ in O.gpu_rows()]
    for name in (f"len{TILE + 2 * W + 1}", "clicks", "len1"):
        b = names.index(name)
        n = lens[b]
        for extra in (0, 3, 1029):
            w1, l1 = _ragged([wav[b, :n]], extra=extra)
            y1, tp1, mg1, _, _ = _apply(m, w1, l1, [gains[b]])
            assert np.array_equal(y1[0, :n].view(np.uint32), y[b, :n].view(np.uint32)) and np.all(y1[0, n:] == 0), (name, extra)
            assert tp1[0] == tp[b] and mg1[0] == mg[b]
    # PCM16 in: the same bits as the fp32 of the same values
    pcm = [wavio.float_to_pcm16(x) for _, x, _ in O.gpu_rows()]
    wp, lp = _ragged(pcm, dtype=np.int16)
    wf, _ = _ragged([p.astype(np.float32) / np.float32(32768.0) for p in pcm])
    yp, tpp, mgp, _, _ = _apply(m, wp, lp, gains)
    yf, tpf, mgf, _, _ = _apply(m, wf, lp, gains)
    assert np.array_equal(yp.view(np.uint32), yf.view(np.uint32)) and np.array_equal(tpp, tpf) and np.array_equal(mgp, mgf)
    # packed, and PCM16 out
    packed, tpk, mgk, _, _ = _apply(m, wav, lens, gains, packed=True)
    assert np.array_equal(packed.view(np.uint32), np.concatenate([y[b, :n] for b, n in enumerate(lens)]).view(np.uint32))
    assert np.array_equal(tpk, tp) and np.array_equal(mgk, mg)
    y16, _, mg16, _, _ = _apply(m, wav, lens, gains, pcm_out=True)
    assert np.array_equal(y16, wavio.float_to_pcm16(y).reshape(y.shape)) and np.array_equal(mg16, mg)
    p16, _, _, _, _ = _apply(m, wav, lens, gains, pcm_out=True, packed=True)
    assert np.array_equal(p16, np.concatenate([y16[b, :n] for b, n in enumerate(lens)]))
    # under the ceiling
    b = names.index("under")
    assert mg[b] == 1.0 and np.array_equal(y[b, :lens[b]].view(np.uint32), (np.float32(gains[b]) * wav[b, :lens[b]]).view(np.uint32))
    # without gains: g = 1
    y0, _, mg0, gu0, _ = _apply(m, wav, lens, None)
    y1, _, mg1, gu1, _ = _apply(m, wav, lens, [1.0] * len(lens))
    assert np.array_equal(y0.view(np.uint32), y1.view(np.uint32)) and np.array_equal(mg0, mg1) and np.all(gu0 == 1.0) and np.all(gu1 == 1.0)


def test_rows_across_the_launch_split_are_the_rows_before_it(dev, reference):
    """The lengths of 128 rows travel with one launch.  Rows 128 + b of the batch of tests/_row_split.py differ from rows b in content, length
    and gain and hold the longest row and a one-sample row: EVERY row, the fillers included, is compared with the float64 oracle of that row
    as test_ragged_batch_agrees_with_the_float64_oracle does (samples, min gain, true peak, envelope, gain used).  Three more rows behind
    them are rows 0 .. 2 again: a row of the second launch is bit for bit the same row of the first."""
    f64, bound = reference
    split = _lib.LIMITER_ROWS_PER_LAUNCH
    bt = RS.limiter_batch(split)
    refs = RS.per_kind(bt, lambda r: O.limit(r.content[: r.length], FS, r.scalar)) + [None] * 3
    refs[-3:] = refs[:3]
    wav, lens = _ragged([bt.rows[b, :n] for b, n in enumerate(bt.lengths)] + [bt.rows[b, : bt.lengths[b]] for b in range(3)])
    gains = list(bt.scalars) + list(bt.scalars[:3])
    m = _lim(dev)
    y, tp, mg, gu, env = _apply(m, wav, lens, gains, envelope=True)
    assert len(lens) == split + 6 and max(lens) == lens[split + 1] and min(lens) == lens[split + 2] == 1
    worst = {False: 0.0, True: 0.0}
    for b, (n, r) in enumerate(zip(lens, refs)):
        assert np.all(y[b, n:] == 0) and gu[b] == np.float32(gains[b]), b
        err = float(np.abs(y[b, :n] - r.y).max())
        worst[b >= split] = max(worst[b >= split], err / bound)
        assert err <= bound, (b, err)
        assert abs(float(mg[b]) - r.min_gain) <= bound / float(r.c), b
        tol = 53 * 2.0 ** -24 * 3 * r.true_peak
        assert abs(float(tp[b]) - r.true_peak) <= tol and np.abs(env[b, :n] - r.p).max() <= tol and np.all(env[b, n:] == 0), b
        assert float(np.abs(y[b, :n]).max()) <= float(r.c) * (1 + EPS) ** 2, b
    print(f"\nlimiter rows across the split: worst error / bound {worst[False]:.3f} before, {worst[True]:.3f} behind the split (bound {bound:.2e})")
    for b in range(3):
        n = lens[b]
        assert np.array_equal(y[split + 3 + b].view(np.uint32), y[b].view(np.uint32)) and not np.isnan(y[b]).any() and np.abs(y[b, :n]).max() > 0.5
        assert tp[split + 3 + b] == tp[b] and mg[split + 3 + b] == mg[b] < 1.0 and gu[split + 3 + b] == gu[b]
        assert np.array_equal(env[split + 3 + b], env[b])
        assert lens[split + b] != n and gains[split + b] != gains[b] and not np.array_equal(y[split + b, :8].view(np.uint32), y[b, :8].view(np.uint32))
    packed, _, _, _, _ = _apply(m, wav, lens, gains, packed=True)
    assert np.array_equal(packed.view(np.uint32), np.concatenate([y[b, :n] for b, n in enumerate(lens)]).view(np.uint32))
    tpm, envm = _meter(m, wav, lens)
    assert np.array_equal(tpm.cpu().numpy(), tp) and np.array_equal(envm.cpu().numpy(), env)


@pytest.mark.parametrize("rate,ms,lengths", [(16000, 2.0, (65, TILE + 65, 2 * TILE + 1)), (96000, 10.0, (TILE + 2 * 960 + 1,))])
def test_shortest_and_longest_lookahead(dev, rate, ms, lengths):
    """W = 32, and W = 960 at 96 kHz: the extremes of the span a workgroup stages.  The bound is this configuration's own: 4 x the float32
    restatement's distance on these rows."""
    m = _lim(dev, rate, ms)
    Wn = O.lookahead(rate, ms)
    assert Wn == m.lookahead == (32 if ms == 2.0 else 960)
    rows = [O.speech(700 + i, S, rate) for i, S in enumerate(lengths)]
    f64 = [O.limit(x, rate, 4.0, W=Wn) for x in rows]
    f32 = [O.limit(x, rate, 4.0, W=Wn, dtype=np.float32) for x in rows]
    bound = 4 * max(float(np.abs(a.y - b.y).max()) for a, b in zip(f64, f32))
    assert 0 < bound <= 1.6e-5
    wav, lens = _ragged(rows)
    y, tp, mg, _, _ = _apply(m, wav, lens, [4.0] * len(rows))
    for b, r in enumerate(f64):
        n = lens[b]
        err = float(np.abs(y[b, :n] - r.y).max())
        print(f"\n{rate} Hz, W = {Wn}, {n} samples: error {err:.2e} of {bound:.2e}, min gain {mg[b]:.4f}")
        assert err <= bound and np.all(y[b, n:] == 0)
        assert abs(float(mg[b]) - r.min_gain) <= bound / float(r.c) and mg[b] < 1.0
        assert float(np.abs(y[b, :n]).max()) <= float(r.c) * (1 + EPS) ** 2


# ------------------------------------------------------------ normalize and the hooks ------------------------------------------------------------
def test_normalize_keeps_the_target_gain_where_the_meter_backs_off(dev, reference):
    """A quiet row with one loud click.  LoudnessMeter.normalize caps the whole row at the click's sample peak and ends far under the target;
    TruePeakLimiter.normalize applies the target gain and dips around the click only.  (Measured: DESIGN.md section 6q.)"""
    from viettts_amd.loudness import LoudnessMeter

    _, bound = reference
    S, k, target = 2 * FS, 10000, -23.0
    x = (0.1 * O.speech(800, S, FS)).astype(np.float32)
    x[k] = 0.9
    m, meter = _lim(dev), LoudnessMeter(FS, device=dev)
    try:
        xt = torch.from_numpy(x[None, :]).to(dev)
        before = meter(xt)
        ym, gm = meter.normalize(xt, target=target)
        yl, r = m.normalize(xt, target=target, meter=meter)
        lm, ll = float(meter(ym).integrated[0]), float(meter(yl).integrated[0])
        I = float(before.integrated[0])
        g = float(r.gains[0])
        print(f"\ninput {I:.2f} LUFS; LoudnessMeter.normalize: gain {20 * np.log10(float(gm[0])):+.2f} dB -> {lm:.2f} LUFS; "
              f"TruePeakLimiter.normalize: gain {20 * np.log10(g):+.2f} dB, deepest reduction {20 * np.log10(float(r.min_gain[0])):.2f} dB -> {ll:.2f} LUFS")
        assert abs(g / float(O.pregain(before.integrated[0].item(), target)) - 1.0) <= EPS and g > 2.0
        assert float(gm[0]) < 1.0 and lm < target - 6.0      # the shortfall of the sample-peak cap
        assert ll > lm + 6.0                                 # (how close to the target is reported, not required)
        assert float(r.min_gain[0]) < 0.5 and float(r.true_peak[0]) == float(m.true_peak(xt)[0])
        y = yl[0].cpu().numpy()
        plain = np.float32(g) * x
        far = np.abs(np.arange(S) - k) > 2 * W + 30
        assert np.array_equal(y[far].view(np.uint32), plain[far].view(np.uint32))        # min_gain < 1 around the click only
        assert np.all(np.abs(y[k - 2 * W:k + 2 * W]) < np.abs(plain[k - 2 * W:k + 2 * W]) + (plain[k - 2 * W:k + 2 * W] == 0))
        ref = O.limit(x, FS, np.float32(g))
        assert np.abs(y - ref.y).max() <= bound and O.true_peak(y, FS) <= max(O.true_peak(ref.y.astype(np.float32), FS), float(ref.c)) + bound
        # PCM16 and packed through the same path
        p16, r16 = m.normalize(xt, target=target, out_dtype="pcm16", packed=True, meter=meter)
        assert np.array_equal(p16.cpu().numpy(), wavio.float_to_pcm16(y)) and torch.equal(r16.min_gain, r.min_gain)
    finally:
        meter.close()


def test_pipeline_limit_is_off_by_default_and_holds_the_ceiling(dev, reference):
    """Three sentences of the synthetic models the pipeline tests use.  ``limit=False`` is the call without the argument, bit for bit; with
    ``loudness=T, limit=True`` every sentence is the oracle's limited row within the bound, its true peak under the ceiling by the same rule as above."""
    from viettts_amd.hifigan.config import V1
    from viettts_amd.hifigan.generator import Generator
    from viettts_amd.hifigan.synth import synthetic_params
    from viettts_amd.limiter import default_limiter
    from viettts_amd.nat.acoustic import AcousticModel
    from viettts_amd.nat.config import FLAGS
    from viettts_amd.nat.duration import DurationModel
    from viettts_amd.nat.synth import synthetic_acoustic_checkpoint, synthetic_duration_checkpoint
    from viettts_amd.pipeline import synthesize_sentences

    _, bound = reference
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
        plain = synthesize_sentences(sents, dm, am, gen, silence_duration=0.05, loudness=-8.0)
        plain = {i: plain[i].copy() for i in plain}
        off = synthesize_sentences(sents, dm, am, gen, silence_duration=0.05, loudness=-8.0, limit=False)
        assert sorted(off) == [0, 1, 2] and all(np.array_equal(off[i].view(np.uint32), plain[i].view(np.uint32)) for i in plain)
        on = synthesize_sentences(sents, dm, am, gen, silence_duration=0.05, loudness=-8.0, limit=True)
        on = {i: on[i].copy() for i in on}
        pcm = synthesize_sentences(sents, dm, am, gen, silence_duration=0.05, loudness=-8.0, limit=True, out_dtype="pcm16")
        lim = default_limiter(dev, FLAGS.sample_rate)
        worked = 0
        for i in range(3):
            assert on[i].dtype == np.float32 and on[i].shape == base[i].shape
            assert np.array_equal(pcm[i], wavio.float_to_pcm16(on[i])), i
            _, r = lim.normalize(base[i][None, :], target=-8.0)  # the gain the hook used, from the same kernels
            ref = O.limit(base[i], FLAGS.sample_rate, np.float32(r.gains[0].item()))
            got, ora = O.true_peak(on[i], FLAGS.sample_rate), O.true_peak(ref.y.astype(np.float32), FLAGS.sample_rate)
            print(f"\nsentence {i}: {len(base[i])} samples, gain {20 * np.log10(float(ref.g)):+.2f} dB, min gain {ref.min_gain:.4f}, "
                  f"true peak {20 * np.log10(max(got, 1e-30)):+.4f} dBTP")
            assert np.abs(on[i] - ref.y).max() <= bound, i
            assert got <= max(ora, float(ref.c)) + bound, i
            worked += ref.min_gain < 1.0
        assert worked >= 1  # the target is loud enough for the limiter to have something to do
        with pytest.raises(ValueError):
            synthesize_sentences(sents, dm, am, gen, limit=True)
    finally:
        gen.close()
        dm.close()
        am.close()


@pytest.mark.parametrize("rate", [16000, 22050])
def test_limiter_cli_prints_true_peak_beside_sample_peak_and_writes_the_limited_file(dev, rate, tmp_path, capsys):
    from viettts_amd import limiter

    x = (0.25 * O.speech(900, 2 * rate, rate)).astype(np.float32)
    x[rate] = 0.95
    src, dst = str(tmp_path / "in.wav"), str(tmp_path / "out.wav")
    pcm = wavio.float_to_pcm16(x)
    wavio.write_wav_pcm16(src, pcm, rate)
    limiter.main(["--wav", src])
    first = capsys.readouterr().out.strip().splitlines()
    tp = O.true_peak(pcm, rate, np.float32)
    assert len(first) == 1 and first[0].startswith(f"true peak {20 * np.log10(tp):.2f} dBTP  sample peak {20 * np.log10(np.abs(pcm).max() / 32768.0):.2f} dBFS")
    limiter.main(["--wav", src, "--target", "-16", "--ceiling-dbtp", "-2", "--output", dst])
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[0] == first[0] and lines[1].startswith("gain +") and "deepest reduction -" in lines[1] and "-2.0 dBTP" in lines[1] and lines[2] == f"wrote {dst}"
    sr, out = wavio.read_wav(dst)
    assert sr == rate and out.shape == pcm.shape
    over = 20 * np.log10(O.true_peak(out.astype(np.int16), rate) / 10 ** (-2.0 / 20))
    print(f"\n{rate} Hz: {lines[1]}; the written file's true peak is {over:+.4f} dB from the ceiling")
    # (not a bound of the contract: the overshoot scale the float64 prototype showed, at most 0.014 dB on white noise, and PCM16 rounding, 2^-16
    # a sample through a filter of absolute sum about 3, which is 0.0005 dB)
    assert over <= 0.05 and np.abs(out.astype(np.float64)).max() / 32768.0 > 0.5 * 10 ** (-2.0 / 20)
    with pytest.raises(SystemExit):
        limiter.main(["--wav", src, "--output", dst])
