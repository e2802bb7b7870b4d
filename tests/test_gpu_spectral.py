"""The spectral kernels (viettts_amd/csrc/spectral.hip, include/vtts_spectral.h) on the GPU against the float64 restatement of the contract
(tests/_spectral_oracle.py).  Frame counts are compared with ==; magnitudes (relative to the row's largest) and the three figures within bounds
the test derives itself: 8 x the distance of the oracle's float32 mode from its float64 mode over the same rows (tests/test_spectral_cpu.py
prints them and shows that every planted fault misses one).  Where a row is too short for its figures' error to be anything but one draw (the
edge and split rows), the magnitudes are held to the oracle and the figures to the header's formulas applied to the magnitudes the kernel
itself returned: that isolates the framing, the reduction and the frame count from the transform's rounding.  Every batch is ragged with NaN
and noise at 1e4 past each row's end; every call goes through the C ABI into NaN-filled outputs and a workspace of 0xFF bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

import _row_split as RS
import _spectral_oracle as O
from viettts_amd import _lib
from viettts_amd._handle import ptr

pytestmark = pytest.mark.gpu
_METERS = {}
CFGS = [O.RESOLUTIONS[n] for n in O.N_FFTS]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    yield torch.device("cuda:0")
    for m in _METERS.values():
        m.close()
    _METERS.clear()


def _meter(cfg, dev):
    from viettts_amd.spectral import SpectralMeter

    if cfg not in _METERS:
        m = _METERS[cfg] = SpectralMeter(*cfg, device=dev)
        assert np.array_equal(m.window().view(np.uint32), O.window(cfg).view(np.uint32)) and m.frames_per_block == O.frames_per_block(cfg)
        m._pack()
        m._packed = True
    return _METERS[cfg]


def _bounds(cfg):
    b = O.bounds(cfg)
    print(f"\n{cfg}: float32 restatement within sc {b.scale_sc:.2e} / logmag {b.scale_logmag:.2e} / lsd {b.scale_lsd:.2e} / mags {b.scale_mags:.2e} of float64: "
          f"bounds {b.sc:.2e} / {b.logmag:.2e} / {b.lsd:.2e} / {b.mags:.2e}")
    return b


def _batch(pairs, pad=37, seed=5):
    """Rows of different lengths as one [N, S] pair; past each row's own end NaN and noise at 1e4 (PCM16: full-scale noise)."""
    lengths = [len(x) for x, _ in pairs]
    S = max(lengths) + pad
    rng = np.random.default_rng(seed)
    dt = pairs[0][0].dtype

    def junk():
        if dt == np.int16:
            return rng.integers(-30000, 30000, S).astype(np.int16)
        j = (1e4 * rng.standard_normal(S)).astype(np.float32)
        j[::3] = np.nan
        return j

    xs, ys = np.stack([junk() for _ in pairs]), np.stack([junk() for _ in pairs])
    for b, (x, y) in enumerate(pairs):
        xs[b, : len(x)], ys[b, : len(y)] = x, y
    return xs, ys, lengths


class Got:
    pass


def _run(m, xs, ys, lengths=None, mags=True, extra=2):
    """forward() through the C ABI into NaN-filled outputs; the magnitudes ``extra`` frames wider than the longest row needs."""
    xt, yt = torch.from_numpy(np.array(xs)).to(m.device), torch.from_numpy(np.array(ys)).to(m.device)
    N, S = xs.shape
    lens = [S] * N if lengths is None else [int(v) for v in lengths]
    T = O.num_frames(max(lens), (m.n_fft, m.win, m.hop)) + extra
    ws = torch.full((max(8, m.workspace_bytes(N, max(lens))),), 0xFF, dtype=torch.uint8, device=m.device)  # NaNs: whatever is read unwritten shows
    f = torch.full((3, N), float("nan"), dtype=torch.float64, device=m.device)
    n = torch.full((N,), -7, dtype=torch.int32, device=m.device)
    mg = torch.full((N, 2, T, m.n_bins), float("nan"), dtype=torch.float32, device=m.device) if mags else None
    dtype = _lib.VTTS_AUDIO_PCM16 if xs.dtype == np.int16 else _lib.VTTS_AUDIO_F32
    m._on_stream("forward", ptr(xt), ptr(yt), dtype, N, S, None if lengths is None else (C.c_int32 * N)(*lens), ptr(f[0]), ptr(f[1]), ptr(f[2]), ptr(n),
                 ptr(mg), T, ptr(ws), ws.numel())
    torch.cuda.synchronize(m.device)
    g = Got()
    g.f, g.n, g.mags = f.cpu().numpy(), n.cpu().numpy(), mg.cpu().numpy() if mags else None
    return g


def _figures_of(mags: np.ndarray):
    """The header's formulas in float64 on magnitudes [2, T, NB] the kernel returned (P = M^2: M is P's correctly rounded fp32 root)."""
    mx, my = mags[0].astype(np.float64), mags[1].astype(np.float64)
    L = 2.0 * np.log(my / mx)
    T, nb = mx.shape
    return (float(np.sqrt(((my - mx) ** 2).sum()) / np.sqrt((mx ** 2).sum())), float(0.5 * np.abs(L).sum() / (T * nb)),
            float(np.sqrt(((10.0 / np.log(10.0) * L) ** 2).sum(axis=1) / nb).sum() / T))


# M = fl32(sqrt(P)) is within 2^-24 of the root, so 2 ln(My / Mx) is within 4 * 2^-24 of ln(Py / Px) on every bin: the figures recomputed
# from the returned magnitudes lie within these of the kernel's (sc uses the magnitudes themselves: fp64 summation order alone)
OWN_TOL = (1e-12, 0.5 * 4 * 2.0 ** -24, 10.0 / np.log(10.0) * 4 * 2.0 ** -24)


def _check_row(g, b, ref, bd, figures_vs_oracle, worst):
    T = ref.n_frames
    assert g.n[b] == T, (b, g.n[b], T)
    mags = g.mags[b, :, :T]
    assert np.isfinite(mags).all() and np.isnan(g.mags[b, :, T:]).all(), b  # every frame of the row written, nothing past them
    dm = float(np.abs(mags - ref.mags).max() / ref.mags.max())
    worst["mags"] = max(worst.get("mags", 0.0), dm / bd.mags)
    assert dm <= bd.mags, (b, dm, bd.mags)
    own = _figures_of(mags)
    for k, name in enumerate(("sc", "logmag", "lsd")):
        got, want = float(g.f[k, b]), getattr(ref, name)
        tol = OWN_TOL[k] * (max(abs(own[k]), 1.0) if k == 0 else 1.0)
        assert abs(got - own[k]) <= tol, (b, name, got, own[k])
        worst[name] = max(worst.get(name, 0.0), abs(got - want) / getattr(bd, name))
        if figures_vs_oracle:
            print(f"  row {b:3d} {name:6s} kernel {got:.9f} oracle {want:.9f}  |d| {abs(got - want):.2e} = {abs(got - want) / getattr(bd, name):.3f} bounds")
            assert abs(got - want) <= getattr(bd, name), (b, name, got, want)


def _report(what, worst):
    print(f"{what}: worst error / bound  " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("cfg", CFGS, ids=str)
def test_accuracy_against_the_float64_oracle(cfg, dev):
    m, bd = _meter(cfg, dev), _bounds(cfg)
    pairs = [O.case(i) for i in range(O.N_CASES)]
    assert O.num_frames(len(pairs[-1][0]), cfg) > 100 * m.frames_per_block  # the long row spans many workgroups
    g = _run(m, *_batch(pairs))
    worst = {}
    for i in range(O.N_CASES):
        _check_row(g, i, O.case_reference(i, cfg)[0], bd, True, worst)
    _report(f"{cfg} accuracy", worst)


@pytest.mark.parametrize("cfg", CFGS, ids=str)
def test_edges_of_the_row_the_hop_and_the_workgroup(cfg, dev):
    m, bd = _meter(cfg, dev), O.bounds(cfg)
    n_fft, _, hop = cfg
    F, lo = m.frames_per_block, O.min_samples(cfg)
    k = lo // hop + 2
    g2 = -(-(lo // hop + 2) // F) + 1  # a workgroup count whose frames lie above the minimum
    lens = [lo, lo + 1, k * hop - 1, k * hop, k * hop + 1, (F * g2 - 1) * hop - 1, (F * g2 - 1) * hop, F * g2 * hop - 1, F * g2 * hop, F * g2 * hop + 1]
    assert O.num_frames(lens[5], cfg) == F * g2 - 1 and O.num_frames(lens[6], cfg) == F * g2 and O.num_frames(lens[8], cfg) == F * g2 + 1
    x, y = O.make_speechlike(max(lens), 71), None
    y = O.degrade(x, 71, 0.4)
    pairs = [(x[:n].copy(), y[:n].copy()) for n in lens]
    g = _run(m, *_batch(pairs))
    worst = {}
    for b, (px, py) in enumerate(pairs):
        _check_row(g, b, O.measure(px, py, cfg), bd, False, worst)
    _report(f"{cfg} edges (figures against the oracle for the record)", worst)
    xs, ys, lengths = _batch(pairs[:2])
    with pytest.raises(_lib.VttsError) as e:
        _run(m, xs, ys, [lo - 1, lo])
    assert e.value.status == -6


@pytest.mark.parametrize("cfg", CFGS, ids=str)
def test_a_row_is_the_same_bits_alone_in_a_batch_and_as_pcm16(cfg, dev):
    m = _meter(cfg, dev)
    F, hop = m.frames_per_block, cfg[2]
    pairs16 = []
    for i, n in ((0, None), (4, None), (5, F * hop * 3 + 1), (O.N_CASES - 1, 40000)):
        x, y = O.case(i)
        pairs16.append((np.rint(x[:n] * 32767.0).astype(np.int16), np.rint(np.clip(y[:n], -1, 1) * 32767.0).astype(np.int16)))
    pairs32 = [(O.as_float32(x), O.as_float32(y)) for x, y in pairs16]
    a16, a32, wide = _run(m, *_batch(pairs16)), _run(m, *_batch(pairs32)), _run(m, *_batch(pairs32, pad=1001, seed=6))  # two strides
    for r, (x, y) in enumerate(pairs32):
        T = O.num_frames(len(x), cfg)
        alone = _run(m, x[None, :], y[None, :])
        for other in (a16, a32, wide):
            assert alone.n[0] == other.n[r] == T
            assert np.array_equal(alone.f.view(np.uint64)[:, 0], other.f.view(np.uint64)[:, r]), r
            assert np.array_equal(alone.mags.view(np.uint32)[0, :, :T], other.mags.view(np.uint32)[r, :, :T]), r
        assert np.isfinite(alone.f).all()


@pytest.mark.parametrize("cfg", CFGS, ids=str)
def test_equal_signals_give_exact_zeros_and_mags_change_no_figure(cfg, dev):
    m = _meter(cfg, dev)
    pairs = [O.case(i) for i in (1, 4, 5)]
    same = [(x, x.copy()) for x, _ in pairs]
    g = _run(m, *_batch(same))
    assert np.array_equal(g.f, np.zeros_like(g.f)), g.f  # sc = logmag = lsd = 0, exactly
    for b, (x, _) in enumerate(same):
        T = O.num_frames(len(x), cfg)
        assert np.array_equal(g.mags.view(np.uint32)[b, 0, :T], g.mags.view(np.uint32)[b, 1, :T])
    xs, ys, lengths = _batch(pairs)
    with_mags, without = _run(m, xs, ys, lengths), _run(m, xs, ys, lengths, mags=False)
    assert np.array_equal(with_mags.f.view(np.uint64), without.f.view(np.uint64)) and np.array_equal(with_mags.n, without.n)
    assert (with_mags.f > 0).all()


def _split_batch(cfg, P):
    """P + 3 rows of [S, 2] (x, y) by the rules of tests/_row_split.py: behind the split the longest row, strictly, and one of the minimum."""
    lo, S = O.min_samples(cfg), 3 * cfg[0] + 200

    def rows(seed, lengths, levels):
        out = []
        for i, (n, level) in enumerate(zip(lengths, levels)):
            x = RS.speechlike(seed + i, S)
            out.append(RS.Row(np.stack([x, O.degrade(x, seed + i, level)], axis=1), n))
        return out

    front, behind = rows(40, (lo + 300, 2 * cfg[0], lo + 77), (0.5, 0.3, 1.0)), rows(50, (lo + 41, S, lo), (0.4, 0.8, 0.5))
    return RS.split_batch(P, front, behind, rows(60, (lo + 1, 2 * cfg[0] + 99, lo + 500, S - 1), (0.6, 0.5, 0.2, 0.9)), min_length=lo)


@pytest.mark.parametrize("cfg", [O.RESOLUTIONS[512], O.RESOLUTIONS[2048]], ids=str)
def test_rows_behind_the_launch_split(cfg, dev):
    """SPECTRAL_ROWS_PER_LAUNCH + 3 rows: the rows behind the split differ from the first rows in both signals and in length, and hold the
    longest row (the grid, the partials' stride and T_stride are the second launch's) and one of the minimum length.  Every row against the
    oracle (once per distinct row); each row behind the split is the row alone, bit for bit."""
    m, bd = _meter(cfg, dev), O.bounds(cfg)
    bt = _split_batch(cfg, _lib.SPECTRAL_ROWS_PER_LAUNCH)
    assert bt.N == _lib.SPECTRAL_ROWS_PER_LAUNCH + 3
    xs, ys = np.ascontiguousarray(bt.rows[:, :, 0]), np.ascontiguousarray(bt.rows[:, :, 1])
    refs = RS.per_kind(bt, lambda r: O.measure(r.content[: r.length, 0], r.content[: r.length, 1], cfg))
    g = _run(m, xs, ys, bt.lengths)
    before, behind = {}, {}
    for b, ref in enumerate(refs):
        _check_row(g, b, ref, bd, False, behind if b >= bt.P else before)
    _report(f"{cfg} rows before the split", before)
    _report(f"{cfg} rows behind the split", behind)
    for b in bt.behind():
        n = bt.lengths[b]
        a = _run(m, xs[b : b + 1, :n], ys[b : b + 1, :n])
        T = refs[b].n_frames
        assert a.n[0] == g.n[b] and np.array_equal(a.f.view(np.uint64)[:, 0], g.f.view(np.uint64)[:, b]), b
        assert np.array_equal(a.mags.view(np.uint32)[0, :, :T], g.mags.view(np.uint32)[b, :, :T]), b


def test_python_meter_and_multi_resolution_means(dev):
    from viettts_amd.spectral import MultiResolutionStft, default_mrstft, format_result, wav_mrstft

    pairs = [O.case(i) for i in (3, 4)]  # 2049 and 4700 samples
    xs, ys, lengths = _batch(pairs)
    xt, yt = torch.from_numpy(xs).to(dev), torch.from_numpy(ys).to(dev)
    mr = default_mrstft("cuda")
    assert mr is default_mrstft(dev) and mr.resolutions == O.DEFAULTS and mr.min_samples == 1025
    r = wav_mrstft(xt, yt, lengths)
    per = []
    for cfg, p in zip(O.DEFAULTS, r.per_resolution):
        m = _meter(cfg, dev)
        g = _run(m, xs, ys, lengths, extra=0)
        q = m(xt, yt, lengths, mags=True)  # the Python class returns what the C ABI wrote ...
        for got, want in ((q.sc, g.f[0]), (q.logmag, g.f[1]), (q.lsd, g.f[2])):
            assert np.array_equal(got.cpu().numpy().view(np.uint64), want.view(np.uint64))
        assert np.array_equal(q.n_frames.cpu().numpy(), g.n) and q.mags.shape == g.mags.shape
        for b, n in enumerate(g.n):
            assert np.array_equal(q.mags[b, :, :n].cpu().numpy().view(np.uint32), g.mags[b, :, :n].view(np.uint32)) and not q.mags[b, :, n:].any()
        assert p.mags is None and torch.equal(p.sc, q.sc) and torch.equal(p.logmag, q.logmag) and torch.equal(p.lsd, q.lsd)  # ... and so does the meter of three
        per.append(q)
    assert torch.equal(r.mrstft, sum(p.sc + p.logmag for p in per) / 3.0) and torch.equal(r.lsd, sum(p.lsd for p in per) / 3.0)
    one = _meter(O.DEFAULTS[0], dev)(xt[0, : lengths[0]].contiguous(), yt[0, : lengths[0]].contiguous())  # one row, 1-D
    assert torch.equal(one.sc, per[0].sc[:1])
    mixed = mr(np.rint(xs[:, :2000] * 32767.0).astype(np.int16), xs[:, :2000].copy())  # numpy in, PCM16 against float32
    assert np.isfinite(mixed.mrstft.cpu().numpy()).all() and float(mixed.mrstft.max()) < 0.05  # the quantisation alone
    text = format_result(r)
    assert text.count("\n") == 3 and "n_fft 2048" in text and "multi-resolution STFT distance" in text
    with pytest.raises(ValueError, match="1025"):
        mr(xt[:, :1024].contiguous(), yt[:, :1024].contiguous())
    with pytest.raises(ValueError, match="1025"):
        mr(xt, yt, [1024, 2000])
    two = MultiResolutionStft(((256, 160, 40), (512, 240, 50)), dev)
    assert two.min_samples == 257 and two(xt[:, :300].contiguous(), yt[:, :300].contiguous()).mrstft.shape == (2,)
    two.close()


def test_command_line_prints_the_three_resolutions_and_the_means(dev, tmp_path, capsys):
    from viettts_amd import spectral, wavio

    x, y = O.case(4)
    px, py = RS.to_pcm16(x), RS.to_pcm16(np.clip(y, -1, 1))
    wavio.write_wav_pcm16(tmp_path / "a.wav", px, O.RATE)
    wavio.write_wav_pcm16(tmp_path / "b.wav", py[:-100], O.RATE)  # lengths within one model hop: the common length is scored
    spectral.main(["--ref", str(tmp_path / "a.wav"), "--test", str(tmp_path / "b.wav")])
    out = capsys.readouterr().out
    want = spectral.wav_mrstft(torch.from_numpy(px[None, :-100].copy()).to(dev), torch.from_numpy(py[None, :-100].copy()).to(dev))
    assert out.strip() == spectral.format_result(want) and out.count("n_fft") == 3 and f"{float(want.mrstft[0]):.4f}" in out
    wavio.write_wav_pcm16(tmp_path / "c.wav", py[:-300], O.RATE)
    with pytest.raises(ValueError, match="model hop"):
        spectral.main(["--ref", str(tmp_path / "a.wav"), "--test", str(tmp_path / "c.wav")])
    wavio.write_wav_pcm16(tmp_path / "d.wav", py, 22050)
    with pytest.raises(ValueError, match="rate"):
        spectral.main(["--ref", str(tmp_path / "a.wav"), "--test", str(tmp_path / "d.wav")])


def test_score_segments_gains_the_spectral_keys_only_with_spectral(dev):
    from viettts_amd import vocoder_eval
    from viettts_amd.hifigan.config import V1
    from viettts_amd.hifigan.disc_synth import synthetic_disc_checkpoint
    from viettts_amd.hifigan.discriminators import Discriminators, fold_checkpoint
    from viettts_amd.hifigan.generator import Generator
    from viettts_amd.hifigan.synth import synthetic_params
    from viettts_amd.spectral import default_mrstft

    gen = Generator(V1, device=dev)
    gen.load_params(synthetic_params(V1, 4321, "scaled"))
    disc = Discriminators(dev).load_params(fold_checkpoint(synthetic_disc_checkpoint(8642)))
    try:
        x = RS.speechlike(41, 2 * 8192)
        y = torch.from_numpy(np.stack([x[:8192], x[8192:]])).to(dev)
        plain = vocoder_eval.score_segments(y, gen, disc)
        assert set(plain) == {"adv", "fm", "mel", "total", "disc"}
        scored = vocoder_eval.score_segments(y, gen, disc, spectral=default_mrstft(dev))
        assert set(scored) == set(plain) | set(vocoder_eval.SPECTRAL_KEYS) == set(plain) | {"mrstft", "sc", "logmag", "lsd"}
        assert all(scored[k] == pytest.approx(plain[k], rel=1e-6) for k in plain)  # the existing figures are what they were
        assert scored["mrstft"] == pytest.approx(scored["sc"] + scored["logmag"], rel=1e-12) and scored["sc"] > 0 and scored["lsd"] > 0
    finally:
        gen.close()
        disc.close()
