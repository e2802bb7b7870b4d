"""The complex STFT kernels (viettts_amd/csrc/stft.hip, include/vtts_stft.h) on the GPU against the float64 restatement of the contract
(tests/_stft_oracle.py), in both framings.  Every bound is derived here: 8 x the distance of the oracle's float32 mode from its float64 mode
over the oracle's rows (tests/test_stft_cpu.py prints them and shows that every planted fault misses one); the projection's is
condition-aware (``_stft_oracle.project_limit``).  What the header calls equal is compared with ==.  Every batch is ragged, with NaN and noise
at 1e4 past each row's samples and frames; every call goes through the C ABI into NaN-filled (int16: canary-filled) outputs."""
import ctypes as C

import numpy as np
import pytest
import torch

import _row_split as RS
import _spectral_oracle as SO
import _stft_oracle as O
from viettts_amd import _lib
from viettts_amd._handle import ptr
from viettts_amd.wavio import float_to_pcm16

pytestmark = pytest.mark.gpu
_STFTS = {}
CANARY16 = -12345


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    yield torch.device("cuda:0")
    for s in _STFTS.values():
        s.close()
    _STFTS.clear()


def _st(cfg, dev):
    from viettts_amd.stft import Stft

    if cfg not in _STFTS:
        s = _STFTS[cfg] = Stft(*cfg[:3], framing=cfg[3], device=dev)
        assert np.array_equal(s.window().view(np.uint32), O.window(cfg).view(np.uint32)) and s.pad == O.pad(cfg)
        s._tables()
    return _STFTS[cfg]


def _junk(rng, shape, dtype):
    if dtype == np.int16:
        return rng.integers(-30000, 30000, shape).astype(np.int16)
    j = (1e4 * rng.standard_normal(shape)).astype(np.float32)
    j.reshape(-1)[::3] = np.nan
    return j


def _wav_batch(rows, pad, seed):
    lengths = [len(x) for x in rows]
    xs = _junk(np.random.default_rng(seed), (len(rows), max(lengths) + pad), rows[0].dtype)
    for b, x in enumerate(rows):
        xs[b, : len(x)] = x
    return xs, lengths


def _spec_batch(specs, frames, extra, seed):
    """[N, T_stride, NB] complex64: row b's first frames[b] frames, junk behind them."""
    NB = specs[0].shape[1]
    buf = _junk(np.random.default_rng(seed), (len(specs), max(frames) + extra, NB, 2), np.float32).view(np.complex64)[..., 0]
    for b, (s, T) in enumerate(zip(specs, frames)):
        buf[b, :T] = s[:T]
    return np.ascontiguousarray(buf)


def _forward(st, cfg, rows, pad=37, extra=2, seed=5, project=None):
    """forward() (or, with project = (mags, tprevs, momentum), project()) through the C ABI.  -> per row the [T_b, NB] spectrum (and the new tprev)."""
    xs, lengths = _wav_batch(rows, pad, seed)
    N, S = xs.shape
    frames = [O.num_frames(n, cfg) for n in lengths]
    T = max(frames) + extra
    xt = torch.from_numpy(xs).to(st.device)
    spec = torch.full((N, T, st.n_bins, 2), float("nan"), dtype=torch.float32, device=st.device)
    dtype = _lib.VTTS_AUDIO_PCM16 if xs.dtype == np.int16 else _lib.VTTS_AUDIO_F32
    lens_c = (C.c_int32 * N)(*lengths)
    if project is None:
        st._on_stream("forward", ptr(xt), dtype, N, S, lens_c, ptr(spec), T)
        tp = None
    else:
        mags, tprevs, momentum = project
        mg = torch.from_numpy(np.ascontiguousarray(_spec_batch([m.astype(np.complex64) for m in mags], frames, extra, seed + 1).real)).to(st.device)
        tp = torch.from_numpy(_spec_batch(tprevs, frames, extra, seed + 2)).to(st.device)
        tp_before = tp.clone()
        st._on_stream("project", ptr(xt), dtype, N, S, lens_c, ptr(mg), ptr(tp), ptr(spec), T, C.c_float(momentum))
    torch.cuda.synchronize(st.device)
    got = spec.cpu().numpy().view(np.complex64)[..., 0]
    for b, Tb in enumerate(frames):
        assert np.isfinite(got[b, :Tb].view(np.float32)).all() and np.isnan(got[b, Tb:].view(np.float32)).all(), b  # every frame of the row, nothing past them
    out = [got[b, :Tb] for b, Tb in enumerate(frames)]
    if tp is None:
        return out
    tpn, tpb = tp.cpu().numpy(), tp_before.cpu().numpy()
    for b, Tb in enumerate(frames):
        assert np.array_equal(tpn[b, Tb:].view(np.uint32), tpb[b, Tb:].view(np.uint32)), b  # tprev past the row's frames is untouched
    return out, [tpn[b, :Tb] for b, Tb in enumerate(frames)]


def _inverse(st, cfg, specs, lengths, pad=37, extra=2, seed=5, pcm=False):
    """inverse() through the C ABI -> per row its S_b samples; the canary past them is checked here."""
    N = len(specs)
    frames = [O.num_frames(n, cfg) for n in lengths]
    buf = torch.from_numpy(_spec_batch(specs, frames, extra, seed)).to(st.device)
    S = max(lengths) + pad
    out = torch.full((N, S), CANARY16, dtype=torch.int16, device=st.device) if pcm else torch.full((N, S), float("nan"), dtype=torch.float32, device=st.device)
    st._on_stream("inverse", ptr(buf), N, buf.shape[1], (C.c_int32 * N)(*lengths), ptr(out), _lib.VTTS_AUDIO_PCM16 if pcm else _lib.VTTS_AUDIO_F32, S)
    torch.cuda.synchronize(st.device)
    got = out.cpu().numpy()
    for b, n in enumerate(lengths):
        assert (got[b, n:] == CANARY16).all() if pcm else np.isnan(got[b, n:]).all(), b  # nothing is written past S_b
        assert pcm or np.isfinite(got[b, :n]).all(), b
    return [got[b, :n] for b, n in enumerate(lengths)]


def _edge_lengths(st, cfg):
    """The smallest lengths at which the framing, the frame count or the workgroups' borders can go wrong."""
    n_fft, _, hop, _ = cfg
    F, W, run = st.blocking()
    lo = O.min_samples(cfg)
    k = lo // hop + 2
    lens = [lo, lo + 1, k * hop - 1, k * hop, k * hop + 1]
    if n_fft - 1 >= lo:
        lens.append(n_fft - 1)  # both reflections meet in one frame
    for per in (F, W):  # T one past a multiple of the frames a workgroup of forward() and a round of inverse() covers
        T = per * (-(-O.num_frames(lo, cfg) // per) + 1) + 1
        lens.append(O.num_samples(T, cfg))
        assert O.num_frames(lens[-1], cfg) == T and O.num_frames(lens[-1] - 1, cfg) == T - 1
    lens += [run, run + 1]  # the last workgroup of inverse() owns a whole run, and one sample
    return [n for n in lens if n >= lo]


def _random_specs(cfg, lengths, seed):
    rng = np.random.default_rng(seed)
    NB = cfg[0] // 2 + 1
    scale = np.float32(cfg[0] / 64.0)  # samples of a few tenths: the PCM16 output uses its range
    return [((rng.standard_normal((O.num_frames(n, cfg), NB)) + 1j * rng.standard_normal((O.num_frames(n, cfg), NB))) * scale).astype(np.complex64) for n in lengths]


@pytest.mark.parametrize("cfg", O.CFGS, ids=str)
def test_inverse_against_the_float64_oracle(cfg, dev):
    st = _st(cfg, dev)
    scale, bound = O.inverse_bound(cfg)
    lengths = _edge_lengths(st, cfg)
    specs = _random_specs(cfg, lengths, 11)
    got = _inverse(st, cfg, specs, lengths)
    worst = 0.0
    for b, n in enumerate(lengths):
        d = O.rel(got[b], O.istft(specs[b], n, cfg))
        worst = max(worst, d)
        assert d <= bound, (b, n, d, bound)
    print(f"\n{cfg}: inverse within {worst:.2e} of float64 (float32 restatement {scale:.2e}, bound {bound:.2e}: {worst / bound:.3f} of it) over S = {lengths}")
    H = cfg[0] // 2
    real_edges = [s.copy() for s in specs]
    for s in real_edges:
        assert s[:, 0].imag.any() and s[:, H].imag.any()
        s[:, 0], s[:, H] = s[:, 0].real, s[:, H].real
    again = _inverse(st, cfg, real_edges, lengths)
    for b in range(len(lengths)):
        assert np.array_equal(got[b].view(np.uint32), again[b].view(np.uint32)), b  # the imaginary parts of bins 0 and H change nothing
    pcm = _inverse(st, cfg, specs, lengths, pcm=True)
    for b in range(len(lengths)):
        assert np.array_equal(pcm[b], float_to_pcm16(got[b])), b  # PCM16 out is the library's one rule on the fp32 output (clipped: some samples lie past 1)
        assert np.abs(pcm[b].astype(np.int32)).max() > 1000


@pytest.mark.parametrize("cfg", O.CFGS, ids=str)
def test_forward_against_the_float64_oracle(cfg, dev):
    st = _st(cfg, dev)
    scale, bound = O.forward_bound(cfg)
    lengths = _edge_lengths(st, cfg)
    x = SO.make_speechlike(max(lengths), 71)
    rows = [x[:n].copy() for n in lengths]
    got = _forward(st, cfg, rows)
    worst = 0.0
    for b, r in enumerate(rows):
        want = O.stft(r, cfg)
        assert got[b].shape == want.shape, (b, got[b].shape, want.shape)
        d = O.rel(got[b], want)
        worst = max(worst, d)
        assert d <= bound, (b, len(r), d, bound)
    print(f"\n{cfg}: forward within {worst:.2e} of float64 (float32 restatement {scale:.2e}, bound {bound:.2e}: {worst / bound:.3f} of it) over S = {lengths}")


@pytest.mark.parametrize("res", [SO.RESOLUTIONS[n] for n in SO.N_FFTS] + [(1024, 1024, 256)], ids=str)
def test_forward_magnitude_is_the_spectral_meters_bit_for_bit(res, dev):
    """The two kernels that run the shared front (csrc/stft_front.h: stft_forward_k and spectral_frames_k) and the meter's floor held together:
    sqrt(max(re^2 + im^2, 1e-7)) of this output in separately rounded fp32 operations is SpectralMeter(mags=True)."""
    from viettts_amd.spectral import SpectralMeter

    cfg = res + ("center",)
    st = _st(cfg, dev)
    rows = [SO.case(i)[0] for i in (0, 3, 4)] + [RS.to_pcm16(SO.case(1)[0]).astype(np.float32) * np.float32(2.0 ** -15)]
    rows = [r for r in rows if len(r) >= O.min_samples(cfg)]
    got = _forward(st, cfg, rows)
    got16 = _forward(st, cfg, [RS.to_pcm16(r) for r in rows])
    meter = SpectralMeter(*res, device=dev)
    try:
        xs, lengths = _wav_batch(rows, 5, 3)
        xs = np.nan_to_num(xs, nan=0.0)
        mags = meter(xs, xs.copy(), lengths, mags=True).mags.cpu().numpy()
    finally:
        meter.close()
    for b, s in enumerate(got):
        z = torch.from_numpy(np.ascontiguousarray(s)).to(dev)
        re, im = z.real.contiguous(), z.imag.contiguous()
        m = torch.sqrt(torch.clamp(re * re + im * im, min=1e-7)).cpu().numpy()  # five torch operations on the device, each rounded on its own
        assert m.dtype == np.float32 and np.array_equal(m.view(np.uint32), mags[b, 0, : len(s)].view(np.uint32)), b
        m = np.sqrt(np.maximum(s.real * s.real + s.imag * s.imag, np.float32(1e-7)))  # ... and numpy's float32 on the host: IEEE
        assert m.dtype == np.float32 and np.array_equal(m.view(np.uint32), mags[b, 0, : len(s)].view(np.uint32)), b
    s16 = _forward(st, cfg, [RS.to_pcm16(r).astype(np.float32) * np.float32(2.0 ** -15) for r in rows])
    for b in range(len(rows)):
        assert np.array_equal(got16[b].view(np.uint32), s16[b].view(np.uint32)), b  # PCM16 in is the fp32 of the same values


def _round_trip_bound(cfg):
    """8 x the float32 restatement's round trip error over the oracle's rows, relative to the row's peak."""
    rows = [O.wave_case(i) for i in range(len(O.ROWS)) if O.ROWS[i][0] >= O.min_samples(cfg)]
    s = max(O.rel(O.istft(O.stft(x, cfg, f32=True), len(x), cfg, f32=True), x.astype(np.float64)) for x in rows)
    return s, O.BOUND_FACTOR * s


@pytest.mark.parametrize("cfg", O.CFGS, ids=str)
def test_round_trip(cfg, dev):
    st = _st(cfg, dev)
    scale, bound = _round_trip_bound(cfg)
    rows = [O.wave_case(i) for i in range(len(O.ROWS)) if O.ROWS[i][0] >= O.min_samples(cfg)]
    back = _inverse(st, cfg, _forward(st, cfg, rows), [len(x) for x in rows])
    worst = max(O.rel(y, x.astype(np.float64)) for x, y in zip(rows, back))
    print(f"\n{cfg}: inverse(forward(x)) within {worst:.2e} of x (float32 restatement {scale:.2e}, bound {bound:.2e}: {worst / bound:.3f} of it)")
    assert worst <= bound
    rows16 = [RS.to_pcm16(x) for x in rows]
    back16 = _inverse(st, cfg, _forward(st, cfg, rows16), [len(x) for x in rows16], pcm=True)
    differ = sum(int((a != b).sum()) for a, b in zip(rows16, back16))
    print(f"{cfg}: PCM16 -> spectrum -> PCM16: {differ} of {sum(len(x) for x in rows16)} samples differ")
    for a, b in zip(rows16, back16):
        assert np.abs(a.astype(np.int32) - b.astype(np.int32)).max() <= 1


@pytest.mark.parametrize("momentum", [0.0, 0.99])
@pytest.mark.parametrize("cfg", [O.CFGS[1], O.CFGS[2], O.CFGS[5], O.CFGS[6], O.CFGS[9]], ids=str)
def test_projection_against_the_float64_oracle(cfg, momentum, dev):
    st = _st(cfg, dev)
    lo = O.min_samples(cfg)
    rows = [O.wave_case(i) for i in range(len(O.ROWS)) if O.ROWS[i][0] >= lo][:3]
    mags = [np.abs(O.stft(SO.degrade(x, 3, 0.3), cfg)).astype(np.float32) for x in rows]
    tprevs = [O.stft(SO.degrade(x, 4, 0.1), cfg).astype(np.complex64) for x in rows]
    spec, tp = _forward(st, cfg, rows, project=(mags, tprevs, momentum))
    plain = _forward(st, cfg, rows)
    worst = 0.0
    for b, x in enumerate(rows):
        assert np.array_equal(tp[b].view(np.uint32), plain[b].view(np.uint32)), b  # tprev <- c, forward()'s bits
        want, c = O.project(x, mags[b], tprevs[b], momentum, cfg)
        a64 = c - O.alpha_of(momentum, False) * tprevs[b].astype(np.complex128)
        lim = O.project_limit(mags[b], a64, tprevs[b], c, cfg)
        d = np.abs(spec[b] - want)
        worst = max(worst, float((d / np.maximum(lim, 1e-300)).max()))
        assert (d <= lim).all(), (b, float((d / np.maximum(lim, 1e-300)).max()))  # no bin left out
        # on the magnitudes, whatever the phase: the root and the sum under it, the quotient and the product are 6 roundings at the most
        assert (np.abs(np.abs(spec[b].astype(np.complex128)) - mags[b]) <= 6 * 2.0 ** -24 * mags[b] + 1e-30).all()
    print(f"\n{cfg} momentum {momentum}: projection at most {worst:.3f} of its condition-aware limit")


def _same(a, b):
    return all(np.array_equal(np.ascontiguousarray(p).view(np.uint8), np.ascontiguousarray(q).view(np.uint8)) for p, q in zip(a, b)) and len(a) == len(b)


@pytest.mark.parametrize("cfg", [O.CFGS[0], O.CFGS[3], O.CFGS[5], O.CFGS[8]], ids=str)
def test_a_row_is_the_same_bits_alone_in_a_batch_and_at_any_stride(cfg, dev):
    st = _st(cfg, dev)
    _, _, run = st.blocking()
    lo = O.min_samples(cfg)
    lengths = [lo + 3, 2 * run + 77, run + cfg[2] + 1, lo + cfg[0]]
    x = SO.make_speechlike(max(lengths), 33)
    rows = [x[-n:].copy() for n in lengths]
    specs = _random_specs(cfg, lengths, 12)
    mags = [np.abs(s).astype(np.float32) for s in specs]
    tprevs = _random_specs(cfg, lengths, 13)
    f_a, i_a, p_a = _forward(st, cfg, rows), _inverse(st, cfg, specs, lengths), _forward(st, cfg, rows, project=(mags, tprevs, 0.99))
    f_w, i_w = _forward(st, cfg, rows, pad=1001, extra=7, seed=6), _inverse(st, cfg, specs, lengths, pad=1001, extra=7, seed=6)
    p_w = _forward(st, cfg, rows, pad=1001, extra=7, seed=6, project=(mags, tprevs, 0.99))
    assert _same(f_a, f_w) and _same(i_a, i_w) and _same(p_a[0], p_w[0]) and _same(p_a[1], p_w[1])  # a second stride, other junk
    for b in range(len(lengths)):
        one = slice(b, b + 1)
        assert _same(_forward(st, cfg, rows[one], pad=0, extra=0), f_a[one]), b  # alone
        assert _same(_inverse(st, cfg, specs[one], lengths[one], pad=0, extra=0), i_a[one]), b
        sp, tp = _forward(st, cfg, rows[one], pad=0, extra=0, project=(mags[one], tprevs[one], 0.99))
        assert _same(sp, p_a[0][one]) and _same(tp, p_a[1][one]), b


def test_rows_behind_the_launch_split(dev):
    """STFT_ROWS_PER_LAUNCH + 1 = 129 tiny rows of different lengths: every stage's rows behind the split are the rows alone, bit for bit."""
    cfg = O.CFGS[0]
    st = _st(cfg, dev)
    N = _lib.STFT_ROWS_PER_LAUNCH + 1
    lo = O.min_samples(cfg)
    lengths = [lo + (37 * b) % 301 for b in range(N)]
    lengths[-1] = lo + 301  # the longest, strictly, lies behind the split: the grid is the second launch's
    assert lengths[-1] > max(lengths[:-1])
    x = SO.make_speechlike(max(lengths) + N, 44)
    rows = [x[b : b + n].copy() for b, n in enumerate(lengths)]
    specs = _random_specs(cfg, lengths, 14)
    mags, tprevs = [np.abs(s).astype(np.float32) for s in specs], _random_specs(cfg, lengths, 15)
    f, i = _forward(st, cfg, rows), _inverse(st, cfg, specs, lengths)
    sp, tp = _forward(st, cfg, rows, project=(mags, tprevs, 0.99))
    for b in (0, 127, 128):
        one = slice(b, b + 1)
        assert _same(_forward(st, cfg, rows[one]), f[one]) and _same(_inverse(st, cfg, specs[one], lengths[one]), i[one]), b
        s1, t1 = _forward(st, cfg, rows[one], project=(mags[one], tprevs[one], 0.99))
        assert _same(s1, sp[one]) and _same(t1, tp[one]), b
        assert O.rel(f[b], O.stft(rows[b], cfg)) <= O.forward_bound(cfg)[1] and O.rel(i[b], O.istft(specs[b], lengths[b], cfg)) <= O.inverse_bound(cfg)[1], b


# ------------------------------------------------------------ Griffin-Lim ------------------------------------------------------------
GL_CASES = (((512, 240, 50, "center"), 6000), ((1024, 1024, 256, "mel"), 6144), ((256, 256, 64, "center"), 6000))
GL_SEEDS = (1, 2, 3)  # several rows, so that a scale is not one draw


def _gl_inputs(cfg, S):
    xs = [SO.make_speechlike(S, 20 + s) for s in GL_SEEDS]
    mags = [np.abs(O.stft(x, cfg)).astype(np.float32) for x in xs]
    rng = np.random.default_rng(99)
    inits = [np.exp(2j * np.pi * rng.random(m.shape)).astype(np.complex64) for m in mags]
    return xs, mags, inits


def _gl_gpu(st, mags, inits, n_iter, S=None):
    from viettts_amd.stft import GriffinLim

    mg, it = torch.from_numpy(np.stack(mags)).to(st.device), torch.from_numpy(np.stack(inits)).to(st.device)
    return GriffinLim(st, n_iter=n_iter, momentum=0.99)(mg, lengths=None if S is None else [S] * len(mags), init=it)


@pytest.mark.parametrize("cfg,S", GL_CASES, ids=str)
def test_griffin_lim_4_iterations_against_the_float64_oracle(cfg, S, dev):
    st = _st(cfg, dev)
    xs, mags, inits = _gl_inputs(cfg, S)
    want = [O.griffinlim(m, S, cfg, 4, 0.99, i) for m, i in zip(mags, inits)]
    scale = max(O.rel(O.griffinlim(m, S, cfg, 4, 0.99, i, f32=True), w) for m, i, w in zip(mags, inits, want))
    got = _gl_gpu(st, mags, inits, 4, S).cpu().numpy()
    worst = max(O.rel(got[b], want[b]) for b in range(len(xs)))
    print(f"\n{cfg}: 4 iterations within {worst:.2e} of float64 (float32 restatement {scale:.2e}, bound {O.BOUND_FACTOR * scale:.2e}: {worst / (O.BOUND_FACTOR * scale):.3f} of it)")
    assert got.shape == (len(xs), S) and worst <= O.BOUND_FACTOR * scale


@pytest.mark.parametrize("cfg,S", GL_CASES, ids=str)
def test_griffin_lim_32_iterations_converge_as_the_float64_oracle(cfg, S, dev):
    from viettts_amd.spectral import SpectralMeter

    st = _st(cfg, dev)
    xs, mags, inits = _gl_inputs(cfg, S)
    res = cfg[:3]
    want = [O.griffinlim(m, S, cfg, 32, 0.99, i) for m, i in zip(mags, inits)]
    f32 = [O.griffinlim(m, S, cfg, 32, 0.99, i, f32=True) for m, i in zip(mags, inits)]
    sc64 = [SO.measure(x, w.astype(np.float32), res).sc for x, w in zip(xs, want)]
    sc32 = [SO.measure(x, w.astype(np.float32), res).sc for x, w in zip(xs, f32)]
    scale = max(abs(a - b) for a, b in zip(sc32, sc64))
    got, start = _gl_gpu(st, mags, inits, 32, S), _gl_gpu(st, mags, inits, 0, S)
    meter = SpectralMeter(*res, device=dev)
    try:
        ref = torch.from_numpy(np.stack(xs)).to(dev)
        sc, sc0 = meter(ref, got).sc.cpu().numpy(), meter(ref, start).sc.cpu().numpy()
    finally:
        meter.close()
    for b in range(len(xs)):
        print(f"\n{cfg} row {b}: spectral convergence {sc0[b]:.4f} -> {sc[b]:.6f} after 32 iterations; float64 oracle {sc64[b]:.6f}, float32 restatement {sc32[b]:.6f}; "
              f"|d| {abs(sc[b] - sc64[b]):.2e} against the bound {O.BOUND_FACTOR * scale:.2e}")
    for b in range(len(xs)):
        assert sc[b] < sc0[b], b
        assert abs(sc[b] - sc64[b]) <= O.BOUND_FACTOR * scale, (b, sc[b], sc64[b], scale)
    # the class is the hand-written loop of inverse() and project(), bit for bit
    mg, spec = torch.from_numpy(np.stack(mags)).to(dev), torch.from_numpy(np.stack(mags) * np.stack(inits)).to(dev)
    tprev = torch.zeros_like(spec)
    for _ in range(32):
        spec = st.project(st.inverse(spec, [S] * len(xs)), mg, tprev, [S] * len(xs), momentum=0.99)
    assert torch.equal(st.inverse(spec, [S] * len(xs)), got)


def test_mel2wave_griffinlim_shapes_alignment_and_rows(dev):
    from viettts_amd.resynth import default_mel_filter
    from viettts_amd.stft import mel2wave_griffinlim, mel_to_linear

    mf = default_mel_filter(dev)
    x = np.stack([SO.make_speechlike(6144, 50), SO.make_speechlike(6144, 51)])
    mel = mf(torch.from_numpy(x).to(dev))
    assert tuple(mel.shape) == (2, 24, 80)
    mag = mel_to_linear(mel, mf)
    assert tuple(mag.shape) == (2, 24, 513) and float(mag.min()) >= 0.0 and torch.isfinite(mag).all()
    wav = mel2wave_griffinlim(mel, n_iter=8)
    assert tuple(wav.shape) == (2, 6144) and wav.dtype == torch.float32 and torch.isfinite(wav).all() and float(wav.abs().max()) > 0.01
    assert tuple(mf(wav).shape) == (2, 24, 80)  # sample-aligned with the mel it came from
    assert torch.equal(mel2wave_griffinlim(mel[1:], n_iter=8)[0], wav[1])  # a row is the row alone
    assert tuple(mel2wave_griffinlim(mel[0].cpu().numpy(), n_iter=1).shape) == (1, 6144)  # [T, 80] numpy in


def test_python_class_refusals_and_the_command_line(dev, tmp_path, capsys):
    from viettts_amd import stft as M
    from viettts_amd import wavio

    with pytest.raises(_lib.VttsError, match="hop 256") as e:
        M.Stft(256, 256, 256, device=dev).inverse(torch.zeros((1, 5, 129), dtype=torch.complex64, device=dev))
    assert e.value.status == -1 and "256 samples" in str(e.value)  # NOLA: the message names the window and the hop
    st = _st(O.CFGS[0], dev)
    with pytest.raises(ValueError, match="complex64"):
        st.inverse(torch.zeros((1, 5, 129), dtype=torch.float32, device=dev))
    with pytest.raises(ValueError, match="init"):
        M.GriffinLim(st)(torch.ones((1, 5, 129), device=dev), init=torch.ones((1, 4, 129), dtype=torch.complex64, device=dev))
    a = M.GriffinLim(st, 2)(torch.ones((1, 9, 129), device=dev), seed=3)
    assert torch.equal(a, M.GriffinLim(st, 2)(torch.ones((1, 9, 129), device=dev), seed=3)) and not torch.equal(a, M.GriffinLim(st, 2)(torch.ones((1, 9, 129), device=dev), seed=4))
    mel = np.log(np.full((12, 80), 0.01, np.float32))
    np.save(tmp_path / "m.npy", mel)
    M.main(["--mel-file", str(tmp_path / "m.npy"), "--output", str(tmp_path / "o.wav"), "--n-iter", "2"])
    sr, pcm = wavio.read_wav(tmp_path / "o.wav")
    assert sr == 16000 and len(pcm) == 12 * 256 and "12 frames" in capsys.readouterr().out


def test_resynth_and_synthesizer_with_the_griffin_lim_vocoder_open_no_checkpoint(dev, tmp_path, capsys, monkeypatch):
    from viettts_amd import resynth, synthesizer, wavio
    from viettts_amd.hifigan import mel2wave

    def refuse(*a, **k):
        raise AssertionError("the HiFi-GAN generator is not opened with --vocoder griffinlim")

    monkeypatch.setattr(mel2wave, "_generator", refuse)
    x = SO.make_speechlike(24000 + 100, 60)
    wavio.write_wav_pcm16(tmp_path / "in.wav", RS.to_pcm16(x), 16000)
    resynth.main(["--input", str(tmp_path / "in.wav"), "--output", str(tmp_path / "out.wav"), "--vocoder", "griffinlim", "--mrstft", "--stoi", "--f0"])
    out = capsys.readouterr().out
    sr, pcm = wavio.read_wav(tmp_path / "out.wav")
    n = 256 * (len(x) // 256)
    assert sr == 16000 and len(pcm) == n and np.abs(pcm.astype(np.int32)).max() > 1000
    assert f"{n} samples" in out and "multi-resolution STFT distance" in out and "STOI" in out and "F0" in out
    mel = resynth.wav2mel(torch.from_numpy(RS.to_pcm16(x)[None, :]).to(dev))[0].cpu().numpy()  # the mel resynth made of the file
    np.save(tmp_path / "m.npy", mel)
    assert synthesizer.main(["--mel-file", str(tmp_path / "m.npy"), "--vocoder", "griffinlim", "--output", str(tmp_path / "s.wav")]) == 0
    sr, pcm2 = wavio.read_wav(tmp_path / "s.wav")
    assert sr == 16000 and len(pcm2) == n and np.array_equal(pcm2, pcm)  # the same mel, the same seed: the same samples from either command line
