"""The fused denoiser (viettts_amd/csrc/denoise.hip, include/vtts_denoise.h) on the GPU: against the float64 restatement of the contract
(tests/_denoise_oracle.py) within 8 x the distance of the oracle's float32 mode from its float64 mode over the oracle's rows
(tests/test_denoise_cpu.py prints the scales and shows that every planted fault misses the bound), and == against
``Stft.inverse(gain_f32(Stft.forward(x)))``, which the header calls equal.  Every batch is ragged, with NaN and noise at 1e4 past each row's
samples; every call goes through the C ABI into NaN-filled (int16: canary-filled) outputs of another stride."""
import ctypes as C

import numpy as np
import pytest
import torch

import _denoise_oracle as D
import _row_split as RS
import _spectral_oracle as SO
import _stft_oracle as O
from viettts_amd import _lib
from viettts_amd._handle import ptr
from viettts_amd.wavio import float_to_pcm16

pytestmark = pytest.mark.gpu
_HANDLES = {}
CANARY16 = -12345
FOUR = [O.CFGS[0], O.CFGS[3], O.CFGS[5], O.CFGS[8]]  # all four transform lengths, both framings, win == n_fft and win < n_fft
assert sorted(c[0] for c in FOUR) == [256, 512, 1024, 2048] and {c[3] for c in FOUR} == {"center", "mel"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    yield torch.device("cuda:0")
    for st, dn in _HANDLES.values():
        dn.close()
        st.close()
    _HANDLES.clear()


def _pair(cfg, dev):
    """(Stft, Denoiser) of a config: the denoiser binds the transform's blob."""
    from viettts_amd.denoise import Denoiser
    from viettts_amd.stft import Stft

    if cfg not in _HANDLES:
        st = Stft(*cfg[:3], framing=cfg[3], device=dev)
        dn = Denoiser(st)
        dn._tables()
        assert dn.packed_blob().data_ptr() == st.packed_blob().data_ptr()
        _HANDLES[cfg] = (st, dn)
    return _HANDLES[cfg]


def _junk(rng, shape, dtype):
    if dtype == np.int16:
        return rng.integers(-30000, 30000, shape).astype(np.int16)
    j = (1e4 * rng.standard_normal(shape)).astype(np.float32)
    j.reshape(-1)[::3] = np.nan
    return j


def _apply(dn, rows, bias, strength=D.STRENGTH, pad=37, out_pad=5, seed=5, pcm=False):
    """apply() through the C ABI -> per row its S_b samples.  NaN and noise behind every row's samples; the sentinel past them is checked here."""
    lengths = [len(x) for x in rows]
    xs = _junk(np.random.default_rng(seed), (len(rows), max(lengths) + pad), rows[0].dtype)
    for b, x in enumerate(rows):
        xs[b, : len(x)] = x
    N, S = xs.shape
    So = max(lengths) + out_pad
    xt = torch.from_numpy(xs).to(dn.device)
    bt = torch.from_numpy(np.ascontiguousarray(bias, dtype=np.float32)).to(dn.device)
    out = torch.full((N, So), CANARY16, dtype=torch.int16, device=dn.device) if pcm else torch.full((N, So), float("nan"), dtype=torch.float32, device=dn.device)
    dn._on_stream("apply", ptr(xt), _lib.VTTS_AUDIO_PCM16 if xs.dtype == np.int16 else _lib.VTTS_AUDIO_F32, N, S, (C.c_int32 * N)(*lengths), ptr(bt), C.c_float(strength),
                  ptr(out), _lib.VTTS_AUDIO_PCM16 if pcm else _lib.VTTS_AUDIO_F32, So)
    torch.cuda.synchronize(dn.device)
    got = out.cpu().numpy()
    for b, n in enumerate(lengths):
        assert (got[b, n:] == CANARY16).all() if pcm else np.isnan(got[b, n:]).all(), b  # nothing is written past lengths[b]
        assert pcm or np.isfinite(got[b, :n]).all(), b
    return [got[b, :n] for b, n in enumerate(lengths)]


def _composed(st, rows, bias, strength=D.STRENGTH, pcm=False):
    """Stft.inverse(gain_f32(Stft.forward(x))) per row: the two kernels of vtts_stft.h with numpy's float32 between them."""
    lengths = [len(x) for x in rows]
    xs = np.zeros((len(rows), max(lengths)), rows[0].dtype)
    for b, x in enumerate(rows):
        xs[b, : len(x)] = x
    spec = st.forward(torch.from_numpy(xs).to(st.device), lengths).cpu().numpy()
    for b, n in enumerate(lengths):
        T = O.num_frames(n, (st.n_fft, st.win, st.hop, st.framing))
        spec[b, :T] = D.gain_f32(spec[b, :T], bias, strength)
    y = st.inverse(torch.from_numpy(spec).to(st.device), lengths, out_dtype="pcm16" if pcm else "f32").cpu().numpy()
    return [y[b, :n] for b, n in enumerate(lengths)]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(np.ascontiguousarray(p).view(np.uint8), np.ascontiguousarray(q).view(np.uint8)) for p, q in zip(a, b))


@pytest.mark.parametrize("cfg", O.CFGS, ids=str)
def test_against_the_float64_oracle(cfg, dev):
    _, dn = _pair(cfg, dev)
    scale, bound = D.bound(cfg)
    idx = D.rows(cfg)
    bias = D.smooth_bias(cfg)
    rows = [O.wave_case(i) for i in idx]
    got = _apply(dn, rows, bias)
    rows16 = [RS.to_pcm16(x) for x in rows]
    got16 = _apply(dn, rows16, bias)
    worst = worst16 = 0.0
    for b, i in enumerate(idx):
        worst = max(worst, O.rel(got[b], D.want(i, cfg)))
        worst16 = max(worst16, O.rel(got16[b], D.denoise(rows16[b], bias, D.STRENGTH, cfg)))
    print(f"\n{cfg}: fused denoise within {worst:.2e} (PCM16 in: {worst16:.2e}) of float64 (float32 restatement {scale:.2e}, bound {bound:.2e}: "
          f"{worst / bound:.3f} and {worst16 / bound:.3f} of it)")
    assert worst <= bound and worst16 <= bound
    as_f32 = _apply(dn, [SO.as_float32(x) for x in rows16], bias)
    assert _same(got16, as_f32)  # PCM16 in is the fp32 of the same values


@pytest.mark.parametrize("cfg", FOUR, ids=str)
def test_bit_for_bit_the_composition_of_forward_gain_and_inverse(cfg, dev):
    st, dn = _pair(cfg, dev)
    bias = D.smooth_bias(cfg)
    rows = [O.wave_case(i) for i in D.rows(cfg)]
    got, want = _apply(dn, rows, bias), _composed(st, rows, bias)
    assert _same(got, want)
    assert all(np.abs(g).max() > 1e-3 for g in got)
    got16, want16 = _apply(dn, rows, bias, pcm=True), _composed(st, rows, bias, pcm=True)
    assert _same(got16, want16) and _same(got16, [float_to_pcm16(g) for g in got])  # the library's one PCM16 rule on the fp32 output
    assert all(np.abs(g.astype(np.int32)).max() > 100 for g in got16)


@pytest.mark.parametrize("cfg", FOUR, ids=str)
def test_run_and_walk_edges_bit_for_bit(cfg, dev):
    """The lengths at which t_lo, t_hi, the reflected reads at both ends and the last partial round flip."""
    st, dn = _pair(cfg, dev)
    W, run = dn.blocking()
    lo = O.min_samples(cfg)
    lengths = [run - 1, run, run + 1, 2 * run + 1, lo]  # run + 1 and 2 run + 1: the last run holds a single sample
    lengths = sorted({n for n in lengths if n >= lo})
    assert lo in lengths and any(n % run == 1 for n in lengths)
    x = SO.make_speechlike(max(lengths), 71)
    rows = [x[-n:].copy() for n in lengths]
    bias = D.smooth_bias(cfg)
    got, want = _apply(dn, rows, bias), _composed(st, rows, bias)
    for b, n in enumerate(lengths):
        assert np.array_equal(got[b].view(np.uint32), want[b].view(np.uint32)), (n, int((got[b] != want[b]).sum()))
    d = max(O.rel(got[b], D.denoise(rows[b], bias, D.STRENGTH, cfg)) for b in range(len(rows)))
    print(f"\n{cfg}: W {W}, run {run}; S = {lengths} within {d:.2e} of float64 (the oracle rows' bound is {D.bound(cfg)[1]:.2e})")


@pytest.mark.parametrize("cfg", FOUR, ids=str)
def test_a_row_is_the_same_bits_alone_in_a_batch_and_at_any_stride(cfg, dev):
    _, dn = _pair(cfg, dev)
    _, run = dn.blocking()
    lo = O.min_samples(cfg)
    lengths = [lo + 3, 2 * run + 77, run + cfg[2] + 1, lo + cfg[0]]
    x = SO.make_speechlike(max(lengths), 33)
    rows = [x[-n:].copy() for n in lengths]
    bias = D.smooth_bias(cfg)
    a = _apply(dn, rows, bias)
    assert _same(a, _apply(dn, rows, bias, pad=1001, out_pad=333, seed=6))  # another stride on either side, other junk past the rows
    for b in range(len(rows)):
        assert _same(_apply(dn, rows[b : b + 1], bias, pad=0, out_pad=0), a[b : b + 1]), b  # alone


def test_rows_behind_the_launch_split(dev):
    """DENOISE_ROWS_PER_LAUNCH + 1 = 129 rows of the shortest accepted length: row 128 is the row alone, bit for bit."""
    cfg = O.CFGS[0]
    st, dn = _pair(cfg, dev)
    N = _lib.DENOISE_ROWS_PER_LAUNCH + 1
    lo = O.min_samples(cfg)
    x = SO.make_speechlike(lo + N, 44)
    rows = [x[b : b + lo].copy() for b in range(N)]
    bias = D.smooth_bias(cfg)
    got = _apply(dn, rows, bias)
    for b in (0, 127, 128):
        assert _same(_apply(dn, rows[b : b + 1], bias), got[b : b + 1]), b
    assert not _same(got[127:128], got[128:129])


@pytest.mark.parametrize("cfg", FOUR, ids=str)
def test_limits_silence_and_the_round_trip(cfg, dev):
    _, dn = _pair(cfg, dev)
    rows = [O.wave_case(i) for i in D.rows(cfg)]
    for pcm in (False, True):
        assert all(not y.any() for y in _apply(dn, rows, D.clamping_bias(cfg), pcm=pcm))  # every bin clamps: exact zeros
    scale, bound = D.round_trip_bound(cfg)
    for bias, s in ((D.smooth_bias(cfg), 0.0), (D.zero_bias(cfg), D.STRENGTH)):
        worst = max(O.rel(y, x.astype(np.float64)) for x, y in zip(rows, _apply(dn, rows, bias, strength=s)))
        print(f"\n{cfg}: strength {s}: within {worst:.2e} of the input (float32 round trip {scale:.2e}, bound {bound:.2e}: {worst / bound:.3f} of it)")
        assert worst <= bound


def test_python_class_paths_and_refusals(dev):
    from viettts_amd.denoise import Denoiser

    cfg = O.CFGS[4]
    st, dn = _pair(cfg, dev)
    idx = D.rows(cfg)
    rows = [O.wave_case(i) for i in idx]
    lengths = [len(x) for x in rows]
    xs = np.zeros((len(rows), max(lengths)), np.float32)
    for b, x in enumerate(rows):
        xs[b, : len(x)] = x
    bias = D.smooth_bias(cfg)
    dn.set_bias(bias)
    y = dn(xs, lengths, strength=D.STRENGTH)
    assert y.shape == xs.shape and y.dtype == torch.float32 and _same([y.cpu().numpy()[b, :n] for b, n in enumerate(lengths)], _apply(dn, rows, bias))
    assert not y.cpu().numpy()[0, lengths[0]:].any()  # zero past a row's own samples
    y16 = dn(torch.from_numpy(xs).to(dev), lengths, strength=D.STRENGTH, out_dtype="pcm16")
    assert y16.dtype == torch.int16 and np.array_equal(y16.cpu().numpy(), float_to_pcm16(y.cpu().numpy()))
    comp = dn.composed(xs, lengths, strength=D.STRENGTH)
    worst = max(O.rel(comp.cpu().numpy()[b, :n], y.cpu().numpy()[b, :n].astype(np.float64)) for b, n in enumerate(lengths))
    print(f"\n{cfg}: composed() within {worst:.2e} of the fused kernel (2 x bound = {2 * D.bound(cfg)[1]:.2e})")
    assert comp.shape == y.shape and worst <= 2 * D.bound(cfg)[1]
    assert torch.equal(Denoiser(cfg, bias=bias, strength=D.STRENGTH, device=dev)(xs, lengths), y)  # its own Stft, the default strength
    # the noise recording's mean magnitude
    got = dn.bias_from_noise(xs, lengths).cpu().numpy()
    spec = st.forward(torch.from_numpy(xs).to(dev), lengths).cpu().numpy()
    want = D.bias_from_noise([spec[b, : O.num_frames(n, cfg)] for b, n in enumerate(lengths)], cfg)
    assert got.dtype == np.float32 and np.abs(got - want).max() <= 2.0 ** -20 * np.abs(want).max() and (np.abs(got - want) <= 2.0 ** -20 * want).all()
    dn.set_bias(bias)
    # refusals
    xt = torch.from_numpy(xs).to(dev)
    with pytest.raises(ValueError, match="must not overlap"):
        dn(xt, lengths, out=xt)
    buf = torch.zeros(xt.numel() + 8, device=dev)
    with pytest.raises(ValueError, match="must not overlap"):
        dn(buf[: xt.numel()].view_as(xt), lengths, out=buf[8:].view_as(xt))
    h_out = torch.zeros_like(xt)
    rc = dn.lib.vtts_denoise_apply(dn._h, ptr(xt), 0, xt.shape[0], xt.shape[1], None, ptr(dn.bias), 0.5, C.c_void_p(xt.data_ptr() + 4 * xt.numel() - 4), 0, xt.shape[1], None)
    assert rc == -1 and b"must not overlap wav_dev" in dn.lib.vtts_last_error() and not h_out.any()
    with pytest.raises(ValueError, match="strength"):
        dn(xt, lengths, strength=-0.01)
    with pytest.raises(ValueError, match="strength"):
        dn(xt, lengths, strength=float("inf"))
    for bad, word in ((bias[:-1], "one per bin"), (-bias, "not negative"), (np.where(np.arange(len(bias)) == 3, np.nan, bias), "finite")):
        with pytest.raises(ValueError, match=word):
            dn.set_bias(bad)
    with pytest.raises(ValueError, match="out_dtype"):
        dn(xt, lengths, out_dtype="f16")
    with pytest.raises(RuntimeError, match="no bias"):
        Denoiser(st)(xt, lengths)
    with pytest.raises(_lib.VttsError, match="hop 256") as e:
        Denoiser((256, 256, 256, "center"), bias=np.ones(129, np.float32), device=dev)(torch.zeros((1, 1000), device=dev))
    assert e.value.status == -1 and "NOLA" in str(e.value)
    with pytest.raises(_lib.VttsError, match="pad \\+ 1"):
        dn(xt[:, :100].contiguous())
    h = C.c_void_p(0)  # before pack() / bind_packed()
    assert dn.lib.vtts_denoise_create(C.byref(_lib.StftCfg(*cfg[:3], 0)), 0, C.byref(h)) == 0
    assert dn.lib.vtts_denoise_apply(h, ptr(xt), 0, 1, xt.shape[1], None, ptr(dn.bias), 0.5, ptr(h_out), 0, xt.shape[1], None) == -2 and b"before pack" in dn.lib.vtts_last_error()
    blob = torch.empty(dn.packed_bytes, dtype=torch.uint8, device=dev)  # ... and its own pack() gives the Stft's blob, byte for byte
    assert dn.lib.vtts_denoise_pack(h, ptr(blob), blob.numel(), None) == 0 and torch.equal(blob, st.packed_blob()[: blob.numel()])
    assert dn.lib.vtts_denoise_apply(h, ptr(xt), 0, 1, xt.shape[1], None, ptr(dn.bias), C.c_float(D.STRENGTH), ptr(h_out), 0, xt.shape[1], None) == 0
    torch.cuda.synchronize(dev)
    assert torch.equal(h_out[0], dn(xt[:1].contiguous(), strength=D.STRENGTH)[0])
    dn.lib.vtts_denoise_destroy(h)


def test_bias_from_generator_is_frame_0_of_the_empty_mels_spectrum(dev):
    from viettts_amd.denoise import Denoiser
    from viettts_amd.hifigan.config import TINY
    from viettts_amd.hifigan.generator import Generator
    from viettts_amd.hifigan.synth import synthetic_params

    gen = Generator(TINY, device=dev)  # the fp32 engine, a small config
    gen.load_params(synthetic_params(TINY, 4321, "scaled"))
    dn = Denoiser((512, 512, 128, "center"), device=dev)
    try:
        for fill in (0.0, -4.0):
            b = dn.bias_from_generator(gen, frames=12, fill=fill)
            wav = gen(torch.full((1, 12, TINY.num_mels), fill, dtype=torch.float32, device=dev))
            c = dn.stft.forward(wav).cpu().numpy()[0, 0]
            re_, im = np.ascontiguousarray(c.real), np.ascontiguousarray(c.imag)
            want = np.sqrt(re_ * re_ + im * im)
            assert want.dtype == np.float32 and b.shape == (257,) and np.array_equal(b.cpu().numpy().view(np.uint32), want.view(np.uint32)), fill
            assert want.max() > 0.0 and dn.bias is b
            assert dn.bias_from_generator(gen, frames=12, fill=fill) is b  # cached on the object
        assert dn.bias_from_generator(gen, frames=12, fill=0.0) is not b
    finally:
        dn.close()
        gen.close()


def test_pipeline_denoise_is_off_by_default_and_is_the_denoiser_behind_the_generator(dev):
    """Three sentences of the synthetic models the pipeline tests use.  ``denoise=None`` is the call without the argument, bit for bit; with
    ``denoise=S`` every sentence is ``Denoiser(bias of this generator)(the generator's output)``, bit for bit."""
    from viettts_amd.denoise import Denoiser
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
    dn = Denoiser(device=dev)
    try:
        rng = np.random.default_rng(41)
        sents = [[FLAGS.sil_index] + list(rng.integers(4, 90, size=n)) + [FLAGS.sil_index] for n in (24, 40, 33)]
        base = synthesize_sentences(sents, dm, am, gen, silence_duration=0.05)
        base = {i: base[i].copy() for i in base}
        off = synthesize_sentences(sents, dm, am, gen, silence_duration=0.05, denoise=None)
        assert sorted(off) == [0, 1, 2] and all(np.array_equal(off[i].view(np.uint32), base[i].view(np.uint32)) for i in base)
        s = 0.5
        on = synthesize_sentences(sents, dm, am, gen, silence_duration=0.05, denoise=s)
        on = {i: on[i].copy() for i in on}
        pcm = synthesize_sentences(sents, dm, am, gen, silence_duration=0.05, denoise=s, out_dtype="pcm16")
        dn.bias_from_generator(gen)
        assert float(dn.bias.max()) > 0.0
        for i in range(3):
            want = dn(base[i][None, :], strength=s).cpu().numpy()[0]
            assert on[i].dtype == np.float32 and np.array_equal(on[i].view(np.uint32), want.view(np.uint32)), i
            assert not np.array_equal(on[i], base[i]) and np.array_equal(pcm[i], float_to_pcm16(on[i])), i
        with pytest.raises(ValueError, match="strength"):
            synthesize_sentences(sents, dm, am, gen, denoise=-1.0)
    finally:
        dn.close()
        gen.close()
        dm.close()
        am.close()


def test_command_line_subtracts_the_room_tone(dev, tmp_path, capsys):
    from viettts_amd import denoise, wavio

    rng = np.random.default_rng(9)
    S = 24000
    hiss = 0.01 * rng.standard_normal(S).astype(np.float32)
    x = hiss.copy()
    x[8000:] += SO.make_speechlike(S - 8000, 60)
    wavio.write_wav_pcm16(tmp_path / "in.wav", RS.to_pcm16(x), 16000)
    denoise.main(["--wav", str(tmp_path / "in.wav"), "--noise-from", "0:0.5", "--strength", "2.0", "--output", str(tmp_path / "out.wav")])
    sr, pcm = wavio.read_wav(tmp_path / "out.wav")
    assert sr == 16000 and len(pcm) == S and "8000 samples of room tone" in capsys.readouterr().out
    quiet = lambda p: float(np.sqrt(np.mean(p[1000:7000].astype(np.float64) ** 2)))  # noqa: E731
    assert quiet(pcm) < 0.5 * quiet(RS.to_pcm16(x)) and np.abs(pcm[8000:].astype(np.int32)).max() > 3000  # the tone's stretch is quieter, the speech is still there


def test_resynth_takes_the_room_tone_out_of_the_input_with_no_checkpoint(dev, tmp_path, capsys):
    from viettts_amd import resynth, wavio

    rng = np.random.default_rng(10)
    S = 12000
    x = 0.01 * rng.standard_normal(S).astype(np.float32)
    x[6000:] += SO.make_speechlike(S - 6000, 61)
    wavio.write_wav_pcm16(tmp_path / "in.wav", RS.to_pcm16(x), 16000)
    resynth.main(["--input", str(tmp_path / "in.wav"), "--output", str(tmp_path / "out.wav"), "--vocoder", "griffinlim", "--denoise", "2.0", "--noise-from", "0:0.3"])
    sr, pcm = wavio.read_wav(tmp_path / "out.wav")
    n = 256 * (S // 256)
    assert sr == 16000 and len(pcm) == n and f"{n} samples" in capsys.readouterr().out and np.abs(pcm.astype(np.int32)).max() > 1000
