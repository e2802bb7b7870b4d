"""include/vtts_denoise.h without a GPU: the numpy restatement (tests/_denoise_oracle.py) against a torch.stft / torch.istft composition, its
own limits (no bias: the round trip; a bias above every bin: silence), the bound the GPU test uses with every planted fault missing it, the
host entry points of the built library, and the command lines' argument errors."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import _denoise_oracle as D
import _spectral_oracle as SO
import _stft_oracle as O
from viettts_amd import _lib

REPO = Path(__file__).resolve().parents[1]
CENTER = [c for c in O.CFGS if c[3] == "center"]


@pytest.fixture(scope="module")
def lib():
    from viettts_amd.csrc.build import build

    build()
    return _lib.load()


def _torch_window(cfg):
    n_fft, win, _, _ = cfg
    lead = (n_fft - win) // 2
    return torch.from_numpy(O.window(cfg)[lead : lead + win].astype(np.float64))


def test_header_exports_and_constants(lib):
    header = D.HEADER.read_text()
    declared = set(re.findall(r"\b(vtts_denoise_[a-z_0-9]+)\s*\(", header))
    assert declared == set(_lib.DENOISE_EXPORTS) == {f"vtts_denoise_{n}" for n in ("create", "destroy", "blocking", "packed_bytes", "pack", "bind_packed", "apply")}
    for name in declared:
        assert hasattr(lib, name), name
    assert not set(_lib.DENOISE_SIGS) & (set(_lib.SIGS) | set(_lib.STFT_SIGS) | set(_lib.SPECTRAL_SIGS))
    k, ks = D.header_constants(), O.header_constants()
    assert int(k["VTTS_DENOISE_MAX_SAMPLES"]) == _lib.DENOISE_MAX_SAMPLES == int(ks["VTTS_STFT_MAX_SAMPLES"])
    assert int(k["VTTS_DENOISE_ROWS_PER_LAUNCH"]) == _lib.DENOISE_ROWS_PER_LAUNCH == 128
    assert float(k["VTTS_DENOISE_NOLA_FLOOR"]) == _lib.DENOISE_NOLA_FLOOR == float(ks["VTTS_STFT_NOLA_FLOOR"])
    text = (REPO / "viettts_amd" / "csrc" / "denoise.hip").read_text()
    assert re.findall(r"^constexpr int (ROWS_PER_LAUNCH) = (\d+);", text, flags=re.M) == [("ROWS_PER_LAUNCH", str(_lib.DENOISE_ROWS_PER_LAUNCH))]
    assert len(re.findall(r"for_each_launch(?:_off)?<ROWS_PER_LAUNCH>\(", text)) == 1 and len(re.findall(r"\+= ROWS_PER_LAUNCH\)", text)) == 0
    assert "#pragma clang fp contract(off)" in text and text.index("#pragma clang fp contract(off)") < text.index('#include "stockham.h"')
    assert not re.search(r"atomic(Add|Max|Min|CAS|Exch)|__hip_atomic", text) and not re.search(r"\b(sinf?|cosf?|sincosf?)\s*\(", text)
    for word in ("contract", "blocking", "LDS", "bit for bit"):  # the header states the contract, the blocking and the LDS formula
        assert word in header, word
    from viettts_amd.csrc import build

    assert "denoise.hip" in build.SOURCES and "stft_back.h" in build.HEADERS and any(str(h).endswith("vtts_denoise.h") for h in build.HEADERS)
    assert build.FILE_FLAGS["denoise.hip"] == build.FILE_FLAGS["stft.hip"]


def test_create_accepts_and_refuses_what_the_stft_does(lib):
    h, s = C.c_void_p(0), C.c_void_p(0)
    bad = [(128, 64, 16, 0), (4096, 1024, 256, 0), (1000, 600, 120, 1), (1024, 600, 0, 0), (1024, 600, -1, 0), (1024, 100, 120, 0), (1024, 1025, 120, 0), (512, 600, 120, 1),
           (1024, 1024, 256, -1), (1024, 1024, 256, 2), (1024, 600, 121, 1)]
    good = [(256, 1, 1, 0), (256, 256, 256, 0), (2048, 2048, 2048, 1), (2048, 2048, 2, 1), (1024, 1024, 256, 1), (512, 240, 50, 1), (1024, 600, 121, 0)]
    for cfg in bad + good:
        rc = lib.vtts_denoise_create(C.byref(_lib.StftCfg(*cfg)), 0, C.byref(h))
        mine = lib.vtts_last_error() if rc else b""
        rs = lib.vtts_stft_create(C.byref(_lib.StftCfg(*cfg)), 0, C.byref(s))
        assert rc == rs == (-1 if cfg in bad else 0), cfg
        if rc:
            assert mine == lib.vtts_last_error() and mine, cfg  # the same refusal in the same words
        else:
            lib.vtts_denoise_destroy(h)
            lib.vtts_stft_destroy(s)
    assert lib.vtts_denoise_create(None, 0, C.byref(h)) == -1 and lib.vtts_denoise_create(C.byref(_lib.StftCfg(256, 256, 64, 0)), 0, None) == -1
    from viettts_amd.denoise import Denoiser

    with pytest.raises(ValueError, match="framing"):
        Denoiser((1024, 1024, 256, "same"))
    with pytest.raises(ValueError, match="ROCm device"):
        Denoiser(device="cpu")
    with pytest.raises(ValueError, match="strength"):
        Denoiser(strength=-0.1)
    with pytest.raises(ValueError, match="strength"):
        Denoiser(strength=float("nan"))


@pytest.mark.parametrize("cfg", [O.CFGS[0], O.CFGS[3], O.CFGS[5], O.CFGS[8]], ids=str)
def test_host_entry_points(cfg, lib):
    from viettts_amd.denoise import Denoiser
    from viettts_amd.stft import Stft

    n_fft, win, hop, framing = cfg
    st = Stft(*cfg[:3], framing=framing, device="cuda:0")  # create() touches no HIP call
    dn = Denoiser(st)
    H = n_fft // 2
    W, run = dn.blocking()
    assert (W, run) == st.blocking()[1:] and run == {256: 1024, 512: 2048, 1024: 4096, 2048: 4096}[n_fft]
    assert 8 * H + 8 * (H // 2 + 2) + 4 * n_fft + 4 * (H + 2) + 8 * W * (H + H // 8) <= SO.K["VTTS_SPECTRAL_LDS_BUDGET"]  # the header's table
    assert dn.packed_bytes == st.packed_bytes == 4 * (n_fft + 2 * H + 2 * (H // 2 + 2))  # the stft blob's layout
    assert lib.vtts_denoise_blocking(dn._h, None, None) == -1 and lib.vtts_denoise_packed_bytes(dn._h, None) == -1
    fake, other = C.c_void_p(1 << 32), C.c_void_p(1 << 36)
    lo = O.min_samples(cfg)
    one = (C.c_int32 * 1)(lo)
    app = lambda lens=one, S=lo, it=0, ot=0, N=1, wav=fake, bias=fake, s=0.5, out=other, os=lo: lib.vtts_denoise_apply(dn._h, wav, it, N, S, lens, bias, s, out, ot, os, None)  # noqa: E731
    assert app() == -2 and b"apply() before pack" in lib.vtts_last_error()  # nothing is dereferenced before the tables are bound
    assert lib.vtts_denoise_bind_packed(dn._h, C.c_void_p(1 << 32 | 8), dn.packed_bytes) == -1 and lib.vtts_denoise_bind_packed(dn._h, fake, dn.packed_bytes - 1) == -5
    assert lib.vtts_denoise_bind_packed(dn._h, fake, dn.packed_bytes) == 0
    assert app(lens=(C.c_int32 * 1)(lo - 1)) == -6 and b"pad + 1" in lib.vtts_last_error()
    assert app(lens=(C.c_int32 * 1)(lo + 1)) == -6 and b"S_stride" in lib.vtts_last_error()
    assert app(S=lo + 1, lens=(C.c_int32 * 1)(lo + 1)) == -6 and b"out_stride" in lib.vtts_last_error()
    assert app(it=2) == -1 and b"dtype" in lib.vtts_last_error() and app(ot=2) == -1
    assert app(N=0) == -1 and app(wav=None) == -1 and app(bias=None) == -1 and app(out=None) == -1
    for s in (-0.5, float("nan"), float("inf")):
        assert app(s=s) == -1 and b"strength" in lib.vtts_last_error()
    for out in (fake, C.c_void_p((1 << 32) + 4 * lo - 4), C.c_void_p((1 << 32) - 4 * lo + 4)):  # the same array, its last sample, its first
        assert app(out=out) == -1 and b"must not overlap wav_dev" in lib.vtts_last_error()
    dn.close()
    st.close()


def test_nola_refusal_names_the_window_and_the_hop(lib):
    fake, other = C.c_void_p(1 << 32), C.c_void_p(1 << 36)
    for cfg, S in (((256, 256, 256, 0), 1000), ((1024, 512, 512, 1), 4000)):  # Hann with hop == win: w[0] = 0 lands between the frames
        h = C.c_void_p(0)
        assert lib.vtts_denoise_create(C.byref(_lib.StftCfg(*cfg)), 0, C.byref(h)) == 0
        n = C.c_size_t(0)
        assert lib.vtts_denoise_packed_bytes(h, C.byref(n)) == 0 and lib.vtts_denoise_bind_packed(h, fake, n.value) == 0
        rc = lib.vtts_denoise_apply(h, fake, 0, 1, S, None, fake, 0.5, other, 0, S, None)  # refused before anything is launched
        msg = lib.vtts_last_error().decode()
        assert rc == -1 and f"window of {cfg[1]} samples" in msg and f"hop {cfg[2]}" in msg and "NOLA" in msg, msg
        lib.vtts_denoise_destroy(h)


# ------------------------------------------------------------ the oracle ------------------------------------------------------------
@pytest.mark.parametrize("cfg", O.CFGS, ids=str)
def test_oracle_limits_and_the_clamped_share(cfg):
    rt = D.round_trip_bound(cfg)[1]
    for i in D.rows(cfg):
        x = O.wave_case(i)
        for bias, s in ((D.zero_bias(cfg), D.STRENGTH), (D.smooth_bias(cfg), 0.0)):  # nothing to subtract: forward -> inverse
            d = O.rel(D.denoise(x, bias, s, cfg), x.astype(np.float64))
            d32 = O.rel(D.denoise(x, bias, s, cfg, f32=True), x.astype(np.float64))
            assert d <= rt and d32 <= rt, (i, d, d32, rt)
        for f32 in (False, True):
            assert not D.denoise(x, D.clamping_bias(cfg), D.STRENGTH, cfg, f32=f32).any(), i  # every bin clamps: exact zeros
        share = D.clamped_share(x, D.smooth_bias(cfg), D.STRENGTH, cfg)
        print(f"\n{cfg} row {i}: {100 * share:.1f} % of the bins clamp under the smooth bias at strength {D.STRENGTH}")
        assert 0.10 <= share <= 0.90, (i, share)
        y = D.want(i, cfg)
        assert 0.0 < np.abs(y).max() < np.abs(x).max() * 1.5 and O.rel(y, x.astype(np.float64)) > 100 * rt  # ... and it is no round trip


@pytest.mark.parametrize("cfg", CENTER, ids=str)
def test_float64_oracle_is_a_torch_composition(cfg):
    n_fft, win, hop, _ = cfg
    bias = D.smooth_bias(cfg)
    kw = dict(hop_length=hop, win_length=win, window=_torch_window(cfg), center=True)
    for i in D.rows(cfg):
        x = O.wave_case(i)
        z = torch.stft(torch.from_numpy(x.astype(np.float64)), n_fft, pad_mode="reflect", return_complex=True, **kw)  # [NB, T]
        sb = torch.from_numpy(float(np.float32(D.STRENGTH)) * bias.astype(np.float64))[:, None]
        z2 = torch.polar(torch.clamp(z.abs() - sb, min=0.0), z.angle())
        z2[0], z2[-1] = z2[0].real + 0j, z2[-1].real + 0j
        w = torch.istft(z2, n_fft, length=len(x), **kw).numpy()
        d = O.rel(D.want(i, cfg), w)
        print(f"\n{cfg} row {i}: float64 oracle within {d:.2e} of torch.stft -> abs / angle / clamp -> torch.istft")
        assert d < 1e-10


@pytest.mark.parametrize("cfg", O.CFGS, ids=str)
def test_every_planted_fault_misses_the_bound(cfg):
    scale, bound = D.bound(cfg)
    print(f"\n{cfg}: float32 restatement within {scale:.2e} of float64 (relative to the row's largest value); bound {bound:.2e}")
    assert 0.0 < bound < 1e-5  # an fp32 scale: a fault is orders above
    i = D.rows(cfg)[-1]
    x, y = O.wave_case(i), D.want(i, cfg)
    assert O.rel(D.denoise(x, D.smooth_bias(cfg), D.STRENGTH, cfg, f32=True), y) <= bound  # the restatement itself passes
    frames = D.noise_frames(cfg)
    y_noise = D.denoise(x, frames, D.STRENGTH, cfg)
    assert np.array_equal(y_noise, D.denoise(x, frames[0], D.STRENGTH, cfg))  # frame 0 of a noise recording is the bias
    assert 0.10 <= D.clamped_share(x, frames[0], D.STRENGTH, cfg) <= 0.90
    for fault in D.FAULTS:
        got = D.denoise(x, frames if fault == "bias_frame_1" else D.smooth_bias(cfg), D.STRENGTH, cfg, fault=fault)
        miss = O.rel(got, y_noise if fault == "bias_frame_1" else y) / bound
        print(f"  {fault:21s} misses by {miss:.3g} x bound")
        assert miss > 1.0, fault


def test_gain_f32_is_the_contracts_five_lines():
    cfg = O.CFGS[4]
    c = O.stft(O.wave_case(4), cfg, f32=True)
    bias = D.smooth_bias(cfg)
    g = D.gain_f32(c, bias, D.STRENGTH)
    assert g.dtype == np.complex64 and g.shape == c.shape
    t, f = 3, 40
    re_, im = np.float32(c[t, f].real), np.float32(c[t, f].imag)
    r = np.sqrt(np.float32(np.float32(re_ * re_) + np.float32(im * im)))
    m = max(np.float32(r - np.float32(np.float32(D.STRENGTH) * bias[f])), np.float32(0))
    d = np.float32(r + np.float32(1e-16))
    assert g[t, f].real == np.float32(m * np.float32(re_ / d)) and g[t, f].imag == np.float32(m * np.float32(im / d))
    assert (np.abs(g) <= np.abs(c) * (1 + 1e-6)).all()  # |c'| <= |c|: the operation is well conditioned
    want = D.bias_from_noise([c], cfg)
    assert want.shape == bias.shape and np.allclose(want, np.abs(c.astype(np.complex128)).mean(axis=0), rtol=1e-6)


# ------------------------------------------------------------ the command lines ------------------------------------------------------------
def test_command_lines_refuse_bad_arguments_before_touching_a_device(tmp_path, capsys, monkeypatch):
    from viettts_amd import denoise, resynth, serving, synthesizer, wavio

    monkeypatch.setattr(torch.cuda, "is_available", lambda: (_ for _ in ()).throw(AssertionError("a device was asked for")))
    wavio.write_wav_pcm16(tmp_path / "in.wav", np.zeros(16000, np.int16), 16000)  # one second
    wav = str(tmp_path / "in.wav")

    def refused(main, argv, *words):
        with pytest.raises(SystemExit) as e:
            main(argv)
        err = capsys.readouterr().err
        assert e.value.code == 2 and all(w in err for w in words), err

    assert synthesizer.build_parser().parse_args([]).denoise is None and resynth.build_parser().parse_args(["--input", "a", "--output", "b"]).denoise is None
    a = denoise.build_parser().parse_args(["--wav", "a.wav", "--noise-from", "0:0.5", "--output", "o.wav"])
    assert (a.strength, a.noise_from) == (1.0, "0:0.5") and denoise.parse_noise_from("0.25:1.5") == (0.25, 1.5)
    assert denoise.noise_span((0.25, 1.0), 16000, 16000) == (4000, 16000)
    # 1. a stream with a denoiser
    refused(synthesizer.main, ["--text", "xin chao", "--stream", "--denoise", "0.01"], "--stream with --denoise", "overlap-add state")
    with pytest.raises(ValueError, match="overlap-add state"):
        serving.SpeechPool(None, None, None, slots=2, Lmax=8, Fmax=8, denoise=0.01)
    # 2. no vocoder to take a bias from
    refused(synthesizer.main, ["--text", "xin chao", "--vocoder", "griffinlim", "--denoise", "0.01"], "no vocoder to take a bias from")
    refused(resynth.main, ["--input", wav, "--output", "o.wav", "--vocoder", "griffinlim", "--denoise", "0.01"], "no vocoder to take a bias from")
    # 3. a stretch of room tone that holds nothing, or ends past the input
    for main, head in ((resynth.main, ["--input", wav, "--output", "o.wav", "--denoise", "1.0"]), (denoise.main, ["--wav", wav, "--output", "o.wav"])):
        refused(main, head + ["--noise-from", "0.5:0.5"], "B must be above A")
        refused(main, head + ["--noise-from", "0.6:0.2"], "B must be above A")
        refused(main, head + ["--noise-from", "0.5:1.5"], "past the end of the input", "16000 samples")
        refused(main, head + ["--noise-from", "half"], "A:B in seconds")
    refused(resynth.main, ["--input", wav, "--output", "o.wav", "--noise-from", "0:0.5"], "--noise-from belongs to --denoise")
    refused(resynth.main, ["--input", wav, "--output", "o.wav", "--denoise", "-1"], "not negative")
    refused(synthesizer.main, ["--text", "xin chao", "--denoise", "-1"], "not negative")
    refused(denoise.main, ["--wav", wav, "--output", "o.wav", "--noise-from", "0:0.5", "--strength", "nan"], "strength")
    refused(denoise.main, ["--output", "o.wav", "--noise-from", "0:0.5"])
    import inspect

    from viettts_amd.pipeline import synthesize_sentences

    assert inspect.signature(synthesize_sentences).parameters["denoise"].default is None
    with pytest.raises(ValueError, match="strength"):
        synthesize_sentences([[1, 2]], None, None, None, denoise=-1.0)


def test_documents_carry_the_entry():
    readme, design = (REPO / "README.md").read_text(), (REPO / "DESIGN.md").read_text()
    assert "vtts_denoise.h" in readme and "viettts_amd.denoise" in readme
    assert "vtts_denoise.h" in design and "Out of scope" in design[design.index("vtts_denoise.h"):]
