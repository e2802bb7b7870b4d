"""include/vtts_stft.h without a GPU: the numpy restatement (tests/_stft_oracle.py) against torch.stft / torch.istft and, for the mel framing,
against its own round trip and tests/_mel_oracle.py; the bounds the GPU test uses, with every planted fault missing one; and the host entry
points of the built library, the Python class and the command lines' argument errors."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import _mel_oracle as MO
import _spectral_oracle as SO
import _stft_oracle as O
from viettts_amd import _lib

REPO = Path(__file__).resolve().parents[1]
CENTER = [c for c in O.CFGS if c[3] == "center"]
MEL = [c for c in O.CFGS if c[3] == "mel"]


@pytest.fixture(scope="module")
def lib():
    from viettts_amd.csrc.build import build

    build()
    return _lib.load()


def _stft(cfg):
    from viettts_amd.stft import Stft

    return Stft(*cfg[:3], framing=cfg[3], device="cuda:0")  # create() touches no HIP call


def _torch_window(cfg):
    n_fft, win, _, _ = cfg
    lead = (n_fft - win) // 2
    return torch.from_numpy(O.window(cfg)[lead : lead + win].astype(np.float64))


@pytest.mark.parametrize("cfg", CENTER, ids=str)
def test_float64_oracle_is_torch_stft_and_istft(cfg):
    n_fft, win, hop, _ = cfg
    for i in range(len(O.ROWS)):
        x = O.wave_case(i)
        if len(x) < O.min_samples(cfg):
            continue
        z = torch.stft(torch.from_numpy(x.astype(np.float64)), n_fft, hop_length=hop, win_length=win, window=_torch_window(cfg), center=True, pad_mode="reflect",
                       return_complex=True).numpy().T
        mine = O.stft(x, cfg)
        assert mine.shape == z.shape == (O.num_frames(len(x), cfg), n_fft // 2 + 1)
        d = O.rel(mine, z)
        s = O.spec_case(i, cfg).astype(np.complex128)
        s0 = s.copy()
        s0[:, 0], s0[:, -1] = s0[:, 0].real, s0[:, -1].real
        w = torch.istft(torch.from_numpy(s0.T.copy()), n_fft, hop_length=hop, win_length=win, window=_torch_window(cfg), center=True, length=len(x)).numpy()
        di = O.rel(O.istft(s, len(x), cfg), w)
        print(f"\n{cfg} row {i}: float64 oracle within {d:.2e} of torch.stft and {di:.2e} of torch.istft")
        assert d < 1e-11 and di < 1e-11
        assert np.array_equal(O.istft(s, len(x), cfg), O.istft(s0, len(x), cfg))  # the imaginary parts of bins 0 and H are no part of it


@pytest.mark.parametrize("cfg", MEL, ids=str)
def test_float64_oracle_in_mel_framing(cfg, monkeypatch):
    for i in range(len(O.ROWS)):
        x = O.wave_case(i)
        if len(x) < O.min_samples(cfg):
            continue
        back = O.istft(O.stft(x, cfg), len(x), cfg)  # the float64 spectrum, not rounded to complex64
        d = float(np.abs(back - x).max())
        print(f"\n{cfg} row {i}: istft(stft(x)) within {d:.2e} of x")
        assert d < 1e-12
    if cfg[:3] == (1024, 1024, 256):  # the mel front end's own resolution: its log-mel from this spectrum
        x = O.wave_case(4)
        X = O.stft(x, cfg)
        fb = MO.slaney_filterbank()
        mine = np.log(np.maximum(np.sqrt(X.real ** 2 + X.imag ** 2 + MO.MAG_EPS) @ fb.T, MO.MEL_FLOOR))
        monkeypatch.setattr(MO, "hann_periodic", lambda n: O.window(cfg).astype(np.float64))  # the header's fp32 window in place of the float64 one
        want = MO.log_mel(x[None, :])[0]
        assert mine.shape == want.shape == (len(x) // 256, 80) and np.abs(mine - want).max() < 1e-11
        monkeypatch.undo()
        assert 0.0 < np.abs(mine - MO.log_mel(x[None, :])[0]).max() < 1e-5  # (the window's rounding to fp32 is all that differs otherwise)


@pytest.mark.parametrize("cfg", O.CFGS, ids=str)
def test_frame_and_sample_counts_on_either_side_of_a_hop_multiple(cfg, lib):
    st = _stft(cfg)
    hop = cfg[2]
    k = O.min_samples(cfg) // hop + 2
    base = O.num_frames(k * hop, cfg)
    for S in (k * hop - 1, k * hop, k * hop + 1):
        want = base - (S < k * hop)
        assert O.num_frames(S, cfg) == want == st.num_frames(S) == O.frame_index(S, cfg).shape[0], (S, want)
    assert st.num_frames(k * hop) == (k + 1 if cfg[3] == "center" else k)
    for T in (base, base + 1, 1000):
        S = st.num_samples(T)
        assert S == O.num_samples(T, cfg) == (hop * (T - 1) if cfg[3] == "center" else hop * T)
        assert st.num_frames(S) == T and st.num_frames(S - 1) == T - 1  # the smallest S with T frames
    if cfg[3] == "center":  # torch's count
        x = torch.zeros(k * hop, dtype=torch.float64)
        assert torch.stft(x, cfg[0], hop_length=hop, win_length=cfg[1], window=_torch_window(cfg), center=True, return_complex=True).shape[1] == k + 1
    else:
        assert st.num_frames(k * hop) == MO.num_frames(k * hop, cfg[0], hop)
    n = C.c_int64(0)
    assert lib.vtts_stft_num_samples(st._h, 0, C.byref(n)) == -6
    if cfg[3] == "center":
        assert lib.vtts_stft_num_samples(st._h, 1, C.byref(n)) == -6 and b"pad + 1" in lib.vtts_last_error()  # 0 samples cannot be reflected
    st.close()


def test_header_exports_and_constants(lib):
    header = O.HEADER.read_text()
    declared = set(re.findall(r"\b(vtts_stft_[a-z_0-9]+)\s*\(", header))
    assert declared == set(_lib.STFT_EXPORTS) == {f"vtts_stft_{n}" for n in ("create", "destroy", "window", "blocking", "num_frames", "num_samples", "min_envelope",
                                                                             "packed_bytes", "pack", "bind_packed", "forward", "inverse", "project")}
    for name in declared:
        assert hasattr(lib, name), name
    assert not set(_lib.STFT_SIGS) & (set(_lib.SIGS) | set(_lib.SPECTRAL_SIGS))
    k = O.header_constants()
    assert int(k["VTTS_STFT_MAX_SAMPLES"]) == _lib.STFT_MAX_SAMPLES == SO.K["VTTS_SPECTRAL_MAX_SAMPLES"]
    assert int(k["VTTS_STFT_ROWS_PER_LAUNCH"]) == _lib.STFT_ROWS_PER_LAUNCH and float(k["VTTS_STFT_NOLA_FLOOR"]) == _lib.STFT_NOLA_FLOOR == O.NOLA_FLOOR == 1e-11
    assert (int(k["VTTS_STFT_CENTER"]), int(k["VTTS_STFT_MEL"])) == (_lib.VTTS_STFT_CENTER, _lib.VTTS_STFT_MEL) == (0, 1)
    text = (REPO / "viettts_amd" / "csrc" / "stft.hip").read_text()
    found = re.findall(r"^constexpr int (ROWS_PER_LAUNCH) = (\d+);", text, flags=re.M)
    assert found == [("ROWS_PER_LAUNCH", str(_lib.STFT_ROWS_PER_LAUNCH))] and len(re.findall(r"for_each_launch(?:_off)?<ROWS_PER_LAUNCH>\(", text)) == 2
    assert len(re.findall(r"\+= ROWS_PER_LAUNCH\)", text)) == 0  # launch_rows.h's loop, and no hand-written one
    assert "#pragma clang fp contract(off)" in text and text.index("#pragma clang fp contract(off)") < text.index('#include "stockham.h"')
    assert "atomic" not in text.replace("no atomic", "") and not re.search(r"\b(sinf?|cosf?|sincosf?)\s*\(", text.replace("std::cos(", "").replace("std::sin(", ""))
    from viettts_amd.csrc import build

    assert "stft.hip" in build.SOURCES and "stockham.h" in build.HEADERS and any(str(h).endswith("vtts_stft.h") for h in build.HEADERS)
    assert "-fno-slp-vectorize" in build.FILE_FLAGS["stft.hip"]


def test_create_refuses_what_the_header_excludes(lib):
    h = C.c_void_p(0)
    for bad in ((128, 64, 16, 0), (4096, 1024, 256, 0), (1000, 600, 120, 1), (1024, 600, 0, 0), (1024, 600, -1, 0), (1024, 100, 120, 0), (1024, 1025, 120, 0), (512, 600, 120, 1)):
        assert lib.vtts_stft_create(C.byref(_lib.StftCfg(*bad)), 0, C.byref(h)) == -1, bad
        assert b"n_fft" in lib.vtts_last_error()
    for framing in (-1, 2):
        assert lib.vtts_stft_create(C.byref(_lib.StftCfg(1024, 1024, 256, framing)), 0, C.byref(h)) == -1 and b"framing" in lib.vtts_last_error()
    assert lib.vtts_stft_create(C.byref(_lib.StftCfg(1024, 600, 121, 1)), 0, C.byref(h)) == -1 and b"n_fft - hop must be even" in lib.vtts_last_error()
    assert lib.vtts_stft_create(C.byref(_lib.StftCfg(1024, 600, 121, 0)), 0, C.byref(h)) == 0  # ... which only the mel framing asks
    lib.vtts_stft_destroy(h)
    assert lib.vtts_stft_create(None, 0, C.byref(h)) == -1 and lib.vtts_stft_create(C.byref(_lib.StftCfg(256, 256, 64, 0)), 0, None) == -1
    for good in ((256, 1, 1, 0), (256, 256, 256, 0), (2048, 2048, 2048, 1), (2048, 2048, 2, 1), (1024, 1024, 256, 1), (512, 240, 50, 1)):
        assert lib.vtts_stft_create(C.byref(_lib.StftCfg(*good)), 0, C.byref(h)) == 0, good
        lib.vtts_stft_destroy(h)
    from viettts_amd.stft import Stft

    with pytest.raises(ValueError, match="framing"):
        Stft(1024, 1024, 256, framing="same", device="cuda:0")
    with pytest.raises(ValueError, match="ROCm device"):
        Stft(1024, 1024, 256, device="cpu")


@pytest.mark.parametrize("cfg", O.CFGS + ((512, 512, 128, "center"), (2048, 2048, 512, "mel"), (256, 100, 3, "center")), ids=str)
def test_min_envelope_is_the_oracles(cfg, lib):
    st = _stft(cfg)
    lo, n_fft, hop = O.min_samples(cfg), cfg[0], cfg[2]
    for S in (lo, lo + 1, n_fft - 1, n_fft + hop, 2 * (n_fft + hop) - 1, 2 * (n_fft + hop), 2 * (n_fft + hop) + 1, 7 * n_fft + 13):
        if S >= lo:
            got, want = st.min_envelope(S), O.min_envelope(S, cfg)
            assert got == pytest.approx(want, rel=1e-12) and want > O.NOLA_FLOOR, (S, got, want)
    st.close()


def test_nola_refusal_names_the_window_and_the_hop(lib):
    fake = C.c_void_p(1 << 32)
    for res, S in (((256, 256, 256), 1000), ((1024, 512, 512), 4000), ((2048, 2048, 2048), 4096)):  # Hann with hop == win: w[0] = 0 lands between the frames
        for framing in ("center", "mel"):
            cfg = res + (framing,)
            st = _stft(cfg)
            assert O.min_envelope(S, cfg) < O.NOLA_FLOOR and st.min_envelope(S) < O.NOLA_FLOOR
            assert lib.vtts_stft_bind_packed(st._h, fake, st.packed_bytes) == 0
            rc = lib.vtts_stft_inverse(st._h, fake, 1, st.num_frames(S), (C.c_int32 * 1)(S), fake, 0, S, None)  # refused before anything is launched
            msg = lib.vtts_last_error().decode()
            assert rc == -1 and f"window of {res[1]} samples" in msg and f"hop {res[2]}" in msg and "NOLA" in msg, msg
            st.close()


@pytest.mark.parametrize("cfg", [O.CFGS[0], O.CFGS[3], O.CFGS[5], O.CFGS[8], (2048, 2048, 2048, "center")], ids=str)
def test_host_entry_points(cfg, lib):
    st = _stft(cfg)
    n_fft, win, hop, framing = cfg
    assert np.array_equal(st.window().view(np.uint32), O.window(cfg).view(np.uint32))  # bit for bit vtts_spectral.h's
    F, W, run = st.blocking()
    assert 1 <= F <= (4 if n_fft == 2048 else 8) and W == (4 if n_fft == 2048 else 8) and run == {256: 1024, 512: 2048, 1024: 4096, 2048: 4096}[n_fft]
    H = n_fft // 2
    assert 8 * H + 8 * (H // 2 + 2) + 4 * (((F - 1) * hop + n_fft + 1) // 2 * 2) + 8 * F * (H + H // 8) <= SO.K["VTTS_SPECTRAL_LDS_BUDGET"] or F == 1  # the header's tables
    assert 8 * H + 8 * (H // 2 + 2) + 4 * n_fft + 8 * W * (H + H // 8) <= SO.K["VTTS_SPECTRAL_LDS_BUDGET"]
    lo = O.min_samples(cfg)
    assert st.pad == O.pad(cfg) and st.n_bins == H + 1 and st.packed_bytes == 4 * (n_fft + 2 * H + 2 * (H // 2 + 2))
    n, e = C.c_int64(0), C.c_double(0.0)
    for S in (lo - 1, 0, -1, _lib.STFT_MAX_SAMPLES + 1):
        assert lib.vtts_stft_num_frames(st._h, S, C.byref(n)) == -6 and b"pad + 1" in lib.vtts_last_error()
        assert lib.vtts_stft_min_envelope(st._h, S, C.byref(e)) == -6
    assert st.num_frames(_lib.STFT_MAX_SAMPLES) == O.num_frames(_lib.STFT_MAX_SAMPLES, cfg)
    assert lib.vtts_stft_num_frames(None, lo, C.byref(n)) == -1 and lib.vtts_stft_num_frames(st._h, lo, None) == -1 and lib.vtts_stft_min_envelope(st._h, lo, None) == -1
    assert lib.vtts_stft_window(st._h, None) == -1 and lib.vtts_stft_blocking(st._h, None, None, None) == -1
    fake = C.c_void_p(1 << 32)
    T = st.num_frames(lo)
    one = (C.c_int32 * 1)(lo)
    fwd = lambda lens=one, S=lo, dtype=0, ts=T, N=1, wav=fake, spec=fake: lib.vtts_stft_forward(st._h, wav, dtype, N, S, lens, spec, ts, None)  # noqa: E731
    inv = lambda lens=one, S=lo, dtype=0, ts=T, N=1, spec=fake, out=fake: lib.vtts_stft_inverse(st._h, spec, N, ts, lens, out, dtype, S, None)  # noqa: E731
    prj = lambda lens=one, S=lo, dtype=0, ts=T, m=0.99, mag=fake, tp=fake, spec=C.c_void_p(1 << 33): lib.vtts_stft_project(st._h, fake, dtype, 1, S, lens, mag, tp, spec, ts, m, None)  # noqa: E731
    for call, name in ((fwd, b"forward"), (inv, b"inverse"), (prj, b"project")):
        assert call() == -2 and name + b"() before pack" in lib.vtts_last_error()  # nothing is dereferenced before the tables are bound
    assert lib.vtts_stft_bind_packed(st._h, C.c_void_p(1 << 32 | 8), st.packed_bytes) == -1 and lib.vtts_stft_bind_packed(st._h, fake, st.packed_bytes - 1) == -5
    assert lib.vtts_stft_bind_packed(st._h, fake, st.packed_bytes) == 0
    for call in (fwd, inv, prj):
        assert call(lens=(C.c_int32 * 1)(lo - 1)) == -6 and b"pad + 1" in lib.vtts_last_error()
        assert call(lens=(C.c_int32 * 1)(lo + 1)) == -6 and b"S_stride" in lib.vtts_last_error()
        assert call(dtype=2) == -1 and b"dtype" in lib.vtts_last_error()
        assert call(ts=T - 1) == -6 and b"T_stride" in lib.vtts_last_error()
    assert fwd(N=0) == -1 and inv(N=0) == -1 and fwd(wav=None) == -1 and fwd(spec=None) == -1 and inv(spec=None) == -1 and inv(out=None) == -1
    assert prj(mag=None) == -1 and prj(tp=None) == -1 and prj(spec=None) == -1
    assert prj(m=1.0) == -1 and b"momentum" in lib.vtts_last_error() and prj(m=-0.1) == -1 and prj(m=float("nan")) == -1
    assert prj(spec=fake) == -1 and b"must not be tprev_dev" in lib.vtts_last_error()
    st.close()


# ------------------------------------------------------------ the bounds and the faults ------------------------------------------------------------
@pytest.mark.parametrize("cfg", O.CFGS, ids=str)
def test_every_planted_fault_misses_a_bound(cfg):
    (fs, fb), (vs, vb) = O.forward_bound(cfg), O.inverse_bound(cfg)
    print(f"\n{cfg}: float32 restatement within forward {fs:.2e} / inverse {vs:.2e} of float64 (relative to the row's largest value); bounds {fb:.2e} / {vb:.2e}")
    assert 0.0 < fb < 1e-5 and 0.0 < vb < 1e-5  # fp32 scales: a fault is orders above
    hop, lo = cfg[2], O.min_samples(cfg)
    S = (lo // hop + 3) * hop  # a hop multiple: the one place where the frame count's fault shows
    x = SO.make_speechlike(S, 17)
    rng = np.random.default_rng(18)
    T = O.num_frames(S, cfg)
    spec = (rng.standard_normal((T, cfg[0] // 2 + 1)) + 1j * rng.standard_normal((T, cfg[0] // 2 + 1))).astype(np.complex64)
    X, y = O.stft(x, cfg), O.istft(spec, S, cfg)
    assert O.rel(O.stft(x, cfg, f32=True), X) <= fb and O.rel(O.istft(spec, S, cfg, f32=True), y) <= vb  # the restatement itself passes
    for fault in O.INVERSE_FAULTS:
        got = O.istft(spec, S, cfg, fault=fault)
        miss = O.rel(np.nan_to_num(got, nan=1e30, posinf=1e30, neginf=-1e30), y) / vb
        print(f"  inverse {fault:19s} misses by {miss:.3g} x bound")
        assert miss > 1.0, fault
    for fault in O.FORWARD_FAULTS:
        got = O.stft(x, cfg, fault=fault)
        if fault == "frames_off_by_one":
            assert got.shape[0] == T - 1  # the count itself
            continue
        miss = O.rel(got, X) / fb
        print(f"  forward {fault:19s} misses by {miss:.3g} x bound")
        assert miss > 1.0, fault
    mag = np.abs(O.stft(SO.degrade(x, 3, 0.3), cfg)).astype(np.float32)
    tprev = O.stft(SO.degrade(x, 4, 0.1), cfg).astype(np.complex64)
    want, c = O.project(x, mag, tprev, 0.99, cfg)
    lim = O.project_limit(mag, c - O.alpha_of(0.99, False) * tprev.astype(np.complex128), tprev, c, cfg)
    ok = np.abs(O.project(x, mag, tprev, 0.99, cfg, f32=True)[0] - want) / np.maximum(lim, 1e-300)
    bad = np.abs(O.project(x, mag, tprev, 0.99, cfg, fault="momentum_on_c")[0] - want) / np.maximum(lim, 1e-300)
    print(f"  projection: float32 restatement at most {ok.max():.3f} of the limit; momentum_on_c misses by {bad.max():.3g} x")
    assert ok.max() <= 1.0 and bad.max() > 1.0


def test_griffin_lim_oracle_converges_and_float32_follows_it():
    cfg, S = (512, 240, 50, "center"), 3000
    x = SO.make_speechlike(S, 21)
    mag = np.abs(O.stft(x, cfg)).astype(np.float32)
    init = np.exp(2j * np.pi * np.random.default_rng(5).random(mag.shape)).astype(np.complex64)
    sc = [SO.measure(x, O.griffinlim(mag, S, cfg, n, 0.99, init).astype(np.float32), cfg[:3]).sc for n in (0, 4, 16)]
    d = O.rel(O.griffinlim(mag, S, cfg, 4, 0.99, init, f32=True), O.griffinlim(mag, S, cfg, 4, 0.99, init))
    print(f"\nspectral convergence after 0 / 4 / 16 iterations: {sc[0]:.3f} / {sc[1]:.3f} / {sc[2]:.3f}; float32 within {d:.2e} of float64 after 4")
    assert sc[0] > sc[1] > sc[2] and d < 1e-4


# ------------------------------------------------------------ the command lines ------------------------------------------------------------
def test_command_lines_refuse_bad_arguments_before_touching_a_device(tmp_path, capsys):
    from viettts_amd import resynth, stft, synthesizer

    a = stft.build_parser().parse_args(["--mel-file", "m.npy", "--output", "o.wav"])
    assert (a.n_iter, a.momentum, a.seed) == (32, 0.99, 0)
    for bad in (["--output", "o.wav"], ["--mel-file", "m.npy"], ["--mel-file", "m.npy", "--output", "o.wav", "--n-iter", "-1"],
                ["--mel-file", "m.npy", "--output", "o.wav", "--momentum", "1.0"]):
        with pytest.raises(SystemExit) as e:
            stft.main(bad)
        assert e.value.code == 2
    np.save(tmp_path / "bad.npy", np.zeros((3, 5, 80), np.float32))
    with pytest.raises(ValueError, match=r"\[T, 80\]"):
        stft.main(["--mel-file", str(tmp_path / "bad.npy"), "--output", str(tmp_path / "o.wav")])
    assert synthesizer.build_parser().parse_args([]).vocoder == "hifigan" and resynth.build_parser().parse_args(["--input", "a", "--output", "b"]).vocoder == "hifigan"
    with pytest.raises(SystemExit) as e:
        synthesizer.main(["--text", "xin chao", "--vocoder", "griffinlim", "--stream"])
    assert e.value.code == 2 and "no streamed inverse" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        synthesizer.build_parser().parse_args(["--vocoder", "wavenet"])
    with pytest.raises(SystemExit) as e:
        resynth.main(["--input", "a.wav", "--output", "b.wav", "--vocoder", "griffinlim", "--dtype", "bf16"])
    assert e.value.code == 2 and "--dtype" in capsys.readouterr().err


def test_documents_point_to_the_inverse():
    for rel_path in ("include/vtts_spectral.h", "viettts_amd/spectral.py"):
        text = (REPO / rel_path).read_text()
        assert "vtts_stft.h" in text and "No inverse transform, no phase" not in text and "no inverse transform, no phase" not in text, rel_path
    assert "vtts_stft.h" in (REPO / "README.md").read_text() and "6w" in (REPO / "DESIGN.md").read_text()
