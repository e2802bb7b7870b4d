"""include/vtts_pitch.h without a GPU: the float32 restatement (tests/_pitch_oracle.py) finds the pitch of known tones and agrees with its
float64 form, every planted deviation from the contract shows on the inputs the GPU test uses, the C ABI's host side, the kernel's ISA
(no FMA outside the divisions) and ``f0_metrics`` on planted contours."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest
import torch

import _pitch_oracle as O
from viettts_amd import _lib

K = O.header_constants()
FPB = K["VTTS_PITCH_FRAMES_PER_BLOCK"]


@pytest.fixture(scope="module")
def lib():
    from viettts_amd.csrc.build import build

    build()
    return _lib.load()


def _create(lib, sample_rate=16000, fmin=50.0, fmax=500.0, threshold=0.15):
    h = C.c_void_p(0)
    rc = lib.vtts_pitch_create(C.byref(_lib.PitchCfg(sample_rate, fmin, fmax, threshold)), 0, C.byref(h))
    return rc, h


def _bits(r: O.Yin) -> np.ndarray:
    return np.stack([r.f0, r.aperiodicity, r.candidate]).view(np.uint32)


# ------------------------------------------------------------ the oracle ------------------------------------------------------------
@pytest.mark.parametrize("f0", [55.0, 80.0, 123.4, 200.0, 333.3, 480.0])
def test_f32_oracle_finds_the_pitch_of_a_steady_tone(f0):
    """Every interior frame (no reflected sample in it) is voiced and within 2 cents.  Measured: 0.02, 0.05, 0.03, 0.20, 0.48, 0.77 cents."""
    r = O.yin_f32(O.tone(f0, 24))
    assert r.f0.shape == (1, 24)
    f, v = r.f0[0, 2:-2], r.voiced[0, 2:-2]
    assert v.all()
    cents = float(np.abs(1200.0 * np.log2(f.astype(np.float64) / f0)).max())
    print(f"\n{f0} Hz: worst {cents:.3f} cents, aperiodicity <= {float(r.aperiodicity[0, 2:-2].max()):.3e}")
    assert cents <= 2.0
    if f0 == 80.0:  # a whole period of 200 samples: d[tau*] is exactly 0
        assert np.all(r.aperiodicity[0, 2:-2] == 0) and np.all(r.tau[0, 2:-2] == 200)


def test_f32_oracle_agrees_with_f64_in_every_frame():
    """1152 frames of gliding, noisy, partly silent rows: tau* and the voicing decision are equal in EVERY frame.  Measured: 1152 of 1152,
    749 voiced; |aperiodicity| differs by 9.8e-7 at most, candidate by 4.5e-7 relative."""
    y = O.agreement_rows()
    a, b = O.agreement_f32(), O.yin_f64(y)
    assert a.tau.size >= 1000
    assert np.array_equal(a.tau, b.tau) and np.array_equal(a.voiced, b.voiced)
    dap = float(np.abs(a.aperiodicity.astype(np.float64) - b.aperiodicity).max())
    dc = float((np.abs(a.candidate.astype(np.float64) - b.candidate) / b.candidate).max())
    print(f"\n{a.tau.size} frames, {int(a.voiced.sum())} voiced: |aperiodicity| differs by {dap:.2e}, candidate by {dc:.2e} relative")
    assert dap <= 1e-5 and dc <= 1e-6
    zero = (y.reshape(y.shape[0], -1, O.HOP) == 0).all(axis=2)  # hops of exact zeros
    all_zero = a.aperiodicity == 1  # c = 1 at every lag: only digital silence gives that
    assert int(a.voiced.sum()) > 0 and int(all_zero.sum()) > 0 and int((~a.voiced & ~all_zero).sum()) > 0
    assert zero.sum() >= all_zero.sum() > 0 and not a.voiced[all_zero].any()


def test_rows_of_a_batch_are_the_rows_alone_in_the_oracle():
    y, lengths = O.ragged_batch(FPB, pcm=False)
    r = O.yin_f32(y, O.DEFAULT, lengths)
    for b, n in enumerate(lengths):
        alone = O.yin_f32(y[b, :n])
        T = O.num_frames(n)
        assert np.array_equal(_bits(alone)[:, 0], _bits(r)[:, b, :T])
        assert np.all(r.f0[b, T:] == 0) and np.all(r.aperiodicity[b, T:] == 1) and np.all(r.candidate[b, T:] == 0)


# ------------------------------------------------------------ planted faults ------------------------------------------------------------
@pytest.mark.parametrize("fault", O.FAULTS)
def test_planted_fault_changes_an_output_bit_on_the_gpu_tests_inputs(fault):
    """tests/test_gpu_pitch.py compares these very inputs with ==, so a kernel with the fault cannot pass it."""
    if fault == "reflect_at_stride":
        y, lengths = O.ragged_batch(FPB, pcm=False)
        cfg = O.DEFAULT
    else:
        y, lengths = O.content_rows()
        cfg = O.threshold_on_a_value() if fault == "le_threshold" else O.DEFAULT
    want, got = O.yin_f32(y, cfg, lengths), O.yin_f32(y, cfg, lengths, fault=fault)
    changed = int((_bits(want) != _bits(got)).sum())
    print(f"\n{fault}: {changed} output words change")
    assert changed >= 1


def test_the_grid_row_has_ties_and_the_first_minimum_wins():
    y = O.grid_row(5)
    assert np.array_equal(y * 8, np.round(y * 8))
    r = O.yin_f32(y)
    tau_min, tau_max = O.lags(O.DEFAULT)
    silent = (O._frames(y, len(y), np.float32) == 0).all(axis=1)  # c = 1 at every lag: a tie over the whole search range
    assert silent.sum() >= 1 and np.all(r.tau[0][silent] == tau_min) and np.all(r.aperiodicity[0][silent] == 1) and not r.voiced[0][silent].any()
    last = O.yin_f32(y, fault="last_minimum")
    assert np.all(last.tau[0][silent] == tau_max)
    tied = r.tau[0] < last.tau[0]  # ... and frames with one impulse in silence: c = 1 over a range of lags only
    assert tied.sum() > silent.sum() and np.all(r.aperiodicity[0][tied] == last.aperiodicity[0][tied]) and not np.any(r.tau[0] > last.tau[0])
    assert np.any((r.aperiodicity[0] == 0) & r.voiced[0])  # the part with an integer period: c = 0 exactly


def test_edge_lengths_list():
    lengths = O.edge_lengths(FPB)
    assert len(lengths) <= 20 and 385 in lengths and len(set(lengths)) == len(lengths)
    assert {O.num_frames(n) for n in lengths} >= {1, 2, FPB - 1, FPB, FPB + 1, 2 * FPB, 2 * FPB + 1}


def test_lag_edge_configurations():
    got = {k: O.lags(c) for k, c in O.LAG_EDGE_CFGS.items()}
    assert [got[k][1] for k in ("tau_max_63", "tau_max_64", "tau_max_65", "tau_max_320", "tau_max_326", "tau_max_512")] == [63, 64, 65, 320, 326, 512]
    assert got["tau_min_2"][0] == 2 and got["one_lag"][0] == got["one_lag"][1]
    assert O.lags(O.DEFAULT) == (32, 320)


# ------------------------------------------------------------ the C ABI's host side ------------------------------------------------------------
def test_header_symbols_all_exported(lib):
    declared = set(re.findall(r"\b(vtts_pitch_[a-z_0-9]+)\s*\(", O.HEADER.read_text()))
    assert declared == set(_lib.PITCH_EXPORTS) == {"vtts_pitch_create", "vtts_pitch_destroy", "vtts_pitch_num_frames", "vtts_pitch_workspace_bytes",
                                                  "vtts_pitch_forward"}
    for name in declared:
        assert hasattr(lib, name), name
        fn = getattr(lib, name)
        assert fn.restype is _lib.PITCH_SIGS[name][0] and list(fn.argtypes) == _lib.PITCH_SIGS[name][1]
    assert K["VTTS_PITCH_FRAMES_PER_BLOCK"] == _lib.PITCH_FRAMES_PER_BLOCK and K["VTTS_PITCH_MAX_LAG"] == _lib.PITCH_MAX_LAG
    assert (K["VTTS_PITCH_NFFT"], K["VTTS_PITCH_HOP"], K["VTTS_PITCH_PAD"], K["VTTS_PITCH_WINDOW"]) == (1024, 256, 384, 512)
    assert not set(_lib.PITCH_SIGS) & set(_lib.SIGS)


def test_pitch_hip_is_built_with_its_flags():
    from viettts_amd.csrc import build

    assert "pitch.hip" in build.SOURCES and "-fno-slp-vectorize" in build.FILE_FLAGS["pitch.hip"] and "-ffp-contract=off" in build.FILE_FLAGS["pitch.hip"]
    assert any(str(h).endswith("vtts_pitch.h") for h in build.HEADERS)


def test_create_accepts_and_refuses_exactly_the_documented_ranges(lib):
    # tau_max 512 (twice), tau_min 2, one lag, thresholds just inside
    good = [dict(), dict(fmin=31.25), dict(sample_rate=16384, fmin=32.0), dict(fmax=8000.0), dict(fmin=100.0, fmax=100.0), dict(threshold=0.999),
            dict(threshold=1e-6)]
    # tau_max 513, tau_min 1, tau_min 160 > tau_max 80, thresholds 0 and 1, and values that are no frequencies or rates at all
    bad = [dict(sample_rate=16416, fmin=32.0), dict(fmax=16000.0), dict(fmin=200.0, fmax=100.0), dict(threshold=0.0), dict(threshold=1.0),
           dict(threshold=float("nan")), dict(fmin=0.0), dict(fmin=-50.0), dict(fmax=float("inf")), dict(sample_rate=0)]
    for kw in good:
        rc, h = _create(lib, **kw)
        assert rc == 0, kw
        lib.vtts_pitch_destroy(h)
    for kw in bad:
        rc, _ = _create(lib, **kw)
        assert rc == -1 and lib.vtts_last_error(), kw
    assert lib.vtts_pitch_create(None, 0, C.byref(C.c_void_p(0))) == -1
    lib.vtts_pitch_destroy(None)


def test_num_frames_is_the_mel_front_ends(lib):
    rc, h = _create(lib)
    assert rc == 0
    m = C.c_void_p(0)
    assert lib.vtts_mel_create(C.byref(_lib.MelCfg(16000, 1024, 256, 80, 0.0, 8000.0)), 0, C.byref(m)) == 0
    a, b = C.c_int64(0), C.c_int64(0)
    for n in (385, 511, 512, 513, 2047, 2048, 1 << 20):
        assert lib.vtts_pitch_num_frames(h, n, C.byref(a)) == 0 and lib.vtts_mel_num_frames(m, n, C.byref(b)) == 0
        assert a.value == b.value == O.num_frames(n), n
    assert lib.vtts_pitch_num_frames(h, 384, C.byref(a)) == -6
    ws = C.c_size_t(7)
    assert lib.vtts_pitch_workspace_bytes(h, 64, 262144, C.byref(ws)) == 0 and ws.value == 0
    assert lib.vtts_pitch_workspace_bytes(h, 0, 4096, C.byref(ws)) == -1 and lib.vtts_pitch_workspace_bytes(h, 1, 384, C.byref(ws)) == -6
    lib.vtts_mel_destroy(m)
    lib.vtts_pitch_destroy(h)


def test_forward_refuses_bad_arguments_before_any_launch(lib):
    """No GPU here: every refusal below has to come from host arithmetic.  The pointers are never dereferenced."""
    rc, h = _create(lib)
    assert rc == 0
    fake = C.c_void_p(0x1000)
    i32 = lambda *v: (C.c_int32 * len(v))(*v)  # noqa: E731

    def fwd(dtype, N, S, lengths, T, f0=fake):
        return lib.vtts_pitch_forward(h, fake, dtype, N, S, lengths, f0, fake, fake, T, None, None)

    assert fwd(2, 1, 4096, None, 16) == -1  # dtype
    assert fwd(0, 0, 4096, None, 16) == -1  # N
    assert fwd(0, 1, 384, None, 1) == -6  # too short to reflect
    assert fwd(0, 2, 4096, i32(4096, 384), 16) == -6 and b"lengths[1]" in lib.vtts_last_error()
    assert fwd(0, 2, 4096, i32(4097, 4096), 16) == -6
    assert fwd(1, 2, 4096, i32(4096, 385), 15) == -6 and b"T_stride" in lib.vtts_last_error()
    assert fwd(0, 1, 4096, None, 16, f0=None) == -1
    lib.vtts_pitch_destroy(h)


def test_the_kernels_chains_are_not_contracted(tmp_path):
    """The == contract needs subtract, multiply and add as three instructions.  hipcc contracts by default, through __fmul_rn / __fadd_rn too
    (csrc/build.py: FILE_FLAGS), so the ISA of pitch.hip as the build compiles it is read: per kernel, the only FMAs are those of the
    correctly rounded divisions, and the chain's 8 * 64 steps show as that many of each of the three instructions."""
    from viettts_amd.csrc import build

    out = tmp_path / "pitch.s"
    cmd = [build._hipcc(), *build.FLAGS, *build.FILE_FLAGS["pitch.hip"], "--cuda-device-only", "-S", str(build.CSRC / "pitch.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"^(_Z\w*pitch_yin_k\w*):[^\n]*\n(.*?)^\.Lfunc_end", out.read_text(), re.M | re.S)
    assert len(kernels) == 2  # float and PCM16 input
    for name, body in kernels:
        n = {k: len(re.findall(r"\b" + k, body)) for k in ("v_sub_f32", "v_mul_f32", "v_add_f32", "v_div_fixup_f32")}
        fused = len(re.findall(r"\bv_(?:fma|fmac|mad|mac)_f32", body))
        print(f"\n{name}: {n}, {fused} fused multiply-adds")
        assert min(n["v_sub_f32"], n["v_mul_f32"], n["v_add_f32"]) >= 8 * 64
        assert n["v_div_fixup_f32"] >= 1 and fused <= 6 * n["v_div_fixup_f32"]


# ------------------------------------------------------------ f0_metrics ------------------------------------------------------------
def test_f0_metrics_on_planted_contours():
    from viettts_amd.pitch import f0_metrics

    rng = np.random.RandomState(3)
    n = 200
    ref = rng.uniform(80.0, 300.0, size=(2, n // 2)).astype(np.float32)
    m = f0_metrics(ref, ref)
    assert m == {"voicing_error": 0.0, "f0_rmse_cents": 0.0, "gross_error": 0.0, "voiced_frames": n}
    a = ref.copy()
    a[0, :13] *= 2.0  # an octave error in k = 13 of n frames
    m = f0_metrics(torch.from_numpy(a), torch.from_numpy(ref))
    assert m["gross_error"] == 13 / n and m["voicing_error"] == 0.0 and m["voiced_frames"] == n
    assert m["f0_rmse_cents"] == pytest.approx(1200.0 * (13 / n) ** 0.5, rel=1e-6)
    m = f0_metrics(ref.astype(np.float64) * 2.0 ** (10.0 / 1200.0), ref)  # 10 cents sharp everywhere
    assert m["f0_rmse_cents"] == pytest.approx(10.0, rel=1e-9) and m["gross_error"] == 0.0
    a = ref.copy()
    a[1, 5:12] = 0.0  # voicing flips in m = 7 frames, 4 of them the other way round
    b = ref.copy()
    b[0, 40:44] = 0.0
    m = f0_metrics(a, b)
    assert m["voicing_error"] == 11 / n and m["voiced_frames"] == n - 11 and m["f0_rmse_cents"] == 0.0
    # frames past a row's own count do not count
    m = f0_metrics(a, b, frames=[40, 5])
    assert m["voicing_error"] == 0.0 and m["voiced_frames"] == 45
    m = f0_metrics(a, b, frames=[44, 12])
    assert m["voicing_error"] == 11 / 56
    # nothing overlaps: nan, no exception
    m = f0_metrics(np.array([0.0, 100.0, 0.0]), np.array([120.0, 0.0, 0.0]))
    assert m["voiced_frames"] == 0 and np.isnan(m["f0_rmse_cents"]) and np.isnan(m["gross_error"]) and m["voicing_error"] == 2 / 3
    with pytest.raises(ValueError):
        f0_metrics(np.zeros(3), np.zeros(4))


def test_tracker_has_no_cpu_path_and_the_cli_parses(lib):
    from viettts_amd import pitch, resynth, vocoder_eval

    with pytest.raises(ValueError):
        pitch.PitchTracker(device="cpu")
    t = pitch.PitchTracker(device="cuda:0")  # host-side only: works without a GPU
    assert (t.tau_min, t.tau_max) == (32, 320) and t.num_frames(4096) == 16 and t.frames_per_workgroup == FPB
    t.close()
    t = pitch.PitchTracker(16000, 31.25, 8000.0, 0.2, device="cuda:0")
    assert (t.tau_min, t.tau_max) == (2, 512)
    t.close()
    with pytest.raises(_lib.VttsError):
        pitch.PitchTracker(fmin=30.0, device="cuda:0")
    a = pitch.build_parser().parse_args(["--wav", "a.wav"])
    assert (a.fmin, a.fmax, a.threshold, a.output) == (50.0, 500.0, 0.15, None)
    assert vocoder_eval.build_parser().parse_args(["--wav", "a.wav", "--generator", "g", "--discriminator", "d"]).f0 is False
    assert vocoder_eval.build_parser().parse_args(["--wav", "a.wav", "--generator", "g", "--discriminator", "d", "--f0"]).f0 is True
    assert resynth.build_parser().parse_args(["--input", "a.wav", "--output", "b.wav"]).f0 is False
    assert resynth.build_parser().parse_args(["--input", "a.wav", "--output", "b.wav", "--f0"]).f0 is True
