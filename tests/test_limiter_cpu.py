"""include/vtts_limiter.h without a GPU: the numpy restatement (tests/_limiter_oracle.py) against the properties the header promises and against
tests/_audio_oracle.py, its float32 mode against its float64 mode on the GPU test's rows (the GPU tests' bound), and the C ABI's host side."""
import ctypes as C
import re

import numpy as np
import pytest

import _audio_oracle as A
import _limiter_oracle as O
from viettts_amd import _lib

FS, W = 16000, 80
EPS = 2.0 ** -23


@pytest.fixture(scope="module")
def lib():
    from viettts_amd.csrc.build import build

    build()
    return _lib.load()


def _create(lib, rate=16000, ms=5.0):
    h = C.c_void_p(0)
    rc = lib.vtts_limiter_create(C.byref(_lib.LimiterCfg(rate, ms)), 0, C.byref(h))
    return rc, h


def _noise(seed, S, amp=1.0):
    return (amp * np.random.default_rng(seed).uniform(-1.0, 1.0, S)).astype(np.float32)


def _click(S, *at, base=0.0):
    x = np.full(S, base, np.float32)
    for k in at:
        x[k] = 1.0
    return x


# ------------------------------------------------------------ the oracle ------------------------------------------------------------
@pytest.mark.parametrize("rate", [16000, 22050, 48000])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_oversampled_signal_is_the_audio_oracles(rate, dtype):
    """u, written out again in _limiter_oracle, equals _audio_oracle.resample(x, fs, 4 fs) exactly: in float64 and in the float32 chain."""
    for x in (O.speech(1, 3001, rate), _click(200, 0, 199), O.tone(rate / 4, 1.0, 777, rate, np.pi / 4), np.zeros(1, np.float32) + 0.5):
        assert np.array_equal(O.oversample(x, rate, dtype), A.resample(x, rate, 4 * rate, dtype=dtype))
    assert O.oversample(np.zeros(0, np.float32), rate, dtype).shape == (0,) and O.true_peak(np.zeros(0, np.float32), rate) == 0.0
    assert A.ratio(rate, 4 * rate) == (4, 1, 96) and O.NJ == 49 <= O.K["VTTS_LIMITER_PHASE_TAPS"]


def test_quarter_rate_sine_at_45_degrees_reads_its_true_peak():
    """Sample peak 0.7071, true peak 1.0: away from the ends the oracle reads 1.0 within 4.9e-7 (measured; the bound is 1e-6).  The zero-extended
    ends ring: 1.011 there, which is the row's true_peak by the contract."""
    x = O.tone(FS / 4, 1.0, 4000, FS, np.pi / 4)
    p = O.envelope(x, FS)
    print(f"\nsample peak {np.abs(x).max():.6f}, true peak inside {p[200:-200].max():.9f}, at the ends {p.max():.6f}")
    assert abs(float(np.abs(x).max()) - np.sqrt(0.5)) <= 1e-6
    assert abs(p[200:-200].max() - 1.0) <= 1e-6
    assert (np.abs(np.maximum(p[200:-201], p[201:-200]) - 1.0) <= 1e-6).all()  # a crest every second sample, between two samples at 0.7071
    assert 1.0 < p.max() <= 1.02
    # the factor's worst case, at the Nyquist frequency and at half of it
    assert abs(-20 * np.log10(np.cos(np.pi / 8)) - 0.688) <= 1e-3 and abs(-20 * np.log10(np.cos(np.pi / 16)) - 0.169) <= 1e-3


ROWS = {
    "speech": (O.speech(11, 9000), 4.0),
    "tone": (O.tone(3777.0, 0.9, 6000, FS, 0.3), 1.7),
    "clicks": (_click(5000, 0, 1234, 1300, 4999) * np.float32(0.8) + O.speech(12, 5000) * np.float32(0.1), 2.0),
    "noise": (_noise(13, 7000), 2.0),
}


@pytest.mark.parametrize("name", list(ROWS))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_gain_never_passes_what_a_sample_asks_for_and_the_sample_peak_holds(name, dtype):
    x, g = ROWS[name]
    r = O.limit(x, FS, g, dtype=dtype)
    assert (r.a <= r.req).all() and (r.a > 0).all() and (r.held <= r.req).all()
    slack = 1 + 1e-15 if dtype is np.float64 else (1 + EPS) ** 2
    assert np.abs(r.y).max() <= float(r.c) * slack
    assert r.min_gain < 1.0 and r.true_peak * g > float(r.c)
    over = O.overshoot_db(r.y, FS, r.c)
    print(f"\n{name} {np.dtype(dtype).name}: min gain {r.min_gain:.4f}, sample peak {np.abs(r.y).max():.7f}, true peak {over:+.4f} dB over the ceiling")
    assert over <= 0.05  # (not a bound of the contract; a float64 prototype showed 0.0001 .. 0.004 dB on speech and 0.014 dB on white noise)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_row_under_the_ceiling_is_multiplied_and_nothing_else(dtype):
    x = O.speech(14, 5000)
    g = np.float32(1.3)
    r = O.limit(x, FS, g, dtype=dtype)
    assert r.true_peak * g <= float(r.c)
    assert (r.a == 1.0).all() and r.min_gain == 1.0
    assert np.array_equal(r.y, (np.dtype(dtype).type(g) * x.astype(dtype)).astype(dtype))


def test_an_isolated_peak_dips_once_and_recovers_after_two_windows():
    """On the gain computer alone (an envelope with one sample over the ceiling): a = c / (g p) at the peak, strictly between that and 1 within
    2 W of it, and exactly 1 outside."""
    c, g, k, S = O.ceiling(), 2.0, 1000, 2000
    p = np.full(S, 0.1)
    p[k] = 1.0
    req, held, a = O.gain_curve(p, g, c, W)
    assert abs(a[k] - float(c) / 2.0) <= 1e-15 and a[k] == a.min()
    assert (held[k - W:k + W + 1] == req[k]).all() and (held[:k - W] == 1).all() and (held[k + W + 1:] == 1).all()
    assert (a[:k - 2 * W] == 1.0).all() and (a[k + 2 * W + 1:] == 1.0).all()
    inside = np.r_[a[k - 2 * W:k], a[k + 1:k + 2 * W + 1]]
    assert ((inside < 1.0) & (inside > a[k])).all()
    assert (np.diff(a[k - 2 * W - 1:k + 1]) < 0).all() and (np.diff(a[k:k + 2 * W + 2]) > 0).all()  # a ramp down, a ramp up
    # the same on a waveform: the click rings into its neighbours' envelope, and the dip still ends 2 W past the last of them
    r = O.limit(_click(S, k), FS, g)
    over = np.flatnonzero(r.req < 1.0)
    assert over.min() >= k - 2 and over.max() <= k + 1 and r.a[k] == r.req[k] == r.a.min()
    assert (r.a[:over.min() - 2 * W] == 1.0).all() and (r.a[over.max() + 2 * W + 1:] == 1.0).all() and (r.a[over.min() - 2 * W:over.max() + 2 * W + 1] < 1.0).all()


def test_two_peaks_merge_at_two_windows_and_separate_past_four():
    c, g, S, k = O.ceiling(), 2.0, 3000, 1000
    for gap in (2 * W, 4 * W + 1, 4 * W + 2):
        p = np.full(S, 0.1)
        p[k] = p[k + gap] = 1.0
        req, held, a = O.gain_curve(p, g, c, W)
        between = a[k:k + gap + 1]
        if gap == 2 * W:        # every window between the peaks holds one of them: the gain stays at the floor
            assert np.abs(between - req[k]).max() <= 1e-15
        elif gap == 4 * W + 1:  # two dips: the two samples in the middle meet one held value under 1 each, all the others are back at 1
            top = (2 * W + req[k]) / (2 * W + 1)
            assert abs(between[2 * W] - top) <= 1e-15 and abs(between[2 * W + 1] - top) <= 1e-15 and between.max() <= top + 1e-15 < 1.0
            assert (np.diff(between[:2 * W + 1]) > 0).all() and (np.diff(between[2 * W + 1:]) < 0).all()
        else:                   # one sample further apart, exactly one sample between them is at 1
            assert (between == 1.0).sum() == 1 and between[2 * W + 1] == 1.0


def test_peaks_at_a_rows_ends_use_the_clamped_windows():
    c, g, S = O.ceiling(), 2.0, 1000
    for k in (0, S - 1):
        p = np.full(S, 0.1)
        p[k] = 1.0
        req, held, a = O.gain_curve(p, g, c, W)
        assert abs(a[k] - req[k]) <= 1e-15 and (a <= req).all()
        far = a[2 * W + 1:] if k == 0 else a[:S - 1 - 2 * W]
        assert (far == 1.0).all()
        near = a[1:2 * W + 1] if k == 0 else a[S - 1 - 2 * W:S - 1]
        assert ((near < 1.0) & (near > a[k])).all()
        # edge replication counts the end sample's held value once per clamped index: next to the end, W clamped terms and W inside
        # the row are at the floor and one is 1 (cut off at the end instead, the mean would be over W + 2 terms)
        n = 1 if k == 0 else S - 2
        assert abs(a[n] - (req[k] * (2 * W) + 1.0) / (2 * W + 1)) <= 1e-15
    for S1 in (1, 2, W, 2 * W + 1):  # rows shorter than a window: all of it clamps
        r = O.limit(O.speech(20 + S1, S1), FS, 4.0)
        assert (r.a <= r.req).all() and r.a.shape == (S1,) and np.abs(r.y).max() <= float(r.c) * (1 + 1e-15)


def test_float32_restatement_against_float64_on_the_gpu_tests_rows():
    """The GPU tests' bound is 4 x this distance (the loudness and STOI tests' rule).  Measured: 5.6e-7; the taps' and
    chains' roundings are 2^-24 relative on samples up to 0.9, so a distance above a few 1e-6 would mean the restatement is not the contract."""
    f64, f32, d = O.gpu_reference()
    print(f"\nfloat32 restatement within {d:.3e} of float64 over {sum(r.y.size for r in f64)} samples: bound {4 * d:.3e}")
    assert 0 < d <= 4e-6
    names = [n for n, _, _ in O.gpu_rows()]
    assert {"clicks", "pairs", "plateau", "under", "len0", f"len{O.TILE}", f"len{O.TILE + 2 * W + 1}"} <= set(names)
    for (n, x, g), a, b in zip(O.gpu_rows(), f64, f32):
        if a.y.size:
            assert (b.a <= b.req).all() and np.abs(b.y).max() <= float(b.c) * (1 + EPS) ** 2, n
            assert (a.min_gain < 1.0) == (n != "under"), n
    over = {n: O.overshoot_db(r.y, FS, r.c) for (n, _, _), r in zip(O.gpu_rows(), f64) if r.y.size}
    print("largest true-peak overshoot of the float64 outputs: %.4f dB (%s)" % (max(over.values()), max(over, key=over.get)))
    assert max(over.values()) <= 0.05
    want = {"speech+3dB": 3.0, "speech+6dB": 6.0, "speech+12dB": 12.0}
    for (n, x, g), r in zip(O.gpu_rows(), f64):
        if n in want:
            assert abs(20 * np.log10(r.true_peak * float(g) / float(r.c)) - want[n]) <= 1e-3


def test_edge_lengths_meet_the_kernels_edges():
    L = O.edge_lengths(FS)
    T = O.TILE
    assert L[:-1] == [0, 1, 2, W, W + 1, 2 * W, 2 * W + 1, 4 * W + 2, T - 1, T, T + 1, T + 2 * W - 1, T + 2 * W + 1, 2 * T + 1] and L[-1] >= 3 * FS
    assert O.lookahead(FS) == W and O.RUN == 16 and T == 4096 == 256 * O.RUN


def test_pregain_rule():
    assert O.pregain(-np.inf) == 1.0 and O.pregain(np.nan) == 1.0 and O.pregain(np.inf) == 1.0
    assert O.pregain(-29.0, -23.0) == np.float32(10 ** 0.3) and O.pregain(-70.0, -23.0) == np.float32(10 ** 1.5) and O.pregain(-10.0, -23.0) < 1.0


# ------------------------------------------------------------ the C ABI's host side ------------------------------------------------------------
def test_header_symbols_all_exported(lib):
    declared = set(re.findall(r"\b(vtts_limiter_[a-z_0-9]+)\s*\(", O.HEADER.read_text()))
    assert declared == set(_lib.LIMITER_EXPORTS) == {f"vtts_limiter_{n}" for n in ("create", "destroy", "lookahead", "taps", "workspace_bytes", "true_peak",
                                                                                   "pregain", "apply")}
    for name in declared:
        assert hasattr(lib, name), name
        fn = getattr(lib, name)
        assert fn.restype is _lib.LIMITER_SIGS[name][0] and list(fn.argtypes) == _lib.LIMITER_SIGS[name][1]
    assert (O.K["VTTS_LIMITER_TILE"], O.K["VTTS_LIMITER_RUN"], O.K["VTTS_LIMITER_PHASE_TAPS"]) == (_lib.LIMITER_TILE, _lib.LIMITER_RUN, _lib.LIMITER_PHASE_TAPS)
    assert (O.K["VTTS_LIMITER_MIN_RATE"], O.K["VTTS_LIMITER_MAX_RATE"]) == (_lib.LIMITER_MIN_RATE, _lib.LIMITER_MAX_RATE)
    assert not set(_lib.LIMITER_SIGS) & (set(_lib.SIGS) | set(_lib.LOUDNESS_SIGS))
    assert not re.search(r"vtts_loudness_[a-z_0-9]+\s*\(", O.HEADER.read_text())


def test_limiter_hip_is_built_without_packed_f32():
    from viettts_amd.csrc import build

    assert "limiter.hip" in build.SOURCES and "-fno-slp-vectorize" in build.FILE_FLAGS["limiter.hip"]
    assert any(str(h).endswith("vtts_limiter.h") for h in build.HEADERS) and "audio_design.h" in build.HEADERS
    src = (build.CSRC / "limiter.hip").read_text()
    common = (build.CSRC / "limiter_common.h").read_text()
    # the design is reused, not restated: both create()s reach it through limiter_common.h's configure()
    assert "asm" not in src and '#include "limiter_common.h"' in src and '#include "audio_design.h"' in common and "limiter_common.h" in build.HEADERS
    for text in (src, common, (build.CSRC / "limiter_stream.hip").read_text()):
        assert "kaiser" not in text.lower()
    assert "ad::design(" in common and "ad::design(" not in src and "ad::design(" not in (build.CSRC / "limiter_stream.hip").read_text()


@pytest.mark.parametrize("rate", [8000, 16000, 22050, 48000])
def test_taps_are_the_audio_stages_prototype_rounded_once(lib, rate):
    rc, h = _create(lib, rate)
    assert rc == 0
    got = np.zeros((4, 52), np.float32)
    assert lib.vtts_limiter_taps(h, got.ctypes.data_as(_lib.fp)) == 0
    proto = A.prototype(rate, 4 * rate)
    want = np.zeros((4, 52), np.float32)
    for p in range(4):
        for j in range(52):
            if p + 4 * j <= 192:
                want[p, 51 - j] = np.float32(proto[p + 4 * j])
    assert np.array_equal(got, want) and (got[0, :3] == 0).all() and (got[1:, :4] == 0).all() and got[0, 3] != 0
    lib.vtts_limiter_destroy(h)


def test_create_refuses_rates_and_lookaheads_outside_the_contract(lib):
    w = C.c_int32(0)
    for rate, ms, want in ((8000, 5.0, 40), (16000, 5.0, 80), (22050, 5.0, 110), (44100, 5.0, 221), (48000, 5.0, 240), (96000, 5.0, 480), (96000, 10.0, 960),
                           (16000, 2.0, 32), (8000, 0.01, 1), (11025, 5.0, 55), (16001, 1.0, 16)):
        rc, h = _create(lib, rate, ms)
        assert rc == 0, (rate, ms)
        assert lib.vtts_limiter_lookahead(h, C.byref(w)) == 0 and w.value == want == O.lookahead(rate, ms), (rate, ms, w.value)
        lib.vtts_limiter_destroy(h)
    for rate, ms in ((7999, 5.0), (96001, 5.0), (0, 5.0), (-16000, 5.0), (16000, 0.0), (16000, -1.0), (16000, 10.5), (16000, float("nan")), (16000, float("inf"))):
        rc, _ = _create(lib, rate, ms)
        assert rc == -1 and lib.vtts_last_error(), (rate, ms)
    _create(lib, 4000)
    assert b"8000 .. 96000" in lib.vtts_last_error()
    _create(lib, 16000, 11.0)
    assert b"lookahead_ms" in lib.vtts_last_error()
    assert lib.vtts_limiter_create(None, 0, C.byref(C.c_void_p(0))) == -1
    lib.vtts_limiter_destroy(None)


def test_calls_refuse_bad_arguments_before_any_launch(lib):
    """No GPU here: every refusal below has to come from host arithmetic.  The pointers are never dereferenced."""
    rc, h = _create(lib)
    assert rc == 0
    fake = C.c_void_p(0x1000)
    i32 = lambda *v: (C.c_int32 * len(v))(*v)  # noqa: E731
    ws = C.c_size_t(0)
    assert lib.vtts_limiter_workspace_bytes(h, 2, 48000, C.byref(ws)) == 0
    assert ws.value == (2 * 12 * 4096 + 2 * 2 * 12) * 4  # the envelope over whole tiles, and two slots per tile
    small = C.c_size_t(0)
    assert lib.vtts_limiter_workspace_bytes(h, 1, 0, C.byref(small)) == 0 and 0 < small.value <= 16
    assert lib.vtts_limiter_workspace_bytes(h, 0, 48000, C.byref(small)) == -1 and lib.vtts_limiter_workspace_bytes(h, 1, -1, C.byref(small)) == -6
    assert lib.vtts_limiter_workspace_bytes(h, 1, 2 ** 31 - 1, C.byref(small)) == -6

    def peak(dtype=0, N=2, S=48000, lengths=None, out=fake, wsp=fake, wsb=None):
        return lib.vtts_limiter_true_peak(h, fake, dtype, N, S, lengths, out, None, wsp, ws.value if wsb is None else wsb, None)

    assert peak(dtype=2) == -1 and peak(N=0) == -1 and peak(out=None) == -1 and peak(wsp=None) == -1
    assert peak(lengths=i32(48000, 48001)) == -6 and b"lengths[1]" in lib.vtts_last_error()
    assert peak(lengths=i32(-1, 48000)) == -6
    assert peak(wsb=ws.value - 16) == -5 and peak(wsp=C.c_void_p(0x1008)) == -1
    assert lib.vtts_limiter_true_peak(h, None, 0, 2, 48000, None, fake, None, fake, ws.value, None) == -1

    def apply(dtype=0, N=2, S=48000, lengths=None, ceiling=-1.0, odt=1, O_stride=48000, out=fake, tp=fake, mg=fake, gu=fake, wsp=fake, wsb=None):
        return lib.vtts_limiter_apply(h, fake, dtype, N, S, lengths, None, ceiling, out, odt, O_stride, tp, mg, gu, None, wsp, ws.value if wsb is None else wsb, None)

    assert apply(dtype=3) == -1 and apply(odt=2) == -1 and apply(N=0) == -1
    assert apply(out=None) == -1 and apply(tp=None) == -1 and apply(mg=None) == -1 and apply(gu=None) == -1 and apply(wsp=None) == -1
    assert apply(ceiling=float("nan")) == -1 and apply(ceiling=float("inf")) == -1
    assert apply(O_stride=47999) == -6 and b"O_stride" in lib.vtts_last_error()
    assert apply(O_stride=-1) == -6
    assert apply(lengths=i32(5, 48001)) == -6
    assert apply(wsb=ws.value - 16) == -5 and apply(wsp=C.c_void_p(0x1004)) == -1

    def pregain(N=2, target=-23.0, mg=30.0, i=fake, g=fake):
        return lib.vtts_limiter_pregain(h, i, N, target, mg, g, None)

    assert pregain(N=0) == -1 and pregain(i=None) == -1 and pregain(g=None) == -1
    assert pregain(target=float("nan")) == -1 and pregain(target=float("-inf")) == -1 and pregain(mg=float("nan")) == -1
    lib.vtts_limiter_destroy(h)


def test_python_module_states_its_interface():
    import inspect

    from viettts_amd import limiter, pipeline, resynth, synthesizer

    a = limiter.build_parser().parse_args(["--wav", "x.wav"])
    assert (a.wav, a.target, a.output, a.ceiling_dbtp, a.max_gain_db, a.lookahead_ms) == ("x.wav", None, None, -1.0, 30.0, 5.0)
    a = limiter.build_parser().parse_args(["--wav", "x.wav", "--target", "-16", "--ceiling-dbtp", "-2", "--output", "y.wav"])
    assert (a.target, a.ceiling_dbtp, a.output) == (-16.0, -2.0, "y.wav")
    assert limiter.LimiterResult._fields == ("true_peak", "min_gain", "gains", "envelope")
    with pytest.raises(ValueError):
        limiter.TruePeakLimiter(16000, device="cpu")
    sig = inspect.signature(limiter.TruePeakLimiter.__init__).parameters
    assert (sig["sample_rate"].default, sig["device"].default, sig["lookahead_ms"].default) == (16000, "cuda:0", 5.0)
    sig = inspect.signature(limiter.TruePeakLimiter.limit).parameters
    assert [sig[k].default for k in ("lengths", "gains", "ceiling_dbtp", "out_dtype", "packed", "envelope")] == [None, None, -1.0, "f32", False, False]
    sig = inspect.signature(limiter.TruePeakLimiter.normalize).parameters
    assert [sig[k].default for k in ("target", "ceiling_dbtp", "max_gain_db", "out_dtype", "packed", "meter")] == [-23.0, -1.0, 30.0, "f32", False, None]
    # the hooks are off by default
    assert inspect.signature(pipeline.synthesize_sentences).parameters["limit"].default is False
    assert synthesizer.build_parser().parse_args([]).limit is False and synthesizer.build_parser().parse_args(["--loudness", "-16", "--limit"]).limit is True
    assert resynth.build_parser().parse_args(["--input", "a.wav", "--output", "b.wav"]).limit is False
    with pytest.raises(SystemExit):
        synthesizer.main(["--text", "xin chào", "--limit"])
    with pytest.raises(ValueError):
        pipeline.synthesize_sentences([[1]], None, None, None, limit=True)
