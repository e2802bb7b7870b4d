"""The audio stage (include/vtts_audio.h) as far as it goes without a GPU: the filter design's two conditions, the oracle against
scipy, the handle's host-side arithmetic against the oracle, refused configurations, exported symbols, the PCM16 WAV writer and the
command lines' new flags."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import _audio_oracle as oracle
from viettts_amd import _lib, wavio

REPO = Path(__file__).resolve().parents[1]
# (in_rate, out_rate) for L / M = 3/1, 1/2, 3/2, 441/160, 160/441, 320/441
RATES = [(16000, 48000), (16000, 8000), (16000, 24000), (16000, 44100), (44100, 16000), (44100, 32000)]
RATIOS = [(3, 1), (1, 2), (3, 2), (441, 160), (160, 441), (320, 441)]


@pytest.fixture(scope="module")
def lib():
    from viettts_amd.csrc.build import build

    build()
    return _lib.load()


def _create(lib, in_rate, out_rate):
    h = C.c_void_p(0)
    cfg = _lib.AudioCfg(in_rate, out_rate)
    return lib.vtts_audio_create(C.byref(cfg), 0, C.byref(h)), h


@pytest.mark.parametrize("rates,lm", list(zip(RATES, RATIOS)), ids=[f"{l}/{m}" for l, m in RATIOS])
def test_design_conditions(rates, lm):
    L, M, half = oracle.ratio(*rates)
    assert (L, M) == lm and half == 24 * max(L, M)
    h = oracle.prototype(*rates)
    assert h.shape == (2 * half + 1,)
    assert np.abs(h - h[::-1]).max() <= 1e-15 * L  # symmetric
    assert abs(h.sum() - L) <= 1e-12 * L
    nfft = 1 << int(np.ceil(np.log2(16 * h.size)))  # 16 points per tap: the response's ripples are resolved
    f, db = oracle.response_db(h, L, nfft)
    fc = 0.5 / max(L, M)  # the narrower Nyquist frequency, in cycles per sample of the prototype's rate
    passband, stopband = np.abs(db[f <= 0.85 * fc]).max(), db[f >= 1.15 * fc].max()
    print(f"\n{L}/{M}: passband deviation {passband:.2e} dB, stopband {stopband:.2f} dB")
    assert passband <= 0.001
    assert stopband <= -96.0


@pytest.mark.parametrize("rates", RATES + [(48000, 16000), (22050, 16000)], ids=lambda r: f"{r[0]}-{r[1]}")
def test_oracle_is_scipys_resample_poly(rates):
    signal = pytest.importorskip("scipy.signal")
    L, M, _ = oracle.ratio(*rates)
    rng = np.random.default_rng(3)
    for S in (1, 17, 3001):
        x = rng.standard_normal(S)
        want = signal.resample_poly(x, L, M, window=oracle.prototype(*rates) / L)
        got = oracle.resample(x, *rates)
        assert got.shape == want.shape == (oracle.out_samples(S, L, M),)
        assert np.abs(got - want).max() <= 1e-13
        # a window of the outputs is the same numbers
        a = got.shape[0] // 3
        assert np.array_equal(oracle.resample(x, *rates, start=a, count=got.shape[0] - a), got[a:])


def test_fp32_restatement_is_close_and_not_equal():
    rng = np.random.default_rng(4)
    x = oracle.speechlike(rng, 6000)
    for rates in RATES[:5]:
        want = oracle.resample(x, *rates)
        err = np.abs(oracle.resample(x, *rates, dtype=np.float32).astype(np.float64) - want).max()
        assert 0 < err < 1e-6 and np.abs(want).max() < 1.0, (rates, err)


@pytest.mark.parametrize("rates", RATES, ids=lambda r: f"{r[0]}-{r[1]}")
def test_handle_arithmetic_is_the_oracles(lib, rates):
    """create() touches no HIP call: ratio, out_samples and the prototype on a host without a GPU.  The prototype is computed by other
    code (a power series for I0, libm's sin) than numpy's: each tap is a handful of fp64 operations on values of at most 1, so the two
    agree to a few 1e-16 per tap times L from the normalisation; 1e-13 L leaves an order of magnitude."""
    rc, h = _create(lib, *rates)
    assert rc == 0, lib.vtts_last_error()
    L, M, half = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _lib.check(lib, lib.vtts_audio_ratio(h, C.byref(L), C.byref(M), C.byref(half)))
    assert (L.value, M.value, half.value) == oracle.ratio(*rates)
    _lib.check(lib, lib.vtts_audio_ratio(h, None, None, None))
    n = C.c_int64(0)
    for S in list(range(0, 1500)) + [6000, 13_500_000, 2**31 - 1]:
        _lib.check(lib, lib.vtts_audio_out_samples(h, S, C.byref(n)))
        assert n.value == oracle.out_samples(S, L.value, M.value), S
    got = np.empty(2 * half.value + 1, dtype=np.float64)
    _lib.check(lib, lib.vtts_audio_prototype(h, got.ctypes.data_as(C.POINTER(C.c_double))))
    want = oracle.prototype(*rates)
    assert np.abs(got - want).max() <= 1e-13 * L.value, float(np.abs(got - want).max())
    sz = C.c_size_t(0)
    _lib.check(lib, lib.vtts_audio_packed_bytes(h, C.byref(sz)))
    per_phase = -(-(2 * half.value + 1) // L.value)
    assert sz.value == 4 * L.value * (-(-per_phase // 4) * 4)
    lib.vtts_audio_destroy(h)


def test_refused_configurations_and_calls(lib):
    def refused(in_rate, out_rate, word):
        rc, _ = _create(lib, in_rate, out_rate)
        assert rc == -1 and word in lib.vtts_last_error(), (in_rate, out_rate, lib.vtts_last_error())

    refused(0, 16000, b"positive")
    refused(16000, 0, b"positive")
    refused(-16000, 16000, b"positive")
    refused(16000, 16001, b"2048")  # R = 16001
    refused(2049, 1, b"2048")
    refused(1, 2049, b"2048")
    refused(44100, 1000, b"span")  # 441 / 10 is inside the table, beyond the span a workgroup stages
    for ok in ((2048, 1025), (1, 2048), (16000, 16000), (48000, 8000), (192000, 8000)):
        rc, h = _create(lib, *ok)
        assert rc == 0, ok
        lib.vtts_audio_destroy(h)
    h = C.c_void_p(0)
    assert lib.vtts_audio_create(None, 0, C.byref(h)) == -1 and b"null" in lib.vtts_last_error()
    rc, h = _create(lib, 16000, 44100)
    assert rc == 0
    n, sz = C.c_int64(0), C.c_size_t(0)
    assert lib.vtts_audio_out_samples(h, -1, C.byref(n)) == -6
    assert lib.vtts_audio_out_samples(h, 5, None) == -1
    assert lib.vtts_audio_prototype(h, None) == -1
    assert lib.vtts_audio_packed_bytes(h, None) == -1
    fwd = lib.vtts_audio_forward
    p = C.c_void_p(256)
    # null pointers, dtypes, then call order (nothing was packed): all before anything touches the GPU
    assert fwd(h, None, 0, 1, 1024, None, p, 0, 0, None) == -1
    assert fwd(h, p, 0, 1, 1024, None, None, 0, 0, None) == -1
    assert fwd(h, p, 2, 1, 1024, None, p, 0, 0, None) == -1 and b"dtype" in lib.vtts_last_error()
    assert fwd(h, p, 0, 1, 1024, None, p, 7, 0, None) == -1 and b"dtype" in lib.vtts_last_error()
    assert fwd(h, p, 0, 1, 1024, None, p, 0, 0, None) == -2 and b"before pack" in lib.vtts_last_error()
    assert lib.vtts_audio_pack(h, None, 1 << 20, None) == -1
    assert lib.vtts_audio_bind_packed(h, p, 16) == -5
    assert lib.vtts_audio_bind_packed(h, C.c_void_p(1 << 20 | 64), 1 << 20) == -1 and b"aligned" in lib.vtts_last_error()
    # a bound blob (never dereferenced here: every call below is refused on the host)
    assert lib.vtts_audio_bind_packed(h, C.c_void_p(1 << 20), 1 << 20) == 0
    assert fwd(h, p, 0, 0, 1024, None, p, 0, 0, None) == -1
    assert fwd(h, p, 0, 1, 0, None, p, 0, 0, None) == -6
    assert fwd(h, p, 0, 1, 1024, None, p, 0, -1, None) == -6
    assert fwd(h, p, 0, 1, 1024, None, p, 0, 2822, None) == -6 and b"O_stride" in lib.vtts_last_error()  # ceil(1024 * 441 / 160) = 2823
    lens = (C.c_int32 * 2)(1024, 1025)
    assert fwd(h, p, 0, 2, 1024, lens, p, 0, 0, None) == -6 and b"lengths[1]" in lib.vtts_last_error()
    lens = (C.c_int32 * 2)(-1, 5)
    assert fwd(h, p, 0, 2, 1024, lens, p, 0, 0, None) == -6 and b"lengths[0]" in lib.vtts_last_error()
    lib.vtts_audio_destroy(h)


def test_header_symbols_all_exported(lib):
    header = (REPO / "include" / "vtts_audio.h").read_text()
    declared = set(re.findall(r"\b(vtts_audio_[a-z_0-9]+)\s*\(", header))
    assert declared == set(_lib.AUDIO_EXPORTS), declared ^ set(_lib.AUDIO_EXPORTS)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.vtts_abi_version() == 2  # the ABI is only added to
    assert int(re.search(r"#define VTTS_AUDIO_OUT_PER_BLOCK (\d+)", header).group(1)) == _lib.AUDIO_OUT_PER_BLOCK
    assert int(re.search(r"#define VTTS_AUDIO_ZEROS (\d+)", header).group(1)) == _lib.AUDIO_ZEROS == oracle.ZEROS
    assert float(re.search(r"#define VTTS_AUDIO_BETA ([0-9.]+)", header).group(1)) == _lib.AUDIO_BETA == oracle.BETA
    assert int(re.search(r"#define VTTS_AUDIO_MAX_R (\d+)", header).group(1)) == _lib.AUDIO_MAX_R == 2048
    assert (_lib.VTTS_AUDIO_F32, _lib.VTTS_AUDIO_PCM16) == (0, 1)


def test_audio_source_is_a_listed_translation_unit():
    from viettts_amd.csrc import build

    assert "audio.hip" in build.SOURCES and "-fno-slp-vectorize" in build.FILE_FLAGS["audio.hip"]
    assert any(str(h).endswith("vtts_audio.h") for h in build.HEADERS) and "audio_design.h" in build.HEADERS


def test_write_wav_pcm16_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    pcm = rng.integers(-32768, 32768, size=4801, dtype=np.int16)
    pcm[:2] = (-32768, 32767)
    wavio.write_wav_pcm16(tmp_path / "a.wav", pcm, 48000)
    sr, back = wavio.read_wav(tmp_path / "a.wav")
    assert sr == 48000 and back.dtype == np.int16 and np.array_equal(back, pcm)
    # the same bytes as write_wav of samples that convert to this PCM
    x = pcm.astype(np.float64) / 32767.0
    assert np.array_equal(wavio.float_to_pcm16(x), np.maximum(pcm, -32767))
    wavio.write_wav(tmp_path / "b.wav", x, 48000)
    wavio.write_wav_pcm16(tmp_path / "c.wav", wavio.float_to_pcm16(x).astype(np.int16), 48000)
    assert (tmp_path / "b.wav").read_bytes() == (tmp_path / "c.wav").read_bytes()
    with pytest.raises(ValueError):
        wavio.write_wav_pcm16(tmp_path / "d.wav", pcm.astype(np.float32), 48000)
    with pytest.raises(ValueError):
        wavio.write_wav_pcm16(tmp_path / "d.wav", pcm[None, :], 48000)


def test_new_cli_flags_parse_and_defaults_stay():
    from viettts_amd import resynth, synthesizer, vocoder_eval

    a = resynth.build_parser().parse_args(["--input", "a.wav", "--output", "b.wav"])
    assert (a.dtype, a.output_rate) == ("f32", None)
    assert resynth.build_parser().parse_args(["--input", "a.wav", "--output", "b.wav", "--output-rate", "48000"]).output_rate == 48000
    s = synthesizer.build_parser().parse_args([])
    assert (s.sample_rate, s.resample, s.low_latency, s.silence_duration, str(s.output)) == (16000, False, False, -1, "clip.wav")
    s = synthesizer.build_parser().parse_args(["--sample-rate", "22050", "--resample"])
    assert (s.sample_rate, s.resample) == (22050, True)
    v = vocoder_eval.build_parser().parse_args(["--wav", "a.wav", "--generator", "g", "--discriminator", "d"])
    assert (v.segment, v.batch, v.config) == (8192, 16, "assets/hifigan/config.json")
    import inspect

    from viettts_amd.pipeline import synthesize_sentences

    p = inspect.signature(synthesize_sentences).parameters
    assert p["out_dtype"].default == "f32" and p["out_rate"].default is None
    assert inspect.signature(resynth.resynthesize).parameters["in_rate"].default is None


def test_resampler_has_no_cpu_path(lib):
    from viettts_amd.audio import Resampler

    with pytest.raises(ValueError):
        Resampler(48000, 16000, device="cpu")
