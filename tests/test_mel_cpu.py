"""The waveform -> log-mel front end (include/vtts_mel.h) as far as it goes without a GPU: exported symbols, the host-side
tables, the frame arithmetic, error paths, the fixture against its restatement, and the reference's import path."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import _mel_oracle as oracle
from viettts_amd import _lib

REPO = Path(__file__).resolve().parents[1]
GOLDEN = REPO / "tests" / "golden" / "mel_golden.npz"


@pytest.fixture(scope="module")
def lib():
    from viettts_amd.csrc.build import build

    build()
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def _create(lib, sr=16000, n_fft=1024, hop=256, n_mels=80, fmin=0.0, fmax=8000.0):
    h = C.c_void_p(0)
    cfg = _lib.MelCfg(sr, n_fft, hop, n_mels, fmin, fmax)
    return lib.vtts_mel_create(C.byref(cfg), 0, C.byref(h)), h


def test_header_symbols_all_exported(lib):
    header = (REPO / "include" / "vtts_mel.h").read_text()
    declared = set(re.findall(r"\b(vtts_mel_[a-z_0-9]+)\s*\(", header))
    assert declared == set(_lib.MEL_EXPORTS), declared ^ set(_lib.MEL_EXPORTS)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.vtts_abi_version() == 2  # the ABI is only added to
    assert int(re.search(r"#define VTTS_MEL_FRAMES_PER_BLOCK (\d+)", header).group(1)) == _lib.MEL_FRAMES_PER_BLOCK
    assert int(re.search(r"#define VTTS_MEL_MIN_SAMPLES (\d+)", header).group(1)) == _lib.MEL_MIN_SAMPLES


def test_mel_source_is_a_listed_translation_unit():
    from viettts_amd.csrc import build

    assert "mel.hip" in build.SOURCES and "-fno-slp-vectorize" in build.FILE_FLAGS["mel.hip"]
    assert any(str(h).endswith("vtts_mel.h") for h in build.HEADERS)


def test_filterbank_is_the_fixtures_basis(lib, golden):
    rc, h = _create(lib)
    assert rc == 0
    fb = np.empty((80, 513), dtype=np.float32)
    _lib.check(lib, lib.vtts_mel_filterbank(h, fb.ctypes.data_as(C.POINTER(C.c_float))))
    lib.vtts_mel_destroy(h)
    want = golden["melfb"].astype(np.float32)
    assert golden["melfb"].dtype == np.float64 and golden["melfb"].shape == (80, 513)
    assert np.all(np.abs(fb - want) <= np.spacing(np.abs(want))), float(np.abs(fb - want).max())  # one fp32 ulp per entry (0 where the basis is 0)
    assert np.all((fb > 0).sum(axis=1) > 0)  # every band has a non-zero weight
    assert np.all(fb >= 0) and int(((fb > 0).sum(axis=0)).max()) <= 2  # at most two bands per bin: what the kernel's band-per-lane loop relies on


def test_slaney_scale_knee():
    assert abs(float(oracle.hz_to_mel(1000.0)) - 15.0) < 1e-12
    assert abs(float(oracle.mel_to_hz(15.0)) - 1000.0) < 1e-9
    assert abs(float(oracle.mel_to_hz(oracle.hz_to_mel(6400.0))) - 6400.0) < 1e-9
    assert abs(float(oracle.hz_to_mel(6400.0)) - 42.0) < 1e-12  # logstep = ln(6.4) / 27: 6.4 kHz is 27 mels above the knee


def test_num_frames_is_the_formula(lib):
    rc, h = _create(lib)
    assert rc == 0
    n = C.c_int64(0)
    for S in list(range(385, 2001)) + [16484]:
        _lib.check(lib, lib.vtts_mel_num_frames(h, S, C.byref(n)))
        assert n.value == (S + 2 * 384 - 1024) // 256 + 1 == oracle.num_frames(S), S
        if S >= 256:
            assert n.value == S // 256
    lib.vtts_mel_destroy(h)


def test_oracle_reproduces_the_fixture(golden):
    """The fixture's mels were produced by the reference's programs (tools/make_mel_golden.py); the restatement the GPU tests use
    must not drift from them."""
    melfb = golden["melfb"]
    assert np.array_equal(oracle.slaney_filterbank(), melfb)
    for name, y in (("speech", golden["speech"].astype(np.float64)), ("pcm", golden["pcm"].astype(np.float64) / 32768.0), ("noise", golden["noise"].astype(np.float64))):
        got = oracle.log_mel(y, melfb)
        assert got.shape == golden["mel_" + name].shape
        assert np.abs(got - golden["mel_" + name]).max() <= 1e-12, name
        e32 = np.abs(oracle.log_mel(y.astype(np.float32), melfb, dtype=np.float32).astype(np.float64) - golden["mel_" + name]).max()
        assert 0 < float(golden["err_ref32_" + name]) < 1e-5
        assert abs(e32 - float(golden["err_ref32_" + name])) <= 0.5 * float(golden["err_ref32_" + name]), (name, e32)  # same arithmetic class on this host's FFT
    assert golden["speech"].shape == (4, 16484) and golden["speech"].dtype == np.float32
    assert golden["pcm"].dtype == np.int16 and golden["noise"].shape == (2, 8192)
    assert np.array_equal(golden["pcm"], np.rint(golden["speech"].astype(np.float64) * 32768.0).astype(np.int16))
    assert 385 in golden["lengths"].tolist() and GOLDEN.stat().st_size < 1 << 20


def test_error_paths(lib):
    def refused(status, **kw):
        rc, _ = _create(lib, **kw)
        assert rc == status and len(lib.vtts_last_error()) > 0, kw

    refused(-1, n_fft=1000, hop=250)  # not a power of two
    refused(-1, hop=512)  # hop != n_fft / 4
    refused(-1, n_fft=2048, hop=512)  # a configuration the kernel is not built for is refused, not approximated
    refused(-1, n_mels=129)
    refused(-1, n_mels=0)
    refused(-1, fmax=9000.0)  # above Nyquist
    refused(-1, fmin=8000.0)
    h = C.c_void_p(0)
    assert lib.vtts_mel_create(None, 0, C.byref(h)) == -1 and b"null" in lib.vtts_last_error()
    rc, h = _create(lib)
    assert rc == 0
    n, sz = C.c_int64(0), C.c_size_t(1)
    assert lib.vtts_mel_num_frames(h, 384, C.byref(n)) == -6 and b"385" in lib.vtts_last_error()
    assert lib.vtts_mel_num_frames(h, 385, None) == -1
    assert lib.vtts_mel_filterbank(h, None) == -1
    assert lib.vtts_mel_workspace_bytes(h, 2, 384, C.byref(sz)) == -6
    assert lib.vtts_mel_workspace_bytes(h, 0, 1024, C.byref(sz)) == -1
    assert lib.vtts_mel_workspace_bytes(h, 64, 262144, C.byref(sz)) == 0 and sz.value == 0
    assert lib.vtts_mel_packed_bytes(h, C.byref(sz)) == 0 and sz.value >= (1024 + 1024 + 514 + 1001) * 4
    # forward: null pointers, then call order (nothing was packed), before anything touches the GPU
    assert lib.vtts_mel_forward(h, None, 0, 1, 1024, None, C.c_void_p(256), 4, None, None) == -1
    assert lib.vtts_mel_forward(h, C.c_void_p(256), 0, 1, 1024, None, None, 4, None, None) == -1
    assert lib.vtts_mel_forward(h, C.c_void_p(256), 7, 1, 1024, None, C.c_void_p(256), 4, None, None) == -1 and b"dtype" in lib.vtts_last_error()
    assert lib.vtts_mel_forward(h, C.c_void_p(256), 0, 1, 1024, None, C.c_void_p(256), 4, None, None) == -2 and b"before pack" in lib.vtts_last_error()
    assert lib.vtts_mel_pack(h, None, 1 << 20, None) == -1
    assert lib.vtts_mel_bind_packed(h, C.c_void_p(256), 16) == -5
    # a bound blob (never dereferenced here: every call below is refused on the host)
    assert lib.vtts_mel_bind_packed(h, C.c_void_p(1 << 20), 1 << 20) == 0
    assert lib.vtts_mel_forward(h, C.c_void_p(256), 0, 1, 384, None, C.c_void_p(256), 4, None, None) == -6 and b"385" in lib.vtts_last_error()
    lens = (C.c_int32 * 2)(1024, 384)
    assert lib.vtts_mel_forward(h, C.c_void_p(256), 0, 2, 1024, lens, C.c_void_p(256), 4, None, None) == -6 and b"lengths[1]" in lib.vtts_last_error()
    lens = (C.c_int32 * 2)(1024, 1025)
    assert lib.vtts_mel_forward(h, C.c_void_p(256), 0, 2, 1024, lens, C.c_void_p(256), 4, None, None) == -6
    assert lib.vtts_mel_forward(h, C.c_void_p(256), 0, 1, 1024, None, C.c_void_p(256), 3, None, None) == -6 and b"T_stride" in lib.vtts_last_error()
    lib.vtts_mel_destroy(h)


def test_reference_import_path_and_signature():
    from vietTTS.nat.dsp import MelFilter
    import viettts_amd.nat.dsp as dsp

    assert MelFilter is dsp.MelFilter
    p = inspect.signature(MelFilter.__init__).parameters
    assert list(p)[:6] == ["self", "sample_rate", "n_fft", "n_mels", "fmin", "fmax"]
    assert p["fmin"].default == 0.0 and p["fmax"].default == 8000
    assert list(inspect.signature(MelFilter.__call__).parameters)[:2] == ["self", "y"]
    with pytest.raises(ValueError):
        MelFilter(16000, 1024, 80, device="cpu")  # no CPU path


def test_resynth_cli_needs_the_checkpoint(tmp_path, monkeypatch):
    from viettts_amd import resynth

    a = resynth.build_parser().parse_args(["--input", "a.wav", "--output", "b.wav"])
    assert a.dtype == "f32"
    monkeypatch.chdir(tmp_path)
    with pytest.raises(FileNotFoundError):
        resynth.main(["--input", "a.wav", "--output", "b.wav"])
