"""include/vtts_stoi.h without a GPU: the numpy restatement (tests/_stoi_oracle.py) against the properties STOI and ESTOI are known by, its
gather form of stage B against the overlap-add form, the band table against its derivation, the bound the GPU test uses and what that bound
can see, and the C ABI's host side."""
import ctypes as C
import re

import numpy as np
import pytest

import _stoi_oracle as O
from viettts_amd import _lib


@pytest.fixture(scope="module")
def lib():
    from viettts_amd.csrc.build import build

    build()
    return _lib.load()


def _create(lib):
    h = C.c_void_p(0)
    rc = lib.vtts_stoi_create(0, C.byref(h))
    return rc, h


# ------------------------------------------------------------ the oracle ------------------------------------------------------------
def test_band_table_equals_its_derivation():
    lo, hi = O.derive_bands()
    assert lo == O.BAND_LO[:-1] == (7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174)
    assert hi == O.BAND_LO[1:] and hi[-1] == 219  # every band ends where the next begins; the last before bin 219
    head = O.HEADER.read_text()
    assert "lo = " + ", ".join(map(str, O.BAND_LO)) in head


@pytest.mark.parametrize("i", range(len(O.CASES)))
def test_gather_form_equals_overlap_add_form_exactly(i):
    x, y = O.case(i)
    a, b = O.case_reference(i)[0], O.measure(x, y, ola=True)
    assert a.n_kept < a.n_frames  # frames really drop: the two forms differ in more than a copy
    assert a.mags.shape == b.mags.shape and np.all(a.mags == b.mags)
    assert np.all(a.stoi_series == b.stoi_series) and np.all(a.estoi_series == b.estoi_series) and (a.stoi, a.estoi) == (b.stoi, b.estoi)


def test_a_signal_against_itself_scores_one():
    for i in (0, 3):
        x, _ = O.case(i)
        r = O.measure(x, x)
        assert r.n_segments > 0 and abs(r.stoi - 1.0) <= 1e-12 and abs(r.estoi - 1.0) <= 1e-12


def test_both_figures_fall_as_noise_rises():
    x, _ = O.case(2)
    got = [O.measure(x, O.degrade(x, 7, level)) for level in (0.1, 0.5, 2.0)]
    print("\n" + "  ".join(f"{r.stoi:.4f}/{r.estoi:.4f}" for r in got))
    assert 1.0 > got[0].stoi > got[1].stoi > got[2].stoi > 0.0
    assert 1.0 > got[0].estoi > got[1].estoi > got[2].estoi > 0.0


def test_scaling_the_processed_signal_changes_nothing():
    for i in (1, 2):
        x, y = O.case(i)
        y64 = y.astype(np.float64)  # (0.01 y in float32 would be rounded again, 6e-8 relative per sample: the property is stated on exact values)
        a, b = O.measure(x, y64), O.measure(x, 0.01 * y64)
        assert a.n_segments > 0 and abs(a.stoi - b.stoi) <= 1e-12 and abs(a.estoi - b.estoi) <= 1e-12
        c = O.measure(x, (np.float32(0.01) * y).astype(np.float32))  # ... and rounded again, it moves by that rounding alone
        assert abs(a.stoi - c.stoi) <= 1e-7 and abs(a.estoi - c.estoi) <= 1e-7


@pytest.mark.parametrize("S,K,M", [(0, 0, 0), (256, 0, 0), (257, 1, 0), (4096, 30, 0), (4097, 31, 1), (4224, 31, 1), (4225, 32, 2)])
def test_frame_and_segment_counts_at_the_edges(lib, S, K, M):
    assert O.counts(S) == (K, M)
    x = O.make_speechlike(max(S, 1), 11)[:S]
    r = O.measure(x, x)
    assert (r.n_frames, r.n_kept, r.n_segments) == (K, K, M)  # nothing quiet in it: every frame is kept
    assert (r.stoi != r.stoi) == (M == 0) and (r.estoi != r.estoi) == (M == 0)
    rc, h = _create(lib)
    n = C.c_int64(-1)
    assert rc == 0 and lib.vtts_stoi_num_frames(h, S, C.byref(n)) == 0 and n.value == K
    lib.vtts_stoi_destroy(h)


def test_silence_keeps_nothing():
    r = O.measure(np.zeros(9001, np.float32), np.zeros(9001, np.float32))
    assert (r.n_frames, r.n_kept, r.n_segments) == (69, 0, 0) and r.stoi != r.stoi


def test_bound_is_derived_and_under_the_cap():
    b = O.bounds()
    print(f"\nfloat32 restatement within {b.scale_mags:.2e} (band magnitudes, relative), {b.scale_series:.2e} (segments), {b.scale_mean:.2e} (figures) "
          f"of float64; bounds {b.mags:.2e}, {b.series:.2e}, {b.mean:.2e}")
    assert 0.0 < b.mean == O.BOUND_FACTOR * b.scale_mean <= O.BOUND_CAP
    assert 0.0 < b.series == O.BOUND_FACTOR * b.scale_series <= O.BOUND_CAP
    assert 0.0 < b.mags == O.BOUND_FACTOR * b.scale_mags <= 1e-5
    assert [c[0] for c in O.CASES] == sorted(c[0] for c in O.CASES) and 4225 <= O.CASES[0][0] and O.CASES[-1][0] <= 20000
    assert len({c[2] for c in O.CASES}) == 2  # two noise levels


@pytest.mark.parametrize("fault", O.FAULTS)
def test_the_bound_sees_each_planted_fault(fault):
    """Each fault moves STOI or ESTOI of every row the GPU test meters by more than ten times the accuracy bound."""
    bound = O.bounds().mean
    moves = []
    for i in range(len(O.CASES)):
        x, y = O.case(i)
        a, b = O.case_reference(i)[0], O.measure(x, y, fault=fault)
        moves.append(max(abs(a.stoi - b.stoi), abs(a.estoi - b.estoi)) if b.n_segments else float("inf"))
    print(f"\n{fault}: " + " ".join(f"{m:.1e}" for m in moves) + f"  (bound {bound:.1e})")
    assert min(moves) > 10.0 * bound


# ------------------------------------------------------------ the C ABI's host side ------------------------------------------------------------
def test_header_symbols_all_exported(lib):
    declared = set(re.findall(r"\b(vtts_stoi_[a-z_0-9]+)\s*\(", O.HEADER.read_text()))
    assert declared == set(_lib.STOI_EXPORTS) == {f"vtts_stoi_{n}" for n in ("create", "destroy", "window", "num_frames", "workspace_bytes", "forward")}
    for name in declared:
        assert hasattr(lib, name), name
        fn = getattr(lib, name)
        assert fn.restype is _lib.STOI_SIGS[name][0] and list(fn.argtypes) == _lib.STOI_SIGS[name][1]
    assert (O.K["VTTS_STOI_MAX_SAMPLES"], O.K["VTTS_STOI_FRAMES_PER_BLOCK"]) == (_lib.STOI_MAX_SAMPLES, _lib.STOI_FRAMES_PER_BLOCK)
    assert (O.K["VTTS_STOI_FRAME"], O.K["VTTS_STOI_HOP"], O.K["VTTS_STOI_BANDS"], O.K["VTTS_STOI_SEG"]) == (O.FRAME, O.HOP, O.BANDS, O.SEG)
    assert (_lib.STOI_FRAME, _lib.STOI_HOP, _lib.STOI_BANDS, _lib.STOI_SEG) == (O.FRAME, O.HOP, O.BANDS, O.SEG)
    assert not set(_lib.STOI_SIGS) & set(_lib.SIGS)


def test_stoi_hip_is_built_without_packed_f32():
    from viettts_amd.csrc import build

    assert "stoi.hip" in build.SOURCES and build.FILE_FLAGS["stoi.hip"] == ["-fno-slp-vectorize"]
    assert any(str(h).endswith("vtts_stoi.h") for h in build.HEADERS)


def test_window_is_the_contracts_bit_for_bit(lib):
    rc, h = _create(lib)
    assert rc == 0
    got = np.empty(256, np.float32)
    assert lib.vtts_stoi_window(h, got.ctypes.data_as(C.POINTER(C.c_float))) == 0
    assert np.array_equal(got.view(np.uint32), O.window().view(np.uint32))
    assert np.abs(got - np.hanning(258)[1:-1]).max() <= 6e-8
    assert lib.vtts_stoi_window(h, None) == -1
    lib.vtts_stoi_destroy(h)


def test_create_and_workspace_bytes_check_their_arguments(lib):
    assert lib.vtts_stoi_create(0, None) == -1 and lib.vtts_last_error()
    lib.vtts_stoi_destroy(None)
    rc, h = _create(lib)
    assert rc == 0
    ws, small, big = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    assert lib.vtts_stoi_workspace_bytes(h, 2, 20000, C.byref(ws)) == 0
    K = O.num_frames(20000)
    assert ws.value == 2 * K * 4 + 2 * K * 8 + 2 * 2 * (K - 30) * 8 + 2 * 2 * 15 * (K - 1) * 4  # the header's layout (every part a multiple of 8 here)
    assert lib.vtts_stoi_workspace_bytes(h, 1, 0, C.byref(small)) == 0 and lib.vtts_stoi_workspace_bytes(h, 64, 163840, C.byref(big)) == 0
    assert 0 < small.value < ws.value < big.value < 16 << 20
    assert lib.vtts_stoi_workspace_bytes(h, 0, 20000, C.byref(ws)) == -1
    assert lib.vtts_stoi_workspace_bytes(h, 1, -1, C.byref(ws)) == -6 and lib.vtts_stoi_workspace_bytes(h, 1, _lib.STOI_MAX_SAMPLES + 1, C.byref(ws)) == -6
    assert lib.vtts_stoi_workspace_bytes(h, 1, _lib.STOI_MAX_SAMPLES, C.byref(ws)) == 0
    assert lib.vtts_stoi_workspace_bytes(h, 1, 20000, None) == -1
    n = C.c_int64(0)
    assert lib.vtts_stoi_num_frames(h, -1, C.byref(n)) == -6 and lib.vtts_stoi_num_frames(h, _lib.STOI_MAX_SAMPLES + 1, C.byref(n)) == -6
    lib.vtts_stoi_destroy(h)


def test_forward_refuses_bad_arguments_before_any_launch(lib):
    """No GPU here: every refusal below has to come from host arithmetic.  The pointers are never dereferenced."""
    rc, h = _create(lib)
    assert rc == 0
    fake = C.c_void_p(0x1000)
    i32 = lambda *v: (C.c_int32 * len(v))(*v)  # noqa: E731
    ws = C.c_size_t(0)
    assert lib.vtts_stoi_workspace_bytes(h, 2, 20000, C.byref(ws)) == 0
    K = O.num_frames(20000)

    def forward(dtype=0, N=2, S=20000, lengths=None, ser=(None, None), M=0, mags=None, T=0, wsp=fake, wsb=None, out=fake, y=fake):
        return lib.vtts_stoi_forward(h, fake, y, dtype, N, S, lengths, out, fake, fake, fake, fake, ser[0], ser[1], M, mags, T, wsp,
                                     ws.value if wsb is None else wsb, None)

    assert forward(dtype=2) == -1
    assert forward(N=0) == -1
    assert forward(out=None) == -1 and forward(wsp=None) == -1 and forward(y=None) == -1
    assert forward(lengths=i32(20000, 20001)) == -6 and b"lengths[1]" in lib.vtts_last_error()
    assert forward(lengths=i32(-1, 20000)) == -6
    assert forward(S=_lib.STOI_MAX_SAMPLES + 1) == -6
    assert forward(ser=(fake, None)) == -1
    assert forward(ser=(fake, fake), M=K - 31) == -6 and b"M_stride" in lib.vtts_last_error()
    assert forward(mags=fake, T=K - 2) == -6 and b"T_stride" in lib.vtts_last_error()
    assert forward(wsb=ws.value - 8) == -5
    assert forward(wsp=C.c_void_p(0x1004)) == -1
    lib.vtts_stoi_destroy(h)


def test_python_module_states_its_interface():
    from viettts_amd import resynth, stoi, vocoder_eval

    a = stoi.build_parser().parse_args(["--clean", "a.wav", "--processed", "b.wav"])
    assert (a.clean, a.processed) == ("a.wav", "b.wav")
    assert stoi.StoiResult._fields == ("stoi", "estoi", "n_frames", "n_kept", "n_segments", "stoi_series", "estoi_series")
    with pytest.raises(ValueError):
        stoi.StoiMeter(device="cpu")
    assert stoi.check_pair(16000, 40000, 16000, 40256) == 40000
    with pytest.raises(ValueError, match="rate"):
        stoi.check_pair(16000, 40000, 22050, 40000)
    with pytest.raises(ValueError, match="one model hop"):
        stoi.check_pair(16000, 40000, 16000, 40257)
    assert vocoder_eval.build_parser().parse_args(["--wav", "a.wav", "--generator", "g", "--discriminator", "d", "--stoi"]).stoi is True
    assert vocoder_eval.build_parser().parse_args(["--wav", "a.wav", "--generator", "g", "--discriminator", "d"]).stoi is False
    assert "NaN" in vocoder_eval.build_parser().format_help() and vocoder_eval.STOI_KEYS == ("stoi", "estoi")
    assert resynth.build_parser().parse_args(["--input", "a.wav", "--output", "b.wav", "--stoi"]).stoi is True


def test_command_line_refuses_a_mismatched_pair_before_the_gpu(tmp_path):
    from viettts_amd import stoi, wavio

    wavio.write_wav_pcm16(str(tmp_path / "a.wav"), np.zeros(8000, np.int16), 16000)
    wavio.write_wav_pcm16(str(tmp_path / "b.wav"), np.zeros(8000, np.int16), 22050)
    wavio.write_wav_pcm16(str(tmp_path / "c.wav"), np.zeros(8300, np.int16), 16000)
    with pytest.raises(ValueError, match="rate"):
        stoi.main(["--clean", str(tmp_path / "a.wav"), "--processed", str(tmp_path / "b.wav")])
    with pytest.raises(ValueError, match="one model hop"):
        stoi.main(["--clean", str(tmp_path / "a.wav"), "--processed", str(tmp_path / "c.wav")])
