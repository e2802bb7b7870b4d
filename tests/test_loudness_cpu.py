"""include/vtts_loudness.h without a GPU: the numpy restatement (tests/_loudness_oracle.py) against the figures of BS.1770 and EBU Tech 3341,
its float32 mode against its float64 mode on the GPU test's inputs, the gate guard of those inputs, and the C ABI's host side."""
import ctypes as C
import re

import numpy as np
import pytest

import _loudness_oracle as O
from viettts_amd import _lib

GPU_CASES = [(name, 16000) for name in O.SIGNALS] + [("low", 22050), ("gated", 48000)]


@pytest.fixture(scope="module")
def lib():
    from viettts_amd.csrc.build import build

    build()
    return _lib.load()


def _create(lib, rate=16000):
    h = C.c_void_p(0)
    rc = lib.vtts_loudness_create(C.byref(_lib.LoudnessCfg(rate)), 0, C.byref(h))
    return rc, h


# ------------------------------------------------------------ the oracle ------------------------------------------------------------
@pytest.mark.parametrize("rate,measured", [(8000, -2.996), (16000, -2.970), (22050, -2.981), (48000, -3.010)])
def test_full_scale_997_hz_sine_meters_minus_3_01_lufs(rate, measured):
    """EBU Tech 3341's meter tolerance is 0.1 LU.  (Below 48 kHz the bilinear transform bends the shelf a little: the measured figures.)"""
    r = O.measure(O.tone(997.0, 1.0, 3 * rate, rate).astype(np.float32), rate)
    print(f"\n{rate} Hz: {r.integrated:.4f} LUFS")
    assert abs(r.integrated - (-3.01)) <= 0.1
    assert abs(r.integrated - measured) <= 2e-3
    assert r.n_blocks == r.n_gated == 27


def test_block_counts_at_the_first_blocks_edges(lib):
    rc, h = _create(lib)
    assert rc == 0
    H = 1600
    n = C.c_int64(-1)
    for S, want in ((4 * H - 1, 0), (4 * H, 1), (5 * H - 1, 1), (5 * H, 2), (0, 0), (3 * H, 0)):
        assert lib.vtts_loudness_num_blocks(h, S, C.byref(n)) == 0 and n.value == want == O.num_blocks(S, 16000), S
        assert O.measure(O.signal("low", S), 16000).n_blocks == want
    assert lib.vtts_loudness_num_blocks(h, -1, C.byref(n)) == -6
    lib.vtts_loudness_destroy(h)


def test_silence_and_short_rows_have_no_loudness_and_gain_one():
    for x in (np.zeros(16000, np.float32), np.zeros(16000, np.int16), O.signal("low", 4 * 1600 - 1)):
        r = O.measure(x)
        assert r.integrated == -np.inf and r.n_gated == 0
        assert O.gain(r) == np.float32(1.0)
    assert O.measure(np.zeros(16000, np.float32)).momentary_max == -np.inf and O.measure(np.zeros(16000, np.float32)).n_blocks == 7


def test_relative_gate_drops_the_quiet_part():
    """28 blocks; the 13 that are silent or mostly at -36 dBFS fall to a gate: 15 gated in, -24.056 LUFS.  Without the relative gate the quiet
    blocks would pull the figure down."""
    x = O.gated_signal(16000)
    r = O.measure(x)
    print(f"\n{r.n_blocks} blocks, {r.n_gated} gated, {r.integrated:.4f} LUFS, {r.gate_room:.2f} LU from a gate")
    assert (r.n_blocks, r.n_gated) == (28, 15)
    assert abs(r.integrated - (-24.056)) <= 1e-3
    l = r.momentary
    above = l > O.ABS_GATE
    assert 15 < above.sum() < 28  # the absolute gate alone keeps more, and not all
    ungated = -0.691 + 10 * np.log10(np.mean(10 ** ((l[above] + 0.691) / 10)))
    assert ungated < r.integrated - 1.0
    assert r.gate_room >= 0.05


def test_each_cap_of_the_gain_rule_binds():
    quiet = O.measure(O.tone(440.0, 0.05, 16000, 16000).astype(np.float32))          # about -29 LUFS, peak 0.05: the target binds
    g = O.gain(quiet)
    assert g == np.float32(10.0 ** ((-23.0 - quiet.integrated) / 20.0)) and 1.0 < g < 10.0 ** 1.5
    faint = O.measure(O.tone(440.0, 1e-3, 16000, 16000).astype(np.float32))         # about -63 LUFS: 40 dB short, max_gain_db binds
    assert O.gain(faint) == np.float32(10.0 ** 1.5)
    click = np.zeros(16000, np.float32)
    click[::1600] = 0.9
    click += O.tone(440.0, 0.01, 16000, 16000).astype(np.float32)
    peaky = O.measure(click)                                                         # quiet but for its clicks: the ceiling binds
    g = O.gain(peaky)
    assert g == np.float32(10.0 ** (-1.0 / 20.0) / np.float64(peaky.sample_peak)) and g < 10.0 ** ((-23.0 - peaky.integrated) / 20.0)
    loud = O.measure(O.tone(440.0, 0.9, 16000, 16000).astype(np.float32))            # above the target: a gain below 1
    assert O.gain(loud) < 1.0


@pytest.mark.parametrize("name,rate", GPU_CASES)
def test_gpu_cases_keep_clear_of_the_gates_and_the_f32_restatement_is_close(name, rate):
    """The gate decisions are discrete: tests/test_gpu_loudness.py may only compare rows whose blocks all lie 0.05 LU or more from either
    gate, and the float32 restatement of the kernel's scheme has to stay inside the 0.1 LU the standard allows."""
    f64, f32 = O.batch_reference(name, rate)
    room = min(r.gate_room for r in f64)
    err = max(O.distance(b, a) for a, b in zip(f64, f32))
    print(f"\n{name} at {rate} Hz: {room:.2f} LU from a gate, float32 restatement within {err:.2e} LU")
    assert room >= 0.05
    assert err <= 0.1 / 4
    for a, b in zip(f64, f32):
        assert (a.n_blocks, a.n_gated) == (b.n_blocks, b.n_gated) and a.sample_peak == b.sample_peak


def test_edge_lengths_meet_the_kernels_edges():
    L = O.edge_lengths(16000)
    assert {6399, 6400, 6401, 8000, O.SEGMENT - 1, O.SEGMENT, O.SEGMENT + 1, 2 * O.SEGMENT + 1} <= set(L)
    assert any(n % O.WAVE_SPAN == 1 for n in L) and any(n % O.WAVE_SPAN == O.WAVE_SPAN - 1 for n in L)
    assert any(n % O.CHUNK == 1 and n % O.WAVE_SPAN != 1 for n in L) and max(L) >= 3 * 16000 and len(L) <= 16


# ------------------------------------------------------------ the C ABI's host side ------------------------------------------------------------
def test_header_symbols_all_exported(lib):
    declared = set(re.findall(r"\b(vtts_loudness_[a-z_0-9]+)\s*\(", O.HEADER.read_text()))
    assert declared == set(_lib.LOUDNESS_EXPORTS) == {f"vtts_loudness_{n}" for n in ("create", "destroy", "coefficients", "num_blocks", "workspace_bytes",
                                                                                     "measure", "normalize")}
    for name in declared:
        assert hasattr(lib, name), name
        fn = getattr(lib, name)
        assert fn.restype is _lib.LOUDNESS_SIGS[name][0] and list(fn.argtypes) == _lib.LOUDNESS_SIGS[name][1]
    assert (O.K["VTTS_LOUDNESS_CHUNK"], O.K["VTTS_LOUDNESS_SEGMENT"]) == (_lib.LOUDNESS_CHUNK, _lib.LOUDNESS_SEGMENT)
    assert (O.K["VTTS_LOUDNESS_MIN_RATE"], O.K["VTTS_LOUDNESS_MAX_RATE"]) == (_lib.LOUDNESS_MIN_RATE, _lib.LOUDNESS_MAX_RATE)
    assert O.SEGMENT == 256 * O.CHUNK and (O.SEGMENT - 1) // (O.K["VTTS_LOUDNESS_MIN_RATE"] // 10) + 2 <= O.K["VTTS_LOUDNESS_SEGMENT_HOPS"]
    assert not set(_lib.LOUDNESS_SIGS) & set(_lib.SIGS)


def test_loudness_hip_is_built_without_packed_f32():
    from viettts_amd.csrc import build

    assert "loudness.hip" in build.SOURCES and "-fno-slp-vectorize" in build.FILE_FLAGS["loudness.hip"]
    assert any(str(h).endswith("vtts_loudness.h") for h in build.HEADERS) and "loudness_design.h" in build.HEADERS


def test_coefficients_are_the_standards_table_at_48_khz(lib):
    got = (C.c_double * 10)()
    for rate in (8000, 16000, 22050, 44100, 48000, 96000):
        rc, h = _create(lib, rate)
        assert rc == 0, rate
        assert lib.vtts_loudness_coefficients(h, got) == 0
        assert np.abs(np.array(got) - O.coefficients(rate)).max() <= 1e-14, rate
        if rate == 48000:
            assert np.abs(np.array(got) - O.BS1770_48K).max() <= 1e-12
        lib.vtts_loudness_destroy(h)


def test_create_refuses_rates_outside_the_contract(lib):
    for rate in (8000, 11020, 22050, 44100, 96000):
        rc, h = _create(lib, rate)
        assert rc == 0, rate
        lib.vtts_loudness_destroy(h)
    for rate in (16001, 22055, 44104, 7990, 96010, 0, -16000):  # not divisible by 10; out of range
        rc, _ = _create(lib, rate)
        assert rc == -1 and lib.vtts_last_error(), rate
    _create(lib, 16005)
    assert b"divisible by 10" in lib.vtts_last_error()
    _create(lib, 4000)
    assert b"8000 .. 96000" in lib.vtts_last_error()
    assert lib.vtts_loudness_create(None, 0, C.byref(C.c_void_p(0))) == -1
    lib.vtts_loudness_destroy(None)


def test_measure_and_normalize_refuse_bad_arguments_before_any_launch(lib):
    """No GPU here: every refusal below has to come from host arithmetic.  The pointers are never dereferenced."""
    rc, h = _create(lib)
    assert rc == 0
    fake = C.c_void_p(0x1000)
    i32 = lambda *v: (C.c_int32 * len(v))(*v)  # noqa: E731
    ws = C.c_size_t(0)
    assert lib.vtts_loudness_workspace_bytes(h, 2, 48000, C.byref(ws)) == 0 and ws.value > 0
    small, big = C.c_size_t(0), C.c_size_t(0)
    assert lib.vtts_loudness_workspace_bytes(h, 1, 0, C.byref(small)) == 0 and lib.vtts_loudness_workspace_bytes(h, 64, 262144, C.byref(big)) == 0
    assert 0 < small.value < ws.value < big.value < 1 << 20  # a few bytes per segment and per hop
    assert lib.vtts_loudness_workspace_bytes(h, 0, 48000, C.byref(ws)) == -1 and lib.vtts_loudness_workspace_bytes(h, 1, -1, C.byref(ws)) == -6
    assert lib.vtts_loudness_workspace_bytes(h, 2, 48000, C.byref(ws)) == 0

    def measure(dtype=0, N=2, S=48000, lengths=None, mom=None, J=0, wsp=fake, wsb=None, out=fake):
        return lib.vtts_loudness_measure(h, fake, dtype, N, S, lengths, out, fake, fake, fake, fake, mom, J, wsp, ws.value if wsb is None else wsb, None)

    assert measure(dtype=2) == -1
    assert measure(N=0) == -1
    assert measure(out=None) == -1 and measure(wsp=None) == -1
    assert measure(lengths=i32(48000, 48001)) == -6 and b"lengths[1]" in lib.vtts_last_error()
    assert measure(lengths=i32(-1, 48000)) == -6
    assert measure(mom=fake, J=O.num_blocks(48000, 16000) - 1) == -6 and b"J_stride" in lib.vtts_last_error()
    assert measure(wsb=ws.value - 256) == -5
    assert measure(wsp=C.c_void_p(0x1004)) == -1

    def normalize(dtype=0, N=2, S=48000, lengths=None, target=-23.0, odt=1, O_stride=48000, gains=fake):
        return lib.vtts_loudness_normalize(h, fake, dtype, N, S, lengths, fake, fake, target, -1.0, 30.0, fake, odt, O_stride, gains, None)

    assert normalize(dtype=3) == -1 and normalize(odt=2) == -1 and normalize(N=0) == -1 and normalize(gains=None) == -1
    assert normalize(target=float("nan")) == -1 and normalize(target=float("-inf")) == -1
    assert normalize(O_stride=47999) == -6 and b"O_stride" in lib.vtts_last_error()
    assert normalize(lengths=i32(5, 48001)) == -6
    lib.vtts_loudness_destroy(h)


def test_python_module_states_its_interface():
    from viettts_amd import loudness

    a = loudness.build_parser().parse_args(["--wav", "x.wav", "--target", "-16", "--output", "y.wav"])
    assert (a.wav, a.target, a.output, a.ceiling_db, a.max_gain_db) == ("x.wav", -16.0, "y.wav", -1.0, 30.0)
    assert loudness.LoudnessResult._fields == ("integrated", "momentary_max", "sample_peak", "n_blocks", "n_gated", "momentary")
    with pytest.raises(ValueError):
        loudness.LoudnessMeter(16000, device="cpu")
