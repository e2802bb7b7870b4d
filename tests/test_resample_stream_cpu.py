"""include/vtts_rsstream.h without a GPU: the emit rule, the streamed numpy state machine (tests/_resample_stream_oracle.py) against the same
chain on the whole row bit for bit, four planted faults that the same cases must see, the C ABI's host side, and the Python and CLI surface."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import _audio_oracle as A
import _resample_stream_oracle as SO
from viettts_amd import _lib

REPO = Path(__file__).resolve().parents[1]
HEADER = REPO / "include" / "vtts_rsstream.h"
NAMES = ("create", "destroy", "ratio", "state_bytes", "packed_bytes", "bind_packed", "reset", "cursor", "emit", "push")


@pytest.fixture(scope="module")
def lib():
    from viettts_amd.csrc.build import build

    build()
    return _lib.load()


def _create(lib, in_rate=16000, out_rate=48000, rows=4, max_chunk=8192):
    h = C.c_void_p(0)
    rc = lib.vtts_rsstream_create(C.byref(_lib.AudioCfg(in_rate, out_rate)), 0, rows, max_chunk, C.byref(h))
    return rc, h


# ------------------------------------------------------------ the emit rule ------------------------------------------------------------
def test_emit_rule_by_hand():
    from viettts_amd.audio import resample_emit

    up, down, odd = (3, 1, 72), (1, 2, 48), (441, 160, 10584)
    table = [  # (received, emitted, count, last), (L, M, half) -> emitted afterwards
        ((0, 0, 24, False), up, 0),        # 3/1: the delay is 24 samples; q(0) = 24 has not arrived
        ((0, 0, 25, False), up, 3),        # q(0) = q(1) = q(2) = 24
        ((0, 0, 26, False), up, 6),
        ((25, 3, 0, False), up, 3),        # a zero count moves nothing
        ((1000, 2928, 1000, False), up, 5928),
        ((0, 0, 0, True), up, 0),          # an empty row
        ((0, 0, 1, True), up, 3),          # last: every output of the row, however short
        ((1000, 2928, 0, True), up, 3000),  # a flush
        ((0, 0, 48, False), down, 0),      # 1/2: the delay is 48 samples; q(0) = 48
        ((0, 0, 49, False), down, 1),
        ((0, 0, 50, False), down, 1),      # q(1) = 50
        ((0, 0, 51, False), down, 2),
        ((0, 0, 5, True), down, 3),
        ((0, 0, 24, False), odd, 0),       # 441/160: ceil(10584 / 441) = 24
        ((0, 0, 25, False), odd, 3),       # m M + half < 25 * 441 = 11025: m <= 2
        ((7, 7, 5, False), (1, 1, 24), 12),  # equal rates: everything, at once
    ]
    for args, (L, M, half), want in table:
        assert resample_emit(*args, L, M, half) == want == SO.emit(*args, L, M, half), (args, L, M)
    for (L, M, half), d in ((up, 24), (down, 48), (odd, 24), ((160, 441, 10584), 67)):
        assert SO.delay(L, M, half) == d == -(-half // L)
    # whatever the chunking, a row of S samples emits out_samples(S), and the rule is what it says: the outputs whose newest input arrived
    rng = np.random.default_rng(3)
    for fi, fo in SO.RATES:
        L, M, half = A.ratio(fi, fo)
        for S in (0, 1, 23, 24, 25, 700):
            for _ in range(8):
                R = F = 0
                while True:
                    n = int(min(rng.integers(0, 200), S - R))
                    last = R + n == S and bool(rng.integers(0, 2) or n == 0 and S == R)
                    Fn = resample_emit(R, F, n, last, L, M, half)
                    assert Fn >= F
                    if not last and L != M:
                        assert Fn == 0 or SO.newest(Fn - 1, L, M, half) <= R + n - 1
                        assert SO.newest(Fn, L, M, half) >= R + n
                    R, F = R + n, Fn
                    if last:
                        break
                assert F == (S if L == M else A.out_samples(S, L, M))


# ------------------------------------------------------------ the streamed oracle ------------------------------------------------------------
def _row(seed, S):
    return A.speechlike(np.random.default_rng(seed), S) if S else np.zeros(0, dtype=np.float32)


def _lengths(fi, fo):
    L, M, half = A.ratio(fi, fo)
    d = max(SO.delay(L, M, half), 2)
    return [1, d - 1, d, d + 1, 3001]


RANDOM = [int(v) for v in np.random.default_rng(9).integers(1, 500, 40) * np.random.default_rng(10).integers(0, 2, 40)] + [333]
_WHOLE = {}


def _whole(fi, fo, seed, S):
    key = (fi, fo, seed, S)
    if key not in _WHOLE:
        _WHOLE[key] = SO.whole(_row(seed, S), fi, fo)
    return _WHOLE[key]


def _agrees(fi, fo, seed, S, sizes, fault=None, flush=False, x=None):
    ref = SO.whole(x, fi, fo) if x is not None else _whole(fi, fo, seed, S)
    ys, st = SO.run(_row(seed, S) if x is None else x, fi, fo, sizes, fault, flush)
    return SO.same(np.concatenate(ys), ref)


@pytest.mark.parametrize("rates", SO.RATES, ids=lambda r: f"{r[0]}-{r[1]}")
def test_streamed_oracle_equals_the_whole_row(rates):
    """Every rate; rows of 1, delay - 1, delay, delay + 1 and 3001 samples all at once, in random sizes with zero-count pushes between them, and
    with an empty last flush; single-sample pushes on a 300-sample row.  The state machine raises if an output reads outside the history the
    contract allows, and asserts the history never passes kp4 - 1 samples."""
    fi, fo = rates
    assert 0 in RANDOM[:-1]
    for i, S in enumerate(_lengths(fi, fo)):
        assert _agrees(fi, fo, 100 + i, S, [S]), S
        assert _agrees(fi, fo, 100 + i, S, [S], flush=True), S
        assert _agrees(fi, fo, 100 + i, S, RANDOM), S
        assert _agrees(fi, fo, 100 + i, S, RANDOM, flush=True), S
    assert _agrees(fi, fo, 7, 300, [1])
    assert _agrees(fi, fo, 7, 300, [1, 0], flush=True)
    L, M, half, kp4, _ = SO.design(fi, fo)
    _, st = SO.run(_row(7, 300), fi, fo, [1])
    assert st.most_history == (0 if L == M else kp4 - 1)  # the bound is met, so a buffer one float shorter would not do


def _fault_cases(fi, fo):
    """(name, x, sizes): a speech row in pushes of 1000, and the same pushes with one NaN where only the padding taps' share of the history
    holds it (x[q(F') - (kp4 - 1)] of the second push's boundary), which a history cut one sample short loses without any finite trace; and with
    one NaN at x[R'] of that boundary, the sample an output emitted one too early would need: at L / 1 its tap is the prototype's first,
    sinc(-24) = 0 up to rounding, so no finite sample there shows."""
    L, M, half, kp4, _ = SO.design(fi, fo)
    x = _row(21, 3001)
    F2 = SO.emit(1000, SO.emit(0, 0, 1000, False, L, M, half), 1000, False, L, M, half)
    y = x.copy()
    y[SO.newest(F2, L, M, half) - (kp4 - 1)] = np.nan
    z = x.copy()
    z[2000] = np.nan
    return [("speech", x, [1000]), ("nan at the history's first sample", y, [1000]), ("nan at the first sample not yet received", z, [1000])]


@pytest.mark.parametrize("fault", SO.FAULTS)
def test_each_planted_fault_breaks_a_case(fault):
    """The state machine with one mistake planted (tests/_resample_stream_oracle.py lists them) must fail a case at every rate that filters."""
    for fi, fo in SO.RATES[:-1]:
        cases = _fault_cases(fi, fo)
        for name, x, sizes in cases:
            assert _agrees(fi, fo, 0, 0, sizes, x=x), (name, fi, fo)  # the cases pass unbroken
        broken = [name for name, x, sizes in cases if not _agrees(fi, fo, 0, 0, sizes, fault=fault, x=x)]
        print(f"\n{fault} {fi}->{fo}: seen by {broken}")
        assert broken, (fault, fi, fo)


def test_the_unbroken_machine_raises_outside_its_history():
    st = SO.Stream(16000, 48000)
    st.push(_row(1, 500))
    st.base += 1  # pretend the history lost its first sample
    st.hist = st.hist[1:]
    with pytest.raises(SO.OutsideHistory):
        st.push(_row(2, 500))


def test_pcm16_in_is_exact_and_out_is_the_rule():
    x = (np.random.default_rng(5).integers(-32768, 32768, 2000)).astype(np.int16)
    ys, _ = SO.run(x, 16000, 24000, [333])
    assert SO.same(np.concatenate(ys), SO.whole(x, 16000, 24000))
    assert np.array_equal(SO.to_pcm16(np.array([np.nan, 2.0, -2.0, 0.25 / 32767, 1.75 / 32767, -1.0], dtype=np.float32)), np.array([0, 32767, -32767, 0, 2, -32767], dtype=np.int16))


# ------------------------------------------------------------ the C ABI's host side ------------------------------------------------------------
def test_header_symbols_all_exported(lib):
    text = HEADER.read_text()
    declared = set(re.findall(r"\b(vtts_rsstream_[a-z_0-9]+)\s*\(", text))
    assert declared == set(_lib.RSSTREAM_EXPORTS) == {f"vtts_rsstream_{n}" for n in NAMES}
    for name in declared:
        fn = getattr(lib, name)
        assert fn.restype is _lib.RSSTREAM_SIGS[name][0] and list(fn.argtypes) == _lib.RSSTREAM_SIGS[name][1]
    assert not set(_lib.RSSTREAM_SIGS) & (set(_lib.SIGS) | set(_lib.LIMSTREAM_SIGS))
    assert not any(n.startswith("vtts_audio_") for n in _lib.RSSTREAM_SIGS)
    assert "#define VTTS_RSSTREAM_MAX_CHUNK (1 << 20)" in text and _lib.RSSTREAM_MAX_CHUNK == 1 << 20
    assert f"#define VTTS_RSSTREAM_ROWS_PER_LAUNCH {_lib.RSSTREAM_ROWS_PER_LAUNCH}\n" in text
    assert not re.search(r"vtts_rsstream_", (REPO / "include" / "vtts_audio.h").read_text())
    assert "vtts_rsstream.h" in (REPO / "include" / "vtts_limstream.h").read_text()


def test_resample_stream_hip_is_built_like_the_other_device_files():
    from viettts_amd.csrc import build

    assert "resample_stream.hip" in build.SOURCES and "-fno-slp-vectorize" in build.FILE_FLAGS["resample_stream.hip"]
    assert {"audio_common.h", "rsstream_host.h"} <= set(build.HEADERS) and any(str(h).endswith("vtts_rsstream.h") for h in build.HEADERS)
    src = (build.CSRC / "resample_stream.hip").read_text()
    assert "asm" not in src and '#include "rsstream_host.h"' in src and '#include "audio_common.h"' in src
    assert '#include "audio_common.h"' in (build.CSRC / "audio.hip").read_text()  # the chain is stated once
    assert "fmaf(" not in src and "fmaf(" not in (build.CSRC / "audio.hip").read_text() and "fmaf(" in (build.CSRC / "audio_common.h").read_text()
    host = (build.CSRC / "rsstream_host.h").read_text()
    assert "#include <hip" not in host and "hipStream" not in host and "hipError" not in host  # plain C++: tools/check_rsstream_host.cpp builds it alone
    assert (REPO / "tools" / "check_rsstream_host.cpp").exists()


def test_create_refuses_what_the_header_rules_out(lib):
    L, M, half = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    for fi, fo in SO.RATES:
        rc, h = _create(lib, fi, fo)
        assert rc == 0 and lib.vtts_rsstream_ratio(h, C.byref(L), C.byref(M), C.byref(half)) == 0
        assert (L.value, M.value, half.value) == A.ratio(fi, fo)
        assert lib.vtts_rsstream_ratio(h, None, None, None) == 0
        lib.vtts_rsstream_destroy(h)
    bad = [dict(in_rate=0), dict(out_rate=-1), dict(in_rate=16000, out_rate=16001), dict(in_rate=48000, out_rate=1000), dict(rows=0), dict(rows=-1),
           dict(rows=(1 << 24) + 1), dict(max_chunk=0), dict(max_chunk=(1 << 20) + 1)]
    for kw in bad:
        rc, _ = _create(lib, **kw)
        assert rc == -1 and lib.vtts_last_error(), kw
    _create(lib, max_chunk=0)
    assert b"max_chunk" in lib.vtts_last_error()
    assert _create(lib, max_chunk=1 << 20)[0] == 0
    assert lib.vtts_rsstream_create(None, 0, 1, 1, C.byref(C.c_void_p(0))) == -1
    lib.vtts_rsstream_destroy(None)


def test_emit_and_state_bytes_and_reset(lib):
    from viettts_amd.audio import resample_emit

    rng = np.random.default_rng(4)
    for fi, fo in SO.RATES:
        L, M, half, kp4, _ = SO.design(fi, fo)
        rc, h = _create(lib, fi, fo, rows=3, max_chunk=1 << 20)
        assert rc == 0
        n = C.c_size_t(0)
        assert lib.vtts_rsstream_state_bytes(h, C.byref(n)) == 0
        assert n.value == (0 if L == M else 3 * 2 * ((kp4 - 1 + 3) // 4 * 4) * 4)  # per row two buffers of kp4 - 1 floats rounded up to 4
        assert lib.vtts_rsstream_packed_bytes(h, C.byref(n)) == 0 and n.value == L * kp4 * 4
        ha = C.c_void_p(0)
        assert lib.vtts_audio_create(C.byref(_lib.AudioCfg(fi, fo)), 0, C.byref(ha)) == 0
        na = C.c_size_t(0)
        assert lib.vtts_audio_packed_bytes(ha, C.byref(na)) == 0 and na.value == n.value  # the Resampler's blob is the session's
        lib.vtts_audio_destroy(ha)
        out = C.c_int64(0)
        for _ in range(300):
            R = int(rng.integers(0, 50000))
            F = resample_emit(0, 0, R, False, L, M, half)
            cnt, last = int(rng.integers(0, 20000)), bool(rng.integers(0, 2))
            assert lib.vtts_rsstream_emit(h, R, F, cnt, int(last), C.byref(out)) == 0
            assert out.value == resample_emit(R, F, cnt, last, L, M, half) == SO.emit(R, F, cnt, last, L, M, half)
        for R in range(0, 3 * SO.delay(L, M, half) + 8):
            assert lib.vtts_rsstream_emit(h, R, 0, 0, 0, C.byref(out)) == 0 and out.value == resample_emit(R, 0, 0, False, L, M, half)
        assert lib.vtts_rsstream_emit(h, (1 << 31) - 2, 0, 1, 1, C.byref(out)) == 0 and out.value == SO.emit((1 << 31) - 2, 0, 1, True, L, M, half)
        assert lib.vtts_rsstream_emit(h, -1, 0, 0, 0, C.byref(out)) == -1 and lib.vtts_rsstream_emit(h, 5, 0, -1, 0, C.byref(out)) == -1
        assert lib.vtts_rsstream_emit(h, 5, -1, 0, 0, C.byref(out)) == -1 and lib.vtts_rsstream_emit(h, (1 << 31) - 1, 0, 1, 0, C.byref(out)) == -1
        assert lib.vtts_rsstream_reset(h, 2) == 0 and lib.vtts_rsstream_reset(h, 3) == -1 and lib.vtts_rsstream_reset(h, -1) == -1
        lib.vtts_rsstream_destroy(h)


def test_push_refuses_bad_arguments_before_any_launch(lib):
    """No GPU here: every refusal below is host arithmetic, and the pointers are never dereferenced."""
    rc, h = _create(lib, rows=3, max_chunk=100)
    assert rc == 0
    fake, blob = C.c_void_p(0x1000), C.c_void_p(1 << 20)
    i32 = lambda *v: (C.c_int32 * len(v))(*v)  # noqa: E731
    got = i32(7, 7, 7, 7)

    def push(rows=(0, 1), counts=(10, 10), lasts=(0, 0), n=None, stride=0, dtype=0, odt=0, state=fake, chunk=fake, out=fake, lasts_null=False):
        return lib.vtts_rsstream_push(h, state, chunk, dtype, len(rows) if n is None else n, i32(*rows), stride, i32(*counts), None if lasts_null else i32(*lasts),
                                      out, odt, got, None)

    def cursors():
        r, f, c = C.c_int64(-1), C.c_int64(-1), C.c_int(-1)
        out = []
        for row in range(3):
            assert lib.vtts_rsstream_cursor(h, row, C.byref(r), C.byref(f), C.byref(c)) == 0
            out.append((r.value, f.value, c.value))
        return out

    assert push() == -2 and b"bind_packed" in lib.vtts_last_error()  # no tap table yet
    assert lib.vtts_rsstream_bind_packed(h, blob, 16) == -5 and lib.vtts_rsstream_bind_packed(h, C.c_void_p(1 << 20 | 64), 1 << 20) == -1
    assert lib.vtts_rsstream_bind_packed(h, None, 1 << 20) == -1 and lib.vtts_rsstream_bind_packed(h, blob, 1 << 20) == 0
    assert push(dtype=2) == -1 and push(odt=2) == -1 and push(n=0) == -1 and push(n=4, rows=(0, 1, 2, 0), counts=(1,) * 4, lasts=(0,) * 4) == -1
    assert push(state=None) == -1 and push(chunk=None) == -1 and push(out=None) == -1 and push(state=C.c_void_p(0x1004)) == -1
    assert push(stride=-1) == -1 and push(stride=9) == -1 and b"c_stride" in lib.vtts_last_error()
    assert push(rows=(0, 3)) == -1 and push(rows=(-1, 0)) == -1 and b"outside" in lib.vtts_last_error()
    assert push(rows=(1, 1)) == -1 and b"twice" in lib.vtts_last_error()
    assert push(counts=(10, 101)) == -1 and b"max_chunk" in lib.vtts_last_error() and push(counts=(-1, 10)) == -1
    assert push(counts=(10, 101), lasts_null=True) == -1
    assert list(got) == [7, 7, 7, 7]  # and nothing was reported as emitted
    assert cursors() == [(0, 0, 0)] * 3  # no bookkeeping moved
    assert lib.vtts_rsstream_cursor(h, 3, None, None, None) == -1 and lib.vtts_rsstream_cursor(h, 0, None, None, None) == 0
    lib.vtts_rsstream_destroy(h)
    # equal rates: no table and no state are needed, and the same refusals hold
    rc, h = _create(lib, 16000, 16000, rows=2, max_chunk=100)
    n = C.c_size_t(1)
    assert rc == 0 and lib.vtts_rsstream_state_bytes(h, C.byref(n)) == 0 and n.value == 0
    assert lib.vtts_rsstream_push(h, None, fake, 0, 1, i32(2), 0, i32(1), None, fake, 0, got, None) == -1 and b"outside" in lib.vtts_last_error()
    lib.vtts_rsstream_destroy(h)


# ------------------------------------------------------------ the surface ------------------------------------------------------------
def test_python_surface_and_defaults():
    from viettts_amd import audio, serving, streaming

    sig = inspect.signature(audio.Resampler.open_stream).parameters
    assert list(sig)[1:] == ["rows", "max_chunk", "out_dtype"] and sig["out_dtype"].default == "f32"
    sig = inspect.signature(audio.ResamplerStream.push).parameters
    assert [sig[k].default for k in ("counts", "last", "rows")] == [None, False, None]
    assert list(inspect.signature(audio.ResamplerStream.reset).parameters) == ["self", "row"]
    assert issubclass(audio.ResamplerStream, audio.NativeHandle) and hasattr(audio.ResamplerStream, "__enter__") and hasattr(audio.ResamplerStream, "__exit__")
    assert list(inspect.signature(audio.resample_emit).parameters) == ["received", "emitted", "count", "last", "L", "M", "half"]
    for fn in (streaming.stream_mel, streaming.synthesize_stream, serving.SpeechPool.__init__):
        assert inspect.signature(fn).parameters["out_rate"].default is None, fn
    for name in ("README.md", "DESIGN.md"):
        assert "vtts_rsstream" in (REPO / name).read_text() and "ResamplerStream" in (REPO / name).read_text(), name


def test_synthesizer_flags(capsys):
    """Every argument error comes before any device is touched: this machine has none."""
    from viettts_amd import synthesizer

    a = synthesizer.build_parser().parse_args([])
    assert a.output_rate is None
    a = synthesizer.build_parser().parse_args(["--stream", "--output-rate", "48000"])
    assert (a.stream, a.output_rate) == (True, 48000)
    with pytest.raises(SystemExit):
        synthesizer.main(["--text", "xin chào", "--stream", "--resample"])
    err = capsys.readouterr().err
    assert "--stream with --resample" in err and "--output-rate" in err
    with pytest.raises(SystemExit):
        synthesizer.main(["--text", "xin chào", "--output-rate", "48000"])
    assert "--sample-rate R --resample" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        synthesizer.main(["--mel-file", "m.npy", "--stream", "--output-rate", "48000", "--sample-rate", "22050"])
    assert "--output-rate with --sample-rate 22050" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        synthesizer.main(["--mel-file", "m.npy", "--stream", "--output-rate", "0"])
    assert "--output-rate" in capsys.readouterr().err
