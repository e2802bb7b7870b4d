"""include/vtts_limstream.h without a GPU: the emit rule, the streamed numpy state machine (tests/_limiter_stream_oracle.py) against the
whole-row restatement (tests/_limiter_oracle.py) with array_equal in float64 and float32, five planted faults that the same cases must see,
the C ABI's host side, and the Python surface."""
import ctypes as C
import inspect
import re
import sys

import numpy as np
import pytest

import _limiter_oracle as O
import _limiter_stream_oracle as SO
from viettts_amd import _lib

FS, W = 16000, 80
D = 2 * W + 24  # the delay
HEADER = O.REPO / "include" / "vtts_limstream.h"


@pytest.fixture(scope="module")
def lib():
    from viettts_amd.csrc.build import build

    build()
    return _lib.load()


def _create(lib, rate=16000, ms=5.0, rows=4, max_chunk=8192, ceiling=-1.0):
    h = C.c_void_p(0)
    rc = lib.vtts_limstream_create(C.byref(_lib.LimiterCfg(rate, ms)), 0, rows, max_chunk, ceiling, C.byref(h))
    return rc, h


# ------------------------------------------------------------ the emit rule ------------------------------------------------------------
def test_emit_rule_by_hand():
    from viettts_amd.limiter import stream_emit

    table = [  # (received, emitted, count, last) -> emitted afterwards, W = 80: the delay is 184
        ((0, 0, D, False), 0),            # R' = 2 W + 24: no sample has its look-ahead yet
        ((0, 0, D + 15, False), 0),       # runs of 16 leave whole, so nothing leaves before R' = 2 W + 40
        ((0, 0, D + 16, False), 16),
        ((0, 0, D + 31, False), 16),
        ((0, 0, D + 32, False), 32),
        ((D + 16, 16, 0, False), 16),     # a zero count moves nothing
        ((D + 16, 16, 1, False), 16),
        ((1000, 816, 16, False), 832),
        ((0, 0, 1, False), 0),
        ((0, 0, 0, True), 0),             # an empty row
        ((0, 0, 5, True), 5),             # last: everything, however short
        ((1000, 816, 0, True), 1000),     # a flush
        ((1000, 816, 7, True), 1007),
        ((5000, 4816, 8192, False), (13192 - D) // 16 * 16),
    ]
    for args, want in table:
        assert stream_emit(*args, W) == want == SO.emit(*args, W), args
    assert stream_emit(0, 0, 2 * 1 + 24 + 16, False, 1) == 16 and stream_emit(0, 0, 2 * 960 + 24 + 15, False, 960) == 0
    # whatever the chunking, a row of S samples emits S
    rng = np.random.default_rng(3)
    for S in (0, 1, D, D + 1, 5000):
        for _ in range(20):
            R = F = 0
            while True:
                n = int(min(rng.integers(0, 400), S - R))
                last = R + n == S and bool(rng.integers(0, 2) or n == 0 and S == R)
                Fn = stream_emit(R, F, n, last, W)
                assert F <= Fn <= R + n and (last or Fn % 16 == 0)
                R, F = R + n, Fn
                if last:
                    break
            assert F == S


# ------------------------------------------------------------ the streamed oracle ------------------------------------------------------------
def _clicks(S, at, seed):
    x = (0.1 * O.speech(seed, S)).astype(np.float32)
    for j, k in enumerate(at):
        x[k] = (0.95 - 0.05 * (j % 8)) * (-1.0) ** j
    return x


def _cases():
    """(name, x, g, chunk sizes).  A push boundary of the click rows: after 1000 + 1000 samples R' = 2000 and F' = 1808."""
    Rb, Fb = 2000, (2000 - D) // 16 * 16
    assert SO.emit(1000, SO.emit(0, 0, 1000, False, W), 1000, False, W) == Fb
    lens = sorted({0, 1, D, D + 1, *O.edge_lengths()})  # (the 3 s row included: 49 pushes, 3000 runs of carried history)
    out = []
    for i, S in enumerate(lens):
        out.append((f"len{S}", O.speech(100 + i, S), 4.0, [1000]))
    sp = O.speech(7, 9000)
    for size in (16, 17, D, D + 1, 4095, 4096, 4097, 8192, 9000):
        out.append((f"speech/{size}", sp, 4.0, [size]))
    out.append(("speech/random", sp, 4.0, [int(v) for v in np.random.default_rng(9).integers(0, 700, 64) * np.random.default_rng(10).integers(0, 2, 64)] + [333]))
    out.append(("speech/1", O.speech(8, 400), 4.0, [1]))
    out.append(("clicks", _clicks(5000, (0, 4999, Fb - 1, Fb, Rb - 25, Rb - 24), 12), 2.0, [1000]))
    out.append(("clicks/window", _clicks(5000, (Fb - 2 * W + 3, Fb - W - 2, 2 * Fb - 2000 - 3 * W // 2), 13), 2.0, [1000]))
    out.append(("quiet", (0.2 * O.speech(14, 5000)).astype(np.float32), 1.0, [1000]))
    # one click whose only trace in what the next push reads is the sample a history cut short would lose: x[F - 2 W - 23], the first sample
    # whose tap under p[F - 2 W] can show (1.1e-5; x[n - 24]'s is 1.4e-20 and those before it are zero padding).  The gain lifts that trace
    # over the ceiling.
    x = (1e-6 * O.speech(16, 4000)).astype(np.float32)
    x[Fb - 2 * W - 23] = 1.0
    trace = O.envelope(x, FS)[Fb - 2 * W]
    assert 5e-6 < trace < 1e-3
    out.append(("history", x, float(np.float32(2.0 * float(O.ceiling()) / trace)), [1000]))
    return out


CASES = _cases()
_REFS = {}


def _ref(case, dtype):
    key = (case[0], np.dtype(dtype).name)
    if key not in _REFS:
        _REFS[key] = O.limit(case[1], FS, case[2], dtype=dtype)
    return _REFS[key]


def _agrees(case, dtype, fault=None):
    """Does the state machine, fed this case's chunks, give the whole row's y, its running true peak after every push and its results?  Float32
    also checks that the run sums start at multiples of 16 from the row's first sample: the order of an fp64 sum does not show in an fp32 bit
    often enough to catch it."""
    name, x, g, sizes = case
    ref = _ref(case, dtype)
    st = SO.Stream(FS, g, dtype=dtype, fault=fault)
    ys, at, k = [], 0, 0
    while True:
        n = min(sizes[k % len(sizes)], len(x) - at)
        k += 1
        last = at + n >= len(x)
        ys.append(st.push(x[at:at + n], last))
        at += n
        final = ref.p[:st.F]
        if st.true_peak != (float(final.max()) if final.size else 0.0):
            return False
        if last:
            break
    y = np.concatenate(ys)
    ok = y.shape == ref.y.shape and np.array_equal(y, ref.y) and st.true_peak == ref.true_peak and st.min_gain == ref.min_gain
    return ok and all(a % SO.RUN == 0 for a in st.anchors)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_streamed_oracle_equals_the_whole_row(dtype):
    """Chunks of 1 (a 400-sample row), 16, 17, 2 W + 24, 2 W + 25, 4095 .. 4097, 8192, random sizes with zero-count pushes between them, one
    single last push; rows of 0, 1, 2 W + 24, 2 W + 25 samples and the kernels' edge lengths; clicks at F' - 1, F', R' - 25, R' - 24 of a push
    boundary and at samples 0 and S - 1."""
    names = [c[0] for c in CASES]
    assert {"len0", "len1", f"len{D}", f"len{D + 1}", *[f"len{S}" for S in O.edge_lengths()], "speech/16", "speech/17", f"speech/{D}", "speech/8192", "speech/9000", "speech/1",
            "speech/random", "clicks"} <= set(names)
    assert 0 in CASES[names.index("speech/random")][3][:-1]
    for case in CASES:
        assert _agrees(case, dtype), case[0]


@pytest.mark.parametrize("fault", SO.FAULTS)
def test_each_planted_fault_breaks_a_case(fault):
    """The state machine with one mistake planted (tests/_limiter_stream_oracle.py lists them) must fail at least one of the cases above: the
    case list can see these faults.  Four of them change a sample or the running true peak.  ``anchor_push`` does not: the order of an fp64
    sum does not reach an fp32 bit often enough, so it is seen only by the state machine's own record of where its run sums start.  That says
    something about this restatement, nothing about a kernel: on the GPU what keeps the runs anchored is that tiles start at F and the emit
    rule keeps F a multiple of 16, which tests/test_gpu_limiter_stream.py checks on every push's emitted count."""
    order = sorted(CASES, key=lambda c: c[0] not in ("history", "clicks/window", "clicks", "quiet"))  # (the cases written for the faults first)
    broken = next((c[0] for c in order if not c[0].startswith("speech/1") and not _agrees(c, np.float32, fault)), None)
    print(f"\n{fault}: first seen by {broken!r}")
    assert broken is not None, fault


def test_a_flush_ends_a_row_that_ended_on_a_chunk_edge():
    x = O.speech(15, 3000)
    ref = O.limit(x, FS, 4.0, dtype=np.float32)
    st = SO.Stream(FS, 4.0, dtype=np.float32)
    ys = [st.push(x[:1500]), st.push(x[1500:]), st.push(x[:0], last=True)]
    assert [len(y) for y in ys] == [1312, 1504, 184] and np.array_equal(np.concatenate(ys), ref.y) and st.min_gain == ref.min_gain


# ------------------------------------------------------------ the C ABI's host side ------------------------------------------------------------
def test_header_symbols_all_exported(lib):
    text = HEADER.read_text()
    declared = set(re.findall(r"\b(vtts_limstream_[a-z_0-9]+)\s*\(", text))
    assert declared == set(_lib.LIMSTREAM_EXPORTS) == {f"vtts_limstream_{n}" for n in ("create", "destroy", "lookahead", "state_bytes", "reset", "emit", "push")}
    for name in declared:
        fn = getattr(lib, name)
        assert fn.restype is _lib.LIMSTREAM_SIGS[name][0] and list(fn.argtypes) == _lib.LIMSTREAM_SIGS[name][1]
    assert not set(_lib.LIMSTREAM_SIGS) & (set(_lib.SIGS) | set(_lib.LIMITER_SIGS))
    assert "#define VTTS_LIMSTREAM_MAX_CHUNK (1 << 20)" in text and _lib.LIMSTREAM_MAX_CHUNK == 1 << 20
    assert f"#define VTTS_LIMSTREAM_ROWS_PER_LAUNCH {_lib.LIMSTREAM_ROWS_PER_LAUNCH}\n" in text
    assert not re.search(r"vtts_limstream_", (O.REPO / "include" / "vtts_limiter.h").read_text())


def test_limiter_stream_hip_is_built_like_the_other_device_files():
    from viettts_amd.csrc import build

    assert "limiter_stream.hip" in build.SOURCES and "-fno-slp-vectorize" in build.FILE_FLAGS["limiter_stream.hip"]
    assert {"limiter_common.h", "limstream_host.h", "stream_rows_host.h", "sample_convert.h"} <= set(build.HEADERS)
    assert any(str(h).endswith("vtts_limstream.h") for h in build.HEADERS)
    src = (build.CSRC / "limiter_stream.hip").read_text()
    assert "asm" not in src and '#include "limstream_host.h"' in src and '#include "limiter_common.h"' in src and '#include "stream_rows_host.h"' in src
    # plain C++: tools/check_limstream_host.cpp and tools/check_stream_rows_host.cpp build them alone
    for name in ("limstream_host.h", "stream_rows_host.h"):
        host = (build.CSRC / name).read_text()
        assert "#include <hip" not in host and "hipStream" not in host and "hipError" not in host, name
    assert "__device__" not in host and "__HIPCC__" not in host  # (the cursors live on the host alone)
    assert (O.REPO / "tools" / "check_stream_rows_host.cpp").exists()
    assert '#include "stream_rows_host.h"' in (build.CSRC / "resample_stream.hip").read_text()  # one copy of the cursors' rules for both streams


def test_the_limiters_arithmetic_and_the_sample_conversions_are_stated_once():
    from viettts_amd.csrc import build

    whole, stream, common = ((build.CSRC / n).read_text() for n in ("limiter.hip", "limiter_stream.hip", "limiter_common.h"))
    assert '#include "limiter_common.h"' in whole  # "the un-streamed bits" by one copy of the chains, the sliding minimum and the run sums
    assert "fmaf(" not in whole and "fmaf(" not in stream and "fmaf(" in common
    for name in ("true_peak4(", "smooth_gains(", "gain_buf_floats("):
        assert len(re.findall(r"^[^/\n]*\b(?:void|float\*|int) " + re.escape(name), common, re.M)) == 1 and name in whole and name in stream, name
        assert not re.search(r"\b(?:void|float\*|int) " + re.escape(name), whole + stream), name
    assert "double s = 0.0" in common and "double s" not in whole and "double s" not in stream  # the fp64 run sums
    defs = [p.name for p in sorted(build.CSRC.iterdir()) if p.suffix in (".hip", ".h") and "to_float(short" in p.read_text()]
    assert defs == ["sample_convert.h"]
    defs = [p.name for p in sorted(build.CSRC.iterdir()) if p.suffix in (".hip", ".h") and re.search(r"short from_float<short>\(", p.read_text())]
    assert defs == ["sample_convert.h"]
    defs = [p.name for p in sorted(build.CSRC.iterdir()) if p.suffix in (".hip", ".h") and re.search(r"\bint check_rows\(", p.read_text())]
    assert defs == ["vtts_internal.h"]  # the limiter's and the loudness meter's, the margin (TILE or SEGMENT) a parameter
    for name in ("limiter.hip", "loudness.hip"):
        assert "check_rows(" in (build.CSRC / name).read_text(), name


def test_create_refuses_what_the_header_rules_out(lib):
    w = C.c_int32(0)
    for rate, ms, want in ((8000, 5.0, 40), (16000, 5.0, 80), (22050, 5.0, 110), (96000, 10.0, 960), (16000, 2.0, 32)):
        rc, h = _create(lib, rate, ms)
        assert rc == 0 and lib.vtts_limstream_lookahead(h, C.byref(w)) == 0 and w.value == want
        lib.vtts_limstream_destroy(h)
    bad = [dict(rate=7999), dict(rate=96001), dict(ms=0.0), dict(ms=10.5), dict(ms=float("nan")), dict(rows=0), dict(rows=-1), dict(max_chunk=0),
           dict(max_chunk=(1 << 20) + 1), dict(ceiling=float("nan")), dict(ceiling=float("inf"))]
    for kw in bad:
        rc, _ = _create(lib, **kw)
        assert rc == -1 and lib.vtts_last_error(), kw
    _create(lib, max_chunk=0)
    assert b"max_chunk" in lib.vtts_last_error()
    assert _create(lib, max_chunk=1 << 20)[0] == 0
    assert lib.vtts_limstream_create(None, 0, 1, 1, -1.0, C.byref(C.c_void_p(0))) == -1
    lib.vtts_limstream_destroy(None)


def test_emit_and_state_bytes_and_reset(lib):
    from viettts_amd.limiter import stream_emit

    rng = np.random.default_rng(4)
    for rate, ms in ((16000, 5.0), (8000, 0.01), (96000, 10.0)):
        Wn = O.lookahead(rate, ms)
        for max_chunk in (1, 8192, 1 << 20):
            rc, h = _create(lib, rate, ms, rows=3, max_chunk=max_chunk)
            assert rc == 0
            n = C.c_size_t(0)
            assert lib.vtts_limstream_state_bytes(h, C.byref(n)) == 0
            # per row: two state buffers of 4 W + 66 floats rounded up to 4, two result floats per tile of the largest push, rounded up to 4
            state = (4 * Wn + 66 + 3) // 4 * 4
            tiles = -(-(max_chunk + 2 * Wn + 39) // O.TILE)
            assert n.value == 3 * ((2 * state + 2 * tiles + 3) // 4 * 4) * 4
            out = C.c_int64(0)
            for _ in range(300):
                R = int(rng.integers(0, 50000))
                F = stream_emit(0, 0, R, False, Wn)
                cnt, last = int(rng.integers(0, max_chunk + 1)), bool(rng.integers(0, 2))
                assert lib.vtts_limstream_emit(h, R, F, cnt, int(last), C.byref(out)) == 0 and out.value == stream_emit(R, F, cnt, last, Wn) == SO.emit(R, F, cnt, last, Wn)
            for R in range(0, 2 * Wn + 80):
                assert lib.vtts_limstream_emit(h, R, 0, 0, 0, C.byref(out)) == 0 and out.value == stream_emit(R, 0, 0, False, Wn)
            assert lib.vtts_limstream_emit(h, 5, 6, 0, 0, C.byref(out)) == -1 and lib.vtts_limstream_emit(h, 5, 0, -1, 0, C.byref(out)) == -1
            assert lib.vtts_limstream_reset(h, 2, 2.0) == 0 and lib.vtts_limstream_reset(h, 3, 1.0) == -1 and lib.vtts_limstream_reset(h, -1, 1.0) == -1
            assert lib.vtts_limstream_reset(h, 0, float("nan")) == -1
            lib.vtts_limstream_destroy(h)


def test_push_refuses_bad_arguments_before_any_launch(lib):
    """No GPU here: every refusal below is host arithmetic, and the pointers are never dereferenced."""
    rc, h = _create(lib, rows=3, max_chunk=100)
    assert rc == 0
    fake = C.c_void_p(0x1000)
    i32 = lambda *v: (C.c_int32 * len(v))(*v)  # noqa: E731
    got = i32(7, 7, 7, 7)

    def push(rows=(0, 1), counts=(10, 10), lasts=(0, 0), n=None, stride=0, dtype=0, odt=0, state=fake, chunk=fake, out=fake, res=fake):
        return lib.vtts_limstream_push(h, state, chunk, dtype, len(rows) if n is None else n, i32(*rows), stride, i32(*counts), i32(*lasts), out, odt, got, res, None)

    assert push(dtype=2) == -1 and push(odt=2) == -1 and push(n=0) == -1 and push(n=4, rows=(0, 1, 2, 0), counts=(1,) * 4, lasts=(0,) * 4) == -1
    assert push(state=None) == -1 and push(chunk=None) == -1 and push(out=None) == -1 and push(res=None) == -1 and push(state=C.c_void_p(0x1004)) == -1
    assert push(stride=-1) == -1 and push(stride=9) == -1 and b"c_stride" in lib.vtts_last_error()
    assert push(rows=(0, 3)) == -1 and push(rows=(-1, 0)) == -1 and b"outside" in lib.vtts_last_error()
    assert push(rows=(1, 1)) == -1 and b"twice" in lib.vtts_last_error()
    assert push(counts=(10, 101)) == -1 and b"max_chunk" in lib.vtts_last_error() and push(counts=(-1, 10)) == -1
    assert list(got) == [7, 7, 7, 7]  # and nothing was reported as emitted
    lib.vtts_limstream_destroy(h)


# ------------------------------------------------------------ the surface ------------------------------------------------------------
def test_python_surface_and_defaults():
    from viettts_amd import limiter, serving, streaming, synthesizer

    sig = inspect.signature(limiter.TruePeakLimiter.open_stream).parameters
    assert list(sig)[1:] == ["rows", "max_chunk", "ceiling_dbtp", "out_dtype"] and (sig["ceiling_dbtp"].default, sig["out_dtype"].default) == (-1.0, "f32")
    sig = inspect.signature(limiter.LimiterStream.push).parameters
    assert [sig[k].default for k in ("counts", "last", "rows")] == [None, False, None]
    assert inspect.signature(limiter.LimiterStream.reset).parameters["gain"].default == 1.0
    assert issubclass(limiter.LimiterStream, limiter.NativeHandle) and hasattr(limiter.LimiterStream, "__enter__") and hasattr(limiter.LimiterStream, "results")
    for fn in (streaming.stream_mel, streaming.synthesize_stream, serving.SpeechPool.__init__):
        sig = inspect.signature(fn).parameters
        assert (sig["limit"].default, sig["gain_db"].default, sig["ceiling_dbtp"].default) == (False, 0.0, -1.0), fn
    with pytest.raises(ValueError):
        limiter.LimiterStream(16000, 1, 100, device="cpu")
    for name in ("README.md", "DESIGN.md"):
        assert "vtts_limstream" in (O.REPO / name).read_text() or "LimiterStream" in (O.REPO / name).read_text(), name


def test_synthesizer_flags(capsys):
    from viettts_amd import synthesizer

    a = synthesizer.build_parser().parse_args([])
    assert a.ceiling_dbtp is None and a.gain_db is None
    a = synthesizer.build_parser().parse_args(["--stream", "--ceiling-dbtp", "-1", "--gain-db", "12"])
    assert (a.stream, a.ceiling_dbtp, a.gain_db) == (True, -1.0, 12.0)
    for argv in (["--text", "xin chào", "--ceiling-dbtp", "-1"], ["--text", "xin chào", "--gain-db", "6"], ["--mel-file", "m.npy", "--ceiling-dbtp", "-1", "--gain-db", "6"]):
        with pytest.raises(SystemExit):
            synthesizer.main(argv)
        assert "--loudness T --limit" in capsys.readouterr().err, argv
    with pytest.raises(SystemExit):
        synthesizer.main(["--text", "xin chào", "--stream", "--gain-db", "6"])
    assert "--gain-db needs --ceiling-dbtp" in capsys.readouterr().err
    with pytest.raises(SystemExit):  # the limiter is designed for the models' rate: no relabelled file
        synthesizer.main(["--mel-file", "m.npy", "--stream", "--ceiling-dbtp", "-1", "--sample-rate", "22050"])
    assert "--ceiling-dbtp with --sample-rate 22050" in capsys.readouterr().err
    # the refusals that were there stay as they are
    with pytest.raises(SystemExit):
        synthesizer.main(["--text", "xin chào", "--limit"])
    assert "--limit needs --loudness" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        synthesizer.main(["--text", "xin chào", "--stream", "--loudness", "-16"])
    assert "--stream with --loudness" in capsys.readouterr().err


def test_limit_off_takes_no_limiter_import_path():
    """What this covers is only that importing ``streaming`` and ``serving`` and planning with them does not import viettts_amd.limiter at module
    level (a process of its own, so that no other test's import counts).  That the ``limit=False`` calls themselves run without the module is
    tests/test_gpu_limiter_stream.py's, where they run with the module made unimportable."""
    import subprocess

    code = ("import sys, viettts_amd.streaming as s, viettts_amd.serving as v\n"
            "s.stream_plan(40, 50, 16, 4), v.RoundPlanner(2, 16, 4).submit(40, 50)\n"
            "assert 'viettts_amd.limiter' not in sys.modules\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=str(O.REPO), capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
