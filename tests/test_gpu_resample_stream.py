"""The streamed resampler (include/vtts_rsstream.h, viettts_amd/csrc/resample_stream.hip) on the GPU.  The yardstick is ``Resampler(in, out)``
on the whole row on the same GPU, and every comparison is exact: NaN positions as positions, everything else as bit patterns.  Pushes go
through the C ABI into outputs and a state pre-filled with NaN: whatever is read before it was written, or written past what a push emits,
shows."""
import ctypes as C

import numpy as np
import pytest
import torch

import _audio_oracle as A
import _resample_stream_oracle as SO
from viettts_amd import _lib
from viettts_amd._handle import ptr
from viettts_amd._lib import VttsError

pytestmark = pytest.mark.gpu
INVALID, STATE = -1, -2
OPB = 1024
_RS = {}
_WHOLE = {}
RANDOM = [int(v) for v in np.random.default_rng(9).integers(1, 500, 40) * np.random.default_rng(10).integers(0, 2, 40)] + [333]
IDS = [f"{a}-{b}" for a, b in SO.RATES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    yield torch.device("cuda:0")
    for r in _RS.values():
        r.close()
    _RS.clear()
    _WHOLE.clear()


def _rs(dev, fi, fo):
    from viettts_amd.audio import Resampler

    if (fi, fo) not in _RS:
        _RS[fi, fo] = Resampler(fi, fo, dev)
    return _RS[fi, fo]


def _row(seed, S, pcm=False):
    x = A.speechlike(np.random.default_rng(seed), S) if S > 1 else np.full(S, 0.25, np.float32)
    return np.rint(x * 32767.0).astype(np.int16) if pcm else x


def _whole(rs, x, out_dtype="f32", key=None):
    """The yardstick: the resampler on the whole row -> a device tensor, computed once per ``key``."""
    k = None if key is None else (rs.in_rate, rs.out_rate, key, x.dtype.str, out_dtype)
    if len(x) == 0:  # (the resampler takes no [1, 0] batch; the contract's empty row has no samples)
        return torch.zeros(0, dtype=torch.int16 if out_dtype == "pcm16" else torch.float32, device=rs.device)
    if k is None or k not in _WHOLE:
        y = rs(torch.from_numpy(x[None, :]).to(rs.device), out_dtype=out_dtype)[0].clone()
        if k is None:
            return y
        _WHOLE[k] = y
    return _WHOLE[k]


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    return SO.same(a.cpu().numpy(), b.cpu().numpy())


def _open(rs, rows, max_chunk, out_dtype="f32"):
    s = rs.open_stream(rows, max_chunk, out_dtype)
    s._state.fill_(0xFF)  # NaNs
    return s


def _push(s, rows, chunks, lasts, packed, lead=0):
    """One push through the C ABI.  ``chunks``: one numpy array per row; ``lead``: samples of padding ahead of a packed push, so that its rows
    start at odd addresses.  Returns the emitted samples per row (device tensors)."""
    n = len(rows)
    counts = [len(c) for c in chunks]
    dt = chunks[0].dtype
    pad = np.full(lead, np.nan if dt == np.float32 else -32768, dt)
    if packed:
        host, stride = np.concatenate([pad, *chunks, np.zeros(1, dt)]), 0
    else:
        stride = max(max(counts), 1) + 3
        host = np.full((n, stride), np.nan if dt == np.float32 else -32768, dt)
        for i, c in enumerate(chunks):
            host[i, :len(c)] = c
    src = torch.from_numpy(host).to(s.device)
    src_ptr = C.c_void_p(src.data_ptr() + lead * src.element_size()) if packed else ptr(src)
    pcm = s.out_dtype == "pcm16"
    room = sum(counts) if s.identity else sum((c * s.L + s.half) // s.M + 2 for c in counts)
    want = [SO.emit(*s.cursor(r)[:2], c, bool(z), s.L, s.M, s.half) - s.cursor(r)[1] for r, c, z in zip(rows, counts, lasts)]
    assert sum(want) <= room  # the header's bound on what a push emits
    out = torch.full((room + 8,), -12345, dtype=torch.int16, device=s.device) if pcm else torch.full((room + 8,), float("nan"), device=s.device)
    i32 = C.c_int32 * n
    got = i32()
    s._on_stream("push", ptr(s._state), src_ptr, int(dt == np.int16), n, i32(*rows), stride, i32(*counts), i32(*[int(v) for v in lasts]), ptr(out), int(pcm), got)
    em = [int(v) for v in got]
    assert em == want, (em, want)  # each push's count is the rule's
    total = sum(em)
    tail = out[total:]
    assert bool((tail == -12345).all() if pcm else torch.isnan(tail).all())  # nothing past what the push emits
    return list(torch.split(out[:total], em))


def _feed(s, xs, sizes, packed, slots=None, flush=False, lead=0):
    """Rows ``xs`` (all of one dtype) in chunks of ``sizes`` (cycled), each row until it ends.  Returns per row the concatenation of its pushes."""
    slots = list(range(len(xs))) if slots is None else slots
    at, parts, live, k = [0] * len(xs), [[] for _ in xs], list(range(len(xs))), 0
    while live:
        size = sizes[k % len(sizes)]
        k += 1
        chunks = [xs[i][at[i]:at[i] + size] for i in live]
        ends = [at[i] + size >= len(xs[i]) for i in live]
        lasts = [e and not flush for e in ends]
        for i, y in zip(live, _push(s, [slots[i] for i in live], chunks, lasts, packed, lead)):
            parts[i].append(y)
        for i in live:
            at[i] += size
        done = [i for i, e in zip(live, ends) if e]
        if flush and done:
            for i, y in zip(done, _push(s, [slots[i] for i in done], [xs[i][:0] for i in done], [True] * len(done), packed, lead)):
                parts[i].append(y)
        live = [i for i in live if i not in done]
    return [torch.cat(p) for p in parts]


def _lengths(fi, fo):
    L, M, half = A.ratio(fi, fo)
    d = max(SO.delay(L, M, half), 2)
    return [1, d - 1, d, d + 1, 3001]


# ------------------------------------------------------------ 1. every rate, every chunking ------------------------------------------------------------
@pytest.mark.parametrize("pcm_in,out_dtype", [(False, "f32"), (False, "pcm16"), (True, "f32")], ids=["f32-f32", "f32-pcm16", "pcm16-f32"])
@pytest.mark.parametrize("rates", SO.RATES, ids=IDS)
def test_any_chunking_gives_the_whole_rows_bits(dev, rates, pcm_in, out_dtype):
    """Rows of 1, delay - 1, delay, delay + 1 and 3001 samples, pushed together in one session: all at once, in random sizes with zero-count
    pushes between them, and with an empty last flush; strided and packed.  Every push's count is the emit rule's (``_push``), the
    concatenation is the un-streamed call's, and so is the total."""
    rs = _rs(dev, *rates)
    xs = [_row(100 + i, S, pcm_in) for i, S in enumerate(_lengths(*rates))]
    want = [_whole(rs, x, out_dtype, key=("len", i)) for i, x in enumerate(xs)]
    for sizes, packed, flush in (([3001], False, False), ([3001], True, True), (RANDOM, True, False), (RANDOM, False, True)):
        with _open(rs, len(xs), 3001, out_dtype) as s:
            got = _feed(s, xs, sizes, packed, flush=flush)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape == (rs.out_samples(len(xs[i])),) and _same(g, w), (rates, sizes[0], packed, flush, len(xs[i]))


@pytest.mark.parametrize("rates", SO.RATES, ids=IDS)
def test_one_sample_chunks(dev, rates):
    rs = _rs(dev, *rates)
    x = _row(7, 300)
    with _open(rs, 1, 1) as s:
        got = _feed(s, [x], [1], True)[0]
        assert s.cursor(0) == (300, rs.out_samples(300), True)
    assert _same(got, _whole(rs, x, key="one"))


# ------------------------------------------------------------ 2. tile edges ------------------------------------------------------------
def _two_pushes(L, M, half, emit):
    """(first count, second count, last): a first push of 200 .. 207 samples and a second that emits exactly ``emit`` outputs, or None if no
    such pair exists."""
    for n1 in range(200, 208):
        F1 = SO.emit(0, 0, n1, False, L, M, half)
        for last in (False, True):
            for n in range(0, 2300):
                if SO.emit(n1, F1, n, last, L, M, half) - F1 == emit:
                    return n1, n, last
    return None


@pytest.mark.parametrize("rates,emit", [((16000, 48000), e) for e in (1023, 1024, 1025, 1026, 2049)] + [((16000, 24000), e) for e in (1023, 1024, 1025, 2049)],
                         ids=lambda v: str(v[1]) if isinstance(v, tuple) else str(v))
def test_pushes_that_emit_around_a_tile(dev, rates, emit):
    """A first push of about 200 samples, then a push that emits exactly ``emit`` outputs, then the rest.  Tiles are anchored at the row's F
    after the first push (528 at 3/1), not at a multiple of 1024.  At 3/1 every push emits a multiple of 3 (F' is 3 R' - 72, or 3 R' on the
    last push), so no push emits exactly 1024 or 1025 there: the test says so, takes 1023, 1026 and 2049 at 3/1, and takes 1023, 1024, 1025
    and 2049 at 3/2, where every count can leave."""
    rs = _rs(dev, *rates)
    L, M, half = A.ratio(*rates)
    x = _row(31, 2600)
    found = _two_pushes(L, M, half, emit)
    if rates == (16000, 48000) and emit in (1024, 1025):
        assert found is None and emit % 3 != 0
        return
    n1, n2, last = found
    F1 = SO.emit(0, 0, n1, False, L, M, half)
    assert F1 % OPB != 0 and (rates != (16000, 48000) or (n1, F1) == (200, 528))
    with _open(rs, 1, 2600, "pcm16") as s:
        parts = [_push(s, [0], [x[:n1]], [False], True)[0], _push(s, [0], [x[n1:n1 + n2]], [last], True)[0]]
        assert len(parts[1]) == emit
        if not last:
            parts.append(_push(s, [0], [x[n1 + n2:]], [True], True)[0])
    assert _same(torch.cat(parts), _whole(rs, x if not last else x[:n1 + n2], "pcm16"))


# ------------------------------------------------------------ 3. four slots at different cursors ------------------------------------------------------------
@pytest.mark.parametrize("rates", [(16000, 44100), (44100, 16000)], ids=["16000-44100", "44100-16000"])
@pytest.mark.parametrize("pcm_in", [False, True], ids=["f32", "pcm16"])
def test_rows_at_different_cursors_in_one_session(dev, rates, pcm_in):
    """Four slots of different lengths, named in a shuffled order, strided and packed (the packed pushes start one sample into their buffer,
    so every row of them sits at an odd address and the unaligned load path runs); the short row closes while the others go on; then its
    slot is reset and reused for another row, with the first row's history still in the buffer."""
    rs = _rs(dev, *rates)
    lens, slots = [2500, 700, 1801, 1200], [2, 0, 3, 1]
    xs = [_row(40 + i, S, pcm_in) for i, S in enumerate(lens)]
    want = [_whole(rs, x, "f32", key=("slots", i)) for i, x in enumerate(xs)]
    for packed in (False, True):
        with _open(rs, 4, 512) as s:
            got = _feed(s, xs, [301, 155, 512, 1], packed, slots=slots, lead=1)
            for g, w in zip(got, want):
                assert _same(g, w), (rates, packed)
            assert s.cursor(0)[2] and s.cursor(3)[2]
            with pytest.raises(VttsError) as e:
                _push(s, [0], [xs[1][:5]], [False], packed)
            assert e.value.status == STATE and s.cursor(0) == (700, rs.out_samples(700), True)
            s.reset(0)  # stale history of the 700-sample row stays in the slot's buffers
            assert s.cursor(0) == (0, 0, False)
            again = _feed(s, [xs[2]], [400], packed, slots=[0], lead=1)[0]
            assert _same(again, want[2]), (rates, packed)


# ------------------------------------------------------------ 4. the rows-per-launch boundary ------------------------------------------------------------
def test_rows_across_the_launch_split(dev):
    rs = _rs(dev, 16000, 24000)
    n = _lib.RSSTREAM_ROWS_PER_LAUNCH + 1
    x = np.stack([_row(500 + i, 64) for i in range(n)])
    want = rs(torch.from_numpy(x).to(dev))
    with _open(rs, n, 64) as s:
        a = _push(s, list(range(n)), [r[:40] for r in x], [False] * n, False)
        b = _push(s, list(range(n)), [r[40:] for r in x], [True] * n, True)
    for i in range(n):
        assert _same(torch.cat([a[i], b[i]]), want[i]), i


def test_pcm16_on_both_sides_off_the_identity_ratio(dev):
    """rs_stream_k<short, short>, the dtype pair the tests above reach only where the rates are equal (a copy): rows of 17, 4097 and
    2 * 4096 + 5 PCM16 samples at 3/2 (more than one tile, no multiple of it), at once and in random sizes with an empty last flush, strided
    and packed.  The whole row's PCM16 is float_to_pcm16 of its fp32 output, so the yardstick's own format is checked as well."""
    from viettts_amd import wavio

    rs = _rs(dev, 16000, 24000)
    xs = [_row(900 + i, S, True) for i, S in enumerate((17, 4097, 2 * 4096 + 5))]
    want = [_whole(rs, x, "pcm16") for x in xs]
    for x, w in zip(xs, want):
        assert w.dtype == torch.int16 and np.array_equal(w.cpu().numpy(), wavio.float_to_pcm16(_whole(rs, x, "f32").cpu().numpy()))
    for sizes, packed, flush in (([2 * 4096 + 5], False, False), (RANDOM, True, True)):
        with _open(rs, len(xs), 2 * 4096 + 5, "pcm16") as s:
            got = _feed(s, xs, sizes, packed, flush=flush)
        for x, g, w in zip(xs, got, want):
            assert g.dtype == torch.int16 and g.shape == w.shape == (rs.out_samples(len(x)),) and _same(g, w), (sizes[0], packed, len(x))


# ------------------------------------------------------------ 5. NaN and Inf ------------------------------------------------------------
@pytest.mark.parametrize("rates", SO.RATES[:-1], ids=IDS[:-1])
def test_nan_and_inf_reach_the_outputs_they_reach_unstreamed(dev, rates):
    """One NaN and one Inf mid-row, the NaN where only the padding taps' share of a push's history holds it."""
    rs = _rs(dev, *rates)
    L, M, half, kp4, _ = SO.design(*rates)
    x = _row(21, 3001)
    F2 = SO.emit(1000, SO.emit(0, 0, 1000, False, L, M, half), 1000, False, L, M, half)
    x[SO.newest(F2, L, M, half) - (kp4 - 1)] = np.nan
    x[2500] = np.inf
    want = _whole(rs, x)
    assert 0 < int(torch.isnan(want).sum()) < len(want) and bool(torch.isinf(want).any())
    for sizes in ([1000], [333]):
        with _open(rs, 1, 1000) as s:
            assert _same(_feed(s, [x], sizes, True)[0], want), (rates, sizes)


# ------------------------------------------------------------ refusals and the Python surface ------------------------------------------------------------
def test_refused_pushes_enqueue_nothing_and_python_push(dev):
    from viettts_amd.audio import Resampler, resample_emit

    rs = _rs(dev, 16000, 48000)
    x = _row(3, 1000)
    want = _whole(rs, x, "pcm16", key="py")
    with rs.open_stream(2, 600, "pcm16") as s:
        assert s.latency == 24 and (s.L, s.M, s.half) == (3, 1, 72)
        y0, c0 = s.push(torch.from_numpy(x[None, :600]).to(dev), rows=[1])
        assert c0 == [resample_emit(0, 0, 600, False, 3, 1, 72)] and y0.dtype == torch.int16
        with pytest.raises(VttsError) as e:
            s.push(torch.from_numpy(x[None, :601]).to(dev), rows=[1])
        assert e.value.status == INVALID and s.cursor(1) == (600, c0[0], False)
        with pytest.raises(VttsError) as e:
            s.push(torch.from_numpy(np.stack([x[:5], x[:5]])).to(dev), rows=[1, 1])
        assert e.value.status == INVALID and s.cursor(1) == (600, c0[0], False)
        y1, c1 = s.push(torch.from_numpy(x[600:]).to(dev), counts=[400], last=True, rows=[1])
        assert c0[0] + c1[0] == 3000 and _same(torch.cat([y0, y1]), want)
        with pytest.raises(ValueError):
            s.push(torch.from_numpy(x[:5]).to(dev))
    # a session without a table refuses, and says why
    fresh = Resampler(16000, 48000, dev)
    try:
        s = fresh.open_stream(1, 10)
        assert fresh._blob is not None and s.packed_blob() is fresh.packed_blob()  # the session binds the blob its Resampler packed
        s.close()
    finally:
        fresh.close()


# ------------------------------------------------------------ 6. hooks ------------------------------------------------------------
@pytest.fixture(scope="module")
def gen():
    from viettts_amd.hifigan.config import V1
    from viettts_amd.hifigan.generator import Generator
    from viettts_amd.hifigan.synth import synthetic_params

    g = Generator(V1, device="cuda:0", dtype="bf16")
    g.load_params(synthetic_params(V1, 4321, "scaled"))
    yield g
    g.close()


def test_stream_mel_out_rate(dev, gen):
    """``stream_mel(out_rate=48000, out_dtype="pcm16")`` on 40 frames in chunks of 16 equals ``Resampler(16000, 48000)`` on the concatenated
    float32 output of ``stream_mel`` without ``out_rate``; with ``limit=True`` on the limited one; ``out_rate=None`` and the models' own rate are
    the call without the argument, byte for byte."""
    from viettts_amd.hifigan.synth import synthetic_mel
    from viettts_amd.streaming import stream_mel

    mel = synthetic_mel(1, 40, 4)[0]
    rs = _rs(dev, 16000, 48000)
    plain = [c.copy() for c in stream_mel(gen, mel, 16)]
    for kw in ({"out_rate": None}, {"out_rate": 16000}):
        off = [c.copy() for c in stream_mel(gen, mel, 16, **kw)]
        assert len(off) == len(plain) and all(a.tobytes() == b.tobytes() for a, b in zip(off, plain))
    p16 = [c.copy() for c in stream_mel(gen, mel, 16, out_dtype="pcm16")]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(p16, [c.copy() for c in stream_mel(gen, mel, 16, out_dtype="pcm16", out_rate=None)]))
    whole = np.concatenate(plain)
    got = [c.copy() for c in stream_mel(gen, mel, 16, out_rate=48000, out_dtype="pcm16")]
    cat = np.concatenate(got)
    assert len(got) == len(plain) and cat.dtype == np.int16 and cat.shape == (3 * 256 * 40,)
    assert len(got[0]) == 3 * (len(plain[0]) - 24)  # 24 samples late
    assert np.array_equal(cat, _whole(rs, whole, "pcm16").cpu().numpy())
    lk = dict(limit=True, gain_db=12.0, ceiling_dbtp=-1.0)
    limited = np.concatenate([c.copy() for c in stream_mel(gen, mel, 16, **lk)])
    got = np.concatenate([c.copy() for c in stream_mel(gen, mel, 16, out_rate=48000, out_dtype="pcm16", **lk)])
    assert not np.array_equal(limited, whole) and np.array_equal(got, _whole(rs, limited, "pcm16").cpu().numpy())


def test_speech_pool_and_synthesize_stream_out_rate(dev, gen):
    """Two overlapping requests on two slots with ``out_rate=8000``: each equals ``Resampler(16000, 8000)`` on the request's own float32
    stream; ``synthesize_stream(out_rate=8000)`` likewise, with ``info`` carrying the converted count and the rate."""
    from pathlib import Path

    from viettts_amd.nat import text2mel as t2m
    from viettts_amd.nat.acoustic import AcousticModel
    from viettts_amd.nat.duration import DurationModel
    from viettts_amd.nat.synth import synthetic_acoustic_checkpoint, synthetic_duration_checkpoint, transcript_sentences
    from viettts_amd.serving import SpeechPool
    from viettts_amd.streaming import synthesize_stream

    dm, am = DurationModel(), AcousticModel(device="cuda:0")
    try:
        dm.load_params(*synthetic_duration_checkpoint())
        am.load_params(*synthetic_acoustic_checkpoint())
        tdir = Path(__file__).parent / "golden" / "text"
        whole = min(transcript_sentences(26, tdir / "transcript.txt", tdir / "lexicon.txt"), key=len)
        sents = [list(whole[:k]) + [t2m.FLAGS.sil_index] for k in range(4, len(whole))]
        sil = 0.05
        _, nfr, trail = t2m.frame_plan(sents, dm(sents), sil)
        picked = []
        for want in (45, 25):
            picked.append(min((k for k in range(len(sents)) if k not in picked), key=lambda k: (abs(nfr[k] - trail[k] - want), k)))
        toks, Ts = [sents[i] for i in picked], [nfr[i] - trail[i] for i in picked]
        rs = _rs(dev, 16000, 8000)
        kw = dict(chunk_frames=16, first_chunk_frames=4)
        plain = [np.concatenate([c.copy() for c in synthesize_stream(t, dm, am, gen, silence_duration=sil, dropout_seed=100 + i, **kw)]) for i, t in enumerate(toks)]
        want = [_whole(rs, p, "pcm16").cpu().numpy() for p in plain]

        def pool(**extra):
            sp = SpeechPool(dm, am, gen, 2, max(len(t) for t in toks), max(nfr[i] for i in picked), out_dtype="pcm16", **kw, **extra)
            ids = [sp.submit(t, silence_duration=sil, dropout_seed=100 + i) for i, t in enumerate(toks)]
            got, done = {}, set()
            for rid, pcm, last in sp.drain():
                assert rid not in done and pcm.dtype == np.int16
                got.setdefault(rid, []).append(pcm.copy())
                if last:
                    done.add(rid)
            sp.close()
            assert done == set(ids)
            return [np.concatenate(got[r]) for r in ids]

        for i, (a, w) in enumerate(zip(pool(out_rate=8000), want)):
            assert a.shape == w.shape == (128 * Ts[i],) and np.array_equal(a, w), i
        for a, b in zip(pool(), pool(out_rate=None)):
            assert a.tobytes() == b.tobytes()
        info = {}
        got = np.concatenate([c.copy() for c in synthesize_stream(toks[0], dm, am, gen, silence_duration=sil, dropout_seed=100, out_dtype="pcm16", out_rate=8000,
                                                                  info=info, **kw)])
        assert np.array_equal(got, want[0]) and info["samples"] == len(got) == 128 * Ts[0] and info["sample_rate"] == 8000
        info = {}
        list(synthesize_stream(toks[0], dm, am, gen, silence_duration=sil, dropout_seed=100, info=info, **kw))
        assert info["samples"] == 256 * Ts[0] and info["sample_rate"] == 16000
    finally:
        dm.close()
        am.close()
