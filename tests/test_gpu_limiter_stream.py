"""The streamed true-peak limiter (include/vtts_limstream.h, viettts_amd/csrc/limiter_stream.hip) on the GPU.  The bit-for-bit yardstick is
``TruePeakLimiter.limit`` on the whole row on the same GPU (``torch.equal``); the accuracy yardstick is the float64 oracle
(tests/_limiter_oracle.py) within tests/test_gpu_limiter.py's bound, 4 x ``gpu_reference().distance``.  Pushes go through the C ABI into
outputs, results and a state pre-filled with NaN: whatever is read before it was written, or written past what a push emits, shows."""
import contextlib
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _limiter_oracle as O
import _row_split as RS
from viettts_amd import _lib, wavio
from viettts_amd._handle import ptr
from viettts_amd._lib import VttsError

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS, W, TILE = 16000, 80, O.TILE
INVALID, STATE = -1, -2
_LIMS = {}
_WHOLE = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    yield torch.device("cuda:0")
    for m in _LIMS.values():
        m.close()
    _LIMS.clear()
    _WHOLE.clear()


def _lim(dev, rate=FS, ms=5.0):
    from viettts_amd.limiter import TruePeakLimiter

    if (rate, ms) not in _LIMS:
        _LIMS[rate, ms] = TruePeakLimiter(rate, device=dev, lookahead_ms=ms)
    return _LIMS[rate, ms]


@contextlib.contextmanager
def _no_limiter_module():
    """viettts_amd.limiter cannot be imported inside: a ``limit=False`` call that reached for it would raise ImportError."""
    saved = sys.modules.get("viettts_amd.limiter")
    sys.modules["viettts_amd.limiter"] = None
    with pytest.raises(ImportError):
        importlib.import_module("viettts_amd.limiter")
    try:
        yield
    finally:
        if saved is None:
            del sys.modules["viettts_amd.limiter"]
        else:
            sys.modules["viettts_amd.limiter"] = saved


def _as(x, pcm):
    return wavio.float_to_pcm16(x) if pcm else np.asarray(x, np.float32)


def _whole(lim, x, g, out_dtype="f32", key=None):
    """The yardstick: ``limit`` on the whole row -> (samples, true_peak, min_gain, gain) as device tensors, computed once per ``key``."""
    k = None if key is None else (lim.sample_rate, lim.lookahead, key, x.dtype.str, out_dtype)
    if len(x) == 0:  # (limit() takes no [1, 0] batch; the contract's empty row: no samples, true_peak 0, min_gain 1)
        t = lambda v: torch.tensor(v, dtype=torch.float32, device=lim.device)  # noqa: E731
        return torch.zeros(0, dtype=torch.int16 if out_dtype == "pcm16" else torch.float32, device=lim.device), t(0.0), t(1.0), t(float(g))
    if k is None or k not in _WHOLE:
        y, r = lim.limit(torch.from_numpy(x[None, :]).to(lim.device), gains=[float(g)], out_dtype=out_dtype)
        got = (y[0].clone(), r.true_peak[0].clone(), r.min_gain[0].clone(), r.gains[0].clone())
        if k is None:
            return got
        _WHOLE[k] = got
    return _WHOLE[k]


def _open(lim, rows, max_chunk, out_dtype="f32", ceiling=-1.0):
    s = lim.open_stream(rows, max_chunk, ceiling, out_dtype)
    s._state.fill_(0xFF)  # NaNs
    s._results.fill_(float("nan"))
    return s


def _push(s, rows, chunks, lasts, packed):
    """One push through the C ABI.  ``chunks``: one numpy array per row.  Returns the emitted samples per row (device tensors)."""
    n = len(rows)
    counts = [len(c) for c in chunks]
    dt = chunks[0].dtype
    if packed:
        host, stride = (np.concatenate(chunks) if sum(counts) else np.zeros(1, dt)), 0
    else:
        stride = max(max(counts), 1) + 3
        host = np.full((n, stride), np.nan if dt == np.float32 else -32768, dt)
        for i, c in enumerate(chunks):
            host[i, :len(c)] = c
    src = torch.from_numpy(host).to(s.device)
    pcm = s.out_dtype == "pcm16"
    room = sum(counts) + n * (s.latency + 15) + 8
    out = torch.full((room,), -12345, dtype=torch.int16, device=s.device) if pcm else torch.full((room,), float("nan"), device=s.device)
    i32 = C.c_int32 * n
    got = i32()
    s._on_stream("push", ptr(s._state), ptr(src), int(dt == np.int16), n, i32(*rows), stride, i32(*counts), i32(*[int(v) for v in lasts]), ptr(out), int(pcm),
                 got, ptr(s._results))
    em = [int(v) for v in got]
    total = sum(em)
    rest = out[total:]
    assert bool((rest == -12345).all()) if pcm else bool(torch.isnan(rest).all())  # nothing is written past what the push emits
    return list(torch.split(out[:total], em)), em


def _feed(s, xs, size, packed, slots=None):
    """Every row of ``xs`` in chunks of ``size`` through one session, all still-open rows in each push, the final chunk of a row as its ``last``
    (a zero-count last push for an empty row).  Returns the rows' emitted samples."""
    slots = list(range(len(xs))) if slots is None else slots
    at = [0] * len(xs)
    parts = [[] for _ in xs]
    live = list(range(len(xs)))
    while live:
        chunks = [xs[i][at[i]:at[i] + size] for i in live]
        lasts = [at[i] + size >= len(xs[i]) for i in live]
        ys, em = _push(s, [slots[i] for i in live], chunks, lasts, packed)
        for i, y, c, e, z in zip(live, ys, chunks, em, lasts):
            assert e == _emitted(at[i], len(c), z, s.lookahead, sum(p.numel() for p in parts[i])) == y.numel()
            parts[i].append(y)
            at[i] += len(c)
        live = [i for i, z in zip(live, lasts) if not z]
    return [torch.cat(p) for p in parts]


def _emitted(received, count, last, Wn, emitted):
    from viettts_amd.limiter import stream_emit

    return stream_emit(received, emitted, count, last, Wn) - emitted


def _rows_16k():
    """A subset of _limiter_oracle.gpu_rows(): the edge lengths up to 2 TILE + 1, and clicks, pairs, plateau, under."""
    keep = {f"len{S}" for S in O.edge_lengths() if S <= 2 * TILE + 1} | {"clicks", "pairs", "plateau", "under"}
    return [(i, n, x, g) for i, (n, x, g) in enumerate(O.gpu_rows()) if n in keep]


def _check_rows(lim, s, rows, got, pcm_in, out_dtype):
    res = s.results()
    for slot, (_, name, x, g) in enumerate(rows):
        y, tp, mg, gu = _whole(lim, _as(x, pcm_in), g, out_dtype, key=name)
        assert got[slot].shape == y.shape and torch.equal(got[slot], y), name
        assert torch.equal(res.true_peak[slot], tp) and torch.equal(res.min_gain[slot], mg) and torch.equal(res.gains[slot], gu), name


# ------------------------------------------------------------ chunkings ------------------------------------------------------------
@pytest.mark.parametrize("pcm_in,out_dtype,packed", [(False, "f32", False), (True, "pcm16", True), (False, "pcm16", True), (True, "f32", False),
                                                     (False, "f32", True), (True, "pcm16", False)])
@pytest.mark.parametrize("size", [16, 17, 2 * W + 24, 2 * W + 25, 4095, 4096, 4097, 8192])
def test_any_chunking_gives_the_whole_rows_bits(dev, size, pcm_in, out_dtype, packed):
    """18 rows from 0 to 16384 samples in one session, every open row in every push (so the rows end at different pushes), float32 and PCM16 in
    and out, strided and packed input: every row's pushes concatenated are ``limit`` on the whole row, and its results after the last push too."""
    lim = _lim(dev)
    rows = _rows_16k()
    assert len(rows) == 18
    with _open(lim, len(rows), size, out_dtype) as s:
        assert s.latency == 2 * W + 24 and s.lookahead == W
        for slot, (_, _, _, g) in enumerate(rows):
            s.reset(slot, float(g))
        got = _feed(s, [_as(x, pcm_in) for _, _, x, _ in rows], size, packed)
        _check_rows(lim, s, rows, got, pcm_in, out_dtype)


def test_one_sample_chunks(dev):
    lim = _lim(dev)
    x = O.speech(31, 400)
    with _open(lim, 1, 1) as s:
        s.reset(0, 4.0)
        got = _feed(s, [x], 1, False)
        y, tp, mg, gu = _whole(lim, x, 4.0)
        r = s.results()
        assert torch.equal(got[0], y) and torch.equal(r.true_peak[0], tp) and torch.equal(r.min_gain[0], mg) and float(mg) < 1.0 and float(r.gains[0]) == 4.0


def test_streamed_rows_agree_with_the_float64_oracle(dev):
    """The accuracy yardstick and its bound are tests/test_gpu_limiter.py's: the float64 restatement, 4 x the float32 restatement's distance."""
    f64, _, d = O.gpu_reference()
    assert 0 < d <= 4e-6
    bound = 4 * d
    lim = _lim(dev)
    rows = _rows_16k()
    with _open(lim, len(rows), 1000) as s:
        for slot, (_, _, _, g) in enumerate(rows):
            s.reset(slot, float(g))
        got = _feed(s, [x for _, _, x, _ in rows], 1000, True)
        res = s.results()
        worst = 0.0
        for slot, (i, name, x, g) in enumerate(rows):
            r = f64[i]
            if not len(x):
                assert float(res.true_peak[slot]) == 0.0 and float(res.min_gain[slot]) == 1.0
                continue
            err = float(np.abs(got[slot].cpu().numpy() - r.y).max())
            worst = max(worst, err)
            assert err <= bound, (name, err)
            assert abs(float(res.min_gain[slot]) - r.min_gain) <= bound / float(r.c), name
            assert abs(float(res.true_peak[slot]) - r.true_peak) <= 53 * 2.0 ** -24 * 3 * r.true_peak, name
            assert (float(res.min_gain[slot]) < 1.0) == (name != "under"), name
        print(f"\nlargest error {worst:.3e} of {bound:.3e}")


# ------------------------------------------------------------ cursors, slots, launches ------------------------------------------------------------
def test_rows_at_different_cursors_in_one_session(dev):
    """Four slots.  Rows are admitted at different pushes, the order of the rows changes from push to push, one row ends while the others are in
    mid-sentence, and its slot is reset and reused by a quiet row after a loud one.  Every row equals the row alone."""
    lim = _lim(dev)
    rng = np.random.default_rng(5)
    xs = {"a": O.speech(41, 9000), "b": O.speech(42, 5003), "c": O.speech(43, 700), "d": (0.05 * O.speech(44, 6001)).astype(np.float32), "e": O.speech(45, 2 * TILE + 300)}
    gains = {"a": 4.0, "b": 8.0, "c": 3.0, "d": 1.0, "e": 5.0}
    slot = {"a": 0, "b": 2, "c": 1, "d": 1, "e": 3}            # d takes c's slot once c has ended
    start = {"a": 0, "b": 2, "c": 1, "e": 3}
    with _open(lim, 4, 1200) as s:
        at = {k: 0 for k in xs}
        parts = {k: [] for k in xs}
        live, tick = [], 0
        while tick < 4 or live:
            for k, t in start.items():
                if t == tick:
                    s.reset(slot[k], gains[k])
                    live.append(k)
            if "c" not in live and at["c"] == len(xs["c"]) and at["d"] == 0 and "d" not in live:
                s.reset(slot["d"], gains["d"])
                live.append("d")
            order = [live[i] for i in rng.permutation(len(live))]
            sizes = {k: int(rng.integers(0, 1201)) for k in order}
            chunks = [xs[k][at[k]:at[k] + sizes[k]] for k in order]
            lasts = [at[k] + sizes[k] >= len(xs[k]) for k in order]
            if order:
                ys, _ = _push(s, [slot[k] for k in order], chunks, lasts, packed=bool(tick % 2))
                for k, y, c, z in zip(order, ys, chunks, lasts):
                    parts[k].append(y)
                    at[k] += len(c)
                    if z:
                        live.remove(k)
                        y0, tp, mg, gu = _whole(lim, xs[k], gains[k])
                        r = s.results()
                        assert torch.equal(torch.cat(parts[k]), y0), k
                        assert torch.equal(r.true_peak[slot[k]], tp) and torch.equal(r.min_gain[slot[k]], mg) and float(r.gains[slot[k]]) == gains[k], k
            tick += 1
        assert all(at[k] == len(xs[k]) for k in xs)
        assert float(s.results().min_gain[1]) == 1.0  # the quiet row in the loud row's slot


def test_rows_across_the_launch_split_are_the_rows_before_it(dev):
    """134 slots pushed at once: the cursors of 128 rows travel with one launch.  Slots 128 + b of the batch of tests/_row_split.py differ from
    slots b in content, length and gain and hold the longest row and a one-sample row: EVERY slot, the fillers included, is ``limit`` on
    that whole row bit for bit, results too, and within the float64 oracle's bound.  Three more slots behind them are rows 0 .. 2 again."""
    _, _, d = O.gpu_reference()
    bound = 4 * d
    split = _lib.LIMSTREAM_ROWS_PER_LAUNCH
    lim = _lim(dev)
    bt = RS.limiter_batch(split)
    xs = [np.array(bt.rows[b, :n]) for b, n in enumerate(bt.lengths)]  # (copies: the shared rows are read-only)
    xs += xs[:3]
    gains = [float(g) for g in bt.scalars] + [float(g) for g in bt.scalars[:3]]
    kind = list(bt.kind) + list(bt.kind[:3])
    refs = RS.per_kind(bt, lambda row: O.limit(row.content[: row.length], FS, row.scalar))
    refs += refs[:3]
    assert len(xs) == split + 6 and max(len(x) for x in xs) == len(xs[split + 1]) and len(xs[split + 2]) == 1
    with _open(lim, split + 6, 100) as s:
        for b, g in enumerate(gains):
            s.reset(b, g)
        got = _feed(s, xs, 100, True)
        r = s.results()
        worst = {False: 0.0, True: 0.0}
        for b, ref in enumerate(refs):
            y, tp, mg, gu = _whole(lim, xs[b], gains[b], key=("split", int(kind[b])))
            assert torch.equal(got[b], y), b
            assert torch.equal(r.true_peak[b], tp) and torch.equal(r.min_gain[b], mg) and torch.equal(r.gains[b], gu) and float(gu) == gains[b], b
            err = float(np.abs(got[b].cpu().numpy() - ref.y).max())
            worst[b >= split] = max(worst[b >= split], err / bound)
            assert err <= bound, (b, err)
            assert abs(float(r.min_gain[b]) - ref.min_gain) <= bound / float(ref.c), b
            assert abs(float(r.true_peak[b]) - ref.true_peak) <= 53 * 2.0 ** -24 * 3 * ref.true_peak, b
        print(f"\nlimiter stream rows across the split: worst error / bound {worst[False]:.3f} before, {worst[True]:.3f} behind the split (bound {bound:.2e})")
        for b in range(3):
            y, tp, mg, _ = _whole(lim, xs[b], gains[b], key=("split", int(kind[b])))
            assert torch.equal(got[b], y) and torch.equal(got[split + 3 + b], y) and float(mg) < 1.0
            assert torch.equal(r.true_peak[split + 3 + b], tp) and torch.equal(r.min_gain[split + 3 + b], mg) and torch.equal(r.min_gain[b], mg)
            assert len(xs[split + b]) != len(xs[b]) and gains[split + b] != gains[b] and not np.array_equal(xs[split + b][:1], xs[b][:1])
        y, _, _, _ = _whole(lim, xs[3], gains[3], key=("split", int(kind[3])))
        assert all(torch.equal(got[b], y) for b in range(3, split) if kind[b] == kind[3]) and kind[3] == kind[7] == kind[split - 1]


@pytest.mark.parametrize("rate,ms,S,size", [(16000, 2.0, 2 * TILE + 1, 1000), (22050, 5.0, TILE + 333, 777), (96000, 10.0, 6017, 2048)])
def test_other_rates_and_lookaheads(dev, rate, ms, S, size):
    """W = 32, W = 110, and W = 960 at 96 kHz: the largest span a workgroup stages."""
    lim = _lim(dev, rate, ms)
    assert lim.lookahead == O.lookahead(rate, ms)
    x = O.speech(700, S, rate)
    for out_dtype in ("f32", "pcm16"):
        with _open(lim, 2, size, out_dtype) as s:
            s.reset(1, 4.0)
            got = _feed(s, [x], size, False, slots=[1])
            y, tp, mg, _ = _whole(lim, x, 4.0, out_dtype)
            r = s.results()
            assert s.latency == 2 * lim.lookahead + 24
            assert torch.equal(got[0], y) and torch.equal(r.true_peak[1], tp) and torch.equal(r.min_gain[1], mg) and float(mg) < 1.0


def test_refused_pushes_enqueue_nothing(dev):
    lim = _lim(dev)
    x = O.speech(46, 3000)
    y, tp, mg, _ = _whole(lim, x, 4.0)
    with _open(lim, 3, 1000) as s:
        s.reset(0, 4.0)
        s.reset(2, 4.0)
        parts, _ = _push(s, [0, 2], [x[:1000], x[:1000]], [False, False], True)
        a, b = [parts[0]], [parts[1]]
        ys, _ = _push(s, [2], [x[1000:2000]], [False], True)
        b.append(ys[0])
        ys, _ = _push(s, [2], [x[2000:3000]], [True], True)  # slot 2 is closed now
        b.append(ys[0])
        assert torch.equal(torch.cat(b), y)
        torch.cuda.synchronize()
        state, results = s._state.clone(), s._results.clone()

        def refused(status, needle, rows, chunks, lasts):
            with pytest.raises(VttsError) as e:
                _push(s, rows, chunks, lasts, True)
            assert e.value.status == status and needle in str(e.value), str(e.value)
            torch.cuda.synchronize()
            assert torch.equal(s._state, state) and torch.equal(s._results.view(torch.int32), results.view(torch.int32))

        refused(STATE, "reset()", [0, 2], [x[1000:1500], x[:10]], [False, False])          # a closed row, beside a legal one
        refused(INVALID, "twice", [0, 1, 0], [x[1000:1500], x[:10], x[:10]], [False] * 3)
        refused(INVALID, "max_chunk", [1, 0], [x[:10], x[1000:2001]], [False, False])
        refused(INVALID, "outside", [0, 3], [x[1000:1500], x[:10]], [False, False])
        refused(INVALID, "outside", [-1], [x[:10]], [False])
        refused(INVALID, "n must be", [0, 1, 2, 0], [x[:10]] * 4, [False] * 4)
        # no slot's bookkeeping moved: slot 0 goes on where it was, slot 1 is still at its start
        ys, em = _push(s, [1, 0], [x[:0], x[1000:2000]], [False, False], True)
        assert em[0] == 0
        a.append(ys[1])
        ys, _ = _push(s, [0], [x[2000:]], [True], False)
        a.append(ys[0])
        assert torch.equal(torch.cat(a), y) and torch.equal(s.results().min_gain[0], mg) and torch.equal(s.results().true_peak[0], tp)


def test_python_push_accepts_what_it_documents(dev):
    """``push`` itself: [n, C] with and without counts, a packed tensor with counts, int16 in, ``last`` as a bool and as a sequence, a flush."""
    lim = _lim(dev)
    xa, xb = O.speech(47, 2500), O.speech(48, 2000)
    with lim.open_stream(2, 1000, out_dtype="pcm16") as s:
        s.reset(0, 4.0)
        s.reset(1, 3.0)
        ya, yb = [], []
        o, em = s.push(torch.from_numpy(np.stack([xa[:1000], xb[:1000]])).to(dev))
        ya.append(o[:em[0]]), yb.append(o[em[0]:])
        o, em = s.push(np.stack([xa[1000:2000], xb[1000:2000]]), counts=[1000, 1000], last=[False, True])
        ya.append(o[:em[0]]), yb.append(o[em[0]:])
        o, em = s.push(torch.from_numpy(xa[2000:]).to(dev), counts=[500], rows=[0])
        ya.append(o)
        o, em = s.push(torch.zeros((1, 0), device=dev), last=True, rows=[0])  # a flush
        ya.append(o)
        assert em == [len(xa) - sum(t.numel() for t in ya[:-1])] and o.dtype == torch.int16
        assert torch.equal(torch.cat(ya), _whole(lim, xa, 4.0, "pcm16")[0]) and torch.equal(torch.cat(yb), _whole(lim, xb, 3.0, "pcm16")[0])
        with pytest.raises(VttsError):
            s.push(xa[:10], counts=[10], rows=[1])  # closed
        with pytest.raises(ValueError):
            s.push(xa[:10], counts=[5], rows=[0])
    with pytest.raises(ValueError):
        lim.open_stream(1, 100, out_dtype="f16")


# ------------------------------------------------------------ hooks ------------------------------------------------------------
@pytest.fixture(scope="module")
def models():
    from pathlib import Path

    from viettts_amd.hifigan.config import V1
    from viettts_amd.hifigan.generator import Generator
    from viettts_amd.hifigan.synth import synthetic_params
    from viettts_amd.nat import text2mel as t2m
    from viettts_amd.nat.acoustic import AcousticModel
    from viettts_amd.nat.duration import DurationModel
    from viettts_amd.nat.synth import synthetic_acoustic_checkpoint, synthetic_duration_checkpoint, transcript_sentences

    dm, am = DurationModel(), AcousticModel(device="cuda:0")
    dm.load_params(*synthetic_duration_checkpoint())
    am.load_params(*synthetic_acoustic_checkpoint())
    gen = Generator(V1, device="cuda:0", dtype="bf16")
    gen.load_params(synthetic_params(V1, 4321, "scaled"))
    tdir = Path(__file__).parent / "golden" / "text"
    whole = min(transcript_sentences(26, tdir / "transcript.txt", tdir / "lexicon.txt"), key=len)
    sents = [list(whole[:k]) + [t2m.FLAGS.sil_index] for k in range(4, len(whole))]
    sil = 0.05
    _, nfr, trail = t2m.frame_plan(sents, dm(sents), sil)
    picked = []
    for want in (60, 25, 40):
        picked.append(min((k for k in range(len(sents)) if k not in picked), key=lambda k: (abs(nfr[k] - trail[k] - want), k)))
    yield {"dm": dm, "am": am, "gen": gen, "sil": sil, "tokens": [sents[i] for i in picked], "T": [nfr[i] - trail[i] for i in picked],
           "Lmax": max(len(sents[i]) for i in picked), "Fmax": max(nfr[i] for i in picked), "rate": t2m.FLAGS.sample_rate}
    gen.close()
    dm.close()
    am.close()


def test_synthesize_stream_limit(dev, models):
    """``limit=True, gain_db=+20``: the chunks concatenated are ``limit`` of the whole un-limited streamed waveform with that gain, bit for bit, as
    float32 and as PCM16; ``limit=False`` is the call without the argument."""
    from viettts_amd.limiter import default_limiter
    from viettts_amd.streaming import synthesize_stream

    m = models
    lim = default_limiter(dev, m["rate"])
    kw = dict(silence_duration=m["sil"], dropout_seed=7, chunk_frames=16, first_chunk_frames=4)
    run = lambda **k: [c.copy() for c in synthesize_stream(m["tokens"][0], m["dm"], m["am"], m["gen"], **kw, **k)]  # noqa: E731
    plain = run()
    with _no_limiter_module():
        off = run(limit=False)
    assert len(off) == len(plain) and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(off, plain))
    whole = np.concatenate(plain)
    g = float(np.float32(10.0 ** (20.0 / 20.0)))
    for out_dtype in ("f32", "pcm16"):
        info = {}
        got = run(limit=True, gain_db=20.0, out_dtype=out_dtype, info=info)
        y, tp, mg, gu = _whole(lim, whole, g, out_dtype)
        cat = np.concatenate(got)
        assert len(got) == len(plain) and cat.shape == whole.shape == (256 * m["T"][0],)
        assert len(got[0]) == max(0, (len(plain[0]) - lim.lookahead * 2 - 24) // 16 * 16) and len(got[-1]) > len(plain[-1])
        assert np.array_equal(cat, y.cpu().numpy()) and cat.dtype == (np.int16 if out_dtype == "pcm16" else np.float32)
        assert info["limiter"] == {"true_peak": float(tp), "min_gain": float(mg), "gain": g} and float(mg) < 1.0
    print(f"\n{len(whole)} samples in {len(plain)} chunks, true peak {float(tp):.4f}, gain {g:.2f}, min gain {float(mg):.4f}")


def test_stream_mel_limit_and_the_cli(dev, models, tmp_path):
    """``stream_mel(limit=True)`` on a saved mel, and ``synthesizer --stream --mel-file --ceiling-dbtp -1 --gain-db 12`` in a process of its own:
    the plain streamed CLI's header, and the samples of ``limit`` on the plain streamed waveform."""
    from viettts_amd.hifigan.config import V1
    from viettts_amd.hifigan.synth import synthetic_mel, synthetic_params
    from viettts_amd.hifigan.weights import save_haiku_pickle
    from viettts_amd.limiter import default_limiter
    from viettts_amd.streaming import stream_mel

    mel = synthetic_mel(1, 40, 4)[0]
    gen = models["gen"]
    lim = default_limiter(dev, models["rate"])
    g = float(np.float32(10.0 ** (12.0 / 20.0)))
    plain = np.concatenate([c.copy() for c in stream_mel(gen, mel, 16)])
    got = np.concatenate([c.copy() for c in stream_mel(gen, mel, 16, out_dtype="pcm16", limit=True, gain_db=12.0, ceiling_dbtp=-1.0)])
    want = _whole(lim, plain, g, "pcm16")[0].cpu().numpy()
    assert got.shape == (256 * 40,) and np.array_equal(got, want)

    (tmp_path / "assets/hifigan").mkdir(parents=True)
    (tmp_path / "assets/infore/hifigan").mkdir(parents=True)
    (tmp_path / "assets/hifigan/config.json").write_text(open(os.path.join(REPO, "assets/hifigan/config.json")).read())
    save_haiku_pickle(tmp_path / "assets/infore/hifigan/hk_hifi.pickle", synthetic_params(V1, 4321, "scaled"))
    np.save(tmp_path / "m.npy", mel)
    env = dict(os.environ, PYTHONPATH=REPO, VTTS_MEL2WAVE_DTYPE="bf16")  # the engine of ``models``: the same kernels, the same bits
    r = subprocess.run([sys.executable, "-m", "viettts_amd.synthesizer", "--mel-file", "m.npy", "--sample-rate", "16000", "--stream", "--chunk-frames", "16",
                        "--output", "lim.wav", "--ceiling-dbtp", "-1", "--gain-db", "12"], cwd=tmp_path, env=env, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    data = (tmp_path / "lim.wav").read_bytes()
    assert data[:44] == wavio.wav_header_pcm16(256 * 40, 16000) and len(data) == 44 + 2 * 256 * 40
    sr, pcm = wavio.read_wav(tmp_path / "lim.wav")
    assert sr == 16000 and np.array_equal(pcm.astype(np.int16), want)
    assert np.abs(want.astype(np.int32)).max() <= int(np.ceil(32767 * 10 ** (-1 / 20) * (1 + 2.0 ** -22)))


def test_speech_pool_limit(dev, models):
    """3 requests on 2 slots (one queues and reuses a slot): every request's PCM16 equals ``synthesize_stream(limit=True)`` of it alone; with
    ``limit=False`` the pool is the pool without the argument."""
    from viettts_amd.serving import SpeechPool
    from viettts_amd.streaming import synthesize_stream

    m = models
    kw = dict(chunk_frames=16, first_chunk_frames=4, out_dtype="pcm16")
    lk = dict(limit=True, gain_db=20.0, ceiling_dbtp=-2.0)

    def pool(**extra):
        sp = SpeechPool(m["dm"], m["am"], m["gen"], 2, m["Lmax"], m["Fmax"], **kw, **extra)
        ids = [sp.submit(t, silence_duration=m["sil"], dropout_seed=100 + i) for i, t in enumerate(m["tokens"])]
        got, done = {}, set()
        for rid, pcm, last in sp.drain():
            assert rid not in done and pcm.dtype == np.int16
            got.setdefault(rid, []).append(pcm.copy())
            if last:
                done.add(rid)
        sp.close()
        assert done == set(ids)
        return [np.concatenate(got[r]) for r in ids]

    alone = [np.concatenate([c.copy() for c in synthesize_stream(t, m["dm"], m["am"], m["gen"], silence_duration=m["sil"], dropout_seed=100 + i, **kw, **lk)])
             for i, t in enumerate(m["tokens"])]
    plain = [np.concatenate([c.copy() for c in synthesize_stream(t, m["dm"], m["am"], m["gen"], silence_duration=m["sil"], dropout_seed=100 + i, **kw)])
             for i, t in enumerate(m["tokens"])]
    for i, (a, b) in enumerate(zip(pool(**lk), alone)):
        assert a.shape == (256 * m["T"][i],) == b.shape and np.array_equal(a, b), i
        assert not np.array_equal(a, plain[i])
    with _no_limiter_module():
        off = pool(limit=False)
    for a, b, c in zip(pool(), off, plain):
        assert np.array_equal(a, b) and np.array_equal(a, c)
