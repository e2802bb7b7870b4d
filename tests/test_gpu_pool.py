"""The acoustic model's slot pool (include/vtts_nat.h: vtts_nat_acoustic_pool_*) and ``viettts_amd.serving.SpeechPool`` on the GPU: rows that enter
and leave a running batch one by one, each against the model's own un-pooled call of that sentence alone, bit for bit.  Synthetic checkpoints."""
import numpy as np
import pytest
import torch

from _nat_sessions import decode_to as _decode_to, finish_all as _finish_all, mel0 as _mel0  # the drivers all widths share
from viettts_amd._lib import VttsError

pytestmark = pytest.mark.gpu
INVALID, STATE = -1, -2
LMAX, FMAX = 32, 128


def _case(seed, L):
    """A sentence as tests/test_gpu_stream.py::_case makes it: about 3 frames per token, one word-end token of no duration."""
    rng = np.random.default_rng(seed)
    tok = list(rng.integers(0, 100, size=L))
    dur = np.abs(rng.normal(3.0, 1.5, size=L)).astype(np.float32)
    dur[rng.integers(0, L)] = 0.0
    nf = max(1, int(np.sum(dur, dtype=np.float32)))
    return tok, dur, nf


# 77, 39, 6 and 110 frames, and a fifth sentence for a slot's second occupant; a dropout seed per row
CASES = {"a": _case(47, 25), "b": _case(48, 12), "c": _case(49, 3), "d": _case(48, 32), "e": _case(50, 9)}
SEEDS = {"a": 11, "b": 12, "c": 13, "d": 14, "e": 15}


@pytest.fixture(scope="module")
def acoustic():
    from viettts_amd.nat.acoustic import AcousticModel
    from viettts_amd.nat.synth import synthetic_acoustic_checkpoint

    m = AcousticModel(device="cuda:0")
    m.load_params(*synthetic_acoustic_checkpoint())
    yield m
    m.close()


@pytest.fixture(scope="module")
def refs(acoustic):
    """Every sentence alone through the un-pooled model, computed once: ``refs[key] = (mel0, mel)``, ``[n, mel_dim]`` each; ``key + "_x3"`` with the
    option bf16x3."""
    assert [CASES[k][2] for k in "abcd"] == [77, 39, 6, 110]
    out = {}
    for x3 in (0, 1):
        acoustic.set_option("bf16x3", x3)
        try:
            for k, (tok, dur, n) in CASES.items():
                mel = acoustic([tok], [dur], [n], dropout_seeds=[SEEDS[k]], to_host=False)[0].clone()
                out[k + ("_x3" if x3 else "")] = (_mel0(acoustic, acoustic._ws, 1, len(tok), n)[0].clone(), mel)
        finally:
            acoustic.set_option("bf16x3", 0)
    return out


def _admit(pool, slot, key):
    tok, dur, n = CASES[key]
    pool.admit(slot, tok, dur, n, dropout_seed=SEEDS[key])


def _pool_mel0(acoustic, pool):
    return _mel0(acoustic, pool._ws, pool.slots, pool.Lmax, pool.Fmax)


def _assert_rows(acoustic, pool, refs, rows, sfx=""):
    """``rows``: {slot: key}.  The slot's decoder mel and mel are the reference's over its frames and zero behind them."""
    mel0 = _pool_mel0(acoustic, pool)
    for slot, key in rows.items():
        r0, r = refs[key + sfx]
        n = r.shape[0]
        assert torch.equal(mel0[slot, :n], r0), (slot, key, "decoder mel")
        assert torch.equal(pool.mel[slot, :n], r), (slot, key, "mel")
        assert not bool(mel0[slot, n:].any()) and not bool(pool.mel[slot, n:].any()), (slot, key)


def _staggered(acoustic, refs, sfx=""):
    """77 frames at tick 0; 39 and 6 frames at tick 5 (odd: state parity and frame parity differ; the three share a 4-row group at different frames);
    110 frames at tick 23 (it passes its frame 64 while its neighbours are done)."""
    with acoustic.open_pool(4, LMAX, FMAX, 50) as pool:
        _admit(pool, 0, "a")
        _decode_to(pool, 5)
        _admit(pool, 1, "b")
        _admit(pool, 2, "c")
        _decode_to(pool, 23)
        _admit(pool, 3, "d")
        _decode_to(pool, 23 + 110)
        assert [pool.cursor(s) for s in range(4)] == [77, 39, 6, 110]
        rows = {0: "a", 1: "b", 2: "c", 3: "d"}
        mel0 = _pool_mel0(acoustic, pool)
        for slot, key in rows.items():
            assert torch.equal(mel0[slot, : CASES[key][2]], refs[key + sfx][0]), (slot, key)
        assert not bool(pool.mel.any())  # no window yet
        _finish_all(pool, 32)
        _assert_rows(acoustic, pool, refs, rows, sfx)


def test_staggered_admissions_equal_each_sentence_alone(acoustic, refs):
    _staggered(acoustic, refs)


def test_staggered_admissions_bf16x3(acoustic, refs):
    assert not torch.equal(refs["a_x3"][1], refs["a"][1])  # the option does change the bits
    acoustic.set_option("bf16x3", 1)
    try:
        _staggered(acoustic, refs, "_x3")
    finally:
        acoustic.set_option("bf16x3", 0)


def test_a_retired_slot_is_reused_beside_a_row_in_mid_sentence(acoustic, refs):
    with acoustic.open_pool(4, LMAX, FMAX, 50) as pool:
        _admit(pool, 0, "a")
        _admit(pool, 2, "c")
        _decode_to(pool, 17)
        pool.finish([(2, 0, 6)])
        first = pool.mel[2].clone()  # the first occupant's rows, read back before the slot goes
        pool.retire(2)
        _admit(pool, 2, "e")  # at an odd tick, the 77-frame row of its group at frame 17
        assert torch.equal(first[:6], refs["c"][1]) and not bool(first[6:].any())
        assert not bool(pool.mel[2].any())  # the slot's rows start from zero again
        _decode_to(pool, 17 + 77)
        _finish_all(pool, 50)
        _assert_rows(acoustic, pool, refs, {0: "a", 2: "e"})


def test_wide_tile_of_forty_slots(acoustic, refs):
    """B > 32: the step with two 32-sentence tiles per wave.  Rows in both tiles, at the tiles' edges, each alone in its 4-row group."""
    with acoustic.open_pool(40, LMAX, FMAX, 50) as pool:
        _admit(pool, 0, "a")
        _decode_to(pool, 3)
        _admit(pool, 31, "b")
        _admit(pool, 32, "c")
        _decode_to(pool, 10)
        _admit(pool, 39, "d")
        _decode_to(pool, 10 + 110)
        _finish_all(pool, 50)
        _assert_rows(acoustic, pool, refs, {0: "a", 31: "b", 32: "c", 39: "d"})
        idle = [s for s in range(40) if s not in (0, 31, 32, 39)]
        assert not bool(pool.mel[idle].any()) and not bool(_pool_mel0(acoustic, pool)[idle].any())


def test_one_finish_call_takes_a_window_per_row(acoustic, refs):
    """Rows at different frames, windows 1, 7 and 50 wide in one call; a right halo that passes the row's end, a window that ends exactly at the
    row's last frame, a first window (no left halo) beside a later one.  Frames below a row's finished mark are final, the rest still zero, rows not
    listed untouched."""
    keys = {0: "a", 1: "b", 2: "c", 3: "d"}

    def check(pool, listed):
        for slot, key in keys.items():
            if not pool.busy[slot]:
                continue
            f = pool.finished[slot]
            assert torch.equal(pool.mel[slot, :f], refs[key][1][:f]) and not bool(pool.mel[slot, f:].any()), (slot, f)
            assert slot in listed or torch.equal(pool.mel[slot], before[slot])

    with acoustic.open_pool(4, LMAX, FMAX, 50) as pool:
        _admit(pool, 0, "a")
        _admit(pool, 2, "c")
        _decode_to(pool, 5)
        _admit(pool, 1, "b")
        _decode_to(pool, 40)  # cursors 40, 35, 6
        before = pool.mel.clone()
        pool.finish([(0, 0, 1), (1, 0, 7), (2, 0, 50)])  # widths 1, 7 and 50; the third is cut at the row's 6 frames
        assert pool.finished[:3] == [1, 7, 6]
        check(pool, {0, 1, 2})
        _admit(pool, 3, "d")
        _decode_to(pool, 80)  # cursors 77, 39, 6, 40
        before = pool.mel.clone()
        pool.finish([(0, 1, 51), (1, 7, 35), (3, 0, 7)])  # 50 wide; right halo [35, 45) past the row's 39 frames; a first window beside later ones
        check(pool, {0, 1, 3})
        before = pool.mel.clone()
        pool.finish([(1, 35, 39), (3, 7, 8)])  # ends exactly at the row's last frame; width 1 in mid-row
        check(pool, {1, 3})
        before = pool.mel.clone()
        pool.finish([(0, 51, 77)])
        check(pool, {0})
        assert pool.finished == [77, 39, 6, 8]


def test_refused_calls_return_their_status_and_enqueue_nothing(acoustic, refs):
    def refused(status, fn, *a, **kw):
        with pytest.raises(VttsError) as e:
            fn(*a, **kw)
        assert e.value.status == status, e.value

    tok, dur, n = CASES["b"]
    refused(STATE, acoustic._on_stream, "pool_decode", 1)  # no pool on this handle (the refs fixture's forward() calls were the last)
    pool = acoustic.open_pool(4, LMAX, FMAX, 8)
    _admit(pool, 1, "b")
    pool.decode(17)
    pool.finish([(1, 0, 7)])
    torch.cuda.synchronize()
    mel, mel0 = pool.mel.clone(), _pool_mel0(acoustic, pool).clone()
    refused(INVALID, pool.admit, 4, tok, dur, n)  # slots are 0 .. 3
    refused(INVALID, pool.admit, -1, tok, dur, n)
    refused(INVALID, pool.admit, 0, list(range(LMAX + 1)), np.ones(LMAX + 1, np.float32), n)  # more tokens than Lmax
    refused(INVALID, pool.admit, 0, tok, dur, 0)
    refused(INVALID, pool.admit, 0, tok, dur, FMAX + 1)
    refused(STATE, pool.admit, 1, tok, dur, n)  # busy
    refused(STATE, pool.retire, 0)  # free
    refused(STATE, pool.finish, [(0, 0, 4)])  # free
    refused(INVALID, pool.retire, 4)
    refused(STATE, pool.finish, [(1, 7, 8)])  # reads the decoder's frames up to 18: the row stands at 17
    refused(INVALID, pool.finish, [(1, 8, 9)])  # a gap
    refused(INVALID, pool.finish, [(1, 4, 7)])  # an overlap
    refused(INVALID, pool.finish, [(1, 7, 7)])  # empty
    refused(INVALID, pool.finish, [(1, 7, 16)])  # wider than max_window
    refused(INVALID, pool.finish, [])
    acoustic.set_option("bf16x3", 1)
    try:
        refused(STATE, pool.decode, 1)  # the option changed since open
    finally:
        acoustic.set_option("bf16x3", 0)
    # a stream that is being captured
    side, x, g = torch.cuda.Stream(), torch.zeros(8, device="cuda:0"), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        x.add_(1.0)
        refused(INVALID, pool.decode, 1)
        refused(INVALID, pool.finish, [(1, 7, 8)])
    torch.cuda.synchronize()
    assert pool.tick == 17 and pool.finished[1] == 7  # the host's copy did not move either
    assert torch.equal(pool.mel, mel) and torch.equal(_pool_mel0(acoustic, pool), mel0)  # nothing ran
    pool.decode(1)
    refused(INVALID, pool.finish, [(1, 7, 8), (1, 8, 9)])  # a slot twice (its first window alone is due now)
    assert pool.finished[1] == 7 and torch.equal(pool.mel, mel)
    pool.finish([(1, 7, 8)])  # and the pool carries on
    assert torch.equal(pool.mel[1, :8], refs["b"][1][:8])
    # forward() ends the pool
    assert torch.equal(acoustic([tok], [dur], [n], dropout_seeds=[SEEDS["b"]], to_host=False)[0], refs["b"][1])
    refused(STATE, pool.decode, 1)
    pool.close()
    pool.close()
    # a stale MelPool cannot drive (or end) a newer pool; nor can a stream
    p1 = acoustic.open_pool(4, LMAX, FMAX, 8)
    p2 = acoustic.open_pool(4, LMAX, FMAX, 8)
    refused(STATE, p1.decode, 1)
    refused(STATE, p1.admit, 0, tok, dur, n)
    p1.close()
    _admit(p2, 0, "c")
    p2.decode(6)
    p2.finish([(0, 0, 6)])
    assert p2.tick == 6 and torch.equal(p2.mel[0, :6], refs["c"][1])
    st = acoustic.open_stream([tok], [dur], [n], max_window=8, dropout_seeds=[SEEDS["b"]])  # a session ends the pool
    refused(STATE, p2.decode, 1)
    p3 = acoustic.open_pool(4, LMAX, FMAX, 8)  # ... and a pool the session
    refused(STATE, st.decode, 8)
    st.close()
    p3.decode(1)
    p3.close()
    p2.close()


@pytest.fixture(scope="module")
def requests():
    """Five requests, about 25 to 70 kept frames: prefixes of the shortest transcript sentence, each closed by the silence token."""
    from pathlib import Path

    from viettts_amd.nat import text2mel as t2m
    from viettts_amd.nat.duration import DurationModel
    from viettts_amd.nat.synth import synthetic_duration_checkpoint, transcript_sentences

    dm = DurationModel()
    dm.load_params(*synthetic_duration_checkpoint())
    tdir = Path(__file__).parent / "golden" / "text"
    whole = min(transcript_sentences(26, tdir / "transcript.txt", tdir / "lexicon.txt"), key=len)
    sents = [list(whole[:k]) + [t2m.FLAGS.sil_index] for k in range(4, len(whole))]
    sil = 0.05
    _, nfr, trail = t2m.frame_plan(sents, dm(sents), sil)
    picked = []
    for want in (25, 70, 40, 55, 33):  # the sentence whose kept frames come nearest, each once
        i = min((k for k in range(len(sents)) if k not in picked), key=lambda k: (abs(nfr[k] - trail[k] - want), k))
        picked.append(i)
    yield {"dm": dm, "sil": sil, "tokens": [sents[i] for i in picked], "T": [nfr[i] - trail[i] for i in picked], "Lmax": max(len(sents[i]) for i in picked),
           "Fmax": max(nfr[i] for i in picked)}
    dm.close()


@pytest.mark.parametrize("first", [None, 4])
def test_speech_pool_equals_every_request_streamed_alone(acoustic, requests, first):
    """3 slots, 5 requests submitted between rounds (two of them queue): every request's PCM16 equals ``synthesize_stream`` of it alone."""
    from viettts_amd.hifigan.config import V1
    from viettts_amd.hifigan.generator import Generator
    from viettts_amd.hifigan.synth import synthetic_params
    from viettts_amd.serving import SpeechPool
    from viettts_amd.streaming import synthesize_stream

    rq = requests
    assert all(t >= 17 for t in rq["T"])  # more than one chunk each
    gen = Generator(V1, device="cuda:0", dtype="bf16")
    gen.load_params(synthetic_params(V1, 4321, "scaled"))
    try:
        kw = dict(chunk_frames=16, first_chunk_frames=first, out_dtype="pcm16")
        alone = [np.concatenate([c.copy() for c in synthesize_stream(t, rq["dm"], acoustic, gen, silence_duration=rq["sil"], dropout_seed=100 + i, **kw)])
                 for i, t in enumerate(rq["tokens"])]
        sp = SpeechPool(rq["dm"], acoustic, gen, 3, rq["Lmax"], rq["Fmax"], **kw)
        got, done, ids = {}, set(), []

        def take(results):
            for rid, pcm, last in results:
                assert rid not in done and pcm.dtype == np.int16
                got.setdefault(rid, []).append(pcm.copy())
                if last:
                    done.add(rid)

        for i in (0, 1, 2):
            ids.append(sp.submit(rq["tokens"][i], silence_duration=rq["sil"], dropout_seed=100 + i))
        take(sp.step())
        ids.append(sp.submit(rq["tokens"][3], silence_duration=rq["sil"], dropout_seed=103))  # every slot is taken: these two queue
        take(sp.step())
        ids.append(sp.submit(rq["tokens"][4], silence_duration=rq["sil"], dropout_seed=104))
        assert len(sp.planner.queue) == 2
        take(sp.drain())
        sp.close()
        assert done == set(ids) and sp.idle
        for i, rid in enumerate(ids):
            pcm = np.concatenate(got[rid])
            assert pcm.shape == (gen.hop * rq["T"][i],) == alone[i].shape
            assert np.array_equal(pcm, alone[i]), i
    finally:
        gen.close()
