"""The slot pool's round logic (``viettts_amd.serving.RoundPlanner``) driven with fake cursors, and the pool's C symbols: no GPU."""
import re
from pathlib import Path

import pytest

from viettts_amd import _lib
from viettts_amd.serving import RoundPlanner
from viettts_amd.streaming import POSTNET_HALO, stream_plan

REPO = Path(__file__).resolve().parents[1]
# (T, n_frames): a trimmed row, a row shorter than a chunk, one of a single frame, rows of several chunks, T = n_frames
REQS = [(57, 77), (6, 6), (1, 3), (110, 110), (39, 45), (64, 70), (33, 33)]


def _run(slots, chunk, first, reqs, step_ticks=None, late=()):
    """Rounds until the planner is idle.  ``late``: (round, T, n) requests submitted before that round.  Returns per id its chunks' steps in issue
    order, its windows, and the admission log [(round, id, slot)]."""
    pl = RoundPlanner(slots, chunk, first)
    meta, chunks, windows, admitted = {}, {}, {}, []
    for T, n in reqs:
        meta[pl.submit(T, n)] = (T, n)
    rnd_no = 0
    while not pl.idle:
        for r, T, n in late:
            if r == rnd_no:
                meta[pl.submit(T, n)] = (T, n)
        owner = {}
        for rid, slot in pl.admissions():
            admitted.append((rnd_no, rid, slot))
        for slot, row in enumerate(pl.rows):
            if row is not None:
                owner[slot] = row
        pl.advance(step_ticks or chunk)
        cursors = {slot: pl.cursor(slot) for slot in owner}  # the fake cursors: what the test itself derives from the clock
        rnd = pl.due(cursors)
        for slot, f0, f1 in rnd.windows:
            row = owner[slot]
            assert 0 < f1 - f0 <= pl.max_window  # no window wider than the pool was opened for
            assert cursors[slot] >= min(f1 + POSTNET_HALO, row.n_frames)  # ... or asked before the decoder has its halo
            windows.setdefault(row.id, []).append((f0, f1))
        for rid, slot, step, last in rnd.chunks:
            assert owner[slot].id == rid and cursors[slot] >= step.decode_upto
            chunks.setdefault(rid, []).append((step, last))
        for rid, slot in rnd.retired:
            assert pl.rows[slot] is None and chunks[rid][-1][1]
        rnd_no += 1
        assert rnd_no < 1000
    return pl, meta, chunks, windows, admitted


@pytest.mark.parametrize("slots, chunk, first", [(3, 32, None), (3, 16, 4), (8, 7, 1), (1, 32, 4), (2, 50, None)])
def test_chunks_cover_every_request_once_in_order_and_equal_the_solo_plan(slots, chunk, first):
    pl, meta, chunks, windows, _ = _run(slots, chunk, first, REQS)
    assert set(chunks) == set(meta) == set(range(len(REQS)))
    for rid, (T, n) in meta.items():
        steps = [s for s, _ in chunks[rid]]
        assert steps == stream_plan(T, n, chunk, first)  # the row's chunks are its solo plan's
        at = 0
        for s in steps:  # [0, T) exactly once, in order
            assert s.chunk.t0 == at < s.chunk.t1
            at = s.chunk.t1
        assert at == T
        assert [last for _, last in chunks[rid]] == [False] * (len(steps) - 1) + [True]
        w = windows[rid]  # windows in order and contiguous from 0, final up to what the last chunk's generator reads
        assert w[0][0] == 0 and all(a[1] == b[0] for a, b in zip(w, w[1:])) and w[-1][1] == steps[-1].mel_upto == T


def test_a_chunk_waits_until_its_rows_cursor_is_there():
    """One tick per round: nothing is issued before the cursor reaches the step's decode_upto, and each step is issued in the round it does."""
    pl = RoundPlanner(2, 8, 2)
    rid = pl.submit(20, 30)
    assert pl.admissions() == [(rid, 0)]
    plan = stream_plan(20, 30, 8, 2)
    issued = 0
    for cur in range(1, 31):
        rnd = pl.due({0: cur})
        want = [s for s in plan[issued:] if s.decode_upto <= cur]
        assert [c[2] for c in rnd.chunks] == want[: len(rnd.chunks)] and (rnd.chunks or not want)
        issued += len(rnd.chunks)
    assert issued == len(plan) and pl.idle


def test_more_requests_than_slots_queue_fifo_and_reuse_retired_slots():
    pl, meta, chunks, _, admitted = _run(3, 32, None, REQS, late=[(1, 12, 12), (2, 90, 100)])
    assert [rid for _, rid, _ in admitted] == sorted(meta)  # first come, first served
    assert [(r, s) for r, _, s in admitted[:3]] == [(0, 0), (0, 1), (0, 2)]  # the first three at once, lowest slot first
    assert all(r > 0 for r, _, _ in admitted[3:])  # the rest waited for a slot
    by_slot = {}
    for _, rid, slot in admitted:
        by_slot.setdefault(slot, []).append(rid)
    assert max(len(v) for v in by_slot.values()) > 1  # a retired slot was taken again
    assert set(chunks) == set(meta)


def test_a_window_never_exceeds_max_window_even_when_steps_pile_up():
    """A row whose cursor ran far ahead (a long decode call) still gets windows of at most max_window; the steps that do not fit wait a round."""
    pl = RoundPlanner(1, 8, 2)
    pl.submit(60, 60)
    pl.admissions()
    total, rounds = 0, 0
    while not pl.idle:
        rnd = pl.due({0: 60})
        assert rnd.chunks and all(f1 - f0 <= pl.max_window for _, f0, f1 in rnd.windows)
        total += len(rnd.chunks)
        rounds += 1
    assert total == len(stream_plan(60, 60, 8, 2)) and rounds > 1


def test_pool_symbols_are_declared_exported_and_have_prototypes():
    from viettts_amd.csrc.build import build

    build()
    lib = _lib.load()
    header = (REPO / "include" / "vtts_nat.h").read_text()
    names = ["vtts_nat_acoustic_pool_" + n for n in ("workspace_bytes", "open", "admit", "decode", "finish", "retire", "close")]
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGS and name in _lib.NAT_EXPORTS, name
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SIGS[name][1] and fn.restype is _lib.SIGS[name][0]
