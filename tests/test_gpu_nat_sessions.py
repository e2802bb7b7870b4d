"""The NAT decoder's streamed, pooled and grouped entry points on the GPU at every kind of model width vtts_nat_acoustic_create() accepts (the sets S, O,
R, W and X of tests/_nat_dims.py), each against the plain call of the same model, BIT FOR BIT: include/vtts_nat.h promises the plain call's bits for every
one of them, and tests/test_gpu_nat_dims.py pins the plain call to the fp64 oracles at each set.  Every comparison here is torch.equal or np.array_equal;
there is no tolerance in this module.  Sentences, drivers and the restated arithmetic are tests/_nat_sessions.py's; tests/test_nat_sessions_cpu.py shows
without a GPU that the cases reach the paths named below.

What runs, per width set unless said otherwise:

* the streaming session (stream_begin / stream_decode / stream_finish) on the ragged batch (1, 1), (2, 16), (9, 33), (64, 65), (65, 129) in windows of 1, 7, 32
  and 50 frames (R and W all four — W's compact window goes through the FOLD instantiation of nat_conv_mfma_k —, S, O and X 7 and 50), asserted after
  every window and as a whole, rows past a sentence's frames included; the same under bf16x3 (chunk 7), where the option must change the bits at every set;
* the slot pool: five slots, admissions at ticks 0, 5, 5 and 23 (an odd tick; three rows of one 4-row group at different frames), a slot retired and reused
  beside rows in mid-sentence (twice), one slot idle throughout; decoder mel and finished mel of every occupant against the sentence alone, zeros behind a
  row's frames and in the idle slot; fp32 and bf16x3 — at S and O the latter is the fp32 step and state layout under a set option;
* once, at S: a pool of 66 slots, all busy (Bp = 128, a second grid row of the wide step), ONE finish call listing all 66 rows from slot 65 down (two
  nat_pool_window_k launches, r0 = 0 and 48), then calls of exactly 48 and 49 rows, then the rest; every row against its sentence alone after every call
  (the eight rows around the tiles', the list's and the column blocks' edges are named in _nat_sessions.WIDE_ALONE; every other row is held to the same
  reference), rows a call does not list unchanged by it;
* forward_groups (group_row0 = [0, 2, 5] on descending and ascending frame counts, one-row groups) and forward_from_encoder (rows of encode() re-ordered, one
  dropped, L = 65 above the subset's 64 tokens; with and without groups) against the plain call; a group's rows read on a second stream after
  wait_group(g).  Boundaries with an EMPTY group ([0, 2, 2, 5], [0, 0, 5]) are what nat_validate() refuses ("every group needs at least one row"): the
  test holds the library to that — VTTS_ERR_INVALID, no groups to wait for afterwards, and the next call unharmed;
* the partitionable Threefry layout of both haiku mask entry points against oracle/nat_oracle.py and tests/_gta_oracle.py at B = 3, F = 17;
* once, at S: finish() wider than max_window (session and pool) and pool_admit() past Lmax or Fmax return VTTS_ERR_INVALID, leave mel and decoder mel as
  they were, and the next valid call gives the reference's bits.

Four faults a reviewer can plant in viettts_amd/csrc/nat.hip, and the test that fails — for the second, why none can (argued from the code; none of them
was run on a GPU here):

1. ``L.r0 = 0`` in pool_finish(): the second launch gathers list entries 48 .. 65 into compact rows 0 .. 17 over entries 0 .. 17, and both scatters read those
   rows, so slots 65 .. 48 receive the windows of slots 17 .. 0, whose sentence or window differs for every pair (asserted on the CPU), and rows 48 .. 65 of
   the compact copy are never written: test_wide_pool_list_split_and_second_column_block fails at its first finish call.
2. ``nat_pool_reset_k<true>`` chosen by ``h->x3`` instead of ``nat_dec_x3(c)``: NO test fails, here or anywhere, because nothing changes.  A slot's eight rows
   in two bf16 planes (nat_zxidx) are the very bytes of its four-row fp32 groups (nat_zidx) at every accepted width, and both instantiations store zeros
   (tests/test_nat_sessions_cpu.py::test_both_layouts_of_the_pools_reset_clear_the_same_bytes restates the two index maps and asserts it).  The combination
   itself — option set, fp32 step, a slot reused — runs in test_pool_equals_each_sentence_alone[S-bf16x3] and [O-bf16x3].  The choice that does show is the
   one beside it: ``dx3`` of nat_pool_ticks() taken from ``h->x3`` launches the split-state step where its 16-row steps do not divide among 8 waves: row blocks
   go missing from the sums, and those two cases fail at the first decoder mel they compare (a kernel outside what it is built for: do not run it).
3. ``C4`` computed from 80 instead of ``MEL``: the window kernels move 20 units per frame where a row has 1 (S), 21 (O) or 32 (W, X): every
   test_streamed_mel_* and test_pool_* case outside R fails at its first window (at S the copy also leaves the compact buffer: do not run it).
4. the POOL instantiations' dynamic-LDS attribute dropped from nat_pool_ticks(): at X the projection step asks for 65 536 bytes, above the 48 KiB a kernel
   gets without it, the launch is refused and pool_decode() returns VTTS_ERR_HIP: both test_pool_equals_each_sentence_alone[X-*] cases fail at their first
   decode.  It makes a launch fail: argue it from the code, do not run it.

One MI355X run of this module: 47 passed (14 streamed, 5 streamed bf16x3, 10 pool, 1 wide pool, 5 forward_groups, 5 forward_from_encoder, 5 mask
layout, 2 refusals) in 5 s, the slowest case 0.6 s (W in windows of one frame); tests/test_nat_sessions_cpu.py adds 8 on the CPU.  No equality failed, and
viettts_amd/csrc/nat.hip is unchanged:

  path                                          S        O        R        W        X
  streamed, fp32 (chunks)                    passed   passed   passed   passed   passed     (7, 50 | 7, 50 | 1, 7, 32, 50 | 1, 7, 32, 50 | 7, 50)
  streamed, bf16x3 (chunk 7; bits differ)    passed   passed   passed   passed   passed     (S, O: the fp32 step inside)
  pool, fp32                                 passed   passed   passed   passed   passed     (X: 64 KiB of dynamic LDS in the POOL step)
  pool, bf16x3                               passed   passed   passed   passed   passed     (S, O: fp32 state layout under a set option, a slot reused)
  66-slot pool, lists of 66 / 48 / 49 rows   passed      -        -        -        -
  forward_groups, wait_group                 passed   passed   passed   passed   passed     (an empty group: refused, as nat_validate() says)
  forward_from_encoder, +/- groups           passed   passed   passed   passed   passed
  partitionable masks, both entry points     passed   passed   passed   passed   passed
  refusals (session, pool)                   passed      -        -        -        -

No chunk had to be cut for time.
"""
from contextlib import contextmanager

import numpy as np
import pytest
import torch

import _gta_oracle as G
import _nat_dims as D
import _nat_sessions as N
from oracle import nat_oracle as O
from viettts_amd._lib import VttsError

pytestmark = pytest.mark.gpu
INVALID, STATE = -1, -2
RNG_KEY = (123456789, 42)
SETS = pytest.mark.parametrize("sid", D.GPU_ORDER)


@contextmanager
def _bf16x3(m, on=True):
    m.set_option("bf16x3", int(on))
    try:
        yield
    finally:
        m.set_option("bf16x3", 0)


@pytest.fixture(scope="module")
def models():
    """``models(sid)``: the width set's model, made at its first use and kept for the module."""
    from viettts_amd.nat.acoustic import AcousticModel

    assert torch.cuda.is_available()
    made = {}

    def get(sid):
        if sid not in made:
            made[sid] = AcousticModel(device="cuda:0", **D.dims(sid))
            made[sid].load_params(*D.checkpoint(sid))
        return made[sid]

    yield get
    for m in made.values():
        m.close()


@pytest.fixture(scope="module")
def refs(models):
    """The plain calls everything is compared with, computed once per (set, option) and never written to: ``refs.batch(sid, x3)`` = the ragged batch's mel
    ``[5, 129, mel]`` on the device; ``refs.alone(sid, L, F, x3)`` = (decoder mel, mel) of the sentence alone, ``[F, mel]`` each."""
    cache = {}

    class Refs:
        @staticmethod
        def batch(sid, x3=False):
            key = (sid, "batch", x3)
            if key not in cache:
                m = models(sid)
                with _bf16x3(m, x3):
                    cache[key] = m(*N.batch(sid), dropout_seeds=N.seeds(), to_host=False)
                for i, (_, F) in enumerate(N.STREAM_CASES):  # rows past a sentence's frames are zero in the reference itself
                    assert not bool(cache[key][i, F:].any()) and bool(torch.isfinite(cache[key][i, :F]).all())
            return cache[key]

        @staticmethod
        def alone(sid, L, F, x3=False):
            key = (sid, L, F, x3)
            if key not in cache:
                m = models(sid)
                c = D.case(sid, L, F)
                with _bf16x3(m, x3):
                    mel = m([c.tokens], [c.dur], [F], dropout_seeds=[N.seed(L, F)], to_host=False)[0]
                cache[key] = (N.mel0(m, m._ws, 1, L, F)[0].clone(), mel)
            return cache[key]

    return Refs


def _refused(status, fn, *a, **kw):
    with pytest.raises(VttsError) as e:
        fn(*a, **kw)
    assert e.value.status == status, e.value


# ------------------------------------------------------------ the streaming session ------------------------------------------------------------
@pytest.mark.parametrize("sid, chunk", [(sid, ch) for sid in D.GPU_ORDER for ch in N.CHUNKS[sid]])
def test_streamed_mel_equals_the_unstreamed_bit_for_bit(models, refs, sid, chunk):
    N.stream_in_windows(models(sid), N.batch(sid), N.seeds(), chunk, refs.batch(sid))


@SETS
def test_streamed_mel_bf16x3_equals_the_unstreamed_bf16x3(models, refs, sid):
    """At S and O the option runs the x3 gate GEMM and postnet around the fp32 step, at R, W and X the split-state step: it changes the bits at every set."""
    m = models(sid)
    assert not torch.equal(refs.batch(sid, True), refs.batch(sid))
    with _bf16x3(m):
        N.stream_in_windows(m, N.batch(sid), N.seeds(), 7, refs.batch(sid, True))


# ------------------------------------------------------------ the slot pool ------------------------------------------------------------
def _admit(pool, sid, slot, case):
    c = D.case(sid, *case)
    pool.admit(slot, c.tokens, c.dur, c.F, dropout_seed=N.seed(*case))


def _pool_mel0(m, pool):
    return N.mel0(m, pool._ws, pool.slots, pool.Lmax, pool.Fmax)


def _assert_rows(m, pool, alone, rows):
    """``rows``: {slot: (L, F)}.  The slot's decoder mel and mel are the sentence's own over its frames and zero behind them."""
    mel0 = _pool_mel0(m, pool)
    for slot, case in rows.items():
        r0, r = alone[case]
        F = case[1]
        assert torch.equal(mel0[slot, :F], r0), (slot, case, "decoder mel")
        assert torch.equal(pool.mel[slot, :F], r), (slot, case, "mel")
        assert not bool(mel0[slot, F:].any()) and not bool(pool.mel[slot, F:].any()), (slot, case)


@pytest.mark.parametrize("x3", [False, True], ids=["fp32", "bf16x3"])
@SETS
def test_pool_equals_each_sentence_alone(models, refs, sid, x3):
    m = models(sid)
    cases = N.STREAM_CASES + ((9, 17),)
    alone = {c: refs.alone(sid, *c, x3) for c in cases}  # before the pool opens: a call of the model ends it
    if x3:
        assert not torch.equal(alone[(64, 65)][1], refs.alone(sid, 64, 65)[1])
    with _bf16x3(m, x3), m.open_pool(5, N.LMAX, N.FMAX, 50) as pool:
        _admit(pool, sid, 0, (64, 65))
        N.decode_to(pool, 5)
        _admit(pool, sid, 1, (9, 33))
        _admit(pool, sid, 2, (2, 16))
        N.decode_to(pool, 23)
        assert [pool.cursor(s) for s in range(5)] == [23, 18, 16, 0, 0]
        pool.finish([(2, 0, 16)])
        first, first0 = pool.mel[2].clone(), _pool_mel0(m, pool)[2].clone()  # the first occupant's rows, read back before the slot goes
        pool.retire(2)
        _admit(pool, sid, 2, (9, 17))  # at an odd tick, its neighbours at frames 23 and 18
        _admit(pool, sid, 3, (65, 129))
        assert torch.equal(first[:16], alone[(2, 16)][1]) and torch.equal(first0[:16], alone[(2, 16)][0]) and not bool(first[16:].any()) and not bool(first0[16:].any())
        assert not bool(pool.mel[2].any()) and not bool(_pool_mel0(m, pool)[2].any())  # the slot's rows start from zero again
        N.decode_to(pool, 23 + 129)
        assert [pool.cursor(s) for s in range(5)] == [65, 33, 17, 129, 0]
        rows = {0: (64, 65), 1: (9, 33), 2: (9, 17), 3: (65, 129)}
        mel0 = _pool_mel0(m, pool)
        for slot, case in rows.items():
            assert torch.equal(mel0[slot, : case[1]], alone[case][0]), (slot, case)
        assert not bool(pool.mel.any())  # no window since the last admission
        N.finish_all(pool, 50)
        _assert_rows(m, pool, alone, rows)
        pool.retire(1)
        _admit(pool, sid, 1, (1, 1))  # a one-frame sentence beside finished rows, at tick 152
        pool.decode(1)
        pool.finish([(1, 0, 1)])
        rows[1] = (1, 1)
        _assert_rows(m, pool, alone, rows)
        assert not bool(pool.mel[4].any()) and not bool(_pool_mel0(m, pool)[4].any())  # the idle slot


def test_wide_pool_list_split_and_second_column_block(models, refs):
    sid = "S"
    m = models(sid)
    alone = {c: tuple(t.cpu().numpy() for t in refs.alone(sid, *c)) for c in N.WIDE_CASES}
    case = [N.wide_case(s) for s in range(N.WIDE_SLOTS)]
    n = [c[1] for c in case]
    with m.open_pool(N.WIDE_SLOTS, N.WIDE_LMAX, N.WIDE_FMAX, N.WIDE_MAX_WINDOW) as pool:
        for t in (0, 1, 4):
            N.decode_to(pool, t)
            for s in range(N.WIDE_SLOTS):
                if N.wide_admit_tick(s) == t:
                    _admit(pool, sid, s, case[s])
        N.decode_to(pool, 4 + N.WIDE_FMAX)
        assert all(pool.busy) and [pool.cursor(s) for s in range(N.WIDE_SLOTS)] == n
        mel0 = _pool_mel0(m, pool).cpu().numpy()
        for s in range(N.WIDE_SLOTS):
            assert np.array_equal(mel0[s, : n[s]], alone[case[s]][0]) and not mel0[s, n[s] :].any(), (s, "decoder mel")
        assert not bool(pool.mel.any())
        calls = N.wide_finish_calls()
        assert [len(c) for c in calls[:3]] == [66, 48, 49]
        before = pool.mel.cpu().numpy()
        for k, wins in enumerate(calls):
            pool.finish(wins)
            got = pool.mel.cpu().numpy()
            listed = {s for s, _, _ in wins}
            for s in range(N.WIDE_SLOTS):
                f = pool.finished[s]
                if s in listed:  # frames below the row's finished mark are final, the rest still zero
                    assert np.array_equal(got[s, :f], alone[case[s]][1][:f]) and not got[s, f:].any(), (k, s, f)
                else:
                    assert np.array_equal(got[s], before[s]), (k, s)
            before = got
        assert pool.finished == n
        for s in N.WIDE_ALONE:  # each with its sentence alone
            assert np.array_equal(before[s, : n[s]], alone[case[s]][1]) and not before[s, n[s] :].any(), s
        for s in range(N.WIDE_SLOTS):  # every row with the first row of the same sentence
            assert np.array_equal(before[s], before[case.index(case[s])]), s


# ------------------------------------------------------------ the grouped hand-over, the encoder run ahead ------------------------------------------------------------
@SETS
def test_forward_groups_equals_the_plain_call(models, sid):
    m = models(sid)
    side = torch.cuda.Stream()
    for order in ((4, 3, 2, 1, 0), (0, 1, 2, 3, 4)):  # descending frame counts (the groups finish one after another), and ascending
        cases = [N.STREAM_CASES[i] for i in order]
        args, sd = N.batch(sid, cases), N.seeds(cases)
        want = m(*args, dropout_seeds=sd, to_host=False)
        torch.cuda.synchronize()
        for r0 in ([0, 2, 5], [0, 1, 4, 5], [0, 5]):
            got = m(*args, dropout_seeds=sd, to_host=False, group_row0=r0)
            for g in range(len(r0) - 1):  # the group's rows, read on a second stream behind wait_group(g)
                m.wait_group(g, side)
                with torch.cuda.stream(side):
                    part = got[r0[g] : r0[g + 1]].clone()
                side.synchronize()
                assert torch.equal(part, want[r0[g] : r0[g + 1]]), (order, r0, g)
            torch.cuda.synchronize()
            assert torch.equal(got, want), (order, r0)
        for r0 in ([0, 2, 2, 5], [0, 0, 5]):  # an empty group: refused, nothing to wait for, and the handle carries on
            _refused(INVALID, m, *args, dropout_seeds=sd, to_host=False, group_row0=r0)
            _refused(STATE, m.wait_group, 0, side)
        assert torch.equal(m(*args, dropout_seeds=sd, to_host=False, group_row0=[0, 2, 5]), want)


@SETS
def test_forward_from_encoder_equals_the_plain_call(models, sid):
    m = models(sid)
    enc = m.encode(N.batch(sid)[0])
    assert enc.shape == (5, N.LMAX, 2 * D.dims(sid)["encoder_dim"])
    for pick, r0 in (((3, 0, 2, 1), [0, 1, 4]), ((4, 3, 2, 1, 0), [0, 2, 5])):  # the first drops the 65-token sentence: L = 65 above the subset's 64
        cases = [N.STREAM_CASES[i] for i in pick]
        args, sd = N.batch(sid, cases), N.seeds(cases)
        rows = enc.index_select(0, torch.tensor(pick, device=enc.device))
        want = m(*args, dropout_seeds=sd, to_host=False)
        got = m(*args, dropout_seeds=sd, to_host=False, encoded=rows)
        grouped = m(*args, dropout_seeds=sd, to_host=False, encoded=rows, group_row0=r0)
        torch.cuda.synchronize()
        assert rows.shape[1] == N.LMAX >= max(L for L, _ in cases) and torch.equal(got, want) and torch.equal(grouped, want), pick


# ------------------------------------------------------------ the partitionable mask layout ------------------------------------------------------------
@SETS
def test_partitionable_mask_layout(models, sid):
    m = models(sid)
    PN, H = D.dims(sid)["prenet_dim"], D.dims(sid)["decoder_dim"]
    hk = m.device_keep_masks_haiku(RNG_KEY, 3, 17, partitionable=True).cpu().numpy()
    want = O.haiku_prenet_keep_masks(np.array(RNG_KEY, dtype=np.uint32), 17, PN, partitionable=True)
    assert hk.shape == (3, 17, 2, PN) and hk.dtype == np.uint8 and all(np.array_equal(hk[b], want.astype(np.uint8)) for b in range(3))
    assert not np.array_equal(want, O.haiku_prenet_keep_masks(np.array(RNG_KEY, dtype=np.uint32), 17, PN))  # it IS another stream
    tk, tz = m.device_teacher_masks_haiku(RNG_KEY, 3, 17, partitionable=True)
    wk, wz = G.haiku_teacher_masks(RNG_KEY, 3, 17, PN, H, partitionable=True)
    assert tk.shape == (3, 17, 2, PN) and tz.shape == (3, 17, 4, H)
    assert np.array_equal(tk.cpu().numpy(), wk.astype(np.uint8)) and np.array_equal(tz.cpu().numpy(), wz.astype(np.uint8))
    ck, cz = G.haiku_teacher_masks(RNG_KEY, 3, 17, PN, H)
    assert not np.array_equal(wk, ck) and not np.array_equal(wz, cz)


# ------------------------------------------------------------ refusals, at S ------------------------------------------------------------
def test_a_session_refuses_a_window_wider_than_max_window(models, refs):
    m, ref = models("S"), refs.batch("S")
    with m.open_stream(*N.batch("S"), max_window=7, dropout_seeds=N.seeds()) as st:
        st.decode(N.FMAX)
        _refused(INVALID, st.finish, 0, 8)
        assert not bool(st.mel.any())  # nothing ran: the mel is what begin() made it
        st.finish(0, 7)
        assert torch.equal(st.mel[:, :7], ref[:, :7]) and not bool(st.mel[:, 7:].any())
        before = st.mel.clone()
        _refused(INVALID, st.finish, 7, 15)
        assert torch.equal(st.mel, before)
        st.finish(7, 14)
        assert torch.equal(st.mel[:, :14], ref[:, :14]) and not bool(st.mel[:, 14:].any())


def test_a_pool_refuses_wide_windows_and_sentences_past_its_limits(models, refs):
    sid = "S"
    m = models(sid)
    alone = {c: refs.alone(sid, *c) for c in ((9, 33), (2, 16))}
    long_, tall = D.case(sid, 30, 32), D.case(sid, 2, 16)
    with m.open_pool(4, N.WIDE_LMAX, N.WIDE_FMAX, 8) as pool:
        _admit(pool, sid, 0, (9, 33))
        pool.decode(33)
        pool.finish([(0, 0, 8)])
        mel, mel0 = pool.mel.clone(), _pool_mel0(m, pool).clone()
        _refused(INVALID, pool.finish, [(0, 8, 17)])  # 9 frames
        _refused(INVALID, pool.admit, 1, long_.tokens, long_.dur, long_.F, dropout_seed=1)  # 30 tokens in a pool of 9
        _refused(INVALID, pool.admit, 1, tall.tokens, tall.dur, N.WIDE_FMAX + 1, dropout_seed=1)  # 34 frames in a pool of 33
        assert pool.finished[0] == 8 and not pool.busy[1] and pool.tick == 33
        assert torch.equal(pool.mel, mel) and torch.equal(_pool_mel0(m, pool), mel0)  # nothing ran
        pool.finish([(0, 8, 16)])
        assert torch.equal(pool.mel[0, :16], alone[(9, 33)][1][:16]) and not bool(pool.mel[0, 16:].any())
        _admit(pool, sid, 1, (2, 16))
        pool.decode(16)
        N.finish_all(pool, 8)
        _assert_rows(m, pool, alone, {0: (9, 33), 1: (2, 16)})
