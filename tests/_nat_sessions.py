"""Sentences, drivers and geometry of the NAT decoder's streamed, pooled and grouped entry points at every model width
(tests/test_nat_sessions_cpu.py, tests/test_gpu_nat_sessions.py): no fixtures, and nothing here needs a GPU to import.

The sentences are tests/_nat_dims.py's (``case(sid, L, F)`` and its checkpoints).  The drivers take the model, so they work at any width; the
reference-width tests (tests/test_gpu_stream.py, tests/test_gpu_pool.py) import them from here.  :func:`geometry` restates from
viettts_amd/csrc/nat.hip the arithmetic the tests rely on, so that the CPU test can check that the chosen cases still reach what they are there for.
"""
from __future__ import annotations

import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
import _nat_dims as D  # noqa: E402

# ---- the sentences ---------------------------------------------------------------------------------------------------------------------------
# (tokens L, frames F).  One ragged batch: rows that end before a window (1 frame), inside one (16, 33), inside a right halo (65 of chunk 32: the
# window [32, 64) reads up to frame 74) and a 129-frame row that crosses frame 64 inside a decode call.
STREAM_CASES = ((1, 1), (2, 16), (9, 33), (64, 65), (65, 129))
LMAX, FMAX = max(L for L, _ in STREAM_CASES), max(F for _, F in STREAM_CASES)
# chunks per width set: all four where the issue asks for them (R: the reference's widths; W: the FOLD postnet), 7 and 50 elsewhere
CHUNKS = {"S": (7, 50), "O": (7, 50), "R": (1, 7, 32, 50), "W": (1, 7, 32, 50), "X": (7, 50)}
HALO = 10  # VTTS_NAT_POSTNET_HALO: the postnet's five K = 5 convolutions
POOL_LIST = 48  # NAT_POOL_LIST: rows per launch of nat_pool_window_k


def seed(L: int, F: int) -> int:
    """A sentence's dropout seed: its own wherever it runs, so that a row can be compared with the sentence alone."""
    return 5000 + 10 * L + F


def batch(sid: str, cases=STREAM_CASES):
    """(tokens, durations, frame counts) of ``cases`` at a width set, as AcousticModel.__call__ takes them."""
    cs = [D.case(sid, L, F) for L, F in cases]
    return [c.tokens for c in cs], [c.dur for c in cs], [c.F for c in cs]


def seeds(cases=STREAM_CASES):
    return [seed(L, F) for L, F in cases]


# ---- the drivers -----------------------------------------------------------------------------------------------------------------------------
def stream_in_windows(am, rows, row_seeds, chunk, ref):
    """``rows`` = (tokens, durations, frame counts).  Windows of ``chunk`` frames, the decoder 10 frames ahead of each: after every window the
    mel's frames below its end are final."""
    import torch

    Fmax = max(rows[2])
    with am.open_stream(*rows, max_window=chunk, dropout_seeds=row_seeds) as st:
        assert st.mel.shape == ref.shape and not am.resident_used
        for f0 in range(0, Fmax, chunk):
            f1 = min(Fmax, f0 + chunk)
            st.decode(f1 + 10)
            assert st.frames_decoded == min(f1 + 10, Fmax)
            st.finish(f0, f1)
            assert torch.equal(st.mel[:, :f1], ref[:, :f1]), (chunk, f0, f1)
        assert torch.equal(st.mel, ref), chunk


def mel0(model, ws, B, Lmax, Fmax):
    """The decoder's mel before the postnet, ``[B, Fmax, mel_dim]``: the sixth buffer of the workspace layout both the un-pooled call and the pool
    use (viettts_amd/csrc/nat.hip: NatAcousticWs — encoder ping-pong x 2, encoder output, both layers' per-token gates, then mel0; 256-byte blocks)."""
    import torch

    al = lambda n: (n + 255) // 256 * 256
    cfg = model.cfg
    bld, g = B * Lmax * cfg.encoder_dim * 4, 4 * cfg.decoder_dim
    off = 2 * al(bld) + al(2 * bld) + 2 * al(B * Lmax * g * 4)
    return ws[off : off + B * Fmax * cfg.mel_dim * 4].view(torch.float32).view(B, Fmax, cfg.mel_dim)


def decode_to(pool, tick):
    """Up to ``tick`` in calls of 32, 7 and 1 ticks, the largest that fits first."""
    while pool.tick < tick:
        pool.decode(next(k for k in (32, 7, 1) if pool.tick + k <= tick))


def finish_all(pool, width):
    """Every busy row's remaining frames in windows of ``width``, all rows of a round in one call."""
    while True:
        wins = [(s, pool.finished[s], min(pool.finished[s] + width, pool.n_frames[s])) for s in range(pool.slots) if pool.busy[s] and pool.finished[s] < pool.n_frames[s]]
        if not wins:
            return
        pool.finish(wins)


# ---- the wide pool: the list split of pool_finish() and the wide step's second column block ---------------------------------------------------
WIDE_SLOTS, WIDE_MAX_WINDOW = 66, 8
WIDE_CASES = ((1, 1), (2, 16), (9, 17), (9, 33))
WIDE_LMAX, WIDE_FMAX = 9, 33
WIDE_ALONE = (0, 31, 32, 47, 48, 63, 64, 65)  # around the 32-sentence tiles, the list's split at 48 and the second 64-column block


def wide_case(slot: int):
    """The slot's sentence.  Neither this nor the first window's width has period 48: list entries j and j + 48 must not agree."""
    return WIDE_CASES[(slot + slot // 8) % 4]


def wide_admit_tick(slot: int) -> int:
    return (0, 1, 4)[slot % 3]


def wide_finish_calls():
    """The pool_finish() calls of the wide pool, ``[(slot, f0, f1), ...]`` each, every row decoded to its end beforehand:

    1. all 66 rows in ONE call, listed from slot 65 down (list entry j is slot 65 - j: the compact row is never the slot), first windows of width 1, 8
       or 3 — one-frame rows with 8 or 3 are cut at the row's last frame;
    2. exactly 48 of the unfinished rows, windows of 1, 2 or 4 frames in mid-row (none of them finishes a row);
    3. exactly 49 of the unfinished rows, windows of 8 frames (a 16-frame row ends inside its window);
    4. and on: every unfinished row, 8 frames each, until none is left."""
    n = [wide_case(s)[1] for s in range(WIDE_SLOTS)]
    done = [0] * WIDE_SLOTS
    calls = []

    def call(slots, width):
        wins = [(s, done[s], done[s] + width(s)) for s in slots]
        for s, _, f1 in wins:
            done[s] = min(f1, n[s])
        calls.append(wins)

    pending = lambda: [s for s in range(WIDE_SLOTS) if done[s] < n[s]]
    call(list(reversed(range(WIDE_SLOTS))), lambda s: (1, 8, 3)[(s + s // 7) % 3])
    call(pending()[:48], lambda s: (1, 2, 4)[s % 3])
    call(pending()[-49:], lambda s: WIDE_MAX_WINDOW)
    while pending():
        call(pending(), lambda s: WIDE_MAX_WINDOW)
    return calls


# ---- the arithmetic of viettts_amd/csrc/nat.hip the tests rely on -------------------------------------------------------------------------------
def reset_bytes(sid: str, slots: int, slot: int, x3: bool) -> set:
    """The bytes of ONE state parity ([p | h1 | h2], ZW = prenet + 2 * decoder rows of Bp columns) that nat_pool_reset_k<X3> clears for a slot: the fp32
    layout keeps four rows of a column together (nat_zidx), the split-state layout eight rows in each of two bf16 planes ZW * Bp elements apart (nat_zxidx)."""
    _, _, _, H, PN, _, _ = D.WIDTHS[sid]
    ZW, Bp = PN + 2 * H, (slots + 63) // 64 * 64
    out = set()
    for row in range(ZW):
        if x3:
            for plane in (0, ZW * Bp):
                o = 2 * (plane + ((row >> 3) * Bp + slot) * 8 + (row & 7))
                out |= {o, o + 1}
        else:
            o = 4 * (((row >> 2) * Bp + slot) * 4 + (row & 3))
            out |= {o, o + 1, o + 2, o + 3}
    return out



def geometry(sid: str, max_window: int, slots: int, listed: int, Fmax: int = FMAX) -> dict:
    """A session or pool of ``slots`` rows of at most ``Fmax`` frames at a width set, opened for windows of ``max_window`` frames, and one finish call that
    lists ``listed`` rows:

    * ``W``: the compact window's pitch, NatStreamWs: roundup64(min(max_window, Fmax) + a halo per side);
    * ``C4``: nat_window_k's and nat_pool_window_k's units per mel row, MEL / 4 float4;
    * ``list_r0``: L.r0 of every nat_pool_window_k launch of pool_finish() (NAT_POOL_LIST rows each); ``list_launches`` their number;
    * ``Bp``, ``lgrid_y``: the state's column count and the step kernels' second grid dimension (nat_pool_ticks: wide ? Bp / 64 : 1, wide = more than 32 rows);
    * ``proj_lds_bytes``: nat_dec_proj_prenet_k's dynamic LDS, for which nat_pool_ticks raises the POOL instantiations' attribute above 48 KiB;
    * ``x3_split_state``: nat_dec_x3() under the option bf16x3 — the split-state step and nat_pool_reset_k<true>; otherwise the fp32 step and state layout."""
    _, _, _, H, PN, MEL, _ = D.WIDTHS[sid]
    r0 = tuple(range(0, listed, POOL_LIST))
    Bp = (slots + 63) // 64 * 64
    return dict(
        W=(min(max_window, Fmax) + 2 * HALO + 63) // 64 * 64, C4=MEL // 4, list_launches=len(r0), list_r0=r0, Bp=Bp, lgrid_y=Bp // 64 if slots > 32 else 1,
        proj_lds_bytes=(2 * H + 1024 + MEL + PN) * 16, x3_split_state=D.x3_split_state(PN, H),
    )
