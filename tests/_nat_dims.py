"""Model widths, sentences and the bar of the NAT width tests (tests/test_nat_dims_cpu.py, tests/test_gpu_nat_dims.py): no fixtures, no GPU.

vtts_nat_acoustic_create() accepts encoder 64 / 128 / 192 / 256, decoder 256 / 512 / 768 / 1024, prenet in multiples of 32 with
2 * encoder + prenet <= 1024, mel 4 .. 128 and postnet 4 .. 1024 in multiples of 4; every other NAT test runs the reference's widths
(256, 512, 256, 80, 512) only.  The kernels are written against runtime widths, and the sets below put each piece of their edge arithmetic at a
value it does not take there.  :func:`geometry` restates that arithmetic from viettts_amd/csrc/nat.hip so that the CPU test can check that a set
still reaches what its line says.

Everything the GPU is compared with comes from here: the numpy oracles (oracle/nat_oracle.py, tests/_gta_oracle.py) in fp64, and the yardstick
``e32`` = the largest max |oracle fp32 - oracle fp64| over ALL cases of a width set for a quantity (a one-frame case alone has an e32 near 1e-8,
a bar no summation order can meet).  The bar is the rule of tests/test_gpu_gta.py::_bar,

    bar(want, e32, cap) = min(4 * e32 + 2^-22 * max |want|, cap).

Oracle results are computed once per (set, case, precision) and shared; callers must not write into them.
"""
from __future__ import annotations

import sys
from functools import lru_cache
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import _gta_oracle as G  # noqa: E402
from oracle import nat_oracle as O  # noqa: E402

# ---- width sets: synthetic_acoustic_checkpoint(seed, vocab_size, enc, dec, prenet, mel, post) -------------------------------------------------
WIDTHS = {
    # 2 iterations per wave in the encoder LSTM (< the prefetch depth 4); Cin = Cout = 4; 256 projection chunks; half a Threefry block; x3 falls back
    "S": (9101, 50, 64, 256, 32, 4, 4),
    # Cin = 84 (no multiple of 8 / 16 / 32); Cout = 36 (guard inside a lane half); 12 projection and 10 prenet chunks with idle threads; x3 falls back
    "O": (9102, 50, 128, 256, 96, 84, 36),
    # 6 iterations per wave; three 1024-column chunks in the mix; 32 m-blocks; MEL = 128; x3 split-state step at K = 896 and 1664
    "W": (9103, 50, 192, 768, 128, 128, 1024),
    # every create() limit at once; one prenet chunk; 64 KiB of dynamic LDS in the projection step; K = 1920 and 2944
    "X": (9104, 50, 64, 1024, 896, 128, 260),
    # the reference's widths (and the default checkpoint of the other NAT tests), for the sharper bar
    "R": (778, 256, 256, 512, 256, 80, 512),
}
GPU_ORDER = ("S", "O", "R", "W", "X")  # the smallest first
DURATION_WIDTHS = (64, 128, 192)  # 256 is tests/test_gpu_nat.py's
DURATION_LENGTHS = (1, 2, 9, 63, 64, 65, 256)

# (tokens L, frames F): around the convolution's 32 / 64-frame split, the mix's 16-frame tiles and its hand-over to the side stream at frame 64,
# and the 64-lane token loops' edges L = 63 / 64 / 65
CASES = ((1, 1), (2, 16), (9, 17), (30, 32), (9, 33), (63, 64), (64, 65), (65, 129))
LONG_CASES = ((800, 40), (2048, 40))  # S only: the mix's dynamic LDS beyond 48 KiB, and the documented limit
ORDER_CASES = ((9, 33), (64, 65), (65, 129))  # the CPU tests' subset

CAP = 5e-5          # encoder, teacher-forced and postnet quantities (tests/test_gpu_gta.py)
CAP_DURATION = 2e-6  # tests/test_gpu_nat.py


def cap_ar(want) -> float:
    """The autoregressive mel's existing bar (tests/test_gpu_nat.py), here the cap."""
    return 5e-4 * max(1.0, float(np.abs(want).max()))


def bar(want, e32: float, cap: float) -> float:
    return min(4.0 * float(e32) + 2.0 ** -22 * float(np.abs(want).max()), float(cap))


def dims(sid: str) -> dict:
    seed, V, enc, dec, prenet, mel, post = WIDTHS[sid]
    return dict(vocab_size=V, encoder_dim=enc, decoder_dim=dec, prenet_dim=prenet, mel_dim=mel, postnet_dim=post)


def x3_split_state(prenet: int, dec: int) -> bool:
    """nat_dec_frames' host condition for the option bf16x3: the split-state step where its 16-row steps divide the row blocks among 8 waves;
    otherwise the x3 gate GEMM and the x3 postnet run around the fp32 step."""
    return prenet % 16 == 0 and dec % 16 == 0 and ((prenet + dec) // 16) % 8 == 0 and ((prenet + 2 * dec) // 16) % 8 == 0


def geometry(sid: str) -> dict:
    """The kernels' index arithmetic at a width set, restated from viettts_amd/csrc/nat.hip."""
    _, _, enc, H, PN, MEL, PD = WIDTHS[sid]

    def waves(K):  # nat_dec_lstm_k / nat_tf_lstm_k: NIT = K / 8 iterations over KW = 8 waves, NWMAX each
        nit = K // 8
        return -(-nit // 8)

    def chunks(width, rows):  # nat_dec_proj_prenet_k: 1024 / width chunks of `per` rows (a multiple of 4); chunks that start at or past `rows` are empty
        n = 1024 // width
        per = (-(-rows // n) + 3) // 4 * 4
        return dict(chunks=n, per=per, idle_threads=1024 - n * width, live_chunks=-(-rows // per))

    return dict(
        enc_lstm_iters=waves(2 * enc), dec_lstm_iters=(waves(PN + H), waves(PN + 2 * H)), tf_lstm_iters=(waves(H), waves(2 * H)), prefetch_depth=4,
        proj=chunks(MEL, 2 * H), prenet1=chunks(PN, MEL), prenet2=chunks(PN, PN),
        proj_lds_bytes=(2 * H + 1024 + MEL + PN) * 16,
        mix_chunks=4 * H // 1024, gate_mblocks=4 * H // 32,
        postnet_steps=(-(-MEL // 32), -(-PD // 32)), postnet_mblocks=(-(-PD // 32), -(-MEL // 32)),
        threefry_blocks=PN / 64.0, x3_split_state=x3_split_state(PN, H),
    )


def mix_lds_bytes(Lmax: int) -> int:
    """nat_gates_mix_k's dynamic LDS: the tokens' midpoints and 16 frames' upsampling weights per token."""
    return ((Lmax + 3) // 4 * 4 + Lmax * 16) * 4


@lru_cache(maxsize=None)
def checkpoint(sid: str):
    from viettts_amd.nat.synth import synthetic_acoustic_checkpoint

    return synthetic_acoustic_checkpoint(*WIDTHS[sid])


@lru_cache(maxsize=None)
def duration_checkpoint(dim: int):
    from viettts_amd.nat.synth import synthetic_duration_checkpoint

    return synthetic_duration_checkpoint(9200 + dim, 50, dim)


@lru_cache(maxsize=None)
def duration_sentence(dim: int, L: int):
    return np.random.default_rng(9300 + 7 * dim + L).integers(0, 50, size=L)


@lru_cache(maxsize=None)
def duration_oracle(dim: int, L: int, fp64: bool):
    P, S = duration_checkpoint(dim)
    return O.duration_model(P, S, duration_sentence(dim, L), dtype=np.float64 if fp64 else np.float32)


@lru_cache(maxsize=None)
def duration_e32(dim: int) -> float:
    return max(float(np.abs(duration_oracle(dim, L, False).astype(np.float64) - duration_oracle(dim, L, True)).max()) for L in DURATION_LENGTHS)


class Case:
    """One sentence of a width set: tokens, durations in frames (scaled to sum to about F, one word-end token of duration 0 as text2mel's rules
    produce), F frames, and for the teacher-forced pass target mels and explicit masks (keep at P = 0.5, zoneout at P = 0.1)."""

    def __init__(self, sid: str, L: int, F: int):
        _, V, _, H, PN, MEL, _ = WIDTHS[sid]
        rng = np.random.default_rng(1000 * L + F + 17 * sum(map(ord, sid)))
        self.sid, self.L, self.F = sid, L, F
        self.tokens = rng.integers(0, V, size=L)
        dur = np.abs(rng.normal(3.0, 1.5, size=L)) + 0.05
        if L > 1:
            dur[rng.integers(0, L)] = 0.0
        self.dur = (dur * (F / dur.sum())).astype(np.float32)
        self.mels = rng.normal(-1.0, 2.0, size=(F, MEL)).astype(np.float32)
        self.keep = rng.random((F, 2, PN)) < 0.5
        self.zone = rng.random((F, 4, H)) < 0.1


@lru_cache(maxsize=None)
def case(sid: str, L: int, F: int) -> Case:
    return Case(sid, L, F)


def _dt(fp64: bool):
    return np.float64 if fp64 else np.float32


def oracle_encoder(sid: str, L: int, F: int, fp64: bool = True):
    return _oracle_encoder(sid, L, F, bool(fp64))


def oracle_teacher(sid: str, L: int, F: int, fp64: bool = True):
    """(pre, mel) of the teacher-forced pass with the case's masks."""
    return _oracle_teacher(sid, L, F, bool(fp64))


def oracle_ar(sid: str, L: int, F: int, fp64: bool = True, seed=None):
    """The autoregressive mel: without dropout, or with the library's own Threefry stream of ``seed``."""
    return _oracle_ar(sid, L, F, bool(fp64), seed)


@lru_cache(maxsize=None)
def _oracle_encoder(sid, L, F, fp64):
    P, S = checkpoint(sid)
    c = case(sid, L, F)
    return O.token_encoder(O.Params(P, S, _dt(fp64)), f"{G.PRE}/~/token_encoder", c.tokens.astype(np.int64), L)


@lru_cache(maxsize=None)
def _oracle_teacher(sid, L, F, fp64):
    P, S = checkpoint(sid)
    c = case(sid, L, F)
    return G.teacher_forced_row(P, S, c.tokens, L, c.dur, c.mels, c.keep, c.zone, _dt(fp64))


def masks_fn(masks):
    return None if masks is None else (lambda f: (masks[f, 0], masks[f, 1]))


@lru_cache(maxsize=None)
def _oracle_ar(sid, L, F, fp64, seed):
    P, S = checkpoint(sid)
    c = case(sid, L, F)
    masks = None if seed is None else O.threefry_keep_masks(int(seed), F, WIDTHS[sid][4])
    return O.acoustic_inference(P, S, c.tokens, c.dur, F, prenet_masks=masks_fn(masks), dtype=_dt(fp64))


def _gap(a32, a64) -> float:
    return float(np.abs(np.asarray(a32, dtype=np.float64) - a64).max())


def e32(sid: str, quantity: str, cases=CASES) -> float:
    """max over `cases` of max |oracle fp32 - oracle fp64| for "enc", "pre" / "mel" (teacher-forced) or "ar"."""
    return _e32(sid, quantity, tuple(cases))


@lru_cache(maxsize=None)
def _e32(sid, quantity, cases):
    worst = 0.0
    for L, F in cases:
        if quantity == "enc":
            g = _gap(oracle_encoder(sid, L, F, False), oracle_encoder(sid, L, F, True))
        elif quantity in ("pre", "mel"):
            i = 0 if quantity == "pre" else 1
            g = _gap(oracle_teacher(sid, L, F, False)[i], oracle_teacher(sid, L, F, True)[i])
        elif quantity == "ar":
            g = _gap(oracle_ar(sid, L, F, False), oracle_ar(sid, L, F, True))
        else:
            raise KeyError(quantity)
        worst = max(worst, g)
    return worst


def e32_ar_seeded(sid: str, seeded_cases) -> float:
    """The same for the autoregressive mel under dropout: ``seeded_cases`` = ((L, F, seed), ...)."""
    return max(_gap(oracle_ar(sid, L, F, False, sd), oracle_ar(sid, L, F, True, sd)) for L, F, sd in seeded_cases)


def postnet(sid: str, pre: np.ndarray, fp64: bool = True) -> np.ndarray:
    """The postnet's residual (mel - pre) of a given decoder mel ``pre [F, mel]``."""
    P, S = checkpoint(sid)
    return G._postnet(O.Params(P, S, _dt(fp64)), np.asarray(pre).astype(_dt(fp64)))


def report(tag: str, got, want, e: float, cap: float):
    """Prints err, e32, bar and their ratio; returns (err, bar).  The caller asserts."""
    err = float(np.abs(np.asarray(got, dtype=np.float64) - want).max())
    b = bar(want, e, cap)
    print(f"[nat dims] {tag}: err {err:.3e}  e32 {e:.3e}  bar {b:.3e}  err/bar {err / b:.3f}  (max |want| {float(np.abs(want).max()):.3f})")
    return err, b
