"""Batches that cross a stage's rows-per-launch split (plain numpy; tests/test_row_split_cpu.py checks them, the tests/test_gpu_*.py run them).

Every batched stage passes its per-row lengths to the kernel as launch arguments, ``P`` rows per launch, and a host loop re-bases every
pointer for the launches after the first.  ``split_batch`` lays out ``P + k`` rows so that a second launch that forgot its row offset on
ANY of them computes something else than the oracle says:

* for every ``b < k`` row ``P + b`` differs from row ``b`` in content, in length and (where the stage takes one) in its per-row scalar: a
  dropped input, lengths or gains offset changes the expected value of row ``P + b`` (tests/test_row_split_cpu.py shows by how much);
* the rows behind the split hold the batch's longest row, strictly, and a row of the stage's minimum length: the per-call maxima are set by
  the second launch, and the first launch's grid is larger than any of its rows needs;
* the rows between are drawn in turn from a handful of distinct (content, length, scalar) triples, so that an oracle is evaluated once per
  distinct row (``per_kind``) and the CPU side of a test stays at seconds.

A dropped OUTPUT offset (or that of a WORKSPACE slice someone reads after the launch) needs no special batch: the second launch then writes
over rows of the first and leaves its own untouched, which the NaN / sentinel pre-fill of every GPU test's outputs shows (and the
overwritten rows fail against the oracle).

The content of a row runs over the whole stride, past the row's own length: "row P + b cut or extended to lengths[b]" is then a plain
slice, and a kernel that reads with another row's length reads signal, not zeros.
"""
from typing import Callable, List, NamedTuple, Optional, Sequence

import numpy as np


class Row(NamedTuple):
    content: np.ndarray  # [S, ...] the row over the whole stride
    length: int
    scalar: Optional[float] = None


class Batch(NamedTuple):
    rows: np.ndarray  # [N, S, ...]
    lengths: List[int]
    scalars: Optional[np.ndarray]  # [N] float32, or None
    kind: np.ndarray  # [N] which distinct Row each row is
    kinds: List[Row]
    P: int
    k: int

    @property
    def N(self) -> int:
        return self.P + self.k

    def behind(self):
        return range(self.P, self.P + self.k)


def split_batch(P: int, front: Sequence[Row], behind: Sequence[Row], fill: Sequence[Row], min_length: int, last_fill: Optional[int] = None, length_cap: Optional[int] = None) -> Batch:
    """Rows 0 .. k - 1 are ``front``, rows P .. P + k - 1 ``behind``, the rows between ``fill`` in turn (row P - 1: ``fill[last_fill]`` if given)."""
    k = len(front)
    assert k == len(behind) >= 1 and P > k and 1 <= len(fill) <= 8
    kinds = list(front) + list(fill) + list(behind)
    S = kinds[0].content.shape[0]
    assert all(r.content.shape == kinds[0].content.shape and 0 <= r.length <= (length_cap or S) for r in kinds)
    kind = np.empty(P + k, np.int64)
    kind[:k] = np.arange(k)
    kind[k:P] = k + np.arange(P - k) % len(fill)
    if last_fill is not None:
        kind[P - 1] = k + last_fill
    kind[P:] = k + len(fill) + np.arange(k)
    for f, b in zip(front, behind):
        assert f.length != b.length and not np.array_equal(f.content, b.content) and (f.scalar is None or f.scalar != b.scalar)
    assert max(r.length for r in behind) > max(r.length for r in list(front) + list(fill))
    assert min(r.length for r in behind) == min_length <= min(r.length for r in kinds)
    rows = np.stack([kinds[i].content for i in kind])
    rows.setflags(write=False)
    scalars = None if kinds[0].scalar is None else np.array([kinds[i].scalar for i in kind], np.float32)
    return Batch(rows, [int(kinds[i].length) for i in kind], scalars, kind, kinds, P, k)


def per_kind(batch: Batch, fn: Callable[[Row], object]) -> list:
    """``fn`` of every row of the batch, evaluated once per distinct row."""
    memo = [fn(r) for r in batch.kinds]
    return [memo[i] for i in batch.kind]


# ---------------------------------------------------------------- signals ----------------------------------------------------------------
def speechlike(seed: int, S: int, rate: int = 16000, peak: float = 0.2) -> np.ndarray:
    """float32: 29 harmonics of a random F0 under a 3 Hz envelope, plus a N(0, 0.003^2) floor (no band near a log floor, no exact zeros)."""
    rng = np.random.default_rng(seed)
    t = np.arange(S) / float(rate)
    f0 = rng.uniform(90.0, 250.0)
    x = sum(np.sin(2 * np.pi * f0 * h * t + rng.uniform(0, 2 * np.pi)) / h for h in range(1, 30))
    x *= 0.55 + 0.45 * np.sin(2 * np.pi * 3.0 * t + rng.uniform(0, 2 * np.pi))
    return (peak * x / np.abs(x).max() + rng.normal(0.0, 0.003, size=S)).astype(np.float32)


def to_pcm16(y: np.ndarray) -> np.ndarray:
    return np.round(np.asarray(y, np.float64) * 32767.0).astype(np.int16)


def _wave_rows(seed: int, S: int, lengths, pcm: bool, scalars=None, peaks=None, rate: int = 16000) -> List[Row]:
    out = []
    for i, n in enumerate(lengths):
        y = speechlike(seed + i, S, rate, 0.2 if peaks is None else peaks[i])
        out.append(Row(to_pcm16(y) if pcm else y, int(n), None if scalars is None else float(scalars[i])))
    return out


# ---------------------------------------------------------------- the stages ----------------------------------------------------------------
FRAME_STRIDE = 3848  # samples: a multiple of 8 (the 16-byte loads hold for both dtypes), 15 frames of 256 and a few samples
FRAME_FRONT, FRAME_BEHIND, FRAME_FILL = (1300, 2049, 777), (385, 3841, 2560), (1025, 3000, 513, 2303)


def frames_batch(P: int, pcm: bool) -> Batch:
    """MelFilter and PitchTracker (hop 256, 8 frames per workgroup, at least 385 samples): rows of 1 to 15 frames, under two workgroups."""
    front, behind, fill = (_wave_rows(s, FRAME_STRIDE, n, pcm) for s, n in ((100, FRAME_FRONT), (200, FRAME_BEHIND), (300, FRAME_FILL)))
    return split_batch(P, front, behind, fill, min_length=385)


def audio_batch(P: int) -> Batch:
    """Resampler: rows of a few hundred samples (16 -> 24 kHz: under one workgroup's 1024 outputs but the longest, 1.5 * 700), an empty row and
    a one-sample row."""
    front, behind, fill = (_wave_rows(s, 704, n, False) for s, n in ((400, (300, 451, 123)), (500, (257, 700, 0)), (600, (200, 333, 1, 512))))
    return split_batch(P, front, behind, fill, min_length=0)


def loudness_batch(P: int) -> Batch:
    """LoudnessMeter at 16 kHz (blocks of 6400 samples every 1600, segments of 8192): rows of one to three blocks at levels of their own (the
    normalize gain is the stage's per-row scalar, and comes from the level), the longest of two segments.  Row P is too short for a block,
    row P - 1 (a fill row) is not empty: the packed offset of row P is the running sum over the whole first launch."""
    S = 11200
    front = _wave_rows(700, S, (6437, 8100, 9000), False, peaks=(0.2, 0.05, 0.4))
    behind = _wave_rows(800, S, (3000, 11111, 0), False, peaks=(0.1, 0.3, 0.15))
    fill = _wave_rows(900, S, (7000, 9601, 6400, 8500), False, peaks=(0.25, 0.08, 0.5, 0.12))
    assert 0 < behind[0].length < 6400 and behind[1].length // 1600 - 3 == 3 and behind[1].length > 8192
    return split_batch(P, front, behind, fill, min_length=0)


def limiter_batch(P: int) -> Batch:
    """TruePeakLimiter and its stream (look-ahead 80 samples at 16 kHz): rows of 1 to 463 samples, peak 0.5, each with a pre-gain of its own
    between 2 and 6: every row but the one-sample one is pushed over the -1 dBTP ceiling, so its gain reduction depends on its gain."""
    front = _wave_rows(1000, 470, (300, 337, 374), False, scalars=(4.0, 3.0, 5.0), peaks=(0.5,) * 3)
    behind = _wave_rows(1100, 470, (211, 463, 1), False, scalars=(2.5, 6.0, 3.5), peaks=(0.5,) * 3)
    fill = _wave_rows(1200, 470, (64, 150, 250, 390), False, scalars=(4.0, 2.0, 5.5, 3.0), peaks=(0.5,) * 4)
    return split_batch(P, front, behind, fill, min_length=1)


def stoi_batch(P: int) -> Batch:
    """StoiMeter (frames of 256 every 128, segments of 30 frames): ``content`` is [S, 2], the clean and the processed signal of
    tests/_stoi_oracle.py.  Lengths around the 4096 / 4097 edge: rows without a segment, with one, and with a few; an empty row."""
    import _stoi_oracle as O

    def rows(seed, lengths, levels):
        out = []
        for i, (n, level) in enumerate(zip(lengths, levels)):
            x = O.make_speechlike(4488, seed + i)
            out.append(Row(np.stack([x, O.degrade(x, seed + i, level)], axis=1), n))
        return out

    front, behind = rows(40, (4097, 4300, 3000), (0.5, 0.3, 1.0)), rows(50, (4096, 4481, 0), (0.4, 0.8, 0.5))
    return split_batch(P, front, behind, rows(60, (4225, 2000, 4224, 4400), (0.6, 0.5, 0.2, 0.9)), min_length=0)


DTW_NARROW_BAND = 1  # the narrow band the split test adds to the default (none): it changes totals below, and every pair keeps a path inside it


def dtw_batch(P: int, D: int = 8) -> Batch:
    """DTW pairs: ``content`` is [Ta + Tb, D] (a's Ta = 44 frames, then b's), ``length`` is la * 64 + lb.  Behind the split: the longest a with
    the longest b, a 1 x n and an n x 1 pair."""
    Ta = Tb = 44

    def pair(seed, la, lb):
        return Row(np.random.RandomState(seed).standard_normal((Ta + Tb, D)).astype(np.float32), la * 64 + lb)

    front = [pair(1, 17, 23), pair(2, 30, 9), pair(3, 5, 33)]
    behind = [pair(11, 1, 37), pair(12, 41, 40), pair(13, 29, 1)]
    fill = [pair(21, 12, 12), pair(22, 33, 20), pair(23, 2, 35), pair(24, 25, 31)]
    for f, b in zip(front, behind):  # both lengths differ, and so do a and b each
        assert f.length // 64 != b.length // 64 and f.length % 64 != b.length % 64
        assert not np.array_equal(f.content[:Ta], b.content[:Ta]) and not np.array_equal(f.content[Ta:], b.content[Ta:])
    assert max(r.length % 64 for r in behind) > max(r.length % 64 for r in front + fill)  # lb_max as well as la_max
    return split_batch(P, front, behind, fill, min_length=1 * 64 + 37, length_cap=64 * Ta + Tb)


def dtw_pairs(batch: Batch):
    """(a [N, Ta, D], b [N, Tb, D], la, lb) of a ``dtw_batch``."""
    Ta = batch.rows.shape[1] // 2
    return batch.rows[:, :Ta], batch.rows[:, Ta:], [n // 64 for n in batch.lengths], [n % 64 for n in batch.lengths]
