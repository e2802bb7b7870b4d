"""include/vtts_dtw.h restated in numpy float32, operation for operation: what the GPU results are compared against with ``==``.

``dtw_f32`` is the contract (cost chain, recurrence with the tie rule, band, backtrace -> total, path_len, span), vectorised along
anti-diagonals so that a 513 x 513 pair takes a fraction of a second; ``dtw_f32_cells`` is the same thing cell by cell (the two are
checked against each other); ``dtw_f64`` is a float64 DP with float64 costs; ``brute_force`` enumerates every monotone path.
"""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np

HEADER = Path(__file__).resolve().parents[1] / "include" / "vtts_dtw.h"
DIAG, UP, LEFT = 0, 1, 2
CONTRACT_ORDER = (DIAG, UP, LEFT)


def header_constants() -> dict:
    """Every ``#define VTTS_DTW_* <integer>`` of the header."""
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+(VTTS_DTW_\w+)\s+(\d+)\s*$", HEADER.read_text(), re.M)}


def local_cost(a: np.ndarray, b: np.ndarray, dtype=np.float32) -> np.ndarray:
    """c[i, j]: one chain in ascending d, s = s + |a[i, d] - b[j, d]|, every operation rounded to ``dtype``."""
    a = np.asarray(a, dtype=dtype)
    b = np.asarray(b, dtype=dtype)
    s = np.zeros((a.shape[0], b.shape[0]), dtype=dtype)
    for d in range(a.shape[1]):
        s = s + np.abs(a[:, None, d] - b[None, :, d])
    return s


def in_band(i, j, la: int, lb: int, r: int):
    """The band predicate, in Python / int64 integers."""
    if r == 0:
        return np.ones(np.broadcast(i, j).shape, dtype=bool) if isinstance(i, np.ndarray) or isinstance(j, np.ndarray) else True
    i = np.asarray(i, dtype=np.int64)
    j = np.asarray(j, dtype=np.int64)
    return np.abs(i * (lb - 1) - j * (la - 1)) <= r * max(la - 1, lb - 1)


def _select(cands, order, dtype):
    """min over the candidates tried in ``order``; a later one replaces an earlier one only if strictly smaller."""
    best = cands[order[0]].copy()
    code = np.full(best.shape, order[0], dtype=np.uint8)
    for k in order[1:]:
        better = cands[k] < best
        best = np.where(better, cands[k], best).astype(dtype)
        code = np.where(better, np.uint8(k), code)
    return best, code


def accumulate(c: np.ndarray, band: int = 0, order=CONTRACT_ORDER):
    """D and the move codes from a cost matrix, anti-diagonal by anti-diagonal, in c's dtype."""
    dtype = c.dtype.type
    la, lb = c.shape
    inf = dtype(np.inf)
    D = np.full((la + 1, lb + 1), inf, dtype=c.dtype)  # D[i + 1, j + 1]; row 0 and column 0 are the +inf outside
    codes = np.zeros((la, lb), dtype=np.uint8)
    for s in range(la + lb - 1):
        i = np.arange(max(0, s - lb + 1), min(la - 1, s) + 1)
        j = s - i
        ok = in_band(i, j, la, lb, band)
        i, j = i[ok], j[ok]
        if i.size == 0:
            continue
        best, code = _select({DIAG: D[i, j], UP: D[i, j + 1], LEFT: D[i + 1, j]}, order, dtype)
        val = (c[i, j] + best).astype(c.dtype)
        if s == 0:
            val, code = c[:1, 0].copy(), np.zeros(1, dtype=np.uint8)
        D[i + 1, j + 1] = val
        codes[i, j] = code
    return D[1:, 1:], codes


def backtrace(codes: np.ndarray):
    """Follow the codes from the corner, clamped as the contract says: path_len and span[la, 2]."""
    la, lb = codes.shape
    span = np.full((la, 2), -1, dtype=np.int32)
    i, j, n = la - 1, lb - 1, 1
    span[i, 1] = j
    while (i, j) != (0, 0):
        code = LEFT if i == 0 else UP if j == 0 else int(codes[i, j])
        if code == LEFT:
            j -= 1
        else:
            span[i, 0] = j
            i -= 1
            if code == DIAG:
                j -= 1
            span[i, 1] = j
        n += 1
    span[0, 0] = 0
    return n, span


def dtw_f32(a, b, band: int = 0, order=CONTRACT_ORDER):
    """(total float32, path_len int, span int32 [la, 2]) of the contract."""
    D, codes = accumulate(local_cost(a, b, np.float32), band, order)
    n, span = backtrace(codes)
    return D[-1, -1], n, span


def dtw_f32_cells(a, b, band: int = 0):
    """The contract cell by cell, as the header words it (small sizes: a Python loop per cell)."""
    c = local_cost(a, b, np.float32)
    la, lb = c.shape
    inf = np.float32(np.inf)
    D = np.full((la, lb), inf, dtype=np.float32)
    codes = np.zeros((la, lb), dtype=np.uint8)
    for i in range(la):
        for j in range(lb):
            if not bool(in_band(i, j, la, lb, band)):
                continue
            if i == 0 and j == 0:
                D[0, 0] = c[0, 0]
                continue
            best, code = (D[i - 1, j - 1] if i and j else inf), DIAG
            up = D[i - 1, j] if i else inf
            left = D[i, j - 1] if j else inf
            if up < best:
                best, code = up, UP
            if left < best:
                best, code = left, LEFT
            D[i, j] = np.float32(c[i, j] + best)
            codes[i, j] = code
    n, span = backtrace(codes)
    return D[-1, -1], n, span


def dtw_f64(a, b) -> float:
    """Plain float64 DP over float64 costs: the minimum total."""
    c = local_cost(a, b, np.float64)
    la, lb = c.shape
    D = np.full((la + 1, lb + 1), np.inf)
    D[0, 0] = 0.0
    for i in range(la):
        for j in range(lb):
            D[i + 1, j + 1] = c[i, j] + min(D[i, j], D[i, j + 1], D[i + 1, j])
    return float(D[la, lb])


def brute_force(a, b) -> float:
    """The minimum float64 total over ALL monotone paths (la, lb <= 5)."""
    c = local_cost(a, b, np.float64)
    la, lb = c.shape
    assert la <= 5 and lb <= 5

    def walk(i, j):
        if i == la - 1 and j == lb - 1:
            return c[i, j]
        tails = []
        if i + 1 < la and j + 1 < lb:
            tails.append(walk(i + 1, j + 1))
        if i + 1 < la:
            tails.append(walk(i + 1, j))
        if j + 1 < lb:
            tails.append(walk(i, j + 1))
        return c[i, j] + min(tails)

    return float(walk(0, 0))


def path_from_span(span: np.ndarray, la: int) -> np.ndarray:
    """[P, 2] cells of the path a span describes."""
    return np.array([(i, j) for i in range(la) for j in range(int(span[i, 0]), int(span[i, 1]) + 1)], dtype=np.int64).reshape(-1, 2)


def path_in_band(span: np.ndarray, la: int, lb: int, r: int) -> bool:
    p = path_from_span(span, la)
    return bool(np.all(in_band(p[:, 0], p[:, 1], la, lb, r)))


def grid_pair(seed: int, la: int, lb: int, D: int = 8):
    """Inputs on the 1/8 grid in [-0.5, 0.5]: every sum of the contract is exact in fp32, and ties are everywhere."""
    rng = np.random.RandomState(seed)
    return (rng.randint(-4, 5, size=(la, D)) / 8.0).astype(np.float32), (rng.randint(-4, 5, size=(lb, D)) / 8.0).astype(np.float32)


# The other five orders in which the three predecessors could be tried.
OTHER_ORDERS = tuple(o for o in ((DIAG, LEFT, UP), (UP, DIAG, LEFT), (UP, LEFT, DIAG), (LEFT, DIAG, UP), (LEFT, UP, DIAG)))


def tie_sizes():
    """(la, lb, seeds wanted) straddling one cost tile and one strip of the header."""
    k = header_constants()
    t, st = k["VTTS_DTW_TILE"], k["VTTS_DTW_STRIP"]
    return [(t - 3, t + 5, 3), (t + 7, t - 2, 3), (st + 3, st - 5, 2), (st - 2, st + 9, 2)]


def tie_sensitive(seed: int, la: int, lb: int, D: int = 8) -> bool:
    """True if every other tie order changes the span of this grid pair."""
    a, b = grid_pair(seed, la, lb, D)
    want = dtw_f32(a, b)[2]
    return all(not np.array_equal(dtw_f32(a, b, order=o)[2], want) for o in OTHER_ORDERS)


def tie_seeds(la: int, lb: int, count: int, D: int = 8, limit: int = 400):
    """The first ``count`` seeds whose grid pair is tie-sensitive."""
    out = []
    for seed in range(limit):
        if tie_sensitive(seed, la, lb, D):
            out.append(seed)
            if len(out) == count:
                return out
    raise AssertionError(f"fewer than {count} tie-sensitive seeds below {limit} at {la} x {lb}")


def planted_warp(seed: int, la: int, D: int, lo: int = 1, hi: int = 3):
    """a with pairwise distinct rows, b = every row of a repeated lo .. hi times, and the repeat counts."""
    rng = np.random.RandomState(seed)
    a = rng.standard_normal((la, D)).astype(np.float32)
    reps = rng.randint(lo, hi + 1, size=la)
    return a, np.repeat(a, reps, axis=0), reps
