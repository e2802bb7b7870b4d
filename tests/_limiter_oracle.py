"""Plain numpy restatement of include/vtts_limiter.h: the 4x oversampled envelope, the true peak, the gain computer (sliding minimum, then a
sliding mean, of the gain each sample asks for) and the output, in float64 (the oracle) and in float32 (the kernel's arithmetic class, whose
distance from float64 on the GPU test's rows is that test's yardstick).

    u[m]    = sum_n x[n] h[m - 4 n + 96]                              (tests/_audio_oracle.py's sum for fs -> 4 fs, written out again here)
    p[n]    = max(|x[n]|, |u[4 n .. 4 n + 3]|),  true_peak = max p
    req[n]  = 1 where g p[n] <= c, else c / (g p[n]);   held[n] = min req[n - W .. n + W];   a[n] = min(req[n], mean held[n - W .. n + W])
    y[n]    = (g x[n]) a[n]                                           (indices clamped to the row: edge replication)
"""
from __future__ import annotations

import re
from functools import lru_cache
from pathlib import Path
from typing import NamedTuple

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import _audio_oracle as A

REPO = Path(__file__).resolve().parents[1]
HEADER = REPO / "include" / "vtts_limiter.h"
K = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(VTTS_LIMITER_[A-Z_]+)\s+(\d+)\s", HEADER.read_text())}
TILE = K["VTTS_LIMITER_TILE"]
RUN = K["VTTS_LIMITER_RUN"]
OS = K["VTTS_LIMITER_OVERSAMPLE"]
HALF = A.ZEROS * OS          # 96
NJ = -(-(2 * HALF + 1) // OS)  # 49 taps a phase at most


def lookahead(fs: int, ms: float = 5.0) -> int:
    return max(1, int(np.floor(float(fs) * float(np.float32(ms)) / 1000.0 + 0.5)))


def ceiling(dbtp: float = -1.0) -> np.float32:
    return np.float32(10.0 ** (float(np.float32(dbtp)) / 20.0))


def as_float(x) -> np.ndarray:
    """PCM16 times 2^-15, anything else as float32: the samples the kernels see."""
    x = np.asarray(x)
    return (x.astype(np.float32) / np.float32(32768.0)) if x.dtype == np.int16 else x.astype(np.float32)


def oversample(x, fs: int, dtype=np.float64) -> np.ndarray:
    """u [4 S].  float64: products in descending n, summed by numpy along the row.  float32: fp32 taps, one rounding per step in ascending n
    (``float32(acc + x h)`` in fp64 is fmaf up to a double rounding)."""
    x = as_float(x)
    S = x.shape[0]
    h = A.prototype(fs, OS * fs)
    u = np.zeros(OS * S, dtype=dtype)
    if S == 0:
        return u
    xp = np.zeros(S + 2 * (NJ - 1), dtype=np.float64)  # x[n] at xp[n + 48]
    xp[NJ - 1:NJ - 1 + S] = x
    for r in range(OS):
        k = r + OS * np.arange(NJ)                      # tap of j = 0 .. 48, on x[n + 24 - j]
        hj = np.where(k <= 2 * HALF, h[np.minimum(k, 2 * HALF)], 0.0)
        win = sliding_window_view(xp, NJ)[24:24 + S]    # row n: x[n - 24 .. n + 24], ascending
        if np.dtype(dtype) == np.float64:
            for c0 in range(0, S, 8192):
                u[r + OS * c0:r + OS * min(S, c0 + 8192):OS] = np.sum(np.ascontiguousarray(win[c0:c0 + 8192, ::-1]) * hj[None, :], axis=1)
        else:
            h32 = hj.astype(np.float32).astype(np.float64)
            acc = np.zeros(S, dtype=np.float32)
            for i in range(NJ):                          # ascending n: j = 48 - i
                acc = (acc.astype(np.float64) + win[:, i] * h32[NJ - 1 - i]).astype(np.float32)
            u[r::OS] = acc
    return u


def envelope(x, fs: int, dtype=np.float64) -> np.ndarray:
    x = as_float(x)
    u = oversample(x, fs, dtype)
    return np.maximum(np.abs(x.astype(dtype)), np.abs(u).reshape(-1, OS).max(axis=1)) if x.shape[0] else np.zeros(0, dtype)


def true_peak(x, fs: int, dtype=np.float64) -> float:
    p = envelope(x, fs, dtype)
    return float(p.max()) if p.size else 0.0


class Limited(NamedTuple):
    y: np.ndarray
    a: np.ndarray
    req: np.ndarray
    held: np.ndarray
    p: np.ndarray
    true_peak: float
    min_gain: float
    g: np.float32
    c: np.float32


def _window_mean(held: np.ndarray, W: int, fixed_order: bool) -> np.ndarray:
    S, Lw = held.shape[0], 2 * W + 1
    hp = np.pad(held.astype(np.float64), W, mode="edge")  # hp[k] = held[clamp(k - W)]: sample n's window is hp[n .. n + 2 W]
    if not fixed_order:
        return sliding_window_view(hp, Lw).sum(axis=1) / Lw
    # the header's order: runs of RUN samples from the row's first; the first of a run sums ascending from 0.0, the others slide
    nrun = -(-S // RUN)
    hp = np.concatenate([hp, np.zeros(RUN)])
    heads = sliding_window_view(hp, Lw)[:nrun * RUN:RUN]
    s = np.zeros(nrun, dtype=np.float64)
    for k in range(Lw):
        s = s + heads[:, k]
    out = np.zeros(nrun * RUN, dtype=np.float64)
    out[0::RUN] = s
    n0 = RUN * np.arange(nrun)
    for t in range(1, RUN):
        n = n0 + t
        s = (s + hp[n + 2 * W]) - hp[n - 1]
        out[t::RUN] = s
    return (out[:S] / float(Lw)).astype(np.float32)


def gain_curve(p, g, c, W: int, dtype=np.float64):
    """(req, held, a) of an envelope ``p``: the gain computer alone."""
    f = np.dtype(dtype).type
    p = np.asarray(p, dtype=dtype)
    gp = (f(np.float32(g)) * p).astype(dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        req = np.where(gp <= f(c), f(1.0), (f(c) / gp).astype(dtype)).astype(dtype)
    held = sliding_window_view(np.pad(req, W, mode="edge"), 2 * W + 1).min(axis=1)
    mean = _window_mean(held, W, f is np.float32).astype(dtype)
    return req, held, np.minimum(req, mean)


def limit(x, fs: int, g=1.0, ceiling_dbtp: float = -1.0, W=None, dtype=np.float64) -> Limited:
    """One row through the contract.  ``dtype=np.float32`` is the kernel's arithmetic: fp32 chains, fp32 products and quotient, the mean in the
    header's fixed fp64 order rounded to fp32."""
    f = np.dtype(dtype).type
    x = as_float(x)
    S = x.shape[0]
    W = lookahead(fs) if W is None else int(W)
    g = np.float32(g)
    c = ceiling(ceiling_dbtp)
    p = envelope(x, fs, dtype)
    if S == 0:
        z = np.zeros(0, dtype)
        return Limited(z, z, z, z, p, 0.0, 1.0, g, c)
    req, held, a = gain_curve(p, g, c, W, dtype)
    y = ((f(g) * x.astype(dtype)).astype(dtype) * a).astype(dtype)
    return Limited(y, a, req, held, p, float(p.max()), float(a.min()), g, c)


def pregain(integrated, target: float = -23.0, max_gain_db: float = 30.0) -> np.float32:
    i = float(np.float32(integrated))
    if not np.isfinite(i):
        return np.float32(1.0)
    return min(np.float32(10.0 ** ((float(np.float32(target)) - i) / 20.0)), np.float32(10.0 ** (float(np.float32(max_gain_db)) / 20.0)))


def overshoot_db(y, fs: int, c) -> float:
    """How far the true peak of ``y`` (metered in float64) passes the ceiling, in dB; negative below it."""
    tp = true_peak(np.asarray(y, dtype=np.float32), fs)
    return 20.0 * np.log10(tp / float(c)) if tp > 0 else -np.inf


# ------------------------------------------------------------ signals ------------------------------------------------------------
def tone(freq: float, amp: float, S: int, fs: int, phase: float = 0.0) -> np.ndarray:
    return (amp * np.sin(2 * np.pi * freq * np.arange(S) / fs + phase)).astype(np.float32)


def speech(seed: int, S: int, fs: int = 16000) -> np.ndarray:
    return A.speechlike(np.random.default_rng(seed), S, float(fs)) if S else np.zeros(0, np.float32)


def gain_for(x, fs: int, over_db: float, ceiling_dbtp: float = -1.0) -> np.float32:
    """The pre-gain that puts the row's true peak ``over_db`` above the ceiling."""
    return np.float32(float(ceiling(ceiling_dbtp)) * 10.0 ** (over_db / 20.0) / true_peak(x, fs))


def edge_lengths(fs: int = 16000, ms: float = 5.0):
    W = lookahead(fs, ms)
    return [0, 1, 2, W, W + 1, 2 * W, 2 * W + 1, 4 * W + 2, TILE - 1, TILE, TILE + 1, TILE + 2 * W - 1, TILE + 2 * W + 1, 2 * TILE + 1, 3 * fs + 37]


@lru_cache(maxsize=None)
def gpu_rows(fs: int = 16000, ms: float = 5.0):
    """The rows of tests/test_gpu_limiter.py's ragged batch: [(name, x float32, g)].  The edge lengths carry speech 4 x over full scale; then
    speech 3 / 6 / 12 dB over the ceiling, clicks at a row's ends and around a tile edge, pairs of clicks 2 W and 4 W + 1 apart across tile
    edges, a plateau longer than the window, and a row under the ceiling."""
    W = lookahead(fs, ms)
    rows = [(f"len{S}", speech(100 + i, S, fs), np.float32(4.0)) for i, S in enumerate(edge_lengths(fs, ms))]
    for i, (db, S) in enumerate(((3.0, 2 * TILE + 1), (6.0, 12000), (12.0, 2 * fs + 11))):
        x = speech(200 + i, S, fs)
        rows.append((f"speech+{db:g}dB", x, gain_for(x, fs, db)))
    S = 3 * TILE + 123
    x = (0.1 * speech(300, S, fs)).astype(np.float32)
    for j, k in enumerate((0, S - 1, TILE - 1, TILE, TILE - W, TILE + W, TILE - 2 * W, TILE + 2 * W)):
        x[k] = (0.95 - 0.05 * j) * (-1.0) ** j
    rows.append(("clicks", x, np.float32(2.0)))
    S = 4 * TILE
    x = (0.1 * speech(301, S, fs)).astype(np.float32)
    for j, k in enumerate((2 * TILE - W, 2 * TILE + W, 3 * TILE - 2 * W, 3 * TILE + 2 * W + 1)):
        x[k] = (0.9 - 0.1 * j) * (-1.0) ** j
    rows.append(("pairs", x, np.float32(2.0)))
    S = 2 * TILE + 19
    x = (0.1 * speech(302, S, fs)).astype(np.float32)
    x[TILE - W - 20:TILE + 2 * W + 25] = 0.9
    rows.append(("plateau", x, np.float32(1.5)))
    rows.append(("under", speech(303, TILE + 77, fs), np.float32(1.25)))
    return tuple(rows)


@lru_cache(maxsize=None)
def gpu_reference(fs: int = 16000, ms: float = 5.0, ceiling_dbtp: float = -1.0):
    """(float64 results, float32 results, distance) of gpu_rows(): distance = the largest |y32 - y64| over every sample of every row, and of
    |min_gain32 - min_gain64| times c.  The GPU tests' bound is 4 x distance (the loudness and STOI tests' rule)."""
    W = lookahead(fs, ms)
    f64 = [limit(x, fs, g, ceiling_dbtp, W, np.float64) for _, x, g in gpu_rows(fs, ms)]
    f32 = [limit(x, fs, g, ceiling_dbtp, W, np.float32) for _, x, g in gpu_rows(fs, ms)]
    d = 0.0
    for a, b in zip(f64, f32):
        if a.y.size:
            d = max(d, float(np.abs(a.y - b.y.astype(np.float64)).max()), abs(a.min_gain - b.min_gain) * float(a.c))
    return f64, f32, d
