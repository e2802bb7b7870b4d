"""include/vtts_pitch.h restated in numpy, operation for operation: what the GPU results are compared against with ``==``.

``yin_f32`` is the contract in float32 (vectorised over frames and lags, a loop over ``j``: milliseconds per hundred frames);
``yin_f64`` is the same in float64.  ``fault=`` plants one deviation from the contract (tests/test_pitch_cpu.py shows that each one
changes the output on the inputs the GPU test uses).  The signals both test files share are made here, once.
"""
from __future__ import annotations

import functools
import math
import re
from pathlib import Path
from typing import NamedTuple

import numpy as np

HEADER = Path(__file__).resolve().parents[1] / "include" / "vtts_pitch.h"
FAULTS = ("fma", "blocked_prefix", "le_threshold", "last_minimum", "base0", "reflect_at_stride", "swap_neighbours", "no_guard")


def header_constants() -> dict:
    """Every ``#define VTTS_PITCH_* <integer>`` of the header."""
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+(VTTS_PITCH_\w+)\s+(\d+)\s*$", HEADER.read_text(), re.M)}


K = header_constants()
NFFT, HOP, PAD, W = K["VTTS_PITCH_NFFT"], K["VTTS_PITCH_HOP"], K["VTTS_PITCH_PAD"], K["VTTS_PITCH_WINDOW"]


class Cfg(NamedTuple):
    sample_rate: int = 16000
    fmin: float = 50.0
    fmax: float = 500.0
    threshold: float = 0.15


DEFAULT = Cfg()


class Yin(NamedTuple):
    f0: np.ndarray            # [N, T]
    aperiodicity: np.ndarray  # [N, T]
    candidate: np.ndarray     # [N, T]
    tau: np.ndarray           # [N, T] int: tau*, -1 past a row's frames
    voiced: np.ndarray        # [N, T] bool


def lags(cfg: Cfg):
    """(tau_min, tau_max): the quotients in double precision, of the float32 values the C struct holds."""
    return math.ceil(cfg.sample_rate / float(np.float32(cfg.fmax))), math.floor(cfg.sample_rate / float(np.float32(cfg.fmin)))


def num_frames(n: int) -> int:
    return (int(n) + 2 * PAD - NFFT) // HOP + 1


def _frames(row: np.ndarray, L: int, dt, mirror_at=None) -> np.ndarray:
    """[T, n_fft] frames of row[:L], reflected at the row's own ends (``mirror_at``: at that sample count instead: a planted fault)."""
    end = L if mirror_at is None else mirror_at
    i = np.arange(-PAD, L + PAD)
    i = np.abs(i)
    i = np.where(i >= end, 2 * (end - 1) - i, i)
    x = row[np.clip(i, 0, len(row) - 1)]
    x = x.astype(dt) * dt(2.0 ** -15) if row.dtype == np.int16 else x.astype(dt)
    T = num_frames(L)
    return np.stack([x[HOP * t : HOP * t + NFFT] for t in range(T)])


def difference(F: np.ndarray, tau_max: int, dt, fault=None) -> np.ndarray:
    base = 0 if fault == "base0" else (NFFT - W - tau_max) // 2
    taus = np.arange(tau_max + 1)
    d = np.zeros((F.shape[0], tau_max + 1), dt)
    with np.errstate(all="ignore"):
        for j in range(W):
            e = (F[:, base + j][:, None] - F[:, base + j + taus]).astype(dt)
            if fault == "fma":
                d = (d.astype(np.float64) + e.astype(np.float64) * e.astype(np.float64)).astype(dt)
            else:
                d = (d + (e * e).astype(dt)).astype(dt)
    return d


def normalise(d: np.ndarray, dt, fault=None) -> np.ndarray:
    T, n = d.shape
    run = np.zeros((T, n), dt)
    with np.errstate(all="ignore"):
        if fault == "blocked_prefix":  # 64-blocked scan: sums inside blocks of 64 lags, then the block offsets
            r = np.zeros(T, dt)
            off = np.zeros(T, dt)
            for tau in range(1, n):
                if (tau - 1) % 64 == 0:
                    off = (off + r).astype(dt)
                    r = np.zeros(T, dt)
                r = (r + d[:, tau]).astype(dt)
                run[:, tau] = (off + r).astype(dt)
        else:
            r = np.zeros(T, dt)
            for tau in range(1, n):
                r = (r + d[:, tau]).astype(dt)
                run[:, tau] = r
        num = (d * np.arange(n).astype(dt)[None, :]).astype(dt)
        if fault == "no_guard":
            c = (num / run).astype(dt)
        else:
            c = np.where(run > 0, (num / np.where(run > 0, run, dt(1))).astype(dt), dt(1)).astype(dt)
    c[:, 0] = dt(1)
    return c


def pick(c: np.ndarray, tau_min: int, tau_max: int, threshold, fault=None):
    T = c.shape[0]
    thr = c.dtype.type(np.float32(threshold))
    with np.errstate(all="ignore"):
        nxt = np.concatenate([c[:, 1:], np.full((T, 1), np.inf, c.dtype)], axis=1)
        below = c <= thr if fault == "le_threshold" else c < thr
        hit = below & (nxt >= c)
        hit[:, :tau_min] = False
        voiced = hit.any(axis=1)
        seg = c[:, tau_min : tau_max + 1]
        if fault == "last_minimum":
            amin = seg.shape[1] - 1 - np.argmin(seg[:, ::-1], axis=1)
        else:
            amin = np.argmin(seg, axis=1)
    tau = np.where(voiced, np.argmax(hit, axis=1), tau_min + amin)
    return tau.astype(np.int64), voiced


def refine(c: np.ndarray, tau: np.ndarray, tau_max: int, rate: int, fault=None):
    dt = c.dtype.type
    rows = np.arange(c.shape[0])
    b = c[rows, tau]
    inside = tau + 1 <= tau_max
    a = c[rows, tau - 1]
    g = c[rows, np.minimum(tau + 1, tau_max)]
    if fault == "swap_neighbours":
        a, g = g, a
    with np.errstate(all="ignore"):
        den = ((a + g).astype(dt) - (b + b).astype(dt)).astype(dt)
        ok = inside & (den > 0)
        delta = ((dt(0.5) * (a - g).astype(dt)).astype(dt) / np.where(ok, den, dt(1))).astype(dt)
        delta = np.minimum(np.maximum(delta, dt(-1)), dt(1))
        tau_f = np.where(ok, (tau.astype(dt) + delta).astype(dt), tau.astype(dt)).astype(dt)
        cand = (dt(rate) / tau_f).astype(dt)
    return cand, b


def yin(y, cfg: Cfg = DEFAULT, lengths=None, dtype=np.float32, fault=None) -> Yin:
    """``y [N, S]`` (or ``[S]``) float32 or int16; row b's first ``lengths[b]`` samples.  Frames past a row's own count hold 0 / 1 / 0."""
    y = np.asarray(y)
    if y.ndim == 1:
        y = y[None]
    N, S = y.shape
    lens = [S] * N if lengths is None else [int(v) for v in lengths]
    tau_min, tau_max = lags(cfg)
    assert 2 <= tau_min <= tau_max <= K["VTTS_PITCH_MAX_LAG"] and min(lens) >= K["VTTS_PITCH_MIN_SAMPLES"] and max(lens) <= S
    T = max(num_frames(n) for n in lens)
    f0 = np.zeros((N, T), dtype)
    ap = np.ones((N, T), dtype)
    cand = np.zeros((N, T), dtype)
    taus = np.full((N, T), -1, np.int64)
    voiced = np.zeros((N, T), bool)
    for b, L in enumerate(lens):
        F = _frames(y[b], L, dtype, S if fault == "reflect_at_stride" else None)
        c = normalise(difference(F, tau_max, dtype, fault), dtype, fault)
        t, v = pick(c, tau_min, tau_max, cfg.threshold, fault)
        cd, a = refine(c, t, tau_max, cfg.sample_rate, fault)
        n = len(t)
        f0[b, :n], ap[b, :n], cand[b, :n], taus[b, :n], voiced[b, :n] = np.where(v, cd, dtype(0)), a, cd, t, v
    return Yin(f0, ap, cand, taus, voiced)


def yin_f32(y, cfg: Cfg = DEFAULT, lengths=None, fault=None) -> Yin:
    return yin(y, cfg, lengths, np.float32, fault)


def yin_f64(y, cfg: Cfg = DEFAULT, lengths=None) -> Yin:
    return yin(y, cfg, lengths, np.float64)


# ---------------------------------------------------------------- signals ----------------------------------------------------------------
def tone(f0: float, n_frames: int = 24, rate: int = 16000) -> np.ndarray:
    """A steady three-harmonic tone, amplitudes 0.3 / 0.15 / 0.1.  Where the period is a whole number of samples, one period is computed and
    repeated, so that the samples are periodic to the bit (sin of a phase 2 pi further on is not)."""
    S = HOP * n_frames
    period = rate / f0
    n = np.arange(int(period)) if period == int(period) else np.arange(S)
    y = sum(a * np.sin(2 * np.pi * f0 * (h + 1) * n / rate) for h, a in enumerate((0.3, 0.15, 0.1))).astype(np.float32)
    return np.resize(y, S)


@functools.lru_cache(maxsize=None)
def glide_row(seed: int, n_frames: int = 96, rate: int = 16000) -> np.ndarray:
    """Eight harmonics with random amplitudes and phases on an F0 that glides 120 + 60 sin(2 pi 0.7 t) + 40 t / duration Hz, peak 0.2, plus
    N(0, 0.01^2) noise; the second fifth is N(0, 0.05^2) noise alone, half of the fourth fifth exact zeros."""
    r = np.random.RandomState(seed)
    S = HOP * n_frames
    t = np.arange(S) / rate
    f = 120 + 60 * np.sin(2 * np.pi * 0.7 * t) + 40 * t / (S / rate)
    ph = 2 * np.pi * np.cumsum(f) / rate
    y = sum(r.uniform(0.2, 1) / k * np.sin(k * ph + r.uniform(0, 6)) for k in range(1, 9))
    y = 0.2 * y / np.abs(y).max() + 0.01 * r.standard_normal(S)
    seg = S // 5
    y[seg : 2 * seg] = 0.05 * r.standard_normal(seg)
    y[3 * seg : 3 * seg + seg // 2] = 0
    y = y.astype(np.float32)
    y.setflags(write=False)
    return y


def square_row(n_samples: int, period: int = 147) -> np.ndarray:
    """A full-scale +-1 square wave: d reaches 4 * 512, where the orders of the chain separate."""
    return np.where((np.arange(n_samples) % period) < period // 2, 1.0, -1.0).astype(np.float32)


def grid_row(seed: int, n_frames: int = 24, period: int = 40) -> np.ndarray:
    """Samples on a 1/8 grid, so that d, run and many c are exact and ties exist: a third with an integer period (c = 0 at every multiple of
    it), a third of single impulses in silence (c = 1 over whole ranges of lags, and frames of exact zeros: c = 1 everywhere), a third of
    grid noise."""
    r = np.random.RandomState(seed)
    S = HOP * n_frames
    y = np.zeros(S, np.float32)
    third = S // 3
    y[:third] = np.resize(r.randint(-7, 8, period) / 8.0, third)
    for p in range(third + 700, 2 * third - 700, 1700):
        y[p] = r.randint(1, 8) / 8.0
    y[2 * third :] = r.randint(-4, 5, S - 2 * third) / 8.0
    return y


# ------------------------------------------------- the inputs of tests/test_gpu_pitch.py -------------------------------------------------
def edge_lengths(F: int) -> list:
    """Row lengths at the framing's and the workgroup tile's edges: F = frames per workgroup."""
    return [385, 511, 512, 513] + [HOP * k + r for k in (F - 1, F, F + 1, 2 * F, 2 * F + 1) for r in (-1, 0, 1)]


def to_pcm16(y: np.ndarray) -> np.ndarray:
    return np.round(np.asarray(y, np.float64) * 32767.0).astype(np.int16)


def rows_of(lengths, pcm: bool = False, fill=None, stride=None) -> np.ndarray:
    """[len(lengths), stride] rows cut from the gliding rows at varying offsets; past a row's own length ``fill`` (default: more signal)."""
    S = max(lengths) if stride is None else stride
    y = np.stack([np.resize(glide_row(i % 12)[37 * i :], S) for i in range(len(lengths))])
    y = to_pcm16(y) if pcm else y.astype(np.float32)
    if fill is not None:
        for b, n in enumerate(lengths):
            y[b, n:] = fill
    return y


def ragged_batch(F: int, pcm: bool):
    """8 rows with lengths from the edge list, a stride beyond all of them, NaN (float) or 0x7FFF (PCM16) behind every row."""
    lengths = [edge_lengths(F)[i] for i in (0, 3, 5, 7, 9, 12, 15, 18)]
    return rows_of(lengths, pcm, 0x7FFF if pcm else np.nan, stride=max(lengths) + 300), lengths


@functools.lru_cache(maxsize=None)
def content_rows():
    """One gliding row (voiced, noise and zero frames), an all-zero row, a full-scale square wave and the tie-rich grid row, ragged."""
    lengths = [HOP * 96, HOP * 12 + 5, HOP * 24, HOP * 24]
    y = np.zeros((4, lengths[0]), np.float32)
    y[0] = glide_row(0)
    y[2, : lengths[2]] = square_row(lengths[2])
    y[3, : lengths[3]] = grid_row(5)
    y.setflags(write=False)
    return y, lengths


@functools.lru_cache(maxsize=None)
def agreement_rows() -> np.ndarray:
    """The twelve rows of the float64 agreement test: 1152 frames."""
    y = np.stack([glide_row(s) for s in range(12)])
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def agreement_f32() -> Yin:
    return yin_f32(agreement_rows())


@functools.lru_cache(maxsize=None)
def threshold_on_a_value() -> Cfg:
    """The default configuration with its threshold moved onto a value c takes: the aperiodicity of an unvoiced frame of content_rows()
    (the minimum of c over the search range), taken from this oracle.  With < that frame stays unvoiced; with <= it turns voiced."""
    y, lengths = content_rows()
    r = yin_f32(y, DEFAULT, lengths)
    ap = r.aperiodicity[0][(~r.voiced[0]) & (r.aperiodicity[0] < 0.9)]
    assert ap.size and 0.15 < float(ap.min()) < 0.9
    return DEFAULT._replace(threshold=float(ap.min()))


LAG_EDGE_CFGS = {  # tau_max 63, 64, 65, 320, 326, 512 at 16 kHz; tau_min 2; one lag only
    "tau_max_63": Cfg(fmin=253.0), "tau_max_64": Cfg(fmin=250.0), "tau_max_65": Cfg(fmin=246.0), "tau_max_320": Cfg(fmin=50.0),
    "tau_max_326": Cfg(fmin=49.0), "tau_max_512": Cfg(fmin=31.25), "tau_min_2": Cfg(fmax=8000.0), "one_lag": Cfg(fmin=100.0, fmax=100.0),
}
