"""include/vtts_loudness.h restated in numpy, in two modes:

* ``measure(x, rate)``: float64, the two biquads run sequentially over the whole row.  This is the reference the kernel is compared with.
* ``measure(x, rate, mode="f32")``: float32, in the kernel's chunked scheme (every chunk of VTTS_LOUDNESS_CHUNK samples filtered from zero
  state, the end states carried along as s -> A^CHUNK s + p, the homogeneous response of the incoming state added afterwards, from tables
  computed in double and rounded once).  It is NOT bit-exact with the kernel, whose scan combines the end states as a tree; its distance
  from the float64 mode is the error scale the GPU test derives its bound from.

and the inputs and row lengths the CPU and GPU tests share."""
from __future__ import annotations

import functools
import math
import re
from pathlib import Path
from typing import NamedTuple

import numpy as np

HEADER = Path(__file__).resolve().parents[1] / "include" / "vtts_loudness.h"

# ITU-R BS.1770-4, table 1 and table 2: the coefficients at 48 kHz (b0 b1 b2 a1 a2 of the shelf, then of the high-pass)
BS1770_48K = np.array([1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
                       1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621])
ABS_GATE = -70.0


def header_constants() -> dict:
    return {k: int(v) for k, v in re.findall(r"#define\s+(VTTS_LOUDNESS_[A-Z_]+)\s+(\d+)\s", HEADER.read_text())}


K = header_constants()
CHUNK, SEGMENT = K["VTTS_LOUDNESS_CHUNK"], K["VTTS_LOUDNESS_SEGMENT"]
WAVE_SPAN = 64 * CHUNK


class Loudness(NamedTuple):
    integrated: float        # LUFS, -inf when no block passes
    momentary_max: float     # -inf without a block
    sample_peak: np.float32  # max |x| of the float32 samples
    n_blocks: int
    n_gated: int
    momentary: np.ndarray    # [J] float64
    gate_room: float         # the smallest distance of a block from either gate, in LU (inf without a block)


def coefficients(rate: int) -> np.ndarray:
    """The header's formulae in double."""
    out = np.empty(10)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    k = math.tan(math.pi * f0 / rate)
    vh = 10.0 ** (G / 20.0)
    vb = vh ** 0.4996667741545416
    a0 = 1.0 + k / Q + k * k
    out[:5] = [(vh + vb * k / Q + k * k) / a0, 2.0 * (k * k - vh) / a0, (vh - vb * k / Q + k * k) / a0, 2.0 * (k * k - 1.0) / a0, (1.0 - k / Q + k * k) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    k = math.tan(math.pi * f0 / rate)
    a0 = 1.0 + k / Q + k * k
    out[5:] = [1.0, -2.0, 1.0, 2.0 * (k * k - 1.0) / a0, (1.0 - k / Q + k * k) / a0]
    return out


def as_float32(x) -> np.ndarray:
    """The samples as the kernel loads them: PCM16 times 2^-15 (exact), float32 as it is."""
    x = np.asarray(x)
    return x.astype(np.float32) * np.float32(1.0 / 32768.0) if x.dtype == np.int16 else x.astype(np.float32, copy=False)


def _biquad(x: np.ndarray, c) -> np.ndarray:
    """One biquad in transposed direct form II, sequentially, in x's precision."""
    try:
        from scipy.signal import lfilter
    except ImportError:
        lfilter = None
    b0, b1, b2, a1, a2 = (x.dtype.type(v) for v in c)
    if lfilter is not None and x.dtype == np.float64:
        return lfilter([b0, b1, b2], [1.0, a1, a2], x)  # the same structure and order of operations
    y = np.empty_like(x)
    s1 = s2 = x.dtype.type(0)
    for n, v in enumerate(x):
        o = b0 * v + s1
        s1 = b1 * v - a1 * o + s2
        s2 = b2 * v - a2 * o
        y[n] = o
    return y


def kweight_f64(x, rate: int) -> np.ndarray:
    c = coefficients(rate)
    return _biquad(_biquad(as_float32(x).astype(np.float64), c[:5]), c[5:])


@functools.lru_cache(maxsize=None)
def tables(rate: int):
    """(float32 coefficients, kappa, T A^CHUNK T^-1 as float32, htab [CHUNK, 4] as float32), A from the ROUNDED coefficients in double.
    The kernel carries the state as q = T s = (s1, s2, s3 + s4, kappa s4), kappa = sqrt(1 + c1 + c2): in the filter's own coordinates the
    high-pass block of A is close to a Jordan block and its powers grow to 136 (viettts_amd/csrc/loudness_design.h)."""
    cf = coefficients(rate).astype(np.float32)
    a1, a2, c1, c2 = (float(cf[i]) for i in (3, 4, 8, 9))
    A = np.array([[-a1, 1.0, 0.0, 0.0], [-a2, 0.0, 0.0, 0.0], [-2.0 - c1, 0.0, -c1, 1.0], [1.0 - c2, 0.0, -c2, 0.0]])
    kappa = np.float32(math.sqrt(1.0 + c1 + c2))
    T = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 1.0], [0, 0, 0, float(kappa)]])
    Ti = np.linalg.inv(T)
    p, h = np.eye(4), np.empty((CHUNK, 4))
    for i in range(CHUNK):
        h[i] = (p[0] + p[2]) @ Ti
        p = A @ p
    return cf, kappa, (T @ p @ Ti).astype(np.float32), h.astype(np.float32)


def kweight_f32(x, rate: int) -> np.ndarray:
    """The kernel's chunked scheme in float32 (no FMA, a sequential carry): the error scale, not the kernel's bits."""
    cf, kappa, AC, htab = tables(rate)
    x = as_float32(x)
    S = len(x)
    n = -(-S // CHUNK)
    c = np.zeros((n, CHUNK), np.float32)
    c.reshape(-1)[:S] = x
    b0, b1, b2, a1, a2, _, _, _, c1, c2 = cf
    s1 = s2 = s3 = s4 = np.zeros(n, np.float32)
    zp = np.empty_like(c)
    for i in range(CHUNK):  # every chunk from zero state
        v = c[:, i]
        y1 = b0 * v + s1
        s1 = b1 * v + (s2 - a1 * y1)
        s2 = b2 * v - a2 * y1
        z = y1 + s3
        s3 = (s4 - np.float32(2.0) * y1) - c1 * z
        s4 = y1 - c2 * z
        zp[:, i] = z
    p = np.stack([s1, s2, s3 + s4, kappa * s4], axis=1)
    sin = np.zeros((n, 4), np.float32)
    s = np.zeros(4, np.float32)
    for k in range(n):  # the carry
        sin[k] = s
        s = (AC @ s).astype(np.float32) + p[k]
    z = zp + (sin[:, None, :] * htab[None, :, :]).sum(axis=2, dtype=np.float32)
    return z.reshape(-1)[:S]


def lufs(z):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(z)


def gate(zf: np.ndarray, x32: np.ndarray, rate: int) -> Loudness:
    """Blocks and gates of the header over the filtered samples ``zf``, in float64."""
    H = rate // 10
    S = len(zf)
    nH = S // H
    J = max(0, nH - 3)
    peak = np.float32(np.abs(x32).max()) if S else np.float32(0)
    e = (zf[: nH * H].astype(np.float64) ** 2).reshape(nH, H).sum(axis=1) if nH else np.zeros(0)
    if J == 0:
        return Loudness(-np.inf, -np.inf, peak, 0, 0, np.zeros(0), np.inf)
    zb = (e[:-3] + e[1:-2] + e[2:-1] + e[3:]) / (4.0 * H)
    l = lufs(zb)
    above = l > ABS_GATE
    room = np.abs(l - ABS_GATE).min()
    if not above.any():
        return Loudness(-np.inf, float(l.max()), peak, J, 0, l, float(room))
    rel = float(lufs(zb[above].mean())) - 10.0
    room = min(room, np.abs(l - rel).min())
    keep = above & (l > rel)
    integrated = float(lufs(zb[keep].mean())) if keep.any() else -np.inf
    return Loudness(integrated, float(l.max()), peak, J, int(keep.sum()), l, float(room))


def measure(x, rate: int = 16000, mode: str = "f64") -> Loudness:
    x32 = as_float32(x)
    zf = kweight_f64(x32, rate) if mode == "f64" else kweight_f32(x32, rate)
    return gate(zf, x32, rate)


def num_blocks(n: int, rate: int) -> int:
    return max(0, n // (rate // 10) - 3)


def gain(r: Loudness, target: float = -23.0, ceiling_db: float = -1.0, max_gain_db: float = 30.0) -> np.float32:
    """The header's gain rule: each term in double, rounded to float32, then the min; 1 without a loudness."""
    if not np.isfinite(r.integrated):
        return np.float32(1.0)
    with np.errstate(divide="ignore"):
        terms = [10.0 ** ((target - r.integrated) / 20.0), 10.0 ** (max_gain_db / 20.0), 10.0 ** (ceiling_db / 20.0) / np.float64(r.sample_peak)]
    return np.float32(min(np.float32(t) for t in terms))


# ------------------------------------------------------------ inputs ------------------------------------------------------------
def tone(freq: float, amp: float, n: int, rate: int) -> np.ndarray:
    return amp * np.sin(2.0 * np.pi * freq * np.arange(n) / rate)


def gated_signal(rate: int = 16000) -> np.ndarray:
    """0.55 s of silence, 1.05 s of 440 Hz at -36 dBFS, 1.55 s at -20 dBFS: the quiet part is above the absolute gate and below the relative."""
    n0, n1, n2 = (int(round(t * rate)) for t in (0.55, 1.05, 1.55))
    return np.concatenate([np.zeros(n0), tone(440.0, 10.0 ** (-36.0 / 20.0), n1, rate), tone(440.0, 10.0 ** (-20.0 / 20.0), n2, rate)]).astype(np.float32)


def signal(name: str, n: int, rate: int = 16000):
    """``n`` samples of one of the inputs that expose a broken state carry; "noise" is int16 PCM, the others float32."""
    if name == "dc":  # the high-pass must have forgotten the step by the later segments
        return (0.5 + tone(1000.0, 0.01, n, rate)).astype(np.float32)
    if name == "low":  # 30 Hz is where the high-pass is steep: its poles sit at 1 - 0.015
        return (tone(30.0, 0.5, n, rate) + tone(1000.0, 0.01, n, rate)).astype(np.float32)
    if name == "gated":
        g = gated_signal(rate)
        return np.concatenate([g, g])[:n] if n > len(g) else g[:n]
    if name == "noise":
        return np.random.default_rng(1770).integers(-32768, 32768, n).astype(np.int16)
    raise KeyError(name)


SIGNALS = ("dc", "low", "gated", "noise")


def edge_lengths(rate: int = 16000) -> list:
    """Row lengths at every edge of the kernel's grid: the first block, a whole segment and one past it, three segments' worth of state
    carry, a wave's span, and one row of about 3 s."""
    H = rate // 10
    return [4 * H - 1, 4 * H, 4 * H + 1, 5 * H, SEGMENT - 1, SEGMENT, SEGMENT + 1, 2 * SEGMENT + 1, 5 * WAVE_SPAN - 1, 5 * WAVE_SPAN + 1,
            CHUNK * (-(-4 * H // CHUNK) + 1) - 1, CHUNK * (-(-4 * H // CHUNK) + 1) + 1, int(3.15 * rate)]


@functools.lru_cache(maxsize=None)
def batch(name: str, rate: int = 16000):
    """(rows [N, S_stride] with S_stride above the longest row and junk past every row's end, lengths) of one input.  Read-only."""
    lengths = edge_lengths(rate)
    full = signal(name, max(lengths), rate)
    stride = max(lengths) + 37
    junk = np.int16(12345) if full.dtype == np.int16 else np.float32(0.75)
    rows = np.full((len(lengths), stride), junk, dtype=full.dtype)
    for b, n in enumerate(lengths):
        rows[b, :n] = full[:n]
    rows.setflags(write=False)
    return rows, lengths


@functools.lru_cache(maxsize=None)
def batch_reference(name: str, rate: int = 16000):
    """(float64 results, float32-mode results) of every row of ``batch(name, rate)``."""
    rows, lengths = batch(name, rate)
    return ([measure(rows[b, :n], rate) for b, n in enumerate(lengths)], [measure(rows[b, :n], rate, "f32") for b, n in enumerate(lengths)])


def restatement_error(cases) -> float:
    """The largest distance in LU between the float32 restatement and float64 over ``cases`` [(name, rate)]: integrated, momentary maximum
    and every momentary value above the absolute gate."""
    worst = 0.0
    for name, rate in cases:
        for a, b in zip(*batch_reference(name, rate)):
            worst = max(worst, distance(b, a))
    return worst


def distance(got: Loudness, ref: Loudness) -> float:
    """Largest |difference| in LU over the figures the contract bounds; both sides -inf counts as equal."""
    d = 0.0
    for g, r in ((got.integrated, ref.integrated), (got.momentary_max, ref.momentary_max)):
        if np.isfinite(r) or np.isfinite(g):
            d = max(d, abs(float(g) - float(r)))
    m = ref.momentary > ABS_GATE
    if m.any():
        d = max(d, float(np.abs(np.asarray(got.momentary, np.float64)[m] - ref.momentary[m]).max()))
    return d


def bound(cases) -> float:
    """The GPU test's bound: 4 x the restatement's error (the kernel's reduction order differs from the restatement's), at least 1e-3 LU, at
    most the 0.1 LU meter tolerance of EBU Tech 3341."""
    return min(max(4.0 * restatement_error(cases), 1e-3), 0.1)
