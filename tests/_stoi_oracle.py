"""include/vtts_stoi.h restated in numpy:

* ``measure(x, y)``: float64 from the kept frames on (stage A's energies are fp64 sums of exact squares in the header's own order in
  every mode, so the keep mask is the kernel's bit for bit).  This is the reference the kernel is compared with.
* ``measure(x, y, f32=True)``: stages B and C in float32 (``scipy.fft.rfft`` keeps single precision).  It is NOT bit-exact with the kernel,
  whose transform is factored differently and whose stage C is fp64; its distance from the float64 mode is the error scale the GPU test
  derives its bound from.
* ``measure(x, y, ola=True)``: stage B as the papers state it: window, overlap-add the kept frames at hop 128, re-frame.
* ``measure(x, y, fault=NAME)``: one planted fault of FAULTS, for the test that the bound can see each of them.

and the inputs, row lengths and bounds the CPU and GPU tests share."""
from __future__ import annotations

import functools
import re
from pathlib import Path
from typing import NamedTuple, Optional

import numpy as np
import scipy.fft

HEADER = Path(__file__).resolve().parents[1] / "include" / "vtts_stoi.h"

FRAME, HOP, NFFT, BANDS, SEG = 256, 128, 512, 15, 30
RATE = 10000
EPS = 2.0 ** -52
BAND_LO = (7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219)  # include/vtts_stoi.h
FAULTS = ("band_lo_minus", "band_lo_plus", "window_phase", "periodic_hann", "no_removal", "wrong_kept", "no_clip", "drop_prev", "seg31")
BOUND_FACTOR = 8.0   # the issue's: the bound is 8 x the float32 restatement's distance from float64 ...
BOUND_CAP = 1e-5     # ... and never above this on the figures


def header_constants() -> dict:
    return {k: int(v) for k, v in re.findall(r"#define\s+(VTTS_STOI_[A-Z_]+)\s+(\d+)\s", HEADER.read_text())}


K = header_constants()
FPB = K["VTTS_STOI_FRAMES_PER_BLOCK"]


class Stoi(NamedTuple):
    stoi: float               # nan without a segment
    estoi: float
    n_frames: int             # K
    n_kept: int               # Kk
    n_segments: int           # M
    kept: np.ndarray          # [Kk] the kept candidate frames
    energy: np.ndarray        # [K] float64
    mags: np.ndarray          # [2, 15, T]: X, then Y
    stoi_series: np.ndarray   # [M]
    estoi_series: np.ndarray


def derive_bands() -> tuple:
    """Third octaves from 150 Hz on the 512-point grid at 10 kHz: band j runs from the bin nearest 150 * 2^((2 j - 1) / 6) Hz up to, not
    including, the bin nearest 150 * 2^((2 j + 1) / 6) Hz.  Returns (first bins, end bins)."""
    f = RATE * np.arange(NFFT // 2 + 1) / NFFT
    j = np.arange(BANDS)
    lo = [int(np.argmin((f - 150.0 * 2.0 ** ((2 * i - 1) / 6.0)) ** 2)) for i in j]
    hi = [int(np.argmin((f - 150.0 * 2.0 ** ((2 * i + 1) / 6.0)) ** 2)) for i in j]
    return tuple(lo), tuple(hi)


def window(fault: Optional[str] = None) -> np.ndarray:
    """hanning(258)[1:-1] in double, rounded once to float32."""
    r = np.arange(FRAME, dtype=np.float64)
    if fault == "window_phase":
        return (0.5 - 0.5 * np.cos(2.0 * np.pi * r / (FRAME + 1))).astype(np.float32)
    if fault == "periodic_hann":
        return (0.5 - 0.5 * np.cos(2.0 * np.pi * r / FRAME)).astype(np.float32)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * (r + 1.0) / (FRAME + 1))).astype(np.float32)


def num_frames(S: int) -> int:
    return -(-(S - FRAME) // HOP) if S > FRAME else 0


def counts(S: int) -> tuple:
    """(K, M) of a row that keeps every frame."""
    k = num_frames(S)
    return k, max(0, max(0, k - 1) - (SEG - 1))


def as_float32(x) -> np.ndarray:
    x = np.asarray(x)
    if x.dtype == np.int16:
        return x.astype(np.float32) * np.float32(2.0 ** -15)  # exact
    assert x.dtype in (np.float32, np.float64), x.dtype  # (float64: the oracle alone, for properties stated on exact values)
    return x


def candidate_frames(x: np.ndarray, w: np.ndarray) -> np.ndarray:
    """p_k[r] = fl32(x[128 k + r] w[r]): [K, 256] float32."""
    k = num_frames(len(x))
    idx = HOP * np.arange(k)[:, None] + np.arange(FRAME)[None, :]
    return x[idx] * w[None, :] if k else np.zeros((0, FRAME), np.float32)


def energies(p: np.ndarray) -> np.ndarray:
    """The header's order: four strided squares per lane, then the halvings 32 .. 1."""
    q = p.astype(np.float64).reshape(-1, 4, 64) ** 2
    s = ((q[:, 0] + q[:, 1]) + q[:, 2]) + q[:, 3]
    h = 32
    while h:
        s = s[:, :h] + s[:, h : 2 * h]
        h //= 2
    return s[:, 0]


def keep_list(e: np.ndarray) -> np.ndarray:
    if not len(e):
        return np.zeros(0, np.int64)
    return np.flatnonzero(e > 1e-4 * e.max())


def gather_frames(p: np.ndarray, kept: np.ndarray, dt, fault: Optional[str] = None) -> np.ndarray:
    """u_t of stage B: [T, 256] in ``dt``."""
    T = max(0, len(kept) - 1)
    u = p[kept[:T]].astype(dt)
    if T:
        u[:, HOP:] += p[kept[1 : T + 1], :HOP].astype(dt)
        if T > 1 and fault != "drop_prev":
            u[1:, :HOP] += p[kept[: T - 1], HOP:].astype(dt)
    return u


def ola_frames(p: np.ndarray, kept: np.ndarray, dt) -> np.ndarray:
    """The same frames the long way: overlap-add the kept frames at hop 128, then re-frame with range(0, len - 256, 128)."""
    z = np.zeros((len(kept) + 1) * HOP if len(kept) else 0, dt)
    for i, k in enumerate(kept):
        z[HOP * i : HOP * i + FRAME] += p[k].astype(dt)
    starts = range(0, len(z) - FRAME, HOP)
    return np.stack([z[s : s + FRAME] for s in starts]) if len(starts) else np.zeros((0, FRAME), dt)


def band_magnitudes(u: np.ndarray, w: np.ndarray, dt, lo=BAND_LO) -> np.ndarray:
    """[15, T] in ``dt``."""
    if not len(u):
        return np.zeros((BANDS, 0), dt)
    v = u * w.astype(dt)[None, :]
    z = scipy.fft.rfft(v, NFFT, axis=-1)
    assert z.dtype == (np.complex64 if dt == np.float32 else np.complex128)
    P = z.real * z.real + z.imag * z.imag
    return np.stack([np.sqrt(P[:, lo[j] : lo[j + 1]].sum(axis=-1, dtype=dt)) for j in range(BANDS)]).astype(dt)


def segments(X: np.ndarray, Y: np.ndarray, dt, seg: int = SEG, clip: bool = True):
    """(d_m of STOI, d_m of ESTOI), each [M] in ``dt``."""
    T = X.shape[1]
    M = max(0, T - seg + 1)
    if not M:
        return np.zeros(0, dt), np.zeros(0, dt)
    eps, c = dt(EPS), dt(1.0 + 10.0 ** (15.0 / 20.0))
    idx = np.arange(M)[:, None] + np.arange(seg)[None, :]
    xs, ys = X[:, idx].transpose(1, 0, 2), Y[:, idx].transpose(1, 0, 2)  # [M, 15, seg]

    def norm(a, axis):
        return np.sqrt((a * a).sum(axis=axis, keepdims=True))

    def normalise(a, axis):
        a = a - a.mean(axis=axis, keepdims=True)
        return a / (norm(a, axis) + eps)

    yp = ys * (norm(xs, 2) / (norm(ys, 2) + eps))
    if clip:
        yp = np.minimum(yp, c * xs)
    d_stoi = (normalise(xs, 2) * normalise(yp, 2)).sum(axis=(1, 2)) / dt(BANDS)
    d_estoi = (normalise(normalise(xs, 2), 1) * normalise(normalise(ys, 2), 1)).sum(axis=(1, 2)) / dt(seg)
    assert d_stoi.dtype == dt and d_estoi.dtype == dt
    return d_stoi, d_estoi


def measure(x, y, f32: bool = False, ola: bool = False, fault: Optional[str] = None) -> Stoi:
    assert fault is None or fault in FAULTS, fault
    x, y = as_float32(x), as_float32(y)
    assert x.shape == y.shape and x.ndim == 1
    dt = np.float32 if f32 else np.float64
    w = window(fault)
    p, q = candidate_frames(x, w), candidate_frames(y, w)
    e = energies(p)
    kept = keep_list(e)
    if fault == "no_removal":
        kept = np.arange(len(e))
    if fault == "wrong_kept" and len(kept) > 2:
        kept = kept.copy()
        kept[len(kept) // 2] = kept[len(kept) // 2 + 1]
    lo = list(BAND_LO)
    if fault in ("band_lo_minus", "band_lo_plus"):
        lo[8] += -1 if fault == "band_lo_minus" else 1
    frames = ola_frames if ola else functools.partial(gather_frames, fault=fault)
    X, Y = band_magnitudes(frames(p, kept, dt), w, dt, lo), band_magnitudes(frames(q, kept, dt), w, dt, lo)
    ds, de = segments(X, Y, dt, seg=31 if fault == "seg31" else SEG, clip=fault != "no_clip")
    M = len(ds)
    nan = float("nan")
    return Stoi(float(ds.mean(dtype=dt)) if M else nan, float(de.mean(dtype=dt)) if M else nan, len(e), len(kept), M, kept, e, np.stack([X, Y]), ds, de)


# ------------------------------------------------------------ inputs ------------------------------------------------------------
def make_speechlike(S: int, seed: int, noise: float = 0.02, quiet=None, peak: float = 0.5) -> np.ndarray:
    """``S`` samples at 10 kHz, float32: a harmonic stack on a moving F0 under a 2.5 - 4 Hz envelope, plus envelope-shaped noise.
    ``quiet = (start, stop)`` scales that stretch by 1e-3 (60 dB down: its frames fall to the 40 dB rule)."""
    rng = np.random.default_rng(seed)
    t = np.arange(S) / RATE
    f0 = 140.0 + 40.0 * np.sin(2.0 * np.pi * 0.7 * t + rng.uniform(0, 2 * np.pi)) + 15.0 * np.sin(2.0 * np.pi * 2.3 * t + rng.uniform(0, 2 * np.pi))
    ph = 2.0 * np.pi * np.cumsum(f0) / RATE
    amp = rng.uniform(0.3, 1.0, 24) / np.arange(1, 25) ** 0.7
    sig = sum(a * np.sin(h * ph + rng.uniform(0, 2 * np.pi)) for h, a in zip(range(1, 25), amp))
    env = (0.5 + 0.5 * np.sin(2.0 * np.pi * rng.uniform(2.5, 4.0) * t + rng.uniform(0, 2 * np.pi))) ** 2 + 0.02
    out = env * (sig + noise * np.abs(sig).max() * rng.standard_normal(S))
    out *= peak / max(np.abs(out).max(), 1e-30)
    if quiet is not None:
        out[quiet[0] : quiet[1]] *= 1e-3
    return out.astype(np.float32)


def degrade(x: np.ndarray, seed: int, level: float) -> np.ndarray:
    """The "resynthesis": x plus white noise of ``level`` times x's RMS, a little gain off."""
    rng = np.random.default_rng(1000 + seed)
    rms = float(np.sqrt(np.mean(x.astype(np.float64) ** 2)))
    return (0.9 * x + level * rms * rng.standard_normal(len(x))).astype(np.float32)


# (S, seed, noise level of y, quiet stretch): the rows the GPU accuracy test meters, the CPU test derives the bound from and plants faults in
CASES = (
    (4700, 1, 0.3, (1100, 1700)),
    (6000, 2, 1.0, (0, 700)),
    (9001, 3, 0.3, (4000, 5000)),
    (9001, 4, 1.0, (8200, 9001)),
    (13000, 5, 0.3, (128 * FPB * 6 - 300, 128 * FPB * 6 + 500)),
    (20000, 6, 1.0, (7000, 8100)),
)
LONG = (300000, 9, 0.5, (100000, 130000))  # case len(CASES): one row that spans many workgroups of every kernel
T29 = (4700, 21, 0.3, (1000, 1800))  # 35 candidate frames, 30 kept: T = 29, no segment


@functools.lru_cache(maxsize=None)
def case(i: int):
    S, seed, level, quiet = (CASES + (LONG,))[i]
    x = make_speechlike(S, seed, quiet=quiet)
    return x, degrade(x, seed, level)


@functools.lru_cache(maxsize=None)
def case_reference(i: int):
    """(float64, float32) restatements of case ``i``."""
    x, y = case(i)
    return measure(x, y), measure(x, y, f32=True)


class Bounds(NamedTuple):
    scale_mags: float   # the float32 restatement's largest distance from float64 over the cases: band magnitudes, relative to the row's largest
    scale_series: float  # ... per-segment values
    scale_mean: float   # ... the two figures
    mags: float         # the bounds: BOUND_FACTOR x the scales
    series: float
    mean: float


@functools.lru_cache(maxsize=None)
def bounds() -> Bounds:
    sm = ss = sd = 0.0
    for i in range(len(CASES) + 1):
        a, b = case_reference(i)
        assert (a.n_frames, a.n_kept, a.n_segments) == (b.n_frames, b.n_kept, b.n_segments)
        sm = max(sm, float(np.abs(a.mags - b.mags).max() / a.mags.max()))
        ss = max(ss, float(np.abs(a.stoi_series - b.stoi_series).max()), float(np.abs(a.estoi_series - b.estoi_series).max()))
        sd = max(sd, abs(a.stoi - b.stoi), abs(a.estoi - b.estoi))
    return Bounds(sm, ss, sd, BOUND_FACTOR * sm, BOUND_FACTOR * ss, BOUND_FACTOR * sd)
