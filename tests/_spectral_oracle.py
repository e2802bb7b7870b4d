"""include/vtts_spectral.h restated in numpy:

* ``measure(x, y, cfg)``: float64 throughout, from the fp32 samples and the fp32 window the header defines.  This is the reference the kernel
  is compared with.
* ``measure(x, y, cfg, f32=True)``: window products, transform (``scipy.fft.rfft`` keeps single precision), powers and magnitudes in float32;
  the terms and their sums in float64, as the header has them.  It is NOT bit-exact with the kernel, whose transform is factored differently;
  its distance from the float64 mode is the error scale the GPU test derives its bound from.
* ``measure(x, y, cfg, fault=NAME)``: one planted fault of FAULTS, for the test that the bounds can see each of them.

and the resolutions, inputs and bounds the CPU and GPU tests share.  ``cfg`` is ``(n_fft, win, hop)``."""
from __future__ import annotations

import functools
import re
from pathlib import Path
from typing import NamedTuple, Optional

import numpy as np
import scipy.fft

HEADER = Path(__file__).resolve().parents[1] / "include" / "vtts_spectral.h"

RATE = 16000
P_FLOOR = 1e-7
N_FFTS = (256, 512, 1024, 2048)
# one resolution per transform length: Parallel WaveGAN's three and a short one; win < n_fft in all, hops that divide no n_fft (50, 120, 240)
RESOLUTIONS = {256: (256, 160, 40), 512: (512, 240, 50), 1024: (1024, 600, 120), 2048: (2048, 1200, 240)}
DEFAULTS = (RESOLUTIONS[1024], RESOLUTIONS[2048], RESOLUTIONS[512])
FAULTS = ("symmetric_hann", "window_not_centred", "zero_padding", "frames_minus_one", "clamp_on_m", "sc_by_y", "no_nyquist", "log10_logmag")
BOUND_FACTOR = 8.0  # the issue's: every bound is 8 x the float32 restatement's distance from float64 over the cases


def header_constants() -> dict:
    return {k: int(v) for k, v in re.findall(r"#define\s+(VTTS_SPECTRAL_[A-Z_0-9]+)\s+(\d+)\s", HEADER.read_text())}


K = header_constants()


class Spectral(NamedTuple):
    sc: float
    logmag: float
    lsd: float
    n_frames: int
    mags: np.ndarray  # [2, T, n_fft / 2 + 1]: Mx, then My


def window(cfg, fault: Optional[str] = None) -> np.ndarray:
    """[n_fft] float32: the periodic Hann of ``win`` computed in double and rounded once, (n_fft - win) // 2 zeros in front."""
    n_fft, win, _ = cfg
    r = np.arange(win, dtype=np.float64)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * r / (win - 1 if fault == "symmetric_hann" else win))
    out = np.zeros(n_fft, np.float32)
    lead = 0 if fault == "window_not_centred" else (n_fft - win) // 2
    out[lead : lead + win] = w.astype(np.float32)
    return out


def num_frames(S: int, cfg) -> int:
    return 1 + S // cfg[2]


def min_samples(cfg) -> int:
    return cfg[0] // 2 + 1


def lds_bytes(cfg, F: int) -> int:
    """The header's table."""
    n_fft, _, hop = cfg
    H = n_fft // 2
    span = (F - 1) * hop + n_fft
    return 32 * F + 8 * H + 8 * (H // 2 + 2) + 2 * 4 * (span + span % 2) + 8 * F * (H + H // 8)


def frames_per_block(cfg) -> int:
    F = K["VTTS_SPECTRAL_MAX_FRAMES_PER_BLOCK_2048"] if cfg[0] == 2048 else K["VTTS_SPECTRAL_MAX_FRAMES_PER_BLOCK"]
    while F > 1 and lds_bytes(cfg, F) > K["VTTS_SPECTRAL_LDS_BUDGET"]:
        F -= 1
    return F


def as_float32(x) -> np.ndarray:
    x = np.asarray(x)
    if x.dtype == np.int16:
        return x.astype(np.float32) * np.float32(2.0 ** -15)  # exact
    assert x.dtype == np.float32, x.dtype
    return x


def frame_samples(x: np.ndarray, cfg, fault: Optional[str] = None) -> np.ndarray:
    """[T, n_fft] of the row's own samples: frame t covers padded samples [hop t, hop t + n_fft)."""
    n_fft, _, hop = cfg
    S = len(x)
    assert S >= min_samples(cfg), (S, cfg)
    T = num_frames(S, cfg) - (1 if fault == "frames_minus_one" else 0)
    g = hop * np.arange(T)[:, None] + np.arange(n_fft)[None, :] - n_fft // 2
    if fault == "zero_padding":
        return np.where((g >= 0) & (g < S), x[np.clip(g, 0, S - 1)], x.dtype.type(0))
    g = np.where(g < 0, -g, g)
    g = np.where(g >= S, 2 * (S - 1) - g, g)
    return x[g]


def powers(x: np.ndarray, cfg, f32: bool = False, fault: Optional[str] = None):
    """(P, M), each [T, n_fft / 2 + 1] in float32 or float64."""
    dt = np.float32 if f32 else np.float64
    v = frame_samples(x, cfg, fault).astype(dt) * window(cfg, fault).astype(dt)[None, :]
    z = scipy.fft.rfft(v, axis=-1)
    assert z.dtype == (np.complex64 if f32 else np.complex128)
    p = z.real * z.real + z.imag * z.imag
    if fault == "clamp_on_m":
        m = np.maximum(np.sqrt(p), dt(P_FLOOR))
        return m * m, m
    p = np.maximum(p, dt(P_FLOOR))
    return p, np.sqrt(p)


def measure(x, y, cfg, f32: bool = False, fault: Optional[str] = None) -> Spectral:
    assert fault is None or fault in FAULTS, fault
    x, y = as_float32(x), as_float32(y)
    assert x.shape == y.shape and x.ndim == 1
    (px, mx), (py, my) = powers(x, cfg, f32, fault), powers(y, cfg, f32, fault)
    mags = np.stack([mx, my])
    px, mx, py, my = (a.astype(np.float64) for a in (px, mx, py, my))  # the terms and their sums are fp64 in every mode
    if fault == "no_nyquist":
        px, mx, py, my = (a[:, :-1] for a in (px, mx, py, my))
    T, nb = px.shape
    L = np.log(py / px)
    sc = float(np.sqrt(((my - mx) ** 2).sum()) / np.sqrt(((my if fault == "sc_by_y" else mx) ** 2).sum()))
    logmag = float((0.5 * np.abs(L) / (np.log(10.0) if fault == "log10_logmag" else 1.0)).sum() / (T * nb))
    lsd = float(np.sqrt(((10.0 / np.log(10.0) * L) ** 2).sum(axis=1) / nb).sum() / T)
    return Spectral(sc, logmag, lsd, T, mags)


# ------------------------------------------------------------ inputs ------------------------------------------------------------
def make_speechlike(S: int, seed: int, noise: float = 0.02, quiet=None, peak: float = 0.5) -> np.ndarray:
    """``S`` samples at 16 kHz, float32, after tests/_stoi_oracle.py: a harmonic stack on a moving F0 under a 2.5 - 4 Hz envelope, plus
    envelope-shaped noise, so that few bins sit at the 1e-7 clamp.  ``quiet = (start, stop)`` scales that stretch by 1e-3: there the bins DO
    sit at the clamp (the clamp's place, on P or on M, shows only there)."""
    rng = np.random.default_rng(seed)
    t = np.arange(S) / RATE
    f0 = 140.0 + 40.0 * np.sin(2.0 * np.pi * 0.7 * t + rng.uniform(0, 2 * np.pi)) + 15.0 * np.sin(2.0 * np.pi * 2.3 * t + rng.uniform(0, 2 * np.pi))
    ph = 2.0 * np.pi * np.cumsum(f0) / RATE
    amp = rng.uniform(0.3, 1.0, 40) / np.arange(1, 41) ** 0.7
    sig = sum(a * np.sin(h * ph + rng.uniform(0, 2 * np.pi)) for h, a in zip(range(1, 41), amp))
    env = (0.5 + 0.5 * np.sin(2.0 * np.pi * rng.uniform(2.5, 4.0) * t + rng.uniform(0, 2 * np.pi))) ** 2 + 0.02
    out = env * (sig + noise * np.abs(sig).max() * rng.standard_normal(S))
    out *= peak / max(np.abs(out).max(), 1e-30)
    if quiet is not None:
        out[quiet[0] : quiet[1]] *= 1e-3
    return out.astype(np.float32)


def degrade(x: np.ndarray, seed: int, level: float) -> np.ndarray:
    """The "resynthesis": x a little gain off, plus white noise of ``level`` times x's RMS."""
    rng = np.random.default_rng(1000 + seed)
    rms = float(np.sqrt(np.mean(x.astype(np.float64) ** 2)))
    return (0.9 * x + level * rms * rng.standard_normal(len(x))).astype(np.float32)


# (S, seed, noise level of y, quiet stretch): the rows the GPU accuracy test meters, the CPU test derives the bounds from and plants faults in.
# A figure is a mean over the row's bins, and its fp32 error is what is left of the bins' errors after that mean: on a row of a dozen frames
# it is one draw of wide spread.  Three rows are that short, so that the scale (the largest distance over the cases) is not a single draw.
CASES = (
    (1100, 1, 0.3, None),
    (1300, 7, 0.5, None),
    (1700, 8, 0.2, None),
    (2049, 2, 1.0, None),
    (4700, 3, 0.3, (1500, 2600)),
    (9001, 4, 1.0, None),
    (13000, 5, 0.1, (6000, 9000)),
    (20000, 6, 0.5, None),
)
LONG = (300000, 9, 0.3, (100000, 130000))  # case len(CASES): one row that spans many workgroups
N_CASES = len(CASES) + 1


@functools.lru_cache(maxsize=None)
def case(i: int):
    S, seed, level, quiet = (CASES + (LONG,))[i]
    x = make_speechlike(S, seed, quiet=quiet)
    return x, degrade(x, seed, level)


@functools.lru_cache(maxsize=None)
def case_reference(i: int, cfg):
    """(float64, float32) restatements of case ``i`` at ``cfg``."""
    x, y = case(i)
    return measure(x, y, cfg), measure(x, y, cfg, f32=True)


class Bounds(NamedTuple):
    scale_sc: float      # the float32 restatement's largest distance from float64 over the cases
    scale_logmag: float
    scale_lsd: float
    scale_mags: float    # ... relative to the row's largest magnitude
    sc: float            # the bounds: BOUND_FACTOR x the scales
    logmag: float
    lsd: float
    mags: float


@functools.lru_cache(maxsize=None)
def bounds(cfg) -> Bounds:
    s = [0.0, 0.0, 0.0, 0.0]
    for i in range(N_CASES):
        a, b = case_reference(i, cfg)
        assert a.n_frames == b.n_frames
        s[0] = max(s[0], abs(a.sc - b.sc))
        s[1] = max(s[1], abs(a.logmag - b.logmag))
        s[2] = max(s[2], abs(a.lsd - b.lsd))
        s[3] = max(s[3], float(np.abs(a.mags - b.mags).max() / a.mags.max()))
    return Bounds(*s, *(BOUND_FACTOR * v for v in s))


def misses(want: Spectral, got, b: Bounds) -> dict:
    """By how many bounds each figure of ``got`` (anything with sc, logmag, lsd) lies from ``want``."""
    return {"sc": abs(got.sc - want.sc) / b.sc, "logmag": abs(got.logmag - want.logmag) / b.logmag, "lsd": abs(got.lsd - want.lsd) / b.lsd}
