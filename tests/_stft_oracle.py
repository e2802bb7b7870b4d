"""include/vtts_stft.h restated in numpy, for both framings.  ``cfg`` is ``(n_fft, win, hop, framing)`` with framing "center" or "mel".

* ``stft`` / ``istft`` / ``project`` / ``griffinlim``: float64 throughout, from the fp32 samples (or spectra) and the fp32 window the header
  defines.  These are the references the kernels are compared with.
* the same with ``f32=True``: window products, transforms (``scipy.fft`` keeps single precision), overlap-add sums, quotient and the projection's
  arithmetic in float32.  They are NOT bit-exact with the kernels, whose transform is factored differently; their distance from the float64 mode
  is the error scale every GPU bound is derived from (BOUND_FACTOR x, the rule of tests/_spectral_oracle.py).
* the same with ``fault=NAME``: one planted fault of FAULTS, for the test that the bounds can see each of them.

and the inputs and bounds the CPU and GPU tests share."""
from __future__ import annotations

import functools
import re
from pathlib import Path
from typing import Optional

import numpy as np
import scipy.fft

import _spectral_oracle as SO

HEADER = Path(__file__).resolve().parents[1] / "include" / "vtts_stft.h"
BOUND_FACTOR = SO.BOUND_FACTOR
NOLA_FLOOR = 1e-11
# the issue's resolutions (n_fft, win, hop): win == n_fft and win < n_fft, hops that divide n_fft and hops that do not
RESOLUTIONS = ((256, 256, 64), (512, 240, 50), (1024, 1024, 256), (1024, 600, 120), (2048, 1200, 240))
FRAMINGS = ("center", "mel")
CFGS = tuple(r + (f,) for r in RESOLUTIONS for f in FRAMINGS)
# descending_t: the frames are overlap-added in descending order, frame t where frame T - 1 - t belongs (the order of a float64 SUM alone
# moves nothing a bound could see).  frames_off_by_one: T of S - 1 samples, which differs exactly where S is a multiple of hop.
INVERSE_FAULTS = ("descending_t", "envelope_w", "no_scale", "bin0_imag", "frames_off_by_one")
FORWARD_FAULTS = ("reflect_off_by_one", "wrong_framing_pad", "frames_off_by_one")
PROJECT_FAULTS = ("momentum_on_c",)
FAULTS = INVERSE_FAULTS + FORWARD_FAULTS[:2] + PROJECT_FAULTS


def header_constants() -> dict:
    return {k: v for k, v in re.findall(r"#define\s+(VTTS_STFT_[A-Z_0-9]+)\s+([-+.e\d]+)\s", HEADER.read_text())}


def window(cfg) -> np.ndarray:
    return SO.window(cfg[:3])


def pad(cfg) -> int:
    n_fft, _, hop, framing = cfg
    assert framing in FRAMINGS, framing
    return (n_fft - hop) // 2 if framing == "mel" else n_fft // 2


def num_frames(S: int, cfg) -> int:
    return (S + 2 * pad(cfg) - cfg[0]) // cfg[2] + 1


def num_samples(T: int, cfg) -> int:
    """The smallest S with T frames."""
    return (T - 1) * cfg[2] + cfg[0] - 2 * pad(cfg)


def min_samples(cfg) -> int:
    return max(pad(cfg) + 1, cfg[0] - 2 * pad(cfg))


def _other(cfg):
    return cfg[:3] + ("mel" if cfg[3] == "center" else "center",)


def frame_index(S: int, cfg, fault: Optional[str] = None) -> np.ndarray:
    """[T, n_fft] row-sample indices: frame t covers padded samples [hop t, hop t + n_fft), padded sample p is row sample p - P, reflected."""
    n_fft, _, hop, _ = cfg
    assert S >= min_samples(cfg), (S, cfg)
    P = pad(_other(cfg)) if fault == "wrong_framing_pad" else pad(cfg)
    T = num_frames(S - 1, cfg) if fault == "frames_off_by_one" else num_frames(S, cfg)
    g = hop * np.arange(T)[:, None] + np.arange(n_fft)[None, :] - P
    if fault == "reflect_off_by_one":
        g = np.where(g < 0, -g - 1, g)
        g = np.where(g >= S, 2 * S - 1 - g, g)
    else:
        g = np.where(g < 0, -g, g)
        g = np.where(g >= S, 2 * (S - 1) - g, g)
    return np.clip(g, 0, S - 1)


def stft(x, cfg, f32: bool = False, fault: Optional[str] = None) -> np.ndarray:
    """[S] float32 (or int16) -> [T, n_fft / 2 + 1] complex128 (complex64 with f32).  A float64 row (the float64 Griffin-Lim loop's own
    waveform between two of its steps) is taken as it is."""
    assert fault is None or fault in FORWARD_FAULTS, fault
    x = np.asarray(x)
    x = x if x.dtype == np.float64 and not f32 else SO.as_float32(x)
    dt = np.float32 if f32 else np.float64
    v = x[frame_index(len(x), cfg, fault)].astype(dt) * window(cfg).astype(dt)[None, :]
    z = scipy.fft.rfft(v, axis=-1)
    assert z.dtype == (np.complex64 if f32 else np.complex128)
    return z


def istft(spec, S: int, cfg, f32: bool = False, fault: Optional[str] = None) -> np.ndarray:
    """[>= T, n_fft / 2 + 1] complex64 -> [S] float64 (float32 with f32): the header's steps 1 to 3."""
    assert fault is None or fault in INVERSE_FAULTS, fault
    n_fft, _, hop, _ = cfg
    H, P = n_fft // 2, pad(cfg)
    dt, cdt = (np.float32, np.complex64) if f32 else (np.float64, np.complex128)
    T = num_frames(S - 1, cfg) if fault == "frames_off_by_one" else num_frames(S, cfg)
    X = np.asarray(spec)[:T].astype(cdt)
    X0 = X.copy()
    X0[:, 0], X0[:, H] = X0[:, 0].real, X0[:, H].real
    v = scipy.fft.irfft(X0, n_fft, axis=-1, norm="forward")  # unscaled
    assert v.dtype == dt
    if fault == "bin0_imag":  # what the inverse split step gives when the two imaginary parts are not dropped
        v[:, 0::2] -= (X[:, 0].imag + X[:, H].imag)[:, None]
        v[:, 1::2] += (X[:, 0].imag - X[:, H].imag)[:, None]
    w = window(cfg).astype(dt)
    ww = w if fault == "envelope_w" else w * w
    y, e = np.zeros(max(hop * (T - 1) + n_fft, P + S), dt), np.zeros(max(hop * (T - 1) + n_fft, P + S), dt)
    for t in range(T):  # ascending: each sample's sums gain their terms in this order
        at = hop * (T - 1 - t if fault == "descending_t" else t)
        y[at : at + n_fft] += v[t] * w
        e[at : at + n_fft] += ww
    with np.errstate(divide="ignore", invalid="ignore"):
        out = y[P : P + S] / e[P : P + S]
    return out if fault == "no_scale" else out * dt(1.0 / n_fft)


def alpha_of(momentum: float, f32: bool):
    m = np.float32(momentum)
    return m / (np.float32(1.0) + m) if f32 else float(m) / (1.0 + float(m))


def project(x, mag, tprev, momentum: float, cfg, f32: bool = False, fault: Optional[str] = None):
    """-> (spec, c): c = stft(x); a = c - alpha tprev; spec = mag a / (|a| + 1e-16).  The new tprev is c."""
    assert fault is None or fault in PROJECT_FAULTS, fault
    c = stft(x, cfg, f32)
    T = c.shape[0]
    dt = np.float32 if f32 else np.float64
    al = alpha_of(momentum, f32)
    tp = (c if fault == "momentum_on_c" else np.asarray(tprev)[:T]).astype(c.dtype)
    ar, ai = c.real - al * tp.real, c.imag - al * tp.imag
    d = np.sqrt(ar * ar + ai * ai) + dt(1e-16)
    mg = np.asarray(mag)[:T].astype(dt)
    out = np.empty(c.shape, c.dtype)
    out.real, out.imag = mg * (ar / d), mg * (ai / d)
    assert ar.dtype == dt and out.dtype == c.dtype
    return out, c


def griffinlim(mag, S: int, cfg, n_iter: int, momentum: float, init, f32: bool = False) -> np.ndarray:
    """torchaudio's fast Griffin-Lim from the given unit phases: n_iter x (istft, project) and a final istft."""
    cdt = np.complex64 if f32 else np.complex128
    T = num_frames(S, cfg)
    mag = np.asarray(mag)[:T].astype(np.float32)
    spec = (mag.astype(cdt) * np.asarray(init)[:T].astype(cdt)).astype(cdt)
    tprev = np.zeros_like(spec)
    for _ in range(n_iter):
        wav = istft(spec, S, cfg, f32)
        spec, tprev = project(wav, mag, tprev, momentum, cfg, f32)
    return istft(spec, S, cfg, f32)


def min_envelope(S: int, cfg) -> float:
    """min over the S output samples of sum_t w^2, every sample visited, in float64 from the fp32 window."""
    n_fft, _, hop, _ = cfg
    P, T = pad(cfg), num_frames(S, cfg)
    w2 = window(cfg).astype(np.float64) ** 2
    e = np.zeros(max(hop * (T - 1) + n_fft, P + S))
    for t in range(T):
        e[hop * t : hop * t + n_fft] += w2
    return float(e[P : P + S].min())


# ------------------------------------------------------------ inputs and bounds ------------------------------------------------------------
ROWS = ((1100, 1), (1300, 7), (1700, 8), (2049, 2), (4700, 3))  # (S, seed): several rows, so that a scale is not one draw


@functools.lru_cache(maxsize=None)
def wave_case(i: int) -> np.ndarray:
    S, seed = ROWS[i]
    return SO.make_speechlike(S, seed)


@functools.lru_cache(maxsize=None)
def spec_case(i: int, cfg) -> np.ndarray:
    """A random complex spectrum of ROWS[i]'s frame count: nothing Hermitian about bins 0 and H, nothing consistent between frames."""
    T = num_frames(ROWS[i][0], cfg)
    rng = np.random.default_rng(500 + i)
    return (rng.standard_normal((T, cfg[0] // 2 + 1)) + 1j * rng.standard_normal((T, cfg[0] // 2 + 1))).astype(np.complex64)


def rel(got, want) -> float:
    """The largest distance relative to the reference's largest absolute value."""
    return float(np.abs(np.asarray(got) - want).max() / np.abs(want).max())


@functools.lru_cache(maxsize=None)
def forward_bound(cfg):
    """(scale, bound): the float32 restatement's largest relative distance from float64 over ROWS, and BOUND_FACTOR x it."""
    s = max(rel(stft(wave_case(i), cfg, f32=True), stft(wave_case(i), cfg)) for i in range(len(ROWS)) if ROWS[i][0] >= min_samples(cfg))
    return s, BOUND_FACTOR * s


@functools.lru_cache(maxsize=None)
def inverse_bound(cfg):
    s = max(rel(istft(spec_case(i, cfg), ROWS[i][0], cfg, f32=True), istft(spec_case(i, cfg), ROWS[i][0], cfg)) for i in range(len(ROWS)) if ROWS[i][0] >= min_samples(cfg))
    return s, BOUND_FACTOR * s


def project_limit(mag, a64, tprev, c64, cfg) -> np.ndarray:
    """Per bin, how far a projection may lie from the float64 one.  The phase of a is ill-conditioned where |a| is tiny: an error eps in a
    turns it by eps / |a|, and by no more than 2 (two unit vectors).  eps = the forward bound on c (relative to the row's largest |c|) plus the
    fp32 product and difference of a = c - alpha tprev (2 roundings of 2^-24 relative to |tprev| and |c|: 2^-22 of the larger covers both);
    the quotient, the product with mag, the square root and the sum under it are 8 more roundings relative to mag."""
    eps = forward_bound(cfg)[1] * np.abs(c64).max() + 2.0 ** -22 * max(np.abs(tprev).max(), np.abs(c64).max())
    with np.errstate(divide="ignore"):
        turn = np.minimum(2.0, eps / np.abs(a64))
    return mag.astype(np.float64) * (turn + 8.0 * 2.0 ** -24)
