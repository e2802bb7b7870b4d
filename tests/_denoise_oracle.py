"""include/vtts_denoise.h restated in numpy on top of tests/_stft_oracle.py.  ``cfg`` is ``(n_fft, win, hop, framing)``.

* ``denoise``: float64 throughout from the fp32 samples, the fp32 bias and the fp32 strength: the reference the kernel is compared with.
* the same with ``f32=True``: the float32 restatement, every operation of the contract rounded (``_stft_oracle.stft`` / ``istft`` in their
  float32 mode around ``gain_f32``).  NOT bit-exact with the kernel, whose transform is factored differently; its distance from the float64 mode
  is the error scale the GPU bound is derived from (BOUND_FACTOR x, the rule of tests/_spectral_oracle.py).
* ``gain_f32``: the contract's five lines on a complex64 spectrum in IEEE float32: what stands between ``Stft.forward`` and ``Stft.inverse`` in
  the bit-for-bit comparison.
* the same with ``fault=NAME``: one planted fault of FAULTS, for the test that the bound can see each of them.

``bias`` is ``[n_fft / 2 + 1]``, or ``[T, n_fft / 2 + 1]`` magnitudes of a noise recording's frames, of which frame 0 is the bias (the published
recipe takes the first frame of the vocoder's output for a zero mel); the fault ``bias_frame_1`` takes frame 1 and needs that form."""
from __future__ import annotations

import functools
import re
from pathlib import Path
from typing import Optional

import numpy as np

import _spectral_oracle as SO
import _stft_oracle as O

HEADER = Path(__file__).resolve().parents[1] / "include" / "vtts_denoise.h"
BOUND_FACTOR = O.BOUND_FACTOR
EPS = np.float32(1e-16)
STRENGTH = 0.5  # the tests' strength: not 1, so that its square is another number
FAULTS = ("subtract_after_clamp", "power_not_magnitude", "bias_frame_1", "no_clamp", "phase_dropped", "strength_squared", "descending_t")


def header_constants() -> dict:
    return {k: v for k, v in re.findall(r"#define\s+(VTTS_DENOISE_[A-Z_0-9]+)\s+([-+.e\d]+)\s", HEADER.read_text())}


def gain_f32(spec, bias, strength) -> np.ndarray:
    """[T, NB] complex64 -> complex64: r = sqrt(re^2 + im^2); m = max(r - strength bias, 0); c' = m (c / (r + 1e-16)), each operation float32."""
    spec = np.asarray(spec)
    assert spec.dtype == np.complex64, spec.dtype
    re_, im = np.ascontiguousarray(spec.real), np.ascontiguousarray(spec.imag)
    sb = np.float32(strength) * np.asarray(bias, dtype=np.float32)
    r = np.sqrt(re_ * re_ + im * im)
    m = np.maximum(r - sb[None, :], np.float32(0.0))
    d = r + EPS
    out = np.empty(spec.shape, np.complex64)
    out.real, out.imag = m * (re_ / d), m * (im / d)
    assert r.dtype == m.dtype == d.dtype == np.float32
    return out


def _gain(c, bias, strength, f32: bool, fault: Optional[str]):
    if f32 and fault is None:
        return gain_f32(c, bias, strength)
    dt = np.float32 if f32 else np.float64
    s = dt(np.float32(strength))
    sb = (s * s if fault == "strength_squared" else s) * np.asarray(bias, dtype=np.float32).astype(dt)[None, :]
    re_, im = c.real.astype(dt), c.imag.astype(dt)
    r = np.sqrt(re_ * re_ + im * im)
    if fault == "power_not_magnitude":  # the root forgotten: the subtraction and the quotient see the power
        r = re_ * re_ + im * im
    if fault == "subtract_after_clamp":
        m = np.maximum(r, dt(0.0)) - sb
    elif fault == "no_clamp":
        m = r - sb
    else:
        m = np.maximum(r - sb, dt(0.0))
    d = r + dt(EPS)
    out = np.empty(c.shape, c.dtype)
    if fault == "phase_dropped":
        out.real, out.imag = m, dt(0.0)
    else:
        out.real, out.imag = m * (re_ / d), m * (im / d)
    return out


def denoise(x, bias, strength, cfg, f32: bool = False, fault: Optional[str] = None) -> np.ndarray:
    """[S] float32 (or int16) -> [S] float64 (float32 with f32)."""
    assert fault is None or fault in FAULTS, fault
    bias = np.asarray(bias, dtype=np.float32)
    if fault == "bias_frame_1":
        assert bias.ndim == 2, "bias_frame_1 needs the noise recording's frames"
        bias = bias[1]
    elif bias.ndim == 2:
        bias = bias[0]
    assert bias.shape == (cfg[0] // 2 + 1,) and (bias >= 0).all() and np.isfinite(bias).all() and strength >= 0
    x = SO.as_float32(np.asarray(x))
    c = O.stft(x, cfg, f32)
    return O.istft(_gain(c, bias, strength, f32, fault), len(x), cfg, f32, fault="descending_t" if fault == "descending_t" else None)


def bias_from_noise(rows, cfg) -> np.ndarray:
    """The mean over all frames of all rows of r, the contract's float32 magnitude of the float32 spectrum given per row, summed in float64."""
    tot, n = np.zeros(cfg[0] // 2 + 1), 0
    for c in rows:
        c = np.asarray(c)
        assert c.dtype == np.complex64
        re_, im = np.ascontiguousarray(c.real), np.ascontiguousarray(c.imag)
        tot += np.sqrt(re_ * re_ + im * im).astype(np.float64).sum(axis=0)
        n += c.shape[0]
    return tot / n


# ------------------------------------------------------------ inputs and bounds ------------------------------------------------------------
def rows(cfg):
    """The indices of _stft_oracle.ROWS the config accepts."""
    return [i for i in range(len(O.ROWS)) if O.ROWS[i][0] >= O.min_samples(cfg)]


@functools.lru_cache(maxsize=None)
def smooth_bias(cfg) -> np.ndarray:
    """A smooth positive profile with STRENGTH x bias around the median magnitude of the speech-like rows' bins (0.5 x to 1.5 x across the
    band): a real share of the bins clamps to zero and a real share does not."""
    med = float(np.median(np.concatenate([np.abs(O.stft(O.wave_case(i), cfg)).ravel() for i in rows(cfg)])))
    f = np.arange(cfg[0] // 2 + 1) / (cfg[0] // 2)
    return (med / STRENGTH * (1.0 + 0.5 * np.cos(np.pi * f))).astype(np.float32)


def zero_bias(cfg) -> np.ndarray:
    return np.zeros(cfg[0] // 2 + 1, np.float32)


def clamping_bias(cfg) -> np.ndarray:
    """So large that every bin clamps: a sample of at most 1 gives a bin of at most n_fft."""
    return np.full(cfg[0] // 2 + 1, 1e6, np.float32)


def clamped_share(x, bias, strength, cfg) -> float:
    c = O.stft(x, cfg)
    return float((np.abs(c) <= float(np.float32(strength)) * np.asarray(bias, np.float64)[None, :]).mean())


@functools.lru_cache(maxsize=None)
def noise_frames(cfg) -> np.ndarray:
    """[T, NB] float32 magnitudes of a faint hum and hiss, what a vocoder gives for an empty mel: frame 0 is the recipe's bias."""
    S = max(4 * cfg[0], O.min_samples(cfg))
    rng = np.random.default_rng(77)
    n = np.arange(S)
    y = (0.01 * np.sin(2 * np.pi * 0.031 * n) + 0.004 * rng.standard_normal(S)).astype(np.float32)
    scale = float(smooth_bias(cfg).mean())
    m = np.abs(O.stft(y, cfg))
    return (m * (scale / m.mean())).astype(np.float32)


@functools.lru_cache(maxsize=None)
def want(i: int, cfg) -> np.ndarray:
    """The float64 reference of row i under the smooth bias at the tests' strength, computed once."""
    return denoise(O.wave_case(i), smooth_bias(cfg), STRENGTH, cfg)


@functools.lru_cache(maxsize=None)
def bound(cfg):
    """(scale, bound): the float32 restatement's largest relative distance from float64 over ROWS, and BOUND_FACTOR x it."""
    s = max(O.rel(denoise(O.wave_case(i), smooth_bias(cfg), STRENGTH, cfg, f32=True), want(i, cfg)) for i in rows(cfg))
    return s, BOUND_FACTOR * s


@functools.lru_cache(maxsize=None)
def round_trip_bound(cfg):
    """BOUND_FACTOR x the float32 restatement's round trip error over ROWS, relative to the row's peak (tests/test_gpu_stft.py's rule)."""
    s = max(O.rel(O.istft(O.stft(O.wave_case(i), cfg, f32=True), O.ROWS[i][0], cfg, f32=True), O.wave_case(i).astype(np.float64)) for i in rows(cfg))
    return s, BOUND_FACTOR * s
