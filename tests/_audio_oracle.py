"""Plain numpy restatement of the audio stage's contract (include/vtts_audio.h): the prototype filter and the resampling sum in
fp64, evaluated for any window of outputs, and the kernel's arithmetic class in fp32 (fp32 taps, one fused multiply-add chain in
ascending n) whose error against fp64 is the GPU tests' yardstick.

    g = gcd(in, out), L = out / g, M = in / g, R = max(L, M), half = 24 R
    h[n] = L w[n] / sum(w),  w[n] = sinc(n / R) / R * kaiser(2 half + 1, 10)[n + half]
    y[m] = sum_n x[n] h[m M - n L + half],  n = max(0, ceil((m M - half) / L)) .. min(S - 1, floor((m M + half) / L))
"""
from __future__ import annotations

from math import gcd

import numpy as np

ZEROS = 24
BETA = 10.0


def ratio(in_rate: int, out_rate: int):
    """(L, M, half)"""
    g = gcd(int(in_rate), int(out_rate))
    L, M = int(out_rate) // g, int(in_rate) // g
    return L, M, ZEROS * max(L, M)


def prototype(in_rate: int, out_rate: int) -> np.ndarray:
    """h[-half .. half], float64."""
    L, M, half = ratio(in_rate, out_rate)
    R = max(L, M)
    n = np.arange(-half, half + 1, dtype=np.float64)
    w = np.sinc(n / R) / R * np.kaiser(2 * half + 1, BETA)
    return L * w / w.sum()


def out_samples(S: int, L: int, M: int) -> int:
    return -(-int(S) * L // M)


def response_db(h: np.ndarray, L: int, nfft: int):
    """(f, dB): the prototype's gain over its DC gain L at f = k / nfft cycles per sample of the rate L * in_rate, k = 0 .. nfft / 2."""
    H = np.abs(np.fft.rfft(h, nfft)) / L
    return np.arange(nfft // 2 + 1) / nfft, 20.0 * np.log10(np.maximum(H, 1e-300))


def _gather(x: np.ndarray, L: int, M: int, half: int, start: int, count: int):
    """For outputs m = start .. start + count - 1: tap indices k[m, j] = p + j L and sample indices n[m, j] = q - j (t = m M + half,
    q = t div L, p = t mod L), j = 0 .. ceil((2 half + 1) / L) - 1, with a mask of the pairs inside both the filter and the row."""
    S = x.shape[0]
    m = np.arange(start, start + count, dtype=np.int64)
    t = m * M + half
    q, p = t // L, t % L
    j = np.arange(-(-(2 * half + 1) // L), dtype=np.int64)
    k = p[:, None] + j[None, :] * L
    n = q[:, None] - j[None, :]
    ok = (k <= 2 * half) & (n >= 0) & (n < S)
    return np.where(ok, k, 0), np.where(ok, n, 0), ok


def resample(x, in_rate: int, out_rate: int, start: int = 0, count=None, dtype=np.float64) -> np.ndarray:
    """Outputs ``start .. start + count - 1`` (all of them by default) of one row ``x [S]``.

    ``dtype=np.float64``: the oracle.  ``dtype=np.float32``: fp32 samples and taps, accumulated in ascending n with one rounding to
    fp32 per step (the product of two fp32 numbers is exact in fp64, so ``float32(acc + x * h)`` computed in fp64 is fmaf up to a
    double rounding): the arithmetic class of the kernel."""
    x = np.asarray(x)
    assert x.ndim == 1
    L, M, half = ratio(in_rate, out_rate)
    h = prototype(in_rate, out_rate)
    So = out_samples(x.shape[0], L, M)
    if count is None:
        count = So - start
    assert 0 <= start and start + count <= So
    out = np.empty(count, dtype=dtype)
    step = 8192
    for c0 in range(0, count, step):
        c1 = min(count, c0 + step)
        k, n, ok = _gather(x, L, M, half, start + c0, c1 - c0)
        if np.dtype(dtype) == np.float64:
            out[c0:c1] = np.sum(np.where(ok, x[n].astype(np.float64) * h[k], 0.0), axis=1)
        else:
            xs = np.where(ok, x[n].astype(np.float32), np.float32(0)).astype(np.float64)
            hs = np.where(ok, h.astype(np.float32)[k], np.float32(0)).astype(np.float64)
            acc = np.zeros(c1 - c0, dtype=np.float32)
            for jj in range(k.shape[1] - 1, -1, -1):  # descending j = ascending n
                acc = (acc.astype(np.float64) + xs[:, jj] * hs[:, jj]).astype(np.float32)
            out[c0:c1] = acc
    return out


def speechlike(rng, S: int, rate: float = 16000.0) -> np.ndarray:
    """Harmonics of a random pitch under a slow envelope, peak 0.5, over a noise floor: float32 [S]."""
    t = np.arange(S) / rate
    f0 = rng.uniform(90.0, 250.0)
    x = sum(np.sin(2 * np.pi * f0 * k * t + rng.uniform(0, 2 * np.pi)) / k for k in range(1, 25))
    x *= 0.55 + 0.45 * np.sin(2 * np.pi * 3.0 * t + rng.uniform(0, 2 * np.pi))
    return (0.5 * x / np.abs(x).max() + rng.normal(0.0, 0.003, size=S)).astype(np.float32)
