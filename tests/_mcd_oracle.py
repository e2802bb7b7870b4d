"""include/vtts_mcd.h restated in numpy float32, operation for operation (what the GPU results are compared against with ``==``), a float64
oracle whose cepstra come from ``scipy.fft.dct(type=2, norm="ortho")[..., 1 : K + 1]``, and the bound between the two.

The recurrence, band and backtrace are tests/_dtw_oracle.py's ``accumulate`` / ``backtrace``, by import: only the local cost differs.

The bound (u = 2^-24, gamma_n = n u / (1 - n u); every input finite and no square underflowing):

* cepstrum.  The table is the exact basis rounded once (relative u); the chain of M products and M - 1 additions in ascending m has the
  textbook dot-product error.  Together  |c32[t, k] - c[t, k]| <= gamma_(M+2) S[t, k],  S[t, k] = sum_m |dct[k][m] x[t, m]|  (``ec`` below).
* difference.  e32_k = fl(ca32_k - cb32_k):  |e32_k - e_k| <= E_k = ec_a[k] + ec_b[k] + u |e32_k|.
* distance.  The chain s = s + e e is a dot product of e32 with itself: s32 = |e32|^2 (1 + t), |t| <= gamma_(K+1); the correctly rounded
  root adds u.  With the triangle inequality | |e32| - |e| | <= |E|_2:   |d32 - d| <= B_d = |E|_2 + gamma_(K+2) d32.
* aligned MCD.  alpha / L times the sum of the B_d (the float64 sum of L <= 2^31 values adds less than L 2^-53 relative: counted as one more u).
* DTW total.  Rounding to fp32 is monotone, so the fp32 recurrence gives min over paths of the path's left-to-right fp32 sum; a path of
  P <= la + lb - 1 cells sums to within  P max B_d + gamma_P P max d32  of its exact sum, and two minima over the same paths differ by at
  most the largest difference of a path:  |total32 - total| <= B_total = (la + lb - 1) (max B_d + gamma_(la+lb) max d32).
  MCD-DTW = alpha total / path_len is compared where the two optimal paths have one length (asserted by the tests that use it).
"""
from __future__ import annotations

import math
import re
from pathlib import Path

import numpy as np

import _dtw_oracle as DO

HEADER = Path(__file__).resolve().parents[1] / "include" / "vtts_mcd.h"
ALPHA = 10.0 * math.sqrt(2.0) / math.log(10.0)
U = 2.0 ** -24


def header_constants() -> dict:
    """Every ``#define VTTS_MCD_* <number>`` of the header."""
    return {m.group(1): float(m.group(2)) if "." in m.group(2) else int(m.group(2))
            for m in re.finditer(r"^#define\s+(VTTS_MCD_\w+)\s+([0-9.]+)\s*$", HEADER.read_text(), re.M)}


def gamma(n: int) -> float:
    return n * U / (1.0 - n * U)


def basis(M: int, K: int, first: int = 1, normalised: bool = True) -> np.ndarray:
    """dct[k][m], k = first .. first + K - 1, in double (the header's expression, left to right, libm's cos) rounded once to float32."""
    scale = math.sqrt(2.0 / M) if normalised else 2.0
    return np.array([[scale * math.cos(math.pi * k * (2 * m + 1) / (2.0 * M)) for m in range(M)] for k in range(first, first + K)], dtype=np.float32)


def cepstra_f32(x: np.ndarray, table: np.ndarray) -> np.ndarray:
    """c[t, k]: one float32 chain in ascending m, product and sum each rounded."""
    x = np.asarray(x, dtype=np.float32)
    s = np.zeros((x.shape[0], table.shape[0]), dtype=np.float32)
    for m in range(x.shape[1]):
        s = s + table[None, :, m] * x[:, m, None]
    return s


def cost_f32(ca: np.ndarray, cb: np.ndarray, root: bool = True) -> np.ndarray:
    """d[i, j]: one float32 chain in ascending k of (ca - cb)^2, then the correctly rounded root."""
    s = np.zeros((ca.shape[0], cb.shape[0]), dtype=np.float32)
    for k in range(ca.shape[1]):
        e = ca[:, None, k] - cb[None, :, k]
        s = s + e * e
    return np.sqrt(s) if root else s


def frames_f32(ca: np.ndarray, cb: np.ndarray, root: bool = True) -> np.ndarray:
    """d(t, t) over the frames both hold."""
    L = min(len(ca), len(cb))
    s = np.zeros((L,), dtype=np.float32)
    for k in range(ca.shape[1]):
        e = ca[:L, k] - cb[:L, k]
        s = s + e * e
    return np.sqrt(s) if root else s


def aligned_sum(d: np.ndarray, block: int) -> float:
    """The header's order: blocks of ``block`` frames, each added in ascending t from 0.0, the blocks' sums in ascending order from 0.0."""
    total = 0.0
    for t0 in range(0, len(d), block):
        s = 0.0
        for v in d[t0 : t0 + block]:
            s = s + float(v)
        total = total + s
    return total


def mcd_aligned_f32(a, b, L=None, K: int = 13, block: int = 64, table=None, root: bool = True, alpha: float = ALPHA):
    """(MCD in dB as a Python float, d [L] float32, the float64 sum) of the contract; ``table`` / ``root`` / ``alpha`` plant faults."""
    L = min(len(a), len(b)) if L is None else L
    table = basis(a.shape[1], K) if table is None else table
    d = frames_f32(cepstra_f32(a[:L], table), cepstra_f32(b[:L], table), root)
    s = aligned_sum(d, block)
    return (alpha * s / L if L else float("nan")), d, s


def mcd_dtw_f32(a, b, K: int = 13, band: int = 0, table=None, root: bool = True):
    """(total float32, path_len, span) of the contract."""
    table = basis(a.shape[1], K) if table is None else table
    D, codes = DO.accumulate(cost_f32(cepstra_f32(a, table), cepstra_f32(b, table), root), band)
    n, span = DO.backtrace(codes)
    return D[-1, -1], n, span


def dtw_cells_f32(ca: np.ndarray, cb: np.ndarray, band: int = 0):
    """The contract cell by cell over cepstra, as the headers word it (small sizes: Python loops)."""
    la, lb, K = len(ca), len(cb), ca.shape[1]
    inf = np.float32(np.inf)
    D = np.full((la, lb), inf, dtype=np.float32)
    codes = np.zeros((la, lb), dtype=np.uint8)
    for i in range(la):
        for j in range(lb):
            if not bool(DO.in_band(i, j, la, lb, band)):
                continue
            s = np.float32(0.0)
            for k in range(K):
                e = np.float32(ca[i, k] - cb[j, k])
                s = np.float32(s + np.float32(e * e))
            c = np.sqrt(s)
            if i == 0 and j == 0:
                D[0, 0] = c
                continue
            best, code = (D[i - 1, j - 1] if i and j else inf), DO.DIAG
            up = D[i - 1, j] if i else inf
            left = D[i, j - 1] if j else inf
            if up < best:
                best, code = up, DO.UP
            if left < best:
                best, code = left, DO.LEFT
            D[i, j] = np.float32(c + best)
            codes[i, j] = code
    n, span = DO.backtrace(codes)
    return D[-1, -1], n, span


# ------------------------------------------------------------ float64 ------------------------------------------------------------
def cepstra_f64(x, K: int) -> np.ndarray:
    from scipy.fft import dct

    return dct(np.asarray(x, dtype=np.float64), type=2, norm="ortho", axis=-1)[..., 1 : K + 1]


def cost_f64(ca, cb) -> np.ndarray:
    return np.sqrt(((ca[:, None, :] - cb[None, :, :]) ** 2).sum(axis=2))


def mcd_aligned_f64(a, b, L=None, K: int = 13) -> float:
    L = min(len(a), len(b)) if L is None else L
    ca, cb = cepstra_f64(a[:L], K), cepstra_f64(b[:L], K)
    return ALPHA * float(np.sqrt(((ca - cb) ** 2).sum(axis=1)).sum()) / L


def mcd_dtw_f64(a, b, K: int = 13, band: int = 0):
    """(total float64, path_len, span) of the float64 DP under the contract's tie rule."""
    D, codes = DO.accumulate(cost_f64(cepstra_f64(a, K), cepstra_f64(b, K)), band)
    n, span = DO.backtrace(codes)
    return float(D[-1, -1]), n, span


# ------------------------------------------------------------ the bound ------------------------------------------------------------
def cepstrum_bound(x, table) -> np.ndarray:
    """ec[t, k] = gamma_(M+2) sum_m |dct[k][m] x[t, m]|, in float64."""
    x = np.asarray(x, dtype=np.float64)
    return gamma(x.shape[1] + 2) * (np.abs(x)[:, None, :] * np.abs(table.astype(np.float64))[None, :, :]).sum(axis=2)


def cost_bound(a, b, K: int = 13):
    """(B_d [la, lb] float64, d32 [la, lb]) of the module docstring."""
    table = basis(a.shape[1], K)
    ca, cb = cepstra_f32(a, table), cepstra_f32(b, table)
    eca, ecb = cepstrum_bound(a, table), cepstrum_bound(b, table)
    e32 = np.abs(ca.astype(np.float64)[:, None, :] - cb.astype(np.float64)[None, :, :])
    E = eca[:, None, :] + ecb[None, :, :] + U * e32
    d32 = cost_f32(ca, cb).astype(np.float64)
    return np.sqrt((E ** 2).sum(axis=2)) + gamma(K + 2) * d32, d32


def aligned_bound(a, b, L=None, K: int = 13) -> float:
    """The bound on |MCD32 - MCD64| of an aligned row, dB."""
    L = min(len(a), len(b)) if L is None else L
    B, d32 = cost_bound(a[:L], b[:L], K)
    return ALPHA * (float(np.diag(B).sum()) + U * float(np.diag(d32).sum())) / L


def dtw_total_bound(a, b, K: int = 13) -> float:
    """B_total of the module docstring (on total, not scaled by alpha)."""
    B, d32 = cost_bound(a, b, K)
    P = len(a) + len(b) - 1
    return P * (float(B.max()) + gamma(P + 1) * float(d32.max()))


def speechlike_mels(seed: int, T: int, M: int = 80, env_seed=None, level: float = 0.0) -> np.ndarray:
    """Natural-log-mel-like rows (float32): a smooth spectral envelope that drifts over time (drawn from ``env_seed``, or from ``seed``)
    plus band noise, around -5 + ``level``."""
    rng, env_rng = np.random.RandomState(seed), np.random.RandomState(seed if env_seed is None else env_seed)
    m = np.arange(M)[None, :] / float(M)
    t = np.arange(T)[:, None] / 40.0
    env = -5.0 + 2.0 * np.cos(2 * np.pi * (m * env_rng.uniform(0.5, 2.0) + t * env_rng.uniform(0.2, 1.0))) - 3.0 * m
    return (env + level + 0.5 * rng.standard_normal((T, M))).astype(np.float32)


def mel_pair(seed: int, Ta: int, Tb: int, M: int = 80):
    """A "recording" and a "resynthesis": one envelope, band noise of their own, and 0.7 nepers between their levels (what c0 would see)."""
    return speechlike_mels(seed, Ta, M, env_seed=seed + 1000), speechlike_mels(seed + 100, Tb, M, env_seed=seed + 1000, level=0.7)
