"""Plain numpy restatement of the streamed resampler's contract (include/vtts_rsstream.h): the kernel's fp32 chain on a whole row, and a
state machine fed chunk by chunk that carries ONLY the history the contract allows, x[max(0, q(F') - (kp4 - 1)) .. R'), and raises when an
output would read anything else.

    t = m M + half, q = t div L, p = t mod L
    y[m] = fmaf chain over i = 0 .. kp4 - 1 of x[q - (kp4 - 1) + i] * row[p][i],  row[p][kp4 - 1 - j] = float32(h[p + j L]) or 0

The fused multiply-add is emulated through float64: a float32 x float32 product is exact there, and both sides of every comparison here use
the same emulation, so whole row against chunks is a statement about indices, history and order, not about the emulation's last bit.

``Stream(..., fault=NAME)`` plants one mistake (``FAULTS``); a read the contract forbids then gives 0 instead of raising, as stale memory
would give something.
"""
from __future__ import annotations

import numpy as np

import _audio_oracle as A

OPB = 1024  # include/vtts_audio.h: VTTS_AUDIO_OUT_PER_BLOCK
RATES = [(16000, 48000), (16000, 8000), (16000, 24000), (16000, 44100), (16000, 22050), (44100, 16000), (16000, 16000)]
FAULTS = ("history_short", "emit_early", "zero_at_chunk", "tile_at_chunk")


class OutsideHistory(AssertionError):
    pass


_DESIGNS = {}


def design(in_rate: int, out_rate: int):
    """(L, M, half, kp4, rows [L, kp4] float32): the phase-major table, rows reversed and right-aligned, the padding zeros first."""
    key = (int(in_rate), int(out_rate))
    if key not in _DESIGNS:
        L, M, half = A.ratio(in_rate, out_rate)
        h = A.prototype(in_rate, out_rate).astype(np.float32)
        kp4 = (-(-(2 * half + 1) // L) + 3) // 4 * 4
        rows = np.zeros((L, kp4), dtype=np.float32)
        for p in range(L):
            k = p + np.arange(kp4) * L
            ok = k <= 2 * half
            rows[p, (kp4 - 1 - np.arange(kp4))[ok]] = h[k[ok]]
        _DESIGNS[key] = (L, M, half, kp4, rows)
    return _DESIGNS[key]


def emit(received: int, emitted: int, count: int, last: bool, L: int, M: int, half: int) -> int:
    r = received + count
    if L == M:
        return r
    if last:
        return -(-r * L // M)
    return max(emitted, 0, -(-(r * L - half) // M))


def newest(m: int, L: int, M: int, half: int) -> int:
    return (m * M + half) // L


def delay(L: int, M: int, half: int) -> int:
    """Input samples a row's output trails its input by: ceil(half / L)."""
    return 0 if L == M else -(-half // L)


def _chains(xw: np.ndarray, taps: np.ndarray) -> np.ndarray:
    """xw, taps [n, kp4] float32 -> [n] float32: acc = fmaf(x, w, acc) in ascending i."""
    acc = np.zeros(xw.shape[0], dtype=np.float32)
    xd, td = xw.astype(np.float64), taps.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(xw.shape[1]):
            acc = (acc.astype(np.float64) + xd[:, i] * td[:, i]).astype(np.float32)
    return acc


def to_f32(x: np.ndarray) -> np.ndarray:
    """The kernel's load: PCM16 times 2^-15, exact."""
    x = np.asarray(x)
    return (x.astype(np.float32) / np.float32(32768.0)) if x.dtype == np.int16 else x.astype(np.float32)


def to_pcm16(y: np.ndarray) -> np.ndarray:
    """include/vtts_audio.h: clip, times 32767 in double, round half to even; NaN gives 0."""
    y = np.asarray(y, dtype=np.float32)
    c = np.clip(np.where(np.isnan(y), np.float32(0), y), -1.0, 1.0).astype(np.float64)
    return np.rint(c * 32767.0).astype(np.int16)


def whole(x, in_rate: int, out_rate: int) -> np.ndarray:
    """The chain on the whole row: float32 [ceil(S L / M)], zero extension at the row's own ends."""
    x = to_f32(x)
    L, M, half, kp4, rows = design(in_rate, out_rate)
    if L == M:
        return x.copy()
    S = x.shape[0]
    m = np.arange(A.out_samples(S, L, M), dtype=np.int64)
    t = m * M + half
    q, p = t // L, t % L
    n = q[:, None] - (kp4 - 1) + np.arange(kp4)[None, :]
    ok = (n >= 0) & (n < S)
    xw = np.where(ok, x[np.where(ok, n, 0)] if S else np.float32(0), np.float32(0)).astype(np.float32)
    return _chains(xw, rows[p])


class Stream:
    """One row slot.  ``push(chunk, last)`` returns the emitted float32 samples."""

    def __init__(self, in_rate: int, out_rate: int, fault=None):
        assert fault is None or fault in FAULTS
        self.L, self.M, self.half, self.kp4, self.rows = design(in_rate, out_rate)
        self.fault = fault
        self.R = self.F = 0
        self.base = 0                             # absolute index of hist[0]
        self.hist = np.zeros(0, dtype=np.float32)
        self.closed = False
        self.most_history = 0

    def push(self, chunk, last: bool = False) -> np.ndarray:
        assert not self.closed
        L, M, half, kp4 = self.L, self.M, self.half, self.kp4
        chunk = to_f32(chunk)
        R, F = self.R, self.F
        Rn = R + chunk.shape[0]
        Fn = emit(R, F, chunk.shape[0], last, L, M, half)
        if L == M:
            self.R = self.F = Rn
            self.closed = last
            return chunk.copy()
        if self.fault == "emit_early" and not last and Fn > 0:
            Fn += 1
        buf = np.concatenate([self.hist, chunk])  # x[base .. R')
        assert self.base + self.hist.shape[0] == R
        out = np.empty(Fn - F, dtype=np.float32)
        for m0 in range(F, Fn, OPB):  # tiles anchored at F: a tile's outputs take their phase and newest sample from the tile's base
            live = min(OPB, Fn - m0)
            anchor = m0
            if self.fault == "tile_at_chunk":
                anchor = -(-R * L // M) + (m0 - F)  # the first output past the chunk's start
            t0 = anchor * M + half
            q0, p0 = t0 // L, t0 % L
            i = np.arange(live, dtype=np.int64)
            q = q0 + (p0 + i * M) // L
            p = (p0 + i * M) % L
            n = q[:, None] - (kp4 - 1) + np.arange(kp4)[None, :]
            lo = R if self.fault == "zero_at_chunk" else 0  # where zero extension begins
            zero = (n < lo) | ((n >= Rn) if last else False)
            legal = zero | ((n >= self.base) & (n < Rn))
            if not legal.all():
                if self.fault is None:
                    bad = n[~legal]
                    raise OutsideHistory(f"outputs {m0} .. {m0 + live - 1} read x[{bad.min()} .. {bad.max()}], the row holds x[{self.base} .. {Rn})")
                zero = zero | ~legal
            xw = np.where(zero, np.float32(0), buf[np.where(zero, 0, n - self.base)] if buf.size else np.float32(0)).astype(np.float32)
            out[m0 - F:m0 - F + live] = _chains(xw, self.rows[p])
        self.R, self.F, self.closed = Rn, Fn, last
        if not last:
            keep = max(0, newest(Fn, L, M, half) - (kp4 - 1))
            if self.fault == "history_short":
                keep += 1
            keep = min(keep, Rn)
            self.hist = buf[keep - self.base:].copy()
            self.base = keep
            self.most_history = max(self.most_history, self.hist.shape[0])
            if self.fault is None:
                assert self.hist.shape[0] <= kp4 - 1, (self.hist.shape[0], kp4)
        return out


def run(x, in_rate: int, out_rate: int, sizes, fault=None, flush: bool = False):
    """Feed ``x`` in chunks of ``sizes`` (cycled; zeros are zero-count pushes).  ``flush``: the row's samples go in non-last pushes and an
    empty last push ends it.  Returns (per-push outputs, the Stream)."""
    st = Stream(in_rate, out_rate, fault)
    x = np.asarray(x)
    ys, at, k = [], 0, 0
    while True:
        n = min(int(sizes[k % len(sizes)]), len(x) - at)
        k += 1
        end = at + n >= len(x)
        ys.append(st.push(x[at:at + n], last=end and not flush))
        at += n
        if end:
            break
    if flush:
        ys.append(st.push(x[:0], last=True))
    return ys, st


def same(a: np.ndarray, b: np.ndarray) -> bool:
    """NaN positions as positions, everything else as bit patterns."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32)))
