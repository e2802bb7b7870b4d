"""Plain numpy restatement of include/vtts_limstream.h: a state machine that is fed a row chunk by chunk, carries the history the contract
names, and computes only the span a push may finalise, from tests/_limiter_oracle.py's pieces (``envelope``, ``gain_curve``'s req).  It never
sees the whole row.  In float64 (the oracle) and float32 (the kernel's arithmetic class), as _limiter_oracle.

``fault`` plants one mistake a streamed implementation can make (tests/test_limiter_stream_cpu.py shows that its cases see each):

    "short_history"   the history lacks x[n - 23], the first sample whose tap can show in a result (x[n - 27 .. n - 25] meet the phases' zero
                      padding and x[n - 24] a tap of 1.4e-20: the contract's 2 W + 27 follows the tap table's layout)
    "clamp_window"    indices are clamped at the start of what a push has staged instead of at the row's sample 0
    "early_end"       the row's end (zero extension, edge replication) is applied to what has arrived, before ``last``
    "peak_not_final"  the running true peak reads p[n] with n + 24 >= R
    "anchor_push"     whole runs are not waited for: the run sums are anchored at the push's first sample instead of the row's
"""
from __future__ import annotations

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import _limiter_oracle as O

RUN = O.RUN
LEAD, TRAIL = 27, 24  # a phase's taps meet x[n - 27 .. n + 24]; the first three (four) of them are zero padding
FAULTS = ("short_history", "clamp_window", "early_end", "peak_not_final", "anchor_push")


def emit(received: int, emitted: int, count: int, last: bool, W: int) -> int:
    """The emit rule, written out again (viettts_amd.limiter.stream_emit and vtts_limstream_emit are compared with it)."""
    r = received + count
    if last:
        return r
    whole = (r - 2 * W - TRAIL) // RUN * RUN if r > 2 * W + TRAIL else 0
    return max(emitted, whole)


class Stream:
    """One row.  ``push(chunk, last)`` returns the samples that leave, as ``dtype``; ``true_peak`` and ``min_gain`` run along."""

    def __init__(self, fs: int, g=1.0, ceiling_dbtp: float = -1.0, W=None, dtype=np.float64, fault=None):
        assert fault is None or fault in FAULTS
        self.fs, self.dtype, self.fault = fs, dtype, fault
        self.W = O.lookahead(fs) if W is None else int(W)
        self.g, self.c = np.float32(g), O.ceiling(ceiling_dbtp)
        self.R = self.F = self.base = 0           # received, emitted, and the absolute index of hist[0]
        self.hist = np.zeros(0, np.float32)
        self.true_peak, self.min_gain = 0.0, 1.0
        self.closed = False
        self.anchors = []                         # the absolute samples the run sums were started at

    def _emit(self, count, last):
        W = self.W
        if self.fault == "early_end" and not last:
            return max(self.F, (self.R + count) // RUN * RUN)
        if self.fault == "anchor_push" and not last:
            return max(self.F, self.R + count - 2 * W - TRAIL)
        return emit(self.R, self.F, count, last, W)

    def _mean(self, hv, E, F):
        """Mean of hv[i .. i + 2 W] for i < E: float64 plainly, float32 in the header's order with runs anchored at F."""
        W, Lw = self.W, 2 * self.W + 1
        if np.dtype(self.dtype) == np.float64:
            return sliding_window_view(hv.astype(np.float64), Lw)[:E].sum(axis=1) / Lw
        nrun = -(-E // RUN)
        self.anchors += [F + RUN * i for i in range(nrun)]
        hp = np.concatenate([hv.astype(np.float64), np.zeros(2 * RUN)])
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
        return (out[:E] / float(Lw)).astype(np.float32)

    def push(self, chunk, last: bool = False) -> np.ndarray:
        assert not self.closed
        f = np.dtype(self.dtype).type
        W = self.W
        x = O.as_float(chunk)
        R, F = self.R, self.F
        Rn, Fn = R + x.shape[0], self._emit(x.shape[0], last)
        xs = np.concatenate([self.hist, x])                        # x[base .. Rn)
        final = last or self.fault == "early_end"                  # is the row's end known?
        E = Fn - F
        y = np.zeros(0, self.dtype)
        if E > 0:
            lo, hi = F - 2 * W - LEAD, Fn + 2 * W + TRAIL          # the samples this push reads: zero before 0 and, at the end, past Rn
            assert final or hi <= Rn
            idx = np.arange(lo, hi)
            have = (idx >= self.base) & (idx < Rn)                 # (below base only with a planted short history: read as zero)
            xwin = np.zeros(hi - lo, np.float32)
            xwin[have] = xs[idx[have] - self.base]
            p = O.envelope(xwin, self.fs, self.dtype)[LEAD:LEAD + E + 4 * W]    # p[F - 2 W + k]
            floor = max(0, F - W) if self.fault == "clamp_window" else 0
            top = Rn - 1 if final else Fn + 2 * W                  # (without an end nothing reaches the top)
            n = np.clip(np.arange(F - 2 * W, Fn + 2 * W), floor, top)
            req = O.gain_curve(p[n - (F - 2 * W)], self.g, self.c, 0, self.dtype)[0]      # req[clamp(F - 2 W + k)]
            held = sliding_window_view(req, 2 * W + 1).min(axis=1)                          # held[F - W + j] of a sample inside the row
            m = np.clip(np.arange(F - W, Fn + W), 0, top)
            hv = held[m - (F - W)]                                                          # held[clamp(F - W + j)]
            a = np.minimum(req[2 * W:2 * W + E], self._mean(hv, E, F).astype(self.dtype))
            xc = xwin[2 * W + LEAD:2 * W + LEAD + E]
            y = ((f(self.g) * xc.astype(self.dtype)).astype(self.dtype) * a).astype(self.dtype)
            seen = p[2 * W:2 * W + E]
            if self.fault == "peak_not_final":                     # everything that has arrived, its last 24 samples included
                tail = np.concatenate([xs, np.zeros(TRAIL + LEAD, np.float32)])
                seen = O.envelope(tail, self.fs, self.dtype)[:xs.shape[0]]
            self.true_peak = max(self.true_peak, float(seen.max()))
            self.min_gain = min(self.min_gain, float(a.min()))
        keep = 2 * W + (LEAD if self.fault != "short_history" else TRAIL - 2)
        nb = max(0, Fn - keep)
        self.hist, self.base = xs[nb - self.base:].copy(), nb
        self.R, self.F, self.closed = Rn, Fn, bool(last)
        return y

