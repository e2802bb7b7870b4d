"""nat_conv_mfma_k's summation order restated on the CPU, for judging a postnet figure outside the bar of tests/test_gpu_nat_dims.py.

The kernel forms every output element as ONE fp32 fma chain: the bias first, then for each 32-channel step, each tap, each (q, e) of the step's 16
channel pairs the two lane halves' channels 32 cs + 4 q + e and + 16; with more than 512 input channels the chain is cut every 8 steps and the
parts are added at the end (the kernel's FOLD).  This script runs the five postnet layers in that order in fp32 (an fma as the
fp64 sum of the exact product, rounded to fp32) on the oracle's own fp32 teacher-forced `pre` of one sentence of a width set of tests/_nat_dims.py and
prints its distance from the fp64 postnet beside the oracle's blocked fp32 sums' and the bar.

    python tools/restate_nat_conv_order.py W 65 129
"""
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO), str(REPO / "tests")]
import _gta_oracle as G  # noqa: E402
import _nat_dims as D  # noqa: E402
from oracle import nat_oracle as O  # noqa: E402


def conv_kernel_order(x, w, b):
    K, Cin, Cout = w.shape
    F = x.shape[0]
    xp = np.zeros((F + K - 1, Cin), np.float32)
    xp[(K - 1) // 2 : (K - 1) // 2 + F] = x
    acc = np.broadcast_to(b, (F, Cout)).astype(np.float32).copy()
    tot = np.zeros_like(acc)
    ncs = (Cin + 31) // 32
    for cs in range(ncs):
        if K == 5 and Cin > 512 and cs % 8 == 0 and cs:  # FOLD: the sums of 8 steps are set aside and the parts added at the end
            tot, acc = tot + acc, np.zeros_like(acc)
        for j in range(K):
            for qe in range(16):
                for lh in range(2):
                    c = 32 * cs + 16 * lh + qe
                    if c < Cin:
                        acc = (acc.astype(np.float64) + np.outer(xp[j : j + F, c].astype(np.float64), w[j, c].astype(np.float64))).astype(np.float32)
    return tot + acc


def main(sid, L, F):
    P, S = D.checkpoint(sid)
    pre = np.asarray(D.oracle_teacher(sid, L, F, False)[0], np.float32)
    p = O.Params(P, S, np.float32)
    y = pre
    for i in range(5):
        cv = "conv1_d" if i == 0 else f"conv1_d_{i}"
        y = conv_kernel_order(y, p.get(f"{G.PRE}/~/{cv}", "w"), p.get(f"{G.PRE}/~/{cv}", "b"))
        if i < 4:
            bn = "batch_norm" if i == 0 else f"batch_norm_{i}"
            sc, of = p.get(f"{G.PRE}/~/{bn}", "scale").reshape(-1), p.get(f"{G.PRE}/~/{bn}", "offset").reshape(-1)
            mu, var = p.get(f"{G.PRE}/~/{bn}/~/mean_ema", "average", True).reshape(-1), p.get(f"{G.PRE}/~/{bn}/~/var_ema", "average", True).reshape(-1)
            inv = (sc / np.sqrt(var + np.float32(O.BN_EPS))).astype(np.float32)  # pack time: inv = scale * rsqrt(var + eps)
            y = np.tanh(((y - mu) * inv + of).astype(np.float32)).astype(np.float32)
    want = D.postnet(sid, pre)
    e32 = float(np.abs(D.postnet(sid, pre, fp64=False).astype(np.float64) - want).max())
    err = float(np.abs(y.astype(np.float64) - want).max())
    b = D.bar(want, e32, D.CAP)
    print(f"{sid} ({L}, {F}): postnet in the kernel's order, fp32, vs fp64: {err:.3e}; the oracle's blocked fp32 sums (e32): {e32:.3e}; bar {b:.3e}; err / bar {err / b:.3f}")


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]))
