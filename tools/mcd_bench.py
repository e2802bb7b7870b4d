"""Time the MCD kernels (viettts_amd/csrc/mcd.hip) next to (1) the same contract composed from torch-ROCm operators (a matmul with the
basis, a row-wise norm or the blocked broadcast ``((ca - cb) ** 2).sum(-1).sqrt()``, and tools/align_bench.py's torch DTW over that cost;
the recurrence is not fed from ``torch.cdist``: in this tool's first run its ``donot_use_mm_for_euclid_dist`` mode left the 64-pair cases'
totals disagreeing with the kernels', as tools/align_bench.py found for p = 1; the default mode's agreement with the broadcast is
reported), (2) ``log_mel_dtw`` on the same mels (the L1
DTW over 80 bands that MCD-DTW's cost kernel shrinks) and (3) the HBM floor of the bytes each pass has to move.

Cases: aligned MCD of 64 x 1024 frames; MCD-DTW of 64 pairs of 768 x 768 without a band and with band 32; one pair of 2048 x 2048.
Device-event timing, warm-up, medians; the sides alternate run by run in one process.  The torch side's figures differ from the kernels' in
the last bits (its matmul and cdist have their own order), so the agreement is reported, not asserted; tests/test_gpu_mcd.py holds the
kernels to the contract.

    python tools/mcd_bench.py [--iters 20] [--torch-iters 3] [--output profiles/mcd_bench.json]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tools"))
from align_bench import TorchDtw, alternated_ms  # noqa: E402
from viettts_amd.align import Dtw  # noqa: E402
from viettts_amd.mcd import ALPHA, Mcd  # noqa: E402

M, K = 80, 13
HBM_BYTES_PER_S = 8.0e12  # MI355X peak HBM3E bandwidth: the floor below is bytes over this
ALIGNED = (64, 1024)
DTW_CASES = ((64, 768, 768, 0), (64, 768, 768, 32), (1, 2048, 2048, 0))


class TorchDtwOverCost(TorchDtw):
    """tools/align_bench.py's recurrence and backtrace over the L2 cost of cepstra (a matmul with the basis, a blocked broadcast)."""

    def __init__(self, la, lb, band, device, basis):
        super().__init__(la, lb, band, device)
        self.basis_t = basis.t().contiguous()

    def __call__(self, a, b):
        return self.from_cost(self.cost(a @ self.basis_t, b @ self.basis_t))

    def cost(self, ca, cb):
        N, la, lb = ca.shape[0], ca.shape[1], cb.shape[1]
        c = torch.empty((N, la, lb), device=self.dev)
        rows = max(1, (1 << 26) // (N * lb * ca.shape[2]))  # the broadcast difference of `rows` query rows at a time: at most 256 MB
        for r0 in range(0, la, rows):
            c[:, r0 : r0 + rows] = ((ca[:, r0 : r0 + rows, None, :] - cb[:, None, :, :]) ** 2).sum(dim=-1).sqrt()
        return c

    def from_cost(self, c):
        # TorchDtw.__call__ from its cost tensor on: the same statements, fed the L2 cost
        la, lb, dev = self.la, self.lb, self.dev
        N = c.shape[0]
        inf = float("inf")
        if self.band:
            c = c.masked_fill(self.outside, inf)
        D = torch.full((N, la + 1, lb + 1), inf, device=dev)
        codes = torch.zeros((N, la, lb), dtype=torch.uint8, device=dev)
        one, two = torch.ones((), dtype=torch.uint8, device=dev), torch.full((), 2, dtype=torch.uint8, device=dev)
        for s, (i, j) in enumerate(self.diag):
            best, up, left = D[:, i, j], D[:, i, j + 1], D[:, i + 1, j]
            m = up < best
            best = torch.where(m, up, best)
            code = m.to(torch.uint8)
            m = left < best
            best = torch.where(m, left, best)
            code = torch.where(m, two, code)
            val = c[:, i, j] + best
            if s == 0:
                val, code = c[:, :1, 0], torch.zeros_like(code)
            D[:, i + 1, j + 1] = val
            codes[:, i, j] = code
        n = torch.arange(N, device=dev)
        i = torch.full((N,), la - 1, device=dev)
        j = torch.full((N,), lb - 1, device=dev)
        length = torch.ones((N,), dtype=torch.int64, device=dev)
        for _ in range(la + lb - 2):
            active = (i > 0) | (j > 0)
            code = codes[n, i, j]
            code = torch.where(i == 0, two, torch.where(j == 0, one, code))
            i = i - (active & (code != 2)).to(i.dtype)
            j = j - (active & (code != 1)).to(j.dtype)
            length = length + active.to(length.dtype)
        return D[:, la, lb], length


def floor_ms(nbytes: float) -> float:
    return nbytes / HBM_BYTES_PER_S * 1e3


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--torch-iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--output", default=str(REPO / "profiles" / "mcd_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mcd_bench needs the GPU"
    dev = torch.device("cuda:0")
    doc = {"method": f"device events, {a.warmup} warm-ups of every side, medians of {a.iters} (kernels, log_mel_dtw) and {a.torch_iters} (torch) runs alternated in "
                     "one process; torch side = matmul with the basis + row norm (aligned) or blocked broadcast L2 + tools/align_bench.py's anti-diagonal recurrence "
                     f"and backtrace; *_per_call_of_10_ms = ten calls per timed window over ten; hbm_floor_ms = bytes each pass must move / {HBM_BYTES_PER_S:.1e} B/s; anything not in this file is unmeasured",
           "device": torch.cuda.get_device_name(0), "n_mels": M, "n_ceps": K, "cases": []}
    g = torch.Generator(device="cpu").manual_seed(23)

    N, T = ALIGNED
    x, y = (torch.randn((N, T, M), generator=g) - 5.0).to(dev), (torch.randn((N, T, M), generator=g) - 5.0).to(dev)
    m = Mcd(M, K, 0, dev)
    basis_t = torch.from_numpy(m.basis()).to(dev).t().contiguous()

    def torch_aligned():
        return ALPHA * (x @ basis_t - y @ basis_t).norm(dim=2).double().mean(dim=1)

    got, ref = m.aligned(x, y), torch_aligned()
    torch.cuda.synchronize()
    r = alternated_ms({"kernels": lambda: m.aligned(x, y), "torch": torch_aligned}, {"kernels": a.iters, "torch": a.iters}, a.warmup)
    # the C ABI alone on prepared buffers, and the torch composition, ten calls per timed window: the launches queue up, so the window
    # holds the device's time and not the host's per call
    import ctypes as C

    from viettts_amd._handle import ptr

    lens = (C.c_int32 * N)(*([T] * N))
    total = torch.empty((N,), dtype=torch.float64, device=dev)
    ws = m._workspace(m.aligned_workspace_bytes(N, T))

    def abi_x10():
        for _ in range(10):
            m._on_stream("aligned", ptr(x), ptr(y), N, T, T, lens, ptr(total), ptr(None), 0, ptr(ws), ws.numel())

    def torch_x10():
        for _ in range(10):
            torch_aligned()

    r10 = alternated_ms({"abi_x10": abi_x10, "torch_x10": torch_x10}, {"abi_x10": a.iters, "torch_x10": a.iters}, a.warmup)
    nbytes = 2 * N * T * M * 4 + N * ((T + 63) // 64) * 8 * 2 + N * 8  # both mels in, the block sums out and in, the sums out
    rec = {"case": "aligned", "N": N, "T": T, "max_rel_diff_vs_torch": float(((got - ref).abs() / ref.abs()).max()), "bytes": nbytes,
           "hbm_floor_ms": floor_ms(nbytes), "kernels": r["kernels"], "torch": r["torch"], "speedup_vs_torch": r["torch"]["median_ms"] / r["kernels"]["median_ms"],
           "share_of_hbm_floor": floor_ms(nbytes) / r["kernels"]["median_ms"],
           "abi_per_call_of_10_ms": r10["abi_x10"]["median_ms"] / 10, "torch_per_call_of_10_ms": r10["torch_x10"]["median_ms"] / 10,
           "abi_share_of_hbm_floor": floor_ms(nbytes) / (r10["abi_x10"]["median_ms"] / 10)}
    print(json.dumps(rec), flush=True)
    doc["cases"].append(rec)
    m.close()

    for N, la, lb, band in DTW_CASES:
        x, y = (torch.randn((N, la, M), generator=g) - 5.0).to(dev), (torch.randn((N, lb, M), generator=g) - 5.0).to(dev)
        m, d = Mcd(M, K, band, dev), Dtw(M, band, dev)
        t = TorchDtwOverCost(la, lb, band, dev, torch.from_numpy(m.basis()).to(dev))
        got, ref = m.dtw(x, y), t(x, y)
        ca, cb = x @ t.basis_t, y @ t.basis_t
        cd = torch.cdist(ca, cb, p=2.0)
        cdist_diff = float(((cd - t.cost(ca, cb)).abs() / t.cost(ca, cb).abs().clamp_min(1e-30)).max())
        torch.cuda.synchronize()
        del cd
        r = alternated_ms({"kernels": lambda: m.dtw(x, y), "log_mel_dtw": lambda: d.dtw(x, y), "torch": lambda: t(x, y)},
                          {"kernels": a.iters, "log_mel_dtw": a.iters, "torch": a.torch_iters}, a.warmup)
        strips, steps, words = -(-la // 256), -(-(lb + 255) // 64) * 64, -(-lb // 16)
        # cepstra pass: mels in, cepstra out; cost pass: cepstra in, cost out; wavefront: cost in, codes out; backtrace: codes in (at most), span out
        nbytes = N * ((la + lb) * M * 4 + 2 * (la + lb) * K * 4 + 2 * strips * steps * 256 * 4 + 2 * la * words * 4 + la * 8)
        rec = {"case": "dtw", "N": N, "la": la, "lb": lb, "band": band, "workspace_bytes": m.dtw_workspace_bytes(N, la, lb),
               "total_max_rel_diff_vs_torch": float(((got.total - ref[0]).abs() / ref[0].abs()).max()),
               "path_len_equal": bool(torch.equal(got.path_len.long(), ref[1])), "cdist_max_rel_diff_vs_broadcast": cdist_diff, "bytes_without_band": nbytes, "hbm_floor_ms": floor_ms(nbytes),
               "kernels": r["kernels"], "log_mel_dtw": r["log_mel_dtw"], "torch": r["torch"],
               "speedup_vs_torch": r["torch"]["median_ms"] / r["kernels"]["median_ms"],
               "time_vs_log_mel_dtw": r["kernels"]["median_ms"] / r["log_mel_dtw"]["median_ms"],
               "share_of_hbm_floor": floor_ms(nbytes) / r["kernels"]["median_ms"], "cells_per_s": N * la * lb / (r["kernels"]["median_ms"] * 1e-3)}
        print(json.dumps(rec), flush=True)
        doc["cases"].append(rec)
        m.close()
        d.close()
        del t, ref
    Path(a.output).parent.mkdir(parents=True, exist_ok=True)
    Path(a.output).write_text(json.dumps(doc, indent=1) + "\n")
    print(f"wrote {a.output}")


if __name__ == "__main__":
    main()
