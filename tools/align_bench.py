"""Time batched DTW (viettts_amd/csrc/dtw.hip) next to the same contract written with torch-ROCm operators: a cost tensor
(the broadcast ``|a - b|`` summed over the features, a block of query rows at a time; ``torch.cdist(p=1)`` is not used: at 64 x 768 x 768
it returned wrong distances for the later pairs of the batch on this torch build, which this tool's agreement figures showed), one round of gathers / selects / scatters per anti-diagonal, and a batched backtrace that follows the codes.
Shapes: 64 pairs of 768 x 768 x 80 (the GTA bench's shape) and one pair of 2048 x 2048 x 80; band 0 and band 32.  Device-event
timing, warm-up, medians; the two sides alternate run by run in one process.  The torch side's index tensors are built once, outside
the timed region.  Its totals differ from the kernels' in the last bits (torch's sum over the features has its own order), so the agreement is reported,
not asserted; tests/test_gpu_dtw.py holds the kernels to the contract.

    python tools/align_bench.py [--iters 20] [--torch-iters 5] [--out profiles/align_bench.json]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
from viettts_amd.align import Dtw  # noqa: E402

SHAPES = ((64, 768, 768, 80), (1, 2048, 2048, 80))
BANDS = (0, 32)


class TorchDtw:
    """include/vtts_dtw.h with torch operators, for full-length pairs [N, la, D] x [N, lb, D]."""

    def __init__(self, la: int, lb: int, band: int, device):
        self.la, self.lb, self.band, self.dev = la, lb, band, device
        self.diag = []
        for s in range(la + lb - 1):
            i = torch.arange(max(0, s - lb + 1), min(la - 1, s) + 1, device=device)
            self.diag.append((i, s - i))
        if band:
            i = torch.arange(la, device=device, dtype=torch.int64)[:, None]
            j = torch.arange(lb, device=device, dtype=torch.int64)[None, :]
            self.outside = (i * (lb - 1) - j * (la - 1)).abs() > band * max(la - 1, lb - 1)

    def __call__(self, a: torch.Tensor, b: torch.Tensor):
        la, lb, dev = self.la, self.lb, self.dev
        N = a.shape[0]
        inf = float("inf")
        c = torch.empty((N, la, lb), device=dev)
        rows = max(1, (1 << 26) // (N * lb * a.shape[2]))  # the broadcast difference of `rows` query rows at a time: at most 256 MB
        for r0 in range(0, la, rows):
            c[:, r0 : r0 + rows] = (a[:, r0 : r0 + rows, None, :] - b[:, None, :, :]).abs().sum(dim=-1)
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
        first = torch.full((N, la), -1, device=dev)
        last = torch.full((N, la), -1, device=dev)
        last[:, la - 1] = lb - 1
        length = torch.ones((N,), dtype=torch.int64, device=dev)
        for _ in range(la + lb - 2):
            active = (i > 0) | (j > 0)
            code = codes[n, i, j]
            code = torch.where(i == 0, two, torch.where(j == 0, one, code))
            up_row = active & (code != 2)
            first.scatter_(1, i[:, None], torch.where(up_row, j, first.gather(1, i[:, None])[:, 0])[:, None])
            i = i - up_row.to(i.dtype)
            j = j - (active & (code != 1)).to(j.dtype)
            last.scatter_(1, i[:, None], torch.where(up_row, j, last.gather(1, i[:, None])[:, 0])[:, None])
            length = length + active.to(length.dtype)
        first[:, 0] = 0
        return D[:, la, lb], length, torch.stack([first, last], dim=2)


def alternated_ms(fns: dict, iters: dict, warmup: int) -> dict:
    """Per function: median, min and max of device-event times; one run of each per round while it still has runs left."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for it in range(max(iters.values())):
        for k, fn in fns.items():
            if it >= iters[k]:
                continue
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "runs": len(v)} for k, v in times.items()}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--torch-iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(REPO / "profiles" / "align_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "align_bench needs the GPU"
    dev = torch.device("cuda:0")
    doc = {"method": f"device events, {a.warmup} warm-ups of both sides, medians of {a.iters} (kernels) and {a.torch_iters} (torch) runs alternated in one "
                     "process; torch side = blocked broadcast |a - b|.sum(-1) + one round of gathers/selects/scatters per anti-diagonal + a batched backtrace over the codes, "
                     "index tensors prebuilt",
           "device": torch.cuda.get_device_name(0), "cases": []}
    for N, la, lb, D in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(17)
        x = torch.randn((N, la, D), generator=g).to(dev)
        y = torch.randn((N, lb, D), generator=g).to(dev)
        for band in BANDS:
            d, t = Dtw(D, band, dev), TorchDtw(la, lb, band, dev)
            got, ref = d.dtw(x, y), t(x, y)
            torch.cuda.synchronize()
            rec = {"N": N, "la": la, "lb": lb, "D": D, "band": band, "workspace_bytes": d.workspace_bytes(N, la, lb),
                   "total_max_rel_diff_vs_torch": float(((got.total - ref[0]).abs() / ref[0].abs()).max()),
                   "path_len_equal": bool(torch.equal(got.path_len.long(), ref[1])),
                   "span_rows_equal_fraction": float((got.span.long() == ref[2]).all(dim=2).float().mean())}
            r = alternated_ms({"kernels": lambda: d.dtw(x, y), "torch": lambda: t(x, y)}, {"kernels": a.iters, "torch": a.torch_iters}, a.warmup)
            rec.update(kernels=r["kernels"], torch=r["torch"], speedup_vs_torch=r["torch"]["median_ms"] / r["kernels"]["median_ms"],
                       cells_per_s=N * la * lb / (r["kernels"]["median_ms"] * 1e-3))
            print(json.dumps(rec), flush=True)
            doc["cases"].append(rec)
            d.close()
            del t, ref
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
