"""Time the discriminators' scoring pass on the GPU and write profiles/disc_bench.json.

    python tools/disc_bench.py [--iters 10] [--out profiles/disc_bench.json]

Shapes: 2 x 16 x 8192 (upstream's training batch and segment) and 2 x 8 x 80000 (validation clips).  Device-event times of
``forward`` and ``forward + losses``; FLOPs and bytes computed from the shapes; the share of the 157 TF fp32-MFMA peak; the bound
(compute, or the 283 MB weight stream).  Baseline: the same forward restated on torch-ROCm's own operators in fp32 on the same GPU,
alternated with the library in the same process; if the framework cannot run it, the JSON says so and nothing is substituted.
The per-layer FLOPs and bytes are stored beside the totals.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))
import _disc_oracle as oracle  # noqa: E402  (the architecture table and fmap_shapes only)

PEAK_F32_MFMA = 157.3e12
HBM_BW = 8.0e12


def layer_costs(N: int, T: int):
    """Per convolution: FLOPs (2 per multiply-add) and compulsory bytes (weights once, input once, output once), from shapes."""
    shapes = oracle.fmap_shapes(T)
    rows = []
    for i, (key, (cin, cout, k, s, pad, g)) in enumerate(oracle.conv_keys()):
        c, l, p = shapes[i]
        out_elems = N * c * l * p
        first = key.endswith("convs.0")
        in_elems = N * T if first else N * shapes[i - 1][0] * shapes[i - 1][1] * shapes[i - 1][2]
        w_elems = cout * (cin // g) * k
        rows.append({"key": key, "flops": 2.0 * out_elems * (cin // g) * k, "bytes": 4.0 * (w_elems + in_elems + out_elems),
                     "weight_bytes": 4.0 * w_elems, "out_elems": out_elems})
    return rows


def torch_forward(dev_params, y):
    """The restatement on the framework's own GPU operators, fp32, weights already on the device."""
    N, T = y.shape
    fmaps = []
    for d, p in enumerate(oracle.PERIODS):
        x = y[:, None, :]
        if T % p:
            x = F.pad(x, (0, p - T % p), mode="reflect")
        x = x.reshape(N, 1, -1, p)
        for i, (_, _, _, s, pad, _) in enumerate(oracle.MPD_CONVS):
            w, b = dev_params[f"mpd.discriminators.{d}.convs.{i}"]
            x = F.leaky_relu(F.conv2d(x, w[..., None], b, stride=(s, 1), padding=(pad, 0)), 0.1)
            fmaps.append(x)
        w, b = dev_params[f"mpd.discriminators.{d}.conv_post"]
        fmaps.append(F.conv2d(x, w[..., None], b, padding=(1, 0)))
    x0 = y[:, None, :]
    for d in range(3):
        if d:
            x0 = F.avg_pool1d(x0, 4, 2, padding=2)
        x = x0
        for i, (_, _, _, s, pad, g) in enumerate(oracle.MSD_CONVS):
            w, b = dev_params[f"msd.discriminators.{d}.convs.{i}"]
            x = F.leaky_relu(F.conv1d(x, w, b, stride=s, padding=pad, groups=g), 0.1)
            fmaps.append(x)
        w, b = dev_params[f"msd.discriminators.{d}.conv_post"]
        fmaps.append(F.conv1d(x, w, b, padding=1))
    return fmaps


def timed(fn, iters):
    """Median device-event milliseconds of fn() over iters runs."""
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), [float(t) for t in ts]


def main() -> None:
    from viettts_amd import _lib
    from viettts_amd.hifigan.disc_synth import synthetic_disc_checkpoint
    from viettts_amd.hifigan.discriminators import Discriminators, fold_checkpoint

    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", type=Path, default=REPO / "profiles" / "disc_bench.json")
    ap.add_argument("--shapes", default="16x8192,8x80000", help="BxT pairs; rows per pass = 2 B")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    params = fold_checkpoint(synthetic_disc_checkpoint(8642))
    d = Discriminators(dev).load_params(params)
    dev_params = {k: (torch.from_numpy(w).to(dev), torch.from_numpy(b).to(dev)) for k, (w, b) in params.items()}
    result = {"device": torch.cuda.get_device_name(0), "peak_fp32_mfma_flops": PEAK_F32_MFMA, "iters": a.iters, "shapes": []}
    for spec in a.shapes.split(","):
        B, T = (int(v) for v in spec.split("x"))
        N = 2 * B
        y = torch.from_numpy(oracle.make_inputs(B, T, 7)).to(dev)
        costs = layer_costs(N, T)
        flops, byts, wbytes = sum(c["flops"] for c in costs), sum(c["bytes"] for c in costs), sum(c["weight_bytes"] for c in costs)
        nf, ns = d.buffer_sizes(N, T)
        fb = torch.empty(nf, dtype=torch.float32, device=dev)
        sb = torch.empty(ns, dtype=torch.float32, device=dev)
        loss_out = torch.empty(_lib.DISC_LOSS_FLOATS, dtype=torch.float32, device=dev)
        fwd = lambda: d.forward_raw(y, fb, sb)  # noqa: E731
        both = lambda: (d.forward_raw(y, fb, sb), d.losses_raw(fb, sb, B, T, loss_out))  # noqa: E731
        entry = {"B": B, "T": T, "rows": N, "flops": flops, "bytes": byts, "weight_bytes": wbytes,
                 "bound_ms_compute": flops / PEAK_F32_MFMA * 1e3, "bound_ms_hbm": byts / HBM_BW * 1e3}
        entry["bound"] = "compute" if entry["bound_ms_compute"] >= entry["bound_ms_hbm"] else "memory (weights + feature maps)"
        baseline_error = None
        try:
            with torch.no_grad():
                torch_forward(dev_params, y)
            torch.cuda.synchronize()
        except Exception as e:  # recorded, never replaced by something else
            baseline_error = f"{type(e).__name__}: {e}"[:400]
        fwd(), both()
        torch.cuda.synchronize()
        lib_ms, base_ms, both_ms = [], [], []
        for _ in range(a.iters):  # alternated in one process
            lib_ms.append(timed(fwd, 1)[0])
            both_ms.append(timed(both, 1)[0])
            if baseline_error is None:
                with torch.no_grad():
                    base_ms.append(timed(lambda: torch_forward(dev_params, y), 1)[0])
        entry["forward_ms"] = float(np.median(lib_ms))
        entry["forward_ms_all"] = lib_ms
        entry["forward_losses_ms"] = float(np.median(both_ms))
        entry["tflops"] = flops / entry["forward_ms"] / 1e9
        entry["share_of_fp32_mfma_peak"] = flops / (entry["forward_ms"] * 1e-3) / PEAK_F32_MFMA
        if baseline_error is None:
            entry["torch_rocm_fp32_forward_ms"] = float(np.median(base_ms))
            entry["torch_rocm_fp32_forward_ms_all"] = base_ms
            entry["speedup_vs_torch_rocm"] = entry["torch_rocm_fp32_forward_ms"] / entry["forward_ms"]
        else:
            entry["torch_rocm_fp32_forward_ms"] = None
            entry["baseline_error"] = baseline_error
        entry["layers"] = [{"key": c["key"], "gflop": c["flops"] / 1e9, "mbytes": c["bytes"] / 1e6} for c in costs]
        result["shapes"].append(entry)
        print(json.dumps({k: v for k, v in entry.items() if not k.endswith("_all") and k != "layers"}), flush=True)
        del fb, sb
        torch.cuda.empty_cache()
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(json.dumps(result, indent=1) + "\n")
    print(f"wrote {a.out} at {time.strftime('%Y-%m-%d')}")


if __name__ == "__main__":
    main()
