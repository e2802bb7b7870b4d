"""Time the loudness meter (viettts_amd/csrc/loudness.hip) next to the HBM floor of the passes its design makes and next to the same
contract on the host (scipy.signal.lfilter + numpy; torch has no IIR operator and torchaudio is not a dependency).  Device-event timing,
warm-up, medians.

    python tools/loudness_bench.py [--iters 20] [--host-rows 4] [--no-host] [--output profiles/loudness_bench.json]

The HBM floor counts what the design moves: measure reads the samples twice (segment end states, then hop sums); normalise reads them once
more and writes the output once.  The host side is timed on --host-rows rows and scaled to the batch, and includes what a user would have
to do today: the device-to-host copy of the samples.  The figures are recorded, never asserted by a test.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from viettts_amd.loudness import LoudnessMeter  # noqa: E402

N, S, RATE = 64, 262144, 16000
HBM_BYTES_PER_S = 8.0e12  # MI355X: 8 TB/s peak


def timed_ms(fn, warmup: int, iters: int) -> list:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return times


def stats(times: list) -> dict:
    return {"median_ms": float(np.median(times)), "min_ms": float(min(times)), "max_ms": float(max(times)), "runs": len(times)}


def host_contract(x: np.ndarray, coef: np.ndarray, rate: int, target: float = -23.0):
    """include/vtts_loudness.h for one float32 row with scipy and numpy: (integrated, PCM16 at the target)."""
    from scipy.signal import lfilter

    z = lfilter(coef[5:8], [1.0, coef[8], coef[9]], lfilter(coef[0:3], [1.0, coef[3], coef[4]], x.astype(np.float64)))
    H = rate // 10
    nH = len(z) // H
    e = (z[: nH * H] ** 2).reshape(nH, H).sum(axis=1)
    zb = (e[:-3] + e[1:-2] + e[2:-1] + e[3:]) / (4.0 * H)
    with np.errstate(divide="ignore"):
        l = -0.691 + 10.0 * np.log10(zb)
        keep = l > -70.0
        rel = -0.691 + 10.0 * np.log10(zb[keep].mean()) - 10.0 if keep.any() else -np.inf
        keep &= l > rel
        integrated = -0.691 + 10.0 * np.log10(zb[keep].mean()) if keep.any() else -np.inf
    g = np.float32(1.0)
    if np.isfinite(integrated):
        g = np.float32(min(10.0 ** ((target - integrated) / 20.0), 10.0 ** 1.5, 10.0 ** (-1.0 / 20.0) / float(np.abs(x).max())))
    return integrated, np.rint(np.clip((x * g).astype(np.float64), -1.0, 1.0) * 32767.0).astype(np.int16)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-rows", type=int, default=4)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--output", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "loudness_bench needs the GPU"
    dev = torch.device("cuda:0")
    m = LoudnessMeter(RATE, device=dev)
    g = torch.Generator(device="cpu").manual_seed(1770)
    t = torch.arange(S) / float(RATE)
    f = 90.0 + 160.0 * torch.rand((N, 1), generator=g)
    amp = 0.02 + 0.3 * torch.rand((N, 1), generator=g)
    y = (amp * torch.sin(2 * np.pi * f * t[None, :]) + 0.01 * torch.randn((N, S), generator=g)).to(dev)
    pcm = (y * 32767.0).round().to(torch.int16)
    rec = {"N": N, "S": S, "sample_rate": RATE, "hbm_bytes_per_s_assumed": HBM_BYTES_PER_S}
    rec["measure_f32"] = stats(timed_ms(lambda: m(y), a.warmup, a.iters))
    rec["measure_pcm16"] = stats(timed_ms(lambda: m(pcm), a.warmup, a.iters))
    rec["measure_normalize_f32_to_pcm16"] = stats(timed_ms(lambda: m.normalize(y, out_dtype="pcm16"), a.warmup, a.iters))
    rec["measure_hbm_bytes_f32"] = 2 * N * S * 4
    rec["measure_normalize_hbm_bytes_f32_to_pcm16"] = 3 * N * S * 4 + N * S * 2
    rec["measure_hbm_floor_ms"] = 1e3 * rec["measure_hbm_bytes_f32"] / HBM_BYTES_PER_S
    rec["measure_normalize_hbm_floor_ms"] = 1e3 * rec["measure_normalize_hbm_bytes_f32_to_pcm16"] / HBM_BYTES_PER_S
    rec["measure_over_hbm_floor"] = rec["measure_f32"]["median_ms"] / rec["measure_hbm_floor_ms"]
    rec["measure_normalize_over_hbm_floor"] = rec["measure_normalize_f32_to_pcm16"]["median_ms"] / rec["measure_normalize_hbm_floor_ms"]
    rec["samples_per_s_measure_f32"] = N * S / (rec["measure_f32"]["median_ms"] * 1e-3)
    if not a.no_host:
        coef = m.coefficients()
        rows = min(a.host_rows, N)
        r = m(y)
        out, _ = m.normalize(y, out_dtype="pcm16")
        torch.cuda.synchronize()
        host_contract(y[0, : 4 * RATE].cpu().numpy(), coef, RATE)  # warm-up: scipy's import and first call stay out of the timing
        t0 = time.perf_counter()
        host = y[:rows].cpu().numpy()
        t1 = time.perf_counter()
        res = [host_contract(host[b], coef, RATE) for b in range(rows)]
        t2 = time.perf_counter()
        rec["host_rows_timed"] = rows
        rec["host_copy_ms_scaled_to_batch"] = 1e3 * (t1 - t0) * N / rows
        rec["host_scipy_numpy_ms_scaled_to_batch"] = 1e3 * (t2 - t1) * N / rows
        rec["integrated_max_abs_difference_vs_host_lu"] = float(max(abs(float(r.integrated[b]) - res[b][0]) for b in range(rows)))
        rec["pcm16_max_abs_difference_vs_host_steps"] = int(max(np.abs(out[b].cpu().numpy().astype(np.int32) - res[b][1].astype(np.int32)).max() for b in range(rows)))
        rec["speedup_vs_host_measure_normalize"] = (rec["host_copy_ms_scaled_to_batch"] + rec["host_scipy_numpy_ms_scaled_to_batch"]) / rec["measure_normalize_f32_to_pcm16"]["median_ms"]
    print(json.dumps(rec), flush=True)
    m.close()
    if a.output:
        doc = {"method": f"device events around the public calls (allocation of the results included), {a.warmup} warm-ups, medians of {a.iters} runs in one process; "
                         "hbm floors = bytes the design moves (measure: the samples twice; normalise: once more, plus the output) over an assumed 8 TB/s peak, "
                         "not a measurement; host side = device-to-host copy + scipy.signal.lfilter + numpy on a few rows, scaled to the batch",
               "device": torch.cuda.get_device_name(0), "cases": [rec]}
        Path(a.output).parent.mkdir(parents=True, exist_ok=True)
        Path(a.output).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
