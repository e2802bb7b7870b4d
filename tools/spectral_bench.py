"""Time the spectral distances (viettts_amd/csrc/spectral.hip) next to the HBM floor of the passes their design makes and next to the same
contract written with torch-ROCm operators on the same device (``torch.stft`` plus reductions).  Device-event timing, warm-up, medians.

    python tools/spectral_bench.py [--iters 20] [--inner 5] [--torch-rows 64] [--output profiles/spectral_bench.json]

64 rows of 262 144 samples at 16 kHz: the three-resolution meter (Parallel WaveGAN's resolutions), each resolution alone, and each with both
magnitude spectrograms written.  The HBM floor counts what the design moves: each resolution reads both signals once (the frames' overlap is
served from LDS) and writes 32 B per workgroup; with ``mags=True`` it writes 4 B per bin, frame and signal besides.  The figures are recorded,
never asserted by a test.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from viettts_amd.spectral import PWG_RESOLUTIONS, MultiResolutionStft  # noqa: E402

N, S, RATE = 64, 262144, 16000
HBM_BYTES_PER_S = 8.0e12  # MI355X: 8 TB/s peak


def timed_ms(fn, warmup: int, iters: int, inner: int) -> list:
    """``iters`` windows of ``inner`` back-to-back calls each; per-call milliseconds."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / inner)
    return times


def stats(times: list) -> dict:
    return {"median_ms": float(np.median(times)), "min_ms": float(min(times)), "max_ms": float(max(times)), "runs": len(times)}


def torch_contract(x: torch.Tensor, y: torch.Tensor, cfg, w: torch.Tensor):
    """include/vtts_spectral.h at one resolution with torch operators, [N, S] float32 -> (sc, logmag, lsd) float64 [N] (sums in torch's order)."""
    n_fft, win, hop = cfg
    px, py = (torch.stft(s, n_fft, hop_length=hop, win_length=win, window=w, center=True, pad_mode="reflect", return_complex=True).abs().square().clamp_min(1e-7)
              for s in (x, y))  # [N, NB, T]
    mx, my = px.sqrt().double(), py.sqrt().double()
    L = (py.double() / px.double()).log()
    sc = (my - mx).square().sum(dim=(1, 2)).sqrt() / mx.square().sum(dim=(1, 2)).sqrt()
    logmag = 0.5 * L.abs().mean(dim=(1, 2))
    lsd = (10.0 / np.log(10.0) * L).square().mean(dim=1).sqrt().mean(dim=1)
    return sc, logmag, lsd


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5, help="back-to-back calls per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-rows", type=int, default=N, help="rows the torch restatement is timed on (scaled to the batch)")
    ap.add_argument("--output", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "spectral_bench needs the GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(2020)
    t = torch.arange(S) / float(RATE)
    f0 = 90.0 + 160.0 * torch.rand((N, 1), generator=g)
    env = (0.5 + 0.5 * torch.sin(2 * np.pi * (2.5 + 1.5 * torch.rand((N, 1), generator=g)) * t[None, :])) ** 2 + 0.02
    x = env * sum(torch.sin(2 * np.pi * h * f0 * t[None, :]) / h for h in range(1, 9)) * 0.2 + 0.002 * torch.randn((N, S), generator=g)
    y = 0.9 * x + 0.02 * torch.randn((N, S), generator=g)
    x, y = x.to(dev), y.to(dev)
    mr = MultiResolutionStft(PWG_RESOLUTIONS, dev)
    r = mr(x, y)
    torch.cuda.synchronize()
    rec = {"N": N, "S": S, "rate": RATE, "resolutions": [list(c) for c in PWG_RESOLUTIONS], "hbm_bytes_per_s_assumed": HBM_BYTES_PER_S,
           "calls_per_timed_window": a.inner, "frames_per_block": [m.frames_per_block for m in mr.meters]}
    rec["mrstft_f32"] = stats(timed_ms(lambda: mr(x, y), a.warmup, a.iters, a.inner))
    rows = max(1, min(a.torch_rows, N))
    xr, yr = x[:rows].contiguous(), y[:rows].contiguous()
    total_bytes, torch_total = 0, 0.0
    for cfg, m, p in zip(PWG_RESOLUTIONS, mr.meters, r.per_resolution):
        key = "n_fft_%d" % cfg[0]
        T = m.num_frames(S)
        groups = -(-T // m.frames_per_block)
        c = {"frames_per_row": T, "meter_f32": stats(timed_ms(lambda: m(x, y), a.warmup, a.iters, a.inner)),
             "meter_f32_with_mags": stats(timed_ms(lambda: m(x, y, mags=True), a.warmup, max(3, a.iters // 4), 1))}
        c["hbm_bytes"] = 2 * N * S * 4 + N * groups * 32 * 2
        c["hbm_bytes_with_mags"] = c["hbm_bytes"] + 2 * N * T * m.n_bins * 4
        c["hbm_floor_ms"] = 1e3 * c["hbm_bytes"] / HBM_BYTES_PER_S
        c["hbm_floor_with_mags_ms"] = 1e3 * c["hbm_bytes_with_mags"] / HBM_BYTES_PER_S
        c["meter_over_hbm_floor"] = c["meter_f32"]["median_ms"] / c["hbm_floor_ms"]
        c["frames_per_s"] = 2 * N * T / (c["meter_f32"]["median_ms"] * 1e-3)  # transforms: both signals
        w = torch.from_numpy(m.window()[(cfg[0] - cfg[1]) // 2 : (cfg[0] - cfg[1]) // 2 + cfg[1]].copy()).to(dev)
        ref = torch_contract(xr, yr, cfg, w)
        tt = timed_ms(lambda: torch_contract(xr, yr, cfg, w), 1, max(3, a.iters // 4), 1)
        c["torch_operators_ms_scaled_to_batch"] = {k: (v * N / rows if k.endswith("_ms") else v) for k, v in stats(tt).items()}
        c["speedup_vs_torch_operators"] = c["torch_operators_ms_scaled_to_batch"]["median_ms"] / c["meter_f32"]["median_ms"]
        for name, got, want in zip(("sc", "logmag", "lsd"), (p.sc, p.logmag, p.lsd), ref):
            c[name + "_max_abs_difference_vs_torch"] = float((got[:rows] - want).abs().max())
        rec[key] = c
        total_bytes += c["hbm_bytes"]
        torch_total += c["torch_operators_ms_scaled_to_batch"]["median_ms"]
    rec["torch_rows_timed"] = rows
    rec["mrstft_hbm_bytes"] = total_bytes
    rec["mrstft_hbm_floor_ms"] = 1e3 * total_bytes / HBM_BYTES_PER_S
    rec["mrstft_over_hbm_floor"] = rec["mrstft_f32"]["median_ms"] / rec["mrstft_hbm_floor_ms"]
    rec["mrstft_torch_operators_ms_scaled_to_batch"] = torch_total
    rec["mrstft_speedup_vs_torch_operators"] = torch_total / rec["mrstft_f32"]["median_ms"]
    rec["samples_per_s_mrstft_f32"] = N * S / (rec["mrstft_f32"]["median_ms"] * 1e-3)
    print(json.dumps(rec), flush=True)
    mr.close()
    if a.output:
        doc = {"method": f"device events around windows of {a.inner} back-to-back public calls (allocation of the results included; with mags: single calls), {a.warmup} "
                         f"warm-ups, medians of {a.iters} windows in one process; hbm floors = bytes the design moves (both signals once per resolution, 32 B per "
                         "workgroup written and read back; with mags 4 B per bin, frame and signal) over an assumed 8 TB/s peak, not a measurement; torch side = the "
                         "same contract with torch.stft and reductions on the same device, the three resolutions' medians added",
               "device": torch.cuda.get_device_name(0), "cases": [rec]}
        Path(a.output).parent.mkdir(parents=True, exist_ok=True)
        Path(a.output).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
