"""Time the intelligibility meter (viettts_amd/csrc/stoi.hip) next to the HBM floor of the passes its design makes and next to the same
contract written with torch-ROCm operators on the same device (unfold, rfft, a band matrix, unfold again; the ragged kept-frame gather
row by row, as a user would write it).  Device-event timing, warm-up, medians.

    python tools/stoi_bench.py [--iters 20] [--inner 10] [--torch-rows 64] [--output profiles/stoi_bench.json]

64 rows of 262 144 samples at 16 kHz: ``wav_stoi`` converts both signals to 10 kHz (163 840 samples) first; the meter alone is timed on that
output.  The HBM floor counts what the design moves: the energy pass reads the clean samples once, the spectrum pass reads both signals
once (the frames' overlap is left to the caches) and writes 120 B per frame; the conversion reads both signals at 16 kHz and writes them at
10 kHz.  The figures are recorded, never asserted by a test.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from viettts_amd.audio import resampler  # noqa: E402
from viettts_amd.stoi import StoiMeter, wav_stoi  # noqa: E402

N, S16, RATE = 64, 262144, 16000
HBM_BYTES_PER_S = 8.0e12  # MI355X: 8 TB/s peak
BAND_LO = (7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219)


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


def torch_contract(x: torch.Tensor, y: torch.Tensor, w: torch.Tensor, band: torch.Tensor):
    """include/vtts_stoi.h with torch operators, [N, S] float32 at 10 kHz -> (stoi [N], estoi [N]) float64 (sums in torch's own order)."""
    eps, c = 2.0 ** -52, 1.0 + 10.0 ** (15.0 / 20.0)
    K = -(-(x.shape[1] - 256) // 128)
    p, q = x.unfold(1, 256, 128)[:, :K] * w, y.unfold(1, 256, 128)[:, :K] * w  # [N, K, 256]
    e = p.double().square().sum(-1)
    keep = e > 1e-4 * e.max(dim=1, keepdim=True).values
    out = []
    for b in range(x.shape[0]):  # ragged from here on
        idx = keep[b].nonzero()[:, 0]
        T = idx.numel() - 1
        if T < 30:
            out.append((float("nan"), float("nan")))
            continue
        mags = []
        for f in (p[b], q[b]):
            f = f[idx]
            u = f[:T].clone()
            u[:, 128:] += f[1:, :128]
            u[1:, :128] += f[: T - 1, 128:]
            z = torch.fft.rfft(u * w, 512)
            mags.append(((z.real.square() + z.imag.square()).double() @ band).sqrt().T)  # [15, T]
        xs, ys = (m.unfold(1, 30, 1).permute(1, 0, 2) for m in mags)  # [M, 15, 30]

        def normalise(a, dim):
            a = a - a.mean(dim=dim, keepdim=True)
            return a / (a.norm(dim=dim, keepdim=True) + eps)

        yp = torch.minimum(ys * (xs.norm(dim=2, keepdim=True) / (ys.norm(dim=2, keepdim=True) + eps)), c * xs)
        d = (normalise(xs, 2) * normalise(yp, 2)).sum(dim=(1, 2)) / 15.0
        de = (normalise(normalise(xs, 2), 1) * normalise(normalise(ys, 2), 1)).sum(dim=(1, 2)) / 30.0
        out.append((d.mean(), de.mean()))
    return torch.tensor([[float(v) for v in r] for r in out], dtype=torch.float64).T


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10, help="back-to-back calls per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-rows", type=int, default=N, help="rows the torch restatement is timed on (scaled to the batch)")
    ap.add_argument("--output", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "stoi_bench needs the GPU"
    dev = torch.device("cuda:0")
    m = StoiMeter(device=dev)
    g = torch.Generator(device="cpu").manual_seed(2011)
    t = torch.arange(S16) / float(RATE)
    f0 = 90.0 + 160.0 * torch.rand((N, 1), generator=g)
    env = (0.5 + 0.5 * torch.sin(2 * np.pi * (2.5 + 1.5 * torch.rand((N, 1), generator=g)) * t[None, :])) ** 2 + 0.02
    x16 = env * sum(torch.sin(2 * np.pi * h * f0 * t[None, :]) / h for h in range(1, 9)) * 0.2
    x16[:, S16 // 3 : S16 // 3 + 20000] *= 1e-3  # a stretch that falls to the 40 dB rule
    y16 = 0.9 * x16 + 0.02 * torch.randn((N, S16), generator=g)
    x16, y16 = x16.to(dev), y16.to(dev)
    rs = resampler(RATE, 10000, dev)
    x10, y10 = rs(x16), rs(y16)
    S10 = x10.shape[1]
    r = m(x10, y10)
    torch.cuda.synchronize()
    K = m.num_frames(S10)
    kept = int(r.n_kept.sum())
    rec = {"N": N, "S_16k": S16, "S_10k": S10, "frames_per_row": K, "kept_frames": kept, "segments": int(r.n_segments.sum()),
           "hbm_bytes_per_s_assumed": HBM_BYTES_PER_S, "calls_per_timed_window": a.inner}
    rec["meter_f32"] = stats(timed_ms(lambda: m(x10, y10), a.warmup, a.iters, a.inner))
    rec["meter_f32_with_series"] = stats(timed_ms(lambda: m(x10, y10, series=True), a.warmup, a.iters, a.inner))
    rec["wav_stoi_16k_f32"] = stats(timed_ms(lambda: wav_stoi(x16, y16, rate=RATE, meter=m), a.warmup, a.iters, a.inner))
    rec["meter_hbm_bytes"] = 3 * N * S10 * 4 + N * K * 12 + kept * 120
    rec["wav_stoi_hbm_bytes"] = rec["meter_hbm_bytes"] + 2 * N * (S16 + S10) * 4
    rec["meter_hbm_floor_ms"] = 1e3 * rec["meter_hbm_bytes"] / HBM_BYTES_PER_S
    rec["wav_stoi_hbm_floor_ms"] = 1e3 * rec["wav_stoi_hbm_bytes"] / HBM_BYTES_PER_S
    rec["meter_over_hbm_floor"] = rec["meter_f32"]["median_ms"] / rec["meter_hbm_floor_ms"]
    rec["wav_stoi_over_hbm_floor"] = rec["wav_stoi_16k_f32"]["median_ms"] / rec["wav_stoi_hbm_floor_ms"]
    rec["samples_per_s_meter_f32"] = N * S10 / (rec["meter_f32"]["median_ms"] * 1e-3)
    rows = max(1, min(a.torch_rows, N))
    w = torch.from_numpy(m.window()).to(dev)
    band = torch.zeros((257, 15), dtype=torch.float64, device=dev)
    for j in range(15):
        band[BAND_LO[j] : BAND_LO[j + 1], j] = 1.0
    xr, yr = x10[:rows].contiguous(), y10[:rows].contiguous()
    ref = torch_contract(xr, yr, w, band)
    tt = timed_ms(lambda: torch_contract(xr, yr, w, band), 1, max(3, a.iters // 4), 1)
    rec["torch_rows_timed"] = rows
    rec["torch_operators_ms_scaled_to_batch"] = {k: (v * N / rows if k.endswith("_ms") else v) for k, v in stats(tt).items()}
    rec["stoi_max_abs_difference_vs_torch"] = float((r.stoi[:rows].double().cpu() - ref[0]).abs().max())
    rec["estoi_max_abs_difference_vs_torch"] = float((r.estoi[:rows].double().cpu() - ref[1]).abs().max())
    rec["speedup_vs_torch_operators"] = rec["torch_operators_ms_scaled_to_batch"]["median_ms"] / rec["meter_f32"]["median_ms"]
    print(json.dumps(rec), flush=True)
    m.close()
    if a.output:
        doc = {"method": f"device events around windows of {a.inner} back-to-back public calls (allocation of the results included), {a.warmup} warm-ups, medians of "
                         f"{a.iters} windows in one process; hbm floors = bytes the design moves (clean samples once for the energies, both signals once for the "
                         "spectra, 12 B per candidate frame, 120 B per kept frame; wav_stoi: plus both signals in at 16 kHz and out at 10 kHz) over an assumed 8 TB/s "
                         "peak, not a measurement; torch side = the same contract with torch operators on the same device, its ragged part row by row, each call "
                         "ending in the host read of its results",
               "device": torch.cuda.get_device_name(0), "cases": [rec]}
        Path(a.output).parent.mkdir(parents=True, exist_ok=True)
        Path(a.output).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
