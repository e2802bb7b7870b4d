"""Time the fused YIN pass (viettts_amd/csrc/pitch.hip) next to the same contract composed from torch-ROCm operators and next to the
lane-operation estimate of its difference function.  Device-event timing, warm-up, medians; both sides alternate in one process.

    python tools/pitch_bench.py [--iters 20] [--torch-iters 3] [--no-torch] [--output profiles/pitch_bench.json]

The torch side follows include/vtts_pitch.h step by step (reflect pad, unfold, broadcast difference over all lags, cumulative sum, pick,
refinement) but sums in torch's own order, so its results are compared by voicing decision and tau*, not bit for bit; frames are taken in
chunks so that the [frames, lags, 512] difference tensor stays under --chunk-bytes.  The figures are recorded, never asserted by a test.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from viettts_amd.pitch import PitchTracker  # noqa: E402

SHAPES = ((64, 262144), (1, 16384))
NFFT, HOP, PAD, W = 1024, 256, 384, 512
# the estimate's machine: 256 CUs x 4 SIMDs x 16 fp32 lanes per clock at 2.4 GHz, no packed or dual issue (the contract forbids the FMA)
LANE_OPS_PER_S = 256 * 64 * 2.4e9


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


def torch_composed(y: torch.Tensor, trk: PitchTracker, chunk_bytes: int):
    """(f0, aperiodicity, candidate, tau) [N, T] of the header's contract with torch operators."""
    N = y.shape[0]
    tmin, tmax, thr = trk.tau_min, trk.tau_max, float(np.float32(trk.threshold))
    base = (NFFT - W - tmax) // 2
    yp = torch.nn.functional.pad(y.unsqueeze(1), (PAD, PAD), mode="reflect").squeeze(1)
    fr = yp.unfold(1, NFFT, HOP).reshape(-1, NFFT)  # [N T, 1024], a view until the reshape
    per = max(1, chunk_bytes // (4 * (tmax + 1) * W))
    taus = torch.arange(tmax + 1, device=y.device, dtype=torch.float32)
    outs = []
    for f0 in range(0, fr.shape[0], per):
        x = fr[f0 : f0 + per]
        e = x[:, None, base : base + W] - x[:, base : base + W + tmax].unfold(1, W, 1)  # [F, lags, 512]
        d = (e * e).sum(-1)
        d[:, 0] = 0
        run = torch.cumsum(d, dim=1)
        c = torch.where(run > 0, d * taus / torch.where(run > 0, run, torch.ones_like(run)), torch.ones_like(d))
        c[:, 0] = 1
        nxt = torch.cat([c[:, 1:], torch.full_like(c[:, :1], float("inf"))], dim=1)
        hit = (c < thr) & (nxt >= c)
        hit[:, :tmin] = False
        voiced = hit.any(dim=1)
        tau = torch.where(voiced, hit.int().argmax(dim=1), tmin + c[:, tmin:].argmin(dim=1))
        b = c.gather(1, tau[:, None])[:, 0]
        a = c.gather(1, (tau - 1)[:, None])[:, 0]
        g = c.gather(1, (tau + 1).clamp(max=tmax)[:, None])[:, 0]
        den = (a + g) - (b + b)
        ok = (tau + 1 <= tmax) & (den > 0)
        delta = (0.5 * (a - g) / torch.where(ok, den, torch.ones_like(den))).clamp(-1, 1)
        cand = float(trk.sample_rate) / torch.where(ok, tau.float() + delta, tau.float())
        outs.append(torch.stack([torch.where(voiced, cand, torch.zeros_like(cand)), b, cand, tau.float()]))
    return torch.cat(outs, dim=1).reshape(4, N, -1)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--torch-iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunk-bytes", type=int, default=1 << 30)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--output", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "pitch_bench needs the GPU"
    dev = torch.device("cuda:0")
    trk = PitchTracker(device=dev)
    lags = trk.tau_max + 1
    cases = []
    for N, S in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(11)
        t = torch.arange(S) / 16000.0
        f = 90.0 + 160.0 * torch.rand((N, 1), generator=g)
        y = sum(torch.sin(2 * np.pi * f * k * t[None, :]) / k for k in range(1, 6))
        y = (0.2 * y / y.abs().amax(dim=1, keepdim=True) + 0.01 * torch.randn((N, S), generator=g)).to(dev)
        pcm = (y * 32767.0).round().to(torch.int16)
        T = trk.num_frames(S)
        lane_ops = float(W) * lags * 3 * N * T
        rec = {"N": N, "S": S, "frames": N * T, "tau_min": trk.tau_min, "tau_max": trk.tau_max, "difference_lane_ops": lane_ops,
               "valu_estimate_ms": 1e3 * lane_ops / LANE_OPS_PER_S}
        rec["fused_f32"] = stats(timed_ms(lambda: trk(y), a.warmup, a.iters))
        rec["fused_pcm16"] = stats(timed_ms(lambda: trk(pcm), a.warmup, a.iters))
        rec["frames_per_s_f32"] = N * T / (rec["fused_f32"]["median_ms"] * 1e-3)
        rec["fused_over_valu_estimate"] = rec["fused_f32"]["median_ms"] / rec["valu_estimate_ms"]
        if not a.no_torch:
            ref = torch_composed(y, trk, a.chunk_bytes)
            got = trk(y)
            torch.cuda.synchronize()
            voiced_eq = (got.f0 > 0) == (ref[0] > 0)
            tau_eq = voiced_eq & (torch.round(trk.sample_rate / got.candidate) == torch.round(trk.sample_rate / ref[2]))
            rec["voicing_equal_fraction_vs_torch"] = float(voiced_eq.float().mean())
            rec["voicing_and_rounded_period_equal_fraction_vs_torch"] = float(tau_eq.float().mean())
            rec["voiced_fraction"] = float((got.f0 > 0).float().mean())
            rec["torch"] = stats(timed_ms(lambda: torch_composed(y, trk, a.chunk_bytes), 1, a.torch_iters))
            rec["fused_f32_again"] = stats(timed_ms(lambda: trk(y), 1, a.iters))  # after the torch side: the spread between the two is the noise
            rec["speedup_vs_torch"] = rec["torch"]["median_ms"] / rec["fused_f32"]["median_ms"]
        print(json.dumps(rec), flush=True)
        cases.append(rec)
    trk.close()
    if a.output:
        doc = {"method": f"device events, {a.warmup} warm-ups, medians of {a.iters} (kernel) and {a.torch_iters} (torch) runs in one process; torch side = reflect pad + "
                         "unfold + broadcast difference over all lags in chunks of frames + cumsum + pick + refinement; valu_estimate_ms = 512 * (tau_max + 1) * 3 lane "
                         "operations per frame over 256 CUs * 64 lanes * 2.4 GHz (an estimate from lane counts and clock, not a measurement)",
               "device": torch.cuda.get_device_name(0), "cases": cases}
        Path(a.output).parent.mkdir(parents=True, exist_ok=True)
        Path(a.output).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
