"""Time the true-peak meter and limiter (viettts_amd/csrc/limiter.hip) next to the HBM floor of the passes its design makes and next to the
same contract composed from torch-ROCm operators.  Device-event timing, warm-up, medians.

    python tools/limiter_bench.py [--iters 20] [--no-torch] [--output profiles/limiter_bench.json]

The HBM floor counts what the design moves over an assumed peak; it is an estimate, not a measurement.  true_peak reads the samples once.
limit reads them twice, writes and reads the fp32 envelope, and writes the output.  normalize adds the loudness meter's two reads.  The torch
composition is Resampler(fs, 4 fs) (this project's kernel: torch has no polyphase operator) -> abs -> max over 4 for the envelope, then
where / -max_pool1d(-req) / avg_pool1d on replicate-padded rows / min / two multiplies / clamp-round-to-int16; its mean is an fp32 pooling sum,
so it follows the contract only to fp32 summation error.  The figures are recorded, never asserted by a test.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from viettts_amd.audio import Resampler  # noqa: E402
from viettts_amd.limiter import TruePeakLimiter  # noqa: E402
from viettts_amd.loudness import LoudnessMeter  # noqa: E402

N, S, RATE = 64, 262144, 16000
HBM_BYTES_PER_S = 8.0e12  # MI355X: 8 TB/s peak
# launches per call at N <= 128 rows, read off the host code (limiter.hip, loudness.hip), not measured
LAUNCHES = {"true_peak": 2, "limit": 4, "normalize": 3 + 1 + 4}


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


def torch_envelope(rs: Resampler, y: torch.Tensor) -> torch.Tensor:
    u = rs(y)
    return torch.maximum(y.abs(), u.abs().view(y.shape[0], y.shape[1], 4).amax(dim=2))


def torch_limit(rs: Resampler, y: torch.Tensor, g: torch.Tensor, c: float, W: int) -> torch.Tensor:
    """The contract from torch operators, into PCM16."""
    p = torch_envelope(rs, y)
    gp = g[:, None] * p
    req = torch.where(gp <= c, torch.ones_like(gp), c / gp)
    held = -F.max_pool1d(F.pad(-req[:, None, :], (W, W), mode="replicate"), 2 * W + 1, stride=1)
    mean = F.avg_pool1d(F.pad(held, (W, W), mode="replicate"), 2 * W + 1, stride=1)[:, 0, :]
    out = (g[:, None] * y) * torch.minimum(req, mean)
    return (out.clamp(-1.0, 1.0).double() * 32767.0).round().to(torch.int16)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--output", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "limiter_bench needs the GPU"
    dev = torch.device("cuda:0")
    lim = TruePeakLimiter(RATE, device=dev)
    meter = LoudnessMeter(RATE, device=dev)
    gen = torch.Generator(device="cpu").manual_seed(1770)
    t = torch.arange(S) / float(RATE)
    f = 90.0 + 160.0 * torch.rand((N, 1), generator=gen)
    amp = 0.02 + 0.3 * torch.rand((N, 1), generator=gen)
    y = amp * torch.sin(2 * np.pi * f * t[None, :]) + 0.01 * torch.randn((N, S), generator=gen)
    y[:, 1000::32768] += 0.6  # eight plosive-like clicks a row: what the sample-peak cap backs a whole row off for
    y = y.to(dev)
    W = lim.lookahead
    c = float(np.float32(10.0 ** (-1.0 / 20.0)))
    # limit: every row 6 dB over the ceiling, so that every workgroup takes the limiting path
    g6 = (c * 10.0 ** (6.0 / 20.0) / lim.true_peak(y)).contiguous()
    rec = {"N": N, "S": S, "sample_rate": RATE, "lookahead_samples": W, "hbm_bytes_per_s_assumed": HBM_BYTES_PER_S, "launches_per_call": LAUNCHES}
    rec["true_peak_f32"] = stats(timed_ms(lambda: lim.true_peak(y), a.warmup, a.iters))
    rec["limit_f32_to_pcm16"] = stats(timed_ms(lambda: lim.limit(y, gains=g6, out_dtype="pcm16"), a.warmup, a.iters))
    rec["normalize_f32_to_pcm16"] = stats(timed_ms(lambda: lim.normalize(y, target=-16.0, out_dtype="pcm16", meter=meter), a.warmup, a.iters))
    _, r = lim.normalize(y, target=-16.0, out_dtype="pcm16", meter=meter)
    rec["normalize_rows_limited"] = int((r.min_gain < 1.0).sum())
    rec["true_peak_hbm_bytes"] = N * S * 4
    rec["limit_hbm_bytes"] = N * S * (4 + 4 + 4 + 4 + 2)
    rec["normalize_hbm_bytes"] = rec["limit_hbm_bytes"] + 2 * N * S * 4
    for k in ("true_peak", "limit", "normalize"):
        rec[f"{k}_hbm_floor_ms_estimate"] = 1e3 * rec[f"{k}_hbm_bytes"] / HBM_BYTES_PER_S
    rec["true_peak_over_hbm_floor"] = rec["true_peak_f32"]["median_ms"] / rec["true_peak_hbm_floor_ms_estimate"]
    rec["limit_over_hbm_floor"] = rec["limit_f32_to_pcm16"]["median_ms"] / rec["limit_hbm_floor_ms_estimate"]
    rec["normalize_over_hbm_floor"] = rec["normalize_f32_to_pcm16"]["median_ms"] / rec["normalize_hbm_floor_ms_estimate"]
    rec["samples_per_s_limit"] = N * S / (rec["limit_f32_to_pcm16"]["median_ms"] * 1e-3)
    if not a.no_torch:
        rs = Resampler(RATE, 4 * RATE, device=dev)
        rec["torch_true_peak_f32"] = stats(timed_ms(lambda: torch_envelope(rs, y).amax(dim=1), a.warmup, a.iters))
        rec["torch_limit_f32_to_pcm16"] = stats(timed_ms(lambda: torch_limit(rs, y, g6, c, W), a.warmup, a.iters))

        def torch_normalize():
            i = meter(y).integrated
            g = torch.where(torch.isfinite(i), torch.minimum(10.0 ** ((-16.0 - i.double()) / 20.0), torch.tensor(10.0 ** 1.5, device=dev, dtype=torch.float64)).float(),
                            torch.ones_like(i))
            return torch_limit(rs, y, g, c, W)

        rec["torch_normalize_f32_to_pcm16"] = stats(timed_ms(torch_normalize, a.warmup, a.iters))
        ours, _ = lim.limit(y, gains=g6, out_dtype="pcm16")
        theirs = torch_limit(rs, y, g6, c, W)
        rec["true_peak_equals_torch_composition"] = bool(torch.equal(lim.true_peak(y), torch_envelope(rs, y).amax(dim=1)))
        rec["pcm16_max_abs_difference_vs_torch_steps"] = int((ours.int() - theirs.int()).abs().max())
        rec["speedup_vs_torch_true_peak"] = rec["torch_true_peak_f32"]["median_ms"] / rec["true_peak_f32"]["median_ms"]
        rec["speedup_vs_torch_limit"] = rec["torch_limit_f32_to_pcm16"]["median_ms"] / rec["limit_f32_to_pcm16"]["median_ms"]
        rec["speedup_vs_torch_normalize"] = rec["torch_normalize_f32_to_pcm16"]["median_ms"] / rec["normalize_f32_to_pcm16"]["median_ms"]
        rs.close()
    print(json.dumps(rec), flush=True)
    lim.close()
    meter.close()
    if a.output:
        doc = {"method": f"device events around the public calls (allocation of the results included), {a.warmup} warm-ups, medians of {a.iters} runs in one process; "
                         "hbm floors = bytes the design moves (true_peak: the samples once; limit: the samples twice, the fp32 envelope written and read, the PCM16 output; "
                         "normalize: the meter's two reads more) over an assumed 8 TB/s peak, an estimate and not a measurement; torch side = this project's Resampler kernel for the "
                         "4x signal, then abs / amax / where / max_pool1d / avg_pool1d / minimum / mul / clamp / round from torch-ROCm; launches_per_call is read off the host code",
               "not_measured": "other rates and look-aheads (W = 960 stages and sums 12 x as much per sample), PCM16 input, ragged batches, more than 128 rows, "
                               "counters or per-kernel times, a second device",
               "device": torch.cuda.get_device_name(0), "cases": [rec]}
        Path(a.output).parent.mkdir(parents=True, exist_ok=True)
        Path(a.output).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
