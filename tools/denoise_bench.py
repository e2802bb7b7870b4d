"""Time the fused denoiser (viettts_amd/csrc/denoise.hip) next to the same operation composed from the transform's own kernels
(``Denoiser.composed``: ``Stft.forward``, the gain as torch operators, ``Stft.inverse``) and next to the HBM floor of the bytes the fused pass
moves.  Device-event timing, warm-up, the two sides alternated window by window in one process, medians.

    python tools/denoise_bench.py [--iters 10] [--inner 10] [--output profiles/denoise_bench.json]

64 rows of 262 144 samples at n_fft 1024 / win 1024 / hop 256 and at 2048 / 1200 / 240, torch.stft's framing: the fused pass into fp32 and into
PCM16, and the composition into fp32.  The figures are recorded, never asserted by a test.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from viettts_amd.denoise import Denoiser  # noqa: E402

N, S, RATE = 64, 262144, 16000
RESOLUTIONS = ((1024, 1024, 256), (2048, 1200, 240))
HBM_BYTES_PER_S = 8.0e12  # MI355X: 8 TB/s peak
STRENGTH = 0.5


def alternated_ms(fns: dict, warmup: int, iters: int, inner: int) -> dict:
    """``iters`` rounds; in a round every side gets one window of ``inner`` back-to-back calls.  Per-call milliseconds per side."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(iters):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / inner)
    return {name: {"median_ms": float(np.median(t)), "min_ms": float(min(t)), "max_ms": float(max(t)), "runs": len(t)} for name, t in times.items()}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--inner", type=int, default=10, help="back-to-back calls per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--output", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "denoise_bench needs the GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(2021)
    t = torch.arange(S) / float(RATE)
    f0 = 90.0 + 160.0 * torch.rand((N, 1), generator=g)
    env = (0.5 + 0.5 * torch.sin(2 * np.pi * (2.5 + 1.5 * torch.rand((N, 1), generator=g)) * t[None, :])) ** 2 + 0.02
    x = (env * sum(torch.sin(2 * np.pi * h * f0 * t[None, :]) / h for h in range(1, 9)) * 0.2 + 0.002 * torch.randn((N, S), generator=g)).to(dev)
    cases = []
    for res in RESOLUTIONS:
        dn = Denoiser(res + ("center",), device=dev)
        dn.bias_from_noise(x[:, :16384].contiguous())  # about the signal's own mean magnitude: at this strength a real share of the bins clamps
        out32, out16 = torch.zeros_like(x), torch.zeros((N, S), dtype=torch.int16, device=dev)
        fused, comp = dn.fused(x, strength=STRENGTH), dn.composed(x, strength=STRENGTH)
        T = dn.stft.num_frames(S)
        rec = {"N": N, "S": S, "resolution": list(res), "framing": "center", "frames_per_row": T, "blocking": list(dn.blocking()), "strength": STRENGTH,
               "hbm_bytes_per_s_assumed": HBM_BYTES_PER_S, "calls_per_timed_window": a.inner,
               "share_of_bins_clamped": float((dn._magnitudes(dn.stft.forward(x[:4].contiguous())) <= STRENGTH * dn.bias).float().mean()),
               "fused_max_abs_difference_vs_composed": float((fused - comp).abs().max()), "output_peak": float(fused.abs().max()),
               "composed_spectrum_bytes": N * T * dn.n_bins * 8}
        times = alternated_ms({"fused_f32": lambda: dn.fused(x, strength=STRENGTH, out=out32), "fused_pcm16": lambda: dn.fused(x, strength=STRENGTH, out_dtype="pcm16", out=out16),
                               "composed_f32": lambda: dn.composed(x, strength=STRENGTH)}, a.warmup, a.iters, a.inner)
        for name, per_sample in (("fused_f32", 8), ("fused_pcm16", 6)):
            times[name]["hbm_bytes"] = N * S * per_sample
            times[name]["hbm_floor_ms"] = 1e3 * N * S * per_sample / HBM_BYTES_PER_S
            times[name]["over_hbm_floor"] = times[name]["median_ms"] / times[name]["hbm_floor_ms"]
        rec.update(times)
        rec["composed_over_fused_f32"] = times["composed_f32"]["median_ms"] / times["fused_f32"]["median_ms"]
        cases.append(rec)
        print(json.dumps(rec), flush=True)
        dn.close()
    if a.output:
        doc = {"method": f"device events around windows of {a.inner} back-to-back public calls, the three sides alternated window by window, {a.iters} windows each after "
                         f"{a.warmup} warm-up calls, medians in one process; the fused calls write into a preallocated output, composed() allocates its spectrum and "
                         "its result inside the window (that is the composition a caller has); hbm floors = the samples read and written once (4 + 4 or 4 + 2 bytes) over an "
                         "assumed 8 TB/s peak, not a measurement",
               "device": torch.cuda.get_device_name(0), "cases": cases}
        Path(a.output).parent.mkdir(parents=True, exist_ok=True)
        Path(a.output).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
