"""Time the fused waveform -> log-mel pass (viettts_amd/csrc/mel.hip) next to the same transform composed from torch ops and next
to the HBM time of its input plus output bytes.  Device-event timing, warm-up, median of --iters runs per shape.

    python tools/mel_bench.py [--iters 30] [--no-torch]

One JSON line per shape.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from viettts_amd.nat.dsp import MelFilter  # noqa: E402

HBM_BYTES_PER_S = 8.0e12  # MI355X peak
SHAPES = ((64, 262144), (1, 131072))


def median_ms(fn, warmup: int, iters: int) -> float:
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
    return float(np.median(times))


def torch_composed(y: torch.Tensor, melfb: torch.Tensor, window: torch.Tensor) -> torch.Tensor:
    yp = torch.nn.functional.pad(y.unsqueeze(1), (384, 384), mode="reflect").squeeze(1)
    spec = torch.stft(yp, 1024, hop_length=256, win_length=1024, window=window, center=False, onesided=True, return_complex=True)
    mag = torch.sqrt(spec.real * spec.real + spec.imag * spec.imag + 1e-9)
    return torch.log(torch.clamp(torch.matmul(melfb, mag), min=1e-5)).transpose(1, 2)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mel_bench needs the GPU"
    assert a.iters >= 20
    dev = torch.device("cuda:0")
    mf = MelFilter(16000, 1024, 80, 0.0, 8000, device=dev)
    melfb = torch.from_numpy(mf.melfb).to(dev)
    window = torch.hann_window(1024, device=dev)
    for N, S in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(5)
        y = (0.1 * torch.randn((N, S), generator=g)).to(dev)
        pcm = (y * 32768.0).round().clamp(-32768, 32767).to(torch.int16)
        T = mf.num_frames(S)
        out = torch.empty((N, T, 80), dtype=torch.float32, device=dev)
        rec = {"N": N, "S": S, "frames": N * T}
        rec["fused_f32_ms"] = median_ms(lambda: mf(y, out=out), a.warmup, a.iters)
        rec["fused_pcm16_ms"] = median_ms(lambda: mf(pcm, out=out), a.warmup, a.iters)
        rec["hbm_floor_f32_ms"] = 1e3 * (y.numel() * 4 + out.numel() * 4) / HBM_BYTES_PER_S
        rec["frames_per_s_f32"] = N * T / (rec["fused_f32_ms"] * 1e-3)
        if not a.no_torch:
            try:
                ref = torch_composed(y, melfb, window)
                torch.cuda.synchronize()
                rec["max_abs_vs_torch"] = float((mf(y) - ref).abs().max())
                rec["torch_composed_ms"] = median_ms(lambda: torch_composed(y, melfb, window), a.warmup, a.iters)
                rec["speedup_vs_torch"] = rec["torch_composed_ms"] / rec["fused_f32_ms"]
            except RuntimeError as e:  # torch's FFT is not usable on this device: reported, not hidden
                rec["torch_composed_ms"] = None
                rec["torch_error"] = str(e)[:200]
        print(json.dumps(rec), flush=True)
    mf.close()


if __name__ == "__main__":
    main()
