"""Time the complex STFT stages (viettts_amd/csrc/stft.hip) next to the HBM floor of the bytes each pass moves and next to the same contract
written with torch-ROCm operators on the same device (``torch.stft`` / ``torch.istft`` and torchaudio's Griffin-Lim update spelled out).
Device-event timing, warm-up, medians.

    python tools/stft_bench.py [--iters 10] [--inner 20] [--output profiles/stft_bench.json]

64 rows of 262 144 samples at n_fft 1024 / win 1024 / hop 256, torch.stft's framing: the forward complex transform, the inverse, one
Griffin-Lim iteration (inverse + projection) and ``GriffinLim(32)`` end to end.  The figures are recorded, never asserted by a test.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from viettts_amd.stft import GriffinLim, Stft, random_phases  # noqa: E402

N, S, RATE = 64, 262144, 16000
RES = (1024, 1024, 256)
HBM_BYTES_PER_S = 8.0e12  # MI355X: 8 TB/s peak


def timed_ms(fn, warmup: int, iters: int, inner: int) -> dict:
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
    return {"median_ms": float(np.median(times)), "min_ms": float(min(times)), "max_ms": float(max(times)), "runs": len(times)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20, help="back-to-back calls per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--output", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "stft_bench needs the GPU"
    dev = torch.device("cuda:0")
    n_fft, win, hop = RES
    g = torch.Generator(device="cpu").manual_seed(2021)
    t = torch.arange(S) / float(RATE)
    f0 = 90.0 + 160.0 * torch.rand((N, 1), generator=g)
    env = (0.5 + 0.5 * torch.sin(2 * np.pi * (2.5 + 1.5 * torch.rand((N, 1), generator=g)) * t[None, :])) ** 2 + 0.02
    x = (env * sum(torch.sin(2 * np.pi * h * f0 * t[None, :]) / h for h in range(1, 9)) * 0.2 + 0.002 * torch.randn((N, S), generator=g)).to(dev)
    st = Stft(*RES, framing="center", device=dev)
    w = torch.from_numpy(st.window()).to(dev)
    T, NB = st.num_frames(S), st.n_bins
    spec = st.forward(x)
    mag = spec.abs().contiguous()
    init = random_phases(mag.shape, dev, 0)
    tprev, out = torch.zeros_like(spec), torch.zeros_like(spec)
    alpha = 0.99 / 1.99

    def t_stft(v):
        return torch.stft(v, n_fft, hop_length=hop, win_length=win, window=w, center=True, pad_mode="reflect", return_complex=True)  # [N, NB, T]

    def t_istft(z):
        return torch.istft(z, n_fft, hop_length=hop, win_length=win, window=w, center=True, length=S)

    tspec = t_stft(x)
    tmag, tstate = tspec.abs(), {"tprev": torch.zeros_like(tspec)}

    def t_iteration(z):
        rebuilt = t_stft(t_istft(z))
        ang = rebuilt - alpha * tstate["tprev"]
        tstate["tprev"] = rebuilt
        return tmag * (ang / (ang.abs() + 1e-16))

    def t_griffinlim(n_iter):
        z, tstate["tprev"] = tmag * init.transpose(1, 2), torch.zeros_like(tspec)
        for _ in range(n_iter):
            z = t_iteration(z)
        return t_istft(z)

    spec_bytes, wav_bytes = N * T * NB * 8, N * S * 4
    moved = {"forward": wav_bytes + spec_bytes, "inverse": spec_bytes + wav_bytes,
             "iteration": (spec_bytes + wav_bytes) + (wav_bytes + spec_bytes // 2 + spec_bytes + 2 * spec_bytes)}  # inverse + (wav, mag, tprev in; spec, tprev out)
    moved["griffinlim_32"] = 32 * moved["iteration"] + moved["inverse"]
    gl = GriffinLim(st, 32, 0.99)
    ours = {"forward": lambda: st.forward(x), "inverse": lambda: st.inverse(spec), "iteration": lambda: st.project(st.inverse(spec), mag, tprev, momentum=0.99, out=out),
            "griffinlim_32": lambda: gl(mag, init=init)}
    theirs = {"forward": lambda: t_stft(x), "inverse": lambda: t_istft(tspec), "iteration": lambda: t_iteration(tspec), "griffinlim_32": lambda: t_griffinlim(32)}
    rec = {"N": N, "S": S, "resolution": list(RES), "framing": "center", "frames_per_row": T, "blocking": list(st.blocking()), "hbm_bytes_per_s_assumed": HBM_BYTES_PER_S,
           "calls_per_timed_window": a.inner}
    rec["forward_max_abs_difference_vs_torch"] = float((spec.transpose(1, 2) - tspec).abs().max())
    rec["inverse_max_abs_difference_vs_torch"] = float((st.inverse(spec) - t_istft(tspec)).abs().max())
    for name in ("forward", "inverse", "iteration", "griffinlim_32"):
        long = name == "griffinlim_32"
        c = {"stft_hip": timed_ms(ours[name], 1 if long else a.warmup, 3 if long else a.iters, 1 if long else a.inner),
             "torch_operators": timed_ms(theirs[name], 1, 3, 1 if long else 5)}
        c["hbm_bytes"] = moved[name]
        c["hbm_floor_ms"] = 1e3 * moved[name] / HBM_BYTES_PER_S
        c["over_hbm_floor"] = c["stft_hip"]["median_ms"] / c["hbm_floor_ms"]
        c["speedup_vs_torch_operators"] = c["torch_operators"]["median_ms"] / c["stft_hip"]["median_ms"]
        rec[name] = c
    print(json.dumps(rec), flush=True)
    if a.output:
        doc = {"method": f"device events around windows of {a.inner} back-to-back public calls (allocation of the results included; the torch side: 3 windows of 5 calls; "
                         f"griffinlim_32 on either side: 3 single calls), {a.warmup} warm-ups, medians in one process; hbm floors = bytes each pass reads and writes once (waveform 4 B, spectrum 8 B, "
                         "magnitudes 4 B per entry) over an assumed 8 TB/s peak, not a measurement; torch side = the same contract with torch.stft, torch.istft and "
                         "torchaudio's griffinlim update written with torch operators on the same device",
               "device": torch.cuda.get_device_name(0), "cases": [rec]}
        Path(a.output).parent.mkdir(parents=True, exist_ok=True)
        Path(a.output).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
