"""Time the streamed resampler's push against what it replaces, on one GPU -> profiles/resample_stream_bench.json.

    python tools/resample_stream_bench.py [--output profiles/resample_stream_bench.json]

Shapes: one mid-row push (history present) of 1 x 8192 and of 32 x 8192 samples, 16 kHz -> 48 kHz and 16 kHz -> 44.1 kHz, into PCM16.  Legs,
device events around the public calls, 3 warm-ups, medians of 20, one process, the legs interleaved:

    push       ResamplerStream.push (the one fused kernel)
    composed   the same bits from the un-streamed public call: Resampler on history + chunk, then a slice.  The window starts at a multiple
               of M samples at or below the history's first sample, so that its outputs keep their phases (checked against the push with
               torch.equal before anything is timed)
    to_pcm16   audio.to_pcm16 of the chunk alone: the floor, no conversion

and stream_mel on 208 synthetic frames (chunks of 32, the first of 8), wall time to the first and to the last chunk, with and without
``out_rate=48000``.  ``min_ms`` and ``max_ms`` are a leg's spread over its 20 runs.  Anything not in the file is unmeasured.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

CHUNK, WARM, RUNS = 8192, 3, 20


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def push_legs(n: int, out_rate: int, dev) -> dict:
    import _audio_oracle as A
    from viettts_amd.audio import Resampler, resample_emit, to_pcm16

    rs = Resampler(16000, out_rate, dev)
    L, M, half = rs.L, rs.M, rs.half
    kp4 = (-(-(2 * half + 1) // L) + 3) // 4 * 4
    S = CHUNK * (WARM + RUNS + 2)
    x = torch.from_numpy(np.stack([A.speechlike(np.random.default_rng(900 + b), S) for b in range(n)])).to(dev)
    times = {"push": [], "composed": [], "to_pcm16": []}
    with rs.open_stream(n, CHUNK, out_dtype="pcm16") as s:
        s.push(x[:, :CHUNK])
        R = CHUNK
        F = resample_emit(0, 0, R, False, L, M, half)
        for it in range(WARM + RUNS):
            chunk = x[:, R:R + CHUNK]
            Fn = resample_emit(R, F, CHUNK, False, L, M, half)
            t_push, (y, em) = _timed(lambda: s.push(chunk))
            B = max(0, (F * M + half) // L - (kp4 - 1)) // M * M  # the window's first sample: a multiple of M under the history
            mB = B * L // M

            def composed():
                win = torch.cat([x[:, B:R], chunk], dim=1)  # what a caller without the fused kernel keeps and joins
                yy = rs(win, out_dtype="pcm16")
                return yy[:, F - mB:Fn - mB].contiguous()

            t_comp, yc = _timed(composed)
            t_pcm, _ = _timed(lambda: to_pcm16(chunk.contiguous()))
            assert em == [Fn - F] * n and torch.equal(y.view(n, -1), yc)
            per_push = Fn - F
            if it >= WARM:
                times["push"].append(t_push), times["composed"].append(t_comp), times["to_pcm16"].append(t_pcm)
            R, F = R + CHUNK, Fn
    rs.close()
    out = {k: _stats(v) for k, v in times.items()}
    out["outputs_per_push"] = per_push
    spread = max(out[k]["max_ms"] - out[k]["min_ms"] for k in ("push", "composed"))
    out["push_not_slower_than_composed_within_spread"] = bool(out["push"]["median_ms"] <= out["composed"]["median_ms"] + spread)
    return out


def stream_legs(dev) -> dict:
    from viettts_amd.hifigan.config import V1
    from viettts_amd.hifigan.generator import Generator
    from viettts_amd.hifigan.synth import synthetic_mel, synthetic_params
    from viettts_amd.streaming import stream_mel

    gen = Generator(V1, device=dev, dtype="bf16")
    gen.load_params(synthetic_params(V1, 4321, "scaled"))
    mel = torch.from_numpy(np.ascontiguousarray(synthetic_mel(1, 208, 4)[0])).to(dev)
    times = {(rate, which): [] for rate in (None, 48000) for which in ("first", "last")}
    total = {}
    for it in range(WARM + RUNS):
        for rate in (None, 48000):
            torch.cuda.synchronize()
            t0, first, count = time.perf_counter(), None, 0
            for c in stream_mel(gen, mel, 32, 8, out_dtype="pcm16", out_rate=rate):
                first = first or time.perf_counter()
                count += len(c)
            t1 = time.perf_counter()
            total[rate] = count
            if it >= WARM:
                times[rate, "first"].append(1e3 * (first - t0)), times[rate, "last"].append(1e3 * (t1 - t0))
    gen.close()
    return {"frames": 208, "chunk_frames": 32, "first_chunk_frames": 8, "samples_16000": total[None], "samples_48000": total[48000],
            **{f"out_rate_{rate or 'none'}_to_{which}_chunk": _stats(v) for (rate, which), v in times.items()}}


def main(argv=None) -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--output", default=os.path.join(REPO, "profiles", "resample_stream_bench.json"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"device": torch.cuda.get_device_name(dev), "in_rate": 16000, "chunk": CHUNK, "out_dtype": "pcm16", "warmups": WARM, "runs": RUNS}
    for rate in (48000, 44100):
        for n in (1, 32):
            res[f"to_{rate}_rows_{n}"] = push_legs(n, rate, dev)
    res["stream_mel"] = stream_legs(dev)
    os.makedirs(os.path.dirname(a.output), exist_ok=True)
    with open(a.output, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
