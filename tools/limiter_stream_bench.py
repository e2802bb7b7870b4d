"""Time the streamed true-peak limiter's push against what it replaces, on one GPU -> profiles/limiter_stream_bench.json.

    python tools/limiter_stream_bench.py [--out profiles/limiter_stream_bench.json]

Shapes: one push of 1 x 8192 and one of 32 x 8192 samples at 16 kHz, mid-row (state present), every row 6 dB over the ceiling.  Legs, device
events around the public calls, 3 warm-ups, medians of 20, one process, the legs interleaved:

    push       LimiterStream.push (the fused kernel and the result merge)
    composed   the same bits from the un-streamed public calls: TruePeakLimiter.limit on 288 samples of history + the chunk, then a slice
               (checked against the push with torch.equal before anything is timed)
    to_pcm16   audio.to_pcm16 of the chunk: what the streamed paths pay today, without any level control

and synthesize_stream on the synthetic models, wall time to the first and to the last chunk, with ``limit`` off and on.  ``spread`` is a leg's
minimum and maximum over its 20 runs.
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

CHUNK, HIST, WARM, RUNS = 8192, 288, 3, 20


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def push_legs(n: int, dev) -> dict:
    import _limiter_oracle as O
    from viettts_amd.audio import to_pcm16
    from viettts_amd.limiter import TruePeakLimiter, stream_emit

    lim = TruePeakLimiter(16000, dev)
    Wn = lim.lookahead
    S = CHUNK * (WARM + RUNS + 2)
    rows = [O.speech(900 + b, S) for b in range(n)]
    gains = [float(O.gain_for(x, 16000, 6.0)) for x in rows]
    x = torch.from_numpy(np.stack(rows)).to(dev)
    g = torch.tensor(gains, device=dev)
    times = {"push": [], "composed": [], "to_pcm16": []}
    with lim.open_stream(n, CHUNK, out_dtype="pcm16") as s:
        for b in range(n):
            s.reset(b, gains[b])
        s.push(x[:, :CHUNK])
        R = CHUNK
        F = stream_emit(0, 0, R, False, Wn)
        for it in range(WARM + RUNS):
            chunk = x[:, R:R + CHUNK]
            Fn = stream_emit(R, F, CHUNK, False, Wn)
            t_push, (y, em) = _timed(lambda: s.push(chunk))

            def composed():
                win = torch.cat([x[:, F - HIST:R], chunk], dim=1)  # what a caller without the fused kernel keeps and joins
                yy, _ = lim.limit(win, gains=g, out_dtype="pcm16")
                return yy[:, HIST:HIST + Fn - F].contiguous()

            t_comp, yc = _timed(composed)
            t_pcm, _ = _timed(lambda: to_pcm16(chunk.contiguous()))
            assert em == [Fn - F] * n and torch.equal(y.view(n, -1), yc)
            if it >= WARM:
                times["push"].append(t_push), times["composed"].append(t_comp), times["to_pcm16"].append(t_pcm)
            R, F = R + CHUNK, Fn
    lim.close()
    out = {k: _stats(v) for k, v in times.items()}
    spread = max(out[k]["max_ms"] - out[k]["min_ms"] for k in ("push", "composed"))
    out["push_not_slower_than_composed_within_spread"] = bool(out["push"]["median_ms"] <= out["composed"]["median_ms"] + spread)
    return out


def stream_legs(dev) -> dict:
    from viettts_amd.hifigan.config import V1
    from viettts_amd.hifigan.generator import Generator
    from viettts_amd.hifigan.synth import synthetic_params
    from viettts_amd.nat.acoustic import AcousticModel
    from viettts_amd.nat.config import FLAGS
    from viettts_amd.nat.duration import DurationModel
    from viettts_amd.nat.synth import synthetic_acoustic_checkpoint, synthetic_duration_checkpoint
    from viettts_amd.streaming import synthesize_stream

    dm, am = DurationModel(device=dev), AcousticModel(device=dev)
    dm.load_params(*synthetic_duration_checkpoint())
    am.load_params(*synthetic_acoustic_checkpoint())
    gen = Generator(V1, device=dev, dtype="bf16")
    gen.load_params(synthetic_params(V1, 4321, "scaled"))
    rng = np.random.default_rng(41)
    toks = [FLAGS.sil_index] + list(rng.integers(4, 90, size=40)) + [FLAGS.sil_index]
    times = {(lim, which): [] for lim in (False, True) for which in ("first", "last")}
    info = {}
    for it in range(WARM + RUNS):
        for lim in (False, True):
            kw = dict(limit=True, gain_db=20.0) if lim else {}
            torch.cuda.synchronize()
            t0, first = time.perf_counter(), None
            for _ in synthesize_stream(toks, dm, am, gen, silence_duration=0.05, chunk_frames=32, first_chunk_frames=8, out_dtype="pcm16", info=info, **kw):
                first = first or time.perf_counter()
            t1 = time.perf_counter()
            if it >= WARM:
                times[lim, "first"].append(1e3 * (first - t0)), times[lim, "last"].append(1e3 * (t1 - t0))
    gen.close(), dm.close(), am.close()
    return {"frames": info["frames"], "samples": info["samples"], "chunk_frames": 32, "first_chunk_frames": 8,
            **{f"limit_{'on' if lim else 'off'}_to_{which}_chunk": _stats(v) for (lim, which), v in times.items()}}


def main(argv=None) -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "limiter_stream_bench.json"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"device": torch.cuda.get_device_name(dev), "sample_rate": 16000, "chunk": CHUNK, "history": HIST, "warmups": WARM, "runs": RUNS,
           "rows_1": push_legs(1, dev), "rows_32": push_legs(32, dev), "synthesize_stream": stream_legs(dev)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
