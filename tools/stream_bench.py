"""Time to the FIRST audio of one sentence: the un-streamed path against ``viettts_amd.streaming.synthesize_stream``, alternated call by call in
one process on one GPU.

    python tools/stream_bench.py [--iters 30] [--warmup 5] [--chunks 16,32,64] [--out profiles/stream_latency.json]

Workload: tools/latency_bench.py's B = 1 sentence (the median-length line of tests/golden/text/transcript.txt), synthetic checkpoints, the bf16
vocoder.  Modes: "unstreamed" = duration model -> ``frame_plan`` -> ``AcousticModel.__call__(to_host=False)`` -> generator on the kept frames ->
host (every sample arrives at once: first = last); "stream_cN" = ``synthesize_stream`` with ``chunk_frames = N``.  Per call, host wall clock from
the call to the first chunk's samples on the host and to the last chunk's, the frames the decoder had been asked for when the first chunk left,
and for the streamed modes the wall clock of every step (chunk k's arrival).  Reported: median, min and max over --iters calls per mode.  Nothing
is asserted: the numbers are what README and DESIGN.md section 6j quote.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
from latency_bench import SILENCE, stats, workloads  # noqa: E402
from viettts_amd.hifigan.config import V1  # noqa: E402
from viettts_amd.hifigan.generator import Generator  # noqa: E402
from viettts_amd.hifigan.synth import synthetic_params  # noqa: E402
from viettts_amd.nat import text2mel as t2m  # noqa: E402
from viettts_amd.nat.acoustic import AcousticModel  # noqa: E402
from viettts_amd.nat.duration import DurationModel  # noqa: E402
from viettts_amd.nat.synth import synthetic_acoustic_checkpoint, synthetic_duration_checkpoint  # noqa: E402
from viettts_amd.streaming import synthesize_stream  # noqa: E402

SEED = 7


def unstreamed(dm, am, gen, toks):
    """The path as it was before streaming existed.  Returns (first us, last us, frames decoded at the first sample, per-step us, frames kept)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    frames, nfr, trail = t2m.frame_plan([toks], dm([toks]), SILENCE)
    T = nfr[0] - trail[0]
    mel = am([toks], frames, nfr, dropout_seeds=[SEED], to_host=False)
    wav = gen(mel[:, :T].contiguous())[0].cpu().numpy()  # (.cpu() synchronises)
    t = (time.perf_counter() - t0) * 1e6
    assert wav.shape == (256 * T,)
    return t, t, nfr[0], [t], T


def streamed(dm, am, gen, toks, chunk):
    torch.cuda.synchronize()
    info, steps, n = {}, [], 0
    t0 = time.perf_counter()
    for c in synthesize_stream(toks, dm, am, gen, silence_duration=SILENCE, dropout_seed=SEED, chunk_frames=chunk, info=info):
        steps.append((time.perf_counter() - t0) * 1e6)
        n += c.shape[0]
    assert n == info["samples"]
    return steps[0], steps[-1], info["frames_decoded_at_first_chunk"], steps, info["frames"]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--chunks", type=str, default="16,32,64")
    ap.add_argument("--out", type=Path, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "stream_bench needs the GPU"
    dm = DurationModel()
    dm.load_params(*synthetic_duration_checkpoint())
    am = AcousticModel(device="cuda:0")
    am.load_params(*synthetic_acoustic_checkpoint())
    gen = Generator(V1, device="cuda:0", dtype="bf16")
    gen.load_params(synthetic_params(V1, 4321, "scaled"))
    toks = workloads()["b1"][0]
    modes = [("unstreamed", lambda: unstreamed(dm, am, gen, toks))]
    modes += [(f"stream_c{c}", lambda c=int(c): streamed(dm, am, gen, toks, c)) for c in a.chunks.split(",") if c]
    for _ in range(a.warmup):
        for _, run in modes:
            run()
    runs = {name: {"first": [], "last": [], "decoded": [], "steps": []} for name, _ in modes}
    kept = None
    for _ in range(a.iters):  # alternated: whatever else loads the box hits every mode
        for name, run in modes:
            first, last, decoded, steps, kept = run()
            r = runs[name]
            r["first"].append(first), r["last"].append(last), r["decoded"].append(decoded), r["steps"].append(steps)
    rec = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "vocoder": "bf16", "silence_duration": SILENCE,
           "tokens": len(toks), "frames_kept": int(kept), "audio_seconds": kept * 256 / 16000, "modes": {}}
    for name, r in runs.items():
        m = {"first_chunk_us": stats(r["first"]), "last_chunk_us": stats(r["last"]), "frames_decoded_before_first_yield": int(np.median(r["decoded"])),
             "step_arrival_us_median": [float(v) for v in np.median(np.asarray(r["steps"]), axis=0)]}
        rec["modes"][name] = m
        print(json.dumps({name: {k: m[k] for k in ("first_chunk_us", "last_chunk_us", "frames_decoded_before_first_yield")}}), flush=True)
    if a.out:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text(json.dumps(rec, indent=1) + "\n")
    gen.close()
    am.close()
    dm.close()


if __name__ == "__main__":
    main()
