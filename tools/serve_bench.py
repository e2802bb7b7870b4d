"""Many listeners on one GPU: ``viettts_amd.serving.SpeechPool`` against the same requests served one after another with
``viettts_amd.streaming.synthesize_stream``, and the cost of the pooled decoder step against the step it generalises.

    python tools/serve_bench.py [--slots 32] [--rates 5,20,80] [--chunk 32] [--iters 9] [--out profiles/serve_latency.json]

Requests: the 26 sentences of tests/golden/text/transcript.txt, synthetic checkpoints, the bf16 vocoder, PCM16 out.  Arrivals: exponential gaps from
numpy's PCG64 with a fixed seed, at each of --rates requests per second; the clock is the host's wall clock, a request is submitted by the first
round (pool) or served by the first free turn (fifo) at or after its arrival.  Per request: arrival -> first samples on the host, arrival -> last
samples; reported per mode and rate: median and worst.  Nothing is asserted about these.

Step cost: ``pool_decode`` of 32 rows admitted at tick 0 against ``stream_decode`` of the same 32 rows, all frames in one call, host wall clock
around a synchronised call, the two alternated --iters times in one process; the ratio of the medians is recorded (the bar: within 5 %, twice the box-to-box spread).
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
from viettts_amd.hifigan.config import V1  # noqa: E402
from viettts_amd.hifigan.generator import Generator  # noqa: E402
from viettts_amd.hifigan.synth import synthetic_params  # noqa: E402
from viettts_amd.nat import text2mel as t2m  # noqa: E402
from viettts_amd.nat.acoustic import AcousticModel  # noqa: E402
from viettts_amd.nat.duration import DurationModel  # noqa: E402
from viettts_amd.nat.synth import synthetic_acoustic_checkpoint, synthetic_duration_checkpoint, transcript_sentences  # noqa: E402
from viettts_amd.serving import SpeechPool  # noqa: E402
from viettts_amd.streaming import synthesize_stream  # noqa: E402

SILENCE, ARRIVAL_SEED = 0.05, 2024


def summary(first, last):
    ms = lambda v: {"median_ms": float(np.median(v)) * 1e3, "worst_ms": float(np.max(v)) * 1e3}
    return {"first_samples": ms(first), "last_samples": ms(last)}


def serve_pool(dm, am, gen, sents, arrivals, slots, Lmax, Fmax, chunk):
    sp = SpeechPool(dm, am, gen, slots, Lmax, Fmax, chunk_frames=chunk)
    first, last, owner, nxt = {}, {}, {}, 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while nxt < len(sents) or not sp.idle:
        now = time.perf_counter() - t0
        while nxt < len(sents) and arrivals[nxt] <= now:
            owner[sp.submit(sents[nxt], silence_duration=SILENCE, dropout_seed=nxt)] = nxt
            nxt += 1
        if sp.idle:  # nobody to serve: wait for the next arrival
            time.sleep(max(0.0, arrivals[nxt] - (time.perf_counter() - t0)))
            continue
        for rid, _, done in sp.step():
            t = time.perf_counter() - t0 - arrivals[owner[rid]]
            first.setdefault(rid, t)
            if done:
                last[rid] = t
    sp.close()
    return [first[r] for r in sorted(first)], [last[r] for r in sorted(last)]


def serve_fifo(dm, am, gen, sents, arrivals, chunk):
    first, last = [], []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i, toks in enumerate(sents):
        time.sleep(max(0.0, arrivals[i] - (time.perf_counter() - t0)))
        f = None
        for _ in synthesize_stream(toks, dm, am, gen, silence_duration=SILENCE, dropout_seed=i, chunk_frames=chunk, out_dtype="pcm16"):
            if f is None:
                f = time.perf_counter() - t0 - arrivals[i]
        first.append(f)
        last.append(time.perf_counter() - t0 - arrivals[i])
    return first, last


def step_cost(dm, am, sents, iters):
    """Wall clock of every frame step of 32 rows: the session's decode against the pool's, alternated."""
    rows = [sents[i % len(sents)] for i in range(32)]
    frames, nfr, _ = t2m.frame_plan(rows, dm(rows), SILENCE)
    Lmax, Fmax, seeds = max(len(r) for r in rows), int(max(nfr)), list(range(32))
    t = {"stream_decode": [], "pool_decode": []}
    for it in range(iters + 2):
        with am.open_stream(rows, frames, nfr, max_window=32, dropout_seeds=seeds) as st:
            torch.cuda.synchronize()
            a = time.perf_counter()
            st.decode(Fmax)
            torch.cuda.synchronize()
            ts = time.perf_counter() - a
        with am.open_pool(32, Lmax, Fmax, 32) as pool:
            for s in range(32):
                pool.admit(s, rows[s], frames[s], nfr[s], dropout_seed=seeds[s])
            torch.cuda.synchronize()
            a = time.perf_counter()
            pool.decode(Fmax)
            torch.cuda.synchronize()
            tp = time.perf_counter() - a
        if it >= 2:  # two warm-up rounds
            t["stream_decode"].append(ts), t["pool_decode"].append(tp)
    ms, mp = float(np.median(t["stream_decode"])), float(np.median(t["pool_decode"]))
    return {"rows": 32, "frames": Fmax, "iters": iters, "stream_decode_ms": ms * 1e3, "pool_decode_ms": mp * 1e3, "stream_us_per_frame": ms * 1e6 / Fmax,
            "pool_us_per_tick": mp * 1e6 / Fmax, "pool_over_stream": mp / ms, "within_5_percent": bool(abs(mp / ms - 1.0) <= 0.05)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--rates", type=str, default="5,20,80")
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--out", type=Path, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "serve_bench needs the GPU"
    dm = DurationModel()
    dm.load_params(*synthetic_duration_checkpoint())
    am = AcousticModel(device="cuda:0")
    am.load_params(*synthetic_acoustic_checkpoint())
    gen = Generator(V1, device="cuda:0", dtype="bf16")
    gen.load_params(synthetic_params(V1, 4321, "scaled"))
    tdir = ROOT / "tests" / "golden" / "text"
    sents = transcript_sentences(26, tdir / "transcript.txt", tdir / "lexicon.txt")
    _, nfr, trail = t2m.frame_plan(sents, dm(sents), SILENCE)
    Lmax, Fmax = max(len(s) for s in sents), int(max(nfr))
    kept = [n - t for n, t in zip(nfr, trail)]
    rec = {"device": torch.cuda.get_device_name(0), "requests": len(sents), "slots": a.slots, "chunk_frames": a.chunk, "vocoder": "bf16", "out_dtype": "pcm16",
           "silence_duration": SILENCE, "frames_kept_median": float(np.median(kept)), "frames_kept_max": int(max(kept)), "audio_seconds_total": sum(kept) * 256 / 16000,
           "arrival_seed": ARRIVAL_SEED, "rates": {}}
    zero = [0.0] * len(sents)
    serve_pool(dm, am, gen, sents[:4], zero, a.slots, Lmax, Fmax, a.chunk)  # warm-up of both modes
    serve_fifo(dm, am, gen, sents[:2], zero, a.chunk)
    for rate in [float(r) for r in a.rates.split(",") if r]:
        arrivals = np.cumsum(np.random.default_rng(ARRIVAL_SEED).exponential(1.0 / rate, size=len(sents))).tolist()
        pf, plast = serve_pool(dm, am, gen, sents, arrivals, a.slots, Lmax, Fmax, a.chunk)
        ff, flast = serve_fifo(dm, am, gen, sents, arrivals, a.chunk)
        rec["rates"][f"{rate:g}_per_s"] = {"last_arrival_s": arrivals[-1], "pool": summary(pf, plast), "fifo_synthesize_stream": summary(ff, flast)}
        print(json.dumps({f"{rate:g}_per_s": rec["rates"][f"{rate:g}_per_s"]}), flush=True)
    rec["step_cost"] = step_cost(dm, am, sents, a.iters)
    print(json.dumps({"step_cost": rec["step_cost"]}), flush=True)
    if a.out:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text(json.dumps(rec, indent=1) + "\n")
    gen.close()
    am.close()
    dm.close()


if __name__ == "__main__":
    main()
