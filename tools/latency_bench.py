"""Latency of ONE sentence (and of four) from token ids to a synchronised waveform, with the acoustic decoder's frame loop as today's three launches
per frame and as the resident kernel (option "resident" of include/vtts_nat.h), alternated call by call in one process on one GPU.

    python tools/latency_bench.py [--iters 30] [--warmup 5] [--grids 64,128,256] [--out profiles/latency_b1.json]

Workload: the median-length line of tests/golden/text/transcript.txt (B = 1) and the four lines around the median (B = 4), synthetic checkpoints
(viettts_amd/nat/synth.py), the bf16 vocoder, steady state (--warmup calls of each mode first).  Per call: host wall clock from the call to the
synchronised result (it includes every enqueue), and device-event times per stage — duration model (its read-back included), host frame rules (host
clock), token encoder, gate GEMM + mix, decoder loop, postnet (the library's own events: option "stage_times"), vocoder.  Reported: median, min and
max over --iters calls per mode, microseconds per frame of the decoder loop, and the real-time factor at 16 kHz (wall clock / audio seconds).
--grids adds the resident kernel on each of those grids (option "resident_grid") to the alternation: the A/B behind the library's default.
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
from viettts_amd.nat.config import FLAGS  # noqa: E402
from viettts_amd.nat.duration import DurationModel  # noqa: E402
from viettts_amd.nat.synth import synthetic_acoustic_checkpoint, synthetic_duration_checkpoint, transcript_sentences  # noqa: E402

SILENCE = 0.05
STAGES = ("duration_model", "host_rules", "token_encoder", "gates", "decoder_loop", "postnet", "vocoder")


def workloads():
    tdir = ROOT / "tests" / "golden" / "text"
    sents = transcript_sentences(26, tdir / "transcript.txt", tdir / "lexicon.txt")
    order = sorted(range(len(sents)), key=lambda i: (len(sents[i]), i))
    mid = len(order) // 2
    return {"b1": [sents[order[mid]]], "b4": [sents[i] for i in order[mid - 2 : mid + 2]]}


def one_call(dm, am, gen, sents, resident: int, grid: int):
    """One synthesis; returns ({stage: us}, wall us, frames per sentence)."""
    am.set_option("resident", resident)
    am.set_option("resident_grid", grid)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev[0].record()
    secs = dm(sents)
    ev[1].record()
    h0 = time.perf_counter()
    frames, nfr, _ = t2m.frame_plan(sents, secs, SILENCE)
    h1 = time.perf_counter()
    ev[2].record()
    enc = am.encode(sents)
    ev[3].record()
    mel = am(sents, frames, nfr, dropout_seeds=[7] * len(sents), to_host=False, encoded=enc)
    ev[4].record()
    wav = gen(mel)
    ev[5].record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e6
    if resident:
        assert am.resident_used and not am.resident_status(), "the resident kernel was not taken, or gave up"
    else:
        assert not am.resident_used
    st = {
        "duration_model": ev[0].elapsed_time(ev[1]) * 1e3,
        "host_rules": (h1 - h0) * 1e6,
        "token_encoder": ev[2].elapsed_time(ev[3]) * 1e3,
        "gates": float(am.get_option("stage_gates_us")),
        "decoder_loop": float(am.get_option("stage_decoder_us")),
        "postnet": float(am.get_option("stage_postnet_us")),
        "vocoder": ev[4].elapsed_time(ev[5]) * 1e3,
    }
    del wav
    return st, wall, nfr


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--grids", type=str, default="", help="comma-separated resident grids to add to the alternation (64,128,256)")
    ap.add_argument("--out", type=Path, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "latency_bench needs the GPU"
    dm = DurationModel()
    dm.load_params(*synthetic_duration_checkpoint())
    am = AcousticModel(device="cuda:0")
    am.load_params(*synthetic_acoustic_checkpoint())
    am.set_option("stage_times", 1)
    gen = Generator(V1, device="cuda:0", dtype="bf16")
    gen.load_params(synthetic_params(V1, 4321, "scaled"))
    modes = [("launches", 0, 0), ("resident", 1, 0)] + [(f"resident_grid{g}", 1, int(g)) for g in a.grids.split(",") if g]
    rec = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "vocoder": "bf16", "silence_duration": SILENCE, "workloads": {}}
    for wname, sents in workloads().items():
        for _ in range(a.warmup):
            for _, res, grid in modes:
                one_call(dm, am, gen, sents, res, grid)
        runs = {m[0]: {"wall": [], **{s: [] for s in STAGES}} for m in modes}
        nfr = None
        for _ in range(a.iters):  # alternated: whatever else loads the box hits every mode
            for name, res, grid in modes:
                st, wall, nfr = one_call(dm, am, gen, sents, res, grid)
                runs[name]["wall"].append(wall)
                for s in STAGES:
                    runs[name][s].append(st[s])
        fmax, audio_s = max(nfr), max(nfr) * (FLAGS.n_fft // 4) / FLAGS.sample_rate
        w = {"B": len(sents), "tokens": [len(s) for s in sents], "frames": [int(n) for n in nfr], "audio_seconds_longest": audio_s, "modes": {}}
        for name, r in runs.items():
            m = {"wall_us": stats(r["wall"]), "stages_us": {s: stats(r[s]) for s in STAGES}}
            m["decoder_us_per_frame"] = {k: v / fmax for k, v in m["stages_us"]["decoder_loop"].items()}
            m["rtf_16khz"] = m["wall_us"]["median"] * 1e-6 / audio_s
            m["token_encoder_share_of_wall"] = m["stages_us"]["token_encoder"]["median"] / m["wall_us"]["median"]
            w["modes"][name] = m
            print(json.dumps({wname: {name: {"wall_us": m["wall_us"], "decoder_loop_us": m["stages_us"]["decoder_loop"], "decoder_us_per_frame": m["decoder_us_per_frame"],
                                             "rtf_16khz": m["rtf_16khz"]}}}), flush=True)
        rec["workloads"][wname] = w
    am.set_option("resident", 0)
    am.set_option("resident_grid", 0)
    if a.out:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text(json.dumps(rec, indent=1) + "\n")
    gen.close()
    am.close()
    dm.close()


if __name__ == "__main__":
    main()
