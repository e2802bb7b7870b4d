"""Time the audio stage (viettts_amd/csrc/audio.hip): sample-rate conversion with fp32 and PCM16 on either side, next to the HBM time
of its input plus output bytes and next to the same filter on torch's own operators, and the sentence pipeline with fp32 and with
PCM16 read-back.  Device-event timing, warm-up, median of --iters runs per shape; the two sides of every comparison alternate in
one process.

    python tools/audio_bench.py [--iters 30] [--no-torch] [--no-pipeline] [--parent-pipeline FILE] [--out profiles/audio_bench.json]

--parent-pipeline: another revision's viettts_amd/pipeline.py; its default path is alternated against this tree's.
Writes one JSON document.
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
from viettts_amd import wavio  # noqa: E402
from viettts_amd.audio import Resampler  # noqa: E402

HBM_BYTES_PER_S = 8.0e12  # MI355X peak
SHAPES = ((64, 262144), (1, 131072))
RATES = ((16000, 48000), (16000, 44100), (16000, 8000), (44100, 16000))
ESZ = {"f32": 4, "pcm16": 2}


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


def alternated_ms(fns: dict, warmup: int, iters: int) -> dict:
    """Medians of several functions timed in turn, one run of each per round."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: float(np.median(v)) for k, v in times.items()}


class TorchPolyphase:
    """The same filter as ONE strided conv1d: outputs m = r + L k share the phase p_r and step M samples per k, so channel r of
    conv1d(x, W [L, 1, width], stride = M) is that residue's outputs; W[r] holds phase p_r's taps at residue r's offset."""

    def __init__(self, rs: Resampler, device):
        L, M, half = rs.L, rs.M, rs.half
        h = rs.prototype.astype(np.float32)
        kp = -(-(2 * half + 1) // L)
        t = np.arange(L, dtype=np.int64) * M + half
        q, p = t // L, t % L
        self.q_min, width = int(q.min()), int(q.max() - q.min()) + kp
        W = np.zeros((L, 1, width), dtype=np.float32)
        for r in range(L):
            for j in range(kp):
                k = int(p[r]) + j * L
                if k <= 2 * half:
                    W[r, 0, int(q[r]) - self.q_min + (kp - 1) - j] = h[k]
        self.W = torch.from_numpy(W).to(device)
        self.L, self.M, self.kp, self.width = L, M, kp, width

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        N, S = x.shape
        So = -(-S * self.L // self.M)
        K = -(-So // self.L)
        left = self.kp - 1 - self.q_min
        right = max(0, (K - 1) * self.M + self.width - (S + left))
        xp = torch.nn.functional.pad(x.unsqueeze(1), (left, right))
        y = torch.nn.functional.conv1d(xp, self.W, stride=self.M)[:, :, :K]
        return y.permute(0, 2, 1).reshape(N, K * self.L)[:, :So]


def resample_section(dev, warmup, iters, with_torch):
    recs = []
    for rates in RATES:
        rs = Resampler(*rates, dev)
        for N, S in SHAPES:
            g = torch.Generator(device="cpu").manual_seed(5)
            x = (0.1 * torch.randn((N, S), generator=g)).to(dev)
            pcm = (x * 32768.0).round().clamp(-32768, 32767).to(torch.int16)
            So = rs.out_samples(S)
            rec = {"in_rate": rates[0], "out_rate": rates[1], "L": rs.L, "M": rs.M, "N": N, "S": S, "out_samples": N * So}
            for din, src in (("f32", x), ("pcm16", pcm)):
                for dout in ("f32", "pcm16"):
                    key = f"{din}_to_{dout}"
                    rec[key + "_ms"] = median_ms(lambda: rs(src, out_dtype=dout), warmup, iters)
                    rec[key + "_hbm_floor_ms"] = 1e3 * (N * S * ESZ[din] + N * So * ESZ[dout]) / HBM_BYTES_PER_S
            rec["out_samples_per_s_f32"] = N * So / (rec["f32_to_f32_ms"] * 1e-3)
            if with_torch:
                try:
                    tp = TorchPolyphase(rs, dev)
                    ref = tp(x)
                    torch.cuda.synchronize()
                    rec["max_abs_vs_torch"] = float((rs(x) - ref).abs().max())
                    both = alternated_ms({"kernel": lambda: rs(x), "torch": lambda: tp(x)}, warmup, iters)
                    rec["alternated_kernel_f32_ms"], rec["torch_polyphase_conv1d_ms"] = both["kernel"], both["torch"]
                    rec["speedup_vs_torch"] = both["torch"] / both["kernel"]
                    del tp, ref
                except RuntimeError as e:  # torch's convolution is not usable at this shape: reported, not hidden
                    rec["torch_polyphase_conv1d_ms"] = None
                    rec["torch_error"] = str(e)[:200]
            print(json.dumps(rec), flush=True)
            recs.append(rec)
        rs.close()
    return recs


def pipeline_section(rounds, parent_file):
    from viettts_amd import dist as vdist
    from viettts_amd import pipeline
    from viettts_amd.hifigan.config import V1
    from viettts_amd.hifigan.generator import Generator
    from viettts_amd.nat.acoustic import AcousticModel
    from viettts_amd.nat.duration import DurationModel
    from viettts_amd.hifigan.synth import synthetic_params
    from viettts_amd.nat.synth import synthetic_acoustic_checkpoint, synthetic_duration_checkpoint, transcript_sentences

    gen = Generator(V1, device="cuda:0", dtype="bf16")
    gen.load_params(synthetic_params(V1, 4321, "scaled"))
    dm = vdist.setup_model_dp(DurationModel(device="cuda:0"), lambda m: m.load_params(*synthetic_duration_checkpoint()))
    am = vdist.setup_model_dp(AcousticModel(device="cuda:0"), lambda m: m.load_params(*synthetic_acoustic_checkpoint()))
    tdir = REPO / "tests" / "golden" / "text"
    sents = transcript_sentences(256, str(tdir / "transcript.txt"), str(tdir / "lexicon.txt"))
    variants = {"f32": (pipeline.synthesize_sentences, {}), "pcm16": (pipeline.synthesize_sentences, {"out_dtype": "pcm16"})}
    if parent_file:
        spec = importlib.util.spec_from_file_location("viettts_amd.pipeline_parent", parent_file)
        parent = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = parent
        spec.loader.exec_module(parent)
        variants["parent_f32"] = (parent.synthesize_sentences, {})
    runs = {k: [] for k in variants}
    for it in range(rounds + 2):  # the first two rounds warm allocators and code objects
        for name, (fn, kw) in variants.items():
            tm = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            wavs = fn(sents, dm, am, gen, silence_duration=0.05, dropout_seed=7, timing=tm, **kw)
            torch.cuda.synchronize()
            total = time.perf_counter() - t0
            host = 0.0
            if "pcm16" not in name:  # what a WAV writer still has to do with fp32 samples
                t1 = time.perf_counter()
                _ = [wavio.float_to_pcm16(w) for w in wavs.values()]
                host = time.perf_counter() - t1
            nbytes = int(sum(w.nbytes for w in wavs.values()))
            del wavs
            if it >= 2:
                runs[name].append({"generator_ms": tm["generator_s"] * 1e3, "total_ms": total * 1e3, "host_pcm16_ms": host * 1e3, "returned_bytes": nbytes})
    out = {"sentences": 256, "rounds": rounds, "generator": "bf16"}
    for name, rr in runs.items():
        out[name] = {k: float(np.median([r[k] for r in rr])) for k in rr[0]}
        out[name]["total_ms_min_max"] = [float(min(r["total_ms"] for r in rr)), float(max(r["total_ms"] for r in rr))]
        out[name]["generator_plus_host_pcm16_ms"] = out[name]["generator_ms"] + out[name]["host_pcm16_ms"]
    dm.close()
    am.close()
    gen.close()
    print(json.dumps(out), flush=True)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=10, help="alternated rounds of the pipeline section")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-pipeline", action="store_true")
    ap.add_argument("--parent-pipeline", default=None)
    ap.add_argument("--out", default=str(REPO / "profiles" / "audio_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "audio_bench needs the GPU"
    assert a.iters >= 20
    dev = torch.device("cuda:0")
    doc = {"method": f"device events, {a.warmup} warm-ups, median of {a.iters}; hbm_floor = (input + output bytes) / 8 TB/s; torch baseline = one strided "
                     "conv1d in polyphase form, alternated with the kernel run by run",
           "device": torch.cuda.get_device_name(0)}
    doc["resample"] = resample_section(dev, a.warmup, a.iters, not a.no_torch)
    # the host conversion the issue's figure is about: float_to_pcm16 on 9.6 M samples, on this host's CPU
    x = (0.1 * np.random.default_rng(0).standard_normal(9_600_000)).astype(np.float32)
    t0 = time.perf_counter()
    want = wavio.float_to_pcm16(x)
    doc["host_float_to_pcm16_9p6M_ms"] = (time.perf_counter() - t0) * 1e3
    from viettts_amd.audio import to_pcm16

    xd = torch.from_numpy(x).to(dev)
    doc["device_to_pcm16_9p6M_ms"] = median_ms(lambda: to_pcm16(xd), a.warmup, a.iters)
    doc["device_to_pcm16_9p6M_equal"] = bool(np.array_equal(to_pcm16(xd).cpu().numpy(), want))
    if not a.no_pipeline:
        doc["pipeline_256"] = pipeline_section(a.rounds, a.parent_pipeline)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
