"""Time the teacher-forced acoustic pass (vtts_nat_acoustic_forward_teacher) next to the autoregressive forward() at the same shapes, in the
same run on the same GPU, and the whole wav -> GTA mel path.  Both entries are called through the C ABI on pre-uploaded operands and pre-drawn
masks (device events around the call, warm-up, the two alternated, median of --iters), so the figures are GPU time of the passes, not of
Python's batching.

    python tools/gta_bench.py [--iters 15] [--out profiles/gta_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -o gta -- python tools/gta_bench.py --profile-pass     # one call of each at 64 x 768, in a run of its own
    python tools/gta_bench.py --kernel-db DIR/.../gta_results.db --out profiles/gta_bench.json      # adds the per-step kernel times to the JSON

Shapes: 64 rows x 256 tokens x 768 frames (the reference's corpus batch: vietTTS/nat/config.py batch_size, max_phoneme_seq_len, max_wave_len / hop)
and the 256 sentences of ``synthetic_sentences()`` with seeded durations (~5 frames per phoneme, word ends 0).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sqlite3
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from viettts_amd import _lib  # noqa: E402
from viettts_amd.nat.acoustic import AcousticModel  # noqa: E402
from viettts_amd.nat.config import FLAGS  # noqa: E402
from viettts_amd._handle import ptr  # noqa: E402
from viettts_amd.nat.synth import synthetic_acoustic_checkpoint, synthetic_sentences  # noqa: E402

RNG_KEY = np.array([0x1234ABCD, 0x0F1E2D3C], dtype=np.uint32)
STEP_KERNELS = ("nat_tf_lstm_k", "nat_dec_lstm_k", "nat_dec_proj_prenet_k")


def shapes():
    rng = np.random.default_rng(7)
    corpus = [rng.integers(0, 100, size=256) for _ in range(64)]
    cd = [(w / w.sum() * 768).astype(np.float32) for w in (rng.uniform(0.2, 1.8, size=256) for _ in range(64))]
    yield "corpus_64x768", corpus, cd, [768] * 64
    sents = synthetic_sentences(256)
    durs, nfs = [], []
    for s in sents:
        d = np.abs(rng.normal(5.0, 2.0, size=len(s))).astype(np.float32)
        d[np.asarray(s) == FLAGS.word_end_index] = 0.0
        durs.append(d)
        nfs.append(max(1, int(np.sum(d, dtype=np.float32))))
    yield "sentences_256", sents, durs, nfs


class Operands:
    """Everything both entries read, uploaded once."""

    def __init__(self, m: AcousticModel, sents, durs, nfs):
        dev = m.device
        self.B, self.L, self.F = len(sents), max(len(s) for s in sents), max(nfs)
        tok = np.zeros((self.B, self.L), np.int32)
        dur = np.zeros((self.B, self.L), np.float32)
        for i, s in enumerate(sents):
            tok[i, : len(s)] = s
            dur[i, : len(s)] = durs[i]
        self.tok, self.dur = torch.from_numpy(tok).to(dev), torch.from_numpy(dur).to(dev)
        self.len = torch.tensor([len(s) for s in sents], dtype=torch.int32, device=dev)
        self.nf = torch.tensor(nfs, dtype=torch.int32, device=dev)
        g = torch.Generator(device="cpu").manual_seed(3)
        self.mels = (torch.randn((self.B, self.F, m.mel_dim), generator=g) * 1.5 - 3.0).to(dev)
        self.keep, self.zone = m.device_teacher_masks_haiku(RNG_KEY, self.B, self.F, partitionable=False)
        self.out = torch.empty((self.B, self.F, m.mel_dim), dtype=torch.float32, device=dev)
        n = C.c_size_t(0)
        _lib.check(m.lib, m.lib.vtts_nat_acoustic_forward_teacher_workspace_bytes(m._h, self.B, self.L, self.F, C.byref(n)))
        self.ws = torch.empty(int(n.value), dtype=torch.uint8, device=dev)


def call_forward(m, o):
    st = C.c_void_p(torch.cuda.current_stream(m.device).cuda_stream)
    _lib.check(m.lib, m.lib.vtts_nat_acoustic_forward(m._h, ptr(o.tok), ptr(o.len), ptr(o.dur), ptr(o.nf), o.B, o.L, o.F, ptr(o.keep), ptr(o.out), ptr(o.ws),
                                                      o.ws.numel(), st))


def call_teacher(m, o):
    st = C.c_void_p(torch.cuda.current_stream(m.device).cuda_stream)
    _lib.check(m.lib, m.lib.vtts_nat_acoustic_forward_teacher(m._h, ptr(o.tok), ptr(o.len), ptr(o.dur), ptr(o.nf), o.B, o.L, o.F, ptr(o.mels), ptr(o.keep),
                                                              ptr(o.zone), ptr(o.out), None, ptr(o.ws), o.ws.numel(), st))


def timed_ms(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def kernel_stats(db_path):
    db = sqlite3.connect(db_path)
    out = {}
    for name, calls, tot, avg in db.execute("select name, total_calls, total_duration, average from top_kernels"):
        for k in STEP_KERNELS:
            if k in name:
                key = k + ("<" + name.split("<", 1)[1].split(">", 1)[0] + ">" if "<" in name else "")
                out[key] = {"calls": int(calls), "avg_us": float(avg), "total_ms": float(tot) / 1e3}  # the view reports microseconds
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=Path, default=None)
    ap.add_argument("--profile-pass", action="store_true", help="one call of each entry at the corpus shape and nothing else (run it under rocprofv3)")
    ap.add_argument("--kernel-db", type=Path, default=None, help="rocprofv3 results .db of a --profile-pass run: merge the step kernels' times into --out")
    a = ap.parse_args()
    if a.kernel_db is not None:
        rec = json.loads(a.out.read_text()) if a.out and a.out.exists() else {}
        rec["step_kernels_rocprofv3"] = kernel_stats(str(a.kernel_db))
        (a.out.write_text(json.dumps(rec, indent=1) + "\n") if a.out else print(json.dumps(rec)))
        return
    assert torch.cuda.is_available(), "gta_bench needs the GPU"
    m = AcousticModel(device="cuda:0")
    m.load_params(*synthetic_acoustic_checkpoint())
    rec = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "shapes": {}}
    for name, sents, durs, nfs in shapes():
        o = Operands(m, sents, durs, nfs)
        if a.profile_pass:
            call_forward(m, o)
            call_teacher(m, o)
            torch.cuda.synchronize()
            break
        for _ in range(a.warmup):
            call_forward(m, o)
            call_teacher(m, o)
        torch.cuda.synchronize()
        tf, tt = [], []
        for _ in range(a.iters):  # alternated: whatever else loads the box hits both
            tf.append(timed_ms(lambda: call_forward(m, o)))
            tt.append(timed_ms(lambda: call_teacher(m, o)))
        r = {"B": o.B, "Lmax": o.L, "Fmax": o.F, "frames": int(sum(nfs)), "forward_ms": float(np.median(tf)), "forward_teacher_ms": float(np.median(tt)),
             "forward_ms_min_max": [float(min(tf)), float(max(tf))], "forward_teacher_ms_min_max": [float(min(tt)), float(max(tt))]}
        r["teacher_over_forward"] = r["forward_teacher_ms"] / r["forward_ms"]
        rec["shapes"][name] = r
        print(json.dumps({name: r}), flush=True)
        del o
    if not a.profile_pass:
        # wav -> log-mel (PCM16) -> teacher-forced pass -> GTA mel on the device, reference padding, 64 x (768 * 256) samples
        from viettts_amd.nat import gta
        from viettts_amd.nat.dsp import MelFilter

        mf = MelFilter(FLAGS.sample_rate, FLAGS.n_fft, FLAGS.mel_dim, 0.0, 8000, device="cuda:0")
        rng = np.random.default_rng(9)
        tok = rng.integers(0, 100, size=(64, 256)).astype(np.int32)
        w = rng.uniform(0.2, 1.8, size=(64, 256))
        dur_s = (w / w.sum(axis=1, keepdims=True) * (768 * 256 / 16000)).astype(np.float32)
        wavs = torch.from_numpy((rng.normal(0, 0.1, size=(64, 768 * 256)) * 32768).clip(-32768, 32767).astype(np.int16)).to(m.device)
        batch = gta.AcousticInput(tok, np.full(64, 256, np.int32), dur_s, wavs, np.full(64, 768 * 256, np.int32))
        fn = lambda: gta.forward_fn(m, mf, RNG_KEY, batch, reference_padding=True, to_host=False)
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ts = [timed_ms(fn) for _ in range(a.iters)]
        rec["wav_to_gta_mel_64x768_ms"] = float(np.median(ts))  # includes the mask draw and the host's batching of tokens / durations
        print(json.dumps({"wav_to_gta_mel_64x768_ms": rec["wav_to_gta_mel_64x768_ms"]}), flush=True)
        mf.close()
        if a.out:
            a.out.parent.mkdir(parents=True, exist_ok=True)
            a.out.write_text(json.dumps(rec, indent=1) + "\n")
    m.close()


if __name__ == "__main__":
    main()
