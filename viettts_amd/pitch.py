"""Track pitch on the GPU: batched YIN F0 on the mel front end's framing (include/vtts_pitch.h, viettts_amd/csrc/pitch.hip), and the F0
error figures between two contours.

    PitchTracker(16000, fmin=50, fmax=500, threshold=0.15, device="cuda:0")(y, lengths)   # [N, S] -> PitchResult(f0, aperiodicity, candidate), each [N, T]
    f0_metrics(f0_a, f0_b, frames)                 # voicing error, F0 RMSE in cents, gross error share, both-voiced frame count
    wav_f0_metrics(wav_a, wav_b, lengths)          # the same from two waveform batches of one shape

    python -m viettts_amd.pitch --wav F.wav [--output f0.npy] [--fmin 50 --fmax 500 --threshold 0.15]

``f0[N, T]`` lines up with ``MelFilter``'s ``mel[N, T, 80]`` frame for frame (same padding, hop and frame count).  The reference has
no pitch stage; nothing here is re-exported under ``vietTTS/``.  No CPU fallback: the kernel is the only implementation of the tracker
(the metrics are torch operators and run wherever their inputs live).
"""
from __future__ import annotations

import argparse
import ctypes as C
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._handle import NativeHandle, ptr
from .audio import waveform_rows

GROSS_ERROR_SHARE = 0.2  # both-voiced frames further apart than this share of the reference F0 count as gross errors


class PitchResult(NamedTuple):
    f0: torch.Tensor            # [N, T] float32: Hz, 0 where unvoiced and past a row's own frames
    aperiodicity: torch.Tensor  # [N, T] float32: c[tau*] of the header, 1 past a row's own frames; re-threshold without another pass
    candidate: torch.Tensor     # [N, T] float32: the F0 candidate whatever the voicing decision, 0 past a row's own frames


class PitchTracker(NativeHandle):
    """``PitchTracker(sample_rate, fmin, fmax, threshold, device)(y, lengths=None)`` — ``y [N, S]`` float32 or int16 PCM (a tensor on the
    device or a numpy array) -> :class:`PitchResult`.  Row b is reflected at its own end; every row's results are bit for bit what the row
    gives alone.  Asynchronous on torch's current stream of the device.  One tracker serves one call at a time on one device."""

    def __init__(self, sample_rate: int = 16000, fmin: float = 50.0, fmax: float = 500.0, threshold: float = 0.15, device="cuda:0", lib_path=None):
        super().__init__("vtts_pitch", device, lib_path, "tracker")
        self.sample_rate, self.fmin, self.fmax, self.threshold = int(sample_rate), float(fmin), float(fmax), float(threshold)
        self.frames_per_workgroup = _lib.PITCH_FRAMES_PER_BLOCK
        cfg = _lib.PitchCfg(self.sample_rate, self.fmin, self.fmax, self.threshold)
        self._create(C.byref(cfg))  # refuses lag ranges outside 2 .. 512 and thresholds outside (0, 1)
        # the header's rule, on the float32 values the struct holds
        self.tau_min, self.tau_max = math.ceil(self.sample_rate / float(cfg.fmax)), math.floor(self.sample_rate / float(cfg.fmin))

    def num_frames(self, n_samples: int) -> int:
        n = C.c_int64(0)
        self._call("num_frames", int(n_samples), C.byref(n))
        return int(n.value)

    def __call__(self, y, lengths=None) -> PitchResult:
        y, lens, lens_c = waveform_rows(y, lengths, self.device, "y")
        N, S = y.shape
        T = max(self.num_frames(n) for n in set(lens))  # refuses rows too short to reflect
        out = torch.empty((3, N, T), dtype=torch.float32, device=self.device)
        dtype = _lib.VTTS_MEL_PCM16 if y.dtype == torch.int16 else _lib.VTTS_MEL_F32
        self._on_stream("forward", ptr(y), dtype, N, S, lens_c, ptr(out[0]), ptr(out[1]), ptr(out[2]), T, None)
        return PitchResult(out[0], out[1], out[2])


_TRACKERS: dict = {}


def default_tracker(device, sample_rate: int = 16000, fmin: float = 50.0, fmax: float = 500.0, threshold: float = 0.15) -> PitchTracker:
    """One PitchTracker per (configuration, device), created at first use: the CLIs'."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(sample_rate), float(fmin), float(fmax), float(threshold), device)
    t = _TRACKERS.get(key)
    if t is None:
        t = _TRACKERS[key] = PitchTracker(sample_rate, fmin, fmax, threshold, device)
    return t


def _contour(x) -> torch.Tensor:
    x = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))
    return (x[None] if x.dim() == 1 else x).double()


def f0_metrics(f0_a, f0_b, frames=None) -> dict:
    """``f0_a`` against the reference contour ``f0_b``, both ``[N, T]`` (or ``[T]``) with 0 = unvoiced; ``frames``: valid frames per row
    (all ``T`` without).  Torch operators on the contours' device, float64.

        voicing_error   share of valid frames whose voicing differs
        f0_rmse_cents   RMS of 1200 log2(a / b) over the frames voiced in both
        gross_error     share of the both-voiced frames with |a - b| > 20 % of b
        voiced_frames   frames voiced in both

    With no both-voiced frame the two F0 figures are ``nan``."""
    a, b = _contour(f0_a), _contour(f0_b)
    if a.shape != b.shape:
        raise ValueError(f"the two contours differ in shape: {tuple(a.shape)} vs {tuple(b.shape)}")
    b = b.to(a.device)
    valid = torch.ones_like(a, dtype=torch.bool)
    if frames is not None:
        fr = torch.as_tensor([int(v) for v in frames], device=a.device)
        if fr.numel() != a.shape[0]:
            raise ValueError("frames must hold one count per row")
        valid = torch.arange(a.shape[1], device=a.device)[None, :] < fr[:, None]
    va, vb = (a > 0) & valid, (b > 0) & valid
    both = va & vb
    n_valid, n_both = int(valid.sum()), int(both.sum())
    out = {"voicing_error": float((va != vb).sum()) / n_valid if n_valid else float("nan"), "f0_rmse_cents": float("nan"), "gross_error": float("nan"),
           "voiced_frames": n_both}
    if n_both:
        ra, rb = a[both], b[both]
        cents = 1200.0 * torch.log2(ra / rb)
        out["f0_rmse_cents"] = float(torch.sqrt((cents * cents).mean()))
        out["gross_error"] = float(((ra - rb).abs() > GROSS_ERROR_SHARE * rb).sum()) / n_both
    return out


def wav_f0_metrics(a, b, lengths=None, tracker: Optional[PitchTracker] = None) -> dict:
    """:func:`f0_metrics` of two waveform batches of one shape (float32 or int16 PCM ``[N, S]``), ``a`` against the reference ``b``, over
    each row's own frames."""
    from .resynth import _on_device

    if tracker is None:
        dev = a.device if isinstance(a, torch.Tensor) and a.is_cuda else (b.device if isinstance(b, torch.Tensor) and b.is_cuda else torch.device("cuda", torch.cuda.current_device()))
        tracker = default_tracker(dev)
    ra = tracker(_on_device(a, tracker.device), lengths)
    rb = tracker(_on_device(b, tracker.device), lengths)
    if ra.f0.shape != rb.f0.shape:
        raise ValueError(f"the two batches differ in shape: {tuple(ra.f0.shape)} vs {tuple(rb.f0.shape)}")
    frames = None if lengths is None else [tracker.num_frames(int(n)) for n in lengths]
    return f0_metrics(ra.f0, rb.f0, frames)


def format_metrics(m: dict) -> str:
    """The one line ``resynth --f0`` prints."""
    return (f"F0 RMSE {m['f0_rmse_cents']:.1f} cents  voicing error {100 * m['voicing_error']:.2f} %  gross error {100 * m['gross_error']:.2f} %  "
            f"({m['voiced_frames']} frames voiced in both)")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="F0 contour of a recording on the GPU (YIN on the mel front end's frames)")
    ap.add_argument("--wav", required=True, help="PCM16 mono .wav; any rate but 16 kHz is converted on the GPU")
    ap.add_argument("--output", default=None, help="write the [T, 3] float32 array (f0, aperiodicity, candidate) as .npy")
    ap.add_argument("--fmin", type=float, default=50.0)
    ap.add_argument("--fmax", type=float, default=500.0)
    ap.add_argument("--threshold", type=float, default=0.15)
    return ap


def main(argv=None) -> None:
    from . import wavio
    from .nat.config import FLAGS

    a = build_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("viettts_amd.pitch needs an MI355X visible to PyTorch-ROCm; there is no CPU path")
    dev = torch.device("cuda", torch.cuda.current_device())
    trk = default_tracker(dev, FLAGS.sample_rate, a.fmin, a.fmax, a.threshold)
    sr, pcm = wavio.read_wav(a.wav)
    y = torch.from_numpy(np.ascontiguousarray(pcm.astype(np.int16))[None, :]).to(dev)
    if sr != FLAGS.sample_rate:
        from .audio import resampler

        y = resampler(sr, FLAGS.sample_rate, dev)(y, out_dtype="pcm16")
    r = trk(y)
    f0 = r.f0[0]
    v = f0[f0 > 0]
    line = f"{f0.numel()} frames, {100.0 * v.numel() / f0.numel():.1f} % voiced"
    if v.numel():
        line += f", F0 median {float(v.median()):.1f} Hz, range {float(v.min()):.1f} .. {float(v.max()):.1f} Hz"
    print(line)
    if a.output:
        np.save(a.output, torch.stack([r.f0[0], r.aperiodicity[0], r.candidate[0]], dim=1).cpu().numpy())


if __name__ == "__main__":
    main()
