"""Intelligibility on the GPU: batched STOI (Taal et al. 2011) and ESTOI (Jensen & Taal 2016) of a processed waveform against the clean
waveform it is sample-aligned with (include/vtts_stoi.h, viettts_amd/csrc/stoi.hip).

    m = StoiMeter(device="cuda:0")
    r = m(clean, processed, lengths)           # [N, S] at 10 kHz -> StoiResult(stoi, estoi, n_frames, n_kept, n_segments, stoi_series, estoi_series)
    r = wav_stoi(clean, processed, lengths, rate=16000)   # converts both to 10 kHz on the device first (viettts_amd.audio.Resampler)

    python -m viettts_amd.stoi --clean A.wav --processed B.wav

The figures are defined at 10 kHz; the meter itself counts samples.  A row with fewer than 30 analysis frames after the silent frames are
removed (less than about 0.4 s of speech) has no figure: NaN, not the 1e-5 placeholder some host packages return.  Unaligned pairs, stereo,
gradients and the streamed paths are out of scope.  The reference has no such stage; nothing here is re-exported under ``vietTTS/``.  No
CPU fallback: the kernels are the only implementation.
"""
from __future__ import annotations

import argparse
import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._handle import NativeHandle, ptr
from .audio import waveform_rows

RATE = 10000  # the rate STOI is defined at


class StoiResult(NamedTuple):
    stoi: torch.Tensor          # [N] float32: nan for a row without a segment
    estoi: torch.Tensor         # [N] float32
    n_frames: torch.Tensor      # [N] int32: candidate frames (256 samples at hop 128)
    n_kept: torch.Tensor        # [N] int32: those within 40 dB of the clean row's loudest
    n_segments: torch.Tensor    # [N] int32: 30-frame segments of the kept frames' signal
    stoi_series: Optional[torch.Tensor]   # [N, M] float32 with ``series=True``: every segment's value, nan past a row's own segments
    estoi_series: Optional[torch.Tensor]


class StoiMeter(NativeHandle):
    """``StoiMeter(device)(clean, processed, lengths=None, series=False)`` — both ``[N, S]`` (or ``[S]``) float32 or int16 PCM at 10 kHz (tensors
    on the device or numpy arrays), one ``lengths`` for both -> :class:`StoiResult`, tensors on the device.  A row's results are bit for bit
    what the row gives alone.  Asynchronous on torch's current stream of the device.  One meter serves one call at a time on one device."""

    def __init__(self, device="cuda:0", lib_path=None):
        super().__init__("vtts_stoi", device, lib_path, "meter")
        self._create()
        self._last = (0, 0)

    def window(self) -> np.ndarray:
        """The 256 float32 window values the kernels use."""
        out = np.empty(_lib.STOI_FRAME, dtype=np.float32)
        self._call("window", out.ctypes.data_as(C.POINTER(C.c_float)))
        return out

    def num_frames(self, n_samples: int) -> int:
        n = C.c_int64(0)
        self._call("num_frames", int(n_samples), C.byref(n))
        return int(n.value)

    def __call__(self, clean, processed, lengths=None, series: bool = False, mags: bool = False):
        """With ``mags=True`` returns ``(StoiResult, band magnitudes [N, 2, 15, T] float32)``: X then Y of include/vtts_stoi.h, for tests;
        entries past a row's own ``n_kept - 1`` frames are zero."""
        one_row = getattr(clean, "ndim", 2) == 1
        if one_row:
            clean, processed = clean[None, :], processed[None, :]
        x, lens, lens_c = waveform_rows(clean, lengths, self.device, "clean")
        y, _, _ = waveform_rows(processed, None, self.device, "processed")
        if x.shape != y.shape:
            raise ValueError(f"clean and processed differ in shape: {tuple(x.shape)} vs {tuple(y.shape)}")
        if x.dtype != y.dtype:  # one dtype for both on the C side; PCM16 -> float32 is exact
            x, y = (t.to(torch.float32) * 2.0 ** -15 if t.dtype == torch.int16 else t for t in (x, y))
        N, S = x.shape
        if N < 1:
            raise ValueError("at least one row is needed")
        longest = max(lens)
        K = self.num_frames(longest)  # refuses rows above STOI_MAX_SAMPLES
        T, M = max(0, K - 1), max(0, K - _lib.STOI_SEG)
        need = C.c_size_t(0)
        self._call("workspace_bytes", N, longest, C.byref(need))
        ws = self._workspace(int(need.value))
        f = torch.empty((2, N), dtype=torch.float32, device=self.device)
        n = torch.empty((3, N), dtype=torch.int32, device=self.device)
        ser = torch.empty((2, N, M), dtype=torch.float32, device=self.device) if series else None
        mg = torch.zeros((N, 2, _lib.STOI_BANDS, T), dtype=torch.float32, device=self.device) if mags else None
        dtype = _lib.VTTS_AUDIO_PCM16 if x.dtype == torch.int16 else _lib.VTTS_AUDIO_F32
        self._on_stream("forward", ptr(x), ptr(y), dtype, N, S, lens_c, ptr(f[0]), ptr(f[1]), ptr(n[0]), ptr(n[1]), ptr(n[2]),
                        ptr(ser[0]) if series else None, ptr(ser[1]) if series else None, M, ptr(mg), T, ptr(ws), ws.numel())
        self._last = (N, K)
        r = StoiResult(f[0], f[1], n[0], n[1], n[2], ser[0] if series else None, ser[1] if series else None)
        return (r, mg) if mags else r

    def kept_frames(self) -> torch.Tensor:
        """``[N, K]`` int32 of the last call: each row's kept candidate frames in ascending order, then -1 (a copy of the head of the
        workspace, whose layout include/vtts_stoi.h states)."""
        N, K = self._last
        if self._ws is None or N * K == 0:
            return torch.empty((N, K), dtype=torch.int32, device=self.device)
        return self._ws[: 4 * N * K].view(torch.int32).view(N, K).clone()


_METERS: dict = {}


def default_stoi_meter(device) -> StoiMeter:
    """One StoiMeter per device, created at first use: the command lines'."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    m = _METERS.get(device)
    if m is None:
        m = _METERS[device] = StoiMeter(device)
    return m


def wav_stoi(clean, processed, lengths=None, rate: int = 16000, series: bool = False, meter: Optional[StoiMeter] = None) -> StoiResult:
    """STOI and ESTOI of ``processed`` against ``clean`` (both ``[N, S]`` or ``[S]`` at ``rate``; tensors on a device or, with ``meter``, numpy
    arrays): both are converted to 10 kHz on the device with ``audio.resampler(rate, 10000, device)`` unless ``rate`` is 10000 already, and
    ``lengths`` go through the resampler's own length rule."""
    if meter is None:
        t = clean if isinstance(clean, torch.Tensor) else processed
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise ValueError("wav_stoi needs a tensor on the device, or a meter")
        meter = default_stoi_meter(t.device)
    if int(rate) != RATE:
        from .audio import resampler

        rs = resampler(int(rate), RATE, meter.device)
        clean, processed = rs(clean, lengths=lengths), rs(processed, lengths=lengths)
        if lengths is not None:
            lengths = rs.out_lengths(lengths)
    return meter(clean, processed, lengths, series=series)


def format_result(r: StoiResult, row: int = 0) -> str:
    """The one line the command lines print for a row."""
    return (f"STOI {float(r.stoi[row]):.4f}  ESTOI {float(r.estoi[row]):.4f}  ({int(r.n_segments[row])} segments from {int(r.n_kept[row])} of "
            f"{int(r.n_frames[row])} frames within 40 dB)")


def check_pair(rate_a: int, n_a: int, rate_b: int, n_b: int, hop: int = 256) -> int:
    """The command line's rule, on the host: one rate, and lengths within one model hop.  Returns the common length."""
    if rate_a != rate_b:
        raise ValueError(f"the two files differ in rate: {rate_a} vs {rate_b} Hz")
    if abs(n_a - n_b) > hop:
        raise ValueError(f"the two files differ in length by more than one model hop ({hop} samples): {n_a} vs {n_b}; unaligned pairs are out of scope")
    return min(n_a, n_b)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="STOI and ESTOI of a processed recording against the clean one, on the GPU")
    ap.add_argument("--clean", required=True, help="PCM16 mono .wav: the reference")
    ap.add_argument("--processed", required=True, help="PCM16 mono .wav at the same rate, sample-aligned with --clean (lengths within one model hop)")
    return ap


def main(argv=None) -> None:
    from . import wavio

    a = build_parser().parse_args(argv)
    sr, x = wavio.read_wav(a.clean)
    sr2, y = wavio.read_wav(a.processed)
    n = check_pair(sr, len(x), sr2, len(y))  # before the GPU is touched
    if not torch.cuda.is_available():
        raise RuntimeError("viettts_amd.stoi needs an MI355X visible to PyTorch-ROCm; there is no CPU path")
    dev = torch.device("cuda", torch.cuda.current_device())
    to_dev = lambda p: torch.from_numpy(np.ascontiguousarray(p[:n].astype(np.int16))[None, :]).to(dev)  # noqa: E731
    print(format_result(wav_stoi(to_dev(x), to_dev(y), rate=sr)))


if __name__ == "__main__":
    main()
