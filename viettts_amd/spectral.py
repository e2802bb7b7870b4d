"""Spectral distances on the GPU: the multi-resolution STFT distance (spectral convergence + log-magnitude L1 at three resolutions: Yamamoto
et al., Parallel WaveGAN, 2020) and log-spectral distance of a signal under test against the reference it is sample-aligned with, and the
forward magnitude STFT at any of four transform lengths (include/vtts_spectral.h, viettts_amd/csrc/spectral.hip).

    m = SpectralMeter(1024, 600, 120, device="cuda:0")          # one resolution: n_fft, win, hop
    r = m(ref, test, lengths)                                   # [N, S] -> SpectralResult(sc, logmag, lsd, n_frames, mags)
    r = m(ref, test, lengths, mags=True)                        # ... with r.mags [N, 2, T, n_fft / 2 + 1]: |STFT| of ref, then of test
    r = wav_mrstft(ref, test, lengths)                          # Parallel WaveGAN's three resolutions -> MrStftResult

    python -m viettts_amd.spectral --ref A.wav --test B.wav

Framing is ``torch.stft(center=True, pad_mode="reflect")`` with a periodic Hann window centred in ``n_fft``.  Magnitudes only, no gradients: the
complex spectrum, the inverse transform and Griffin-Lim are ``viettts_amd.stft`` (include/vtts_stft.h).  Unaligned pairs and stereo are out of scope.  The reference has no such stage; nothing here is
re-exported under ``vietTTS/``.  No CPU fallback: the kernels are the only implementation.
"""
from __future__ import annotations

import argparse
import ctypes as C
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._handle import NativeHandle, ptr
from .audio import waveform_rows

PWG_RESOLUTIONS = ((1024, 600, 120), (2048, 1200, 240), (512, 240, 50))  # (n_fft, win, hop): Parallel WaveGAN's


class SpectralResult(NamedTuple):
    sc: torch.Tensor          # [N] float64: spectral convergence, || |Y| - |X| ||_F / || |X| ||_F
    logmag: torch.Tensor      # [N] float64: mean | ln |Y| - ln |X| |
    lsd: torch.Tensor         # [N] float64: log-spectral distance in dB, the mean over frames of the RMS over bins
    n_frames: torch.Tensor    # [N] int32: 1 + S // hop
    mags: Optional[torch.Tensor] = None  # [N, 2, T, n_fft / 2 + 1] float32 with ``mags=True``: zero past a row's own frames


class MrStftResult(NamedTuple):
    mrstft: torch.Tensor      # [N] float64: the mean over the resolutions of sc + logmag
    lsd: torch.Tensor         # [N] float64: the mean over the resolutions
    per_resolution: Tuple[SpectralResult, ...]


class SpectralMeter(NativeHandle):
    """``SpectralMeter(n_fft, win, hop, device)(ref, test, lengths=None, mags=False)`` — both ``[N, S]`` (or ``[S]``) float32 or int16 PCM
    (tensors on the device or numpy arrays), one ``lengths`` for both -> :class:`SpectralResult`, tensors on the device.  A row's results are
    bit for bit what the row gives alone.  Asynchronous on torch's current stream of the device.  One meter serves one call at a time."""

    def __init__(self, n_fft: int = 1024, win: int = 600, hop: int = 120, device="cuda:0", lib_path=None):
        super().__init__("vtts_spectral", device, lib_path, "meter")
        self.n_fft, self.win, self.hop = int(n_fft), int(win), int(hop)
        self._create(C.byref(_lib.SpectralCfg(self.n_fft, self.win, self.hop)))
        self._packed = False

    @property
    def n_bins(self) -> int:
        return self.n_fft // 2 + 1

    @property
    def min_samples(self) -> int:
        return self.n_fft // 2 + 1

    def window(self) -> np.ndarray:
        """The ``n_fft`` float32 window values the kernels use."""
        out = np.empty(self.n_fft, dtype=np.float32)
        self._call("window", out.ctypes.data_as(C.POINTER(C.c_float)))
        return out

    def num_frames(self, n_samples: int) -> int:
        n = C.c_int64(0)
        self._call("num_frames", int(n_samples), C.byref(n))
        return int(n.value)

    @property
    def frames_per_block(self) -> int:
        n = C.c_int(0)
        self._call("frames_per_block", C.byref(n))
        return int(n.value)

    def workspace_bytes(self, N: int, S: int) -> int:
        n = C.c_size_t(0)
        self._call("workspace_bytes", int(N), int(S), C.byref(n))
        return int(n.value)

    def __call__(self, ref, test, lengths=None, mags: bool = False) -> SpectralResult:
        one_row = getattr(ref, "ndim", 2) == 1
        if one_row:
            ref, test = ref[None, :], test[None, :]
        x, lens, lens_c = waveform_rows(ref, lengths, self.device, "ref")
        y, _, _ = waveform_rows(test, None, self.device, "test")
        if x.shape != y.shape:
            raise ValueError(f"ref and test differ in shape: {tuple(x.shape)} vs {tuple(y.shape)}")
        if x.dtype != y.dtype:  # one dtype for both on the C side; PCM16 -> float32 is exact
            x, y = (t.to(torch.float32) * 2.0 ** -15 if t.dtype == torch.int16 else t for t in (x, y))
        N, S = x.shape
        if N < 1:
            raise ValueError("at least one row is needed")
        longest = max(lens)
        T = self.num_frames(longest)  # refuses what no row may be
        if not self._packed:
            self._pack()
            self._packed = True
        ws = self._workspace(max(8, self.workspace_bytes(N, longest)))
        f = torch.empty((3, N), dtype=torch.float64, device=self.device)
        n = torch.empty(N, dtype=torch.int32, device=self.device)
        mg = torch.zeros((N, 2, T, self.n_bins), dtype=torch.float32, device=self.device) if mags else None
        dtype = _lib.VTTS_AUDIO_PCM16 if x.dtype == torch.int16 else _lib.VTTS_AUDIO_F32
        self._on_stream("forward", ptr(x), ptr(y), dtype, N, S, lens_c, ptr(f[0]), ptr(f[1]), ptr(f[2]), ptr(n), ptr(mg), T, ptr(ws), ws.numel())
        return SpectralResult(f[0], f[1], f[2], n, mg)


class MultiResolutionStft:
    """``MultiResolutionStft(resolutions, device)(ref, test, lengths=None)`` -> :class:`MrStftResult`: one :class:`SpectralMeter` per
    ``(n_fft, win, hop)``; ``mrstft`` is the mean over the resolutions of ``sc + logmag``, ``lsd`` the mean of theirs, per row."""

    def __init__(self, resolutions=PWG_RESOLUTIONS, device="cuda:0", lib_path=None):
        self.resolutions = tuple(tuple(int(v) for v in r) for r in resolutions)
        if not self.resolutions:
            raise ValueError("at least one resolution is needed")
        self.meters = tuple(SpectralMeter(*r, device=device, lib_path=lib_path) for r in self.resolutions)
        self.device = self.meters[0].device
        self.min_samples = max(m.min_samples for m in self.meters)

    def __call__(self, ref, test, lengths=None) -> MrStftResult:
        shortest = min(int(v) for v in lengths) if lengths is not None else int(ref.shape[-1])
        if shortest < self.min_samples:
            raise ValueError(f"a row of {shortest} samples is shorter than the {self.min_samples} the largest n_fft / 2 + 1 needs")
        rs = tuple(m(ref, test, lengths) for m in self.meters)
        k = float(len(rs))
        return MrStftResult(sum(r.sc + r.logmag for r in rs) / k, sum(r.lsd for r in rs) / k, rs)

    def close(self) -> None:
        for m in self.meters:
            m.close()


_METERS: dict = {}


def default_mrstft(device) -> MultiResolutionStft:
    """One MultiResolutionStft at Parallel WaveGAN's resolutions per device, created at first use: the command lines'."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    m = _METERS.get(device)
    if m is None:
        m = _METERS[device] = MultiResolutionStft(device=device)
    return m


def wav_mrstft(ref, test, lengths=None, meter: Optional[MultiResolutionStft] = None) -> MrStftResult:
    """The multi-resolution STFT distance and LSD of ``test`` against ``ref`` (both ``[N, S]`` or ``[S]``; tensors on a device or, with
    ``meter``, numpy arrays)."""
    if meter is None:
        t = ref if isinstance(ref, torch.Tensor) else test
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise ValueError("wav_mrstft needs a tensor on the device, or a meter")
        meter = default_mrstft(t.device)
    return meter(ref, test, lengths)


def format_result(r: MrStftResult, resolutions=PWG_RESOLUTIONS, row: int = 0) -> str:
    """The lines the command lines print for a row: one per resolution and the two means."""
    lines = [f"n_fft {n:4d} win {w:4d} hop {h:3d}: SC {float(p.sc[row]):.4f}  log-mag L1 {float(p.logmag[row]):.4f}  LSD {float(p.lsd[row]):.2f} dB  "
             f"({int(p.n_frames[row])} frames)" for (n, w, h), p in zip(resolutions, r.per_resolution)]
    lines.append(f"multi-resolution STFT distance {float(r.mrstft[row]):.4f}  LSD {float(r.lsd[row]):.2f} dB  (means over {len(r.per_resolution)} resolutions)")
    return "\n".join(lines)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="multi-resolution STFT distance and log-spectral distance of a recording against its reference, on the GPU")
    ap.add_argument("--ref", required=True, help="PCM16 mono .wav: the reference")
    ap.add_argument("--test", required=True, help="PCM16 mono .wav at the same rate, sample-aligned with --ref (lengths within one model hop)")
    return ap


def main(argv=None) -> None:
    from . import wavio
    from .stoi import check_pair

    a = build_parser().parse_args(argv)
    sr, x = wavio.read_wav(a.ref)
    sr2, y = wavio.read_wav(a.test)
    n = check_pair(sr, len(x), sr2, len(y))  # before the GPU is touched
    if not torch.cuda.is_available():
        raise RuntimeError("viettts_amd.spectral needs an MI355X visible to PyTorch-ROCm; there is no CPU path")
    dev = torch.device("cuda", torch.cuda.current_device())
    to_dev = lambda p: torch.from_numpy(np.ascontiguousarray(p[:n].astype(np.int16))[None, :]).to(dev)  # noqa: E731
    print(format_result(wav_mrstft(to_dev(x), to_dev(y))))


if __name__ == "__main__":
    main()
