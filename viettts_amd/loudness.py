"""Loudness on the GPU: batched ITU-R BS.1770-4 integrated loudness (the "LUFS" of EBU R 128) of mono waveforms, and a per-row gain to a
target level written as float32 or PCM16 (include/vtts_loudness.h, viettts_amd/csrc/loudness.hip).

    m = LoudnessMeter(16000, device="cuda:0")
    r = m(wav, lengths)                        # [N, S] -> LoudnessResult(integrated, momentary_max, sample_peak, n_blocks, n_gated, momentary)
    pcm, gains = m.normalize(wav, lengths, target=-23.0, ceiling_db=-1.0, max_gain_db=30.0, out_dtype="pcm16")

    python -m viettts_amd.loudness --wav F.wav [--target -23 --output out.wav]

Everything stays on the device: ``normalize`` reads the meter's results where the kernel left them.  The ceiling acts on the SAMPLE peak;
true-peak metering and the look-ahead limiter are ``viettts_amd.limiter.TruePeakLimiter`` (its ``normalize`` runs this meter and holds the ceiling
in dBTP instead); there is no loudness range or multichannel weighting, and the streamed synthesis paths are not hooked
(integrated loudness needs the whole utterance).  The reference has no loudness stage; nothing here is re-exported under ``vietTTS/``.
No CPU fallback: the kernels are the only implementation.
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


class LoudnessResult(NamedTuple):
    integrated: torch.Tensor      # [N] float32: LUFS, -inf for a row shorter than 0.4 s or with no block above the gates
    momentary_max: torch.Tensor   # [N] float32: the loudest 400 ms block, -inf without a block
    sample_peak: torch.Tensor     # [N] float32: max |x|, exact
    n_blocks: torch.Tensor        # [N] int32: 400 ms blocks at 75 % overlap
    n_gated: torch.Tensor         # [N] int32: the blocks above both gates
    momentary: Optional[torch.Tensor]  # [N, J] float32 with ``series=True``: every block's loudness, -inf past a row's own blocks


class LoudnessMeter(NativeHandle):
    """``LoudnessMeter(sample_rate, device)(wav, lengths=None, series=False)`` — ``wav [N, S]`` (or ``[S]``) float32 or int16 PCM (a tensor
    on the device or a numpy array) -> :class:`LoudnessResult`, tensors on the device.  The K-weighting filter starts from zero state at each
    row's own first sample; a row's results are bit for bit what the row gives alone.  Asynchronous on torch's current stream of the device.
    One meter serves one call at a time on one device."""

    def __init__(self, sample_rate: int = 16000, device="cuda:0", lib_path=None):
        super().__init__("vtts_loudness", device, lib_path, "meter")
        self.sample_rate = int(sample_rate)
        self._create(C.byref(_lib.LoudnessCfg(self.sample_rate)))  # refuses rates outside 8 .. 96 kHz or not divisible by 10
        self.hop = self.sample_rate // 10

    def coefficients(self) -> np.ndarray:
        """The K-weighting coefficients in double: shelf b0 b1 b2 a1 a2, then high-pass b0 b1 b2 a1 a2."""
        out = (C.c_double * 10)()
        self._call("coefficients", out)
        return np.array(out, dtype=np.float64)

    def num_blocks(self, n_samples: int) -> int:
        n = C.c_int64(0)
        self._call("num_blocks", int(n_samples), C.byref(n))
        return int(n.value)

    def _rows(self, wav):
        if isinstance(wav, np.ndarray) and wav.ndim == 1:
            wav = wav[None, :]
        if isinstance(wav, torch.Tensor) and wav.dim() == 1:
            wav = wav[None, :]
        return wav

    def __call__(self, wav, lengths=None, series: bool = False) -> LoudnessResult:
        y, lens, lens_c = waveform_rows(self._rows(wav), lengths, self.device, "wav")
        N, S = y.shape
        longest = max(lens) if lens else 0
        need = C.c_size_t(0)
        self._call("workspace_bytes", N, longest, C.byref(need))
        ws = self._workspace(int(need.value))
        f = torch.empty((3, N), dtype=torch.float32, device=self.device)
        n = torch.empty((2, N), dtype=torch.int32, device=self.device)
        J = self.num_blocks(longest)
        mom = torch.empty((N, J), dtype=torch.float32, device=self.device) if series else None
        dtype = _lib.VTTS_AUDIO_PCM16 if y.dtype == torch.int16 else _lib.VTTS_AUDIO_F32
        self._on_stream("measure", ptr(y), dtype, N, S, lens_c, ptr(f[0]), ptr(f[1]), ptr(f[2]), ptr(n[0]), ptr(n[1]), ptr(mom), J, ptr(ws), ws.numel())
        return LoudnessResult(f[0], f[1], f[2], n[0], n[1], mom)

    def normalize(self, wav, lengths=None, target: float = -23.0, ceiling_db: float = -1.0, max_gain_db: float = 30.0, out_dtype: str = "f32",
                  packed: bool = False):
        """Meter every row and multiply it by ``min(10^((target - I) / 20), 10^(max_gain_db / 20), 10^(ceiling_db / 20) / sample_peak)`` (1 for
        a row without a loudness).  Returns ``(samples, gains)``: ``[N, S]`` float32 or int16 with zeros past a row's own samples, or with
        ``packed=True`` one 1-D tensor holding the rows back to back; ``gains [N]`` float32."""
        if out_dtype not in ("f32", "pcm16"):
            raise ValueError(f"out_dtype must be 'f32' or 'pcm16', got {out_dtype!r}")
        y, lens, lens_c = waveform_rows(self._rows(wav), lengths, self.device, "wav")
        r = self(y, lengths)
        N, S = y.shape
        tdt = torch.int16 if out_dtype == "pcm16" else torch.float32
        total = sum(lens) if packed else N * S
        buf = torch.empty(max(total, 1), dtype=tdt, device=self.device)  # (one element where nothing is written: the C side wants a pointer)
        gains = torch.empty(N, dtype=torch.float32, device=self.device)
        dtype = _lib.VTTS_AUDIO_PCM16 if y.dtype == torch.int16 else _lib.VTTS_AUDIO_F32
        odt = _lib.VTTS_AUDIO_PCM16 if out_dtype == "pcm16" else _lib.VTTS_AUDIO_F32
        self._on_stream("normalize", ptr(y), dtype, N, S, lens_c, ptr(r.integrated), ptr(r.sample_peak), float(target), float(ceiling_db), float(max_gain_db),
                        ptr(buf), odt, 0 if packed else S, ptr(gains))
        return (buf[:total] if packed else buf[:total].view(N, S)), gains


_METERS: dict = {}


def default_meter(device, sample_rate: int = 16000) -> LoudnessMeter:
    """One LoudnessMeter per (rate, device), created at first use: the CLIs' and the pipeline's."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(sample_rate), device)
    m = _METERS.get(key)
    if m is None:
        m = _METERS[key] = LoudnessMeter(sample_rate, device)
    return m


def format_result(r: LoudnessResult, row: int = 0) -> str:
    """The one line the command lines print for a row."""
    return (f"integrated {float(r.integrated[row]):.2f} LUFS  momentary max {float(r.momentary_max[row]):.2f} LUFS  "
            f"sample peak {20.0 * float(torch.log10(r.sample_peak[row].double())):.2f} dBFS  ({int(r.n_gated[row])} of {int(r.n_blocks[row])} blocks gated in)")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="BS.1770 integrated loudness of a recording on the GPU, and its gain to a target level")
    ap.add_argument("--wav", required=True, help="PCM16 mono .wav; metered at its own rate (8 .. 96 kHz, divisible by 10)")
    ap.add_argument("--target", type=float, default=None, help="target level in LUFS; with --output, the normalised PCM16 is written at the input's rate")
    ap.add_argument("--ceiling-db", type=float, default=-1.0, help="sample-peak ceiling in dBFS")
    ap.add_argument("--max-gain-db", type=float, default=30.0)
    ap.add_argument("--output", default=None)
    return ap


def main(argv=None) -> None:
    from . import wavio

    a = build_parser().parse_args(argv)
    if a.output and a.target is None:
        raise SystemExit("--output needs --target")
    if not torch.cuda.is_available():
        raise RuntimeError("viettts_amd.loudness needs an MI355X visible to PyTorch-ROCm; there is no CPU path")
    dev = torch.device("cuda", torch.cuda.current_device())
    sr, pcm = wavio.read_wav(a.wav)
    y = torch.from_numpy(np.ascontiguousarray(pcm.astype(np.int16))[None, :]).to(dev)
    m = default_meter(dev, sr)
    print(format_result(m(y)))
    if a.target is not None:
        out, gains = m.normalize(y, target=a.target, ceiling_db=a.ceiling_db, max_gain_db=a.max_gain_db, out_dtype="pcm16")
        g = float(gains[0])
        print(f"gain {20.0 * np.log10(g):+.2f} dB to {a.target:.1f} LUFS (ceiling {a.ceiling_db:.1f} dBFS, at most {a.max_gain_db:.1f} dB)")
        if a.output:
            wavio.write_wav_pcm16(a.output, out[0].cpu().numpy(), sr)
            print(f"wrote {a.output}")


if __name__ == "__main__":
    main()
