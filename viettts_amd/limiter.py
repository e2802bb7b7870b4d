"""True-peak metering and a look-ahead limiter on the GPU (include/vtts_limiter.h, viettts_amd/csrc/limiter.hip): the inter-sample peak of mono
waveforms from a 4x oversampled reconstruction, and a per-sample gain that keeps it under a ceiling in dBTP, written as float32 or PCM16.

    lim = TruePeakLimiter(16000, device="cuda:0", lookahead_ms=5.0)
    tp = lim.true_peak(wav, lengths)                                    # [N] float32, linear (1.0 = 0 dBTP)
    y, r = lim.limit(wav, lengths, gains=None, ceiling_dbtp=-1.0)       # r = LimiterResult(true_peak, min_gain, gains, envelope)
    pcm, r = lim.normalize(wav, lengths, target=-16.0, ceiling_dbtp=-1.0, out_dtype="pcm16")

    python -m viettts_amd.limiter --wav F.wav [--target -16 --ceiling-dbtp -1 --output out.wav]

``normalize`` is ``LoudnessMeter`` -> the gain to the target (no peak term) -> the limiter, without a host round trip: where
``LoudnessMeter.normalize`` backs a whole row off for one plosive, this holds the plosive down and leaves the row at its gain.  The limited
row is not metered again, so it ends a little under the target where the limiter worked.  The oversampling factor is 4 at every rate (a
component at the Nyquist frequency reads up to 0.69 dB low).  No loudness range, no release shaping but the symmetric window, no multiband or
soft knee, mono only, and the streamed paths are not hooked.  No CPU fallback: the kernels are the only implementation.
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


class LimiterResult(NamedTuple):
    true_peak: torch.Tensor           # [N] float32: the INPUT's true peak, linear; 0 for an empty row
    min_gain: torch.Tensor            # [N] float32: the deepest reduction min a[n], 1 where the limiter did nothing
    gains: torch.Tensor               # [N] float32: the pre-gain each row was multiplied by
    envelope: Optional[torch.Tensor]  # [N, S] float32 with ``envelope=True``: max(|x[n]|, |u[4 n .. 4 n + 3]|), 0 past a row's own samples


def _rows(wav):
    if isinstance(wav, (np.ndarray, torch.Tensor)) and wav.ndim == 1:
        wav = wav[None, :]
    return wav


class TruePeakLimiter(NativeHandle):
    """``TruePeakLimiter(sample_rate, device, lookahead_ms)``.  ``wav [N, S]`` (or ``[S]``) is float32 or int16 PCM, a tensor on the device or
    a numpy array; results are tensors on the device.  A row's results are bit for bit what the row gives alone.  Asynchronous on torch's
    current stream of the device.  One limiter serves one call at a time on one device."""

    def __init__(self, sample_rate: int = 16000, device="cuda:0", lookahead_ms: float = 5.0, lib_path=None):
        super().__init__("vtts_limiter", device, lib_path, "limiter")
        self.sample_rate = int(sample_rate)
        self.lookahead_ms = float(lookahead_ms)
        self._create(C.byref(_lib.LimiterCfg(self.sample_rate, self.lookahead_ms)))  # refuses rates outside 8 .. 96 kHz, look-ahead outside (0, 10] ms
        w = C.c_int32(0)
        self._call("lookahead", C.byref(w))
        self.lookahead = int(w.value)

    def taps(self) -> np.ndarray:
        """The kernels' taps, ``[4, 52]`` float32: phase r in ascending n, the zero padding first."""
        out = np.zeros((4, _lib.LIMITER_PHASE_TAPS), dtype=np.float32)
        self._call("taps", out.ctypes.data_as(_lib.fp))
        return out

    def _scratch(self, N: int, longest: int) -> torch.Tensor:
        need = C.c_size_t(0)
        self._call("workspace_bytes", N, longest, C.byref(need))
        return self._workspace(int(need.value))

    def true_peak(self, wav, lengths=None, envelope: bool = False):
        """``[N]`` float32 true peaks; with ``envelope=True`` ``(true_peak, envelope [N, S])``."""
        y, lens, lens_c = waveform_rows(_rows(wav), lengths, self.device, "wav")
        N, S = y.shape
        ws = self._scratch(N, max(lens) if lens else 0)
        tp = torch.empty(N, dtype=torch.float32, device=self.device)
        env = torch.empty((N, S), dtype=torch.float32, device=self.device) if envelope else None
        dtype = _lib.VTTS_AUDIO_PCM16 if y.dtype == torch.int16 else _lib.VTTS_AUDIO_F32
        self._on_stream("true_peak", ptr(y), dtype, N, S, lens_c, ptr(tp), ptr(env), ptr(ws), ws.numel())
        return (tp, env) if envelope else tp

    def limit(self, wav, lengths=None, gains=None, ceiling_dbtp: float = -1.0, out_dtype: str = "f32", packed: bool = False, envelope: bool = False):
        """Multiply row b by ``gains[b]`` (``[N]`` float32 on the device, a sequence, or None for 1) and hold its true peak at ``ceiling_dbtp``.
        Returns ``(samples, LimiterResult)``: ``[N, S]`` float32 or int16 with zeros past a row's own samples, or with ``packed=True`` one 1-D
        tensor holding the rows back to back."""
        if out_dtype not in ("f32", "pcm16"):
            raise ValueError(f"out_dtype must be 'f32' or 'pcm16', got {out_dtype!r}")
        y, lens, lens_c = waveform_rows(_rows(wav), lengths, self.device, "wav")
        N, S = y.shape
        if gains is not None:
            gains = torch.as_tensor(gains, dtype=torch.float32, device=self.device).contiguous()
            if gains.shape != (N,):
                raise ValueError("gains must hold one float32 per row")
        ws = self._scratch(N, max(lens) if lens else 0)
        tdt = torch.int16 if out_dtype == "pcm16" else torch.float32
        total = sum(lens) if packed else N * S
        buf = torch.empty(max(total, 1), dtype=tdt, device=self.device)  # (one element where nothing is written: the C side wants a pointer)
        f = torch.empty((3, N), dtype=torch.float32, device=self.device)
        env = torch.empty((N, S), dtype=torch.float32, device=self.device) if envelope else None
        dtype = _lib.VTTS_AUDIO_PCM16 if y.dtype == torch.int16 else _lib.VTTS_AUDIO_F32
        odt = _lib.VTTS_AUDIO_PCM16 if out_dtype == "pcm16" else _lib.VTTS_AUDIO_F32
        self._on_stream("apply", ptr(y), dtype, N, S, lens_c, ptr(gains), float(ceiling_dbtp), ptr(buf), odt, 0 if packed else S, ptr(f[0]), ptr(f[1]), ptr(f[2]),
                        ptr(env), ptr(ws), ws.numel())
        return (buf[:total] if packed else buf[:total].view(N, S)), LimiterResult(f[0], f[1], f[2], env)

    def normalize(self, wav, lengths=None, target: float = -23.0, ceiling_dbtp: float = -1.0, max_gain_db: float = 30.0, out_dtype: str = "f32",
                  packed: bool = False, meter=None):
        """Meter every row (``meter``: a ``LoudnessMeter`` of this rate and device, the cached one by default), multiply it by
        ``min(10^((target - I) / 20), 10^(max_gain_db / 20))`` (1 for a row without a loudness) and limit it at ``ceiling_dbtp``.  Returns what
        :meth:`limit` returns."""
        from .loudness import default_meter

        y, lens, _ = waveform_rows(_rows(wav), lengths, self.device, "wav")
        meter = default_meter(self.device, self.sample_rate) if meter is None else meter
        r = meter(y, lengths)
        N = y.shape[0]
        gains = torch.empty(N, dtype=torch.float32, device=self.device)
        self._on_stream("pregain", ptr(r.integrated), N, float(target), float(max_gain_db), ptr(gains))
        return self.limit(y, lengths, gains=gains, ceiling_dbtp=ceiling_dbtp, out_dtype=out_dtype, packed=packed)


_LIMITERS: dict = {}


def default_limiter(device, sample_rate: int = 16000) -> TruePeakLimiter:
    """One TruePeakLimiter (5 ms look-ahead) per (rate, device), created at first use: the CLIs' and the pipeline's."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(sample_rate), device)
    m = _LIMITERS.get(key)
    if m is None:
        m = _LIMITERS[key] = TruePeakLimiter(sample_rate, device)
    return m


def _db(v: float) -> float:
    return 20.0 * float(np.log10(v)) if v > 0 else float("-inf")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="True peak of a recording on the GPU, and its gain to a target loudness under a true-peak ceiling")
    ap.add_argument("--wav", required=True, help="PCM16 mono .wav; metered at its own rate (8 .. 96 kHz)")
    ap.add_argument("--target", type=float, default=None, help="target level in LUFS (the rate must then be divisible by 10); with --output, the limited PCM16 is written at the input's rate")
    ap.add_argument("--ceiling-dbtp", type=float, default=-1.0, help="true-peak ceiling in dBTP")
    ap.add_argument("--max-gain-db", type=float, default=30.0)
    ap.add_argument("--lookahead-ms", type=float, default=5.0)
    ap.add_argument("--output", default=None)
    return ap


def main(argv=None) -> None:
    from . import wavio

    a = build_parser().parse_args(argv)
    if a.output and a.target is None:
        raise SystemExit("--output needs --target")
    if not torch.cuda.is_available():
        raise RuntimeError("viettts_amd.limiter needs an MI355X visible to PyTorch-ROCm; there is no CPU path")
    dev = torch.device("cuda", torch.cuda.current_device())
    sr, pcm = wavio.read_wav(a.wav)
    y = torch.from_numpy(np.ascontiguousarray(pcm.astype(np.int16))[None, :]).to(dev)
    lim = default_limiter(dev, sr) if a.lookahead_ms == 5.0 else TruePeakLimiter(sr, dev, a.lookahead_ms)
    tp = float(lim.true_peak(y)[0])
    sp = float(y.abs().max()) / 32768.0 if y.numel() else 0.0
    print(f"true peak {_db(tp):.2f} dBTP  sample peak {_db(sp):.2f} dBFS  (4x oversampled, look-ahead {lim.lookahead} samples)")
    if a.target is not None:
        out, r = lim.normalize(y, target=a.target, ceiling_dbtp=a.ceiling_dbtp, max_gain_db=a.max_gain_db, out_dtype="pcm16")
        print(f"gain {_db(float(r.gains[0])):+.2f} dB to {a.target:.1f} LUFS (at most {a.max_gain_db:.1f} dB), deepest reduction {_db(float(r.min_gain[0])):.2f} dB "
              f"under a ceiling of {a.ceiling_dbtp:.1f} dBTP")
        if a.output:
            wavio.write_wav_pcm16(a.output, out[0].cpu().numpy(), sr)
            print(f"wrote {a.output}")


if __name__ == "__main__":
    main()
