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
soft knee, mono only.  No CPU fallback: the kernels are the only implementation.

    with lim.open_stream(rows=4, max_chunk=8192, out_dtype="pcm16") as s:   # LimiterStream: the same bits, chunk by chunk, 2 W + 24 samples late
        s.reset(0, gain=2.0)
        pcm, counts = s.push(chunk, last=False, rows=[0])                   # include/vtts_limstream.h, viettts_amd/csrc/limiter_stream.hip
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
        self._lib_path = lib_path
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

    def open_stream(self, rows: int, max_chunk: int, ceiling_dbtp: float = -1.0, out_dtype: str = "f32") -> "LimiterStream":
        """A streamed session of this limiter's rate, look-ahead and device: ``rows`` independent row slots fed chunk by chunk
        (:class:`LimiterStream`), each chunk of at most ``max_chunk`` samples."""
        return LimiterStream(self.sample_rate, rows, max_chunk, self.device, self.lookahead_ms, ceiling_dbtp, out_dtype, lib_path=self._lib_path)


def stream_emit(received: int, emitted: int, count: int, last: bool, W: int) -> int:
    """The streamed limiter's emit rule (include/vtts_limstream.h): the emitted count after a push of ``count`` samples onto ``received``
    of which ``emitted`` have left.  Whole runs of 16 whose look-ahead (2 W + 24 samples) has arrived; everything on ``last``."""
    r = int(received) + int(count)
    if last:
        return r
    return max(int(emitted), max(0, r - 2 * int(W) - 24) // _lib.LIMITER_RUN * _lib.LIMITER_RUN)


class LimiterStream(NativeHandle):
    """``TruePeakLimiter.limit`` fed chunk by chunk (include/vtts_limstream.h, viettts_amd/csrc/limiter_stream.hip): ``rows`` slots, each
    with its own cursor and pre-gain.  For every row the concatenation of what its pushes return equals ``limit`` on the whole row with
    ``gains[b] = gain``, bit for bit, and :meth:`results` after its last push equals ``limit``'s.  One launch per push for every row of it
    (and one small merge of the results); asynchronous on torch's current stream.  A context manager."""

    def __init__(self, sample_rate: int, rows: int, max_chunk: int, device="cuda:0", lookahead_ms: float = 5.0, ceiling_dbtp: float = -1.0,
                 out_dtype: str = "f32", lib_path=None):
        if out_dtype not in ("f32", "pcm16"):
            raise ValueError(f"out_dtype must be 'f32' or 'pcm16', got {out_dtype!r}")
        super().__init__("vtts_limstream", device, lib_path, "limiter stream")
        self.sample_rate, self.rows, self.max_chunk, self.out_dtype = int(sample_rate), int(rows), int(max_chunk), out_dtype
        self.ceiling_dbtp = float(ceiling_dbtp)
        self._create(C.byref(_lib.LimiterCfg(self.sample_rate, float(lookahead_ms))), tail=(self.rows, self.max_chunk, self.ceiling_dbtp))
        w = C.c_int32(0)
        self._call("lookahead", C.byref(w))
        self.lookahead = int(w.value)
        self.latency = 2 * self.lookahead + 24  # samples a row's output trails its input by (plus up to 15: whole runs of 16 leave)
        need = C.c_size_t(0)
        self._call("state_bytes", C.byref(need))
        self._state = torch.empty(int(need.value), dtype=torch.uint8, device=self.device)  # (never cleared: nothing is read before a row's sample 0)
        self._results = torch.zeros((self.rows, 3), dtype=torch.float32, device=self.device)
        self._dummy = torch.zeros(4, dtype=torch.float32, device=self.device)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self) -> None:
        super().close()
        self._state = self._results = self._dummy = None

    def reset(self, row: int, gain: float = 1.0) -> None:
        """Start a new row in slot ``row`` with the pre-gain ``gain`` (linear).  Host bookkeeping only."""
        self._call("reset", int(row), float(gain))

    def push(self, chunks, counts=None, last=False, rows=None):
        """Feed ``chunks``: ``[n, C]`` (row i's first ``counts[i]`` samples, all C without ``counts``) or a packed 1-D tensor with ``counts``;
        float32 or int16 on the device.  ``rows``: the slots, ``range(n)`` by default; ``last``: a bool or one per row.  Returns ``(packed,
        counts)``: the emitted samples of every row back to back (float32 or int16) and how many each row emitted."""
        if not isinstance(chunks, torch.Tensor):
            chunks = torch.as_tensor(np.asarray(chunks))
        if chunks.dtype not in (torch.float32, torch.int16):
            raise ValueError("chunks must be float32 or int16")
        chunks = chunks.to(self.device).contiguous()
        if chunks.dim() == 2:
            n, stride = int(chunks.shape[0]), int(chunks.shape[1])
            counts = [stride] * n if counts is None else [int(c) for c in counts]
            if len(counts) != n or (counts and max(counts) > stride):
                raise ValueError("counts must hold one count per row, none above the chunk's width")
            if stride == 0:  # (the C side reads a zero stride as packed, which an all-empty push is as well)
                chunks = chunks.reshape(-1)
        elif chunks.dim() == 1 and counts is not None:
            counts = [int(c) for c in counts]
            n, stride = len(counts), 0
            if sum(counts) != chunks.numel():
                raise ValueError("a packed push holds exactly sum(counts) samples")
        else:
            raise ValueError("chunks must be [n, C], or 1-D with counts")
        rows = list(range(n)) if rows is None else [int(r) for r in rows]
        lasts = [bool(last)] * n if isinstance(last, (bool, int, np.bool_)) else [bool(v) for v in last]
        if len(rows) != n or len(lasts) != n:
            raise ValueError("rows and last must hold one entry per row of the push")
        if n < 1:
            raise ValueError("a push names at least one row")
        i32 = C.c_int32 * n
        got = i32()
        pcm = self.out_dtype == "pcm16"
        room = sum(counts) + n * (self.latency + 15)
        out = torch.empty(max(room, 1), dtype=torch.int16 if pcm else torch.float32, device=self.device)
        src = chunks if chunks.numel() else self._dummy
        self._on_stream("push", ptr(self._state), ptr(src), _lib.VTTS_AUDIO_PCM16 if chunks.dtype == torch.int16 else _lib.VTTS_AUDIO_F32, n, i32(*rows),
                        stride, i32(*counts), i32(*[int(v) for v in lasts]), ptr(out), _lib.VTTS_AUDIO_PCM16 if pcm else _lib.VTTS_AUDIO_F32, got,
                        ptr(self._results))
        emitted = [int(v) for v in got]
        return out[:sum(emitted)], emitted

    def results(self) -> LimiterResult:
        """Per slot, on the device: the running ``true_peak`` and ``min_gain`` over the samples emitted so far (``limit``'s after a row's last
        push) and the pre-gain; ``envelope`` is None."""
        r = self._results
        return LimiterResult(r[:, 0], r[:, 1], r[:, 2], None)


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
