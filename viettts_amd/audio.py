"""The audio stage either side of the models, on the GPU (include/vtts_audio.h, viettts_amd/csrc/audio.hip): rational sample-rate
conversion with a Kaiser-windowed sinc, and PCM16 in and out, one fused kernel.

    Resampler(48000, 16000, device)(wav)                      # [N, S] float32 or int16 -> [N, ceil(S / 3)] float32
    Resampler(16000, 44100, device)(wav, lengths, out_dtype="pcm16", packed=True)   # ragged rows, packed int16, ready for a WAV file
    to_pcm16(wav)                                             # wavio.float_to_pcm16 on the device, bit for bit
    with Resampler(16000, 48000, device).open_stream(rows=4, max_chunk=8192, out_dtype="pcm16") as s:   # ResamplerStream: the same bits,
        pcm, counts = s.push(chunk, last=False, rows=[0])     # chunk by chunk (include/vtts_rsstream.h, viettts_amd/csrc/resample_stream.hip)

The reference has no such stage: it writes 16 kHz samples with ``sf.write`` and relabels them when asked for another rate.
No CPU fallback: the input lives on (or is copied to) the GPU.
"""
from __future__ import annotations

import ctypes as C
from typing import List

import numpy as np
import torch

from . import _lib
from ._handle import NativeHandle, ptr

_DTYPES = {"f32": (torch.float32, _lib.VTTS_AUDIO_F32), "pcm16": (torch.int16, _lib.VTTS_AUDIO_PCM16)}


def waveform_rows(x, lengths, device, what: str):
    """A waveform argument as the kernels take it: ``x`` (numpy array or tensor on ``device``, float32 or int16, ``[N, S]``) as a contiguous
    device tensor, and ``lengths`` (samples per row, or None for all ``S``) as a list and as the ``c_int32`` array the C side reads (None
    without ``lengths``).  ``what`` names the argument in messages."""
    if isinstance(x, np.ndarray):
        if x.dtype != np.int16:
            x = x.astype(np.float32, copy=False)
        x = torch.from_numpy(np.ascontiguousarray(x)).to(device)
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{what} must be a torch.Tensor on {device} or a numpy array")
    if x.device != device:
        raise ValueError(f"{what} is on {x.device}, expected {device}")
    if x.dim() != 2 or x.dtype not in (torch.float32, torch.int16):
        raise ValueError(f"{what} must be float32 or int16 [N, S], got {tuple(x.shape)} {x.dtype}")
    x = x.contiguous()
    N, S = x.shape
    if lengths is None:
        return x, [S] * N, None
    lens = [int(v) for v in (lengths.tolist() if isinstance(lengths, (torch.Tensor, np.ndarray)) else lengths)]
    if len(lens) != N:
        raise ValueError("lengths must hold one sample count per row")
    return x, lens, (C.c_int32 * N)(*lens)


class Resampler(NativeHandle):
    """``Resampler(in_rate, out_rate, device)(wav, lengths=None, out_dtype="f32", packed=False)``.

    ``wav`` is ``[N, S]`` (or ``[S]``) float32 or int16 PCM, a tensor on the device or a numpy array.  Row b's first ``lengths[b]``
    samples (all ``S`` without ``lengths``) give ``out_samples(lengths[b])`` output samples, filtered with zeros beyond the row's own
    ends: bit for bit what the row gives alone.  The result is ``[N, longest]`` with zeros past a row's own count, or with
    ``packed=True`` one 1-D tensor holding the rows back to back.  ``in_rate == out_rate`` converts the format only.
    Asynchronous on torch's current stream of the device.  One Resampler serves one call at a time on one device."""

    def __init__(self, in_rate: int, out_rate: int, device="cuda:0", lib_path=None):
        super().__init__("vtts_audio", device, lib_path, "resampler")
        self._lib_path = lib_path
        self.in_rate, self.out_rate = int(in_rate), int(out_rate)
        self._create(C.byref(_lib.AudioCfg(self.in_rate, self.out_rate)))
        L, M, half = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._call("ratio", C.byref(L), C.byref(M), C.byref(half))
        self.L, self.M, self.half = int(L.value), int(M.value), int(half.value)

    @property
    def prototype(self) -> np.ndarray:
        """The ``2 * half + 1`` float64 taps the table was rounded from."""
        h = np.empty(2 * self.half + 1, dtype=np.float64)
        self._call("prototype", h.ctypes.data_as(C.POINTER(C.c_double)))
        return h

    def out_samples(self, n_in: int) -> int:
        n = C.c_int64(0)
        self._call("out_samples", int(n_in), C.byref(n))
        return int(n.value)

    def out_lengths(self, lengths) -> List[int]:
        return [self.out_samples(int(n)) for n in lengths]

    def __call__(self, wav, lengths=None, out_dtype: str = "f32", packed: bool = False) -> torch.Tensor:
        if out_dtype not in _DTYPES:
            raise ValueError(f"out_dtype must be 'f32' or 'pcm16', got {out_dtype!r}")
        one_row = getattr(wav, "ndim", 2) == 1
        if one_row:
            wav = wav[None, :]
        wav, lens, lens_c = waveform_rows(wav, lengths, self.device, "wav")
        N, S = wav.shape
        if N < 1 or S < 1:
            raise ValueError(f"wav must have at least one row and one sample, got {tuple(wav.shape)}")
        outs = [self.out_samples(n) for n in lens] if lengths is not None else [self.out_samples(S)] * N
        tdt, code = _DTYPES[out_dtype]
        if packed:
            out, o_stride = torch.empty((sum(outs),), dtype=tdt, device=self.device), 0
        else:
            o_stride = max(max(outs), 1)
            out = torch.empty((N, o_stride), dtype=tdt, device=self.device)
        if self._blob is None:  # the tap table goes to the device once, at the first call
            self._pack()
        in_code = _lib.VTTS_AUDIO_PCM16 if wav.dtype == torch.int16 else _lib.VTTS_AUDIO_F32
        if out.numel():
            self._on_stream("forward", ptr(wav), in_code, N, S, lens_c, ptr(out), code, o_stride)
        if not packed and max(outs) == 0:
            out = out[:, :0]
        return out[0] if one_row and not packed else out

    def open_stream(self, rows: int, max_chunk: int, out_dtype: str = "f32") -> "ResamplerStream":
        """A streamed session of this resampler's rates and device: ``rows`` independent row slots fed chunk by chunk
        (:class:`ResamplerStream`), each chunk of at most ``max_chunk`` samples.  The session binds this resampler's tap table."""
        return ResamplerStream(self, rows, max_chunk, out_dtype)


def resample_emit(received: int, emitted: int, count: int, last: bool, L: int, M: int, half: int) -> int:
    """The streamed resampler's emit rule (include/vtts_rsstream.h): the emitted count after a push of ``count`` samples onto ``received``
    of which ``emitted`` have left.  The outputs whose newest input ``(m M + half) // L`` has arrived; ``ceil(R' L / M)`` on ``last``;
    ``R'`` when the rates are equal (``L == M == 1``)."""
    r = int(received) + int(count)
    L, M, half = int(L), int(M), int(half)
    if L == M:
        return r
    if last:
        return -((-r * L) // M)
    return max(int(emitted), 0, -((half - r * L) // M))


class ResamplerStream(NativeHandle):
    """``Resampler`` fed chunk by chunk (include/vtts_rsstream.h, viettts_amd/csrc/resample_stream.hip): ``rows`` slots, each with its own
    cursor.  For every row the concatenation of what its pushes return equals the resampler on the whole row, bit for bit, ``latency``
    input samples late.  One launch per push for every row of it; asynchronous on torch's current stream.  A context manager."""

    def __init__(self, resampler: Resampler, rows: int, max_chunk: int, out_dtype: str = "f32"):
        if out_dtype not in _DTYPES:
            raise ValueError(f"out_dtype must be 'f32' or 'pcm16', got {out_dtype!r}")
        super().__init__("vtts_rsstream", resampler.device, resampler._lib_path, "resampler stream")
        self.in_rate, self.out_rate, self.rows, self.max_chunk, self.out_dtype = resampler.in_rate, resampler.out_rate, int(rows), int(max_chunk), out_dtype
        self._create(C.byref(_lib.AudioCfg(self.in_rate, self.out_rate)), tail=(self.rows, self.max_chunk))
        self.L, self.M, self.half = resampler.L, resampler.M, resampler.half
        self.identity = self.in_rate == self.out_rate
        self.latency = 0 if self.identity else -(-self.half // self.L)  # input samples a row's output trails its input by
        if not self.identity:
            if resampler._blob is None:  # the tap table goes to the device once
                resampler._pack()
            self.adopt_packed(resampler.packed_blob())
        need = C.c_size_t(0)
        self._call("state_bytes", C.byref(need))
        self._state = torch.empty(int(need.value), dtype=torch.uint8, device=self.device)  # (never cleared: nothing is read before a row's sample 0)
        self._dummy = torch.zeros(4, dtype=torch.float32, device=self.device)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self) -> None:
        super().close()
        self._state = self._dummy = None

    def reset(self, row: int) -> None:
        """Start a new row in slot ``row``.  Host bookkeeping only."""
        self._call("reset", int(row))

    def cursor(self, row: int):
        """``(received, emitted, closed)`` of slot ``row``, as the host holds them."""
        r, f, c = C.c_int64(0), C.c_int64(0), C.c_int(0)
        self._call("cursor", int(row), C.byref(r), C.byref(f), C.byref(c))
        return int(r.value), int(f.value), bool(c.value)

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
        tdt, code = _DTYPES[self.out_dtype]
        room = sum(counts) if self.identity else sum((c * self.L + self.half) // self.M + 2 for c in counts)
        out = torch.empty(max(room, 1), dtype=tdt, device=self.device)
        src = chunks if chunks.numel() else self._dummy
        self._on_stream("push", ptr(self._state), ptr(src), _lib.VTTS_AUDIO_PCM16 if chunks.dtype == torch.int16 else _lib.VTTS_AUDIO_F32, n, i32(*rows),
                        stride, i32(*counts), i32(*[int(v) for v in lasts]), ptr(out), code, got)
        emitted = [int(v) for v in got]
        return out[:sum(emitted)], emitted


_RESAMPLERS: dict = {}


def resampler(in_rate: int, out_rate: int, device) -> Resampler:
    """One Resampler per (rates, device), created at first use: the CLIs' and the pipeline's."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(in_rate), int(out_rate), device)
    r = _RESAMPLERS.get(key)
    if r is None:
        r = _RESAMPLERS[key] = Resampler(in_rate, out_rate, device)
    return r


def to_pcm16(wav, lengths=None, packed: bool = False) -> torch.Tensor:
    """``wavio.float_to_pcm16`` on the device, bit for bit (NaN gives 0): float32 (or int16, copied) ``[N, S]`` or ``[S]`` -> int16."""
    if isinstance(wav, torch.Tensor) and wav.is_cuda:
        device = wav.device
    else:
        device = torch.device("cuda", torch.cuda.current_device())
    return resampler(1, 1, device)(wav, lengths=lengths, out_dtype="pcm16", packed=packed)
