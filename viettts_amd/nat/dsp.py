"""vietTTS/nat/dsp.py:104-128 — ``MelFilter``: waveform -> 80-band log-mel, the transform the acoustic model is trained on and the
vocoder is conditioned on (vietTTS/hifigan/create_mel.py ``mel_spectrogram`` computes the same thing in torch).

The reference builds the filter bank with librosa and runs an XLA FFT; here one fused HIP kernel (include/vtts_mel.h,
viettts_amd/csrc/mel.hip) turns the samples into ``[N, T, n_mels]`` log-mel, the layout ``Generator.__call__`` takes, without
the spectrum ever reaching HBM.  No CPU fallback: the input lives on (or is copied to) the GPU.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from .. import _lib


class MelFilter:
    """``MelFilter(sample_rate, n_fft, n_mels, fmin, fmax)(y)`` — ``y [N, S]`` float32 or int16 PCM -> ``[N, T, n_mels]`` float32.

    hop = n_fft / 4 and window = n_fft, as in the reference's ``__call__``.  One MelFilter serves one call at a time on one device.
    """

    def __init__(self, sample_rate: int, n_fft: int, n_mels: int, fmin=0.0, fmax=8000, device="cuda:0", lib_path=None):
        self.lib = _lib.load(lib_path)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("MelFilter needs a ROCm device ('cuda:N'); there is no CPU path")
        self.sample_rate, self.n_fft, self.n_mels, self.hop = int(sample_rate), int(n_fft), int(n_mels), int(n_fft) // 4
        self.frames_per_workgroup = _lib.MEL_FRAMES_PER_BLOCK
        self._h = C.c_void_p(0)
        cfg = _lib.MelCfg(self.sample_rate, self.n_fft, self.hop, self.n_mels, float(fmin), float(fmax))
        dev_index = self.device.index if self.device.index is not None else 0
        _lib.check(self.lib, self.lib.vtts_mel_create(C.byref(cfg), dev_index, C.byref(self._h)))
        self._blob: Optional[torch.Tensor] = None

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self.lib.vtts_mel_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def melfb(self) -> np.ndarray:
        """The ``[n_mels, n_fft / 2 + 1]`` float32 basis (the reference's attribute of the same name)."""
        fb = np.empty((self.n_mels, self.n_fft // 2 + 1), dtype=np.float32)
        _lib.check(self.lib, self.lib.vtts_mel_filterbank(self._h, fb.ctypes.data_as(C.POINTER(C.c_float))))
        return fb

    def num_frames(self, n_samples: int) -> int:
        n = C.c_int64(0)
        _lib.check(self.lib, self.lib.vtts_mel_num_frames(self._h, int(n_samples), C.byref(n)))
        return int(n.value)

    def _pack(self):
        """The tables go to the device once, at the first call."""
        if self._blob is None:
            n = C.c_size_t(0)
            _lib.check(self.lib, self.lib.vtts_mel_packed_bytes(self._h, C.byref(n)))
            blob = torch.empty(int(n.value), dtype=torch.uint8, device=self.device)
            stream = torch.cuda.current_stream(self.device)
            with torch.cuda.device(self.device):
                _lib.check(self.lib, self.lib.vtts_mel_pack(self._h, C.c_void_p(blob.data_ptr()), blob.numel(), C.c_void_p(stream.cuda_stream)))
            self._blob = blob

    def __call__(self, y, lengths=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Asynchronous on torch's current stream of the device.  ``lengths``: samples per row (ints, host); row b is reflected at its
        own end and frames past its own count hold ``log(1e-5)``."""
        if isinstance(y, np.ndarray):
            if y.dtype != np.int16:
                y = y.astype(np.float32, copy=False)
            y = torch.from_numpy(np.ascontiguousarray(y)).to(self.device)
        if not isinstance(y, torch.Tensor):
            raise TypeError("y must be a torch.Tensor on the filter's device or a numpy array")
        if y.device != self.device:
            raise ValueError(f"y is on {y.device}, MelFilter on {self.device}")
        if y.dim() != 2 or y.dtype not in (torch.float32, torch.int16):
            raise ValueError(f"y must be float32 or int16 [N, S], got {tuple(y.shape)} {y.dtype}")
        y = y.contiguous()
        N, S = y.shape
        if lengths is None:
            lens, lens_c = [S] * N, None
        else:
            lens = [int(v) for v in (lengths.tolist() if isinstance(lengths, (torch.Tensor, np.ndarray)) else lengths)]
            if len(lens) != N:
                raise ValueError("lengths must hold one sample count per row")
            lens_c = (C.c_int32 * N)(*lens)
        T = max(self.num_frames(n) for n in set(lens))  # refuses rows too short to reflect
        shape = (N, T, self.n_mels)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        elif out.shape != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != self.device:
            raise ValueError("out must be a contiguous float32 [N, T, n_mels] tensor on the filter's device")
        self._pack()
        stream = torch.cuda.current_stream(self.device)
        dtype = _lib.VTTS_MEL_PCM16 if y.dtype == torch.int16 else _lib.VTTS_MEL_F32
        with torch.cuda.device(self.device):
            _lib.check(
                self.lib,
                self.lib.vtts_mel_forward(self._h, C.c_void_p(y.data_ptr()), dtype, N, S, lens_c, C.c_void_p(out.data_ptr()), T, None,
                                          C.c_void_p(stream.cuda_stream)),
            )
        return out
