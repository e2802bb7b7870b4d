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
from .._handle import NativeHandle, ptr
from ..audio import waveform_rows


class MelFilter(NativeHandle):
    """``MelFilter(sample_rate, n_fft, n_mels, fmin, fmax)(y)`` — ``y [N, S]`` float32 or int16 PCM -> ``[N, T, n_mels]`` float32.

    hop = n_fft / 4 and window = n_fft, as in the reference's ``__call__``.  One MelFilter serves one call at a time on one device.
    """

    def __init__(self, sample_rate: int, n_fft: int, n_mels: int, fmin=0.0, fmax=8000, device="cuda:0", lib_path=None):
        super().__init__("vtts_mel", device, lib_path, "filter")
        self.sample_rate, self.n_fft, self.n_mels, self.hop = int(sample_rate), int(n_fft), int(n_mels), int(n_fft) // 4
        self.frames_per_workgroup = _lib.MEL_FRAMES_PER_BLOCK
        self._create(C.byref(_lib.MelCfg(self.sample_rate, self.n_fft, self.hop, self.n_mels, float(fmin), float(fmax))))

    @property
    def melfb(self) -> np.ndarray:
        """The ``[n_mels, n_fft / 2 + 1]`` float32 basis (the reference's attribute of the same name)."""
        fb = np.empty((self.n_mels, self.n_fft // 2 + 1), dtype=np.float32)
        self._call("filterbank", fb.ctypes.data_as(C.POINTER(C.c_float)))
        return fb

    def num_frames(self, n_samples: int) -> int:
        n = C.c_int64(0)
        self._call("num_frames", int(n_samples), C.byref(n))
        return int(n.value)

    def __call__(self, y, lengths=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Asynchronous on torch's current stream of the device.  ``lengths``: samples per row (ints, host); row b is reflected at its
        own end and frames past its own count hold ``log(1e-5)``."""
        y, lens, lens_c = waveform_rows(y, lengths, self.device, "y")
        N, S = y.shape
        T = max(self.num_frames(n) for n in set(lens))  # refuses rows too short to reflect
        shape = (N, T, self.n_mels)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        elif out.shape != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != self.device:
            raise ValueError("out must be a contiguous float32 [N, T, n_mels] tensor on the filter's device")
        if self._blob is None:  # the tables go to the device once, at the first call
            self._pack()
        dtype = _lib.VTTS_MEL_PCM16 if y.dtype == torch.int16 else _lib.VTTS_MEL_F32
        self._on_stream("forward", ptr(y), dtype, N, S, lens_c, ptr(out), T, None)
        return out
