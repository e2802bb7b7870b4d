"""The complex short-time Fourier transform on the GPU in both directions, and Griffin-Lim on top of it: a spectrogram back to samples without a
vocoder checkpoint (include/vtts_stft.h, viettts_amd/csrc/stft.hip).

    st = Stft(1024, 1024, 256, framing="mel", device="cuda:0")  # one resolution: n_fft, win, hop; framing "center" (torch.stft's) or "mel"
    spec = st.forward(wav, lengths)                             # [N, S] float32 / int16 -> [N, T, n_fft / 2 + 1] complex64
    wav = st.inverse(spec, lengths)                             # ... and back: torch.istft's contract, [N, S] float32 (or int16 PCM)
    spec = st.project(wav, mag, tprev, lengths, momentum=0.99)  # Griffin-Lim's update; tprev is read and overwritten
    wav = GriffinLim(st, n_iter=32)(mag)                        # [N, T, n_fft / 2 + 1] magnitudes -> [N, S]
    wav = mel2wave_griffinlim(mel)                              # a model mel [N, T, 80] -> [N, 256 T], sample-aligned with the generator's output

    python -m viettts_amd.stft --mel-file m.npy --output out.wav [--n-iter 32] [--momentum 0.99] [--seed 0]

Hann windows and the four transform lengths of ``SpectralMeter`` only; no gradients, no streamed inverse.  ``mel_to_linear`` is the
pseudo-inverse of the mel basis (a torch matmul: plumbing, not a kernel), not a non-negative least-squares fit.  Nothing here claims
Griffin-Lim's audio quality against HiFi-GAN's.  The reference has no such stage; nothing here is re-exported under ``vietTTS/``.  No CPU
fallback: the kernels are the only implementation.
"""
from __future__ import annotations

import argparse
import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._handle import NativeHandle, ptr
from .audio import waveform_rows

FRAMINGS = {"center": _lib.VTTS_STFT_CENTER, "mel": _lib.VTTS_STFT_MEL}
MODEL_RESOLUTION = (1024, 1024, 256)  # the mel front end's n_fft, win, hop


class Stft(NativeHandle):
    """``Stft(n_fft, win, hop, framing="center", device)``: one resolution of the complex STFT.  Every result of a row is bit for bit what the
    row gives alone.  Asynchronous on torch's current stream of the device.  One ``Stft`` serves one call at a time."""

    def __init__(self, n_fft: int = 1024, win: int = 1024, hop: int = 256, framing: str = "center", device="cuda:0", lib_path=None):
        super().__init__("vtts_stft", device, lib_path, "transform")
        if framing not in FRAMINGS:
            raise ValueError(f"framing must be one of {sorted(FRAMINGS)} (got {framing!r})")
        self.n_fft, self.win, self.hop, self.framing = int(n_fft), int(win), int(hop), framing
        self._create(C.byref(_lib.StftCfg(self.n_fft, self.win, self.hop, FRAMINGS[framing])))

    @property
    def n_bins(self) -> int:
        return self.n_fft // 2 + 1

    @property
    def pad(self) -> int:
        return (self.n_fft - self.hop) // 2 if self.framing == "mel" else self.n_fft // 2

    def window(self) -> np.ndarray:
        """The ``n_fft`` float32 window values the kernels use."""
        out = np.empty(self.n_fft, dtype=np.float32)
        self._call("window", out.ctypes.data_as(C.POINTER(C.c_float)))
        return out

    def blocking(self):
        """(frames per workgroup of forward / project, waves and run of samples per workgroup of inverse): no result depends on them."""
        f, w, r = C.c_int(0), C.c_int(0), C.c_int(0)
        self._call("blocking", C.byref(f), C.byref(w), C.byref(r))
        return int(f.value), int(w.value), int(r.value)

    def num_frames(self, n_samples: int) -> int:
        n = C.c_int64(0)
        self._call("num_frames", int(n_samples), C.byref(n))
        return int(n.value)

    def num_samples(self, frames: int) -> int:
        n = C.c_int64(0)
        self._call("num_samples", int(frames), C.byref(n))
        return int(n.value)

    def min_envelope(self, n_samples: int) -> float:
        e = C.c_double(0.0)
        self._call("min_envelope", int(n_samples), C.byref(e))
        return float(e.value)

    def _tables(self) -> None:
        if self._blob is None:  # the tables go to the device once, at the first call
            self._pack()

    def _spec_like(self, spec, name: str, dtype, N: int, T: int) -> torch.Tensor:
        if not isinstance(spec, torch.Tensor) or spec.device != self.device or spec.dtype != dtype or spec.dim() != 3 or spec.shape[2] != self.n_bins:
            raise ValueError(f"{name} must be a {dtype} [N, T, {self.n_bins}] tensor on {self.device}")
        if N and (spec.shape[0] != N or spec.shape[1] < T):
            raise ValueError(f"{name} is {tuple(spec.shape)}: {N} rows of at least {T} frames are needed")
        return spec if spec.is_contiguous() else spec.contiguous()

    def forward(self, wav, lengths=None) -> torch.Tensor:
        """``wav [N, S]`` (float32 or int16 PCM; a tensor on the device or a numpy array) -> ``[N, T, n_bins]`` complex64, zero past a row's
        own frames."""
        x, lens, lens_c = waveform_rows(wav, lengths, self.device, "wav")
        N, S = x.shape
        T = max(self.num_frames(n) for n in set(lens))  # refuses what no row may be
        self._tables()
        spec = torch.zeros((N, T, self.n_bins), dtype=torch.complex64, device=self.device)
        dtype = _lib.VTTS_AUDIO_PCM16 if x.dtype == torch.int16 else _lib.VTTS_AUDIO_F32
        self._on_stream("forward", ptr(x), dtype, N, S, lens_c, ptr(spec), T)
        return spec

    def inverse(self, spec, lengths=None, out_dtype: str = "f32", out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``spec [N, T, n_bins]`` complex64 -> ``[N, S]`` float32 (``"pcm16"``: int16).  ``lengths``: SAMPLES per row; without them every
        row has ``num_samples(T)``.  Zero past a row's own samples.  Raises ``VttsError`` where the window and hop have no inverse (NOLA)."""
        if out_dtype not in ("f32", "pcm16"):
            raise ValueError("out_dtype must be 'f32' or 'pcm16'")
        spec = self._spec_like(spec, "spec", torch.complex64, 0, 0)
        N, T = int(spec.shape[0]), int(spec.shape[1])
        if lengths is None:
            lens, lens_c, S = None, None, self.num_samples(T)
        else:
            lens = [int(v) for v in (lengths.tolist() if isinstance(lengths, (torch.Tensor, np.ndarray)) else lengths)]
            if len(lens) != N:
                raise ValueError("lengths must hold one sample count per row")
            lens_c, S = (C.c_int32 * N)(*lens), max(lens)
        self._tables()
        tdt = torch.int16 if out_dtype == "pcm16" else torch.float32
        if out is None:
            out = torch.zeros((N, S), dtype=tdt, device=self.device)
        elif out.shape != (N, S) or out.dtype != tdt or not out.is_contiguous() or out.device != self.device:
            raise ValueError(f"out must be a contiguous {tdt} [{N}, {S}] tensor on the transform's device")
        self._on_stream("inverse", ptr(spec), N, T, lens_c, ptr(out), _lib.VTTS_AUDIO_PCM16 if out_dtype == "pcm16" else _lib.VTTS_AUDIO_F32, S)
        return out

    def project(self, wav, mag, tprev, lengths=None, momentum: float = 0.99, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Griffin-Lim's update in one launch: ``c = forward(wav)``, ``a = c - momentum / (1 + momentum) * tprev``, returns
        ``mag * a / (|a| + 1e-16)`` and leaves ``c`` in ``tprev`` (``[N, T, n_bins]`` complex64, zeros before the first iteration)."""
        x, lens, lens_c = waveform_rows(wav, lengths, self.device, "wav")
        N, S = x.shape
        T = max(self.num_frames(n) for n in set(lens))
        mag = self._spec_like(mag, "mag", torch.float32, N, T)
        if not isinstance(tprev, torch.Tensor) or not tprev.is_contiguous():
            raise ValueError("tprev must be a contiguous tensor (it is overwritten)")
        self._spec_like(tprev, "tprev", torch.complex64, N, T)
        if out is None:
            out = torch.zeros_like(tprev)
        elif out.shape != tprev.shape or out.dtype != torch.complex64 or not out.is_contiguous() or out.device != self.device or out.data_ptr() == tprev.data_ptr():
            raise ValueError("out must be a contiguous complex64 tensor of tprev's shape on the transform's device, and not tprev")
        if mag.shape[1] != tprev.shape[1]:
            raise ValueError(f"mag has {mag.shape[1]} frames per row, tprev {tprev.shape[1]}")
        self._tables()
        dtype = _lib.VTTS_AUDIO_PCM16 if x.dtype == torch.int16 else _lib.VTTS_AUDIO_F32
        self._on_stream("project", ptr(x), dtype, N, S, lens_c, ptr(mag), ptr(tprev), ptr(out), int(tprev.shape[1]), C.c_float(momentum))
        return out


def random_phases(shape, device, seed: int = 0) -> torch.Tensor:
    """Unit complex numbers of uniform phase from a seeded torch generator on the device."""
    g = torch.Generator(device=device)
    g.manual_seed(int(seed))
    ph = torch.rand(tuple(shape), generator=g, device=device, dtype=torch.float32) * (2.0 * np.pi)
    return torch.polar(torch.ones_like(ph), ph)


class GriffinLim:
    """``GriffinLim(stft, n_iter=32, momentum=0.99)(mag, lengths=None, init=None, seed=0)``: ``mag [N, T, n_bins]`` float32 -> ``[N, S]``
    float32 by torchaudio's fast Griffin-Lim: ``n_iter`` x (inverse, project) and a final inverse, ``2 n_iter + 1`` launches per 128 rows.
    ``lengths``: samples per row (default ``stft.num_samples(T)``); ``init``: complex unit phases of ``mag``'s shape (default: uniform, from
    ``seed``)."""

    def __init__(self, stft: Stft, n_iter: int = 32, momentum: float = 0.99):
        if n_iter < 0:
            raise ValueError("n_iter must not be negative")
        if not 0.0 <= momentum < 1.0:
            raise ValueError("momentum must be in [0, 1)")
        self.stft, self.n_iter, self.momentum = stft, int(n_iter), float(momentum)

    def __call__(self, mag, lengths=None, init=None, seed: int = 0) -> torch.Tensor:
        st = self.stft
        if isinstance(mag, np.ndarray):
            mag = torch.from_numpy(np.ascontiguousarray(mag, dtype=np.float32)).to(st.device)
        mag = st._spec_like(mag, "mag", torch.float32, 0, 0)
        if init is None:
            init = random_phases(mag.shape, st.device, seed)
        elif not isinstance(init, torch.Tensor) or init.shape != mag.shape or init.dtype != torch.complex64 or init.device != st.device:
            raise ValueError("init must be a complex64 tensor of mag's shape on the transform's device")
        spec = (mag * init).contiguous()
        other, tprev = torch.zeros_like(spec), torch.zeros_like(spec)
        for _ in range(self.n_iter):
            wav = st.inverse(spec, lengths)
            st.project(wav, mag, tprev, lengths, self.momentum, out=other)
            spec, other = other, spec
        return st.inverse(spec, lengths)


def mel_to_linear(logmel, mel_filter) -> torch.Tensor:
    """``clamp(exp(logmel) @ pinv(fb).T, min=0)``: a log-mel ``[N, T, n_mels]`` -> linear magnitudes ``[N, T, n_fft / 2 + 1]``.  The
    pseudo-inverse of the filter's basis is computed once per filter, on the host in float64."""
    pinv = getattr(mel_filter, "_pinv_t", None)
    if pinv is None:
        pinv = torch.from_numpy(np.linalg.pinv(mel_filter.melfb.astype(np.float64)).T.astype(np.float32).copy()).to(mel_filter.device)  # [n_mels, n_bins]
        mel_filter._pinv_t = pinv
    if isinstance(logmel, np.ndarray):
        logmel = torch.from_numpy(np.ascontiguousarray(logmel, dtype=np.float32))
    logmel = logmel.to(mel_filter.device, torch.float32)
    if logmel.dim() != 3 or logmel.shape[2] != pinv.shape[0]:
        raise ValueError(f"logmel must be [N, T, {pinv.shape[0]}], got {tuple(logmel.shape)}")
    return torch.clamp(torch.exp(logmel) @ pinv, min=0.0).contiguous()


_MODEL_STFT: dict = {}


def model_stft(device) -> Stft:
    """The mel front end's resolution and framing (1024 / 1024 / 256, "mel"), one per device."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    st = _MODEL_STFT.get(device)
    if st is None:
        st = _MODEL_STFT[device] = Stft(*MODEL_RESOLUTION, framing="mel", device=device)
    return st


def mel2wave_griffinlim(mel, n_iter: int = 32, momentum: float = 0.99, seed: int = 0, device=None, mel_filter=None) -> torch.Tensor:
    """A model mel ``[N, T, 80]`` (or ``[T, 80]``) -> ``[N, 256 T]`` float32 on the device, with no checkpoint: sample-aligned with what the
    generator gives for the same mel.  Each row is what the row gives alone (under its own initial phases)."""
    from .resynth import default_mel_filter

    if device is None:
        device = mel.device if isinstance(mel, torch.Tensor) and mel.is_cuda else torch.device("cuda", torch.cuda.current_device())
    mf = mel_filter or default_mel_filter(device)
    if getattr(mel, "ndim", 3) == 2:
        mel = mel[None]
    mag = mel_to_linear(mel, mf)
    st = model_stft(mf.device)
    init = torch.stack([random_phases(mag.shape[1:], st.device, seed) for _ in range(mag.shape[0])])  # a row's phases do not depend on the batch
    return GriffinLim(st, n_iter, momentum)(mag, init=init)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="viettts_amd.stft", description="a saved log-mel -> wav by Griffin-Lim on the GPU, with no vocoder checkpoint")
    ap.add_argument("--mel-file", required=True, help=".npy log-mel, [T, 80] or [1, T, 80]")
    ap.add_argument("--output", required=True)
    ap.add_argument("--n-iter", type=int, default=32)
    ap.add_argument("--momentum", type=float, default=0.99)
    ap.add_argument("--seed", type=int, default=0)
    return ap


def main(argv=None) -> None:
    from . import wavio
    from .nat.config import FLAGS

    ap = build_parser()
    a = ap.parse_args(argv)
    if a.n_iter < 0:
        ap.error("--n-iter must not be negative")
    if not 0.0 <= a.momentum < 1.0:
        ap.error("--momentum must be in [0, 1)")
    mel = np.load(a.mel_file).astype(np.float32)
    mel = mel[None] if mel.ndim == 2 else mel
    if mel.ndim != 3 or mel.shape[0] != 1 or mel.shape[2] != 80:
        raise ValueError(f"--mel-file must hold [T, 80] or [1, T, 80], got {mel.shape}")
    if not torch.cuda.is_available():
        raise RuntimeError("viettts_amd.stft needs an MI355X visible to PyTorch-ROCm; there is no CPU path")
    wav = mel2wave_griffinlim(mel, a.n_iter, a.momentum, a.seed)
    wavio.write_wav(a.output, wav[0].cpu().numpy(), FLAGS.sample_rate)
    print(f"wrote {a.output}: {wav.shape[1]} samples from {mel.shape[1]} frames, {a.n_iter} Griffin-Lim iterations")


if __name__ == "__main__":
    main()
