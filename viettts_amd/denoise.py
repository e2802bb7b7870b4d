"""The vocoder-bias denoiser on the GPU: STFT-domain spectral subtraction in one fused pass (include/vtts_denoise.h,
viettts_amd/csrc/denoise.hip).  What published HiFi-GAN / WaveGlow inference scripts expose as ``--denoising-strength``: the magnitude spectrum
of the vocoder's output for an empty mel, times a strength, is subtracted from every frame's magnitude, the phase is kept, the result inverted.
With a bias measured from a stretch of room tone it is plain spectral subtraction for a recording.

    dn = Denoiser((1024, 1024, 256, "center"), device="cuda:0")  # or Denoiser(stft): binds that Stft's tables
    dn.bias_from_generator(generator)                            # the recipe's bias: frame 0 of |STFT(generator(zero mel))|; cached
    dn.bias_from_noise(room_tone)                                # ... or the mean magnitude over a noise recording's frames
    wav = dn(wav, lengths, strength=0.01)                        # [N, S] float32 / int16 -> [N, S] float32 (or int16 PCM); the fused kernel
    wav = dn.composed(wav, lengths, strength=0.01)               # Stft.forward, the gain as torch operators, Stft.inverse: the yardstick

    python -m viettts_amd.denoise --wav F.wav --noise-from A:B --strength S --output out.wav

No spectral floor, no over-subtraction factor, no Wiener or gated variant, no time-varying bias, no stereo, no streamed state, no gradients; and
no claim about audible quality, which needs a real checkpoint and listening.  The reference has no such stage.  No CPU fallback: the kernels
are the only implementation."""
from __future__ import annotations

import argparse
import ctypes as C
import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._handle import NativeHandle, ptr
from .audio import waveform_rows
from .stft import FRAMINGS, Stft

DEFAULT_CFG = (1024, 1024, 256, "center")
_DTYPES = {"f32": (torch.float32, _lib.VTTS_AUDIO_F32), "pcm16": (torch.int16, _lib.VTTS_AUDIO_PCM16)}


def check_strength(strength) -> float:
    s = float(strength)
    if not (math.isfinite(s) and s >= 0.0):
        raise ValueError(f"strength must be finite and not negative (got {strength!r})")
    return s


def _overlap(a: torch.Tensor, b: torch.Tensor) -> bool:
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


class Denoiser(NativeHandle):
    """``Denoiser(stft_or_cfg, bias=None, strength=0.01, device)``: one resolution and framing (an ``Stft`` whose tables are then shared, or
    ``(n_fft, win, hop, framing)``).  Every result of a row is bit for bit what the row gives alone, and bit for bit
    ``Stft.inverse(gain(Stft.forward(wav)))`` with the header's gain in IEEE float32.  Asynchronous on torch's current stream of the device.
    One ``Denoiser`` serves one call at a time."""

    def __init__(self, stft_or_cfg=DEFAULT_CFG, bias=None, strength: float = 0.01, device=None, lib_path=None):
        if isinstance(stft_or_cfg, Stft):
            stft = stft_or_cfg
            if device is not None and torch.device(device).type == "cuda" and torch.device(device).index not in (None, stft.device.index):
                raise ValueError(f"the Stft is on {stft.device}, the denoiser was asked for {device}")
            device = stft.device
            self._own_stft = False
        else:
            cfg = tuple(stft_or_cfg)
            if len(cfg) != 4 or cfg[3] not in FRAMINGS:
                raise ValueError(f"a denoiser is made from an Stft or from (n_fft, win, hop, framing), framing one of {sorted(FRAMINGS)} (got {stft_or_cfg!r})")
            device = "cuda:0" if device is None else device
            stft = None
            self._own_stft = True
        super().__init__("vtts_denoise", device, lib_path, "denoiser")
        if stft is None:
            stft = Stft(*cfg[:3], framing=cfg[3], device=self.device, lib_path=lib_path)
        self.stft = stft
        self.n_fft, self.win, self.hop, self.framing = stft.n_fft, stft.win, stft.hop, stft.framing
        self._create(C.byref(_lib.StftCfg(self.n_fft, self.win, self.hop, FRAMINGS[self.framing])))
        self.strength = check_strength(strength)
        self.bias: Optional[torch.Tensor] = None
        self._generator_bias: dict = {}
        if bias is not None:
            self.set_bias(bias)

    def close(self) -> None:
        super().close()
        if getattr(self, "_own_stft", False) and getattr(self, "stft", None) is not None:
            self.stft.close()
        self.bias = None

    @property
    def n_bins(self) -> int:
        return self.n_fft // 2 + 1

    def blocking(self) -> Tuple[int, int]:
        """(waves, run of output samples) of one workgroup: no result depends on them."""
        w, r = C.c_int(0), C.c_int(0)
        self._call("blocking", C.byref(w), C.byref(r))
        return int(w.value), int(r.value)

    def _tables(self) -> None:
        if self._blob is None:  # the Stft's tables, on the device once: the two handles read one blob
            self.stft._tables()
            self.adopt_packed(self.stft.packed_blob())

    # ---- the bias ---------------------------------------------------------------------------------
    def set_bias(self, bias) -> torch.Tensor:
        """``bias``: ``[n_fft / 2 + 1]`` non-negative finite values, a numpy array or a tensor."""
        b = bias.detach().to("cpu", torch.float64).numpy() if isinstance(bias, torch.Tensor) else np.asarray(bias, dtype=np.float64)
        if b.shape != (self.n_bins,):
            raise ValueError(f"bias must hold [{self.n_bins}] values, one per bin (got {tuple(b.shape)})")
        if not np.isfinite(b).all() or (b < 0).any():
            raise ValueError("bias must be finite and not negative: it is a magnitude spectrum")
        if isinstance(bias, torch.Tensor) and bias.device == self.device and bias.dtype == torch.float32:
            self.bias = bias.detach().contiguous().clone()
        else:
            self.bias = torch.from_numpy(b.astype(np.float32)).to(self.device)
        return self.bias

    def _magnitudes(self, spec: torch.Tensor) -> torch.Tensor:
        """The header's r of every bin: three torch operations and a root, each rounded on its own."""
        re, im = spec.real.contiguous(), spec.imag.contiguous()
        return torch.sqrt(re * re + im * im)

    def bias_from_generator(self, generator, frames: int = 88, fill: float = 0.0) -> torch.Tensor:
        """The published recipe: the generator on a ``[1, frames, num_mels]`` mel filled with ``fill``, and the magnitude of frame 0 of its
        ``Stft.forward``.  Cached per generator, ``frames`` and ``fill``."""
        key = (id(generator), int(frames), float(fill))
        b = self._generator_bias.get(key)
        if b is None:
            mel = torch.full((1, int(frames), generator.cfg.num_mels), float(fill), dtype=torch.float32, device=self.device)
            b = self._magnitudes(self.stft.forward(generator(mel))[:, :1])[0, 0].contiguous()
            self._generator_bias[key] = b
        self.bias = b
        return b

    def bias_from_noise(self, wav, lengths=None) -> torch.Tensor:
        """The mean of the magnitude over all frames of all rows of a noise recording, summed in float64 on the device."""
        x, lens, _ = waveform_rows(wav, lengths, self.device, "wav")
        r = self._magnitudes(self.stft.forward(x, lens))  # zero past a row's own frames
        n = sum(self.stft.num_frames(v) for v in lens)
        self.bias = (r.to(torch.float64).reshape(-1, self.n_bins).sum(dim=0) / float(n)).to(torch.float32)
        return self.bias

    # ---- the two paths ----------------------------------------------------------------------------
    def _args(self, wav, lengths, strength, out_dtype):
        if out_dtype not in _DTYPES:
            raise ValueError("out_dtype must be 'f32' or 'pcm16'")
        s = self.strength if strength is None else check_strength(strength)
        if self.bias is None:
            raise RuntimeError("the denoiser has no bias: set_bias(), bias_from_generator() or bias_from_noise() first")
        x, lens, lens_c = waveform_rows(wav, lengths, self.device, "wav")
        for n in set(lens):
            self.stft.num_frames(n)  # refuses what no row may be
        return x, lens, lens_c, s

    def fused(self, wav, lengths=None, strength: Optional[float] = None, out_dtype: str = "f32", out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``wav [N, S]`` (float32 or int16 PCM; a tensor on the device or a numpy array) -> ``[N, S]`` float32 (``"pcm16"``: int16) in one
        launch per 128 rows; zero past a row's own samples (an ``out`` of the caller's is left as it is there)."""
        x, lens, lens_c, s = self._args(wav, lengths, strength, out_dtype)
        N, S = x.shape
        tdt, code = _DTYPES[out_dtype]
        if out is None:
            out = torch.zeros((N, S), dtype=tdt, device=self.device)
        elif not isinstance(out, torch.Tensor) or out.shape != (N, S) or out.dtype != tdt or not out.is_contiguous() or out.device != self.device:
            raise ValueError(f"out must be a contiguous {tdt} [{N}, {S}] tensor on the denoiser's device")
        elif _overlap(out, x):
            raise ValueError("out must not overlap wav: a frame reads samples that another workgroup writes")
        self._tables()
        in_code = _lib.VTTS_AUDIO_PCM16 if x.dtype == torch.int16 else _lib.VTTS_AUDIO_F32
        self._on_stream("apply", ptr(x), in_code, N, S, lens_c, ptr(self.bias), C.c_float(s), ptr(out), code, S)
        return out

    __call__ = fused

    def composed(self, wav, lengths=None, strength: Optional[float] = None, out_dtype: str = "f32") -> torch.Tensor:
        """The same through ``Stft.forward``, the gain as torch operators on the device and ``Stft.inverse``: a spectrum in device memory and
        several launches.  The yardstick of tools/denoise_bench.py; within the float32 bound of ``__call__``, not bit for bit (torch's operators
        need not round as the header does)."""
        x, lens, _, s = self._args(wav, lengths, strength, out_dtype)
        spec = self.stft.forward(x, lens)
        re, im = spec.real.contiguous(), spec.imag.contiguous()
        r = torch.sqrt(re * re + im * im)
        m = torch.clamp(r - torch.tensor(s, dtype=torch.float32, device=self.device) * self.bias, min=0.0)
        d = r + 1e-16
        y = self.stft.inverse(torch.complex(m * (re / d), m * (im / d)), lens, out_dtype=out_dtype)
        return y if y.shape[1] == x.shape[1] else torch.nn.functional.pad(y, (0, x.shape[1] - y.shape[1]))


def generator_denoiser(generator, frames: int = 88) -> Denoiser:
    """The denoiser behind a generator, with that generator's own bias: one per generator, made at the first call."""
    dn = getattr(generator, "_denoiser", None)
    if dn is None:
        dn = generator._denoiser = Denoiser(DEFAULT_CFG, device=generator.device)
        dn.bias_from_generator(generator, frames)
    return dn


# ------------------------------------------------------------ the command lines ------------------------------------------------------------
def parse_noise_from(text: str) -> Tuple[float, float]:
    """``A:B`` in seconds, ``0 <= A < B``; ValueError with the reason otherwise."""
    parts = str(text).split(":")
    try:
        a, b = (float(p) for p in parts)
    except ValueError:
        raise ValueError(f"--noise-from takes A:B in seconds (got {text!r})") from None
    if not (math.isfinite(a) and math.isfinite(b)) or a < 0.0:
        raise ValueError(f"--noise-from takes A:B in seconds from the start of the input, A >= 0 (got {text!r})")
    if b <= a:
        raise ValueError(f"--noise-from {text}: B must be above A, the stretch of room tone has to hold samples")
    return a, b


def noise_span(span: Tuple[float, float], n_samples: int, rate: int) -> Tuple[int, int]:
    """The samples of ``A:B`` in an input of ``n_samples`` at ``rate``; ValueError where the stretch ends past the input."""
    lo, hi = int(round(span[0] * rate)), int(round(span[1] * rate))
    if hi > n_samples:
        raise ValueError(f"--noise-from {span[0]:g}:{span[1]:g} ends at sample {hi}, past the end of the input ({n_samples} samples at {rate} Hz)")
    return lo, hi


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="viettts_amd.denoise", description="spectral subtraction of a recording on the GPU, the bias from a stretch of its room tone")
    ap.add_argument("--wav", required=True, help="PCM16 mono .wav")
    ap.add_argument("--noise-from", required=True, metavar="A:B", help="seconds A..B of the input hold room tone only: the bias is their mean magnitude spectrum")
    ap.add_argument("--strength", type=float, default=1.0, help="the multiple of the bias that is subtracted from every frame's magnitude")
    ap.add_argument("--output", required=True)
    return ap


def main(argv=None) -> None:
    from . import wavio

    ap = build_parser()
    a = ap.parse_args(argv)
    try:  # argument errors before anything touches a device
        s = check_strength(a.strength)
        span = parse_noise_from(a.noise_from)
    except ValueError as e:
        ap.error(str(e))
    sr, pcm = wavio.read_wav(a.wav)
    try:
        lo, hi = noise_span(span, len(pcm), sr)
    except ValueError as e:
        ap.error(str(e))
    if not torch.cuda.is_available():
        raise RuntimeError("viettts_amd.denoise needs an MI355X visible to PyTorch-ROCm; there is no CPU path")
    dn = Denoiser(DEFAULT_CFG, device=torch.device("cuda", torch.cuda.current_device()))
    x = torch.from_numpy(np.ascontiguousarray(pcm.astype(np.int16))[None, :]).to(dn.device)
    dn.bias_from_noise(x[:, lo:hi].contiguous())
    out = dn(x, strength=s, out_dtype="pcm16")
    wavio.write_wav_pcm16(a.output, out[0].cpu().numpy(), sr)
    print(f"wrote {a.output}: {len(pcm)} samples, {s:g} x the mean magnitude of {hi - lo} samples of room tone subtracted")
    dn.close()


if __name__ == "__main__":
    main()
