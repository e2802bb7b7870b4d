"""Analysis -> resynthesis on the GPU: waveform -> log-mel (``MelFilter``, include/vtts_mel.h) -> waveform (``Generator``), the
standard check of a vocoder checkpoint, and the mel-domain distance between two waveforms (the quantity HiFi-GAN's mel loss is
computed on).  The mel stays in HBM between the two kernels' worlds: ``MelFilter`` writes the ``[N, T, 80]`` layout the generator reads.

    python -m viettts_amd.resynth --input in.wav --output out.wav [--dtype f32|bf16|bf16x3] [--output-rate 48000] [--f0] [--loudness -23 [--limit]] [--stoi] [--mrstft] [--mcd]
    python -m viettts_amd.resynth --input in.wav --output out.wav --vocoder griffinlim      # no checkpoint at all: viettts_amd.stft
    python -m viettts_amd.resynth --input in.wav --output out.wav --denoise 0.01            # the vocoder's own bias out of the result: viettts_amd.denoise
    python -m viettts_amd.resynth --input in.wav --output out.wav --denoise 1.0 --noise-from 0:0.5   # the input's room tone out of the input

reads PCM16 mono at any rate (anything but the model's 16 kHz is converted on the GPU first: ``viettts_amd.audio.Resampler``), writes
at the model's rate or, converted again, at ``--output-rate``; uses the same ``assets/hifigan/config.json`` and ``hk_hifi.pickle`` as ``mel2wave`` and raises
``FileNotFoundError`` without them.  ``--f0`` adds one line: F0 RMSE in cents, voicing error and gross error of the result against the input
(``viettts_amd.pitch``).
"""
from __future__ import annotations

import argparse
from typing import Optional

import numpy as np
import torch

from . import wavio
from .nat.config import FLAGS as NAT_FLAGS
from .nat.dsp import MelFilter

_FILTERS: dict = {}


def default_mel_filter(device) -> MelFilter:
    """The reference's configuration (vietTTS/nat/config.py:43-47): 16 kHz, n_fft 1024, 80 bands, 0 .. 8000 Hz; one per device."""
    device = torch.device(device)
    f = _FILTERS.get(device)
    if f is None:
        f = _FILTERS[device] = MelFilter(NAT_FLAGS.sample_rate, 1024, 80, 0.0, 8000, device=device)
    return f


def _on_device(wav, device) -> torch.Tensor:
    if isinstance(wav, torch.Tensor):
        return wav.to(device)
    wav = np.asarray(wav)
    if wav.dtype != np.int16:
        wav = wav.astype(np.float32, copy=False)
    return torch.from_numpy(np.ascontiguousarray(wav)).to(device)


def wav2mel(wav, lengths=None, mel_filter: Optional[MelFilter] = None, device=None, out=None) -> torch.Tensor:
    """``wav [N, S]`` (float32 or int16 PCM; torch tensor or numpy array) -> ``[N, T, 80]`` float32 log-mel on the device."""
    if mel_filter is None:
        if device is None:
            device = wav.device if isinstance(wav, torch.Tensor) and wav.is_cuda else torch.device("cuda", torch.cuda.current_device())
        mel_filter = default_mel_filter(device)
    return mel_filter(_on_device(wav, mel_filter.device), lengths=lengths, out=out)


def resynthesize(wav, generator, lengths=None, mel_filter: Optional[MelFilter] = None, in_rate: Optional[int] = None) -> torch.Tensor:
    """``generator.forward_ragged(MelFilter(wav), frames)``: ``[N, 256 * T]`` float32, row b's first ``256 * (lengths[b] // 256)``
    samples valid and the rest zero.  ``in_rate``: the rate of ``wav`` (and the unit of ``lengths``) when it is not the mel filter's;
    the rows are converted on the GPU first, and ``T`` counts frames of the converted rows."""
    mf = mel_filter or default_mel_filter(generator.device)
    y = _on_device(wav, generator.device)
    if in_rate is not None and int(in_rate) != mf.sample_rate:
        from .audio import resampler

        rs = resampler(int(in_rate), mf.sample_rate, generator.device)
        y = rs(y, lengths=lengths)
        if lengths is not None:
            lengths = rs.out_lengths(lengths)
    mel = mf(y, lengths=lengths)
    lens = [y.shape[1]] * y.shape[0] if lengths is None else [int(v) for v in lengths]
    return generator.forward_ragged(mel, [mf.num_frames(n) for n in lens])


def log_mel_l1(a, b, lengths=None, mel_filter: Optional[MelFilter] = None) -> float:
    """Mean absolute log-mel difference of two waveform batches of one shape (over each row's own frames)."""
    if mel_filter is None:
        dev = a.device if isinstance(a, torch.Tensor) and a.is_cuda else (b.device if isinstance(b, torch.Tensor) and b.is_cuda else torch.device("cuda", torch.cuda.current_device()))
        mel_filter = default_mel_filter(dev)
    ma = wav2mel(a, lengths, mel_filter)
    mb = wav2mel(b, lengths, mel_filter)
    if ma.shape != mb.shape:
        raise ValueError(f"the two batches differ in shape: {tuple(ma.shape)} vs {tuple(mb.shape)}")
    d = (ma - mb).abs()
    if lengths is None:
        return float(d.mean())
    frames = torch.tensor([mel_filter.num_frames(int(n)) for n in lengths], device=d.device)
    valid = (torch.arange(d.shape[1], device=d.device)[None, :] < frames[:, None]).to(d.dtype)
    return float((d.sum(dim=2) * valid).sum() / (valid.sum() * d.shape[2]))


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="wav -> log-mel -> wav through the HiFi-GAN generator on the GPU")
    ap.add_argument("--input", required=True, help="PCM16 mono .wav; any rate but the model's is converted on the GPU")
    ap.add_argument("--output", required=True)
    ap.add_argument("--dtype", default="f32", choices=("f32", "bf16", "bf16x3"))
    ap.add_argument("--output-rate", type=int, default=None, help="convert the result to this rate on the GPU (default: the model's rate)")
    ap.add_argument("--f0", action="store_true", help="also print F0 RMSE (cents), voicing error and gross error of the result against the input (viettts_amd.pitch)")
    ap.add_argument("--loudness", type=float, default=None, help="write the result at this BS.1770 integrated loudness in LUFS (viettts_amd.loudness); the figures printed are of the result before the gain")
    ap.add_argument("--limit", action="store_true", help="with --loudness: the full gain to the target and a look-ahead limiter under -1 dBTP (viettts_amd.limiter) in place of the sample-peak cap")
    ap.add_argument("--stoi", action="store_true", help="also print STOI and ESTOI of the result against the input at 10 kHz (viettts_amd.stoi); NaN below 30 analysis frames")
    ap.add_argument("--mrstft", action="store_true", help="also print the multi-resolution STFT distance and the log-spectral distance of the result against the input (viettts_amd.spectral); needs 1025 samples")
    ap.add_argument("--mcd", action="store_true", help="also print the mel-cepstral distortion in dB of the result against the input, frame by frame (viettts_amd.mcd: 13 log-mel cepstra, c0 left out)")
    ap.add_argument("--vocoder", default="hifigan", choices=("hifigan", "griffinlim"), help="griffinlim: log-mel -> wav by Griffin-Lim on the GPU (viettts_amd.stft): "
                    "no checkpoint is opened; --dtype does not apply")
    ap.add_argument("--denoise", type=float, default=None, metavar="S", help="subtract S x a bias spectrum (viettts_amd.denoise): the vocoder's own, from its output "
                    "for an empty mel, out of the result; or with --noise-from the input's room tone out of the input, ahead of the mel front end")
    ap.add_argument("--noise-from", default=None, metavar="A:B", help="with --denoise: seconds A..B of the input hold room tone only, the bias is their mean magnitude spectrum")
    return ap


class _Device:
    """What main() needs of a generator when there is none: the device."""

    def __init__(self, device):
        self.device = device


def main(argv=None) -> None:
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.limit and a.loudness is None:
        raise SystemExit("--limit needs --loudness")
    span = None
    if a.noise_from is not None and a.denoise is None:
        ap.error("--noise-from belongs to --denoise S")
    if a.denoise is not None:  # argument errors before anything touches a device
        from .denoise import check_strength, noise_span, parse_noise_from

        try:
            check_strength(a.denoise)
            span = None if a.noise_from is None else parse_noise_from(a.noise_from)
        except ValueError as e:
            ap.error(str(e).replace("strength", "--denoise"))
        if span is None and a.vocoder == "griffinlim":
            ap.error("--vocoder griffinlim with --denoise and no --noise-from: there is no vocoder to take a bias from")
        if span is not None:
            try:
                sr0, pcm0 = wavio.read_wav(a.input)  # (host work: the stretch has to lie inside the input)
                noise_span(span, len(pcm0), sr0)
            except ValueError as e:
                ap.error(str(e))
    if a.vocoder == "griffinlim":
        if a.dtype != "f32":
            ap.error("--vocoder griffinlim with --dtype: the engine's precision belongs to the HiFi-GAN generator")
        if not torch.cuda.is_available():
            raise RuntimeError("viettts_amd.resynth needs an MI355X visible to PyTorch-ROCm; there is no CPU path")
        gen = _Device(torch.device("cuda", torch.cuda.current_device()))
    else:
        from .hifigan.mel2wave import _generator

        gen = _generator(a.dtype)  # FileNotFoundError without config / checkpoint, before the input is touched
    sr, pcm = wavio.read_wav(a.input)
    model_rate = NAT_FLAGS.sample_rate
    y = _on_device(pcm.astype(np.int16)[None, :], gen.device)
    if sr != model_rate:
        from .audio import resampler

        y = resampler(sr, model_rate, gen.device)(y)
    if span is not None:  # the input's room tone out of the input
        from .denoise import DEFAULT_CFG, Denoiser

        dn = Denoiser(DEFAULT_CFG, device=gen.device)
        lo, hi = (int(round(t * model_rate)) for t in span)
        dn.bias_from_noise(y[:, lo:min(hi, y.shape[1])].contiguous())
        y = dn(y, strength=a.denoise, out_dtype="pcm16" if y.dtype == torch.int16 else "f32")
        dn.close()
    if a.vocoder == "griffinlim":
        from .stft import mel2wave_griffinlim

        wav = mel2wave_griffinlim(wav2mel(y, device=gen.device))
    else:
        wav = resynthesize(y, gen)
        if a.denoise is not None and span is None:  # the vocoder's own bias out of its output
            from .denoise import generator_denoiser

            wav = generator_denoiser(gen)(wav, lengths=[256 * (y.shape[1] // 256)], strength=a.denoise)
    n = 256 * (y.shape[1] // 256)
    written = wav
    if a.loudness is not None and a.limit:
        from .limiter import default_limiter

        written, res = default_limiter(gen.device, model_rate).normalize(wav, lengths=[n], target=a.loudness)
        print(f"loudness: gain {20.0 * np.log10(float(res.gains[0])):+.2f} dB to {a.loudness:.1f} LUFS, limited by at most "
              f"{-20.0 * np.log10(float(res.min_gain[0])):.2f} dB under -1.0 dBTP")
    elif a.loudness is not None:
        from .loudness import default_meter

        written, gains = default_meter(gen.device, model_rate).normalize(wav, lengths=[n], target=a.loudness)
        print(f"loudness: gain {20.0 * np.log10(float(gains[0])):+.2f} dB to {a.loudness:.1f} LUFS")
    if a.output_rate is None or a.output_rate == model_rate:
        wavio.write_wav(a.output, written[0, :n].cpu().numpy(), model_rate)
    else:
        from .audio import resampler

        out = resampler(model_rate, a.output_rate, gen.device)(written[0, :n].contiguous(), out_dtype="pcm16")
        wavio.write_wav_pcm16(a.output, out.cpu().numpy(), a.output_rate)
    print(f"wrote {a.output}: {n} samples, log-mel L1 against the input {log_mel_l1(wav[:, :n], y[:, :n].contiguous()):.4f}")
    if a.f0:
        from .pitch import default_tracker, format_metrics, wav_f0_metrics

        print(format_metrics(wav_f0_metrics(wav[:, :n].contiguous(), y[:, :n].contiguous(), tracker=default_tracker(gen.device, model_rate))))
    if a.stoi:
        from .stoi import format_result, wav_stoi

        print(format_result(wav_stoi(y[:, :n].contiguous(), wav[:, :n].contiguous(), rate=model_rate)))
    if a.mrstft:
        from .spectral import format_result as format_mrstft, wav_mrstft

        print(format_mrstft(wav_mrstft(y[:, :n].contiguous(), wav[:, :n].contiguous())))
    if a.mcd:
        from .mcd import wav_mcd

        print(f"MCD {float(wav_mcd(y[:, :n].contiguous(), wav[:, :n].contiguous())[0]):.3f} dB of the result against the input ({n // 256} frames, 13 log-mel cepstra)")


if __name__ == "__main__":
    main()
