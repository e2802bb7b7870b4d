"""Score a vocoder checkpoint with the objective HiFi-GAN optimises, on the GPU: wav -> log-mel (``MelFilter``) -> generator ->
(y, y_hat) through the discriminators (``Discriminators``, include/vtts_disc.h), segment by segment.

    python -m viettts_amd.vocoder_eval --wav a.wav b.wav --generator hk_hifi.pickle --discriminator do_02500000 [--segment 8192] [--f0] [--loudness] [--stoi] [--mrstft] [--mcd]

prints, averaged over the segments, the adversarial term (generator_loss of MPD + MSD), the feature-matching term (feature_loss of
MPD + MSD), the log-mel L1 and their HiFi-GAN sum ``adv + fm + 45 * mel``.  Reads PCM16 mono (any rate but the model's is converted
on the GPU first: ``viettts_amd.audio.Resampler``), the
generator as ``mel2wave`` reads it (``assets/hifigan/config.json`` + a Haiku pickle) and upstream's ``do_*`` file; raises
``FileNotFoundError`` without them, before any input is touched.  Forward only: nothing is trained.
``--f0`` adds one line: F0 RMSE in cents, voicing error and gross error of ``y_hat`` against ``y`` (``viettts_amd.pitch``), averaged over the passes.
``--stoi`` adds one line: STOI and ESTOI of ``y_hat`` against ``y`` (``viettts_amd.stoi``), each pass's segments laid end to end as one row.
``--mrstft`` adds one line: the multi-resolution STFT distance (spectral convergence + log-magnitude L1 at Parallel WaveGAN's three resolutions)
and the log-spectral distance of ``y_hat`` against ``y`` (``viettts_amd.spectral``), per segment, averaged.
``--mcd`` adds one line: the mel-cepstral distortion in dB of ``y_hat`` against ``y``, frame by frame (``viettts_amd.mcd``), per segment, averaged.
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

from . import wavio
from .nat.config import FLAGS as NAT_FLAGS

MEL_WEIGHT = 45.0
F0_KEYS = ("f0_rmse_cents", "voicing_error", "gross_error")  # what score_segments adds with a tracker
LOUDNESS_KEYS = ("lufs_y", "lufs_y_hat")  # ... and with a meter
STOI_KEYS = ("stoi", "estoi")  # ... and with a stoi_meter
SPECTRAL_KEYS = ("mrstft", "sc", "logmag", "lsd")  # ... and with spectral
MCD_KEYS = ("mcd",)  # ... and with mcd


def score_segments(y: torch.Tensor, generator, discriminators, mel_filter=None, tracker=None, meter=None, stoi_meter=None, rate=None, spectral=None, mcd=None) -> dict:
    """``y [B, S]`` float32 on the device, S a multiple of 256: one generator pass, one 2 B-row discriminator pass, one reduction.
    With ``tracker`` (a ``viettts_amd.pitch.PitchTracker``) the result also holds ``f0_rmse_cents``, ``voicing_error`` and ``gross_error`` of
    ``y_hat`` against ``y`` (``pitch.f0_metrics``); with ``meter`` (a ``viettts_amd.loudness.LoudnessMeter``) ``lufs_y`` and ``lufs_y_hat``: the
    BS.1770 integrated loudness of the pass's segments laid end to end (nan when no block passes the gates); with ``stoi_meter`` (a
    ``viettts_amd.stoi.StoiMeter``) ``stoi`` and ``estoi`` of ``y_hat`` against ``y``, likewise laid end to end as one row at ``rate`` (the
    model's without it) and converted to 10 kHz on the device (nan when the row holds no 30-frame segment); with ``spectral`` (a
    ``viettts_amd.spectral.MultiResolutionStft``) ``mrstft``, ``sc``, ``logmag`` and ``lsd`` of ``y_hat`` against ``y``: each segment is a row
    of its own (it must hold the largest ``n_fft / 2 + 1`` samples), the figures are the means over the segments of the means over the
    resolutions; with ``mcd`` (a ``viettts_amd.mcd.Mcd``) ``mcd``: the aligned mel-cepstral distortion in dB of ``y_hat`` against ``y``, the
    mean over the segments."""
    from .resynth import default_mel_filter, log_mel_l1

    mf = mel_filter or default_mel_filter(generator.device)
    y_hat = generator(mf(y))[:, : y.shape[1]].contiguous()
    L = discriminators.losses(y, y_hat)
    mel = log_mel_l1(y_hat, y, mel_filter=mf)
    out = {"adv": L.gen, "fm": L.feature, "mel": mel, "total": L.gen + L.feature + MEL_WEIGHT * mel, "disc": L.disc}
    if tracker is not None:
        from .pitch import wav_f0_metrics

        m = wav_f0_metrics(y_hat, y, tracker=tracker)
        out.update({k: m[k] for k in F0_KEYS})
    if meter is not None:  # one row: a segment alone may be shorter than a 400 ms block
        for k, w in zip(LOUDNESS_KEYS, (y, y_hat)):
            v = float(meter(w.reshape(1, -1)).integrated[0])
            out[k] = v if v > float("-inf") else float("nan")
    if stoi_meter is not None:  # one row: a segment alone may hold fewer than 30 frames
        from .stoi import wav_stoi

        r = wav_stoi(y.reshape(1, -1), y_hat.reshape(1, -1), rate=int(rate or NAT_FLAGS.sample_rate), meter=stoi_meter)
        out.update(stoi=float(r.stoi[0]), estoi=float(r.estoi[0]))
    if spectral is not None:  # per segment: a segment is its own utterance to the reflection padding
        r = spectral(y, y_hat)
        k = float(len(r.per_resolution))
        out.update(mrstft=float(r.mrstft.mean()), sc=float(sum(p.sc for p in r.per_resolution).mean() / k),
                   logmag=float(sum(p.logmag for p in r.per_resolution).mean() / k), lsd=float(r.lsd.mean()))
    if mcd is not None:
        out.update(mcd=float(mcd.aligned(mf(y_hat), mf(y)).mean()))
    return out


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="adversarial, feature-matching and mel terms of a HiFi-GAN checkpoint on the GPU")
    ap.add_argument("--wav", nargs="+", required=True, help="PCM16 mono .wav files; any rate but the model's is converted on the GPU")
    ap.add_argument("--generator", required=True, help="the generator's Haiku pickle (hk_hifi.pickle)")
    ap.add_argument("--discriminator", required=True, help="upstream's do_* checkpoint (keys mpd, msd)")
    ap.add_argument("--config", default="assets/hifigan/config.json")
    ap.add_argument("--segment", type=int, default=8192, help="samples per scored segment (a multiple of 256)")
    ap.add_argument("--batch", type=int, default=16, help="segments per pass")
    ap.add_argument("--f0", action="store_true", help="also print F0 RMSE (cents), voicing error and gross error of y_hat against y (viettts_amd.pitch)")
    ap.add_argument("--loudness", action="store_true", help="also print the BS.1770 integrated loudness of y and y_hat and their difference (viettts_amd.loudness)")
    ap.add_argument("--stoi", action="store_true", help="also print STOI and ESTOI of y_hat against y at 10 kHz (viettts_amd.stoi), each pass's segments laid end to end as "
                    "one row: the default --segment 8192 is 5120 samples or 38 frames at 10 kHz, and a pass whose row holds fewer than 30 frames "
                    "after its silent ones are dropped (one segment much shorter than 8192) gives NaN and is left out of the mean")
    ap.add_argument("--mrstft", action="store_true", help="also print the multi-resolution STFT distance (spectral convergence + log-magnitude L1 at n_fft 1024, "
                    "2048 and 512) and the log-spectral distance of y_hat against y (viettts_amd.spectral), per segment: --segment must be at least 1025")
    ap.add_argument("--mcd", action="store_true", help="also print the mel-cepstral distortion in dB of y_hat against y, frame by frame (viettts_amd.mcd: 13 log-mel "
                    "cepstra, c0 left out), per segment")
    return ap


def main(argv=None) -> None:
    a = build_parser().parse_args(argv)
    for path, what in ((a.generator, "generator checkpoint"), (a.discriminator, "discriminator checkpoint"), (a.config, "generator config")):
        if not os.path.exists(path):
            raise FileNotFoundError(f"{what} {path} not found")
    if a.segment < 512 or a.segment % 256:
        raise ValueError("--segment must be a multiple of 256, at least 512")
    if not torch.cuda.is_available():
        raise RuntimeError("vocoder_eval needs an MI355X visible to PyTorch-ROCm; there is no CPU path")
    from .hifigan.config import HifiganConfig
    from .hifigan.discriminators import Discriminators
    from .hifigan.generator import Generator
    from .hifigan.weights import load_haiku_pickle

    dev = torch.device("cuda", torch.cuda.current_device())
    gen = Generator(HifiganConfig.from_json(a.config), device=dev)
    gen.load_params(load_haiku_pickle(a.generator))
    disc = Discriminators.from_checkpoint(a.discriminator, device=dev)
    segs = []
    for path in a.wav:
        sr, pcm = wavio.read_wav(path)
        if sr != NAT_FLAGS.sample_rate:
            from .audio import resampler

            x = resampler(sr, NAT_FLAGS.sample_rate, dev)(pcm.astype(np.int16)).cpu().numpy()
        else:
            x = pcm.astype(np.float32) / 32768.0
        segs += [x[i : i + a.segment] for i in range(0, len(x) - a.segment + 1, a.segment)]
    if not segs:
        raise ValueError(f"no input holds a whole segment of {a.segment} samples")
    trk = None
    if a.f0:
        from .pitch import default_tracker

        trk = default_tracker(dev, NAT_FLAGS.sample_rate)
    meter = None
    if a.loudness:
        from .loudness import default_meter

        meter = default_meter(dev, NAT_FLAGS.sample_rate)
    stoi_meter = None
    if a.stoi:
        from .stoi import default_stoi_meter

        stoi_meter = default_stoi_meter(dev)
    spectral = None
    if a.mrstft:
        from .spectral import default_mrstft

        spectral = default_mrstft(dev)
    mcd = None
    if a.mcd:
        from .mcd import default_mcd

        mcd = default_mcd(dev)
    tot, n, f0_tot, f0_n = {}, 0, {}, {}
    for i in range(0, len(segs), a.batch):
        y = torch.from_numpy(np.stack(segs[i : i + a.batch])).to(dev)
        r = score_segments(y, gen, disc, tracker=trk, meter=meter, stoi_meter=stoi_meter, spectral=spectral, mcd=mcd)
        f0 = {k: r.pop(k) for k in F0_KEYS + LOUDNESS_KEYS + STOI_KEYS if k in r}
        for k, v in r.items():
            tot[k] = tot.get(k, 0.0) + v * y.shape[0]
        n += y.shape[0]
        for k, v in f0.items():  # a pass without a frame voiced in both has no F0 figure (nan): it is left out of that figure's mean
            if v == v:
                f0_tot[k], f0_n[k] = f0_tot.get(k, 0.0) + v * y.shape[0], f0_n.get(k, 0) + y.shape[0]
    m = {k: v / n for k, v in tot.items()}
    print(f"{n} segments of {a.segment} samples: adversarial {m['adv']:.4f}  feature matching {m['fm']:.4f}  log-mel L1 {m['mel']:.4f}  "
          f"adv + fm + {MEL_WEIGHT:g} * mel = {m['total']:.4f}  (discriminator loss {m['disc']:.4f})")
    if spectral is not None:
        print(f"spectral distance of y_hat against y, mean over the segments: multi-resolution STFT {m['mrstft']:.4f}  (SC {m['sc']:.4f} + log-mag L1 "
              f"{m['logmag']:.4f})  LSD {m['lsd']:.2f} dB")
    if mcd is not None:
        print(f"mel-cepstral distortion of y_hat against y, mean over the segments: MCD {m['mcd']:.3f} dB")
    if trk is not None:
        f = {k: f0_tot[k] / f0_n[k] if f0_n.get(k) else float("nan") for k in F0_KEYS}
        print(f"F0 of y_hat against y, mean over the passes: RMSE {f['f0_rmse_cents']:.1f} cents  voicing error {100 * f['voicing_error']:.2f} %  "
              f"gross error {100 * f['gross_error']:.2f} %")
    if meter is not None:
        f = {k: f0_tot[k] / f0_n[k] if f0_n.get(k) else float("nan") for k in LOUDNESS_KEYS}
        print(f"integrated loudness, mean over the passes: y {f['lufs_y']:.2f} LUFS  y_hat {f['lufs_y_hat']:.2f} LUFS  "
              f"difference {f['lufs_y_hat'] - f['lufs_y']:+.2f} LU")
    if stoi_meter is not None:
        f = {k: f0_tot[k] / f0_n[k] if f0_n.get(k) else float("nan") for k in STOI_KEYS}
        print(f"intelligibility of y_hat against y, mean over the passes: STOI {f['stoi']:.4f}  ESTOI {f['estoi']:.4f}")


if __name__ == "__main__":
    main()
