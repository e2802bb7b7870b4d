"""Drop-in for the reference CLI ``python -m vietTTS.synthesizer`` (vietTTS/synthesizer.py:12-39).

Same flags, defaults and prints; the text normalisation applies the reference's substitutions in the
reference's order (:21-31).  Unlike the reference this module has a ``main()`` (importing the
reference runs the whole pipeline at import time).  One addition:
``--mel-file`` synthesises from a saved ``[T, 80]`` / ``[1, T, 80]`` float32 mel (.npy) so the
mel->waveform path can be driven on its own (the text path runs the NAT duration and acoustic models of
``viettts_amd/nat`` like the reference's), and ``--low-latency`` runs the acoustic decoder's frame loop as one resident kernel
(``viettts_amd.nat.text2mel.set_low_latency``), and ``--resample`` makes ``--sample-rate R`` a conversion to R on the GPU
(``viettts_amd.audio.Resampler``) where the reference, and this CLI without the flag, only label the 16 kHz samples with R, and ``--stream``
writes the output chunk by chunk while the acoustic decoder is still running (``viettts_amd.streaming``): the WAV header first — the sample count
is known before the first decoder frame — then PCM16 per chunk of ``--chunk-frames`` mel frames, flushed; ``--output -`` writes the raw PCM16 to
stdout (the two printed lines go to stderr then); ``--stream --output-rate R`` converts the streamed samples to R chunk by chunk
(``viettts_amd.audio.ResamplerStream``), the header carrying R and the converted count; ``--denoise S`` subtracts S times the vocoder's own bias
spectrum (its output for an empty mel) from the clip directly behind the generator (``viettts_amd.denoise``), not with ``--stream`` and not with
``--vocoder griffinlim``.

    python -m viettts_amd.synthesizer --text "..." --output clip.wav --lexicon-file assets/infore/lexicon.txt
"""
from __future__ import annotations

import re
import unicodedata
from argparse import ArgumentParser
from pathlib import Path

import numpy as np

from .nat.config import FLAGS


def nat_normalize_text(text: str) -> str:
    """vietTTS/synthesizer.py:21-31 — NFKC, lower, punctuation -> " sil ", collapse."""
    sil = FLAGS.special_phonemes[FLAGS.sil_index]
    text = unicodedata.normalize("NFKC", text).lower().strip()
    steps = (
        (r"[\n.,:]+", f" {sil} "),
        ('"', " "),
        (r"\s+", " "),
        (r"[.,:;?!]+", f" {sil} "),
        ("[ ]+", " "),
        (f"( {sil}+)+ ", f" {sil} "),
    )
    for pattern, repl in steps:
        text = text.replace(pattern, repl) if pattern == '"' else re.sub(pattern, repl, text)
    return text.strip()


def build_parser() -> ArgumentParser:
    p = ArgumentParser(prog="viettts_amd.synthesizer")
    p.add_argument("--text", type=str)
    p.add_argument("--output", default="clip.wav", type=Path)
    p.add_argument("--sample-rate", default=16000, type=int)
    p.add_argument("--silence-duration", default=-1, type=float)
    p.add_argument("--lexicon-file", default=None)
    p.add_argument("--mel-file", default=None, type=Path, help="(extension) synthesise from a saved mel instead of text")
    p.add_argument("--low-latency", action="store_true", help="(extension) run the acoustic decoder's frame loop as one resident kernel")
    p.add_argument("--resample", action="store_true", help="(extension) convert the samples to --sample-rate on the GPU instead of relabelling them")
    p.add_argument("--stream", action="store_true", help="(extension) write the audio chunk by chunk while the decoder is still running")
    p.add_argument("--chunk-frames", default=32, type=int, help="(extension) mel frames per streamed chunk")
    p.add_argument("--loudness", default=None, type=float, help="(extension) bring the clip to this BS.1770 integrated loudness in LUFS, on the GPU")
    p.add_argument("--limit", action="store_true", help="(extension) with --loudness: the full gain to the target and a look-ahead limiter under -1 dBTP "
                   "(viettts_amd.limiter) in place of the sample-peak cap")
    p.add_argument("--ceiling-dbtp", default=None, type=float, help="(extension) with --stream: hold the true peak under this ceiling in dBTP, chunk by chunk "
                   "(viettts_amd.limiter.LimiterStream)")
    p.add_argument("--gain-db", default=None, type=float, help="(extension) with --stream --ceiling-dbtp: a fixed gain in dB ahead of the limiter")
    p.add_argument("--output-rate", default=None, type=int, help="(extension) with --stream: convert the samples to this rate on the GPU, chunk by chunk "
                   "(viettts_amd.audio.ResamplerStream); the header carries it")
    p.add_argument("--vocoder", default="hifigan", choices=("hifigan", "griffinlim"), help="(extension) griffinlim: mel -> wav by Griffin-Lim on the GPU "
                   "(viettts_amd.stft) with the NAT checkpoints only; the HiFi-GAN checkpoint is not opened")
    p.add_argument("--denoise", default=None, type=float, metavar="S", help="(extension) subtract S x the vocoder's own bias spectrum (its output for an empty "
                   "mel) from the clip, directly behind the generator (viettts_amd.denoise); the published scripts' --denoising-strength")
    return p


def _stream(args) -> int:
    """``--stream``: header, then PCM16 chunk by chunk.  With ``--mel-file`` only the vocoder streams."""
    import sys

    from .streaming import stream_mel, stream_text
    from .wavio import wav_header_pcm16

    raw = str(args.output) == "-"
    say = (lambda *a: print(*a, file=sys.stderr)) if raw else print
    info = {}
    lim = {} if args.ceiling_dbtp is None else {"limit": True, "gain_db": args.gain_db or 0.0, "ceiling_dbtp": args.ceiling_dbtp}
    rate = args.sample_rate
    if args.output_rate is not None:  # (main() has checked that --sample-rate is the models' then)
        lim["out_rate"] = rate = args.output_rate
    if args.mel_file is not None:
        from .hifigan.mel2wave import _generator

        mel = np.load(args.mel_file).astype(np.float32)
        mel = mel[0] if mel.ndim == 3 else mel
        gen = _generator()
        info["samples"] = gen.hop * mel.shape[0]
        if args.output_rate is not None:
            from math import gcd

            g = gcd(FLAGS.sample_rate, rate)
            info["samples"] = -(-info["samples"] * (rate // g) // (FLAGS.sample_rate // g))  # include/vtts_audio.h: ceil(S L / M)
        chunks = stream_mel(gen, mel, args.chunk_frames, out_dtype="pcm16", **lim)
    else:
        text = nat_normalize_text(args.text)
        say("Normalized text input:", text)
        chunks = stream_text(text, args.lexicon_file, args.silence_duration, chunk_frames=args.chunk_frames, out_dtype="pcm16", info=info, **lim)
    first = next(chunks, None)  # (the text path knows its sample count once the duration model has run: before the first decoder frame)
    say("writing output to file", args.output)
    f = sys.stdout.buffer if raw else open(str(args.output), "wb")
    try:
        if not raw:
            f.write(wav_header_pcm16(info["samples"], rate))
        while first is not None:
            f.write(first.astype("<i2", copy=False).tobytes())
            f.flush()
            first = next(chunks, None)
    finally:
        if not raw:
            f.close()
    return 0


def main(argv=None) -> int:
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.limit and args.loudness is None:
        parser.error("--limit needs --loudness")
    if not args.stream and (args.ceiling_dbtp is not None or args.gain_db is not None):
        parser.error("--ceiling-dbtp and --gain-db belong to --stream; for a whole clip use --loudness T --limit")
    if args.gain_db is not None and args.ceiling_dbtp is None:
        parser.error("--gain-db needs --ceiling-dbtp")
    if args.ceiling_dbtp is not None and args.sample_rate != FLAGS.sample_rate:
        parser.error(f"--ceiling-dbtp with --sample-rate {args.sample_rate}: the streamed samples are the models' {FLAGS.sample_rate} Hz, and the limiter's "
                     "look-ahead and oversampling filter are designed for that rate; a relabelled file would carry another true peak")
    if args.output_rate is not None:
        if not args.stream:
            parser.error("--output-rate belongs to --stream; for a whole clip use --sample-rate R --resample")
        if args.output_rate < 1:
            parser.error("--output-rate must be positive")
        if args.sample_rate != FLAGS.sample_rate:
            parser.error(f"--output-rate with --sample-rate {args.sample_rate}: the streamed samples are the models' {FLAGS.sample_rate} Hz and --output-rate "
                         "converts them; leave --sample-rate alone")
    if args.denoise is not None:  # argument errors before anything touches a device
        if not (args.denoise >= 0.0 and args.denoise != float("inf")):
            parser.error("--denoise must be finite and not negative")
        if args.stream:
            parser.error("--stream with --denoise: a streamed denoiser needs per-row overlap-add state between chunks; there is none yet")
        if args.vocoder == "griffinlim":
            parser.error("--vocoder griffinlim with --denoise: there is no vocoder to take a bias from")
    if args.stream:  # argument errors before anything touches a device
        if args.vocoder == "griffinlim":
            parser.error("--stream with --vocoder griffinlim: Griffin-Lim iterates over the whole clip; there is no streamed inverse transform")
        if args.resample:
            parser.error("--stream with --resample: --resample converts a whole clip; a stream converts chunk by chunk with --output-rate R")
        if args.low_latency:
            parser.error("--stream with --low-latency: a streamed decoder runs the per-frame launches, not the resident kernel")
        if args.loudness is not None:
            parser.error("--stream with --loudness: integrated loudness needs the whole utterance")
        if args.chunk_frames < 1:
            parser.error("--chunk-frames must be positive")
        if args.mel_file is None and args.text is None:
            raise SystemExit("--text (or --mel-file) is required")
        return _stream(args)
    from .wavio import write_wav, write_wav_pcm16

    if args.mel_file is not None:
        mel = np.load(args.mel_file).astype(np.float32)
        if mel.ndim == 2:
            mel = mel[None]
    else:
        if args.text is None:
            raise SystemExit("--text (or --mel-file) is required")
        from .nat.text2mel import set_low_latency, text2mel

        if args.low_latency:
            set_low_latency(True)
        text = nat_normalize_text(args.text)
        print("Normalized text input:", text)
        mel = text2mel(text, args.lexicon_file, args.silence_duration)
    if args.vocoder == "griffinlim":
        from .stft import mel2wave_griffinlim

        wave = np.squeeze(mel2wave_griffinlim(np.asarray(mel, dtype=np.float32)).cpu().numpy())
    else:
        from .hifigan.mel2wave import mel2wave

        wave = mel2wave(mel)
        if args.denoise is not None:
            from .denoise import generator_denoiser
            from .hifigan.mel2wave import _generator

            wave = np.squeeze(generator_denoiser(_generator())(np.asarray(wave, dtype=np.float32).reshape(1, -1), strength=args.denoise).cpu().numpy())
    if args.loudness is not None and args.limit:
        from .limiter import default_limiter

        out, res = default_limiter("cuda", FLAGS.sample_rate).normalize(np.asarray(wave, dtype=np.float32).reshape(1, -1), target=args.loudness)
        print(f"loudness: gain {20.0 * np.log10(float(res.gains[0])):+.2f} dB to {args.loudness:.1f} LUFS, limited by at most "
              f"{-20.0 * np.log10(float(res.min_gain[0])):.2f} dB under -1.0 dBTP")
        wave = out[0].cpu().numpy()
    elif args.loudness is not None:
        from .loudness import default_meter

        meter = default_meter("cuda", FLAGS.sample_rate)
        out, gains = meter.normalize(np.asarray(wave, dtype=np.float32).reshape(1, -1), target=args.loudness)
        print(f"loudness: gain {20.0 * np.log10(float(gains[0])):+.2f} dB to {args.loudness:.1f} LUFS")
        wave = out[0].cpu().numpy()
    print("writing output to file", args.output)
    if args.resample and args.sample_rate != FLAGS.sample_rate:
        from .audio import Resampler

        rs = Resampler(FLAGS.sample_rate, args.sample_rate, "cuda")
        write_wav_pcm16(args.output, rs(np.asarray(wave, dtype=np.float32), out_dtype="pcm16").cpu().numpy(), args.sample_rate)
        rs.close()
    else:
        write_wav(args.output, wave, args.sample_rate)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
