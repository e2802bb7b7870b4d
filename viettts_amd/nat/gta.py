"""vietTTS/nat/gta.py:28-82 — ground-truth-aligned (GTA) mels: the teacher-forced acoustic model over recordings and their
alignments, the data one fine-tunes the HiFi-GAN vocoder on.  On one GPU: wav -> log-mel (:class:`~viettts_amd.nat.dsp.MelFilter`,
PCM16 mode) -> teacher-forced acoustic model (:meth:`~viettts_amd.nat.acoustic.AcousticModel.teacher_forced`) -> GTA mel; the
target mel never leaves HBM.

Corpus loading (TextGrid parsing, the reference's ``load_textgrid_wav``) is not part of this package: :func:`generate_gta` consumes
an iterator of ``(names, batch)`` with ``batch`` shaped like the reference's ``AcousticInput``.

Two semantics for a padded batch, chosen by ``reference_padding``:

* **rows alone** (default; this library's rule everywhere else): row i is its first ``lengths[i]`` tokens and its first
  ``wav_lengths[i]`` samples, i.e. the reference run on that utterance alone, unpadded;
* **reference padding**: the reference's corpus run, element for element — its loader hands the model a ``lengths`` that never
  resets the backward encoder LSTM, and the model treats all padded token columns (token 0, duration 0) as tokens and all frames of
  the padded wav as frames (the postnet's convolutions see decoder frames past the crop).

Either way the masks are the reference's six draws from ``rng`` at the batch's ``(B, F)``; they depend on the batch shape and the
row index, so a file's content follows the batching, as in the reference.
"""
from __future__ import annotations

import pathlib
from typing import Iterable, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from .config import FLAGS


class AcousticInput(NamedTuple):
    """vietTTS/nat/config.py:69-75."""

    phonemes: np.ndarray     # [B, L] int token ids, 0-padded
    lengths: np.ndarray      # [B] tokens per row
    durations: np.ndarray    # [B, L] SECONDS per token, 0-padded
    wavs: np.ndarray         # [B, S] int16 PCM (numpy or a device tensor), 0-padded
    wav_lengths: np.ndarray  # [B] samples per row
    mels: Optional[np.ndarray] = None  # ignored: computed from wavs (gta.py:29-38)


def forward_fn(model, melfilter, rng, batch, reference_padding: bool = False, to_host: bool = True):
    """gta.py:28-40 ``forward_fn_(params, aux, rng, inputs)`` with the parameters inside ``model``: the mel with the postnet residual,
    ``[B, F, mel_dim]`` (host array, or the device tensor with ``to_host=False``), F = frames of the padded wav.  Rows-alone mode zeroes a
    row past its own ``wav_length // hop`` frames."""
    hop = melfilter.hop
    wavs = batch.wavs
    if isinstance(wavs, np.ndarray) and wavs.dtype != np.int16:
        raise ValueError("wavs must be int16 PCM (gta.py:32 scales them by 2**-15; MelFilter's PCM16 mode does that on the GPU)")
    B = len(batch.phonemes)
    wav_lengths = [int(v) for v in np.asarray(batch.wav_lengths).reshape(-1)]
    if reference_padding:
        mels = melfilter(wavs)  # the padded rows as they are, zeros included
        F = int(mels.shape[1])
        lens, n_frames = [int(np.asarray(batch.phonemes).shape[1])] * B, [F] * B
    else:
        mels = melfilter(wavs, lengths=wav_lengths)  # each row reflected at its own end
        lens = [int(v) for v in np.asarray(batch.lengths).reshape(-1)]
        n_frames = [max(1, n // hop) for n in wav_lengths]
    frames = np.asarray(batch.durations, dtype=np.float32) * np.float32(melfilter.sample_rate) / np.float32(hop)  # gta.py:37, fp32, nothing rounded
    tokens = np.asarray(batch.phonemes)
    out = model.teacher_forced([tokens[i, : lens[i]] for i in range(B)], [frames[i, : lens[i]] for i in range(B)], mels, n_frames=n_frames, rng=rng,
                               to_host=False)
    return out.cpu().numpy() if to_host else out


def generate_gta(out_dir, batches: Iterable[Tuple[Sequence[str], AcousticInput]], ckpt=None, reference_padding: bool = False, model=None, melfilter=None):
    """gta.py:46-76: for every ``(names, batch)`` write ``out_dir/NAME.npy`` = ``mel[idx, :wav_length // hop].T``, float32 ``[mel_dim, l]``.
    ``ckpt``: path of ``acoustic_latest_ckpt.pickle`` (default ``FLAGS.ckpt_dir``).  ``model`` / ``melfilter``: ready objects instead (then
    ``model.checkpoint_rng`` is the key).  Returns the paths written."""
    out_dir = pathlib.Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    if model is None:
        from .acoustic import AcousticModel
        from .text2mel import load_acoustic_checkpoint

        params, aux, rng = load_acoustic_checkpoint(ckpt, with_rng=True)
        model = AcousticModel()
        model.load_params(params, aux)
        model.checkpoint_rng = rng
    rng = getattr(model, "checkpoint_rng", None)
    if rng is None:
        raise ValueError("the checkpoint carries no rng key: the reference's dropout and zoneout masks cannot be drawn")
    if melfilter is None:
        from .dsp import MelFilter

        melfilter = MelFilter(FLAGS.sample_rate, FLAGS.n_fft, FLAGS.mel_dim, 0.0, 8000, device=str(model.device))
    written = []
    for names, batch in batches:
        mel = forward_fn(model, melfilter, rng, batch, reference_padding=reference_padding)
        for idx, fn in enumerate(names):
            l = int(np.asarray(batch.wav_lengths).reshape(-1)[idx]) // melfilter.hop  # gta.py:75
            file = out_dir / f"{fn}.npy"
            np.save(file, np.asarray(mel[idx, :l], dtype=np.float32).T)
            written.append(file)
    return written
