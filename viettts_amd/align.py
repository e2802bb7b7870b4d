"""Align recordings to text on the GPU: batched dynamic time warping between log-mels (include/vtts_dtw.h, viettts_amd/csrc/dtw.hip).

    Dtw(n_feat=80, band=0, device="cuda:0").dtw(a, b, la, lb)      # [N, Ta, D] against [N, Tb, D] -> DtwResult(total, path_len, span)
    log_mel_dtw(mel_a, mel_b, la, lb)                              # per pair: total / (path_len * n_feat), the DTW log-mel distance
    wav_dtw_distance(wav_a, wav_b, lengths_a, lengths_b)           # the same from two waveform batches of different lengths
    align(wavs, token_lists, wav_lengths, duration_model, acoustic_model)   # alignment by synthesis -> durations for the GTA pass

    python -m viettts_amd.align --wav F.wav --text "..." [--lexicon-file L] [--band R] [--output durations.json]

Alignment by synthesis: the acoustic model's own mel of the text, whose token boundaries are known exactly (they are the frame plan's
cumulative durations), is warped onto the recording's mel; the warp carries the boundaries over.  The result is an ``AcousticInput``
:func:`viettts_amd.nat.gta.forward_fn` / ``generate_gta`` take as it is, so a folder of recordings and transcripts is enough for
ground-truth-aligned mels.  The reference has no such module (its durations come from forced-aligner TextGrids); nothing here is
re-exported under ``vietTTS/``.  No CPU fallback: the kernels are the only implementation.  No claim about alignment quality on real
speech is made here.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._handle import NativeHandle, ptr


class DtwResult(NamedTuple):
    total: torch.Tensor     # [N] float32: D(la - 1, lb - 1)
    path_len: torch.Tensor  # [N] int32: cells on the path
    span: torch.Tensor      # [N, Ta, 2] int32: first and last column of the path in each query row, -1 past la


def _lengths(v, N: int, full: int, what: str):
    if v is None:
        return [full] * N
    v = [int(x) for x in (v.tolist() if isinstance(v, (torch.Tensor, np.ndarray)) else v)]
    if len(v) != N:
        raise ValueError(f"{what} must hold one length per pair")
    return v


class Dtw(NativeHandle):
    """``Dtw(n_feat, band, device).dtw(a, b, la=None, lb=None)``: every pair's optimal warp under the contract of include/vtts_dtw.h
    (L1 local cost, predecessors diagonal / up / left with a fixed tie rule, optional band ``r``), bit for bit what the pair gives alone.

    The handle's workspace only grows; a batch whose workspace would pass ``workspace_budget`` bytes is run in slices of pairs.
    Asynchronous on torch's current stream of the device.  One Dtw serves one call at a time."""

    def __init__(self, n_feat: int = 80, band: int = 0, device="cuda:0", max_frames: int = _lib.DTW_MAX_FRAMES, workspace_budget: int = 1 << 30, lib_path=None):
        super().__init__("vtts_dtw", device, lib_path, "aligner")
        self.n_feat, self.band, self.max_frames, self.workspace_budget = int(n_feat), int(band), int(max_frames), int(workspace_budget)
        self._create(C.byref(_lib.DtwCfg(self.n_feat, self.band, self.max_frames)))

    def workspace_bytes(self, N: int, Ta: int, Tb: int) -> int:
        n = C.c_size_t(0)
        self._call("workspace_bytes", int(N), int(Ta), int(Tb), C.byref(n))
        return int(n.value)

    def _rows(self, x, what: str) -> torch.Tensor:
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self.device)
        if not isinstance(x, torch.Tensor) or x.device != self.device or x.dtype != torch.float32:
            raise ValueError(f"{what} must be a float32 tensor on {self.device} or a numpy array")
        if x.dim() == 2:
            x = x[None]
        if x.dim() != 3 or x.shape[2] != self.n_feat or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError(f"{what} must be [N, T, {self.n_feat}] with N, T >= 1, got {tuple(x.shape)}")
        return x.contiguous()

    def dtw(self, a, b, la=None, lb=None) -> DtwResult:
        a, b = self._rows(a, "a"), self._rows(b, "b")
        N, Ta, Tb = a.shape[0], a.shape[1], b.shape[1]
        if b.shape[0] != N:
            raise ValueError(f"a holds {N} sequences, b {b.shape[0]}")
        la, lb = _lengths(la, N, Ta, "la"), _lengths(lb, N, Tb, "lb")
        total = torch.empty((N,), dtype=torch.float32, device=self.device)
        path_len = torch.empty((N,), dtype=torch.int32, device=self.device)
        span = torch.empty((N, Ta, 2), dtype=torch.int32, device=self.device)
        per_slice = max(1, min(N, self.workspace_budget // max(1, self.workspace_bytes(1, Ta, Tb))))
        for n0 in range(0, N, per_slice):
            n1 = min(N, n0 + per_slice)
            ws = self._workspace(self.workspace_bytes(n1 - n0, Ta, Tb))
            k = n1 - n0
            self._on_stream("forward", ptr(a[n0:n1]), ptr(b[n0:n1]), k, Ta, Tb, (C.c_int32 * k)(*la[n0:n1]), (C.c_int32 * k)(*lb[n0:n1]),
                            ptr(total[n0:n1]), ptr(path_len[n0:n1]), ptr(span[n0:n1]), ptr(ws), ws.numel())
        return DtwResult(total, path_len, span)


_DTWS: dict = {}


def aligner(n_feat: int, band: int, device) -> Dtw:
    """One Dtw per (n_feat, band, device), created at first use."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(n_feat), int(band), device)
    d = _DTWS.get(key)
    if d is None:
        d = _DTWS[key] = Dtw(n_feat, band, device)
    return d


def path(span_row, la: int) -> np.ndarray:
    """The path a span row set describes: ``[P, 2]`` host int array of (i, j) cells, from (0, 0) to (la - 1, last)."""
    s = np.asarray(span_row.cpu() if isinstance(span_row, torch.Tensor) else span_row)[: int(la)].astype(np.int64)
    counts = s[:, 1] - s[:, 0] + 1
    i = np.repeat(np.arange(int(la), dtype=np.int64), counts)
    j = np.concatenate([np.arange(f, l + 1, dtype=np.int64) for f, l in s]) if len(s) else np.zeros((0,), np.int64)
    return np.stack([i, j], axis=1)


def log_mel_dtw(mel_a, mel_b, la=None, lb=None, band: int = 0) -> torch.Tensor:
    """Per pair ``total / (path_len * n_feat)``: the mean absolute log-mel difference along the optimal warp (float64 ``[N]`` on the device)."""
    dev = mel_a.device if isinstance(mel_a, torch.Tensor) and mel_a.is_cuda else (mel_b.device if isinstance(mel_b, torch.Tensor) and mel_b.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    d = aligner(int(mel_a.shape[-1]), band, dev)
    r = d.dtw(mel_a, mel_b, la, lb)
    return r.total.double() / (r.path_len.double() * d.n_feat)


def wav_dtw_distance(wav_a, wav_b, lengths_a=None, lengths_b=None, mel_filter=None, band: int = 0) -> torch.Tensor:
    """:func:`log_mel_dtw` of two waveform batches ``[N, Sa]`` and ``[N, Sb]`` (float32 or int16 PCM), each through ``resynth.wav2mel``."""
    from . import resynth

    if mel_filter is None:
        dev = next((w.device for w in (wav_a, wav_b) if isinstance(w, torch.Tensor) and w.is_cuda), torch.device("cuda", torch.cuda.current_device()))
        mel_filter = resynth.default_mel_filter(dev)
    ma = resynth.wav2mel(wav_a, lengths_a, mel_filter)
    mb = resynth.wav2mel(wav_b, lengths_b, mel_filter)
    la = None if lengths_a is None else [mel_filter.num_frames(int(n)) for n in lengths_a]
    lb = None if lengths_b is None else [mel_filter.num_frames(int(n)) for n in lengths_b]
    return log_mel_dtw(ma, mb, la, lb, band)


def token_edges(frames_f32, la: int) -> np.ndarray:
    """The query frame each token ends at.  The acoustic model gives frame f to the token with ``end_{k-1} <= f < end_k``, ``end`` the
    cumulative durations in frames; so ``edge_k = min(la, ceil(cumsum_k))``, accumulated in float64, and the last edge is ``la``."""
    fr = np.asarray(frames_f32, dtype=np.float64).reshape(-1)
    if fr.size == 0:
        return np.zeros((0,), dtype=np.int64)
    edges = np.minimum(int(la), np.ceil(np.cumsum(fr))).astype(np.int64)
    edges[-1] = int(la)
    return edges


def transfer_frames(edges, span_row, la: int, lb: int) -> np.ndarray:
    """Reference-side frame count of every token: query edge e lands at 0 (e = 0), ``lb`` (e = la) or ``first[e]``, the first reference
    column of query row e.  Non-negative integers that sum to ``lb``; a token of no query frames gets none."""
    first = np.asarray(span_row.cpu() if isinstance(span_row, torch.Tensor) else span_row)[: int(la), 0].astype(np.int64)
    e = np.concatenate([[0], np.asarray(edges, dtype=np.int64)])
    bound = np.where(e <= 0, 0, np.where(e >= int(la), int(lb), first[np.clip(e, 0, int(la) - 1)]))
    return np.diff(bound)


def transfer_durations(edges, span_row, la: int, lb: int, hop: int, sample_rate: int) -> np.ndarray:
    """:func:`transfer_frames` in seconds (float32): what ``AcousticInput.durations`` holds."""
    return (transfer_frames(edges, span_row, la, lb).astype(np.float64) * hop / sample_rate).astype(np.float32)


class Alignment(NamedTuple):
    batch: "object"          # viettts_amd.nat.gta.AcousticInput: phonemes, lengths, durations (seconds), wavs, wav_lengths
    frames: np.ndarray       # [B, L] int64 recording frames per token, 0-padded; row b sums to lb[b]
    distance: np.ndarray     # [B] float64 DTW log-mel distance between the model's mel and the recording's
    la: list                 # frames of the model's own mel per sentence
    lb: list                 # frames of each recording
    dtw: DtwResult
    query_mel: torch.Tensor  # [B, max la, mel_dim] the model's mel
    target_mel: torch.Tensor  # [B, max lb, mel_dim] the recordings' mel


def align(wavs_pcm16, token_lists: Sequence[Sequence[int]], wav_lengths, duration_model, acoustic_model, mel_filter=None, band: int = 0,
          dropout_seed: Optional[int] = 0, silence_duration: float = -1.0) -> Alignment:
    """Durations of ``token_lists`` in the recordings ``wavs_pcm16 [B, S]`` (int16, numpy or device tensor; row b's first
    ``wav_lengths[b]`` samples): predicted durations -> frame plan -> the acoustic model's mel over all of its frames (no trailing-silence
    cut, left on the device) -> DTW against ``MelFilter(wavs, wav_lengths)`` -> the token boundaries on the recording's frames."""
    from .nat.gta import AcousticInput
    from .nat.text2mel import frame_plan

    B = len(token_lists)
    wav_lengths = [int(v) for v in np.asarray(wav_lengths).reshape(-1)]
    if B < 1 or len(wav_lengths) != B:
        raise ValueError("one recording and one length per token list")
    device = acoustic_model.device
    if mel_filter is None:
        from .resynth import default_mel_filter

        mel_filter = default_mel_filter(device)
    seconds = duration_model([list(t) for t in token_lists])
    frames_q, la, _ = frame_plan([list(t) for t in token_lists], seconds, silence_duration)
    if min(la) < 1:
        raise ValueError("a sentence's predicted durations give no frame")
    seeds = None if dropout_seed is None else [int(dropout_seed)] * B
    query = acoustic_model([list(t) for t in token_lists], frames_q, la, dropout_seeds=seeds, to_host=False)
    target = mel_filter(wavs_pcm16, lengths=wav_lengths)
    lb = [mel_filter.num_frames(n) for n in wav_lengths]
    res = aligner(mel_filter.n_mels, band, device).dtw(query, target, la, lb)
    span = res.span.cpu().numpy()
    dist = (res.total.double() / (res.path_len.double() * mel_filter.n_mels)).cpu().numpy()
    L = max(len(t) for t in token_lists)
    phonemes = np.zeros((B, L), dtype=np.int32)
    frames = np.zeros((B, L), dtype=np.int64)
    durations = np.zeros((B, L), dtype=np.float32)
    for i, t in enumerate(token_lists):
        edges = token_edges(frames_q[i], la[i])
        phonemes[i, : len(t)] = np.asarray(t)
        frames[i, : len(t)] = transfer_frames(edges, span[i], la[i], lb[i])
        durations[i, : len(t)] = transfer_durations(edges, span[i], la[i], lb[i], mel_filter.hop, mel_filter.sample_rate)
    batch = AcousticInput(phonemes=phonemes, lengths=np.asarray([len(t) for t in token_lists], dtype=np.int32), durations=durations, wavs=wavs_pcm16,
                          wav_lengths=np.asarray(wav_lengths, dtype=np.int64))
    return Alignment(batch, frames, dist, list(la), lb, res, query, target)


def build_parser() -> argparse.ArgumentParser:
    from .nat.config import FLAGS

    ap = argparse.ArgumentParser(description="align a recording to its text on the GPU: seconds per token, and the DTW log-mel distance to the model's own rendering")
    ap.add_argument("--wav", required=True, help="PCM16 mono .wav; any rate but the model's is converted on the GPU")
    ap.add_argument("--text", required=True)
    ap.add_argument("--lexicon-file", default=str(FLAGS.data_dir / "lexicon.txt"))
    ap.add_argument("--band", type=int, default=0, help="band r of include/vtts_dtw.h (0: none)")
    ap.add_argument("--output", default=None, help="write {tokens, durations, distance} as JSON")
    return ap


def main(argv=None) -> None:
    from . import wavio
    from .nat.config import FLAGS
    from .nat.text2mel import acoustic_model, duration_model, text2tokens

    a = build_parser().parse_args(argv)
    dm, am = duration_model(), acoustic_model()  # FileNotFoundError without checkpoints, before the input is touched
    tokens = text2tokens(a.text, a.lexicon_file)
    sr, pcm = wavio.read_wav(a.wav)
    y = torch.from_numpy(np.ascontiguousarray(pcm.astype(np.int16))[None, :]).to(am.device)
    if sr != FLAGS.sample_rate:
        from .audio import resampler

        y = resampler(sr, FLAGS.sample_rate, am.device)(y, out_dtype="pcm16")
    r = align(y, [tokens], [y.shape[1]], dm, am, band=a.band)
    out = {"tokens": [int(t) for t in tokens], "durations": [float(d) for d in r.batch.durations[0, : len(tokens)]], "distance": float(r.distance[0])}
    print("tokens   ", out["tokens"])
    print("seconds  ", [round(d, 4) for d in out["durations"]])
    print(f"distance  {out['distance']:.4f} (DTW log-mel L1 between the model's rendering and the recording, {r.la[0]} x {r.lb[0]} frames)")
    if a.output:
        with open(a.output, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()
