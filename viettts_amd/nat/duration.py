"""Host-side owner of the NAT duration model on one GPU.

Mirrors ``predict_duration(tokens)`` of the reference (vietTTS/nat/text2mel.py:22-34): build
``DurationModel(is_training=False)`` (vietTTS/nat/model.py:53-70), hand it the checkpoint's ``params`` and ``aux``
dicts, apply it to token ids.  All arithmetic happens in the HIP library (include/vtts_nat.h); PyTorch-ROCm only
provides device memory and the stream.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .. import _lib
from .._handle import NativeHandle, ptr
from .config import FLAGS

HaikuDict = Dict[str, Dict[str, np.ndarray]]


def _lookup(d: HaikuDict, tail: str, name: str) -> np.ndarray:
    """An array by the tail of its Haiku module path (the leading scope depends on how the reference wrapped the
    module in hk.transform: ``duration_model/~/...`` for text2mel.py:23-24)."""
    hits = [k for k in d if (k == tail or k.endswith("/" + tail)) and name in d[k]]
    # "linear" also ends "lstm/linear": keep the shortest path, i.e. the module directly under the model scope
    hits.sort(key=len)
    hits = [k for k in hits if len(k) == len(hits[0])] if hits else hits
    if len(hits) != 1:
        raise KeyError(f"checkpoint has {len(hits)} modules ending in {tail!r} with an array {name!r}")
    return np.ascontiguousarray(d[hits[0]][name], dtype=np.float32)


def padded_rows(sentences: Sequence[Sequence[int]], durations: Optional[Sequence] = None, width: Optional[int] = None):
    """Token ids, and per-token durations where given, as zero-padded host arrays ``[B, width]`` (int32, float32 or None); ``width`` defaults
    to the longest sentence."""
    L = max(len(s) for s in sentences) if width is None else int(width)
    tok = np.zeros((len(sentences), L), dtype=np.int32)
    dur = np.zeros((len(sentences), L), dtype=np.float32) if durations is not None else None
    for i, s in enumerate(sentences):
        tok[i, : len(s)] = np.asarray(s, dtype=np.int32)
        if dur is not None:
            dur[i, : len(s)] = np.asarray(durations[i], dtype=np.float32).reshape(-1)
    return tok, dur


class DurationModel(NativeHandle):
    """``DurationModel()(tokens_list) -> [seconds per token]`` for a batch of sentences (the reference runs them one
    at a time; rows are independent)."""

    def __init__(self, vocab_size: int = FLAGS.vocab_size, lstm_dim: int = FLAGS.duration_lstm_dim, device="cuda:0", lib_path=None):
        super().__init__("vtts_nat_duration", device, lib_path, "model")
        self.vocab_size, self.lstm_dim = int(vocab_size), int(lstm_dim)
        self._create(C.byref(_lib.NatDurationCfg(self.vocab_size, self.lstm_dim)))

    def load_params(self, params: HaikuDict, state: HaikuDict) -> None:
        """``dic["params"]`` and ``dic["aux"]`` of duration_latest_ckpt.pickle (text2mel.py:27-28).  ``param_table()`` lists (module tail,
        array name, shape)."""
        for mod, name, shape in self.param_table():
            a = _lookup(state if name == "average" else params, mod, name)
            if a.shape != shape:
                raise ValueError(f"{mod}/{name}: checkpoint shape {a.shape}, the architecture needs {shape}")
            self._set_param(mod, name, a)
        self._pack()

    def __call__(self, sentences: Sequence[Sequence[int]]) -> List[np.ndarray]:
        """Token-id lists -> per-sentence float32 arrays of seconds per token."""
        if len(sentences) == 0:
            return []
        out, lens = self.launch(sentences)
        host = out.cpu().numpy()
        return [host[i, : lens[i]].copy() for i in range(len(lens))]

    def launch(self, sentences: Sequence[Sequence[int]]):
        """The same forward pass, enqueued on the current stream and NOT waited for: ``(seconds [B, Lmax] on the device, lengths)``.  A pipeline
        records an event behind it, enqueues more work and reads the tensor back on a copy stream (viettts_amd/pipeline.py)."""
        if self._blob is None:
            raise RuntimeError("no parameters loaded")
        B = len(sentences)
        if B == 0:
            raise ValueError("empty batch")
        lens = [len(s) for s in sentences]
        if min(lens) < 1:
            raise ValueError("empty token sequence")
        Lmax = max(lens)
        tok_d = torch.from_numpy(padded_rows(sentences)[0]).to(self.device)
        len_d = torch.tensor(lens, dtype=torch.int32, device=self.device)
        out = torch.empty((B, Lmax), dtype=torch.float32, device=self.device)
        n = C.c_size_t(0)
        self._call("workspace_bytes", B, Lmax, C.byref(n))
        ws = self._workspace(int(n.value))
        self._on_stream("forward", ptr(tok_d), ptr(len_d), B, Lmax, ptr(out), ptr(ws), ws.numel())
        return out, lens
