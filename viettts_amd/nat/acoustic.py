"""Host-side owner of the NAT acoustic model on one GPU.

Mirrors the network apply inside ``predict_mel(tokens, durations)`` of the reference (vietTTS/nat/text2mel.py:61-82):
``AcousticModel(is_training=False).inference(tokens, durations, n_frames)`` (vietTTS/nat/model.py:128-151) with the
checkpoint's ``params`` / ``aux`` dicts.  All arithmetic happens in the HIP library (include/vtts_nat.h); PyTorch-ROCm only
provides device memory and the stream.  There is no CPU path.

The prenet's dropout is on at inference in the reference (model.py:95-100) and draws from JAX's threefry PRNG through
Haiku's key chain, starting from the checkpoint's ``rng``.  ``dropout_rng`` (that key, uint32[2]) has the library draw THAT
stream on the GPU (jax.random's classic threefry layout; restated in oracle/nat_oracle.py, pinned by JAX's documented
``PRNGKey(0)`` answers, not by a JAX run); ``dropout_seeds`` draws this library's own per-sentence streams on the GPU (one
seed per sentence, independent of batching: the throughput pipeline's choice); ``keep_masks`` (boolean
``[n_frames, 2, 256]`` per sentence) makes the dropout explicit; none of them runs without dropout.
:func:`bernoulli_keep_masks` draws host masks from numpy's PCG64 for tests.
"""
from __future__ import annotations

import ctypes as C
import logging
import os
from typing import Optional, Sequence

import numpy as np
import torch

from .. import _lib
from .._handle import NativeHandle, ptr
from .config import FLAGS
from .duration import HaikuDict, _lookup, padded_rows


def bernoulli_keep_masks(n_frames: int, seed: int, prenet_dim: int = 256) -> np.ndarray:
    """``[n_frames, 2, prenet_dim]`` boolean keep masks, P(keep) = 0.5 (hk.dropout(key, 0.5, x), model.py:97, :99)."""
    return np.random.default_rng(seed).random((n_frames, 2, prenet_dim)) >= 0.5


_STREAM_LOGGED = set()


def _log_stream_once(partitionable: bool) -> None:
    """Which dropout mask stream the reference-faithful path draws (vietTTS/nat/text2mel.py:65-73 hands the checkpoint's rng to whatever JAX
    is installed; the reference pins no version): said once, so that a mel that differs from a JAX >= 0.5 run is not a silent surprise."""
    if partitionable not in _STREAM_LOGGED:
        _STREAM_LOGGED.add(partitionable)
        # WARNING, not INFO: invisible at the default log level, a mel that differs from a run of the reference under another JAX release
        # would be a silent surprise
        logging.getLogger("viettts_amd.nat").warning(
            "prenet dropout masks: jax.random threefry, %s layout, under dm-haiku's PRNGSequence key chain (set VTTS_JAX_THREEFRY_PARTITIONABLE=%d for the other one)",
            "partitionable (JAX >= 0.5 default; unpinned restatement)" if partitionable else "classic (JAX < 0.5 default)", 0 if partitionable else 1)


class AcousticModel(NativeHandle):
    def __init__(self, device="cuda:0", lib_path=None, vocab_size: int = FLAGS.vocab_size, encoder_dim: int = FLAGS.acoustic_encoder_dim,
                 decoder_dim: int = FLAGS.acoustic_decoder_dim, prenet_dim: int = 256, mel_dim: int = FLAGS.mel_dim, postnet_dim: int = FLAGS.postnet_dim):
        super().__init__("vtts_nat_acoustic", device, lib_path, "model")
        self.cfg = _lib.NatAcousticCfg(vocab_size, encoder_dim, decoder_dim, prenet_dim, mel_dim, postnet_dim)
        self.mel_dim, self.prenet_dim, self.encoder_dim = mel_dim, prenet_dim, encoder_dim
        self._create(C.byref(self.cfg))

    def load_params(self, params: HaikuDict, state: HaikuDict) -> None:
        """``dic["params"]`` and ``dic["aux"]`` of acoustic_latest_ckpt.pickle (text2mel.py:62-71)."""
        for mod, name, shape in self.param_table():
            a = _lookup(state if name == "average" else params, "acoustic_model/~/" + mod, name)
            if a.shape != shape:
                raise ValueError(f"{mod}/{name}: checkpoint shape {a.shape}, the architecture needs {shape}")
            self._set_param(mod, name, a)
        self._pack()

    def device_keep_masks(self, seeds: Sequence[int], Fmax: int) -> torch.Tensor:
        """``[B, Fmax, 2, prenet_dim]`` uint8 keep masks drawn on the GPU (include/vtts_nat.h: Threefry-2x32-20, one
        64-bit seed per sentence; oracle/nat_oracle.py::threefry_keep_masks is the CPU restatement)."""
        B = len(seeds)
        sd = torch.tensor([int(x) & 0x7FFFFFFFFFFFFFFF for x in seeds], dtype=torch.int64, device=self.device)
        keep = torch.empty((B, int(Fmax), 2, self.prenet_dim), dtype=torch.uint8, device=self.device)
        self._on_stream("keep_masks", ptr(sd), B, int(Fmax), ptr(keep))
        return keep

    def device_keep_masks_haiku(self, rng_key, B: int, Fmax: int, partitionable: Optional[bool] = None) -> torch.Tensor:
        """``[B, Fmax, 2, prenet_dim]`` uint8 keep masks as the REFERENCE draws them from the checkpoint's ``rng`` (a
        jax.random.PRNGKey, uint32[2]): jax.random's threefry under dm-haiku's key chain (include/vtts_nat.h:
        vtts_nat_acoustic_keep_masks_haiku[_mode]; restated in oracle/nat_oracle.py::haiku_prenet_keep_masks).  The same masks for
        every sentence, as every run of the reference starts from the same key.

        ``partitionable``: which counter layout — False = the classic one (every JAX before 0.5, pinned by JAX's documented
        known answers), True = ``jax_threefry_partitionable`` (JAX >= 0.5's default; restated from recollection, unpinned).  None
        reads ``VTTS_JAX_THREEFRY_PARTITIONABLE`` (unset / 0 = classic).  The stream in use is logged once per process."""
        if partitionable is None:
            partitionable = os.environ.get("VTTS_JAX_THREEFRY_PARTITIONABLE", "0") not in ("", "0")
        _log_stream_once(bool(partitionable))
        k = np.asarray(rng_key, dtype=np.uint32).reshape(2)
        keep = torch.empty((int(B), int(Fmax), 2, self.prenet_dim), dtype=torch.uint8, device=self.device)
        self._on_stream("keep_masks_haiku_mode", int(k[0]), int(k[1]), int(bool(partitionable)), int(B), int(Fmax), ptr(keep))
        return keep

    def device_teacher_masks_haiku(self, rng_key, B: int, F: int, partitionable: Optional[bool] = None):
        """The masks of :meth:`teacher_forced` as the REFERENCE draws them from the checkpoint's ``rng`` (model.py:149, :162-165; include/vtts_nat.h:
        vtts_nat_acoustic_teacher_masks_haiku): ``(keep [B, F, 2, prenet_dim], zone [B, F, 4, decoder_dim])`` uint8 on the device.  Each of the six
        draws covers the whole ``(B, F, D)`` tensor, so a row's masks depend on ``B``, ``F`` and its row index.  ``partitionable`` as for
        :meth:`device_keep_masks_haiku` (mode 1 is the same unpinned restatement)."""
        if partitionable is None:
            partitionable = os.environ.get("VTTS_JAX_THREEFRY_PARTITIONABLE", "0") not in ("", "0")
        _log_stream_once(bool(partitionable))
        k = np.asarray(rng_key, dtype=np.uint32).reshape(2)
        keep = torch.empty((int(B), int(F), 2, self.prenet_dim), dtype=torch.uint8, device=self.device)
        zone = torch.empty((int(B), int(F), 4, int(self.cfg.decoder_dim)), dtype=torch.uint8, device=self.device)
        self._on_stream("teacher_masks_haiku", int(k[0]), int(k[1]), int(bool(partitionable)), int(B), int(F), ptr(keep), ptr(zone))
        return keep, zone

    def _mask_tensor(self, m, B: int, Fmax: int, inner: tuple) -> torch.Tensor:
        """A mask argument (device tensor, host array, or one host array per row) as a contiguous uint8 ``[B, Fmax, *inner]`` device tensor."""
        if isinstance(m, torch.Tensor):
            if tuple(m.shape) != (B, Fmax) + inner or m.device != self.device:
                raise ValueError(f"mask tensor must be [{B}, {Fmax}, {inner[0]}, {inner[1]}] on {self.device} (got {tuple(m.shape)} on {m.device})")
            return m.to(torch.uint8).contiguous()
        host = np.zeros((B, Fmax) + inner, dtype=np.uint8)
        if len(m) != B:
            raise ValueError("one mask per row")
        for i, row in enumerate(m):
            row = np.asarray(row)
            if row.shape[1:] != inner or row.shape[0] > Fmax:
                raise ValueError(f"row {i}: mask shape {row.shape}, expected [<= {Fmax}, {inner[0]}, {inner[1]}]")
            host[i, : row.shape[0]] = row.astype(bool)
        return torch.from_numpy(host).to(self.device)

    def teacher_forced(self, sentences: Sequence[Sequence[int]], durations_frames: Sequence[np.ndarray], mels, n_frames: Optional[Sequence[int]] = None,
                       rng=None, masks=None, to_host: bool = True, return_pre: bool = False):
        """The TEACHER-FORCED pass, ``AcousticModel(is_training=False).__call__`` of the reference (vietTTS/nat/model.py:146-169; what
        vietTTS/nat/gta.py runs to dump ground-truth-aligned mels): per row token ids, per-token durations in FRAMES (fp32, not rounded) and the
        TARGET mel — ``mels`` is a float32 ``[B, F, mel_dim]`` device tensor or host array, or one ``[F_row, mel_dim]`` host array per row; the
        one-frame shift happens in the library.  ``n_frames``: frames per row (default: ``F`` / each row's own).

        Dropout and zoneout (both on in the reference with ``is_training=False``): ``rng`` (the checkpoint's jax PRNGKey, uint32[2]) draws the
        reference's own six masks on the GPU at ``(B, F)``; ``masks = (keep [B, F, 2, prenet_dim], zone [B, F, 4, decoder_dim])`` (device tensors,
        host arrays or per-row host arrays; zone = 1 keeps the previous state) makes them explicit — with them a row's result does not depend on
        its batch; neither = no dropout and no zoneout.

        A row's tokens past ``len(sentences[i])`` do not exist (this library's rule everywhere).  The reference's corpus run treats the padded
        columns of its batch as tokens: pass every row padded (token 0, duration 0) to the common length and ``n_frames = F`` to reproduce it.

        Returns the mel with the postnet residual (the reference's second value; per-row host arrays ``[n_frames, mel_dim]``, or with
        ``to_host=False`` the device tensor ``[B, F, mel_dim]``, rows past ``n_frames`` zero); ``return_pre=True`` returns ``(pre, mel)``."""
        if self._blob is None:
            raise RuntimeError("no parameters loaded")
        if rng is not None and masks is not None:
            raise ValueError("rng draws the masks: give rng or masks, not both")
        B = len(sentences)
        lens = [len(s) for s in sentences]
        if B == 0 or min(lens) < 1:
            raise ValueError("empty batch or token sequence")
        if isinstance(mels, (torch.Tensor, np.ndarray)):
            if mels.ndim != 3 or mels.shape[0] != B or mels.shape[2] != self.mel_dim:
                raise ValueError(f"mels must be [{B}, F, {self.mel_dim}] (got {tuple(mels.shape)})")
            Fmax = int(mels.shape[1])
            if isinstance(mels, np.ndarray):
                mels = torch.from_numpy(np.ascontiguousarray(mels, dtype=np.float32))
            if mels.dtype != torch.float32:
                raise ValueError("mels must be float32")
            mel_d = mels.to(self.device).contiguous()
            n_frames = [Fmax] * B if n_frames is None else [int(n) for n in n_frames]
        else:
            rows = [np.asarray(m, dtype=np.float32) for m in mels]
            if len(rows) != B or any(r.ndim != 2 or r.shape[1] != self.mel_dim for r in rows):
                raise ValueError(f"mels: one [F_row, {self.mel_dim}] array per row")
            n_frames = [r.shape[0] for r in rows] if n_frames is None else [int(n) for n in n_frames]
            Fmax = max(r.shape[0] for r in rows)
            host = np.zeros((B, Fmax, self.mel_dim), dtype=np.float32)
            for i, r in enumerate(rows):
                host[i, : r.shape[0]] = r
            mel_d = torch.from_numpy(host).to(self.device)
        if len(n_frames) != B or min(n_frames) < 1 or max(n_frames) > Fmax:
            raise ValueError(f"n_frames: one count in 1 .. {Fmax} per row")
        Lmax = max(lens)
        tok, dur = padded_rows(sentences, durations_frames)
        keep_d = zone_d = None
        if rng is not None:
            keep_d, zone_d = self.device_teacher_masks_haiku(rng, B, Fmax)
        elif masks is not None:
            keep_d = None if masks[0] is None else self._mask_tensor(masks[0], B, Fmax, (2, self.prenet_dim))
            zone_d = None if masks[1] is None else self._mask_tensor(masks[1], B, Fmax, (4, int(self.cfg.decoder_dim)))
        tok_d = torch.from_numpy(tok).to(self.device)
        dur_d = torch.from_numpy(dur).to(self.device)
        len_d = torch.tensor(lens, dtype=torch.int32, device=self.device)
        nf_d = torch.tensor(n_frames, dtype=torch.int32, device=self.device)
        out = torch.empty((B, Fmax, self.mel_dim), dtype=torch.float32, device=self.device)
        pre = torch.empty_like(out) if return_pre else None
        n = C.c_size_t(0)
        self._call("forward_teacher_workspace_bytes", B, Lmax, Fmax, C.byref(n))
        ws = self._workspace(int(n.value))
        self._on_stream("forward_teacher", ptr(tok_d), ptr(len_d), ptr(dur_d), ptr(nf_d), B, Lmax, Fmax, ptr(mel_d), ptr(keep_d), ptr(zone_d), ptr(out),
                        ptr(pre), ptr(ws), ws.numel())
        if not to_host:
            return (pre, out) if return_pre else out
        host = out.cpu().numpy()
        res = [host[i, : n_frames[i]].copy() for i in range(B)]
        if not return_pre:
            return res
        hpre = pre.cpu().numpy()
        return [hpre[i, : n_frames[i]].copy() for i in range(B)], res

    def set_option(self, key: str, value: int) -> None:
        """``"bf16x3"``: 1 = the postnet's matrix products as three bf16 x bf16 terms on the bf16 matrix pipe (include/vtts_nat.h); 0 = fp32 (default).
        ``"resident"``: 1 = calls with one to four sentences run the decoder's frame loop as one resident kernel instead of three launches per
        frame (the low-latency path; fp32, same oracle bar, rounding of its own; every other call takes the launches as before — see
        :attr:`resident_used`); 0 = the launches (default).  ``"resident_grid"``: 0 / 64 / 128 / 256 workgroups for it (0 = the library's default)."""
        self._call("set_option", key.encode(), int(value))

    def get_option(self, key: str) -> int:
        v = C.c_int(0)
        self._call("get_option", key.encode(), C.byref(v))
        return int(v.value)

    @property
    def resident_used(self) -> bool:
        """Whether the last call ran the decoder loop as the resident kernel (option ``"resident"``)."""
        return bool(self.get_option("resident_used"))

    def resident_status(self) -> bool:
        """After a synchronisation: True if a wait inside the last resident launch ran out of its 100 ms budget (the kernel then gave up and the
        frames it did not produce are zero).  ``VttsError`` (VTTS_ERR_STATE) if this model has not launched the resident kernel."""
        v = C.c_int(0)
        self._call("resident_status", C.byref(v))
        return bool(v.value)

    def wait_group(self, group: int, stream: Optional[torch.cuda.Stream] = None) -> None:
        """Make ``stream`` (default: torch's current stream) wait until the rows of ``group`` of the last ``group_row0`` call are complete."""
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.device(self.device):
            self._call("wait_group", int(group), C.c_void_p(st.cuda_stream))

    def encode(self, sentences: Sequence[Sequence[int]]) -> torch.Tensor:
        """The token encoder alone (include/vtts_nat.h: vtts_nat_acoustic_encode), enqueued on the current stream: ``[B, Lmax, 2 * encoder_dim]`` on the
        device.  It needs the tokens only — a pipeline runs it while the host still turns durations into frame counts — and a row does not depend
        on its batch: select / re-order rows (``enc[rows]``) and hand them to :meth:`__call__` as ``encoded``."""
        if self._blob is None:
            raise RuntimeError("no parameters loaded")
        B = len(sentences)
        lens = [len(s) for s in sentences]
        if B == 0 or min(lens) < 1:
            raise ValueError("empty batch or token sequence")
        Lmax = max(lens)
        tok_d = torch.from_numpy(padded_rows(sentences)[0]).to(self.device)
        len_d = torch.tensor(lens, dtype=torch.int32, device=self.device)
        enc = torch.empty((B, Lmax, 2 * self.encoder_dim), dtype=torch.float32, device=self.device)
        n = C.c_size_t(0)
        self._call("workspace_bytes", B, Lmax, 1, C.byref(n))
        ws = self._workspace(int(n.value))
        self._on_stream("encode", ptr(tok_d), ptr(len_d), B, Lmax, ptr(enc), ptr(ws), ws.numel())
        return enc

    def _device_inputs(self, sentences, durations_frames, n_frames, Lmax: int, Fmax: int, keep_masks, dropout_seeds, dropout_rng, with_tokens: bool = True):
        """What forward() and stream_begin() read, on the device: padded tokens (None without ``with_tokens``) and durations, lengths, frame counts and
        the keep masks of whichever dropout argument is given (None for no dropout)."""
        B = len(sentences)
        tok, dur = padded_rows(sentences, durations_frames, Lmax)
        keep_d = None
        if keep_masks is not None:
            keep = np.zeros((B, Fmax, 2, self.prenet_dim), dtype=np.uint8)
            for i, m in enumerate(keep_masks):
                keep[i, : n_frames[i]] = np.asarray(m, dtype=bool)[: n_frames[i]]
            keep_d = torch.from_numpy(keep).to(self.device)
        elif dropout_rng is not None:
            keep_d = self.device_keep_masks_haiku(dropout_rng, B, Fmax)
        elif dropout_seeds is not None:
            keep_d = self.device_keep_masks(dropout_seeds, Fmax)
        tok_d = torch.from_numpy(tok).to(self.device) if with_tokens else None  # (the C side ignores the tokens when the encoder's output is given)
        dur_d = torch.from_numpy(dur).to(self.device)
        len_d = torch.tensor([len(s) for s in sentences], dtype=torch.int32, device=self.device)
        nf_d = torch.tensor([int(n) for n in n_frames], dtype=torch.int32, device=self.device)
        return tok_d, dur_d, len_d, nf_d, keep_d

    def __call__(self, sentences: Sequence[Sequence[int]], durations_frames: Sequence[np.ndarray], n_frames: Sequence[int],
                 keep_masks: Optional[Sequence[np.ndarray]] = None, dropout_seeds: Optional[Sequence[int]] = None, to_host: bool = True,
                 dropout_rng=None, group_row0: Optional[Sequence[int]] = None, encoded: Optional[torch.Tensor] = None):
        """Per sentence: token ids, per-token durations in FRAMES, number of frames -> mel ``[n_frames, mel_dim]``.
        Dropout: explicit ``keep_masks`` (host arrays), or ``dropout_rng`` (the checkpoint's jax PRNGKey, uint32[2]: the
        reference's own mask stream, drawn on the GPU), or ``dropout_seeds`` (one int per sentence: this library's own
        per-sentence streams, drawn on the GPU), or none of them (no dropout).  ``to_host=False`` returns the device tensor ``[B, Fmax, mel_dim]`` (rows past a
        sentence's ``n_frames`` are zero) instead of per-sentence host arrays: the generator's input stays in HBM.
        ``group_row0`` (with ``to_host=False``): row boundaries ``[0, ..., B]`` of groups whose mel is handed over as soon as the decoder has
        produced the group's last frame (include/vtts_nat.h: vtts_nat_acoustic_forward_groups); a consumer stream waits for group g with
        :meth:`wait_group`.  Same mel, bit for bit.
        ``encoded``: these sentences' rows of an :meth:`encode` output, in this call's order (``[B, L, 2 * encoder_dim]``, L >= the longest
        sentence): the token encoder is skipped.  Same mel, bit for bit."""
        if self._blob is None:
            raise RuntimeError("no parameters loaded")
        B = len(sentences)
        lens = [len(s) for s in sentences]
        if B == 0 or min(lens) < 1 or min(n_frames) < 1:
            raise ValueError("empty batch, token sequence or frame count")
        Lmax, Fmax = max(lens), int(max(n_frames))
        # every argument check before anything is uploaded or grown
        if group_row0 is not None and to_host:
            raise ValueError("group_row0 hands the mel over on the device: use to_host=False")
        if dropout_seeds is not None and keep_masks is None and dropout_rng is None and len(dropout_seeds) != B:
            raise ValueError("one dropout seed per sentence")
        if encoded is not None:
            if encoded.dim() != 3 or encoded.shape[0] != B or encoded.shape[1] < Lmax or encoded.shape[2] != 2 * self.encoder_dim or encoded.dtype != torch.float32:
                raise ValueError(f"encoded must be float32 [{B}, >= {Lmax}, {2 * self.encoder_dim}] (got {tuple(encoded.shape)} {encoded.dtype})")
            encoded = encoded.contiguous()
            Lmax = int(encoded.shape[1])
        tok_d, dur_d, len_d, nf_d, keep_d = self._device_inputs(sentences, durations_frames, n_frames, Lmax, Fmax, keep_masks, dropout_seeds, dropout_rng,
                                                                with_tokens=encoded is None)
        out = torch.empty((B, Fmax, self.mel_dim), dtype=torch.float32, device=self.device)
        n = C.c_size_t(0)
        self._call("workspace_bytes", B, Lmax, Fmax, C.byref(n))
        ws = self._workspace(int(n.value))
        args = (ptr(len_d), ptr(dur_d), ptr(nf_d), B, Lmax, Fmax, ptr(keep_d), ptr(out), ptr(ws), ws.numel())
        if encoded is None and group_row0 is None:
            self._on_stream("forward", ptr(tok_d), *args)
        else:  # the groups' row boundaries and longest frame counts travel behind the stream (no groups: boundaries [0], one unused count)
            r0 = [int(v) for v in group_row0] if group_row0 is not None else [0]
            ng = len(r0) - 1
            gfr = [max(int(n) for n in n_frames[r0[g] : r0[g + 1]]) if r0[g + 1] > r0[g] else 0 for g in range(ng)]
            groups = (ng, (C.c_int32 * (ng + 1))(*r0), (C.c_int32 * max(ng, 1))(*(gfr or [0])))
            if encoded is not None:
                self._on_stream("forward_from_encoder", ptr(encoded), *args, tail=groups)
            else:
                self._on_stream("forward_groups", ptr(tok_d), *args, tail=groups)
        if not to_host:
            return out
        host = out.cpu().numpy()
        if self.resident_used and self.resident_status():
            raise RuntimeError("the resident decoder kernel gave up: a wait between its workgroups exceeded 100 ms (the mel is incomplete)")
        return [host[i, : n_frames[i]].copy() for i in range(B)]

    def open_stream(self, sentences: Sequence[Sequence[int]], durations_frames: Sequence[np.ndarray], n_frames: Sequence[int], max_window: int,
                    keep_masks: Optional[Sequence[np.ndarray]] = None, dropout_seeds: Optional[Sequence[int]] = None, dropout_rng=None) -> "MelStream":
        """:meth:`__call__` cut along time (include/vtts_nat.h: the streaming session): the same arguments and rules; the token encoder and the
        conditioning of every frame are enqueued now, the decoder's frames and the postnet as the returned :class:`MelStream` is asked for them.
        ``max_window``: the most frames one :meth:`MelStream.finish` will cover.  One open stream per model: a second ``open_stream`` or any call of
        the model ends it."""
        if self._blob is None:
            raise RuntimeError("no parameters loaded")
        B = len(sentences)
        lens = [len(s) for s in sentences]
        if B == 0 or min(lens) < 1 or min(n_frames) < 1:
            raise ValueError("empty batch, token sequence or frame count")
        if int(max_window) < 1:
            raise ValueError("max_window must be positive")
        if dropout_seeds is not None and keep_masks is None and dropout_rng is None and len(dropout_seeds) != B:
            raise ValueError("one dropout seed per sentence")
        Lmax, Fmax = max(lens), int(max(n_frames))
        inputs = self._device_inputs(sentences, durations_frames, n_frames, Lmax, Fmax, keep_masks, dropout_seeds, dropout_rng)
        mel = torch.empty((B, Fmax, self.mel_dim), dtype=torch.float32, device=self.device)
        n = C.c_size_t(0)
        self._call("stream_workspace_bytes", B, Lmax, Fmax, int(max_window), C.byref(n))
        ws = self._workspace(int(n.value))
        tok_d, dur_d, len_d, nf_d, keep_d = inputs
        self._session = getattr(self, "_session", 0) + 1
        self._on_stream("stream_begin", ptr(tok_d), ptr(len_d), ptr(dur_d), ptr(nf_d), B, Lmax, Fmax, ptr(keep_d), ptr(mel), ptr(ws), ws.numel(), int(max_window))
        return MelStream(self, self._session, mel, (inputs, ws), Fmax)

    def open_pool(self, slots: int, Lmax: int, Fmax: int, max_window: int, dropout: bool = True) -> "MelPool":
        """A slot pool (include/vtts_nat.h): ``slots`` rows of at most ``Lmax`` tokens and ``Fmax`` frames that sentences enter and leave one by one
        while the decoder steps all of them (:class:`MelPool`).  ``max_window``: the most frames of a row one :meth:`MelPool.finish` covers.
        ``dropout=False``: no keep masks, no row has dropout.  One pool or stream per model: opening another, or any call of the model, ends it."""
        if self._blob is None:
            raise RuntimeError("no parameters loaded")
        slots, Lmax, Fmax, max_window = int(slots), int(Lmax), int(Fmax), int(max_window)
        if min(slots, Lmax, Fmax, max_window) < 1:
            raise ValueError("slots, Lmax, Fmax and max_window must be positive")
        mel = torch.empty((slots, Fmax, self.mel_dim), dtype=torch.float32, device=self.device)
        keep = torch.ones((slots, Fmax, 2, self.prenet_dim), dtype=torch.uint8, device=self.device) if dropout else None
        n = C.c_size_t(0)
        self._call("pool_workspace_bytes", slots, Lmax, Fmax, max_window, C.byref(n))
        ws = self._workspace(int(n.value))
        self._session = getattr(self, "_session", 0) + 1
        self._on_stream("pool_open", slots, Lmax, Fmax, max_window, ptr(keep), ptr(mel), ptr(ws), ws.numel())
        return MelPool(self, self._session, mel, keep, ws, slots, Lmax, Fmax, max_window)


class MelPool:
    """An open slot pool of an :class:`AcousticModel` (:meth:`AcousticModel.open_pool`).  ``mel`` is the ``[slots, Fmax, mel_dim]`` device tensor the
    windows land in.  The host's copy of the pool's clock: ``tick``, and per slot ``busy``, ``start``, ``n_frames``, ``finished`` and
    :meth:`cursor`.  Work is enqueued on torch's current stream of the model's device.  A context manager; :meth:`close` is idempotent."""

    def __init__(self, model: AcousticModel, ticket: int, mel: torch.Tensor, keep, ws, slots: int, Lmax: int, Fmax: int, max_window: int):
        self._model, self._ticket, self.mel, self._keep, self._ws = model, ticket, mel, keep, ws
        self.slots, self.Lmax, self.Fmax, self.max_window = slots, Lmax, Fmax, max_window
        self.tick = 0
        self.busy = [False] * slots
        self.start, self.n_frames, self.finished = [0] * slots, [0] * slots, [0] * slots
        self._held = [None] * slots  # a slot's tokens and durations on the device: the library reads them until the slot is retired

    def _mine(self) -> bool:  # a later open_pool() / open_stream() took the handle: this object must not drive (or end) that one
        return self._model is not None and self._model._session == self._ticket

    def _on_stream(self, name: str, *args) -> None:
        if not self._mine():
            raise _lib.VttsError(-2, f"{name}: this pool is closed")
        self._model._on_stream(name, *args)

    def cursor(self, slot: int) -> int:
        """Frames of the slot's row the ticks enqueued so far decode."""
        return min(max(self.tick - self.start[slot], 0), self.n_frames[slot]) if self.busy[slot] else 0

    def admit(self, slot: int, tokens: Sequence[int], durations_frames, n_frames: int, dropout_seed: Optional[int] = None, keep_mask=None) -> None:
        """A sentence into the free slot ``slot``: token ids, per-token durations in FRAMES, its frame count; its first frame is decoded by the next
        tick.  Dropout as :meth:`AcousticModel.__call__`: ``keep_mask`` (``[n_frames, 2, prenet_dim]`` host array) or ``dropout_seed``, else none."""
        m, slot, n_frames = self._model, int(slot), int(n_frames)
        if not self._mine():
            raise _lib.VttsError(-2, "pool_admit: this pool is closed")
        if (keep_mask is not None or dropout_seed is not None) and self._keep is None:
            raise ValueError("the pool was opened with dropout=False")
        tok, dur = padded_rows([list(tokens)], [np.asarray(durations_frames, dtype=np.float32)], max(self.Lmax, len(tokens)))
        tok_d, dur_d = torch.from_numpy(tok[0]).to(m.device), torch.from_numpy(dur[0]).to(m.device)
        fill = self._keep is not None and 0 <= slot < self.slots and not self.busy[slot] and 1 <= n_frames <= self.Fmax and 1 <= len(tokens) <= self.Lmax
        if fill:  # the slot's keep rows, in stream order in front of the admission (a call the library will refuse fills nothing)
            if keep_mask is not None:
                row = np.ones((self.Fmax, 2, m.prenet_dim), dtype=np.uint8)
                row[:n_frames] = np.asarray(keep_mask, dtype=bool)[:n_frames]
                self._keep[slot].copy_(torch.from_numpy(row).to(m.device))
            elif dropout_seed is not None:
                self._keep[slot].copy_(m.device_keep_masks([dropout_seed], self.Fmax)[0])
            else:
                self._keep[slot].fill_(1)
        self._on_stream("pool_admit", slot, ptr(tok_d), len(tokens), ptr(dur_d), n_frames)
        self._held[slot] = (tok_d, dur_d)
        self.busy[slot], self.start[slot], self.n_frames[slot], self.finished[slot] = True, self.tick, n_frames, 0

    def decode(self, nticks: int) -> None:
        """Enqueue ``nticks`` frame steps of every slot."""
        self._on_stream("pool_decode", int(nticks))
        self.tick += int(nticks)

    def finish(self, windows: Sequence[tuple]) -> None:
        """``windows``: ``(slot, f0, f1)`` each, a slot at most once.  Enqueue postnet + residual of those frames of those rows into :attr:`mel`, all in
        one pass; per row the windows come in order and contiguous, and the row's cursor must have reached ``min(f1 + 10, n_frames)``."""
        n = len(windows)
        arr = [(C.c_int32 * max(n, 1))(*[int(w[k]) for w in windows]) for k in range(3)]
        self._on_stream("pool_finish", n, *arr)
        for sl, _, f1 in windows:
            self.finished[sl] = min(int(f1), self.n_frames[sl])

    def retire(self, slot: int) -> None:
        """Free the slot; its row decodes no further frame."""
        self._on_stream("pool_retire", int(slot))
        self.busy[int(slot)] = False
        self._held[int(slot)] = None

    def close(self) -> None:
        if self._model is not None:
            if self._mine() and self._model._h.value:
                self._model._call("pool_close")
            self._model = self._held = self._keep = self._ws = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MelStream:
    """An open streaming session of an :class:`AcousticModel` (:meth:`AcousticModel.open_stream`).  ``mel`` is the ``[B, Fmax, mel_dim]`` device tensor
    the windows land in; ``frames_decoded`` the host's copy of the decoder's cursor.  Work is enqueued on torch's current stream of the model's
    device.  A context manager; :meth:`close` is idempotent and also runs when the object is collected."""

    def __init__(self, model: AcousticModel, ticket: int, mel: torch.Tensor, held, n_frames_max: int):
        self._model, self._ticket, self.mel, self._held, self.n_frames_max = model, ticket, mel, held, n_frames_max
        self.frames_decoded = 0

    def _mine(self) -> bool:  # a later open_stream() took the handle's one session: this object must not drive (or end) that one
        return self._model is not None and self._model._session == self._ticket

    def _on_stream(self, name: str, *args) -> None:
        if not self._mine():
            raise _lib.VttsError(-2, f"{name}: this stream is closed")
        self._model._on_stream(name, *args)

    def decode(self, upto: int) -> None:
        """Enqueue the decoder's frames up to ``upto`` (exclusive; clipped to the longest row)."""
        self._on_stream("stream_decode", int(upto))
        self.frames_decoded = max(self.frames_decoded, min(int(upto), self.n_frames_max))

    def finish(self, f0: int, f1: int) -> None:
        """Enqueue postnet + residual of the frames ``[f0, f1)`` of every row into :attr:`mel`; the decoder must have reached ``f1 + 10``."""
        self._on_stream("stream_finish", int(f0), int(f1))

    def close(self) -> None:
        if self._model is not None:
            if self._mine() and self._model._h.value:
                self._model._call("stream_end")
            self._model = self._held = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
