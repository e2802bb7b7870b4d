"""Host-side owner of one HiFi-GAN generator on one GPU.

Mirrors the reference's ``Generator`` module (vietTTS/hifigan/model.py:77-125) as used by
``mel2wave`` (vietTTS/hifigan/mel2wave.py:28-38): construct from the hyper-parameters, hand it the
``hk_hifi.pickle`` parameter dict, call it on an NWC mel batch.  All arithmetic happens in the HIP
library (include/vtts_hifigan.h); PyTorch-ROCm only provides device memory and the stream.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from .. import _lib
from .._handle import NativeHandle, ptr
from .config import HifiganConfig, V1
from .weights import ParamDict, check_params, conv_specs


class Generator(NativeHandle):
    """``Generator(cfg)(mel)`` — mel ``[B, T, num_mels]`` float32 NWC -> wav ``[B, hop*T]`` float32.

    No CPU fallback: construction fails if the HIP extension is missing, and ``__call__`` fails
    unless the tensors live on a ROCm device.

    Concurrency: one Generator serves ONE call at a time.  The C handle keeps per-call state (ragged lengths, profiling
    counters, its side streams) and this object keeps one cached workspace tensor: two torch streams driving the same
    Generator concurrently would race on both.  Use one Generator per stream (the packed weights can be shared:
    ``other.adopt_packed(gen.packed_blob())``).
    """

    def __init__(self, cfg: HifiganConfig = V1, device="cuda:0", dtype: str = "f32", lib_path=None):
        super().__init__("vtts_hifigan", device, lib_path, "generator")
        self.cfg = cfg
        self.dtype = {"f32": _lib.VTTS_F32, "bf16": _lib.VTTS_BF16, "bf16x3": _lib.VTTS_BF16X3}[dtype]  # bf16x3: the fp32 engine's layouts and entry points
        self.dtype_name = dtype
        self._create(C.byref(_lib.make_cfg(cfg)), tail=(self.dtype,))
        self.hop = cfg.hop

    # ---- parameters (param_table(): the same 156 arrays hk_hifi.pickle holds) ---------------------
    @property
    def max_frames_per_pass(self) -> int:
        """Utterances of this many mel frames or more are refused by the C ABI (an utterance's largest activation must stay
        below 2^31 bytes: include/vtts_hifigan.h, vtts_hifigan_workspace_bytes); they go through viettts_amd.longform."""
        return self.get_option("max_frames_per_pass")  # the engine's own rule (engine.hip: check_pass_size), not a copy of it

    def load_params(self, params: ParamDict) -> None:
        """Re-lay-out a Haiku parameter dict into the packed device blob (once, not per call as
        the reference does at mel2wave.py:35-36)."""
        check_params(self.cfg, params)
        for spec in conv_specs(self.cfg):
            for which in ("w", "b"):
                self._set_param(spec.key, which, params[spec.key][which])
        self._pack()

    # ---- options --------------------------------------------------------------------------------
    def set_option(self, name: str, value: int) -> None:
        self._call("set_option", name.encode(), int(value))
        # the cached workspace stays: every call asks the engine for the size and _workspace() only ever grows it

    def get_option(self, name: str) -> int:
        v = C.c_int64(0)
        self._call("get_option", name.encode(), C.byref(v))
        return int(v.value)

    # ---- forward --------------------------------------------------------------------------------
    def workspace_bytes(self, B: int, T: int) -> int:
        n = C.c_size_t(0)
        self._call("workspace_bytes", B, T, C.byref(n))
        return int(n.value)

    def _check_mel(self, mel: torch.Tensor):
        if not isinstance(mel, torch.Tensor):
            raise TypeError("mel must be a torch.Tensor on the generator's device")
        if mel.device != self.device:
            raise ValueError(f"mel is on {mel.device}, generator on {self.device}")
        if mel.dtype != torch.float32 or mel.dim() != 3 or mel.shape[2] != self.cfg.num_mels:
            raise ValueError(f"mel must be float32 [B, T, {self.cfg.num_mels}] (NWC), got {tuple(mel.shape)} {mel.dtype}")
        if mel.shape[0] < 1 or mel.shape[1] < 1:
            raise ValueError("mel must have at least one utterance and one frame")
        return mel.contiguous()

    def _check_out(self, out: Optional[torch.Tensor], shape, what: str) -> torch.Tensor:
        """``out`` as given, or a new tensor: a contiguous float32 tensor of ``shape`` on this generator's device (``what`` names the shape)."""
        if out is None:
            return torch.empty(shape, dtype=torch.float32, device=self.device)
        if out.shape != tuple(shape) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != self.device:
            raise ValueError(f"out must be a contiguous float32 {what} tensor on the generator's device")
        return out

    def __call__(self, mel: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Asynchronous on torch's current stream of the device."""
        mel = self._check_mel(mel)
        B, T, _ = mel.shape
        out = self._check_out(out, (B, self.hop * T), "[B, hop*T]")
        ws = self._workspace(self.workspace_bytes(B, T))
        self._on_stream("forward", ptr(mel), B, T, ptr(out), ptr(ws), ws.numel())
        return out

    def forward_ragged(self, mel: torch.Tensor, frames, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Utterances of different lengths in one batch (every engine): ``mel`` ``[B, Tmax, num_mels]`` with utterance b's
        ``frames[b]`` frames at the start of its slot.  ``out[b, :hop*frames[b]]`` equals ``self(mel[b:b+1, :frames[b]])``
        bit for bit (fp32 engine: for frame counts that are multiples of 4 — an utterance run alone with another count takes the generic
        first transposed convolution, whose sums run in another order: ~1e-7); the rest of the row is zero.  ``frames``: int sequence or
        int32 tensor on the device."""
        mel = self._check_mel(mel)
        B, T, _ = mel.shape
        if isinstance(frames, torch.Tensor):
            fr = frames.to(device=self.device, dtype=torch.int32).contiguous()
            fr_host = None
        else:
            fr_host = [int(v) for v in frames]
            fr = torch.tensor(fr_host, dtype=torch.int32, device=self.device)
        if fr.numel() != B or (fr_host is not None and (min(fr_host) < 1 or max(fr_host) > T)):
            raise ValueError("frames must hold one count per utterance, 1 <= frames[b] <= mel.shape[1]")
        out = self._check_out(out, (B, self.hop * T), "[B, hop*T]")
        ws = self._workspace(self.workspace_bytes(B, T))
        self._on_stream("forward_ragged", ptr(mel), ptr(fr), B, T, ptr(out), ptr(ws), ws.numel())
        return out

    def forward_tap(self, mel: torch.Tensor, tap: str):
        """(wav, tap tensor) — test hook; tap in {"conv_pre","ups_i","mrf_i","pre_tanh"}."""
        mel = self._check_mel(mel)
        B, T, _ = mel.shape
        n = C.c_size_t(0)
        self._call("tap_elems", tap.encode(), B, T, C.byref(n))
        tap_t = torch.empty(int(n.value), dtype=torch.float32, device=self.device)
        out = torch.empty((B, self.hop * T), dtype=torch.float32, device=self.device)
        ws = self._workspace(self.workspace_bytes(B, T))
        self._on_stream("forward_tap", ptr(mel), B, T, ptr(out), ptr(ws), ws.numel(), tail=(tap.encode(), ptr(tap_t)))
        if tap == "pre_tanh":
            tap_t = tap_t.view(B, self.hop * T)
        else:
            tap_t = tap_t.view(B, -1)
        return out, tap_t

    def run_module(self, key: str, x: torch.Tensor, slope_in: float = 1.0, res: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Run one convolution module (per-layer KATs).
        fp32 handle: ``x`` is ``[B, C, L]`` channel-major (``[B, L, num_mels]`` for conv_pre) -> ``[B, Cout, Lout]``.
        bf16 handle: everything is channels-last fp32, ``x`` ``[B, L, C]`` -> ``[B, Lout, Cout]`` (``[B, Lout]`` for conv_post).
        ``out``: the result tensor to write (checked as in ``__call__``), else a new one."""
        spec = {s.key: s for s in conv_specs(self.cfg)}[key]
        x = x.contiguous()
        channels_last = self.dtype_name == "bf16" or key == "generator/~/conv1_d"
        if channels_last:
            B, L, _ = x.shape
        else:
            B, _, L = x.shape
        lout = L * spec.stride
        if self.dtype_name == "bf16":
            shape = (B, lout) if key == "generator/~/conv1_d_1" else (B, lout, spec.cout)
        else:
            shape = (B, spec.cout, lout)
        y = self._check_out(out, shape, "[" + ", ".join(str(d) for d in shape) + "]")
        if res is not None:
            res = res.contiguous()
        self._on_stream("run_module", key.encode(), ptr(x), B, L, C.c_float(slope_in), ptr(res), ptr(y))
        return y

    def run_pair(self, key_c1: str, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One fused ResBlock pair ``x' = convs2_z(lrelu(convs1_z(lrelu(x)))) + x`` named by its first convolution.
        bf16 handles: ``x`` fp32 ``[B, L, C]`` channels-last (rounded to bf16 on the way in) -> same shape;
        fp32 handles: ``x`` ``[B, C, L]`` channel-major -> same shape.
        ``out``: the result tensor to write (checked as in ``__call__``), else a new one.  On a bf16 handle the kernel writes an internal bf16
        buffer that is then converted into ``out``."""
        x = x.contiguous()
        if self.dtype_name == "bf16":
            B, L, _ = x.shape
        else:
            B, _, L = x.shape
        y = self._check_out(out, tuple(x.shape), "[" + ", ".join(str(d) for d in x.shape) + "]")
        self._on_stream("run_pair", key_c1.encode(), ptr(x), B, L, ptr(y))
        return y

    def run_resblock(self, key_c1_0: str, x: torch.Tensor, route: int = 0, rows=None, slope_out: float = 1.0, acc_add: bool = False,
                     div: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One ResBlock1 named by its ``convs1_0`` key, launched as the engine launches it (test hook): ``route`` 0 = the whole-ResBlock
        kernel, 1 = three fused-pair launches, 2 (fp32 / bf16x3 handles only) = the six convolutions one by one, under the options
        ``tiles`` and ``kernels``; then ``v = rb(x) (+ out)``, ``v / div``, ``leaky_relu(v, slope_out)``.
        bf16 handles: ``x`` fp32 ``[B, L, C]`` channels-last (``x`` and ``out`` rounded to bf16 on the way in); fp32 / bf16x3 handles:
        ``[B, C, L]``, ``slope_out`` must be 1.  ``rows``: per-utterance valid row counts (int sequence or int32 device tensor) or None.
        ``out`` is in-out (checked as in ``__call__``): rows no kernel writes keep what went in; ``acc_add`` needs it."""
        x = x.contiguous()
        if self.dtype_name == "bf16":
            B, L, _ = x.shape
        else:
            B, _, L = x.shape
        if acc_add and out is None:
            raise ValueError("acc_add needs the accumulator in `out`")
        y = self._check_out(out, tuple(x.shape), "[" + ", ".join(str(d) for d in x.shape) + "]")
        if rows is not None:
            rows = torch.as_tensor(rows).to(device=self.device, dtype=torch.int32).contiguous()
            if rows.numel() != B:
                raise ValueError("rows must hold one count per utterance")
        self._on_stream("run_resblock", key_c1_0.encode(), int(route), ptr(x), ptr(rows), B, L, C.c_float(slope_out), int(bool(acc_add)),
                        C.c_float(div), ptr(y))
        return y

    # ---- dominant-kernel timing (bench.py roofline) ----------------------------------------------
    def profile_read(self, reset: bool = True):
        ms, n, fl = C.c_double(0), C.c_int64(0), C.c_double(0)
        self._call("profile_read", C.byref(ms), C.byref(n), C.byref(fl), int(reset))
        name = self.lib.vtts_hifigan_profile_kernel(self._h)
        return {"ms": ms.value, "launches": int(n.value), "flops": fl.value, "kernel": name.decode() if name else ""}
