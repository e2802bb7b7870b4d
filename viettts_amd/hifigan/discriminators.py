"""vietTTS/hifigan/torch_model.py:221-414 — MultiPeriodDiscriminator, MultiScaleDiscriminator and the three losses as a
forward-only scoring pass on the GPU (include/vtts_disc.h, viettts_amd/csrc/disc.hip).  No gradients, no CPU fallback.

    d = Discriminators.from_checkpoint("do_02500000", device="cuda:0")
    scores, fmaps = d.forward(y)            # y [N, T]; 8 score tensors, 8 lists of feature maps, the reference's shapes
    L = d.losses(y, y_hat)                  # y, y_hat [B, T]; one 2 B-row pass, every weight streamed once

The loader folds weight norm / spectral norm on the host in fp64 and rounds once.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .. import _lib
from .._handle import NativeHandle, ptr

PERIODS = (2, 3, 5, 7, 11)
MPD_LAYERS, MSD_LAYERS = 6, 8  # feature maps per discriminator

_SUFFIXES = (".parametrizations.weight.original0", ".parametrizations.weight.original1", ".parametrizations.weight.original",
             ".parametrizations.weight.0._u", ".parametrizations.weight.0._v", ".weight_orig", ".weight_u", ".weight_g", ".weight_v",
             ".weight", ".bias")


def _f64(t) -> np.ndarray:
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.asarray(t, dtype=np.float64)


def fold_module(entries: Dict[str, object]) -> Tuple[np.ndarray, np.ndarray]:
    """One convolution's state-dict entries (suffix -> tensor) -> (effective weight [Cout, Cin / groups, k], bias), float32.

    Accepted styles: plain ``weight``; old-style weight norm ``weight_g`` / ``weight_v``; parametrised weight norm
    ``parametrizations.weight.original0`` (g) / ``original1`` (v); spectral norm in eval mode, ``weight_orig / (u . (W_mat v))`` with the
    stored ``weight_u`` / ``weight_v`` (or the parametrised ``original`` / ``0._u`` / ``0._v``) and no power iteration.
    Folded in fp64, rounded once."""
    e = {k.lstrip("."): v for k, v in entries.items()}
    if "weight_orig" in e or "parametrizations.weight.original" in e:
        w = _f64(e.get("weight_orig", e.get("parametrizations.weight.original")))
        u = _f64(e.get("weight_u", e.get("parametrizations.weight.0._u")))
        v = _f64(e.get("weight_v", e.get("parametrizations.weight.0._v")))
        sigma = float(u @ (w.reshape(w.shape[0], -1) @ v))
        w = w / sigma
    elif "weight_g" in e or "parametrizations.weight.original0" in e:
        g = _f64(e.get("weight_g", e.get("parametrizations.weight.original0")))
        v = _f64(e.get("weight_v", e.get("parametrizations.weight.original1")))
        norm = np.sqrt((v.reshape(v.shape[0], -1) ** 2).sum(axis=1)).reshape((-1,) + (1,) * (v.ndim - 1))
        w = v * (g / norm)
    elif "weight" in e:
        w = _f64(e["weight"])
    else:
        raise KeyError(f"no weight among {sorted(e)}")
    if "bias" not in e:
        raise KeyError(f"no bias among {sorted(e)}")
    if w.ndim == 4:  # Conv2d (k, 1) kernels
        w = w[..., 0]
    return np.ascontiguousarray(w, dtype=np.float32), np.ascontiguousarray(_f64(e["bias"]), dtype=np.float32)


def fold_state_dict(sd: Dict[str, object], prefix: str) -> Dict[str, Tuple[np.ndarray, np.ndarray]]:
    """A MultiPeriodDiscriminator / MultiScaleDiscriminator state dict -> ``{prefix.module: (w, b)}`` (prefix "mpd" or "msd")."""
    modules: Dict[str, Dict[str, object]] = {}
    for key, val in sd.items():
        for suf in _SUFFIXES:
            if key.endswith(suf):
                modules.setdefault(key[: -len(suf)], {})[suf] = val
                break
    return {f"{prefix}.{name}": fold_module(ent) for name, ent in modules.items()}


def fold_checkpoint(ckpt: Dict[str, Dict[str, object]]) -> Dict[str, Tuple[np.ndarray, np.ndarray]]:
    """Upstream's ``do_*`` dictionary (keys ``mpd``, ``msd``; anything else, e.g. optimiser state, is ignored)."""
    for k in ("mpd", "msd"):
        if k not in ckpt:
            raise KeyError(f"discriminator checkpoint has no '{k}' entry (keys: {sorted(ckpt)})")
    out = fold_state_dict(ckpt["mpd"], "mpd")
    out.update(fold_state_dict(ckpt["msd"], "msd"))
    return out


@dataclass
class DiscLosses:
    """Everything ``torch_model.py``'s ``feature_loss`` / ``discriminator_loss`` / ``generator_loss`` return for (MPD, MSD), as floats."""

    feature_mpd: float   # feature_loss(fmap_f_r, fmap_f_g), factor 2 inside
    feature_msd: float
    disc_mpd: float      # discriminator_loss(y_df_hat_r, y_df_hat_g)[0]
    disc_msd: float
    gen_mpd: float       # generator_loss(y_df_hat_g)[0]
    gen_msd: float
    feature: float       # feature_mpd + feature_msd
    disc: float
    gen: float
    r_losses_mpd: List[float]  # discriminator_loss's per-discriminator lists (5 and 3 entries)
    g_losses_mpd: List[float]
    r_losses_msd: List[float]
    g_losses_msd: List[float]
    gen_losses_mpd: List[float]
    gen_losses_msd: List[float]
    fmap_l1: List[float]       # mean |r - g| of the 54 feature maps, MPD's 30 first
    raw: Optional[torch.Tensor] = None  # the device buffer of include/vtts_disc.h's layout


class Discriminators(NativeHandle):
    """Both discriminator stacks on one ROCm device.  One instance serves one call at a time."""

    def __init__(self, device="cuda:0", lib_path=None):
        super().__init__("vtts_disc", device, lib_path, "discriminator stack")
        self._create()

    # ---- weights ----
    def load_params(self, params: Dict[str, Tuple[np.ndarray, np.ndarray]]) -> "Discriminators":
        """``{key: (w [Cout, Cin / groups, k], b [Cout])}`` effective fp32 weights for all 54 convolutions."""
        for key, (w, b) in params.items():
            self._set_param(key, "w", w)
            self._set_param(key, "b", b)
        self._pack()
        return self

    def load_checkpoint_dict(self, ckpt) -> "Discriminators":
        return self.load_params(fold_checkpoint(ckpt))

    @classmethod
    def from_checkpoint(cls, path, device="cuda:0") -> "Discriminators":
        """Upstream's ``do_*`` file (``torch.save({"mpd": ..., "msd": ..., ...})``)."""
        ckpt = torch.load(str(path), map_location="cpu")
        return cls(device).load_checkpoint_dict(ckpt)

    # ---- geometry ----
    def fmap_info(self, i: int, N: int, T: int):
        """(C, L, columns, element offset) of feature map i in the buffer of an N-row, T-sample call."""
        c, l, p, off = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._call("fmap_info", i, N, T, C.byref(c), C.byref(l), C.byref(p), C.byref(off))
        return int(c.value), int(l.value), int(p.value), int(off.value)

    def buffer_sizes(self, N: int, T: int) -> Tuple[int, int]:
        """Floats of the feature-map buffer and of the score buffer."""
        infos = [self.fmap_info(i, N, T) for i in range(_lib.DISC_NUM_FMAPS)]
        c, l, p, off = infos[-1]
        scores = sum(N * infos[i][1] * infos[i][2] for i in self._post_indices())
        return off + N * c * l * p, scores

    @staticmethod
    def _post_indices():
        return [MPD_LAYERS * d + MPD_LAYERS - 1 for d in range(5)] + [5 * MPD_LAYERS + MSD_LAYERS * d + MSD_LAYERS - 1 for d in range(3)]

    # ---- compute ----
    def _check_input(self, y: torch.Tensor) -> torch.Tensor:
        if not isinstance(y, torch.Tensor):
            y = torch.as_tensor(np.asarray(y, dtype=np.float32))
        if y.dim() == 3 and y.shape[1] == 1:  # the reference passes [B, 1, T]
            y = y[:, 0]
        if y.dim() != 2:
            raise ValueError(f"expected [N, T] (or [N, 1, T]) waveforms, got {tuple(y.shape)}")
        return y.to(device=self.device, dtype=torch.float32).contiguous()

    def forward_raw(self, y: torch.Tensor, fmaps_buf: Optional[torch.Tensor] = None, scores_buf: Optional[torch.Tensor] = None):
        """One pass over y [N, T]; returns the two flat float32 buffers (given ones are used as they are: tests pre-fill them)."""
        if self._blob is None:
            raise RuntimeError("no weights loaded: call load_params() / load_checkpoint_dict() / from_checkpoint()")
        y = self._check_input(y)
        N, T = y.shape
        nf, ns = self.buffer_sizes(N, T)
        if fmaps_buf is None:
            fmaps_buf = torch.empty(nf, dtype=torch.float32, device=self.device)
        if scores_buf is None:
            scores_buf = torch.empty(ns, dtype=torch.float32, device=self.device)
        for buf, n in ((fmaps_buf, nf), (scores_buf, ns)):
            if buf.numel() != n or buf.dtype != torch.float32 or buf.device != self.device or not buf.is_contiguous():
                raise ValueError(f"buffers must be contiguous float32 of {nf} and {ns} elements on {self.device}")
        self._on_stream("forward", ptr(y), N, T, ptr(fmaps_buf), ptr(scores_buf), None)
        return fmaps_buf, scores_buf

    def views(self, fmaps_buf: torch.Tensor, scores_buf: torch.Tensor, N: int, T: int):
        """(scores: 8 tensors [N, L * columns], fmaps: 8 lists of [N, C, L, columns] (MPD) / [N, C, L] (MSD) views)."""
        scores, fmaps, so, i = [], [], 0, 0
        for d in range(8):
            maps = []
            for _ in range(MPD_LAYERS if d < 5 else MSD_LAYERS):
                c, l, p, off = self.fmap_info(i, N, T)
                v = fmaps_buf[off : off + N * c * l * p]
                maps.append(v.view(N, c, l, p) if d < 5 else v.view(N, c, l))
                i += 1
            n = N * l * p
            scores.append(scores_buf[so : so + n].view(N, l * p))
            so += n
            fmaps.append(maps)
        return scores, fmaps

    def forward(self, y):
        y = self._check_input(y)
        fb, sb = self.forward_raw(y)
        return self.views(fb, sb, y.shape[0], y.shape[1])

    def losses_raw(self, fmaps_buf: torch.Tensor, scores_buf: torch.Tensor, B: int, T: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        if out is None:
            out = torch.empty(_lib.DISC_LOSS_FLOATS, dtype=torch.float32, device=self.device)
        self._on_stream("losses", ptr(fmaps_buf), ptr(scores_buf), B, T, ptr(out))
        return out

    @staticmethod
    def unpack_losses(raw: torch.Tensor) -> DiscLosses:
        r = raw[: _lib.DISC_LOSS_RESULTS].cpu().tolist()
        t = r[_lib.DISC_LOSS_TOTALS :]
        real, fake, gen = (r[o : o + 8] for o in (_lib.DISC_LOSS_REAL, _lib.DISC_LOSS_FAKE, _lib.DISC_LOSS_GEN))
        return DiscLosses(feature_mpd=t[0], feature_msd=t[1], disc_mpd=t[2], disc_msd=t[3], gen_mpd=t[4], gen_msd=t[5], feature=t[6], disc=t[7],
                          gen=t[8], r_losses_mpd=real[:5], g_losses_mpd=fake[:5], r_losses_msd=real[5:], g_losses_msd=fake[5:],
                          gen_losses_mpd=gen[:5], gen_losses_msd=gen[5:], fmap_l1=r[: _lib.DISC_NUM_FMAPS], raw=raw)

    def losses(self, y, y_hat) -> DiscLosses:
        """y, y_hat [B, T]: real and generated rows run as ONE 2 B-row pass (every weight is read once), then one reduction pass."""
        y, y_hat = self._check_input(y), self._check_input(y_hat)
        if y.shape != y_hat.shape:
            raise ValueError(f"y {tuple(y.shape)} and y_hat {tuple(y_hat.shape)} must have one shape")
        B, T = y.shape
        fb, sb = self.forward_raw(torch.cat([y, y_hat]))
        return self.unpack_losses(self.losses_raw(fb, sb, B, T))
