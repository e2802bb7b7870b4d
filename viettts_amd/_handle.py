"""What every Python owner of a native handle shares: the device rule, the handle's lifetime, calls on torch's current stream, the packed
parameter blob and a grow-only workspace.  ``Generator``, ``DurationModel``, ``AcousticModel``, ``MelFilter``, ``Discriminators`` and
``Resampler`` derive from :class:`NativeHandle` and keep only their own configuration, argument checks and result shaping.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib


def ptr(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class NativeHandle:
    """Owner of one ``<prefix>`` C handle (include/vtts_*.h) on one ROCm device.  ``noun`` is the word its messages use."""

    def __init__(self, prefix: str, device, lib_path, noun: str):
        self._h = C.c_void_p(0)
        self._blob: Optional[torch.Tensor] = None
        self._ws: Optional[torch.Tensor] = None
        self._prefix, self._noun = prefix, noun
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"{type(self).__name__} needs a ROCm device ('cuda:N'); there is no CPU path")
        if self.device.index is None:  # the C handle and every tensor of this owner name the same GPU
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.lib = _lib.load(lib_path)

    # ---- lifetime -------------------------------------------------------------------------------
    def _create(self, *args, tail=()) -> None:
        """``<prefix>_create(*args, device index, *tail, &handle)``."""
        _lib.check(self.lib, getattr(self.lib, self._prefix + "_create")(*args, self.device.index, *tail, C.byref(self._h)))

    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            getattr(self.lib, self._prefix + "_destroy")(self._h)
            self._h = C.c_void_p(0)
        self._blob = self._ws = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- calls ----------------------------------------------------------------------------------
    def _call(self, name: str, *args) -> None:
        _lib.check(self.lib, getattr(self.lib, f"{self._prefix}_{name}")(self._h, *args))

    def _on_stream(self, name: str, *args, tail=()) -> None:
        """``_call`` on this owner's device with torch's current stream behind ``args`` (and ``tail`` behind the stream)."""
        stream = torch.cuda.current_stream(self.device)
        with torch.cuda.device(self.device):
            self._call(name, *args, C.c_void_p(stream.cuda_stream), *tail)

    # ---- parameters -----------------------------------------------------------------------------
    def param_table(self):
        """[(key, which, shape)] of the arrays the C side expects."""
        n = C.c_int(0)
        self._call("num_params", C.byref(n))
        out = []
        for i in range(n.value):
            key, which = C.c_char_p(), C.c_char_p()
            shape = (C.c_int64 * 3)()
            nd = C.c_int(0)
            self._call("param_info", i, C.byref(key), C.byref(which), shape, C.byref(nd))
            out.append((key.value.decode(), which.value.decode(), tuple(int(shape[d]) for d in range(nd.value))))
        return out

    def _set_param(self, key: str, which: str, array) -> None:
        a = np.ascontiguousarray(array, dtype=np.float32)
        self._call("set_param", key.encode(), which.encode(), a.ctypes.data_as(C.c_void_p), (C.c_int64 * a.ndim)(*a.shape), a.ndim)

    @property
    def packed_bytes(self) -> int:
        n = C.c_size_t(0)
        self._call("packed_bytes", C.byref(n))
        return int(n.value)

    def _pack(self) -> None:
        """Lay the parameters out in a new device blob (uint8 from the caching allocator: >= 512-B aligned) and keep it."""
        blob = torch.empty(self.packed_bytes, dtype=torch.uint8, device=self.device)
        self._on_stream("pack", ptr(blob), blob.numel())
        self._blob = blob

    def packed_blob(self) -> torch.Tensor:
        if self._blob is None:
            raise RuntimeError("no parameters loaded")
        return self._blob

    def adopt_packed(self, blob: torch.Tensor) -> None:
        """Bind a blob another owner of the same configuration packed (weights broadcast once over RCCL: viettts_amd/dist.py)."""
        if blob.dtype != torch.uint8 or blob.numel() < self.packed_bytes or blob.device != self.device:
            raise ValueError(f"packed blob must be a uint8 tensor of packed_bytes on this {self._noun}'s device")
        self._call("bind_packed", ptr(blob), blob.numel())
        self._blob = blob

    # ---- workspace ------------------------------------------------------------------------------
    def _workspace(self, nbytes: int) -> torch.Tensor:
        """At least ``nbytes`` of scratch; it only ever grows."""
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None  # (released before its replacement is allocated)
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws
