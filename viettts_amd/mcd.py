"""Mel-cepstral distortion on the GPU (include/vtts_mcd.h, viettts_amd/csrc/mcd.hip): MCD in dB of time-aligned log-mels, and MCD-DTW of
two log-mel sequences of different lengths.

    Mcd(n_mels=80, n_ceps=13, band=0, device="cuda:0")
        .basis()                                  # [K, M] the DCT-II rows 1 .. K the kernels use
        .cepstra(logmel, lens)                    # [N, T, M] -> [N, T, K], zeros past each row's length
        .aligned(mel_a, mel_b, lens, frames)      # [N] float64 MCD in dB (and the per-frame distances [N, T] float32)
        .dtw(mel_a, mel_b, la, lb)                # McdDtwResult(mcd, total, path_len, span)
    mel_mcd(mel_a, mel_b, lens)                   # the same through one Mcd per (n_mels, n_ceps, band, device)
    mel_mcd_dtw(mel_a, mel_b, la, lb, band=0)
    wav_mcd(wav_a, wav_b, lengths_a, lengths_b, dtw=False)       # two waveform batches through resynth.wav2mel

    python -m viettts_amd.mcd --ref A.wav --test B.wav [--dtw] [--band R] [--n-ceps 13]

The figure: ``alpha * mean_t sqrt(sum_k (ca[t, k] - cb[t, k])^2)`` with ``alpha = 10 sqrt(2) / ln 10``, over the orthonormal DCT-II
coefficients 1 .. K of the natural-log mel (c0, the energy term, is left out); MCD-DTW is ``alpha * total / path_len`` along the optimal
warp of include/vtts_dtw.h's recurrence under that frame distance.  ``total`` and ``path_len`` come back too, so a caller can normalise by
the reference's frames.

Out of scope: SPTK / WORLD mel-generalised cepstra (frequency-warped all-pole cepstra: this is the log-mel-cepstrum MCD, and its figures
are not those of an SPTK pipeline), c0-inclusive variants, voiced-only or silence masks, other DTW step patterns or slope weights,
soft-DTW, gradients, the streamed paths, and any claim about how the figure relates to listening tests.  The reference has no such stage;
nothing here is re-exported under ``vietTTS/``.  No CPU fallback: the kernels are the only implementation.
"""
from __future__ import annotations

import argparse
import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._handle import NativeHandle, ptr
from .align import _lengths

ALPHA = _lib.MCD_ALPHA


class McdDtwResult(NamedTuple):
    mcd: torch.Tensor       # [N] float64: alpha * total / path_len, dB
    total: torch.Tensor     # [N] float32: the summed frame distances along the path
    path_len: torch.Tensor  # [N] int32: cells on the path
    span: torch.Tensor      # [N, Ta, 2] int32: first and last column of the path in each row of a, -1 past la


class Mcd(NativeHandle):
    """One ``vtts_mcd`` handle: ``n_ceps`` DCT-II coefficients of ``n_mels`` natural-log mel bands, and the DTW band ``r`` of
    include/vtts_dtw.h (``dtw`` only).  Every row's results are bit for bit what the row gives alone.  The workspace only grows; a DTW batch
    whose workspace would pass ``workspace_budget`` bytes runs in slices of pairs.  Asynchronous on torch's current stream of the device.
    One Mcd serves one call at a time."""

    def __init__(self, n_mels: int = 80, n_ceps: int = 13, band: int = 0, device="cuda:0", max_frames: int = _lib.DTW_MAX_FRAMES,
                 workspace_budget: int = 1 << 30, lib_path=None):
        super().__init__("vtts_mcd", device, lib_path, "cepstral meter")
        self.n_mels, self.n_ceps, self.band, self.max_frames = int(n_mels), int(n_ceps), int(band), int(max_frames)
        self.workspace_budget = int(workspace_budget)
        self._create(C.byref(_lib.McdCfg(self.n_mels, self.n_ceps, self.band, self.max_frames)))

    def basis(self) -> np.ndarray:
        out = np.empty((self.n_ceps, self.n_mels), dtype=np.float32)
        self._call("basis", out.ctypes.data_as(_lib.fp))
        return out

    def _mels(self, x, what: str) -> torch.Tensor:
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self.device)
        if not isinstance(x, torch.Tensor) or x.device != self.device or x.dtype != torch.float32:
            raise ValueError(f"{what} must be a float32 tensor on {self.device} or a numpy array")
        if x.dim() == 2:
            x = x[None]
        if x.dim() != 3 or x.shape[2] != self.n_mels or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError(f"{what} must be [N, T, {self.n_mels}] with N, T >= 1, got {tuple(x.shape)}")
        return x.contiguous()

    @staticmethod
    def _checked(lens, limit: int, what: str, low: int = 0):
        if min(lens) < low or max(lens) > limit:
            raise ValueError(f"{what} must lie in {low} .. {limit}")
        return lens

    def cepstra(self, logmel, lens=None) -> torch.Tensor:
        """``[N, T, n_mels]`` -> ``[N, T, n_ceps]`` float32; frames from ``lens[n]`` on are zeros (and are never read)."""
        x = self._mels(logmel, "logmel")
        N, T = x.shape[0], x.shape[1]
        lens = self._checked(_lengths(lens, N, T, "lens"), T, "lens")
        out = torch.empty((N, T, self.n_ceps), dtype=torch.float32, device=self.device)
        self._on_stream("cepstra", ptr(x), N, T, (C.c_int32 * N)(*lens), ptr(out))
        return out

    def aligned_workspace_bytes(self, N: int, T: int) -> int:
        n = C.c_size_t(0)
        self._call("aligned_workspace_bytes", int(N), int(T), C.byref(n))
        return int(n.value)

    def dtw_workspace_bytes(self, N: int, Ta: int, Tb: int) -> int:
        n = C.c_size_t(0)
        self._call("dtw_workspace_bytes", int(N), int(Ta), int(Tb), C.byref(n))
        return int(n.value)

    def aligned(self, mel_a, mel_b, lens=None, frames: bool = False):
        """MCD in dB of every row's first ``lens[n]`` frames (``min(Ta, Tb)`` without ``lens``): ``[N]`` float64 on the device, nan for a
        row of no frames.  With ``frames`` also the per-frame distances ``[N, min(Ta, Tb)]`` float32 (not scaled by alpha), zeros past
        the length."""
        a, b = self._mels(mel_a, "mel_a"), self._mels(mel_b, "mel_b")
        N, T = a.shape[0], min(a.shape[1], b.shape[1])
        if b.shape[0] != N:
            raise ValueError(f"mel_a holds {N} rows, mel_b {b.shape[0]}")
        lens = self._checked(_lengths(lens, N, T, "lens"), T, "lens")
        total = torch.empty((N,), dtype=torch.float64, device=self.device)
        per_frame = torch.empty((N, T), dtype=torch.float32, device=self.device) if frames else None
        ws = self._workspace(self.aligned_workspace_bytes(N, T))
        self._on_stream("aligned", ptr(a), ptr(b), N, a.shape[1], b.shape[1], (C.c_int32 * N)(*lens), ptr(total), ptr(per_frame), T, ptr(ws), ws.numel())
        mcd = ALPHA * total / torch.tensor(lens, dtype=torch.float64, device=self.device)
        return (mcd, per_frame) if frames else mcd

    def dtw(self, mel_a, mel_b, la=None, lb=None) -> McdDtwResult:
        a, b = self._mels(mel_a, "mel_a"), self._mels(mel_b, "mel_b")
        N, Ta, Tb = a.shape[0], a.shape[1], b.shape[1]
        if b.shape[0] != N:
            raise ValueError(f"mel_a holds {N} sequences, mel_b {b.shape[0]}")
        la = self._checked(_lengths(la, N, Ta, "la"), min(Ta, self.max_frames), "la", 1)
        lb = self._checked(_lengths(lb, N, Tb, "lb"), min(Tb, self.max_frames), "lb", 1)
        total = torch.empty((N,), dtype=torch.float32, device=self.device)
        path_len = torch.empty((N,), dtype=torch.int32, device=self.device)
        span = torch.empty((N, Ta, 2), dtype=torch.int32, device=self.device)
        per_slice = max(1, min(N, self.workspace_budget // max(1, self.dtw_workspace_bytes(1, Ta, Tb))))
        for n0 in range(0, N, per_slice):
            n1 = min(N, n0 + per_slice)
            k = n1 - n0
            ca, cb = self.cepstra(a[n0:n1], la[n0:n1]), self.cepstra(b[n0:n1], lb[n0:n1])
            ws = self._workspace(self.dtw_workspace_bytes(k, Ta, Tb))
            self._on_stream("dtw", ptr(ca), ptr(cb), k, Ta, Tb, (C.c_int32 * k)(*la[n0:n1]), (C.c_int32 * k)(*lb[n0:n1]),
                            ptr(total[n0:n1]), ptr(path_len[n0:n1]), ptr(span[n0:n1]), ptr(ws), ws.numel())
        return McdDtwResult(ALPHA * total.double() / path_len.double(), total, path_len, span)


_MCDS: dict = {}


def _device_of(*xs) -> torch.device:
    return next((x.device for x in xs if isinstance(x, torch.Tensor) and x.is_cuda), None) or torch.device("cuda", torch.cuda.current_device())


def default_mcd(device, n_mels: int = 80, n_ceps: int = 13, band: int = 0) -> Mcd:
    """One Mcd per (n_mels, n_ceps, band, device), created at first use: the functions' and the command lines'."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(n_mels), int(n_ceps), int(band), device)
    m = _MCDS.get(key)
    if m is None:
        m = _MCDS[key] = Mcd(n_mels, n_ceps, band, device)
    return m


def mel_mcd(mel_a, mel_b, lens=None, n_ceps: int = 13) -> torch.Tensor:
    """Aligned MCD in dB of two log-mel batches ``[N, T, M]``, per row (float64 ``[N]`` on the device)."""
    return default_mcd(_device_of(mel_a, mel_b), int(mel_a.shape[-1]), n_ceps).aligned(mel_a, mel_b, lens)


def mel_mcd_dtw(mel_a, mel_b, la=None, lb=None, band: int = 0, n_ceps: int = 13) -> McdDtwResult:
    """MCD-DTW of ``[N, Ta, M]`` against ``[N, Tb, M]``."""
    return default_mcd(_device_of(mel_a, mel_b), int(mel_a.shape[-1]), n_ceps, band).dtw(mel_a, mel_b, la, lb)


def wav_mcd(wav_a, wav_b, lengths_a=None, lengths_b=None, dtw: bool = False, band: int = 0, mel_filter=None, n_ceps: int = 13):
    """MCD of two waveform batches ``[N, Sa]`` and ``[N, Sb]`` (float32 or int16 PCM at the mel filter's rate), each through
    ``resynth.wav2mel``.  Aligned (``dtw=False``): over the frames both rows hold, ``[N]`` float64; ``dtw=True``: a McdDtwResult."""
    from . import resynth

    if mel_filter is None:
        mel_filter = resynth.default_mel_filter(_device_of(wav_a, wav_b))
    ma, mb = resynth.wav2mel(wav_a, lengths_a, mel_filter), resynth.wav2mel(wav_b, lengths_b, mel_filter)
    la = None if lengths_a is None else [mel_filter.num_frames(int(n)) for n in lengths_a]
    lb = None if lengths_b is None else [mel_filter.num_frames(int(n)) for n in lengths_b]
    m = default_mcd(mel_filter.device, mel_filter.n_mels, n_ceps, band if dtw else 0)
    if dtw:
        return m.dtw(ma, mb, la, lb)
    N = ma.shape[0]
    lens = [min(x, y) for x, y in zip(la or [ma.shape[1]] * N, lb or [mb.shape[1]] * N)]
    return m.aligned(ma, mb, lens)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="mel-cepstral distortion (dB) of a recording against a reference, on the GPU: log-mel cepstra, not SPTK's")
    ap.add_argument("--ref", required=True, help="PCM16 mono .wav: the reference; any rate but the model's is converted on the GPU")
    ap.add_argument("--test", required=True, help="PCM16 mono .wav; without --dtw at the reference's rate and within one model hop of its length")
    ap.add_argument("--dtw", action="store_true", help="MCD-DTW: warp --test onto --ref first (include/vtts_dtw.h's recurrence)")
    ap.add_argument("--band", type=int, default=0, help="with --dtw: band r of include/vtts_dtw.h (0: none)")
    ap.add_argument("--n-ceps", type=int, default=13, help="cepstral coefficients 1 .. K (c0 is left out)")
    return ap


def main(argv=None) -> None:
    from . import wavio
    from .nat.config import FLAGS
    from .stoi import check_pair

    ap = build_parser()
    a = ap.parse_args(argv)
    if a.band and not a.dtw:
        ap.error("--band needs --dtw")
    if a.band < 0 or not 1 <= a.n_ceps <= _lib.MCD_MAX_CEPS:
        ap.error(f"--band must be >= 0 and --n-ceps in 1 .. {_lib.MCD_MAX_CEPS}")
    (sr_a, x), (sr_b, y) = wavio.read_wav(a.ref), wavio.read_wav(a.test)
    if not a.dtw:
        n = check_pair(sr_a, len(x), sr_b, len(y))  # before the GPU is touched
        x, y = x[:n], y[:n]
    if not torch.cuda.is_available():
        raise RuntimeError("viettts_amd.mcd needs an MI355X visible to PyTorch-ROCm; there is no CPU path")
    dev = torch.device("cuda", torch.cuda.current_device())

    def on_device(pcm, sr):
        w = torch.from_numpy(np.ascontiguousarray(pcm.astype(np.int16))[None, :]).to(dev)
        if sr != FLAGS.sample_rate:
            from .audio import resampler

            w = resampler(sr, FLAGS.sample_rate, dev)(w, out_dtype="pcm16")
        return w

    wa, wb = on_device(x, sr_a), on_device(y, sr_b)
    r = wav_mcd(wa, wb, dtw=a.dtw, band=a.band, n_ceps=a.n_ceps)
    from .resynth import default_mel_filter

    fa, fb = (default_mel_filter(dev).num_frames(int(w.shape[1])) for w in (wa, wb))
    if a.dtw:
        print(f"MCD-DTW {float(r.mcd[0]):.3f} dB  ({fa} x {fb} frames, path of {int(r.path_len[0])} cells, {a.n_ceps} log-mel cepstra, band {a.band})")
    else:
        print(f"MCD {float(r[0]):.3f} dB  ({min(fa, fb)} frames, {a.n_ceps} log-mel cepstra)")


if __name__ == "__main__":
    main()
