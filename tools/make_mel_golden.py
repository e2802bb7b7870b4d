"""Mint tests/golden/mel_golden.npz: seeded waveforms, the Slaney basis, and their fp64 log-mels as the REFERENCE'S OWN programs
compute them.

    python tools/make_mel_golden.py --reference /path/to/NTT123-vietTTS-checkout [--out tests/golden/mel_golden.npz]

Needs a checkout of the reference at mint time only; nothing of it is copied, and no test reads it.  Two routes are run and
must agree with tests/_mel_oracle.py to 1e-12 before anything is written:

  * vietTTS/nat/dsp.py::MelFilter, imported from the checkout by file path, with stand-in modules for ``jax`` / ``jax.numpy``
    (numpy, so everything runs in fp64) and ``librosa.filters.mel`` (tests/_mel_oracle.slaney_filterbank: librosa is not
    installed here, so the basis is our reading of it — DESIGN.md says what that leaves unpinned);
  * vietTTS/hifigan/create_mel.py::mel_spectrogram's formula — reflect pad, torch.stft(center=False) with a Hann window,
    sqrt(re^2 + im^2 + 1e-9), basis, log(clamp(1e-5)) — in fp64 with the same basis.

Arrays written (all seeded, reproducible bit for bit):
  speech  float32 [4, 16484]   29 harmonics (amplitude 1/h) of an f0 in 90 .. 250 Hz under a 3 Hz envelope, peak-scaled to 0.2, plus
                               white noise of sigma 0.003; 16484 = 64 * 256 + 100 is not a multiple of the hop
  pcm     int16   [4, 16484]   round(speech * 2^15)
  noise   float32 [2, 8192]    white, sigma 0.3
  lengths int32   [4]          a ragged case for ``speech``; one row has the minimum, 385
  melfb   float64 [80, 513]
  mel_<input>      float64     the log-mel of each input (pcm: of pcm / 2^15)
  err_ref32_<input> float64    max |fp32 restatement with numpy's complex64 FFT - fp64| : the reference's own arithmetic class,
                               the yardstick of tests/test_gpu_mel.py
"""
from __future__ import annotations

import argparse
import importlib.util
import sys
import types
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "tests"))
import _mel_oracle as oracle  # noqa: E402

SR, N_FFT, HOP, N_MELS, FMIN, FMAX = 16000, 1024, 256, 80, 0.0, 8000


def make_inputs():
    rng = np.random.default_rng(20261016)
    S = 64 * 256 + 100
    t = np.arange(S) / SR
    speech = np.zeros((4, S))
    for b in range(4):
        f0 = rng.uniform(90.0, 250.0)
        ph = rng.uniform(0.0, 2.0 * np.pi, size=29)
        x = sum(np.sin(2.0 * np.pi * f0 * h * t + ph[h - 1]) / h for h in range(1, 30))
        x = x * (0.55 + 0.45 * np.sin(2.0 * np.pi * 3.0 * t + rng.uniform(0.0, 2.0 * np.pi)))
        speech[b] = 0.2 * x / np.abs(x).max() + rng.normal(0.0, 0.003, size=S)
    speech = speech.astype(np.float32)
    pcm = np.clip(np.rint(speech.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
    noise = rng.normal(0.0, 0.3, size=(2, 8192)).astype(np.float32)
    lengths = np.array([S, 385, 5000, 12 * 1024 + 17], dtype=np.int32)
    return speech, pcm, noise, lengths


def reference_jax_melfilter(reference: Path):
    """The reference's MelFilter class, its jax / librosa imports served by numpy-backed stand-ins."""
    jnp = types.ModuleType("jax.numpy")
    for name in ("arange", "hanning", "pad", "reshape", "sqrt", "square", "einsum", "log", "clip", "stack", "ndarray", "fft"):
        setattr(jnp, name, getattr(np, name))
    jax = types.ModuleType("jax")
    jax.numpy = jnp
    jax.jit = lambda fn=None, **kw: fn
    jax.device_put = lambda x: x
    librosa = types.ModuleType("librosa")
    librosa.filters = types.ModuleType("librosa.filters")
    librosa.filters.mel = lambda sr, n_fft, n_mels, fmin, fmax: oracle.slaney_filterbank(sr, n_fft, n_mels, fmin, fmax)
    saved = {k: sys.modules.get(k) for k in ("jax", "jax.numpy", "librosa", "librosa.filters")}
    sys.modules.update({"jax": jax, "jax.numpy": jnp, "librosa": librosa, "librosa.filters": librosa.filters})
    try:
        spec = importlib.util.spec_from_file_location("_reference_nat_dsp", reference / "vietTTS" / "nat" / "dsp.py")
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod.MelFilter


def torch_route(y: np.ndarray, melfb: np.ndarray) -> np.ndarray:
    import torch

    yt = torch.from_numpy(y.astype(np.float64))
    p = int((N_FFT - HOP) / 2)
    yt = torch.nn.functional.pad(yt.unsqueeze(1), (p, p), mode="reflect").squeeze(1)
    spec = torch.stft(yt, N_FFT, hop_length=HOP, win_length=N_FFT, window=torch.hann_window(N_FFT, dtype=torch.float64), center=False,
                      pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
    mag = torch.sqrt(torch.view_as_real(spec).pow(2).sum(-1) + 1e-9)
    mel = torch.matmul(torch.from_numpy(melfb), mag)
    return torch.log(torch.clamp(mel, min=1e-5)).transpose(1, 2).numpy()  # [N, T, 80]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, type=Path, help="checkout of NTT123/vietTTS")
    ap.add_argument("--out", type=Path, default=REPO / "tests" / "golden" / "mel_golden.npz")
    a = ap.parse_args()

    speech, pcm, noise, lengths = make_inputs()
    melfb = oracle.slaney_filterbank(SR, N_FFT, N_MELS, FMIN, FMAX)
    ref_filter = reference_jax_melfilter(a.reference)(SR, N_FFT, N_MELS, FMIN, FMAX)
    assert np.array_equal(np.asarray(ref_filter.melfb), melfb)
    out = {"speech": speech, "pcm": pcm, "noise": noise, "lengths": lengths, "melfb": melfb}
    for name, y in (("speech", speech.astype(np.float64)), ("pcm", pcm.astype(np.float64) / 32768.0), ("noise", noise.astype(np.float64))):
        via_jax_route = np.asarray(ref_filter(y))
        via_torch_route = torch_route(y, melfb)
        ours = oracle.log_mel(y, melfb, dtype=np.float64)
        assert via_jax_route.dtype == np.float64 and via_jax_route.shape == ours.shape == via_torch_route.shape
        d1, d2 = np.abs(via_jax_route - ours).max(), np.abs(via_torch_route - ours).max()
        print(f"{name}: shape {ours.shape}, reference MelFilter vs restatement {d1:.2e}, torch.stft route vs restatement {d2:.2e}")
        assert d1 <= 1e-12 and d2 <= 1e-12
        err32 = float(np.abs(oracle.log_mel(y.astype(np.float32), melfb, dtype=np.float32).astype(np.float64) - via_jax_route).max())
        print(f"   fp32 restatement (complex64 FFT) vs fp64: {err32:.3e}; bands at the floor: {int((ours <= np.log(1e-5)).sum())}; max |mel| {np.abs(ours).max():.3f}")
        out["mel_" + name] = via_jax_route
        out["err_ref32_" + name] = np.float64(err32)
    np.savez_compressed(a.out, **out)
    print(f"wrote {a.out}: {a.out.stat().st_size} bytes")


if __name__ == "__main__":
    main()
