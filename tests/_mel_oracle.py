"""Plain numpy restatement of the reference's waveform -> log-mel transform (vietTTS/nat/dsp.py: MelFilter.__call__;
vietTTS/hifigan/create_mel.py: mel_spectrogram computes the same thing through torch.stft(center=False)).

    reflect-pad by (n_fft - hop) / 2, frames of n_fft every hop, periodic Hann, DFT bins 0 .. n_fft / 2,
    mag = sqrt(re^2 + im^2 + 1e-9), mel = melfb @ mag, out[N, T, n_mels] = log(max(mel, 1e-5))

``dtype=np.float64`` is the oracle the tests compare against; ``dtype=np.float32`` runs the same steps in fp32 with numpy's
complex64 FFT, the arithmetic class of the reference's own fp32 run: its error against fp64 is the tests' yardstick.

The filter bank is OUR reading of ``librosa.filters.mel`` at its defaults (Slaney scale, Slaney area normalisation); librosa
itself is not a dependency of this repository.
"""
from __future__ import annotations

import numpy as np

F_SP = 200.0 / 3.0  # Hz per mel below the knee
MIN_LOG_HZ = 1000.0  # the knee ...
MIN_LOG_MEL = MIN_LOG_HZ / F_SP  # ... is mel 15
LOGSTEP = np.log(6.4) / 27.0
MAG_EPS = 1e-9
MEL_FLOOR = 1e-5


def hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    lin = f / F_SP
    return np.where(f >= MIN_LOG_HZ, MIN_LOG_MEL + np.log(np.maximum(f, MIN_LOG_HZ) / MIN_LOG_HZ) / LOGSTEP, lin)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= MIN_LOG_MEL, MIN_LOG_HZ * np.exp(LOGSTEP * (np.maximum(m, MIN_LOG_MEL) - MIN_LOG_MEL)), F_SP * m)


def slaney_filterbank(sample_rate=16000, n_fft=1024, n_mels=80, fmin=0.0, fmax=8000.0) -> np.ndarray:
    """[n_mels, n_fft / 2 + 1] float64 triangles, each scaled by 2 / (hz[i + 2] - hz[i])."""
    nb = n_fft // 2 + 1
    fftfreqs = np.arange(nb, dtype=np.float64) * (float(sample_rate) / n_fft)
    hz = mel_to_hz(np.linspace(float(hz_to_mel(fmin)), float(hz_to_mel(fmax)), n_mels + 2))
    fdiff = np.diff(hz)
    ramps = hz[:, None] - fftfreqs[None, :]
    fb = np.zeros((n_mels, nb), dtype=np.float64)
    for i in range(n_mels):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        fb[i] = np.maximum(0.0, np.minimum(lower, upper))
    return fb * (2.0 / (hz[2 : n_mels + 2] - hz[:n_mels]))[:, None]


def hann_periodic(n: int) -> np.ndarray:
    return np.hanning(n + 1)[:-1]


def num_frames(n_samples: int, n_fft: int = 1024, hop: int = 256) -> int:
    p = (n_fft - hop) // 2
    return (n_samples + 2 * p - n_fft) // hop + 1


def log_mel(y, melfb=None, n_fft: int = 1024, hop: int = 256, dtype=np.float64) -> np.ndarray:
    """y [N, S] -> [N, T, n_mels] in ``dtype`` (every step, the FFT included, runs in it)."""
    dtype = np.dtype(dtype)
    y = np.asarray(y)
    assert y.ndim == 2
    if melfb is None:
        melfb = slaney_filterbank(n_fft=n_fft)
    melfb = np.asarray(melfb).astype(dtype)
    y = y.astype(dtype)
    p = (n_fft - hop) // 2
    ypad = np.pad(y, ((0, 0), (p, p)), mode="reflect")
    T = (ypad.shape[1] - n_fft) // hop + 1
    idx = np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]
    frames = ypad[:, idx] * hann_periodic(n_fft).astype(dtype)  # [N, T, n_fft]
    spec = np.fft.fft(frames.astype(np.complex64 if dtype == np.float32 else np.complex128), axis=-1)[..., : n_fft // 2 + 1]
    assert spec.dtype == (np.complex64 if dtype == np.float32 else np.complex128)
    re, im = spec.real, spec.imag
    mag = np.sqrt(re * re + im * im + dtype.type(MAG_EPS))
    mel = np.einsum("ms,nts->ntm", melfb, mag)
    out = np.log(np.maximum(mel, dtype.type(MEL_FLOOR)))
    assert out.dtype == dtype
    return out


def log_mel_ragged(y, lengths, melfb=None, dtype=np.float64) -> np.ndarray:
    """Row b is its first lengths[b] samples run alone; frames past its own count hold log(1e-5)."""
    y = np.asarray(y)
    T = max(num_frames(int(n)) for n in lengths)
    nm = (slaney_filterbank() if melfb is None else np.asarray(melfb)).shape[0]
    out = np.full((y.shape[0], T, nm), np.log(np.dtype(dtype).type(MEL_FLOOR)), dtype=dtype)
    for b, n in enumerate(lengths):
        m = log_mel(y[b : b + 1, : int(n)], melfb, dtype=dtype)[0]
        out[b, : m.shape[0]] = m
    return out
