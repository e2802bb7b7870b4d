"""Numpy restatement of the reference's TEACHER-FORCED acoustic pass, ``AcousticModel(is_training=False).__call__``
(vietTTS/nat/model.py:146-169), the forward ``vietTTS/nat/gta.py:28-40`` runs to dump ground-truth-aligned mels — built on the
primitives of ``oracle/nat_oracle.py`` (token encoder, Gaussian upsampling, LSTM step, convolution, BatchNorm, the threefry
restatements), in fp64 (the oracle the GPU tests compare against) or fp32.

``tools/make_gta_golden.py`` executes the reference's own ``__call__`` over ``oracle/haiku_shim.py`` and refuses to write
``tests/golden/nat_gta_golden.npz`` unless :func:`teacher_forced` agrees with it to 1e-12 in fp64, so the wiring here — the
one-frame shift, upsampling over all token columns, one dropout draw per prenet layer over the whole batch, zoneout on the
recurrent state but not on the decoder's output, the order of the six rng draws — is pinned to the reference's source, executed.
The third-party primitives are as pinned as ``oracle/nat_oracle.py`` says.

Test infrastructure only.
"""
from __future__ import annotations

import sys
from pathlib import Path
from typing import Optional, Tuple

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from oracle import nat_oracle as O  # noqa: E402

PRE = "acoustic_model"


def shift_right(mels: np.ndarray) -> np.ndarray:
    """gta.py:34-36: the decoder's input at frame f is the target mel of frame f - 1, a zero frame first.  ``mels [..., F, D]``."""
    out = np.zeros_like(mels)
    out[..., 1:, :] = mels[..., :-1, :]
    return out


def haiku_teacher_masks(rng, B: int, F: int, prenet_dim: int = 256, H: int = 512, partitionable: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """The six draws of ``__call__`` from the checkpoint's ``rng`` through ``hk.next_rng_key()`` ((K_n, S_n) = split(K_{n-1})):
    S_1, S_2 the prenet's dropouts (model.py:97,:99: ONE ``uniform < 0.5`` over ``(B, F, prenet_dim)`` each), S_3 .. S_6
    ``bernoulli(0.1, (B, F, H))`` for layer 0 h, layer 0 c, layer 1 h, layer 1 c (model.py:162-165; tree order of the decoder's
    initial state).  Returns ``keep [B, F, 2, prenet_dim]`` and ``zone [B, F, 4, H]`` (True = keep the previous state), bool."""
    key = np.asarray(rng, dtype=np.uint32).reshape(2)
    split, uniform = (O.jax_partitionable_split, O.jax_partitionable_uniform) if partitionable else (O.jax_legacy_split, O.jax_legacy_uniform)
    draws = []
    for d in range(6):
        key, sub = split(key, 2)
        D, p = (prenet_dim, 0.5) if d < 2 else (H, 0.1)
        draws.append((uniform(sub, B * F * D) < np.float32(p)).reshape(B, F, D))
    return np.stack(draws[:2], axis=2), np.stack(draws[2:], axis=2)


def _postnet(P: O.Params, x: np.ndarray) -> np.ndarray:
    y = x
    for i in range(5):  # model.py:113-121 without dropout
        cv = "conv1_d" if i == 0 else f"conv1_d_{i}"
        y = O.conv1d_same(y, P.get(f"{PRE}/~/{cv}", "w"), P.get(f"{PRE}/~/{cv}", "b"))
        if i < 4:
            bn = "batch_norm" if i == 0 else f"batch_norm_{i}"
            y = O.batchnorm_eval(y, P.get(f"{PRE}/~/{bn}", "scale"), P.get(f"{PRE}/~/{bn}", "offset"),
                                 P.get(f"{PRE}/~/{bn}/~/mean_ema", "average", state=True), P.get(f"{PRE}/~/{bn}/~/var_ema", "average", state=True))
            y = np.tanh(y)
    return y


def teacher_forced_row(params, state, tokens, length: int, durations_frames, mels, keep: Optional[np.ndarray] = None,
                       zone: Optional[np.ndarray] = None, dtype=np.float64, return_states: bool = False):
    """One row of the batch: ``tokens [L]`` (ALL L columns are tokens for the convolutions and the upsampling; ``length`` enters
    the backward encoder LSTM's reset mask only, model.py:38), ``durations_frames [L]``, target ``mels [F, mel]``,
    ``keep [F, 2, PN]`` / ``zone [F, 4, H]`` bool or None.  Returns ``(mel1, mel1 + residual)``, each ``[F, mel]``."""
    P = O.Params(params, state, dtype)
    dt = np.dtype(dtype).type
    tokens = np.asarray(tokens, dtype=np.int64)
    mels = np.asarray(mels).astype(dtype)
    F = mels.shape[0]
    x = O.token_encoder(P, f"{PRE}/~/token_encoder", tokens, int(length))  # :147
    cond = O.gaussian_upsample(x, np.asarray(durations_frames).astype(dtype), F)  # :148
    f1, f2 = P.get(f"{PRE}/~/linear_1", "w"), P.get(f"{PRE}/~/linear_2", "w")
    p = np.maximum(shift_right(mels) @ f1, dt(0))  # :149, :95-100
    if keep is not None:
        p = np.where(keep[:, 0], p * dt(2), dt(0))
    p = np.maximum(p @ f2, dt(0))
    if keep is not None:
        p = np.where(keep[:, 1], p * dt(2), dt(0))
    xin = np.concatenate([cond, p], axis=-1)  # :150
    w1, b1 = P.get(f"{PRE}/~/lstm/linear", "w"), P.get(f"{PRE}/~/lstm/linear", "b")
    w2, b2 = P.get(f"{PRE}/~/lstm_1/linear", "w"), P.get(f"{PRE}/~/lstm_1/linear", "b")
    H = b1.shape[0] // 4
    h1 = np.zeros(H, dtype); c1 = np.zeros(H, dtype); h2 = np.zeros(H, dtype); c2 = np.zeros(H, dtype)
    hs = np.empty((F, 2 * H), dtype)
    states = np.empty((F, 4, H), dtype)
    for t in range(F):  # zoneout_decoder (:154-160)
        n1, nc1 = O.lstm_step(xin[t], h1, c1, w1, b1)
        n2, nc2 = O.lstm_step(np.concatenate([xin[t], n1]), h2, c2, w2, b2)  # layer 2 sees layer 1's UN-ZONED output
        hs[t] = np.concatenate([n1, n2])  # ... and so does the projection
        if zone is not None:  # state = m * prev + (1 - m) * new, m in {0, 1}
            h1, c1 = np.where(zone[t, 0], h1, n1), np.where(zone[t, 1], c1, nc1)
            h2, c2 = np.where(zone[t, 2], h2, n2), np.where(zone[t, 3], c2, nc2)
        else:
            h1, c1, h2, c2 = n1, nc1, n2, nc2
        states[t] = np.stack([h1, c1, h2, c2])
    mel1 = hs @ P.get(f"{PRE}/~/linear", "w") + P.get(f"{PRE}/~/linear", "b")  # :167
    out = (mel1, mel1 + _postnet(P, mel1))  # :168-169
    return out + (states,) if return_states else out


def teacher_forced(params, state, tokens, lengths, durations_frames, mels, keep=None, zone=None, dtype=np.float64):
    """The batch ``tokens [B, L]``, ``lengths [B]``, ``durations_frames [B, L]``, ``mels [B, F, mel]``, masks ``[B, F, ...]``:
    rows are independent once the masks are given.  Returns ``(mel1, mel2)``, each ``[B, F, mel]``."""
    rows = [teacher_forced_row(params, state, tokens[b], lengths[b], durations_frames[b], mels[b], None if keep is None else keep[b],
                               None if zone is None else zone[b], dtype) for b in range(len(tokens))]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
