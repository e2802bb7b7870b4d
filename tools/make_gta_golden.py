"""Mint tests/golden/nat_gta_golden.npz: the TEACHER-FORCED acoustic pass as the REFERENCE'S OWN program computes it.

    python tools/make_gta_golden.py --reference /path/to/NTT123-vietTTS-checkout [--out tests/golden/nat_gta_golden.npz]

Needs a checkout of the reference at mint time only; nothing of it is copied, and no test reads it.  What is EXECUTED is the
reference's ``vietTTS/nat/model.py::AcousticModel(is_training=False).__call__`` (model.py:146-169), imported from the checkout,
with ``oracle/haiku_shim.py`` standing in for haiku / jax (as oracle/make_nat_golden.py does for the inference side).  The shim
has no ``jax.random.bernoulli``; it is added here at run time as ``uniform(key, shape) < float32(p)`` on the shim's classic
threefry layout.  The shim's ``jnp.arange`` is numpy's, whose int64 ruler (model.py:103) would promote an fp32 run to fp64 from
the upsampling on; it is replaced for each run by one that returns the run's float type, as JAX's promotion does, and the
zoneout masks are handed out as 0 / 1 in that type for the same reason (model.py:158's ``1 - m``), so that the "fp32 run" is
fp32 throughout (asserted on the outputs' dtype).
The checkpoint is ``synthetic_acoustic_checkpoint()`` with the rng key of oracle/make_nat_golden.py.

What is RESTATED instead of executed are three lines of ``vietTTS/nat/gta.py`` (its imports need a TextGrid loader and tqdm):
  * gta.py:34-36  the one-frame shift of the target mels      -> tests/_gta_oracle.shift_right
  * gta.py:37     durations in frames = seconds * sample_rate / (n_fft // 4), in fp32, nothing rounded
  * gta.py:75-76  the crop ``mel[idx, :wav_length // hop].T`` -> checked by the CPU test of viettts_amd/nat/gta.py
and gta.py:29-32 (``MelFilter(wavs / 2**15)``) is tests/_mel_oracle.py, itself pinned to the reference's MelFilter by
tools/make_mel_golden.py.

Nothing is written unless ``tests/_gta_oracle.py`` agrees with the executed reference to 1e-12 in fp64 on every case.

Cases (all from three seeded utterances; ``*_mel1`` / ``*_mel2`` = the two return values, fp64; ``*_err_ref32`` = max |the
reference's fp32 run - its fp64 run| over both, the yardstick of tests/test_gpu_gta.py):
  a_   B = 3, tokens padded to 24 (token 0, duration 0) from true lengths 24 / 17 / 11, 40 frames, ``lengths = 24`` for every row:
       the reference-padding case (the corpus run of gta.py).  Also the int16 ``a_wavs [3, 40 * 256]`` (zero past ``a_wav_lengths``)
       whose fp64 log-mel, cast to fp32, IS ``a_mels``.
  b0_ b1_ b2_   the same utterances each run ALONE, unpadded, at its own frame count wav_length // 256, masks drawn at (1, F_row)
  c_   utterance 1 with a single frame
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))
import _gta_oracle as G  # noqa: E402
import _mel_oracle as M  # noqa: E402

RNG_KEY = np.array([0x1234ABCD, 0x0F1E2D3C], dtype=np.uint32)  # oracle/make_nat_golden.py's
SR, HOP, L, F = 16000, 256, 24, 40
TRUE_LEN = (24, 17, 11)
WAV_LEN = (F * HOP, 31 * HOP + 77, 23 * HOP + 200)


def make_inputs():
    rng = np.random.default_rng(20261017)
    tokens = np.zeros((3, L), np.int32)
    dur_s = np.zeros((3, L), np.float32)
    S = F * HOP
    t = np.arange(S) / SR
    wavs = np.zeros((3, S), np.int16)
    for b, n in enumerate(TRUE_LEN):
        tokens[b, :n] = rng.integers(4, 90, size=n)
        tokens[b, 0] = tokens[b, n - 1] = 0  # sil
        w = rng.uniform(0.3, 1.7, size=n)
        dur_s[b, :n] = (w / w.sum() * (WAV_LEN[b] / SR)).astype(np.float32)
        f0 = rng.uniform(100.0, 220.0)
        x = sum(np.sin(2.0 * np.pi * f0 * h * t + rng.uniform(0, 2 * np.pi)) / h for h in range(1, 25))
        x = 0.25 * x / np.abs(x).max() + rng.normal(0.0, 0.003, size=S)
        wavs[b, : WAV_LEN[b]] = np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16)[: WAV_LEN[b]]
    return tokens, dur_s, wavs


def load_reference(reference: Path):
    from oracle import haiku_shim as shim
    from oracle import nat_oracle as O

    mods = shim.install()
    # (values 0 / 1 in the run's float type, not bool: numpy would promote model.py:158's ``1 - m`` to int64 and the state to fp64)
    mods["jax.random"].bernoulli = lambda key, p, shape: (O.jax_legacy_uniform(key, int(np.prod(shape))) < np.float32(p)).reshape(shape).astype(shim._DTYPE[0])
    for m in [k for k in sys.modules if k == "vietTTS" or k.startswith("vietTTS.")]:
        del sys.modules[m]  # the repository's drop-in package of the same name must not shadow the reference
    sys.path.insert(0, str(reference))
    import haiku as hk
    import vietTTS.nat.model as ref_model
    from vietTTS.nat.config import AcousticInput

    assert Path(ref_model.__file__).resolve().is_relative_to(reference.resolve()), ref_model.__file__
    net = hk.transform_with_state(lambda x: ref_model.AcousticModel(is_training=False)(x))
    return shim, net, AcousticInput


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, type=Path, help="checkout of NTT123/vietTTS")
    ap.add_argument("--out", type=Path, default=REPO / "tests" / "golden" / "nat_gta_golden.npz")
    a = ap.parse_args()

    from viettts_amd.nat.synth import synthetic_acoustic_checkpoint

    params, state = synthetic_acoustic_checkpoint()
    tokens, dur_s, wavs = make_inputs()
    dur_f = (dur_s * np.float32(SR) / np.float32(HOP)).astype(np.float32)  # gta.py:37, fp32
    mels = M.log_mel(wavs.astype(np.float64) / 32768.0, dtype=np.float64).astype(np.float32)  # gta.py:29-32
    assert mels.shape == (3, F, 80)
    shim, net, AcousticInput = load_reference(a.reference)

    jnp = sys.modules["jax.numpy"]

    def run_reference(tok, lens, dur, mel, dtype):
        shim.set_dtype(dtype)
        # JAX promotes int32 (op) float32 to float32; numpy, which backs the shim, to float64 — model.py:103's integer ruler would silently turn
        # everything behind the upsampling into an fp64 run.  For the run's duration arange hands out the run's own float type instead.
        jnp.arange = lambda *args, **kw: np.arange(*args, **kw).astype(dtype)
        cast = lambda d: {k: {n: (np.asarray(v).astype(dtype) if np.asarray(v).dtype.kind == "f" else v) for n, v in d[k].items()} for k in d}
        inp = AcousticInput(phonemes=tok, lengths=lens, durations=dur.astype(dtype), wavs=None, wav_lengths=None, mels=G.shift_right(mel.astype(dtype)))
        (m1, m2), _ = net.apply(cast(params), cast(state), RNG_KEY, inp)
        assert net.last_rng_draws == 6, net.last_rng_draws
        assert m1.dtype == dtype and m2.dtype == dtype
        return np.asarray(m1), np.asarray(m2)

    out = {"rng_key": RNG_KEY, "a_wavs": wavs, "a_wav_lengths": np.array(WAV_LEN, np.int32), "true_lengths": np.array(TRUE_LEN, np.int32)}

    def case(prefix, tok, lens, dur, mel):
        B, Fc = mel.shape[:2]
        r64 = run_reference(tok, lens, dur, mel, np.float64)
        r32 = run_reference(tok, lens, dur, mel, np.float32)
        keep, zone = G.haiku_teacher_masks(RNG_KEY, B, Fc)
        ours = G.teacher_forced(params, state, tok, lens, dur, mel, keep, zone, np.float64)
        d = max(float(np.abs(ours[i] - r64[i]).max()) for i in range(2))
        err32 = max(float(np.abs(r32[i].astype(np.float64) - r64[i]).max()) for i in range(2))
        print(f"{prefix}: B {B}, L {tok.shape[1]}, F {Fc}: restatement vs executed reference {d:.2e}; reference fp32 vs fp64 {err32:.2e}; max |mel2| {np.abs(r64[1]).max():.3f}")
        if not d <= 1e-12:
            raise SystemExit(f"{prefix}: tests/_gta_oracle.py disagrees with the executed reference ({d:.3e} > 1e-12): nothing written")
        out.update({prefix + "tokens": tok.astype(np.int32), prefix + "lengths": np.asarray(lens, np.int32), prefix + "durations_frames": dur.astype(np.float32),
                    prefix + "mels": mel.astype(np.float32), prefix + "mel1": r64[0], prefix + "mel2": r64[1], prefix + "err_ref32": np.float64(err32)})

    case("a_", tokens, np.full(3, L, np.int32), dur_f, mels)
    for b, n in enumerate(TRUE_LEN):
        Fb = WAV_LEN[b] // HOP
        case(f"b{b}_", tokens[b : b + 1, :n], np.array([n], np.int32), dur_f[b : b + 1, :n], mels[b : b + 1, :Fb])
    case("c_", tokens[1:2, : TRUE_LEN[1]], np.array([TRUE_LEN[1]], np.int32), dur_f[1:2, : TRUE_LEN[1]], mels[1:2, :1])
    np.savez_compressed(a.out, **out)
    print(f"wrote {a.out}: {a.out.stat().st_size} bytes")


if __name__ == "__main__":
    main()
