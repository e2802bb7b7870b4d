"""Mint tests/golden/disc_golden.npz: the HiFi-GAN discriminators' feature maps, scores and losses as the REFERENCE'S OWN modules
compute them in fp64 on seeded synthetic weights.

    python tools/make_disc_golden.py --reference /path/to/NTT123-vietTTS-checkout [--out tests/golden/disc_golden.npz]

Needs a checkout of the reference at mint time only: vietTTS/hifigan/torch_model.py is imported from it by file path; nothing of
it is copied and no test reads it.  Steps, each asserted before anything is written:

  1. viettts_amd.hifigan.disc_synth's checkpoint is loaded into the reference's MultiPeriodDiscriminator / MultiScaleDiscriminator
     (eval mode: spectral norm without a power iteration); the effective weights the modules compute agree with
     viettts_amd.hifigan.discriminators.fold_checkpoint to fp32 rounding.
  2. The norms are removed and the folded fp32 weights put in their place, so that reference and restatement hold the same numbers;
     then tests/_disc_oracle.py == reference in fp64 to 1e-12 of each layer's max-abs, for every feature map, score and loss.

Arrays written (``<T>`` = 11, 37, 2310, 4099 with B = 2, and 16411 with B = 1; rows 0 .. B - 1 real, B .. 2 B - 1 generated):
  weight_seed, shapes [n, 3] (T, B, input seed)
  y_11, y_37                 float32 inputs; the larger ones are remade from their seed (tests/_disc_oracle.make_inputs) and
  ysum_<T>                   pinned by their fp64 sum
  scores_<T>                 float64, the eight score tensors flattened one after the other
  stats_<T>                  float64 [54, 3]: per feature map sum, abs-sum, max-abs
  losses_<T>                 float64 [87]: fmap_l1 [54], real [8], fake [8], gens [8], then _disc_oracle.LOSS_NAMES
  err_ref32_fmap_<T> [54], err_ref32_score_<T> [8], err_ref32_loss_<T> [87]
                             error of the reference's modules run in fp32 on the CPU against their fp64 run: max |diff| over the
                             tensor / the fp64 max-abs (feature maps, scores), relative error (losses) — the arithmetic-class
                             yardstick of tests/test_gpu_disc.py
  fmap37_<i>                 every feature map of T = 37 in full for rows 0 and B, rounded once to float32 (fp64 would not fit the
                             1 MB a committed file may have; the fp64 statistics above cover all rows)
"""
from __future__ import annotations

import argparse
import importlib.util
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))
import _disc_oracle as oracle  # noqa: E402
from viettts_amd.hifigan.disc_synth import synthetic_disc_checkpoint  # noqa: E402
from viettts_amd.hifigan.discriminators import fold_checkpoint  # noqa: E402

WEIGHT_SEED = 8642
SHAPES = ((11, 2, 111), (37, 2, 137), (2310, 2, 12310), (4099, 2, 14099), (16411, 1, 116411))  # (T, B, input seed)


def loss_vector(d) -> np.ndarray:
    return np.concatenate([d["fmap_l1"], d["real"], d["fake"], d["gens"], np.array([d[k] for k in oracle.LOSS_NAMES])]).astype(np.float64)


def reference_modules(reference: Path):
    spec = importlib.util.spec_from_file_location("_reference_torch_model", reference / "vietTTS" / "hifigan" / "torch_model.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def module_of(root, path: str):
    m = root
    for part in path.split("."):
        m = m[int(part)] if part.isdigit() else getattr(m, part)
    return m


def reference_run(mod, mpd, msd, y2, B, dtype):
    y = torch.from_numpy(y2).to(dtype)[:, None, :]
    with torch.no_grad():
        pr, pg, fpr, fpg = mpd(y[:B], y[B:])
        sr, sg, fsr, fsg = msd(y[:B], y[B:])
        fmaps = [torch.cat([r, g]) for dr, dg in zip(fpr + fsr, fpg + fsg) for r, g in zip(dr, dg)]
        scores = [torch.cat([r, g]) for r, g in zip(pr + sr, pg + sg)]
        fm = [mod.feature_loss(fpr, fpg), mod.feature_loss(fsr, fsg)]
        dl = [mod.discriminator_loss(pr, pg), mod.discriminator_loss(sr, sg)]
        gl = [mod.generator_loss(pg), mod.generator_loss(sg)]
        l1 = [torch.mean(torch.abs(r - g)) for dr, dg in zip(fpr + fsr, fpg + fsg) for r, g in zip(dr, dg)]
    d = {"fmap_l1": np.array([float(v) for v in l1]), "real": np.array(dl[0][1] + dl[1][1], dtype=np.float64),
         "fake": np.array(dl[0][2] + dl[1][2], dtype=np.float64), "gens": np.array([float(v) for v in gl[0][1] + gl[1][1]])}
    d["feature_mpd"], d["feature_msd"] = float(fm[0]), float(fm[1])
    d["disc_mpd"], d["disc_msd"] = float(dl[0][0]), float(dl[1][0])
    d["gen_mpd"], d["gen_msd"] = float(gl[0][0]), float(gl[1][0])
    d["feature"], d["disc"], d["gen"] = d["feature_mpd"] + d["feature_msd"], d["disc_mpd"] + d["disc_msd"], d["gen_mpd"] + d["gen_msd"]
    return scores, fmaps, d


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, type=Path, help="checkout of NTT123/vietTTS")
    ap.add_argument("--out", type=Path, default=REPO / "tests" / "golden" / "disc_golden.npz")
    a = ap.parse_args()
    torch.manual_seed(0)
    mod = reference_modules(a.reference)
    ckpt = synthetic_disc_checkpoint(WEIGHT_SEED)
    params = fold_checkpoint(ckpt)
    mpd, msd = mod.MultiPeriodDiscriminator(), mod.MultiScaleDiscriminator()
    mpd.load_state_dict(ckpt["mpd"])
    msd.load_state_dict(ckpt["msd"])
    mpd.eval().double()
    msd.eval().double()
    # 1. the fold: run once so that the norm hooks compute `weight`, then compare
    with torch.no_grad():
        z = torch.zeros(1, 1, 64, dtype=torch.float64)
        mpd(z, z)
        msd(z, z)
    worst = 0.0
    for key, _ in oracle.conv_keys():
        root, path = (mpd, key[4:]) if key.startswith("mpd.") else (msd, key[4:])
        w_ref = module_of(root, path).weight.detach().numpy()
        w_ref = w_ref[..., 0] if w_ref.ndim == 4 else w_ref
        w, _b = params[key]
        worst = max(worst, float(np.abs(w_ref - w).max() / np.abs(w_ref).max()))
    print(f"fold vs the reference's modules (eval): worst max|diff| / max|w| = {worst:.3e}")
    assert worst <= 2.0 ** -23
    # 2. the same numbers on both sides: plain convolutions holding the folded fp32 weights
    for key, _ in oracle.conv_keys():
        root, path = (mpd, key[4:]) if key.startswith("mpd.") else (msd, key[4:])
        m = module_of(root, path)
        if hasattr(m, "weight_orig"):
            torch.nn.utils.remove_spectral_norm(m)
        else:
            torch.nn.utils.remove_weight_norm(m)
        w, b = params[key]
        with torch.no_grad():
            m.weight.copy_(torch.from_numpy(w).double().reshape(m.weight.shape))
            m.bias.copy_(torch.from_numpy(b).double())

    out = {"weight_seed": np.int64(WEIGHT_SEED), "shapes": np.array(SHAPES, dtype=np.int64)}
    for T, B, seed in SHAPES:
        y2 = oracle.make_inputs(B, T, seed)
        mpd.double(), msd.double()
        s_ref, f_ref, l_ref = reference_run(mod, mpd, msd, y2, B, torch.float64)
        s_our, f_our = oracle.forward(params, y2, torch.float64)
        l_our = oracle.losses(s_our, f_our, B)
        worst = 0.0
        for r, o in list(zip(f_ref, f_our)) + list(zip(s_ref, s_our)):
            assert r.shape == o.shape and r.dtype == torch.float64, (r.shape, o.shape)
            worst = max(worst, float((r - o).abs().max() / r.abs().max()))
        lv_ref, lv_our = loss_vector(l_ref), loss_vector(l_our)
        lworst = float(np.abs(lv_ref / lv_our - 1).max())
        print(f"T={T} B={B}: restatement vs reference, feature maps and scores {worst:.2e}, losses {lworst:.2e}")
        assert worst <= 1e-12 and lworst <= 1e-12
        assert [tuple(f.shape[1:]) for f in f_ref] == [(c, l, p) if i < 30 else (c, l) for i, (c, l, p) in enumerate(oracle.fmap_shapes(T))]
        mpd.float(), msd.float()
        s32, f32, l32 = reference_run(mod, mpd, msd, y2, B, torch.float32)
        e_f = np.array([float((x.double() - r).abs().max() / r.abs().max()) for x, r in zip(f32, f_ref)])
        e_s = np.array([float((x.double() - r).abs().max() / r.abs().max()) for x, r in zip(s32, s_ref)])
        e_l = np.abs(loss_vector(l32) / lv_ref - 1)
        print(f"   reference fp32 vs fp64: worst feature map {e_f.max():.2e}, score {e_s.max():.2e}, loss {e_l.max():.2e}")
        if T <= 37:
            out[f"y_{T}"] = y2
        out[f"ysum_{T}"] = np.float64(y2.astype(np.float64).sum())
        out[f"scores_{T}"] = np.concatenate([s.numpy().ravel() for s in s_ref])
        out[f"stats_{T}"] = np.array([[float(f.sum()), float(f.abs().sum()), float(f.abs().max())] for f in f_ref])
        out[f"losses_{T}"] = lv_ref
        out[f"err_ref32_fmap_{T}"], out[f"err_ref32_score_{T}"], out[f"err_ref32_loss_{T}"] = e_f, e_s, e_l
        if T == 37:
            for i, f in enumerate(f_ref):
                out[f"fmap37_{i}"] = f[[0, B]].numpy().astype(np.float32)
    np.savez_compressed(a.out, **out)
    size = a.out.stat().st_size
    print(f"wrote {a.out}: {size} bytes")
    assert size < 1_000_000, "a committed file must stay under 1 MB"


if __name__ == "__main__":
    main()
