"""Test-side restatement of the HiFi-GAN discriminators' forward pass and the three losses on torch's own CPU operators.

Written from the architecture table of include/vtts_disc.h; it carries no text of the reference.  tools/make_disc_golden.py
asserts, at mint time, that it agrees with the reference's modules to 1e-12 in fp64; tests/test_disc_cpu.py holds it to the minted
fixture.  dtype-generic (torch.float64 for expectations, torch.float32 for the arithmetic-class yardstick), CPU only.

``params``: ``{key: (w [Cout, Cin / groups, k], b [Cout])}`` effective weights, keys as in the C ABI
("mpd.discriminators.0.convs.3"), as ``viettts_amd.hifigan.discriminators.fold_checkpoint`` returns them.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

PERIODS = (2, 3, 5, 7, 11)
SLOPE = 0.1
# (cin, cout, k, stride, pad, groups)
MPD_CONVS = ((1, 32, 5, 3, 2, 1), (32, 128, 5, 3, 2, 1), (128, 512, 5, 3, 2, 1), (512, 1024, 5, 3, 2, 1), (1024, 1024, 5, 1, 2, 1))
MSD_CONVS = ((1, 128, 15, 1, 7, 1), (128, 128, 41, 2, 20, 4), (128, 256, 41, 2, 20, 16), (256, 512, 41, 4, 20, 16), (512, 1024, 41, 4, 20, 16),
             (1024, 1024, 41, 1, 20, 16), (1024, 1024, 5, 1, 2, 1))
POST = (1024, 1, 3, 1, 1, 1)


def conv_keys():
    """The 54 convolutions in feature-map order: (key, (cin, cout, k, stride, pad, groups))."""
    out = []
    for d in range(5):
        out += [(f"mpd.discriminators.{d}.convs.{i}", s) for i, s in enumerate(MPD_CONVS)] + [(f"mpd.discriminators.{d}.conv_post", POST)]
    for d in range(3):
        out += [(f"msd.discriminators.{d}.convs.{i}", s) for i, s in enumerate(MSD_CONVS)] + [(f"msd.discriminators.{d}.conv_post", POST)]
    return out


def fmap_shapes(T: int):
    """[(C, L, columns)] of the 54 feature maps of a T-sample row."""
    shapes = []
    for p in PERIODS:
        L = -(-T // p)
        for (_, cout, k, s, pad, _) in MPD_CONVS + (POST,):
            L = (L + 2 * pad - k) // s + 1
            shapes.append((cout, L, p))
    L0 = T
    for d in range(3):
        if d:
            L0 = L0 // 2 + 1
        L = L0
        for (_, cout, k, s, pad, _) in MSD_CONVS + (POST,):
            L = (L + 2 * pad - k) // s + 1
            shapes.append((cout, L, 1))
    return shapes


def _t(a, dtype):
    return torch.from_numpy(np.asarray(a)).to(dtype)


def forward(params, y, dtype=torch.float64):
    """y [N, T] -> (scores: 8 tensors [N, L * columns], fmaps: 54 tensors [N, C, L, columns] (MPD) / [N, C, L] (MSD))."""
    y = _t(y, dtype)
    N, T = y.shape
    scores, fmaps = [], []
    with torch.no_grad():
        for d, p in enumerate(PERIODS):
            x = y[:, None, :]
            if T % p:
                x = F.pad(x, (0, p - T % p), mode="reflect")
            x = x.reshape(N, 1, -1, p)
            for i, (_, _, _, s, pad, _) in enumerate(MPD_CONVS):
                w, b = params[f"mpd.discriminators.{d}.convs.{i}"]
                x = F.leaky_relu(F.conv2d(x, _t(w, dtype)[..., None], _t(b, dtype), stride=(s, 1), padding=(pad, 0)), SLOPE)
                fmaps.append(x)
            w, b = params[f"mpd.discriminators.{d}.conv_post"]
            x = F.conv2d(x, _t(w, dtype)[..., None], _t(b, dtype), padding=(1, 0))
            fmaps.append(x)
            scores.append(x.reshape(N, -1))
        x0 = y[:, None, :]
        for d in range(3):
            if d:
                x0 = F.avg_pool1d(x0, 4, 2, padding=2)
            x = x0
            for i, (_, _, _, s, pad, g) in enumerate(MSD_CONVS):
                w, b = params[f"msd.discriminators.{d}.convs.{i}"]
                x = F.leaky_relu(F.conv1d(x, _t(w, dtype), _t(b, dtype), stride=s, padding=pad, groups=g), SLOPE)
                fmaps.append(x)
            w, b = params[f"msd.discriminators.{d}.conv_post"]
            x = F.conv1d(x, _t(w, dtype), _t(b, dtype), padding=1)
            fmaps.append(x)
            scores.append(x.reshape(N, -1))
    return scores, fmaps


def losses(scores, fmaps, B: int):
    """Rows 0 .. B - 1 real, B .. 2 B - 1 generated.  Returns numpy arrays / floats in the tensors' dtype:
    fmap_l1 [54], real [8], fake [8], gens [8] and the totals feature_mpd / feature_msd (factor 2 inside), disc_mpd / disc_msd,
    gen_mpd / gen_msd, feature, disc, gen."""
    l1 = [torch.mean(torch.abs(f[:B] - f[B:])) for f in fmaps]
    real = [torch.mean((1 - s[:B]) ** 2) for s in scores]
    fake = [torch.mean(s[B:] ** 2) for s in scores]
    gen = [torch.mean((1 - s[B:]) ** 2) for s in scores]
    out = {"fmap_l1": torch.stack(l1).numpy(), "real": torch.stack(real).numpy(), "fake": torch.stack(fake).numpy(), "gens": torch.stack(gen).numpy()}
    out["feature_mpd"], out["feature_msd"] = (2 * sum(l1[:30])).item(), (2 * sum(l1[30:])).item()
    out["disc_mpd"] = sum(r + g for r, g in zip(real[:5], fake[:5])).item()
    out["disc_msd"] = sum(r + g for r, g in zip(real[5:], fake[5:])).item()
    out["gen_mpd"], out["gen_msd"] = sum(gen[:5]).item(), sum(gen[5:]).item()
    out["feature"] = out["feature_mpd"] + out["feature_msd"]
    out["disc"] = out["disc_mpd"] + out["disc_msd"]
    out["gen"] = out["gen_mpd"] + out["gen_msd"]
    return out


LOSS_NAMES = ("feature_mpd", "feature_msd", "disc_mpd", "disc_msd", "gen_mpd", "gen_msd", "feature", "disc", "gen")


def make_inputs(B: int, T: int, seed: int):
    """The fixture's inputs: y ~ 0.2 N(0, 1) clipped to [-1, 1], y_hat = y + 0.05 N(0, 1); one float32 [2 B, T] array, real rows first."""
    rng = np.random.default_rng(seed)
    y = np.clip(0.2 * rng.standard_normal((B, T)), -1.0, 1.0)
    y_hat = y + 0.05 * rng.standard_normal((B, T))
    return np.concatenate([y, y_hat]).astype(np.float32)
