"""Deterministic synthetic discriminator checkpoints, in the style of ``synth.synthetic_params``.

No pretrained ``do_*`` file exists offline, so parity and timing runs use seeded random weights of the real architecture, in the
key styles torch writes: every convolution of MPD and of MSD scales 1 and 2 under (old-style) weight norm, MSD scale 0 under
spectral norm.  One CPU ``torch.Generator``; modules in the C ABI's order (MPD periods, then MSD scales; convs then conv_post);
per module first the direction tensor, then the gain (or u, v), then the bias:

  weight_v / weight_orig  ~ N(0, 2 / fan_in),  fan_in = (Cin / groups) * k
  weight_g                ~ U[0.5, 1.5)         one per output channel: the effective row norm
  bias                    ~ N(0, 0.01^2)
  weight_u, weight_v      (spectral norm) ``SN_ITERS`` power iterations in fp64 from a seeded N(0, 1) start, stored as float32.
                          A random u, v pair makes sigma = u . (W v) tiny and the scale's activations grow to ~1e12 by its last
                          layer; converged vectors give the matrix's largest singular value, as a trained checkpoint holds.
"""
from __future__ import annotations

import math

import torch

SN_ITERS = 30

# (cin, cout, k, groups) per convolution
MPD_CONVS = ((1, 32, 5, 1), (32, 128, 5, 1), (128, 512, 5, 1), (512, 1024, 5, 1), (1024, 1024, 5, 1), (1024, 1, 3, 1))
MSD_CONVS = ((1, 128, 15, 1), (128, 128, 41, 4), (128, 256, 41, 16), (256, 512, 41, 16), (512, 1024, 41, 16), (1024, 1024, 41, 16),
             (1024, 1024, 5, 1), (1024, 1, 3, 1))


def _names(n_convs: int):
    return [f"convs.{i}" for i in range(n_convs - 1)] + ["conv_post"]


def synthetic_disc_checkpoint(seed: int = 8642) -> dict:
    """``{"mpd": state_dict, "msd": state_dict}`` — the shape of upstream's ``do_*`` file (its optimiser entries left out)."""
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    mpd, msd = {}, {}
    for d in range(5):
        for name, (cin, cout, k, groups) in zip(_names(6), MPD_CONVS):
            base = f"discriminators.{d}.{name}"
            fan = (cin // groups) * k
            mpd[base + ".weight_v"] = torch.randn((cout, cin // groups, k, 1), generator=g) * math.sqrt(2.0 / fan)
            mpd[base + ".weight_g"] = 0.5 + torch.rand((cout, 1, 1, 1), generator=g)
            mpd[base + ".bias"] = torch.randn((cout,), generator=g) * 0.01
    for d in range(3):
        for name, (cin, cout, k, groups) in zip(_names(8), MSD_CONVS):
            base = f"discriminators.{d}.{name}"
            fan = (cin // groups) * k
            w = torch.randn((cout, cin // groups, k), generator=g) * math.sqrt(2.0 / fan)
            if d == 0:
                wm = w.double().reshape(cout, -1)
                u = torch.randn((cout,), generator=g).double()
                u = u / u.norm()
                for _ in range(SN_ITERS):
                    v = wm.t() @ u
                    v = v / v.norm()
                    u = wm @ v
                    u = u / u.norm()
                msd[base + ".weight_orig"] = w
                msd[base + ".weight_u"] = u.float()
                msd[base + ".weight_v"] = v.float()
            else:
                msd[base + ".weight_v"] = w
                msd[base + ".weight_g"] = 0.5 + torch.rand((cout, 1, 1), generator=g)
            msd[base + ".bias"] = torch.randn((cout,), generator=g) * 0.01
    return {"mpd": mpd, "msd": msd}
