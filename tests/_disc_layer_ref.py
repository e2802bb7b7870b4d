"""One discriminator layer at a time on torch's own CPU operators, the comparison tests/test_gpu_disc_layers.py holds the kernels to, and the
loss reduction's yardstick (CPU only).

tests/_disc_oracle.py runs the whole chain; a deep layer compared through it carries every earlier layer's error.  Here layer i is computed
alone, from the input the kernel itself read (the GPU's own feature map i - 1, or the waveform), in fp64 for the expectation and in fp32 for the
arithmetic-class yardstick.  tests/test_disc_tiles_cpu.py holds layer_reference() to the oracle's chain and checks that the comparison fails
when it should.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import _disc_oracle as oracle
import _disc_tiles as tiles

EPS = 2.0 ** -22


def layer_reference(params, i: int, x, dtype):
    """Feature map i of `x` alone.  x: the waveforms [N, T] for a first layer, else the previous layer's map ([N, C, L, p] MPD, [N, C, L] MSD).
    The layer includes what its kernel includes: the reflect pad and reshape (MPD first), the scale's nested average pools (MSD first),
    LeakyReLU except after conv_post."""
    ly = tiles.layers()[i]
    key, (_, _, _, s, pad, g) = oracle.conv_keys()[i]
    w, b = (torch.from_numpy(np.asarray(a)).to(dtype) for a in params[key])
    x = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)
    with torch.no_grad():
        if ly["kind"] == "mpd_first":
            N, T = x.shape
            p = ly["p"]
            x = x[:, None, :]
            if T % p:
                x = F.pad(x, (0, p - T % p), mode="reflect")
            x = x.reshape(N, 1, -1, p)
        elif ly["kind"] == "msd_first":
            x = x[:, None, :]
            for _ in range(ly["disc"] - 5):
                x = F.avg_pool1d(x, 4, 2, padding=2)
        if ly["disc"] < 5:
            y = F.conv2d(x, w[..., None], b, stride=(s, 1), padding=(pad, 0))
        else:
            y = F.conv1d(x, w, b, stride=s, padding=pad, groups=g)
        if ly["kind"] != "post":
            y = F.leaky_relu(y, oracle.SLOPE)
    return y.numpy()


def compare_layer(got, ref64, ref32, post: bool = False):
    """The bar of one layer, over every element:  max|got - fp64| / max|fp64|  <=  4 e32 + 2^-22,  e32 = max|fp32 - fp64| / max|fp64|;
    conv_post, which accumulates in double and rounds once: <= 2^-22 alone.  Every element must be finite (the buffers start as NaN).
    Returns (ok, err, e32, bound)."""
    got, ref64, ref32 = (np.asarray(a, dtype=np.float64) for a in (got, ref64, ref32))
    assert got.shape == ref64.shape == ref32.shape, (got.shape, ref64.shape, ref32.shape)
    scale = float(np.abs(ref64).max())
    e32 = float(np.abs(ref32 - ref64).max()) / scale
    bound = EPS if post else 4.0 * e32 + EPS
    if not np.isfinite(got).all():
        return False, float("nan"), e32, bound
    err = float(np.abs(got - ref64).max()) / scale
    return err <= bound, err, e32, bound


def loss_yardstick(fmaps, scores, B: int):
    """The 87 results of include/vtts_disc.h's layout from 54 maps and 8 scores of 2 B rows (float32 arrays, real rows first): the element
    arithmetic in numpy float32 as the reference's fp32 tensors do it, every sum and mean in fp64, the totals as _disc_oracle.losses sums them."""
    one = np.float32(1.0)
    l1 = [np.abs(f[:B] - f[B:]).astype(np.float64).mean() for f in fmaps]
    real = [np.square(one - s[:B]).astype(np.float64).mean() for s in scores]
    fake = [np.square(s[B:]).astype(np.float64).mean() for s in scores]
    gen = [np.square(one - s[B:]).astype(np.float64).mean() for s in scores]
    for f in list(fmaps) + list(scores):
        assert f.dtype == np.float32
    f_mpd, f_msd = 2 * sum(l1[:30]), 2 * sum(l1[30:])
    d_mpd, d_msd = sum(r + g for r, g in zip(real[:5], fake[:5])), sum(r + g for r, g in zip(real[5:], fake[5:]))
    g_mpd, g_msd = sum(gen[:5]), sum(gen[5:])
    return np.array(l1 + real + fake + gen + [f_mpd, f_msd, d_mpd, d_msd, g_mpd, g_msd, f_mpd + f_msd, d_mpd + d_msd, g_mpd + g_msd], dtype=np.float64)
