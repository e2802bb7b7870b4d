"""The generator configurations the tests run beyond V1 / TINY / TINY2: one entry per kind of architecture ``vtts_hifigan_create()`` accepts
that routes its layers differently (engine.hip: run_layer, route_f32, route_bf16, plan_pass; DESIGN.md §6u has the route of every layer).
Shared by tests/test_gen_configs_cpu.py (planning, the oracle's transposed convolution, the fp32 yardstick) and
tests/test_gpu_gen_configs.py (the engines against the fp64 oracle).

Every entry says which engines must accept it, what the refusing engines' error must name, and the frame counts T it is run at.  Weights are
``synthetic_params(cfg, seed, "scaled")``, mels ``synthetic_mel(B, T, mel_seed(T), cfg.num_mels)``; the fp64 oracle of an (entry, T) is
computed once per process and never modified."""
from __future__ import annotations

import dataclasses
import functools
from dataclasses import dataclass
from typing import Dict, Tuple

import numpy as np

from oracle import hifigan_oracle as orc
from viettts_amd.hifigan.config import TINY, TINY2, V1, HifiganConfig
from viettts_amd.hifigan.synth import synthetic_mel, synthetic_params
from viettts_amd.hifigan.weights import conv_specs

ENGINES = ("f32", "bf16x3", "bf16")
TIGHT = 2e-5  # tests/test_gpu_parity.py: what the fp32 kernels meet against the fp64 oracle
BATCH = 2  # utterances of the oracle runs


@dataclass(frozen=True)
class Entry:
    name: str
    cfg: HifiganConfig
    frames: Tuple[int, ...]
    refusals: Dict[str, str] = dataclasses.field(default_factory=dict)  # engine -> a substring of vtts_last_error()
    seed: int = 4321
    reaches: str = ""

    @property
    def accepts(self):
        return tuple(e for e in ENGINES if e not in self.refusals)


_PRE = "no kernel for module generator/~/conv1_d (%d->%d"  # the bf16 engine's conv_pre tile is (8..128 mels in steps of 8) -> 512, k = 7


def _v1(**kw):
    return dataclasses.replace(V1, **kw)


TABLE = (
    Entry("V1_NK1", _v1(resblock_kernel_sizes=(7,), resblock_dilation_sizes=((1, 3, 5),)), (3, 13), reaches="an MRF of one ResBlock"),
    Entry("V1_NK2", _v1(resblock_kernel_sizes=(3, 11), resblock_dilation_sizes=((1, 3, 5), (2, 4, 1))), (3, 13),
          reaches="fp32 parallel chains at nk = 2; another dilation order"),
    Entry("V1_NK4", _v1(resblock_kernel_sizes=(3, 7, 11, 3), resblock_dilation_sizes=((1, 3, 5), (1, 3, 5), (1, 3, 5), (2, 4, 1))), (3, 13),
          reaches="nk = 4 (VTTS_MAX_KERNELS); mean by 1/4; two ResBlocks of one class in a stage"),
    Entry("V1_DIL", _v1(resblock_dilation_sizes=((1, 3, 9), (1, 3, 5), (2, 6, 4))), (3, 13),
          {"bf16": "no kernel for module generator/~/res_block1_0/~/convs1_2"}, reaches="a generic convolution inside MFMA ResBlocks"),
    Entry("V1_K", _v1(resblock_kernel_sizes=(3, 5, 13)), (3, 13), {"bf16": "no kernel for module generator/~/res_block1_1/~/convs1_0"},
          reaches="k = 5 and 13 generic beside k = 3 MFMA"),
    Entry("V1_MEL8", _v1(num_mels=8), (3, 13), reaches="conv_pre routes: 8 mels"),
    Entry("V1_MEL64", _v1(num_mels=64), (3, 13), reaches="conv_pre routes: 64 mels"),
    Entry("V1_MEL128", _v1(num_mels=128), (3, 13), reaches="conv_pre routes: 128 mels, the bf16 tile's full width"),
    Entry("V1_MEL100", _v1(num_mels=100), (3, 13), {"bf16": _PRE % (100, 512)}, reaches="conv_pre routes: no multiple of 8"),
    Entry("HALF", _v1(upsample_initial_channel=256), (5, 6, 8, 13), {"bf16": _PRE % (80, 256)},
          reaches="MFMA tiles at other stages; generic ups_1 / ups_3; C = 16; the generic tanh conv_post"),
    Entry("V3", HifiganConfig(resblock="2", upsample_rates=(8, 8, 4), upsample_kernel_sizes=(16, 16, 8), upsample_initial_channel=256,
                              resblock_kernel_sizes=(3, 5, 7), resblock_dilation_sizes=((1, 2), (2, 6), (3, 12))), (3, 13),
          {"bf16": _PRE % (80, 256)}, reaches="three stages; ResBlock2 on MFMA channel counts; dilation 12; ups_2 with k = 2s and no tile"),
    Entry("DEEP8", HifiganConfig(upsample_rates=(2,) * 8, upsample_kernel_sizes=(4,) * 8, upsample_initial_channel=256,
                                 resblock_kernel_sizes=(3, 7), resblock_dilation_sizes=((1, 3, 5), (1, 2, 4))), (5, 6, 13),
          {"bf16": _PRE % (80, 256)}, reaches="L = 2T parity switch at C = 128; TileUp2 / TileUp3 at other lengths; C down to 1; eight stages"),
    Entry("ODD", HifiganConfig(num_mels=20, upsample_rates=(3, 5, 2), upsample_kernel_sizes=(3, 7, 5), upsample_initial_channel=24,
                               resblock_kernel_sizes=(3, 5), resblock_dilation_sizes=((1, 2, 3), (1, 1, 7))), (1, 5, 9),
          {"bf16": _PRE % (20, 24)}, reaches="pad_a = k - 1; odd k - s; Cout 12 / 6 / 3; every L odd"),
    Entry("ONE", HifiganConfig(upsample_rates=(4,), upsample_kernel_sizes=(8,), upsample_initial_channel=64), (3, 13),
          {"bf16": _PRE % (80, 64)}, reaches="one stage; C = 32 ResBlocks right behind ups_0; conv_post_fast at 32 -> 1"),
)
BY_NAME = {e.name: e for e in TABLE}
for _e in TABLE:
    _e.cfg.validate()


def cases(engines=ENGINES):
    """(entry, engine) for every engine of `engines` that must accept the entry."""
    return [(e, eng) for e in TABLE for eng in engines if eng in e.accepts]


def case_id(c):
    return f"{c[0].name}-{c[1]}"


def mel_seed(T: int) -> int:
    return 700 + T


@functools.lru_cache(maxsize=None)
def params(name: str):
    e = BY_NAME[name]
    return synthetic_params(e.cfg, e.seed, "scaled")


@functools.lru_cache(maxsize=None)
def mel(name: str, T: int, B: int = BATCH):
    m = synthetic_mel(B, T, mel_seed(T), BY_NAME[name].cfg.num_mels)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def oracle(name: str, T: int):
    """fp64 oracle of entry `name` on mel(name, T): (waveform [B, hop T], pre-tanh [B, hop T], {tap: [B, L, C]}), read-only."""
    e = BY_NAME[name]
    taps = []
    y, pre = orc.generator_forward(params(name), mel(name, T), e.cfg, np.float64, return_pre_tanh=True, taps=taps)
    out = (y[..., 0], pre[..., 0], {k: v for k, v in taps if not k.startswith("res_block")})
    for a in (out[0], out[1], *out[2].values()):
        a.setflags(write=False)
    return out


def tap_names(cfg: HifiganConfig):
    return ["conv_pre"] + [f"{t}_{i}" for i in range(cfg.num_upsamples) for t in ("ups", "mrf")]


def signature(s):
    return (s.kind, s.cin, s.cout, s.k, s.dilation, s.stride)


def new_layers():
    """{entry name: [ConvSpec]}: per entry, one module for every signature (kind, Cin, Cout, k, dilation, stride) that neither V1, TINY, TINY2
    nor an earlier entry of the table contains.  conv_pre (time-major input) and conv_post (tanh) count as kinds of their own."""
    def sig(s):
        role = {"generator/~/conv1_d": "pre", "generator/~/conv1_d_1": "post"}.get(s.key, s.kind)
        return (role,) + signature(s)[1:]

    seen = {sig(s) for cfg in (V1, TINY, TINY2) for s in conv_specs(cfg)}
    out = {}
    for e in TABLE:
        mine = []
        for s in conv_specs(e.cfg):
            g = sig(s)
            if g not in seen:
                seen.add(g)
                mine.append(s)
        out[e.name] = mine
    return out
