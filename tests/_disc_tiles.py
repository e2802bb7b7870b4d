"""Launch geometry of the discriminator kernels (viettts_amd/csrc/disc.hip), restated for tests/test_gpu_disc_layers.py (no GPU; torch only
through tests/_disc_oracle.py's shape arithmetic, imported when a function needs it).

A row of a layer's output is Nout = L * p flat positions (p = the period's columns for MPD, 1 for MSD), cut into tiles of NT positions by
blockIdx.x.  Where a row meets a tile edge is where the kernels' guards and index arithmetic can go wrong: the last tile's `n < Nout` store guard,
the `Nout > 64` switch between two template instances of the wide classes, and, for the periods 3, 5, 7 and 11, a second tile that starts in
mid-row (NT is no multiple of p, so jrel0 != 0; that case exists only where Nout > NT).  targets() names, for each of the 54 layers and each tile
width of its class, the two row lengths that sit on the edge; cover() finds sample counts T that produce them.
tests/test_disc_tiles_cpu.py reads the same numbers out of disc.hip and fails when the source moves one.
"""
from __future__ import annotations

from functools import lru_cache

PERIODS = (2, 3, 5, 7, 11)
MIN_T = 11  # VTTS_DISC_MIN_SAMPLES

# disc_conv_k: vtts_disc_forward's launch_gemm<WM, WN, MW, NW, M16> per class, keyed by Cout / group (512 stands for `cout_g >= 512`).
# Two entries: (Nout > WIDE_SWITCH, otherwise); one entry: the class has one instance.
GEMM_LAUNCH = {
    512: ((4, 1, 2, 4, False), (4, 1, 2, 2, False)),
    128: ((4, 1, 1, 4, False), (4, 1, 1, 2, False)),
    64: ((2, 2, 1, 2, False),),
    32: ((1, 4, 1, 2, False),),
    16: ((1, 4, 1, 2, True),),
}
WIDE_SWITCH = 64   # `const bool wide = Nout > 64`
FIRST_BLOCK = 256  # positions per workgroup of mpd_first_k and msd_first_k
POST_BLOCK = 64    # positions per workgroup of disc_post_k

# (cin, cout, k, stride, pad, groups) as in include/vtts_disc.h
MPD_CONVS = ((1, 32, 5, 3, 2, 1), (32, 128, 5, 3, 2, 1), (128, 512, 5, 3, 2, 1), (512, 1024, 5, 3, 2, 1), (1024, 1024, 5, 1, 2, 1))
MSD_CONVS = ((1, 128, 15, 1, 7, 1), (128, 128, 41, 2, 20, 4), (128, 256, 41, 2, 20, 16), (256, 512, 41, 4, 20, 16), (512, 1024, 41, 4, 20, 16),
             (1024, 1024, 41, 1, 20, 16), (1024, 1024, 5, 1, 2, 1))
POST = (1024, 1, 3, 1, 1, 1)


def gemm_nt(args) -> int:
    """NT = WN * NW * 32 of a launch_gemm instance"""
    _, wn, _, nw, _ = args
    return wn * nw * 32


def gemm_class(cout_g: int) -> int:
    return 512 if cout_g >= 512 else cout_g


@lru_cache(maxsize=None)
def layers():
    """The 54 layers in feature-map order: dicts with index, disc (0 .. 7), layer (index within the discriminator), kind ("mpd_first", "msd_first",
    "gemm", "post"), p, the convolution's (cin, cout, k, stride, pad, groups), cls (the tile class's name) and widths (its tile widths NT)."""
    out = []
    for d in range(8):
        convs = (MPD_CONVS if d < 5 else MSD_CONVS) + (POST,)
        for j, spec in enumerate(convs):
            cin, cout, k, s, pad, g = spec
            if j == 0:
                kind, cls, widths = ("mpd_first" if d < 5 else "msd_first"), "first", (FIRST_BLOCK,)
            elif j == len(convs) - 1:
                kind, cls, widths = "post", "post", (POST_BLOCK,)
            else:
                c = gemm_class(cout // g)
                kind, cls, widths = "gemm", f"gemm{c}", tuple(sorted({gemm_nt(a) for a in GEMM_LAUNCH[c]}))
            out.append(dict(index=len(out), disc=d, layer=j, kind=kind, p=PERIODS[d] if d < 5 else 1, spec=spec, cls=cls, widths=widths))
    return tuple(out)


def launched_nt(layer: dict, nout: int) -> int:
    """positions per workgroup of the instance vtts_disc_forward launches for a row of nout positions"""
    if layer["kind"] != "gemm":
        return layer["widths"][0]
    inst = GEMM_LAUNCH[gemm_class(layer["spec"][1] // layer["spec"][5])]
    return gemm_nt(inst[0] if len(inst) == 1 or nout > WIDE_SWITCH else inst[1])


@lru_cache(maxsize=None)
def _nouts(T: int):
    from _disc_oracle import fmap_shapes

    return tuple(L * p for (_, L, p) in fmap_shapes(T))


def nout(i: int, T: int) -> int:
    return _nouts(T)[i]


def _first_T(i: int, v: int, hi: int = 1 << 22) -> int:
    """the smallest T >= MIN_T whose layer i has at least v positions per row (Nout never falls as T grows)"""
    lo = MIN_T
    assert nout(i, hi) >= v, (i, v)
    while lo < hi:
        mid = (lo + hi) // 2
        if nout(i, mid) >= v:
            hi = mid
        else:
            lo = mid + 1
    return lo


@lru_cache(maxsize=None)
def targets():
    """For each layer and each tile width NT of its class: the largest reachable Nout <= NT ("le") and the smallest reachable Nout > NT ("gt").
    Tuples (layer index, NT, side, Nout, T_lo, T_hi): every T in T_lo .. T_hi gives that layer exactly Nout positions per row."""
    out = []
    for ly in layers():
        i = ly["index"]
        for nt in ly["widths"]:
            t_gt = _first_T(i, nt + 1)            # the first T past the edge
            assert t_gt > MIN_T, (i, nt)          # so the row before the edge exists too
            v_gt, v_le = nout(i, t_gt), nout(i, t_gt - 1)
            out.append((i, nt, "le", v_le, _first_T(i, v_le), t_gt - 1))
            out.append((i, nt, "gt", v_gt, t_gt, _first_T(i, v_gt + 1) - 1))
    return tuple(out)


@lru_cache(maxsize=None)
def cover():
    """A small set of lengths that reaches every target: {T: [(layer index, NT, side, Nout), ...]}, ascending in T.  Greedy from the smallest T
    upward: take the uncovered target whose range of lengths starts first; of the range starts that lie inside its range, the one that serves
    the most uncovered targets (the smallest on a tie) is the next length.  Short lengths first keeps the GPU tests' CPU side small."""
    starts = sorted({t[4] for t in targets()})
    todo = sorted(targets(), key=lambda t: (t[4], t[5]))
    out = {}
    while todo:
        first = todo[0]
        T = max((s for s in starts if first[4] <= s <= first[5]), key=lambda s: (sum(t[4] <= s <= t[5] for t in todo), -s))
        out[T] = [t[:4] for t in todo if t[4] <= T <= t[5]]
        todo = [t for t in todo if not t[4] <= T <= t[5]]
    return dict(sorted(out.items()))
