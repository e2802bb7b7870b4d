"""The config table of tests/_gen_configs.py without a GPU: what ``vtts_hifigan_create()`` plans or refuses for every entry and engine, the
oracle's transposed convolution at every (k, stride) of the table against an independent definition, and the fp32 yardstick that shows the
table's inputs are ones where fp32 round-off alone stays inside the GPU tests' bar."""
import ctypes as C

import numpy as np
import pytest
import torch

import _gen_configs as gc
from oracle import hifigan_oracle as orc
from viettts_amd import _lib
from viettts_amd.hifigan.weights import ConvSpec, conv_specs, haiku_weight_to_torch, num_parameters

DTYPES = {"f32": _lib.VTTS_F32, "bf16x3": _lib.VTTS_BF16X3, "bf16": _lib.VTTS_BF16}


@pytest.fixture(scope="module")
def lib():
    from viettts_amd.csrc.build import build

    build()  # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def _create(lib, cfg, engine):
    h = C.c_void_p(0)
    cs = _lib.make_cfg(cfg)
    rc = lib.vtts_hifigan_create(C.byref(cs), 0, DTYPES[engine], C.byref(h))
    return rc, h


@pytest.mark.parametrize("engine", gc.ENGINES)
@pytest.mark.parametrize("entry", gc.TABLE, ids=lambda e: e.name)
def test_create_accepts_or_refuses_as_the_table_says(lib, entry, engine):
    """create() plans without a device.  An accepted entry's inventory (parameter names, shapes, order, hop) is ``conv_specs(cfg)``'s, its packed
    blob is a positive multiple of 256 bytes and every (B, T) of the table has a workspace size; a refused one names the module it has no
    kernel for."""
    rc, h = _create(lib, entry.cfg, engine)
    if engine in entry.refusals:
        assert rc == -1 and not h.value
        msg = lib.vtts_last_error().decode()
        assert entry.refusals[engine] in msg, msg
        return
    assert rc == 0, lib.vtts_last_error()
    try:
        specs = conv_specs(entry.cfg)
        n = C.c_int(0)
        _lib.check(lib, lib.vtts_hifigan_num_params(h, C.byref(n)))
        assert n.value == 2 * len(specs)
        total = 0
        for i in range(n.value):
            key, which = C.c_char_p(), C.c_char_p()
            shape = (C.c_int64 * 3)()
            nd = C.c_int(0)
            _lib.check(lib, lib.vtts_hifigan_param_info(h, i, C.byref(key), C.byref(which), shape, C.byref(nd)))
            s = specs[i // 2]
            want = tuple(s.w_shape) if i % 2 == 0 else (s.cout,)
            assert (key.value.decode(), which.value, tuple(shape[: nd.value])) == (s.key, b"wb"[i % 2 : i % 2 + 1], want)
            total += int(np.prod(want))
        assert total == num_parameters(entry.cfg)
        hop = C.c_int64(0)
        _lib.check(lib, lib.vtts_hifigan_get_option(h, b"hop", C.byref(hop)))
        assert hop.value == entry.cfg.hop
        nb = C.c_size_t(0)
        _lib.check(lib, lib.vtts_hifigan_packed_bytes(h, C.byref(nb)))
        assert nb.value > 0 and nb.value % 256 == 0
        assert nb.value >= total * (2 if engine == "bf16" else 4)  # every weight is in the blob at least once (bf16: conv_post in fp32)
        for B in (1, gc.BATCH, 3):
            for T in entry.frames:
                ws = C.c_size_t(0)
                _lib.check(lib, lib.vtts_hifigan_workspace_bytes(h, B, T, C.byref(ws)))
                assert ws.value > 0 and ws.value % 256 == 0, (B, T)
    finally:
        lib.vtts_hifigan_destroy(h)


def test_table_is_the_issue_s():
    """Every kind of route the table is there for is in it (a row dropped by mistake would otherwise go unnoticed)."""
    names = [e.name for e in gc.TABLE]
    assert names == ["V1_NK1", "V1_NK2", "V1_NK4", "V1_DIL", "V1_K", "V1_MEL8", "V1_MEL64", "V1_MEL128", "V1_MEL100", "HALF", "V3", "DEEP8", "ODD", "ONE"]
    assert [e.name for e in gc.TABLE if "bf16" in e.accepts] == ["V1_NK1", "V1_NK2", "V1_NK4", "V1_MEL8", "V1_MEL64", "V1_MEL128"]
    assert all({"f32", "bf16x3"} <= set(e.accepts) for e in gc.TABLE)
    assert [e.cfg.num_kernels for e in gc.TABLE[:3]] == [1, 2, 4]
    d8 = gc.BY_NAME["DEEP8"]
    assert d8.cfg.num_upsamples == 8 and d8.cfg.stage_channels(7) == 1 and {t % 2 for t in d8.frames} == {0, 1}
    assert {t % 4 for t in gc.BY_NAME["HALF"].frames} >= {0, 1, 2}  # T % 4 == 0: ups_0 on its MFMA tile at stage 0; 1, 2: both parities off it
    new = gc.new_layers()
    assert all(new[e.name] for e in gc.TABLE if e.name not in ("V1_NK1",)), {k: len(v) for k, v in new.items()}  # (V1_NK1 is a subset of V1)


# --------------------------------------------------------------------------------------------------------------------------------
# the oracle's transposed convolution, so far pinned to the reference through the goldens at k == 2 * stride only
# --------------------------------------------------------------------------------------------------------------------------------
def _table_convT_shapes():
    return sorted({(s.k, s.stride) for e in gc.TABLE for s in conv_specs(e.cfg) if s.kind == "convT"})


def _convT_case(k, s, T):
    rng = np.random.default_rng(1000 * k + 10 * s + T)
    B, cin, cout = 2, 3, 2
    return rng.standard_normal((B, T, cin)), rng.standard_normal((k, cout, cin)), rng.standard_normal(cout)


def _brute_conv_transpose(x, w, b, s):
    """hk.Conv1DTranspose(stride=s, padding="SAME") from its definition, in plain fp64 loops: zero-stuff (xd[s t] = x[t]), pad the stuffed
    signal by lax's "SAME" pads for a transposed convolution, correlate without flipping the kernel; w [k, Cout, Cin]."""
    B, T, cin = x.shape
    k, cout, _ = w.shape
    pa, pb = orc.conv_transpose_same_pads(k, s)
    n = (T - 1) * s + 1 + pa + pb
    y = np.zeros((B, n - k + 1, cout))
    for bi in range(B):
        xd = [[0.0] * cin for _ in range(n)]
        for t in range(T):
            for ci in range(cin):
                xd[pa + s * t][ci] = float(x[bi, t, ci])
        for p in range(n - k + 1):
            for co in range(cout):
                acc = float(b[co])
                for j in range(k):
                    for ci in range(cin):
                        acc += float(w[j, co, ci]) * xd[p + j][ci]
                y[bi, p, co] = acc
    return y


def test_table_has_the_transposed_shapes_the_goldens_lack():
    shapes = _table_convT_shapes()
    assert (16, 8) in shapes and (4, 2) in shapes  # k == 2 s: what V1's goldens pin
    assert any(s > k - 1 for k, s in shapes)  # pad_a = k - 1
    assert any((k - s) % 2 == 1 for k, s in shapes)  # odd k - s: the ceil in pad_a
    assert any(k < 2 * s and s <= k - 1 for k, s in shapes) and any(k > 2 * s for k, s in shapes)


@pytest.mark.parametrize("T", [1, 2, 7])
@pytest.mark.parametrize("ks", _table_convT_shapes(), ids=lambda v: f"k{v[0]}s{v[1]}")
def test_oracle_conv_transpose_matches_the_definition(ks, T):
    k, s = ks
    x, w, b = _convT_case(k, s, T)
    got = orc.conv1d_transpose(x, w, b, s)
    want = _brute_conv_transpose(x, w, b, s)
    assert got.shape == want.shape == (2, s * T, 2)
    assert np.abs(got - want).max() < 1e-12
    if (k - s) % 2 == 0:
        # torch's ConvTranspose1d(padding = (k - s) / 2) through the weight relation of the repository's converter (weights.py: w_hk[j, o, i] = w_torch[i, o, k - 1 - j])
        spec = ConvSpec("ups", "ups", "convT", 3, 2, k, 1, s)
        wt = torch.from_numpy(haiku_weight_to_torch(spec, w).copy())
        yt = torch.nn.functional.conv_transpose1d(torch.from_numpy(x).transpose(1, 2), wt, torch.from_numpy(b), stride=s, padding=(k - s) // 2)
        assert np.abs(yt.transpose(1, 2).numpy() - got).max() < 1e-12


@pytest.mark.parametrize("ks", _table_convT_shapes(), ids=lambda v: f"k{v[0]}s{v[1]}")
def test_oracle_conv_transpose_matches_lax(ks):
    """Where jax is installed: ``lax.conv_transpose(padding="SAME")`` itself, called the way hk.Conv1DTranspose calls it (channels-last data, kernel
    [k, Cout, Cin])."""
    jax = pytest.importorskip("jax")
    k, s = ks
    x, w, b = _convT_case(k, s, 7)
    y = jax.lax.conv_transpose(np.asarray(x, np.float32), np.asarray(w, np.float32), (s,), "SAME", dimension_numbers=("NWC", "WOI", "NWC"))
    got = orc.conv1d_transpose(x, w, np.zeros_like(b), s)
    assert np.abs(np.asarray(y, np.float64) - got).max() < 1e-4


# --------------------------------------------------------------------------------------------------------------------------------
# the fp32 yardstick
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", gc.TABLE, ids=lambda e: e.name)
def test_fp32_round_off_stays_inside_the_bar(entry, capsys):
    """The oracle evaluated in fp32 against itself in fp64 on the table's own weights and mels: max|dy| < TIGHT / 4.  fp32 round-off alone (in
    numpy's summation order) uses a quarter of the bar the fp32 engine answers to on these inputs; the rest is the kernels' own order.
    DESIGN.md §6u records the worst value per entry."""
    worst = 0.0
    for T in entry.frames:
        y64, _, _ = gc.oracle(entry.name, T)
        y32 = orc.generator_forward(gc.params(entry.name), gc.mel(entry.name, T), entry.cfg, np.float32)[..., 0]
        assert y32.dtype == np.float32 and y32.shape == y64.shape == (gc.BATCH, entry.cfg.hop * T)
        assert np.abs(y64).max() < 1.0 and np.abs(y64).max() > 1e-3  # a signal, out of tanh's saturation
        worst = max(worst, float(np.abs(y32 - y64).max()))
    with capsys.disabled():
        print(f"\n[{entry.name} fp32 oracle vs fp64 oracle, T in {entry.frames}] worst max|dy| {worst:.3e}")
    assert worst < gc.TIGHT / 4, worst


def test_deep8_five_frames_have_no_interior():
    """DEEP8 at T = 5 against the first five frames of T = 6: tests/test_gpu_parity.py::test_receptive_field_halo's rule compares the samples whose
    receptive field stays clear of the cut.  Here there are none: conv_pre reaches 3 frames and the k = 7 ResBlock of stage 0 another 15
    (3 (d + 1) columns per pair at rates 1, 2, 4, two columns per frame), so every sample of the five frames sees frame 5.  Shown on the
    oracle; the GPU test therefore compares both lengths with the oracle only."""
    e = gc.BY_NAME["DEEP8"]
    m6 = gc.mel("DEEP8", 6)
    y6 = gc.oracle("DEEP8", 6)[0]
    y5 = orc.generator_forward(gc.params("DEEP8"), m6[:, :5], e.cfg, np.float64)[..., 0]
    assert np.abs(y6[:, : 5 * e.cfg.hop] - y5).min() > 0.0
