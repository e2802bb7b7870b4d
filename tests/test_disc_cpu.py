"""The discriminators' host side without a GPU: the C ABI's exports, geometry and error paths, the oracle against the minted
fixture, the weight folding against torch's own modules, and the drop-in surface."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import _disc_oracle as oracle
from viettts_amd import _lib

REPO = Path(__file__).resolve().parents[1]
GOLDEN = REPO / "tests" / "golden" / "disc_golden.npz"


@pytest.fixture(scope="module")
def lib():
    from viettts_amd.csrc.build import build

    build()
    return _lib.load()


@pytest.fixture(scope="module")
def handle(lib):
    h = C.c_void_p(0)
    _lib.check(lib, lib.vtts_disc_create(0, C.byref(h)))
    yield h
    lib.vtts_disc_destroy(h)


@pytest.fixture(scope="module")
def params():
    from viettts_amd.hifigan.disc_synth import synthetic_disc_checkpoint
    from viettts_amd.hifigan.discriminators import fold_checkpoint

    return fold_checkpoint(synthetic_disc_checkpoint(8642))


def test_header_symbols_exported_and_source_listed(lib):
    from viettts_amd.csrc import build

    header = (REPO / "include" / "vtts_disc.h").read_text()
    declared = set(re.findall(r"\b(vtts_disc_[a-z_0-9]+)\s*\(", header))
    assert declared == set(_lib.DISC_EXPORTS), declared ^ set(_lib.DISC_EXPORTS)
    for name in declared:
        assert hasattr(lib, name), name
    assert "disc.hip" in build.SOURCES and "-fno-slp-vectorize" in build.FILE_FLAGS["disc.hip"]
    assert any(str(h).endswith("vtts_disc.h") for h in build.HEADERS)
    for name, val in (("VTTS_DISC_NUM_FMAPS", _lib.DISC_NUM_FMAPS), ("VTTS_DISC_MIN_SAMPLES", _lib.DISC_MIN_SAMPLES),
                      ("VTTS_DISC_LOSS_REAL", _lib.DISC_LOSS_REAL), ("VTTS_DISC_LOSS_FAKE", _lib.DISC_LOSS_FAKE), ("VTTS_DISC_LOSS_GEN", _lib.DISC_LOSS_GEN),
                      ("VTTS_DISC_LOSS_TOTALS", _lib.DISC_LOSS_TOTALS), ("VTTS_DISC_LOSS_RESULTS", _lib.DISC_LOSS_RESULTS)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == val
    assert _lib.DISC_LOSS_FLOATS == 128 + 2 * (54 + 24) * 64


def test_param_table(lib, handle):
    n = C.c_int(0)
    _lib.check(lib, lib.vtts_disc_num_params(handle, C.byref(n)))
    assert n.value == 108
    keys = oracle.conv_keys()
    total = 0
    for i in range(n.value):
        key, which = C.c_char_p(), C.c_char_p()
        shape, nd = (C.c_int64 * 3)(), C.c_int(0)
        _lib.check(lib, lib.vtts_disc_param_info(handle, i, C.byref(key), C.byref(which), shape, C.byref(nd)))
        k, (cin, cout, ks, _s, _p, g) = keys[i // 2]
        assert key.value.decode() == k
        if i % 2 == 0:
            assert which.value == b"w" and nd.value == 3 and tuple(shape) == (cout, cin // g, ks)
            total += cout * (cin // g) * ks
        else:
            assert which.value == b"b" and nd.value == 1 and shape[0] == cout
    assert total == 70_676_896  # the effective weights: 283 MB of fp32
    nb = C.c_size_t(0)
    _lib.check(lib, lib.vtts_disc_packed_bytes(handle, C.byref(nb)))
    assert total * 4 <= nb.value < total * 4 + (1 << 20)
    nf = C.c_int(0)
    _lib.check(lib, lib.vtts_disc_num_fmaps(handle, C.byref(nf)))
    assert nf.value == 54


def _info(lib, h, i, N, T):
    c, l, p, off = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
    _lib.check(lib, lib.vtts_disc_fmap_info(h, i, N, T, C.byref(c), C.byref(l), C.byref(p), C.byref(off)))
    return c.value, l.value, p.value, off.value


@pytest.mark.parametrize("T", [11, 37, 2310, 4099, 8192])
def test_fmap_info_gives_the_reference_shapes(lib, handle, T):
    N = 4
    want = oracle.fmap_shapes(T)
    end = 0
    for i in range(54):
        c, l, p, off = _info(lib, handle, i, N, T)
        assert (c, l, p) == want[i], (i, (c, l, p), want[i])
        assert off >= end and off % 64 == 0
        end = off + N * c * l * p
    if T == 4099:
        assert [_info(lib, handle, i, N, T)[1] for i in range(6)] == [684, 228, 76, 26, 26, 26]
        assert [_info(lib, handle, 30 + 8 * d, N, T)[1] for d in range(3)] == [4099, 2050, 1026]
    if T in (11, 37, 2310, 4099):  # the shapes the reference's modules produced when the fixture was minted
        g = np.load(GOLDEN)
        assert g[f"scores_{T}"].size == N * sum(want[i][1] * want[i][2] for i in (5, 11, 17, 23, 29, 37, 45, 53))
        if T == 37:
            for i in range(54):
                assert g[f"fmap37_{i}"].shape[1:] == (want[i] if i < 30 else want[i][:2])


def test_error_paths(lib, handle):
    c = C.c_int64(0)
    n = C.c_size_t(0)
    assert lib.vtts_disc_fmap_info(handle, 0, 2, 10, C.byref(c), C.byref(c), C.byref(c), C.byref(c)) == -6  # T < 11: VTTS_ERR_SHAPE
    assert b"11" in lib.vtts_last_error()
    assert lib.vtts_disc_workspace_bytes(handle, 2, 10, C.byref(n)) == -6
    assert lib.vtts_disc_workspace_bytes(handle, 0, 64, C.byref(n)) == -1  # N < 1
    assert lib.vtts_disc_workspace_bytes(handle, 2, 11, C.byref(n)) == 0 and n.value == 0
    assert lib.vtts_disc_fmap_info(handle, 54, 2, 64, C.byref(c), C.byref(c), C.byref(c), C.byref(c)) == -1
    h = C.c_void_p(0)
    _lib.check(lib, lib.vtts_disc_create(0, C.byref(h)))
    rc = lib.vtts_disc_forward(h, C.c_void_p(256), 2, 64, C.c_void_p(256), C.c_void_p(256), None, None)
    assert rc == -2 and b"before pack" in lib.vtts_last_error()
    assert lib.vtts_disc_pack(h, C.c_void_p(256), 1 << 30, None) == -3 and b"never set" in lib.vtts_last_error()
    _lib.check(lib, lib.vtts_disc_packed_bytes(h, C.byref(n)))
    assert lib.vtts_disc_bind_packed(h, C.c_void_p(256), n.value - 4) == -5  # a wrong-size blob
    assert lib.vtts_disc_bind_packed(h, C.c_void_p(260), n.value) == -1  # misaligned
    buf = (C.c_float * 8)()
    shp = (C.c_int64 * 3)(1, 2, 3)
    assert lib.vtts_disc_set_param(h, b"mpd.discriminators.9.convs.0", b"w", buf, shp, 3) == -1
    assert lib.vtts_disc_set_param(h, b"mpd.discriminators.0.convs.0", b"w", buf, shp, 3) == -6
    assert lib.vtts_disc_set_param(h, b"mpd.discriminators.0.convs.0", b"q", buf, shp, 3) == -1
    assert lib.vtts_disc_losses(h, C.c_void_p(256), C.c_void_p(256), 0, 64, C.c_void_p(256), None) == -1
    assert lib.vtts_disc_losses(h, C.c_void_p(256), C.c_void_p(256), 1, 10, C.c_void_p(256), None) == -6
    lib.vtts_disc_destroy(h)


def _loss_vector(L):
    return np.concatenate([L["fmap_l1"], L["real"], L["fake"], L["gens"], np.array([L[k] for k in oracle.LOSS_NAMES])]).astype(np.float64)


@pytest.mark.parametrize("T", [11, 37, 2310, 4099, 16411])
def test_oracle_reproduces_the_fixture(params, T):
    g = np.load(GOLDEN)
    assert int(g["weight_seed"]) == 8642
    (B, seed), = [(int(b), int(s)) for t, b, s in g["shapes"] if int(t) == T]
    y2 = oracle.make_inputs(B, T, seed)
    assert float(y2.astype(np.float64).sum()) == float(g[f"ysum_{T}"])
    if f"y_{T}" in g:
        assert np.array_equal(y2, g[f"y_{T}"])
    scores, fmaps = oracle.forward(params, y2, torch.float64)
    got_scores = np.concatenate([s.numpy().ravel() for s in scores])
    assert np.abs(got_scores - g[f"scores_{T}"]).max() <= 1e-12 * np.abs(g[f"scores_{T}"]).max()
    stats = np.array([[float(f.sum()), float(f.abs().sum()), float(f.abs().max())] for f in fmaps])
    want = g[f"stats_{T}"]
    assert (np.abs(stats - want) <= 1e-12 * want[:, 1:2]).all()  # sums against the abs-sum: cancellation-proof
    lv = _loss_vector(oracle.losses(scores, fmaps, B))
    assert np.abs(lv / g[f"losses_{T}"] - 1).max() <= 1e-12
    if T == 37:
        for i, f in enumerate(fmaps):
            full = g[f"fmap37_{i}"]  # float32: rounded once from the reference's fp64 run
            assert np.array_equal(f[[0, B]].numpy().astype(np.float32), full), i


def test_fixture_is_small():
    assert GOLDEN.stat().st_size < 1_000_000


def _conv(spectral, parametrised):
    torch.manual_seed(5)
    m = torch.nn.Conv1d(8, 12, 5, groups=2)
    if spectral:
        m = torch.nn.utils.spectral_norm(m)
        with torch.no_grad():
            for _ in range(3):  # train-mode forwards move u, v; eval below freezes them
                m(torch.randn(1, 8, 16))
    elif parametrised:
        m = torch.nn.utils.parametrizations.weight_norm(m)
        with torch.no_grad():
            m.parametrizations.weight.original0.mul_(1.7)
    else:
        m = torch.nn.utils.weight_norm(m)
        with torch.no_grad():
            m.weight_g.mul_(1.7)
    return m.eval()


@pytest.mark.parametrize("style", ["weight_norm", "parametrised_weight_norm", "spectral_norm", "plain"])
def test_weight_folding_matches_torch_modules(style):
    from viettts_amd.hifigan.discriminators import fold_state_dict

    if style == "plain":
        torch.manual_seed(5)
        m = torch.nn.Conv1d(8, 12, 5, groups=2).eval()
    else:
        m = _conv(style == "spectral_norm", style == "parametrised_weight_norm")
    with torch.no_grad():
        m(torch.zeros(1, 8, 16))  # eval: the hooks compute the effective weight, no power iteration
        want = m.weight.detach().numpy().astype(np.float64)
    sd = {"discriminators.0.convs.1." + k: v for k, v in m.state_dict().items()}
    if style == "weight_norm":
        assert any(k.endswith("weight_g") for k in sd)
    if style == "parametrised_weight_norm":
        assert any(k.endswith("parametrizations.weight.original0") for k in sd)
    if style == "spectral_norm":
        assert any(k.endswith("weight_orig") for k in sd) and any(k.endswith("weight_u") for k in sd)
    out = fold_state_dict(sd, "msd")
    assert list(out) == ["msd.discriminators.0.convs.1"]
    w, b = out["msd.discriminators.0.convs.1"]
    assert w.dtype == np.float32 and w.shape == (12, 4, 5)
    assert np.abs(w - want).max() <= 2.0 ** -22 * np.abs(want).max()  # torch folds in fp32, we fold in fp64 and round once
    assert np.array_equal(b, m.bias.detach().numpy())


def test_checkpoint_dict_round_trips(params):
    from viettts_amd.hifigan.disc_synth import synthetic_disc_checkpoint
    from viettts_amd.hifigan.discriminators import fold_checkpoint

    ckpt = synthetic_disc_checkpoint(8642)
    assert set(ckpt) == {"mpd", "msd"}
    assert [k for k, _ in oracle.conv_keys()] == sorted(params, key=[k for k, _ in oracle.conv_keys()].index) and len(params) == 54
    for key, (cin, cout, k, _s, _p, g) in oracle.conv_keys():
        w, b = params[key]
        assert w.shape == (cout, cin // g, k) and b.shape == (cout,) and w.dtype == b.dtype == np.float32
    # weight norm: the effective row norm is the gain, in [0.5, 1.5)
    w, _ = params["mpd.discriminators.2.convs.3"]
    norms = np.sqrt((w.astype(np.float64) ** 2).sum(axis=(1, 2)))
    assert 0.5 <= norms.min() and norms.max() < 1.5
    # spectral norm with iterated u, v: u . (W v) approaches the largest singular value from below, so the folded matrix's is
    # 1 or just above (a random u, v pair would leave it orders of magnitude larger)
    w, _ = params["msd.discriminators.0.convs.2"]
    top = np.linalg.norm(w.reshape(w.shape[0], -1).astype(np.float64), 2)
    assert 1.0 - 1e-6 <= top < 1.1, top
    # plain effective weights in a do_*-shaped dictionary give themselves back; extra entries are ignored
    plain = {"mpd": {}, "msd": {}, "steps": 5, "optim_d": {}}
    for key, (w, b) in params.items():
        plain[key[:3]][key[4:] + ".weight"] = torch.from_numpy(w[..., None] if key.startswith("mpd") else w)
        plain[key[:3]][key[4:] + ".bias"] = torch.from_numpy(b)
    again = fold_checkpoint(plain)
    assert set(again) == set(params)
    for key in ("mpd.discriminators.4.convs.1", "msd.discriminators.0.convs.3", "msd.discriminators.2.conv_post"):
        assert np.array_equal(again[key][0], params[key][0]) and np.array_equal(again[key][1], params[key][1])
    with pytest.raises(KeyError):
        fold_checkpoint({"mpd": {}})


def test_dropin_surface_and_no_cpu_path():
    from vietTTS.hifigan import torch_model as tm
    from viettts_amd.hifigan.discriminators import Discriminators

    with pytest.raises(ValueError):
        Discriminators("cpu")
    assert list(inspect.signature(tm.MultiPeriodDiscriminator.forward).parameters) == ["self", "y", "y_hat"]
    assert list(inspect.signature(tm.MultiScaleDiscriminator.forward).parameters) == ["self", "y", "y_hat"]
    assert list(inspect.signature(tm.feature_loss).parameters) == ["fmap_r", "fmap_g"]
    assert list(inspect.signature(tm.discriminator_loss).parameters) == ["disc_real_outputs", "disc_generated_outputs"]
    assert list(inspect.signature(tm.generator_loss).parameters) == ["disc_outputs"]
    tm.MultiPeriodDiscriminator(), tm.MultiScaleDiscriminator()  # no constructor arguments, as the reference
    with pytest.raises(TypeError):
        tm.feature_loss([[torch.zeros(1)]], [[torch.zeros(1)]])  # no eager path
    from viettts_amd import vocoder_eval

    with pytest.raises(FileNotFoundError):
        vocoder_eval.main(["--wav", "nothing.wav", "--generator", "no_such_g", "--discriminator", "no_such_do"])
