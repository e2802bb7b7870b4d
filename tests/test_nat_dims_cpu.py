"""The NAT width tests' host side (tests/_nat_dims.py), without a GPU:

* vtts_nat_acoustic_create()'s contract: every width set of the table is accepted, and a table of widths outside the documented set is refused
  with a message that names the rule (decoder widths 32 and 288 used to pass create() and fail in every forward);
* the table still reaches the kernel edges its lines claim (the arithmetic of viettts_amd/csrc/nat.hip restated in _nat_dims.geometry);
* the bar of tests/test_gpu_nat_dims.py is neither too tight nor too loose, judged on the oracles alone:
  - it ADMITS the reference computed in another order: the fp32 oracle with every product against a parameter matrix summed as 8-row slices added
    in sequence (the k-blocking of the LSTM step kernels) stays inside it, teacher-forced and autoregressive;
  - it SEES a lost k-slice: the fp64 oracle with the last 4 input channels of the first postnet convolution, the last 8 rows of the decoder's
    second LSTM matrix, or the last token's upsampling weight dropped lies outside it, for every quantity the change feeds.
"""
import copy
import ctypes as C

import numpy as np
import pytest

import _gta_oracle as G
import _nat_dims as D
from oracle import nat_oracle as O
from viettts_amd import _lib


@pytest.fixture(scope="module")
def lib():
    from viettts_amd.csrc.build import build

    build()  # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def _create(lib, vocab, enc, dec, prenet, mel, post):
    h = C.c_void_p(0)
    rc = lib.vtts_nat_acoustic_create(C.byref(_lib.NatAcousticCfg(vocab, enc, dec, prenet, mel, post)), 0, C.byref(h))
    msg = lib.vtts_last_error().decode() if rc else ""
    if rc == 0:
        lib.vtts_nat_acoustic_destroy(h)
    return rc, msg


@pytest.mark.parametrize("sid", sorted(D.WIDTHS))
def test_create_accepts_every_width_set(lib, sid):
    rc, msg = _create(lib, *D.WIDTHS[sid][1:])
    assert rc == 0, msg


# (vocab, enc, dec, prenet, mel, post), the words the message must contain
REFUSED = [
    ((50, 32, 256, 32, 80, 512), ("encoder width", "64, 128, 192 or 256")),
    ((50, 320, 256, 32, 80, 512), ("encoder width", "64, 128, 192 or 256")),
    ((50, 64, 32, 32, 80, 512), ("decoder_dim", "256, 512, 768 or 1024", "32")),
    ((50, 64, 288, 32, 80, 512), ("decoder_dim", "256, 512, 768 or 1024", "288")),
    ((50, 64, 1056, 32, 80, 512), ("decoder_dim", "256, 512, 768 or 1024", "1056")),
    ((50, 64, 256, 48, 80, 512), ("prenet_dim", "multiple of 32", "48")),
    ((50, 256, 256, 544, 80, 512), ("prenet_dim", "2 * encoder_dim + prenet_dim <= 1024", "544")),  # 2 * 256 + 544 = 1056
    ((50, 64, 256, 32, 6, 512), ("mel_dim", "multiple of 4", "6")),
    ((50, 64, 256, 32, 132, 512), ("mel_dim", "4 .. 128", "132")),
    ((50, 64, 256, 32, 80, 6), ("postnet_dim", "multiple of 4", "6")),
    ((50, 64, 256, 32, 80, 1028), ("postnet_dim", "4 .. 1024", "1028")),
]


@pytest.mark.parametrize("cfg, words", REFUSED, ids=["enc32", "enc320", "dec32", "dec288", "dec1056", "prenet48", "sum1056", "mel6", "mel132", "post6", "post1028"])
def test_create_refuses_with_a_message_naming_the_rule(lib, cfg, words):
    rc, msg = _create(lib, *cfg)
    assert rc == -1, (cfg, "accepted")
    for w in words:
        assert w in msg, (cfg, msg)


def test_the_table_reaches_the_edges_it_names():
    g = {sid: D.geometry(sid) for sid in D.WIDTHS}
    S, Oo, W, X, R = (g[k] for k in "SOWXR")
    assert S["enc_lstm_iters"] == 2 < S["prefetch_depth"] and W["enc_lstm_iters"] == 6 and R["enc_lstm_iters"] == 8
    assert (R["dec_lstm_iters"], R["tf_lstm_iters"]) == ((12, 20), (8, 16))  # what every other NAT test runs
    assert S["proj"]["chunks"] == 256 and S["proj"]["live_chunks"] == 128 and S["prenet1"]["live_chunks"] == 1 and S["threefry_blocks"] == 0.5
    assert S["postnet_steps"] == (1, 1) and S["postnet_mblocks"] == (1, 1)
    assert Oo["prenet1"]["chunks"] == 10 and Oo["prenet1"]["idle_threads"] == 64 and Oo["proj"]["idle_threads"] == 16
    assert D.WIDTHS["O"][5] % 8 != 0 and D.WIDTHS["O"][6] % 32 == 4  # Cin = 84: the clamp cc = Cin - 4 inside a step; Cout = 36: the guard inside a lane half
    assert W["mix_chunks"] == 3 and W["postnet_mblocks"][0] == 32 and D.WIDTHS["W"][5] == 128
    assert X["prenet1"]["chunks"] == 1 and X["proj_lds_bytes"] == 64 * 1024 and max(v["proj_lds_bytes"] for v in g.values()) == 64 * 1024
    assert [g[k]["x3_split_state"] for k in "SOWXR"] == [False, False, True, True, True]
    assert (D.WIDTHS["W"][4] + D.WIDTHS["W"][3], D.WIDTHS["W"][4] + 2 * D.WIDTHS["W"][3]) == (896, 1664)
    assert (D.WIDTHS["X"][4] + D.WIDTHS["X"][3], D.WIDTHS["X"][4] + 2 * D.WIDTHS["X"][3]) == (1920, 2944)
    # the mix raises its dynamic-LDS attribute from 723 tokens on; the long cases sit beyond it, the reference-width tests (<= 256 tokens) below
    assert D.mix_lds_bytes(722) <= 48 * 1024 < D.mix_lds_bytes(723) and all(D.mix_lds_bytes(L) > 48 * 1024 for L, _ in D.LONG_CASES)
    assert D.mix_lds_bytes(2048) <= 160 * 1024  # the CU's LDS
    for sid, (_, V, *_rest) in D.WIDTHS.items():
        for L, F in D.CASES:
            c = D.case(sid, L, F)
            assert c.tokens.max() < V and c.dur.shape == (L,) and abs(float(c.dur.sum()) - F) < 1e-3 * F and (L == 1 or (c.dur == 0).sum() == 1)


# ------------------------------------------------ the bar admits the reference in another order ------------------------------------------------
class _Sliced(np.ndarray):
    """A parameter matrix whose products ``x @ w`` are summed as 8-row slices added in sequence: each slice's partial sum is formed on its own and
    then added to the running sum.  For a vector ``x`` the slice's sum is written out (rows added in order): the BLAS behind numpy forms a
    vector-matrix product in blocks of 8 rows itself, so slicing alone would reproduce its bits."""

    def __rmatmul__(self, x):
        w = np.asarray(self)
        x = np.asarray(x)

        def part(k):
            if x.ndim == 1:
                return (x[k : k + 8, None] * w[k : k + 8]).sum(axis=0)
            return np.ascontiguousarray(x[..., k : k + 8]) @ w[k : k + 8]

        acc = part(0)
        for k in range(8, w.shape[0], 8):
            acc = acc + part(k)
        return acc


def _warm(sid):
    """Every shared oracle value of a width set, computed BEFORE a test patches the oracle."""
    return {q: D.e32(sid, q) for q in ("enc", "pre", "mel", "ar")}


def _patch_sliced_products(monkeypatch):
    plain = O.Params.get

    def get(self, suffix, name, state=False):
        a = plain(self, suffix, name, state)
        return a.view(_Sliced) if name == "w" else a

    monkeypatch.setattr(O.Params, "get", get)


def test_sliced_products_are_another_order_of_the_same_sum(monkeypatch):
    _patch_sliced_products(monkeypatch)
    P, S = D.checkpoint("O")
    w = O.Params(P, S, np.float32).get(f"{G.PRE}/~/lstm_1/linear", "w")
    x = np.random.default_rng(1).standard_normal(w.shape[0]).astype(np.float32)
    got, plain = x @ w, x @ np.asarray(w)
    assert type(got) is np.ndarray and got.dtype == np.float32 and not np.array_equal(got, plain)
    assert np.abs(got - x.astype(np.float64) @ np.asarray(w, dtype=np.float64)).max() < 1e-5


@pytest.mark.parametrize("sid", ["S", "O", "W", "R"])
def test_the_bar_admits_the_oracle_in_another_summation_order(monkeypatch, sid):
    _warm(sid)
    _patch_sliced_products(monkeypatch)
    P, S = D.checkpoint(sid)
    worst = {}
    for L, F in D.ORDER_CASES:
        c = D.case(sid, L, F)
        pre, mel = G.teacher_forced_row(P, S, c.tokens, L, c.dur, c.mels, c.keep, c.zone, np.float32)
        ar = O.acoustic_inference(P, S, c.tokens, c.dur, F, dtype=np.float32)
        assert not isinstance(pre, _Sliced) and pre.dtype == np.float32
        want_pre, want_mel = D.oracle_teacher(sid, L, F)
        want_ar = D.oracle_ar(sid, L, F)
        for q, got, want, cap in (("pre", pre, want_pre, D.CAP), ("mel", mel, want_mel, D.CAP), ("ar", ar, want_ar, D.cap_ar(want_ar))):
            err, b = D.report(f"{sid} ({L}, {F}) {q}, oracle fp32 in 8-row slices", got, want, D.e32(sid, q), cap)
            worst[q] = max(worst.get(q, 0.0), err / b)
            assert 0.0 < err <= b, (sid, L, F, q, err, b)
    print(f"[nat dims] {sid}: worst err / bar of the sliced fp32 oracle {worst}")


# ------------------------------------------------ the bar sees a lost k-slice ------------------------------------------------
def _outputs(P, S, c):
    pre, mel = G.teacher_forced_row(P, S, c.tokens, c.L, c.dur, c.mels, c.keep, c.zone, np.float64)
    return {"pre": pre, "mel": mel, "ar": O.acoustic_inference(P, S, c.tokens, c.dur, c.F, dtype=np.float64)}


def _assert_outside(what, sid, c, got, feeds):
    want = dict(zip(("pre", "mel"), D.oracle_teacher(sid, c.L, c.F)), ar=D.oracle_ar(sid, c.L, c.F))
    for q in ("pre", "mel", "ar"):
        cap = D.cap_ar(want[q]) if q == "ar" else D.CAP
        err, b = D.report(f"{sid} ({c.L}, {c.F}) {q}, {what}", got[q], want[q], D.e32(sid, q), cap)
        if q in feeds:
            assert err > b, (what, q, err, b)
        else:
            assert err < 1e-12, (what, q, err)  # (not bit-equal: the copied parameters' alignment moves the BLAS's blocking)


@pytest.mark.parametrize("L, F", D.ORDER_CASES)
def test_the_bar_sees_a_lost_slice_of_the_first_postnet_convolution(L, F):
    P, S = D.checkpoint("O")
    P = copy.deepcopy(P)
    P[f"{G.PRE}/~/conv1_d"]["w"][:, -4:, :] = 0.0
    _assert_outside("last 4 input channels of postnet layer 0 zeroed", "O", D.case("O", L, F), _outputs(P, S, D.case("O", L, F)), ("mel", "ar"))


@pytest.mark.parametrize("L, F", D.ORDER_CASES)
def test_the_bar_sees_a_lost_slice_of_the_second_decoder_lstm(L, F):
    P, S = D.checkpoint("O")
    P = copy.deepcopy(P)
    P[f"{G.PRE}/~/lstm_1/linear"]["w"][-8:, :] = 0.0
    _assert_outside("last 8 rows of lstm_1/linear zeroed", "O", D.case("O", L, F), _outputs(P, S, D.case("O", L, F)), ("pre", "mel", "ar"))


@pytest.mark.parametrize("L, F", D.ORDER_CASES)
def test_the_bar_sees_a_lost_upsampling_weight(monkeypatch, L, F):
    def upsample_without_the_last_token(x, durations, n_frames):  # O.gaussian_upsample, the last token's column of the weights dropped
        dt = x.dtype
        ruler = np.arange(n_frames, dtype=dt)
        end_pos = np.cumsum(durations.astype(dt))
        mid_pos = end_pos - durations.astype(dt) / dt.type(2)
        z = -np.square(mid_pos[None, :] - ruler[:, None]) / dt.type(10.0)
        w = np.exp(z - z.max(axis=-1, keepdims=True))
        w = w / w.sum(axis=-1, keepdims=True)
        w[:, -1] = 0
        return w @ x

    x = np.random.default_rng(2).standard_normal((7, 5))
    d = np.array([1.0, 2.0, 0.0, 3.0, 1.5, 2.5, 1.0])
    plain, dropped = O.gaussian_upsample(x, d, 11), upsample_without_the_last_token(x, d, 11)
    assert np.abs(plain[:3] - dropped[:3]).max() < 1e-3 < np.abs(plain[-1] - dropped[-1]).max()  # the same function but for the frames near the last token
    _warm("O")
    monkeypatch.setattr(O, "gaussian_upsample", upsample_without_the_last_token)
    P, S = D.checkpoint("O")
    _assert_outside("last token's upsampling weight dropped", "O", D.case("O", L, F), _outputs(P, S, D.case("O", L, F)), ("pre", "mel", "ar"))
