"""include/vtts_dtw.h without a GPU: the float32 restatement (tests/_dtw_oracle.py) against a float64 DP and a brute force over all
monotone paths, the tie rule's visibility on the inputs the GPU test uses, the band's reachability, the duration transfer of
viettts_amd/align.py on planted warps, and the C ABI's host side.  Everything is compared with ==: the contract has no tolerance."""
import ctypes as C
import re

import numpy as np
import pytest

import _dtw_oracle as O
from viettts_amd import _lib, align

K = O.header_constants()


@pytest.fixture(scope="module")
def lib():
    from viettts_amd.csrc.build import build

    build()
    return _lib.load()


def _create(lib, n_feat=80, band=0, max_frames=_lib.DTW_MAX_FRAMES):
    h = C.c_void_p(0)
    rc = lib.vtts_dtw_create(C.byref(_lib.DtwCfg(n_feat, band, max_frames)), 0, C.byref(h))
    return rc, h


# ------------------------------------------------------------ the oracle ------------------------------------------------------------
@pytest.mark.parametrize("la,lb", [(1, 1), (1, 5), (5, 1), (2, 3), (4, 4), (5, 5), (3, 5)])
def test_f32_oracle_equals_brute_force_and_fp64_dp_on_grid_inputs(la, lb):
    for seed in range(6):
        a, b = O.grid_pair(seed, la, lb)
        total, n, span = O.dtw_f32(a, b)
        assert float(total) == O.dtw_f64(a, b) == O.brute_force(a, b)
        p = O.path_from_span(span, la)
        assert n == len(p) and tuple(p[0]) == (0, 0) and tuple(p[-1]) == (la - 1, lb - 1)
        step = np.diff(p, axis=0)
        assert set(map(tuple, step)) <= {(1, 1), (1, 0), (0, 1)}
        assert float(O.local_cost(a, b, np.float64)[p[:, 0], p[:, 1]].sum()) == float(total)  # the path costs what total says


@pytest.mark.parametrize("la,lb,band", [(37, 23, 0), (23, 37, 0), (40, 40, 2), (17, 45, 1), (45, 17, 3), (1, 9, 1), (9, 1, 2)])
def test_vectorised_oracle_equals_the_cell_by_cell_one(la, lb, band):
    for seed in range(3):
        a, b = O.grid_pair(seed, la, lb)
        t0, n0, s0 = O.dtw_f32(a, b, band)
        t1, n1, s1 = O.dtw_f32_cells(a, b, band)
        assert t0 == t1 and n0 == n1 and np.array_equal(s0, s1)
        if band == 0:
            assert float(t0) == O.dtw_f64(a, b)


@pytest.mark.parametrize("la,lb,count", O.tie_sizes())
def test_tie_rule_is_visible_on_the_kept_seeds(la, lb, count):
    """The GPU test takes O.tie_seeds(...) at straddling sizes; here: such seeds exist, and each one's span changes under EVERY other order of
    trying the predecessors, while the total (the minimum) does not."""
    seeds = O.tie_seeds(la, lb, count)
    assert len(seeds) == count
    for seed in seeds:
        a, b = O.grid_pair(seed, la, lb)
        total, _, span = O.dtw_f32(a, b)
        for order in O.OTHER_ORDERS:
            t, _, s = O.dtw_f32(a, b, order=order)
            assert t == total and not np.array_equal(s, span), (seed, order)


# ------------------------------------------------------------ the band ------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 2])
def test_band_reaches_the_corner_for_all_lengths_up_to_48(r):
    """Reachability through allowed cells only, by the three moves, for every la, lb <= 48."""
    for la in range(1, 49):
        for lb in range(1, 49):
            ok = O.in_band(np.arange(la)[:, None], np.arange(lb)[None, :], la, lb, r)
            reach = np.zeros((la + 1, lb + 1), dtype=bool)
            reach[1, 1] = ok[0, 0]
            for i in range(la):
                row = reach[i + 1]
                fed = reach[i, :-1] | reach[i, 1:]  # diagonal, up
                for j in range(lb):
                    if ok[i, j] and (fed[j] or row[j]):
                        row[j + 1] = True
            assert reach[la, lb], (la, lb, r)


@pytest.mark.parametrize("la,lb", [(40, 40), (31, 47), (47, 31)])
def test_band_run_equals_full_run_when_the_full_path_is_inside(la, lb):
    inside = 0
    for seed in range(8):
        rng = np.random.RandomState(seed)
        a = rng.standard_normal((la, 8)).astype(np.float32)
        b = rng.standard_normal((lb, 8)).astype(np.float32)
        full = O.dtw_f32(a, b)
        for r in (1, 2, 4, 8, 64):
            got = O.dtw_f32(a, b, r)
            assert O.path_in_band(got[2], la, lb, r) and got[0] >= full[0]
            if O.path_in_band(full[2], la, lb, r):
                inside += 1
                assert got[0] == full[0] and got[1] == full[1] and np.array_equal(got[2], full[2])
    assert inside >= 8  # r = 64 holds every path


# ------------------------------------------------------------ durations ------------------------------------------------------------
def _tokens_over(la, rng, zero_every=4):
    """Token frame counts (float32, integers, some zero) that sum to la."""
    counts = []
    left = la
    while left > 0:
        if len(counts) % zero_every == zero_every - 1:
            counts.append(0)
            continue
        c = int(min(left, rng.randint(1, 6)))
        counts.append(c)
        left -= c
    counts.append(0)  # a zero-length token at the end, too
    return np.asarray(counts, dtype=np.float32)


@pytest.mark.parametrize("seed,la,D", [(0, 30, 8), (1, 61, 5), (2, 7, 3)])
def test_planted_warp_is_recovered_exactly(seed, la, D):
    a, b, reps = O.planted_warp(seed, la, D)
    lb = len(b)
    total, n, span = O.dtw_f32(a, b)
    starts = np.concatenate([[0], np.cumsum(reps)[:-1]])
    assert total == 0 and np.array_equal(span[:, 0], starts) and np.array_equal(span[:, 1], starts + reps - 1) and n == lb
    tok = _tokens_over(la, np.random.RandomState(seed + 100))
    edges = align.token_edges(tok, la)
    assert edges[-1] == la and np.array_equal(edges, np.cumsum(tok).astype(np.int64))
    frames = align.transfer_frames(edges, span, la, lb)
    e = np.concatenate([[0], edges])
    planted = np.array([reps[e[k] : e[k + 1]].sum() for k in range(len(tok))])
    assert np.array_equal(frames, planted) and frames.sum() == lb and (frames >= 0).all()
    assert not frames[tok == 0].any()  # a zero-length token stays zero
    sec = align.transfer_durations(edges, span, la, lb, 256, 16000)
    assert sec.dtype == np.float32 and np.array_equal(sec, (planted * 256.0 / 16000.0).astype(np.float32))
    # the compressed direction: the repeated sequence is the query; tokens that end where a run ends get one column per run
    total, n, span_c = O.dtw_f32(b, a)
    assert total == 0 and n == lb and np.array_equal(span_c[:, 0], np.repeat(np.arange(la), reps)) and np.array_equal(span_c[:, 0], span_c[:, 1])
    edges_c = np.concatenate([[0], np.cumsum(reps)])[e][1:]
    frames_c = align.transfer_frames(edges_c, span_c, lb, la)
    assert np.array_equal(frames_c, tok.astype(np.int64)) and frames_c.sum() == la
    assert np.array_equal(align.path(span, la), O.path_from_span(span, la))


def test_token_edges_round_up_and_clip():
    fr = np.asarray([0.4, 0.4, 0.4, 2.0, 0.0, 1.7], dtype=np.float32)
    assert align.token_edges(fr, 4).tolist() == [1, 1, 2, 4, 4, 4]  # ceil of the float64 cumulative sums, clipped, the last one forced
    assert align.token_edges(fr, 9).tolist() == [1, 1, 2, 4, 4, 9]
    span = np.stack([np.arange(9) * 2, np.arange(9) * 2 + 1], axis=1)
    assert align.transfer_frames([1, 1, 2, 4, 4, 9], span, 9, 18).tolist() == [2, 0, 2, 4, 0, 10]


# ------------------------------------------------------------ the C ABI's host side ------------------------------------------------------------
def test_header_symbols_all_exported(lib):
    header = O.HEADER.read_text()
    declared = set(re.findall(r"\b(vtts_dtw_[a-z_0-9]+)\s*\(", header))
    assert declared == set(_lib.DTW_EXPORTS) == {"vtts_dtw_create", "vtts_dtw_destroy", "vtts_dtw_workspace_bytes", "vtts_dtw_forward"}
    for name in declared:
        assert hasattr(lib, name), name
    assert K["VTTS_DTW_MAX_FEAT"] == _lib.DTW_MAX_FEAT and K["VTTS_DTW_MAX_FRAMES"] == _lib.DTW_MAX_FRAMES
    assert {"VTTS_DTW_STRIP", "VTTS_DTW_TILE", "VTTS_DTW_CODES_PER_WORD", "VTTS_DTW_BT_ROWS", "VTTS_DTW_BT_WORDS"} <= set(K)


def test_create_validates_without_a_gpu(lib):
    for bad in (dict(n_feat=0), dict(n_feat=129), dict(band=-1), dict(max_frames=0), dict(max_frames=_lib.DTW_MAX_FRAMES + 1)):
        rc, _ = _create(lib, **bad)
        assert rc == -1 and lib.vtts_last_error(), bad
    for good in (dict(n_feat=1), dict(n_feat=128, band=7, max_frames=1)):
        rc, h = _create(lib, **good)
        assert rc == 0
        lib.vtts_dtw_destroy(h)


def _documented_bytes(N, ta, tb):
    strip, tile, cpw = K["VTTS_DTW_STRIP"], K["VTTS_DTW_TILE"], K["VTTS_DTW_CODES_PER_WORD"]
    strips = -(-ta // strip)
    steps = -(-(tb + strip - 1) // tile) * tile
    cost = strips * steps * strip
    codes = ta * -(-tb // cpw)
    return N * (-(-4 * (cost + codes) // 256) * 256)


def test_workspace_bytes_is_the_documented_formula_and_monotone(lib):
    rc, h = _create(lib)
    assert rc == 0
    n = C.c_size_t(0)
    prev = 0
    for N, ta, tb in [(1, 1, 1), (1, 255, 16), (1, 256, 17), (1, 257, 17), (2, 257, 17), (64, 768, 768), (64, 4096, 4096)]:
        assert lib.vtts_dtw_workspace_bytes(h, N, ta, tb, C.byref(n)) == 0
        assert n.value == _documented_bytes(N, ta, tb) >= prev
        prev = n.value
    assert prev > 2 ** 32  # the per-pair offsets are 64-bit
    for N, ta, tb in [(0, 8, 8), (1, 0, 8), (1, 8, 0), (1, 4097, 8), (1, 8, 4097)]:
        assert lib.vtts_dtw_workspace_bytes(h, N, ta, tb, C.byref(n)) == -1
    lib.vtts_dtw_destroy(h)


def test_forward_refuses_bad_lengths_and_small_workspaces_before_any_launch(lib):
    """No GPU here: every refusal below has to come from host arithmetic.  The pointers are never dereferenced."""
    rc, h = _create(lib, n_feat=4, max_frames=64)
    assert rc == 0
    fake = C.c_void_p(0x1000)
    i32 = lambda *v: (C.c_int32 * len(v))(*v)  # noqa: E731

    def fwd(N, ta, tb, la, lb, ws_bytes):
        return lib.vtts_dtw_forward(h, fake, fake, N, ta, tb, la, lb, fake, fake, fake, fake, ws_bytes, None)

    for la, lb in [((0, 3), (3, 3)), ((3, 9), (3, 3)), ((3, 3), (0, 3)), ((3, 3), (3, 9)), ((-1, 3), (3, 3))]:
        assert fwd(2, 8, 8, i32(*la), i32(*lb), 1 << 30) == -1, (la, lb)
        assert b"pair" in lib.vtts_last_error()
    assert fwd(1, 65, 8, i32(3), i32(3), 1 << 30) == -1  # the stride itself is bounded by max_frames
    assert fwd(2, 8, 8, i32(3, 3), i32(3, 3), _documented_bytes(2, 8, 8) - 1) == -5  # VTTS_ERR_NOMEM
    assert fwd(2, 8, 8, None, i32(3, 3), 1 << 30) == -1
    lib.vtts_dtw_destroy(h)


# ------------------------------------------------------------ the command line ------------------------------------------------------------
def test_align_cli_needs_the_checkpoints(tmp_path, monkeypatch):
    import viettts_amd.nat.text2mel as t2m

    a = align.build_parser().parse_args(["--wav", "a.wav", "--text", "xin chao"])
    assert a.band == 0 and a.output is None
    monkeypatch.chdir(tmp_path)
    t2m.set_duration_model(None)
    t2m.set_acoustic_model(None)
    with pytest.raises(FileNotFoundError):  # before the recording is touched, like resynth
        align.main(["--wav", "a.wav", "--text", "xin chao"])
