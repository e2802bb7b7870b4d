"""The DTW kernels (include/vtts_dtw.h, viettts_amd/csrc/dtw.hip) on the GPU against the numpy float32 restatement of the contract
(tests/_dtw_oracle.py; tests/test_dtw_cpu.py checks that one against a float64 DP and a brute force).  total, path_len and span are
compared with ==: the contract fixes every fp32 operation and its order, so there is no tolerance anywhere in this file.

Sizes come from the header's constants: for every tile / strip / code-word size S the lengths 1, 2, S - 1, S, S + 1, 2 S - 1, 2 S, 2 S + 1.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _dtw_oracle as O
import _row_split as RS
from viettts_amd import _lib, align
from viettts_amd._handle import ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = O.header_constants()
SIZES = sorted({v for S in (K["VTTS_DTW_CODES_PER_WORD"], K["VTTS_DTW_TILE"], K["VTTS_DTW_STRIP"], K["VTTS_DTW_BT_ROWS"],
                            K["VTTS_DTW_BT_WORDS"] * K["VTTS_DTW_CODES_PER_WORD"]) for v in (1, 2, S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1)})
# the diagonal, the anti-diagonal (its ends are the extreme corners) and the two one-row / one-column cases
EDGE_PAIRS = sorted({(s, s) for s in SIZES} | {(s, t) for s, t in zip(SIZES, reversed(SIZES))} | {(1, 257), (257, 1)})


@pytest.fixture(scope="module")
def dtws():
    assert torch.cuda.is_available()
    made = {}

    def get(n_feat, band=0, **kw):
        key = (n_feat, band, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = align.Dtw(n_feat, band, DEV, **kw)
        return made[key]

    yield get
    for d in made.values():
        d.close()


def _normal(seed, la, lb, D):
    rng = np.random.RandomState(seed)
    return rng.standard_normal((la, D)).astype(np.float32), rng.standard_normal((lb, D)).astype(np.float32)


def _host(res):
    torch.cuda.synchronize()
    return res.total.cpu().numpy(), res.path_len.cpu().numpy(), res.span.cpu().numpy()


def _assert_equal(got, n, want, la, what):
    total, path_len, span = got
    w_total, w_len, w_span = want
    assert total[n].dtype == np.float32 and total[n] == w_total, (what, "total", float(total[n]), float(w_total))
    assert path_len[n] == w_len, (what, "path_len", int(path_len[n]), w_len)
    assert np.array_equal(span[n, :la], w_span), (what, "span")
    assert (span[n, la:] == -1).all(), (what, "span rows past la")


@pytest.mark.parametrize("D", [1, 80, 128])
def test_edges_of_every_tile_strip_and_code_word(dtws, D):
    assert len(EDGE_PAIRS) <= 44 and (1, SIZES[-1]) in EDGE_PAIRS and (SIZES[-1], 1) in EDGE_PAIRS and SIZES[-1] == 2 * K["VTTS_DTW_STRIP"] + 1
    d = dtws(D)
    for k, (la, lb) in enumerate(EDGE_PAIRS):
        a, b = _normal(1000 * D + k, la, lb, D)
        _assert_equal(_host(d.dtw(a, b)), 0, O.dtw_f32(a, b), la, (la, lb, D))


@pytest.mark.parametrize("la,lb,count", O.tie_sizes())
def test_tie_rich_grid_inputs(dtws, la, lb, count):
    """Inputs on the 1/8 grid, where every other order of trying the predecessors gives another span (asserted in tests/test_dtw_cpu.py for
    exactly these seeds): the comparison cannot pass with the wrong tie rule."""
    d = dtws(8)
    for seed in O.tie_seeds(la, lb, count):
        a, b = O.grid_pair(seed, la, lb)
        want = O.dtw_f32(a, b)
        _assert_equal(_host(d.dtw(a, b)), 0, want, la, (la, lb, seed))
        assert float(want[0]) == O.dtw_f64(a, b)


def test_ragged_batch_equals_each_row_alone(dtws):
    D, N = 80, 8
    rng = np.random.RandomState(5)
    las = [int(v) for v in rng.choice(SIZES, size=N)]
    lbs = [int(v) for v in rng.choice(SIZES, size=N)]
    las[0], lbs[0], las[1], lbs[1] = SIZES[-1], SIZES[-2], 1, SIZES[-1]
    Ta, Tb = SIZES[-1] + 7, SIZES[-1] + 18  # larger than every length
    a = np.full((N, Ta, D), np.nan, dtype=np.float32)  # the padding is never read
    b = np.full((N, Tb, D), np.nan, dtype=np.float32)
    for n in range(N):
        a[n, : las[n]], b[n, : lbs[n]] = _normal(70 + n, las[n], lbs[n], D)
    d = dtws(D)
    got = _host(d.dtw(a, b, las, lbs))
    assert got[2].shape == (N, Ta, 2)
    ws = d._ws
    for n in range(N):
        alone = _host(d.dtw(a[n, : las[n]], b[n, : lbs[n]]))
        assert alone[0][0] == got[0][n] and alone[1][0] == got[1][n] and np.array_equal(alone[2][0], got[2][n, : las[n]]), n
        _assert_equal(got, n, O.dtw_f32(a[n, : las[n]], b[n, : lbs[n]]), las[n], n)
    # a smaller batch reuses the grown workspace
    small = _host(d.dtw(a[:3], b[:3], las[:3], lbs[:3]))
    assert d._ws is ws and d._ws.data_ptr() == ws.data_ptr()
    assert np.array_equal(small[0], got[0][:3]) and np.array_equal(small[1], got[1][:3]) and np.array_equal(small[2], got[2][:3])


@pytest.mark.parametrize("la,lb", [(257, 129), (129, 257)])
@pytest.mark.parametrize("r", [1, 4, 32])
def test_band(dtws, la, lb, r):
    """r = 1 leaves whole cost tiles out (the band is a few cells wide, a tile 64); r = 32 at these sizes still cuts the corners."""
    a, b = _normal(900 + r, la, lb, 80)
    want = O.dtw_f32(a, b, r)
    assert np.isfinite(want[0]) and O.path_in_band(want[2], la, lb, r)
    tile = K["VTTS_DTW_TILE"]
    if r == 1:
        assert not O.in_band(0, tile, la, lb, r) and not O.in_band(tile, 0, la, lb, r)  # the tiles next to the first one lie outside
    _assert_equal(_host(dtws(80, r).dtw(a, b)), 0, want, la, (la, lb, r))
    ag, bg = O.grid_pair(r, la, lb)  # ties, under a band
    _assert_equal(_host(dtws(8, r).dtw(ag, bg)), 0, O.dtw_f32(ag, bg, r), la, (la, lb, r, "grid"))


def test_sliced_batch_equals_the_unsliced_one(dtws):
    D, N, Ta, Tb = 80, 5, 70, 90
    rng = np.random.RandomState(11)
    a, b = rng.standard_normal((N, Ta, D)).astype(np.float32), rng.standard_normal((N, Tb, D)).astype(np.float32)
    las, lbs = [70, 1, 33, 64, 65], [90, 90, 17, 1, 80]
    whole = _host(dtws(D).dtw(a, b, las, lbs))
    tiny = dtws(D, workspace_budget=1)  # one pair per slice
    sliced = _host(tiny.dtw(a, b, las, lbs))
    assert tiny._ws.numel() == tiny.workspace_bytes(1, Ta, Tb) < dtws(D).workspace_bytes(N, Ta, Tb)
    for x, y in zip(whole, sliced):
        assert np.array_equal(x, y)
    two = dtws(D, workspace_budget=2 * tiny.workspace_bytes(1, Ta, Tb))  # slices of two, the last one of one
    for x, y in zip(whole, _host(two.dtw(a, b, las, lbs))):
        assert np.array_equal(x, y)
    _assert_equal(whole, 2, O.dtw_f32(a[2, :33], b[2, :17]), 33, "row 2")


def _run_prefilled(d, a, b, las, lbs):
    """forward() through the C ABI, the whole batch in ONE call, into outputs pre-filled with NaN / -7: what no launch writes shows."""
    at, bt_ = (torch.from_numpy(np.array(x)).to(d.device) for x in (a, b))  # (copies: the shared rows are read-only)
    N, Ta, Tb = at.shape[0], at.shape[1], bt_.shape[1]
    total = torch.full((N,), float("nan"), dtype=torch.float32, device=d.device)
    path_len = torch.full((N,), -7, dtype=torch.int32, device=d.device)
    span = torch.full((N, Ta, 2), -7, dtype=torch.int32, device=d.device)
    ws = d._workspace(d.workspace_bytes(N, Ta, Tb)).fill_(0xFF)
    d._on_stream("forward", ptr(at), ptr(bt_), N, Ta, Tb, (C.c_int32 * N)(*las), (C.c_int32 * N)(*lbs), ptr(total), ptr(path_len), ptr(span), ptr(ws), ws.numel())
    torch.cuda.synchronize()
    return total.cpu().numpy(), path_len.cpu().numpy(), span.cpu().numpy()


@pytest.mark.parametrize("band", [0, RS.DTW_NARROW_BAND])
def test_pairs_behind_the_launch_split_against_the_oracle(dtws, band):
    """DTW_PAIRS_PER_LAUNCH + 3 pairs (tests/_row_split.py) in one forward(): the pairs behind the split differ from the first ones in a, in b
    and in both lengths, and hold the longest a and b, a 1 x n and an n x 1 pair.  total, path_len and the whole span of every pair == dtw_f32
    (once per distinct pair); each pair behind the split is that pair run alone."""
    bt = RS.dtw_batch(_lib.DTW_PAIRS_PER_LAUNCH)
    a, b, las, lbs = RS.dtw_pairs(bt)
    assert bt.N == _lib.DTW_PAIRS_PER_LAUNCH + 3 and a.shape[2] == 8
    d = dtws(8, band)
    want = RS.per_kind(bt, lambda r: O.dtw_f32(r.content[: r.length // 64], r.content[a.shape[1] : a.shape[1] + r.length % 64], band))
    got = _run_prefilled(d, a, b, las, lbs)
    for n in range(bt.N):
        assert np.isfinite(want[n][0])
        _assert_equal(got, n, want[n], las[n], (n, las[n], lbs[n], band))
    for n in bt.behind():
        alone = _host(d.dtw(np.array(a[n, : las[n]]), np.array(b[n, : lbs[n]])))
        assert alone[0][0] == got[0][n] and alone[1][0] == got[1][n] and np.array_equal(alone[2][0], got[2][n, : las[n]]), n
    print(f"\ndtw pairs behind the split, band {band}: {bt.k} pairs ==, worst error / bar 0 (the contract is ==)")


def test_planted_warp_recovers_token_frame_counts(dtws):
    la, D = 150, 80
    a, b, reps = O.planted_warp(3, la, D)
    lb = len(b)
    total, path_len, span = _host(dtws(D).dtw(a, b))
    starts = np.concatenate([[0], np.cumsum(reps)[:-1]])
    assert total[0] == 0 and path_len[0] == lb and np.array_equal(span[0, :, 0], starts) and np.array_equal(span[0, :, 1], starts + reps - 1)
    tok = np.asarray([3, 0, 5, 1, 0, 0, 7] * 9 + [6, 0], dtype=np.float32)  # 150 query frames over 65 tokens, many of them empty
    assert tok.sum() == la
    edges = align.token_edges(tok, la)
    e = np.concatenate([[0], edges])
    planted = np.array([reps[e[k] : e[k + 1]].sum() for k in range(len(tok))])
    assert np.array_equal(align.transfer_frames(edges, span[0], la, lb), planted)
    sec = align.transfer_durations(edges, span[0], la, lb, 256, 16000)
    assert np.array_equal(sec, (planted * 256.0 / 16000.0).astype(np.float32)) and not sec[tok == 0].any()
    assert np.array_equal(align.path(span[0], la), O.path_from_span(span[0], la))
    dist = align.log_mel_dtw(torch.from_numpy(a).to(DEV)[None], torch.from_numpy(b).to(DEV)[None])
    assert dist.shape == (1,) and float(dist[0]) == 0.0


def test_wav_dtw_distance_goes_through_the_mel_filter():
    from viettts_amd import resynth

    rng = np.random.RandomState(21)
    wa, wb = (0.1 * rng.standard_normal((2, 6000))).astype(np.float32), (0.1 * rng.standard_normal((2, 9000))).astype(np.float32)
    na, nb = [6000, 4100], [9000, 5000]
    got = align.wav_dtw_distance(wa, wb, na, nb).cpu().numpy()
    mf = resynth.default_mel_filter(torch.device(DEV))
    ma, mb = resynth.wav2mel(wa, na, mf).cpu().numpy(), resynth.wav2mel(wb, nb, mf).cpu().numpy()
    for n in range(2):
        la, lb = mf.num_frames(na[n]), mf.num_frames(nb[n])
        total, path_len, _ = O.dtw_f32(ma[n, :la], mb[n, :lb])
        assert got[n] == float(total) / (path_len * 80) and got[n] > 0
    same = align.wav_dtw_distance(wa, wa, na, na).cpu().numpy()
    assert same.tolist() == [0.0, 0.0]


def test_align_end_to_end_with_synthetic_models():
    """Seeded synthetic duration / acoustic models; the "recordings" are what the generator makes of the model's own mel.  Checked: the frames
    per token sum to each recording's frame count, tokens of no query frames get none, the span is the oracle's on the two mels copied to
    the host, and the AcousticInput goes through gta.forward_fn.  Nothing here says anything about alignment quality."""
    from viettts_amd.hifigan.config import V1
    from viettts_amd.hifigan.generator import Generator
    from viettts_amd.hifigan.synth import synthetic_params
    from viettts_amd.nat import gta
    from viettts_amd.nat.acoustic import AcousticModel
    from viettts_amd.nat.config import FLAGS
    from viettts_amd.nat.dsp import MelFilter
    from viettts_amd.nat.duration import DurationModel
    from viettts_amd.nat.synth import synthetic_acoustic_checkpoint, synthetic_duration_checkpoint
    from viettts_amd.nat.text2mel import frame_plan
    from viettts_amd.pipeline import synthesize_sentences

    dm, am = DurationModel(device=DEV), AcousticModel(device=DEV)
    dm.load_params(*synthetic_duration_checkpoint())
    am.load_params(*synthetic_acoustic_checkpoint())
    gen = Generator(V1, device=DEV, dtype="f32")
    gen.load_params(synthetic_params(V1, 4321, "scaled"))
    mf = MelFilter(16000, 1024, 80, 0.0, 8000, device=DEV)
    try:
        rng = np.random.default_rng(41)
        sents = [[FLAGS.sil_index] + [int(v) for v in rng.integers(4, 90, size=int(rng.integers(3, 12)))] + [FLAGS.word_end_index, FLAGS.sil_index] for _ in range(3)]
        wavs = synthesize_sentences(sents, dm, am, gen, silence_duration=0.05, out_dtype="pcm16")
        wl = [int(wavs[i].shape[0]) for i in range(3)]
        pcm = np.zeros((3, max(wl)), dtype=np.int16)
        for i in range(3):
            pcm[i, : wl[i]] = wavs[i]
        r = align.align(pcm, sents, wl, dm, am, mel_filter=mf, silence_duration=0.05)
        torch.cuda.synchronize()
        frames_q, la, _ = frame_plan(sents, dm(sents), 0.05)
        assert r.la == la and r.lb == [n // 256 for n in wl]
        span = r.dtw.span.cpu().numpy()
        q, t = r.query_mel.cpu().numpy(), r.target_mel.cpu().numpy()
        for i in range(3):
            L = len(sents[i])
            assert r.frames[i, :L].sum() == r.lb[i] and (r.frames[i] >= 0).all() and not r.frames[i, L:].any()
            edges = np.concatenate([[0], align.token_edges(frames_q[i], la[i])])
            empty = np.diff(edges) == 0
            assert empty[L - 2] and not r.frames[i, :L][empty].any()  # the word-end token has no duration, and keeps none
            want = O.dtw_f32(q[i, : la[i]], t[i, : r.lb[i]])
            assert float(r.dtw.total[i]) == float(want[0]) and int(r.dtw.path_len[i]) == want[1] and np.array_equal(span[i, : la[i]], want[2])
            assert r.distance[i] == float(want[0]) / (want[1] * 80)
            assert np.array_equal(r.batch.durations[i, :L], (r.frames[i, :L] * 256.0 / 16000.0).astype(np.float32))
        assert r.batch.phonemes.shape == r.batch.durations.shape and [int(v) for v in r.batch.lengths] == [len(s) for s in sents]
        mel = gta.forward_fn(am, mf, np.array([0, 42], dtype=np.uint32), r.batch)
        assert mel.shape == (3, max(r.lb), 80) and np.isfinite(mel).all()
    finally:
        for h in (dm, am, gen, mf):
            h.close()
