"""The MCD kernels (include/vtts_mcd.h, viettts_amd/csrc/mcd.hip) on the GPU against the numpy float32 restatement of the contract
(tests/_mcd_oracle.py; tests/test_mcd_cpu.py checks that one against a float64 oracle built on scipy's DCT).  Cepstra, per-frame distances,
the float64 sums, total, path_len and span are compared with ==: the contract fixes every operation and its order.  Only the end-to-end
checks against the float64 oracle use a tolerance: the bound derived in tests/_mcd_oracle.py.

Every output of a C-ABI call below is pre-filled with NaN or -7.  T and S in the sizes are VTTS_DTW_TILE and VTTS_DTW_STRIP, F is
VTTS_MCD_FRAMES_PER_BLOCK, all read from the headers.
"""
import ctypes as C
import re
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest
import torch

import _dtw_oracle as DO
import _mcd_oracle as O
import _row_split as RS
from viettts_amd import _lib, align, mcd
from viettts_amd._handle import ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KD, KM = DO.header_constants(), O.header_constants()
T, S, F = KD["VTTS_DTW_TILE"], KD["VTTS_DTW_STRIP"], KM["VTTS_MCD_FRAMES_PER_BLOCK"]
CSRC = Path(__file__).resolve().parents[1] / "viettts_amd" / "csrc"
SHAPES = [(80, 13), (80, 1), (80, 64), (3, 2), (128, 13), (81, 12)]
LENGTHS = [1, 2, F - 1, F, F + 1, 257]
PAIRS = [(1, 1), (1, 9), (9, 1), (T - 3, T + 5), (T + 7, T - 2), (S + 3, S - 5), (S - 2, S + 9), (2 * S + 1, 37)]


@pytest.fixture(scope="module")
def mcds():
    assert torch.cuda.is_available()
    made = {}

    def get(n_mels=80, n_ceps=13, band=0, **kw):
        key = (n_mels, n_ceps, band, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = mcd.Mcd(n_mels, n_ceps, band, DEV, **kw)
        return made[key]

    yield get
    for m in made.values():
        m.close()


def _dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)


def _i32(v):
    return (C.c_int32 * len(v))(*[int(x) for x in v])


def _raw_cepstra(m, x, lens):
    """vtts_mcd_cepstra, the whole batch in ONE call, into an output pre-filled with NaN."""
    xt = _dev(x)
    N, Tx = xt.shape[0], xt.shape[1]
    out = torch.full((N, Tx, m.n_ceps), float("nan"), dtype=torch.float32, device=DEV)
    m._on_stream("cepstra", ptr(xt), N, Tx, _i32(lens), ptr(out))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _raw_aligned(m, a, b, lens, f_stride=None):
    at, bt_ = _dev(a), _dev(b)
    N, Tmin = at.shape[0], min(at.shape[1], bt_.shape[1])
    total = torch.full((N,), float("nan"), dtype=torch.float64, device=DEV)
    frames = None if f_stride is None else torch.full((N, f_stride), float("nan"), dtype=torch.float32, device=DEV)
    ws = m._workspace(m.aligned_workspace_bytes(N, Tmin)).fill_(0xFF)
    m._on_stream("aligned", ptr(at), ptr(bt_), N, at.shape[1], bt_.shape[1], _i32(lens), ptr(total), ptr(frames), f_stride or 0, ptr(ws), ws.numel())
    torch.cuda.synchronize()
    return total.cpu().numpy(), None if frames is None else frames.cpu().numpy()


def _raw_dtw(m, ca, cb, las, lbs):
    at, bt_ = _dev(ca), _dev(cb)
    N, Ta, Tb = at.shape[0], at.shape[1], bt_.shape[1]
    total = torch.full((N,), float("nan"), dtype=torch.float32, device=DEV)
    path_len = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    span = torch.full((N, Ta, 2), -7, dtype=torch.int32, device=DEV)
    ws = m._workspace(m.dtw_workspace_bytes(N, Ta, Tb)).fill_(0xFF)
    m._on_stream("dtw", ptr(at), ptr(bt_), N, Ta, Tb, _i32(las), _i32(lbs), ptr(total), ptr(path_len), ptr(span), ptr(ws), ws.numel())
    torch.cuda.synchronize()
    return total.cpu().numpy(), path_len.cpu().numpy(), span.cpu().numpy()


def _assert_dtw(got, n, want, la, what):
    total, path_len, span = got
    assert total[n].dtype == np.float32 and total[n] == want[0], (what, "total", float(total[n]), float(want[0]))
    assert path_len[n] == want[1], (what, "path_len", int(path_len[n]), want[1])
    assert np.array_equal(span[n, :la], want[2]), (what, "span")
    assert (span[n, la:] == -1).all(), (what, "span rows past la")


def _ragged(seed, lens, stride, M, junk):
    """[N, stride, M]: row n's first lens[n] frames are mel-like; behind them NaN (even rows) or 1e4 N(0, 1) (odd rows) when ``junk``."""
    rng = np.random.RandomState(seed)
    x = np.empty((len(lens), stride, M), dtype=np.float32)
    for n, L in enumerate(lens):
        x[n] = (1e4 * rng.standard_normal((stride, M))).astype(np.float32) if (n % 2 and junk) else (np.nan if junk else 0.0)
        x[n, :L] = O.speechlike_mels(seed * 100 + n, L, M) if L else 0
    return x


@lru_cache(maxsize=None)
def _table(M, Kc):
    return O.basis(M, Kc)


# ------------------------------------------------------------ cepstra ------------------------------------------------------------
@pytest.mark.parametrize("M,Kc", SHAPES)
def test_cepstra_equal_the_restatement(mcds, M, Kc):
    m = mcds(M, Kc)
    assert np.array_equal(m.basis(), _table(M, Kc))
    lens = LENGTHS + [0]
    stride = max(lens) + 3
    x = _ragged(M + Kc, lens, stride, M, junk=True)
    got = _raw_cepstra(m, x, lens)
    for n, L in enumerate(lens):
        want = O.cepstra_f32(x[n, :L], _table(M, Kc))
        assert np.array_equal(got[n, :L], want), (n, L)
        assert not got[n, L:].any() and np.isfinite(got[n]).all(), (n, L, "zeros past the length")
        if L:
            alone = m.cepstra(np.array(x[n, :L])).cpu().numpy()  # the row alone, at its own stride ...
            wide = np.full((1, stride + F + 5, M), np.nan, dtype=np.float32)  # ... and at a larger one
            wide[0, :L] = x[n, :L]
            assert np.array_equal(alone[0], got[n, :L]) and np.array_equal(_raw_cepstra(m, wide, [L])[0, :L], got[n, :L]), (n, L)


# ------------------------------------------------------------ aligned ------------------------------------------------------------
@pytest.mark.parametrize("M,Kc", [(80, 13), (80, 64), (3, 2), (81, 12)])
def test_aligned_equals_the_restatement(mcds, M, Kc):
    m = mcds(M, Kc)
    lens = LENGTHS + [0]
    a = _ragged(7 * M + Kc, lens, max(lens) + 3, M, junk=True)
    b = _ragged(9 * M + Kc, lens, max(lens) + 10, M, junk=True)  # Ta_stride != Tb_stride
    f_stride = max(lens) + 2 * F  # past the last block of the grid as well
    total, frames = _raw_aligned(m, a, b, lens, f_stride)
    total_only, none = _raw_aligned(m, a, b, lens)
    assert none is None and np.array_equal(total, total_only)  # frame_dev NULL and given: one sum
    for n, L in enumerate(lens):
        _, d, s = O.mcd_aligned_f32(a[n], b[n], L, K=Kc, block=F)
        assert np.array_equal(frames[n, :L], d) and not frames[n, L:].any(), (n, L)
        assert total[n] == s and total.dtype == np.float64, (n, L, total[n], s)
        if L:  # d(t, t) is the diagonal of the cost the DTW runs on
            table = _table(M, Kc)
            assert np.array_equal(np.diag(O.cost_f32(O.cepstra_f32(a[n, :L], table), O.cepstra_f32(b[n, :L], table))), d)
    same, same_frames = _raw_aligned(m, a, a, lens, f_stride)
    assert not same.any() and not same_frames.any()  # exactly 0
    # the Python owner: dB, nan for the empty row, the frames on request
    db, fr = m.aligned(a, b, lens, frames=True)
    db2 = m.aligned(a, b, lens)
    torch.cuda.synchronize()
    db, db2, fr = db.cpu().numpy(), db2.cpu().numpy(), fr.cpu().numpy()
    assert np.array_equal(db[:-1], db2[:-1]) and np.isnan(db[-1]) and np.array_equal(fr, frames[:, : fr.shape[1]])
    assert np.array_equal(db[:-1], O.ALPHA * total[:-1] / np.asarray(lens[:-1], dtype=np.float64))
    # a row alone, at strides of its own
    n = lens.index(F + 1)
    alone = m.aligned(np.array(a[n, : F + 1]), np.array(b[n, : F + 9]), [F + 1]).cpu().numpy()
    assert alone[0] == db[n]


def test_aligned_frame_distance_is_the_dtw_cost_of_one_by_one_pairs(mcds):
    m = mcds(80, 13)
    L = F + 3
    a, b = O.mel_pair(5, L, L)
    total, frames = _raw_aligned(m, a[None], b[None], [L], L)
    r = m.dtw(a[:, None, :].copy(), b[:, None, :].copy())  # L pairs of one frame each: total = d(t, t)
    torch.cuda.synchronize()
    assert np.array_equal(r.total.cpu().numpy(), frames[0]) and (r.path_len.cpu().numpy() == 1).all() and not r.span.cpu().numpy().any()


# ------------------------------------------------------------ dtw ------------------------------------------------------------
def _pair_batch(seed, M, pairs):
    las, lbs = [p[0] for p in pairs], [p[1] for p in pairs]
    a = np.full((len(pairs), max(las) + 2, M), np.nan, dtype=np.float32)
    b = np.full((len(pairs), max(lbs) + 5, M), np.nan, dtype=np.float32)
    for n, (la, lb) in enumerate(pairs):
        a[n, :la], b[n, :lb] = O.mel_pair(seed + n, la, lb, M)
    return a, b, las, lbs


@lru_cache(maxsize=None)
def _dtw_cepstra(Kc):
    """The eight pairs' mels and the restatement's cepstra of them (zeros past the lengths), once per K."""
    a, b, las, lbs = _pair_batch(40 + Kc, 80, PAIRS)
    ca, cb = np.zeros(a.shape[:2] + (Kc,), np.float32), np.zeros(b.shape[:2] + (Kc,), np.float32)
    for n in range(len(PAIRS)):
        ca[n, : las[n]], cb[n, : lbs[n]] = O.cepstra_f32(a[n, : las[n]], _table(80, Kc)), O.cepstra_f32(b[n, : lbs[n]], _table(80, Kc))
    return a, b, las, lbs, ca, cb


@pytest.mark.parametrize("band", [0, 1, 2, 32])
@pytest.mark.parametrize("Kc", [13, 1, 64])
def test_dtw_equals_the_restatement(mcds, Kc, band):
    """The eight pairs as one ragged batch (NaN behind every length), through cepstra() and dtw() as the Python owner runs them."""
    m = mcds(80, Kc, band)
    a, b, las, lbs, ca, cb = _dtw_cepstra(Kc)
    got_ca, got_cb = _raw_cepstra(m, a, las), _raw_cepstra(m, b, lbs)
    assert np.array_equal(got_ca, ca) and np.array_equal(got_cb, cb)
    got = _raw_dtw(m, got_ca, got_cb, las, lbs)
    for n, (la, lb) in enumerate(PAIRS):
        D, codes = DO.accumulate(O.cost_f32(ca[n, :la], cb[n, :lb]), band)
        want = (D[-1, -1],) + DO.backtrace(codes)
        assert np.isfinite(want[0]) and DO.path_in_band(want[2], la, lb, band)
        _assert_dtw(got, n, want, la, (la, lb, Kc, band))
    r = m.dtw(a, b, las, lbs)
    torch.cuda.synchronize()
    assert np.array_equal(r.total.cpu().numpy(), got[0]) and np.array_equal(r.path_len.cpu().numpy(), got[1]) and np.array_equal(r.span.cpu().numpy(), got[2])
    assert np.array_equal(r.mcd.cpu().numpy(), O.ALPHA * got[0].astype(np.float64) / got[1].astype(np.float64))
    if (Kc, band) in ((13, 0), (13, 2)):  # each pair alone, at its own strides
        for n, (la, lb) in enumerate(PAIRS):
            alone = _raw_dtw(m, ca[n : n + 1, :la], cb[n : n + 1, :lb], [la], [lb])
            assert alone[0][0] == got[0][n] and alone[1][0] == got[1][n] and np.array_equal(alone[2][0], got[2][n, :la]), (n, band)


@pytest.mark.parametrize("la,lb,count", DO.tie_sizes())
def test_dtw_tie_rich_grid_inputs(mcds, la, lb, count):
    """Cepstra on the 1/8 grid handed to dtw() directly.  With K = 1 the distance is |a - b| exactly and every sum is exact: the seeds are
    those whose span changes under EVERY other order of trying the predecessors (tests/_dtw_oracle.py: tie_seeds), so the comparison cannot
    pass with another tie rule.  With K = 13 the distances are roots of multiples of 1/64: still full of ties, compared as they come."""
    m1, m13 = mcds(80, 1), mcds(80, 13)
    for seed in DO.tie_seeds(la, lb, min(count, 2), D=1):
        a, b = DO.grid_pair(seed, la, lb, 1)
        D, codes = DO.accumulate(O.cost_f32(a, b), 0)
        want = (D[-1, -1],) + DO.backtrace(codes)
        ref = DO.dtw_f32(a, b)
        assert want[0] == ref[0] and want[1] == ref[1] and np.array_equal(want[2], ref[2]) and float(want[0]) == DO.dtw_f64(a, b)
        _assert_dtw(_raw_dtw(m1, a[None], b[None], [la], [lb]), 0, want, la, (la, lb, seed))
    for band in (0, 2):
        a, b = DO.grid_pair(la + band, la, lb, 13)
        D, codes = DO.accumulate(O.cost_f32(a, b), band)
        m = mcds(80, 13, band) if band else m13
        _assert_dtw(_raw_dtw(m, a[None], b[None], [la], [lb]), 0, (D[-1, -1],) + DO.backtrace(codes), la, (la, lb, "grid 13", band))


# ------------------------------------------------------------ the rows-per-launch split ------------------------------------------------------------
def _split_constant(name, pattern):
    found = re.findall(pattern, (CSRC / name).read_text(), flags=re.M)
    assert len(found) == 1, (name, found)
    return int(found[0])


def test_rows_behind_the_launch_split(mcds):
    """P + 3 rows in one call of each entry (tests/_row_split.py): the rows behind the split differ from the first ones in content and in
    length, and hold the longest row and the shortest.  P comes from the sources' host loops."""
    P = _split_constant("mcd.hip", r"^constexpr int ROWS_PER_LAUNCH = (\d+);")
    PD = _split_constant("dtw_common.h", r"^constexpr int DTW_PAIRS_PER_LAUNCH = (\d+);")
    assert P == _lib.MCD_ROWS_PER_LAUNCH == KM["VTTS_MCD_ROWS_PER_LAUNCH"] and PD == _lib.DTW_PAIRS_PER_LAUNCH
    src = (CSRC / "mcd.hip").read_text()
    assert len(re.findall(r"for_each_launch(?:_off)?<ROWS_PER_LAUNCH>\(", src)) == 2 and len(re.findall(r"\+= vtts::DTW_PAIRS_PER_LAUNCH\)", src)) == 1
    assert len(re.findall(r"\+= ROWS_PER_LAUNCH\)", src)) == 0  # launch_rows.h's loop, and no hand-written one
    M, Kc, St = 8, 4, F + 6
    m = mcds(M, Kc)
    table = _table(M, Kc)

    def rows(seed, lengths):
        return [RS.Row(np.concatenate([O.speechlike_mels(seed + i, St, M), O.speechlike_mels(seed + 50 + i, St, M)], axis=1), n) for i, n in enumerate(lengths)]

    bt = RS.split_batch(P, rows(100, (17, 30, 5)), rows(200, (0, St, 29)), rows(300, (12, 33, 2, F + 1)), min_length=0)
    a, b = np.ascontiguousarray(bt.rows[:, :, :M]), np.ascontiguousarray(bt.rows[:, :, M:])
    assert bt.N == P + 3
    want_c = RS.per_kind(bt, lambda r: O.cepstra_f32(r.content[: r.length, :M], table))
    want_a = RS.per_kind(bt, lambda r: O.mcd_aligned_f32(r.content[:, :M], r.content[:, M:], r.length, K=Kc, block=F))
    got_c = _raw_cepstra(m, a, bt.lengths)
    total, frames = _raw_aligned(m, a, b, bt.lengths, St)
    for n in range(bt.N):
        L = bt.lengths[n]
        assert np.array_equal(got_c[n, :L], want_c[n]) and not got_c[n, L:].any(), n
        assert total[n] == want_a[n][2] and np.array_equal(frames[n, :L], want_a[n][1]) and not frames[n, L:].any(), n
    # dtw: tests/_row_split.py's pairs, their 8 columns read as cepstra
    m8 = mcds(9, 8)
    for band in (0, RS.DTW_NARROW_BAND):
        bd = RS.dtw_batch(PD)
        ca, cb, las, lbs = RS.dtw_pairs(bd)
        Ta = ca.shape[1]

        def one(r):
            D, codes = DO.accumulate(O.cost_f32(r.content[: r.length // 64], r.content[Ta : Ta + r.length % 64]), band)
            return (D[-1, -1],) + DO.backtrace(codes)

        want = RS.per_kind(bd, one)
        got = _raw_dtw(mcds(9, 8, band) if band else m8, ca, cb, las, lbs)
        for n in range(bd.N):
            _assert_dtw(got, n, want[n], las[n], (n, las[n], lbs[n], band))


# ------------------------------------------------------------ end to end ------------------------------------------------------------
def test_mel_functions_agree_with_the_float64_oracle_within_the_derived_bound():
    Ta, Tb = 90, 75
    a, b = O.mel_pair(11, Ta, Tb)
    got = mcd.mel_mcd(_dev(a[None, :Tb]), _dev(b[None]))
    r = mcd.mel_mcd_dtw(_dev(a[None]), _dev(b[None]))
    torch.cuda.synchronize()
    want, bound = O.mcd_aligned_f64(a[:Tb], b), O.aligned_bound(a[:Tb], b)
    print(f"\nmel_mcd {float(got[0]):.6f} dB, float64 {want:.6f} dB, bound {bound:.3g}")
    assert got.dtype == torch.float64 and abs(float(got[0]) - want) <= bound
    t64, n64, s64 = O.mcd_dtw_f64(a, b)
    tb = O.dtw_total_bound(a, b)
    print(f"mel_mcd_dtw total {float(r.total[0]):.6f}, float64 {t64:.6f}, bound {tb:.3g}; path {int(r.path_len[0])} / {n64} cells")
    assert abs(float(r.total[0]) - t64) <= tb
    assert int(r.path_len[0]) == n64 and np.array_equal(r.span[0].cpu().numpy(), s64)  # one path (tests/test_mcd_cpu.py asserts it for the restatement on such pairs)
    assert abs(float(r.mcd[0]) - O.ALPHA * t64 / n64) <= O.ALPHA * tb / n64


def test_wav_mcd_goes_through_the_mel_filter():
    from viettts_amd import resynth

    na, nb = [6000, 4100], [6000, 5000]
    wa = np.stack([RS.speechlike(31 + i, 6000) for i in range(2)])
    wb = np.stack([RS.speechlike(31 + i, 6000) + 0.02 * np.random.RandomState(i).standard_normal(6000).astype(np.float32) for i in range(2)])
    got = mcd.wav_mcd(wa, wb, na, nb).cpu().numpy()
    dt = mcd.wav_mcd(wa, wb, na, nb, dtw=True, band=4)
    mf = resynth.default_mel_filter(torch.device(DEV))
    ma, mb = resynth.wav2mel(wa, na, mf).cpu().numpy(), resynth.wav2mel(wb, nb, mf).cpu().numpy()
    for n in range(2):
        la, lb = mf.num_frames(na[n]), mf.num_frames(nb[n])
        L = min(la, lb)
        assert got[n] == O.mcd_aligned_f32(ma[n], mb[n], L, block=F)[0] and got[n] > 0
        assert abs(got[n] - O.mcd_aligned_f64(ma[n], mb[n], L)) <= O.aligned_bound(ma[n, :L], mb[n, :L])
        want = O.mcd_dtw_f32(ma[n, :la], mb[n, :lb], band=4)
        assert float(dt.total[n]) == float(want[0]) and int(dt.path_len[n]) == want[1] and np.array_equal(dt.span[n, :la].cpu().numpy(), want[2])
        assert abs(float(dt.total[n]) - O.mcd_dtw_f64(ma[n, :la], mb[n, :lb], band=4)[0]) <= O.dtw_total_bound(ma[n, :la], mb[n, :lb])
    assert mcd.wav_mcd(wa, wa, na, na).cpu().numpy().tolist() == [0.0, 0.0]
    same = mcd.wav_mcd(wa, wa, na, na, dtw=True)
    assert same.mcd.cpu().numpy().tolist() == [0.0, 0.0] and same.path_len.cpu().numpy().tolist() == [mf.num_frames(n) for n in na]


def test_the_l1_dtw_is_unchanged_beside_it(mcds):
    """One call of the existing contract after the MCD kernels have run on the same inputs."""
    a, b = O.mel_pair(21, T + 7, S + 3)
    r = mcds(80, 13).dtw(a, b)
    d = align.Dtw(80, 0, DEV)
    res = d.dtw(a, b)
    torch.cuda.synchronize()
    want = DO.dtw_f32(a, b)
    assert float(res.total[0]) == float(want[0]) and int(res.path_len[0]) == want[1] and np.array_equal(res.span[0].cpu().numpy(), want[2])
    assert float(r.total[0]) == float(O.mcd_dtw_f32(a, b)[0])
    assert float(align.log_mel_dtw(_dev(a[None]), _dev(b[None]))[0]) == float(want[0]) / (want[1] * 80)
    d.close()
