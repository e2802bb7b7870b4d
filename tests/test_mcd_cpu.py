"""include/vtts_mcd.h without a GPU: the basis, closed forms of the float64 oracle, the float32 restatement (tests/_mcd_oracle.py) against
the float64 oracle within the derived bound, planted faults far outside it, the vectorised restatement against a cell-by-cell one, the C
ABI's host side and the Python / command-line argument errors.

The bound between the float32 contract and float64 is DERIVED, not measured (tests/_mcd_oracle.py's docstring): the
table is the basis rounded once and the cepstrum a dot product of M terms, so |c32 - c| <= gamma_(M+2) sum_m |dct[k][m] x[m]|; the
difference of two cepstra adds one rounding; the distance is a dot product of K terms under a correctly rounded root, so
|d32 - d| <= |E|_2 + gamma_(K+2) d32 with E_k the bound on the k-th difference; the aligned MCD is alpha times the mean of those, and the DTW
total moves by at most the worst path's accumulated bound, (la + lb - 1) (max B_d + gamma_(la+lb) max d32).
"""
import ctypes as C
import math
import re

import numpy as np
import pytest

import _dtw_oracle as DO
import _mcd_oracle as O
from viettts_amd import _lib

K = O.header_constants()
FAR = 100.0  # a planted fault misses the float64 oracle by at least this many times the (worst-case) bound


@pytest.fixture(scope="module")
def lib():
    from viettts_amd.csrc.build import build

    build()
    return _lib.load()


def _create(lib, n_mels=80, n_ceps=13, band=0, max_frames=_lib.DTW_MAX_FRAMES):
    h = C.c_void_p(0)
    rc = lib.vtts_mcd_create(C.byref(_lib.McdCfg(n_mels, n_ceps, band, max_frames)), 0, C.byref(h))
    return rc, h


# ------------------------------------------------------------ the basis ------------------------------------------------------------
@pytest.mark.parametrize("M,Kc", [(80, 13), (80, 1), (80, 64), (3, 2), (128, 13), (81, 12), (128, 64), (2, 1)])
def test_basis_is_the_oracles_bit_for_bit_orthonormal_and_scipys(lib, M, Kc):
    from scipy.fft import dct

    rc, h = _create(lib, M, Kc)
    assert rc == 0
    got = np.full((Kc, M), np.nan, dtype=np.float32)
    assert lib.vtts_mcd_basis(h, got.ctypes.data_as(_lib.fp)) == 0
    lib.vtts_mcd_destroy(h)
    want = O.basis(M, Kc)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    g = got.astype(np.float64)
    assert np.abs(g @ g.T - np.eye(Kc)).max() <= 1e-7
    exact = dct(np.eye(M), type=2, norm="ortho", axis=0)[1 : Kc + 1]  # column m is the transform of e_m: row k is dct[k][:]
    # one float32 rounding of scipy's float64 value; the slack is the double rounding of the cosine's argument (below pi K, three operations)
    assert (np.abs(g - exact) <= 2.0 ** -24 * np.abs(exact) + 2.0 ** -50 * math.pi * Kc).all()


def test_alpha_is_the_headers_and_the_bindings():
    assert K["VTTS_MCD_ALPHA"] == _lib.MCD_ALPHA == O.ALPHA == 10.0 * math.sqrt(2.0) / math.log(10.0)
    assert K["VTTS_MCD_MAX_MELS"] == _lib.MCD_MAX_MELS and K["VTTS_MCD_MAX_CEPS"] == _lib.MCD_MAX_CEPS
    assert K["VTTS_MCD_FRAMES_PER_BLOCK"] == _lib.MCD_FRAMES_PER_BLOCK and K["VTTS_MCD_ROWS_PER_LAUNCH"] == _lib.MCD_ROWS_PER_LAUNCH


# ------------------------------------------------------------ closed forms, float64 ------------------------------------------------------------
def _exact_row(M, k):
    return math.sqrt((1.0 if k == 0 else 2.0) / M) * np.cos(np.pi * k * (2 * np.arange(M) + 1) / (2.0 * M))


def test_closed_forms_in_float64():
    M, Kc, T = 80, 13, 9
    a = O.speechlike_mels(1, T, M).astype(np.float64)
    assert O.mcd_aligned_f64(a, a, K=Kc) == 0.0
    for k in range(0, M, 1):
        for delta in (0.25, -1.5):
            got = O.mcd_aligned_f64(a, a + delta * _exact_row(M, k)[None, :], K=Kc)
            want = O.ALPHA * abs(delta) if 1 <= k <= Kc else 0.0
            assert abs(got - want) <= 1e-12, (k, delta, got, want)


@pytest.mark.parametrize("seed,la", [(0, 30), (1, 61), (2, 7)])
def test_planted_warp_gives_zero_and_the_repeat_counts(seed, la):
    """A warp planted on the cepstra's inputs: identical frames have identical cepstra, so the distance along the planted path is exactly 0
    in float32 and in float64, and the spans are the repeat counts."""
    a, b, reps = DO.planted_warp(seed, la, 80)
    starts = np.concatenate([[0], np.cumsum(reps)[:-1]])
    for total, n, span in (O.mcd_dtw_f64(a, b), O.mcd_dtw_f32(a, b)):
        assert total == 0 and n == len(b)
        assert np.array_equal(span[:, 0], starts) and np.array_equal(span[:, 1], starts + reps - 1)


# ------------------------------------------------------------ float32 against float64 ------------------------------------------------------------
CASES = [(80, 13, 70, 3), (80, 64, 33, 4), (80, 1, 20, 5), (3, 2, 65, 6), (128, 13, 17, 7), (81, 12, 40, 8)]


@pytest.mark.parametrize("M,Kc,T,seed", CASES)
def test_f32_restatement_is_within_the_derived_bound_of_float64(M, Kc, T, seed):
    """See the module docstring for the derivation.  Also checked: the bound on the aligned figure stays below a tenth of a dB, under what
    papers resolve, and the planted faults below miss by orders of magnitude more."""
    a, b = O.mel_pair(seed, T, T + 5, M)
    got, _, _ = O.mcd_aligned_f32(a, b, K=Kc)
    want, bound = O.mcd_aligned_f64(a, b, K=Kc), O.aligned_bound(a, b, K=Kc)
    print(f"\nM {M} K {Kc}: MCD32 {got:.6f} dB, MCD64 {want:.6f} dB, |diff| {abs(got - want):.3g}, bound {bound:.3g}")
    assert abs(got - want) <= bound <= 0.1, (got, want, bound)
    t32, n32, s32 = O.mcd_dtw_f32(a, b, Kc)
    t64, n64, s64 = O.mcd_dtw_f64(a, b, Kc)
    tb = O.dtw_total_bound(a, b, Kc)
    assert abs(float(t32) - t64) <= tb, (float(t32), t64, tb)
    assert n32 == n64 and np.array_equal(s32, s64)  # one path on these inputs: the MCD-DTW figures are comparable
    assert abs(O.ALPHA * float(t32) / n32 - O.ALPHA * t64 / n64) <= O.ALPHA * tb / n64


@pytest.mark.parametrize("fault", ["c0", "rows", "unnormalised", "no_root", "alpha"])
def test_planted_faults_miss_the_float64_oracle_by_far(fault):
    M, Kc, T = 80, 13, 70
    a, b = O.mel_pair(3, T, T, M)
    want, bound = O.mcd_aligned_f64(a, b, K=Kc), O.aligned_bound(a, b, K=Kc)
    kw = {"c0": dict(table=np.concatenate([(O.basis(M, 1, first=0) / np.float32(math.sqrt(2.0))).astype(np.float32), O.basis(M, Kc)])),
          "rows": dict(table=np.concatenate([(O.basis(M, 1, first=0) / np.float32(math.sqrt(2.0))).astype(np.float32), O.basis(M, Kc - 1)])),
          "unnormalised": dict(table=O.basis(M, Kc, normalised=False)),
          "no_root": dict(root=False),
          "alpha": dict(alpha=10.0 / math.log(10.0))}[fault]
    got, _, _ = O.mcd_aligned_f32(a, b, K=Kc, **kw)
    assert abs(got - want) >= FAR * bound, (fault, got, want, bound)
    if fault in ("c0", "rows", "unnormalised", "no_root"):  # the DTW total sees the cost's faults as well (alpha is applied behind it)
        t64 = O.mcd_dtw_f64(a, b, Kc)[0]
        t32 = float(O.mcd_dtw_f32(a, b, Kc, table=kw.get("table"), root=kw.get("root", True))[0])
        assert abs(t32 - t64) >= 10.0 * O.dtw_total_bound(a, b, Kc), (fault, t32, t64)


@pytest.mark.parametrize("la,lb,band", [(13, 9, 0), (9, 13, 0), (12, 12, 2), (7, 15, 1), (15, 7, 2), (1, 6, 1), (6, 1, 0)])
def test_vectorised_restatement_equals_the_cell_by_cell_one(la, lb, band):
    for seed in range(2):
        a, b = O.speechlike_mels(seed, la, 20), O.speechlike_mels(seed + 50, lb, 20)
        table = O.basis(20, 5)
        ca, cb = O.cepstra_f32(a, table), O.cepstra_f32(b, table)
        t0, n0, s0 = O.mcd_dtw_f32(a, b, 5, band)
        t1, n1, s1 = O.dtw_cells_f32(ca, cb, band)
        assert t0 == t1 and n0 == n1 and np.array_equal(s0, s1)
        # the cepstrum chain, scalar by scalar
        s = np.float32(0.0)
        for m in range(20):
            s = np.float32(s + np.float32(table[2, m] * a[la - 1, m]))
        assert s == ca[la - 1, 2]
        assert np.array_equal(np.diag(O.cost_f32(ca, cb))[: min(la, lb)], O.frames_f32(ca, cb))  # d(t, t) is the cost's diagonal


def test_aligned_sum_order_is_by_blocks():
    d = (np.random.RandomState(0).standard_normal(150) ** 2).astype(np.float32)
    s = O.aligned_sum(d, 64)
    assert s == (float(np.cumsum(d[:64].astype(np.float64))[-1]) + float(np.cumsum(d[64:128].astype(np.float64))[-1])) + float(np.cumsum(d[128:].astype(np.float64))[-1])
    assert O.aligned_sum(d[:0], 64) == 0.0


# ------------------------------------------------------------ the C ABI's host side ------------------------------------------------------------
def test_header_symbols_all_exported(lib):
    declared = set(re.findall(r"\b(vtts_mcd_[a-z_0-9]+)\s*\(", O.HEADER.read_text())) - {"vtts_mcd_cfg"}
    assert declared == set(_lib.MCD_EXPORTS) == {f"vtts_mcd_{n}" for n in ("create", "destroy", "basis", "cepstra", "aligned_workspace_bytes", "aligned",
                                                                         "dtw_workspace_bytes", "dtw")}
    for name in declared:
        fn = getattr(lib, name)
        assert fn.restype is _lib.MCD_SIGS[name][0] and list(fn.argtypes) == _lib.MCD_SIGS[name][1]
    assert not set(_lib.MCD_SIGS) & (set(_lib.SIGS) | set(_lib.DTW_SIGS))
    assert set(_lib.DTW_EXPORTS) == {"vtts_dtw_create", "vtts_dtw_destroy", "vtts_dtw_workspace_bytes", "vtts_dtw_forward"}


def test_build_lists_the_new_files():
    from viettts_amd.csrc import build

    assert "mcd.hip" in build.SOURCES and "-fno-slp-vectorize" in build.FILE_FLAGS["mcd.hip"] and "-ffp-contract=off" in build.FILE_FLAGS["mcd.hip"]
    assert "dtw_common.h" in build.HEADERS and any(str(h).endswith("vtts_mcd.h") for h in build.HEADERS)
    assert build.FILE_FLAGS["dtw.hip"] == ["-fno-slp-vectorize"]
    dtw_src = (build.CSRC / "dtw.hip").read_text()
    assert '#include "dtw_common.h"' in dtw_src and '#include "dtw_common.h"' in (build.CSRC / "mcd.hip").read_text()
    assert "dtw_path_launch" not in O.HEADER.read_text() and "dtw_path_launch" not in DO.HEADER.read_text()  # internal


def test_create_validates_without_a_gpu(lib):
    for bad in (dict(n_mels=0), dict(n_mels=129), dict(n_ceps=0), dict(n_ceps=80), dict(n_mels=13, n_ceps=13), dict(n_mels=128, n_ceps=65), dict(band=-1),
                dict(max_frames=0), dict(max_frames=_lib.DTW_MAX_FRAMES + 1)):
        rc, _ = _create(lib, **bad)
        assert rc == -1 and lib.vtts_last_error(), bad
    for good in (dict(n_mels=2, n_ceps=1), dict(n_mels=128, n_ceps=64, band=7, max_frames=1), dict(n_mels=80, n_ceps=64)):
        rc, h = _create(lib, **good)
        assert rc == 0, good
        lib.vtts_mcd_destroy(h)


def _dtw_bytes(N, ta, tb):
    k = DO.header_constants()
    strip, tile, cpw = k["VTTS_DTW_STRIP"], k["VTTS_DTW_TILE"], k["VTTS_DTW_CODES_PER_WORD"]
    cost = -(-ta // strip) * (-(-(tb + strip - 1) // tile) * tile) * strip
    return N * (-(-4 * (cost + ta * -(-tb // cpw)) // 256) * 256)


def _aligned_bytes(N, T):
    return -(-8 * N * -(-T // K["VTTS_MCD_FRAMES_PER_BLOCK"]) // 256) * 256


def test_workspace_formulas_are_the_documented_ones(lib):
    rc, h = _create(lib)
    rc2, d = C.c_int(0), C.c_void_p(0)
    assert rc == 0 and lib.vtts_dtw_create(C.byref(_lib.DtwCfg(13, 0, _lib.DTW_MAX_FRAMES)), 0, C.byref(d)) == 0
    n, m = C.c_size_t(0), C.c_size_t(0)
    for N, ta, tb in [(1, 1, 1), (1, 255, 16), (1, 256, 17), (1, 257, 17), (2, 257, 17), (64, 768, 768), (64, 4096, 4096)]:
        assert lib.vtts_mcd_dtw_workspace_bytes(h, N, ta, tb, C.byref(n)) == 0 and lib.vtts_dtw_workspace_bytes(d, N, ta, tb, C.byref(m)) == 0
        assert n.value == m.value == _dtw_bytes(N, ta, tb)
    for N, ta, tb in [(0, 8, 8), (1, 0, 8), (1, 8, 0), (1, 4097, 8), (1, 8, 4097)]:
        assert lib.vtts_mcd_dtw_workspace_bytes(h, N, ta, tb, C.byref(n)) == -1
    for N, T in [(1, 1), (1, 64), (1, 65), (3, 1000), (64, 1024), (200, 5000)]:
        assert lib.vtts_mcd_aligned_workspace_bytes(h, N, T, C.byref(n)) == 0 and n.value == _aligned_bytes(N, T)
    for N, T in [(0, 8), (1, 0), (1, -3)]:
        assert lib.vtts_mcd_aligned_workspace_bytes(h, N, T, C.byref(n)) == -1
    lib.vtts_mcd_destroy(h)
    lib.vtts_dtw_destroy(d)


def test_calls_refuse_bad_arguments_before_any_launch(lib):
    """No GPU here: every refusal below has to come from host arithmetic.  The pointers are never dereferenced."""
    rc, h = _create(lib, n_mels=8, n_ceps=4, max_frames=64)
    assert rc == 0
    fake = C.c_void_p(0x1000)
    i32 = lambda *v: (C.c_int32 * len(v))(*v)  # noqa: E731
    big = 1 << 30
    # cepstra
    assert lib.vtts_mcd_cepstra(h, None, 2, 8, i32(3, 3), fake, None) == -1
    assert lib.vtts_mcd_cepstra(h, fake, 2, 8, i32(3, 3), None, None) == -1
    assert lib.vtts_mcd_cepstra(h, fake, 0, 8, i32(3, 3), fake, None) == -1
    assert lib.vtts_mcd_cepstra(h, fake, 2, 0, i32(0, 0), fake, None) == -1
    for lens in ((3, 9), (-1, 3)):
        assert lib.vtts_mcd_cepstra(h, fake, 2, 8, i32(*lens), fake, None) == -1 and b"lens" in lib.vtts_last_error()
    # aligned
    al = lambda a, b, N, ta, tb, lens, s, f, fs, ws, nb: lib.vtts_mcd_aligned(h, a, b, N, ta, tb, lens, s, f, fs, ws, nb, None)  # noqa: E731
    assert al(None, fake, 2, 8, 9, i32(3, 3), fake, None, 0, fake, big) == -1
    assert al(fake, None, 2, 8, 9, i32(3, 3), fake, None, 0, fake, big) == -1
    assert al(fake, fake, 2, 8, 9, i32(3, 3), None, None, 0, fake, big) == -1
    assert al(fake, fake, 2, 8, 9, i32(3, 9), fake, None, 0, fake, big) == -1  # one length serves both: it is bounded by the shorter stride
    assert al(fake, fake, 2, 9, 8, i32(9, 3), fake, None, 0, fake, big) == -1
    assert al(fake, fake, 2, 8, 9, i32(3, 5), fake, fake, 4, fake, big) == -1  # ... and by the frame output's
    assert al(fake, fake, 2, 8, 9, None, fake, fake, 4, fake, big) == -1
    assert al(fake, fake, 2, 8, 9, i32(3, 3), fake, None, 0, fake, _aligned_bytes(2, 8) - 1) == -5  # VTTS_ERR_NOMEM
    assert al(fake, fake, 2, 8, 9, i32(3, 3), fake, None, 0, None, big) == -5
    assert al(fake, fake, 2, 8, 9, i32(3, 3), fake, None, 0, C.c_void_p(0x1010), big) == -1  # alignment
    # dtw
    dt = lambda N, ta, tb, la, lb, nb, ws=fake: lib.vtts_mcd_dtw(h, fake, fake, N, ta, tb, la, lb, fake, fake, fake, ws, nb, None)  # noqa: E731
    for la, lb in [((0, 3), (3, 3)), ((3, 9), (3, 3)), ((3, 3), (0, 3)), ((3, 3), (3, 9)), ((-1, 3), (3, 3))]:
        assert dt(2, 8, 8, i32(*la), i32(*lb), big) == -1, (la, lb)
        assert b"pair" in lib.vtts_last_error()
    assert dt(1, 65, 8, i32(3), i32(3), big) == -1  # the stride itself is bounded by max_frames
    assert dt(2, 8, 8, i32(3, 3), i32(3, 3), _dtw_bytes(2, 8, 8) - 1) == -5
    assert dt(2, 8, 8, i32(3, 3), i32(3, 3), big, None) == -5
    assert dt(2, 8, 8, None, i32(3, 3), big) == -1
    assert lib.vtts_mcd_basis(h, None) == -1
    lib.vtts_mcd_destroy(h)


# ------------------------------------------------------------ Python and the command lines ------------------------------------------------------------
def test_python_argument_errors(lib):
    import torch

    from viettts_amd import mcd

    with pytest.raises(ValueError):
        mcd.Mcd(device="cpu")
    for bad in (dict(n_ceps=0), dict(n_ceps=80), dict(n_mels=129), dict(band=-1)):
        with pytest.raises(_lib.VttsError):
            mcd.Mcd(device="cuda:0", **bad)
    m = mcd.Mcd(80, 13, 0, "cuda:0")  # create() touches no HIP call
    assert np.array_equal(m.basis(), O.basis(80, 13))
    host = torch.zeros((2, 5, 80))
    for call in (lambda: m.cepstra(host), lambda: m.aligned(host, host), lambda: m.dtw(host, host), lambda: m.cepstra("x")):
        with pytest.raises(ValueError):
            call()
    m.close()
    assert mcd.ALPHA == O.ALPHA and mcd.McdDtwResult._fields == ("mcd", "total", "path_len", "span")
    for word in ("SPTK", "c0", "soft-DTW", "gradients", "listening tests", "streamed"):
        assert word in mcd.__doc__, word


def test_cli_argument_errors(tmp_path):
    from viettts_amd import mcd, resynth, vocoder_eval, wavio

    a = mcd.build_parser().parse_args(["--ref", "a.wav", "--test", "b.wav"])
    assert not a.dtw and a.band == 0 and a.n_ceps == 13
    for argv in (["--ref", "a.wav"], ["--ref", "a.wav", "--test", "b.wav", "--band", "3"], ["--ref", "a.wav", "--test", "b.wav", "--n-ceps", "0"],
                 ["--ref", "a.wav", "--test", "b.wav", "--dtw", "--band", "-1"]):
        with pytest.raises(SystemExit):
            mcd.main(argv)
    rng = np.random.RandomState(0)
    pa, pb, pc = (str(tmp_path / n) for n in ("a.wav", "b.wav", "c.wav"))
    wavio.write_wav_pcm16(pa, (3000 * rng.standard_normal(8000)).astype(np.int16), 16000)
    wavio.write_wav_pcm16(pb, (3000 * rng.standard_normal(8000 + 257)).astype(np.int16), 16000)
    wavio.write_wav_pcm16(pc, (3000 * rng.standard_normal(8000)).astype(np.int16), 22050)
    with pytest.raises(ValueError, match="one model hop"):  # before the GPU is touched
        mcd.main(["--ref", pa, "--test", pb])
    with pytest.raises(ValueError, match="rate"):
        mcd.main(["--ref", pa, "--test", pc])
    assert resynth.build_parser().parse_args(["--input", "a", "--output", "b", "--mcd"]).mcd
    assert not resynth.build_parser().parse_args(["--input", "a", "--output", "b"]).mcd
    assert vocoder_eval.build_parser().parse_args(["--wav", "a", "--generator", "g", "--discriminator", "d", "--mcd"]).mcd
    assert vocoder_eval.MCD_KEYS == ("mcd",)
    import inspect

    assert inspect.signature(vocoder_eval.score_segments).parameters["mcd"].default is None
