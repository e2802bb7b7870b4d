"""include/vtts_spectral.h without a GPU: the numpy restatement (tests/_spectral_oracle.py) against torch.stft, the frame count, the host entry
points of the built library, and the bounds the GPU test uses: every planted fault misses at least one of them."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import _spectral_oracle as O
from viettts_amd import _lib

REPO = Path(__file__).resolve().parents[1]
CFGS = [O.RESOLUTIONS[n] for n in O.N_FFTS]


@pytest.fixture(scope="module")
def lib():
    from viettts_amd.csrc.build import build

    build()
    return _lib.load()


def _meter(cfg):
    from viettts_amd.spectral import SpectralMeter

    return SpectralMeter(*cfg, device="cuda:0")  # create() touches no HIP call


def _torch_mags(x: np.ndarray, cfg) -> np.ndarray:
    """[T, n_fft / 2 + 1] float64: an independent implementation of the framing and the transform."""
    n_fft, win, hop = cfg
    w = torch.from_numpy(O.window(cfg)[(n_fft - win) // 2 : (n_fft - win) // 2 + win].astype(np.float64))
    z = torch.stft(torch.from_numpy(x.astype(np.float64)), n_fft, hop_length=hop, win_length=win, window=w, center=True, pad_mode="reflect", return_complex=True)
    return z.abs().numpy().T


@pytest.mark.parametrize("cfg", CFGS, ids=str)
def test_float64_oracle_is_torch_stft(cfg):
    assert cfg[1] < cfg[0] and cfg[0] % cfg[2]  # win < n_fft, and a hop that does not divide n_fft
    for i in (0, 4, 5):
        x, _ = O.case(i)
        _, m = O.powers(x, cfg)
        want = np.maximum(_torch_mags(x, cfg), np.sqrt(O.P_FLOOR))
        assert m.shape == want.shape == (O.num_frames(len(x), cfg), cfg[0] // 2 + 1)
        d = float(np.abs(m - want).max() / want.max())
        print(f"\n{cfg} case {i}: float64 oracle within {d:.2e} of torch.stft (relative to the largest magnitude)")
        assert d < 1e-11


@pytest.mark.parametrize("cfg", CFGS, ids=str)
def test_frame_count_on_either_side_of_a_hop_multiple(cfg, lib):
    m = _meter(cfg)
    hop = cfg[2]
    k = O.min_samples(cfg) // hop + 2
    for S in (k * hop - 1, k * hop, k * hop + 1):
        want = k + (S >= k * hop)
        x = O.make_speechlike(S, 3)
        assert O.num_frames(S, cfg) == want == m.num_frames(S) == _torch_mags(x, cfg).shape[0] == O.frame_samples(x, cfg).shape[0]
    m.close()


def test_header_exports_and_constants(lib):
    header = O.HEADER.read_text()
    declared = set(re.findall(r"\b(vtts_spectral_[a-z_0-9]+)\s*\(", header))
    assert declared == set(_lib.SPECTRAL_EXPORTS) == {f"vtts_spectral_{n}" for n in ("create", "destroy", "window", "frames_per_block", "num_frames", "packed_bytes",
                                                                                   "pack", "bind_packed", "workspace_bytes", "forward")}
    for name in declared:
        assert hasattr(lib, name), name
    assert not set(_lib.SPECTRAL_SIGS) & set(_lib.SIGS)
    k = O.K
    assert k["VTTS_SPECTRAL_MAX_SAMPLES"] == _lib.SPECTRAL_MAX_SAMPLES and k["VTTS_SPECTRAL_ROWS_PER_LAUNCH"] == _lib.SPECTRAL_ROWS_PER_LAUNCH
    assert (k["VTTS_SPECTRAL_MAX_FRAMES_PER_BLOCK"], k["VTTS_SPECTRAL_MAX_FRAMES_PER_BLOCK_2048"]) == (_lib.SPECTRAL_MAX_FRAMES_PER_BLOCK, _lib.SPECTRAL_MAX_FRAMES_PER_BLOCK_2048)
    assert k["VTTS_SPECTRAL_LDS_BUDGET"] == _lib.SPECTRAL_LDS_BUDGET == 80 * 1024  # two workgroups in a CU's 160 KB
    text = (REPO / "viettts_amd" / "csrc" / "spectral.hip").read_text()
    found = re.findall(r"^constexpr int (ROWS_PER_LAUNCH) = (\d+);", text, flags=re.M)
    assert found == [("ROWS_PER_LAUNCH", str(_lib.SPECTRAL_ROWS_PER_LAUNCH))] and len(re.findall(r"for_each_launch(?:_off)?<ROWS_PER_LAUNCH>\(", text)) >= 1
    assert len(re.findall(r"\+= ROWS_PER_LAUNCH\)", text)) == 0  # launch_rows.h's loop, and no hand-written one
    from viettts_amd.csrc import build

    assert "spectral.hip" in build.SOURCES and any(str(h).endswith("vtts_spectral.h") for h in build.HEADERS)


def test_the_transform_family_is_stated_once():
    """The butterflies, the Stockham pass and the wave helpers have one definition each among the native sources, and the files whose bits rest
    on single roundings take them in after their pragma (a header's inline functions are compiled in the including file's contraction mode)."""
    from viettts_amd.csrc import build

    texts = {p.name: p.read_text() for p in sorted(build.CSRC.iterdir()) if p.suffix in (".hip", ".h")}
    homes = {r"\bvoid dft4\(": "stockham.h", r"\bvoid wave_sync\(\)": "wave_common.h", r"\bdouble wave_sum\(": "wave_common.h",
             r"\bvoid pass\(": "stockham.h", r"\bvoid radix\(": "stockham.h", r"\bvoid fft512_888\(": "stockham.h",
             r"\bfloat2 cmul\(": "stockham.h", r"\bvoid stage_reflected\(": "stft_front.h", r"g = 2 \* \(S - 1\) - g": "stft_front.h",
             r"ldexpf\(": "sample_convert.h", r"std::cos\(2\.0 \* pi \* m / H\)": "stft_host.h", r"n_fft must be 256, 512, 1024 or 2048 \(got": "stft_host.h"}
    for pattern, home in homes.items():
        assert [n for n, t in texts.items() if re.search(pattern, t)] == [home], pattern
    pragma = "#pragma clang fp contract(off)"
    for name, header in (("spectral.hip", "stft_front.h"), ("stft.hip", "stft_front.h"), ("stft.hip", "stockham.h"), ("stoi.hip", "stockham.h")):
        t = texts[name]
        assert t.count(pragma) == 1 and t.index(pragma) < t.index(f'#include "{header}"'), (name, header)
    assert "#pragma clang fp" not in texts["mel.hip"] and '#include "stockham.h"' in texts["mel.hip"]  # its FMAs are part of its bits
    assert "-ffp-contract=off" in build.FILE_FLAGS["pitch.hip"] and '#include "wave_common.h"' in texts["pitch.hip"]
    for header in ("wave_common.h", "stockham.h", "stft_front.h", "stft_host.h"):
        assert header in build.HEADERS, header
    included = {h for t in texts.values() for h in re.findall(r'#include "([a-z_0-9]+\.h)"', t)}
    assert included <= set(build.HEADERS), included - set(build.HEADERS)  # every header feeds the rebuild digest


def test_create_refuses_what_the_header_excludes(lib):
    h = C.c_void_p(0)
    for bad in ((128, 64, 16), (4096, 1024, 256), (1000, 600, 120), (1024, 600, 0), (1024, 600, -1), (1024, 100, 120), (1024, 1025, 120), (512, 600, 120)):
        cfg = _lib.SpectralCfg(*bad)
        assert lib.vtts_spectral_create(C.byref(cfg), 0, C.byref(h)) == -1, bad
        assert b"n_fft" in lib.vtts_last_error()
    assert lib.vtts_spectral_create(None, 0, C.byref(h)) == -1
    for good in ((256, 1, 1), (256, 256, 256), (2048, 2048, 2048), (2048, 2048, 1), (1024, 1024, 256), (512, 240, 50)):
        cfg = _lib.SpectralCfg(*good)
        assert lib.vtts_spectral_create(C.byref(cfg), 0, C.byref(h)) == 0, good
        lib.vtts_spectral_destroy(h)


@pytest.mark.parametrize("cfg", CFGS + [(2048, 2048, 2048), (2048, 1400, 700), (1024, 1024, 600), (512, 512, 512), (256, 256, 1)], ids=str)
def test_host_entry_points(cfg, lib):
    m = _meter(cfg)
    n_fft, win, hop = cfg
    w = m.window()
    assert np.array_equal(w.view(np.uint32), O.window(cfg).view(np.uint32))  # bit for bit
    lead = (n_fft - win) // 2
    assert not w[:lead].any() and not w[lead + win :].any() and w[lead] == 0.0 and (win < 3 or w[lead + 1] > 0.0)
    F = m.frames_per_block
    assert F == O.frames_per_block(cfg) and 1 <= F <= (4 if n_fft == 2048 else 8)
    assert O.lds_bytes(cfg, F) <= O.K["VTTS_SPECTRAL_LDS_BUDGET"] or F == 1
    if cfg in CFGS:
        assert F == (4 if n_fft == 2048 else 8)  # the default resolutions run at the full count
    lo = O.min_samples(cfg)
    assert m.min_samples == lo and m.n_bins == n_fft // 2 + 1
    for S in (lo, lo + 1, 5 * n_fft + 3, _lib.SPECTRAL_MAX_SAMPLES):
        T = m.num_frames(S)
        assert T == 1 + S // hop
        assert m.workspace_bytes(3, S) == 3 * -(-T // F) * 4 * 8
    n = C.c_int64(0)
    for S in (lo - 1, 0, -1, _lib.SPECTRAL_MAX_SAMPLES + 1):
        assert getattr(lib, "vtts_spectral_num_frames")(m._h, S, C.byref(n)) == -6 and b"n_fft / 2 + 1" in lib.vtts_last_error()
    nb = C.c_size_t(0)
    assert lib.vtts_spectral_workspace_bytes(m._h, 0, lo, C.byref(nb)) == -1 and lib.vtts_spectral_workspace_bytes(m._h, 1, lo - 1, C.byref(nb)) == -6
    H = n_fft // 2
    assert m.packed_bytes == 4 * (n_fft + 2 * H + 2 * (H // 2 + 2))
    fake = C.c_void_p(1 << 32)
    rc = lib.vtts_spectral_forward(m._h, fake, fake, 0, 1, lo, None, fake, fake, fake, fake, None, 0, fake, 1 << 20, None)
    assert rc == -2 and b"before pack" in lib.vtts_last_error()  # nothing is dereferenced before the tables are bound
    assert lib.vtts_spectral_bind_packed(m._h, fake, m.packed_bytes) == 0
    args = lambda lens, S, dtype=0, ws=1 << 20, mg=None, ts=0: (m._h, fake, fake, dtype, len(lens), S, (C.c_int32 * len(lens))(*lens), fake, fake, fake, fake, mg, ts, fake, ws, None)  # noqa: E731
    assert lib.vtts_spectral_forward(*args([lo, lo - 1], lo)) == -6 and b"n_fft / 2 + 1" in lib.vtts_last_error()
    assert lib.vtts_spectral_forward(*args([lo + 1], lo)) == -6 and b"S_stride" in lib.vtts_last_error()
    assert lib.vtts_spectral_forward(*args([lo], lo, dtype=2)) == -1
    assert lib.vtts_spectral_forward(*args([lo], lo, ws=8)) == -5 and b"workspace" in lib.vtts_last_error()
    assert lib.vtts_spectral_forward(*args([lo], lo, mg=fake, ts=m.num_frames(lo) - 1)) == -6 and b"T_stride" in lib.vtts_last_error()
    m.close()


def test_what_the_header_says_about_frames_per_workgroup():
    """The hops up to which each transform length keeps its full count, as the header quotes them."""
    full = {n: max(h for h in range(1, n + 1) if O.frames_per_block((n, n, h)) == (4 if n == 2048 else 8)) for n in O.N_FFTS}
    assert full == {256: 256, 512: 512, 1024: 543, 2048: 676}, full
    assert min(O.frames_per_block((2048, 2048, h)) for h in range(1, 2049)) == 2
    text = O.HEADER.read_text()
    assert "up to hop 676" in text and "up to hop 543" in text


@pytest.mark.parametrize("cfg", CFGS, ids=str)
def test_equal_signals_give_exact_zeros(cfg):
    x, _ = O.case(2)
    for f32 in (False, True):
        r = O.measure(x, x.copy(), cfg, f32=f32)
        assert (r.sc, r.logmag, r.lsd) == (0.0, 0.0, 0.0) and np.array_equal(r.mags[0], r.mags[1])


@pytest.mark.parametrize("cfg", CFGS, ids=str)
def test_every_planted_fault_misses_a_bound(cfg):
    b = O.bounds(cfg)
    print(f"\n{cfg}: float32 restatement within sc {b.scale_sc:.2e}  logmag {b.scale_logmag:.2e}  lsd {b.scale_lsd:.2e}  mags {b.scale_mags:.2e} of float64; "
          f"bounds {b.sc:.2e} / {b.logmag:.2e} / {b.lsd:.2e} / {b.mags:.2e}")
    assert 0.0 < b.sc < 1e-6 and 0.0 < b.logmag < 1e-5 and 0.0 < b.lsd < 1e-4 and 0.0 < b.mags < 1e-5  # fp32 scales: a fault is orders above
    cases = (0, 4, 5)  # 4 holds a quiet stretch: the only place where the clamp's side shows
    for fault in O.FAULTS:
        worst = {}
        for i in cases:
            x, y = O.case(i)
            want, got = O.case_reference(i, cfg)[0], O.measure(x, y, cfg, fault=fault)
            for k, v in O.misses(want, got, b).items():
                worst[k] = max(worst.get(k, 0.0), v)
            if got.mags.shape == want.mags.shape:
                worst["mags"] = max(worst.get("mags", 0.0), float(np.abs(got.mags - want.mags).max() / want.mags.max()) / b.mags)
            if got.n_frames != want.n_frames:
                worst["n_frames"] = float("inf")
        print(f"  {fault:19s} misses by (x bound): " + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()))
        assert max(v for k, v in worst.items() if k != "n_frames") > 1.0, (fault, worst)  # a figure or a magnitude, not the count alone
