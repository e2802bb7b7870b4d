"""The launch-regime table of tests/_launch_regimes.py against the HIP sources it restates (CPU only).

tests/test_gpu_launch_regimes.py derives its lengths from that table so that each launch lands in the large-launch path of its kernel (wide tile,
XCD-aware order, staged stores) or exactly on a threshold's edge.  If a pull request moves a threshold or a tile size in the sources and not in the
table, those tests would go on passing while testing the small-launch path again.  This test reads the numbers out of viettts_amd/csrc/*.hip
(named constants, the defaults of the #ifndef VTTS_* geometry macros, the tile aliases' template arguments) and fails loudly instead."""
import re
from pathlib import Path

import pytest

import _launch_regimes as R

CSRC = Path(__file__).resolve().parents[1] / "viettts_amd" / "csrc"


def _src(name):
    return (CSRC / name).read_text()


def _constexpr(src, name):
    m = re.findall(rf"constexpr\s+(?:int|long)\s+{name}\s*=\s*(\d+)\s*;", src)
    assert len(m) == 1, f"constexpr {name}: found {m}"
    return int(m[0])


def _macros(src):
    """the default value of every #define VTTS_* NAME <integer> (the geometry macros' #ifndef defaults)"""
    return {k: int(v) for k, v in re.findall(r"^#define\s+(VTTS_\w+)\s+(\d+)\b", src, re.M)}


def _split_args(s):
    out, depth, cur = [], 0, ""
    for ch in s:
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    out.append(cur.strip())
    return out


def _eval(expr, macros, ks):
    """a template argument such as `KS == 3 ? VTTS_G128K3_N1 : 256` with the macros' defaults and KS bound"""
    e = re.sub(r"\bVTTS_\w+\b", lambda m: str(macros[m.group(0)]), expr)
    m = re.fullmatch(r"(.+?)\?(.+?):(.+)", e)
    if m:
        e = f"({m.group(2)}) if ({m.group(1)}) else ({m.group(3)})"
    return int(eval(e, {}, {"KS": ks}))  # noqa: S307 — integer expressions of our own sources


def _tile_arg(src, alias, index, ks=None):
    """template argument `index` of the tile alias `alias` (template <int KS> using alias = Tile<...>; std::conditional_t followed on KS)"""
    m = re.search(rf"using\s+{alias}\s*=\s*(.+?);\s*(?://.*)?$", src, re.M)
    assert m, f"no 'using {alias} = ...' in the source"
    rhs = m.group(1).strip()
    macros = _macros(src)
    c = re.fullmatch(r"std::conditional_t<(.+)>", rhs)
    if c:
        cond, a, b = _split_args(c.group(1))
        pick = a if _eval(cond, macros, ks) else b
        return _tile_arg(src, pick.split("<")[0].strip(), index, ks)
    args = _split_args(rhs[rhs.index("<") + 1 : rhs.rindex(">")])
    return _eval(args[index], macros, ks)


def test_thresholds_match_the_sources():
    rbg, rbk = _src("kernels_bf16_rbg.hip"), _src("kernels_bf16_rbk.hip")
    f32, fp, x3, rx = _src("kernels_f32_mfma.hip"), _src("kernels_f32_pair.hip"), _src("kernels_x3.hip"), _src("kernels_x3_rb.hip")
    T = R.THRESHOLDS
    assert _constexpr(rbg, "G_MIN_WGS") == T["G_MIN_WGS"]
    assert _constexpr(rbg, "XCD_MAP_MIN_TILES") == T["XCD_MAP_MIN_TILES"]
    # the fp32 / split kernels share ONE threshold and ONE tile mapping (device_common.h): the table's four names are the four kernels that use it
    common = _src("device_common.h")
    for name in ("F32_XCD_MIN_TILES", "FP_XCD_MIN_TILES", "X3_XCD_MIN_TILES", "RX_XCD_MIN_TILES"):
        assert _constexpr(common, "XCD_MIN_TILES") == T[name], name
    launcher = f32[f32.index("hipError_t launch_conv1d_f32_mfma(") :]
    assert _constexpr(launcher[: launcher.index("\n}\n")], "MIN_WGS") == T["F32_MIN_WGS"]
    # resblock_bf16_k's window threshold is a literal in two places: the kernel's xmap and the launcher's grid padding
    kern = re.findall(r"const bool xmap = \(a\.L \+ NT - 1\) / NT >= (\d+);", rbk)
    grid = re.findall(r"if \(\(int\)grid\.x >= (\d+)\) grid\.x = \(grid\.x \+ 7\) / 8 \* 8;", rbk)
    assert kern and grid and {int(v) for v in kern + grid} == {T["RB_BF16_XCD_MIN"]}, (kern, grid)
    # the kernels that share a threshold with their launcher name the same constant in both places
    assert re.search(r"grid\.x >= XCD_MAP_MIN_TILES\) grid\.x = \(grid\.x \+ 7\) / 8 \* 8", rbg)
    assert re.search(r"gridDim\.x >= XCD_MIN_TILES\)", common) and re.search(r"tiles >= XCD_MIN_TILES \? \(tiles \+ 7\) / 8 \* 8 : tiles", common)
    for src, name in ((f32, "kernels_f32_mfma.hip"), (fp, "kernels_f32_pair.hip"), (x3, "kernels_x3.hip"), (rx, "kernels_x3_rb.hip")):
        assert "_XCD_MIN_TILES" not in src, name  # no private copy of the threshold
        assert len(re.findall(r"if \(!xcd_tile\(L, \w+, tile\)\) return;", src)) == 1 and len(re.findall(r"dim3 grid\(xcd_grid_x\(", src)) == 1, name


def test_decision_rules_match_the_sources():
    """the wide/narrow decisions count workgroups with the tiles the table says they do"""
    rbg, f32 = _src("kernels_bf16_rbg.hip"), _src("kernels_f32_mfma.hip")
    # launch_pair_g_bf16: every channel count decides with the k = 11 wide tile's NT2
    dec = re.findall(r"case (\d+): return narrow\(G(\d+)<(\d+)>::NT2\)", rbg) + [("32", c, k) for c, k in re.findall(r"narrow\(G(\d+)<(\d+)>::NT2\) \? launch_g<GTail", rbg)]
    assert sorted({(int(c), int(g), int(k)) for c, g, k in dec}) == [(C, C, 11) for C in (32, 64, 128, 256)], dec
    assert re.search(r"\(long\)\(\(a\.L \+ nt2 - 1\) / nt2\) \* a\.B < G_MIN_WGS", rbg)
    got = {int(c): (int(nt), int(mt)) for c, nt, mt in re.findall(r"case (\d+): return narrow\((\d+), (\d+)\) \? launch_ks<Tile\d+S>", f32)}
    assert got == R.F32_CONV_DECISION, got
    assert re.search(r"wide_wgs\(a, NT, mtiles\) < MIN_WGS", f32)


@pytest.mark.parametrize("k", [3, 7, 11])
def test_tile_sizes_match_the_sources(k):
    rbg, f32, fp = _src("kernels_bf16_rbg.hip"), _src("kernels_f32_mfma.hip"), _src("kernels_f32_pair.hip")
    x3, rx, rbk = _src("kernels_x3.hip"), _src("kernels_x3_rb.hip"), _src("kernels_bf16_rbk.hip")
    for C in (256, 128, 64, 32):
        assert _tile_arg(rbg, f"G{C}", 2, k) == R.BF16_PAIR_N1_WIDE[C][k], ("GTile N1", C, k)
        assert _tile_arg(rbg, f"G{C}S", 2, k) == R.BF16_PAIR_N1_NARROW[C], ("narrow GTile N1", C, k)
        assert _tile_arg(f32, f"Tile{C}", 4, k) == R.F32_CONV_NT_WIDE[C], ("ConvTile NT", C, k)
        assert _tile_arg(f32, f"Tile{C}S", 4, k) == R.F32_CONV_NT_NARROW[C], ("narrow ConvTile NT", C, k)
        assert _tile_arg(f32, f"Tile{C}", 3, k) == _tile_arg(f32, f"Tile{C}S", 3, k) == R.F32_CONV_MT[C], ("ConvTile MT", C, k)
        assert _tile_arg(x3, f"X{C}", 2, k) == R.X3_PAIR_N1[C][k], ("XTile N1", C, k)
        if C in R.F32_PAIR_N1:
            assert _tile_arg(fp, f"FP{C}", 2, k) == R.F32_PAIR_N1[C], ("F32PairTile N1", C, k)
        if k in R.BF16_RB_W.get(C, {}):
            assert _tile_arg(rbk, f"RB{C}", 2, k) == R.BF16_RB_W[C][k], ("RBTile W", C, k)
        if k in R.X3_RB_W.get(C, {}):
            assert _tile_arg(rx, f"RX{C}", 2, k) == R.X3_RB_W[C][k], ("RXTile W", C, k)


def test_upsampler_tiles_match_the_sources():
    x3 = _src("kernels_x3.hip")
    for i, n1 in R.X3_UPS_N1.items():
        assert _tile_arg(x3, f"UX{i}", 3) == n1, (i, n1)
    # the stride-2 upsamplers store through the staged fp32 area (STAGED) when it fits the planes' LDS: the GPU test relies on that epilogue
    for i in (2, 3):
        cin, cout, sh, n1, wm = (_tile_arg(x3, f"UX{i}", j) for j in (0, 1, 2, 3, 4))
        rows16 = -(-(n1 + 2) // 16) * 16
        assert sh == 1 and wm * 32 * (2 * n1 + 4) * 4 <= 2 * rows16 * cin * 2, i


def test_whole_resblock_margin_matches_the_sources():
    """rb_margin / rb_window_nt restate M = H (d0 + d1 + d2) + 3 H and NT = W - 2 M of both whole-ResBlock kernels and of their launchers
    (tests/_bf16_rb_ref.py computes the window-edge lengths of tests/test_gpu_bf16_resblock.py from them)"""
    for name in ("kernels_bf16_rbk.hip", "kernels_x3_rb.hip"):
        src = _src(name)
        assert len(re.findall(r"const int M = H \* \(d0 \+ d1 \+ d2\) \+ 3 \* H;", src)) == 1, name
        assert len(re.findall(r"const int NT = W - 2 \* M;", src)) == 1, name
        assert len(re.findall(r"const int NT = T::W - 2 \* \(T::H \* dsum \+ 3 \* T::H\);", src)) == 1, name
        assert re.search(r"static constexpr int H = \(KS - 1\) / 2[;,]", src), name
    assert [R.rb_margin(k) for k in (3, 7, 11)] == [12, 36, 60]
    assert R.rb_window_nt(256, 3) == 232 and R.rb_window_nt(512, 7) == 440 and R.rb_window_nt(512, 11) == 392 and R.rb_window_nt(128, 3) == 104
    assert R.rb_margin(7, (1, 2, 4)) == 3 * 7 + 9 and R.rb_window_nt(512, 7, (1, 2, 4)) == 512 - 60
