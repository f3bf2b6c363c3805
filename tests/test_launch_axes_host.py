"""tests/launch_axes.py against the sources and against its own purpose (no GPU): (a) every tile size the restatement
uses is the one csrc launches with, read from the sources; (b) the new GPU cases take every launch axis of k_lnl_quad,
k_clnl_mix, k_clnl_solve, k_spectra_amp and k_spectra_scale to at least two workgroups, each axis with a last workgroup
that is partly filled, and every case reaches what it is listed for."""
import os
import re

from tests import launch_axes as A

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fakepta_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _ints(pattern, text, count=1):
    """The integer groups of the pattern's matches in text; exactly `count` matches."""
    found = re.findall(pattern, text)
    assert len(found) == count, (pattern, found)
    return [tuple(int(x) for x in (m if isinstance(m, tuple) else (m,))) for m in found]


# ----------------------------------------------------------------------------- (a) the constants are the sources'
def test_lnl_tiles_are_the_sources():
    lnl, host = _src("lnl.hip"), _src("lnl_host.h")
    assert _ints(r"constexpr int kLnlGrid = (\d+);", lnl) == [(A.LNL_GRID,)]
    assert _ints(r"constexpr int kLnlRpad = (\d+);", lnl) == [(A.LNL_RPAD,)]
    assert _ints(r"constexpr int kLnlWaves = (\d+);", lnl) == [(4,)]
    assert _ints(r"groups_of\(int32_t K\) \{ return \(K \+ (\d+)\) / (\d+); \}", host) == \
        [(A.LNL_GROUP - 1, A.LNL_GROUP)]
    assert _ints(r"const int nh = KG <= (\d+) \? (\d+) : (\d+);", lnl) == [(A.LNL_KG_WIDE,) + A.LNL_NH]
    # the kernel's offsets and the launch's extents are written in these names
    assert len(re.findall(r"r0 = \(int\)blockIdx\.x \* 16 \* NH, g0 = \(int\)blockIdx\.y \* kLnlGrid", lnl)) == 1
    assert len(re.findall(r"R_pad = st\.rpad = \(R \+ kLnlRpad - 1\) / kLnlRpad \* kLnlRpad;", lnl)) == 1
    assert len(re.findall(r"n_rt = \(R_pad \+ 16 \* nh - 1\) / \(16 \* nh\), n_gc = \(G \+ kLnlGrid - 1\) / kLnlGrid;",
                          lnl)) == 1
    assert len(re.findall(r"lds = sizeof\(double\) \* 16 \* \(size_t\)KG \* 16 \* \(size_t\)nh;", lnl)) == 1
    for nh in A.LNL_NH:
        assert f"k_lnl_quad<{nh}><<<grid, block, lds, c->stream>>>" in lnl


def test_clnl_tiles_are_the_sources():
    clnl, host = _src("clnl.hip"), _src("clnl_host.h")
    assert _ints(r"pad64\(int64_t n\) \{ return \(n \+ (\d+)\) / (\d+) \* (\d+); \}", host) == \
        [(A.CLNL_TILE - 1, A.CLNL_TILE, A.CLNL_TILE)]
    assert _ints(r"R_pad = st\.rpad = \(R \+ (\d+)\) / (\d+) \* (\d+);", clnl) == \
        [(A.CLNL_RPAD - 1, A.CLNL_RPAD, A.CLNL_RPAD)]
    assert len(re.findall(r"vld = fpta_clnl::pad64\(R_pad\)", clnl)) == 1
    # both launches: dim3((unsigned)(vld / 64), ...
    assert _ints(r"k_clnl_(?:mix|solve)<<<dim3\(\(unsigned\)\(vld / (\d+)\),", clnl, 2) == [(A.CLNL_TILE,)] * 2
    # and the kernels' own offsets
    assert _ints(r"r = \(int\)blockIdx\.x \* (\d+) \+ 16 \* wave \+ lr", clnl) == [(A.CLNL_TILE,)]
    assert _ints(r"V = a\.V \+ o \* n_pad \* vld \+ tile \* (\d+);", clnl) == [(A.CLNL_TILE,)]
    assert _ints(r"Y = a\.Y \+ \(m \* \(int64_t\)gridDim\.x \+ tile\) \* n_pad \* (\d+);", clnl) == [(A.CLNL_TILE,)]
    assert _ints(r"r = tile \* (\d+) \+ lane;", clnl) == [(A.CLNL_TILE,)]


def test_spectra_tiles_are_the_sources():
    spectra, internal = _src("spectra.hip"), _src("fpta_internal.h")
    assert _ints(r"constexpr int kRealPad = (\d+);", internal) == [(A.REAL_PAD,)]
    assert len(re.findall(r"R_pad = \(n_real \+ kRealPad - 1\) / kRealPad \* kRealPad;", spectra)) == 1
    assert _ints(r"k_spectra_amp<<<dim3\(\(unsigned\)\(\(R_pad \+ (\d+)\) / (\d+)\),", spectra) == \
        [(A.SPECTRA_AMP - 1, A.SPECTRA_AMP)]
    assert _ints(r"k_spectra_scale<<<dim3\(\(unsigned\)\(\(R_pad / 2 \+ (\d+)\) / (\d+)\),", spectra) == \
        [(A.SPECTRA_SCALE // 2 - 1, A.SPECTRA_SCALE // 2)]
    assert _ints(r"const int32_t r = blockIdx\.x \* (\d+) \+ threadIdx\.x;", spectra) == [(A.SPECTRA_AMP,)]
    assert _ints(r"const int32_t r = \(blockIdx\.x \* (\d+) \+ threadIdx\.x\) \* 2;", spectra) == \
        [(A.SPECTRA_SCALE // 2,)]
    assert A.REAL_PAD % 2 == 0  # k_spectra_scale's pairs


def test_the_restatement_on_the_shapes_the_suite_had():
    """The table of the shapes tested so far: one workgroup on every axis."""
    for K, G, R in ((62, 17, 33), (60, 3, 48), (18, 17, 17)):
        a = A.lnl_launch(K, G, R)
        assert (a["nh"], a["R_pad"], a["n_rt"], a["n_gc"]) == (4, 64 if R > 32 else 32, 1, 1)
    assert A.lnl_launch(256, 3, 33)["nh"] == 2 and A.lnl_launch(256, 3, 33)["n_rt"] == 2
    assert [A.clnl_launch(R)["tiles"] for R in (1, 16, 33, 48)] == [1, 1, 1, 1]
    s = A.spectra_launch(256)
    assert (s["R_pad"], s["amp"], s["scale"]) == (256, 1, 1)
    s = A.spectra_launch(1024)
    assert (s["R_pad"], s["amp"], s["scale"]) == (1024, 4, 2)


# ----------------------------------------------------------------------------- (b) the cases reach what they are for
def _lnl(case):
    P, N, G, R, empty = case
    return A.lnl_launch(2 * N, G, R)


def test_every_lnl_case_reaches_what_it_is_listed_for():
    a = _lnl(A.LNL_STAGE2[0])  # K = 4 on <4>: tiles 64 + 64 + 32 of R_pad = 160; chunks 32 + 32 + 6
    assert (a["K"], a["nh"], a["R_pad"], a["padded"], a["chunks"]) == (4, 4, 160, [64, 64, 32], [32, 32, 6])
    assert a["real"] == [64, 64, 2]
    a = _lnl(A.LNL_STAGE2[1])  # two row groups; second tile half full; a second chunk of one point (three waves idle)
    assert (a["KG"], a["nh"], a["padded"], a["chunks"]) == (2, 4, [64, 32], [32, 1])
    assert a["chunks"][-1] < 4  # fewer grid points than waves
    a = _lnl(A.LNL_STAGE2[2])  # K = 128, KG = 8: the full 64 KB; exactly two full tiles and one full chunk
    assert (a["K"], a["KG"], a["nh"], a["lds"]) == (128, A.LNL_KG_WIDE, 4, A.LNL_LDS)
    assert (a["padded"], a["real"], a["chunks"]) == ([64, 64], [64, 64], [32])
    a = _lnl(A.LNL_STAGE2[3])  # K = 130, the smallest <2> shape: three 32-wide tiles, two chunks
    assert (a["K"], a["KG"], a["nh"], a["padded"], a["chunks"]) == (130, 9, 2, [32, 32, 32], [32, 1])
    assert A.lnl_launch(128, 1, 1)["nh"] == 4 and a["lds"] <= A.LNL_LDS  # K is even: 130 is the first past 128
    b = A.LNL_BITWISE
    a = A.lnl_launch(2 * b["N"], b["G"], b["R"])
    assert (a["nh"], a["real"], a["chunks"]) == (4, [64, 64, 2], [32, 32, 6])
    # the picks: the first and last realization of tile 0, the first of tiles 1 and 2, the last realization; the last
    # row of chunk 0, both ends of chunk 1, the first row of chunk 2, the last row
    assert sorted({r // a["tile"] for r in b["reals"]}) == [0, 1, 2] and b["R"] - 1 in b["reals"]
    assert {0, a["tile"] - 1, a["tile"], 2 * a["tile"]} <= set(b["reals"]) and max(b["reals"]) < b["R"]
    assert sorted({g // A.LNL_GRID for g in b["rows"]}) == [0, 1, 2] and b["G"] - 1 in b["rows"]
    assert {A.LNL_GRID - 1, A.LNL_GRID, 2 * A.LNL_GRID - 1, 2 * A.LNL_GRID} <= set(b["rows"])
    b = A.LNL_BATCH
    a = A.lnl_launch(b["K"], b["nA"] * b["ngamma"], b["R"])
    assert (a["nh"], a["n_rt"], a["n_gc"], a["chunks"]) == (4, 3, 3, [32, 32, 8])


def test_every_lnl_axis_passes_one_workgroup_and_ends_partly_filled():
    runs = [_lnl(c) for c in A.LNL_STAGE2]
    for nh in A.LNL_NH:
        mine = [a for a in runs if a["nh"] == nh]
        assert any(a["n_gc"] >= 2 for a in mine), nh                      # grid chunks (blockIdx.y), <4> and <2>
        assert any(a["chunks"][-1] < A.LNL_GRID for a in mine if a["n_gc"] >= 2), nh
    wide = [a for a in runs if a["nh"] == 4]
    assert any(a["n_rt"] >= 2 for a in wide)                              # realization tiles (blockIdx.x) of <4>
    assert any(a["n_rt"] >= 2 and a["padded"][-1] < a["tile"] for a in wide)
    assert any(a["n_rt"] >= 2 and a["padded"][-1] == a["tile"] for a in wide)  # and exactly full
    assert any(a["KG"] == A.LNL_KG_WIDE and a["lds"] == A.LNL_LDS for a in wide)  # the columns: the last KG of <4>
    assert any(a["KG"] == A.LNL_KG_WIDE + 1 for a in runs)                    # and the first of <2>


def test_the_clnl_cases_pass_one_tile_and_end_partly_filled():
    a = A.clnl_launch(A.CLNL_R)  # vld = 192: three tiles, the last with 32 padded and 32 dead columns
    assert (a["R_pad"], a["vld"], a["tiles"], a["padded"], a["real"]) == (160, 192, 3, [64, 64, 32], [64, 64, 2])
    assert a["tiles"] >= 2 and 0 < a["padded"][-1] < A.CLNL_TILE
    assert sorted({r // A.CLNL_TILE for r in A.CLNL_REALS}) == [0, 1, 2] and A.CLNL_R - 1 in A.CLNL_REALS
    assert {0, A.CLNL_TILE - 1, A.CLNL_TILE, 2 * A.CLNL_TILE} <= set(A.CLNL_REALS)
    (P0, K0, G0), (P1, K1, G1) = A.CLNL_STAGES
    assert P0 * K0 == 12 and P1 * K1 == 70
    assert -(-P0 * K0 // A.CLNL_TILE) == 1 and -(-P1 * K1 // A.CLNL_TILE) == 2  # block rows: Y_j is read back with 2


def test_the_spectra_case_passes_one_block_and_ends_partly_filled():
    c = A.SPECTRA
    s = A.spectra_launch(c["R"])
    # R_pad = 640: three k_spectra_amp blocks, two k_spectra_scale blocks with the second a quarter full
    assert (s["R_pad"], s["amp"], s["scale"]) == (640, 3, 2)
    assert s["amp_fill"] == [256, 256, 128] and s["scale_fill"] == [512, 128]
    assert 4 * s["scale_fill"][-1] == A.SPECTRA_SCALE and 0 < s["amp_fill"][-1] < A.SPECTRA_AMP
    assert c["real0"] % 2 == 1 and c["n_rn"] % 2 == 1 and set(c["paths"]) == {4, 3}
    assert sorted({r // A.SPECTRA_AMP for r in c["picks"]}) == [0, 1, 2]
    assert sorted({r // A.SPECTRA_SCALE for r in c["picks"]}) == [0, 1]
    assert {0, 255, 256, 511, 512, c["R"] - 1} == set(c["picks"])
