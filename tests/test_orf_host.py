"""Anisotropic ORF, host side (no GPU): fpta_healpix_pix2ang_ring against the 50-digit pixel centres of
tests/golden/g12_orf.npz (tools/gen_orf_golden.py) and the published nside 1 / 2 ring tables, the C-ABI surface, the
healpy-free import of the drop-in module, the numpy model of tests/orf_reference.py against hd() and the fixture, and
csrc/orf_host.h (validation, pixel <-> ring maps, tile / K-split plan) in a stand-alone C++ program built with the
address and undefined-behaviour sanitizers."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import orf_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fakepta_amd.h")
LIB = os.path.join(ROOT, "fakepta_amd", "lib", "libfakepta_amd.so")
CSRC = os.path.join(ROOT, "fakepta_amd", "csrc")
ENTRY_POINTS = ("fpta_healpix_pix2ang_ring", "fpta_orf_anisotropic", "fpta_orf_plan")
EPS = np.finfo(np.float64).eps
NSIDES = (1, 2, 3, 4, 8)


@pytest.fixture(scope="module")
def g(golden):
    return golden("g12_orf.npz")


@pytest.fixture(scope="module")
def capi():
    from fakepta_amd import _capi
    return _capi


# ----------------------------------------------------------------------------- pixel centres
@pytest.mark.parametrize("nside", NSIDES)
def test_pix2ang_matches_the_mpmath_centres(capi, g, nside):
    theta, phi = capi.pix2ang_ring(nside)
    assert theta.shape == phi.shape == (12 * nside * nside,)
    e_t, e_p = np.max(np.abs(theta - g[f"theta_{nside}"])), np.max(np.abs(phi - g[f"phi_{nside}"]))
    print(f"nside {nside}: theta off by {e_t / EPS:.2f} eps, phi by {e_p / EPS:.2f} eps")
    assert e_t <= 4 * EPS and e_p <= 4 * EPS
    # a subset in any order gives the same values
    pick = np.array([12 * nside * nside - 1, 0, nside, 5 * nside * nside])
    t2, p2 = capi.pix2ang_ring(nside, pick)
    np.testing.assert_array_equal(t2, theta[pick])
    np.testing.assert_array_equal(p2, phi[pick])


def test_pix2ang_ring_tables_of_nside_1_and_2(capi):
    """The published RING tables written out: z and phi / pi of every pixel of nside 1 and 2."""
    q = np.array([1, 3, 5, 7]) / 4.0
    z1 = np.repeat([2 / 3, 0.0, -2 / 3], 4)
    f1 = np.concatenate([q, np.arange(4) / 2.0, q])
    e = np.arange(8)
    z2 = np.concatenate([np.full(4, 11 / 12), np.full(8, 2 / 3), np.full(8, 1 / 3), np.full(8, 0.0),
                         np.full(8, -1 / 3), np.full(8, -2 / 3), np.full(4, -11 / 12)])
    f2 = np.concatenate([q, (2 * e + 1) / 8.0, e / 4.0, (2 * e + 1) / 8.0, e / 4.0, (2 * e + 1) / 8.0, q])
    for nside, z, f in ((1, z1, f1), (2, z2, f2)):
        theta, phi = capi.pix2ang_ring(nside)
        np.testing.assert_allclose(np.cos(theta), z, rtol=0, atol=2 * EPS)
        np.testing.assert_allclose(phi, f * np.pi, rtol=0, atol=4 * EPS)


@pytest.mark.parametrize("nside", NSIDES + (16, 37))
def test_pix2ang_ring_structure(capi, nside):
    """z never increases with the pixel index, the rings hold 4, 8, .., 4 nside, .., 8, 4 pixels, and the map is
    mirror-symmetric about the equator: pixel j of ring i and pixel j of ring 4 nside - i share phi, theta <-> pi - theta."""
    theta, phi = capi.pix2ang_ring(nside)
    npix = 12 * nside * nside
    assert np.all(np.diff(theta) >= 0) and np.all((phi >= 0) & (phi < 2 * np.pi))
    starts = np.concatenate([[0], np.flatnonzero(np.diff(theta) > 0) + 1, [npix]])
    sizes = np.diff(starts)
    want = [4 * min(i, nside, 4 * nside - i) for i in range(1, 4 * nside)]
    assert list(sizes) == want and len(sizes) == 4 * nside - 1
    for r in range(len(sizes)):
        a, b = starts[r], starts[len(sizes) - 1 - r]
        np.testing.assert_array_equal(phi[a:a + sizes[r]], phi[b:b + sizes[r]])
        np.testing.assert_allclose(theta[a:a + sizes[r]], np.pi - theta[b:b + sizes[r]], rtol=0, atol=2 * EPS)
        assert np.all(np.diff(phi[a:a + sizes[r]]) > 0)  # phi rises within a ring


def test_pix2ang_rejects_what_is_out_of_range(capi):
    for nside, ipix, match in ((3, [108], "element 0: pixel 108"), (3, [0, 5, -1], "element 2: pixel -1"),
                               (0, [0], "nside 0"), (1025, [0], "nside 1025")):
        with pytest.raises(capi.FptaError, match=match):
            capi.pix2ang_ring(nside, ipix)
    with pytest.raises(capi.FptaError, match="nside 0"):
        capi.pix2ang_ring(0)
    theta, phi = capi.pix2ang_ring(3, [107])  # the last pixel of a non-power-of-two nside
    assert abs(theta[0] - np.arccos(-1 + 4 / 108)) <= 4 * EPS and abs(phi[0] - 7 * np.pi / 4) <= 4 * EPS
    assert capi.pix2ang_ring(5, np.zeros(0, dtype=np.int64))[0].shape == (0,)


# ----------------------------------------------------------------------------- C ABI and the Python surface
def test_abi_declares_exports_and_binds_the_entry_points(capi):
    text = open(HEADER).read()
    lib = ctypes.CDLL(LIB)
    for name in ENTRY_POINTS:
        assert re.search(rf"^int\s+{name}\s*\(", text, flags=re.M), name
        assert hasattr(lib, name) and name in capi.EXPORTED
    assert re.search(r"^#define\s+FPTA_OPT_ORF_SPLIT\s+27\b", text, flags=re.M)
    assert capi.OPT_ORF_SPLIT == 27 and capi.OPT_ORF_SPLIT in capi.OPTIONS
    n = int(re.search(r"^#define\s+FPTA_ORF_PLAN_LEN\s+(\d+)\b", text, flags=re.M).group(1))
    assert n == capi.ORF_PLAN_LEN == len(capi.ORF_PLAN_KEYS)
    assert re.search(r"^#define\s+FPTA_VERSION\s+10300\b", text, flags=re.M)
    assert hasattr(capi.Context, "orf_anisotropic")
    host = open(os.path.join(CSRC, "orf_host.h")).read()
    assert "#include <hip" not in host and "__global__" not in host and "__device__" not in host  # plain C++
    assert "orf.hip" in open(os.path.join(CSRC, "Makefile")).read()


def test_correlated_noises_imports_without_healpy():
    code = ("import sys; from fakepta import correlated_noises as cn; import fakepta_amd.orf as orf; "
            "assert 'healpy' not in sys.modules, 'healpy was imported'; "
            "assert callable(cn.anisotropic) and callable(cn.anisotropic_array); "
            "assert orf.npix2nside(768) == 8; print(orf.pix2ang_ring(2)[0].size)")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "48", r.stderr
    src = open(os.path.join(ROOT, "fakepta", "correlated_noises.py")).read()
    assert "import_module" not in src and "import healpy" not in src


def test_npix2nside_and_map_shapes():
    from fakepta_amd import orf
    assert [orf.npix2nside(12 * n * n) for n in (1, 2, 3, 64, 1024)] == [1, 2, 3, 64, 1024]
    for bad in (0, -12, 11, 13, 47, 12 * 9 + 1, 24):
        with pytest.raises(ValueError):
            orf.npix2nside(bad)
    with pytest.raises(ValueError):  # refused before any context is asked for
        orf.anisotropic_orf(np.array([[1.0, 0, 0]]), np.ones(47))
    with pytest.raises(ValueError):
        orf.anisotropic_orf(np.array([[1.0, 0, 0]]), np.ones((2, 2, 12)))


def test_plan_report(capi):
    """fpta_orf_plan: the K-splits are a function of (n_psr, nside) alone, a forced count is clamped to the chunks,
    and the shape is checked."""
    p = capi.orf_plan(130, 8)
    assert (p["tile"], p["chunk"], p["map_group"], p["n_tiles"], p["n_chunks"]) == (64, 16, 4, 6, 48)
    assert p["n_split"] * p["chunks_per_split"] >= 48 > (p["n_split"] - 1) * p["chunks_per_split"]
    for n_map in (1, 3, 9, 81):
        q = capi.orf_plan(130, 8, n_map)
        assert q["n_split"] == p["n_split"] and q["n_groups"] == (n_map + 3) // 4
        assert q["workspace_bytes"] == 8 * 4096 * 4 * q["groups_per_launch"] * q["n_split"] * q["n_tiles"]
    assert [capi.orf_plan(17, 8, split=s)["n_split"] for s in (1, 2, 3, 7, 48, 49, 10 ** 6)] == [1, 2, 3, 7, 48, 48, 48]
    assert capi.orf_plan(17, 1, split=5)["n_split"] == 1  # 12 pixels: one chunk
    big = capi.orf_plan(1000, 64)
    assert big["n_tiles"] == 136 and big["n_chunks"] == 3072 and big["workspace_bytes"] <= 256 << 20
    for args, match in (((5, 0), "nside 0"), ((5, 2000), "nside 2000"), ((9000, 2), "n_psr 9000")):
        with pytest.raises(capi.FptaError, match=match):
            capi.orf_plan(*args)
    with pytest.raises(capi.FptaError, match="npix 47 is not 12 nside"):
        capi.orf_plan(5, 2, npix=47)


# ----------------------------------------------------------------------------- the numpy model
def test_numpy_model_approaches_hellings_downs():
    """h = 1 is an isotropic background: the pixel sum is a quadrature of the Hellings-Downs integral. The deviation
    falls with nside and is below 1e-3 at nside 16 (a quadrature error, not a rounding error)."""
    pos = R.random_positions(np.random.default_rng(2), 20)
    hd = R.hd_matrix(pos)
    dev = [np.max(np.abs(R.orf_numpy(pos, np.ones(12 * n * n)) - hd)) for n in (8, 16, 32)]
    print("deviation from hd() at nside 8, 16, 32:", " ".join(f"{d:.2e}" for d in dev))
    assert dev[0] > dev[1] > dev[2] and dev[1] < 1e-3


def test_numpy_model_matches_the_fixture(g):
    assert list(g["nsides"]) == list(NSIDES) and list(g["case_names"]) == ["p5n2", "p5n4", "p17n8"]
    for name, n_psr, nside, n_map in (("p5n2", 5, 2, 3), ("p5n4", 5, 4, 1), ("p17n8", 17, 8, 1)):
        pos, maps, truth = g[f"{name}_pos"], g[f"{name}_maps"], g[f"{name}_truth"]
        assert pos.shape == (n_psr, 3) and maps.shape == (n_map, 12 * nside * nside)
        assert truth.shape == (n_map, n_psr, n_psr)
        assert maps.min() >= 0.2 and maps.max() <= 2.0
        np.testing.assert_allclose(np.linalg.norm(pos, axis=1), 1.0, rtol=0, atol=4 * EPS)
        assert R.min_d(pos, nside) >= R.D_MIN
        np.testing.assert_array_equal(truth, truth.transpose(0, 2, 1))
        peak = np.max(np.abs(truth))
        e64 = np.max(np.abs(R.orf_numpy(pos, maps) - truth))
        eld = np.max(np.abs(R.orf_longdouble(pos, maps) - truth))
        print(f"{name}: fp64 model off by {e64 / peak:.2e} of peak (stored {np.max(g[name + '_err64']) / peak:.2e}), "
              f"longdouble by {eld / peak:.2e}")
        # D >= 1e-3 amplifies an eps of the pixel direction by at most 1 / D in the nearest pixel's term, one of npix
        assert e64 <= 64 * EPS * peak and eld <= 2 * EPS * peak
        # the model's centres are the fixture's
        z, st, phi = R.centres(nside)
        np.testing.assert_allclose(np.arctan2(st, z), g[f"theta_{nside}"], rtol=0, atol=4 * EPS)
        np.testing.assert_allclose(phi, g[f"phi_{nside}"], rtol=0, atol=4 * EPS)


def test_fixture_truth_reevaluates(g):
    pytest.importorskip("mpmath")
    np.testing.assert_array_equal(R.orf_mp(g["p5n2_pos"][:2], g["p5n2_maps"][1:2])[0], g["p5n2_truth"][1, :2, :2])
    theta, phi = R.pix2ang_mp(3)
    np.testing.assert_array_equal(theta, g["theta_3"])
    np.testing.assert_array_equal(phi, g["phi_3"])


# ----------------------------------------------------------------------------- orf_host.h under the sanitizers
_MAIN = r"""
#include <cstdio>
#include <cstring>
#include <limits>
#include <set>
#include "orf_host.h"
using namespace fpta_orf;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)
static bool refused(int64_t n_psr, const double* pos, int64_t nside, int64_t npix, int64_t n_map, const double* h,
                    const char* expect) {
  std::string why;
  const bool ok = validate(n_psr, pos, nside, npix, n_map, h, why);
  std::printf("validate: %s\n", ok ? "ok" : why.c_str());
  return !ok && why.find(expect) != std::string::npos;
}
int main() {
  // every pixel of nside 1 .. 8 against the inverse map and the ring table
  for (int64_t nside = 1; nside <= 8; ++nside) {
    const std::vector<Ring> t = ring_table((int32_t)nside);
    CHECK((int64_t)t.size() == 4 * nside - 1);
    int64_t next = 0;
    for (int64_t i = 1; i <= 4 * nside - 1; ++i) {
      const Ring& r = t[(size_t)(i - 1)];
      CHECK(r.first == next && r.count == 4 * (i < nside ? i : i <= 3 * nside ? nside : 4 * nside - i));
      CHECK(i == 1 || r.z < t[(size_t)(i - 2)].z);
      CHECK(r.z == -t[(size_t)(4 * nside - 1 - i)].z && r.st == t[(size_t)(4 * nside - 1 - i)].st);
      CHECK(std::fabs(r.z * r.z + r.st * r.st - 1.0) < 4e-16);
      next += r.count;
    }
    CHECK(next == npix_of(nside));
    for (int64_t p = 0; p < npix_of(nside); ++p) {
      const RingPos rp = pix_ring(nside, p);
      CHECK(rp.ring >= 1 && rp.ring <= 4 * nside - 1 && rp.j >= 1 && rp.j <= t[(size_t)(rp.ring - 1)].count);
      CHECK(ring_pix(nside, rp.ring, rp.j) == p);
      double th, ph;
      pix2ang(nside, p, th, ph);
      CHECK(th > 0.0 && th < 3.14159265358979 && ph >= 0.0 && ph < 6.28318530717958);
      CHECK(std::fabs(std::cos(th) - t[(size_t)(rp.ring - 1)].z) < 4e-16);
    }
    CHECK(npix2nside(npix_of(nside)) == nside && npix2nside(npix_of(nside) + 1) == 0);
  }
  CHECK(isqrt(0) == 0 && isqrt(24) == 4 && isqrt(25) == 5 && isqrt((int64_t)1 << 52) == (int64_t)1 << 26);
  CHECK(npix2nside(0) == 0 && npix2nside(24) == 0 && npix2nside(12 * 1024 * 1024) == 1024);
  // validation
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  std::vector<double> pos = {1, 0, 0, 0, 1, 0, 0.6, 0, 0.8}, h(2 * 48, 1.0);
  std::string why;
  CHECK(validate(3, pos.data(), 2, 48, 2, h.data(), why));
  CHECK(validate(0, nullptr, 2, 48, 0, nullptr, why));
  CHECK(refused(3, pos.data(), 0, 0, 2, h.data(), "nside 0"));
  CHECK(refused(3, pos.data(), 1025, 12582912 + 25164, 2, h.data(), "nside 1025"));
  CHECK(refused(3, pos.data(), 2, 47, 2, h.data(), "npix 47"));
  CHECK(refused(3, pos.data(), 3, 48, 2, h.data(), "npix 48"));
  CHECK(refused(kPsrMax + 1, pos.data(), 2, 48, 2, h.data(), "n_psr"));
  h[48 + 17] = nan;
  CHECK(refused(3, pos.data(), 2, 48, 2, h.data(), "map 1, pixel 17"));
  CHECK(validate(3, pos.data(), 2, 48, 1, h.data(), why));  // the bad value lies in a map that is not passed
  h[48 + 17] = -inf;
  CHECK(refused(3, pos.data(), 2, 48, 2, h.data(), "map 1, pixel 17"));
  h[48 + 17] = 1.0;
  pos[7] = nan;
  CHECK(refused(3, pos.data(), 2, 48, 2, h.data(), "pulsar 2: position not finite"));
  pos[7] = 0.0;
  pos[4] = 1.0 + 3e-8;
  CHECK(refused(3, pos.data(), 2, 48, 2, h.data(), "pulsar 1: position is not a unit vector"));
  pos[4] = 1.0 + 5e-9;
  CHECK(validate(3, pos.data(), 2, 48, 2, h.data(), why));
  pos[4] = 0.0;
  CHECK(refused(3, pos.data(), 2, 48, 2, h.data(), "pulsar 1"));
  // plan invariants
  for (int64_t P = 1; P <= 200; ++P)
    for (int64_t split = 0; split <= 9; ++split)
      for (int64_t nside : {1, 3, 8}) {
        const Plan p = make_plan(P, nside, 5, split);
        const Plan one = make_plan(P, nside, 1, split);
        CHECK(p.n_split == one.n_split && p.per_split == one.per_split && p.n_tiles == one.n_tiles);
        CHECK(p.n_tr == (P + kTile - 1) / kTile && p.n_tiles == p.n_tr * (p.n_tr + 1) / 2);
        CHECK(p.n_chunks * kChunk >= npix_of(nside) && (p.n_chunks - 1) * kChunk < npix_of(nside));
        CHECK(p.n_groups == 2 && p.launch_groups >= 1 && p.launch_groups <= p.n_groups);
        CHECK(p.part_doubles == (int64_t)p.launch_groups * kMapGroup * p.n_split * p.n_tiles * kTile * kTile);
        if (split >= 1) CHECK(p.n_split == (split < p.n_chunks ? split : p.n_chunks) ||
                              (p.n_split < split && (int64_t)p.per_split * (p.n_split) >= p.n_chunks));
        // the tiles cover the lower triangle exactly once
        std::set<std::pair<int32_t, int32_t>> seen;
        for (int32_t t = 0; t < p.n_tiles; ++t) {
          int32_t bi, bj;
          tile_of(t, bi, bj);
          CHECK(bj >= 0 && bj <= bi && bi < p.n_tr && t == bi * (bi + 1) / 2 + bj);
          CHECK(seen.insert({bi, bj}).second);
        }
        CHECK((int32_t)seen.size() == p.n_tr * (p.n_tr + 1) / 2);
        // the splits partition the chunks, none empty
        int32_t next = 0;
        for (int32_t s = 0; s < p.n_split; ++s) {
          int32_t c0, c1;
          split_range(p, s, c0, c1);
          CHECK(c0 == next && c1 > c0);
          next = c1;
        }
        CHECK(next == p.n_chunks);
      }
  const Plan none = make_plan(0, 4, 3, 0), nomap = make_plan(7, 4, 0, 0);
  CHECK(none.n_tiles == 0 && none.part_doubles == 0 && nomap.n_split == 0);
  std::printf("%s\n", fails ? "failed" : "all ok");
  return fails ? 1 : 0;
}
"""


def test_host_planner_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    (tmp_path / "main.cpp").write_text(_MAIN)
    exe = str(tmp_path / "orf_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, str(tmp_path / "main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("all ok"), r.stdout[-2000:] + r.stderr[-2000:]
