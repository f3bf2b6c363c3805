"""Continuous-wave populations in a batch block, host side (no GPU): the C-ABI surface, fakepta_amd.cw's
population_tables, and the planner of csrc/cw_batch_host.h (argument and source validation, the TOA slab table of
k_cw_block) in a stand-alone C++ program built with the address and undefined-behaviour sanitizers."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fakepta_amd.h")
LIB = os.path.join(ROOT, "fakepta_amd", "lib", "libfakepta_amd.so")
CSRC = os.path.join(ROOT, "fakepta_amd", "csrc")


@pytest.fixture(scope="module")
def g(golden):
    return golden("g10_cw.npz")


def test_abi_declares_and_exports_batch_cw_accumulate():
    text = open(HEADER).read()
    assert re.search(r"^int\s+fpta_batch_cw_accumulate\s*\(", text, flags=re.M)
    assert re.search(r"^#define\s+FPTA_VERSION\s+10300\b", text, flags=re.M)
    assert hasattr(ctypes.CDLL(LIB), "fpta_batch_cw_accumulate")
    from fakepta_amd import _capi
    assert "fpta_batch_cw_accumulate" in _capi.EXPORTED
    assert callable(_capi.Context.batch_cw_accumulate)
    from fakepta_amd.batch import BatchSimulator
    assert callable(BatchSimulator.add_cgw)


def test_population_tables(monkeypatch, g):
    from fakepta_amd import _capi, cw

    def no_context(*a, **k):
        raise AssertionError("a device context was requested")
    monkeypatch.setattr(_capi, "get_context", no_context)
    src = g["src"]
    # one table for every realization: [S, 9], one row, a dict
    n_tab, offs, tab = cw.population_tables(src, 7)
    assert n_tab == 1 and offs.dtype == np.int64 and list(offs) == [0, 10]
    np.testing.assert_array_equal(tab, src)
    assert tab.dtype == np.float64 and tab.flags.c_contiguous
    n_tab, offs, tab = cw.population_tables(src[3], 7)
    assert n_tab == 1 and list(offs) == [0, 1]
    np.testing.assert_array_equal(tab, src[3:4])
    n_tab, offs, tab = cw.population_tables(src.tolist(), 7)  # a list of rows is one table
    assert n_tab == 1 and list(offs) == [0, 10]
    d = dict(costheta=[0.1, 0.2], phi=[1, 2], cosinc=0.5, log10_mc=9, log10_fgw=-8, log10_h=-14, phase0=0, psi=0,
             psrterm=[True, False])
    n_tab, offs, tab = cw.population_tables(d, 3)
    assert n_tab == 1 and list(offs) == [0, 2]
    np.testing.assert_array_equal(tab, [[0.1, 1, 0.5, 9, -8, -14, 0, 0, 1], [0.2, 2, 0.5, 9, -8, -14, 0, 0, 0]])
    # [R, S, 9]
    cube = np.stack([src[:4], src[4:8], src[6:10]])
    n_tab, offs, tab = cw.population_tables(cube, 3)
    assert n_tab == 3 and list(offs) == [0, 4, 8, 12]
    np.testing.assert_array_equal(tab, cube.reshape(12, 9))
    # a list of R ragged tables, an empty one among them
    n_tab, offs, tab = cw.population_tables([src[:0], src[:1], np.zeros((0, 9)), src[2:10], []], 5)
    assert n_tab == 5 and list(offs) == [0, 0, 1, 1, 9, 9]
    np.testing.assert_array_equal(tab, np.concatenate([src[:1], src[2:10]]))
    n_tab, offs, tab = cw.population_tables([src[:0], src[:0]], 2)  # nothing at all
    assert n_tab == 2 and list(offs) == [0, 0, 0] and tab.shape == (0, 9)
    # equal-length tables in a list are R tables too, not one
    n_tab, offs, tab = cw.population_tables([src[:2], src[2:4]], 2)
    assert n_tab == 2 and list(offs) == [0, 2, 4]
    # wrong shapes
    for bad, n_real in ((cube, 4), ([src[:1], src[:2]], 3), (src[:, :8], 2), (cube[:, :, :8], 3),
                        (np.zeros((2, 2, 2, 9)), 2), ([src[:1], src[:2, :8]], 2), (src, 0)):
        with pytest.raises(ValueError):
            cw.population_tables(bad, n_real)
    with pytest.raises(TypeError):
        cw.population_tables(dict(costheta=0.1), 2)


_MAIN = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "cw_batch_host.h"
#include "cw_host.h"
// "slabs n_psr n_0 .. n_{P-1}": prints "slab first psr count" per slab.
// "plan n_psr n_0 .. tmax n_real stride n_tab offs_0 .. offs_{n_tab} n_rows rows..": the pulsars sit on the x axis at
// distance 1e11 s; prints "ok n_src n_slab" or "bad reason".
int main() {
  char mode[16];
  int n_psr = 0;
  if (std::scanf("%15s %d", mode, &n_psr) != 2 || n_psr < 0) return 2;
  std::vector<int64_t> offs(1, 0);
  for (int p = 0; p < n_psr; ++p) {
    long n = 0;
    if (std::scanf("%ld", &n) != 1) return 2;
    offs.push_back(offs.back() + n);
  }
  if (!std::strcmp(mode, "slabs")) {
    std::vector<fpta_cwb::Slab> slabs;
    fpta_cwb::make_slabs(n_psr, offs.data(), slabs);
    for (const fpta_cwb::Slab& s : slabs) std::printf("slab %ld %d %d\n", (long)s.first, (int)s.psr, (int)s.count);
    return 0;
  }
  double tmax = 0;
  int n_real = 0, n_tab = 0;
  long stride = 0, n_rows = 0;
  if (std::scanf("%lf %d %ld %d", &tmax, &n_real, &stride, &n_tab) != 4 || n_tab < 0) return 2;
  std::vector<int64_t> so((size_t)n_tab + 1);
  for (int64_t& v : so) {
    long x = 0;
    if (std::scanf("%ld", &x) != 1) return 2;
    v = x;
  }
  if (std::scanf("%ld", &n_rows) != 1 || n_rows < 0) return 2;
  std::vector<double> src((size_t)n_rows * fpta_cw::kNPar);
  for (double& v : src)
    if (std::scanf("%lf", &v) != 1) return 2;
  std::vector<double> pos((size_t)n_psr * 3, 0.0), dist((size_t)(stride ? (long)n_real * n_psr : n_psr), 1e11);
  for (int p = 0; p < n_psr; ++p) pos[3 * (size_t)p] = 1.0;
  fpta_cwb::Plan plan;
  std::string why;
  if (fpta_cwb::make_plan(n_psr, offs.data(), tmax, n_real, pos.data(), dist.data(), stride, n_tab, so.data(),
                          src.data(), 1.0, plan, why))
    std::printf("ok %ld %ld\n", (long)plan.n_src, (long)plan.slabs.size());
  else
    std::printf("bad %s\n", why.c_str());
  return 0;
}
"""


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("cw_batch_host")
    (d / "main.cpp").write_text(_MAIN)
    exe = str(d / "cw_batch_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, str(d / "main.cpp"), "-o", exe], check=True)

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return r.stdout.splitlines()
    return run


@pytest.mark.parametrize("counts", [[1, 63, 257, 70], [256], [257], [1]])
def test_slab_table_covers_every_toa_once(host_program, counts):
    lines = host_program(f"slabs {len(counts)} " + " ".join(map(str, counts)) + "\n")
    offs = np.concatenate([[0], np.cumsum(counts)])
    seen = np.zeros(offs[-1], dtype=int)
    for ln in lines:
        tag, first, psr, count = ln.split()
        first, psr, count = int(first), int(psr), int(count)
        assert tag == "slab" and 1 <= count <= 256
        assert offs[psr] <= first and first + count <= offs[psr + 1]  # inside one pulsar
        seen[first:first + count] += 1
    np.testing.assert_array_equal(seen, 1)
    assert len(lines) == sum(-(-n // 256) for n in counts)


def _plan_input(g, n_real, n_tab, offs, rows, stride=0):
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 9)
    counts = np.diff(g["offs"])
    return (f"plan {len(counts)} " + " ".join(map(str, counts)) + f" {float(g['toas'].max())!r} {n_real} {stride} "
            f"{n_tab} " + " ".join(map(str, offs)) + f" {len(rows)}\n"
            + "\n".join(" ".join(repr(float(v)) for v in row) for row in rows) + "\n")


def test_planner_accepts_ragged_tables(host_program, g):
    src = g["src"]
    rows = np.concatenate([src[:1], src[:3], src])
    assert host_program(_plan_input(g, 4, 4, [0, 0, 1, 4, 14], rows)) == ["ok 14 5"]
    assert host_program(_plan_input(g, 4, 1, [0, 10], src)) == ["ok 10 5"]
    assert host_program(_plan_input(g, 4, 4, [0, 0, 0, 0, 0], src[:0], stride=4)) == ["ok 0 5"]


def test_planner_refusals(host_program, g):
    src = g["src"]
    three = np.concatenate([src[:2], src[2:5], src[5:8]])  # realizations 0, 1, 2 hold 2, 3 and 3 sources
    offs3 = [0, 2, 5, 8]
    line, = host_program(_plan_input(g, 3, 3, [0, 5, 2, 8], three))
    assert line.startswith("bad ") and "not monotone" in line
    line, = host_program(_plan_input(g, 3, 3, [1, 2, 5, 8], three))
    assert line.startswith("bad ") and "src_offs[0]" in line
    line, = host_program(_plan_input(g, 3, 2, [0, 2, 8], three))  # n_tab neither 1 nor R
    assert line.startswith("bad ") and "2 source tables for a block of 3 realizations" in line
    line, = host_program(_plan_input(g, 3, 4, [0, 2, 5, 8, 8], three))
    assert line.startswith("bad ") and "4 source tables for a block of 3 realizations" in line
    line, = host_program(_plan_input(g, 3, 3, offs3, three, stride=2))
    assert line.startswith("bad ") and "pdist_stride" in line
    bad = three.copy()
    bad[6, 4] = np.nan  # realization 2, source 1
    line, = host_program(_plan_input(g, 3, 3, offs3, bad))
    assert line == "bad realization 2, source 1: non-finite log10_fgw"
    bad = three.copy()
    bad[4, 3:5] = 8.0, -6.0  # realization 1, source 2: log10_mc 8 at log10_fgw -6 has K max(t) ~ 16
    line, = host_program(_plan_input(g, 3, 3, offs3, bad))
    assert line.startswith("bad realization 1, source 2: coalesces inside the data span")
    bad = src.copy()
    bad[7, 0] = 1.0000001  # one table for all: realization 0
    line, = host_program(_plan_input(g, 3, 1, [0, 10], bad))
    assert line == "bad realization 0, source 7: |cos_gwtheta| > 1"
