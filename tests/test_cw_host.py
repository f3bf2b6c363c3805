"""Continuous-wave source, host side (no GPU): the C-ABI surface, the Python module, the integrity of the fixture
tests/golden/g10_cw.npz (tools/gen_cw_golden.py) and the host constants / validation of csrc/cw_host.h in a
stand-alone C++ program built with the address and undefined-behaviour sanitizers."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import cw_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fakepta_amd.h")
LIB = os.path.join(ROOT, "fakepta_amd", "lib", "libfakepta_amd.so")
CSRC = os.path.join(ROOT, "fakepta_amd", "csrc")


@pytest.fixture(scope="module")
def g(golden):
    return golden("g10_cw.npz")


def test_abi_declares_and_exports_cw_accumulate():
    text = open(HEADER).read()
    assert re.search(r"^int\s+fpta_cw_accumulate\s*\(", text, flags=re.M)
    assert re.search(r"^#define\s+FPTA_CW_NPAR\s+9\b", text, flags=re.M)
    assert re.search(r"^#define\s+FPTA_OPT_CW_SPLIT\s+26\b", text, flags=re.M)
    assert hasattr(ctypes.CDLL(LIB), "fpta_cw_accumulate")
    from fakepta_amd import _capi
    assert "fpta_cw_accumulate" in _capi.EXPORTED
    assert _capi.OPT_CW_SPLIT == 26 and _capi.OPT_CW_SPLIT in _capi.OPTIONS and _capi.K_CW == 6


def test_module_imports_and_refuses_evolve_false(monkeypatch):
    from fakepta_amd import _capi, cw

    def no_context(*a, **k):
        raise AssertionError("a device context was requested")
    monkeypatch.setattr(_capi, "get_context", no_context)
    with pytest.raises(NotImplementedError):
        cw.cw_delay(np.arange(3.0), np.array([1.0, 0, 0]), (1.0, 0.2), log10_h=-14, evolve=False)
    # the dict form of the sources uses Pulsar.add_cgw's argument names
    tab = cw.source_table(dict(costheta=[0.1, 0.2], phi=[1, 2], cosinc=0.5, log10_mc=9, log10_fgw=-8, log10_h=-14,
                               phase0=0, psi=0, psrterm=[True, False]))
    np.testing.assert_array_equal(tab, [[0.1, 1, 0.5, 9, -8, -14, 0, 0, 1], [0.2, 2, 0.5, 9, -8, -14, 0, 0, 0]])
    assert cw.COLUMNS == R.COLUMNS


def test_fixture_integrity(g):
    offs, src = g["offs"], g["src"]
    assert list(np.diff(offs)) == [1, 63, 257, 70] and src.shape == (10, 9)
    assert g["truth"].shape == (10, offs[-1]) and np.all(g["err_ref64"] > 0)
    np.testing.assert_array_equal(g["peak"], np.max(np.abs(g["truth"]), axis=1))
    assert sorted(map(tuple, src[:5, 3:5])) == sorted(map(tuple, src[5:, 3:5]))
    assert not src[:5, 8].any() and src[5:, 8].all()
    for s in range(len(src)):
        kw = dict(zip(R.COLUMNS, src[s]))
        ref = np.concatenate([R.cw_delay_numpy(g["toas"][offs[p]:offs[p + 1]], g["pos"][p], g["pdist"][p], **kw)
                              for p in range(4)])
        err = np.max(np.abs(ref - g["truth"][s]))
        print(f"source {s}: literal fp64 error {err:.3e}, stored {g['err_ref64'][s]:.3e}")
        assert err <= 2.0 * g["err_ref64"][s]  # 1.0 x with the generator's libm; another host's may differ by an ulp


def test_fixture_truth_reevaluates_bitwise(g):
    pytest.importorskip("mpmath")
    offs, src = g["offs"], g["src"]
    for s in range(len(src)):
        kw = dict(zip(R.COLUMNS, src[s]))
        for p, k in ((0, 0), (1, 62), (2, 128)):  # three TOAs per source, one of them at the large epochs
            i = offs[p] + k
            got = R.cw_delay_mp(g["toas"][i:i + 1], g["pos"][p], g["pdist"][p], **kw)
            assert got[0] == g["truth"][s, i], (s, p, k)


_MAIN = r"""
#include <cstdio>
#include <vector>
#include "cw_host.h"
// stdin: n_src, tmax, then n_src rows of 9 parameters. stdout: per accepted source "ok s K C a0", and for the first
// refused one "bad s reason" (validation stops there, as fpta_cw_accumulate does).
int main() {
  long n = 0;
  double tmax = 0;
  if (std::scanf("%ld %lf", &n, &tmax) != 2 || n < 0) return 2;
  std::vector<double> src((size_t)n * fpta_cw::kNPar);
  for (double& v : src)
    if (std::scanf("%lf", &v) != 1) return 2;
  std::vector<fpta_cw::SrcEval> ev((size_t)n);
  std::vector<fpta_cw::SrcGeom> gm((size_t)n);
  std::string why;
  const long bad = (long)fpta_cw::validate_sources(n, src.data(), tmax, ev.data(), gm.data(), why);
  for (long s = 0; s < (bad < 0 ? n : bad); ++s) {
    fpta_cw::SrcConst k;
    std::string w2;
    if (!fpta_cw::source_constants(&src[(size_t)s * fpta_cw::kNPar], k, w2)) return 3;
    std::printf("ok %ld %.17g %.17g %.17g\n", s, ev[(size_t)s].K, ev[(size_t)s].C, k.a0);
  }
  if (bad >= 0) std::printf("bad %ld %s\n", bad, why.c_str());
  std::printf("split %d %d %d %d\n", (int)fpta_cw::split_count(10000, 2500, 0), (int)fpta_cw::split_count(4096, 200000, 0),
              (int)fpta_cw::split_count(10, 391, 3), (int)fpta_cw::split_count(10, 391, 50));
  return 0;
}
"""


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("cw_host")
    (d / "main.cpp").write_text(_MAIN)
    exe = str(d / "cw_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, str(d / "main.cpp"), "-o", exe], check=True)

    def run(src, tmax):
        text = f"{len(src)} {tmax!r}\n" + "\n".join(" ".join(repr(float(v)) for v in row) for row in src) + "\n"
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return r.stdout.splitlines()
    return run


def test_host_constants_match_numpy(g, host_program):
    from fakepta import constants as const
    src = g["src"]
    lines = host_program(src, float(g["toas"].max()))
    assert len(lines) == len(src) + 1 and lines[-1].startswith("split ")
    for s, line in enumerate(lines[:-1]):
        tag, idx, K, C, a0 = line.split()
        assert tag == "ok" and int(idx) == s
        mc = 10 ** src[s, 3] * const.Tsun
        w0 = np.pi * 10 ** src[s, 4]
        dist = 2 * mc ** (5 / 3) * w0 ** (2 / 3) / 10 ** src[s, 5]
        want = (256 / 5 * mc ** (5 / 3) * w0 ** (8 / 3), w0 ** (-5 / 3) / (32 * mc ** (5 / 3)),
                mc ** (5 / 3) / (dist * w0 ** (1 / 3)))
        np.testing.assert_allclose([float(K), float(C), float(a0)], want, rtol=1e-14, atol=0)
    # the split rule: few TOAs and many sources split, a full device does not, a forced count is clamped to n_src
    n_b, n_a, forced3, forced50 = map(int, lines[-1].split()[1:])
    assert n_b > 1 and n_a == 1 and forced3 == 3 and forced50 == 10


@pytest.mark.parametrize("col,value,reason", [(4, float("nan"), "non-finite log10_fgw"),
                                              (6, float("inf"), "non-finite phase0"),
                                              (0, 1.0000001, "|cos_gwtheta| > 1"),
                                              (2, -1.5, "|cos_inc| > 1"),
                                              (4, -6.0, "coalesces")])
def test_host_validation_names_the_source(g, host_program, col, value, reason):
    src = g["src"].copy()
    src[7, col] = value  # source 7 has log10_mc 8: at log10_fgw -6, K max(t) is ~16
    lines = host_program(src, float(g["toas"].max()))
    assert [ln.split()[0] for ln in lines[:-1]] == ["ok"] * 7 + ["bad"]
    tag, idx, why = lines[-2].split(None, 2)
    assert int(idx) == 7 and reason in why
