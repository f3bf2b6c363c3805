"""Sky scrambles of the optimal statistic, host side (no GPU): the C-ABI surface, fakepta_amd.os's scramble_positions
and derive_scrambles, and csrc/os_scramble_host.h (the pair-index map of the rows the kernels read, and every refusal
of fpta_batch_set_os_scrambles with its message) in a stand-alone C++ program built with the address and
undefined-behaviour sanitizers."""
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
SYMBOLS = ("fpta_batch_set_os_scrambles", "fpta_batch_os_scrambles_info", "fpta_batch_os_scrambles",
           "fpta_os_scrambles", "fpta_os_scramble_match")


def test_abi_declares_exports_and_binds_the_scramble_calls():
    text = open(HEADER).read()
    assert re.search(r"^#define\s+FPTA_VERSION\s+10300\b", text, flags=re.M)
    from fakepta_amd import _capi
    lib = ctypes.CDLL(LIB)
    for name in SYMBOLS:
        assert re.search(rf"^int\s+{name}\s*\(", text, flags=re.M), name
        assert hasattr(lib, name), name
        assert name in _capi.EXPORTED, name
    for method in ("batch_set_os_scrambles", "batch_os_scrambles_info", "batch_os_scrambles", "os_scrambles",
                   "os_scramble_match"):
        assert callable(getattr(_capi.Context, method))
    from fakepta_amd.batch import BatchSimulator
    assert callable(BatchSimulator.set_sky_scrambles) and callable(BatchSimulator.sky_scrambles)
    from fakepta import fake_pta
    assert callable(fake_pta.optimal_statistic_scrambles_array)
    assert "os_scramble.hip" in open(os.path.join(CSRC, "Makefile")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in SYMBOLS:
        assert f"`{name}`" in doc, name


def test_scramble_positions_are_unit_vectors_and_follow_the_seed(monkeypatch):
    from fakepta_amd import _capi
    from fakepta_amd import os as osm

    def no_context(*a, **k):
        raise AssertionError("a device context was requested")
    monkeypatch.setattr(_capi, "get_context", no_context)
    pos = osm.scramble_positions(200, 17, seed=5)
    assert pos.shape == (200, 17, 3) and pos.dtype == np.float64 and pos.flags.c_contiguous
    assert np.all(np.abs(np.linalg.norm(pos, axis=-1) - 1.0) <= 1e-12)  # the library's own bound
    np.testing.assert_array_equal(osm.scramble_positions(200, 17, seed=5), pos)
    assert np.any(osm.scramble_positions(200, 17, seed=6) != pos)
    # uniform on the sphere: every coordinate has mean 0 and variance 1 / 3 (3400 draws: 6 sigma is 0.06 and 0.03)
    flat = pos.reshape(-1, 3)
    assert np.all(np.abs(flat.mean(axis=0)) < 0.06) and np.all(np.abs(flat.var(axis=0) - 1 / 3) < 0.03)
    assert osm.scramble_positions(0, 4).shape == (0, 4, 3)
    with pytest.raises(ValueError):
        osm.scramble_positions(-1, 4)


def test_derive_scrambles_on_hand_made_counts():
    from fakepta_amd import os as osm
    snr = np.array([[2.5, -0.5, 0.0], [1.0, 1.0, 1.0]])
    cnt = np.array([[0, 9, 4], [3, 3, 3]], dtype=np.int64)
    mean, std, mx = np.array([0.1, 0.2, 0.3]), np.ones(3), np.array([2.0, 3.0, 4.0])
    out = osm.derive_scrambles(snr, cnt, 9, mean, std, mx, n_orf=1)
    np.testing.assert_array_equal(out["p_value"], [[0.1, 1.0, 0.5]])  # (1 + count) / (1 + 9)
    np.testing.assert_array_equal(out["snr"], snr[:1])
    np.testing.assert_array_equal(out["count_ge"], cnt[:1])
    assert out["null_mean"] is mean and out["null_std"] is std and out["null_max"] is mx and "snr_null" not in out
    both = osm.derive_scrambles(snr, cnt, 9)
    assert both["p_value"].shape == (2, 3) and both["p_value"].min() == 0.1 and "null_mean" not in both
    null = np.zeros((9, 3))
    assert osm.derive_scrambles(snr, cnt, 9, snr_null=null)["snr_null"] is null
    for bad_cnt, J in ((cnt, 8), (-cnt, 9), (cnt.astype(float), 9), (cnt, 0)):
        with pytest.raises(ValueError):
            osm.derive_scrambles(snr, bad_cnt, J)


_MAIN = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "os_scramble_host.h"
// "map P": prints "pairs n_pair n_pad", then "pair e a b" for every entry of the map.
// "check P n_scr form with_nab [data]": form 0 positions [n_scr][P][3] follow, 1 matrices [n_scr][P][P] follow, 2
// neither is given, 3 both are given, 4 positions are given but never read (the shape alone is refused); with_nab 1:
// N_ab [P][P] follows the scrambles. Prints "ok" or "bad reason".
int main() {
  char mode[16];
  long P = 0;
  if (std::scanf("%15s %ld", mode, &P) != 2) return 2;
  if (!std::strcmp(mode, "map")) {
    std::vector<int32_t> ab;
    fpta_scr::make_pair_map(P, ab);
    std::printf("pairs %ld %ld\n", (long)fpta_scr::n_pair(P), (long)fpta_scr::n_pair_pad(P));
    if ((long)ab.size() != 2 * (long)fpta_scr::n_pair_pad(P)) return 3;
    for (size_t e = 0; e < ab.size() / 2; ++e) std::printf("pair %ld %d %d\n", (long)e, ab[2 * e], ab[2 * e + 1]);
    return 0;
  }
  long n_scr = 0;
  int form = 0, with_nab = 0;
  if (std::scanf("%ld %d %d", &n_scr, &form, &with_nab) != 3) return 2;
  std::vector<double> in, nab;
  if (form == 0 || form == 1) {
    in.resize((size_t)(n_scr * P * (form == 0 ? 3 : P)));
    for (double& v : in)
      if (std::scanf("%lf", &v) != 1) return 2;
  }
  if (with_nab) {
    nab.resize((size_t)(P * P));
    for (double& v : nab)
      if (std::scanf("%lf", &v) != 1) return 2;
  }
  const double one = 0.0;
  const double* pos = form == 0 ? in.data() : form == 3 || form == 4 ? &one : nullptr;
  const double* G = form == 1 ? in.data() : form == 3 ? &one : nullptr;
  std::string why;
  if (fpta_scr::validate(P, n_scr, pos, G, with_nab ? nab.data() : nullptr, why))
    std::printf("ok\n");
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
    d = tmp_path_factory.mktemp("os_scramble_host")
    (d / "main.cpp").write_text(_MAIN)
    exe = str(d / "os_scramble_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, str(d / "main.cpp"), "-o", exe], check=True)

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return r.stdout.splitlines()
    return run


@pytest.mark.parametrize("P", [2, 3, 16, 17, 33])
def test_pair_map_is_tril_order_with_marked_padding(host_program, P):
    lines = host_program(f"map {P}\n")
    ia, ib = np.tril_indices(P, -1)
    n_pair = P * (P - 1) // 2
    n_pad = -(-n_pair // 16) * 16
    assert lines[0] == f"pairs {n_pair} {n_pad}" and len(lines) == 1 + n_pad
    got = np.array([[int(v) for v in ln.split()[1:]] for ln in lines[1:]])
    np.testing.assert_array_equal(got[:, 0], np.arange(n_pad))
    np.testing.assert_array_equal(got[:n_pair, 1], ia)  # every pair a > b once, in np.tril_indices' order
    np.testing.assert_array_equal(got[:n_pair, 2], ib)
    assert np.all(got[:n_pair, 1] > got[:n_pair, 2])
    np.testing.assert_array_equal(got[n_pair:, 1:], -1)  # the padding is marked
    assert len({(a, b) for _, a, b in got[:n_pair]}) == n_pair


def _check_input(P, n_scr, form, data=None, nab=None):
    text = f"check {P} {n_scr} {form} {0 if nab is None else 1}\n"
    for arr in (data, nab):
        if arr is not None:
            text += " ".join(repr(float(v)) for v in np.asarray(arr, dtype=np.float64).ravel()) + "\n"
    return text


def test_every_refusal_and_its_message(host_program):
    from fakepta_amd import os as osm
    P, J = 5, 4
    pos = osm.scramble_positions(J, P, seed=3)
    nab = np.ones((P, P)) - np.eye(P)
    G = np.random.default_rng(1).normal(size=(J, P, P))
    G = G + G.transpose(0, 2, 1)
    assert host_program(_check_input(P, J, 0, pos, nab)) == ["ok"]
    assert host_program(_check_input(P, J, 1, G, nab)) == ["ok"]
    assert host_program(_check_input(P, J, 0, pos)) == ["ok"]  # without N_ab: no norm to refuse
    assert host_program(_check_input(P, 0, 4)) == ["ok"]

    def refused(text):
        line, = host_program(text)
        assert line.startswith("bad "), line
        return line[4:]
    # the shape, before anything is read
    assert refused(_check_input(P, 65537, 4)) == "65537 scrambles, more than 65536"
    assert refused(_check_input(1, J, 4)) == "fewer than 2 pulsars: no pair to scramble"
    assert refused(_check_input(P, J, 2)) == "exactly one of positions and matrices must be given"
    assert refused(_check_input(P, J, 3)) == "exactly one of positions and matrices must be given"
    n_pad = -(-(200 * 199 // 2) // 16) * 16  # 200 pulsars: 19 904 padded pairs, 65 536 scrambles of them are > 8 GiB
    assert refused(_check_input(200, 65536, 4)) == (f"the pair rows take {8 * 65536 * n_pad} bytes (8 n_scr n_pair_pad), "
                                                    "more than 8 GiB")
    assert host_program(_check_input(182, 0, 4)) == ["ok"]
    # positions
    bad = pos.copy()
    bad[2, 3, 1] = np.inf
    assert refused(_check_input(P, J, 0, bad, nab)) == "scramble 2, pulsar 3: position is not finite"
    bad = pos.copy()
    bad[1, 4] *= 1.0 + 4e-12
    assert refused(_check_input(P, J, 0, bad, nab)) == "scramble 1, pulsar 4: position is not of unit length"
    bad = pos.copy()
    bad[3, 0] *= 1.0 + 5e-13  # within 1e-12: taken
    assert host_program(_check_input(P, J, 0, bad, nab)) == ["ok"]
    bad = pos.copy()
    bad[3, 4] = bad[3, 1]  # coincident directions: x = 0 and hd is NaN
    assert refused(_check_input(P, J, 0, bad, nab)) == "scramble 3, pair (1, 4): pair weight is not finite"
    # matrices
    bad = G.copy()
    bad[2, 4, 0] = bad[2, 0, 4] = np.nan
    assert refused(_check_input(P, J, 1, bad, nab)) == "scramble 2, pair (0, 4): pair weight is not finite"
    bad = G.copy()
    bad[0, 1, 3] = np.inf  # the upper triangle is checked too
    assert refused(_check_input(P, J, 1, bad, nab)) == "scramble 0, pair (1, 3): pair weight is not finite"
    bad = G.copy()
    bad[1, 2, 1] += 1e-9
    assert refused(_check_input(P, J, 1, bad, nab)) == "scramble 1, pair (1, 2): not symmetric"
    # the norm
    bad = G.copy()
    bad[3] = 0.0
    assert refused(_check_input(P, J, 1, bad, nab)) == "scramble 3: norm is not positive"
    one = np.zeros((P, P))
    one[4, 2] = one[2, 4] = 1.0  # every pair with a weight has N_ab = 0
    only = np.zeros((1, P, P))
    only[0, 1, 0] = only[0, 0, 1] = 2.0
    assert refused(_check_input(P, 1, 1, only, one)) == "scramble 0: norm is not positive"
    assert refused(_check_input(P, J, 0, pos, np.zeros((P, P)))) == "scramble 0: norm is not positive"
    # the first bad scramble is the one reported
    bad = G.copy()
    bad[3] = 0.0
    bad[1, 2, 1] += 1e-9
    assert refused(_check_input(P, J, 1, bad, nab)) == "scramble 1, pair (1, 2): not symmetric"
