"""Timing-model projection, host side (no GPU): csrc/tm_host.h (validation, the basis build and its rank rule) in a
stand-alone C++ program built with the address and undefined-behaviour sanitizers, against the np.longdouble definition
of tests/tm_reference.py; the C-ABI surface; the argument checks of BatchSimulator.synth(fit=True) and
set_timing_model that need no device; the import of the drop-in module."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import tm_reference as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fakepta_amd.h")
LIB = os.path.join(ROOT, "fakepta_amd", "lib", "libfakepta_amd.so")
CSRC = os.path.join(ROOT, "fakepta_amd", "csrc")
ENTRY_POINTS = ("fpta_batch_set_timing_model", "fpta_batch_project", "fpta_tm_project")
EPS = np.finfo(np.float64).eps
LD = np.longdouble
YEAR = 365.25 * 86400.0

# argv: in out. in: int64 n, m, has_w, then M [n][m] and w [n] (fp64). out: int64 k, Q [n][16], s [n], norms [m] (the
# orthogonalised norms rounded to fp64). Without arguments: the checks that need no data.
_MAIN = r"""
#include <cstdio>
#include <cstring>
#include <limits>
#include "tm_host.h"
using namespace fpta_tm;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)
static bool refused(int64_t P, const int64_t* offs, int64_t n_col, const double* M, const int32_t* ncol,
                    const double* w, const char* expect) {
  std::string why;
  const bool ok = validate(P, offs, n_col, M, ncol, w, why);
  std::printf("validate: %s\n", ok ? "ok" : why.c_str());
  return !ok && why.find(expect) != std::string::npos;
}
static int self_checks() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const int64_t offs[4] = {0, 3, 3, 7};  // the middle pulsar has no TOAs
  std::vector<double> M17(7 * 17, 1.0), w(7, 2.0);
  std::string why;
  CHECK(validate(3, offs, 16, M17.data(), nullptr, w.data(), why));   // m = 16
  CHECK(validate(3, offs, 0, nullptr, nullptr, nullptr, why));        // m = 0
  CHECK(validate(0, nullptr, 8, nullptr, nullptr, nullptr, why));
  CHECK(refused(3, offs, 17, M17.data(), nullptr, w.data(), "n_col 17"));
  CHECK(refused(3, offs, -1, M17.data(), nullptr, w.data(), "n_col -1"));
  const int32_t over[3] = {2, 0, 5}, fine[3] = {2, 0, 4}, neg[3] = {2, -1, 4};
  CHECK(refused(3, offs, 4, M17.data(), over, nullptr, "pulsar 2: 5 columns"));
  CHECK(refused(3, offs, 4, M17.data(), neg, nullptr, "pulsar 1: -1 columns"));
  CHECK(validate(3, offs, 4, M17.data(), fine, nullptr, why));
  std::vector<double> M(7 * 4, 1.0);
  M[5 * 4 + 2] = nan;
  CHECK(refused(3, offs, 4, M.data(), nullptr, nullptr, "pulsar 2, TOA 2, column 2: not finite"));
  M[5 * 4 + 2] = -inf;
  CHECK(refused(3, offs, 4, M.data(), fine, nullptr, "pulsar 2, TOA 2, column 2"));
  M[5 * 4 + 2] = 1.0;
  M[1 * 4 + 3] = nan;  // pulsar 0 uses two columns only: column 3 is never read
  CHECK(validate(3, offs, 4, M.data(), fine, nullptr, why));
  CHECK(refused(3, offs, 4, M.data(), nullptr, nullptr, "pulsar 0, TOA 1, column 3"));
  M[1 * 4 + 3] = 1.0;
  for (double bad : {0.0, -1.0, nan, inf}) {
    w[4] = bad;
    CHECK(refused(3, offs, 4, M.data(), nullptr, w.data(), "pulsar 2, TOA 1: weight"));
  }
  w[4] = 1e-300;
  CHECK(validate(3, offs, 4, M.data(), nullptr, w.data(), why));
  const int64_t down[3] = {0, 4, 3}, off1[2] = {1, 4};
  CHECK(refused(2, down, 4, M.data(), nullptr, nullptr, "offs decreases"));
  CHECK(refused(1, off1, 4, M.data(), nullptr, nullptr, "offs[0]"));
  // an all-zero column, a repeated column and a zero matrix
  {
    const int64_t n = 6;
    std::vector<double> A(n * 4), Q(n * kMaxCol, -1.0), s(n, -1.0);
    for (int64_t t = 0; t < n; ++t) {
      A[t * 4] = 1.0;
      A[t * 4 + 1] = 0.0;
      A[t * 4 + 2] = (double)t;
      A[t * 4 + 3] = 1.0;
    }
    long double norms[4];
    CHECK(build_basis(n, 4, A.data(), 4, nullptr, 0.0, Q.data(), s.data(), norms) == 2);
    CHECK(std::fabs(norms[0] - 1.0L) < 1e-18L && norms[1] == 0.0L && norms[2] > 0.5L && norms[3] < 1e-18L);
    for (int64_t t = 0; t < n; ++t) {
      CHECK(s[t] == 1.0 && std::fabs(Q[t * kMaxCol] - 1.0 / std::sqrt(6.0)) < 4e-16);
      for (int j = 2; j < kMaxCol; ++j) CHECK(Q[t * kMaxCol + j] == 0.0);
    }
    std::vector<double> Z(n * 3, 0.0);
    CHECK(build_basis(n, 3, Z.data(), 3, nullptr, 0.0, Q.data(), s.data()) == 0);
    CHECK(build_basis(n, 0, nullptr, 0, nullptr, 0.0, Q.data(), s.data()) == 0);
    for (int64_t i = 0; i < n * kMaxCol; ++i) CHECK(Q[i] == 0.0);
    // rcond: the ramp against the constant has orthogonalised norm ~0.58 of its own: a rule of 0.9 drops it
    CHECK(build_basis(n, 3, A.data(), 4, nullptr, 0.9, Q.data(), s.data()) == 1);
  }
  // the plan of an array: per-pulsar column counts, a pulsar without TOAs, the weights' square roots
  {
    std::vector<double> A(7 * 2);
    for (int64_t t = 0; t < 7; ++t) {
      A[t * 2] = 1.0;
      A[t * 2 + 1] = (double)(t * t);
    }
    const int32_t ncol[3] = {2, 2, 1};
    std::vector<double> ww = {1, 4, 9, 16, 25, 36, 49};
    Plan plan;
    CHECK(make_plan(3, offs, 2, A.data(), ncol, ww.data(), 0.0, plan, why));
    CHECK(plan.rank.size() == 3 && plan.rank[0] == 2 && plan.rank[1] == 0 && plan.rank[2] == 1 && plan.max_rank == 2);
    CHECK(plan.Q.size() == 7 * kMaxCol && plan.s.size() == 7);
    for (int64_t t = 0; t < 7; ++t) CHECK(plan.s[t] == (double)(t + 1));
    for (int64_t t = 3; t < 7; ++t) CHECK(plan.Q[t * kMaxCol + 1] == 0.0 && plan.Q[t * kMaxCol] > 0.0);
    ww[2] = 0.0;
    CHECK(!make_plan(3, offs, 2, A.data(), ncol, ww.data(), 0.0, plan, why) && why.find("weight") != std::string::npos);
  }
  std::printf("%s\n", fails ? "failed" : "all ok");
  return fails ? 1 : 0;
}
int main(int argc, char** argv) {
  if (argc < 3) return self_checks();
  std::FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  int64_t hdr[3];
  if (std::fread(hdr, sizeof(int64_t), 3, in) != 3) return 2;
  const int64_t n = hdr[0], m = hdr[1];
  std::vector<double> M((size_t)(n * m)), w((size_t)n);
  if (std::fread(M.data(), sizeof(double), M.size(), in) != M.size()) return 2;
  if (hdr[2] && std::fread(w.data(), sizeof(double), w.size(), in) != w.size()) return 2;
  std::fclose(in);
  std::vector<double> Q((size_t)(n * kMaxCol)), s((size_t)n), nd((size_t)m);
  std::vector<long double> norms((size_t)m);
  const int64_t k = build_basis(n, (int32_t)m, M.data(), m, hdr[2] ? w.data() : nullptr, 0.0, Q.data(), s.data(),
                                norms.data());
  for (int64_t j = 0; j < m; ++j) nd[(size_t)j] = (double)norms[(size_t)j];
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  std::fwrite(&k, sizeof(int64_t), 1, out);
  std::fwrite(Q.data(), sizeof(double), Q.size(), out);
  std::fwrite(s.data(), sizeof(double), s.size(), out);
  std::fwrite(nd.data(), sizeof(double), nd.size(), out);
  std::fclose(out);
  return 0;
}
"""


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("tm_host")
    (d / "main.cpp").write_text(_MAIN)
    exe = str(d / "tm_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, str(d / "main.cpp"), "-o", exe], check=True)
    return exe


def test_host_planner_under_the_sanitizers(host_exe):
    """Validation (m = 0 and 16 accepted, 17 refused, non-finite M and w <= 0 refused with the index named), an
    all-zero column, a repeated column, rcond, per-pulsar column counts and a pulsar without TOAs."""
    r = subprocess.run([host_exe], capture_output=True, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("all ok"), r.stdout[-3000:] + r.stderr[-3000:]


def _layouts():
    rng = np.random.default_rng(20250)
    t = np.sort(rng.uniform(0.0, 15 * YEAR, 2000))
    t5 = np.sort(rng.uniform(0.0, 15 * YEAR, 5))
    sig = rng.uniform(1e-7, 1e-6, 2000)
    return {"three_band": (T.mmat(t, T.three_band(rng, 2000)), 1 / sig ** 2, 8),
            "single_frequency": (T.mmat(t, np.full(2000, 1400.0)), None, 5),
            "five_toas": (T.mmat(t5, T.three_band(rng, 5)), 1 / sig[:5] ** 2, 5)}


@pytest.mark.parametrize("name", ["three_band", "single_frequency", "five_toas"])
def test_basis_matches_the_longdouble_definition(host_exe, tmp_path, name):
    """2000 TOAs over 15 yr on three bands (rank 8), on one frequency (rank 5: the three DM columns are multiples of
    the spin columns) and 5 TOAs (rank 5): the rank, Q^T Q = I to 4 eps, the span of the longdouble basis, s."""
    M, w, rank = _layouts()[name]
    n, m = M.shape
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.array([n, m, 0 if w is None else 1], dtype=np.int64).tobytes())
        fh.write(np.ascontiguousarray(M).tobytes())
        if w is not None:
            fh.write(np.ascontiguousarray(w).tobytes())
    r = subprocess.run([host_exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(tmp_path / "out.bin", "rb").read()
    k = int(np.frombuffer(raw[:8], dtype=np.int64)[0])
    body = np.frombuffer(raw[8:], dtype=np.float64)
    Q, s, norms = body[:n * 16].reshape(n, 16), body[n * 16:n * 17], body[n * 17:]
    Qt, norms_t, keep = T.basis_ld(M, w)
    T.assert_clear_rank(norms_t, keep, M)
    print(f"{name}: rank {k}, orthogonalised norms", " ".join(f"{float(x):.1e}" for x in norms_t))
    assert k == rank == Qt.shape[1] and len(norms) == m
    np.testing.assert_allclose(norms[keep], norms_t[keep].astype(np.float64), rtol=1e-12)
    assert np.all(norms[~keep] <= T.DROP_MAX)
    assert np.all(Q[:, k:] == 0.0)
    np.testing.assert_array_equal(s, np.ones(n) if w is None else np.sqrt(w.astype(LD)).astype(np.float64))
    Ql = Q[:, :k].astype(LD)
    gram = np.abs(Ql.T @ Ql - np.eye(k, dtype=LD)).max()
    span = np.abs(Ql - Qt @ (Qt.T @ Ql)).max()  # what of Q lies outside the truth's span
    same = np.abs(Ql - Qt).max()
    print(f"{name}: |Q^T Q - I| {float(gram) / EPS:.2f} eps, outside the span {float(span) / EPS:.2f} eps, "
          f"|Q - Q_ld| {float(same) / EPS:.2f} eps")
    assert gram <= 4 * EPS and span <= 4 * EPS and same <= 4 * EPS


def test_abi_declares_exports_and_binds_the_entry_points():
    from fakepta_amd import _capi
    text = open(HEADER).read()
    lib = ctypes.CDLL(LIB)
    for name in ENTRY_POINTS:
        assert re.search(rf"^int\s+{name}\s*\(", text, flags=re.M), name
        assert hasattr(lib, name) and name in _capi.EXPORTED
    assert re.search(r"^#define\s+FPTA_VERSION\s+10300\b", text, flags=re.M)
    assert re.search(r"^#define\s+FPTA_K_N\s+8\b", text, flags=re.M)
    for method in ("batch_set_timing_model", "batch_project", "tm_project"):
        assert hasattr(_capi.Context, method)
    host = open(os.path.join(CSRC, "tm_host.h")).read()
    assert "#include <hip" not in host and "__global__" not in host and "__device__" not in host  # plain C++
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "tm.hip" in make and "tm_host.h" in make


class _RecordingCtx:
    """Stands in for a device context: records the calls a BatchSimulator makes."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a, **k):
            self.calls.append(name)
            if name == "batch_set_timing_model":
                return np.zeros(2, dtype=np.int32)
        return call


class _Psr:
    def __init__(self, n, m=3):
        self.toas = np.linspace(0.0, 1e8, n)
        self.freqs = np.full(n, 1400.0)
        self.Mmat = np.vander(self.toas / 1e8, m)
        self.signal_model = {}
        self.s2 = np.linspace(1.0, 2.0, n)

    def _white_sigma2(self):
        return self.s2


def test_batch_simulator_argument_checks_need_no_device():
    from fakepta_amd.batch import BatchSimulator
    ctx = _RecordingCtx()
    psrs = [_Psr(5), _Psr(7)]
    sim = BatchSimulator(psrs, signals=[], white=False, ctx=ctx)
    n0 = len(ctx.calls)
    with pytest.raises(ValueError, match="no timing model"):
        sim.synth(4, fit=True)
    assert len(ctx.calls) == n0  # refused before anything reached the context
    for bad in ([psrs[0].Mmat], [psrs[0].Mmat, psrs[1].Mmat[:-1]], [psrs[0].Mmat, np.ones(7)],
                [psrs[0].Mmat, np.ones((7, 17))]):
        with pytest.raises(ValueError):
            sim.set_timing_model(bad)
    for bad in ("ecorr", np.ones(11), [np.ones(5), np.ones(6)]):
        with pytest.raises(ValueError):
            sim.set_timing_model(weights=bad)
    assert len(ctx.calls) == n0
    rank = sim.set_timing_model()
    assert ctx.calls[n0:] == ["batch_set_timing_model"] and len(rank) == 2
    sim.synth(4, fit=True, to_host=False)
    assert ctx.calls[n0 + 1:] == ["batch_synth", "batch_project"]
    sim.set_timing_model([])  # cleared
    with pytest.raises(ValueError, match="no timing model"):
        sim.synth(4, fit=True)


def test_stacked_design_and_weights():
    from fakepta_amd import tm
    psrs = [_Psr(5, 3), _Psr(7, 0), _Psr(2, 4)]
    M, ncol = tm.stack_design([p.Mmat for p in psrs])
    assert M.shape == (14, 4) and list(ncol) == [3, 0, 4] and ncol.dtype == np.int32
    np.testing.assert_array_equal(M[:5, :3], psrs[0].Mmat)
    assert np.all(M[:5, 3] == 0) and np.all(M[5:12] == 0)
    np.testing.assert_array_equal(M[12:], psrs[2].Mmat)
    w = tm.weights_of(psrs, "white", 14)
    np.testing.assert_array_equal(w, 1 / np.concatenate([p.s2 for p in psrs]))
    assert tm.weights_of(psrs, None, 14) is None
    np.testing.assert_array_equal(tm.weights_of(psrs, [p.s2 for p in psrs], 14), np.concatenate([p.s2 for p in psrs]))


def test_fake_pta_imports_with_nothing_new():
    """The drop-in module gained two functions and one import, fakepta_amd.tm, which itself needs numpy and the
    binding only."""
    code = ("from fakepta import fake_pta as fp; import fakepta_amd.tm as tm; "
            "assert callable(fp.fit_timing_model_array) and callable(fp.Pulsar.fit_timing_model); print(tm.MAX_COL)")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "16", r.stderr
    tm_src = open(os.path.join(ROOT, "fakepta_amd", "tm.py")).read()
    assert sorted(re.findall(r"^(?:import|from)\s+(\S+)", tm_src, flags=re.M)) == [".", "numpy"]
