"""Fourier fit, host side (no GPU): csrc/fit_host.h (validation, the column build, the rank rule and the operator A_p)
in a stand-alone C++ program built with the address and undefined-behaviour sanitizers, against the np.longdouble
definition of tests/fit_reference.py; the C-ABI surface; the argument checks of BatchSimulator.set_fourier_fit and
fakepta_amd.fit that need no device; the units of power_spectrum."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import fit_reference as F
from tests import tm_reference as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fakepta_amd.h")
LIB = os.path.join(ROOT, "fakepta_amd", "lib", "libfakepta_amd.so")
CSRC = os.path.join(ROOT, "fakepta_amd", "csrc")
ENTRY_POINTS = ("fpta_batch_set_fit", "fpta_batch_fit_info", "fpta_batch_fit", "fpta_batch_fit_cross",
                "fpta_fit_coefficients")
EPS = np.finfo(np.float64).eps
LD = np.longdouble
YEAR = 365.25 * 86400.0

# argv: in out. in: int64 n, m, has_w, n_comp, n_modes [n_comp]; then fp64 idx [n_comp], freqf [n_comp], f [sum N],
# t [n], nu [n], M [n][m], w [n]. out: int64 kept Fourier columns; fp64 A [K][n], kept [K], norms [m + K] (the
# orthogonalised norms rounded to fp64). Without arguments: the checks that need no data.
_MAIN = r"""
#include <cstdio>
#include <cstring>
#include <limits>
#include "fit_host.h"
using namespace fpta_fit;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)
struct Case {
  int64_t P = 3;
  int64_t offs[4] = {0, 3, 3, 7};  // the middle pulsar has no TOAs
  std::vector<double> t, nu, M, w, f, idx, freqf;
  std::vector<int32_t> n_modes;
  int64_t n_col = 2;
  Spec sp;
  Case() : t(7), nu(7, 1400.0), M(7 * 2, 1.0), w(7, 2.0), f{1e-8, 2e-8, 3e-8}, idx{0.0, 2.0}, freqf{1400.0, 1400.0},
           n_modes{2, 1} {
    for (int i = 0; i < 7; ++i) {
      t[i] = 1e7 * (i + 1) + 3e5 * i * i;
      M[2 * i + 1] = (double)i;
    }
    spec();
  }
  Spec& spec() {
    sp.n_comp = (int32_t)n_modes.size();
    sp.n_modes = n_modes.data();
    sp.f = f.data();
    sp.f_is_common = true;
    sp.idx = idx.data();
    sp.freqf = freqf.data();
    return sp;
  }
  bool ok(std::string& why) {
    return validate(P, offs, t.data(), nu.data(), sp, n_col, M.data(), nullptr, w.data(), why);
  }
  bool refused(const char* expect) {
    std::string why;
    const bool good = ok(why);
    std::printf("validate: %s\n", good ? "ok" : why.c_str());
    return !good && why.find(expect) != std::string::npos;
  }
};
static int self_checks() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  std::string why;
  { Case c; CHECK(c.ok(why)); }
  // what tm_host.h's validate refuses comes through with its message
  { Case c; c.n_col = 17; CHECK(c.refused("n_col 17")); }
  { Case c; c.M[5 * 2 + 1] = nan; CHECK(c.refused("pulsar 2, TOA 2, column 1: not finite")); }
  for (double bad : {0.0, -1.0, nan, inf}) { Case c; c.w[4] = bad; CHECK(c.refused("pulsar 2, TOA 1: weight")); }
  // the component list
  { Case c; c.sp.n_comp = 0; CHECK(c.refused("0 components")); }
  { Case c; c.sp.n_comp = 5; CHECK(c.refused("5 components")); }
  { Case c; c.n_modes[1] = 0; CHECK(c.refused("component 1: 0 modes")); }
  { Case c; c.n_modes = {200, 57}; c.f.assign(257, 1e-8); c.spec(); CHECK(c.refused("514 Fourier columns, more than 512")); }
  { Case c; c.n_modes = {200, 56}; c.f.assign(256, 1e-8); c.spec(); CHECK(c.ok(why)); }  // K = 512
  for (double bad : {0.0, -1e-8, nan, inf}) {
    Case c; c.f[2] = bad; CHECK(c.refused("component 1, mode 0: frequency is not positive and finite"));
  }
  { Case c; c.f.assign(9, 1e-8); c.f[3 * 2 + 1] = -1.0; c.spec(); c.sp.f_is_common = false;
    CHECK(c.refused("pulsar 2, component 0, mode 1: frequency")); }
  { Case c; c.idx[1] = nan; CHECK(c.refused("component 1: chromatic index")); }
  { Case c; c.freqf[1] = 0.0; CHECK(c.refused("component 1: reference frequency")); }
  { Case c; c.freqf[0] = 0.0; CHECK(c.ok(why)); }  // idx 0: never read
  for (double bad : {0.0, -1400.0, nan}) {
    Case c; c.nu[5] = bad; CHECK(c.refused("pulsar 2, TOA 2: radio frequency is not positive and finite, and component 1"));
  }
  { Case c; c.nu[5] = 0.0; c.idx[1] = 0.0; CHECK(c.ok(why)); }  // no chromatic index: nu is not read
  { Case c; c.t[1] = inf; CHECK(c.refused("pulsar 0, TOA 1: epoch")); }
  // the plan of an array: a pulsar without TOAs, one with fewer TOAs than columns, the statuses
  {
    Case c;
    Plan plan;
    CHECK(make_plan(c.P, c.offs, c.t.data(), c.nu.data(), c.sp, c.n_col, c.M.data(), nullptr, c.w.data(), 0.0, plan,
                    why) == 0);
    CHECK(plan.K == 6 && plan.A.size() == 6 * 7 && plan.kept.size() == 3 * 6 && plan.rank.size() == 3);
    // 3 TOAs and 2 nuisance columns leave one Fourier column; 4 TOAs leave two; none for the empty pulsar
    CHECK(plan.rank[0] == 1 && plan.rank[1] == 0 && plan.rank[2] == 2 && plan.max_rank == 2);
    CHECK(plan.kept[0] == 1 && plan.kept[1] == 0 && plan.kept[12] == 1 && plan.kept[13] == 1 && plan.kept[14] == 0);
    for (int j = 1; j < 6; ++j)
      for (int s = 0; s < 3; ++s) CHECK(plan.A[j * 3 + s] == 0.0);  // dropped rows are exact zeros
    c.w[2] = 0.0;
    CHECK(make_plan(c.P, c.offs, c.t.data(), c.nu.data(), c.sp, c.n_col, c.M.data(), nullptr, c.w.data(), 0.0, plan,
                    why) == 1 && why.find("weight") != std::string::npos);
  }
  // rank cases on one pulsar of 40 TOAs: a zero nuisance column, a repeated frequency, m = 0, rcond
  {
    const int64_t n = 40;
    std::vector<double> t(n), nu(n, 1400.0), M(n * 2), A, f = {1e-8, 2.5e-8, 1e-8};
    for (int64_t i = 0; i < n; ++i) {
      t[i] = 2.3e6 * i + 4e4 * (i % 7);
      M[2 * i] = 0.0;
      M[2 * i + 1] = 1.0;
    }
    const int32_t nm[1] = {3};
    const double idx[1] = {0.0}, ff[1] = {1400.0};
    Spec sp;
    sp.n_comp = 1; sp.n_modes = nm; sp.f = f.data(); sp.idx = idx; sp.freqf = ff;
    A.assign(6 * n, -1.0);
    uint8_t kept[6];
    long double norms[8];
    CHECK(build_operator(n, t.data(), nu.data(), 2, M.data(), 2, nullptr, sp, f.data(), 0.0, A.data(), kept, norms) == 4);
    CHECK(norms[0] == 0.0L && norms[1] > 0.99L);                       // the zero column, the offset
    CHECK(kept[0] && kept[1] && !kept[2] && kept[3] && kept[4] && !kept[5]);  // the repeated mode's cos and sin go
    CHECK(norms[2 + 2] < 1e-15L && norms[2 + 5] < 1e-15L);
    for (int64_t s = 0; s < n; ++s) CHECK(A[2 * n + s] == 0.0 && A[5 * n + s] == 0.0 && A[0 * n + s] != -1.0);
    CHECK(build_operator(n, t.data(), nu.data(), 0, nullptr, 0, nullptr, sp, f.data(), 0.0, A.data(), kept) == 4);
    CHECK(build_operator(n, t.data(), nu.data(), 0, nullptr, 0, nullptr, sp, f.data(), 0.9999, A.data(), kept) <= 2);
  }
  std::printf("%s\n", fails ? "failed" : "all ok");
  return fails ? 1 : 0;
}
int main(int argc, char** argv) {
  if (argc < 3) return self_checks();
  std::FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  int64_t hdr[4];
  if (std::fread(hdr, sizeof(int64_t), 4, in) != 4) return 2;
  const int64_t n = hdr[0], m = hdr[1], nc = hdr[3];
  std::vector<int64_t> nm64((size_t)nc);
  if (std::fread(nm64.data(), sizeof(int64_t), nm64.size(), in) != nm64.size()) return 2;
  std::vector<int32_t> nm(nm64.begin(), nm64.end());
  int64_t nf = 0;
  for (int64_t v : nm64) nf += v;
  std::vector<double> idx((size_t)nc), ff((size_t)nc), f((size_t)nf), t((size_t)n), nu((size_t)n), M((size_t)(n * m)),
      w((size_t)n);
  for (std::vector<double>* v : {&idx, &ff, &f, &t, &nu, &M})
    if (std::fread(v->data(), sizeof(double), v->size(), in) != v->size()) return 2;
  if (hdr[2] && std::fread(w.data(), sizeof(double), w.size(), in) != w.size()) return 2;
  std::fclose(in);
  Spec sp;
  sp.n_comp = (int32_t)nc; sp.n_modes = nm.data(); sp.f = f.data(); sp.idx = idx.data(); sp.freqf = ff.data();
  const int64_t K = 2 * nf;
  std::vector<double> A((size_t)(K * n)), kd((size_t)K), nd((size_t)(m + K));
  std::vector<uint8_t> kept((size_t)K);
  std::vector<long double> norms((size_t)(m + K));
  const int64_t k = build_operator(n, t.data(), nu.data(), (int32_t)m, M.data(), m, hdr[2] ? w.data() : nullptr, sp,
                                   f.data(), 0.0, A.data(), kept.data(), norms.data());
  for (int64_t j = 0; j < K; ++j) kd[(size_t)j] = kept[(size_t)j];
  for (int64_t j = 0; j < m + K; ++j) nd[(size_t)j] = (double)norms[(size_t)j];
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  std::fwrite(&k, sizeof(int64_t), 1, out);
  std::fwrite(A.data(), sizeof(double), A.size(), out);
  std::fwrite(kd.data(), sizeof(double), kd.size(), out);
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
    d = tmp_path_factory.mktemp("fit_host")
    (d / "main.cpp").write_text(_MAIN)
    exe = str(d / "fit_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-pthread", "-I", CSRC, str(d / "main.cpp"), "-o", exe], check=True)
    return exe


def test_host_planner_under_the_sanitizers(host_exe):
    """Every validation message (what tm_host.h refuses, the component list, K = 512 accepted and 514 refused, f, idx,
    freqf, nu with a chromatic index, epochs), a pulsar without TOAs, n_p < K_p, a zero column, a repeated frequency,
    m = 0 and rcond."""
    r = subprocess.run([host_exe], capture_output=True, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("all ok"), r.stdout[-4000:] + r.stderr[-4000:]


def _pulsar(rng, n, span=15 * YEAR):
    t = np.sort(rng.uniform(0.0, span, n))
    nu = T.three_band(rng, n)
    return t, nu, T.mmat(t, nu), 1 / rng.uniform(1e-7, 1e-6, n) ** 2


def _layouts():
    """The shapes of the issue's table (TOAs uniform over the span, make_Mmat's eight columns, three bands, white
    weights), 1 / yr beside the annual columns, and two components on unit weights without a nuisance design."""
    rng = np.random.default_rng(20251)
    span = 15 * YEAR
    out = {}
    for name, n, N in (("n17_N4", 17, 4), ("n33_N9", 33, 9), ("n250_N30", 250, 30), ("n600_N30", 600, 30),
                       ("n2000_N100", 2000, 100), ("n5_N2", 5, 2)):
        t, nu, M, w = _pulsar(rng, n)
        out[name] = (t, nu, M, w, [(np.arange(1, N + 1) / span, 0.0, 1400.0)])
    t, nu, M, w = _pulsar(rng, 300)
    out["one_per_year"] = (t, nu, M, w, [(np.array([0.4 / YEAR, 1 / YEAR, 2.3 / YEAR]), 0.0, 1400.0)])
    t, nu, _, _ = _pulsar(rng, 120)
    out["two_components_m0"] = (t, nu, None, None, [(np.arange(1, 6) / span, 0.0, 1400.0),
                                                     (np.arange(1, 5) / span, 2.0, 1400.0)])
    return out


# a floor a little below the smallest orthogonalised norm of a kept Fourier column measured for these shapes, and
# the kept Fourier columns. On the 15.0-yr span mode 15 is 1 / yr: the pulsars with 30 or 100 modes drop that pair too
_EXPECT = {"n17_N4": (0.05, 8), "n33_N9": (0.015, 18), "n250_N30": (0.03, 58), "n600_N30": (0.03, 58),
           "n2000_N100": (0.2, 198), "n5_N2": (None, 0), "one_per_year": (0.05, 4), "two_components_m0": (0.05, 18)}


@pytest.mark.parametrize("name", sorted(_EXPECT))
def test_operator_matches_the_longdouble_definition(host_exe, tmp_path, name):
    """A_p to <= 1 eps per entry relative to its row's largest entry, the kept mask and the orthogonalised norms."""
    t, nu, M, w, comps = _layouts()[name]
    n, m = len(t), 0 if M is None else M.shape[1]
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.array([n, m, 0 if w is None else 1, len(comps)] + [len(c[0]) for c in comps],
                          dtype=np.int64).tobytes())
        for a in ([c[1] for c in comps], [c[2] for c in comps], np.concatenate([c[0] for c in comps]), t, nu):
            fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        if M is not None:
            fh.write(np.ascontiguousarray(M).tobytes())
        if w is not None:
            fh.write(np.ascontiguousarray(w).tobytes())
    r = subprocess.run([host_exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(tmp_path / "out.bin", "rb").read()
    k = int(np.frombuffer(raw[:8], dtype=np.int64)[0])
    body = np.frombuffer(raw[8:], dtype=np.float64)
    K = 2 * sum(len(c[0]) for c in comps)
    A, kept, norms = body[:K * n].reshape(K, n), body[K * n:K * n + K] != 0, body[K * n + K:]
    At, kept_t, norms_t, keep_all = F.operator_ld(t, nu, M, w, comps)
    T.assert_clear_rank(norms_t, keep_all, M)
    floor, n_kept = _EXPECT[name]
    fn = norms_t[m:]
    print(f"{name}: kept {k} of {K}; orthogonalised Fourier norms: smallest kept "
          f"{float(fn[kept_t].min()) if kept_t.any() else float('nan'):.3g}, largest dropped "
          f"{float(fn[~kept_t].max()) if (~kept_t).any() else 0.0:.3g}")
    assert k == n_kept == int(kept_t.sum()) and len(norms) == m + K
    np.testing.assert_array_equal(kept, kept_t)
    if floor is not None:
        assert fn[kept_t].min() >= floor
    np.testing.assert_allclose(norms[keep_all], norms_t[keep_all].astype(np.float64), rtol=1e-12)
    assert np.all(norms[~keep_all] <= T.DROP_MAX)
    assert np.all(A[~kept] == 0.0)
    if name == "one_per_year":  # 1 / yr is the annual pair of make_Mmat: its cosine and sine are dropped
        assert list(kept) == [True, False, True, True, False, True]
    if kept.any():
        row_max = np.max(np.abs(At[kept]), axis=1, keepdims=True)
        err = float(np.max(np.abs(A[kept].astype(LD) - At[kept]) / row_max)) / EPS
        print(f"{name}: |A - A_ld| <= {err:.3f} eps of the row's largest entry")
        assert err <= 1.0


def test_abi_declares_exports_and_binds_the_entry_points():
    from fakepta_amd import _capi
    text = open(HEADER).read()
    lib = ctypes.CDLL(LIB)
    for name in ENTRY_POINTS:
        assert re.search(rf"^int\s+{name}\s*\(", text, flags=re.M), name
        assert hasattr(lib, name) and name in _capi.EXPORTED
    assert re.search(r"^#define\s+FPTA_VERSION\s+10300\b", text, flags=re.M)
    for method in ("batch_set_fit", "batch_fit", "batch_fit_cross", "fit_coefficients"):
        assert hasattr(_capi.Context, method)
    host = open(os.path.join(CSRC, "fit_host.h")).read()
    assert "#include <hip" not in host and "__global__" not in host and "__device__" not in host  # plain C++
    assert '#include "tm_host.h"' in host and "fpta_tm::validate" in host  # shared, not copied
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "fit.hip" in make and "fit_host.h" in make


class _RecordingCtx:
    """Stands in for a device context: records the calls a BatchSimulator makes."""

    def __init__(self, P):
        self.calls, self.P = [], P

    def __getattr__(self, name):
        def call(*a, **k):
            self.calls.append((name, a, k))
            if name == "batch_set_fit":
                K = 2 * int(np.sum(a[0]))
                return np.full(self.P, K, dtype=np.int32), np.ones((self.P, K), dtype=bool)
        return call


class _Psr:
    def __init__(self, n, m=3, t1=1e8):
        self.toas = np.linspace(0.0, t1, n)
        self.freqs = np.full(n, 1400.0)
        self.Mmat = np.vander(self.toas / 1e8, m)
        self.signal_model = {}
        self.s2 = np.linspace(1.0, 2.0, n)

    def _white_sigma2(self):
        return self.s2


def test_set_fourier_fit_argument_checks_need_no_device():
    from fakepta_amd.batch import BatchSimulator
    psrs = [_Psr(5), _Psr(7, t1=2e8)]
    ctx = _RecordingCtx(len(psrs))
    sim = BatchSimulator(psrs, signals=[], white=False, ctx=ctx)
    sim.segments.append(dict(name="red_noise", kind=0, f=np.array([[1e-8, 2e-8], [3e-8, 6e-8]]), idx=0.0,
                             freqf=1400.0))
    sim.segments.append(dict(name="gw_common", kind=1, f=np.array([1e-8, 2e-8, 3e-8]), idx=0.0, freqf=1400.0))
    n0 = len(ctx.calls)
    for call in (sim.fourier_fit, sim.power_spectrum, sim.cross_spectrum, lambda: sim.hd_curve(domain="fourier")):
        with pytest.raises(ValueError, match="no Fourier fit"):
            call()
    with pytest.raises(ValueError, match="domain"):
        sim.hd_curve(domain="frequency")
    for bad in ([], [(1, 0.0)] * 5, [(0, 0.0)], [(2.5, 0.0)], [(np.ones((3, 4)), 0.0)], [(np.array([1e-8, -1e-8]), 0.0)],
                [(300, 0.0)], [(np.array([1e-8, np.nan]), 0.0)], [(3, np.inf)], [3]):
        with pytest.raises(ValueError):
            sim.set_fourier_fit(bad)
    with pytest.raises(KeyError, match="dm_gp"):
        sim.set_fourier_fit(["dm_gp"])
    with pytest.raises(ValueError, match="common=True"):
        sim.set_fourier_fit(["red_noise"], common=True)
    for bad in ("design", [psrs[0].Mmat], [psrs[0].Mmat, psrs[1].Mmat[:-1]], [psrs[0].Mmat, np.ones((7, 17))]):
        with pytest.raises(ValueError):
            sim.set_fourier_fit(Mmats=bad)
    with pytest.raises(ValueError):
        sim.set_fourier_fit(weights="ecorr")
    assert len(ctx.calls) == n0  # refused before anything reached the context
    # the default: 30 achromatic modes at k / Tspan of the array, one grid, each pulsar's Mmat marginalised
    rank, kept = sim.set_fourier_fit()
    name, a, k = ctx.calls[-1]
    assert name == "batch_set_fit" and list(a[0]) == [30] and list(a[2]) == [0.0] and a[1].shape == (30,)
    np.testing.assert_array_equal(a[1], np.arange(1, 31) / 2e8)
    assert k["M"].shape == (12, 3) and list(k["ncol_psr"]) == [3, 3] and k["weights"].shape == (12,)
    assert list(rank) == [60, 60] and kept.shape == (2, 60)
    # signal names take f and idx of the layout; a per-pulsar one makes every grid per-pulsar
    sim.set_fourier_fit(["gw_common", (2, 2.0)], Mmats=None, weights=None)
    name, a, k = ctx.calls[-1]
    assert list(a[0]) == [3, 2] and a[1].shape == (5,) and list(a[2]) == [0.0, 2.0]
    assert k["M"].shape == (12, 0) and k["weights"] is None
    sim.set_fourier_fit(["red_noise", "gw_common"])
    assert ctx.calls[-1][1][1].shape == (2, 5)
    with pytest.raises(ValueError, match="per-pulsar"):
        sim.cross_spectrum()
    sim.set_fourier_fit(["gw_common"], common=False)
    assert ctx.calls[-1][1][1].shape == (2, 3)


def test_power_spectrum_units_on_coefficients_built_by_hand():
    """(a_cos^2 + a_sin^2) / (2 df), df = diff(append(0, f)), averaged over realizations: amplitudes of variance
    psd df per quadrature give back psd, whatever the grid."""
    from fakepta_amd import fit
    f = np.array([1e-9, 3e-9, 4e-9, 2e-9, 2.5e-9])  # two components: 3 modes and 2 modes
    n_modes = [3, 2]
    coef = np.zeros((2, 10, 4))
    coef[0, 0] = [1.0, -1.0, 1.0, -1.0]      # cos of component 0, mode 0
    coef[0, 3] = [2.0, 2.0, -2.0, -2.0]      # its sine
    coef[0, 2] = 3.0                         # cos of mode 2
    coef[1, 6] = [1.0, 0.0, 0.0, 0.0]        # cos of component 1, mode 0
    coef[1, 9] = 4.0                         # sine of component 1, mode 1
    ps = fit.power_spectrum(coef, n_modes, f)
    assert [p.shape for p in ps] == [(2, 3), (2, 2)]
    np.testing.assert_allclose(ps[0][0], [(1 + 4) / (2 * 1e-9), 0.0, 9 / (2 * 1e-9)], rtol=1e-15)
    np.testing.assert_allclose(ps[1][1], [0.25 / (2 * 2e-9), 16 / (2 * 0.5e-9)], rtol=1e-15)
    assert np.all(ps[0][1] == 0) and np.all(ps[1][0] == 0)
    np.testing.assert_allclose(fit.mode_delta_f(n_modes, f), [1e-9, 2e-9, 1e-9, 2e-9, 0.5e-9], rtol=1e-15)
    # per-pulsar grids: each row's own df
    f2 = np.stack([f, 2 * f])
    ps2 = fit.power_spectrum(coef, n_modes, f2)
    np.testing.assert_allclose(ps2[0][0], ps[0][0], rtol=1e-15)
    np.testing.assert_allclose(ps2[1][1], ps[1][1] / 2, rtol=1e-15)
    # drawn amplitudes: the mean comes back as the psd within the scatter of 2 R degrees of freedom
    rng = np.random.default_rng(8)
    psd = np.array([3e-12, 1e-12, 2e-13])
    fg = np.array([1e-9, 2e-9, 3e-9])
    R = 4000
    a = rng.normal(size=(1, 6, R)) * np.sqrt(np.repeat(psd * fit.delta_f(fg), 1))[[0, 1, 2, 0, 1, 2], None]
    got = fit.power_spectrum(a, [3], fg)[0][0]
    assert np.all(np.abs(got / psd - 1) < 6 / np.sqrt(R))


def test_fake_pta_imports_and_fit_module_needs_numpy_and_the_binding_only():
    code = ("from fakepta import fake_pta as fp; import fakepta_amd.fit as fit; "
            "assert callable(fp.fit_fourier_array) and callable(fp.Pulsar.fit_fourier); print(fit.MAX_COEF)")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "512", r.stderr
    src = open(os.path.join(ROOT, "fakepta_amd", "fit.py")).read()
    assert sorted(re.findall(r"^(?:import|from)\s+(\S+)", src, flags=re.M)) == [".", ".", "numpy"]
