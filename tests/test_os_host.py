"""Optimal statistic, host side (no GPU): csrc/os_host.h (validation, the stacked orthogonalisation, the operator
B_p = F_p^T P_p^-1, Z_p and the pair normalisations N_ab) in a stand-alone C++ program built with the address and
undefined-behaviour sanitizers, against the np.longdouble definition of tests/os_reference.py; the C-ABI surface; the
host algebra and argument checks of fakepta_amd.os that need no device; the unbiasedness of the definition."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import os_reference as OS
from tests import tm_reference as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fakepta_amd.h")
LIB = os.path.join(ROOT, "fakepta_amd", "lib", "libfakepta_amd.so")
CSRC = os.path.join(ROOT, "fakepta_amd", "csrc")
ENTRY_POINTS = ("fpta_batch_set_os", "fpta_batch_os_info", "fpta_batch_os", "fpta_os_statistic")
EPS = np.finfo(np.float64).eps
LD = np.longdouble
YEAR = 365.25 * 86400.0

# argv: in out. in: int64 P, n_col, has_w, C, target, has_mask, n_g, f_common; offs [P + 1]; ncol [P]; n_modes [C]; then
# fp64 idx [C], freqf [C], f [rows][sum N], phi [P][sum N], phi_hat [N], t [n], nu [n], M [n][n_col], w [n] (has_w),
# G [n_g][P][P]; then uint8 mask [C][n] (has_mask). out: fp64 B [K n], Z [P][K][K], N_ab [P][P], rank [P], rows [P].
# Without arguments: the checks that need no data.
_MAIN = r"""
#include <cstdio>
#include <cstring>
#include <limits>
#include "os_host.h"
using namespace fpta_os;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)
struct Case {
  int64_t P = 3;
  int64_t offs[4] = {0, 3, 3, 7};  // the middle pulsar has no TOAs
  std::vector<double> t, nu, M, w, f, idx, freqf, phi, phi_hat, G;
  std::vector<int32_t> n_modes;
  std::vector<uint8_t> mask;
  int64_t n_col = 2;
  int32_t n_g = 2;
  Spec sp;
  Case() : t(7), nu(7, 1400.0), M(7 * 2, 1.0), w(7, 2.0), f{1e-8, 2e-8, 3e-8}, idx{0.0, 2.0}, freqf{1400.0, 1400.0},
           phi(3 * 3, 1e-2), phi_hat{1.0, 0.5}, G(2 * 9, 0.25), n_modes{2, 1} {
    for (int i = 0; i < 7; ++i) {
      t[i] = 1e7 * (i + 1) + 3e5 * i * i;
      M[2 * i + 1] = (double)i;
    }
    spec();
  }
  Spec& spec() {
    sp.comps.n_comp = (int32_t)n_modes.size();
    sp.comps.n_modes = n_modes.data();
    sp.comps.f = f.data();
    sp.comps.f_is_common = true;
    sp.comps.idx = idx.data();
    sp.comps.freqf = freqf.data();
    sp.phi = phi.data();
    sp.mask = mask.empty() ? nullptr : mask.data();
    sp.target = 0;
    sp.phi_hat = phi_hat.data();
    return sp;
  }
  bool ok(std::string& why) {
    return validate(P, offs, t.data(), nu.data(), sp, n_col, M.data(), nullptr, w.data(), n_g, G.data(), why);
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
  // what tm_host.h's and fit_host.h's validate refuse comes through with their messages
  { Case c; c.n_col = 17; CHECK(c.refused("n_col 17")); }
  { Case c; c.M[5 * 2 + 1] = nan; CHECK(c.refused("pulsar 2, TOA 2, column 1: not finite")); }
  for (double bad : {0.0, -1.0, nan, inf}) { Case c; c.w[4] = bad; CHECK(c.refused("pulsar 2, TOA 1: weight")); }
  { Case c; c.n_modes[1] = 0; CHECK(c.refused("component 1: 0 modes")); }
  { Case c; c.f[2] = -1e-8; CHECK(c.refused("component 1, mode 0: frequency is not positive and finite")); }
  { Case c; c.idx[1] = nan; CHECK(c.refused("component 1: chromatic index")); }
  { Case c; c.freqf[1] = 0.0; CHECK(c.refused("component 1: reference frequency")); }
  { Case c; c.nu[5] = 0.0; CHECK(c.refused("pulsar 2, TOA 2: radio frequency is not positive and finite, and component 1")); }
  { Case c; c.t[1] = inf; CHECK(c.refused("pulsar 0, TOA 1: epoch")); }
  // the component list with this file's limits
  { Case c; c.sp.comps.n_comp = 0; CHECK(c.refused("0 components outside [1, 8]")); }
  { Case c; c.n_modes.assign(9, 1); c.f.assign(9, 1e-8); c.idx.assign(9, 0.0); c.freqf.assign(9, 1400.0);
    c.phi.assign(3 * 9, 1.0); c.phi_hat = {1.0}; c.spec(); CHECK(c.refused("9 components outside [1, 8]")); }
  { Case c; c.n_modes = {2, 511}; c.f.assign(513, 1e-8); c.phi.assign(3 * 513, 1.0); c.spec();
    CHECK(c.refused("1026 Fourier columns, more than 1024")); }
  { Case c; c.n_modes = {2, 510}; c.f.assign(512, 1e-8); c.phi.assign(3 * 512, 1.0); c.spec(); CHECK(c.ok(why)); }
  { Case c; c.n_modes = {257, 1}; c.f.assign(258, 1e-8); c.phi.assign(3 * 258, 1.0); c.phi_hat.assign(257, 1.0); c.spec();
    CHECK(c.refused("target component 0: 514 Fourier columns, more than 512")); }
  { Case c; c.n_modes = {256, 1}; c.f.assign(257, 1e-8); c.phi.assign(3 * 257, 1.0); c.phi_hat.assign(256, 1.0); c.spec();
    CHECK(c.ok(why)); }
  for (int32_t bad : {-1, 2}) { Case c; c.sp.target = bad; CHECK(c.refused("target component")); }
  // the prior variances, the template, the pair weights
  for (double bad : {-1e-3, nan, inf}) {
    Case c; c.phi[2 * 3 + 2] = bad; CHECK(c.refused("pulsar 2, component 1, mode 0: prior variance is negative or not finite"));
  }
  { Case c; c.phi[1 * 3 + 1] = 0.0; CHECK(c.ok(why)); }  // a mode left out of the model
  for (double bad : {0.0, -1.0, nan, inf}) {
    Case c; c.phi_hat[1] = bad; CHECK(c.refused("target mode 1: template is not positive and finite"));
  }
  { Case c; c.G[9 + 2 * 3 + 1] = nan; CHECK(c.refused("pair-weight matrix 1, pair (1, 2): not finite")); }
  { Case c; c.G[0 * 3 + 2] = 0.5; CHECK(c.refused("pair-weight matrix 0, pair (0, 2): not symmetric")); }
  { Case c; c.G[4] = nan; CHECK(c.ok(why)); }  // the diagonal is ignored
  { Case c; c.n_g = 0; CHECK(c.ok(why)); }
  // the plan of an array: a pulsar without TOAs has X = 0 (no rows) and Z = 0, so its pairs have N_ab = 0
  {
    Case c;
    Plan plan;
    CHECK(make_plan(c.P, c.offs, c.t.data(), c.nu.data(), c.sp, c.n_col, c.M.data(), nullptr, c.w.data(), 0.0, c.n_g,
                    c.G.data(), plan, why) == 0);
    CHECK(plan.K == 4 && plan.N == 2 && plan.B.size() == 4 * 7 && plan.Z.size() == 3 * 16 && plan.Nab.size() == 9);
    CHECK(plan.rows[0] == 4 && plan.rows[1] == 0 && plan.rows[2] == 4 && plan.max_rows == 4);
    CHECK(plan.rank[0] == 2 && plan.rank[1] == 0 && plan.rank[2] == 2);
    for (int i = 0; i < 16; ++i) CHECK(plan.Z[16 + i] == 0.0);
    CHECK(plan.Nab[0 * 3 + 1] == 0.0 && plan.Nab[1 * 3 + 2] == 0.0 && plan.Nab[2 * 3 + 0] > 0.0);
    CHECK(plan.Nab[2 * 3 + 0] == plan.Nab[0 * 3 + 2] && plan.Nab[0] == 0.0 && plan.Nab[4] == 0.0 && plan.Nab[8] == 0.0);
    c.w[2] = 0.0;
    CHECK(make_plan(c.P, c.offs, c.t.data(), c.nu.data(), c.sp, c.n_col, c.M.data(), nullptr, c.w.data(), 0.0, c.n_g,
                    c.G.data(), plan, why) == 1 && why.find("weight") != std::string::npos);
  }
  // a zero nuisance column and a repeated one are dropped (not marginalised); the Fourier columns never drop, even a
  // repeated frequency; a target mode with phi = 0 still has a row of B
  {
    const int64_t n = 40;
    std::vector<double> t(n), nu(n, 1400.0), M(n * 3), f = {1e-8, 2.5e-8, 1e-8}, phi = {1e-3, 0.0, 1e-3};
    for (int64_t i = 0; i < n; ++i) {
      t[i] = 2.3e6 * i + 4e4 * (i % 7);
      M[3 * i] = 0.0;
      M[3 * i + 1] = 1.0;
      M[3 * i + 2] = 2.0;
    }
    const int32_t nm[1] = {3};
    const double idx[1] = {0.0}, ff[1] = {1400.0}, ph[3] = {1.0, 1.0, 1.0};
    Spec sp;
    sp.comps.n_comp = 1; sp.comps.n_modes = nm; sp.comps.f = f.data(); sp.comps.idx = idx; sp.comps.freqf = ff;
    sp.phi = phi.data(); sp.target = 0; sp.phi_hat = ph;
    std::vector<double> B(6 * n, -1.0), Z(36, -1.0);
    long double norms[3];
    CHECK(build_operator(n, t.data(), nu.data(), 3, M.data(), 3, nullptr, sp, f.data(), phi.data(), nullptr, 0, 0.0,
                         B.data(), Z.data(), norms) == 1);
    CHECK(norms[0] == 0.0L && norms[1] > 0.99L && norms[2] < 1e-15L);
    bool any = false;
    for (int64_t s = 0; s < n; ++s) any = any || B[1 * n + s] != 0.0;
    CHECK(any);                                  // phi = 0: the projection form
    for (int j = 0; j < 6; ++j) CHECK(Z[j * 6 + j] > 0.0);
    // the offset is marginalised: every row of B sums to zero against it
    for (int j = 0; j < 6; ++j) {
      long double s = 0.0L, a = 0.0L;
      for (int64_t i = 0; i < n; ++i) { s += B[j * n + i]; a += std::fabs(B[j * n + i]); }
      CHECK(std::fabs((double)s) <= 1e-13 * (double)a);
    }
  }
  std::printf("%s\n", fails ? "failed" : "all ok");
  return fails ? 1 : 0;
}
template <class V>
static bool rd(std::FILE* in, V& v) { return std::fread(v.data(), sizeof(v[0]), v.size(), in) == v.size(); }
int main(int argc, char** argv) {
  if (argc < 3) return self_checks();
  std::FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  std::vector<int64_t> hdr(8);
  if (!rd(in, hdr)) return 2;
  const int64_t P = hdr[0], n_col = hdr[1], C = hdr[3], n_g = hdr[6];
  std::vector<int64_t> offs((size_t)P + 1), ncol64((size_t)P), nm64((size_t)C);
  if (!rd(in, offs) || !rd(in, ncol64) || !rd(in, nm64)) return 2;
  std::vector<int32_t> ncol(ncol64.begin(), ncol64.end()), nm(nm64.begin(), nm64.end());
  int64_t nf = 0;
  for (int64_t v : nm64) nf += v;
  const int64_t n = offs[(size_t)P], N = nm64[(size_t)hdr[4]], K = 2 * N;
  std::vector<double> idx((size_t)C), ff((size_t)C), f((size_t)((hdr[7] ? 1 : P) * nf)), phi((size_t)(P * nf)),
      phi_hat((size_t)N), t((size_t)n), nu((size_t)n), M((size_t)(n * n_col)), w((size_t)(hdr[2] ? n : 0)),
      G((size_t)(n_g * P * P));
  std::vector<uint8_t> mask((size_t)(hdr[5] ? C * n : 0));
  if (!rd(in, idx) || !rd(in, ff) || !rd(in, f) || !rd(in, phi) || !rd(in, phi_hat) || !rd(in, t) || !rd(in, nu) ||
      !rd(in, M) || !rd(in, w) || !rd(in, G) || !rd(in, mask))
    return 2;
  std::fclose(in);
  Spec sp;
  sp.comps.n_comp = (int32_t)C; sp.comps.n_modes = nm.data(); sp.comps.f = f.data(); sp.comps.f_is_common = hdr[7] != 0;
  sp.comps.idx = idx.data(); sp.comps.freqf = ff.data();
  sp.phi = phi.data(); sp.mask = hdr[5] ? mask.data() : nullptr; sp.target = (int32_t)hdr[4]; sp.phi_hat = phi_hat.data();
  Plan plan;
  std::string why;
  const int made = make_plan(P, offs.data(), t.data(), nu.data(), sp, n_col, M.data(), ncol.data(),
                             hdr[2] ? w.data() : nullptr, 0.0, (int32_t)n_g, G.data(), plan, why);
  if (made) { std::printf("make_plan: %d %s\n", made, why.c_str()); return 3; }
  if ((int64_t)plan.B.size() != K * n) return 4;
  std::vector<double> rank(plan.rank.begin(), plan.rank.end()), rows(plan.rows.begin(), plan.rows.end());
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  for (const std::vector<double>* v : {&plan.B, &plan.Z, &plan.Nab, &rank, &rows})
    std::fwrite(v->data(), sizeof(double), v->size(), out);
  std::fclose(out);
  return 0;
}
"""


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("os_host")
    (d / "main.cpp").write_text(_MAIN)
    exe = str(d / "os_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-pthread", "-I", CSRC, str(d / "main.cpp"), "-o", exe], check=True)
    return exe


def test_host_planner_under_the_sanitizers(host_exe):
    """Every validation message (what tm_host.h and fit_host.h refuse, C = 9, q = 1026 refused and 1024 accepted, K =
    514 refused and 512 accepted, the target index, phi, phi_hat, G not finite and not symmetric, the ignored
    diagonal), a pulsar without TOAs, a zero and a repeated nuisance column, a repeated frequency, phi = 0."""
    r = subprocess.run([host_exe], capture_output=True, text=True)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("all ok"), r.stdout[-6000:] + r.stderr[-4000:]


def _pulsar(rng, n, span=15 * YEAR):
    t = np.sort(rng.uniform(0.0, span, n))
    nu = T.three_band(rng, n)
    return t, nu, T.mmat(t, nu), 1 / rng.uniform(1e-7, 1e-6, n) ** 2


def _white_level(w):
    """The variance white noise alone gives a Fourier coefficient of these TOAs: 2 / sum(w)."""
    return 2.0 / np.sum(w)


def _spectrum(level, w, N, gamma=13 / 3):
    return level * _white_level(w) * np.arange(1, N + 1) ** -gamma


def arrays():
    """The arrays of the host tests, each a dict(psrs = [(t, nu, M, w)], comps = [(f [P, N_c] or [N_c], idx, freqf)],
    phis = [[P, N_c]], masks = None or [None or flags [n_toa]], target). The issue's shapes: 17 TOAs with N = 4 (beside
    a pulsar without TOAs and one whose design repeats a column), 33 with N = 9 (beside a pulsar with a masked
    system-noise component), 250 and 600 with N = 30 (a red process 1e4 x the white level, and one 1e-4 x it; a
    chromatic component)."""
    rng = np.random.default_rng(20261)
    span = 15 * YEAR
    out = {}

    def red(N):
        return np.arange(1, N + 1) / span

    # N = 4: 17 TOAs; no TOAs; 40 TOAs with a design whose fourth column repeats its second
    ps = [_pulsar(rng, 17), _pulsar(rng, 0), _pulsar(rng, 40)]
    t, nu, M, w = ps[2]
    M = M[:, :4].copy()
    M[:, 3] = 2.0 * M[:, 1]
    ps[0] = ps[0][:2] + (ps[0][2][:, :3],) + ps[0][3:]
    ps[2] = (t, nu, M, w)
    ps[1] = ps[1][:2] + (np.zeros((0, 3)), ps[1][3])
    f_rn = np.stack([np.arange(1, 5) / max(np.ptp(p[0]), 1.0) if len(p[0]) else red(4) for p in ps])
    out["N4"] = dict(psrs=ps, comps=[(f_rn, 0.0, 1400.0), (red(4), 0.0, 1400.0)],
                     phis=[np.stack([_spectrum(30.0, p[3], 4, 3.0) if len(p[0]) else np.ones(4) for p in ps]),
                           np.stack([_spectrum(3.0, ps[0][3], 4)] * 3)], masks=None, target=1)
    # N = 9: 33 TOAs; 60 TOAs. A system-noise component of 5 modes acts on a third of the second pulsar's TOAs and
    # on none of the first's; its second mode is left out of the first pulsar's model (phi = 0)
    ps = [_pulsar(rng, 33), _pulsar(rng, 60)]
    ps = [p[:2] + (p[2][:, :3],) + p[3:] for p in ps]
    mask = np.concatenate([np.zeros(33, dtype=np.uint8), (rng.uniform(size=60) < 1 / 3).astype(np.uint8)])
    phi_sys = np.stack([_spectrum(10.0, p[3], 5, 2.0) for p in ps])
    phi_sys[0, 1] = 0.0
    phi_gw = np.stack([_spectrum(5.0, ps[1][3], 9)] * 2)
    phi_gw[0, 7] = 0.0  # a target mode left out of one pulsar's model
    out["N9"] = dict(psrs=ps, comps=[(red(9), 0.0, 1400.0), (red(5), 0.0, 1400.0), (red(9), 0.0, 1400.0)],
                     phis=[np.stack([_spectrum(100.0, p[3], 9, 4.0) for p in ps]), phi_sys, phi_gw],
                     masks=[None, mask, None], target=2)
    # N = 30: 250 TOAs under a red process 1e4 x the white level; 600 TOAs under one 1e-4 x it; a chromatic component
    ps = [_pulsar(rng, 250), _pulsar(rng, 600)]
    out["N30"] = dict(psrs=ps, comps=[(red(30), 0.0, 1400.0), (red(12), 2.0, 1400.0), (red(30), 0.0, 1400.0)],
                      phis=[np.stack([_spectrum(1e4, ps[0][3], 30, 3.0), _spectrum(1e-4, ps[1][3], 30, 3.0)]),
                            np.stack([_spectrum(3.0, p[3], 12, 2.0) for p in ps]),
                            np.stack([_spectrum(10.0, ps[1][3], 30)] * 2)], masks=None, target=2)
    return out


def array_tables(arr):
    """(offs, toas, nu, Mmats, weights, comps_of(p), phis_of(p), masks_of(p)) of one of arrays()."""
    ps = arr["psrs"]
    offs = np.concatenate([[0], np.cumsum([len(p[0]) for p in ps])]).astype(np.int64)

    def comps_of(p):
        return [(np.asarray(f)[p] if np.ndim(f) == 2 else np.asarray(f), idx, ff) for f, idx, ff in arr["comps"]]

    def phis_of(p):
        return [np.asarray(ph)[p] for ph in arr["phis"]]

    def masks_of(p):
        if arr["masks"] is None:
            return None
        return [None if m is None else m[offs[p]:offs[p + 1]] for m in arr["masks"]]

    return (offs, np.concatenate([p[0] for p in ps]), np.concatenate([p[1] for p in ps]), [p[2] for p in ps],
            np.concatenate([p[3] for p in ps]), comps_of, phis_of, masks_of)


_TRUTH = {}


def truth_of(name):
    """Per pulsar (B, Z, norms, keep) of the longdouble definition, computed once per array and shared."""
    if name not in _TRUTH:
        arr = arrays()[name]
        offs, toas, nu, Mmats, w, comps_of, phis_of, masks_of = array_tables(arr)
        per = []
        for p in range(len(offs) - 1):
            sl = slice(int(offs[p]), int(offs[p + 1]))
            B, Z, norms, keep = OS.operator_ld(toas[sl], nu[sl], Mmats[p], w[sl], comps_of(p), phis_of(p),
                                               arr["target"], masks_of(p))
            T.assert_clear_rank(norms, keep, Mmats[p])
            per.append((B, Z, norms, keep))
        _TRUTH[name] = per
    return _TRUTH[name]


def run_host(host_exe, tmp_path, arr, G):
    offs, toas, nu, Mmats, w, _, _, _ = array_tables(arr)
    P, n = len(offs) - 1, int(offs[-1])
    n_col = max(M.shape[1] for M in Mmats)
    Mfull = np.zeros((n, n_col))
    for p, M in enumerate(Mmats):
        Mfull[offs[p]:offs[p + 1], :M.shape[1]] = M
    common = all(np.ndim(c[0]) == 1 for c in arr["comps"])
    fs = [np.asarray(c[0]) if common or np.ndim(c[0]) == 2 else np.tile(c[0], (P, 1)) for c in arr["comps"]]
    n_modes = [f.shape[-1] for f in fs]
    N = n_modes[arr["target"]]
    phi_hat = np.asarray(arr["phis"][arr["target"]])[-1]
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.array([P, n_col, 1, len(fs), arr["target"], 0 if arr["masks"] is None else 1, len(G),
                           1 if common else 0] + list(offs) + [M.shape[1] for M in Mmats] + n_modes,
                          dtype=np.int64).tobytes())
        for a in ([c[1] for c in arr["comps"]], [c[2] for c in arr["comps"]], np.concatenate(fs, axis=-1),
                  np.concatenate(arr["phis"], axis=-1), phi_hat, toas, nu, Mfull, w, G):
            fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        if arr["masks"] is not None:
            fh.write(np.stack([np.ones(n, dtype=np.uint8) if m is None else m for m in arr["masks"]]).tobytes())
    r = subprocess.run([host_exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    body = np.frombuffer(open(tmp_path / "out.bin", "rb").read(), dtype=np.float64)
    K = 2 * N
    o = [0, K * n, K * n + P * K * K, K * n + P * K * K + P * P, K * n + P * K * K + P * P + P]
    B = [body[K * offs[p]:K * offs[p + 1]].reshape(K, -1) for p in range(P)]
    return (B, body[o[1]:o[2]].reshape(P, K, K), body[o[2]:o[3]].reshape(P, P), body[o[3]:o[4]].astype(int),
            body[o[4]:o[4] + P].astype(int), phi_hat)


# |B - B_truth| per entry in eps of the row's largest entry, the largest over a pulsar's rows, as measured: N4 0.433 /
# no TOAs / 0.339, N9 0.484 / 0.474, N30 0.474 / 0.485 (the rounding to fp64 is the whole error). The bound: 4 x the
# largest of them, floor 1 eps.
B_MEASURED_EPS = 0.485
B_BOUND_EPS = max(4 * B_MEASURED_EPS, 1.0)


@pytest.mark.parametrize("name", ["N4", "N9", "N30"])
def test_operator_and_pair_norms_match_the_longdouble_definition(host_exe, tmp_path, name):
    """B_p to <= 1.94 eps per entry relative to its row's largest entry (4 x the 0.485 eps measured), Z_p to the dot-product
    bound (n + 2) eps sum_t |B_kt| |F_tj|, the kept columns of M, N_ab to (K^2 + 3) eps sum |terms|; a pulsar without
    TOAs has no rows, Z = 0 and N_ab = 0 with everyone."""
    arr = arrays()[name]
    offs, toas, nu, Mmats, w, comps_of, phis_of, masks_of = array_tables(arr)
    P = len(offs) - 1
    rng = np.random.default_rng(5)
    G = rng.normal(size=(2, P, P))
    G = G + G.transpose(0, 2, 1)
    B, Z, nab, rank, rows, phi_hat = run_host(host_exe, tmp_path, arr, G)
    per = truth_of(name)
    K = Z.shape[1]
    for p in range(P):
        Bt, Zt, norms, keep = per[p]
        n = Bt.shape[1]
        assert rank[p] == int(keep.sum()) and rows[p] == (K if n else 0)
        if n == 0:
            assert np.all(Z[p] == 0)
            continue
        row_max = np.max(np.abs(Bt), axis=1, keepdims=True)
        assert np.all(row_max > 0)
        err = float(np.max(np.abs(B[p].astype(LD) - Bt) / row_max)) / EPS
        sl = slice(int(offs[p]), int(offs[p + 1]))
        lit = OS.operator_literal(toas[sl], nu[sl], Mmats[p], w[sl], comps_of(p), phis_of(p), arr["target"], keep,
                                  masks_of(p))
        # against the largest entry of B: on the 15-yr span mode 15 is 1 / yr, the annual columns of make_Mmat, and
        # its two rows of B are zero up to rounding (the column is marginalised), so a row-relative figure says nothing
        e_lit = float(np.max(np.abs(lit.astype(LD) - Bt)) / np.max(row_max))
        print(f"{name} pulsar {p} (n = {n}, kept {rank[p]} of {Mmats[p].shape[1]} design columns): |B - B_ld| <= "
              f"{err:.3f} eps of the row's largest entry; the literal fp64 Woodbury form is off by {e_lit:.3g} of the "
              f"largest entry of B")
        assert err <= B_BOUND_EPS
        # the truth is the definition, not a copy of the planner: B M = 0 and B P0 = F^T up to the span of M^T, in
        # longdouble products without an inverse (the fp64 literal form cancels when a red process dominates). A wrong
        # formula gives O(1); longdouble rounding through these condition numbers stays far below 1e-9
        bm, dres = OS.definition_residual(toas[sl], nu[sl], Mmats[p], w[sl], comps_of(p), phis_of(p), arr["target"],
                                          keep, Bt, masks_of(p))
        print(f"{name} pulsar {p}: the truth's |B M| <= {bm:.3g} |B|, |B P0 - F^T| off the span of M <= {dres:.3g}")
        assert bm <= 1e-9 and dres <= 1e-9
        tgt = comps_of(p)[arr["target"]]
        mk = None if masks_of(p) is None else masks_of(p)[arr["target"]]
        F = np.stack([OS.column_ld(toas[sl], nu[sl], tgt[0], tgt[1], tgt[2], k, K // 2, mk) for k in range(K)], axis=1)
        zb = (n + 2) * EPS * (np.abs(Bt) @ np.abs(F)).astype(np.float64)
        assert np.all(np.abs(Z[p].astype(LD) - Zt) <= zb), float(np.max(np.abs(Z[p].astype(LD) - Zt) / zb))
    nab_t, mag = OS.pair_norms([q[1] for q in per], phi_hat)
    tol = (K * K + 3) * EPS * mag.astype(np.float64)
    assert np.all(np.abs(nab.astype(LD) - nab_t) <= tol)
    assert np.all(nab == nab.T) and np.all(np.diag(nab) == 0)
    for p in range(P):
        if per[p][0].shape[1] == 0:
            assert np.all(nab[p] == 0)
        else:
            others = [q for q in range(P) if q != p and per[q][0].shape[1]]
            assert np.all(nab[p, others] > 0)


def test_abi_declares_exports_and_binds_the_entry_points():
    from fakepta_amd import _capi
    text = open(HEADER).read()
    lib = ctypes.CDLL(LIB)
    for name in ENTRY_POINTS:
        assert re.search(rf"^int\s+{name}\s*\(", text, flags=re.M), name
        assert hasattr(lib, name) and name in _capi.EXPORTED
    assert re.search(r"^#define\s+FPTA_VERSION\s+10300\b", text, flags=re.M)
    for method in ("batch_set_os", "batch_os_info", "batch_os", "os_statistic"):
        assert hasattr(_capi.Context, method)
    host = open(os.path.join(CSRC, "os_host.h")).read()
    assert "#include <hip" not in host and "__global__" not in host and "__device__" not in host  # plain C++
    assert '#include "fit_host.h"' in host and "fpta_fit::validate" in host and "fpta_tm::rcond_of" in host  # shared
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "os.hip" in make and "os_host.h" in make
    dev = open(os.path.join(CSRC, "os.hip")).read()
    assert "k_fit_apply<" not in dev and "fit_launch_unbooked" in dev  # the fit's kernel is launched, not forked


class _RecordingCtx:
    """Stands in for a device context: records the calls a BatchSimulator makes."""

    def __init__(self, P):
        self.calls, self.P = [], P

    def __getattr__(self, name):
        def call(*a, **k):
            self.calls.append((name, a, k))
            if name == "batch_set_os":
                return np.full(self.P, 3, dtype=np.int32), np.ones((self.P, self.P)) - np.eye(self.P)
            if name == "batch_os":
                J = len(self.calls_of("batch_set_os")[-1][1][7])
                return np.ones((J, 4)), (np.ones((J, 3, 4)) if k.get("per_mode") else None), None
        return call

    def calls_of(self, name):
        return [c for c in self.calls if c[0] == name]


class _Psr:
    def __init__(self, n, pos, m=3, t1=1e8):
        self.toas = np.linspace(0.0, t1, n)
        self.freqs = np.full(n, 1400.0)
        self.Mmat = np.vander(self.toas / 1e8, m)
        self.signal_model = {}
        self.s2 = np.linspace(1.0, 2.0, n)
        self.pos = np.asarray(pos, dtype=float) / np.linalg.norm(pos)

    def _white_sigma2(self):
        return self.s2


def test_set_optimal_statistic_argument_checks_need_no_device():
    from fakepta_amd.batch import BatchSimulator
    psrs = [_Psr(5, [1, 0, 0]), _Psr(7, [0.3, 1, 0], t1=2e8), _Psr(6, [0.2, 0.1, 1])]  # pairs at 73, 79 and 81 degrees
    ctx = _RecordingCtx(len(psrs))
    sim = BatchSimulator(psrs, signals=[], white=False, ctx=ctx)
    with pytest.raises(ValueError, match="no optimal statistic"):
        sim.optimal_statistic()
    with pytest.raises(ValueError, match="0 common signals"):
        sim.set_optimal_statistic()  # an empty layout
    f2 = np.array([[1e-8, 2e-8]] * 3)
    sim.segments.append(dict(name="red_noise", kind=0, f=f2, amp=np.full((3, 2), 1e-7), idx=0.0, freqf=1400.0,
                             mask=None))
    with pytest.raises(ValueError, match="0 common signals"):
        sim.set_optimal_statistic()
    fc = np.array([1e-8, 2e-8, 3e-8])
    sim.segments.append(dict(name="gw_common", kind=1, f=fc, amp=np.array([3e-7, 2e-7, 1e-7]), idx=0.0, freqf=1400.0,
                             mask=None))
    sim.segments.append(dict(name="other_common", kind=1, f=fc, amp=np.array([1e-7, 1e-7, 1e-7]), idx=0.0,
                             freqf=1400.0, mask=None))
    n0 = len(ctx.calls)
    with pytest.raises(ValueError, match="2 common signals"):
        sim.set_optimal_statistic()
    with pytest.raises(KeyError, match="dm_gp"):
        sim.set_optimal_statistic(target="dm_gp")
    for bad in (dict(orfs=["quadrupole"]), dict(orfs=[np.ones((2, 2))]), dict(orfs=[np.triu(np.ones((3, 3)))]),
                dict(orfs=[np.full((3, 3), np.nan)]), dict(orfs=[]), dict(bins=0), dict(template=[1.0, 2.0]),
                dict(template=[1.0, 0.0, 1.0]), dict(template=[1.0, np.inf, 1.0]), dict(Mmats="design"),
                dict(Mmats=[psrs[0].Mmat]), dict(Mmats=[p.Mmat[:-1] for p in psrs]), dict(weights="ecorr"),
                dict(noise="model"), dict(target=7), dict(target=1.5)):
        with pytest.raises(ValueError):
            sim.set_optimal_statistic(**{"target": "gw_common", **bad})
    assert len(ctx.calls) == n0  # refused before anything reached the context
    # the layout's model: per-pulsar grids for every component, phi = amp^2, the target's template its own amp^2
    rank, nab = sim.set_optimal_statistic(target="gw_common", orfs=("hd", "monopole"), bins=4)
    name, a, k = ctx.calls[-1]
    assert name == "batch_set_os" and list(a[0]) == [2, 3, 3] and a[1].shape == (3, 8) and a[4].shape == (3, 8)
    gw2 = np.array([3e-7, 2e-7, 1e-7]) ** 2
    np.testing.assert_array_equal(a[4][1], np.concatenate([np.full(2, 1e-7) ** 2, gw2, np.full(3, 1e-7) ** 2]))
    assert a[5] == 1 and list(a[6]) == list(gw2) and a[7].shape == (6, 3, 3)
    assert k["M"].shape == (18, 3) and list(k["ncol_psr"]) == [3, 3, 3] and k["weights"].shape == (18,)
    assert np.all(a[7][:, range(3), range(3)] == 0) and np.all(a[7] == a[7].transpose(0, 2, 1))
    np.testing.assert_array_equal(a[7][1], np.ones((3, 3)) - np.eye(3))
    np.testing.assert_array_equal(a[7][2:].sum(axis=0), np.ones((3, 3)) - np.eye(3))  # every pair in one bin
    out = sim.optimal_statistic(per_mode=True)
    assert out["A2"].shape == (2, 4) and out["snr"].shape == (2, 4) and out["A2_joint"].shape == (2, 4)
    assert out["rho_bins"].shape == (4, 4) and out["Q_mode"].shape == (6, 3, 4) and out["norm"].shape == (6,)
    assert list(out["bin_counts"]) == [0, 3, 0, 0] and np.all(np.isnan(out["rho_bins"][0]))
    sim.set_optimal_statistic(target=2, Mmats=None, weights=None, template=[1.0, 2.0, 3.0])
    name, a, k = ctx.calls_of("batch_set_os")[-1]
    assert a[5] == 2 and list(a[6]) == [1.0, 2.0, 3.0] and k["M"].shape == (18, 0) and k["weights"] is None
    assert "A2_joint" not in sim.optimal_statistic()


def test_host_algebra_on_numbers_built_by_hand():
    from fakepta_amd import os as osm
    pos = np.array([[1.0, 0, 0], [0, 1.0, 0], [-1.0, 0, 0], [0, 0, 1.0]])
    G, centres, counts = osm.angular_bins(pos, 4)
    # pairs at 90 degrees sit exactly on an edge of 4 bins: open bins leave them out, as hd_curve does
    assert list(counts) == [0, 0, 0, 0]
    G, centres, counts = osm.angular_bins(pos, 3)
    assert list(counts) == [0, 5, 0] and np.allclose(centres, [np.pi / 6, np.pi / 2, 5 * np.pi / 6])
    with pytest.raises(ValueError):
        osm.angular_bins(pos[:, :2], 3)
    nab = np.array([[0, 2.0, 3.0], [2.0, 0, 5.0], [3.0, 5.0, 0]])
    g1 = np.array([[0, 1.0, 2.0], [1.0, 0, -1.0], [2.0, -1.0, 0]])
    g2 = np.array([[0, 1.0, 0], [1.0, 0, 0], [0, 0, 0]])
    Gs = np.stack([g1, np.ones((3, 3)) - np.eye(3), g2])
    np.testing.assert_allclose(osm.norms(Gs, nab), [2 + 12 + 5, 10, 2], rtol=1e-15)
    C = osm.joint_matrix(Gs[:2], nab)
    np.testing.assert_allclose(C, [[19, 2 + 6 - 5], [3, 10]], rtol=1e-15)
    # Q made from known amplitudes comes back through the joint solve
    A = np.array([[2.0, -1.0], [0.5, 3.0]])  # [orf, realization]
    Q = np.concatenate([C @ A, [[4.0, 0.0]]])
    out = osm.derive(Q, Gs, nab, 2, np.array([0.5]), np.array([1]))
    np.testing.assert_allclose(out["A2_joint"], A, rtol=1e-14)
    np.testing.assert_allclose(out["A2"], Q[:2] / np.array([[19.0], [10.0]]), rtol=1e-15)
    np.testing.assert_allclose(out["snr"], Q[:2] / np.sqrt([[19.0], [10.0]]), rtol=1e-15)
    np.testing.assert_allclose(out["rho_bins"], [[2.0, 0.0]], rtol=1e-15)
    # a pair-weight matrix whose pairs all have N_ab = 0 carries no weight: NaN, not a division error
    out = osm.derive(np.ones((1, 2)), np.stack([g2]), np.zeros((3, 3)), 1)
    assert np.all(np.isnan(out["A2"])) and np.all(np.isnan(out["snr"]))
    for bad, msg in ((np.ones((2, 2)), "must be"), (np.triu(np.ones((3, 3))), "not symmetric"),
                     (np.full((3, 3), np.inf), "not finite")):
        with pytest.raises(ValueError, match=msg):
            osm.check_pair_matrices(bad, 3)
    with pytest.raises(ValueError, match="components"):
        osm.noise_model([dict(f=np.ones(2), amp=np.ones(2))] * 9, 2)
    with pytest.raises(ValueError, match="Fourier columns"):
        osm.noise_model([dict(f=np.ones(300), amp=np.ones(300))] * 2, 2)
    with pytest.raises(ValueError, match="f and amp"):
        osm.noise_model([dict(f=np.ones(3), amp=np.ones(2))], 2)


def test_fake_pta_imports_the_drop_in_and_the_package_still_finds_the_standard_os_module():
    code = ("import os, fakepta_amd, fakepta_amd.os as m; from fakepta import fake_pta as fp; "
            "assert callable(fp.optimal_statistic_array) and hasattr(os, 'path') and not hasattr(m, 'path'); "
            "print(m.MAX_COMP, m.MAX_COL, m.MAX_COEF)")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "8 1024 512", r.stderr


# ----------------------------------------------------------------------------- unbiasedness of the definition
UNBIASED_SEED, UNBIASED_R = 4, 2048  # of the seeds 1 .. 5 tried, 4 leaves most room on both (0.02 and -0.62 standard errors)


def unbiased_layout(identity=False):
    """8 pulsars of 64 .. 128 TOAs (ragged), a red process of 5 modes each, an HD-correlated common process of 5 modes
    (identity=True: the same spectrum with the identity as its factor, i.e. uncorrelated), white noise and a design of
    3 columns. Returns dict(offs, toas, nu, Mmats, sigma, pos, segs (oracle Segments), comps_of, phis_of, f_gw, amp_gw,
    f_rn, amp_rn, L)."""
    from oracle import fakepta_oracle as O
    rng = np.random.default_rng(77)
    P = 8
    n_p = [64, 71, 80, 97, 100, 113, 127, 128]
    span = 10 * YEAR
    toas = [np.sort(rng.uniform(0.0, span, n)) for n in n_p]
    offs = np.concatenate([[0], np.cumsum(n_p)]).astype(np.int64)
    nu = np.concatenate([T.three_band(rng, n) for n in n_p])
    sigma = np.concatenate([rng.uniform(2e-7, 6e-7, n) for n in n_p])
    # within 1.2 rad of the pole: no pair is further apart than 2.4 rad, so the last of 5 angular bins is empty
    # (the first two pulsars sit 2.4 rad apart, so the fourth is not)
    th, az = rng.uniform(0.1, 1.2, P), rng.uniform(0.0, 2 * np.pi, P)
    th[:2], az[:2] = 1.2, (0.0, np.pi)
    pos = np.stack([np.sin(th) * np.cos(az), np.sin(th) * np.sin(az), np.cos(th)], axis=1)
    f_gw = np.arange(1, 6) / span
    amp_gw = np.sqrt(O.powerlaw(f_gw, -13.6, 13 / 3) * O.delta_f(f_gw))
    f_rn = np.stack([np.arange(1, 6) / np.ptp(t) for t in toas])
    amp_rn = np.sqrt(O.powerlaw(f_rn, -13.3, 3.0) * np.diff(np.concatenate([np.zeros((P, 1)), f_rn], 1), axis=1))
    L = np.eye(P) if identity else O.mvn_factor(O.orf_hd(pos))
    segs = [O.Segment(0, 2 * np.pi * f_rn, amp_rn, 0.0), O.Segment(1, 2 * np.pi * f_gw, amp_gw, 0.0, L=L)]
    Mmats = [np.stack([np.ones(len(t)), t / span, (t / span) ** 2], axis=1) for t in toas]
    return dict(offs=offs, toas=np.concatenate(toas), nu=nu, Mmats=Mmats, sigma=sigma, pos=pos, segs=segs, f_gw=f_gw,
                amp_gw=amp_gw, f_rn=f_rn, amp_rn=amp_rn, L=L,
                comps_of=lambda p: [(f_rn[p], 0.0, 1400.0), (f_gw, 0.0, 1400.0)],
                phis_of=lambda p: [amp_rn[p] ** 2, amp_gw ** 2])


_UNBIASED = {}


def unbiased_truth():
    """Per pulsar the truth's (B, Z) of unbiased_layout() (the operator does not depend on the common factor) and N_ab."""
    if not _UNBIASED:
        lay = unbiased_layout()
        per = []
        for p in range(len(lay["offs"]) - 1):
            sl = slice(int(lay["offs"][p]), int(lay["offs"][p + 1]))
            B, Z, norms, keep = OS.operator_ld(lay["toas"][sl], lay["nu"][sl], lay["Mmats"][p],
                                               1 / lay["sigma"][sl] ** 2, lay["comps_of"](p), lay["phis_of"](p), 1)
            T.assert_clear_rank(norms, keep, lay["Mmats"][p])
            per.append((B, Z))
        _UNBIASED["per"] = per
        _UNBIASED["nab"] = OS.pair_norms([q[1] for q in per], lay["amp_gw"] ** 2)[0]
    return _UNBIASED["per"], _UNBIASED["nab"]


def a2_truth(lay, res):
    """A2 [R] of the HD ORF for residuals res [R, n_toa], from the truth alone."""
    from oracle import fakepta_oracle as O
    per, nab = unbiased_truth()
    X, _ = OS.x_truth([q[0] for q in per], lay["offs"], res)
    G = O.orf_hd(lay["pos"])
    np.fill_diagonal(G, 0.0)
    Qm, _, _ = OS.q_truth(X.astype(np.float64), lay["amp_gw"] ** 2, G[None])
    il = np.tril_indices(len(G), -1)
    return (Qm.sum(axis=1)[0] / np.sum(G[il].astype(LD) ** 2 * nab[il])).astype(np.float64)


@pytest.mark.parametrize("identity", [False, True])
def test_the_definition_is_unbiased(identity):
    """R = 2048 realizations of the small array by the oracle's batch semantics: the mean of A2 (HD ORF, the template
    the injected spectrum) is 1 within 5 standard errors, and 0 when the common process is uncorrelated. With this seed
    the truth is 0.02 and -0.62 standard errors away (seeds 1 .. 5: |z| <= 1.5 throughout)."""
    from oracle import fakepta_oracle as O
    lay = unbiased_layout(identity)
    res = O.batch_synth(lay["offs"], lay["toas"], lay["nu"], lay["segs"], UNBIASED_SEED, 0, UNBIASED_R,
                        sigma=lay["sigma"])
    a2 = a2_truth(lay, res)
    want = 0.0 if identity else 1.0
    se = np.std(a2) / np.sqrt(UNBIASED_R)
    print(f"identity={identity}: mean A2 = {np.mean(a2):.4f}, std = {np.std(a2):.4f}, "
          f"(mean - {want}) / standard error = {(np.mean(a2) - want) / se:.2f}")
    assert abs(np.mean(a2) - want) <= 5 * se
