"""Correlated likelihood grid, host side (no GPU): csrc/clnl_host.h (validation, the coupled matrix T per ORF factor in
long double, the scalings s) in a stand-alone C++ program built with the address and undefined-behaviour sanitizers,
against the np.longdouble definition of tests/clnl_reference.py; the definition's two forms against each other, against
tests/lnl_reference.py for Gamma = I and for a zero grid row; the C-ABI surface; the host algebra of fakepta_amd.clnl; a
statement of the definition on oracle realizations (its GPU half is in tests/test_gpu_clnl.py)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import clnl_reference as CR
from tests import lnl_reference as LR
from tests import os_reference as OS
from tests import test_os_host as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fakepta_amd.h")
LIB = os.path.join(ROOT, "fakepta_amd", "lib", "libfakepta_amd.so")
CSRC = os.path.join(ROOT, "fakepta_amd", "csrc")
ENTRY_POINTS = ("fpta_batch_set_clnl", "fpta_batch_clnl_info", "fpta_batch_clnl", "fpta_clnl_grid")
EPS = np.finfo(np.float64).eps
LD = np.longdouble

# argv: in out. in: int64 P, n_col, C, target, has_mask, f_common, G, n_orf; offs [P + 1]; ncol [P]; n_modes [C]; then
# fp64 idx [C], freqf [C], f [rows][sum N], phi [P][sum N], grid [G][N], A [n_orf][P][P], t [n], nu [n], M [n][n_col], w
# [n]; then uint8 mask [C][n] (has_mask). out: fp64 T [n_orf][n][n], s [G][n], B [K n_toa], rank [P], rows [P]. Without
# arguments: the checks that need no data.
_MAIN = r"""
#include <cstdio>
#include <cstring>
#include <limits>
#include "clnl_host.h"
using namespace fpta_clnl;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)
struct Case {
  int64_t P = 3;
  std::vector<int64_t> offs{0, 3, 3, 7};  // the middle pulsar has no TOAs
  std::vector<double> t, nu, M, w, f, idx, freqf, phi, grid, A;
  std::vector<int32_t> n_modes;
  int64_t n_col = 2, G = 2, n_orf = 1;
  bool null_A = false;
  Spec sp;
  Case() : t(7), nu(7, 1400.0), M(7 * 2, 1.0), w(7, 2.0), f{1e-8, 2e-8, 3e-8}, idx{0.0, 2.0}, freqf{1400.0, 1400.0},
           phi(3 * 3, 1e-2), grid{1.0, 0.5, 0.0, 0.0}, A{1, 0, 0, 0, 1, 0, 0, 0, 1}, n_modes{2, 1} {
    for (int i = 0; i < 7; ++i) {
      t[i] = 1e7 * (i + 1) + 3e5 * i * i;
      M[2 * i + 1] = (double)i;
    }
    spec();
  }
  // P pulsars of which only the first has TOAs, a target of N modes alone in the model
  void wide(int64_t P_, int32_t N) {
    P = P_;
    offs.assign((size_t)P + 1, 7);
    offs[0] = 0;
    n_modes = {N};
    f.assign((size_t)N, 1e-8);
    idx = {0.0};
    freqf = {1400.0};
    phi.assign((size_t)(P * N), 1.0);
    grid.assign((size_t)(G * N), 1.0);
    A.assign((size_t)(P * P), 0.0);
    for (int64_t p = 0; p < P; ++p) A[(size_t)(p * P + p)] = 1.0;
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
    sp.mask = nullptr;
    sp.target = 0;
    return sp;
  }
  bool ok(std::string& why) {
    return validate(P, offs.data(), t.data(), nu.data(), sp, n_col, M.data(), nullptr, w.data(), G, grid.data(), n_orf,
                    null_A ? nullptr : A.data(), why);
  }
  bool refused(const char* expect) {
    std::string why;
    const bool good = ok(why);
    std::printf("validate: %s\n", good ? "ok" : why.c_str());
    return !good && why.find(expect) != std::string::npos;
  }
  int plan(Plan& pl, std::string& why) {
    return make_plan(P, offs.data(), t.data(), nu.data(), sp, n_col, M.data(), nullptr, w.data(), 0.0, G, grid.data(),
                     n_orf, A.data(), pl, why);
  }
};
static int self_checks() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  std::string why;
  { Case c; CHECK(c.ok(why)); }
  // what lnl_host.h's validate refuses comes through with its messages
  { Case c; c.w[4] = 0.0; CHECK(c.refused("pulsar 2, TOA 1: weight")); }
  { Case c; c.grid[1 * 2 + 1] = -1.0; CHECK(c.refused("grid row 1, mode 1: prior variance is negative or not finite")); }
  { Case c; c.G = 0; CHECK(c.refused("0 grid points outside [1, 4096]")); }
  // a common grid
  { Case c; c.f = {1e-8, 2e-8, 3e-8, 1e-8, 2e-8, 4e-8, 1e-8, 2e-8, 5e-8}; c.sp.comps.f = c.f.data();
    c.sp.comps.f_is_common = false; CHECK(c.ok(why));  // per-pulsar rows, the target's the same
    c.f[2 * 3 + 1] = 2.5e-8; CHECK(c.refused("target component 0: pulsar 2, mode 1 has its own frequency")); }
  // the ORF factors
  { Case c; c.n_orf = 0; CHECK(c.refused("0 ORFs outside [1, 8]")); }
  { Case c; c.n_orf = 9; c.A.assign(9 * 9, 0.0); CHECK(c.refused("9 ORFs outside [1, 8]")); }
  { Case c; c.n_orf = 8; c.A.assign(8 * 9, 0.5); CHECK(c.ok(why)); }
  { Case c; c.null_A = true; CHECK(c.refused("ORF factors missing")); }
  for (double bad : {nan, inf, -inf}) {
    Case c; c.n_orf = 2; c.A.assign(2 * 9, 1.0); c.A[9 + 1 * 3 + 2] = bad;
    CHECK(c.refused("ORF 1, factor entry (1, 2) is not finite"));
  }
  // the size cap: n = P K <= 16384
  { Case c; c.wide(65, 128); CHECK(c.refused("n = P K = 16640 coefficients, more than 16384")); }
  { Case c; c.wide(64, 128); CHECK(c.ok(why)); }
  // the budget: n_orf G 8 n_pad^2 <= 32 GiB; 16 grid points of n = 16384 are 32 GiB exactly, 17 are 36507222016 bytes
  { Case c; c.G = 16; c.wide(64, 128); CHECK(c.ok(why)); }
  { Case c; c.G = 17; c.wide(64, 128); CHECK(c.refused("the cached factors need 36507222016 bytes")); }
  { Case c; c.G = 9; c.n_orf = 2; c.wide(64, 128); c.A.resize(2 * 64 * 64, 0.0);
    CHECK(c.refused("the cached factors need 38654705664 bytes (n_orf 2, G 9, n 16384)")); }
  // the plan of an array: n = 12 in one block of 64, the padding zero; with A = I the blocks of T off the diagonal are
  // zero, a pulsar without TOAs has a zero block, and T is symmetric bit for bit
  {
    Case c;
    Plan pl;
    CHECK(c.plan(pl, why) == 0);
    CHECK(pl.K == 4 && pl.N == 2 && pl.G == 2 && pl.n_orf == 1 && pl.n == 12 && pl.n_pad == 64);
    CHECK(pl.T.size() == 64 * 64 && pl.s.size() == 2 * 64 && pl.B.size() == 4 * 7 && pl.A.size() == 9);
    CHECK(pl.rows[0] == 4 && pl.rows[1] == 0 && pl.rows[2] == 4 && pl.max_rows == 4);
    CHECK(pl.rank[0] == 2 && pl.rank[1] == 0 && pl.rank[2] == 2);
    for (int i = 0; i < 64; ++i)
      for (int j = 0; j < 64; ++j) {
        const double v = pl.T[(size_t)(i * 64 + j)];
        CHECK(v == pl.T[(size_t)(j * 64 + i)]);
        if (i >= 12 || j >= 12 || i / 4 != j / 4 || i / 4 == 1) CHECK(v == 0.0);
      }
    CHECK(pl.T[0] > 0.0 && pl.T[8 * 64 + 8] > 0.0);
    for (int i = 0; i < 64; ++i) {
      const int k = i % 4;
      CHECK(pl.s[(size_t)i] == (i < 12 ? (k == 0 || k == 2 ? 1.0 : std::sqrt(0.5)) : 0.0));
      CHECK(pl.s[(size_t)(64 + i)] == 0.0);  // the zero grid row
    }
    // a singular factor (rank 1, the monopole's): every block of T is the sum of the pulsars' Z
    Case m;
    m.A = {1, 0, 0, 1, 0, 0, 1, 0, 0};
    Plan pm;
    CHECK(m.plan(pm, why) == 0);
    for (int k = 0; k < 4; ++k)
      for (int l = 0; l < 4; ++l) {
        const double sum = pm.T[(size_t)(k * 64 + l)];
        const double z0 = pl.T[(size_t)(k * 64 + l)], z2 = pl.T[(size_t)((8 + k) * 64 + 8 + l)];
        CHECK(std::fabs(sum - (z0 + z2)) <= 4e-16 * (std::fabs(z0) + std::fabs(z2)));
        for (int i = 0; i < 3; ++i)
          for (int j = 0; j < 3; ++j)
            CHECK(pm.T[(size_t)((4 * i + k) * 64 + 4 * j + l)] == (i == 0 && j == 0 ? sum : 0.0));
      }
    // a zero factor: T = 0
    Case z;
    z.A.assign(9, 0.0);
    Plan pz;
    CHECK(z.plan(pz, why) == 0);
    for (double v : pz.T) CHECK(v == 0.0);
    c.A[4] = nan;
    CHECK(c.plan(pl, why) == 1 && why.find("ORF 0, factor entry (1, 1)") != std::string::npos);
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
  const int64_t P = hdr[0], n_col = hdr[1], C = hdr[2], G = hdr[6], J = hdr[7];
  std::vector<int64_t> offs((size_t)P + 1), ncol64((size_t)P), nm64((size_t)C);
  if (!rd(in, offs) || !rd(in, ncol64) || !rd(in, nm64)) return 2;
  std::vector<int32_t> ncol(ncol64.begin(), ncol64.end()), nm(nm64.begin(), nm64.end());
  int64_t nf = 0;
  for (int64_t v : nm64) nf += v;
  const int64_t n = offs[(size_t)P], N = nm64[(size_t)hdr[3]], K = 2 * N;
  std::vector<double> idx((size_t)C), ff((size_t)C), f((size_t)((hdr[5] ? 1 : P) * nf)), phi((size_t)(P * nf)),
      grid((size_t)(G * N)), A((size_t)(J * P * P)), t((size_t)n), nu((size_t)n), M((size_t)(n * n_col)), w((size_t)n);
  std::vector<uint8_t> mask((size_t)(hdr[4] ? C * n : 0));
  if (!rd(in, idx) || !rd(in, ff) || !rd(in, f) || !rd(in, phi) || !rd(in, grid) || !rd(in, A) || !rd(in, t) ||
      !rd(in, nu) || !rd(in, M) || !rd(in, w) || !rd(in, mask))
    return 2;
  std::fclose(in);
  Spec sp;
  sp.comps.n_comp = (int32_t)C; sp.comps.n_modes = nm.data(); sp.comps.f = f.data(); sp.comps.f_is_common = hdr[5] != 0;
  sp.comps.idx = idx.data(); sp.comps.freqf = ff.data();
  sp.phi = phi.data(); sp.mask = hdr[4] ? mask.data() : nullptr; sp.target = (int32_t)hdr[3];
  Plan plan;
  std::string why;
  const int made = make_plan(P, offs.data(), t.data(), nu.data(), sp, n_col, M.data(), ncol.data(), w.data(), 0.0, G,
                             grid.data(), J, A.data(), plan, why);
  if (made) { std::printf("make_plan: %d %s\n", made, why.c_str()); return 3; }
  const int64_t nn = P * K, np_ = plan.n_pad;
  if (plan.n != nn || (int64_t)plan.T.size() != J * np_ * np_ || (int64_t)plan.s.size() != G * np_) return 4;
  for (int64_t o = 0; o < J; ++o)  // the padding is zero
    for (int64_t i = 0; i < np_; ++i)
      for (int64_t j = 0; j < np_; ++j)
        if ((i >= nn || j >= nn) && plan.T[(size_t)((o * np_ + i) * np_ + j)] != 0.0) return 5;
  std::vector<double> Td((size_t)(J * nn * nn)), sd((size_t)(G * nn));
  for (int64_t o = 0; o < J; ++o)
    for (int64_t i = 0; i < nn; ++i)
      for (int64_t j = 0; j < nn; ++j) Td[(size_t)((o * nn + i) * nn + j)] = plan.T[(size_t)((o * np_ + i) * np_ + j)];
  for (int64_t g = 0; g < G; ++g)
    for (int64_t i = 0; i < np_; ++i) {
      if (i < nn) sd[(size_t)(g * nn + i)] = plan.s[(size_t)(g * np_ + i)];
      else if (plan.s[(size_t)(g * np_ + i)] != 0.0) return 5;
    }
  std::vector<double> rank(plan.rank.begin(), plan.rank.end()), rows(plan.rows.begin(), plan.rows.end());
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  for (const std::vector<double>* v : {&Td, &sd, &plan.B, &rank, &rows})
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
    d = tmp_path_factory.mktemp("clnl_host")
    (d / "main.cpp").write_text(_MAIN)
    exe = str(d / "clnl_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-pthread", "-I", CSRC, str(d / "main.cpp"), "-o", exe], check=True)
    return exe


def test_host_planner_under_the_sanitizers(host_exe):
    """Every validation message (what lnl_host.h refuses; a target whose frequencies differ between pulsars; n_orf 0 and
    9 refused, 8 accepted; missing factors; a NaN and an infinite factor entry named by ORF, row and column; n = 16640
    refused and 16384 accepted; 32 GiB of factors accepted, more refused with the bytes), the plan of a small array (padding,
    symmetry, zero blocks), a rank-1 and a zero factor."""
    r = subprocess.run([host_exe], capture_output=True, text=True)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("all ok"), r.stdout[-6000:] + r.stderr[-4000:]


def run_host(host_exe, tmp_path, arr, grid, A):
    offs, toas, nu, Mmats, w, _, _, _ = H.array_tables(arr)
    P, n = len(offs) - 1, int(offs[-1])
    n_col = max(M.shape[1] for M in Mmats)
    Mfull = np.zeros((n, n_col))
    for p, M in enumerate(Mmats):
        Mfull[offs[p]:offs[p + 1], :M.shape[1]] = M
    assert all(np.ndim(c[0]) == 1 for c in arr["comps"]) and arr["masks"] is None
    fs = [np.asarray(c[0]) for c in arr["comps"]]
    n_modes = [len(f) for f in fs]
    N, G, J = n_modes[arr["target"]], len(grid), len(A)
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.array([P, n_col, len(fs), arr["target"], 0, 1, G, J] + list(offs) + [M.shape[1] for M in Mmats]
                          + n_modes, dtype=np.int64).tobytes())
        for a in ([c[1] for c in arr["comps"]], [c[2] for c in arr["comps"]], np.concatenate(fs),
                  np.concatenate(arr["phis"], axis=-1), grid, A, toas, nu, Mfull, w):
            fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    r = subprocess.run([host_exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    body = np.frombuffer(open(tmp_path / "out.bin", "rb").read(), dtype=np.float64)
    K = 2 * N
    nn = P * K
    o = np.cumsum([0, J * nn * nn, G * nn, K * n, P, P])
    return (body[:o[1]].reshape(J, nn, nn), body[o[1]:o[2]].reshape(G, nn), body[o[2]:o[3]],
            body[o[3]:o[4]].astype(int), body[o[4]:o[5]].astype(int))


# Measured on these shapes (the planner against the truth, both in long double, the planner rounded once to fp64):
#   |T - T_ld| per entry in eps of the row's largest entry, the largest over ORFs and rows:
#     P3N2 0.471, P3N3 0.396, P5N7 0.477;   |s - s_ld| in eps of s: 0.384, 0.291, 0.379
# The rounding to fp64 is the whole error. The bounds: 4 x the largest, floor 1 eps.
T_MEASURED_EPS, S_MEASURED_EPS = 0.477, 0.384
T_BOUND_EPS, S_BOUND_EPS = max(4 * T_MEASURED_EPS, 1.0), max(4 * S_MEASURED_EPS, 1.0)
# The formula against the literal dense form, in units of max(1, |dlnL|), as measured over the four ORFs: P3N2 2.59e-16,
# P3N3 6.08e-16, P5N7 4.88e-16; Gamma = I against lnl_reference: 2.64e-19 (longdouble rounding alone). 4 x margin:
LITERAL_MEASURED, IDENTITY_MEASURED = 6.08e-16, 2.64e-19
LITERAL_BOUND, IDENTITY_BOUND = 4 * LITERAL_MEASURED, 4 * IDENTITY_MEASURED


@pytest.mark.parametrize("name", ["P3N2", "P3N3", "P5N7"])
def test_t_and_s_match_the_longdouble_definition(host_exe, tmp_path, name):
    """T per ORF (Hellings-Downs, the rank-1 monopole, a random SPD matrix, the identity, in one call) to <= 1.91 eps
    per entry relative to its row's largest entry (4 x the measured 0.477) and s to 1.54 eps (4 x 0.384); T is symmetric
    bit for bit; with the identity the blocks off the diagonal are exactly zero; the zero grid row has s = 0."""
    arr = CR.arrays()[name]
    grid = CR.grid_of(arr)
    per = CR.base_of(name)
    P = len(per)
    orfs = CR.orfs_of(P)
    A = np.stack([CR.factor_of(g) for g in orfs.values()])
    T, s, B, rank, rows = run_host(host_exe, tmp_path, arr, grid, A)
    K = len(per[0][1])
    offs = H.array_tables(arr)[0]
    assert list(rank) == [int(q[2].sum()) for q in per]
    assert list(rows) == [K if offs[p + 1] > offs[p] else 0 for p in range(P)]
    worst_t = worst_s = 0.0
    for o, oname in enumerate(orfs):
        Tt = CR.t_matrix([q[1] for q in per], A[o])
        np.testing.assert_array_equal(T[o], T[o].T)
        rmax = np.max(np.abs(Tt), axis=1, keepdims=True)
        live = rmax[:, 0] > 0
        assert np.all(T[o][~live] == 0)
        worst_t = max(worst_t, float(np.max(np.abs(T[o].astype(LD) - Tt)[live] / rmax[live])) / EPS)
        if oname == "identity":
            off = np.kron(1 - np.eye(P), np.ones((K, K))).astype(bool)
            assert np.all(T[o][off] == 0)
    for g in range(len(grid)):
        st = CR.scale_of(grid[g], P)
        live = st > 0
        assert np.all(s[g][~live] == 0)
        if np.any(live):
            worst_s = max(worst_s, float(np.max(np.abs(s[g].astype(LD) - st)[live] / st[live])) / EPS)
    assert np.all(s[1] == 0)
    print(f"{name}: |T - T_ld| <= {worst_t:.3f} eps of the row's largest entry, |s - s_ld| <= {worst_s:.3f} eps")
    assert worst_t <= T_BOUND_EPS and worst_s <= S_BOUND_EPS


_FORMS = {}


def forms_of(name):
    """Per ORF (formula [G, R], literal [G, R]) of one array on three residual vectors, once."""
    if name not in _FORMS:
        arr = CR.arrays()[name]
        per, grid = CR.base_of(name), CR.grid_of(arr)
        offs = H.array_tables(arr)[0]
        P = len(per)
        res = CR.residuals_of(arr, 3)
        Xs = [per[p][0] @ res[:, offs[p]:offs[p + 1]].T.astype(LD) for p in range(P)]
        Zs = [q[1] for q in per]
        out = {}
        for oname, gam in CR.orfs_of(P).items():
            A = CR.factor_of(gam)
            out[oname] = (CR.dlnl_formula(Zs, Xs, A, grid), CR.dlnl_literal(arr, [q[2] for q in per], A, grid, res))
        _FORMS[name] = (out, Zs, Xs, grid)
    return _FORMS[name]


@pytest.mark.parametrize("name", ["P3N2", "P3N3", "P5N7"])
def test_the_formula_is_the_literal_log_density_difference(name):
    """For HD, the monopole, a random SPD Gamma and the identity: the formula equals ln p(r | Gamma, phi_g) - ln p(r |
    phi = 0) of the dense stacked covariance on the null space of the designs (longdouble Cholesky) to 2.43e-15 of
    max(1, |dlnL|) (4 x the measured 6.08e-16); Gamma = I equals lnl_reference's sum over the pulsars to 1.06e-18
    (4 x 2.64e-19); the zero grid row is exactly 0."""
    forms, Zs, Xs, grid = forms_of(name)
    worst = 0.0
    for oname, (f, lit) in forms.items():
        assert np.all(np.isfinite(f.astype(np.float64))) and np.any(f != 0)
        assert np.all(f[1] == 0)  # the all-zero row
        worst = max(worst, float(np.max(np.abs(f - lit) / np.maximum(1, np.abs(lit)))))
    Us = [LR.grid_truth(Z, grid)[:2] for Z in Zs]
    d = LR.dlnl([u[0] for u in Us], [u[1] for u in Us], Xs)[0]
    ident = float(np.max(np.abs(forms["identity"][0] - d) / np.maximum(1, np.abs(d))))
    print(f"{name}: |formula - literal| <= {worst:.3g} max(1, |dlnL|); Gamma = I against lnl_reference {ident:.3g}")
    assert worst <= LITERAL_BOUND and ident <= IDENTITY_BOUND
    # the ORF matters: HD and the identity differ by far more than the bound
    assert float(np.max(np.abs(forms["hd"][0] - forms["identity"][0]))) > 1e-3


def test_abi_declares_exports_and_binds_the_entry_points():
    from fakepta_amd import _capi
    text = open(HEADER).read()
    lib = ctypes.CDLL(LIB)
    for name in ENTRY_POINTS:
        assert re.search(rf"^int\s+{name}\s*\(", text, flags=re.M), name
        assert hasattr(lib, name) and name in _capi.EXPORTED
    assert re.search(r"^#define\s+FPTA_VERSION\s+10300\b", text, flags=re.M)
    for method in ("batch_set_clnl", "batch_clnl_info", "batch_clnl", "clnl_grid"):
        assert hasattr(_capi.Context, method)
    host = open(os.path.join(CSRC, "clnl_host.h")).read()
    assert "#include <hip" not in host and "__global__" not in host and "__device__" not in host  # plain C++
    assert '#include "lnl_host.h"' in host and "fpta_lnl::validate" in host and "fpta_os::run_pool" in host
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "clnl.hip" in make and "clnl_host.h" in make
    dev = open(os.path.join(CSRC, "clnl.hip")).read()
    assert "k_fit_apply<" not in dev and "fit_launch_unbooked" in dev and "dense_cholesky_at" in dev
    assert "atomic" not in dev.lower().replace("no atomics", "")
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS:
        assert name in integ


def test_host_algebra_on_numbers_built_by_hand():
    from fakepta_amd import clnl, lnl
    from fakepta_amd.batch import batch_factor
    psrs = [H._Psr(5, [1, 0, 0]), H._Psr(7, [0.3, 1, 0]), H._Psr(6, [0.2, 0.1, 1])]
    spd = np.array([[2.0, 0.5, 0.1], [0.5, 1.0, 0.2], [0.1, 0.2, 1.5]])
    names, gam, A = clnl.orf_factors(psrs, ("hd", "curn", "monopole", spd))
    assert names == ["hd", "curn", "monopole", "orf3"] and gam.shape == (4, 3, 3) and A.shape == (4, 3, 3)
    for o in range(4):
        np.testing.assert_allclose(A[o] @ A[o].T, gam[o], rtol=0, atol=1e-12)
    np.testing.assert_array_equal(gam[1], np.eye(3))
    np.testing.assert_array_equal(A[1], np.eye(3))
    np.testing.assert_array_equal(A[3], batch_factor(spd))
    assert np.count_nonzero(np.any(A[2] != 0, axis=0)) == 1  # the monopole's factor has one column
    assert clnl.orf_factors(psrs, "hd")[0] == ["hd"]
    asym = spd.copy()
    asym[0, 1] += 1e-6
    for bad, msg in ((asym, "not symmetric"),
                     (np.array([[1.0, 2, 0], [2, 1, 0], [0, 0, 1]]), "not positive semidefinite"),
                     (-np.eye(3), "not positive semidefinite"), (np.eye(2), r"must be \[3, 3\]"),
                     (np.full((3, 3), np.nan), "not finite")):
        with pytest.raises(ValueError, match=msg):
            clnl.orf_factors(psrs, [bad])
    with pytest.raises(ValueError, match="ORFs outside"):
        clnl.orf_factors(psrs, ["hd"] * 9)
    with pytest.raises(ValueError, match="ORFs outside"):
        clnl.orf_factors(psrs, [])
    d = np.array([[[0.0, -1.0], [1.0, -1.0], [0.5, -3.0]], [[2.0, 0.0], [1.0, 0.5], [0.0, 1.0]]])  # [2, G = 3, R = 2]
    out = clnl.derive(d, ["hd", "curn"])
    np.testing.assert_array_equal(out["lnB"], np.stack([lnl.log_bayes(d[0]), lnl.log_bayes(d[1])]))
    np.testing.assert_array_equal(out["lnB_vs_curn"], out["lnB"] - out["lnB"][1])
    assert np.all(out["lnB_vs_curn"][1] == 0) and out["argmax"].tolist() == [[1, 0], [0, 2]]
    assert out["orfs"] == ["hd", "curn"]
    assert "lnB_vs_curn" not in clnl.derive(d, ["hd", "monopole"]) and "posterior" not in out
    Aax, g = np.array([-14.0, -13.5, -13.0]), np.array([13 / 3])
    out = clnl.derive(d, ["hd", "curn"], (Aax, g), want_posterior=True)
    assert out["dlnL"].shape == (2, 3, 1, 2) and out["posterior"].shape == (2, 3, 1, 2)
    assert out["argmax"][0].tolist() == [[1, 0], [0, 2]]
    assert out["log10_A_ml"].tolist() == [[-13.5, -14.0], [-14.0, -13.0]]
    np.testing.assert_allclose(out["posterior"].sum(axis=(1, 2)), 1.0)
    with pytest.raises(ValueError):
        clnl.derive(d, ["hd"])


def test_set_correlated_likelihood_argument_checks_need_no_device():
    from fakepta_amd.batch import BatchSimulator
    psrs = [H._Psr(5, [1, 0, 0]), H._Psr(7, [0.3, 1, 0], t1=2e8), H._Psr(6, [0.2, 0.1, 1])]

    class Ctx(H._RecordingCtx):
        def __getattr__(self, name):
            def call(*a, **k):
                self.calls.append((name, a, k))
                if name == "batch_set_clnl":
                    return np.full(self.P, 3, dtype=np.int32), np.ones((len(a[7]), len(a[6])))
                if name == "batch_clnl":
                    s = self.calls_of("batch_set_clnl")[-1][1]
                    return np.ones((len(s[7]), len(s[6]), 4)), None, None, None
            return call

    ctx = Ctx(len(psrs))
    sim = BatchSimulator(psrs, signals=[], white=False, ctx=ctx)
    with pytest.raises(ValueError, match="no correlated likelihood"):
        sim.correlated_likelihood()
    with pytest.raises(ValueError, match="0 common signals"):
        sim.set_correlated_likelihood(log10_A=[-14.0], gamma=[3.0])
    fc = np.array([1e-8, 2e-8, 3e-8])
    sim.segments.append(dict(name="gw_common", kind=1, f=fc, amp=np.array([3e-7, 2e-7, 1e-7]), idx=0.0, freqf=1400.0,
                             mask=None))
    n0 = len(ctx.calls)
    ok = dict(log10_A=[-14.0], gamma=[3.0])
    for bad in (dict(), dict(phi=-np.ones((2, 3))), dict(ok, orfs=[np.array([[1.0, 2, 0], [2, 1, 0], [0, 0, 1]])]),
                dict(ok, orfs=[np.eye(2)]), dict(ok, orfs=["hd"] * 9), dict(ok, noise="model"), dict(ok, target=7)):
        with pytest.raises(ValueError):
            sim.set_correlated_likelihood(**bad)
    assert len(ctx.calls) == n0  # refused before anything reached the context
    rank = sim.set_correlated_likelihood(log10_A=[-14.0, -13.0], gamma=[3.0, 4.0, 5.0])
    name, a, k = ctx.calls[-1]
    assert name == "batch_set_clnl" and list(a[0]) == [3] and a[5] == 0 and a[6].shape == (6, 3) and len(rank) == 3
    assert a[7].shape == (2, 3, 3) and np.array_equal(a[7][1], np.eye(3)) and k["M"].shape == (18, 3)
    out = sim.correlated_likelihood(posterior=True)
    assert out["dlnL"].shape == (2, 2, 3, 4) and out["lnB"].shape == (2, 4) and out["lnB_vs_curn"].shape == (2, 4)
    assert out["orfs"] == ["hd", "curn"] and out["posterior"].shape == (2, 2, 3, 4) and len(out["argmax"]) == 2
    sim.set_correlated_likelihood(orfs=["monopole"], phi=np.ones((2, 3)), Mmats=None, weights=None)
    assert "lnB_vs_curn" not in sim.correlated_likelihood() and sim.correlated_likelihood()["dlnL"].shape == (1, 2, 4)


# ----------------------------------------------------------------------------- a statement of the definition
# 6 pulsars of tests/test_os_host.unbiased_layout's kind, the common process injected at STATEMENT_AMP x that layout's
# amplitude, 1024 oracle realizations per seed. In expectation ln p(r | HD) - ln p(r | CURN) at the injected spectrum is
# a Kullback-Leibler divergence: > 0 when the data are HD-correlated, < 0 when they are uncorrelated (Gibbs' inequality).
# Measured with clnl_reference for the seeds 1 .. 5 (mean / standard error): see test_gpu_clnl.py's statement test,
# which runs the device on the same realizations; the CPU half here checks the margins on one seed.
STATEMENT_P, STATEMENT_R, STATEMENT_AMP = 6, 1024, 3.0


def statement_layout(identity):
    """The first 6 pulsars of test_os_host.unbiased_layout with the common process at STATEMENT_AMP x its amplitude."""
    from oracle import fakepta_oracle as O
    lay = H.unbiased_layout(identity=identity)
    P = STATEMENT_P
    offs = lay["offs"][:P + 1]
    n = int(offs[-1])
    hd = np.asarray(O.orf_hd(lay["pos"][:P]), dtype=np.float64)
    L = np.eye(P) if identity else np.linalg.cholesky(hd)
    amp = STATEMENT_AMP * lay["amp_gw"]
    segs = [O.Segment(0, 2 * np.pi * lay["f_rn"][:P], lay["amp_rn"][:P], 0.0),
            O.Segment(1, 2 * np.pi * lay["f_gw"], amp, 0.0, L=L)]
    return dict(offs=offs, toas=lay["toas"][:n], nu=lay["nu"][:n], sigma=lay["sigma"][:n], Mmats=lay["Mmats"][:P],
                pos=lay["pos"][:P], f_gw=lay["f_gw"], amp_gw=amp, f_rn=lay["f_rn"][:P], amp_rn=lay["amp_rn"][:P], L=L,
                hd=hd, segs=segs, comps_of=lay["comps_of"], phis_of=lambda p: [lay["amp_rn"][p] ** 2, amp ** 2])


_STATEMENT = {}


def statement_truth(lay):
    """Per pulsar (B0, Z) and per ORF (HD, CURN) (T, s, L) of the statement layout at the injected spectrum, once."""
    if not _STATEMENT:
        P = STATEMENT_P
        per = []
        for p in range(P):
            sl = slice(int(lay["offs"][p]), int(lay["offs"][p + 1]))
            B, Z, _, _ = LR.base_operator(lay["toas"][sl], lay["nu"][sl], lay["Mmats"][p], 1 / lay["sigma"][sl] ** 2,
                                          lay["comps_of"](p), lay["phis_of"](p), 1)
            per.append((B, Z))
        _STATEMENT["per"] = per
        _STATEMENT["A"] = [np.linalg.cholesky(lay["hd"]), np.eye(P)]
    return _STATEMENT["per"], _STATEMENT["A"]


def statement_difference(identity, seed):
    """dlnL_hd - dlnL_curn [R] at the injected spectrum from clnl_reference on STATEMENT_R oracle realizations."""
    from oracle import fakepta_oracle as O
    lay = statement_layout(identity)
    res = O.batch_synth(lay["offs"], lay["toas"], lay["nu"], lay["segs"], seed, 0, STATEMENT_R, sigma=lay["sigma"])
    per, As = statement_truth(lay)
    X, _ = OS.x_truth([q[0] for q in per], lay["offs"], res)
    grid = (lay["amp_gw"] ** 2)[None]
    d = [CR.dlnl_formula([q[1] for q in per], list(X), A, grid)[0] for A in As]
    return (d[0] - d[1]).astype(np.float64)


@pytest.mark.parametrize("identity", [False, True])
def test_the_mean_hd_minus_curn_has_the_sign_of_the_injection(identity):
    """1024 oracle realizations (seed 1) of the 6-pulsar layout: the realization mean of dlnL_hd - dlnL_curn at the
    injected spectrum is > 0 with the process drawn HD-correlated and < 0 with it drawn uncorrelated, by more than 3
    standard errors (the longdouble reference; the device runs the seeds 1 .. 5 in tests/test_gpu_clnl.py)."""
    diff = statement_difference(identity, 1)
    mean, se = float(np.mean(diff)), float(np.std(diff) / np.sqrt(len(diff)))
    print(f"identity {identity}: mean dlnL_hd - dlnL_curn = {mean:.4f} +- {se:.4f} ({mean / se:.1f} standard errors)")
    assert (mean < -3 * se) if identity else (mean > 3 * se)
