"""Likelihood grid, host side (no GPU): csrc/lnl_host.h (validation, the base operator with the target left out, Z in
long double, the per-grid-point factor U, the log-determinant and the device layout of U) in a stand-alone C++ program
built with the address and undefined-behaviour sanitizers, against the np.longdouble definition of
tests/lnl_reference.py; the truth against the definition without an inverse and against the literal dense form; the
C-ABI surface; the host algebra of fakepta_amd.lnl; a statement of the definition on oracle realizations."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import lnl_reference as LR
from tests import os_reference as OS
from tests import test_os_host as H
from tests import tm_reference as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fakepta_amd.h")
LIB = os.path.join(ROOT, "fakepta_amd", "lib", "libfakepta_amd.so")
CSRC = os.path.join(ROOT, "fakepta_amd", "csrc")
ENTRY_POINTS = ("fpta_batch_set_lnl", "fpta_batch_lnl_info", "fpta_batch_lnl", "fpta_lnl_grid")
EPS = np.finfo(np.float64).eps
LD = np.longdouble

# argv: in out. in: int64 P, n_col, C, target, has_mask, f_common, G; offs [P + 1]; ncol [P]; n_modes [C]; then fp64
# idx [C], freqf [C], f [rows][sum N], phi [P][sum N], grid [G][N], t [n], nu [n], M [n][n_col], w [n]; then uint8 mask
# [C][n] (has_mask). out: fp64 B [K n], U [P][G][K][K], ld [P][G], ld_sum [G], rank [P], rows [P]. Without arguments: the
# checks that need no data.
_MAIN = r"""
#include <cstdio>
#include <cstring>
#include <limits>
#include "lnl_host.h"
using namespace fpta_lnl;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)
struct Case {
  int64_t P = 3;
  int64_t offs[4] = {0, 3, 3, 7};  // the middle pulsar has no TOAs
  std::vector<double> t, nu, M, w, f, idx, freqf, phi, grid;
  std::vector<int32_t> n_modes;
  int64_t n_col = 2, G = 2;
  Spec sp;
  Case() : t(7), nu(7, 1400.0), M(7 * 2, 1.0), w(7, 2.0), f{1e-8, 2e-8, 3e-8}, idx{0.0, 2.0}, freqf{1400.0, 1400.0},
           phi(3 * 3, 1e-2), grid{1.0, 0.5, 0.0, 0.0}, n_modes{2, 1} {
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
    sp.mask = nullptr;
    sp.target = 0;
    return sp;
  }
  bool ok(std::string& why) {
    return validate(P, offs, t.data(), nu.data(), sp, n_col, M.data(), nullptr, w.data(), G, grid.data(), why);
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
  // what os_host.h's validate refuses comes through with its messages
  { Case c; c.n_col = 17; CHECK(c.refused("n_col 17")); }
  { Case c; c.w[4] = 0.0; CHECK(c.refused("pulsar 2, TOA 1: weight")); }
  { Case c; c.sp.target = 2; CHECK(c.refused("target component")); }
  { Case c; c.phi[2 * 3 + 2] = -1.0; CHECK(c.refused("pulsar 2, component 1, mode 0: prior variance")); }
  // the grid
  for (double bad : {-1e-3, nan, inf}) {
    Case c; c.grid[1 * 2 + 1] = bad; CHECK(c.refused("grid row 1, mode 1: prior variance is negative or not finite"));
  }
  { Case c; c.grid[0] = nan; CHECK(c.refused("grid row 0, mode 0")); }
  { Case c; c.G = 0; CHECK(c.refused("0 grid points outside [1, 4096]")); }
  { Case c; c.G = 4097; c.grid.assign(4097 * 2, 1.0); CHECK(c.refused("4097 grid points outside [1, 4096]")); }
  { Case c; c.G = 4096; c.grid.assign(4096 * 2, 1.0); CHECK(c.ok(why)); }
  { Case c; c.n_modes = {129, 1}; c.f.assign(130, 1e-8); c.phi.assign(3 * 130, 1.0); c.grid.assign(2 * 129, 1.0); c.spec();
    CHECK(c.refused("target component 0: 258 Fourier columns, more than 256")); }
  { Case c; c.n_modes = {128, 1}; c.f.assign(129, 1e-8); c.phi.assign(3 * 129, 1.0); c.grid.assign(2 * 128, 1.0); c.spec();
    CHECK(c.ok(why)); }
  // the device layout: every (row, column <= the row group's diagonal block) has its own place below packed_size
  for (int32_t K : {2, 16, 18, 60, 62, 256}) {
    std::vector<int> seen((size_t)packed_size(K), 0);
    const int32_t kg = groups_of(K);
    for (int32_t i = 0; i < 16 * kg; ++i)
      for (int32_t j = 0; j < 16 * (i / 16 + 1); ++j) {
        const int64_t at = packed_index(i, j);
        CHECK(at >= 0 && at < packed_size(K));
        if (at >= 0 && at < packed_size(K)) ++seen[(size_t)at];
      }
    for (int v : seen) CHECK(v == 1);
  }
  // the plan of an array: a pulsar without TOAs has no rows, U = diag(sqrt(phi)) (Z = 0) and ld = 0; a grid row of zeros
  // has U = 0 and ld = 0 for everyone
  {
    Case c;
    Plan plan;
    std::vector<double> U((size_t)(3 * 2 * 16), -1.0);
    CHECK(make_plan(c.P, c.offs, c.t.data(), c.nu.data(), c.sp, c.n_col, c.M.data(), nullptr, c.w.data(), 0.0, c.G,
                    c.grid.data(), plan, why, U.data()) == 0);
    CHECK(plan.K == 4 && plan.N == 2 && plan.G == 2 && plan.u_stride == 256 && plan.B.size() == 4 * 7);
    CHECK(plan.U.size() == 3 * 2 * 256 && plan.ld.size() == 6 && plan.ld_sum.size() == 2);
    CHECK(plan.rows[0] == 4 && plan.rows[1] == 0 && plan.rows[2] == 4 && plan.max_rows == 4);
    CHECK(plan.rank[0] == 2 && plan.rank[1] == 0 && plan.rank[2] == 2);
    CHECK(plan.ld[0] > 0.0 && plan.ld[2] == 0.0 && plan.ld[4] > 0.0);
    CHECK(plan.ld[1] == 0.0 && plan.ld[3] == 0.0 && plan.ld[5] == 0.0 && plan.ld_sum[1] == 0.0);
    CHECK(plan.ld_sum[0] > plan.ld[0]);
    for (int i = 0; i < 16; ++i) {
      CHECK(U[16 + i] == 0.0 && U[48 + i] == 0.0 && U[80 + i] == 0.0);   // the zero grid row
      CHECK(std::fabs(U[32 + i] - (i == 0 || i == 10 ? 1.0 : i == 5 || i == 15 ? std::sqrt(0.5) : 0.0)) <= 2e-16);  // no TOAs
    }
    for (int p = 0; p < 3; ++p)
      for (int g = 0; g < 2; ++g)
        for (int i = 0; i < 4; ++i)
          for (int j = 0; j < 4; ++j) {
            const double u = U[(size_t)(((p * 2 + g) * 4 + i) * 4 + j)];
            if (j > i) CHECK(u == 0.0);
            else CHECK(plan.U[(size_t)((p * 2 + g) * 256 + packed_index(i, j))] == u);
          }
    c.grid[3] = -1.0;
    CHECK(make_plan(c.P, c.offs, c.t.data(), c.nu.data(), c.sp, c.n_col, c.M.data(), nullptr, c.w.data(), 0.0, c.G,
                    c.grid.data(), plan, why) == 1 && why.find("grid row 1, mode 1") != std::string::npos);
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
  std::vector<int64_t> hdr(7);
  if (!rd(in, hdr)) return 2;
  const int64_t P = hdr[0], n_col = hdr[1], C = hdr[2], G = hdr[6];
  std::vector<int64_t> offs((size_t)P + 1), ncol64((size_t)P), nm64((size_t)C);
  if (!rd(in, offs) || !rd(in, ncol64) || !rd(in, nm64)) return 2;
  std::vector<int32_t> ncol(ncol64.begin(), ncol64.end()), nm(nm64.begin(), nm64.end());
  int64_t nf = 0;
  for (int64_t v : nm64) nf += v;
  const int64_t n = offs[(size_t)P], N = nm64[(size_t)hdr[3]], K = 2 * N;
  std::vector<double> idx((size_t)C), ff((size_t)C), f((size_t)((hdr[5] ? 1 : P) * nf)), phi((size_t)(P * nf)),
      grid((size_t)(G * N)), t((size_t)n), nu((size_t)n), M((size_t)(n * n_col)), w((size_t)n);
  std::vector<uint8_t> mask((size_t)(hdr[4] ? C * n : 0));
  if (!rd(in, idx) || !rd(in, ff) || !rd(in, f) || !rd(in, phi) || !rd(in, grid) || !rd(in, t) || !rd(in, nu) ||
      !rd(in, M) || !rd(in, w) || !rd(in, mask))
    return 2;
  std::fclose(in);
  Spec sp;
  sp.comps.n_comp = (int32_t)C; sp.comps.n_modes = nm.data(); sp.comps.f = f.data(); sp.comps.f_is_common = hdr[5] != 0;
  sp.comps.idx = idx.data(); sp.comps.freqf = ff.data();
  sp.phi = phi.data(); sp.mask = hdr[4] ? mask.data() : nullptr; sp.target = (int32_t)hdr[3];
  Plan plan;
  std::string why;
  std::vector<double> U((size_t)(P * G * K * K));
  const int made = make_plan(P, offs.data(), t.data(), nu.data(), sp, n_col, M.data(), ncol.data(), w.data(), 0.0, G,
                             grid.data(), plan, why, U.data());
  if (made) { std::printf("make_plan: %d %s\n", made, why.c_str()); return 3; }
  if ((int64_t)plan.B.size() != K * n || (int64_t)plan.U.size() != P * G * plan.u_stride) return 4;
  for (int64_t pg = 0; pg < P * G; ++pg)  // the device layout holds the dense factor's lower triangle
    for (int32_t i = 0; i < K; ++i)
      for (int32_t j = 0; j <= i; ++j)
        if (plan.U[(size_t)(pg * plan.u_stride + packed_index(i, j))] != U[(size_t)((pg * K + i) * K + j)]) return 5;
  std::vector<double> rank(plan.rank.begin(), plan.rank.end()), rows(plan.rows.begin(), plan.rows.end());
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  for (const std::vector<double>* v : {&plan.B, &U, &plan.ld, &plan.ld_sum, &rank, &rows})
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
    d = tmp_path_factory.mktemp("lnl_host")
    (d / "main.cpp").write_text(_MAIN)
    exe = str(d / "lnl_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-pthread", "-I", CSRC, str(d / "main.cpp"), "-o", exe], check=True)
    return exe


def test_host_planner_under_the_sanitizers(host_exe):
    """Every validation message (what os_host.h refuses; a negative, NaN and infinite grid entry named by row and mode;
    G = 0 and 4097 refused, 4096 accepted; K = 258 refused, 256 accepted), the device layout's index map for K = 2 ..
    256, a pulsar without TOAs and a grid row of zeros (U = 0, ld = 0 exactly)."""
    r = subprocess.run([host_exe], capture_output=True, text=True)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("all ok"), r.stdout[-6000:] + r.stderr[-4000:]


def grids():
    """Per array of test_os_host.arrays() the grids of the host tests: name -> [G, N]. G = 1 and G = 5 with an all-zero
    row; rows with zero modes; for N30 a row 1e6 x the intrinsic red level of the 250-TOA pulsar (cond(C) large)."""
    arrs = H.arrays()
    out = {}
    for name, arr in arrs.items():
        base = np.asarray(arr["phis"][arr["target"]])[-1].copy()  # the target's own spectrum on the last pulsar
        N = len(base)
        g5 = np.stack([base, np.zeros(N), 10.0 * base, 0.1 * base * np.arange(1, N + 1) ** 1.5, base])
        g5[2, ::3] = 0.0  # zero modes
        g5[4, N // 2:] = 0.0
        if name == "N30":
            g5[3] = 1e6 * np.asarray(arr["phis"][0])[0]  # 1e6 x the intrinsic red level of the first pulsar
        out[name] = {"G1": g5[2:3].copy(), "G5": g5}
    return out


def run_host(host_exe, tmp_path, arr, grid):
    offs, toas, nu, Mmats, w, _, _, _ = H.array_tables(arr)
    P, n = len(offs) - 1, int(offs[-1])
    n_col = max(M.shape[1] for M in Mmats)
    Mfull = np.zeros((n, n_col))
    for p, M in enumerate(Mmats):
        Mfull[offs[p]:offs[p + 1], :M.shape[1]] = M
    common = all(np.ndim(c[0]) == 1 for c in arr["comps"])
    fs = [np.asarray(c[0]) if common or np.ndim(c[0]) == 2 else np.tile(c[0], (P, 1)) for c in arr["comps"]]
    n_modes = [f.shape[-1] for f in fs]
    N, G = n_modes[arr["target"]], len(grid)
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.array([P, n_col, len(fs), arr["target"], 0 if arr["masks"] is None else 1, 1 if common else 0, G]
                          + list(offs) + [M.shape[1] for M in Mmats] + n_modes, dtype=np.int64).tobytes())
        for a in ([c[1] for c in arr["comps"]], [c[2] for c in arr["comps"]], np.concatenate(fs, axis=-1),
                  np.concatenate(arr["phis"], axis=-1), grid, toas, nu, Mfull, w):
            fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        if arr["masks"] is not None:
            fh.write(np.stack([np.ones(n, dtype=np.uint8) if m is None else m for m in arr["masks"]]).tobytes())
    r = subprocess.run([host_exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    body = np.frombuffer(open(tmp_path / "out.bin", "rb").read(), dtype=np.float64)
    K = 2 * N
    o = np.cumsum([0, K * n, P * G * K * K, P * G, G, P, P])
    B = [body[K * offs[p]:K * offs[p + 1]].reshape(K, -1) for p in range(P)]
    return (B, body[o[1]:o[2]].reshape(P, G, K, K), body[o[2]:o[3]].reshape(P, G), body[o[3]:o[4]],
            body[o[4]:o[5]].astype(int), body[o[5]:o[6]].astype(int))


_TRUTH = {}


def truth_of(name):
    """Per pulsar (B0, Z, keep) of the longdouble definition with the target left out, once per array."""
    if name not in _TRUTH:
        arr = H.arrays()[name]
        offs, toas, nu, Mmats, w, comps_of, phis_of, masks_of = H.array_tables(arr)
        per = []
        for p in range(len(offs) - 1):
            sl = slice(int(offs[p]), int(offs[p + 1]))
            B, Z, norms, keep = LR.base_operator(toas[sl], nu[sl], Mmats[p], w[sl], comps_of(p), phis_of(p),
                                                 arr["target"], masks_of(p))
            T.assert_clear_rank(norms, keep, Mmats[p])
            per.append((B, Z, keep))
        _TRUTH[name] = per
    return _TRUTH[name]


# Measured on these shapes (the planner against the truth, both in long double, the planner rounded once to fp64):
#   |U - U_ld| per entry in eps of the row's largest entry, the largest over pulsars, grid points and rows:
#     N4 0.411 (cond(C) <= 1.41), N9 0.446 (cond(C) <= 1.30), N30 0.995 (cond(C) <= 4.64e9)
#   |ld - ld_ld| in eps of max(1, |ld|): N4 0.097, N9 0.097, N30 0.221
# The rounding to fp64 is nearly the whole error, whatever cond(C). The bounds: 4 x the largest, floor 1 eps.
U_MEASURED_EPS, LD_MEASURED_EPS = 0.995, 0.221
U_BOUND_EPS, LD_BOUND_EPS = max(4 * U_MEASURED_EPS, 1.0), max(4 * LD_MEASURED_EPS, 1.0)
# The truth against the definition without an inverse, |U^T U (I + Z phi) - phi| relative to max(phi), as measured: N4
# 2.84e-19, N9 2.06e-19, N30 2.55e-14 (longdouble rounding through cond(C) = 4.64e9; a wrong formula gives O(1)). dlnL
# against the literal dense form relative to max(1, |dlnL|): N4 4.49e-17, N9 2.24e-16. 4 x margin:
IDENTITY_BOUND, LITERAL_BOUND = 4 * 2.55e-14, 4 * 2.24e-16


@pytest.mark.parametrize("name,gname", [("N4", "G1"), ("N4", "G5"), ("N9", "G5"), ("N30", "G5")])
def test_factors_and_log_determinants_match_the_longdouble_definition(host_exe, tmp_path, name, gname):
    """U_pg to <= 3.98 eps per entry relative to its row's largest entry (4 x the measured 0.995) and ld_pg to <= 1 eps
    of max(1, |ld|) (4 x the measured 0.221, floor 1 eps); ld_sum is the pulsar-order sum; rows of zero modes and the zero grid row are exactly
    zero; a pulsar without TOAs has U = diag(sqrt(phi)), ld = 0. The truth itself satisfies U^T U (I + Z phi) = phi in
    longdouble products without an inverse."""
    arr = H.arrays()[name]
    grid = grids()[name][gname]
    offs = H.array_tables(arr)[0]
    B, U, ld, ld_sum, rank, rows = run_host(host_exe, tmp_path, arr, grid)
    per = truth_of(name)
    P, G, K = U.shape[:3]
    worst_u = worst_ld = worst_c = worst_id = 0.0
    ld_truth = np.zeros((P, G), dtype=LD)
    for p in range(P):
        Bt, Zt, keep = per[p]
        n = Bt.shape[1]
        assert rank[p] == int(keep.sum()) and rows[p] == (K if n else 0)
        if n:
            row_max = np.max(np.abs(Bt), axis=1, keepdims=True)
            assert float(np.max(np.abs(B[p].astype(LD) - Bt) / np.max(row_max))) <= H.B_BOUND_EPS * EPS
        Ut, ldt, cond = LR.grid_truth(Zt, grid)
        ld_truth[p] = ldt
        for g in range(G):
            ph2 = np.concatenate([grid[g], grid[g]])
            assert np.all(U[p, g][np.triu_indices(K, 1)] == 0)
            assert np.all(U[p, g][ph2 == 0] == 0) and np.all(U[p, g][:, ph2 == 0] == 0)
            if not np.any(ph2):
                assert np.all(U[p, g] == 0) and ld[p, g] == 0.0
                continue
            if n == 0:
                assert np.all(np.abs(U[p, g] - np.diag(np.sqrt(ph2))) <= EPS * np.diag(np.sqrt(ph2))) and ld[p, g] == 0.0
                continue
            rmax = np.max(np.abs(Ut[g]), axis=1, keepdims=True)
            live = rmax[:, 0] > 0
            worst_u = max(worst_u, float(np.max(np.abs(U[p, g].astype(LD) - Ut[g])[live] / rmax[live])) / EPS)
            worst_ld = max(worst_ld, float(abs(LD(ld[p, g]) - ldt[g]) / max(LD(1), abs(ldt[g]))) / EPS)
            worst_c = max(worst_c, cond[g])
            # U^T U (I + Z phi) = phi, in longdouble products
            phl = ph2.astype(LD)
            lhs = (Ut[g].T @ Ut[g]) @ (np.eye(K, dtype=LD) + Zt * phl[None, :])
            worst_id = max(worst_id, float(np.max(np.abs(lhs - np.diag(phl))) / np.max(phl)))
    print(f"{name} {gname}: |U - U_ld| <= {worst_u:.3f} eps of the row's largest entry, |ld - ld_ld| <= {worst_ld:.3f} "
          f"eps of max(1, |ld|), cond(C) <= {worst_c:.3g}, |U^T U (I + Z phi) - phi| <= {worst_id:.3g} max(phi)")
    assert worst_u <= U_BOUND_EPS and worst_ld <= LD_BOUND_EPS and worst_id <= IDENTITY_BOUND
    want = np.zeros(G, dtype=LD)
    for p in range(P):
        want = want + ld_truth[p]
    assert np.all(np.abs(ld_sum.astype(LD) - want) <= LD_BOUND_EPS * EPS * np.maximum(1, np.abs(want)))


@pytest.mark.parametrize("name,pulsars", [("N4", (0,)), ("N9", (0, 1))])
def test_the_truth_is_the_literal_log_density_difference(name, pulsars):
    """On the 17-, 33- and 60-TOA pulsars: (q - ld) / 2 of the truth equals ln p(r | phi_g) - ln p(r | phi = 0) of the
    dense covariances restricted to the null space of M (longdouble Cholesky), to 9e-16 of max(1, |dlnL|) (4 x the
    measured 2.24e-16), for random residuals of the model's scale."""
    arr = H.arrays()[name]
    grid = grids()[name]["G5"]
    offs, toas, nu, Mmats, w, comps_of, phis_of, masks_of = H.array_tables(arr)
    rng = np.random.default_rng(11)
    worst = 0.0
    for p in pulsars:
        sl = slice(int(offs[p]), int(offs[p + 1]))
        Bt, Zt, keep = truth_of(name)[p]
        r = rng.normal(size=(3, Bt.shape[1])) / np.sqrt(w[sl]) * 3.0
        X = Bt @ r.T.astype(LD)
        Ut, ldt, _ = LR.grid_truth(Zt, grid)
        for g in range(len(grid)):
            q, _ = LR.quad(Ut[g], X)
            got = (q - ldt[g]) / 2
            lit = LR.literal_dlnl(toas[sl], nu[sl], Mmats[p], w[sl], comps_of(p), phis_of(p), arr["target"], grid[g],
                                  keep, r, masks_of(p))
            worst = max(worst, float(np.max(np.abs(got - lit) / np.maximum(1, np.abs(lit)))))
    print(f"{name}: |dlnL - literal| <= {worst:.3g} max(1, |dlnL|)")
    assert worst <= LITERAL_BOUND


def test_abi_declares_exports_and_binds_the_entry_points():
    from fakepta_amd import _capi
    text = open(HEADER).read()
    lib = ctypes.CDLL(LIB)
    for name in ENTRY_POINTS:
        assert re.search(rf"^int\s+{name}\s*\(", text, flags=re.M), name
        assert hasattr(lib, name) and name in _capi.EXPORTED
    assert re.search(r"^#define\s+FPTA_VERSION\s+10300\b", text, flags=re.M)
    for method in ("batch_set_lnl", "batch_lnl_info", "batch_lnl", "lnl_grid"):
        assert hasattr(_capi.Context, method)
    host = open(os.path.join(CSRC, "lnl_host.h")).read()
    assert "#include <hip" not in host and "__global__" not in host and "__device__" not in host  # plain C++
    assert '#include "os_host.h"' in host and "fpta_os::build_operator" in host and "fpta_os::validate" in host
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "lnl.hip" in make and "lnl_host.h" in make
    dev = open(os.path.join(CSRC, "lnl.hip")).read()
    assert "k_fit_apply<" not in dev and "fit_launch_unbooked" in dev  # the fit's kernel is launched, not forked
    assert "atomic" not in dev.lower().replace("no atomics", "")


def test_host_algebra_on_numbers_built_by_hand():
    from fakepta import spectrum
    from fakepta_amd import lnl
    f = np.arange(1, 6) / 3e8
    A, g = np.array([-14.0, -13.5]), np.array([3.0, 13 / 3, 5.0])
    phi = lnl.powerlaw_grid(f, A, g)
    assert phi.shape == (6, 5)
    for i, a in enumerate(A):
        for j, gm in enumerate(g):
            np.testing.assert_array_equal(phi[i * 3 + j], spectrum.powerlaw(f, a, gm) * np.diff(np.append(0.0, f)))
    for bad in (dict(f=-f), dict(log10_A=[]), dict(gamma=[np.nan]), dict(f=f[None])):
        with pytest.raises(ValueError):
            lnl.powerlaw_grid(**{**dict(f=f, log10_A=A, gamma=g), **bad})
    d = np.array([[0.0, -1.0, 2.0], [1.0, -1.0, 2.0], [0.5, -3.0, np.log(3.0)]])  # [G = 3, R = 3]
    assert list(lnl.argmax(d)) == [1, 0, 0]  # the first of equals
    want = np.log(np.mean(np.exp(d), axis=0))
    np.testing.assert_allclose(lnl.log_bayes(d), want, rtol=1e-15)
    np.testing.assert_allclose(lnl.log_bayes(d + 800.0), want + 800.0, rtol=1e-15)  # no overflow
    post = lnl.posterior(d)
    np.testing.assert_allclose(post, np.exp(d) / np.sum(np.exp(d), axis=0), rtol=1e-15)
    out = lnl.derive(np.arange(12.0).reshape(6, 2) * np.array([1.0, -1.0]), (A, g), want_posterior=True)
    assert out["dlnL"].shape == (2, 3, 2) and out["posterior"].shape == (2, 3, 2)
    assert [int(out["argmax"][0][0]), int(out["argmax"][1][0])] == [1, 2]
    assert [int(out["argmax"][0][1]), int(out["argmax"][1][1])] == [0, 0]
    assert list(out["log10_A_ml"]) == [-13.5, -14.0] and list(out["gamma_ml"]) == [5.0, 3.0]
    q, ld = np.arange(24.0).reshape(2, 3, 4), np.array([[1.0, 2.0, 3.0], [0.0, 0.5, 0.25]])
    out = lnl.derive(np.zeros((3, 4)), None, ld, q)
    np.testing.assert_array_equal(out["dlnL_psr"], 0.5 * (q - ld[:, :, None]))
    assert out["log10_A"] is None and out["argmax"].shape == (4,)
    for bad in (np.zeros(3), np.zeros((0, 3))):
        with pytest.raises(ValueError):
            lnl.log_bayes(bad)
    with pytest.raises(ValueError, match="grid row 1, mode 2"):
        lnl.check_grid(np.array([[1.0, 1.0, 1.0], [1.0, 1.0, -1.0]]), 3)
    with pytest.raises(ValueError, match="grid points outside"):
        lnl.check_grid(np.ones((4097, 2)), 2)
    with pytest.raises(ValueError, match="modes per row"):
        lnl.check_grid(np.ones((2, 2)), 3)
    for bad in (dict(), dict(phi=np.ones((1, 5)), log10_A=A, gamma=g), dict(log10_A=A)):
        with pytest.raises(ValueError):
            lnl.make_grid(f, **bad)
    grid, axes = lnl.make_grid(f, log10_A=A, gamma=g)
    assert grid.shape == (6, 5) and axes[0] is not None


def test_set_likelihood_grid_argument_checks_need_no_device():
    from fakepta_amd.batch import BatchSimulator
    psrs = [H._Psr(5, [1, 0, 0]), H._Psr(7, [0.3, 1, 0], t1=2e8), H._Psr(6, [0.2, 0.1, 1])]

    class Ctx(H._RecordingCtx):
        def __getattr__(self, name):
            def call(*a, **k):
                self.calls.append((name, a, k))
                if name == "batch_set_lnl":
                    return np.full(self.P, 3, dtype=np.int32), np.ones((self.P, len(a[6])))
                if name == "batch_lnl":
                    G = len(self.calls_of("batch_set_lnl")[-1][1][6])
                    return np.ones((G, 4)), (np.ones((self.P, G, 4)) if k.get("per_pulsar") else None), None
            return call

    ctx = Ctx(len(psrs))
    sim = BatchSimulator(psrs, signals=[], white=False, ctx=ctx)
    with pytest.raises(ValueError, match="no likelihood grid"):
        sim.likelihood_grid()
    with pytest.raises(ValueError, match="0 common signals"):
        sim.set_likelihood_grid(log10_A=[-14.0], gamma=[3.0])
    fc = np.array([1e-8, 2e-8, 3e-8])
    sim.segments.append(dict(name="red_noise", kind=0, f=np.array([[1e-8, 2e-8]] * 3), amp=np.full((3, 2), 1e-7),
                             idx=0.0, freqf=1400.0, mask=None))
    sim.segments.append(dict(name="gw_common", kind=1, f=fc, amp=np.array([3e-7, 2e-7, 1e-7]), idx=0.0, freqf=1400.0,
                             mask=None))
    n0 = len(ctx.calls)
    for bad in (dict(), dict(phi=np.ones((2, 2))), dict(phi=-np.ones((2, 3))), dict(phi=np.ones((1, 3)), gamma=[3.0]),
                dict(log10_A=[-14.0]), dict(log10_A=[-14.0], gamma=[3.0], Mmats="design"),
                dict(log10_A=[-14.0], gamma=[3.0], noise="model"), dict(log10_A=[-14.0], gamma=[3.0], target=7)):
        with pytest.raises(ValueError):
            sim.set_likelihood_grid(**bad)
    assert len(ctx.calls) == n0  # refused before anything reached the context
    rank = sim.set_likelihood_grid(log10_A=[-14.0, -13.0], gamma=[3.0, 4.0, 5.0])
    name, a, k = ctx.calls[-1]
    assert name == "batch_set_lnl" and list(a[0]) == [2, 3] and a[5] == 1 and a[6].shape == (6, 3) and len(rank) == 3
    assert k["M"].shape == (18, 3) and k["weights"].shape == (18,)
    out = sim.likelihood_grid(per_pulsar=True, posterior=True)
    assert out["dlnL"].shape == (2, 3, 4) and out["lnB"].shape == (4,) and out["dlnL_psr"].shape == (3, 6, 4)
    assert out["posterior"].shape == (2, 3, 4) and len(out["argmax"]) == 2
    sim.set_likelihood_grid(target="red_noise", phi=np.ones((2, 2)), Mmats=None, weights=None)
    name, a, k = ctx.calls_of("batch_set_lnl")[-1]
    assert a[5] == 0 and a[6].shape == (2, 2) and k["M"].shape == (18, 0) and k["weights"] is None
    assert sim.likelihood_grid()["dlnL"].shape == (2, 4)


# ----------------------------------------------------------------------------- a statement of the definition
# The 3 x 3 grid around the injected (log10_A, gamma) = (-13.6, 13 / 3): log10_A +- 0.15, gamma +- 1.0. With these
# spacings the longdouble reference puts the realization mean of dlnL at the true point for each of the seeds 1 .. 5
# (the margins to the runner-up are printed); the test runs seed 4, the seed of test_os_host's unbiasedness test.
STATEMENT_DA, STATEMENT_DG, STATEMENT_SEED, STATEMENT_R = 0.15, 1.0, 4, 2048


def statement_means(seed):
    from fakepta_amd import lnl
    from oracle import fakepta_oracle as O
    lay = H.unbiased_layout(identity=True)
    res = O.batch_synth(lay["offs"], lay["toas"], lay["nu"], lay["segs"], seed, 0, STATEMENT_R, sigma=lay["sigma"])
    A = -13.6 + STATEMENT_DA * np.arange(-1, 2)
    gam = 13 / 3 + STATEMENT_DG * np.arange(-1, 2)
    grid = lnl.powerlaw_grid(lay["f_gw"], A, gam)
    np.testing.assert_allclose(grid[4], lay["amp_gw"] ** 2, rtol=1e-12)  # the centre is the injected spectrum
    if "per" not in _TRUTH:
        per = []
        for p in range(len(lay["offs"]) - 1):
            sl = slice(int(lay["offs"][p]), int(lay["offs"][p + 1]))
            B, Z, norms, keep = LR.base_operator(lay["toas"][sl], lay["nu"][sl], lay["Mmats"][p],
                                                 1 / lay["sigma"][sl] ** 2, lay["comps_of"](p), lay["phis_of"](p), 1)
            T.assert_clear_rank(norms, keep, lay["Mmats"][p])
            Ut, ldt, _ = LR.grid_truth(Z, grid)
            per.append((B, Ut, ldt))
        _TRUTH["per"] = per
    per = _TRUTH["per"]
    X, _ = OS.x_truth([q[0] for q in per], lay["offs"], res)
    d, _, _, _ = LR.dlnl([q[1] for q in per], [q[2] for q in per], list(X))
    return np.mean(d, axis=1).astype(np.float64), np.std(d.astype(np.float64), axis=1) / np.sqrt(STATEMENT_R)


def test_the_mean_likelihood_ratio_peaks_at_the_injected_spectrum():
    """2048 oracle realizations of test_os_host's 8-pulsar layout with the common process drawn uncorrelated at the
    injected spectrum: the realization mean of dlnL over the 3 x 3 grid (log10_A +- 0.15, gamma +- 1.0) is largest at
    the centre, and positive there (the process is in the data)."""
    mean, se = statement_means(STATEMENT_SEED)
    order = np.argsort(mean)
    print(f"mean dlnL = {np.array2string(mean.reshape(3, 3), precision=3)}, centre - runner-up = "
          f"{mean[4] - mean[order[-2]]:.3f}, standard error of the centre {se[4]:.3f}")
    assert order[-1] == 4 and mean[4] > 0
