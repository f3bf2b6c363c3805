"""Optimal statistic under a spectrum per realization, host side (no GPU): csrc/os_spectra_host.h (validation and the
per-pulsar plan B0_p = T_p^T P0_p^-1, A_p = B0_p T_p) in a stand-alone C++ program built with the address and
undefined-behaviour sanitizers, against the np.longdouble definition of tests/os_spectra_reference.py; the C-ABI
surface; the argument checks and the host algebra of fakepta_amd that need no device; and the unbiasedness of the
per-realization definition on the oracle's draws, with the seed the GPU test uses."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import os_reference as OS
from tests import os_spectra_reference as SR
from tests import tm_reference as T
from tests import test_os_host as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fakepta_amd.h")
LIB = os.path.join(ROOT, "fakepta_amd", "lib", "libfakepta_amd.so")
CSRC = os.path.join(ROOT, "fakepta_amd", "csrc")
ENTRY_POINTS = ("fpta_batch_set_os_spectra", "fpta_batch_os_spectra")
EPS = np.finfo(np.float64).eps
LD = np.longdouble

# argv: in out. in: int64 P, n_col, C, target, has_mask, f_common, n_vary; offs [P + 1]; ncol [P]; n_modes [C]; vary
# [n_vary]; then fp64 idx [C], freqf [C], f [rows][sum N], phi [P][sum N], phi_hat [N], t [n], nu [n], M [n][n_col],
# w [n]; then uint8 mask [C][n] (has_mask). out: fp64 B0 [q n], A [P][q][q], rank [P], rows [P]. Without arguments:
# the checks that need no data.
_MAIN = r"""
#include <cstdio>
#include <cstring>
#include "os_spectra_host.h"
using namespace fpta_oss;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)
struct Case {
  int64_t P = 3;
  int64_t offs[4] = {0, 9, 9, 20};  // the middle pulsar has no TOAs
  std::vector<double> t, nu, M, w, f, idx, freqf, phi, phi_hat, G;
  std::vector<int32_t> n_modes, vary;
  int64_t n_col = 2;
  Spec sp;
  Case() : t(20), nu(20, 1400.0), M(20 * 2, 1.0), w(20, 2.0), f{1e-8, 2e-8, 3e-8, 1e-8, 2e-8}, idx{0.0, 0.0, 2.0},
           freqf{1400.0, 1400.0, 1400.0}, phi(3 * 5, 1e-2), phi_hat{1.0, 0.5}, G(9, 0.25), n_modes{2, 1, 2}, vary{0, 2} {
    for (int i = 0; i < 20; ++i) {
      t[i] = 1e7 * (i + 1) + 3e5 * i * i;
      M[2 * i + 1] = (double)i;
      nu[i] = i % 2 ? 1400.0 : 800.0;
    }
    spec();
  }
  Spec& spec() {
    sp.os.comps.n_comp = (int32_t)n_modes.size();
    sp.os.comps.n_modes = n_modes.data();
    sp.os.comps.f = f.data();
    sp.os.comps.f_is_common = true;
    sp.os.comps.idx = idx.data();
    sp.os.comps.freqf = freqf.data();
    sp.os.phi = phi.data();
    sp.os.mask = nullptr;
    sp.os.target = 2;
    sp.os.phi_hat = phi_hat.data();
    sp.n_vary = (int32_t)vary.size();
    sp.vary = vary.data();
    return sp;
  }
  bool ok(std::string& why) {
    return validate(P, offs, t.data(), nu.data(), sp, n_col, M.data(), nullptr, w.data(), 1, G.data(), why);
  }
  bool refused(const char* expect) {
    std::string why;
    const bool good = ok(why);
    std::printf("validate: %s\n", good ? "ok" : why.c_str());
    return !good && why.find(expect) != std::string::npos;
  }
};
static int self_checks() {
  std::string why;
  { Case c; CHECK(c.ok(why)); }
  // what os_host.h's validate refuses comes through with its messages
  { Case c; c.phi[4] = -1.0; CHECK(c.refused("prior variance is negative or not finite")); }
  { Case c; c.w[3] = 0.0; CHECK(c.refused("weight")); }
  { Case c; c.phi_hat[0] = 0.0; CHECK(c.refused("template is not positive and finite")); }
  // the varied set
  { Case c; c.vary.clear(); c.spec(); CHECK(c.refused("0 varied components outside [1, 4]")); }
  { Case c; c.vary = {0, 1, 0, 1, 2}; c.spec(); CHECK(c.refused("5 varied components outside [1, 4]")); }
  { Case c; c.vary = {0, 3}; c.spec(); CHECK(c.refused("varied component 3 outside [0, 3)")); }
  { Case c; c.vary = {2, 2}; c.spec(); CHECK(c.refused("varied component 2 named twice")); }
  { Case c; c.vary = {2, 0}; c.spec(); CHECK(c.refused("the target component 2 must be the last of the varied set")); }
  { Case c; c.vary = {2}; c.spec(); CHECK(c.ok(why)); }
  { Case c; c.vary = {0, 1, 2}; c.spec(); CHECK(c.ok(why)); }
  // q = 130 refused by name, q = 128 accepted
  { Case c; c.n_modes = {35, 1, 30}; c.f.assign(66, 1e-8); c.phi.assign(3 * 66, 1.0); c.phi_hat.assign(30, 1.0); c.spec();
    CHECK(c.refused("the varied set has 130 Fourier columns, more than 128")); }
  { Case c; c.n_modes = {34, 1, 30}; c.f.assign(65, 1e-8); c.phi.assign(3 * 65, 1.0); c.phi_hat.assign(30, 1.0); c.spec();
    CHECK(c.ok(why)); }
  // the plan of an array: a pulsar without TOAs has no rows and A = 0; A is symmetric; the prior variances of the
  // varied components do not enter; the offset is marginalised (every row of B0 sums to zero against it)
  {
    Case c;
    Plan plan, other;
    CHECK(make_plan(c.P, c.offs, c.t.data(), c.nu.data(), c.sp, c.n_col, c.M.data(), nullptr, c.w.data(), 0.0, 1,
                    c.G.data(), plan, why) == 0);
    CHECK(plan.q == 8 && plan.K == 4 && plan.N == 2 && plan.B0.size() == 8 * 20 && plan.A.size() == 3 * 64);
    CHECK(plan.rows[0] == 8 && plan.rows[1] == 0 && plan.rows[2] == 8 && plan.max_rows == 8);
    CHECK(plan.rank[0] == 2 && plan.rank[1] == 0 && plan.rank[2] == 2);
    for (int i = 0; i < 64; ++i) CHECK(plan.A[64 + i] == 0.0);
    for (int p : {0, 2})
      for (int i = 0; i < 8; ++i) {
        CHECK(plan.A[p * 64 + i * 8 + i] > 0.0);
        for (int j = 0; j < i; ++j) CHECK(plan.A[p * 64 + i * 8 + j] == plan.A[p * 64 + j * 8 + i]);
      }
    for (int j = 0; j < 8; ++j) {
      long double s = 0.0L, a = 0.0L;
      for (int i = 0; i < 9; ++i) { s += plan.B0[j * 9 + i]; a += std::fabs(plan.B0[j * 9 + i]); }
      CHECK(std::fabs((double)s) <= 1e-13 * (double)a);
    }
    c.phi[0] = 7.0; c.phi[4] = 0.0;  // varied entries
    CHECK(make_plan(c.P, c.offs, c.t.data(), c.nu.data(), c.sp, c.n_col, c.M.data(), nullptr, c.w.data(), 0.0, 1,
                    c.G.data(), other, why) == 0);
    CHECK(other.B0 == plan.B0 && other.A == plan.A);
    c.phi[2] = 3.0;  // a fixed entry
    CHECK(make_plan(c.P, c.offs, c.t.data(), c.nu.data(), c.sp, c.n_col, c.M.data(), nullptr, c.w.data(), 0.0, 1,
                    c.G.data(), other, why) == 0);
    CHECK(other.A != plan.A);
    c.w[2] = 0.0;
    CHECK(make_plan(c.P, c.offs, c.t.data(), c.nu.data(), c.sp, c.n_col, c.M.data(), nullptr, c.w.data(), 0.0, 1,
                    c.G.data(), other, why) == 1 && why.find("weight") != std::string::npos);
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
  const int64_t P = hdr[0], n_col = hdr[1], C = hdr[2], n_vary = hdr[6];
  std::vector<int64_t> offs((size_t)P + 1), ncol64((size_t)P), nm64((size_t)C), vary64((size_t)n_vary);
  if (!rd(in, offs) || !rd(in, ncol64) || !rd(in, nm64) || !rd(in, vary64)) return 2;
  std::vector<int32_t> ncol(ncol64.begin(), ncol64.end()), nm(nm64.begin(), nm64.end()), vary(vary64.begin(), vary64.end());
  int64_t nf = 0;
  for (int64_t v : nm64) nf += v;
  const int64_t n = offs[(size_t)P], N = nm64[(size_t)hdr[3]];
  std::vector<double> idx((size_t)C), ff((size_t)C), f((size_t)((hdr[5] ? 1 : P) * nf)), phi((size_t)(P * nf)),
      phi_hat((size_t)N), t((size_t)n), nu((size_t)n), M((size_t)(n * n_col)), w((size_t)n);
  std::vector<uint8_t> mask((size_t)(hdr[4] ? C * n : 0));
  if (!rd(in, idx) || !rd(in, ff) || !rd(in, f) || !rd(in, phi) || !rd(in, phi_hat) || !rd(in, t) || !rd(in, nu) ||
      !rd(in, M) || !rd(in, w) || !rd(in, mask))
    return 2;
  std::fclose(in);
  Spec sp;
  sp.os.comps.n_comp = (int32_t)C; sp.os.comps.n_modes = nm.data(); sp.os.comps.f = f.data();
  sp.os.comps.f_is_common = hdr[5] != 0; sp.os.comps.idx = idx.data(); sp.os.comps.freqf = ff.data();
  sp.os.phi = phi.data(); sp.os.mask = hdr[4] ? mask.data() : nullptr; sp.os.target = (int32_t)hdr[3];
  sp.os.phi_hat = phi_hat.data(); sp.n_vary = (int32_t)n_vary; sp.vary = vary.data();
  Plan plan;
  std::string why;
  const int made = make_plan(P, offs.data(), t.data(), nu.data(), sp, n_col, M.data(), ncol.data(), w.data(), 0.0, 0,
                             nullptr, plan, why);
  if (made) { std::printf("make_plan: %d %s\n", made, why.c_str()); return 3; }
  if ((int64_t)plan.B0.size() != plan.q * n) return 4;
  std::vector<double> rank(plan.rank.begin(), plan.rank.end()), rows(plan.rows.begin(), plan.rows.end());
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  for (const std::vector<double>* v : {&plan.B0, &plan.A, &rank, &rows})
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
    d = tmp_path_factory.mktemp("os_spectra_host")
    (d / "main.cpp").write_text(_MAIN)
    exe = str(d / "os_spectra_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-pthread", "-I", CSRC, str(d / "main.cpp"), "-o", exe], check=True)
    return exe


def test_host_planner_under_the_sanitizers(host_exe):
    """Every validation message of the varied set (empty, five, out of range, repeated, the target not last, q = 130
    refused by name and 128 accepted), what os_host.h refuses, a pulsar without TOAs, the symmetry of A, and that the
    varied components' prior variances do not enter the plan while a fixed one does."""
    r = subprocess.run([host_exe], capture_output=True, text=True)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("all ok"), r.stdout[-6000:] + r.stderr[-4000:]


def arrays():
    """The arrays of the host tests (tests/test_os_host.py's, with a varied set): q4: 17 TOAs, no TOAs, and 40 TOAs
    whose design repeats a column, a red process fixed and a target of 2 modes varied; q18: 33 and 60 TOAs, a masked
    system-noise component in the fixed set, the red process fixed, the target of 9 modes varied (one of its modes has
    phi = 0 for the first pulsar); q120: 250 TOAs under a red process 1e4 x the white level and 600 under one 1e-4 x it,
    a chromatic component fixed, red process and target (30 + 30 modes) varied."""
    base = H.arrays()
    n4 = dict(base["N4"])
    n4["comps"] = [base["N4"]["comps"][0], (base["N4"]["comps"][1][0][:2], 0.0, 1400.0)]
    n4["phis"] = [base["N4"]["phis"][0], base["N4"]["phis"][1][:, :2]]
    return {"q4": dict(n4, vary=[1]), "q18": dict(base["N9"], vary=[2]), "q120": dict(base["N30"], vary=[0, 2])}


def run_host(host_exe, tmp_path, arr):
    offs, toas, nu, Mmats, w, _, _, _ = H.array_tables(arr)
    P, n = len(offs) - 1, int(offs[-1])
    n_col = max(M.shape[1] for M in Mmats)
    Mfull = np.zeros((n, n_col))
    for p, M in enumerate(Mmats):
        Mfull[offs[p]:offs[p + 1], :M.shape[1]] = M
    common = all(np.ndim(c[0]) == 1 for c in arr["comps"])
    fs = [np.asarray(c[0]) if common or np.ndim(c[0]) == 2 else np.tile(c[0], (P, 1)) for c in arr["comps"]]
    n_modes = [f.shape[-1] for f in fs]
    phi_hat = np.asarray(arr["phis"][arr["target"]])[-1]
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.array([P, n_col, len(fs), arr["target"], 0 if arr["masks"] is None else 1, 1 if common else 0,
                           len(arr["vary"])] + list(offs) + [M.shape[1] for M in Mmats] + n_modes + list(arr["vary"]),
                          dtype=np.int64).tobytes())
        for a in ([c[1] for c in arr["comps"]], [c[2] for c in arr["comps"]], np.concatenate(fs, axis=-1),
                  np.concatenate(arr["phis"], axis=-1), phi_hat, toas, nu, Mfull, w):
            fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        if arr["masks"] is not None:
            fh.write(np.stack([np.ones(n, dtype=np.uint8) if m is None else m for m in arr["masks"]]).tobytes())
    r = subprocess.run([host_exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    body = np.frombuffer(open(tmp_path / "out.bin", "rb").read(), dtype=np.float64)
    q = 2 * sum(n_modes[c] for c in arr["vary"])
    o = [q * n, q * n + P * q * q, q * n + P * q * q + P]
    B0 = [body[q * offs[p]:q * offs[p + 1]].reshape(q, -1) for p in range(P)]
    return B0, body[o[0]:o[1]].reshape(P, q, q), body[o[1]:o[2]].astype(int), body[o[2]:o[2] + P].astype(int)


# |B0 - B0_truth| per entry in eps of the row's largest entry, the largest over the rows of a pulsar, as measured: q4
# 0.340 / no TOAs / 0.367, q18 0.458 / 0.444, q120 0.459 / 0.471 (the rounding to fp64 is the whole error). The bound:
# 4 x the largest of them, floor 1 eps.
B0_MEASURED_EPS = 0.471
B0_BOUND_EPS = max(4 * B0_MEASURED_EPS, 1.0)


@pytest.mark.parametrize("name", ["q4", "q18", "q120"])
def test_plan_matches_the_longdouble_definition(host_exe, tmp_path, name):
    """B0_p to 4 x the measured rounding per entry relative to its row's largest entry, A_p to the dot-product bound
    (n + 2) eps sum_t |B0_it| |T_tj| and exactly symmetric, the kept columns of M; and the truth itself is the
    definition: B0 M^ = 0 and B0 P0 = T^T off the span of M, in longdouble products without an inverse."""
    arr = arrays()[name]
    offs, toas, nu, Mmats, w, comps_of, phis_of, masks_of = H.array_tables(arr)
    P, vary = len(offs) - 1, arr["vary"]
    B0, A, rank, rows = run_host(host_exe, tmp_path, arr)
    q = A.shape[1]
    for p in range(P):
        sl = slice(int(offs[p]), int(offs[p + 1]))
        n = sl.stop - sl.start
        assert rows[p] == (q if n else 0)
        if n == 0:
            assert np.all(A[p] == 0) and rank[p] == 0
            continue
        Bt, At, norms, keep = SR.plan_ld(toas[sl], nu[sl], Mmats[p], w[sl], comps_of(p), phis_of(p), vary, masks_of(p))
        T.assert_clear_rank(norms, keep, Mmats[p])
        assert rank[p] == int(keep.sum())
        row_max = np.max(np.abs(Bt), axis=1, keepdims=True)
        live = row_max[:, 0] > 0
        err = float(np.max(np.abs(B0[p].astype(LD) - Bt)[live] / row_max[live])) / EPS
        Tm = SR.varied_columns(toas[sl], nu[sl], comps_of(p), vary, masks_of(p))
        ab = (n + 2) * EPS * (np.abs(Bt) @ np.abs(Tm)).astype(np.float64)
        a_err = np.abs(A[p].astype(LD) - At).astype(np.float64)
        print(f"{name} pulsar {p} (n = {n}, q = {q}): |B0 - B0_ld| <= {err:.3f} eps of the row's largest entry, "
              f"|A - A_ld| <= {float(np.max(a_err / np.maximum(ab, 1e-300))):.3g} of its bound")
        assert err <= B0_BOUND_EPS
        assert np.all(a_err <= ab) and np.all(A[p] == A[p].T)
        ph0 = SR.zeroed(phis_of(p), vary)
        r0 = 0
        for c in vary:
            Kc = 2 * len(comps_of(p)[c][0])
            bm, dres = OS.definition_residual(toas[sl], nu[sl], Mmats[p], w[sl], comps_of(p), ph0, c, keep,
                                              Bt[r0:r0 + Kc], masks_of(p))
            r0 += Kc
            print(f"{name} pulsar {p} component {c}: the truth's |B0 M| <= {bm:.3g} |B0|, |B0 P0 - T^T| off the span "
                  f"of M <= {dres:.3g}")
            assert bm <= 1e-9 and dres <= 1e-9


def test_abi_declares_exports_and_binds_the_entry_points():
    from fakepta_amd import _capi
    text = open(HEADER).read()
    lib = ctypes.CDLL(LIB)
    for name in ENTRY_POINTS:
        assert re.search(rf"^int\s+{name}\s*\(", text, flags=re.M), name
        assert hasattr(lib, name) and name in _capi.EXPORTED
    for method in ("batch_set_os_spectra", "batch_os_spectra"):
        assert hasattr(_capi.Context, method)
    host = open(os.path.join(CSRC, "os_spectra_host.h")).read()
    assert "#include <hip" not in host and "__global__" not in host and "__device__" not in host  # plain C++
    assert '#include "os_host.h"' in host and "fpta_os::build_operator" in host  # shared, not forked
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "os_spectra.hip" in make and "os_spectra_host.h" in make
    dev = open(os.path.join(CSRC, "os_spectra.hip")).read()
    assert "k_fit_apply<" not in dev and "fit_launch_unbooked" in dev and "os_pairs_launch" in dev
    assert "spectra_table" in dev and "fpta_spec::validate" in dev  # the tables and their validation are synth's


def _sim():
    from fakepta_amd.batch import BatchSimulator
    psrs = [H._Psr(5, [1, 0, 0]), H._Psr(7, [0.3, 1, 0], t1=2e8), H._Psr(6, [0.2, 0.1, 1])]
    ctx = H._RecordingCtx(len(psrs))
    sim = BatchSimulator(psrs, signals=[], white=False, ctx=ctx)
    for i, (name, kind, n) in enumerate((("red_noise", 0, 2), ("dm_gp", 0, 60), ("gw_common", 1, 3))):
        f = np.arange(1, n + 1) * 1e-8
        sim.segments.append(dict(name=name, kind=kind, f=np.tile(f, (3, 1)) if kind == 0 else f,
                                 amp=np.full((3, n) if kind == 0 else n, 1e-7), idx=0.0, freqf=1400.0, mask=None, id=i))
    return sim, ctx


def test_argument_checks_need_no_device_and_leave_the_state():
    """q = 130, a table for a signal outside the varied set, a non-finite and a negative row are refused by name
    before anything reaches the context, and what was set stays set."""
    sim, ctx = _sim()
    with pytest.raises(ValueError, match="no statistic is set"):
        sim.optimal_statistic_spectra()
    n0 = len(ctx.calls)
    with pytest.raises(ValueError, match="130 Fourier columns, more than 128"):
        sim.set_optimal_statistic_spectra(["red_noise", "dm_gp"])  # 2 (2 + 60 + 3)
    with pytest.raises(ValueError, match="must name one signal"):
        sim.set_optimal_statistic_spectra(["chrom_gp"])
    assert len(ctx.calls) == n0 and sim._oss is None
    sim.set_optimal_statistic_spectra("red_noise", orfs=("hd", "monopole"), bins=2)
    name, a, k = ctx.calls[-1]
    assert name == "batch_set_os_spectra" and list(a[0]) == [2, 60, 3] and a[5] == 2
    assert list(a[7]) == [0, 2] and list(a[8]) == [0, 2] and a[9].shape == (4, 3, 3) and a[10] == 2
    state = dict(sim._oss)
    n1 = len(ctx.calls)
    ctx.batch_device_out = lambda: (None, None, 4)
    good = np.full((4, 3, 2), 1e-7)
    for spec, msg in (({"dm_gp": dict(amp=np.full((4, 3, 60), 1e-7))}, r"spectra\['dm_gp'\]: the signal is not in the varied"),
                      ({"red_noise": dict(amp=np.where(np.arange(4)[:, None, None] == 2, np.nan, good))},
                       "realization 2, pulsar 0, mode 0: non-finite amplitude"),
                      ({"red_noise": dict(amp=np.where(np.arange(4)[:, None, None] == 1, -good, good))},
                       "realization 1, pulsar 0, mode 0: negative amplitude"),
                      ({"gw_common": dict(log10_A=np.array([-14.0, np.inf, -14.0, -14.0]), gamma=4.0)},
                       "realization 1: non-finite log10_A"),
                      ({"red_noise": dict(amp=good[:3])}, "3 rows for 4 realizations")):
        with pytest.raises(ValueError, match=msg):
            sim.optimal_statistic_spectra(spec)
    assert len(ctx.calls) == n1 and sim._oss == state
    # the target alone; it is added when it is not named, and named last
    sim.set_optimal_statistic_spectra([], target="gw_common")
    assert list(ctx.calls[-1][1][7]) == [2]
    sim.set_optimal_statistic_spectra(["gw_common", "red_noise"])
    assert list(ctx.calls[-1][1][7]) == [0, 2]


def test_per_realization_host_algebra_on_numbers_built_by_hand():
    from fakepta_amd import os as osm
    nab = np.array([[[0, 0, 0], [2.0, 0, 0], [3.0, 5.0, 0]], [[9.0, 0, 0], [4.0, 9.0, 0], [6.0, 10.0, 9.0]]])
    g1 = np.array([[0, 1.0, 2.0], [1.0, 0, -1.0], [2.0, -1.0, 0]])
    Gs = np.stack([g1, np.ones((3, 3)) - np.eye(3), np.zeros((3, 3))])
    sym = osm.symmetric_pair_norms(nab)
    assert np.all(sym == sym.transpose(0, 2, 1)) and np.all(sym[:, range(3), range(3)] == 0) and sym[1, 0, 2] == 6.0
    norm = osm.norms_per_realization(Gs, sym)
    np.testing.assert_allclose(norm, [[19.0, 38.0], [10.0, 20.0], [0.0, 0.0]], rtol=1e-15)
    np.testing.assert_allclose(norm[:, 0], osm.norms(Gs, sym[0]), rtol=1e-15)
    joint = osm.joint_matrix_per_realization(Gs[:2], sym)
    np.testing.assert_allclose(joint[:, :, 0], osm.joint_matrix(Gs[:2], sym[0]), rtol=1e-15)
    np.testing.assert_allclose(joint[:, :, 1], 2 * joint[:, :, 0], rtol=1e-15)
    A = np.array([[2.0, -1.0], [0.5, 3.0]])
    Q = np.concatenate([np.stack([joint[:, :, r] @ A[:, r] for r in range(2)], axis=1), [[4.0, 1.0]]])
    out = osm.derive_per_realization(Q, norm, joint, 2, np.array([0.5]), np.array([0]), nab=nab)
    np.testing.assert_allclose(out["A2_joint"], A, rtol=1e-13)
    np.testing.assert_allclose(out["A2"], Q[:2] / norm[:2], rtol=1e-15)
    np.testing.assert_allclose(out["snr"], Q[:2] / np.sqrt(norm[:2]), rtol=1e-15)
    assert np.all(np.isnan(out["rho_bins"])) and np.all(out["N_ab"] == sym)  # a bin without weight: NaN there
    # a denominator that is 0 in one realization only is NaN there only
    norm2, joint2 = norm.copy(), joint.copy()
    norm2[0, 1], joint2[:, :, 1] = 0.0, 0.0
    out = osm.derive_per_realization(Q, norm2, joint2, 2)
    assert np.isnan(out["A2"][0, 1]) and np.isfinite(out["A2"][0, 0]) and np.isfinite(out["A2"][1, 1])
    assert np.all(np.isnan(out["A2_joint"][:, 1])) and np.all(np.isfinite(out["A2_joint"][:, 0]))


# ----------------------------------------------------------------------------- unbiasedness under each row's truth
def test_the_per_realization_definition_is_unbiased_with_the_gpu_tests_seed():
    """The end-to-end GPU test's condition, with the reference alone: the oracle's draws of the unbiasedness layout with
    log10_A of both processes drawn per realization over a decade (tests/spectra_reference.py), the longdouble truth
    of every realization under its own spectrum, and the mean of A2_r phi_hat / phi_r within 3 standard errors of 1."""
    from oracle import fakepta_oracle as O
    from tests import spectra_reference as SPR
    from tests.test_gpu_os_spectra import E2E_SEED, E2E_R, e2e_spectra
    lay = H.unbiased_layout()
    offs, P, R = lay["offs"], len(lay["offs"]) - 1, E2E_R
    spec = e2e_spectra(lay, R)
    df_rn = np.diff(np.concatenate([np.zeros((P, 1)), lay["f_rn"]], 1), axis=1)
    amp_rn = np.sqrt(O.powerlaw(lay["f_rn"][None], spec["red_noise"]["log10_A"][:, :, None], 3.0) * df_rn[None])
    amp_gw = np.sqrt(O.powerlaw(lay["f_gw"][None], spec["gw_common"]["log10_A"][:, None], 13 / 3) *
                     O.delta_f(lay["f_gw"])[None])
    res = SPR.synth(offs, lay["toas"], lay["nu"], lay["segs"], E2E_SEED, 0, R, {0: amp_rn, 1: amp_gw})
    res = res + O.batch_synth(offs, lay["toas"], lay["nu"], [], E2E_SEED, 0, R, sigma=lay["sigma"])
    G = O.orf_hd(lay["pos"])
    np.fill_diagonal(G, 0.0)
    phi_hat = lay["amp_gw"] ** 2
    a2 = np.zeros(R)
    for r in range(R):
        Bs, Zs = [], []
        for p in range(P):
            sl = slice(int(offs[p]), int(offs[p + 1]))
            B, Z, _, _ = OS.operator_ld(lay["toas"][sl], lay["nu"][sl], lay["Mmats"][p], 1 / lay["sigma"][sl] ** 2,
                                        lay["comps_of"](p), [amp_rn[r, p] ** 2, amp_gw[r] ** 2], 1)
            Bs.append(B)
            Zs.append(Z)
        X, _ = OS.x_truth(Bs, offs, res[r])
        Qm, _, _ = OS.q_truth(X.astype(np.float64), phi_hat, G[None])
        nab = OS.pair_norms(Zs, phi_hat)[0]
        il = np.tril_indices(P, -1)
        a2[r] = float(Qm.sum(axis=1)[0, 0] / np.sum(G[il].astype(LD) ** 2 * nab[il]))
    y = a2 * 10.0 ** (2 * (-13.6 - spec["gw_common"]["log10_A"]))
    se = np.std(y) / np.sqrt(R)
    print(f"mean A2_r phi_hat / phi_r = {np.mean(y):.4f}, standard error {se:.4f}: {(np.mean(y) - 1) / se:.2f} of them")
    assert abs(np.mean(y) - 1.0) <= 3 * se
