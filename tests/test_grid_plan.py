"""The gridded path's planner (csrc/grid_plan.h, plain C++ shared with grid_host.hip and the kernels), run on the CPU.
A stand-alone program reads small layouts, plans them and prints every table; a deliberately naive numpy model, written
from the definitions in the header's comments, recomputes each table: integer tables must agree exactly, the double
tables (d, beta, ecos, esin, tq) to 1e-12 relative (libm against numpy on the same formulas and a 256-point
Gauss-Legendre sum of O(1) terms). The invariants the kernels' unconditional loads rely on are asserted directly. The
program is built with the address and undefined-behaviour sanitizers, and a second time with -DFPTA_DIAG_KERNELS, where
the diagnostic kernels' plans (csrc/diag/grid_plan_diag.h) get invariant checks."""
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import grid_model
from tests.grid_model import bound, chrom_weight, model_groups, model_sizes, model_tables, w0_rows  # noqa: F401

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fakepta_amd", "csrc")

# the planning constants of grid_plan.h (the program prints them; test_constants compares)
TT, ROW_CAP, VMAX, MIN_V, MAX_SEG, DFT_ROWS, GEN_TERMS = 32, 48, 256, 16, 16, 32, 8
F_MAX_SIG, F_PITCH, F_SLOT, F_DW, F_LDS_MAX, F_FQ_MIN, F_PAD_ROWS, F_HALF_TT, F_HALF_NQ = (
    2, 32, 1024, 4, 160 * 1024, 16, 64, 16, 8)
WR_SLOTS, LDS_GROUP, LDS_ROWS_MAX, U_GROUP, U_ROWS_MAX, U_SIG_MAX = 32, 4, 144, 4, 76, 2

_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "grid_plan.h"
#ifdef FPTA_DIAG_KERNELS
#include "diag/grid_plan_diag.h"
#endif
using namespace fpta;
static FILE* in;
static long rdi() {
  long v;
  if (std::fscanf(in, "%ld", &v) != 1) std::exit(3);
  return v;
}
static double rdd() {  // hexadecimal floats: exact
  char buf[64];
  if (std::fscanf(in, "%63s", buf) != 1) std::exit(3);
  return std::strtod(buf, nullptr);
}
template <class T>
static void ints(const char* k, const std::vector<T>& v, const char* end = ",") {
  std::printf("\"%s\":[", k);
  for (size_t i = 0; i < v.size(); ++i) std::printf("%s%lld", i ? "," : "", (long long)v[i]);
  std::printf("]%s\n", end);
}
static void dbls(const char* k, const std::vector<double>& v) {
  std::printf("\"%s\":[", k);
  for (size_t i = 0; i < v.size(); ++i) std::printf("%s%.17g", i ? "," : "", v[i]);
  std::printf("],\n");
}
static void int4s(const char* k, const std::vector<Int4>& v) {
  std::vector<int32_t> f;
  for (const Int4& c : v) f.insert(f.end(), {c.x, c.y, c.z, c.w});
  ints(k, f);
}
int main(int argc, char** argv) {
  in = std::fopen(argv[1], "r");
  if (!in) return 2;
  const long n_layouts = rdi();
  std::printf("{\"constants\":[%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d],\n\"plans\":[\n", kGridTT, kGridRowCap,
              kGridVMax, kGridMinV, kGridMaxSeg, kGridDftRows, kDftGenTerms, kFusedMaxSig, kFusedPitch, kFusedSlot,
              kFusedDW, kFusedLdsMax, kFusedFqMin, kFusedPadRows, kFusedHalfTT, kFusedHalfNQ);
  for (long li = 0; li < n_layouts; ++li) {
    PlanOptions o;
    o.w = (int32_t)rdi();
    o.sigma = rdd();
    o.coalesce = rdi() != 0;
    o.grid_mfma = (int32_t)rdi();
    PlanLayout L;
    L.P = (int32_t)rdi();
    L.n_toa = rdi();
    std::vector<int64_t> offs(L.P + 1);
    for (int64_t& v : offs) v = rdi();
    // exact-size heap arrays: the address sanitizer sees a read past the last TOA
    std::vector<double> toas(L.n_toa), nu(L.n_toa);
    for (double& v : toas) v = rdd();
    for (double& v : nu) v = rdd();
    toas.shrink_to_fit();
    nu.shrink_to_fit();
    L.offs = offs.data();
    L.toas = toas.data();
    L.nu = nu.data();
    const long n_sig = rdi();
    std::vector<std::vector<double>> w0(n_sig);
    std::vector<std::vector<uint8_t>> mask(n_sig);
    for (long i = 0; i < n_sig; ++i) {
      PlanSignal s;
      s.kind = (int32_t)rdi();
      s.nm = (int32_t)rdi();
      s.idx = rdd();
      s.freqf = rdd();
      s.harmonic = (int32_t)rdi();
      w0[i].resize(rdi());
      for (double& v : w0[i]) v = rdd();
      if (rdi()) {
        mask[i].resize(L.n_toa);
        for (uint8_t& v : mask[i]) v = (uint8_t)rdi();
      }
      L.sigs.push_back(s);
    }
    for (long i = 0; i < n_sig; ++i) {
      L.sigs[i].w0 = w0[i].data();
      L.sigs[i].mask = mask[i].empty() ? nullptr : mask[i].data();
    }
    const HostGridPlan H = plan_grid(L, o);
    std::printf("%s{\"ok\":%d,\"why\":\"%s\",\"merges\":%d,\n", li ? "," : "", (int)H.ok, H.why.c_str(), (int)H.merges);
    std::printf("\"members\":[");
    for (size_t g = 0; g < H.members.size(); ++g) {
      std::printf("%s[", g ? "," : "");
      for (size_t i = 0; i < H.members[g].size(); ++i) std::printf("%s%d", i ? "," : "", H.members[g][i]);
      std::printf("]");
    }
    std::printf("],\n");
    ints("anchor", H.anchor);
    ints("last", H.last);
    std::printf("\"segs\":[");
    for (size_t s = 0; s < H.segs.size(); ++s) {
      const PlanSeg& g = H.segs[s];
      std::printf("%s{\"nm\":%d,\"nf\":%d,\"w\":%d,\"half\":%d,\"lde\":%d,\"ntab\":%d,\"ldq\":%d,\"ntq\":%d,\"beta\":%.17g,"
                  "\"rowoff\":%lld,\n", s ? "," : "", g.nm, g.nf, g.w, g.half, g.lde, g.ntab, g.ldq, g.ntq, g.beta,
                  (long long)g.rowoff);
      dbls("ecos", g.ecos);
      dbls("esin", g.esin);
      dbls("tq", g.tq);
      dbls("d", g.d);
      ints("row", g.row);
      ints("hrow_of", g.hrow_of);
      ints("band_lo", g.band_lo);
      ints("band_n", g.band_n, "}");
    }
    std::printf("],\n");
    int4s("chunks", H.chunks);
    ints("psr_chunk0", H.psr_chunk0);
    ints("chunk_of", H.chunk_of);
    ints("tt_of", H.tt_of);
    ints("rows", H.rows);
    ints("fused_lrow0", H.fused_lrow0);
    ints("frows", H.frows);
    int4s("hchunks", H.hchunks);
    ints("hrows", H.hrows);
    ints("hchunk_of", H.hchunk_of);
    ints("htt_of", H.htt_of);
    ints("hv", H.hv);
#ifdef FPTA_DIAG_KERNELS
    if (H.ok) {
      const DiagWindowPlan W = plan_diag_window(H);
      const DiagLdsPlan S = plan_diag_lds(H);
      const DiagUnionPlan U = plan_diag_union(H);
      std::vector<int32_t> wl;
      for (const Int2& e : W.list) wl.insert(wl.end(), {e.x, e.y});
      std::printf("\"wr_ok\":%d,\"lds_ok\":%d,\"lds_rows\":%d,\"u_ok\":%d,\n", (int)W.ok, (int)S.ok, S.lds_rows, (int)U.ok);
      int4s("wr_meta", W.meta);
      ints("wr_list", wl);
      ints("wr_slot", W.slot);
      int4s("lds_groups", S.groups);
      ints("lds_urows", S.urows);
      ints("lds_lrows", S.lrows);
      int4s("u_groups", U.groups);
      ints("u_urows", U.urows);
      ints("u_cbase", U.cbase);
      ints("u_wrow", U.wrow);
    }
#endif
    std::printf("\"vmax\":%d,\"grid_rows\":%lld,\"wd_size\":%zu,\"hwd_size\":%zu,\"fused_ok\":%d,\"fused_lds\":%zu,"
                "\"fused_fq\":%d,\"fused_half_ok\":%d,\"fused_hfq\":%d,\"fused_hvmax\":%d,\"fused_hnq\":%d,"
                "\"fused_half_gain\":%.17g,\"fma_interp_half\":%.17g,\"fma_direct\":%.17g,\"fma_grid\":%.17g,"
                "\"fma_interp\":%.17g,\"fma_dft\":%.17g,\"grid_vals\":%.17g,\"mean_v\":%.17g,\"weight_bytes\":%.17g,"
                "\"err_bound\":%.17g}\n", H.vmax, (long long)H.grid_rows, H.wd_size, H.hwd_size, (int)H.fused_ok,
                H.fused_lds, H.fused_fq, (int)H.fused_half_ok, H.fused_hfq, H.fused_hvmax, H.fused_hnq,
                H.fused_half_gain, H.fma_interp_half, H.fma_direct, H.fma_grid, H.fma_interp, H.fma_dft, H.grid_vals,
                H.mean_v, H.weight_bytes, H.err_bound);
  }
  std::printf("]}\n");
  return 0;
}
"""

# ------------------------------------------------------------------------------------------------ layouts
T0, TSPAN = 53000.0 * 86400.0, 10.0 * 365.25 * 86400.0
W0 = 2.0 * math.pi / TSPAN


def _sig(P, nm, kind=0, idx=0.0, freqf=1400.0, harmonic=1, w0=W0, mask=None):
    return dict(kind=kind, nm=nm, idx=idx, freqf=freqf, harmonic=harmonic,
                w0=np.full(P if kind == 0 else 1, w0), mask=mask)


def _layout(name, counts, sigs, rng, w=15, sigma=1.5, coalesce=1, const_nu=False, toas=None, span=1.0):
    """counts TOAs per pulsar, sorted uniform draws over that fraction of the span; radio frequencies from three
    receivers unless const_nu. sigs: a function of (P, n_toa) -> list of signals."""
    P, n = len(counts), int(sum(counts))
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    if toas is None:
        toas = np.concatenate([np.sort(T0 + span * TSPAN * rng.random(c)) for c in counts]) if n else np.zeros(0)
    nu = np.full(n, 1400.0) if const_nu else rng.choice([800.0, 1400.0, 2300.0], size=n)
    return dict(name=name, P=P, offs=offs, toas=np.asarray(toas, dtype=np.float64), nu=nu, sigs=sigs(P, n), w=w,
                sigma=sigma, coalesce=coalesce, grid_mfma=1)


def make_layouts():
    rng = np.random.default_rng(20240607)
    rn = lambda nm: (lambda P, n: [_sig(P, nm)])
    rn_dm = lambda P, n: [_sig(P, 30), _sig(P, 30, idx=2.0)]
    out = []
    # 1. chunk boundaries at global multiples of kGridTT (TOAs close enough that kGridRowCap cuts nothing)
    for n in (1, 31, 32, 33, 65):
        out.append(_layout(f"p1_n{n}", [n], rn(30), rng, span=0.02))
    # 2. an empty pulsar; the third pulsar's first chunk is cut short by the global-index rule
    out.append(_layout("p3_40_0_7", [40, 0, 7], rn(30), rng, span=0.02))
    out.append(_layout("p3_40_0_30", [40, 0, 30], rn(30), rng, span=0.02))
    # 3. mode counts: nm = 2 takes the max(n, 2 w + 2) floor
    for nm in (2, 30, 100):
        out.append(_layout(f"nm{nm}", [50, 20], rn(nm), rng))
    # 4. sparse TOAs against many modes: kGridRowCap cuts chunks before kGridTT TOAs
    out.append(_layout("sparse_nm100", [10, 12], rn(100), rng))
    # 5. coalescing
    out.append(_layout("rn_dm_mixed_nu", [40, 35], rn_dm, rng))
    out.append(_layout("rn_dm_const_nu", [40, 35], rn_dm, rng, const_nu=True))
    out.append(_layout("rn_common", [40, 35, 20], lambda P, n: [_sig(P, 30), _sig(P, 60, kind=1)], rng))
    out.append(_layout("rn_masked", [40, 35],
                       lambda P, n: [_sig(P, 30), _sig(P, 30, mask=(np.arange(n) % 3 != 0).astype(np.uint8))], rng))
    # 6. coalescing off
    out.append(_layout("rn_dm_const_nu_nocoalesce", [40, 35], rn_dm, rng, const_nu=True, coalesce=0))
    # 7. the fill rule: dense TOAs take (nf1, w1), the layouts above keep (nf0, w0)
    out.append(_layout("fill_dense", [700], rn(30), rng))
    # 8. refusals
    out.append(_layout("no_signals", [10], lambda P, n: [], rng))
    out.append(_layout("non_harmonic", [10], lambda P, n: [_sig(P, 30), _sig(P, 30, harmonic=0)], rng))
    out.append(_layout("too_many_signals", [10], lambda P, n: [_sig(P, 4, w0=W0 * (1 + i)) for i in range(17)], rng))
    out.append(_layout("phase_range", [3], rn(30), rng, toas=[T0, T0 + 1e7, 1e30]))
    out.append(_layout("vmax_exceeded", [40], lambda P, n: [_sig(P, 30) for _ in range(16)], rng, coalesce=0))
    # 9. k_grid_fused's plan
    out.append(_layout("three_signals", [40, 35],
                       lambda P, n: [_sig(P, 30), _sig(P, 30, idx=2.0), _sig(P, 30, idx=4.0)], rng))
    out.append(_layout("lds_exceeded", [40, 35], lambda P, n: [_sig(P, 100), _sig(P, 100, idx=2.0)], rng))
    out.append(_layout("c2_like", [70, 33, 40],
                       lambda P, n: [_sig(P, 30), _sig(P, 100, idx=2.0), _sig(P, 30, kind=1)], rng))
    # 10. more members than the fused kernel's DFT waves sum
    out.append(_layout("nine_members", [40], lambda P, n: [_sig(P, 30) for _ in range(9)], rng))
    return out


def write_layouts(layouts, path):
    def hx(v):
        return " ".join(float(x).hex() for x in v)
    with open(path, "w") as f:
        f.write(f"{len(layouts)}\n")
        for L in layouts:
            f.write(f"{L['w']} {float(L['sigma']).hex()} {L['coalesce']} {L['grid_mfma']}\n")
            f.write(f"{L['P']} {len(L['toas'])}\n{' '.join(str(int(v)) for v in L['offs'])}\n")
            f.write(hx(L["toas"]) + "\n" + hx(L["nu"]) + "\n" + f"{len(L['sigs'])}\n")
            for s in L["sigs"]:
                f.write(f"{s['kind']} {s['nm']} {float(s['idx']).hex()} {float(s['freqf']).hex()} {s['harmonic']} "
                        f"{len(s['w0'])} {hx(s['w0'])} ")
                f.write("0\n" if s["mask"] is None else "1 " + " ".join(str(int(v)) for v in s["mask"]) + "\n")


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """The layouts and the planner's output for them, product and -DFPTA_DIAG_KERNELS builds (two sanitizer compiles)."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("grid_plan")
    (tmp / "main.cpp").write_text(_MAIN)
    layouts = make_layouts()
    write_layouts(layouts, tmp / "layouts.txt")
    plans = {}
    for tag, defs in (("product", []), ("diag", ["-DFPTA_DIAG_KERNELS"])):
        exe = str(tmp / f"grid_plan_{tag}")
        subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", *defs, "-I", CSRC, str(tmp / "main.cpp"), "-o", exe], check=True)
        r = subprocess.run([exe, str(tmp / "layouts.txt")], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        plans[tag] = json.loads(r.stdout)
    return layouts, plans


# ------------------------------------------------------------------------------------------------ the numpy model
# chrom_weight, w0_rows, model_groups, model_sizes, bound and model_tables: tests/grid_model.py
def step_rows(band, n, fq):
    """[4][fq]: band row 4 q + j at [j][q]; rows past the band's n repeat band row 0."""
    return [band[4 * q + j] if 4 * q + j < n else band[0] for j in range(4) for q in range(fq)]


def model(L, diag=False):
    """The whole plan of an accepted layout, table by table."""
    N, P, offs = len(L["toas"]), L["P"], L["offs"]
    members, anchor, last = model_groups(L)
    M = dict(members=members, anchor=anchor, last=last, segs=[])
    for a in anchor:
        s = L["sigs"][a]
        nf, w, fill, lhs, rhs = model_sizes(L, s)
        sig = nf / (2.0 * s["nm"] + 1.0)
        g = dict(nm=s["nm"], nf=nf, w=w, fill=fill, beta=0.98 * math.pi * w * (1.0 - 0.5 / sig))
        psr = np.repeat(np.arange(P), np.diff(offs))
        u = (w0_rows(L, s)[psr] * L["toas"]) / (2.0 * math.pi / nf)
        g["J"] = (np.floor(u - 0.5 * w) + 1).astype(np.int64)  # first of the w rows around u, unwrapped
        g["d"] = u - g["J"]
        g.update(model_tables(s["nm"], nf, w, g["beta"]))
        M["segs"].append(g)
    segs = M["segs"]
    # greedy chunks: consecutive TOAs of a pulsar up to the next global multiple of TT, every signal's span of first
    # rows + w + 1 within ROW_CAP
    chunks, t = [], 0
    for p in range(P):
        t = int(offs[p])
        while t < offs[p + 1]:
            e = t + 1
            while (e < offs[p + 1] and e % TT != 0
                   and all(g["J"][t:e + 1].max() - g["J"][t:e + 1].min() + g["w"] + 1 <= ROW_CAP for g in segs)):
                e += 1
            chunks.append((p, t, e))
            t = e
    M["chunk_toas"] = chunks
    M["chunk_of"] = [ci for ci, (p, a, e) in enumerate(chunks) for _ in range(a, e)]
    M["tt_of"] = [i for (p, a, e) in chunks for i in range(e - a)]
    M["psr_chunk0"] = [sum(1 for c in chunks if c[0] < p) for p in range(P + 1)]
    for g in segs:
        g["band_lo"] = [int(g["J"][a:e].min()) for (p, a, e) in chunks]
        g["band_n"] = [int(g["J"][a:e].max() - g["J"][a:e].min()) + g["w"] for (p, a, e) in chunks]
    V = [max(MIN_V if diag else 0, -(-sum(g["band_n"][ci] for g in segs) // 4) * 4) for ci in range(len(chunks))]
    M["chunks"] = [v for ci, (p, a, e) in enumerate(chunks) for v in (p, a - int(offs[p]), e - a, V[ci])]
    M["vmax"] = vmax = max([4] + V)
    rowoff, lrow0 = 0, 0
    for g in segs:
        g["rowoff"], g["lrow0"] = rowoff, lrow0
        rowoff += P * g["nf"]
        lrow0 += g["nf"]
    M["grid_rows"] = rowoff
    rows, frow_band = [], []
    for ci, (p, a, e) in enumerate(chunks):
        r = [g["rowoff"] + p * g["nf"] + (g["band_lo"][ci] + i) % g["nf"] for g in segs for i in range(g["band_n"][ci])]
        f = [g["lrow0"] + (g["band_lo"][ci] + i) % g["nf"] for g in segs for i in range(g["band_n"][ci])]
        rows += r + [r[0]] * (vmax - len(r))
        frow_band.append(f + [f[0]] * (vmax - len(f)))
    M["rows"] = rows
    for si, g in enumerate(segs):
        voff = [sum(h["band_n"][ci] for h in segs[:si]) for ci in range(len(chunks))]
        g["row"] = [int(g["J"][t]) - g["band_lo"][M["chunk_of"][t]] + voff[M["chunk_of"][t]] for t in range(N)]
    # the fused kernel's plan
    jobs = sum(g["nf"] // 4 // 32 + 1 for g in segs)
    M["fused_lds"] = 8 * (lrow0 * F_PITCH + 2 * F_MAX_SIG * F_SLOT) + 48
    M["fused_ok"] = (len(segs) <= F_MAX_SIG and all(g["nf"] % 4 == 0 and g["ldq"] == (g["nf"] // 4 // 32 + 1) * 32
                                                    for g in segs)
                     and all(len(m) <= GEN_TERMS for m in members) and jobs <= F_DW and M["fused_lds"] <= F_LDS_MAX)
    if not M["fused_ok"]:
        return M
    M["fused_fq"] = fq = max(F_FQ_MIN, -(-(vmax // 4) // 4) * 4)
    M["frows"] = [r for f in frow_band for r in step_rows(f, vmax, fq)]
    # half-chunk bands: TOAs 0..15 and 16..31 of each chunk; a half's band = its own span + w per signal
    hv, hbands, hchunks = [], [], []
    M["hchunk_of"], M["htt_of"] = [0] * N, [0] * N
    for g in segs:
        g["hrow_of"] = [0] * N
    for ci, (p, a, e) in enumerate(chunks):
        nq = [0, 0]
        for h in range(2):
            b0, b1 = a + F_HALF_TT * h, min(e, a + F_HALF_TT * (h + 1))
            band, v = [], 0
            if b0 < b1:
                for g in segs:
                    lo, hi = int(g["J"][b0:b1].min()), int(g["J"][b0:b1].max())
                    for t in range(b0, b1):
                        g["hrow_of"][t] = int(g["J"][t]) - lo + v
                        M["hchunk_of"][t], M["htt_of"][t] = 2 * ci + h, t - b0
                    band += [g["lrow0"] + (lo + i) % g["nf"] for i in range(hi - lo + g["w"])]
                    v += hi - lo + g["w"]
            hv.append(-(-v // 4) * 4)
            hbands.append(band if band else [segs[0]["lrow0"]])
            nq[h] = hv[-1] // 4
        hchunks += [p, a - int(offs[p]), e - a, nq[0] | nq[1] << 16]
    M["hv"], M["hchunks"] = hv, hchunks
    M["fused_hvmax"] = hvmax = max([8] + [-(-v // 8) * 8 for v in hv])
    M["fused_hnq"] = max([1] + [v // 4 for v in hv])
    M["fused_hfq"] = hfq = max(F_HALF_NQ, -(-(hvmax // 4) // 4) * 4)
    M["hrows"] = [r for b, v in zip(hbands, hv) for r in step_rows(b, min(v, len(b)), hfq)]
    steps_full = sum(4.0 * (v // 4) for v in V)
    steps_half = sum(4.0 * max(hv[2 * ci], hv[2 * ci + 1]) // 4 for ci in range(len(chunks)))
    M["fused_half_gain"], M["fma_interp_half"] = steps_full / steps_half, steps_half * TT
    return M


# ------------------------------------------------------------------------------------------------ the tests
def _cases(planned, tag="product"):
    layouts, plans = planned
    assert len(plans[tag]["plans"]) == len(layouts)
    return list(zip(layouts, plans[tag]["plans"]))


def _close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    assert np.allclose(got, want, rtol=1e-12, atol=0.0), (what, np.abs(got - want).max())


def test_constants(planned):
    assert planned[1]["product"]["constants"] == [TT, ROW_CAP, VMAX, MIN_V, MAX_SEG, DFT_ROWS, GEN_TERMS, F_MAX_SIG,
                                                  F_PITCH, F_SLOT, F_DW, F_LDS_MAX, F_FQ_MIN, F_PAD_ROWS, F_HALF_TT,
                                                  F_HALF_NQ]
    assert (grid_model.TT, grid_model.MAX_SEG, grid_model.DFT_ROWS) == (TT, MAX_SEG, DFT_ROWS)


REFUSED = {
    "no_signals": "gridded path: no signals",
    "non_harmonic": "gridded path: every signal needs a harmonic grid f_k = k f_1",
    "too_many_signals": "gridded path: needs 1..16 grid signals (after coalescing)",
    "phase_range": "gridded path: phase out of range",
    "vmax_exceeded": "gridded path: a chunk's band rows over all signals exceed 256",
}


@pytest.mark.parametrize("tag", ["product", "diag"])
def test_refusals(planned, tag):
    seen = set()
    for L, H in _cases(planned, tag):
        if L["name"] in REFUSED:
            assert not H["ok"] and H["why"] == REFUSED[L["name"]], L["name"]
            seen.add(L["name"])
        else:
            assert H["ok"] and H["why"] == "", (L["name"], H["why"])
    assert seen == set(REFUSED)


@pytest.mark.parametrize("tag", ["product", "diag"])
def test_tables_match_model(planned, tag):
    """Every table of every accepted layout against the numpy model: integers exactly, doubles to 1e-12."""
    for L, H in _cases(planned, tag):
        if not H["ok"]:
            continue
        name, M = L["name"], model(L, diag=tag == "diag")
        for k in ("members", "anchor", "last", "chunks", "psr_chunk0", "chunk_of", "tt_of", "vmax", "grid_rows", "rows"):
            assert H[k] == M[k], (name, k)
        assert H["merges"] == int(any(len(m) > 1 for m in M["members"])), name
        assert len(H["segs"]) == len(M["segs"]), name
        for s, (g, m) in enumerate(zip(H["segs"], M["segs"])):
            for k in ("nm", "nf", "w", "half", "lde", "ntab", "ldq", "ntq", "rowoff", "band_lo", "band_n", "row"):
                assert g[k] == m[k], (name, s, k)
            _close(g["beta"], m["beta"], (name, s, "beta"))
            for k in ("d", "ecos", "esin", "tq"):
                _close(g[k], m[k], (name, s, k))
        assert H["fused_ok"] == int(M["fused_ok"]), name
        if len(M["segs"]) <= F_MAX_SIG:  # the LDS bytes of the grids and the draw ring (more signals: not worked out)
            assert H["fused_lds"] == M["fused_lds"], name
        assert H["fused_lrow0"][:len(M["segs"])] == [m["lrow0"] for m in M["segs"]][:len(H["fused_lrow0"])], name
        assert H["fused_half_ok"] == H["fused_ok"], name
        if not M["fused_ok"]:
            assert H["frows"] == [] and H["hrows"] == [] and H["hchunks"] == [], name
            continue
        for k in ("fused_fq", "frows", "hchunks", "hv", "hrows", "hchunk_of", "htt_of", "fused_hvmax", "fused_hnq",
                  "fused_hfq"):
            assert H[k] == M[k], (name, k)
        for g, m in zip(H["segs"], M["segs"]):
            assert g["hrow_of"] == m["hrow_of"], name
        assert H["fused_half_gain"] == M["fused_half_gain"] and H["fma_interp_half"] == M["fma_interp_half"], name


def test_branches_reached(planned):
    """Each layout reaches the branch it is there for."""
    by = {L["name"]: (L, H) for L, H in _cases(planned)}
    n_chunks = lambda name: len(by[name][1]["chunks"]) // 4
    assert [n_chunks(f"p1_n{n}") for n in (1, 31, 32, 33, 65)] == [1, 1, 1, 2, 3]
    L, H = by["p3_40_0_7"]
    assert H["psr_chunk0"] == [0, 2, 2, 3] and H["chunks"][4:7] == [0, 32, 8] and H["chunks"][8:11] == [2, 0, 7]
    L, H = by["p3_40_0_30"]  # the third pulsar starts at global TOA 40: 24 TOAs to the multiple of 32, then 6
    assert H["psr_chunk0"] == [0, 2, 2, 4] and H["chunks"][8:11] == [2, 0, 24] and H["chunks"][12:15] == [2, 24, 6]
    assert by["nm2"][1]["segs"][0]["nf"] == 2 * 15 + 2  # the max(n, 2 w + 2) floor
    assert n_chunks("sparse_nm100") > 10 and by["sparse_nm100"][1]["chunks"][2] < TT  # kGridRowCap cuts the chunks
    assert by["rn_dm_mixed_nu"][1]["members"] == [[0], [1]]
    assert by["rn_dm_const_nu"][1]["members"] == [[0, 1]] and by["rn_dm_const_nu"][1]["merges"] == 1
    assert by["rn_common"][1]["members"] == [[0, 1]] and by["rn_common"][1]["anchor"] == [1]
    assert by["rn_masked"][1]["members"] == [[0], [1]]
    assert by["rn_dm_const_nu_nocoalesce"][1]["members"] == [[0], [1]]
    # the fill rule, by its inequality
    for name, want in (("fill_dense", True), ("sparse_nm100", False), ("nm30", False)):
        L, H = by[name]
        nf, w, fill, lhs, rhs = model_sizes(L, L["sigs"][0])
        assert fill == want == (lhs < rhs) and (H["segs"][0]["nf"], H["segs"][0]["w"]) == (nf, w), name
    assert (by["fill_dense"][1]["segs"][0]["nf"], by["nm30"][1]["segs"][0]["nf"]) == (124, 92)
    assert by["three_signals"][1]["fused_ok"] == 0 and len(by["three_signals"][1]["segs"]) == 3
    L, H = by["lds_exceeded"]
    assert H["fused_ok"] == 0 and H["fused_lds"] > F_LDS_MAX
    assert H["fused_lds"] == 8 * (sum(g["nf"] for g in H["segs"]) * F_PITCH + 2 * F_MAX_SIG * F_SLOT) + 48
    assert by["c2_like"][1]["fused_ok"] == 1 and by["c2_like"][1]["members"] == [[0, 2], [1]]
    L, H = by["nine_members"]
    assert H["ok"] == 1 and H["members"] == [list(range(9))] and H["fused_ok"] == 0


@pytest.mark.parametrize("tag", ["product", "diag"])
def test_chunk_and_band_invariants(planned, tag):
    """What the interpolation kernels rely on, asserted directly on the planner's output."""
    for L, H in _cases(planned, tag):
        if not H["ok"]:
            continue
        name, N, P, offs, segs = L["name"], len(L["toas"]), L["P"], L["offs"], H["segs"]
        ch = np.array(H["chunks"]).reshape(-1, 4)
        nc, vmax = len(ch), H["vmax"]
        # every TOA in exactly one chunk; chunks pulsar-major and contiguous
        cover = [t for p, a, n, v in ch for t in range(offs[p] + a, offs[p] + a + n)]
        assert cover == list(range(N)), name
        assert list(ch[:, 0]) == sorted(ch[:, 0]) and (ch[:, 2] >= 1).all() and (ch[:, 2] <= TT).all(), name
        assert H["chunk_of"] == [ci for ci in range(nc) for _ in range(ch[ci, 2])], name
        assert H["tt_of"] == [i for ci in range(nc) for i in range(ch[ci, 2])], name
        assert H["psr_chunk0"] == [int((ch[:, 0] < p).sum()) for p in range(P + 1)], name
        # the unwrapped first rows, from the tables alone: band_lo + (row - the signal's offset in the chunk)
        voff = np.cumsum([[0] * nc] + [g["band_n"] for g in segs], axis=0)
        J = [np.array(g["band_lo"])[H["chunk_of"]] + np.array(g["row"]) - voff[s][H["chunk_of"]]
             for s, g in enumerate(segs)]
        for ci, (p, a, n, v) in enumerate(ch):
            t0, t1 = offs[p] + a, offs[p] + a + n
            assert t0 // TT == (t1 - 1) // TT, (name, ci)  # no chunk crosses a global multiple of kGridTT
            for s, g in enumerate(segs):
                assert J[s][t0:t1].max() - J[s][t0:t1].min() + g["w"] + 1 <= ROW_CAP, (name, ci)
                assert g["band_lo"][ci] == J[s][t0:t1].min(), (name, ci)
                assert g["band_n"][ci] == J[s][t0:t1].max() - J[s][t0:t1].min() + g["w"], (name, ci)
            if t1 < offs[p + 1] and t1 % TT != 0:  # greedy: the next TOA would have broken the row cap
                assert any(max(J[s][t0:t1 + 1]) - min(J[s][t0:t1 + 1]) + g["w"] + 1 > ROW_CAP
                           for s, g in enumerate(segs)), (name, ci)
            # chunk widths
            assert v % 4 == 0 and v >= voff[-1][ci] and v <= vmax, (name, ci)
            assert v == max(MIN_V if tag == "diag" else 0, (voff[-1][ci] + 3) // 4 * 4), (name, ci)
        assert vmax == max(4, ch[:, 3].max()) and vmax <= VMAX, name
        if tag == "diag":
            assert (ch[:, 3] >= MIN_V).all(), name
        # rows
        rows = np.array(H["rows"]).reshape(nc, vmax)
        assert H["grid_rows"] == P * sum(g["nf"] for g in segs) and (rows >= 0).all() and (rows < H["grid_rows"]).all()
        for ci, (p, a, n, v) in enumerate(ch):
            for s, g in enumerate(segs):
                for i in range(g["band_n"][ci]):
                    assert rows[ci, voff[s][ci] + i] == g["rowoff"] + p * g["nf"] + (g["band_lo"][ci] + i) % g["nf"]
            assert (rows[ci, voff[-1][ci]:] == rows[ci, 0]).all(), (name, ci)
        for s, g in enumerate(segs):  # every weight lands inside the chunk's band
            assert all(0 <= g["row"][t] and g["row"][t] + g["w"] <= ch[H["chunk_of"][t], 3] for t in range(N)), name
            assert g["rowoff"] == P * sum(h["nf"] for h in segs[:s]), name
        assert H["wd_size"] == (nc * vmax + F_PAD_ROWS) * TT and F_PAD_ROWS == 4 * F_FQ_MIN, name
        assert H["weight_bytes"] == 8.0 * H["wd_size"] and H["fma_interp"] == float(ch[:, 3].sum() * TT), name
        assert H["mean_v"] == H["fma_interp"] / TT / nc and H["grid_vals"] == float(H["grid_rows"]), name
        assert H["fma_direct"] == sum(2.0 * s["nm"] * N for s in L["sigs"]), name
        assert H["fma_dft"] == sum(P * (g["nf"] // 4 + 1) * 2.0 * g["nm"] for g in segs), name
        assert H["fma_grid"] == H["fma_dft"] + H["fma_interp"], name
        _close(H["err_bound"], max(bound(g["w"], g["nf"] / (2.0 * g["nm"] + 1.0)) for g in segs), name)
        if not H["fused_ok"]:
            continue
        # frows: [ci][j][q] = the LDS row of band row 4 q + j
        lds_rows, fq = sum(g["nf"] for g in segs), H["fused_fq"]
        fr = np.array(H["frows"]).reshape(nc, 4, fq)
        assert fq % 4 == 0 and fq >= F_FQ_MIN and 4 * fq >= vmax and (fr >= 0).all() and (fr < lds_rows).all(), name
        lrow0 = np.cumsum([0] + [g["nf"] for g in segs])
        for ci, (p, a, n, v) in enumerate(ch):
            band = [lrow0[s] + (g["band_lo"][ci] + i) % g["nf"] for s, g in enumerate(segs) for i in range(g["band_n"][ci])]
            for j in range(4):
                for q in range(fq):
                    r = 4 * q + j
                    assert fr[ci, j, q] == (band[r] if r < len(band) else band[0]), (name, ci, j, q)
        # half bands
        hch = np.array(H["hchunks"]).reshape(nc, 4)
        hv, hfq, hvmax = np.array(H["hv"]), H["fused_hfq"], H["fused_hvmax"]
        assert (hch[:, :3] == ch[:, :3]).all() and (hv % 4 == 0).all(), name
        assert list(hch[:, 3]) == [int(hv[2 * ci] // 4 | (hv[2 * ci + 1] // 4) << 16) for ci in range(nc)], name
        assert hvmax % 8 == 0 and hvmax >= max(8, hv.max()) and H["fused_hnq"] == max(1, hv.max() // 4), name
        assert hfq >= F_HALF_NQ and hfq % 4 == 0 and 4 * hfq >= hvmax, name
        hr = np.array(H["hrows"]).reshape(2 * nc, 4, hfq)
        assert (hr >= 0).all() and (hr < lds_rows).all(), name
        assert H["hwd_size"] == (2 * nc * hvmax + 4 * F_HALF_NQ) * F_HALF_TT, name
        for ci, (p, a, n, v) in enumerate(ch):
            for h in range(2):
                t0, t1 = offs[p] + a + F_HALF_TT * h, offs[p] + a + min(n, F_HALF_TT * (h + 1))
                hn = sum(J[s][t0:t1].max() - J[s][t0:t1].min() + g["w"] for s, g in enumerate(segs)) if t0 < t1 else 0
                assert hv[2 * ci + h] == (hn + 3) // 4 * 4, (name, ci, h)
                for t in range(t0, t1):
                    assert H["hchunk_of"][t] == 2 * ci + h and H["htt_of"][t] == t - t0, (name, t)
                    for g in segs:
                        assert 0 <= g["hrow_of"][t] and g["hrow_of"][t] + g["w"] <= hv[2 * ci + h], (name, t)
        steps_full = float(ch[:, 3].sum())
        steps_half = float(sum(max(hv[2 * ci], hv[2 * ci + 1]) for ci in range(nc)))
        assert H["fused_half_gain"] == steps_full / steps_half and H["fma_interp_half"] == steps_half * TT, name


def test_diag_plans(planned):
    """The diagnostic kernels' plans (variant builds): slots within the ring or union, list offsets in range, every
    band row of every chunk with a slot."""
    reached = set()
    for L, H in _cases(planned, "diag"):
        if not H["ok"]:
            continue
        name, segs = L["name"], H["segs"]
        ch = np.array(H["chunks"]).reshape(-1, 4)
        nc, vmax, n_seg = len(ch), H["vmax"], len(segs)
        rows = np.array(H["rows"]).reshape(nc, vmax)
        nb = [sum(g["band_n"][ci] for g in segs) for ci in range(nc)]
        if H["wr_ok"]:
            reached.add("wr")
            meta, lst = np.array(H["wr_meta"]).reshape(nc, 4), np.array(H["wr_list"]).reshape(-1, 2)
            slot = np.array(H["wr_slot"]).reshape(nc, vmax)
            assert (slot >= 0).all() and (slot < WR_SLOTS * n_seg).all(), name
            for ci in range(nc):
                full_off, full_n, new_off, new_n = meta[ci, 0], meta[ci, 1], meta[ci, 2], meta[ci, 3] & ((1 << 29) - 1)
                assert 0 <= full_off and full_off + full_n <= len(lst) and 0 <= new_off and new_off + new_n <= len(lst)
                assert full_n == nb[ci] and new_n <= full_n, (name, ci)
                # the full list loads every band row into the slot the chunk reads it from
                assert sorted(map(tuple, lst[full_off:full_off + full_n])) == \
                    sorted(zip(slot[ci, :nb[ci]], rows[ci, :nb[ci]])), (name, ci)
                assert len(set(slot[ci, :nb[ci]])) == nb[ci], (name, ci)
        for key, gk, uk, max_rows, max_group in (("lds", "lds_groups", "lds_urows", LDS_ROWS_MAX, LDS_GROUP),
                                                 ("u", "u_groups", "u_urows", U_ROWS_MAX, U_GROUP)):
            if not H[key + "_ok"]:
                continue
            reached.add(key)
            groups, urows = np.array(H[gk]).reshape(-1, 4), np.array(H[uk])
            assert list(groups[:, 0]) == list(np.cumsum([0] + list(groups[:-1, 1]))) and groups[:, 1].sum() == nc, name
            assert (groups[:, 1] <= max_group).all() and (groups[:, 2] <= max_rows).all(), name
            assert list(groups[:, 3]) == list(np.cumsum([0] + list(groups[:-1, 2]))), name
            assert groups[:, 2].sum() == len(urows), name
            for c0, n, U, off in groups:
                for ci in range(c0, c0 + n):
                    assert ch[ci, 0] == ch[c0, 0], (name, ci)
                    if key == "lds":  # the union slot of each band row holds that row's grid-buffer row
                        lr = np.array(H["lds_lrows"]).reshape(nc, vmax)[ci]
                        assert (lr >= 0).all() and (lr < U).all(), (name, ci)
                        assert (urows[off + lr] == rows[ci]).all(), (name, ci)
                    else:  # slot = band row + base of the row's signal
                        cb = np.array(H["u_cbase"]).reshape(nc, 2, U_SIG_MAX)[ci]
                        for v in range(nb[ci]):
                            s = max(i for i in range(U_SIG_MAX) if cb[0, i] <= v)
                            assert 0 <= v + cb[1, s] < U and urows[off + v + cb[1, s]] == rows[ci, v], (name, ci, v)
            if key == "lds":
                assert H["lds_rows"] == groups[:, 2].max(), name
            else:
                wrow = np.array(H["u_wrow"]).reshape(nc, n_seg, TT)
                for s, g in enumerate(segs):
                    for t in range(len(L["toas"])):
                        assert wrow[H["chunk_of"][t], s, H["tt_of"][t]] == g["row"][t], (name, t)
                    for ci in range(nc):
                        assert (wrow[ci, s, ch[ci, 2]:] == -(1 << 20)).all(), (name, ci)
    assert reached == {"wr", "lds", "u"}
