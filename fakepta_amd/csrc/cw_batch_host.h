// Continuous-wave populations in a batch block (fpta_batch_cw_accumulate), host side in plain C++: validation of the
// arguments and of every source, the per-source constants (cw_host.h, long double) and the TOA slab table of
// k_cw_block. No HIP here: cw_batch.hip includes it, and a stand-alone CPU program can include it alone
// (tests/test_cw_batch_host.py builds one under the address sanitizer). Everything a call can refuse is refused here,
// before anything is uploaded or launched.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "cw_host.h"

namespace fpta_cwb {

constexpr int kSlabToas = 256;  // TOAs of one k_cw_block workgroup (one per thread)

// <= kSlabToas consecutive TOAs of one pulsar
struct Slab {
  int64_t first;  // first TOA (index into the concatenated arrays)
  int32_t psr;
  int32_t count;  // 1 .. kSlabToas
};

// Every (pulsar, TOA) exactly once, in TOA order; a slab never crosses a pulsar. A pulsar without TOAs gets none.
inline void make_slabs(int32_t n_psr, const int64_t* offs, std::vector<Slab>& out) {
  out.clear();
  for (int32_t p = 0; p < n_psr; ++p)
    for (int64_t i = offs[p]; i < offs[p + 1]; i += kSlabToas) {
      const int64_t left = offs[p + 1] - i;
      out.push_back({i, p, (int32_t)(left < kSlabToas ? left : kSlabToas)});
    }
}

struct Plan {
  std::vector<fpta_cw::SrcEval> ev;  // [src_offs[n_tab]]: table r's rows at src_offs[r]
  std::vector<fpta_cw::SrcGeom> gm;
  std::vector<Slab> slabs;
  int64_t n_src = 0;  // rows of all tables
};

// Validates one call against a layout (n_psr, offs, tmax = the latest TOA) and a block of n_real realizations, and
// fills the plan. False with the reason in `why`; the first bad source is named "realization r, source s: reason".
// pdist_stride 0: pdist_s [n_psr] for every realization; n_psr: [n_real][n_psr].
inline bool make_plan(int32_t n_psr, const int64_t* offs, double tmax, int32_t n_real, const double* pos,
                      const double* pdist_s, int64_t pdist_stride, int32_t n_tab, const int64_t* src_offs,
                      const double* src, double sign, Plan& plan, std::string& why) {
  if (n_psr <= 0 || !offs || n_real <= 0 || !pos || !pdist_s || !src_offs) {
    why = "bad arguments";
    return false;
  }
  if (n_tab != 1 && n_tab != n_real) {
    why = std::to_string(n_tab) + " source tables for a block of " + std::to_string(n_real) +
          " realizations (1 or one per realization)";
    return false;
  }
  if (src_offs[0] != 0) {
    why = "src_offs[0] must be 0";
    return false;
  }
  for (int32_t r = 0; r < n_tab; ++r)
    if (src_offs[r + 1] < src_offs[r]) {
      why = "src_offs is not monotone at table " + std::to_string(r);
      return false;
    }
  const int64_t n_src = src_offs[n_tab];
  if (n_src > 0 && !src) {
    why = "src missing";
    return false;
  }
  if (n_src > (int64_t)1 << 40) {
    why = "too many sources";
    return false;
  }
  if (pdist_stride != 0 && pdist_stride != n_psr) {
    why = "pdist_stride must be 0 or the number of pulsars";
    return false;
  }
  if (!std::isfinite(sign)) {
    why = "non-finite sign";
    return false;
  }
  for (int32_t p = 0; p < n_psr; ++p)
    for (int k = 0; k < 3; ++k)
      if (!std::isfinite(pos[3 * (int64_t)p + k])) {
        why = "pulsar " + std::to_string(p) + ": non-finite position";
        return false;
      }
  const int64_t n_dist = pdist_stride ? (int64_t)n_real * n_psr : n_psr;
  for (int64_t i = 0; i < n_dist; ++i)
    if (!std::isfinite(pdist_s[i])) {
      why = (pdist_stride ? "realization " + std::to_string(i / n_psr) + ", " : std::string()) + "pulsar " +
            std::to_string(i % n_psr) + ": non-finite distance";
      return false;
    }
  plan.n_src = n_src;
  plan.ev.resize((size_t)n_src);
  plan.gm.resize((size_t)n_src);
  for (int32_t r = 0; r < n_tab; ++r) {
    const int64_t o = src_offs[r], n = src_offs[r + 1] - o;
    std::string w;
    const int64_t bad = fpta_cw::validate_sources(n, src + o * fpta_cw::kNPar, tmax, plan.ev.data() + o,
                                                  plan.gm.data() + o, w);
    if (bad >= 0) {
      why = "realization " + std::to_string(r) + ", source " + std::to_string(bad) + ": " + w;
      return false;
    }
  }
  make_slabs(n_psr, offs, plan.slabs);
  return true;
}

}  // namespace fpta_cwb
