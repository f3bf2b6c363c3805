// Roemer delays of ephemeris errors in a batch block (fpta_batch_roemer_accumulate), host side in plain C++:
// validation of the arguments and of every row (ephem_host.h), the base-orbit slots, the TOA slab table and the
// realization chunk of k_roemer_block. No HIP here: roemer_batch.hip includes it, and a stand-alone CPU program can
// include it alone (tests/test_roemer_batch_host.py builds one under the address sanitizer). Everything a call can
// refuse is refused here, before anything is uploaded or launched.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "ephem_host.h"

namespace fpta_roemerb {

constexpr int kSlabToas = 256;     // TOAs of one k_roemer_block workgroup (one per thread)
constexpr int kRoemerMaxBase = 8;  // base orbits a workgroup keeps in LDS (6 KB each)
constexpr int kMaxChunk = 32;      // realizations of one workgroup, at most
// The chunk rule's one constant: the workgroups a call should still have after chunking (4 per compute unit of a
// 256-unit device). Not measured: DESIGN.md section 5f.
constexpr int64_t kTargetGroups = 1024;

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

// Realizations per workgroup. forced >= 1 (FPTA_OPT_ROEMER_CHUNK): that, clamped to kMaxChunk. 0: as many as leave
// kTargetGroups workgroups, so a small call keeps one realization per workgroup and a large one shares the slot
// prologue among up to kMaxChunk. The result never depends on it.
inline int32_t chunk_size(int64_t n_slab, int32_t n_real, int64_t forced) {
  int64_t c = forced >= 1 ? forced : (n_slab * (int64_t)n_real) / kTargetGroups;
  if (c > kMaxChunk) c = kMaxChunk;
  if (c > n_real) c = n_real;
  return (int32_t)(c < 1 ? 1 : c);
}

// Slots for the distinct base bodies of `rows`, compared bit by bit over their 14 doubles, in order of first
// appearance; a row whose base is beyond the first kRoemerMaxBase distinct ones gets -1.
inline void assign_slots(const std::vector<fpta_ephem::RoemerRow>& rows, std::vector<fpta_ephem::Body>& bases,
                         std::vector<int32_t>& slot) {
  bases.clear();
  slot.assign(rows.size(), -1);
  for (size_t k = 0; k < rows.size(); ++k) {
    const fpta_ephem::Body& b = rows[k].base;
    for (size_t s = 0; s < bases.size(); ++s)
      if (!std::memcmp(&bases[s], &b, sizeof(fpta_ephem::Body))) {
        slot[k] = (int32_t)s;
        break;
      }
    if (slot[k] < 0 && bases.size() < (size_t)kRoemerMaxBase) {
      slot[k] = (int32_t)bases.size();
      bases.push_back(b);
    }
  }
}

struct Plan {
  std::vector<fpta_ephem::RoemerRow> rows;  // [row_offs[n_tab]]: table r's rows at row_offs[r]
  std::vector<int32_t> base_slot;           // per row: its base's slot, or -1
  std::vector<fpta_ephem::Body> bases;      // the slots' bodies, <= kRoemerMaxBase
  std::vector<Slab> slabs;
  int64_t n_row = 0;  // rows of all tables
  int32_t chunk = 1;  // realizations per workgroup
};

// Validates one call against a layout (n_psr, offs, toas) and a block of n_real realizations, and fills the plan.
// False with the reason in `why`; the first bad row is named "realization r, row k: reason". forced_chunk:
// FPTA_OPT_ROEMER_CHUNK.
inline bool make_plan(int32_t n_psr, const int64_t* offs, const double* toas, int32_t n_real, const double* pos,
                      int32_t n_tab, const int64_t* row_offs, const double* rows, double sign, int64_t forced_chunk,
                      Plan& plan, std::string& why) {
  if (n_psr <= 0 || !offs || n_real <= 0 || !pos || !row_offs) {
    why = "bad arguments";
    return false;
  }
  if (n_tab != 1 && n_tab != n_real) {
    why = std::to_string(n_tab) + " row tables for a block of " + std::to_string(n_real) +
          " realizations (1 or one per realization)";
    return false;
  }
  if (row_offs[0] != 0) {
    why = "row_offs[0] must be 0";
    return false;
  }
  for (int32_t r = 0; r < n_tab; ++r)
    if (row_offs[r + 1] < row_offs[r]) {
      why = "row_offs is not monotone at table " + std::to_string(r);
      return false;
    }
  const int64_t n_row = row_offs[n_tab];
  if (n_row > 0 && !rows) {
    why = "rows missing";
    return false;
  }
  if (n_row > (int64_t)1 << 31) {
    why = "too many rows";
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
  const int64_t n_toa = offs[n_psr];
  if (n_toa > 0 && !toas) {
    why = "bad arguments";
    return false;
  }
  double t0, t1;
  int64_t bad = -1;
  if (!fpta_ephem::toa_span(n_toa, toas, t0, t1, bad)) {
    why = "TOA " + std::to_string(bad) + ": not finite";
    return false;
  }
  plan.n_row = n_row;
  plan.rows.resize((size_t)n_row);
  for (int32_t r = 0; r < n_tab; ++r) {
    const int64_t o = row_offs[r], n = row_offs[r + 1] - o;
    std::string w;
    bad = fpta_ephem::validate_rows(n, rows + o * fpta_ephem::kNRow, t0, t1, plan.rows.data() + o, w);
    if (bad >= 0) {
      why = "realization " + std::to_string(r) + ", row " + std::to_string(bad) + ": " + w;
      return false;
    }
  }
  assign_slots(plan.rows, plan.bases, plan.base_slot);
  make_slabs(n_psr, offs, plan.slabs);
  plan.chunk = chunk_size((int64_t)plan.slabs.size(), n_real, forced_chunk);
  return true;
}

}  // namespace fpta_roemerb
