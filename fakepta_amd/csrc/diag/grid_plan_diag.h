// The plans of the diagnostic interpolation kernels (k_grid_interp_wr, k_grid_interp_lds, k_grid_interp_u), made from
// the gridded plan (grid_plan.h) in plain C++. Compiled and called only under -DFPTA_DIAG_KERNELS (make variant); the
// product library holds none of this.
#pragma once
#include "../grid_plan.h"

namespace fpta {

struct Int2 {  // uploaded as int2
  int32_t x, y;
};

// The unwrapped grid rows [lo, end) that signal s's bands of chunks ci .. ci + n - 1 unite to.
inline void band_union_span(const HostGridPlan& H, int32_t s, int32_t ci, int32_t n, int64_t& lo, int64_t& end) {
  const PlanSeg& g = H.segs[s];
  lo = g.band_lo[ci];
  end = g.band_lo[ci] + g.band_n[ci];
  for (int32_t k = 1; k < n; ++k) {
    lo = std::min(lo, g.band_lo[ci + k]);
    end = std::max(end, g.band_lo[ci + k] + (int64_t)g.band_n[ci + k]);
  }
}
// Union rows over all signals of chunks ci .. ci + n - 1.
inline int64_t band_union_rows(const HostGridPlan& H, int32_t ci, int32_t n) {
  int64_t u = 0, lo, end;
  for (int32_t s = 0; s < H.n_seg(); ++s) {
    band_union_span(H, s, ci, n, lo, end);
    u += end - lo;
  }
  return u;
}
// The chunks from ci on that form one group: <= max_group consecutive chunks of one pulsar uniting to <= max_rows rows
// (a single chunk may exceed them: the caller checks).
inline int32_t band_union_group(const HostGridPlan& H, int32_t ci, int32_t max_group, int64_t max_rows) {
  int32_t n = 1;
  while (n < max_group && ci + n < H.n_chunks() && H.chunks[ci + n].x == H.chunks[ci].x &&
         band_union_rows(H, ci, n + 1) <= max_rows)
    ++n;
  return n;
}
// grid-buffer row of signal g's unwrapped row j on pulsar p
inline int32_t band_grid_row(const PlanSeg& g, int32_t p, int64_t j) {
  return (int32_t)(g.rowoff + (int64_t)p * g.nf + plan_wrap(j, g.nf));
}

// k_grid_interp_wr: ring slot kWrSlots s + (unwrapped row mod kWrSlots) per band row; load lists per chunk
struct DiagWindowPlan {
  bool ok = false;
  std::vector<Int4> meta;     // [n_chunks] {full list offset, full count, new list offset, new count | flags}
  std::vector<Int2> list;     // {LDS slot, grid-buffer row}
  std::vector<int32_t> slot;  // [n_chunks][vmax]
};
inline DiagWindowPlan plan_diag_window(const HostGridPlan& H) {
  DiagWindowPlan W;
  const int32_t n_seg = H.n_seg(), n_chunks = H.n_chunks(), vmax = H.vmax;
  W.ok = n_seg <= kWrMaxSig && vmax <= kWrVMax;
  for (int32_t s = 0; s < n_seg && W.ok; ++s)
    for (int32_t ci = 0; ci < n_chunks && W.ok; ++ci) W.ok = H.segs[s].band_n[ci] <= kWrSlots;
  if (!W.ok) return W;
  W.meta.resize(n_chunks);
  W.slot.assign((size_t)n_chunks * vmax, 0);
  for (int32_t ci = 0; ci < n_chunks; ++ci) {
    const int32_t p = H.chunks[ci].x;
    int32_t* sl = W.slot.data() + (size_t)ci * vmax;
    int32_t v = 0;
    for (int32_t s = 0; s < n_seg; ++s)
      for (int32_t i = 0; i < H.segs[s].band_n[ci]; ++i)
        sl[v++] = kWrSlots * s + (int32_t)((H.segs[s].band_lo[ci] + i) & (kWrSlots - 1));
    for (; v < vmax; ++v) sl[v] = sl[0];
    // the bands of chunks ci - back .. ci (same pulsar) in one ring window per signal: compat (back 1) = only the rows
    // the previous band does not hold load, after the chunk before has been computed; near (back 2) = they may load
    // while the chunk two back is computed
    auto window = [&](int32_t back) {
      if (ci < back) return false;
      for (int32_t b = 1; b <= back; ++b)
        if (H.chunks[ci - b].x != p) return false;
      for (int32_t s = 0; s < n_seg; ++s) {
        int64_t lo, end;
        band_union_span(H, s, ci - back, back + 1, lo, end);
        if (end - lo > kWrSlots) return false;
      }
      return true;
    };
    const bool compat = window(1), near = compat && window(2);
    auto add_rows = [&](bool only_new) {
      int32_t n = 0;
      for (int32_t s = 0; s < n_seg; ++s) {
        const PlanSeg& g = H.segs[s];
        for (int32_t i = 0; i < g.band_n[ci]; ++i) {
          const int64_t u = g.band_lo[ci] + i;
          if (only_new && u >= g.band_lo[ci - 1] && u < g.band_lo[ci - 1] + g.band_n[ci - 1]) continue;
          W.list.push_back(Int2{kWrSlots * s + (int32_t)(u & (kWrSlots - 1)), band_grid_row(g, p, u)});
          ++n;
        }
      }
      return n;
    };
    const int32_t full_off = (int32_t)W.list.size();
    const int32_t full_n = add_rows(false);
    int32_t new_off = full_off, new_n = full_n;
    if (compat) {
      new_off = (int32_t)W.list.size();
      new_n = add_rows(true);
    }
    W.meta[ci] = Int4{full_off, full_n, new_off, new_n | (compat ? 0 : kWrFresh) | (near ? 0 : kWrFar)};
  }
  return W;
}

// LDS-staged interpolation (k_grid_interp_lds): groups of <= kLdsGroup consecutive chunks of one pulsar whose
// bands, over all signals, unite to <= kLdsRowsMax rows. Per group the union's grid-buffer rows (signal by
// signal, each signal's rows one contiguous unwrapped range), per chunk the union slot of each band row.
struct DiagLdsPlan {
  bool ok = false;
  std::vector<Int4> groups;  // {first chunk, chunks, union rows U, offset into urows}
  std::vector<int32_t> urows, lrows;
  int32_t lds_rows = 0;      // largest U
};
inline DiagLdsPlan plan_diag_lds(const HostGridPlan& H) {
  DiagLdsPlan D;
  const int32_t n_seg = H.n_seg(), n_chunks = H.n_chunks(), vmax = H.vmax;
  D.lrows.resize((size_t)n_chunks * vmax);
  for (int32_t ci = 0; ci < n_chunks;) {
    const int32_t p = H.chunks[ci].x;
    const int32_t n = band_union_group(H, ci, kLdsGroup, kLdsRowsMax);
    const int64_t U = band_union_rows(H, ci, n);
    // one chunk's bands alone exceed the LDS budget: the register-tiled kernel serves the layout
    if (U > kLdsRowsMax) return D;
    D.groups.push_back(Int4{ci, n, (int32_t)U, (int32_t)D.urows.size()});
    D.lds_rows = std::max(D.lds_rows, (int32_t)U);
    int32_t uoff = 0;
    for (int32_t s = 0; s < n_seg; ++s) {
      const PlanSeg& g = H.segs[s];
      int64_t lo, end;
      band_union_span(H, s, ci, n, lo, end);
      for (int64_t j = lo; j < end; ++j) D.urows.push_back(band_grid_row(g, p, j));
      for (int32_t k = 0; k < n; ++k)  // chunk ci + k: signal s's band rows start at slot uoff + (its lo - lo)
        for (int32_t i = 0; i < g.band_n[ci + k]; ++i)
          D.lrows[(size_t)(ci + k) * vmax + g.voff[ci + k] + i] = uoff + (int32_t)(g.band_lo[ci + k] - lo) + i;
      uoff += (int32_t)(end - lo);
    }
    for (int32_t k = 0; k < n; ++k) {  // pad rows: any valid slot (weight 0)
      int32_t* r = D.lrows.data() + (size_t)(ci + k) * vmax;
      for (int32_t v = H.segs[n_seg - 1].voff[ci + k] + H.segs[n_seg - 1].band_n[ci + k]; v < vmax; ++v) r[v] = r[0];
    }
    ci += n;
  }
  D.ok = !D.groups.empty();
  return D;
}

// k_grid_interp_u: the same grouping under the tighter LDS budget of two workgroups per CU; per chunk the signals'
// band offsets and union bases, per (chunk, signal, TOA slot) the window's first band row
struct DiagUnionPlan {
  bool ok = false;
  std::vector<Int4> groups;
  std::vector<int32_t> urows, cbase, wrow;
};
inline DiagUnionPlan plan_diag_union(const HostGridPlan& H) {
  DiagUnionPlan D;
  const int32_t n_seg = H.n_seg(), n_chunks = H.n_chunks();
  if (n_seg > kUnionSigMax) return D;
  for (int32_t ci = 0; ci < n_chunks;) {
    const int32_t p = H.chunks[ci].x;
    const int32_t n = band_union_group(H, ci, kUnionGroup, kUnionRowsMax);
    const int64_t U = band_union_rows(H, ci, n);
    if (U > kUnionRowsMax) return D;
    D.groups.push_back(Int4{ci, n, (int32_t)U, (int32_t)D.urows.size()});
    int32_t uoff = 0;
    std::vector<int32_t> cb((size_t)n * 2 * kUnionSigMax, 0);
    for (int32_t s = 0; s < n_seg; ++s) {
      const PlanSeg& g = H.segs[s];
      int64_t lo, end;
      band_union_span(H, s, ci, n, lo, end);
      for (int64_t j = lo; j < end; ++j) D.urows.push_back(band_grid_row(g, p, j));
      for (int32_t k = 0; k < n; ++k) {
        const int32_t vo = g.voff[ci + k];
        cb[(size_t)k * 2 * kUnionSigMax + s] = vo;
        cb[(size_t)k * 2 * kUnionSigMax + kUnionSigMax + s] = uoff + (int32_t)(g.band_lo[ci + k] - lo) - vo;
      }
      uoff += (int32_t)(end - lo);
    }
    for (int32_t k = 0; k < n; ++k)
      for (int32_t s = n_seg; s < kUnionSigMax; ++s) {  // absent signals: never selected (offset past every row)
        cb[(size_t)k * 2 * kUnionSigMax + s] = 1 << 20;
        cb[(size_t)k * 2 * kUnionSigMax + kUnionSigMax + s] = 0;
      }
    D.cbase.insert(D.cbase.end(), cb.begin(), cb.end());
    ci += n;
  }
  D.ok = !D.groups.empty();
  if (!D.ok) return D;
  D.wrow.assign((size_t)n_chunks * n_seg * kGridTT, -(1 << 20));  // empty TOA slots: every weight 0
  for (int32_t s = 0; s < n_seg; ++s)
    for (size_t t = 0; t < H.chunk_of.size(); ++t)
      D.wrow[((size_t)H.chunk_of[t] * n_seg + s) * kGridTT + H.tt_of[t]] = H.segs[s].row[t];
  return D;
}

}  // namespace fpta
