// The gridded path's plan of a layout, in plain C++: no HIP here. grid_host.hip's grid_build fills a host view of the
// layout, calls plan_grid and uploads the tables; the kernels read the same constants through fpta_internal.h; and a
// stand-alone CPU program can include this file alone (tests/test_grid_plan.py checks every table against a numpy
// model). A wrong entry here is an out-of-bounds LDS or global read in a kernel. DESIGN.md §5c.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

namespace fpta {

// ------------------------------------------------------------------------------- planning constants
constexpr int kGridTT = 32;      // TOAs per interpolation chunk (k_grid_interp_mfma: even / odd TOAs = two MFMA B-tiles)
constexpr int kGridRowCap = 48;  // cells a chunk's interpolation rows span at most, per signal (w + 1 included)
constexpr int kGridVMax = 256;   // band rows per chunk, all signals (k_grid_interp_mfma keeps them in 4 VGPRs)
constexpr int kGridMinV = 16;    // band rows per chunk at least (k_grid_interp_st: 4 MFMA steps, its lookahead + 1)
constexpr int kGridMaxSeg = 16;  // signals per layout on the gridded path (passed by value as kernel arguments)
#ifndef FPTA_DFT_MJ
#define FPTA_DFT_MJ 2
#endif
constexpr int kDftMJ = FPTA_DFT_MJ;      // k_grid_dft_mfma wave tile: 16 MJ grid rows x 16 kDftMR realizations
constexpr int kDftMR = 4 / FPTA_DFT_MJ;  // (the accumulators stay at 4 MJ MR = 16 tiles: two parities, cos and sin)
constexpr int kGridDftRows = 16 * kDftMJ;  // grid rows per k_grid_dft_mfma row block (quarter range) and k_grid_dft (half)
constexpr int kDftGenTerms = 8;    // members of a grid signal k_grid_dft_gen / k_grid_fused sum (DftGenArgs)
// k_grid_fused (fpta_internal.h)
constexpr int kFusedMaxSig = 2;    // grid signals (the draw ring holds a group of each)
constexpr int kFusedReal = 32;     // realizations per item (two 16-realization MFMA tiles)
constexpr int kFusedPitch = 32;    // doubles per LDS grid row
constexpr int kFusedDW = 4;        // DFT waves per workgroup = DFT jobs (32-row quarter-range chunks) at most
constexpr int kFusedGroupModes = 16;  // modes per draw group: two 4-mode k-steps of both parities
constexpr int kFusedSlot = kFusedGroupModes * kFusedReal * 2;  // doubles per signal of a ring slot [16 modes][32][cos, sin]
constexpr int kFusedLdsMax = 160 * 1024;
constexpr int kFusedFqMin = 16;    // floor of FusedArgs::fq: padding k_grid_fused's unconditional band-step loads rely on
constexpr int kFusedPadRows = 4 * kFusedFqMin;  // zero-weight band rows past the last chunk (GridPlan::wd): the same padding
constexpr int kFusedHalfTT = 16;   // TOAs of a half chunk
constexpr int kFusedHalfNQ = 8;    // band steps of each half whose operands an interpolation wave holds
// limits of the diagnostic kernels' plans (diag/grid_plan_diag.h; the kernels: fpta_internal.h)
constexpr int kWrSlots = 32, kWrMaxSig = 2, kWrVMax = 40;
constexpr int kWrFresh = 1 << 30;  // GridWindow::meta .w flag: load every band row, after the previous chunk is done
constexpr int kWrFar = 1 << 29;    // .w flag: the new rows may load only once the chunk two back is done
constexpr int kLdsGroup = 4, kLdsRowsMax = 144;
constexpr int kUnionGroup = 4, kUnionRowsMax = 76, kUnionSigMax = 2;

struct Int4 {  // uploaded as int4
  int32_t x, y, z, w;
};

// ------------------------------------------------------------------------------- input: a host view of a layout
struct PlanSignal {
  int32_t kind = 0, nm = 0;  // SegDesc::kind, ::nm
  double idx = 0.0, freqf = 0.0;
  int32_t harmonic = 0;
  const double* w0 = nullptr;      // first angular frequency per row ([P] for kind 0, [1] for kind 1)
  const uint8_t* mask = nullptr;   // [n_toa] or null: none
};
struct PlanLayout {
  int32_t P = 0;
  int64_t n_toa = 0;
  const int64_t* offs = nullptr;  // [P + 1]
  const double* toas = nullptr;   // [n_toa] seconds
  const double* nu = nullptr;     // [n_toa] MHz
  std::vector<PlanSignal> sigs;
};
struct PlanOptions {
  int32_t w = 0;       // kernel width (grid cells)
  double sigma = 0.0;  // oversampling
  bool coalesce = false;
  int32_t grid_mfma = 1;  // bit 0: the DFT runs on the quarter range (fma_dft)
};

// ------------------------------------------------------------------------------- output
struct PlanSeg {  // one grid signal
  int32_t nm = 0;  // its anchor's modes
  int32_t nf = 0, w = 0, half = 0, lde = 0, ntab = 0, ldq = 0, ntq = 0;
  double beta = 0.0;
  int64_t rowoff = 0;
  std::vector<double> ecos, esin;  // [ntab][lde] half-range tables (k_grid_dft)
  std::vector<double> tq;          // [4][ntq][ldq] quarter-range tables by mode parity (k_grid_dft_mfma)
  std::vector<int32_t> row;        // [n_toa] band row of the TOA's first weight (the signal's offset in the chunk included)
  std::vector<double> d;           // [n_toa] offset u - J of the TOA from its first interpolation row
  std::vector<int32_t> hrow_of;    // [n_toa] the same row in the TOA's half-chunk band
  // working tables of the stages
  std::vector<int64_t> J;          // [n_toa] first interpolation row: unwrapped, then (plan_chunks) within the chunk's band
  std::vector<int64_t> band_lo;    // [n_chunks] first grid row (unwrapped) of the signal's band
  std::vector<int32_t> band_n;     // [n_chunks] band rows of the signal (span + w)
  std::vector<int32_t> voff;       // [n_chunks] the band's first row among the chunk's band rows
};
// What the host keeps of a plan: GridPlan (capi_host.h) is these figures plus the device tables.
struct PlanFigures {
  bool ok = false;           // usable for this layout (harmonic, <= kGridMaxSeg signals)
  std::string why;           // reason when !ok
  // grid signals (FPTA_OPT_GRID_COALESCE): members (layout signal indices, ascending), the anchor (the member with
  // the most modes: its coefficient columns receive the others' and its grid/weights serve the group) and the last
  // member (the group's coefficients are complete once it is drawn)
  std::vector<std::vector<int32_t>> members;
  std::vector<int32_t> anchor, last;
  bool merges = false;       // some grid signal has > 1 member
  std::vector<int32_t> psr_chunk0;  // [P + 1] first chunk of each pulsar (chunks are pulsar-major)
  int32_t vmax = 0;          // largest V: row pitch of the row-index and weight tables
  int64_t grid_rows = 0;     // rows of the grid buffer: sum over signals of P nf
  // k_grid_fused plan (FPTA_OPT_INTERP_FUSED): every grid signal's grid for kFusedReal realizations in LDS (signal s
  // at LDS row fused_lrow0[s]), the draw ring after them; fused_lds the workgroup's LDS bytes (worked out for
  // <= kFusedMaxSig signals, also when they are why fused_ok is false); fused_fq band steps per (chunk, lane group)
  bool fused_ok = false;
  size_t fused_lds = 0;
  int32_t fused_fq = 0;
  std::vector<int32_t> fused_lrow0;
  // half-chunk bands of the fused kernel (FusedHalf): fused_half_gain = the interpolation MFMAs of whole-chunk bands
  // over those of half-chunk bands; fused_hnq the band steps of the widest half
  bool fused_half_ok = false;
  int32_t fused_hfq = 0, fused_hvmax = 0, fused_hnq = 0;
  double fused_half_gain = 0.0;
  double fma_interp_half = 0.0;  // interpolation FMAs per realization on half-chunk bands (both halves run max(nq0, nq1) steps)
  double mean_v = 0.0;       // mean band rows per chunk
  double fma_grid = 0.0;     // FMAs per realization: DFT + interpolation
  double fma_dft = 0.0;      // FMAs per realization in k_grid_dft
  double fma_interp = 0.0;   // FMAs per realization in k_grid_interp (dense band, padded TOA slots)
  double grid_vals = 0.0;    // grid values per realization (sum over signals of P nf)
  double weight_bytes = 0.0; // interpolation weight tables
  double fma_direct = 0.0;   // FMAs per realization of the direct contraction
  double err_bound = 1.0;    // the ES kernel's design estimate of the relative aliasing error, exp(-pi w sqrt(1 - 1/sigma)):
                             // not a bound, a single top mode is off by up to 2.8e-11 per unit coefficient at the
                             // shipped (15, 1.5), 18 times the estimate (tests/test_grid_modes.py)
};
struct HostGridPlan : PlanFigures {
  std::vector<PlanSeg> segs;
  std::vector<Int4> chunks;  // {pulsar, first TOA (pulsar-local), count, band rows V (multiple of 4)}
  std::vector<int32_t> chunk_of, tt_of;
  std::vector<int32_t> rows;  // [n_chunks][vmax]
  size_t wd_size = 0;         // doubles of the weights [n_chunks][vmax][kGridTT], + kFusedPadRows rows
  std::vector<int32_t> frows; // [n_chunks][4][fused_fq]
  std::vector<Int4> hchunks;  // {pulsar, first TOA, count, nq0 | nq1 << 16}
  std::vector<int32_t> hrows, hchunk_of, htt_of;  // hrows [n_chunks][2][4][fused_hfq]
  std::vector<int32_t> hv;    // [2 n_chunks] band rows of each half (padded to 4)
  size_t hwd_size = 0;        // doubles of the half weights [2 n_chunks][fused_hvmax][16], + 4 kFusedHalfNQ rows
  int32_t n_seg() const { return (int32_t)segs.size(); }
  int32_t n_chunks() const { return (int32_t)chunks.size(); }
};

// grid row j (unwrapped, any sign) of a grid of nf points
inline int32_t plan_wrap(int64_t j, int32_t nf) { return (int32_t)((j % nf + nf) % nf); }

// Gauss-Legendre nodes/weights on [-1, 1] (Newton on P_n; host, once per plan).
inline void gauss_legendre(int n, std::vector<double>& x, std::vector<double>& wt) {
  x.assign(n, 0.0);
  wt.assign(n, 0.0);
  for (int i = 0; i < (n + 1) / 2; ++i) {
    double z = std::cos(M_PI * (i + 0.75) / (n + 0.5)), dp = 1.0;
    for (int it = 0; it < 100; ++it) {
      double p0 = 1.0, p1 = z;
      for (int k = 2; k <= n; ++k) {
        const double p2 = ((2.0 * k - 1.0) * z * p1 - (k - 1.0) * p0) / k;
        p0 = p1;
        p1 = p2;
      }
      dp = n * (z * p1 - p0) / (z * z - 1.0);
      const double dz = p1 / dp;
      z -= dz;
      if (std::fabs(dz) < 1e-16) break;
    }
    x[i] = -z;
    x[n - 1 - i] = z;
    wt[i] = wt[n - 1 - i] = 2.0 / ((1.0 - z * z) * dp * dp);
  }
}

// Grid signals: with FPTA_OPT_GRID_COALESCE, a signal joins the first earlier grid signal with the same base
// frequency w0 on every pulsar and the same chromatic weight (factor x mask) on every TOA. Their sums
// ch(t) sum_k c_k cos(k w0 t) + s_k sin(k w0 t) then add in coefficient space (k_coef_merge): one DFT, one band.
inline void plan_coalesce(const PlanLayout& L, const PlanOptions& o, HostGridPlan& H) {
  const int32_t n_layout = (int32_t)L.sigs.size();
  std::vector<std::vector<double>> chv(n_layout);
  auto ch_of = [&](int32_t i) -> const std::vector<double>& {
    if (chv[i].empty()) {
      const PlanSignal& d = L.sigs[i];
      chv[i].resize(L.n_toa);
      for (int64_t t = 0; t < L.n_toa; ++t) {
        double ch = 1.0;  // chrom_factor (device_common.h), same operations
        if (d.idx != 0.0) {
          const double x = d.freqf / L.nu[t];
          ch = d.idx == 2.0 ? x * x : d.idx == 1.0 ? x : std::pow(x, d.idx);
        }
        chv[i][t] = (d.mask && !d.mask[t]) ? 0.0 : ch;
      }
    }
    return chv[i];
  };
  auto w0_of = [&](int32_t i, int32_t p) { return L.sigs[i].w0[L.sigs[i].kind == 0 ? p : 0]; };
  for (int32_t i = 0; i < n_layout; ++i) {
    int32_t join = -1;
    for (size_t g = 0; o.coalesce && g < H.members.size() && join < 0; ++g) {
      // a grid signal merges at most kGridMaxSeg other members (CoefMerge::src): a full group starts a new one
      if (H.members[g].size() > (size_t)kGridMaxSeg) continue;
      const int32_t f = H.members[g][0];
      bool same = true;
      for (int32_t p = 0; p < L.P && same; ++p) same = w0_of(i, p) == w0_of(f, p);
      if (same) same = ch_of(i) == ch_of(f);
      if (same) join = (int32_t)g;
    }
    if (join < 0) {
      H.members.push_back({i});
    } else {
      H.members[join].push_back(i);
      H.merges = true;
    }
  }
  for (const std::vector<int32_t>& m : H.members) {
    int32_t a = m[0];
    for (int32_t i : m)
      if (L.sigs[i].nm > L.sigs[a].nm) a = i;
    H.anchor.push_back(a);
    H.last.push_back(m.back());
  }
}

// Per grid signal: the options' (w, sigma) give nf0 = sigma (2 N + 1) grid points, a multiple of 4 (the MFMA DFT
// runs on the quarter range); it computes whole blocks of kGridDftRows rows of the quarter range, so nf1 = 4 (rows
// of those blocks - 1) points cost it nothing more. The larger effective oversampling sigma1 = nf1 / (2 N + 1)
// reaches the options' design estimate with a narrower kernel w1; the signal takes (nf1, w1) when its interpolation
// band (w + the cells a 32-TOA chunk spans) is estimated narrower. Then per (signal, TOA) the first interpolation
// row J (unwrapped) and the offset d = u - J, u = theta / h. False: a phase is out of range.
inline bool plan_grid_sizes(const PlanLayout& L, const PlanOptions& o, HostGridPlan& H) {
  const double bound_target = H.err_bound;
  H.err_bound = 0.0;
  for (size_t s = 0; s < H.segs.size(); ++s) {
    PlanSeg& g = H.segs[s];
    const PlanSignal& d = L.sigs[H.anchor[s]];
    g.nm = d.nm;
    int32_t n = (int32_t)std::ceil(o.sigma * (2.0 * d.nm + 1.0));
    int32_t n0 = (std::max(n, 2 * o.w + 2) + 3) / 4 * 4, w0 = o.w;
    // grid cells per TOA per grid point: mean over pulsars of w0 dt / (2 pi), dt the mean TOA spacing
    double rho = 0.0;
    for (int32_t p = 0; p < L.P; ++p) {
      const int64_t a0 = L.offs[p], a1 = L.offs[p + 1];
      double tmin = L.toas[a0], tmax = L.toas[a0];
      for (int64_t t = a0; t < a1; ++t) {
        tmin = std::min(tmin, L.toas[t]);
        tmax = std::max(tmax, L.toas[t]);
      }
      if (a1 - a0 > 1) rho += d.w0[d.kind == 0 ? p : 0] * (tmax - tmin) / (double)(a1 - a0 - 1) / (2.0 * M_PI);
    }
    rho /= L.P;
    const int32_t blocks = (n0 / 4 + kGridDftRows) / kGridDftRows;  // ceil((nf / 4 + 1) / rows per block)
    const int32_t n1 = 4 * (blocks * kGridDftRows - 1);
    const double sig1 = n1 / (2.0 * d.nm + 1.0);
    int32_t w1 = o.w;
    while (w1 > 4 && std::exp(-M_PI * (w1 - 1) * std::sqrt(1.0 - 1.0 / sig1)) <= bound_target) --w1;
    const bool fill = n1 > n0 && 2 * w1 + 2 <= n1 && w1 + kGridTT * n1 * rho < w0 + kGridTT * n0 * rho - 0.25;
    g.nf = fill ? n1 : n0;
    g.w = fill ? w1 : w0;
    const double sig = g.nf / (2.0 * d.nm + 1.0);
    // shape parameter of the exponential-of-semicircle kernel for oversampling sigma (2.31 w at sigma = 2)
    g.beta = 0.98 * M_PI * g.w * (1.0 - 0.5 / sig);
    H.err_bound = std::max(H.err_bound, std::exp(-M_PI * g.w * std::sqrt(1.0 - 1.0 / sig)));
    const double hw = 0.5 * g.w;
    const double h = 2.0 * M_PI / g.nf;
    g.J.resize(L.n_toa);
    g.d.resize(L.n_toa);
    for (int32_t p = 0; p < L.P; ++p) {
      const double w0 = d.w0[d.kind == 0 ? p : 0];
      for (int64_t t = L.offs[p]; t < L.offs[p + 1]; ++t) {
        const double u = (w0 * L.toas[t]) / h;
        if (!std::isfinite(u) || std::fabs(u) > 1e15) {
          H.why = "gridded path: phase out of range";
          return false;
        }
        const int64_t j = (int64_t)std::floor(u - hw) + 1;
        g.J[t] = j;
        g.d[t] = u - (double)j;
      }
    }
  }
  return true;
}

// Chunks: <= kGridTT consecutive TOAs of one pulsar, every signal's band <= kGridRowCap rows; J becomes the row of the
// TOA's first weight in its signal's band. False: too many chunks.
inline bool plan_chunks(const PlanLayout& L, HostGridPlan& H) {
  const int32_t n_seg = H.n_seg();
  H.chunk_of.resize(L.n_toa);
  H.tt_of.resize(L.n_toa);
  std::vector<int64_t> lo(n_seg), hi(n_seg);
  for (int32_t p = 0; p < L.P; ++p) {
    int64_t t = L.offs[p];
    const int64_t t_end = L.offs[p + 1];
    while (t < t_end) {
      const int64_t t0 = t;
      for (int32_t s = 0; s < n_seg; ++s) lo[s] = hi[s] = H.segs[s].J[t];
      ++t;
      // chunks end on multiples of kGridTT in the global TOA index: every full chunk then writes whole
      // 256-byte runs of each realization row
      const int64_t t_lim = std::min(t_end, (t0 / kGridTT + 1) * kGridTT);
      while (t < t_lim) {
        bool fits = true;
        for (int32_t s = 0; s < n_seg && fits; ++s) {
          const int64_t j = H.segs[s].J[t];
          fits = std::max(hi[s], j) - std::min(lo[s], j) + H.segs[s].w + 1 <= kGridRowCap;
        }
        if (!fits) break;
        for (int32_t s = 0; s < n_seg; ++s) {
          lo[s] = std::min(lo[s], H.segs[s].J[t]);
          hi[s] = std::max(hi[s], H.segs[s].J[t]);
        }
        ++t;
      }
      const int32_t ci = H.n_chunks();
      H.chunks.push_back(Int4{p, (int32_t)(t0 - L.offs[p]), (int32_t)(t - t0), 0});
      for (int64_t u = t0; u < t; ++u) {
        H.chunk_of[u] = ci;
        H.tt_of[u] = (int32_t)(u - t0);
      }
      for (int32_t s = 0; s < n_seg; ++s) {
        PlanSeg& g = H.segs[s];
        g.band_lo.push_back(lo[s]);
        g.band_n.push_back((int32_t)(hi[s] - lo[s]) + g.w);
        for (int64_t u = t0; u < t; ++u) g.J[u] -= lo[s];  // row of the TOA's first weight in its band
      }
    }
  }
  if (H.chunks.size() > (size_t)0x7FFFFFFF / 8) {
    H.why = "gridded path: too many chunks";
    return false;
  }
  const int32_t n_chunks = H.n_chunks();
  H.psr_chunk0.assign((size_t)L.P + 1, 0);
  for (int32_t ci = n_chunks - 1; ci >= 0; --ci) H.psr_chunk0[H.chunks[ci].x] = ci;
  H.psr_chunk0[L.P] = n_chunks;
  for (int32_t p = L.P - 1; p >= 0; --p)  // a pulsar without TOAs has no chunk: it starts where the next one does
    if (L.offs[p + 1] == L.offs[p]) H.psr_chunk0[p] = H.psr_chunk0[p + 1];
  return true;
}

// Band rows of a chunk: every signal's band back to back (virtual rows voff_s ..), padded to a multiple of 4 once per
// chunk (k_grid_interp_mfma: 4 rows per MFMA step; pad rows re-read a valid row at weight 0), and in diagnostic builds
// to at least kGridMinV rows (k_grid_interp_st's operand lookahead never passes the next chunk; the product kernels
// would only run zero-weight steps on them). rows [n_chunks][vmax]: the grid-buffer row of each band row, signal s's
// grid block at row rowoff_s. False: too many band rows, or too large a grid.
inline bool plan_band_tables(const PlanLayout& L, HostGridPlan& H) {
  const int32_t n_chunks = H.n_chunks();
  for (PlanSeg& g : H.segs) g.voff.resize(n_chunks);
  int32_t vmax = 4;
  for (int32_t ci = 0; ci < n_chunks; ++ci) {
    int32_t v = 0;
    for (PlanSeg& g : H.segs) {
      g.voff[ci] = v;
      v += g.band_n[ci];
    }
    H.chunks[ci].w = (v + 3) & ~3;
#ifdef FPTA_DIAG_KERNELS
    H.chunks[ci].w = std::max(kGridMinV, H.chunks[ci].w);
#endif
    vmax = std::max(vmax, H.chunks[ci].w);
  }
  if (vmax > kGridVMax) {
    H.why = "gridded path: a chunk's band rows over all signals exceed " + std::to_string(kGridVMax);
    return false;
  }
  H.vmax = vmax;
  int64_t grid_rows = 0;
  for (PlanSeg& g : H.segs) {
    g.rowoff = grid_rows;
    grid_rows += (int64_t)L.P * g.nf;
  }
  if (grid_rows > 0x7FFFFFFF) {
    H.why = "gridded path: grid too large";
    return false;
  }
  H.grid_rows = grid_rows;
  H.rows.resize((size_t)n_chunks * vmax);
  for (int32_t ci = 0; ci < n_chunks; ++ci) {
    int32_t* r = H.rows.data() + (size_t)ci * vmax;
    const int32_t p = H.chunks[ci].x;
    int32_t v = 0;
    for (const PlanSeg& g : H.segs)
      for (int32_t i = 0; i < g.band_n[ci]; ++i)
        r[v++] = (int32_t)(g.rowoff + (int64_t)p * g.nf + plan_wrap(g.band_lo[ci] + i, g.nf));
    for (; v < vmax; ++v) r[v] = r[0];
  }
  // weight rows of signal s: its band's virtual offset in the chunk + the TOA's first row in the band
  for (PlanSeg& g : H.segs) {
    g.row.resize(L.n_toa);
    for (int64_t t = 0; t < L.n_toa; ++t) g.row[t] = (int32_t)g.J[t] + g.voff[H.chunk_of[t]];
  }
  // + kFusedPadRows band rows after the last chunk: k_grid_fused loads NQ band steps' weights of every chunk unclamped
  H.wd_size = ((size_t)n_chunks * vmax + kFusedPadRows) * kGridTT;
  for (int32_t ci = 0; ci < n_chunks; ++ci) H.fma_interp += (double)H.chunks[ci].w * kGridTT;
  H.mean_v = H.fma_interp / kGridTT / std::max(n_chunks, 1);
  H.weight_bytes = (double)(sizeof(double) * H.wd_size);
  return true;
}

// Deconvolution tables of every grid signal, and the plan's FMA figures.
// q_k = (2 pi / nf) / phi_hat(k), phi_hat(k) = alpha int_{-1}^{1} phi(z) cos(k alpha z) dz, alpha = pi w / nf
inline void plan_deconv_tables(const PlanLayout& L, const PlanOptions& o, HostGridPlan& H) {
  std::vector<double> gx, gw;
  gauss_legendre(256, gx, gw);
  for (const PlanSignal& d : L.sigs) H.fma_direct += 2.0 * d.nm * (double)L.n_toa;
  for (PlanSeg& g : H.segs) {
    g.half = g.nf / 2;
    g.lde = (g.half + kGridDftRows) / kGridDftRows * kGridDftRows;  // row blocks of k_grid_dft_mfma and k_grid_dft
    g.ntab = (g.nm + 7) / 8 * 8;         // whole pairs of 4-mode MFMA k-steps (zero rows)
    const double alpha = M_PI * g.w / g.nf, beta = g.beta;
    g.ecos.assign((size_t)g.ntab * g.lde, 0.0);
    g.esin.assign((size_t)g.ntab * g.lde, 0.0);
    for (int32_t m = 0; m < g.nm; ++m) {
      const int64_t k = m + 1;
      double ph = 0.0;
      for (size_t q = 0; q < gx.size(); ++q)
        ph += gw[q] * std::exp(beta * (std::sqrt(1.0 - gx[q] * gx[q]) - 1.0)) * std::cos(k * alpha * gx[q]);
      const double qk = (2.0 * M_PI / g.nf) / (alpha * ph);
      for (int32_t j = 0; j <= g.half; ++j) {
        const double a = 2.0 * M_PI * (double)((k * j) % g.nf) / g.nf;  // exact argument reduction
        g.ecos[(size_t)m * g.lde + j] = qk * std::cos(a);
        g.esin[(size_t)m * g.lde + j] = qk * std::sin(a);
      }
    }
    // quarter-range tables by parity: [0] cos / [1] sin of odd k = 2 t + 1 (m = 2 t), [2] / [3] of even k = 2 t + 2
    g.ldq = (g.nf / 4 + kGridDftRows) / kGridDftRows * kGridDftRows;
    g.ntq = ((g.nm + 1) / 2 + 7) / 8 * 8;
    g.tq.assign((size_t)4 * g.ntq * g.ldq, 0.0);
    for (int32_t m = 0; m < g.nm; ++m) {
      const int32_t par = m & 1, t = m >> 1;
      for (int32_t j = 0; j <= g.nf / 4; ++j) {
        g.tq[((size_t)(2 * par) * g.ntq + t) * g.ldq + j] = g.ecos[(size_t)m * g.lde + j];
        g.tq[((size_t)(2 * par + 1) * g.ntq + t) * g.ldq + j] = g.esin[(size_t)m * g.lde + j];
      }
    }
    // multiply-adds per realization: quarter range by parity on MFMA, half range on VALU
    H.fma_dft += (double)L.P * ((o.grid_mfma & 1) ? (g.nf / 4 + 1) * 2.0 * g.nm : (g.half + 1) * 2.0 * g.nm);
    H.grid_vals += (double)L.P * g.nf;
    H.fma_grid = H.fma_dft + H.fma_interp;
  }
}

// A band's LDS rows by band step, [4][fq]: band row 4 q + j at [j][q] (a lane's rows of consecutive steps contiguous:
// 16-byte loads); steps past the band's n rows repeat its first row.
inline void plan_step_rows(const std::vector<int32_t>& band_row, int32_t n, int32_t fq, int32_t* r) {
  for (int32_t j = 0; j < 4; ++j)
    for (int32_t q = 0; q < fq; ++q) r[j * fq + q] = 4 * q + j < n ? band_row[4 * q + j] : band_row[0];
}

// k_grid_fused: the grids of kFusedReal realizations plus the draw ring fit in LDS, n_seg <= kFusedMaxSig, and every
// 32-row DFT chunk is one DFT wave's job. frows [n_chunks][4][fq], fq = the band steps rounded up to 4 and at least
// kFusedFqMin.
inline void plan_fused_rows(HostGridPlan& H) {
  const int32_t n_seg = H.n_seg(), n_chunks = H.n_chunks(), vmax = H.vmax;
  int32_t jobs = 0, rows = 0;
  bool ok = n_seg <= kFusedMaxSig;
  for (int32_t s = 0; s < n_seg && ok; ++s) {
    const PlanSeg& g = H.segs[s];
    ok = g.nf % 4 == 0 && g.ldq == (g.nf / 4 + 32) / 32 * 32;
    H.fused_lrow0.push_back(rows);
    jobs += (g.nf / 4 + 32) / 32;
    rows += g.nf;
  }
  H.fused_lds = sizeof(double) * ((size_t)rows * kFusedPitch + 2 * kFusedMaxSig * kFusedSlot) + 48;
  bool members_ok = true;
  for (const std::vector<int32_t>& m : H.members) members_ok = members_ok && m.size() <= (size_t)kDftGenTerms;
  H.fused_ok = ok && members_ok && jobs <= kFusedDW && H.fused_lds <= (size_t)kFusedLdsMax;
  if (!H.fused_ok) return;
  H.fused_fq = std::max(kFusedFqMin, (vmax / 4 + 3) & ~3);
  std::vector<int32_t> band_row(vmax);
  H.frows.resize((size_t)n_chunks * 4 * H.fused_fq);
  for (int32_t ci = 0; ci < n_chunks; ++ci) {
    int32_t v = 0;
    for (int32_t s = 0; s < n_seg; ++s)
      for (int32_t i = 0; i < H.segs[s].band_n[ci]; ++i)
        band_row[v++] = H.fused_lrow0[s] + plan_wrap(H.segs[s].band_lo[ci] + i, H.segs[s].nf);
    for (; v < vmax; ++v) band_row[v] = band_row[0];
    plan_step_rows(band_row, vmax, H.fused_fq, H.frows.data() + (size_t)ci * 4 * H.fused_fq);
  }
}

// Half-chunk bands (FusedHalf): TOAs 0..15 and 16..31 of each chunk get bands of their own (a 32-TOA chunk's band
// is w + the cells its 32 TOAs span; a half's, w + the cells of 16). Per half the signals' bands back to back,
// padded to whole band steps; the weights by the half-band layout of k_grid_weights.
inline void plan_half_bands(const PlanLayout& L, HostGridPlan& H) {
  const int32_t n_seg = H.n_seg(), n_chunks = H.n_chunks();
  const int64_t N = L.n_toa;
  H.hchunks.resize(n_chunks);
  H.hv.assign((size_t)2 * n_chunks, 0);
  H.hchunk_of.resize(N);
  H.htt_of.resize(N);
  std::vector<std::vector<int64_t>> hlo(n_seg, std::vector<int64_t>((size_t)2 * n_chunks, 0));
  std::vector<std::vector<int32_t>> hvoff(n_seg, std::vector<int32_t>((size_t)2 * n_chunks, 0));
  std::vector<std::vector<int32_t>> hn(n_seg, std::vector<int32_t>((size_t)2 * n_chunks, 0));
  double steps_full = 0.0, steps_half = 0.0;
  for (int32_t ci = 0; ci < n_chunks; ++ci) {
    const Int4& ch = H.chunks[ci];
    const int64_t a0 = L.offs[ch.x] + ch.y, a1 = a0 + ch.z;
    int32_t nqh[2] = {0, 0};
    for (int32_t h = 0; h < 2; ++h) {
      const int64_t b0 = a0 + kFusedHalfTT * h, b1 = std::min(a1, b0 + kFusedHalfTT);
      if (b0 >= b1) continue;
      const size_t hc = (size_t)2 * ci + h;
      int32_t v = 0;
      for (int32_t s = 0; s < n_seg; ++s) {
        int64_t lo1 = INT64_MAX, hi1 = INT64_MIN;
        for (int64_t u = b0; u < b1; ++u) {
          const int64_t j = H.segs[s].J[u] + H.segs[s].band_lo[ci];  // unwrapped first row of the TOA
          lo1 = std::min(lo1, j);
          hi1 = std::max(hi1, j);
        }
        hlo[s][hc] = lo1;
        hvoff[s][hc] = v;
        hn[s][hc] = (int32_t)(hi1 - lo1) + H.segs[s].w;
        v += hn[s][hc];
      }
      H.hv[hc] = (v + 3) & ~3;
      nqh[h] = H.hv[hc] / 4;
      for (int64_t u = b0; u < b1; ++u) {
        H.hchunk_of[u] = 2 * ci + h;
        H.htt_of[u] = (int32_t)(u - b0);
      }
    }
    H.hchunks[ci] = Int4{ch.x, ch.y, ch.z, nqh[0] | (nqh[1] << 16)};
    steps_full += 4.0 * (ch.w / 4);
    steps_half += 4.0 * std::max(nqh[0], nqh[1]);  // the kernel runs both halves' longer step count
  }
  int32_t hvmax = 8, hnq = 1;
  for (int32_t v : H.hv) {
    hvmax = std::max(hvmax, (v + 7) & ~7);
    hnq = std::max(hnq, v / 4);
  }
  const int32_t hfq = std::max(kFusedHalfNQ, (hvmax / 4 + 3) & ~3);
  H.hrows.resize((size_t)n_chunks * 2 * 4 * hfq);
  for (size_t hc = 0; hc < (size_t)2 * n_chunks; ++hc) {
    std::vector<int32_t> band_row(std::max(H.hv[hc], 1), H.fused_lrow0[0]);
    int32_t v = 0;
    for (int32_t s = 0; s < n_seg; ++s)
      for (int32_t i = 0; i < hn[s][hc]; ++i)
        band_row[v++] = H.fused_lrow0[s] + plan_wrap(hlo[s][hc] + i, H.segs[s].nf);
    for (; v < (int32_t)band_row.size(); ++v) band_row[v] = band_row[0];
    plan_step_rows(band_row, H.hv[hc], hfq, H.hrows.data() + hc * 4 * hfq);
  }
  for (int32_t s = 0; s < n_seg; ++s) {
    PlanSeg& g = H.segs[s];
    g.hrow_of.resize(N);
    for (int64_t t = 0; t < N; ++t) {
      const size_t hc = (size_t)H.hchunk_of[t];
      g.hrow_of[t] = (int32_t)(g.J[t] + g.band_lo[hc / 2] - hlo[s][hc]) + hvoff[s][hc];
    }
  }
  // + the rows the kernel's unconditional loads may read past the last half (kFusedHalfNQ steps)
  H.hwd_size = ((size_t)2 * n_chunks * hvmax + 4 * kFusedHalfNQ) * kFusedHalfTT;
  H.fused_hfq = hfq;
  H.fused_hvmax = hvmax;
  H.fused_hnq = hnq;
  H.fused_half_gain = steps_half > 0.0 ? steps_full / steps_half : 0.0;
  H.fma_interp_half = steps_half * 4.0 * kGridTT / 4.0;  // 4 rows x 32 TOAs per (both-halves) step
  H.fused_half_ok = true;
}

// The gridded plan of layout L: per grid signal the grid size nf and the deconvolved real-DFT tables, the chunking of
// every pulsar's TOAs into runs of <= kGridTT whose interpolation rows span at most kGridRowCap cells, the band-row
// tables, and k_grid_fused's plan. Not usable -> ok = false + why (what the stages before the refusal made stays).
inline HostGridPlan plan_grid(const PlanLayout& L, const PlanOptions& o) {
  HostGridPlan H;
  H.err_bound = std::exp(-M_PI * o.w * std::sqrt(1.0 - 1.0 / o.sigma));
  if (L.sigs.empty()) {
    H.why = "gridded path: no signals";
    return H;
  }
  for (const PlanSignal& d : L.sigs)
    if (!d.harmonic) {
      H.why = "gridded path: every signal needs a harmonic grid f_k = k f_1";
      return H;
    }
  plan_coalesce(L, o, H);
  if (H.members.size() > (size_t)kGridMaxSeg) {
    H.why = "gridded path: needs 1.." + std::to_string(kGridMaxSeg) + " grid signals (after coalescing)";
    return H;
  }
  H.segs.resize(H.members.size());  // grid signals from here on
  if (!plan_grid_sizes(L, o, H) || !plan_chunks(L, H) || !plan_band_tables(L, H)) return H;
  plan_deconv_tables(L, o, H);
  plan_fused_rows(H);
  if (H.fused_ok) plan_half_bands(L, H);
  H.ok = true;
  return H;
}

}  // namespace fpta
