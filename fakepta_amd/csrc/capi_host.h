// Host side of libfakepta_amd.so shared by its translation units (not part of the C-ABI): capi.hip (context, options,
// drop-in and batch entry points, path selection, dense covariance), grid_host.hip (the gridded plan and its launches)
// and multi.hip (several devices in one process; one process per GPU over RCCL). All arithmetic on the path runs in
// the kernels (kernels.hip, grid_mfma.hip, grid_fused.hip, dense.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/fakepta_amd.h"
#include "fpta_internal.h"

using namespace fpta;

namespace fpta_os {
struct Plan;  // os_host.h
}

namespace __attribute__((visibility("hidden"))) capi {  // library-internal: not exported

extern thread_local std::string g_err;  // the last error of a call without a context

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  void swap(DevBuf& o) {
    std::swap(p, o.p);
    std::swap(cap, o.cap);
  }
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap && p) return hipSuccess;
    release();
    size_t want = std::max<size_t>(bytes, 256);
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) {
      p = nullptr;
      return e;
    }
    cap = want;
    return hipSuccess;
  }
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

struct Seg {
  SegDesc d{};
  int32_t nm_orig = 0;
  std::vector<double> h_w0;  // first angular frequency per row ([P] for kind 0, [1] for kind 1)
  std::vector<uint8_t> h_mask;  // host copy of the TOA mask (empty: none), for grid coalescing
  // per-realization spectra (spectra.hip): the amplitudes as uploaded [rows][nm] (the zero rule), and {f, delta f}
  // [rows][nm][2] of the frequencies as given (delta f = f_k - f_{k-1}, f_{-1} = 0; padding mode: zeros), uploaded
  // into fdf by the first power-law table of the signal
  std::vector<double> h_amp, h_fdf;
  DevBuf w, amp, L, LT, mask, fdf;
};

// Gridded-synthesis tables of one signal (grid.hip): real-DFT table E; its grid block starts at row rowoff of
// the plan's grid buffer.
struct GridSeg {
  int32_t nf = 0, half = 0, lde = 0, ntab = 0;
  int64_t rowoff = 0;
  DevBuf ecos, esin;  // half-range tables (k_grid_dft)
  int32_t ldq = 0, ntq = 0;
  DevBuf tq;          // quarter-range tables by mode parity (k_grid_dft_mfma)
};

// Gridded-synthesis plan of a layout (built once per layout, reused by every batch).
// fpta_batch_grid_info_n slot 15 (1 + 4 kind + 2 white + part): kinds 0 .. 10 the interpolation kernels
// (_capi.interp_kernel_name), kInterpKindFused0 + i k_grid_fused instance i of launch_grid_fused's table
constexpr int kInterpKindFused0 = 11;
struct GridPlan : PlanFigures {  // the plan's host-side figures: grid_plan.h
  bool built = false;
  int32_t w = 0;             // kernel width (grid cells)
  double sigma = 0.0;        // oversampling
  int32_t n_chunks = 0;
  DevBuf chunks;             // int4 {pulsar, first TOA (pulsar-local), count, band rows V (multiple of 4)}
  DevBuf rows;               // [n_chunks][vmax] int32 grid-buffer row of each band row (all signals back to back)
  DevBuf wd;                 // [n_chunks][vmax][kGridTT] interpolation weights (chromatic factor, mask folded in)
  DevBuf g, g2;              // [grid_rows][R_pad] grid values of the batch (two buffers when pipelined)
  // partial-checksum groups (FPTA_OPT_FUSE_CHECKSUMS): <= pg_size consecutive chunks of one pulsar each; pgfirst
  // [n_pg + 1] the first chunk of each group, psr_pg [P + 1] the first group of each pulsar
  int32_t pg_size = 0, n_pg = 0;
  DevBuf pgfirst, psr_pg;
  DevBuf psr_c0;  // device copy of psr_chunk0 (k_grid_interp_psr without partial checksums)
  DevBuf frows;  // k_grid_fused: [n_chunks][4][fused_fq] the LDS row of each band row
  // half-chunk bands of the fused kernel (FusedHalf): hchunks {pulsar, first TOA, count, nq0 | nq1 << 16}, hrows
  // [n_chunks][2][4][fused_hfq], hwd [2 n_chunks][fused_hvmax][16] (+ padding)
  DevBuf hchunks, hrows, hwd;
  // The diagnostic kernels' plans (diag/grid_plan_diag.h): made in variant builds only, cleared in the product library
  struct Diag {
    // k_grid_interp_wr plan (GridWindow): <= 2 grid signals, each signal's band rows in a ring of kWrSlots LDS slots by
    // unwrapped row; per chunk the slot of each band row, and the rows to load: all its band rows (full) or those not
    // in the previous chunk's band (new; = full and flagged fresh when the two bands do not fit one ring window)
    bool wr_ok = false;
    DevBuf wr_meta, wr_list, wr_slot;
    // k_grid_interp_lds plan: groups int4 {first chunk, chunks, union rows U, offset into urows}; urows the grid-
    // buffer rows of each group's union; lrows [n_chunks][vmax] the union slot of each band row
    bool lds_ok = false;
    int32_t n_groups = 0, lds_rows = 0;
    DevBuf groups, urows, lrows;
    // k_grid_interp_u plan (GridUnion): groups of <= kUnionGroup chunks with <= kUnionRowsMax union rows; per chunk the
    // signals' band offsets and union bases; per (chunk, signal, TOA slot) the window's first band row and {d, ch}
    bool u_ok = false;
    int32_t u_groups = 0, u_sig = 0;
    DevBuf ugroups, uurows, ucbase, udch, uwrow;
    int32_t u_w[kUnionSigMax] = {0, 0};
    double u_hw[kUnionSigMax] = {0.0, 0.0}, u_beta[kUnionSigMax] = {0.0, 0.0};
    void clear() {
      wr_ok = lds_ok = u_ok = false;
      n_groups = lds_rows = u_groups = u_sig = 0;
    }
  } diag;
  std::vector<GridSeg*> segs;  // one per grid signal
  int64_t g_rpad = 0;        // R_pad the grid buffers are sized for
  ~GridPlan() { clear(); }
  void clear() {
    for (GridSeg* g : segs) delete g;
    segs.clear();
    static_cast<PlanFigures&>(*this) = PlanFigures();
    built = false;
    n_chunks = 0;
    diag.clear();
    g_rpad = 0;
    pg_size = n_pg = 0;
  }
};

// A device-resident pulsar array plus its GP signals.
struct Layout {
  int32_t P = 0;
  int64_t n_toa = 0;
  int64_t max_np = 0;
  std::vector<int64_t> h_offs;
  std::vector<double> h_toas, h_nu;
  DevBuf offs, toas, nu, psr_of;
  std::vector<Seg*> segs;
  DevBuf segdesc;
  int32_t K = 0;
  bool dirty = true;
  uint64_t version = 0;  // bumped by every layout_finalize that rebuilds (signals, TOAs changed)
  // recurrence seeds [n_seg][n_toa] (double4), valid when every segment is harmonic
  DevBuf seeds;
  bool all_harmonic = false;
  // tile table cache of the tiled synthesis kernels: valid for (tiles_toa, tiles_real, tiles_n_real)
  DevBuf tiles;
  int32_t n_tiles = 0;
  int32_t tiles_toa = 0, tiles_real = 0;
  int64_t tiles_n_real = -1;
  GridPlan grid;
  ~Layout() { clear_signals(); }
  void clear_signals() {
    for (Seg* s : segs) delete s;
    segs.clear();
    K = 0;
    dirty = true;
    tiles_n_real = -1;
    grid.clear();
  }
};

// The consumers of the block that fpta_batch_synth leaves on the device (tm.hip, fit.hip, os.hip, lnl.hip, fe.hip,
// clnl.hip). A slot owns the device tables and results of one feature: the context holds one for the batch layout and
// one for the feature's one-shot call. A state says what the batch slot holds (set: the feature is set; R, rpad: the
// realizations of its last result, 0: none, and their padding); it is all zero while the feature is not set, and
// fpta_batch_set_toas clears it.

// A block [R][ld] of residuals on the device, rows of n_psr pulsars: the resident block, or a one-shot call's upload
struct Block {
  double* res = nullptr;
  int64_t ld = 0;
  int32_t R = 0, n_psr = 0;
};

// Timing-model projection: the basis Q [n_toa][16], s = sqrt(w), CSR offsets and ranks
struct TmSlot {
  DevBuf q, s, offs, rank;
};
struct TmState {
  bool set = false;
  void clear() { *this = TmState(); }
};

// The operator slot k_fit_apply runs on: pulsar p's operator [K][n_p] at K offs[p], CSR offsets, the rows to make per
// pulsar (the Fourier fit: its kept-column counts; 0 skips the pulsar) and the coefficients [P][K][rpad]
struct FitSlot {
  DevBuf a, offs, rows, coef;
};
struct FitState {
  bool set = false, common = false;  // common: one frequency grid for the array
  int32_t K = 0, modes = 0, R = 0, rpad = 0;
  void clear() { *this = FitState(); }
};

// Optimal statistic: k_fit_apply's second operator slot (B_p, X), the template phi_hat [N], the J pair-weight matrices
// [J][P][P] and the results Q_mode [J][N][rpad], Q [J][rpad]; the plan's N_ab [P][P] for the sky scrambles, on the
// device and on the host
constexpr int kOsRpad = 32;  // k_fit_apply's realization padding, which the statistic's kernels rely on
struct OsSlot {
  FitSlot x;
  DevBuf phi, g, qm, q, nab;
  std::vector<double> h_nab;
};
struct OsState {
  bool set = false;
  int32_t K = 0, N = 0, J = 0, R = 0, rpad = 0;  // K = 2 N: the target's Fourier columns
  void clear() { *this = OsState(); }
};

// Likelihood grid: k_fit_apply's third operator slot (B_p with the target left out of the model, X), the factors U
// [P][G][u_stride] (lnl_host.h's layout), the log-determinants [P][G] and the results q [P][G][rpad], dlnL [G][rpad]
struct LnlSlot {
  FitSlot x;
  DevBuf u, ld, q, d;
};
struct LnlState {
  bool set = false;
  int32_t K = 0, N = 0, G = 0, R = 0, rpad = 0;  // K = 2 N: the target's Fourier columns
  void clear() { *this = LnlState(); }
};

// Continuous-wave F-statistics: k_fit_apply's fourth operator slot (B_p with the frequency grid as rows, X), the antenna
// table in k_fe_sky's tile layout [tiles of 8 directions][k-steps of 4 pulsars][64 lanes], M^-1 [n_sky][G][10], m^-1
// [P][G][3] and the results Fe_f / arg [G][rpad], Fe_max / arg [rpad] (the argmax as direction and frequency), Fp
// [G][rpad] and, when asked for, the map [n_sky][G][rpad]
struct FeSlot {
  FitSlot x;
  DevBuf f, minv, pinv, fef, argf, femax, argmax, fp, map;
};
struct FeState {
  bool set = false;
  int32_t K = 0, G = 0, n_sky = 0, R = 0, rpad = 0;  // K = 2 G: the cosine rows, then the sine rows
  void clear() { *this = FeState(); }
};

// Correlated likelihood grid: k_fit_apply's fifth operator slot (B_p with the target left out of the model, X), the ORF
// factors A [n_orf][P][P], T [n_orf][n_pad][n_pad], the scalings s [G][n_pad], the cached Cholesky factors l
// [n_orf][G][n_pad][n_pad] with their log-determinants ld [n_orf][G] (pt, info: the factorisation's panel and info
// word), V [n_pad][vld], the substitution's Y tiles [n_orf][G][vld / 64][n_pad][64] and the results q, d
// [n_orf][G][rpad]
struct ClnlSlot {
  FitSlot x;
  DevBuf a, t, s, l, ld, pt, info, v, y, q, d;
};
struct ClnlState {
  bool set = false;
  int32_t K = 0, G = 0, n_orf = 0, R = 0, rpad = 0;  // K = 2 N: the target's Fourier columns per pulsar
  int64_t n = 0, n_pad = 0;                          // P K and its round-up to 64
  void clear() { *this = ClnlState(); }
};

// Optimal statistic under a spectrum per realization (os_spectra.hip): k_fit_apply's sixth operator slot (B0_p, z
// [P][q][rpad]), A_p [P][q][q], the template phi_hat [N] and its square
// roots over the K columns, the J pair-weight matrices, the call's raw tables and amplitude tables [P or 1][nm][rpad]
// (k_spectra_amp), and the results X [P][K][rpad], Z' and N_ab of one realization chunk, the contractions
// [J + n_orf^2][R], Q_mode [J][N][rpad], Q [J][rpad]
struct OssSlot {
  FitSlot x;
  DevBuf a, phi, sph, g, raw, tab, xc, zp, nab, nrm, qm, q;
};
struct OssState {
  bool set = false;
  int32_t q = 0, K = 0, N = 0, J = 0, n_orf = 0, n_vary = 0, R = 0, rpad = 0;  // K = 2 N: the last K of the q columns
  int32_t seg[4] = {0, 0, 0, 0};                                            // the layout signal of each varied component
  void clear() { *this = OssState(); }
};

// Sky scrambles of the optimal statistic (os_scramble.hip), on top of an OsSlot: the pair map [n_pair_pad][2], the
// scrambles' pair rows Gs [J][n_pair_pad] with norm [J] and match [J][n_orf], the observed ORFs' rows Go
// [n_orf][n_pair_pad] with their norms and sums of squares, the call's inputs (positions or matrices), and the results
// Y [n_pair_pad][rpad], Qs [J][rpad], snr_obs and count_ge [n_orf][rpad], the null's mean, std and max [3][rpad] and,
// when asked for, snr_null [J][rpad]
struct ScrSlot {
  DevBuf map, in, gs, norm, ss, match, go, onorm, oss, y, qs, snr, cnt, mom, null;
};
struct ScrState {
  bool set = false;
  int32_t J = 0, n_orf = 0, R = 0, rpad = 0;  // J scrambles against the n_orf matrices of the statistic that is set
  int64_t n_pair = 0, n_pad = 0;
  void clear() { *this = ScrState(); }
};

}  // namespace capi

using namespace capi;

struct fpta_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  Layout batch, scratch;
  // batch white noise
  DevBuf sigma, block_of, esig, zb_epochs, corr_autos, corr_parts, corr_dst;
  bool has_sigma = false, has_blocks = false;
  int64_t n_blocks = 0;
  // work buffers
  DevBuf coef, zbuf, out, sums, zin, xout, hostz, scratch_out, scratch_z, scratch_zb, scratch_sigma,
      scratch_block_of, scratch_esig, dbg_a, dbg_b;
  // fpta_cw_accumulate (cw.hip): TOAs, pulsar positions and light-travel times, per-source and per-(pulsar, source)
  // tables, the 64-TOA wave table, partial sums [n_split][n_toa]
  DevBuf cw_toas, cw_pos, cw_L, cw_ev, cw_gm, cw_pair, cw_waves, cw_part;
  int64_t cw_split = 0;  // FPTA_OPT_CW_SPLIT: 0 auto (fpta_cw::split_count), n >= 1 forces n source splits
  // fpta_batch_cw_accumulate (cw_batch.hip): pulsar positions, light-travel times [P] or [R][P], the CSR offsets of the
  // source tables, the per-source tables of all realizations, the 256-TOA slab table, and the delay vector [n_toa] of
  // the one-table mode
  DevBuf cwb_pos, cwb_L, cwb_offs, cwb_ev, cwb_gm, cwb_slabs, cwb_v;
  // fpta_ephem_* / fpta_roemer_accumulate (ephem.hip): TOAs (or M), the body / row table (or e), pulsar positions,
  // the 64-TOA wave table, the output (planetssb, delays, residuals or E) and sunssb
  DevBuf eph_toas, eph_tab, eph_pos, eph_waves, eph_out, eph_sun;
  // fpta_batch_roemer_accumulate (roemer_batch.hip): pulsar positions, the CSR offsets of the row tables, the row
  // records of all realizations and their base slots, the slots' bodies, the 256-TOA slab table, and the delay vector
  // [n_toa] of the one-table mode
  DevBuf rmb_pos, rmb_offs, rmb_rows, rmb_slots, rmb_bases, rmb_slabs, rmb_v;
  int64_t roemer_chunk = 0;  // FPTA_OPT_ROEMER_CHUNK: 0 auto (fpta_roemerb::chunk_size), n >= 1 forces n (clamped to 32)
  // fpta_orf_anisotropic (orf.hip): pulsar positions, the HEALPix ring table, the maps, the K-split partial tiles of
  // one launch, the ORFs of one launch
  DevBuf orf_pos, orf_rings, orf_h, orf_part, orf_out;
  int64_t orf_split = 0;  // FPTA_OPT_ORF_SPLIT: 0 auto (fpta_orf::make_plan), n >= 1 forces n K-splits
  // The consumers of the resident block, each with the slot of the batch layout, the slot of its one-shot call and the
  // state of the former: the timing-model projection (tm.hip), the Fourier fit (fit.hip; cross_rows the cosine / sine
  // row of every mode and cross_x the cross-spectra of one fpta_batch_fit_cross), the optimal statistic (os.hip), the
  // likelihood grid (lnl.hip), the continuous-wave F-statistics (fe.hip), the correlated likelihood grid (clnl.hip) and
  // the optimal statistic under a spectrum per realization (os_spectra.hip; batch layout only).
  // res1: the residuals of a one-shot call, which ends with the stream idle.
  TmSlot tm, tm1;
  TmState tm_st;
  FitSlot fit, fit1;
  FitState fit_st;
  DevBuf cross_rows, cross_x;
  OsSlot os, os1;
  OsState os_st;
  ScrSlot scr, scr1;
  ScrState scr_st;
  LnlSlot lnl, lnl1;
  LnlState lnl_st;
  FeSlot fe, fe1;
  FeState fe_st;
  ClnlSlot clnl, clnl1;
  ClnlState clnl_st;
  OssSlot oss;
  OssState oss_st;
  DevBuf res1;
  // a new layout: every table above is per TOA of the layout it was set for, and the last results go with them
  void clear_consumers() {
    tm_st.clear();
    fit_st.clear();
    os_st.clear();
    scr_st.clear();
    lnl_st.clear();
    fe_st.clear();
    clnl_st.clear();
    oss_st.clear();
  }
  DevBuf fused_q;  // k_grid_fused's item queues: 8 per-XCD tickets + a done counter, zero between launches
  bool fused_q_ready = false;
  int32_t out_R = 0;
  int64_t out_ld = 0;
  // options
  int synth_path = 0;
  int mfma_min_real = 16;
  int profile = 0;
  int anchor = 0;  // 0: phasor recurrence anchored once per segment
  int valu_variant = 1;  // seeded (MT 2, NT 16): fastest on C2 (profiles/r01_sweep_*.txt)
  int fuse_white = 1;    // add white/ECORR in the seeded kernel's epilogue
  int fuse_sums = 0;     // gridded path: interpolation writes partial checksums (FPTA_OPT_FUSE_CHECKSUMS)
  int mix_mfma = 1;      // ORF mixing of large arrays on fp64 MFMA (k_mix_mfma) or VALU (k_mix_tiled)
  // batch coefficients on a side stream (FPTA_OPT_OVERLAP): gen / mix of signal i run there and signal i's
  // consumer on the ctx stream waits for ev_sig[i] only, so the gridded DFT of one signal overlaps the draws of
  // the next (VALU Philox beside fp64 MFMA). ev_begin orders the side stream after everything queued before.
  int overlap = 1;
  int interp_ws = 1;      // gridded interpolation on the warp-specialised kernel (FPTA_OPT_INTERP_WS)
  int last_interp = 0;    // interpolation kernel of the last gridded block: 1 + 4 kind + 2 white + part (0: none)
  int last_fused_shape = -1;  // draw shape of the last gridded block's k_grid_fused instance (fused_sched.h; 0: the
                              // fallback); -1: that block ran another kernel (fpta_debug_fused_shape)
  double last_fma_interp = 0.0;  // its interpolation MFMA FMAs per realization as run (half-chunk bands: both halves)
  int grid_coalesce = 1;  // gridded path: signals sharing w0 and the chromatic weight share one grid (FPTA_OPT_GRID_COALESCE)
  int part_group = kPartGroup;  // fused partial checksums: consecutive chunks per partial row (FPTA_OPT_PART_GROUP)
  int interp_psr = 1;  // k_grid_interp_psr where the layout allows it (FPTA_OPT_INTERP_PSR)
  int interp_wr = 0;   // k_grid_interp_wr for plain blocks where the plan allows it (FPTA_OPT_INTERP_WR)
  int interp_fused = 1;  // k_grid_fused for plain blocks where the plan allows it (FPTA_OPT_INTERP_FUSED): 1 with
                         // half-chunk bands where they save >= 3 % of the interpolation MFMAs, 2 whole-chunk bands, 3
                         // half-chunk bands whenever planned
  // pipelined per-pulsar blocks read their coefficients in the interpolation (ctx stream): two coefficient buffers,
  // coef2 the other one; coef_slot = the grid-buffer index whose block owns c->coef; prev_psr: the last pipelined
  // block ran that way (its draws waited for the interpolation two blocks back, not for the whole ctx stream)
  DevBuf coef2;
  int coef_slot = 0;
  bool prev_psr = false;
  // FPTA_OPT_FUSED_NEXT_MIX: the last k_grid_fused launch also made the mix of common signal `seg` for the block
  // (layout, version, seed, real0, n_real, R_pad) into buffer `buf` (c->coef2 then, c->coef once that block swaps).
  // run_coefficients takes it when the next block has exactly that key; otherwise the side streams wait for that
  // kernel (event `done`) before they write a coefficient buffer.
  int fused_next_mix = 1;
  struct NextMix {
    bool valid = false;
    const Layout* layout = nullptr;
    uint64_t version = 0, seed = 0;
    int64_t real0 = 0;
    int32_t n_real = 0, R_pad = 0, seg = -1;
    const void* buf = nullptr;
    hipEvent_t done = nullptr;  // recorded on the ctx stream after that kernel (a miss makes the side streams wait for it)
  } next_mix;
  // the last batch block (seed, first realization, size): the next block's first realization is predicted at this
  // block's stride (simulate_sharded: the batch; bench.py on G ranks: G x R)
  struct LastBlock {
    bool valid = false;
    uint64_t seed = 0;
    int64_t real0 = 0;
    int32_t n_real = 0;
  } last_blk;
  bool next_mix_made = false, next_mix_used = false;  // fpta_batch_grid_info_n slots 17, 18 of the last block
  // fpta_batch_synth_spectra (spectra.hip): the current block's per-realization amplitude tables. tab[i]: signal i's
  // table [P or 1][nm][R_pad] in spec_tab, or null (the layout's amplitudes). A tabled signal is drawn with unit
  // amplitudes (spec_ones) and its columns are scaled by its table right after (k_spectra_scale): the amplitude stays
  // the last factor. per_pulsar: a per-pulsar signal has a table (the block drops gen_fused). The tables are built
  // on spec_st and the host waits for it, so they are complete before any draw is queued; ev_spec_done: the last
  // scaling of the previous tabled block (the next build waits for it).
  struct SpecRun {
    bool on = false, per_pulsar = false;
    std::vector<const double*> tab;
  } spec;
  DevBuf spec_raw, spec_tab, spec_ones;
  size_t spec_ones_n = 0;
  hipStream_t spec_st = nullptr;
  hipEvent_t ev_spec_done = nullptr;
  bool spec_done_set = false;
  bool coef_queued = true;  // the last run_coefficients queued work (a pipelined block that queued none: no grid-ready wait)
  int async_sums = 0;    // streamed jobs: partial-checksum reductions on their own stream (FPTA_OPT_ASYNC_SUMS; measured
                         // no faster on C3, profiles/r03h_ab_c3_async_sums.txt: the reductions then compete with the interpolation)
  int gen_mix = 2;       // common signals of 64..256 pulsars: draws and ORF mixing in one kernel (k_gen_mix,
                         // FPTA_OPT_GEN_MIX; 2: 16-realization waves, C3 -3.7 % vs 1, profiles/r03z_gen_mix_waves.txt);
                         // 0 k_gen into zbuf, then k_mix_mfma
  int dft_gen = 1;       // gridded path: grid signals with a per-pulsar member draw their coefficients inside the DFT
                         // (k_grid_dft_gen, FPTA_OPT_DFT_GEN): no k_gen launch, no coefficient round trip for them
  bool gen_fused = false;  // the current block runs k_grid_dft_gen for those grid signals (set by batch_common)
  int64_t blk_real0 = 0;   // the current block's first realization and Philox key (k_grid_dft_gen draws)
  uint32_t blk_k0 = 0, blk_k1 = 0;
  int interp_lds = 0;    // gridded interpolation with the grid rows staged in LDS where the plan allows (measured
                         // slower on C2: 0.745 vs 0.67 ms, profiles/r02g_*; kept as an option)
  hipStream_t side = nullptr;
  hipEvent_t ev_begin = nullptr;
  std::vector<hipEvent_t> ev_sig;
  bool coef_side = false;  // the last coefficients were made on the side stream and are not all waited for
  // recorded on the ctx stream right after the last reader of the coefficient buffer was queued (the gridded
  // DFT, or the coefficient download): the next block's draws wait for it instead of for the whole previous
  // block, so they overlap that block's interpolation
  hipEvent_t ev_coef_free = nullptr;
  bool coef_free_set = false;
  // pipelined gridded batches (FPTA_OPT_OVERLAP, path 4): the draws, merges and DFT of a block all run on the side
  // stream, into one of two grid buffers, so they overlap the previous block's interpolation on the ctx stream.
  // ev_gready: the block's DFT is done (its interpolation waits); ev_gfree[i]: the interpolation reading grid
  // buffer i is done (the DFT that next writes buffer i waits); coef_last_side: the last reader of coef was a
  // side-stream DFT, so the next block's draws need no ctx-stream wait.
  hipEvent_t ev_gready = nullptr;
  hipEvent_t ev_gfree[2] = {nullptr, nullptr};
  bool gfree_set[2] = {false, false};
  int gbuf = 0;
  bool coef_last_side = false;
  // FPTA_OPT_SIDE_SPLIT: grid signal split_g (per-pulsar members only) of the current pipelined block runs its draws
  // and DFT on side2. At each block start side waits for side2's previous work (ev_s2done) and side2 for side's
  // (ev_s2begin), so a layout change never lets one stream write columns the other still reads; ev_gready2: side2's
  // DFT is done. side_split 2: side2's DFT also waits for the common signals' draws queued on side before it
  // (ev_s2mix), so those draws get the room beside the previous block's interpolation first.
  int side_split = 2;
  hipStream_t side2 = nullptr;
  hipEvent_t ev_s2begin = nullptr, ev_s2done = nullptr, ev_gready2 = nullptr, ev_s2mix = nullptr;
  bool s2done_set = false;
  int32_t split_g = -1;
  bool coef_copy_pending = false;  // the block's coefficients are still to be downloaded after the synthesis
  DevBuf part[2], part_tmp; // partial checksums [n_chunks][R_pad][2] (two buffers, by block), reduction scratch
  bool part_ready = false;  // part[part_cur] holds the partials of the current block (c->out, out_R)
  int32_t part_chunks = 0, part_rpad = 0;
  int part_cur = 0, part_next = 0;
  // streamed jobs reduce a block's partials on their own stream (red), beside the next block's interpolation, which
  // writes the other partials buffer; ev_pfree[i]: the reduction reading part[i] is done (the interpolation that next
  // writes part[i] waits for it); red_pending: red has work the ctx stream has not joined
  hipStream_t red = nullptr;
  hipEvent_t ev_pready = nullptr, ev_pfree[2] = {nullptr, nullptr}, ev_red = nullptr;
  bool pfree_set[2] = {false, false};
  bool red_pending = false;
  int last_path = 0;     // synthesis path of the last batch (1 direct, 2 MFMA, 3 VALU, 4 gridded)
  std::string path_reason;  // why the last batch did not take the gridded path (empty if it did)
  // gridded path defaults: w = 15 at sigma = 1.5 (the kernel's design estimate exp(-pi w sqrt(1 - 1/sigma)) = 1.5e-12:
  // not a bound, a single top mode is off by up to 2.8e-11 per unit coefficient, tests/test_grid_modes.py). The
  // measured flat-spectrum worst case at real-MJD epochs is <= ~6e-12 relative (tests/test_gpu_grid.py at the shipped
  // defaults; the numpy model of oracle.grid_synth and the GPU agree); w = 14 (estimate 9.4e-12) is refused by the
  // auto path. sigma = 1.5 keeps the
  // grid (DFT) a quarter smaller than sigma = 2 (tools/sweep_grid.py --params, profiles/r01_sweep_wsig.txt)
  int grid_w = 15;       // gridded path: kernel width in grid cells
  int grid_sigma100 = 150;  // gridded path: oversampling x 100
  int grid_mfma = 1;     // gridded path: bit 0 k_grid_dft_mfma (else k_grid_dft); the interpolation is always on
                         // MFMA (k_grid_interp_ws / k_grid_interp_mfma)
  // profiling
  struct Pending {
    int which;
    hipEvent_t a, b;
  };
  std::vector<Pending> pending;
  std::vector<hipEvent_t> pool;
  int64_t kcount[FPTA_K_N] = {};
  double kms[FPTA_K_N] = {};
  // dense-covariance path: inputs, basis G^T [k_pad][n_pad], matrix C [n_pad][n_pad], panel, draws
  DevBuf dn_toas, dn_nu, dn_f, dn_sw, dn_segof, dn_segidx, dn_segff, dn_white, dn_GT, dn_C, dn_PT, dn_info, dn_r,
      dn_y, dn_out, dn_Z;
  // what the last dense call left in those buffers (fpta_debug_dense): its extents, the normals' leading dimension
  // and draw count, and the stage it reached (0 nothing or a failed call, 1 covariance, 2 factor + solve, 3 factor +
  // draws)
  struct DenseLast {
    int64_t n = 0, n_pad = 0, ldz = 0;
    int32_t n_modes = 0, k_pad = 0, n_real = 0;
    int stage = 0;
  } dn_last;
};

namespace __attribute__((visibility("hidden"))) capi {  // library-internal: not exported

int fail(fpta_ctx* c, int code, const std::string& msg);
int hip_fail(fpta_ctx* c, hipError_t e, const char* what);

// Debug build (make debug, -DFPTA_DEBUG): synchronize after every launch so a device fault is
// reported by the launch that caused it, and the kernels' FPTA_DCHECK bounds checks are compiled in.
// Release builds read no environment variable and never add work or synchronisation.
#ifdef FPTA_DEBUG
constexpr bool debug_sync() { return true; }
#else
constexpr bool debug_sync() { return false; }
#endif

#define HIPCHK(ctx, expr, what)                                                           \
  do {                                                                                    \
    hipError_t _e = (expr);                                                               \
    if (_e == hipSuccess && debug_sync() && std::strstr(what, "launch"))                  \
      _e = hipStreamSynchronize((ctx)->stream);                                           \
    if (_e != hipSuccess) return hip_fail(ctx, _e, what);                                 \
  } while (0)

hipEvent_t get_event(fpta_ctx* c);

// Bracket a launch with HIP events on the ctx stream when profiling is on.
struct KTimer {
  fpta_ctx* c;
  int which;
  hipStream_t st;
  hipEvent_t a = nullptr, b = nullptr;
  // ext: the events are handed to the launch (hipExtLaunchKernel: the kernel's own dispatch timestamps, no marker
  // packets between the step's kernels); unused (the launch took another path) they go back to the pool untimed
  bool ext = false, bound = false;
  KTimer(fpta_ctx* c_, int w, hipStream_t s = nullptr, bool ext_ = false)
      : c(c_), which(w), st(s ? s : c_->stream), ext(ext_) {
    if (c->profile) {
      a = get_event(c);
      b = get_event(c);
      if (a && !ext) (void)hipEventRecord(a, st);
    }
  }
  // the launch's start / stop events (null with profiling off)
  hipEvent_t start_ev() {
    bound = ext && a && b;
    return bound ? a : nullptr;
  }
  hipEvent_t stop_ev() const { return bound ? b : nullptr; }
  // the launch's result: a launch that failed recorded neither event, so they go back to the pool untimed
  hipError_t checked(hipError_t e) {
    if (e != hipSuccess) bound = false;
    return e;
  }
  ~KTimer() {
    if (!c->profile || !a || !b) return;
    if (!ext) (void)hipEventRecord(b, st);
    if (!ext || bound) {
      c->pending.push_back({which, a, b});
    } else {
      c->pool.push_back(a);
      c->pool.push_back(b);
    }
  }
};

// capi.hip
int join_red(fpta_ctx* c);
int upload(fpta_ctx* c, DevBuf& buf, const void* src, size_t bytes, const char* what);
int wait_coef(fpta_ctx* c, size_t i);
int wait_coef_all(fpta_ctx* c);
bool grid_gen_fused(const fpta_ctx* c, const Layout& L, size_t g);
bool psr_layout(const fpta_ctx* c, const Layout& L);
bool fused_layout(const fpta_ctx* c, const Layout& L);
int32_t next_mix_seg(const fpta_ctx* c, const Layout& L, int32_t R_pad);
int batch_common(fpta_ctx* c, uint64_t seed, int64_t real0, int32_t n_real, const double* zin, int32_t zin_nm,
                 double* out, double* coeffs_out, bool white);
// spectra.hip: scale signal i's coefficient columns by the current block's table (after its unit-amplitude draws)
int spectra_scale(fpta_ctx* c, const Layout& L, size_t i, int32_t R_pad, double* coef, hipStream_t st);
// spectra.hip: k_spectra_amp for one table of signal s, already on the device as the host gave it (raw), into tab
// [P or 1][nm][R_pad] on stream st; a power-law table uploads the signal's frequencies first
int spectra_table(fpta_ctx* c, Seg& s, int32_t P, int32_t form, int32_t per_pulsar, const double* raw, int32_t n_real,
                  int32_t R_pad, double* tab, hipStream_t st);
int launch_block_checksums(fpta_ctx* c, bool async = false, hipStream_t* used = nullptr, double* dst = nullptr,
                           bool* direct = nullptr);

// In-place lower Cholesky of the n leading rows of C (leading dimension ld, readable to the next multiple of 64;
// right-looking, 64-wide panels: diagonal block in LDS, panel solve into PT [64][ldp], MFMA trailing update) on the ctx
// stream, which it waits for. info_dev: the device's info word; pivot: -1, or the first non-positive pivot's row (the
// factor is then invalid). Books one FPTA_K_DENSE entry.
int dense_cholesky_at(fpta_ctx* c, double* C, int64_t ld, int64_t n, double* PT, int64_t ldp, int* info_dev,
                      int64_t& pivot);

// The opening of a call on the resident block, `who` the prefix of its messages. block_check refuses a null context,
// for an injection a context without a layout ("set_toas first"), a context without a block ("nothing synthesized
// yet") and for an injection a block narrower than the layout, in that order, and gives the block. block_open, after
// the caller's own refusals: the device, the join of a streamed job's reductions, which may still run beside the ctx
// stream, and for a call that writes the block the end of the interpolation's partial checksums, which describe the
// block as it was.
int block_check(fpta_ctx* c, const char* who, bool inject, Block& b);
int block_open(fpta_ctx* c, bool writes);

// The frame of a one-shot call on any array: n_vec residual vectors [n_vec][n_toa] of n_psr pulsars, `who` the prefix
// of its messages. Between the steps the call makes its own plan, copies its own tables out and returns early where
// there is nothing to launch.
struct OneShot {
  fpta_ctx* c;
  const char* who;
  int32_t n_psr;
  const int64_t* offs;
  int32_t n_vec;
  const double* res;
  int64_t n_toa() const { return n_psr > 0 ? offs[n_psr] : 0; }
  int check() const;  // a null context, "bad arguments"
  // the plan's outcome (0 made, 1 refused for the reason why, 2 out of host memory), then "res missing"
  int planned(int made, const std::string& why) const;
  int upload(Block& b) const;  // the device, and the residuals into c->res1
  int done() const;            // the stream has run: the residuals' upload is done with its source
};

// fit.hip: k_fit_apply on any operator slot (coef [n_psr][K][R_pad] = A_p r, cleared first; rows[p] == 0: the pulsar
// is skipped), the upload of such a slot's operator, offsets and rows (the caller syncs before it where a previous
// launch may still read them), and the download of a buffer [rows][R_pad] as [rows][R]. fit_launch books one
// FPTA_K_DENSE entry; fit_launch_unbooked none (the caller's KTimer spans it).
int fit_launch_unbooked(fpta_ctx* c, const Block& b, int32_t K, FitSlot& s, int32_t& R_pad);
int fit_launch(fpta_ctx* c, const Block& b, int32_t K, FitSlot& s, int32_t& R_pad);
int fit_upload(fpta_ctx* c, const char* who, FitSlot& s, int32_t K, const std::vector<double>& A, int32_t n_psr,
               const int64_t* offs, const std::vector<int32_t>& rows);
int fit_download(fpta_ctx* c, const DevBuf& coef, int64_t rows, int32_t R, int32_t R_pad, double* host);

// os.hip: k_os_pairs and k_os_reduce on coefficients X [P][2 N][R_pad] (R_pad a multiple of 32), the template phi
// [N] and J >= 1 matrices G: Q_mode into qm [J][N][R_pad], Q into q [J][R_pad]. No timer entry: the caller's spans it.
int os_pairs_launch(fpta_ctx* c, const double* X, const double* phi, const double* G, double* qm, double* q,
                    int32_t n_psr, int32_t N, int32_t R_pad, int32_t J);

// os.hip, for os_scramble.hip: the upload of a plan's tables into a slot, both stages on a block without a timer entry
// (the caller's spans them; st.rpad is set), and the download of the wanted results
int os_upload(fpta_ctx* c, const fpta_os::Plan& plan, int32_t n_psr, const int64_t* offs, const double* phi_hat,
              int32_t n_g, const double* G, OsSlot& s);
int os_launch_unbooked(fpta_ctx* c, const Block& b, OsSlot& s, OsState& st);
int os_results(fpta_ctx* c, const Block& b, const OsSlot& s, const OsState& st, double* Q, double* Q_mode, double* X);

// cw_batch.hip: the one-table mode of an injection, every realization of the block getting the same delay vector.
// bcast_vector sizes v [n_toa of the batch layout] and clears it; the caller's drop-in kernel fills it; bcast_add
// then runs k_cw_bcast, block[r][i] += v[i]. Neither books a timer entry: the caller's spans its kernel and the add.
int bcast_vector(fpta_ctx* c, const char* who, DevBuf& v);
int bcast_add(fpta_ctx* c, const char* who, const DevBuf& v, const Block& b);

// grid_host.hip
constexpr double kGridAutoRatio = 0.5;  // auto path: gridded when it needs < half the direct FMAs
// auto path: gridded only when the design estimate exp(-pi w sqrt(1 - 1/sigma)) of the width/oversampling pair is
// within this. The measured flat-spectrum worst case is ~3-4x the estimate, a single top mode ~18x (w = 16,
// sigma = 1.5: estimate 2.5e-13, measured <= 3.6e-12; w = 15: 1.5e-12 / 6e-12; w = 14: 9.4e-12 / 3.2e-11, refused). A
// forced path 4 runs any accepted pair: the caller opted in, and fpta_batch_grid_info reports the estimate.
constexpr double kGridAutoMaxErr = 2e-12;
int grid_build(fpta_ctx* c, Layout& L);
int grid_part_groups(fpta_ctx* c, GridPlan& G, int32_t P, int32_t size);
int grid_run(fpta_ctx* c, Layout& L, SynthArgs& a, int32_t R_pad, bool pipe = false);

}  // namespace capi
