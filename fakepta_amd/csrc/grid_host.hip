// The gridded path's host side: the plan of a layout (chunks, band rows, weights, grid signals, the fused kernel's
// plan) and the launches of one block (DFTs and interpolation). DESIGN.md §5c.
#include "capi_host.h"

namespace __attribute__((visibility("hidden"))) capi {  // library-internal: not exported

// ------------------------------------------------------------------------------- gridded plan
// The plan itself is plain C++ (grid_plan.h: plan_grid and its stages); here it is uploaded.
static_assert(sizeof(Int4) == sizeof(int4) && offsetof(Int4, y) == offsetof(int4, y) &&
                  offsetof(Int4, z) == offsetof(int4, z) && offsetof(Int4, w) == offsetof(int4, w),
              "Int4 tables are uploaded as int4");

#ifdef FPTA_DIAG_KERNELS
}  // namespace capi
#include "diag/grid_plan_diag.h"
namespace __attribute__((visibility("hidden"))) capi {
static_assert(sizeof(Int2) == sizeof(int2) && offsetof(Int2, y) == offsetof(int2, y), "uploaded as int2");

// The window-ring, LDS-union and union-row plans of the diagnostic kernels, made from plan H and uploaded.
static int grid_build_diag(fpta_ctx* c, GridPlan::Diag& D, const HostGridPlan& H) {
  const DiagWindowPlan W = plan_diag_window(H);
  const DiagLdsPlan S = plan_diag_lds(H);
  const DiagUnionPlan U = plan_diag_union(H);
  int rc;
  D.wr_ok = W.ok;
  if (W.ok && ((rc = upload(c, D.wr_meta, W.meta.data(), sizeof(int4) * W.meta.size(), "window plan")) ||
               (rc = upload(c, D.wr_list, W.list.data(), sizeof(int2) * std::max<size_t>(W.list.size(), 1),
                            "window rows")) ||
               (rc = upload(c, D.wr_slot, W.slot.data(), sizeof(int32_t) * W.slot.size(), "window slots"))))
    return rc;
  D.lds_ok = S.ok;
  D.n_groups = (int32_t)S.groups.size();
  D.lds_rows = S.lds_rows;
  if (S.ok && ((rc = upload(c, D.groups, S.groups.data(), sizeof(int4) * S.groups.size(), "grid groups")) ||
               (rc = upload(c, D.urows, S.urows.data(), sizeof(int32_t) * S.urows.size(), "grid union rows")) ||
               (rc = upload(c, D.lrows, S.lrows.data(), sizeof(int32_t) * S.lrows.size(), "grid LDS rows"))))
    return rc;
  D.u_ok = U.ok;
  D.u_groups = (int32_t)U.groups.size();
  D.u_sig = H.n_seg();
  if (U.ok) {
    for (int32_t s = 0; s < H.n_seg(); ++s) {
      D.u_w[s] = H.segs[s].w;
      D.u_hw[s] = 0.5 * (double)H.segs[s].w;
      D.u_beta[s] = H.segs[s].beta;
    }
    if ((rc = upload(c, D.ugroups, U.groups.data(), sizeof(int4) * U.groups.size(), "union groups")) ||
        (rc = upload(c, D.uurows, U.urows.data(), sizeof(int32_t) * U.urows.size(), "union rows")) ||
        (rc = upload(c, D.ucbase, U.cbase.data(), sizeof(int32_t) * U.cbase.size(), "union bases")) ||
        (rc = upload(c, D.uwrow, U.wrow.data(), sizeof(int32_t) * U.wrow.size(), "union window rows")))
      return rc;
    const size_t dbytes = sizeof(double) * 2 * (size_t)H.n_chunks() * H.n_seg() * kGridTT;
    HIPCHK(c, D.udch.ensure(dbytes), "union weight parameters alloc");
    HIPCHK(c, hipMemsetAsync(D.udch.p, 0, dbytes, c->stream), "union weight parameters memset");
  }
  return FPTA_OK;
}
#endif

// Build the gridded plan (grid.hip) of layout L: plan_grid on a host view of L, its tables uploaded, and the dense
// banded weights made on the device (k_grid_weights). Not usable -> ok = false + why.
int grid_build(fpta_ctx* c, Layout& L) {
  GridPlan& G = L.grid;
  if (G.built && G.w == c->grid_w && G.sigma == c->grid_sigma100 / 100.0) return FPTA_OK;
  G.clear();
  G.built = true;
  G.w = c->grid_w;
  G.sigma = c->grid_sigma100 / 100.0;
  PlanLayout V;
  V.P = L.P;
  V.n_toa = L.n_toa;
  V.offs = L.h_offs.data();
  V.toas = L.h_toas.data();
  V.nu = L.h_nu.data();
  for (const Seg* sg : L.segs)
    V.sigs.push_back(PlanSignal{sg->d.kind, sg->d.nm, sg->d.idx, sg->d.freqf, sg->d.harmonic, sg->h_w0.data(),
                                sg->h_mask.empty() ? nullptr : sg->h_mask.data()});
  HostGridPlan H = plan_grid(V, PlanOptions{G.w, G.sigma, c->grid_coalesce != 0, c->grid_mfma});
  static_cast<PlanFigures&>(G) = H;  // a refused plan keeps what the stages before the refusal made
  G.ok = false;                       // until the tables are on the device
  if (!G.fused_ok) G.fused_lds = 0;   // the planner reports the bytes that were too many
  int rc;
  if (!H.psr_chunk0.empty()) {  // the chunks were made
    G.n_chunks = H.n_chunks();
    if ((rc = upload(c, G.psr_c0, G.psr_chunk0.data(), sizeof(int32_t) * G.psr_chunk0.size(), "pulsar chunks")))
      return rc;
  }
  if (!H.ok) return FPTA_OK;
  const int32_t n_seg = H.n_seg();
  const int64_t N = L.n_toa;
  if ((rc = upload(c, G.chunks, H.chunks.data(), sizeof(int4) * H.chunks.size(), "grid chunks")) ||
      (rc = upload(c, G.rows, H.rows.data(), sizeof(int32_t) * H.rows.size(), "grid band rows")))
    return rc;
#ifdef FPTA_DIAG_KERNELS
  if ((rc = grid_build_diag(c, G.diag, H))) return rc;
#endif
  DevBuf d_chunk_of, d_tt_of, d_row, d_d;
  if ((rc = upload(c, d_chunk_of, H.chunk_of.data(), sizeof(int32_t) * N, "grid chunk_of")) ||
      (rc = upload(c, d_tt_of, H.tt_of.data(), sizeof(int32_t) * N, "grid tt_of")))
    return rc;
  const size_t wbytes = sizeof(double) * H.wd_size;
  HIPCHK(c, G.wd.ensure(wbytes), "grid weights alloc");
  HIPCHK(c, hipMemsetAsync(G.wd.p, 0, wbytes, c->stream), "grid weights memset");
  // per grid signal its tables, then its weights; half: into the half-chunk bands' layout
  auto weights = [&](int32_t s, bool half) -> int {
    const PlanSeg& g = H.segs[s];
    const std::vector<int32_t>& row = half ? g.hrow_of : g.row;
    if ((rc = upload(c, d_row, row.data(), sizeof(int32_t) * N, half ? "half rows" : "grid rows")) ||
        (rc = upload(c, d_d, g.d.data(), sizeof(double) * N, "grid offsets")))
      return rc;
    HIPCHK(c,
           launch_grid_weights(c->stream, L.segs[G.anchor[s]]->d, N, L.nu.as<double>(), d_chunk_of.as<int32_t>(),
                               d_tt_of.as<int32_t>(), d_row.as<int32_t>(), d_d.as<double>(), g.w, g.beta,
                               half ? H.fused_hvmax : H.vmax, half ? G.hwd.as<double>() : G.wd.as<double>(),
                               !half && G.diag.u_ok ? G.diag.udch.as<double>() : nullptr, s, n_seg, half ? 1 : 0),
           half ? "k_grid_weights (half bands) launch" : "k_grid_weights launch");
    // d_row / d_d are reused
    HIPCHK(c, hipStreamSynchronize(c->stream), half ? "half weights sync" : "grid weights sync");
    return FPTA_OK;
  };
  for (int32_t s = 0; s < n_seg; ++s) {
    const PlanSeg& g = H.segs[s];
    GridSeg* gs = new GridSeg();
    G.segs.push_back(gs);
    gs->nf = g.nf;
    gs->half = g.half;
    gs->lde = g.lde;
    gs->ntab = g.ntab;
    gs->rowoff = g.rowoff;
    gs->ldq = g.ldq;
    gs->ntq = g.ntq;
    if ((rc = upload(c, gs->ecos, g.ecos.data(), sizeof(double) * g.ecos.size(), "grid ecos")) ||
        (rc = upload(c, gs->esin, g.esin.data(), sizeof(double) * g.esin.size(), "grid esin")) ||
        (rc = upload(c, gs->tq, g.tq.data(), sizeof(double) * g.tq.size(), "grid quarter tables")) ||
        (rc = weights(s, false)))
      return rc;
  }
  if (H.fused_ok && (rc = upload(c, G.frows, H.frows.data(), sizeof(int32_t) * H.frows.size(), "fused LDS rows")))
    return rc;
  if (H.fused_half_ok) {
    if ((rc = upload(c, G.hchunks, H.hchunks.data(), sizeof(int4) * H.hchunks.size(), "fused half chunks")) ||
        (rc = upload(c, G.hrows, H.hrows.data(), sizeof(int32_t) * H.hrows.size(), "fused half rows")))
      return rc;
    const size_t hbytes = sizeof(double) * H.hwd_size;
    HIPCHK(c, G.hwd.ensure(hbytes), "half weights alloc");
    HIPCHK(c, hipMemsetAsync(G.hwd.p, 0, hbytes, c->stream), "half weights memset");
    if ((rc = upload(c, d_chunk_of, H.hchunk_of.data(), sizeof(int32_t) * N, "half chunk_of")) ||
        (rc = upload(c, d_tt_of, H.htt_of.data(), sizeof(int32_t) * N, "half tt_of")))
      return rc;
    for (int32_t s = 0; s < n_seg; ++s)
      if ((rc = weights(s, true))) return rc;
  }
  G.ok = true;
  return FPTA_OK;
}

// Partial-checksum groups of G: each pulsar's chunks cut into runs of <= size consecutive chunks (a group never spans
// two pulsars, so a workgroup that owns a pulsar owns its groups), uploaded once per (plan, size).
int grid_part_groups(fpta_ctx* c, GridPlan& G, int32_t P, int32_t size) {
  if (G.pg_size == size) return FPTA_OK;
  std::vector<int32_t> first, psr((size_t)P + 1);
  for (int32_t p = 0; p < P; ++p) {
    psr[p] = (int32_t)first.size();
    for (int32_t ci = G.psr_chunk0[p]; ci < G.psr_chunk0[p + 1]; ci += size) first.push_back(ci);
  }
  psr[P] = (int32_t)first.size();
  first.push_back(G.n_chunks);
  int rc;
  if ((rc = upload(c, G.pgfirst, first.data(), sizeof(int32_t) * first.size(), "partial groups")) ||
      (rc = upload(c, G.psr_pg, psr.data(), sizeof(int32_t) * psr.size(), "partial groups of pulsars")))
    return rc;
  G.n_pg = (int32_t)first.size() - 1;
  G.pg_size = size;
  return FPTA_OK;
}

// Run the gridded synthesis: one DFT launch per grid signal, then one interpolation launch for all.
// pipe (run_coefficients drew this block on the side stream in pipelined mode): the DFTs follow there, into grid
// buffer c->gbuf, and the interpolation on the ctx stream waits only for them.
int grid_run(fpta_ctx* c, Layout& L, SynthArgs& a, int32_t R_pad, bool pipe) {
  GridPlan& G = L.grid;
  GridSegs gsegs{};
  gsegs.n = (int32_t)G.segs.size();
  const size_t gbytes = sizeof(double) * (size_t)G.grid_rows * R_pad;
  // k_grid_interp_psr: no DFT launch, no grid buffer; in a pipelined block the coefficients drawn on the side stream
  // into buffer gi are this block's (run_coefficients)
  const bool psr = psr_layout(c, L) && !a.w_on && !a.accumulate && (!pipe || c->prev_psr);
  // k_grid_fused: the DFTs run inside the synthesis kernel too (plain blocks: no white epilogue, no partial checksums)
  const bool fused = !psr && fused_layout(c, L) && !a.w_on && !a.accumulate &&
                     !(c->fuse_sums && a.out == c->out.as<double>()) && (!pipe || c->prev_psr);
  // grid buffers only for the kernels that read one (two of 0.41 GB each on C2)
  if (!psr && !fused && (G.g_rpad != R_pad || (pipe && G.g2.cap < gbytes))) {
    if (c->side) HIPCHK(c, hipStreamSynchronize(c->side), "side sync");  // no reader of a buffer being regrown
    if (c->side2) HIPCHK(c, hipStreamSynchronize(c->side2), "side sync");
    HIPCHK(c, hipStreamSynchronize(c->stream), "grid regrow sync");
    HIPCHK(c, G.g.ensure(gbytes), "grid alloc");
    if (pipe) HIPCHK(c, G.g2.ensure(gbytes), "grid alloc");
    G.g_rpad = R_pad;
  }
  const int gi = pipe ? c->gbuf : 0;
  double* const gbase = gi ? G.g2.as<double>() : G.g.as<double>();
  if (pipe) {
    for (hipEvent_t* e : {&c->ev_gready, &c->ev_gfree[0], &c->ev_gfree[1]})
      if (!*e) HIPCHK(c, hipEventCreateWithFlags(e, hipEventDisableTiming), "event create");
    // the DFT overwrites buffer gi: the interpolation that last read it (two blocks back) must be done
    if (c->gfree_set[gi]) HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_gfree[gi], 0), "grid buffer wait");
  }
  // a pipelined block whose draws and mixing queued nothing on the side stream (the previous block's kernel mixed its
  // common signal, FPTA_OPT_FUSED_NEXT_MIX; its other signals drawn inside the kernel): no grid-ready event to wait for
  bool gwait = pipe;
  if (psr || fused) {
    GridSeg* gs = G.segs[0];
    GridSegDev& g = gsegs.s[0];
    g.g = nullptr;
    g.nf = gs->nf;
    g.half = gs->half;
    g.nm = L.segs[G.anchor[0]]->d.nm;
    g.col0 = L.segs[G.anchor[0]]->d.col0;
    g.tq = gs->tq.as<double>();
    g.ldq = gs->ldq;
    g.ntq = gs->ntq;
    gwait = pipe && c->coef_queued;
    if (gwait) HIPCHK(c, hipEventRecord(c->ev_gready, c->side), "event record");
    if (pipe) {
      c->coef_last_side = false;  // the interpolation on the ctx stream reads the coefficients
    } else {
      int rc = wait_coef_all(c);
      if (rc) return rc;
    }
  } else {
    KTimer kt(c, FPTA_K_GRID, pipe ? c->side : c->stream);
    for (size_t s = 0; s < G.segs.size(); ++s) {
      GridSeg* gs = G.segs[s];
      const SegDesc& d = L.segs[G.anchor[s]]->d;  // a coalesced grid signal reads its anchor's merged columns
      GridSegDev& g = gsegs.s[s];
      g.ecos = gs->ecos.as<double>();
      g.esin = gs->esin.as<double>();
      g.g = gbase + gs->rowoff * R_pad;
      g.nf = gs->nf;
      g.half = gs->half;
      g.lde = gs->lde;
      g.nm = d.nm;
      g.col0 = d.col0;
      g.ntab = gs->ntab;
      g.tq = gs->tq.as<double>();
      g.ldq = gs->ldq;
      g.ntq = gs->ntq;
    }
    const bool early_free = c->coef_side && !c->coef_copy_pending;
    const int32_t split = pipe && c->split_g < gsegs.n ? c->split_g : -1;
    c->split_g = -1;
    // the DFTs of a set of grid signals on one stream: each k_grid_dft_gen signal its own launch, the others in one
    // k_grid_dft_mfma / k_grid_dft launch
    auto dfts = [&](hipStream_t sd, const std::vector<int32_t>& sigs) -> int {
      GridSegs rest{};
      for (int32_t s : sigs) {
        if (!grid_gen_fused(c, L, (size_t)s)) {
          rest.s[rest.n++] = gsegs.s[s];
          continue;
        }
        DftGenArgs d{};
        d.g = gsegs.s[s];
        std::vector<int32_t> order{G.anchor[s]};  // the merge order: anchor, then the others in layout order
        for (int32_t i : G.members[s])
          if (i != G.anchor[s]) order.push_back(i);
        for (int32_t i : order) {
          const SegDesc& sd2 = L.segs[i]->d;
          d.term_kind[d.n_terms] = sd2.kind;
          d.term_seg[d.n_terms] = i;
          d.term_nm[d.n_terms] = sd2.nm;
          d.term_col0[d.n_terms] = sd2.col0;
          d.term_amp[d.n_terms] = sd2.amp;
          ++d.n_terms;
        }
        d.coef = a.coef;
        d.P = L.P;
        d.K = a.K;
        d.R_pad = R_pad;
        d.n_real = a.n_real;
        d.real0 = c->blk_real0;
        d.k0 = c->blk_k0;
        d.k1 = c->blk_k1;
        HIPCHK(c, launch_grid_dft_gen(sd, d), "k_grid_dft_gen launch");
      }
      if (rest.n)
        HIPCHK(c,
               (c->grid_mfma & 1) ? launch_grid_dft_mfma(sd, rest, L.P, a.coef, a.K, R_pad)
                                  : launch_grid_dft(sd, rest, L.P, a.coef, a.K, R_pad),
               "k_grid_dft launch");
      return FPTA_OK;
    };
    std::vector<int32_t> all_sigs(gsegs.n);
    for (int32_t s = 0; s < gsegs.n; ++s) all_sigs[s] = s;
    if (pipe && split >= 0) {
      // the split signal's DFT on side2 (after its draws there), the others' on side
      std::vector<int32_t> rest_sigs;
      for (int32_t s = 0; s < gsegs.n; ++s)
        if (s != split) rest_sigs.push_back(s);
      {
        if (c->gfree_set[gi]) HIPCHK(c, hipStreamWaitEvent(c->side2, c->ev_gfree[gi], 0), "grid buffer wait");
        if (c->side_split == 2) {
          if (!c->ev_s2mix) HIPCHK(c, hipEventCreateWithFlags(&c->ev_s2mix, hipEventDisableTiming), "event create");
          HIPCHK(c, hipEventRecord(c->ev_s2mix, c->side), "event record");
          HIPCHK(c, hipStreamWaitEvent(c->side2, c->ev_s2mix, 0), "side wait");
        }
        KTimer kt2(c, FPTA_K_GRID, c->side2);
        int rc = dfts(c->side2, {split});
        if (rc) return rc;
      }
      HIPCHK(c, hipEventRecord(c->ev_gready2, c->side2), "event record");
      c->s2done_set = true;
      int rc = dfts(c->side, rest_sigs);
      if (rc) return rc;
    } else if (pipe) {
      int rc = dfts(c->side, all_sigs);
      if (rc) return rc;
    } else if (c->coef_side) {
      // one DFT launch per grid signal, each after that signal's draws (and merge) only (side stream); in the
      // order their draws complete
      std::vector<int32_t> order(gsegs.n);
      for (int32_t s = 0; s < gsegs.n; ++s) order[s] = s;
      std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return G.last[x] < G.last[y]; });
      for (int32_t s : order) {
        GridSegs one{};
        one.s[0] = gsegs.s[s];
        one.n = 1;
        int rc = wait_coef(c, (size_t)G.last[s]);
        if (rc) return rc;
        HIPCHK(c,
               (c->grid_mfma & 1) ? launch_grid_dft_mfma(c->stream, one, L.P, a.coef, a.K, R_pad)
                                  : launch_grid_dft(c->stream, one, L.P, a.coef, a.K, R_pad),
               "k_grid_dft launch");
      }
      c->coef_side = false;
    } else {
      int rc = dfts(c->stream, all_sigs);
      if (rc) return rc;
    }
    if (pipe) {
      HIPCHK(c, hipEventRecord(c->ev_gready, c->side), "event record");
      c->coef_last_side = !c->coef_copy_pending;  // else the download on the ctx stream is the last reader
    } else if (early_free) {  // the DFT was the last reader of coef: the next block may draw during the interpolation
      if (!c->ev_coef_free) HIPCHK(c, hipEventCreateWithFlags(&c->ev_coef_free, hipEventDisableTiming), "event create");
      HIPCHK(c, hipEventRecord(c->ev_coef_free, c->stream), "event record");
      c->coef_free_set = true;
    }
  }
  // partial checksums of a batch block (written into the context's own block, not accumulated)
  if (c->fuse_sums && a.out == c->out.as<double>() && !a.accumulate) {
    const int pi = c->part_next;
    DevBuf& pb = c->part[pi];
    const size_t pbytes = sizeof(double) * 2 * (size_t)G.n_chunks * R_pad;
    if (pb.cap < pbytes && c->red) HIPCHK(c, hipStreamSynchronize(c->red), "partials regrow sync");
    HIPCHK(c, pb.ensure(pbytes), "partial checksums alloc");
    // the reduction of the block that last wrote this buffer (on the red stream) must have read it
    if (c->pfree_set[pi]) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_pfree[pi], 0), "partials buffer wait");
    a.part = pb.as<double>();
    int rc = grid_part_groups(c, G, L.P, c->part_group);
    if (rc) return rc;
    c->part_cur = pi;
    c->part_next = pi ^ 1;
  }
  if (gwait) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_gready, 0), "grid ready wait");
  if (pipe && c->s2done_set) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_gready2, 0), "grid ready wait");
  // the fused launch takes the timing events itself (no marker packets around it); the diagnostic options that take
  // another kernel for a fused layout time it with recorded events
#ifdef FPTA_DIAG_KERNELS
  const bool ext = fused && c->interp_ws != 4 && c->interp_ws != 5 && !c->interp_wr;
#else
  const bool ext = fused;
#endif
  KTimer kt(c, FPTA_K_SYNTH, nullptr, ext);
  GridBand band{G.chunks.as<int4>(), G.rows.as<int32_t>(), G.wd.as<double>(), gbase, G.n_chunks, G.vmax,
                G.grid_rows, a.part ? G.pgfirst.as<int32_t>() : nullptr, a.part ? G.n_pg : G.n_chunks};
  // the warp-specialised kernel for plain blocks; with fused partial checksums its reduce-scatter temporaries take
  // its VGPRs to 230 and the register kernel is faster (C3: 47.9 vs 52.5 ms per job, profiles/r02k_ab_c2c3_ws.txt)
  // k_grid_interp_ws tiles 512 realizations (4 compute waves x 128): when R_pad leaves some of the last tile's compute
  // waves idle, the 256-realization tiles of k_grid_interp_ws2 waste less (C4, R_pad = 256: half of every ws tile;
  // 6.8-7.4 vs 8.4 ms/step, profiles/r04a_c4_ws2.txt)
  // (the automatic k_grid_interp_ws2 choice for such R_pad, diagnostic builds only since round 6: no shipped layout
  // reaches it)
#ifdef FPTA_DIAG_KERNELS
  const bool ws2_fits = c->interp_ws == 1 && (R_pad + 255) / 256 * 256 - R_pad < (R_pad + 511) / 512 * 512 - R_pad;
#else
  const bool ws2_fits = false;
#endif
  int kind;  // the interpolation kernel (fpta_batch_grid_info_n slot 15)
  if (false) {
#ifdef FPTA_DIAG_KERNELS
  } else if (c->interp_ws == 5 && !c->interp_lds && G.diag.u_ok && !a.w_on) {
    kind = 5;
    band.pgfirst = nullptr;  // the diagnostic kernels write one partial row per chunk
    band.n_pg = G.n_chunks;
    const GridPlan::Diag& D = G.diag;
    GridUnion un{D.ugroups.as<int4>(), D.uurows.as<int32_t>(), D.ucbase.as<int32_t>(), D.udch.as<double>(),
                 D.uwrow.as<int32_t>(), D.u_groups, D.u_sig, {D.u_w[0], D.u_w[1]}, {D.u_hw[0], D.u_hw[1]},
                 {D.u_beta[0], D.u_beta[1]}};
    HIPCHK(c, launch_grid_interp_u(c->stream, a, band, un, R_pad), "k_grid_interp_u launch");
  } else if (c->interp_ws == 4 && !c->interp_lds) {
    kind = 4;
    band.pgfirst = nullptr;
    band.n_pg = G.n_chunks;
    HIPCHK(c, launch_grid_interp_st(c->stream, a, band, R_pad), "k_grid_interp_st launch");
  } else if (c->interp_wr && G.diag.wr_ok && !c->interp_lds && c->interp_ws > 0 && !a.w_on && !a.accumulate &&
             !a.part && R_pad % kWrReal == 0 && !psr) {
    kind = 10;
    GridWindow wrp{G.diag.wr_meta.as<int4>(), G.diag.wr_list.as<int2>(), G.diag.wr_slot.as<int32_t>()};
    HIPCHK(c, launch_grid_interp_wr(c->stream, a, band, wrp, R_pad), "k_grid_interp_wr launch");
#endif
  } else if (fused) {
    // half-chunk bands (FPTA_OPT_INTERP_FUSED 1: where they save >= 3 % of the interpolation MFMAs; 3: always)
    const bool half = G.fused_half_ok &&
                      (c->interp_fused == 3 || (c->interp_fused == 1 && G.fused_half_gain >= 1.03));
    const int32_t nq = half ? G.fused_hnq : G.vmax / 4;
    FusedArgs f{};
    if (half) f.h = FusedHalf{G.hchunks.as<int4>(), G.hrows.as<int32_t>(), G.hwd.as<double>(), G.fused_hfq, G.fused_hvmax};
    f.n_sig = (int32_t)G.segs.size();
    for (int32_t s = 0; s < f.n_sig; ++s) {
      const GridSeg* gs = G.segs[s];
      const SegDesc& d = L.segs[G.anchor[s]]->d;
      FusedSig& fs = f.s[s];
      fs.tq = gs->tq.as<double>();
      fs.ldq = gs->ldq;
      fs.ntq = gs->ntq;
      fs.nf = gs->nf;
      fs.nm = d.nm;
      fs.lrow0 = G.fused_lrow0[s];
      fs.n_rc = (gs->nf / 4 + 32) / 32;
      if (grid_gen_fused(c, L, (size_t)s)) {  // k_grid_dft_gen's terms: the anchor, then the others in layout order
        std::vector<int32_t> order{G.anchor[s]};
        for (int32_t i : G.members[s])
          if (i != G.anchor[s]) order.push_back(i);
        for (int32_t i : order) {
          const SegDesc& sd2 = L.segs[i]->d;
          fs.term_kind[fs.n_terms] = sd2.kind;
          fs.term_seg[fs.n_terms] = i;
          fs.term_nm[fs.n_terms] = sd2.nm;
          fs.term_col0[fs.n_terms] = sd2.col0;
          fs.term_amp[fs.n_terms] = sd2.amp;
          ++fs.n_terms;
        }
      } else {  // k_grid_dft_mfma's operand: the anchor's (merged) columns of the coefficient buffer
        fs.term_kind[0] = 1;
        fs.term_seg[0] = G.anchor[s];
        fs.term_nm[0] = d.nm;
        fs.term_col0[0] = d.col0;
        fs.n_terms = 1;
      }
    }
    // The DFT waves interpolate an item's chunks while more than join_reserve are left, then build the next item
    // while the interpolation waves take the rest. In MFMA-equivalents (64 cycles): a ring iteration of a DFT wave is
    // its 32 MFMAs + ~20 per generated term (a Philox call and two Box-Muller pairs per lane), a chunk 4 per band step
    // + ~12 (operand loads, stores). The reserve is kFusedJoinSafety times the chunks the interpolation waves do in a
    // build: C2 (~7 x 72 per build, ~48 per chunk: reserve 63 of its 63 chunks per item) hardly joins; C4 (~7 x 32,
    // ~32 per chunk: reserve ~42 of 313) joins for most of an item. (The estimate is about half the measured build
    // time on C2; the factor 1.5 was the best of 0.5 .. 5 on both, profiles/round5/r5mn_*.)
    {
      int it_max = 0, gen = 0;
      for (int32_t s = 0; s < f.n_sig; ++s) {
        const int nm = f.s[s].nm;
        it_max = std::max(it_max, fused_groups(nm));
        for (int i = 0; i < f.s[s].n_terms; ++i) gen += f.s[s].term_kind[i] == 0;
      }
      const double build = it_max * (32.0 + 20.0 * gen);
      const double chunk = G.mean_v + 12.0;
      f.join_reserve = (int32_t)std::min(1.0e6, std::ceil(kFusedJoinSafety * kFusedIW * build / chunk));
    }
    f.ring_off = (G.fused_lrow0.back() + G.segs.back()->nf) * kFusedPitch;
    // a pipelined block whose common signals are mixed by a separate k_mix_mfma (P > kGenMixMaxP, C4): the next
    // block's mix is queued on the side stream while this kernel runs
    {
      bool sep_mix = false;
      for (const Seg* sg : L.segs) sep_mix = sep_mix || (sg->d.kind == 1 && L.P > kGenMixMaxP);
      f.cu_pct = pipe && sep_mix ? FPTA_FUSED_MIX_CU_PCT : 100;
    }
    f.lrows = G.frows.as<int32_t>();
    f.fq = G.fused_fq;
    f.psr_c0 = G.psr_c0.as<int32_t>();
    f.real0 = c->blk_real0;
    f.k0 = c->blk_k0;
    f.k1 = c->blk_k1;
#ifdef FPTA_FUSED_PROF
    HIPCHK(c, c->dbg_a.ensure(sizeof(unsigned long long) * 8 * 8 * 4096), "fused profile alloc");
    HIPCHK(c, hipMemsetAsync(c->dbg_a.p, 0, sizeof(unsigned long long) * 8 * 8 * 4096, c->stream), "profile memset");
    f.prof = c->dbg_a.as<unsigned long long>();
#endif
    // The item queues are zeroed once: every launch leaves them zero (its last workgroup resets them), which holds
    // because fused launches only go on the context stream, one after another. The debug build re-zeroes them before
    // every launch, so a launch that did not complete cannot make the next one skip items unnoticed.
#ifdef FPTA_DEBUG
    c->fused_q_ready = false;
#endif
    if (!c->fused_q_ready) {
      HIPCHK(c, c->fused_q.ensure(sizeof(uint32_t) * kFusedQueueWords), "fused queue alloc");
      HIPCHK(c, hipMemsetAsync(c->fused_q.p, 0, sizeof(uint32_t) * kFusedQueueWords, c->stream), "fused queue memset");
      c->fused_q_ready = true;
    }
    f.queue = c->fused_q.as<uint32_t>();
    // FPTA_OPT_FUSED_NEXT_MIX: the next block's common-signal mix (this seed and size) as spare-time tickets, into the
    // coefficient buffer that block swaps in (c->coef2: this block's kernel and k_gen_mix's of the block before read
    // it no more; grown already, so it is not reallocated under the kernel). The next block's first realization:
    // real0 + this block's stride from the last one of the same seed and size when that is a whole number of blocks
    // (G ranks' interleaved blocks), else real0 + n_real.
    c->next_mix_made = false;
    // (a block with per-realization amplitude tables makes none; it could make the next block's fixed-amplitude mix,
    // which is not built: the block after a tabled one runs k_gen_mix)
    const int32_t nms = pipe && c->prev_psr && !c->spec.on ? next_mix_seg(c, L, R_pad) : -1;
    const size_t coef_bytes = sizeof(double) * (size_t)L.P * std::max(L.K, 1) * R_pad;
    const uint64_t blk_seed = (uint64_t)c->blk_k0 | ((uint64_t)c->blk_k1 << 32);
    const fpta_ctx::LastBlock& lb = c->last_blk;
    const int64_t step = c->blk_real0 - lb.real0;
    const int64_t stride =
        lb.valid && lb.seed == blk_seed && lb.n_real == a.n_real && step >= a.n_real && step % a.n_real == 0 ? step
                                                                                                         : a.n_real;
    if (nms >= 0 && c->coef2.cap >= coef_bytes && c->blk_real0 + stride + a.n_real <= ((int64_t)1 << 32)) {
      const SegDesc& d = L.segs[nms]->d;
      FusedMix& m = f.mix;
      m.LT = d.LT;
      m.amp = d.amp;
      m.coef = c->coef2.as<double>();
      m.real0 = c->blk_real0 + stride;
      m.k0 = c->blk_k0;
      m.k1 = c->blk_k1;
      m.lt_ld = d.lt_ld;
      m.lt_rows = d.lt_rows;
      m.P = L.P;
      m.K = a.K;
      m.col0 = d.col0;
      m.R_pad = R_pad;
      m.n_real = a.n_real;
      m.n_q = d.n_q;
      m.lower = d.l_lower;
      m.seg = nms;
      m.nm = d.nm;
      m.n_tiles = d.nm * (R_pad / 16) * ((L.P + kFusedMixGroup - 1) / kFusedMixGroup);
    }
    hipEvent_t e0 = kt.start_ev();
    int ki = 0;
    HIPCHK(c, kt.checked(launch_grid_fused(c->stream, a, band, f, nq, G.fused_lds, e0, kt.stop_ev(), half, &ki,
                                           &c->last_fused_shape)),
           "k_grid_fused launch");
    kind = kInterpKindFused0 + ki;  // fpta_batch_grid_info_n slot 15: the instance launched
    if (f.mix.n_tiles > 0) {
      fpta_ctx::NextMix& nx = c->next_mix;
      nx.valid = true;
      nx.layout = &L;
      nx.version = L.version;
      nx.seed = blk_seed;
      nx.real0 = f.mix.real0;
      nx.n_real = a.n_real;
      nx.R_pad = R_pad;
      nx.seg = nms;
      nx.buf = c->coef2.p;
      nx.done = nullptr;  // the event recorded after this launch (pipe: ev_gfree of this block's buffer index, below)
      c->next_mix_made = true;
    }
    c->last_fma_interp = half ? G.fma_interp_half : G.fma_interp;
  } else if (psr) {
    kind = G.vmax <= 16 ? 6 : 7;  // launch_grid_interp_psr: NQ = 4 or 8 band steps
    HIPCHK(c,
           launch_grid_interp_psr(c->stream, a, band, gsegs.s[0],
                                  a.part ? G.psr_pg.as<int32_t>() : G.psr_c0.as<int32_t>(), L.P, R_pad),
           "k_grid_interp_psr launch");
  } else if ((c->interp_ws == 3 || ws2_fits) && !c->interp_lds && !a.w_on && !a.accumulate && !a.part) {
    kind = 2;
    HIPCHK(c, launch_grid_interp_ws(c->stream, a, band, R_pad, true), "k_grid_interp_ws2 launch");
  } else if (c->interp_ws && !c->interp_lds && !a.w_on && !a.accumulate && (!a.part || c->interp_ws == 2)) {
    kind = 1;
    HIPCHK(c, launch_grid_interp_ws(c->stream, a, band, R_pad), "k_grid_interp_ws launch");
#ifdef FPTA_DIAG_KERNELS
  } else if (c->interp_lds && G.diag.lds_ok && !a.w_on) {
    kind = 3;
    band.pgfirst = nullptr;
    band.n_pg = G.n_chunks;
    const GridPlan::Diag& D = G.diag;
    GridLds lds{D.groups.as<int4>(), D.urows.as<int32_t>(), D.lrows.as<int32_t>(), D.n_groups, D.lds_rows};
    HIPCHK(c, launch_grid_interp_lds(c->stream, a, band, lds, R_pad), "k_grid_interp_lds launch");
#endif
  } else {
    kind = 0;
    HIPCHK(c, launch_grid_interp_mfma(c->stream, a, band, R_pad), "k_grid_interp_mfma launch");
  }
  c->last_interp = 1 + kind * 4 + (a.w_on ? 2 : 0) + (a.part ? 1 : 0);
  if (kind < kInterpKindFused0) c->last_fused_shape = -1;
  if (kind < kInterpKindFused0) c->last_fma_interp = G.fma_interp;
  if (pipe) {  // buffer gi is free once this interpolation is done; the next block's DFT writes the other one
    HIPCHK(c, hipEventRecord(c->ev_gfree[gi], c->stream), "event record");
    if (c->next_mix_made) c->next_mix.done = c->ev_gfree[gi];  // the kernel that writes the next block's mix is done
    c->gfree_set[gi] = true;
    c->gbuf = gi ^ 1;
  }
  if (a.part) {
    c->part_ready = true;
    c->part_chunks = band.n_pg;  // partial rows
    c->part_rpad = R_pad;
  }
  return FPTA_OK;
}

}  // namespace capi
