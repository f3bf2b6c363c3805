// Roemer delays of ephemeris errors injected into the context's last batch block, in place
// (fpta_batch_roemer_accumulate):
//   block[r][i] += sign * sum over the rows k of realization r's table of delay_k(t_i, pulsar of i)
// with the delay of k_roemer_main (ephem.hip) and the orbit arithmetic of ephem_device.h. Every realization has its own
// row table (ragged, CSR), validated and turned into RoemerRow records on the host (roemer_batch_host.h).
//
//   k_roemer_block  one workgroup of 4 waves per (slab of <= 256 consecutive TOAs of one pulsar, chunk of C consecutive
//                   realizations), one TOA per lane. The unperturbed orbit of a body depends on the TOA only, so on
//                   entry every lane evaluates the call's distinct base bodies (<= kRoemerMaxBase slots, deduplicated
//                   on the host) once and keeps the three components in LDS at [slot][component][thread]: a lane reads
//                   only what it wrote, so there is no barrier. The loop over the chunk's realizations and their rows
//                   then reads the row record and its slot at wave-uniform addresses (the scalar cache, as
//                   k_roemer_main does) and takes one of three wave-uniform branches: a mass-only row of a slotted
//                   body evaluates no orbit, an element row of a slotted body one (the perturbed), a row beyond the
//                   slots one or two as k_roemer_main. Rows are summed in ascending order in one register and
//                   sign * acc is rounded as a product before it is added: realization r gets bit for bit what
//                   fpta_roemer_accumulate adds to zeros for table r, whatever C. A realization without rows stores
//                   nothing, a chunk without rows leaves before the prologue; spare lanes of a partial slab repeat its
//                   last TOA and store nothing. No atomics, the block is read and written once.
//   one table for every realization: the delay vector is made once by k_roemer_main<false> on zeros (the drop-in
//                   call's own arithmetic) and added to every row by k_cw_bcast (cw_batch.hip), through the helpers
//                   of the one-table mode that both injections share (bcast_vector, bcast_add).
#include "capi_host.h"
#include "ephem_device.h"
#include "roemer_batch_host.h"
#include "device_common.h"

namespace __attribute__((visibility("hidden"))) capi {

using fpta_roemerb::kRoemerMaxBase;
using fpta_roemerb::Slab;

constexpr int kRmbThreads = fpta_roemerb::kSlabToas;  // one TOA per thread

// grid: ceil(n_real / chunk) x n_slab workgroups in x, the slab fastest. Dynamic LDS: n_base x 3 x kRmbThreads
// doubles. tab_stride 1: realization r sums table r.
__global__ __launch_bounds__(kRmbThreads) void k_roemer_block(
    const Slab* __restrict__ slabs, uint32_t n_slab, const double* __restrict__ toas, int64_t n_toa,
    const double* __restrict__ pos, const int64_t* __restrict__ row_offs, const RoemerRow* __restrict__ rows,
    const int32_t* __restrict__ base_slot, const Body* __restrict__ bases, int32_t n_base, double se, double ce,
    double sign, int32_t n_real, int32_t chunk, int64_t ld, double* __restrict__ block) {
  extern __shared__ double s_orbit[];  // [n_base][3][kRmbThreads]
  const uint32_t cg = blockIdx.x / n_slab, slab = blockIdx.x - cg * n_slab;
  const int32_t r0 = (int32_t)cg * chunk, r1 = min(n_real, r0 + chunk);
  FPTA_DCHECK(r0 < n_real, "k_roemer_block chunk", r0, n_real);
  if (row_offs[r1] <= row_offs[r0]) return;  // nothing to add in this chunk
  const Slab w = slabs[slab];
  const int32_t tid = (int32_t)threadIdx.x;
  const int32_t lane = min(tid, w.count - 1);  // spare lanes repeat the last TOA and store nothing
  const bool live = tid < w.count;
  const int64_t i = w.first + lane;
  FPTA_DCHECK(w.count >= 1 && w.count <= kRmbThreads, "k_roemer_block slab", w.count, kRmbThreads + 1);
  FPTA_DCHECK(i >= 0 && i < n_toa && i < ld, "k_roemer_block toa", i, n_toa < ld ? n_toa : ld);
  FPTA_DCHECK(n_base >= 0 && n_base <= kRoemerMaxBase, "k_roemer_block slots", n_base, kRoemerMaxBase + 1);
  const double t = centuries(toas[i]);
  const double px = pos[3 * w.psr], py = pos[3 * w.psr + 1], pz = pos[3 * w.psr + 2];
  for (int32_t b = 0; b < n_base; ++b) {
    const Vec3 o = orbit_eq(bases[b], t, se, ce);
    double* __restrict__ q = s_orbit + (size_t)b * 3 * kRmbThreads + tid;
    q[0] = o.x;
    q[kRmbThreads] = o.y;
    q[2 * kRmbThreads] = o.z;
  }
  for (int32_t r = r0; r < r1; ++r) {
    const int64_t k0 = row_offs[r], k1 = row_offs[r + 1];
    if (k1 <= k0) continue;
    double acc = 0.0;
    for (int64_t k = k0; k < k1; ++k) {
      const RoemerRow* __restrict__ row = rows + k;
      const int32_t slot = base_slot[k];
      const bool same = row->same != 0.0;
      FPTA_DCHECK(slot >= -1 && slot < n_base, "k_roemer_block slot", slot, n_base);
      Vec3 o, p;  // the base orbit (read only when the row has element deviations) and the perturbed one
      if (slot >= 0) {  // every branch here is wave-uniform
        const double* __restrict__ q = s_orbit + (size_t)slot * 3 * kRmbThreads + tid;
        o = {q[0], q[kRmbThreads], q[2 * kRmbThreads]};
        p = same ? o : orbit_eq(row->pert, t, se, ce);
      } else {
        p = orbit_eq(row->pert, t, se, ce);
        o = same ? p : orbit_eq(row->base, t, se, ce);
      }
      double dx = row->dmass_w * p.x, dy = row->dmass_w * p.y, dz = row->dmass_w * p.z;
      if (!same) {
        const double mw = row->mass_w;
        dx += mw * (p.x - o.x);
        dy += mw * (p.y - o.y);
        dz += mw * (p.z - o.z);
      }
      acc += fma(dz, pz, fma(dy, py, dx * px));
    }
    // the product rounded on its own, as fma(sign, acc, 0) of the drop-in call on zeros is: an opaque value (the
    // compiler contracts a plain or __dmul_rn product into fma(sign, acc, sample), which differs unless sign is +-1)
    double add = sign * acc;
    asm volatile("" : "+v"(add));
    if (live) block[(int64_t)r * ld + i] += add;
  }
}

}  // namespace capi

using namespace capi;

extern "C" int fpta_batch_roemer_accumulate(fpta_ctx* c, const double* pos, int32_t n_tab, const int64_t* row_offs,
                                            const double* rows, double sign) {
  const char* who = "batch_roemer_accumulate";
  Block b;
  int rc;
  if ((rc = block_check(c, who, true, b))) return rc;
  const Layout& L = c->batch;
  const int32_t R = b.R;
  const int64_t n_toa = L.n_toa;
  // everything is validated and the row records made here, before anything is uploaded or launched
  fpta_roemerb::Plan plan;
  std::string why;
  if (!fpta_roemerb::make_plan(L.P, L.h_offs.data(), L.h_toas.data(), R, pos, n_tab, row_offs, rows, sign,
                               c->roemer_chunk, plan, why))
    return fail(c, FPTA_EINVAL, "batch_roemer_accumulate: " + why);
  if (plan.n_row == 0 || n_toa == 0) return FPTA_OK;  // the block, and what is known about it, stay as they are
  const bool shared = n_tab == 1;  // every realization gets the same delay vector
  const int64_t n_slab = (int64_t)plan.slabs.size(), n_cg = ((int64_t)R + plan.chunk - 1) / plan.chunk;
  if (!shared && n_slab * n_cg > 0x7FFFFFFF) return fail(c, FPTA_EINVAL, "batch_roemer_accumulate: block too large");

  if ((rc = block_open(c, true))) return rc;
  std::vector<EphWave> waves;  // (lives until the sync below)
  if (shared) {
    if ((rc = bcast_vector(c, who, c->rmb_v))) return rc;
    KTimer kt(c, FPTA_K_EPHEM);
    if ((rc = roemer_sum_launch(c, L.P, L.h_offs.data(), L.toas.as<double>(), pos, plan.rows, sign, n_toa, waves,
                                c->rmb_v.as<double>())))
      return rc;
    if ((rc = bcast_add(c, who, c->rmb_v, b))) return rc;
  } else {
    const fpta_ephem::Obliquity ob = fpta_ephem::obliquity();
    const int32_t n_base = (int32_t)plan.bases.size();
    const size_t lds = sizeof(double) * 3 * kRmbThreads * (size_t)n_base;  // 6 KB per slot, <= 48 KB
    if ((rc = upload(c, c->rmb_pos, pos, sizeof(double) * 3 * (size_t)L.P, "roemer batch pos"))) return rc;
    if ((rc = upload(c, c->rmb_offs, row_offs, sizeof(int64_t) * ((size_t)n_tab + 1), "roemer batch offsets")))
      return rc;
    if ((rc = upload(c, c->rmb_rows, plan.rows.data(), sizeof(RoemerRow) * plan.rows.size(), "roemer batch rows")))
      return rc;
    if ((rc = upload(c, c->rmb_slots, plan.base_slot.data(), sizeof(int32_t) * plan.base_slot.size(),
                     "roemer batch slots")))
      return rc;
    if ((rc = upload(c, c->rmb_bases, plan.bases.data(), sizeof(Body) * plan.bases.size(), "roemer batch bases")))
      return rc;
    if ((rc = upload(c, c->rmb_slabs, plan.slabs.data(), sizeof(Slab) * plan.slabs.size(), "roemer batch slabs")))
      return rc;
    KTimer kt(c, FPTA_K_EPHEM);
    k_roemer_block<<<dim3((unsigned)(n_slab * n_cg)), dim3(kRmbThreads), lds, c->stream>>>(
        c->rmb_slabs.as<Slab>(), (uint32_t)n_slab, L.toas.as<double>(), n_toa, c->rmb_pos.as<double>(),
        c->rmb_offs.as<int64_t>(), c->rmb_rows.as<RoemerRow>(), c->rmb_slots.as<int32_t>(), c->rmb_bases.as<Body>(),
        n_base, ob.sn, ob.cs, sign, R, plan.chunk, b.ld, b.res);
    HIPCHK(c, hipGetLastError(), "k_roemer_block launch");
  }
  // the tables above are this call's own host memory: the stream has taken them once it has run
  HIPCHK(c, hipStreamSynchronize(c->stream), "batch_roemer_accumulate sync");
  return FPTA_OK;
}
