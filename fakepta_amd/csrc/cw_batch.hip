// Continuous-wave populations injected into the context's last batch block, in place (fpta_batch_cw_accumulate):
//   block[r][i] += sign * sum over the sources s of realization r's table of delay(t_i; s, pulsar of i)
// with the delay of cw_device.h, the one fpta_cw_accumulate evaluates. Every realization has its own source table
// (ragged, CSR); the per-source constants of all of them are made on the host (cw_batch_host.h), the (pulsar, source)
// pair constants inside the kernel, so no table grows with R x P x S.
//
//   k_cw_block  one workgroup of 4 waves per (slab of <= 256 consecutive TOAs of one pulsar, realization), one TOA per
//               lane. The realization's sources go through LDS in tiles of kCwbTile: thread j makes {Es, Ec, shift} of
//               source s0 + j for this (realization, pulsar) (cw_pair, as k_cw_prep does), and after a barrier every
//               wave that holds a TOA loops over the tile. The pair is read at a wave-uniform LDS address (a broadcast)
//               and moved to scalar registers, the per-source record comes through the scalar cache as in k_cw_main,
//               so the loop body is k_cw_main's and the pulsar-term branch a scalar one. Sources are summed in
//               ascending order in one register: no atomics, the block is read and written once, and realization r
//               gets bit for bit what fpta_cw_accumulate adds to zeros in one piece (FPTA_OPT_CW_SPLIT 1). A realization
//               without sources returns at once; spare lanes of a partial wave repeat the slab's last TOA and store
//               nothing; a wave without TOAs only helps with the pairs.
//   k_cw_bcast  one table for every realization (and one distance per pulsar): block[r][i] += v[i], v the delay vector
//               that k_cw_prep / k_cw_main / k_cw_reduce made on the device with the drop-in call's split rule.
//               Memory-bound: each thread adds its column's v to kCwbRows rows.
#include "capi_host.h"
#include "cw_batch_host.h"
#include "cw_device.h"
#include "device_common.h"

namespace __attribute__((visibility("hidden"))) capi {

using fpta_cwb::Slab;

constexpr int kCwbThreads = fpta_cwb::kSlabToas;  // one TOA per thread
constexpr int kCwbTile = 128;                     // sources of one LDS tile (4 KB of pairs)
static_assert(kCwbTile <= kCwbThreads, "one thread per source of a tile");

// a wave-uniform double held in vector registers, as a scalar value
__device__ __forceinline__ double cwb_uniform(double x) {
  const uint64_t u = (uint64_t)__double_as_longlong(x);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// grid: n_real x n_slab workgroups in x, the slab fastest. tab_stride 1: realization r sums table r; 0: table 0.
// L_stride 0: Ls [n_psr]; n_psr: Ls [n_real][n_psr].
__global__ __launch_bounds__(kCwbThreads) void k_cw_block(
    const Slab* __restrict__ slabs, uint32_t n_slab, const double* __restrict__ toas, int64_t n_toa,
    const double* __restrict__ pos, const double* __restrict__ Ls, int64_t L_stride,
    const int64_t* __restrict__ src_offs, int32_t tab_stride, const SrcEval* __restrict__ ev,
    const SrcGeom* __restrict__ gm, double sign, int32_t n_real, int64_t ld, double* __restrict__ block) {
  __shared__ CwPair sp[kCwbTile];
  const uint32_t r = blockIdx.x / n_slab, slab = blockIdx.x - r * n_slab;
  FPTA_DCHECK((int32_t)r < n_real, "k_cw_block realization", r, n_real);
  const int64_t tab = (int64_t)r * tab_stride;
  const int64_t s_begin = src_offs[tab], s_end = src_offs[tab + 1];
  if (s_end <= s_begin) return;  // nothing to add: the whole workgroup leaves before any barrier
  const Slab w = slabs[slab];
  const int32_t tid = (int32_t)threadIdx.x;
  const int32_t lane = min(tid, w.count - 1);  // spare lanes repeat the last TOA and store nothing
  const int64_t i = w.first + lane;
  FPTA_DCHECK(w.count >= 1 && w.count <= kCwbThreads, "k_cw_block slab", w.count, kCwbThreads + 1);
  FPTA_DCHECK(i >= 0 && i < n_toa && i < ld, "k_cw_block toa", i, n_toa < ld ? n_toa : ld);
  const double t = toas[i];
  const double px = pos[3 * w.psr], py = pos[3 * w.psr + 1], pz = pos[3 * w.psr + 2];
  const double L = Ls[(int64_t)r * L_stride + w.psr];
  // the wave's first TOA is inside the slab (wave-uniform: the first lane's thread index)
  const bool wave_live = (int32_t)__builtin_amdgcn_readfirstlane(tid) < w.count;
  double acc = 0.0;
  for (int64_t s0 = s_begin; s0 < s_end; s0 += kCwbTile) {
    const int32_t nt = (int32_t)min((int64_t)kCwbTile, s_end - s0);
    if (tid < nt) sp[tid] = cw_pair(gm[s0 + tid], px, py, pz, L, sign);
    __syncthreads();
    if (wave_live) {
      const SrcEval* __restrict__ et = ev + s0;
      for (int32_t k = 0; k < nt; ++k) {
        const SrcEval e = et[k];
        const CwPair q = sp[k];
        acc += cw_delay(e, cwb_uniform(q.Es), cwb_uniform(q.Ec), cwb_uniform(q.shift), t);
      }
    }
    __syncthreads();  // the next tile overwrites the pairs
  }
  if (tid < w.count) block[(int64_t)r * ld + i] += acc;
}

// grid: ceil(n_real / kCwbRows) x ceil(n_toa / 256) workgroups in x, the column chunk fastest
__global__ __launch_bounds__(256) void k_cw_bcast(const double* __restrict__ v, int64_t n_toa, uint32_t n_chunk,
                                                   int32_t n_real, int64_t ld, double* __restrict__ block) {
  const uint32_t rg = blockIdx.x / n_chunk, chunk = blockIdx.x - rg * n_chunk;
  const int64_t i = (int64_t)chunk * 256 + threadIdx.x;
  if (i >= n_toa) return;
  FPTA_DCHECK(i < ld, "k_cw_bcast column", i, ld);
  const double x = v[i];
  const int32_t r0 = (int32_t)rg * kCwbRows, r1 = min(n_real, r0 + kCwbRows);
  FPTA_DCHECK(r0 < n_real, "k_cw_bcast realization", r0, n_real);
  for (int32_t r = r0; r < r1; ++r) block[(int64_t)r * ld + i] += x;
}

int bcast_vector(fpta_ctx* c, const char* who, DevBuf& v) {
  const std::string what = std::string(who) + " delay vector";
  const size_t bytes = sizeof(double) * (size_t)c->batch.n_toa;
  HIPCHK(c, v.ensure(bytes), what.c_str());
  HIPCHK(c, hipMemsetAsync(v.p, 0, bytes, c->stream), what.c_str());
  return FPTA_OK;
}

int bcast_add(fpta_ctx* c, const char* who, const DevBuf& v, const Block& b) {
  const int64_t n_toa = c->batch.n_toa;
  const int64_t n_chunk = (n_toa + 255) / 256, n_rg = ((int64_t)b.R + kCwbRows - 1) / kCwbRows;
  // (a block that large, 32 TB, fits no device: the refusal only guards the grid's arithmetic)
  if (n_chunk * n_rg > 0x7FFFFFFF) return fail(c, FPTA_EINVAL, std::string(who) + ": block too large");
  k_cw_bcast<<<dim3((unsigned)(n_chunk * n_rg)), dim3(256), 0, c->stream>>>(v.as<double>(), n_toa, (uint32_t)n_chunk,
                                                                           b.R, b.ld, b.res);
  HIPCHK(c, hipGetLastError(), "k_cw_bcast launch");
  return FPTA_OK;
}

}  // namespace capi

using namespace capi;

extern "C" int fpta_batch_cw_accumulate(fpta_ctx* c, const double* pos, const double* pdist_s, int64_t pdist_stride,
                                        int32_t n_tab, const int64_t* src_offs, const double* src, double sign) {
  const char* who = "batch_cw_accumulate";
  Block b;
  int rc;
  if ((rc = block_check(c, who, true, b))) return rc;
  const Layout& L = c->batch;
  const int32_t R = b.R;
  const int64_t n_toa = L.n_toa;
  // everything is validated and the per-source constants made here, before anything is uploaded or launched
  double tmax = L.h_toas[0];
  for (int64_t i = 1; i < n_toa; ++i) tmax = std::max(tmax, L.h_toas[(size_t)i]);
  fpta_cwb::Plan plan;
  std::string why;
  if (!fpta_cwb::make_plan(L.P, L.h_offs.data(), tmax, R, pos, pdist_s, pdist_stride, n_tab, src_offs, src, sign, plan,
                           why))
    return fail(c, FPTA_EINVAL, "batch_cw_accumulate: " + why);
  if (plan.n_src == 0) return FPTA_OK;  // the block, and what is known about it, stay as they are
  const bool shared = n_tab == 1 && pdist_stride == 0;  // every realization gets the same delay vector
  const int64_t n_slab = (int64_t)plan.slabs.size();
  if (shared) {
    if (plan.n_src > 0x7FFFFFFF || (int64_t)L.P * plan.n_src > (int64_t)1 << 31)
      return fail(c, FPTA_EINVAL, "batch_cw_accumulate: more than 2^31 (pulsar, source) pairs");
  } else if (n_slab * R > 0x7FFFFFFF) {
    return fail(c, FPTA_EINVAL, "batch_cw_accumulate: too many TOA slabs x realizations");
  }

  if ((rc = block_open(c, true))) return rc;
  CwRun run;  // (its wave table lives until the sync below)
  if (shared) {
    if ((rc = cw_prepare(c, L.P, L.h_offs.data(), pos, pdist_s, plan.ev, plan.gm, run))) return rc;
    if ((rc = bcast_vector(c, who, c->cwb_v))) return rc;
    KTimer kt(c, FPTA_K_CW);
    if ((rc = cw_launch(c, run, L.toas.as<double>(), sign, c->cwb_v.as<double>()))) return rc;
    if ((rc = bcast_add(c, who, c->cwb_v, b))) return rc;
  } else {
    const size_t n_dist = pdist_stride ? (size_t)R * (size_t)L.P : (size_t)L.P;
    if ((rc = upload(c, c->cwb_pos, pos, sizeof(double) * 3 * (size_t)L.P, "cw batch pos"))) return rc;
    if ((rc = upload(c, c->cwb_L, pdist_s, sizeof(double) * n_dist, "cw batch pdist"))) return rc;
    if ((rc = upload(c, c->cwb_offs, src_offs, sizeof(int64_t) * ((size_t)n_tab + 1), "cw batch offsets"))) return rc;
    if ((rc = upload(c, c->cwb_ev, plan.ev.data(), sizeof(SrcEval) * plan.ev.size(), "cw batch sources"))) return rc;
    if ((rc = upload(c, c->cwb_gm, plan.gm.data(), sizeof(SrcGeom) * plan.gm.size(), "cw batch source geometry")))
      return rc;
    if ((rc = upload(c, c->cwb_slabs, plan.slabs.data(), sizeof(Slab) * plan.slabs.size(), "cw batch slabs"))) return rc;
    KTimer kt(c, FPTA_K_CW);
    k_cw_block<<<dim3((unsigned)(n_slab * R)), dim3(kCwbThreads), 0, c->stream>>>(
        c->cwb_slabs.as<Slab>(), (uint32_t)n_slab, L.toas.as<double>(), n_toa, c->cwb_pos.as<double>(),
        c->cwb_L.as<double>(), pdist_stride, c->cwb_offs.as<int64_t>(), n_tab == 1 ? 0 : 1, c->cwb_ev.as<SrcEval>(),
        c->cwb_gm.as<SrcGeom>(), sign, R, b.ld, b.res);
    HIPCHK(c, hipGetLastError(), "k_cw_block launch");
  }
  // the tables above are this call's own host memory: the stream has taken them once it has run
  HIPCHK(c, hipStreamSynchronize(c->stream), "batch_cw_accumulate sync");
  return FPTA_OK;
}
