// Timing-model projection (fpta_batch_set_timing_model, fpta_batch_project, fpta_tm_project): the weighted
// least-squares remainder r' = r - (Q g) / s, g = Q^T (s o r), of every realization of a block [R][ld] in place, with
// the per-pulsar orthonormal basis Q [n_toa][16] and s = sqrt(w) of tm_host.h, on v_mfma_f64_16x16x4_f64.
//
//   k_tm_project  one pulsar x one tile of 16 realizations per workgroup of kTmWaves waves; wave w takes the pulsar's
//                 16-TOA chunks w, w + kTmWaves, .. in both sweeps (ascending, then descending). In a chunk lane
//                 (lr, lg) owns TOAs 2 lg, 2 lg + 1, 8 + 2 lg and 9 + 2 lg of realization lr (tm_toa): two 16-byte runs
//                 of its own row, so the four lane groups of a row read 64 contiguous bytes per load, and the same
//                 addresses in both sweeps.
//                 Sweep 1: g [16][16 realizations] += Q^T (s o r), four k-steps per chunk; k-step q takes the q-th TOA
//                 of each lane group (the reduction index may be any fixed permutation of the TOAs). The waves'
//                 partial g are summed through LDS in wave order, so every wave holds the same g.
//                 Sweep 2: 16 TOAs x 16 realizations of Q g in ceil(k_p / 4) k-steps. Accumulator register q of lane
//                 group lg is g row lg + 4 q, which is what k-step q wants as its B operand, so g never moves; the A
//                 operand's row i is the (i >> 2)-th TOA of lane group i & 3, so the result's rows lg + 4 q are the
//                 lane's own TOAs.
// No atomics and no dependence on the neighbours: a realization's result is the same whatever R, its position in the
// block and the realizations that share its tile. Rows start at offs[p]: 8-byte aligned only, so the 16-byte accesses
// are typed 8-byte aligned; the pulsar's last, partial chunk goes element by element under a mask, and a lane past
// the last realization reads the last one and stores nothing.
#include "capi_host.h"
#include "tm_host.h"
#include "device_common.h"

namespace __attribute__((visibility("hidden"))) capi {

constexpr int kTmCol = fpta_tm::kMaxCol;
constexpr int kTmReal = 16;   // realizations of a tile
constexpr int kTmChunk = 16;  // TOAs of a chunk
// waves of a workgroup: more waves per tile mean fewer tiles in flight, so that the second sweep finds its tile in the
// caches (variant builds: make variant DEFS=-DFPTA_TM_WAVES=4)
#ifndef FPTA_TM_WAVES
#define FPTA_TM_WAVES 16
#endif
constexpr int kTmWaves = FPTA_TM_WAVES;
static_assert(kTmCol == 16 && kTmReal == 16 && kTmChunk == 16, "k_tm_project's lane maps are written for 16 x 16 x 16");
static_assert(kTmWaves >= 1 && kTmWaves <= 16, "a workgroup holds at most 16 waves");

typedef double d2u __attribute__((ext_vector_type(2), aligned(8)));  // two doubles at an 8-byte aligned address

struct TmArgs {
  double* res;          // [R][ld]
  int64_t ld;
  int32_t R, n_rt;      // realizations, tiles of kTmReal of them
  const double* Q;      // [n_toa][kTmCol]
  const double* s;      // [n_toa]
  const int64_t* offs;  // [n_psr + 1]
  const int32_t* rank;  // [n_psr]
};

// the chunk-local TOA of lane group lg's q-th sample
__device__ __forceinline__ int tm_toa(int lg, int q) { return ((q >> 1) << 3) + 2 * lg + (q & 1); }

// grid: n_psr x n_rt workgroups, the realization tile fastest (neighbours share a pulsar's Q)
__global__ __launch_bounds__(64 * kTmWaves) void k_tm_project(TmArgs a) {
  __shared__ double sG[kTmWaves][4][64];
  const int p = (int)(blockIdx.x / (unsigned)a.n_rt), rt = (int)(blockIdx.x - (unsigned)p * (unsigned)a.n_rt);
  const int kp = a.rank[p];
  if (kp == 0) return;  // nothing to remove: the samples stay as they are
  const int64_t o = a.offs[p];
  const int n = (int)(a.offs[p + 1] - o);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lg = lane >> 4;
  const int real = rt * kTmReal + lr;
  const bool live = real < a.R;
  double* __restrict__ row = a.res + (int64_t)(live ? real : a.R - 1) * a.ld + o;
  const double* __restrict__ Q = a.Q + o * kTmCol;
  const double* __restrict__ s = a.s + o;
  const int n_full = n / kTmChunk;                         // whole chunks
  const bool tail = wave == n_full % kTmWaves && n_full * kTmChunk < n;  // this wave takes the partial one
  const int t_tail = n_full * kTmChunk;
  FPTA_DCHECK(o + n <= a.ld, "k_tm_project row", o + n, a.ld + 1);

  d4 g = d4{0.0, 0.0, 0.0, 0.0};
  for (int c = wave; c < n_full; c += kTmWaves) {
    const int t = c * kTmChunk + 2 * lg;
    const d2u x0 = *(const d2u*)(row + t), x1 = *(const d2u*)(row + t + 8);
    const d2u s0 = *(const d2u*)(s + t), s1 = *(const d2u*)(s + t + 8);
    const double x[4] = {x0.x * s0.x, x0.y * s0.y, x1.x * s1.x, x1.y * s1.y};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double qv = Q[(int64_t)(c * kTmChunk + tm_toa(lg, q)) * kTmCol + lr];
      g = __builtin_amdgcn_mfma_f64_16x16x4f64(qv, x[q], g, 0, 0, 0);
    }
  }
  if (tail) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int t = t_tail + tm_toa(lg, q);
      const bool in = t < n;
      const double x = in ? row[t] * s[t] : 0.0;
      const double qv = in ? Q[(int64_t)t * kTmCol + lr] : 0.0;
      g = __builtin_amdgcn_mfma_f64_16x16x4f64(qv, x, g, 0, 0, 0);
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) sG[wave][q][lane] = g[q];
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    double v = sG[0][q][lane];
#pragma unroll
    for (int w = 1; w < kTmWaves; ++w) v += sG[w][q][lane];
    g[q] = v;
  }

  const int nks = (kp + 3) >> 2;
  const int ta = tm_toa(lr & 3, lr >> 2);  // the chunk-local TOA of A-operand row lr
  // the chunks in descending order: what the first sweep read last is the likeliest to be in the L2 still
  if (tail) {
    const bool qin = t_tail + ta < n;
    d4 d = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
      if (ks < nks) {
        const double qv = qin ? Q[(int64_t)(t_tail + ta) * kTmCol + 4 * ks + lg] : 0.0;
        d = __builtin_amdgcn_mfma_f64_16x16x4f64(qv, g[ks], d, 0, 0, 0);
      }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int t = t_tail + tm_toa(lg, q);
      if (live && t < n) row[t] = row[t] - d[q] / s[t];
    }
  }
  for (int c = wave + (n_full - 1 - wave) / kTmWaves * kTmWaves; c >= wave && n_full > wave; c -= kTmWaves) {
    const double* __restrict__ qa = Q + (int64_t)(c * kTmChunk + ta) * kTmCol + lg;
    d4 d = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
      if (ks < nks) d = __builtin_amdgcn_mfma_f64_16x16x4f64(qa[4 * ks], g[ks], d, 0, 0, 0);
    const int t = c * kTmChunk + 2 * lg;
    d2u x0 = *(const d2u*)(row + t), x1 = *(const d2u*)(row + t + 8);
    const d2u s0 = *(const d2u*)(s + t), s1 = *(const d2u*)(s + t + 8);
    x0.x -= d[0] / s0.x;
    x0.y -= d[1] / s0.y;
    x1.x -= d[2] / s1.x;
    x1.y -= d[3] / s1.y;
    if (live) {
      *(d2u*)(row + t) = x0;
      *(d2u*)(row + t + 8) = x1;
    }
  }
}

// The launch of a block [R][ld] against device tables; n_psr x ceil(R / 16) workgroups
static int tm_launch(fpta_ctx* c, const Block& b, const TmSlot& s) {
  TmArgs a;
  a.res = b.res;
  a.ld = b.ld;
  a.R = b.R;
  a.n_rt = (b.R + kTmReal - 1) / kTmReal;
  a.Q = s.q.as<double>();
  a.s = s.s.as<double>();
  a.offs = s.offs.as<int64_t>();
  a.rank = s.rank.as<int32_t>();
  const int64_t blocks = (int64_t)b.n_psr * a.n_rt;
  if (blocks > 0x7FFFFFFF) return fail(c, FPTA_EINVAL, "tm_project: too many pulsars x realization tiles");
  KTimer kt(c, FPTA_K_DENSE);
  k_tm_project<<<dim3((unsigned)blocks), dim3(64 * kTmWaves), 0, c->stream>>>(a);
  HIPCHK(c, hipGetLastError(), "k_tm_project launch");
  return FPTA_OK;
}

static int tm_upload(fpta_ctx* c, const fpta_tm::Plan& plan, int32_t n_psr, const int64_t* offs, TmSlot& s) {
  int rc;
  if ((rc = upload(c, s.q, plan.Q.data(), sizeof(double) * plan.Q.size(), "tm basis"))) return rc;
  if ((rc = upload(c, s.s, plan.s.data(), sizeof(double) * plan.s.size(), "tm weights"))) return rc;
  if ((rc = upload(c, s.offs, offs, sizeof(int64_t) * ((size_t)n_psr + 1), "tm offs"))) return rc;
  if ((rc = upload(c, s.rank, plan.rank.data(), sizeof(int32_t) * (size_t)n_psr, "tm ranks"))) return rc;
  return FPTA_OK;
}

}  // namespace capi

using namespace capi;

extern "C" int fpta_batch_set_timing_model(fpta_ctx* c, int32_t n_col, const double* M, const int32_t* ncol_psr,
                                           const double* weights, double rcond, int32_t* rank_out) {
  if (!c) return fail(nullptr, FPTA_EINVAL, "null ctx");
  const Layout& L = c->batch;
  if (L.P <= 0) return fail(c, FPTA_ESTATE, "set_timing_model: set_toas first");
  if (n_col == 0) {
    c->tm_st.clear();
    if (rank_out) std::fill(rank_out, rank_out + L.P, 0);
    return FPTA_OK;
  }
  // everything is validated and the basis built here, before anything is uploaded
  std::string why;
  fpta_tm::Plan plan;
  if (!fpta_tm::make_plan(L.P, L.h_offs.data(), n_col, M, ncol_psr, weights, rcond, plan, why))
    return fail(c, FPTA_EINVAL, "set_timing_model: " + why);
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  c->tm_st.clear();
  // a projection of the previous model may still read the tables (an upload into a buffer that does not grow)
  HIPCHK(c, hipStreamSynchronize(c->stream), "set_timing_model sync");
  int rc;
  if ((rc = tm_upload(c, plan, L.P, L.h_offs.data(), c->tm))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream), "set_timing_model sync");
  c->tm_st.set = true;
  if (rank_out) std::copy(plan.rank.begin(), plan.rank.end(), rank_out);
  return FPTA_OK;
}

extern "C" int fpta_batch_project(fpta_ctx* c) {
  Block b;
  int rc;
  if ((rc = block_check(c, "project", false, b))) return rc;
  if (!c->tm_st.set) return fail(c, FPTA_ESTATE, "project: no timing model (set_timing_model first)");
  if ((rc = block_open(c, true))) return rc;
  return tm_launch(c, b, c->tm);
}

extern "C" int fpta_tm_project(fpta_ctx* c, int32_t n_psr, const int64_t* offs, const double* M, int32_t n_col,
                               const int32_t* ncol_psr, const double* weights, double rcond, int32_t n_vec, double* res,
                               int32_t* rank_out) {
  const OneShot one{c, "tm_project", n_psr, offs, n_vec, res};
  int rc;
  if ((rc = one.check())) return rc;
  std::string why;
  fpta_tm::Plan plan;
  const bool made = fpta_tm::make_plan(n_psr, offs, n_col, M, ncol_psr, weights, rcond, plan, why);
  if ((rc = one.planned(made ? 0 : 1, why))) return rc;
  if (rank_out) std::copy(plan.rank.begin(), plan.rank.end(), rank_out);
  if (n_psr == 0 || n_vec == 0 || one.n_toa() == 0 || plan.max_rank == 0) return FPTA_OK;  // res stays as it is
  Block b;
  if ((rc = one.upload(b))) return rc;
  if ((rc = tm_upload(c, plan, n_psr, offs, c->tm1))) return rc;
  if ((rc = tm_launch(c, b, c->tm1))) return rc;
  HIPCHK(c, hipMemcpyAsync(res, b.res, sizeof(double) * (size_t)b.R * (size_t)b.ld, hipMemcpyDeviceToHost, c->stream),
         "tm_project download");
  return one.done();
}
