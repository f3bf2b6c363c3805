// Likelihood ratio of a common process on a spectrum grid (fpta_batch_set_lnl, fpta_batch_lnl_info, fpta_batch_lnl,
// fpta_lnl_grid): per realization and grid point dlnL[g][r] = sum_p (q[p][g][r] - ld[p][g]) / 2 with q = |U_pg X_p,r|^2.
// The definition is in include/fakepta_amd.h; the operator B_p, the factors U_pg and the log-determinants are
// lnl_host.h's.
//
//   stage 1  X = B_p r of every realization: k_fit_apply (fit.hip) on this file's operator slot and coefficient buffer
//            [P][K][R_pad]. The same instances as the Fourier fit and the optimal statistic, whose slots are not touched.
//   stage 2  k_lnl_quad<NH>: a workgroup of 4 waves owns one pulsar, a tile of 16 NH realizations and up to kLnlGrid
//            grid points. It stages the X tile (rows past K and realizations past R_pad as zeros) into LDS once, in the
//            order the MFMA's B operand wants it: [block of 8 columns][realization block][lane] as pairs, one 16-byte
//            LDS read per pair of k-steps. Wave w then takes the grid points w, w + 4, .. of the chunk. Per grid point
//            and 16-row group j of U it runs the k-steps 0 .. 4 (j + 1) - 1 only (U is lower triangular: the triangular
//            saving), v_mfma_f64_16x16x4_f64 with A = U's [16 rows][4 columns] read from memory as one 16-byte run per
//            lane and pair of k-steps (lnl_host.h lays U out so that a wave's load is 1 KB contiguous and a grid point's
//            loads one stream, of which four stay in flight), and each A value feeds NH MFMAs. After a group's last
//            k-step the lane adds the squares of its four accumulator rows, in row order, to its running sum of the
//            realization; after the last group the four lanes that hold a realization
//            are summed by a butterfly. A fixed order, no atomics, nothing shared between realizations or grid points:
//            q[p][g][r] is the same whatever R, G, the realization's position and its neighbours, and NH (4 while the X
//            tile of 64 realizations fits 64 KB of LDS, K <= 128, else 2) changes no column's operations.
//   k_lnl_reduce: dlnL[g][r] = sum_p (q[p][g][r] - ld[p][g]) / 2 in pulsar order, one thread per (g, r).
// Padding realizations have X = 0 (the cleared buffer) and give q = 0; they are not downloaded.
#include "capi_host.h"
#include "lnl_host.h"
#include "device_common.h"

namespace __attribute__((visibility("hidden"))) capi {

constexpr int kLnlWaves = 4;   // waves of a workgroup
constexpr int kLnlGrid = 32;   // grid points of a workgroup, at most
constexpr int kLnlRpad = 32;   // k_fit_apply's realization padding
constexpr int kLnlAhead = 4;   // blocks of U a wave keeps in flight

typedef double ld2 __attribute__((ext_vector_type(2)));

struct LnlArgs {
  const double* X;   // [P][K][R_pad]
  const double* U;   // [P][G][u_stride], lnl_host.h's layout
  double* q;         // [P][G][R_pad]
  int64_t u_stride;
  int32_t K, KG, G, R_pad;
};

// grid: (tiles of 16 NH realizations, chunks of kLnlGrid grid points, P); dynamic LDS: 16 KG x 16 NH doubles
template <int NH>
__global__ __launch_bounds__(64 * kLnlWaves) void k_lnl_quad(LnlArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sLnl[];
  const ld2* sX = (const ld2*)sLnl;  // [block of 8 columns][realization block][lane]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15;
  const int r0 = (int)blockIdx.x * 16 * NH, g0 = (int)blockIdx.y * kLnlGrid, p = (int)blockIdx.z;
  const int K = a.K, KG = a.KG, T = KG * (KG + 1);  // T: 8-column blocks of one grid point's U
  constexpr int W = 16 * NH;

  // the X tile: element (column k, realization rr of the tile), coalesced along the realizations
  const double* __restrict__ Xp = a.X + (int64_t)p * K * a.R_pad;
  for (int i = tid; i < 16 * KG * W; i += 64 * kLnlWaves) {
    const int k = i / W, rr = i - k * W, r = r0 + rr;
    const bool in = k < K && r < a.R_pad;
    const double x = Xp[(int64_t)(in ? k : 0) * a.R_pad + (in ? r : 0)];
    const int slot = (((k >> 3) * NH + (rr >> 4)) * 64 + ((k & 7) >> 1) * 16 + (rr & 15)) * 2 + (k & 1);
    sLnl[slot] = in ? x : 0.0;
  }
  __syncthreads();

  const int g_end = min(g0 + kLnlGrid, a.G);
  for (int g = g0 + wave; g < g_end; g += kLnlWaves) {  // wave-uniform
    const ld2* __restrict__ Ug = (const ld2*)(a.U + ((int64_t)p * a.G + g) * a.u_stride) + lane;
    double sum[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) sum[h] = 0.0;
    // the grid point's blocks of U are one contiguous stream, group after group: kLnlAhead loads stay in flight
    d4 acc[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) acc[h] = d4{0.0, 0.0, 0.0, 0.0};
    ld2 u[kLnlAhead];
#pragma unroll
    for (int d = 0; d < kLnlAhead; ++d) u[d] = Ug[(d < T ? d : T - 1) * 64];
    for (int t0 = 0, q = 0, nq = 2; t0 < T; t0 += kLnlAhead) {
#pragma unroll
      for (int d = 0; d < kLnlAhead; ++d) {
        const int t = t0 + d;
        if (t < T) {  // wave-uniform
          const ld2 cur = u[d];
          u[d] = Ug[(t + kLnlAhead < T ? t + kLnlAhead : T - 1) * 64];
#pragma unroll
          for (int h = 0; h < NH; ++h) {
            const ld2 b = sX[(q * NH + h) * 64 + lane];
            acc[h] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur.x, b.x, acc[h], 0, 0, 0);
            acc[h] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur.y, b.y, acc[h], 0, 0, 0);
          }
          if (++q == nq) {  // the row group's diagonal block is done: its squares, then the next group
#pragma unroll
            for (int h = 0; h < NH; ++h) {
              double s = sum[h];
              s = fma(acc[h][0], acc[h][0], s);
              s = fma(acc[h][1], acc[h][1], s);
              s = fma(acc[h][2], acc[h][2], s);
              s = fma(acc[h][3], acc[h][3], s);
              sum[h] = s;
              acc[h] = d4{0.0, 0.0, 0.0, 0.0};
            }
            q = 0;
            nq += 2;
          }
        }
      }
    }
    double* __restrict__ qg = a.q + ((int64_t)p * a.G + g) * a.R_pad;
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      double s = sum[h];
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      const int r = r0 + h * 16 + lr;
      if (lane < 16 && r < a.R_pad) qg[r] = s;
    }
  }
}

// dlnL[g][r] = sum_p (q[p][g][r] - ld[p][g]) / 2, in pulsar order; one thread per (g, r)
__global__ __launch_bounds__(256) void k_lnl_reduce(const double* __restrict__ q, const double* __restrict__ ld,
                                                     int32_t P, int32_t G, int32_t R_pad, int64_t n,
                                                     double* __restrict__ d) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const int64_t g = e / R_pad;
  double s = 0.0;
  for (int32_t p = 0; p < P; ++p) s += 0.5 * (q[(int64_t)p * G * R_pad + e] - ld[(int64_t)p * G + g]);
  d[e] = s;
}

// Device copies of a plan's tables. U is the large one (8 P G u_stride bytes), then the operator (8 K n_toa bytes).
static int lnl_upload(fpta_ctx* c, const fpta_lnl::Plan& plan, int32_t n_psr, const int64_t* offs, LnlSlot& s) {
  int rc;
  if ((rc = fit_upload(c, "lnl", s.x, plan.K, plan.B, n_psr, offs, plan.rows))) return rc;
  const size_t b_u = sizeof(double) * plan.U.size();
  if (s.u.ensure(b_u) != hipSuccess)
    return fail(c, FPTA_ENOMEM, "lnl: no device memory for the factors of " + std::to_string(b_u) +
                                    " bytes (K = " + std::to_string(plan.K) + ", G = " + std::to_string(plan.G) + ")");
  if ((rc = upload(c, s.u, plan.U.data(), b_u, "lnl factors"))) return rc;
  if ((rc = upload(c, s.ld, plan.ld.data(), sizeof(double) * plan.ld.size(), "lnl log-determinants"))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream), "lnl upload sync");
  return FPTA_OK;
}

// Both stages and the reduction on a block of st.K columns and st.G grid points; one FPTA_K_DENSE entry. The results
// stay in the slot, padded to st.rpad realizations: X [P][K][rpad], q [P][G][rpad], dlnL [G][rpad].
static int lnl_launch(fpta_ctx* c, const Block& b, LnlSlot& s, LnlState& st) {
  const int32_t R = b.R, n_psr = b.n_psr, K = st.K, G = st.G;
  const int32_t R_pad = st.rpad = (R + kLnlRpad - 1) / kLnlRpad * kLnlRpad;
  const size_t b_x = sizeof(double) * (size_t)n_psr * (size_t)K * (size_t)R_pad;
  const size_t b_q = sizeof(double) * (size_t)n_psr * (size_t)G * (size_t)R_pad, b_d = sizeof(double) * (size_t)G * R_pad;
  if (s.x.coef.ensure(b_x) != hipSuccess || s.q.ensure(b_q) != hipSuccess || s.d.ensure(b_d) != hipSuccess)
    return fail(c, FPTA_ENOMEM, "lnl: no device memory for " + std::to_string(b_x + b_q + b_d) + " bytes of results");
  const int32_t KG = fpta_lnl::groups_of(K);
  const int nh = KG <= 8 ? 4 : 2;  // the X tile [16 KG][16 NH] doubles stays within 64 KB of LDS
  const int64_t n_rt = (R_pad + 16 * nh - 1) / (16 * nh), n_gc = (G + kLnlGrid - 1) / kLnlGrid;
  if (n_rt > 0x7FFFFFFF || n_gc > 65535 || n_psr > 65535)
    return fail(c, FPTA_EINVAL, "lnl: too many realization tiles, grid chunks or pulsars");
  KTimer kt(c, FPTA_K_DENSE);
  int32_t rp = 0;
  int rc = fit_launch_unbooked(c, b, K, s.x, rp);
  if (rc) return rc;
  if (rp != R_pad) return fail(c, FPTA_EINVAL, "lnl: k_fit_apply's realization padding changed");
  if (G == 0 || R == 0 || n_psr == 0) return FPTA_OK;
  LnlArgs a;
  a.X = s.x.coef.as<double>();
  a.U = s.u.as<double>();
  a.q = s.q.as<double>();
  a.u_stride = fpta_lnl::packed_size(K);
  a.K = K;
  a.KG = KG;
  a.G = G;
  a.R_pad = R_pad;
  const dim3 grid((unsigned)n_rt, (unsigned)n_gc, (unsigned)n_psr), block(64 * kLnlWaves);
  const size_t lds = sizeof(double) * 16 * (size_t)KG * 16 * (size_t)nh;
  if (nh == 4)
    k_lnl_quad<4><<<grid, block, lds, c->stream>>>(a);
  else
    k_lnl_quad<2><<<grid, block, lds, c->stream>>>(a);
  HIPCHK(c, hipGetLastError(), "k_lnl_quad launch");
  const int64_t n = (int64_t)G * R_pad;
  k_lnl_reduce<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream>>>(
      s.q.as<double>(), s.ld.as<double>(), n_psr, G, R_pad, n, s.d.as<double>());
  HIPCHK(c, hipGetLastError(), "k_lnl_reduce launch");
  return FPTA_OK;
}

// The wanted results of lnl_launch on that block, unpadded
static int lnl_results(fpta_ctx* c, const Block& b, const LnlSlot& s, const LnlState& st, double* dlnl, double* q_psr,
                       double* X) {
  int rc;
  if (dlnl && (rc = fit_download(c, s.d, st.G, b.R, st.rpad, dlnl))) return rc;
  if (q_psr && (rc = fit_download(c, s.q, (int64_t)b.n_psr * st.G, b.R, st.rpad, q_psr))) return rc;
  if (X && (rc = fit_download(c, s.x.coef, (int64_t)b.n_psr * st.K, b.R, st.rpad, X))) return rc;
  return FPTA_OK;
}

}  // namespace capi

using namespace capi;

extern "C" int fpta_batch_set_lnl(fpta_ctx* c, int32_t n_comp, const int32_t* n_modes, const double* f,
                                  int32_t f_is_common, const double* idx, const double* freqf, const double* phi,
                                  const uint8_t* mask, int32_t target, int32_t n_col, const double* M,
                                  const int32_t* ncol_psr, const double* weights, double rcond, int32_t n_grid,
                                  const double* phi_grid, int32_t* rank_out, double* ld_out) {
  if (!c) return fail(nullptr, FPTA_EINVAL, "null ctx");
  const Layout& L = c->batch;
  if (L.P <= 0) return fail(c, FPTA_ESTATE, "set_lnl: set_toas first");
  if (n_comp == 0) {
    c->lnl_st.clear();
    if (rank_out) std::fill(rank_out, rank_out + L.P, 0);
    return FPTA_OK;
  }
  // everything is validated and the tables built here, before anything is uploaded
  std::string why;
  fpta_lnl::Plan plan;
  const fpta_os::Spec sp =
      fpta_os::make_spec(fpta_fit::make_spec(n_comp, n_modes, f, f_is_common, idx, freqf), phi, mask, target);
  const int made = fpta_lnl::make_plan(L.P, L.h_offs.data(), L.h_toas.data(), L.h_nu.data(), sp, n_col, M, ncol_psr,
                                       weights, rcond, n_grid, phi_grid, plan, why);
  if (made) return fail(c, made == 2 ? FPTA_ENOMEM : FPTA_EINVAL, "set_lnl: " + why);
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  c->lnl_st.clear();
  // a grid with the previous tables may still read them
  HIPCHK(c, hipStreamSynchronize(c->stream), "set_lnl sync");
  int rc;
  if ((rc = lnl_upload(c, plan, L.P, L.h_offs.data(), c->lnl))) return rc;
  c->lnl_st = LnlState{true, plan.K, plan.N, plan.G};
  if (rank_out) std::copy(plan.rank.begin(), plan.rank.end(), rank_out);
  if (ld_out) std::copy(plan.ld.begin(), plan.ld.end(), ld_out);
  return FPTA_OK;
}

extern "C" int fpta_batch_lnl_info(fpta_ctx* c, int64_t* info) {
  if (!c || !info) return fail(c, FPTA_EINVAL, "lnl_info: bad arguments");
  const LnlState& st = c->lnl_st;  // all zero while no grid is set
  const int64_t v[4] = {st.K, st.N, st.G, st.R};
  std::copy(v, v + 4, info);
  return FPTA_OK;
}

extern "C" int fpta_batch_lnl(fpta_ctx* c, double* dlnl, double* q_psr, double* X) {
  Block b;
  int rc;
  if ((rc = block_check(c, "lnl", false, b))) return rc;
  LnlState& st = c->lnl_st;
  if (!st.set) return fail(c, FPTA_ESTATE, "lnl: no likelihood grid is set (set_lnl first)");
  if ((rc = block_open(c, false))) return rc;
  st.R = 0;
  if ((rc = lnl_launch(c, b, c->lnl, st))) return rc;
  st.R = b.R;
  return lnl_results(c, b, c->lnl, st, dlnl, q_psr, X);
}

extern "C" int fpta_lnl_grid(fpta_ctx* c, int32_t n_psr, const int64_t* offs, const double* toas, const double* nu,
                             int32_t n_comp, const int32_t* n_modes, const double* f, int32_t f_is_common,
                             const double* idx, const double* freqf, const double* phi, const uint8_t* mask,
                             int32_t target, int32_t n_col, const double* M, const int32_t* ncol_psr,
                             const double* weights, double rcond, int32_t n_grid, const double* phi_grid,
                             int32_t n_vec, const double* res, double* dlnl, double* q_psr, double* X,
                             int32_t* rank_out, double* ld_out, double* U_out) {
  const OneShot one{c, "lnl_grid", n_psr, offs, n_vec, res};
  int rc;
  if ((rc = one.check())) return rc;
  std::string why;
  fpta_lnl::Plan plan;
  const fpta_os::Spec sp =
      fpta_os::make_spec(fpta_fit::make_spec(n_comp, n_modes, f, f_is_common, idx, freqf), phi, mask, target);
  const int made = fpta_lnl::make_plan(n_psr, offs, toas, nu, sp, n_col, M, ncol_psr, weights, rcond, n_grid, phi_grid,
                                       plan, why, U_out);
  if ((rc = one.planned(made, why))) return rc;
  if (rank_out) std::copy(plan.rank.begin(), plan.rank.end(), rank_out);
  if (ld_out) std::copy(plan.ld.begin(), plan.ld.end(), ld_out);
  if (n_vec == 0) return FPTA_OK;
  if (n_psr == 0 || one.n_toa() == 0) {  // nothing to launch: every X and q is zero and so is every log-determinant
    if (dlnl) std::fill(dlnl, dlnl + (int64_t)plan.G * n_vec, 0.0);
    if (q_psr) std::fill(q_psr, q_psr + (int64_t)n_psr * plan.G * n_vec, 0.0);
    if (X) std::fill(X, X + (int64_t)n_psr * plan.K * n_vec, 0.0);
    return FPTA_OK;
  }
  Block b;
  if ((rc = one.upload(b))) return rc;
  if ((rc = lnl_upload(c, plan, n_psr, offs, c->lnl1))) return rc;
  LnlState st{true, plan.K, plan.N, plan.G};
  if ((rc = lnl_launch(c, b, c->lnl1, st))) return rc;
  if ((rc = lnl_results(c, b, c->lnl1, st, dlnl, q_psr, X))) return rc;
  return one.done();
}
