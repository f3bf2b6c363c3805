// Optimal statistic (fpta_batch_set_os, fpta_batch_os_info, fpta_batch_os, fpta_os_statistic): per realization the
// noise-weighted cross-correlation of every pulsar pair against J pair-weight matrices. The definition is in
// include/fakepta_amd.h; the per-pulsar operator B_p = F_p^T P_p^-1 and the pair normalisations are os_host.h's.
//
//   stage 1  X = B_p r of every realization: k_fit_apply (fit.hip) on this file's operator slot and coefficient buffer
//            [P][K][R_pad]. The same instances as the Fourier fit, whose own slot is not touched.
//   stage 2  k_os_pairs<JC>: Q_mode[j][m][r] = phi_hat_m sum_{a > b} G_j[a][b] (X_a,cos X_b,cos + X_a,sin X_b,sin). A
//            workgroup of 4 waves owns 16 realizations of one mode and JC = 1, 2, 4 or 8 of the J matrices (the smallest
//            that holds J, else slices of 8) and walks every lower 16 x 16 tile pair of pulsars. Per tile pair it stages
//            the two X tiles [16 realizations][cos, sin][16 pulsars] and the JC G tiles (a <= b, pulsars past P and
//            matrices past J as zeros) in LDS, from registers that were loaded during the previous pair's products; a
//            wave then takes 4 realizations: one v_mfma_f64_16x16x4_f64 per realization makes the 256 pair products of
//            the mode (k = cos, sin, 0, 0), and the lane contracts its four pairs (row (lane >> 4) + 4 q, column lane &
//            15) with its four G values of each matrix. The pair products are made once and used for all JC matrices.
//            Lane partials are kept over the tile pairs and summed over the 64 lanes by a butterfly at the end: a fixed
//            order, no atomics, nothing shared between realizations, so a realization's Q is the same whatever R, its
//            position and its neighbours; a matrix's sums are the same operations in every instance.
//            k_os_reduce: Q[j][r] = sum_m Q_mode[j][m][r] in mode order.
// Padding realizations have X = 0 (the cleared buffer) and give exact zeros; they are not downloaded.
#include "capi_host.h"
#include "os_host.h"
#include "device_common.h"

namespace __attribute__((visibility("hidden"))) capi {

constexpr int kOsReal = 16;   // realizations of a workgroup
constexpr int kOsWaves = 4;   // waves of a workgroup
constexpr int kOsRW = kOsReal / kOsWaves;  // realizations of a wave
constexpr int kOsJ = 8;       // pair-weight matrices of a workgroup, at most
// (kOsRpad, k_fit_apply's realization padding, a multiple of kOsReal: capi_host.h)
static_assert(kOsRpad % kOsReal == 0 && kOsReal == 16 && kOsWaves * 64 == 256,
              "k_os_pairs stages 16 x 16 tiles with 256 threads and never reads past the padded realizations");

struct OsArgs {
  const double* X;    // [P][K][R_pad], K = 2 N: the cosine rows, then the sine rows
  const double* phi;  // [N] the template
  const double* G;    // [J][P][P] symmetric
  double* Qm;         // [J][N][R_pad]
  int32_t P, N, R_pad, J, n_tile;
};

// grid: (R_pad / 16, N, ceil(J / JC)); JC = 1, 2, 4, 8 matrices per workgroup (the smallest that holds J, else 8)
template <int JC>
__global__ __launch_bounds__(64 * kOsWaves) void k_os_pairs(OsArgs a) {
  __shared__ double sX[2][kOsReal][2][16];  // [row tile, column tile][realization][cos, sin][pulsar]
  __shared__ double sG[JC][4][64];          // [matrix][accumulator register][lane]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lg = lane >> 4;
  const int r0 = (int)blockIdx.x * kOsReal, m = (int)blockIdx.y, j0 = (int)blockIdx.z * JC;
  const int K = 2 * a.N;
  const int s_rr = tid & 15, s_pi = tid >> 4;  // the X element this thread stages: realization, pulsar of the tile
  FPTA_DCHECK(r0 + kOsReal <= a.R_pad, "k_os_pairs realization", r0 + kOsReal, a.R_pad + 1);
  double part[JC][kOsRW];
#pragma unroll
  for (int jj = 0; jj < JC; ++jj)
#pragma unroll
    for (int rr = 0; rr < kOsRW; ++rr) part[jj][rr] = 0.0;

  // this thread's share of a tile pair's operands: X of (row tile, column tile) x (cos, sin), and one G value per matrix
  // (accumulator register q = wave of lane `lane`; a <= b, pulsars past P and matrices past J: zero)
  auto fetch = [&](int ta, int tb, double (&xv)[4], double (&gv)[JC]) {
#pragma unroll
    for (int tile = 0; tile < 2; ++tile) {
      const int p = (tile ? tb : ta) * 16 + s_pi;
#pragma unroll
      for (int cs = 0; cs < 2; ++cs) {
        double v = 0.0;
        if (p < a.P) v = a.X[((int64_t)p * K + cs * a.N + m) * a.R_pad + r0 + s_rr];
        xv[2 * tile + cs] = v;
      }
    }
    const int pa = ta * 16 + lg + 4 * wave, pb = tb * 16 + lr;
    const bool in = pa < a.P && pb < pa;  // the strict lower triangle: a > b
#pragma unroll
    for (int jj = 0; jj < JC; ++jj) {
      double v = 0.0;
      if (in && j0 + jj < a.J) v = a.G[((int64_t)(j0 + jj) * a.P + pa) * a.P + pb];
      gv[jj] = v;
    }
  };

  double xv[4], gv[JC];
  fetch(0, 0, xv, gv);
  const int n_pairs = a.n_tile * (a.n_tile + 1) / 2;
  for (int t = 0, ta = 0, tb = 0; t < n_pairs; ++t) {
    __syncthreads();  // the previous tile pair's reads are done
#pragma unroll
    for (int tile = 0; tile < 2; ++tile)
#pragma unroll
      for (int cs = 0; cs < 2; ++cs) sX[tile][s_rr][cs][s_pi] = xv[2 * tile + cs];
#pragma unroll
    for (int jj = 0; jj < JC; ++jj) sG[jj][wave][lane] = gv[jj];
    __syncthreads();
    if (++tb > ta) {  // the next tile pair, row by row of the lower triangle
      ++ta;
      tb = 0;
    }
    if (t + 1 < n_pairs) fetch(ta, tb, xv, gv);  // in flight during this pair's products
    d4 acc[kOsRW];
#pragma unroll
    for (int rr = 0; rr < kOsRW; ++rr) {
      const int r = wave * kOsRW + rr;
      const double av = lg < 2 ? sX[0][r][lg & 1][lr] : 0.0, bv = lg < 2 ? sX[1][r][lg & 1][lr] : 0.0;
      acc[rr] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, d4{0.0, 0.0, 0.0, 0.0}, 0, 0, 0);
    }
#pragma unroll
    for (int jj = 0; jj < JC; ++jj) {
      const double g0 = sG[jj][0][lane], g1 = sG[jj][1][lane], g2 = sG[jj][2][lane], g3 = sG[jj][3][lane];
#pragma unroll
      for (int rr = 0; rr < kOsRW; ++rr) {
        double s = part[jj][rr];
        s = fma(acc[rr][0], g0, s);
        s = fma(acc[rr][1], g1, s);
        s = fma(acc[rr][2], g2, s);
        s = fma(acc[rr][3], g3, s);
        part[jj][rr] = s;
      }
    }
  }

  const double ph = a.phi[m];
#pragma unroll
  for (int jj = 0; jj < JC; ++jj)
#pragma unroll
    for (int rr = 0; rr < kOsRW; ++rr) {
      double s = part[jj][rr];
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
      if (lane == 0 && j0 + jj < a.J)
        a.Qm[((int64_t)(j0 + jj) * a.N + m) * a.R_pad + r0 + wave * kOsRW + rr] = ph * s;
    }
}

// Q[j][r] = sum_m Qm[j][m][r], in mode order; one thread per (j, r)
__global__ __launch_bounds__(256) void k_os_reduce(const double* __restrict__ Qm, int32_t N, int32_t R_pad, int64_t n,
                                                    double* __restrict__ Q) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const int64_t j = e / R_pad, r = e - j * R_pad;
  double s = 0.0;
  for (int32_t m = 0; m < N; ++m) s += Qm[(j * N + m) * R_pad + r];
  Q[e] = s;
}

// Device copies of a plan's tables, the template and the matrices, and N_ab (the sky scrambles' denominators)
int os_upload(fpta_ctx* c, const fpta_os::Plan& plan, int32_t n_psr, const int64_t* offs, const double* phi_hat,
                     int32_t n_g, const double* G, OsSlot& s) {
  int rc;
  if ((rc = fit_upload(c, "os", s.x, plan.K, plan.B, n_psr, offs, plan.rows))) return rc;
  if ((rc = upload(c, s.phi, phi_hat, sizeof(double) * (size_t)plan.N, "os template"))) return rc;
  if ((rc = upload(c, s.g, G, sizeof(double) * (size_t)n_g * (size_t)n_psr * (size_t)n_psr, "os pair weights")))
    return rc;
  s.h_nab = plan.Nab;
  if ((rc = upload(c, s.nab, plan.Nab.data(), sizeof(double) * plan.Nab.size(), "os pair norms"))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream), "os upload sync");
  return FPTA_OK;
}

// Both stages on a block of st.K columns and st.J matrices; one FPTA_K_DENSE entry. The results stay in the slot, padded
// to st.rpad realizations: X [P][K][rpad], Q_mode [J][N][rpad], Q [J][rpad].
static int os_launch(fpta_ctx* c, const Block& b, OsSlot& s, OsState& st) {
  if ((st.J + kOsJ - 1) / kOsJ > 65535 || st.K / 2 > 65535)  // refused before the timer entry opens
    return fail(c, FPTA_EINVAL, "os: too many pair-weight matrices or modes");
  KTimer kt(c, FPTA_K_DENSE);
  return os_launch_unbooked(c, b, s, st);
}

// The same without the timer entry (os_scramble.hip's spans its own kernels too)
int os_launch_unbooked(fpta_ctx* c, const Block& b, OsSlot& s, OsState& st) {
  const int32_t R = b.R, n_psr = b.n_psr, K = st.K, J = st.J, N = K / 2;
  const int32_t R_pad = st.rpad = (R + kOsRpad - 1) / kOsRpad * kOsRpad;
  const size_t b_x = sizeof(double) * (size_t)n_psr * (size_t)K * (size_t)R_pad;
  const size_t b_qm = sizeof(double) * (size_t)J * (size_t)N * (size_t)R_pad, b_q = sizeof(double) * (size_t)J * R_pad;
  if (s.x.coef.ensure(b_x) != hipSuccess || s.qm.ensure(b_qm) != hipSuccess || s.q.ensure(b_q) != hipSuccess)
    return fail(c, FPTA_ENOMEM, "os: no device memory for " + std::to_string(b_x + b_qm + b_q) + " bytes of results");
  if ((J + kOsJ - 1) / kOsJ > 65535 || N > 65535)
    return fail(c, FPTA_EINVAL, "os: too many pair-weight matrices or modes");
  int32_t rp = 0;
  int rc = fit_launch_unbooked(c, b, K, s.x, rp);
  if (rc) return rc;
  if (rp != R_pad) return fail(c, FPTA_EINVAL, "os: k_fit_apply's realization padding changed");
  if (J == 0 || R == 0) return FPTA_OK;
  return os_pairs_launch(c, s.x.coef.as<double>(), s.phi.as<double>(), s.g.as<double>(), s.qm.as<double>(),
                         s.q.as<double>(), n_psr, N, R_pad, J);
}

// Stage 2 on any coefficient buffer (os_launch, and os_spectra.hip on the coefficients of its solve)
int os_pairs_launch(fpta_ctx* c, const double* X, const double* phi, const double* G, double* qm, double* q,
                    int32_t n_psr, int32_t N, int32_t R_pad, int32_t J) {
  const int jc = J <= 1 ? 1 : J <= 2 ? 2 : J <= 4 ? 4 : kOsJ;  // matrices per workgroup
  const int64_t n_jc = (J + jc - 1) / jc;
  if (n_jc > 65535 || N > 65535) return fail(c, FPTA_EINVAL, "os: too many pair-weight matrices or modes");
  if (R_pad % kOsRpad)
    return fail(c, FPTA_EINVAL, "os: the coefficients' realization padding is no multiple of " + std::to_string(kOsRpad));
  OsArgs a;
  a.X = X;
  a.phi = phi;
  a.G = G;
  a.Qm = qm;
  a.P = n_psr;
  a.N = N;
  a.R_pad = R_pad;
  a.J = J;
  a.n_tile = (n_psr + 15) / 16;
  const dim3 grid((unsigned)(R_pad / kOsReal), (unsigned)N, (unsigned)n_jc), block(64 * kOsWaves);
  if (jc == 1)
    k_os_pairs<1><<<grid, block, 0, c->stream>>>(a);
  else if (jc == 2)
    k_os_pairs<2><<<grid, block, 0, c->stream>>>(a);
  else if (jc == 4)
    k_os_pairs<4><<<grid, block, 0, c->stream>>>(a);
  else
    k_os_pairs<kOsJ><<<grid, block, 0, c->stream>>>(a);
  HIPCHK(c, hipGetLastError(), "k_os_pairs launch");
  const int64_t n = (int64_t)J * R_pad;
  k_os_reduce<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream>>>(qm, N, R_pad, n, q);
  HIPCHK(c, hipGetLastError(), "k_os_reduce launch");
  return FPTA_OK;
}

// The wanted results of os_launch on that block, unpadded
int os_results(fpta_ctx* c, const Block& b, const OsSlot& s, const OsState& st, double* Q, double* Q_mode,
                      double* X) {
  int rc;
  if (Q && st.J > 0 && (rc = fit_download(c, s.q, st.J, b.R, st.rpad, Q))) return rc;
  if (Q_mode && st.J > 0 && (rc = fit_download(c, s.qm, (int64_t)st.J * st.N, b.R, st.rpad, Q_mode))) return rc;
  if (X && (rc = fit_download(c, s.x.coef, (int64_t)b.n_psr * st.K, b.R, st.rpad, X))) return rc;
  return FPTA_OK;
}

}  // namespace capi

using namespace capi;

extern "C" int fpta_batch_set_os(fpta_ctx* c, int32_t n_comp, const int32_t* n_modes, const double* f,
                                 int32_t f_is_common, const double* idx, const double* freqf, const double* phi,
                                 const uint8_t* mask, int32_t target, const double* phi_hat, int32_t n_col,
                                 const double* M, const int32_t* ncol_psr, const double* weights, double rcond,
                                 int32_t n_g, const double* G, int32_t* rank_out, double* nab_out) {
  if (!c) return fail(nullptr, FPTA_EINVAL, "null ctx");
  const Layout& L = c->batch;
  if (L.P <= 0) return fail(c, FPTA_ESTATE, "set_os: set_toas first");
  if (n_comp == 0) {
    c->os_st.clear();
    c->scr_st.clear();
    if (rank_out) std::fill(rank_out, rank_out + L.P, 0);
    return FPTA_OK;
  }
  // everything is validated and the operators built here, before anything is uploaded
  std::string why;
  fpta_os::Plan plan;
  const fpta_os::Spec sp = fpta_os::make_spec(fpta_fit::make_spec(n_comp, n_modes, f, f_is_common, idx, freqf), phi,
                                              mask, target, phi_hat);
  const int made = fpta_os::make_plan(L.P, L.h_offs.data(), L.h_toas.data(), L.h_nu.data(), sp, n_col, M, ncol_psr,
                                      weights, rcond, n_g, G, plan, why);
  if (made) return fail(c, made == 2 ? FPTA_ENOMEM : FPTA_EINVAL, "set_os: " + why);
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  c->os_st.clear();
  c->scr_st.clear();  // the scrambles' norms and matches were this statistic's
  // a statistic with the previous operator may still read the tables
  HIPCHK(c, hipStreamSynchronize(c->stream), "set_os sync");
  int rc;
  if ((rc = os_upload(c, plan, L.P, L.h_offs.data(), phi_hat, n_g, G, c->os))) return rc;
  c->os_st = OsState{true, plan.K, plan.N, n_g};
  if (rank_out) std::copy(plan.rank.begin(), plan.rank.end(), rank_out);
  if (nab_out) std::copy(plan.Nab.begin(), plan.Nab.end(), nab_out);
  return FPTA_OK;
}

extern "C" int fpta_batch_os_info(fpta_ctx* c, int64_t* info) {
  if (!c || !info) return fail(c, FPTA_EINVAL, "os_info: bad arguments");
  const OsState& st = c->os_st;  // all zero while no statistic is set
  const int64_t v[4] = {st.K, st.N, st.J, st.R};
  std::copy(v, v + 4, info);
  return FPTA_OK;
}

extern "C" int fpta_batch_os(fpta_ctx* c, double* Q, double* Q_mode, double* X) {
  Block b;
  int rc;
  if ((rc = block_check(c, "os", false, b))) return rc;
  OsState& st = c->os_st;
  if (!st.set) return fail(c, FPTA_ESTATE, "os: no optimal statistic is set (set_os first)");
  if ((rc = block_open(c, false))) return rc;
  st.R = 0;
  if ((rc = os_launch(c, b, c->os, st))) return rc;
  st.R = b.R;
  return os_results(c, b, c->os, st, Q, Q_mode, X);
}

extern "C" int fpta_os_statistic(fpta_ctx* c, int32_t n_psr, const int64_t* offs, const double* toas, const double* nu,
                                 int32_t n_comp, const int32_t* n_modes, const double* f, int32_t f_is_common,
                                 const double* idx, const double* freqf, const double* phi, const uint8_t* mask,
                                 int32_t target, const double* phi_hat, int32_t n_col, const double* M,
                                 const int32_t* ncol_psr, const double* weights, double rcond, int32_t n_g,
                                 const double* G, int32_t n_vec, const double* res, double* Q, double* Q_mode,
                                 double* X, int32_t* rank_out, double* nab_out) {
  const OneShot one{c, "os_statistic", n_psr, offs, n_vec, res};
  int rc;
  if ((rc = one.check())) return rc;
  std::string why;
  fpta_os::Plan plan;
  const fpta_os::Spec sp = fpta_os::make_spec(fpta_fit::make_spec(n_comp, n_modes, f, f_is_common, idx, freqf), phi,
                                              mask, target, phi_hat);
  const int made = fpta_os::make_plan(n_psr, offs, toas, nu, sp, n_col, M, ncol_psr, weights, rcond, n_g, G, plan, why);
  if ((rc = one.planned(made, why))) return rc;
  if (rank_out) std::copy(plan.rank.begin(), plan.rank.end(), rank_out);
  if (nab_out) std::copy(plan.Nab.begin(), plan.Nab.end(), nab_out);
  if (n_vec == 0) return FPTA_OK;
  if (n_psr == 0 || one.n_toa() == 0) {  // nothing to launch: every X and every Q is zero
    if (Q) std::fill(Q, Q + (int64_t)n_g * n_vec, 0.0);
    if (Q_mode) std::fill(Q_mode, Q_mode + (int64_t)n_g * plan.N * n_vec, 0.0);
    if (X) std::fill(X, X + (int64_t)n_psr * plan.K * n_vec, 0.0);
    return FPTA_OK;
  }
  Block b;
  if ((rc = one.upload(b))) return rc;
  if ((rc = os_upload(c, plan, n_psr, offs, phi_hat, n_g, G, c->os1))) return rc;
  OsState st{true, plan.K, plan.N, n_g};
  if ((rc = os_launch(c, b, c->os1, st))) return rc;
  if ((rc = os_results(c, b, c->os1, st, Q, Q_mode, X))) return rc;
  return one.done();
}
