// Correlated likelihood grid (fpta_batch_set_clnl, fpta_batch_clnl_info, fpta_batch_clnl, fpta_clnl_grid): per
// realization, ORF and grid point dlnL[o][g][r] = (|L_og^-1 D_g V_o[:, r]|^2 - ld_og) / 2 with C_og = I + D_g T_o D_g =
// L_og L_og^T. The definition is in include/fakepta_amd.h; the operator B_p, T_o and s_g are clnl_host.h's.
//
//   set time  k_clnl_fill writes C_og = I + D_g T_o D_g for every grid point of an ORF (the padding rows and columns
//             are the identity's), dense.hip's blocked Cholesky factors each in place (dense_cholesky_at),
//             k_clnl_logdet sums ld_og = 2 sum_i ln L_ii in index order. The factors stay on the device: nothing is
//             factored per block.
//   stage 1   X = B_p r of every realization: k_fit_apply (fit.hip) on this file's operator slot.
//   stage 2   k_clnl_mix: V_o = (A_o^T (x) I) X, per mode l the product [P x P]^T [P x R] on v_mfma_f64_16x16x4_f64; a
//             wave owns 16 output pulsars x 16 realizations and runs the k-steps over the pulsars in order.
//   stage 3   k_clnl_solve: the forward substitution L Y = D V with 64 right-hand sides per workgroup (4 waves),
//             left-looking and blocked by 64 rows. Per block row b the four waves form sum_{j < b} L_bj Y_j as a 64 x
//             64 tile of 2 x 2 MFMA fragments each, L read row-major from the cache (a lane's four k-steps are one
//             32-byte run: k-step s of lane group lg is column 16 k + 4 lg + s, for A and B alike) and Y_j read back
//             from the workgroup's own tile in global memory, 32 columns a step with the next step's loads issued
//             first; the right-hand side s V - sum goes to LDS, and wave 0 solves the diagonal block from LDS with one
//             right-hand side per lane (right-looking, the row in registers), adds the squares in row order to the
//             lane's q and writes the block's Y. (tile, grid point, ORF) are the grid dimensions of one launch.
//             No atomics, a fixed order, nothing shared between realizations, grid points or ORFs: a column's bits
//             depend on nothing but its own V.
//   k_clnl_reduce: dlnL = (q - ld) / 2, one thread per (o, g, r).
// Every buffer the kernels read is padded to the tile edges they read to: n_pad = n rounded up to 64, vld = R_pad
// rounded up to 64. Padding rows have s = 0 and identity rows of L: Y = 0 there; padding realizations have V = 0.
#include "capi_host.h"
#include "clnl_host.h"
#include "device_common.h"

namespace __attribute__((visibility("hidden"))) capi {

// C[g][i][j] = (i == j) + s_g[i] T[i][j] s_g[j] on the padded extent; grid (n_pad^2 / 256, G)
__global__ __launch_bounds__(256) void k_clnl_fill(const double* __restrict__ T, const double* __restrict__ s,
                                                    int64_t n_pad, double* __restrict__ C) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, g = blockIdx.y;
  if (e >= n_pad * n_pad) return;
  const int64_t i = e / n_pad, j = e - i * n_pad;
  const double* sg = s + g * n_pad;
  C[g * n_pad * n_pad + e] = (i == j ? 1.0 : 0.0) + sg[i] * T[e] * sg[j];
}

// ld[m] = 2 sum_i ln L_m[i][i] over the n leading rows in index order; one workgroup per matrix
__global__ __launch_bounds__(256) void k_clnl_logdet(const double* __restrict__ L, int64_t n, int64_t n_pad,
                                                      double* __restrict__ ld) {
  __shared__ double part[256];
  const double* Lm = L + (int64_t)blockIdx.x * n_pad * n_pad;
  double acc = 0.0;
  for (int64_t i0 = 0; i0 < n; i0 += 256) {
    const int64_t i = i0 + threadIdx.x;
    part[threadIdx.x] = i < n ? log(Lm[i * (n_pad + 1)]) : 0.0;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int cnt = (int)min<int64_t>(256, n - i0);
      for (int t = 0; t < cnt; ++t) acc += part[t];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) ld[blockIdx.x] = 2.0 * acc;
}

// V[o][(j, l)][r] = sum_p A_o[p][j] X[p][l][r]; grid (vld / 64, ceil(P / 16), K n_orf), wave w of the workgroup takes
// the realizations 64 blockIdx.x + 16 w ..
__global__ __launch_bounds__(256) void k_clnl_mix(const double* __restrict__ A, const double* __restrict__ X, int32_t P,
                                                   int32_t K, int32_t R_pad, int64_t n_pad, int64_t vld,
                                                   double* __restrict__ V) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 15, lg = lane >> 4;
  const int r = (int)blockIdx.x * 64 + 16 * wave + lr, j0 = (int)blockIdx.y * 16;
  const int o = (int)blockIdx.z / K, l = (int)blockIdx.z - o * K;
  const double* Ao = A + (int64_t)o * P * P;
  const bool ja = j0 + lr < P, rb = r < R_pad;
  d4 acc = d4{0.0, 0.0, 0.0, 0.0};
  for (int p0 = 0; p0 < P; p0 += 4) {
    const int p = p0 + lg;
    const double a = p < P && ja ? Ao[(int64_t)p * P + j0 + lr] : 0.0;
    const double b = p < P && rb ? X[((int64_t)p * K + l) * R_pad + r] : 0.0;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
  }
  double* Vo = V + (int64_t)o * n_pad * vld;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = j0 + lg + 4 * q;
    if (j < P && rb) Vo[((int64_t)j * K + l) * vld + r] = acc[q];
  }
}

struct ClnlArgs {
  const double* L;  // [n_orf][G][n_pad][n_pad]
  const double* s;  // [G][n_pad]
  const double* V;  // [n_orf][n_pad][vld]
  double* Y;        // [n_orf][G][vld / 64][n_pad][64]
  double* q;        // [n_orf][G][R_pad]
  int64_t n_pad, vld;
  int32_t G, R_pad;
};

// grid: (vld / 64 tiles of realizations, G, n_orf)
__global__ __launch_bounds__(256) void k_clnl_solve(ClnlArgs a) {
  __shared__ double W[64][64];   // the block row's right-hand sides [row][realization]
  __shared__ double Ld[64][64];  // the diagonal block, its diagonal as reciprocals
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lg = lane >> 4;
  const int wi = wave >> 1, wj = wave & 1;
  const int64_t tile = blockIdx.x, g = blockIdx.y, o = blockIdx.z, n_pad = a.n_pad, vld = a.vld;
  const int64_t m = o * a.G + g;
  const double* __restrict__ L = a.L + m * n_pad * n_pad;
  const double* __restrict__ sg = a.s + g * n_pad;
  const double* __restrict__ V = a.V + o * n_pad * vld + tile * 64;
  double* Y = a.Y + (m * (int64_t)gridDim.x + tile) * n_pad * 64;
  double qsum = 0.0;
  for (int64_t r0 = 0; r0 < n_pad; r0 += 64) {
    for (int e = tid; e < 64 * 64; e += 256) {
      const int i = e >> 6, j = e & 63;
      const double v = L[(r0 + i) * n_pad + r0 + j];
      Ld[i][j] = i == j ? 1.0 / v : v;
    }
    d4 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y) acc[x][y] = d4{0.0, 0.0, 0.0, 0.0};
    // 32 columns a step, the next step's operands loaded before this step's 32 MFMAs: two steps of loads in flight
    const double* La = L + (r0 + 32 * wi + lr) * n_pad + 4 * lg;
    const double* Yb = Y + (int64_t)(4 * lg) * 64 + 32 * wj + lr;
    d4 ca[2][2];
    double cb[2][4][2];
    auto load = [&](int64_t k, d4(&A2)[2][2], double(&B2)[2][4][2]) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const double* pa = La + k + 16 * h;
        const double* pb = Yb + (k + 16 * h) * 64;
        A2[h][0] = *(const d4*)pa;
        A2[h][1] = *(const d4*)(pa + 16 * n_pad);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          B2[h][t][0] = pb[t * 64];
          B2[h][t][1] = pb[t * 64 + 16];
        }
      }
    };
    if (r0 > 0) load(0, ca, cb);
    for (int64_t k = 0; k < r0; k += 32) {
      d4 na[2][2];
      double nb[2][4][2];
      load(k + 32 < r0 ? k + 32 : k, na, nb);  // the last step loads its own operands again: in bounds, not used
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(ca[h][0][t], cb[h][t][0], acc[0][0], 0, 0, 0);
          acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(ca[h][0][t], cb[h][t][1], acc[0][1], 0, 0, 0);
          acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(ca[h][1][t], cb[h][t][0], acc[1][0], 0, 0, 0);
          acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(ca[h][1][t], cb[h][t][1], acc[1][1], 0, 0, 0);
        }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        ca[h][0] = na[h][0];
        ca[h][1] = na[h][1];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          cb[h][t][0] = nb[h][t][0];
          cb[h][t][1] = nb[h][t][1];
        }
      }
    }
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = 32 * wi + 16 * x + lg + 4 * q, col = 32 * wj + 16 * y + lr;
          W[row][col] = sg[r0 + row] * V[(r0 + row) * vld + col] - acc[x][y][q];
        }
    __syncthreads();
    if (wave == 0) {
      double x[64];
#pragma unroll
      for (int l = 0; l < 64; ++l) x[l] = W[l][lane];
#pragma unroll
      for (int l = 0; l < 64; ++l) {
        x[l] *= Ld[l][l];
#pragma unroll
        for (int j = l + 1; j < 64; ++j) x[j] = fma(-x[l], Ld[j][l], x[j]);
      }
#pragma unroll
      for (int l = 0; l < 64; ++l) {
        qsum = fma(x[l], x[l], qsum);
        Y[(r0 + l) * 64 + lane] = x[l];
      }
    }
    __syncthreads();
  }
  const int64_t r = tile * 64 + lane;
  if (wave == 0 && r < a.R_pad) a.q[m * a.R_pad + r] = qsum;
}

// dlnL[o][g][r] = (q[o][g][r] - ld[o][g]) / 2; one thread per entry
__global__ __launch_bounds__(256) void k_clnl_reduce(const double* __restrict__ q, const double* __restrict__ ld,
                                                      int32_t R_pad, int64_t n, double* __restrict__ d) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  d[e] = 0.5 * (q[e] - ld[e / R_pad]);
}

// Device copies of a plan's tables, then the factor and log-determinant of every (ORF, grid point). The cache is the
// large one (8 n_orf G n_pad^2 bytes). ld_out NULL or [n_orf][G]. who: the prefix of the messages.
static int clnl_setup(fpta_ctx* c, const std::string& who, const fpta_clnl::Plan& plan, int32_t n_psr,
                      const int64_t* offs, ClnlSlot& s, double* ld_out) {
  int rc;
  if ((rc = fit_upload(c, "clnl", s.x, plan.K, plan.B, n_psr, offs, plan.rows))) return rc;
  const int64_t n = plan.n, n_pad = plan.n_pad, G = plan.G, n_orf = plan.n_orf;
  if (ld_out) std::fill(ld_out, ld_out + n_orf * G, 0.0);
  if (n == 0) return FPTA_OK;
  const size_t b_mat = sizeof(double) * (size_t)(n_pad * n_pad), b_l = b_mat * (size_t)(n_orf * G);
  if (s.l.ensure(b_l) != hipSuccess || s.t.ensure(b_mat * (size_t)n_orf) != hipSuccess ||
      s.pt.ensure(sizeof(double) * 64 * (size_t)n_pad) != hipSuccess || s.info.ensure(sizeof(int)) != hipSuccess ||
      s.ld.ensure(sizeof(double) * (size_t)(n_orf * G)) != hipSuccess)
    return fail(c, FPTA_ENOMEM, who + ": no device memory for the cached factors of " + std::to_string(b_l) +
                                    " bytes (n_orf = " + std::to_string(n_orf) + ", G = " + std::to_string(G) +
                                    ", n_pad = " + std::to_string(n_pad) + ")");
  if ((rc = upload(c, s.a, plan.A.data(), sizeof(double) * plan.A.size(), "clnl ORF factors"))) return rc;
  if ((rc = upload(c, s.t, plan.T.data(), sizeof(double) * plan.T.size(), "clnl T"))) return rc;
  if ((rc = upload(c, s.s, plan.s.data(), sizeof(double) * plan.s.size(), "clnl scalings"))) return rc;
  const dim3 fgrid((unsigned)(n_pad * n_pad / 256), (unsigned)G);
  for (int64_t o = 0; o < n_orf; ++o) {
    KTimer kt(c, FPTA_K_DENSE);
    k_clnl_fill<<<fgrid, dim3(256), 0, c->stream>>>(s.t.as<double>() + o * n_pad * n_pad, s.s.as<double>(), n_pad,
                                                     s.l.as<double>() + o * G * n_pad * n_pad);
    HIPCHK(c, hipGetLastError(), "k_clnl_fill launch");
  }
  for (int64_t m = 0; m < n_orf * G; ++m) {
    int64_t pivot = -1;
    if ((rc = dense_cholesky_at(c, s.l.as<double>() + m * n_pad * n_pad, n_pad, n, s.pt.as<double>(), n_pad,
                                s.info.as<int>(), pivot)))
      return rc;
    if (pivot >= 0)
      return fail(c, FPTA_EINVAL, who + ": ORF " + std::to_string(m / G) + ", grid point " + std::to_string(m % G) +
                                      ": I + D T D is not positive definite (pivot " + std::to_string(pivot) + ")");
  }
  {
    KTimer kt(c, FPTA_K_DENSE);
    k_clnl_logdet<<<dim3((unsigned)(n_orf * G)), dim3(256), 0, c->stream>>>(s.l.as<double>(), n, n_pad,
                                                                            s.ld.as<double>());
    HIPCHK(c, hipGetLastError(), "k_clnl_logdet launch");
  }
  if (ld_out)
    HIPCHK(c, hipMemcpyAsync(ld_out, s.ld.p, sizeof(double) * (size_t)(n_orf * G), hipMemcpyDeviceToHost, c->stream),
           "clnl log-determinants");
  HIPCHK(c, hipStreamSynchronize(c->stream), "clnl setup sync");
  return FPTA_OK;
}

// All stages on a block; one FPTA_K_DENSE entry. The results stay in the slot: X [P][K][rpad], V [n_orf][n_pad][vld]
// (vld = rpad rounded up to 64), q and dlnL [n_orf][G][rpad].
static int clnl_launch(fpta_ctx* c, const Block& b, ClnlSlot& s, ClnlState& st) {
  const int32_t R = b.R, n_psr = b.n_psr, K = st.K, G = st.G, n_orf = st.n_orf;
  const int32_t R_pad = st.rpad = (R + 31) / 32 * 32;  // k_fit_apply's realization padding
  const int64_t n_pad = st.n_pad, vld = fpta_clnl::pad64(R_pad), n_out = (int64_t)n_orf * G * R_pad;
  const size_t b_x = sizeof(double) * (size_t)n_psr * (size_t)K * (size_t)R_pad;
  const size_t b_v = sizeof(double) * (size_t)(n_orf * n_pad * vld), b_y = b_v * (size_t)G;
  const size_t b_q = sizeof(double) * (size_t)n_out;
  if (s.x.coef.ensure(b_x) != hipSuccess || s.v.ensure(b_v) != hipSuccess || s.y.ensure(b_y) != hipSuccess ||
      s.q.ensure(b_q) != hipSuccess || s.d.ensure(b_q) != hipSuccess)
    return fail(c, FPTA_ENOMEM, "clnl: no device memory for " + std::to_string(b_x + b_v + b_y + 2 * b_q) +
                                    " bytes of results and work space (the substitution's Y, 8 n_orf G n_pad R, is " +
                                    std::to_string(b_y) + ")");
  KTimer kt(c, FPTA_K_DENSE);
  int32_t rp = 0;
  int rc = fit_launch_unbooked(c, b, K, s.x, rp);
  if (rc) return rc;
  if (rp != R_pad) return fail(c, FPTA_EINVAL, "clnl: k_fit_apply's realization padding changed");
  if (R == 0 || n_psr == 0 || st.n == 0) return FPTA_OK;
  HIPCHK(c, hipMemsetAsync(s.v.p, 0, b_v, c->stream), "clnl V memset");
  k_clnl_mix<<<dim3((unsigned)(vld / 64), (unsigned)((n_psr + 15) / 16), (unsigned)(K * n_orf)), dim3(256), 0,
               c->stream>>>(s.a.as<double>(), s.x.coef.as<double>(), n_psr, K, R_pad, n_pad, vld, s.v.as<double>());
  HIPCHK(c, hipGetLastError(), "k_clnl_mix launch");
  ClnlArgs a;
  a.L = s.l.as<double>();
  a.s = s.s.as<double>();
  a.V = s.v.as<double>();
  a.Y = s.y.as<double>();
  a.q = s.q.as<double>();
  a.n_pad = n_pad;
  a.vld = vld;
  a.G = G;
  a.R_pad = R_pad;
  k_clnl_solve<<<dim3((unsigned)(vld / 64), (unsigned)G, (unsigned)n_orf), dim3(256), 0, c->stream>>>(a);
  HIPCHK(c, hipGetLastError(), "k_clnl_solve launch");
  k_clnl_reduce<<<dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, c->stream>>>(
      s.q.as<double>(), s.ld.as<double>(), R_pad, n_out, s.d.as<double>());
  HIPCHK(c, hipGetLastError(), "k_clnl_reduce launch");
  return FPTA_OK;
}

// The wanted results of clnl_launch on that block, unpadded: dlnl, q [n_orf][G][R], V [n_orf][n][R], X [P][K][R]
static int clnl_results(fpta_ctx* c, const Block& b, const ClnlSlot& s, const ClnlState& st, double* dlnl, double* q,
                        double* V, double* X) {
  int rc;
  const int64_t og = (int64_t)st.n_orf * st.G;
  if (st.n == 0) {  // nothing was launched past stage 1
    if (dlnl) std::fill(dlnl, dlnl + og * b.R, 0.0);
    if (q) std::fill(q, q + og * b.R, 0.0);
  } else {
    if (dlnl && (rc = fit_download(c, s.d, og, b.R, st.rpad, dlnl))) return rc;
    if (q && (rc = fit_download(c, s.q, og, b.R, st.rpad, q))) return rc;
    const int32_t vld = (int32_t)fpta_clnl::pad64(st.rpad);
    if (V)
      for (int32_t o = 0; o < st.n_orf; ++o) {
        DevBuf view;  // rows of one ORF's V; not owned
        view.p = s.v.as<double>() + (int64_t)o * st.n_pad * vld;
        rc = fit_download(c, view, st.n, b.R, vld, V + (int64_t)o * st.n * b.R);
        view.p = nullptr;
        if (rc) return rc;
      }
  }
  if (X && (rc = fit_download(c, s.x.coef, (int64_t)b.n_psr * st.K, b.R, st.rpad, X))) return rc;
  return FPTA_OK;
}

static ClnlState clnl_state(const fpta_clnl::Plan& plan) {
  ClnlState st;
  st.set = true;
  st.K = plan.K;
  st.G = plan.G;
  st.n_orf = plan.n_orf;
  st.n = plan.n;
  st.n_pad = plan.n_pad;
  return st;
}

}  // namespace capi

using namespace capi;

extern "C" int fpta_batch_set_clnl(fpta_ctx* c, int32_t n_comp, const int32_t* n_modes, const double* f,
                                   int32_t f_is_common, const double* idx, const double* freqf, const double* phi,
                                   const uint8_t* mask, int32_t target, int32_t n_col, const double* M,
                                   const int32_t* ncol_psr, const double* weights, double rcond, int32_t n_grid,
                                   const double* phi_grid, int32_t n_orf, const double* A, int32_t* rank_out,
                                   double* ld_out) {
  if (!c) return fail(nullptr, FPTA_EINVAL, "null ctx");
  const Layout& L = c->batch;
  if (L.P <= 0) return fail(c, FPTA_ESTATE, "set_clnl: set_toas first");
  if (n_comp == 0) {
    c->clnl_st.clear();
    if (rank_out) std::fill(rank_out, rank_out + L.P, 0);
    return FPTA_OK;
  }
  // everything is validated and the host tables built here, before anything is uploaded
  std::string why;
  fpta_clnl::Plan plan;
  const fpta_os::Spec sp =
      fpta_os::make_spec(fpta_fit::make_spec(n_comp, n_modes, f, f_is_common, idx, freqf), phi, mask, target);
  const int made = fpta_clnl::make_plan(L.P, L.h_offs.data(), L.h_toas.data(), L.h_nu.data(), sp, n_col, M, ncol_psr,
                                        weights, rcond, n_grid, phi_grid, n_orf, A, plan, why);
  if (made) return fail(c, made == 2 ? FPTA_ENOMEM : FPTA_EINVAL, "set_clnl: " + why);
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  c->clnl_st.clear();
  // a grid with the previous tables may still read them
  HIPCHK(c, hipStreamSynchronize(c->stream), "set_clnl sync");
  int rc;
  if ((rc = clnl_setup(c, "set_clnl", plan, L.P, L.h_offs.data(), c->clnl, ld_out))) return rc;
  c->clnl_st = clnl_state(plan);
  if (rank_out) std::copy(plan.rank.begin(), plan.rank.end(), rank_out);
  return FPTA_OK;
}

extern "C" int fpta_batch_clnl_info(fpta_ctx* c, int64_t* info) {
  if (!c || !info) return fail(c, FPTA_EINVAL, "clnl_info: bad arguments");
  const ClnlState& st = c->clnl_st;  // all zero while no grid is set
  const int64_t v[4] = {st.K, st.G, st.n_orf, st.R};
  std::copy(v, v + 4, info);
  return FPTA_OK;
}

extern "C" int fpta_batch_clnl(fpta_ctx* c, double* dlnl, double* q, double* V, double* X) {
  Block b;
  int rc;
  if ((rc = block_check(c, "clnl", false, b))) return rc;
  ClnlState& st = c->clnl_st;
  if (!st.set) return fail(c, FPTA_ESTATE, "clnl: no correlated likelihood grid is set (set_clnl first)");
  if ((rc = block_open(c, false))) return rc;
  st.R = 0;
  if ((rc = clnl_launch(c, b, c->clnl, st))) return rc;
  st.R = b.R;
  return clnl_results(c, b, c->clnl, st, dlnl, q, V, X);
}

extern "C" int fpta_clnl_grid(fpta_ctx* c, int32_t n_psr, const int64_t* offs, const double* toas, const double* nu,
                              int32_t n_comp, const int32_t* n_modes, const double* f, int32_t f_is_common,
                              const double* idx, const double* freqf, const double* phi, const uint8_t* mask,
                              int32_t target, int32_t n_col, const double* M, const int32_t* ncol_psr,
                              const double* weights, double rcond, int32_t n_grid, const double* phi_grid,
                              int32_t n_orf, const double* A, int32_t n_vec, const double* res, double* dlnl,
                              double* q, double* V, double* X, int32_t* rank_out, double* ld_out, double* T_out) {
  const OneShot one{c, "clnl_grid", n_psr, offs, n_vec, res};
  int rc;
  if ((rc = one.check())) return rc;
  std::string why;
  fpta_clnl::Plan plan;
  const fpta_os::Spec sp =
      fpta_os::make_spec(fpta_fit::make_spec(n_comp, n_modes, f, f_is_common, idx, freqf), phi, mask, target);
  const int made = fpta_clnl::make_plan(n_psr, offs, toas, nu, sp, n_col, M, ncol_psr, weights, rcond, n_grid,
                                        phi_grid, n_orf, A, plan, why);
  if ((rc = one.planned(made, why))) return rc;
  if (rank_out) std::copy(plan.rank.begin(), plan.rank.end(), rank_out);
  if (T_out)
    for (int64_t o = 0; o < plan.n_orf; ++o)
      for (int64_t i = 0; i < plan.n; ++i)
        std::copy(plan.T.begin() + (o * plan.n_pad + i) * plan.n_pad,
                  plan.T.begin() + (o * plan.n_pad + i) * plan.n_pad + plan.n, T_out + (o * plan.n + i) * plan.n);
  const int64_t og = (int64_t)plan.n_orf * plan.G;
  if (n_vec == 0 && n_psr > 0 && one.n_toa() > 0) {  // the tables alone
    HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
    rc = clnl_setup(c, "clnl_grid", plan, n_psr, offs, c->clnl1, ld_out);  // ends with the stream idle
    for (DevBuf* buf : {&c->clnl1.l, &c->clnl1.t}) buf->release();
    return rc;
  }
  if (n_psr == 0 || one.n_toa() == 0) {  // nothing to launch: T = 0, so every X, V, q and ld is zero
    if (ld_out) std::fill(ld_out, ld_out + og, 0.0);
    if (dlnl) std::fill(dlnl, dlnl + og * n_vec, 0.0);
    if (q) std::fill(q, q + og * n_vec, 0.0);
    if (V) std::fill(V, V + (int64_t)plan.n_orf * plan.n * n_vec, 0.0);
    if (X) std::fill(X, X + (int64_t)n_psr * plan.K * n_vec, 0.0);
    return FPTA_OK;
  }
  Block b;
  if ((rc = one.upload(b))) return rc;
  if ((rc = clnl_setup(c, "clnl_grid", plan, n_psr, offs, c->clnl1, ld_out))) return rc;
  ClnlState st = clnl_state(plan);
  if ((rc = clnl_launch(c, b, c->clnl1, st))) return rc;
  if ((rc = clnl_results(c, b, c->clnl1, st, dlnl, q, V, X))) return rc;
  if ((rc = one.done())) return rc;
  // the stream is idle: a one-shot call keeps neither its factors nor the substitution's work space
  for (DevBuf* buf : {&c->clnl1.l, &c->clnl1.t, &c->clnl1.y, &c->clnl1.v}) buf->release();
  return FPTA_OK;
}
