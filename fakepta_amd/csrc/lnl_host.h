// Likelihood ratio of a common process on a spectrum grid (fpta_batch_set_lnl, fpta_batch_lnl, fpta_lnl_grid): input
// validation, the per-pulsar operator B_p = F_p^T P0_p^-1 with the target left out of the model, Z_p = B_p F_p, and per
// grid point the factor U_pg and the log-determinant ld_pg, on the host in plain C++ and long double. No HIP here:
// lnl.hip includes it for the tables its kernels read, and a stand-alone CPU program can include it alone
// (tests/test_lnl_host.py builds one under the address sanitizer). The definition is in include/fakepta_amd.h. The
// noise model, its validation and the operator are os_host.h's: build_operator with the target's phi set to 0 takes
// the projection form for every target column.
#pragma once
#include "os_host.h"

namespace fpta_lnl {

constexpr int32_t kMaxCoef = 256;   // Fourier columns of the target, K = 2 N
constexpr int32_t kMaxGrid = 4096;  // grid points
constexpr int32_t kPoolMax = 16;    // planner threads, at most
using fpta_fit::kTwoPi;
using fpta_os::Spec;  // phi_hat is not read here

// Everything the entry points refuse: what os_host.h's validate refuses (without a template and pair weights), K > 256
// and the grid phi_grid [n_grid][N] (finite, >= 0, 1 <= n_grid <= 4096).
inline bool validate(int64_t n_psr, const int64_t* offs, const double* toas, const double* nu, const Spec& sp,
                     int64_t n_col, const double* M, const int32_t* ncol_psr, const double* weights, int64_t n_grid,
                     const double* phi_grid, std::string& why) {
  const std::vector<double> ones((size_t)fpta_os::kMaxCoef / 2, 1.0);
  Spec s = sp;
  s.phi_hat = ones.data();
  if (!fpta_os::validate(n_psr, offs, toas, nu, s, n_col, M, ncol_psr, weights, 0, nullptr, why)) return false;
  const int32_t N = sp.comps.n_modes[sp.target];
  if (2 * N > kMaxCoef) {
    why = "target component " + std::to_string(sp.target) + ": " + std::to_string(2 * N) +
          " Fourier columns, more than " + std::to_string(kMaxCoef);
    return false;
  }
  if (n_grid < 1 || n_grid > kMaxGrid) {
    why = std::to_string(n_grid) + " grid points outside [1, " + std::to_string(kMaxGrid) + "]";
    return false;
  }
  if (!phi_grid) {
    why = "grid missing";
    return false;
  }
  for (int64_t g = 0; g < n_grid; ++g)
    for (int32_t k = 0; k < N; ++k) {
      const double v = phi_grid[g * N + k];
      if (!(v >= 0.0 && std::isfinite(v))) {
        why = "grid row " + std::to_string(g) + ", mode " + std::to_string(k) +
              ": prior variance is negative or not finite";
        return false;
      }
    }
  return true;
}

// Column k of the target on n TOAs, without the weights (os_host.h's column: (freqf / nu)^idx cos / sin, 0 off the mask)
inline void target_column(int64_t n, const double* t, const double* nu, const Spec& sp, const double* f,
                          const uint8_t* mask, int64_t mask_stride, int32_t k, long double* out) {
  const fpta_fit::Spec& cs = sp.comps;
  const int32_t c = sp.target, N = cs.n_modes[c];
  int32_t f0 = 0;
  for (int32_t i = 0; i < c; ++i) f0 += cs.n_modes[i];
  const long double fk = (long double)f[f0 + (k < N ? k : k - N)];
  const uint8_t* mk = mask ? mask + (int64_t)c * mask_stride : nullptr;
  for (int64_t i = 0; i < n; ++i) {
    const long double ch =
        cs.idx[c] == 0.0 ? 1.0L : std::pow((long double)cs.freqf[c] / (long double)nu[i], (long double)cs.idx[c]);
    const long double arg = kTwoPi * fk * (long double)t[i];
    out[i] = mk && !mk[i] ? 0.0L : ch * (k < N ? std::cos(arg) : std::sin(arg));
  }
}

// The device layout of one (pulsar, grid point)'s U: row groups of 16 rows, group j with the columns 0 .. 16 (j + 1) - 1
// (up to its diagonal block) as 2 (j + 1) blocks of 8 columns; a block is [64 lanes][2]: lane (lg = lane >> 4, lr =
// lane & 15) holds U[16 j + lr][8 q + 2 lg] and U[16 j + lr][8 q + 2 lg + 1], the A operands of its two k-steps. Rows
// and columns past K are zero.
inline int32_t groups_of(int32_t K) { return (K + 15) / 16; }
inline int64_t packed_size(int32_t K) { return (int64_t)128 * groups_of(K) * (groups_of(K) + 1); }
inline int64_t packed_index(int32_t row, int32_t col) {
  const int32_t j = row >> 4, lr = row & 15, q = col >> 3, lg = (col & 7) >> 1, e = col & 1;
  return ((int64_t)j * (j + 1) + q) * 128 + (int64_t)(lg * 16 + lr) * 2 + e;
}

// C = I + s Z s (s = sqrt(phi) per column, Z's lower triangle read), C = L L^T, U = L^-1 diag(s), ld = 2 sum ln L_ii,
// all in long double, sums in index order. U [K][K] row-major, lower triangular. Lw: scratch [K][K].
inline long double factor_point(int32_t K, const long double* Z, const long double* s, long double* Lw,
                                long double* U) {
  long double ld = 0.0L;
  for (int32_t i = 0; i < K; ++i) {
    for (int32_t j = 0; j <= i; ++j) {
      long double a = s[i] * Z[(int64_t)i * K + j] * s[j] + (i == j ? 1.0L : 0.0L);
      for (int32_t l = 0; l < j; ++l) a -= Lw[(int64_t)i * K + l] * Lw[(int64_t)j * K + l];
      Lw[(int64_t)i * K + j] = i == j ? std::sqrt(a) : a / Lw[(int64_t)j * K + j];
    }
    ld += std::log(Lw[(int64_t)i * K + i]);
  }
  for (int32_t j = 0; j < K; ++j) {
    for (int32_t i = 0; i < j; ++i) U[(int64_t)i * K + j] = 0.0L;
    if (s[j] == 0.0L) {
      for (int32_t i = j; i < K; ++i) U[(int64_t)i * K + j] = 0.0L;
      continue;
    }
    U[(int64_t)j * K + j] = s[j] / Lw[(int64_t)j * K + j];
    for (int32_t i = j + 1; i < K; ++i) {
      long double a = 0.0L;
      for (int32_t l = j; l < i; ++l) a += Lw[(int64_t)i * K + l] * U[(int64_t)l * K + j];
      U[(int64_t)i * K + j] = -a / Lw[(int64_t)i * K + i];
    }
  }
  return 2.0L * ld;
}

// Every pulsar's operator B_p (fp64, pulsar p's [K][n_p] at K offs[p] of B) and Z_p = B_p F_p (long double, from the
// unrounded B_p, [n_psr][K][K]) with the target left out of the base model; rows[p] = K for a pulsar with TOAs (else
// the entry is left alone: X = 0 and Z = 0), rank[p] the kept columns of M. The pulsars are independent and write
// disjoint parts; up to cap threads. True when one of them ran out of memory.
inline bool build_operators(int64_t n_psr, const int64_t* offs, const double* toas, const double* nu, const Spec& sp,
                            int64_t n_col, const double* M, const int32_t* ncol_psr, const double* weights,
                            double rcond, int64_t cap, double* B, int32_t* rows, int32_t* rank, long double* Zall) {
  const fpta_fit::Spec& cs = sp.comps;
  const int64_t n_toa = n_psr > 0 ? offs[n_psr] : 0, n_f = fpta_fit::modes_of(cs);
  const int32_t N = cs.n_modes[sp.target];
  const int64_t K = 2 * N;
  int32_t f0_t = 0;
  for (int32_t c = 0; c < sp.target; ++c) f0_t += cs.n_modes[c];
  const int64_t work_op = (2 * n_f) * (2 * n_f) * n_toa;
  return fpta_os::run_pool(n_psr, std::min<int64_t>({cap, work_op >> 24, n_psr}), [&](int64_t p) {
    const int64_t o = offs[p], n = offs[p + 1] - o;
    const int32_t m = ncol_psr ? ncol_psr[p] : (int32_t)n_col;
    if (n == 0) return;  // X = 0 and Z = 0
    rows[(size_t)p] = (int32_t)K;
    const double* f = cs.f + (cs.f_is_common ? 0 : p * n_f);
    std::vector<double> phi0(sp.phi + p * n_f, sp.phi + (p + 1) * n_f), Zd((size_t)(K * K));
    std::fill(phi0.begin() + f0_t, phi0.begin() + f0_t + N, 0.0);  // the target is not part of the base model
    std::vector<long double> Bl((size_t)K * (size_t)n), Fk((size_t)n);
    const uint8_t* mk = sp.mask ? sp.mask + o : nullptr;
    rank[(size_t)p] = fpta_os::build_operator(n, toas + o, nu + o, m, M ? M + o * n_col : nullptr, n_col,
                                              weights ? weights + o : nullptr, sp, f, phi0.data(), mk, n_toa, rcond,
                                              B + K * o, Zd.data(), nullptr, Bl.data());
    long double* Z = Zall + p * K * K;
    for (int32_t j = 0; j < K; ++j) {
      target_column(n, toas + o, nu + o, sp, f, mk, n_toa, j, Fk.data());
      for (int32_t k = 0; k < K; ++k) {
        const long double* row = Bl.data() + (size_t)k * (size_t)n;
        long double s = 0.0L;
        for (int64_t i = 0; i < n; ++i) s += row[i] * Fk[(size_t)i];
        Z[(int64_t)k * K + j] = s;
      }
    }
  });
}

// The tables of a whole array as the kernels and the callers read them
struct Plan {
  int32_t K = 0, N = 0, G = 0;
  int64_t u_stride = 0;        // packed_size(K): doubles of one (pulsar, grid point)
  std::vector<double> B;       // pulsar p's operator [K][n_p] starts at K offs[p]
  std::vector<int32_t> rows;   // [n_psr] K for a pulsar with TOAs, else 0 (k_fit_apply's count of rows to make)
  std::vector<int32_t> rank;   // [n_psr] kept columns of M
  std::vector<double> U;       // [n_psr][G][u_stride], the device layout
  std::vector<double> ld;      // [n_psr][G]
  std::vector<double> ld_sum;  // [G], summed in pulsar order in long double
  int32_t max_rows = 0;
};

// Validates, then builds every pulsar's operator and every (pulsar, grid point)'s U and ld. 0: done. 1: refused, the
// reason in why. 2: the tables' memory could not be had, the size in why. U_dense NULL or [n_psr][G][K][K]: the plan's
// fp64 U, row-major, zeros above the diagonal. The plan is unspecified unless 0 comes back.
inline int make_plan(int64_t n_psr, const int64_t* offs, const double* toas, const double* nu, const Spec& sp,
                     int64_t n_col, const double* M, const int32_t* ncol_psr, const double* weights, double rcond,
                     int64_t n_grid, const double* phi_grid, Plan& plan, std::string& why, double* U_dense = nullptr) {
  if (!validate(n_psr, offs, toas, nu, sp, n_col, M, ncol_psr, weights, n_grid, phi_grid, why)) return 1;
  const fpta_fit::Spec& cs = sp.comps;
  const int64_t n_toa = n_psr > 0 ? offs[n_psr] : 0;
  plan.N = cs.n_modes[sp.target];
  plan.K = 2 * plan.N;
  plan.G = (int32_t)n_grid;
  plan.u_stride = packed_size(plan.K);
  plan.max_rows = 0;
  const int64_t K = plan.K, G = n_grid;
  const double bytes = 8.0 * ((double)K * (double)n_toa + (double)n_psr * (double)G * (double)(plan.u_stride + 1));
  try {
    plan.B.assign((size_t)K * (size_t)n_toa, 0.0);
    plan.U.assign((size_t)n_psr * (size_t)G * (size_t)plan.u_stride, 0.0);
    plan.ld.assign((size_t)n_psr * (size_t)G, 0.0);
    plan.ld_sum.assign((size_t)G, 0.0);
    plan.rows.assign((size_t)n_psr, 0);
    plan.rank.assign((size_t)n_psr, 0);
    std::vector<long double> Zall((size_t)n_psr * (size_t)(K * K), 0.0L), ld_ld((size_t)n_psr * (size_t)G, 0.0L);
    // sqrt(phi_g) per column, shared by the pulsars
    std::vector<long double> sg((size_t)G * (size_t)K);
    for (int64_t g = 0; g < G; ++g)
      for (int64_t k = 0; k < K; ++k)
        sg[(size_t)(g * K + k)] = std::sqrt((long double)phi_grid[g * plan.N + (k < plan.N ? k : k - plan.N)]);
    const unsigned hw = std::thread::hardware_concurrency();
    const int64_t cap = std::min<int64_t>((int64_t)(hw ? hw : 1), kPoolMax);
    bool no_mem = build_operators(n_psr, offs, toas, nu, sp, n_col, M, ncol_psr, weights, rcond, cap, plan.B.data(),
                                  plan.rows.data(), plan.rank.data(), Zall.data());
    if (no_mem) throw std::bad_alloc();
    // the grid: items are (pulsar, chunk of grid points)
    const int64_t chunk = 8, n_ch = (G + chunk - 1) / chunk, items = n_psr * n_ch;
    const int64_t work_g = n_psr * G * K * K * K;
    no_mem = fpta_os::run_pool(items, std::min<int64_t>({cap, std::max<int64_t>(work_g >> 22, 1), items}),
                               [&](int64_t it) {
      const int64_t p = it / n_ch, g0 = (it - p * n_ch) * chunk, g1 = std::min(g0 + chunk, G);
      std::vector<long double> Lw((size_t)(K * K)), U((size_t)(K * K));
      for (int64_t g = g0; g < g1; ++g) {
        ld_ld[(size_t)(p * G + g)] = factor_point((int32_t)K, Zall.data() + p * K * K, sg.data() + g * K, Lw.data(),
                                                  U.data());
        plan.ld[(size_t)(p * G + g)] = (double)ld_ld[(size_t)(p * G + g)];
        double* pk = plan.U.data() + (p * G + g) * plan.u_stride;
        double* dn = U_dense ? U_dense + (p * G + g) * K * K : nullptr;
        for (int32_t i = 0; i < K; ++i)
          for (int32_t j = 0; j < K; ++j) {
            const double u = (double)U[(size_t)((int64_t)i * K + j)];
            if (j <= i) pk[packed_index(i, j)] = u;
            if (dn) dn[(int64_t)i * K + j] = u;
          }
      }
    });
    if (no_mem) throw std::bad_alloc();
    for (int64_t g = 0; g < G; ++g) {
      long double s = 0.0L;
      for (int64_t p = 0; p < n_psr; ++p) s += ld_ld[(size_t)(p * G + g)];
      plan.ld_sum[(size_t)g] = (double)s;
    }
    for (int64_t p = 0; p < n_psr; ++p) plan.max_rows = std::max(plan.max_rows, plan.rows[(size_t)p]);
  } catch (const std::bad_alloc&) {
    why = "no host memory for the tables of " + std::to_string(bytes) + " bytes (operator 8 K n_toa, U 8 P G " +
          std::to_string(plan.u_stride) + "; K = " + std::to_string(plan.K) + ", n_toa = " + std::to_string(n_toa) +
          ", G = " + std::to_string(plan.G) + ")";
    return 2;
  }
  return 0;
}

}  // namespace fpta_lnl
