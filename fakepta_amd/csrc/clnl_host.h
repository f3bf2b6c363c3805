// Correlated likelihood grid (fpta_batch_set_clnl, fpta_batch_clnl, fpta_clnl_grid): the likelihood grid of lnl_host.h
// with the target's prior coupled between pulsars by an overlap reduction function, cov(a_pk, a_ql) = Gamma_pq phi_k
// delta_kl. Input validation, the per-pulsar operator B_p and Z_p of lnl_host.h, the grid-independent coupled matrix
// T = sum_p (A_p. A_p.^T) (x) Z_p per ORF factor A (A A^T = Gamma) and the scalings s_g = sqrt(phi_g), on the host in
// plain C++ and long double. No HIP here: clnl.hip includes it for the tables its kernels read, and a stand-alone CPU
// program can include it alone (tests/test_clnl_host.py builds one under the address sanitizer). The definition is in
// include/fakepta_amd.h.
#pragma once
#include "lnl_host.h"

namespace fpta_clnl {

constexpr int32_t kMaxOrf = 8;                    // ORF factors of one call
constexpr int64_t kMaxN = 16384;                  // n = P K, the coupled system's size
constexpr int64_t kBudget = (int64_t)32 << 30;    // bytes of cached Cholesky factors, n_orf G 8 n_pad^2
using fpta_lnl::kPoolMax;
using fpta_lnl::Spec;

inline int64_t pad64(int64_t n) { return (n + 63) / 64 * 64; }

// Everything the entry points refuse: what lnl_host.h's validate refuses, a target whose frequencies differ between
// pulsars, n_orf outside [1, 8], a factor entry that is not finite, n = P K > 16384 and cached factors beyond the
// budget.
inline bool validate(int64_t n_psr, const int64_t* offs, const double* toas, const double* nu, const Spec& sp,
                     int64_t n_col, const double* M, const int32_t* ncol_psr, const double* weights, int64_t n_grid,
                     const double* phi_grid, int64_t n_orf, const double* A, std::string& why) {
  if (!fpta_lnl::validate(n_psr, offs, toas, nu, sp, n_col, M, ncol_psr, weights, n_grid, phi_grid, why)) return false;
  if (!sp.comps.f_is_common) {  // per-pulsar rows: the target's must all be the first pulsar's
    const int64_t n_f = fpta_fit::modes_of(sp.comps);
    int64_t f0 = 0;
    for (int32_t c = 0; c < sp.target; ++c) f0 += sp.comps.n_modes[c];
    for (int64_t p = 1; p < n_psr; ++p)
      for (int32_t k = 0; k < sp.comps.n_modes[sp.target]; ++k)
        if (sp.comps.f[p * n_f + f0 + k] != sp.comps.f[f0 + k]) {
          why = "target component " + std::to_string(sp.target) + ": pulsar " + std::to_string(p) + ", mode " +
                std::to_string(k) + " has its own frequency; a correlated process needs one grid for the array";
          return false;
        }
  }
  if (n_orf < 1 || n_orf > kMaxOrf) {
    why = std::to_string(n_orf) + " ORFs outside [1, " + std::to_string(kMaxOrf) + "]";
    return false;
  }
  if (!A) {
    why = "ORF factors missing";
    return false;
  }
  for (int64_t o = 0; o < n_orf; ++o)
    for (int64_t p = 0; p < n_psr; ++p)
      for (int64_t j = 0; j < n_psr; ++j)
        if (!std::isfinite(A[(o * n_psr + p) * n_psr + j])) {
          why = "ORF " + std::to_string(o) + ", factor entry (" + std::to_string(p) + ", " + std::to_string(j) +
                ") is not finite";
          return false;
        }
  const int64_t n = n_psr * 2 * (int64_t)sp.comps.n_modes[sp.target];
  if (n > kMaxN) {
    why = "the coupled system has n = P K = " + std::to_string(n) + " coefficients, more than " + std::to_string(kMaxN);
    return false;
  }
  const int64_t n_pad = pad64(n), bytes = n_orf * n_grid * 8 * n_pad * n_pad;
  if (bytes > kBudget) {
    why = "the cached factors need " + std::to_string(bytes) + " bytes (n_orf " + std::to_string(n_orf) + ", G " +
          std::to_string(n_grid) + ", n " + std::to_string(n) + "), more than the budget of " +
          std::to_string(kBudget);
    return false;
  }
  return true;
}

// The tables of a whole array as the kernels and the callers read them. Index (p, k) of the coupled system is p K + k.
struct Plan {
  int32_t K = 0, N = 0, G = 0, n_orf = 0;
  int64_t n = 0, n_pad = 0;   // P K and its round-up to 64
  std::vector<double> B;      // pulsar p's operator [K][n_p] starts at K offs[p]
  std::vector<int32_t> rows;  // [n_psr] K for a pulsar with TOAs, else 0
  std::vector<int32_t> rank;  // [n_psr] kept columns of M
  std::vector<double> A;      // [n_orf][n_psr][n_psr], as given
  std::vector<double> T;      // [n_orf][n_pad][n_pad], symmetric, the padding zero
  std::vector<double> s;      // [G][n_pad] sqrt(phi_g) per column, tiled over the pulsars, the padding zero
  int32_t max_rows = 0;
};

// T of one ORF factor A [P][P] from Z [P][K][K] (long double; its lower triangles are read, as lnl_host.h's factor
// reads them): block (i, j) = sum_p A_pi A_pj Z_p, summed in pulsar order in long double and rounded once. Items are
// the block rows i; item i writes the blocks (i, j <= i) and their mirrors (j, i). True when memory ran out.
inline bool build_t(int64_t P, int64_t K, const double* A, const long double* Z, int64_t n_pad, double* T,
                    int64_t cap) {
  const int64_t work = P * P * P * K * K / 2;
  return fpta_os::run_pool(P, std::min<int64_t>({cap, std::max<int64_t>(work >> 22, 1), P}), [&](int64_t i) {
    std::vector<long double> acc((size_t)(K * K));
    for (int64_t j = 0; j <= i; ++j) {
      std::fill(acc.begin(), acc.end(), 0.0L);
      for (int64_t p = 0; p < P; ++p) {
        const long double w = (long double)A[p * P + i] * (long double)A[p * P + j];
        if (w == 0.0L) continue;
        const long double* Zp = Z + p * K * K;
        for (int64_t k = 0; k < K; ++k)
          for (int64_t l = 0; l < K; ++l) acc[(size_t)(k * K + l)] += w * Zp[k >= l ? k * K + l : l * K + k];
      }
      for (int64_t k = 0; k < K; ++k)
        for (int64_t l = 0; l < K; ++l) {
          const double v = (double)acc[(size_t)(k * K + l)];
          T[(i * K + k) * n_pad + j * K + l] = v;
          T[(j * K + l) * n_pad + i * K + k] = v;
        }
    }
  });
}

// Validates, then builds every pulsar's operator, T per ORF and s per grid point. 0: done. 1: refused, the reason in
// why. 2: the tables' memory could not be had, the size in why. The plan is unspecified unless 0 comes back.
inline int make_plan(int64_t n_psr, const int64_t* offs, const double* toas, const double* nu, const Spec& sp,
                     int64_t n_col, const double* M, const int32_t* ncol_psr, const double* weights, double rcond,
                     int64_t n_grid, const double* phi_grid, int64_t n_orf, const double* A, Plan& plan,
                     std::string& why) {
  if (!validate(n_psr, offs, toas, nu, sp, n_col, M, ncol_psr, weights, n_grid, phi_grid, n_orf, A, why)) return 1;
  const int64_t n_toa = n_psr > 0 ? offs[n_psr] : 0;
  plan.N = sp.comps.n_modes[sp.target];
  plan.K = 2 * plan.N;
  plan.G = (int32_t)n_grid;
  plan.n_orf = (int32_t)n_orf;
  plan.n = n_psr * plan.K;
  plan.n_pad = pad64(plan.n);
  plan.max_rows = 0;
  const int64_t K = plan.K, G = n_grid, n_pad = plan.n_pad;
  const double bytes = 8.0 * ((double)K * (double)n_toa + (double)(n_orf * n_pad) * (double)n_pad +
                              (double)(G * n_pad)) +
                       16.0 * (double)(n_psr * K * K);
  try {
    plan.B.assign((size_t)K * (size_t)n_toa, 0.0);
    plan.rows.assign((size_t)n_psr, 0);
    plan.rank.assign((size_t)n_psr, 0);
    plan.A.assign(A, A + n_orf * n_psr * n_psr);
    plan.T.assign((size_t)(n_orf * n_pad * n_pad), 0.0);
    plan.s.assign((size_t)(G * n_pad), 0.0);
    std::vector<long double> Zall((size_t)n_psr * (size_t)(K * K), 0.0L);
    for (int64_t g = 0; g < G; ++g)
      for (int64_t p = 0; p < n_psr; ++p)
        for (int64_t k = 0; k < K; ++k)
          plan.s[(size_t)(g * n_pad + p * K + k)] =
              (double)std::sqrt((long double)phi_grid[g * plan.N + (k < plan.N ? k : k - plan.N)]);
    const unsigned hw = std::thread::hardware_concurrency();
    const int64_t cap = std::min<int64_t>((int64_t)(hw ? hw : 1), kPoolMax);
    bool no_mem = fpta_lnl::build_operators(n_psr, offs, toas, nu, sp, n_col, M, ncol_psr, weights, rcond, cap,
                                            plan.B.data(), plan.rows.data(), plan.rank.data(), Zall.data());
    if (no_mem) throw std::bad_alloc();
    for (int64_t o = 0; o < n_orf; ++o)
      if (build_t(n_psr, K, A + o * n_psr * n_psr, Zall.data(), n_pad, plan.T.data() + o * n_pad * n_pad, cap))
        throw std::bad_alloc();
    for (int64_t p = 0; p < n_psr; ++p) plan.max_rows = std::max(plan.max_rows, plan.rows[(size_t)p]);
  } catch (const std::bad_alloc&) {
    why = "no host memory for the tables of " + std::to_string(bytes) +
          " bytes (operator 8 K n_toa, T 8 n_orf n_pad^2; K = " + std::to_string(plan.K) + ", n_toa = " + std::to_string(n_toa) + ", n_pad = " + std::to_string(n_pad) + ")";
    return 2;
  }
  return 0;
}

}  // namespace fpta_clnl
