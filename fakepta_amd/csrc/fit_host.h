// Fourier fit (fpta_batch_set_fit, fpta_batch_fit, fpta_fit_coefficients): input validation and the per-pulsar
// operator A_p = R_FF^-1 Q_F^T diag(s), on the host in plain C++. No HIP here: fit.hip includes it for the table its
// kernel reads, and a stand-alone CPU program can include it alone (tests/test_fit_host.py builds one under the
// address sanitizer). The definition is in include/fakepta_amd.h. The nuisance design's validation, the weights and
// the rank rule's constants are those of tm_host.h.
#pragma once
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <new>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "tm_host.h"

namespace fpta_fit {

constexpr int32_t kMaxComp = 4;    // components of one fit
constexpr int32_t kMaxCoef = 512;  // Fourier columns of one pulsar, K = sum_c 2 N_c
constexpr long double kTwoPi = 6.283185307179586476925286766559005768L;

// What a fit is made of, as the entry points take it. f is [sum_c N_c] when f_is_common, else [n_psr][sum_c N_c];
// within a row component c's frequencies start at sum_{c' < c} N_c'.
struct Spec {
  int32_t n_comp = 0;
  const int32_t* n_modes = nullptr;  // [n_comp]
  const double* f = nullptr;
  bool f_is_common = true;
  const double* idx = nullptr;    // [n_comp] chromatic index
  const double* freqf = nullptr;  // [n_comp] reference radio frequency
};

// The component tables as the C entry points pass them
inline Spec make_spec(int32_t n_comp, const int32_t* n_modes, const double* f, int32_t f_is_common, const double* idx,
                      const double* freqf) {
  Spec sp;
  sp.n_comp = n_comp;
  sp.n_modes = n_modes;
  sp.f = f;
  sp.f_is_common = f_is_common != 0;
  sp.idx = idx;
  sp.freqf = freqf;
  return sp;
}

inline int64_t modes_of(const Spec& sp) {
  int64_t n = 0;
  for (int32_t c = 0; c < sp.n_comp; ++c) n += sp.n_modes[c];
  return n;
}

// Everything the entry points refuse beyond tm_host.h's validate (the pulsar table, the nuisance design, the
// weights): the component list, the frequencies, the TOAs and the radio frequencies where a chromatic index needs
// them. False with the reason in why. max_comp and max_coef: the limits of the caller (os_host.h has wider ones).
inline bool validate(int64_t n_psr, const int64_t* offs, const double* toas, const double* nu, const Spec& sp,
                     int64_t n_col, const double* M, const int32_t* ncol_psr, const double* weights,
                     std::string& why, int32_t max_comp = kMaxComp, int32_t max_coef = kMaxCoef) {
  if (!fpta_tm::validate(n_psr, offs, n_col, M, ncol_psr, weights, why)) return false;
  if (sp.n_comp < 1 || sp.n_comp > max_comp) {
    why = std::to_string(sp.n_comp) + " components outside [1, " + std::to_string(max_comp) + "]";
    return false;
  }
  if (!sp.n_modes || !sp.f || !sp.idx || !sp.freqf) {
    why = "component tables missing";
    return false;
  }
  int64_t n_f = 0;
  for (int32_t c = 0; c < sp.n_comp; ++c) {
    if (sp.n_modes[c] < 1 || sp.n_modes[c] > max_coef / 2) {
      why = "component " + std::to_string(c) + ": " + std::to_string(sp.n_modes[c]) + " modes outside [1, " +
            std::to_string(max_coef / 2) + "]";
      return false;
    }
    n_f += sp.n_modes[c];
    if (!std::isfinite(sp.idx[c])) {
      why = "component " + std::to_string(c) + ": chromatic index is not finite";
      return false;
    }
    if (sp.idx[c] != 0.0 && !(sp.freqf[c] > 0.0 && std::isfinite(sp.freqf[c]))) {
      why = "component " + std::to_string(c) + ": reference frequency is not positive and finite";
      return false;
    }
  }
  if (2 * n_f > max_coef) {
    why = std::to_string(2 * n_f) + " Fourier columns, more than " + std::to_string(max_coef);
    return false;
  }
  const int64_t rows = sp.f_is_common ? 1 : n_psr;
  for (int64_t p = 0; p < rows; ++p) {
    int64_t k0 = 0;
    for (int32_t c = 0; c < sp.n_comp; ++c) {
      for (int64_t k = 0; k < sp.n_modes[c]; ++k) {
        const double f = sp.f[p * n_f + k0 + k];
        if (!(f > 0.0 && std::isfinite(f))) {
          why = (sp.f_is_common ? std::string() : "pulsar " + std::to_string(p) + ", ") + "component " +
                std::to_string(c) + ", mode " + std::to_string(k) + ": frequency is not positive and finite";
          return false;
        }
      }
      k0 += sp.n_modes[c];
    }
  }
  const int64_t n_toa = n_psr > 0 ? offs[n_psr] : 0;
  if (n_toa > 0 && (!toas || !nu)) {
    why = "TOAs or radio frequencies missing";
    return false;
  }
  for (int64_t p = 0; p < n_psr; ++p)
    for (int64_t t = offs[p]; t < offs[p + 1]; ++t) {
      if (!std::isfinite(toas[t])) {
        why = "pulsar " + std::to_string(p) + ", TOA " + std::to_string(t - offs[p]) + ": epoch is not finite";
        return false;
      }
      for (int32_t c = 0; c < sp.n_comp; ++c)
        if (sp.idx[c] != 0.0 && !(nu[t] > 0.0 && std::isfinite(nu[t]))) {
          why = "pulsar " + std::to_string(p) + ", TOA " + std::to_string(t - offs[p]) +
                ": radio frequency is not positive and finite, and component " + std::to_string(c) +
                " has a chromatic index";
          return false;
        }
    }
  return true;
}

// The operator of one pulsar: n TOAs t with radio frequencies nu, the m <= 16 leading columns of M (row stride ldm),
// weights w (NULL: unit), the components of sp with this pulsar's frequencies f [sum_c N_c]. The columns of
// W^(1/2) [M F] are scaled to unit norm and taken in order, M's first, through modified Gram-Schmidt, twice, in long
// double; an all-zero column and one whose norm after both passes is <= rcond are dropped (tm_host.h's rule). With
// W^(1/2) [M F]_kept D = Q R (D the scaling), row j of A [K][n] is row j of D_F R_FF^-1 Q_F^T diag(s) for a kept
// Fourier column j and zero for a dropped one, rounded once to fp64. kept [K] gets 1 / 0; norms (NULL or [m + K]) the
// orthogonalised norm of every column; A_ld (NULL or [K][n]) the unrounded operator. Returns the number of kept
// Fourier columns.
inline int32_t build_operator(int64_t n, const double* t, const double* nu, int32_t m, const double* M, int64_t ldm,
                              const double* w, const Spec& sp, const double* f, double rcond, double* A,
                              uint8_t* kept, long double* norms = nullptr, long double* A_ld = nullptr) {
  const long double rc = fpta_tm::rcond_of(rcond);
  const int32_t K = (int32_t)(2 * modes_of(sp)), nc = m + K;
  std::vector<long double> sq((size_t)n), v((size_t)n), chrom((size_t)n);
  for (int64_t i = 0; i < n; ++i) sq[(size_t)i] = w ? std::sqrt((long double)w[i]) : 1.0L;
  for (int64_t i = 0; i < (int64_t)K * n; ++i) A[i] = 0.0;
  if (A_ld)
    for (int64_t i = 0; i < (int64_t)K * n; ++i) A_ld[i] = 0.0L;
  for (int32_t j = 0; j < K; ++j) kept[j] = 0;
  // the kept columns' basis vectors, their column index, their scaling and R (dense upper triangle by kept order)
  std::vector<std::vector<long double>> Q;
  std::vector<int32_t> col_of;
  std::vector<long double> scale;
  std::vector<std::vector<long double>> Rcol;  // Rcol[j][i], i <= j
  std::vector<long double> proj;
  int32_t comp = 0, k_in = 0, f0 = 0;  // of the Fourier column being built
  for (int32_t j = 0; j < nc; ++j) {
    if (j < m) {
      for (int64_t i = 0; i < n; ++i) v[(size_t)i] = sq[(size_t)i] * (long double)M[i * ldm + j];
    } else {
      if (k_in == 0)
        for (int64_t i = 0; i < n; ++i)
          chrom[(size_t)i] = sp.idx[comp] == 0.0
                                 ? 1.0L
                                 : std::pow((long double)sp.freqf[comp] / (long double)nu[i], (long double)sp.idx[comp]);
      const int32_t N = sp.n_modes[comp];
      const long double fk = (long double)f[f0 + (k_in < N ? k_in : k_in - N)];
      for (int64_t i = 0; i < n; ++i) {
        const long double arg = kTwoPi * fk * (long double)t[i];
        v[(size_t)i] = sq[(size_t)i] * (chrom[(size_t)i] * (k_in < N ? std::cos(arg) : std::sin(arg)));
      }
      if (++k_in == 2 * N) {
        k_in = 0;
        f0 += N;
        ++comp;
      }
    }
    long double nrm2 = 0.0L;
    for (int64_t i = 0; i < n; ++i) nrm2 += v[(size_t)i] * v[(size_t)i];
    if (norms) norms[j] = 0.0L;
    if (!(nrm2 > 0.0L)) continue;
    const long double cn = std::sqrt(nrm2), inv = 1.0L / cn;
    for (int64_t i = 0; i < n; ++i) v[(size_t)i] *= inv;
    proj.assign(Q.size(), 0.0L);
    for (int pass = 0; pass < 2; ++pass)
      for (size_t q = 0; q < Q.size(); ++q) {
        const long double* qv = Q[q].data();
        long double dot = 0.0L;
        for (int64_t i = 0; i < n; ++i) dot += qv[i] * v[(size_t)i];
        for (int64_t i = 0; i < n; ++i) v[(size_t)i] -= dot * qv[i];
        proj[q] += dot;
      }
    nrm2 = 0.0L;
    for (int64_t i = 0; i < n; ++i) nrm2 += v[(size_t)i] * v[(size_t)i];
    const long double nrm = std::sqrt(nrm2);
    if (norms) norms[j] = nrm;
    if (!(nrm > rc)) continue;
    for (int64_t i = 0; i < n; ++i) v[(size_t)i] /= nrm;
    proj.push_back(nrm);
    Q.push_back(v);
    col_of.push_back(j);
    scale.push_back(cn);
    Rcol.push_back(proj);
    if (j >= m) kept[j - m] = 1;
  }
  // back substitution over the Fourier block, last kept column first: x_j = (q_j - sum_{i > j} R_ji x_i) / R_jj. A
  // nuisance column never enters: R^-1 is upper triangular, so the Fourier rows of R^-1 Q^T need Q_F only.
  const size_t nk = Q.size();
  size_t first_f = nk;
  for (size_t q = 0; q < nk; ++q)
    if (col_of[q] >= m) {
      first_f = q;
      break;
    }
  int32_t n_kept = 0;
  for (size_t jj = nk; jj-- > first_f;) {
    std::vector<long double>& x = Q[jj];  // q_j becomes x_j in place; the later ones already are
    for (size_t i = jj + 1; i < nk; ++i) {
      const long double r = Rcol[i][jj];
      const long double* xi = Q[i].data();
      for (int64_t s = 0; s < n; ++s) x[(size_t)s] -= r * xi[s];
    }
    const long double d = 1.0L / Rcol[jj][jj];
    for (int64_t s = 0; s < n; ++s) x[(size_t)s] *= d;
    ++n_kept;
  }
  for (size_t jj = first_f; jj < nk; ++jj) {
    const int64_t row = col_of[jj] - m;
    const long double d = 1.0L / scale[jj];
    for (int64_t s = 0; s < n; ++s) {
      const long double a = Q[jj][(size_t)s] * d * sq[(size_t)s];
      A[row * n + s] = (double)a;
      if (A_ld) A_ld[row * n + s] = a;
    }
  }
  return n_kept;
}

// The tables of a whole array as k_fit_apply reads them
struct Plan {
  int32_t K = 0;              // Fourier columns of every pulsar
  std::vector<double> A;      // pulsar p's operator [K][n_p] starts at K offs[p]
  std::vector<uint8_t> kept;  // [n_psr][K]
  std::vector<int32_t> rank;  // [n_psr] kept Fourier columns
  int32_t max_rank = 0;
};

// Validates, then builds every pulsar's operator. 0: done. 1: refused, the reason in why. 2: the operator's memory
// (8 K n_toa bytes) could not be had, the size in why. The plan is unspecified unless 0 comes back.
inline int make_plan(int64_t n_psr, const int64_t* offs, const double* toas, const double* nu, const Spec& sp,
                     int64_t n_col, const double* M, const int32_t* ncol_psr, const double* weights, double rcond,
                     Plan& plan, std::string& why) {
  if (!validate(n_psr, offs, toas, nu, sp, n_col, M, ncol_psr, weights, why)) return 1;
  const int64_t n_toa = n_psr > 0 ? offs[n_psr] : 0, n_f = modes_of(sp);
  plan.K = (int32_t)(2 * n_f);
  plan.max_rank = 0;
  try {
    plan.A.assign((size_t)plan.K * (size_t)n_toa, 0.0);
    plan.kept.assign((size_t)n_psr * (size_t)plan.K, 0);
    plan.rank.assign((size_t)n_psr, 0);
    // the pulsars are independent and write disjoint parts of the plan: up to 16 threads take them in turn
    std::atomic<int64_t> next{0};
    std::atomic<bool> no_mem{false};
    auto work = [&]() {
      try {
        for (int64_t p = next++; p < n_psr; p = next++) {
          const int64_t o = offs[p], n = offs[p + 1] - o;
          const int32_t m = ncol_psr ? ncol_psr[p] : (int32_t)n_col;
          if (n == 0) continue;
          plan.rank[(size_t)p] = build_operator(
              n, toas + o, nu + o, m, M ? M + o * n_col : nullptr, n_col, weights ? weights + o : nullptr, sp,
              sp.f + (sp.f_is_common ? 0 : p * n_f), rcond, plan.A.data() + (int64_t)plan.K * o,
              plan.kept.data() + p * plan.K);
        }
      } catch (const std::bad_alloc&) {
        no_mem = true;
      }
    };
    const unsigned hw = std::thread::hardware_concurrency();
    const int64_t n_thr = std::min<int64_t>({(int64_t)(hw ? hw : 1), 16, (plan.K * n_toa) >> 22, n_psr});
    std::vector<std::thread> pool;
    try {
      pool.reserve((size_t)std::max<int64_t>(n_thr, 1));
      for (int64_t i = 1; i < n_thr; ++i) pool.emplace_back(work);
    } catch (const std::system_error&) {
      // no more threads to be had: the ones that started and this one share the pulsars
    }
    work();
    for (std::thread& t : pool) t.join();
    if (no_mem) throw std::bad_alloc();
    for (int64_t p = 0; p < n_psr; ++p) plan.max_rank = std::max(plan.max_rank, plan.rank[(size_t)p]);
  } catch (const std::bad_alloc&) {
    why = "no host memory for the operator of " + std::to_string(8.0 * (double)plan.K * (double)n_toa) +
          " bytes (8 K n_toa, K = " + std::to_string(plan.K) + ", n_toa = " + std::to_string(n_toa) + ")";
    return 2;
  }
  return 0;
}

}  // namespace fpta_fit
