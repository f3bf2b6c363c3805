// Optimal statistic (fpta_batch_set_os, fpta_batch_os, fpta_os_statistic): input validation, the per-pulsar operator
// B_p = F_p^T P_p^-1 and Z_p = F_p^T P_p^-1 F_p, and the pair normalisations N_ab, on the host in plain C++. No HIP
// here: os.hip includes it for the tables its kernels read, and a stand-alone CPU program can include it alone
// (tests/test_os_host.py builds one under the address sanitizer). The definition is in include/fakepta_amd.h. The
// pulsar table, the nuisance design, the weights and the rank rule are tm_host.h's; the component list, the
// frequencies, the epochs and the radio frequencies are checked by fit_host.h's validate with this file's limits.
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

#include "fit_host.h"

namespace fpta_os {

constexpr int32_t kMaxComp = 8;     // Gaussian-process components of the noise model
constexpr int32_t kMaxCol = 1024;   // Fourier columns of all components of one pulsar, q
constexpr int32_t kMaxCoef = 512;   // Fourier columns of the target component, K = 2 N
using fpta_fit::kTwoPi;

// The noise model and the target, as the entry points take them. n_modes, f, f_is_common, idx, freqf: fit_host.h's
// Spec. phi [n_psr][sum_c N_c]: the prior variance of every mode of every pulsar (cosine and sine alike; 0 leaves the
// mode out of that pulsar's model). mask NULL, or [n_comp][n_toa]: component c acts on TOA t where mask[c n_toa + t]
// != 0 (system noise). target: the component whose columns are F_p; phi_hat [N_target] its template spectrum.
struct Spec {
  fpta_fit::Spec comps;
  const double* phi = nullptr;
  const uint8_t* mask = nullptr;
  int32_t target = 0;
  const double* phi_hat = nullptr;
};

// The same from the C entry points' arguments (the likelihood grid has no template)
inline Spec make_spec(const fpta_fit::Spec& comps, const double* phi, const uint8_t* mask, int32_t target,
                      const double* phi_hat = nullptr) {
  Spec sp;
  sp.comps = comps;
  sp.phi = phi;
  sp.mask = mask;
  sp.target = target;
  sp.phi_hat = phi_hat;
  return sp;
}

// Everything the entry points refuse beyond fit_host.h's validate. G: n_g pair-weight matrices [n_psr][n_psr].
inline bool validate(int64_t n_psr, const int64_t* offs, const double* toas, const double* nu, const Spec& sp,
                     int64_t n_col, const double* M, const int32_t* ncol_psr, const double* weights, int32_t n_g,
                     const double* G, std::string& why) {
  const fpta_fit::Spec& cs = sp.comps;
  if (!fpta_fit::validate(n_psr, offs, toas, nu, cs, n_col, M, ncol_psr, weights, why, kMaxComp, kMaxCol)) return false;
  if (sp.target < 0 || sp.target >= cs.n_comp) {
    why = "target component " + std::to_string(sp.target) + " outside [0, " + std::to_string(cs.n_comp) + ")";
    return false;
  }
  const int32_t N = cs.n_modes[sp.target];
  if (2 * N > kMaxCoef) {
    why = "target component " + std::to_string(sp.target) + ": " + std::to_string(2 * N) +
          " Fourier columns, more than " + std::to_string(kMaxCoef);
    return false;
  }
  if (!sp.phi || !sp.phi_hat) {
    why = "prior variances or template missing";
    return false;
  }
  const int64_t n_f = fpta_fit::modes_of(cs);
  for (int64_t p = 0; p < n_psr; ++p) {
    int64_t k0 = 0;
    for (int32_t c = 0; c < cs.n_comp; ++c) {
      for (int64_t k = 0; k < cs.n_modes[c]; ++k) {
        const double v = sp.phi[p * n_f + k0 + k];
        if (!(v >= 0.0 && std::isfinite(v))) {
          why = "pulsar " + std::to_string(p) + ", component " + std::to_string(c) + ", mode " + std::to_string(k) +
                ": prior variance is negative or not finite";
          return false;
        }
      }
      k0 += cs.n_modes[c];
    }
  }
  for (int32_t k = 0; k < N; ++k)
    if (!(sp.phi_hat[k] > 0.0 && std::isfinite(sp.phi_hat[k]))) {
      why = "target mode " + std::to_string(k) + ": template is not positive and finite";
      return false;
    }
  if (n_g < 0 || (n_g > 0 && n_psr > 0 && !G)) {
    why = "pair-weight matrices missing";
    return false;
  }
  for (int32_t j = 0; j < n_g; ++j) {
    const double* g = G + (int64_t)j * n_psr * n_psr;
    for (int64_t a = 0; a < n_psr; ++a)
      for (int64_t b = 0; b < a; ++b) {
        if (!std::isfinite(g[a * n_psr + b]) || !std::isfinite(g[b * n_psr + a])) {
          why = "pair-weight matrix " + std::to_string(j) + ", pair (" + std::to_string(b) + ", " + std::to_string(a) +
                "): not finite";
          return false;
        }
        if (g[a * n_psr + b] != g[b * n_psr + a]) {
          why = "pair-weight matrix " + std::to_string(j) + ", pair (" + std::to_string(b) + ", " + std::to_string(a) +
                "): not symmetric";
          return false;
        }
      }
  }
  return true;
}

// The operator of one pulsar: n TOAs t with radio frequencies nu, the m <= 16 leading columns of M (row stride ldm),
// weights w (NULL: unit), this pulsar's frequencies f and prior variances phi [sum_c N_c], component c's TOA flags at
// mask + c mask_stride (mask NULL: every component acts everywhere).
//
// The stacked matrix S = [W^(1/2) T ; D^(1/2)], T = [M, the Fourier columns with phi > 0], D = 0 on M's columns and
// 1 / phi on the others, has S^T S = T^T W T + D, so with S = Q R, Q = [Q1 ; Q2]:
//   P^-1 = W^(1/2) (I - Q1 Q1^T) W^(1/2)   and   P^-1 T e_j = W^(1/2) Q1 R^-T e_j D_jj  for a column with D_jj > 0.
// The second form has no subtraction and is the one used for every target column that is part of the model; a target
// column with phi = 0 is not, and its row is W^(1/2) (I - Q1 Q1^T) W^(1/2) F_k, by the same Gram-Schmidt passes. The
// columns of S are scaled to unit norm and taken in order: M's, the other components', the target's last (R^-T e_j
// then involves the target's block only). Modified Gram-Schmidt, twice, in long double. M's columns follow tm_host.h's
// rank rule (all zero, or orthogonalised norm <= rcond: dropped, and then not marginalised); a Fourier column cannot
// drop, its D row is positive.
//
// B [K][n] gets F_p^T P_p^-1 rounded once to fp64, Z [K][K] = B F_p (from the unrounded B) rounded to fp64; norms
// (NULL or [m]) the orthogonalised norm of M's columns; B_ld (NULL or [K][n]) the unrounded operator. Returns the
// number of kept columns of M.
inline int32_t build_operator(int64_t n, const double* t, const double* nu, int32_t m, const double* M, int64_t ldm,
                              const double* w, const Spec& sp, const double* f, const double* phi,
                              const uint8_t* mask, int64_t mask_stride, double rcond, double* B, double* Z,
                              long double* norms = nullptr, long double* B_ld = nullptr) {
  const fpta_fit::Spec& cs = sp.comps;
  const long double rc = fpta_tm::rcond_of(rcond);
  const int32_t N = cs.n_modes[sp.target], K = 2 * N;
  std::vector<int32_t> f0_of((size_t)cs.n_comp);
  for (int32_t c = 0, k0 = 0; c < cs.n_comp; k0 += cs.n_modes[c], ++c) f0_of[(size_t)c] = k0;
  // the Fourier columns of the model in order: (component, column within it), the target's last
  std::vector<int32_t> col_c, col_k;
  for (int pass = 0; pass < 2; ++pass)
    for (int32_t c = 0; c < cs.n_comp; ++c) {
      if ((c == sp.target) != (pass == 1)) continue;
      const int32_t Nc = cs.n_modes[c];
      for (int32_t k = 0; k < 2 * Nc; ++k)
        if (phi[f0_of[(size_t)c] + (k < Nc ? k : k - Nc)] > 0.0) {
          col_c.push_back(c);
          col_k.push_back(k);
        }
    }
  const int32_t qa = (int32_t)col_c.size(), nc = m + qa;
  const int64_t L = n + qa;
  std::vector<long double> sq((size_t)n), v((size_t)L), chrom((size_t)n);
  for (int64_t i = 0; i < n; ++i) sq[(size_t)i] = w ? std::sqrt((long double)w[i]) : 1.0L;
  // column k of component c on this pulsar's TOAs, without the weights: (freqf / nu)^idx cos / sin, 0 off the mask
  int32_t chrom_of = -1;
  auto fourier = [&](int32_t c, int32_t k, long double* out) {
    if (chrom_of != c) {
      for (int64_t i = 0; i < n; ++i)
        chrom[(size_t)i] = cs.idx[c] == 0.0
                               ? 1.0L
                               : std::pow((long double)cs.freqf[c] / (long double)nu[i], (long double)cs.idx[c]);
      chrom_of = c;
    }
    const int32_t Nc = cs.n_modes[c];
    const long double fk = (long double)f[f0_of[(size_t)c] + (k < Nc ? k : k - Nc)];
    const uint8_t* mk = mask ? mask + (int64_t)c * mask_stride : nullptr;
    for (int64_t i = 0; i < n; ++i) {
      const long double arg = kTwoPi * fk * (long double)t[i];
      out[i] = mk && !mk[i] ? 0.0L : chrom[(size_t)i] * (k < Nc ? std::cos(arg) : std::sin(arg));
    }
  };
  std::vector<std::vector<long double>> Q;      // the kept columns' basis vectors [L]
  std::vector<long double> scale;               // their norm before the passes
  std::vector<std::vector<long double>> Rcol;   // Rcol[j][i], i <= j, of the scaled columns
  std::vector<int32_t> kept_of((size_t)qa, -1);  // Fourier column of the model -> its place among the kept ones
  std::vector<long double> proj;
  // both Gram-Schmidt passes of x [len of the basis vectors] against the kept columns; proj (if given) gets the sums
  auto passes = [&](std::vector<long double>& x, std::vector<long double>* pr) {
    for (int pass = 0; pass < 2; ++pass)
      for (size_t q = 0; q < Q.size(); ++q) {
        const long double* qv = Q[q].data();
        long double dot = 0.0L;
        for (int64_t i = 0; i < L; ++i) dot += qv[i] * x[(size_t)i];
        for (int64_t i = 0; i < L; ++i) x[(size_t)i] -= dot * qv[i];
        if (pr) (*pr)[q] += dot;
      }
  };
  int32_t rank_m = 0;
  for (int32_t j = 0; j < nc; ++j) {
    std::fill(v.begin(), v.end(), 0.0L);
    if (j < m) {
      for (int64_t i = 0; i < n; ++i) v[(size_t)i] = sq[(size_t)i] * (long double)M[i * ldm + j];
    } else {
      const int32_t a = j - m, c = col_c[(size_t)a], k = col_k[(size_t)a], Nc = cs.n_modes[c];
      fourier(c, k, v.data());
      for (int64_t i = 0; i < n; ++i) v[(size_t)i] *= sq[(size_t)i];
      v[(size_t)(n + a)] = 1.0L / std::sqrt((long double)phi[f0_of[(size_t)c] + (k < Nc ? k : k - Nc)]);
    }
    long double nrm2 = 0.0L;
    for (int64_t i = 0; i < L; ++i) nrm2 += v[(size_t)i] * v[(size_t)i];
    if (j < m && norms) norms[j] = 0.0L;
    if (!(nrm2 > 0.0L)) continue;
    const long double cn = std::sqrt(nrm2), inv = 1.0L / cn;
    for (int64_t i = 0; i < L; ++i) v[(size_t)i] *= inv;
    proj.assign(Q.size(), 0.0L);
    passes(v, &proj);
    nrm2 = 0.0L;
    for (int64_t i = 0; i < L; ++i) nrm2 += v[(size_t)i] * v[(size_t)i];
    const long double nrm = std::sqrt(nrm2);
    if (j < m) {
      if (norms) norms[j] = nrm;
      if (!(nrm > rc)) continue;
      ++rank_m;
    } else {
      kept_of[(size_t)(j - m)] = (int32_t)Q.size();
    }
    for (int64_t i = 0; i < L; ++i) v[(size_t)i] /= nrm;
    proj.push_back(nrm);
    Q.push_back(v);
    scale.push_back(cn);
    Rcol.push_back(proj);
  }
  // the rows of B, in long double
  const size_t nk = Q.size();
  std::vector<long double> Bl((size_t)K * (size_t)n, 0.0L), Fk((size_t)n), y(nk), acc((size_t)n);
  int32_t a_t = 0;  // the model's Fourier columns before the target's
  for (int32_t a = 0; a < qa; ++a)
    if (col_c[(size_t)a] != sp.target) ++a_t;
  for (int32_t k = 0, a = a_t; k < K; ++k) {
    long double* row = Bl.data() + (size_t)k * (size_t)n;
    const double ph = phi[f0_of[(size_t)sp.target] + (k < N ? k : k - N)];
    if (ph > 0.0) {
      // y = R^-T e_jj by forward substitution (zero before jj), row = s o (Q1 y) D / (the column's scaling)
      const size_t jj = (size_t)kept_of[(size_t)a++];
      y[jj] = 1.0L / Rcol[jj][jj];
      for (size_t i = jj + 1; i < nk; ++i) {
        long double s = 0.0L;
        for (size_t l = jj; l < i; ++l) s += Rcol[i][l] * y[l];
        y[i] = -s / Rcol[i][i];
      }
      std::fill(acc.begin(), acc.end(), 0.0L);
      for (size_t i = jj; i < nk; ++i) {
        const long double yi = y[i];
        const long double* qv = Q[i].data();
        for (int64_t s = 0; s < n; ++s) acc[(size_t)s] += yi * qv[s];
      }
      const long double d = (1.0L / (long double)ph) / scale[jj];
      for (int64_t s = 0; s < n; ++s) row[s] = sq[(size_t)s] * acc[(size_t)s] * d;
    } else {
      // not part of the model: the projection form
      std::fill(v.begin(), v.end(), 0.0L);
      fourier(sp.target, k, v.data());
      for (int64_t i = 0; i < n; ++i) v[(size_t)i] *= sq[(size_t)i];
      passes(v, nullptr);
      for (int64_t s = 0; s < n; ++s) row[s] = sq[(size_t)s] * v[(size_t)s];
    }
  }
  for (int64_t i = 0; i < (int64_t)K * n; ++i) {
    B[i] = (double)Bl[(size_t)i];
    if (B_ld) B_ld[i] = Bl[(size_t)i];
  }
  // Z = B F, column by column of F
  for (int32_t j = 0; j < K; ++j) {
    fourier(sp.target, j, Fk.data());
    for (int32_t k = 0; k < K; ++k) {
      const long double* row = Bl.data() + (size_t)k * (size_t)n;
      long double s = 0.0L;
      for (int64_t i = 0; i < n; ++i) s += row[i] * Fk[(size_t)i];
      Z[(int64_t)k * K + j] = (double)s;
    }
  }
  return rank_m;
}

// N_ab = tr(Z_a phi_hat Z_b phi_hat), phi_hat the diagonal over the K columns (mode k of the cosine and of the sine)
inline double pair_norm(int32_t K, const double* Za, const double* Zb, const double* phi_hat) {
  const int32_t N = K / 2;
  long double s = 0.0L;
  for (int32_t j = 0; j < K; ++j) {
    const long double pj = (long double)phi_hat[j < N ? j : j - N];
    for (int32_t k = 0; k < K; ++k)
      s += (long double)Za[(int64_t)j * K + k] * (long double)phi_hat[k < N ? k : k - N] *
           (long double)Zb[(int64_t)k * K + j] * pj;
  }
  return (double)s;
}

// The tables of a whole array as the kernels and the callers read them
struct Plan {
  int32_t K = 0, N = 0;        // Fourier columns and modes of the target
  std::vector<double> B;       // pulsar p's operator [K][n_p] starts at K offs[p]
  std::vector<int32_t> rows;   // [n_psr] K for a pulsar with TOAs, else 0 (k_fit_apply's count of rows to make)
  std::vector<int32_t> rank;   // [n_psr] kept columns of M
  std::vector<double> Z;       // [n_psr][K][K]
  std::vector<double> Nab;     // [n_psr][n_psr], symmetric, zero diagonal
  int32_t max_rows = 0;
};

// up to n_thr threads take the items 0 .. n_items - 1 in turn; true when one of them ran out of memory
template <class Fn>
inline bool run_pool(int64_t n_items, int64_t n_thr, Fn fn) {
  std::atomic<int64_t> next{0};
  std::atomic<bool> no_mem{false};
  auto work = [&]() {
    try {
      for (int64_t i = next++; i < n_items; i = next++) fn(i);
    } catch (const std::bad_alloc&) {
      no_mem = true;
    }
  };
  std::vector<std::thread> pool;
  try {
    pool.reserve((size_t)std::max<int64_t>(n_thr, 1));
    for (int64_t i = 1; i < n_thr; ++i) pool.emplace_back(work);
  } catch (const std::system_error&) {
    // no more threads to be had: the ones that started and this one share the items
  }
  work();
  for (std::thread& th : pool) th.join();
  return no_mem;
}

// Validates, then builds every pulsar's operator and every pair's N_ab. 0: done. 1: refused, the reason in why. 2: the
// tables' memory (the operator is 8 K n_toa bytes) could not be had, the size in why. The plan is unspecified unless 0
// comes back.
inline int make_plan(int64_t n_psr, const int64_t* offs, const double* toas, const double* nu, const Spec& sp,
                     int64_t n_col, const double* M, const int32_t* ncol_psr, const double* weights, double rcond,
                     int32_t n_g, const double* G, Plan& plan, std::string& why) {
  if (!validate(n_psr, offs, toas, nu, sp, n_col, M, ncol_psr, weights, n_g, G, why)) return 1;
  const fpta_fit::Spec& cs = sp.comps;
  const int64_t n_toa = n_psr > 0 ? offs[n_psr] : 0, n_f = fpta_fit::modes_of(cs);
  plan.N = cs.n_modes[sp.target];
  plan.K = 2 * plan.N;
  plan.max_rows = 0;
  const int64_t K = plan.K;
  try {
    plan.B.assign((size_t)K * (size_t)n_toa, 0.0);
    plan.Z.assign((size_t)n_psr * (size_t)(K * K), 0.0);
    plan.Nab.assign((size_t)n_psr * (size_t)n_psr, 0.0);
    plan.rows.assign((size_t)n_psr, 0);
    plan.rank.assign((size_t)n_psr, 0);
    const unsigned hw = std::thread::hardware_concurrency();
    const int64_t cap = std::min<int64_t>((int64_t)(hw ? hw : 1), 16);
    // the pulsars are independent and write disjoint parts of the plan
    const int64_t work_op = (2 * n_f) * (2 * n_f) * n_toa;
    bool no_mem = run_pool(n_psr, std::min<int64_t>({cap, work_op >> 24, n_psr}), [&](int64_t p) {
      const int64_t o = offs[p], n = offs[p + 1] - o;
      const int32_t m = ncol_psr ? ncol_psr[p] : (int32_t)n_col;
      if (n == 0) return;  // X = 0 and Z = 0
      plan.rows[(size_t)p] = plan.K;
      plan.rank[(size_t)p] = build_operator(
          n, toas + o, nu + o, m, M ? M + o * n_col : nullptr, n_col, weights ? weights + o : nullptr, sp,
          cs.f + (cs.f_is_common ? 0 : p * n_f), sp.phi + p * n_f, sp.mask ? sp.mask + o : nullptr, n_toa, rcond,
          plan.B.data() + K * o, plan.Z.data() + p * K * K);
    });
    if (no_mem) throw std::bad_alloc();
    // the pairs: row a of N_ab for b < a, mirrored
    const int64_t work_n = n_psr * n_psr * K * K;
    no_mem = run_pool(n_psr, std::min<int64_t>({cap, work_n >> 24, n_psr}), [&](int64_t a) {
      for (int64_t b = 0; b < a; ++b)
        plan.Nab[(size_t)(a * n_psr + b)] =
            pair_norm(plan.K, plan.Z.data() + a * K * K, plan.Z.data() + b * K * K, sp.phi_hat);
    });
    if (no_mem) throw std::bad_alloc();
    for (int64_t a = 0; a < n_psr; ++a)
      for (int64_t b = 0; b < a; ++b) plan.Nab[(size_t)(b * n_psr + a)] = plan.Nab[(size_t)(a * n_psr + b)];
    for (int64_t p = 0; p < n_psr; ++p) plan.max_rows = std::max(plan.max_rows, plan.rows[(size_t)p]);
  } catch (const std::bad_alloc&) {
    why = "no host memory for the operator of " + std::to_string(8.0 * (double)plan.K * (double)n_toa) +
          " bytes (8 K n_toa, K = " + std::to_string(plan.K) + ", n_toa = " + std::to_string(n_toa) + ")";
    return 2;
  }
  return 0;
}

}  // namespace fpta_os
