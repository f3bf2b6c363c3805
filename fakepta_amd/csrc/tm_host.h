// Timing-model projection (fpta_batch_set_timing_model, fpta_batch_project, fpta_tm_project): input validation and the
// per-pulsar basis, on the host in plain C++. No HIP here: tm.hip includes it for the tables its kernel reads, and a
// stand-alone CPU program can include it alone (tests/test_tm_host.py builds one under the address sanitizer). The
// definition is in include/fakepta_amd.h.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

namespace fpta_tm {

constexpr int32_t kMaxCol = 16;          // columns of one pulsar's design matrix; the row length of the Q table
constexpr double kDefaultRcond = 1e-10;  // rcond <= 0 asks for this

inline long double rcond_of(double rcond) { return rcond > 0.0 ? (long double)rcond : (long double)kDefaultRcond; }

// Everything the entry points refuse: the shape, the column counts, the entries of the columns in use, the weights.
// M [n_toa][n_col] row-major; ncol_psr NULL (every pulsar uses n_col columns) or [n_psr]; weights NULL (unit) or
// [n_toa]. False with the reason in why.
inline bool validate(int64_t n_psr, const int64_t* offs, int64_t n_col, const double* M, const int32_t* ncol_psr,
                     const double* weights, std::string& why) {
  if (n_psr < 0 || (n_psr > 0 && !offs)) {
    why = "bad pulsar table";
    return false;
  }
  if (n_col < 0 || n_col > kMaxCol) {
    why = "n_col " + std::to_string(n_col) + " outside [0, " + std::to_string(kMaxCol) + "]";
    return false;
  }
  if (n_psr == 0) return true;
  if (offs[0] != 0) {
    why = "offs[0] must be 0";
    return false;
  }
  for (int64_t p = 0; p < n_psr; ++p)
    if (offs[p + 1] < offs[p]) {
      why = "pulsar " + std::to_string(p) + ": offs decreases";
      return false;
    }
  if (n_col > 0 && offs[n_psr] > 0 && !M) {
    why = "M missing";
    return false;
  }
  for (int64_t p = 0; p < n_psr; ++p) {
    const int64_t m = ncol_psr ? ncol_psr[p] : n_col;
    if (m < 0 || m > n_col) {
      why = "pulsar " + std::to_string(p) + ": " + std::to_string(m) + " columns outside [0, n_col = " +
            std::to_string(n_col) + "]";
      return false;
    }
    for (int64_t t = offs[p]; t < offs[p + 1]; ++t) {
      for (int64_t j = 0; j < m; ++j)
        if (!std::isfinite(M[t * n_col + j])) {
          why = "pulsar " + std::to_string(p) + ", TOA " + std::to_string(t - offs[p]) + ", column " +
                std::to_string(j) + ": not finite";
          return false;
        }
      if (weights && !(weights[t] > 0.0 && std::isfinite(weights[t]))) {
        why = "pulsar " + std::to_string(p) + ", TOA " + std::to_string(t - offs[p]) +
              ": weight is not positive and finite";
        return false;
      }
    }
  }
  return true;
}

// The basis of one pulsar: n TOAs, the m <= kMaxCol leading columns of M (row stride ldm), weights w (NULL: unit).
// Every column of W^(1/2) M is scaled to unit norm, then orthogonalised against the columns kept so far by modified
// Gram-Schmidt, twice (one re-orthogonalisation), in long double. A column that is all zero, or whose norm after both
// passes is <= rcond (times its scaled norm, 1), is dropped. Q [n][kMaxCol] gets the kept columns rounded to fp64 and
// zeros behind them, s [n] = sqrt(w) rounded to fp64; norms (NULL or [m]) the orthogonalised norm of every column (0
// for an all-zero one). Returns the rank k <= min(m, n).
inline int32_t build_basis(int64_t n, int32_t m, const double* M, int64_t ldm, const double* w, double rcond, double* Q,
                           double* s, long double* norms = nullptr) {
  const long double rc = rcond_of(rcond);
  std::vector<long double> sq((size_t)n), v((size_t)n);
  std::vector<std::vector<long double>> kept;
  for (int64_t t = 0; t < n; ++t) {
    sq[(size_t)t] = w ? std::sqrt((long double)w[t]) : 1.0L;
    s[t] = (double)sq[(size_t)t];
    for (int32_t j = 0; j < kMaxCol; ++j) Q[t * kMaxCol + j] = 0.0;
  }
  for (int32_t j = 0; j < m; ++j) {
    long double nrm2 = 0.0L;
    for (int64_t t = 0; t < n; ++t) {
      v[(size_t)t] = sq[(size_t)t] * (long double)M[t * ldm + j];
      nrm2 += v[(size_t)t] * v[(size_t)t];
    }
    if (norms) norms[j] = 0.0L;
    if (!(nrm2 > 0.0L)) continue;
    const long double inv = 1.0L / std::sqrt(nrm2);
    for (int64_t t = 0; t < n; ++t) v[(size_t)t] *= inv;
    for (int pass = 0; pass < 2; ++pass)
      for (const std::vector<long double>& q : kept) {
        long double dot = 0.0L;
        for (int64_t t = 0; t < n; ++t) dot += q[(size_t)t] * v[(size_t)t];
        for (int64_t t = 0; t < n; ++t) v[(size_t)t] -= dot * q[(size_t)t];
      }
    nrm2 = 0.0L;
    for (int64_t t = 0; t < n; ++t) nrm2 += v[(size_t)t] * v[(size_t)t];
    const long double nrm = std::sqrt(nrm2);
    if (norms) norms[j] = nrm;
    if (!(nrm > rc)) continue;
    for (int64_t t = 0; t < n; ++t) v[(size_t)t] /= nrm;
    kept.push_back(v);
  }
  const int32_t k = (int32_t)kept.size();
  for (int32_t i = 0; i < k; ++i)
    for (int64_t t = 0; t < n; ++t) Q[t * kMaxCol + i] = (double)kept[(size_t)i][(size_t)t];
  return k;
}

// The tables of a whole array as k_tm_project reads them
struct Plan {
  std::vector<double> Q;      // [n_toa][kMaxCol]
  std::vector<double> s;      // [n_toa]
  std::vector<int32_t> rank;  // [n_psr]
  int32_t max_rank = 0;
};

// Validates, then builds every pulsar's basis. False with the reason in why; the plan is then unspecified.
inline bool make_plan(int64_t n_psr, const int64_t* offs, int64_t n_col, const double* M, const int32_t* ncol_psr,
                      const double* weights, double rcond, Plan& plan, std::string& why) {
  if (!validate(n_psr, offs, n_col, M, ncol_psr, weights, why)) return false;
  const int64_t n_toa = n_psr > 0 ? offs[n_psr] : 0;
  plan.Q.assign((size_t)n_toa * kMaxCol, 0.0);
  plan.s.assign((size_t)n_toa, 1.0);
  plan.rank.assign((size_t)n_psr, 0);
  plan.max_rank = 0;
  for (int64_t p = 0; p < n_psr; ++p) {
    const int64_t o = offs[p], n = offs[p + 1] - o;
    const int32_t m = ncol_psr ? ncol_psr[p] : (int32_t)n_col;
    if (n == 0) continue;
    const int32_t k = build_basis(n, m, M ? M + o * n_col : nullptr, n_col, weights ? weights + o : nullptr, rcond,
                                  plan.Q.data() + o * kMaxCol, plan.s.data() + o);
    plan.rank[(size_t)p] = k;
    if (k > plan.max_rank) plan.max_rank = k;
  }
  return true;
}

}  // namespace fpta_tm
