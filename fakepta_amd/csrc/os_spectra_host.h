// Optimal statistic under a noise spectrum per realization (fpta_batch_set_os_spectra, fpta_batch_os_spectra), host
// side in plain C++: validation and the per-pulsar plan. No HIP here: os_spectra.hip includes it for the tables its
// kernels read, and a stand-alone CPU program can include it alone (tests/test_os_spectra_host.py builds one under
// the address sanitizer). The definition is in include/fakepta_amd.h.
//
// The components are split into a varied set V (the target last) and the fixed rest. With T_p the stacked Fourier
// columns of V (q of them) and P0_p the covariance without V, the plan of a pulsar is
//   B0_p = T_p^T P0_p^-1  [q][n_p]   and   A_p = B0_p T_p  [q][q],
// made by os_host.h's build_operator, one call per varied component as its target, with the prior variance of every
// varied mode set to 0: the columns of V are then not part of the model, and their rows take the projection form
// W^(1/2) (I - Q1 Q1^T) W^(1/2) F_k of the fixed model's basis (the same basis in every call: the fixed columns keep
// their order). Everything that depends on a realization's spectrum is left to the device.
#pragma once
#include "os_host.h"

namespace fpta_oss {

constexpr int32_t kMaxVary = 4;   // components of the varied set
constexpr int32_t kMaxCol = 128;  // Fourier columns of the varied set, q
using fpta_fit::kTwoPi;

// The noise model and the target as os_host.h takes them, and the varied set: component indices, distinct, the
// target's last
struct Spec {
  fpta_os::Spec os;
  int32_t n_vary = 0;
  const int32_t* vary = nullptr;
};

inline int32_t cols_of(const Spec& sp) {
  int32_t q = 0;
  for (int32_t v = 0; v < sp.n_vary; ++v) q += 2 * sp.os.comps.n_modes[sp.vary[v]];
  return q;
}

// Everything the entry point refuses beyond os_host.h's validate
inline bool validate(int64_t n_psr, const int64_t* offs, const double* toas, const double* nu, const Spec& sp,
                     int64_t n_col, const double* M, const int32_t* ncol_psr, const double* weights, int32_t n_g,
                     const double* G, std::string& why) {
  if (!fpta_os::validate(n_psr, offs, toas, nu, sp.os, n_col, M, ncol_psr, weights, n_g, G, why)) return false;
  const fpta_fit::Spec& cs = sp.os.comps;
  if (sp.n_vary < 1 || sp.n_vary > kMaxVary || !sp.vary) {
    why = std::to_string(sp.n_vary) + " varied components outside [1, " + std::to_string(kMaxVary) + "]";
    return false;
  }
  for (int32_t v = 0; v < sp.n_vary; ++v) {
    if (sp.vary[v] < 0 || sp.vary[v] >= cs.n_comp) {
      why = "varied component " + std::to_string(sp.vary[v]) + " outside [0, " + std::to_string(cs.n_comp) + ")";
      return false;
    }
    for (int32_t u = 0; u < v; ++u)
      if (sp.vary[u] == sp.vary[v]) {
        why = "varied component " + std::to_string(sp.vary[v]) + " named twice";
        return false;
      }
  }
  if (sp.vary[sp.n_vary - 1] != sp.os.target) {
    why = "the target component " + std::to_string(sp.os.target) + " must be the last of the varied set";
    return false;
  }
  int64_t q = 0;
  for (int32_t v = 0; v < sp.n_vary; ++v) q += 2 * (int64_t)cs.n_modes[sp.vary[v]];
  if (q > kMaxCol) {
    why = "the varied set has " + std::to_string(q) + " Fourier columns, more than " + std::to_string(kMaxCol);
    return false;
  }
  return true;
}

// Column k of component c (k < N_c: the cosine of mode k, else the sine of mode k - N_c) on a pulsar's TOAs, without
// the weights: os_host.h's column, (freqf / nu)^idx cos / sin, 0 off the mask
inline void fourier_column(const fpta_fit::Spec& cs, int32_t c, int32_t k, int64_t n, const double* t, const double* nu,
                           const double* f_c, const uint8_t* mk, long double* out) {
  const int32_t Nc = cs.n_modes[c];
  const long double fk = (long double)f_c[k < Nc ? k : k - Nc];
  for (int64_t i = 0; i < n; ++i) {
    const long double chrom =
        cs.idx[c] == 0.0 ? 1.0L : std::pow((long double)cs.freqf[c] / (long double)nu[i], (long double)cs.idx[c]);
    const long double arg = kTwoPi * fk * (long double)t[i];
    out[i] = mk && !mk[i] ? 0.0L : chrom * (k < Nc ? std::cos(arg) : std::sin(arg));
  }
}

// The plan of one pulsar (the arguments of os_host.h's build_operator; phi this pulsar's row [sum_c N_c], of which
// the varied components' entries are ignored). B0 [q][n] rounded once to fp64; A [q][q] = B0 T from the unrounded B0,
// the lower triangle summed in TOA order and mirrored. Returns the kept columns of M.
inline int32_t build_plan(int64_t n, const double* t, const double* nu, int32_t m, const double* M, int64_t ldm,
                          const double* w, const Spec& sp, const double* f, const double* phi, const uint8_t* mask,
                          int64_t mask_stride, double rcond, double* B0, double* A) {
  const fpta_fit::Spec& cs = sp.os.comps;
  const int64_t n_f = fpta_fit::modes_of(cs);
  const int32_t q = cols_of(sp);
  std::vector<int32_t> f0_of((size_t)cs.n_comp);
  for (int32_t c = 0, k0 = 0; c < cs.n_comp; k0 += cs.n_modes[c], ++c) f0_of[(size_t)c] = k0;
  std::vector<double> phi0(phi, phi + n_f);
  for (int32_t v = 0; v < sp.n_vary; ++v)
    std::fill_n(phi0.begin() + f0_of[(size_t)sp.vary[v]], cs.n_modes[sp.vary[v]], 0.0);
  std::vector<long double> Bl((size_t)q * (size_t)n), col((size_t)n);
  std::vector<double> Zv;
  int32_t rank = 0;
  for (int32_t v = 0, r0 = 0; v < sp.n_vary; ++v) {
    const int32_t Kv = 2 * cs.n_modes[sp.vary[v]];
    fpta_os::Spec one = sp.os;
    one.target = sp.vary[v];
    Zv.assign((size_t)Kv * (size_t)Kv, 0.0);
    rank = fpta_os::build_operator(n, t, nu, m, M, ldm, w, one, f, phi0.data(), mask, mask_stride, rcond,
                                   B0 + (int64_t)r0 * n, Zv.data(), nullptr, Bl.data() + (size_t)r0 * (size_t)n);
    r0 += Kv;
  }
  for (int32_t v = 0, j0 = 0; v < sp.n_vary; ++v) {
    const int32_t c = sp.vary[v], Kv = 2 * cs.n_modes[c];
    for (int32_t k = 0; k < Kv; ++k) {
      const int32_t j = j0 + k;
      fourier_column(cs, c, k, n, t, nu, f + f0_of[(size_t)c], mask ? mask + (int64_t)c * mask_stride : nullptr,
                     col.data());
      for (int32_t i = j; i < q; ++i) {
        const long double* row = Bl.data() + (size_t)i * (size_t)n;
        long double s = 0.0L;
        for (int64_t e = 0; e < n; ++e) s += row[e] * col[(size_t)e];
        A[(int64_t)i * q + j] = A[(int64_t)j * q + i] = (double)s;
      }
    }
    j0 += Kv;
  }
  return rank;
}

// The tables of a whole array as the kernels read them
struct Plan {
  int32_t q = 0, K = 0, N = 0;  // columns of the varied set; columns and modes of the target (the last K of q)
  std::vector<double> B0;       // pulsar p's operator [q][n_p] starts at q offs[p]
  std::vector<int32_t> rows;    // [n_psr] q for a pulsar with TOAs, else 0
  std::vector<int32_t> rank;    // [n_psr] kept columns of M
  std::vector<double> A;        // [n_psr][q][q], zero for a pulsar without TOAs
  int32_t max_rows = 0;
};

// Validates, then plans every pulsar. 0: done. 1: refused, the reason in why. 2: the tables' memory (8 q n_toa bytes of
// operator) could not be had, the size in why. The plan is unspecified unless 0 comes back.
inline int make_plan(int64_t n_psr, const int64_t* offs, const double* toas, const double* nu, const Spec& sp,
                     int64_t n_col, const double* M, const int32_t* ncol_psr, const double* weights, double rcond,
                     int32_t n_g, const double* G, Plan& plan, std::string& why) {
  if (!validate(n_psr, offs, toas, nu, sp, n_col, M, ncol_psr, weights, n_g, G, why)) return 1;
  const fpta_fit::Spec& cs = sp.os.comps;
  const int64_t n_toa = n_psr > 0 ? offs[n_psr] : 0, n_f = fpta_fit::modes_of(cs);
  plan.N = cs.n_modes[sp.os.target];
  plan.K = 2 * plan.N;
  plan.q = cols_of(sp);
  plan.max_rows = 0;
  const int64_t q = plan.q;
  try {
    plan.B0.assign((size_t)q * (size_t)n_toa, 0.0);
    plan.A.assign((size_t)n_psr * (size_t)(q * q), 0.0);
    plan.rows.assign((size_t)n_psr, 0);
    plan.rank.assign((size_t)n_psr, 0);
    const unsigned hw = std::thread::hardware_concurrency();
    const int64_t cap = std::min<int64_t>((int64_t)(hw ? hw : 1), 16);
    const int64_t work = (2 * n_f) * (2 * n_f) * n_toa;
    const bool no_mem = fpta_os::run_pool(n_psr, std::min<int64_t>({cap, work >> 24, n_psr}), [&](int64_t p) {
      const int64_t o = offs[p], n = offs[p + 1] - o;
      const int32_t m = ncol_psr ? ncol_psr[p] : (int32_t)n_col;
      if (n == 0) return;  // z = 0 and A = 0
      plan.rows[(size_t)p] = plan.q;
      plan.rank[(size_t)p] =
          build_plan(n, toas + o, nu + o, m, M ? M + o * n_col : nullptr, n_col, weights ? weights + o : nullptr, sp,
                     cs.f + (cs.f_is_common ? 0 : p * n_f), sp.os.phi + p * n_f, sp.os.mask ? sp.os.mask + o : nullptr,
                     n_toa, rcond, plan.B0.data() + q * o, plan.A.data() + p * q * q);
    });
    if (no_mem) throw std::bad_alloc();
    for (int64_t p = 0; p < n_psr; ++p) plan.max_rows = std::max(plan.max_rows, plan.rows[(size_t)p]);
  } catch (const std::bad_alloc&) {
    why = "no host memory for the operator of " + std::to_string(8.0 * (double)plan.q * (double)n_toa) +
          " bytes (8 q n_toa, q = " + std::to_string(plan.q) + ", n_toa = " + std::to_string(n_toa) + ")";
    return 2;
  }
  return 0;
}

}  // namespace fpta_oss
