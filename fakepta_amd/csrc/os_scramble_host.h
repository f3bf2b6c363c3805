// Sky scrambles of the optimal statistic (fpta_batch_set_os_scrambles, fpta_batch_os_scrambles, fpta_os_scrambles,
// fpta_os_scramble_match): the pair rows' index map and everything the entry points refuse, on the host in plain C++.
// No HIP here: os_scramble.hip includes it, and a stand-alone CPU program can include it alone
// (tests/test_os_scramble_host.py builds one under the address sanitizer). The definition is in include/fakepta_amd.h.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

namespace fpta_scr {

constexpr int64_t kMaxScr = 65536;                 // scrambles of one set
constexpr int64_t kMaxRowBytes = (int64_t)8 << 30;  // their pair rows, 8 n_scr n_pair_pad bytes
constexpr int64_t kPairPad = 16;                   // the pair axis is padded to k_scr_gemm's k-chunk
constexpr double kUnitTol = 1e-12;                 // | |p| - 1 | of a position

// The pairs a > b of P pulsars in the order of np.tril_indices(P, -1): pair e = a (a - 1) / 2 + b
inline int64_t n_pair(int64_t P) { return P > 1 ? P * (P - 1) / 2 : 0; }
inline int64_t n_pair_pad(int64_t P) { return (n_pair(P) + kPairPad - 1) / kPairPad * kPairPad; }
inline int64_t pair_index(int64_t a, int64_t b) { return a * (a - 1) / 2 + b; }

// The map the kernels read: ab[2 e] = a, ab[2 e + 1] = b for the n_pair pairs, -1, -1 for the padding
inline void make_pair_map(int64_t P, std::vector<int32_t>& ab) {
  ab.assign((size_t)(2 * n_pair_pad(P)), -1);
  for (int64_t a = 1; a < P; ++a)
    for (int64_t b = 0; b < a; ++b) {
      const int64_t e = pair_index(a, b);
      ab[(size_t)(2 * e)] = (int32_t)a;
      ab[(size_t)(2 * e + 1)] = (int32_t)b;
    }
}

// x = (1 - p_a . p_b) / 2 with every operation rounded once, in this order (k_scr_orf does the same, so the host's
// refusal of a non-finite weight and the device's rows agree on which pairs are coincident)
inline double pair_x(const double* pa, const double* pb) {
  const double dot = (pa[0] * pb[0] + pa[1] * pb[1]) + pa[2] * pb[2];
  return (1.0 - dot) * 0.5;
}

// Hellings-Downs: 1.5 x ln x - x / 4 + 1 / 2 (x <= 0: NaN, as fakepta.correlated_noises.hd)
inline double hd_weight(double x) { return 1.5 * x * std::log(x) - 0.25 * x + 0.5; }

// The shape of a set: n_scr scrambles of n_psr pulsars, exactly one of pos [n_scr][n_psr][3] and G
// [n_scr][n_psr][n_psr]. Nothing is read.
inline bool validate_shape(int64_t n_psr, int64_t n_scr, const double* pos, const double* G, std::string& why) {
  if (n_scr < 0) {
    why = "negative scramble count";
    return false;
  }
  if (n_scr > kMaxScr) {
    why = std::to_string(n_scr) + " scrambles, more than " + std::to_string(kMaxScr);
    return false;
  }
  if (n_psr < 2) {
    why = "fewer than 2 pulsars: no pair to scramble";
    return false;
  }
  if ((pos != nullptr) == (G != nullptr)) {
    why = "exactly one of positions and matrices must be given";
    return false;
  }
  const int64_t bytes = 8 * n_scr * n_pair_pad(n_psr);
  if (bytes > kMaxRowBytes) {
    why = "the pair rows take " + std::to_string(bytes) + " bytes (8 n_scr n_pair_pad), more than 8 GiB";
    return false;
  }
  return true;
}

// One scramble's inputs and, with nab [n_psr][n_psr] (NULL: not asked), its norm sum_{a > b} G_ab^2 N_ab > 0
inline bool validate_one(int64_t n_psr, int64_t j, const double* pos, const double* G, const double* nab,
                         std::string& why) {
  const std::string sj = "scramble " + std::to_string(j);
  if (pos) {
    const double* p = pos + j * n_psr * 3;
    for (int64_t a = 0; a < n_psr; ++a) {
      const double* v = p + 3 * a;
      if (!(std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]))) {
        why = sj + ", pulsar " + std::to_string(a) + ": position is not finite";
        return false;
      }
      const double len = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
      if (!(std::fabs(len - 1.0) <= kUnitTol)) {
        why = sj + ", pulsar " + std::to_string(a) + ": position is not of unit length";
        return false;
      }
    }
  }
  long double norm = 0.0L;
  for (int64_t a = 1; a < n_psr; ++a)
    for (int64_t b = 0; b < a; ++b) {
      double g;
      if (pos) {
        g = hd_weight(pair_x(pos + (j * n_psr + a) * 3, pos + (j * n_psr + b) * 3));
      } else {
        const double* m = G + j * n_psr * n_psr;
        g = m[a * n_psr + b];
        if (std::isfinite(g) && std::isfinite(m[b * n_psr + a]) && g != m[b * n_psr + a]) {
          why = sj + ", pair (" + std::to_string(b) + ", " + std::to_string(a) + "): not symmetric";
          return false;
        }
        if (!std::isfinite(m[b * n_psr + a])) g = m[b * n_psr + a];
      }
      if (!std::isfinite(g)) {
        why = sj + ", pair (" + std::to_string(b) + ", " + std::to_string(a) + "): pair weight is not finite";
        return false;
      }
      if (nab) norm += (long double)g * (long double)g * (long double)nab[a * n_psr + b];
    }
  if (nab && !(norm > 0.0L)) {
    why = sj + ": norm is not positive";
    return false;
  }
  return true;
}

// Everything at once, scramble by scramble (the entry points spread validate_one over threads and report the first)
inline bool validate(int64_t n_psr, int64_t n_scr, const double* pos, const double* G, const double* nab,
                     std::string& why) {
  if (!validate_shape(n_psr, n_scr, pos, G, why)) return false;
  for (int64_t j = 0; j < n_scr; ++j)
    if (!validate_one(n_psr, j, pos, G, nab, why)) return false;
  return true;
}

}  // namespace fpta_scr
