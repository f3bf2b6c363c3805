// Continuous-wave F-statistics (fpta_batch_set_fe, fpta_batch_fe, fpta_fe_statistic): input validation, the per-pulsar
// operator B_p with the rows c_g^T P_p^-1 and s_g^T P_p^-1, the 2 x 2 matrices m_pg and their inverses, the antenna
// table and per (direction, frequency) the 4 x 4 matrix M and its inverse, on the host in plain C++ and long double. No
// HIP here: fe.hip includes it for the tables its kernels read, and a stand-alone CPU program can include it alone
// (tests/test_fe_host.py builds one under the address sanitizer). The definition is in include/fakepta_amd.h. The noise
// model, its validation and the operator are os_host.h's: the frequency grid is appended to the noise model as a common
// achromatic target component with phi = 0, for which build_operator takes the projection form W^(1/2) (I - Q1 Q1^T)
// W^(1/2) F_k.
#pragma once
#include "lnl_host.h"

namespace fpta_fe {

constexpr int32_t kMaxComp = 7;      // Gaussian-process components of the noise model
constexpr int32_t kMaxFreq = 256;    // gravitational-wave frequencies, G
constexpr int32_t kMaxSky = 12288;   // directions, n_sky (nside 32)
constexpr int32_t kMaxPsr = 256;     // pulsars: k_fe_sky keeps the X tile of all of them in 64 KB of LDS
constexpr int32_t kPoolMax = 16;     // planner threads, at most
constexpr double kRcondFe = 1e-10;   // the default of rcond_fe
using fpta_fit::kTwoPi;

inline long double rcond_fe_of(double rcond_fe) {
  return rcond_fe > 0.0 && std::isfinite(rcond_fe) ? (long double)rcond_fe : (long double)kRcondFe;
}

// The inputs beyond the noise model: the frequencies fgw [n_f], the directions sky [n_sky][2] = (cos theta, phi) and
// the pulsars' unit vectors pos [n_psr][3]
struct Grid {
  int64_t n_f = 0;
  const double* fgw = nullptr;
  int64_t n_sky = 0;
  const double* sky = nullptr;
  const double* pos = nullptr;
};

// Entry (i, j), i <= j, of a symmetric 4 x 4 matrix in the 10 numbers of its upper triangle, row by row
inline int32_t tri4(int32_t i, int32_t j) { return i * 4 - i * (i - 1) / 2 + (j - i); }

// What the entry points refuse about the grid, naming the frequency, direction or pulsar
inline bool validate_grid(int64_t n_psr, const Grid& g, std::string& why) {
  if (n_psr > kMaxPsr) {
    why = "n_psr " + std::to_string(n_psr) + ": more than " + std::to_string(kMaxPsr) + " pulsars";
    return false;
  }
  if (g.n_f < 1 || g.n_f > kMaxFreq) {
    why = std::to_string(g.n_f) + " frequencies outside [1, " + std::to_string(kMaxFreq) + "]";
    return false;
  }
  if (g.n_sky < 1 || g.n_sky > kMaxSky) {
    why = std::to_string(g.n_sky) + " directions outside [1, " + std::to_string(kMaxSky) + "]";
    return false;
  }
  if (!g.fgw || !g.sky || (n_psr > 0 && !g.pos)) {
    why = "frequencies, directions or pulsar positions missing";
    return false;
  }
  for (int64_t k = 0; k < g.n_f; ++k)
    if (!(g.fgw[k] > 0.0 && std::isfinite(g.fgw[k]))) {
      why = "frequency " + std::to_string(k) + ": not positive and finite";
      return false;
    }
  for (int64_t s = 0; s < g.n_sky; ++s) {
    const double ct = g.sky[2 * s], ph = g.sky[2 * s + 1];
    if (!(ct >= -1.0 && ct <= 1.0)) {
      why = "direction " + std::to_string(s) + ": cos_gwtheta outside [-1, 1]";
      return false;
    }
    if (!std::isfinite(ph)) {
      why = "direction " + std::to_string(s) + ": gwphi is not finite";
      return false;
    }
  }
  for (int64_t p = 0; p < n_psr; ++p) {
    const double x = g.pos[3 * p], y = g.pos[3 * p + 1], z = g.pos[3 * p + 2], n2 = x * x + y * y + z * z;
    if (!(std::isfinite(n2) && std::fabs(n2 - 1.0) <= 1e-6)) {
      why = "pulsar " + std::to_string(p) + ": position is not a unit vector";
      return false;
    }
  }
  return true;
}

// F+ and Fx of the pulsar at unit vector (px, py, pz) for the direction (cos theta, phi), cw_device.h's cw_pair in long
// double. False when 1 + omhat . p is zero or a value is not finite (the pulsar lies exactly where the wave goes).
inline bool antenna(double cth_d, double phi_d, double px, double py, double pz, long double& fplus,
                    long double& fcross) {
  const long double cth = (long double)cth_d, sth = std::sqrt(1.0L - cth * cth);
  const long double cph = std::cos((long double)phi_d), sph = std::sin((long double)phi_d);
  const long double x = (long double)px, y = (long double)py, z = (long double)pz;
  const long double mp = sph * x - cph * y;
  const long double nq = -cth * cph * x - cth * sph * y + sth * z;
  const long double op = -sth * cph * x - sth * sph * y - cth * z;
  const long double den = 1.0L + op;
  fplus = fcross = 0.0L;
  if (!(den != 0.0L) || !std::isfinite(den)) return false;
  fplus = 0.5L * (mp * mp - nq * nq) / den;
  fcross = (mp * nq) / den;
  if (!std::isfinite(fplus) || !std::isfinite(fcross)) {
    fplus = fcross = 0.0L;
    return false;
  }
  return true;
}

// The inverse of a symmetric n x n matrix A (row-major, both triangles given) by the definition's rule: scaled to unit
// diagonal, Cholesky, L^-1 by forward substitution, A^-1 = D^-1/2 L^-T L^-1 D^-1/2; sums in index order. False (the
// point is singular) for a diagonal that is not positive and finite, an entry that is not finite, or a pivot (the
// diagonal of the scaled Schur complement, before its square root) <= rc.
template <int n>
inline bool inverse_spd(const long double* A, long double rc, long double* inv) {
  long double d[n], S[n][n], L[n][n] = {}, Li[n][n] = {};
  for (int i = 0; i < n; ++i) {
    if (!(A[i * n + i] > 0.0L) || !std::isfinite(A[i * n + i])) return false;
    d[i] = 1.0L / std::sqrt(A[i * n + i]);
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      if (!std::isfinite(A[i * n + j])) return false;
      S[i][j] = i == j ? 1.0L : d[i] * A[i * n + j] * d[j];
    }
  for (int j = 0; j < n; ++j) {
    long double piv = S[j][j];
    for (int l = 0; l < j; ++l) piv -= L[j][l] * L[j][l];
    if (!(piv > rc)) return false;
    L[j][j] = std::sqrt(piv);
    for (int i = j + 1; i < n; ++i) {
      long double a = S[i][j];
      for (int l = 0; l < j; ++l) a -= L[i][l] * L[j][l];
      L[i][j] = a / L[j][j];
    }
  }
  for (int j = 0; j < n; ++j) {
    Li[j][j] = 1.0L / L[j][j];
    for (int i = j + 1; i < n; ++i) {
      long double a = 0.0L;
      for (int l = j; l < i; ++l) a += L[i][l] * Li[l][j];
      Li[i][j] = -a / L[i][i];
    }
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      long double a = 0.0L;
      for (int l = std::max(i, j); l < n; ++l) a += Li[l][i] * Li[l][j];
      inv[i * n + j] = d[i] * a * d[j];
    }
  return true;
}

// The tables of a whole array as the kernels and the callers read them
struct Plan {
  int32_t G = 0, K = 0, n_sky = 0;
  std::vector<double> B;        // pulsar p's operator [K][n_p] starts at K offs[p]: rows g the cosines, G + g the sines
  std::vector<int32_t> rows;    // [n_psr] K for a pulsar with TOAs, else 0 (k_fit_apply's count of rows to make)
  std::vector<int32_t> rank;    // [n_psr] kept columns of M
  std::vector<double> F;        // [2 n_sky][n_psr]: row 2 s F+, row 2 s + 1 Fx; 0 where antenna() fails
  std::vector<double> M, Minv;  // [n_sky][G][10] upper triangles (tri4); Minv NaN at a singular point
  std::vector<double> m, minv;  // [n_psr][G][3] = (s|s), (s|c), (c|c) and the inverse's; minv 0 for a singular m_pg
  std::vector<int32_t> n_eff;   // [G] pulsars with a regular m_pg
  int32_t max_rows = 0;
};

// Validates, then builds every table. 0: done. 1: refused, the reason in why. 2: the tables' memory could not be had,
// the size in why. comps, phi [n_psr][sum N_c], mask: the noise model as os_host.h takes it (n_comp 0 .. 7). The plan
// is unspecified unless 0 comes back.
inline int make_plan(int64_t n_psr, const int64_t* offs, const double* toas, const double* nu,
                     const fpta_fit::Spec& comps, const double* phi, const uint8_t* mask, const Grid& grid,
                     int64_t n_col, const double* M, const int32_t* ncol_psr, const double* weights, double rcond,
                     double rcond_fe, Plan& plan, std::string& why) {
  if (n_psr < 0 || (n_psr > 0 && !offs)) {
    why = "bad pulsar table";
    return 1;
  }
  if (!validate_grid(n_psr, grid, why)) return 1;
  const int32_t C = comps.n_comp;
  if (C < 0 || C > kMaxComp) {
    why = std::to_string(C) + " components outside [0, " + std::to_string(kMaxComp) + "]";
    return 1;
  }
  const int64_t n_toa = n_psr > 0 ? offs[n_psr] : 0, G = grid.n_f, K = 2 * G, S = grid.n_sky;
  const long double rc = rcond_fe_of(rcond_fe), rc_tm = fpta_tm::rcond_of(rcond);
  double bytes = 0.0;
  try {
    // the noise model with the frequency grid appended as the target: common, achromatic, phi = 0, acting everywhere
    int64_t nf0 = 0;
    for (int32_t c = 0; c < C; ++c) {
      if (!comps.n_modes || comps.n_modes[c] < 0) break;  // the shared validation names it
      nf0 += comps.n_modes[c];
    }
    const int64_t nf = nf0 + G;
    const bool common = C == 0 || comps.f_is_common;
    const int64_t f_rows = common ? 1 : n_psr;
    bytes = 8.0 * ((double)K * (double)n_toa + (double)f_rows * (double)nf + (double)n_psr * (double)nf +
                   2.0 * (double)S * (double)n_psr + 20.0 * (double)S * (double)G + 6.0 * (double)n_psr * (double)G) +
            (mask ? (double)(C + 1) * (double)n_toa : 0.0);
    std::vector<int32_t> nm((size_t)C + 1);
    std::vector<double> idx((size_t)C + 1, 0.0), ff((size_t)C + 1, 1400.0), f((size_t)(f_rows * nf)),
        ph((size_t)(n_psr * nf), 0.0);
    for (int32_t c = 0; c < C; ++c) {
      nm[(size_t)c] = comps.n_modes ? comps.n_modes[c] : 0;
      if (comps.idx) idx[(size_t)c] = comps.idx[c];
      if (comps.freqf) ff[(size_t)c] = comps.freqf[c];
    }
    nm[(size_t)C] = (int32_t)G;
    if (C > 0 && (!comps.f || !phi || !comps.idx || !comps.freqf || !comps.n_modes)) {
      why = "noise-model tables missing";
      return 1;
    }
    for (int64_t r = 0; r < f_rows; ++r) {
      if (nf0) std::copy(comps.f + r * nf0, comps.f + (r + 1) * nf0, f.begin() + r * nf);
      std::copy(grid.fgw, grid.fgw + G, f.begin() + r * nf + nf0);
    }
    for (int64_t p = 0; p < n_psr && nf0; ++p) std::copy(phi + p * nf0, phi + (p + 1) * nf0, ph.begin() + p * nf);
    std::vector<uint8_t> mk;
    if (mask) {
      mk.assign((size_t)((C + 1) * n_toa), 1);
      std::copy(mask, mask + (int64_t)C * n_toa, mk.begin());
    }
    const fpta_os::Spec sp = fpta_os::make_spec(
        fpta_fit::make_spec(C + 1, nm.data(), f.data(), common ? 1 : 0, idx.data(), ff.data()), ph.data(),
        mask ? mk.data() : nullptr, C);
    {
      const std::vector<double> ones((size_t)G, 1.0);
      fpta_os::Spec s = sp;
      s.phi_hat = ones.data();
      if (!fpta_os::validate(n_psr, offs, toas, nu, s, n_col, M, ncol_psr, weights, 0, nullptr, why)) return 1;
    }
    plan.G = (int32_t)G;
    plan.K = (int32_t)K;
    plan.n_sky = (int32_t)S;
    plan.max_rows = 0;
    plan.B.assign((size_t)K * (size_t)n_toa, 0.0);
    plan.rows.assign((size_t)n_psr, 0);
    plan.rank.assign((size_t)n_psr, 0);
    plan.F.assign((size_t)(2 * S * n_psr), 0.0);
    plan.M.assign((size_t)(S * G * 10), 0.0);
    plan.Minv.assign((size_t)(S * G * 10), 0.0);
    plan.m.assign((size_t)(n_psr * G * 3), 0.0);
    plan.minv.assign((size_t)(n_psr * G * 3), 0.0);
    plan.n_eff.assign((size_t)G, 0);
    std::vector<long double> m_ld((size_t)(n_psr * G * 3), 0.0L);
    std::vector<uint8_t> counted((size_t)(n_psr * G), 0);
    const unsigned hw = std::thread::hardware_concurrency();
    const int64_t cap = std::min<int64_t>((int64_t)(hw ? hw : 1), kPoolMax);
    // the operators and m_pg: the pulsars are independent and write disjoint parts of the plan
    const int64_t work_op = (2 * nf) * (2 * nf) * n_toa;
    bool no_mem = fpta_os::run_pool(n_psr, std::min<int64_t>({cap, work_op >> 24, n_psr}), [&](int64_t p) {
      const int64_t o = offs[p], n = offs[p + 1] - o;
      const int32_t mc = ncol_psr ? ncol_psr[p] : (int32_t)n_col;
      if (n == 0) return;  // X = 0 and m_pg = 0: singular at every frequency
      plan.rows[(size_t)p] = plan.K;
      const double* fp = f.data() + (common ? 0 : p * nf);
      const uint8_t* mp = mask ? mk.data() + o : nullptr;
      std::vector<double> Zd((size_t)(K * K));
      std::vector<long double> Bl((size_t)K * (size_t)n), cg((size_t)n), sg((size_t)n);
      plan.rank[(size_t)p] = fpta_os::build_operator(n, toas + o, nu + o, mc, M ? M + o * n_col : nullptr, n_col,
                                                     weights ? weights + o : nullptr, sp, fp, ph.data() + p * nf, mp,
                                                     n_toa, rcond, plan.B.data() + K * o, Zd.data(), nullptr,
                                                     Bl.data());
      for (int64_t g = 0; g < G; ++g) {
        fpta_lnl::target_column(n, toas + o, nu + o, sp, fp, mp, n_toa, (int32_t)g, cg.data());
        fpta_lnl::target_column(n, toas + o, nu + o, sp, fp, mp, n_toa, (int32_t)(G + g), sg.data());
        const long double* bc = Bl.data() + (size_t)g * (size_t)n;
        const long double* bs = Bl.data() + (size_t)(G + g) * (size_t)n;
        long double ss = 0.0L, sc = 0.0L, cc = 0.0L, sws = 0.0L, cwc = 0.0L;
        for (int64_t i = 0; i < n; ++i) ss += bs[i] * sg[(size_t)i];
        for (int64_t i = 0; i < n; ++i) sc += bs[i] * cg[(size_t)i];
        for (int64_t i = 0; i < n; ++i) cc += bc[i] * cg[(size_t)i];
        const double* wp = weights ? weights + o : nullptr;
        for (int64_t i = 0; i < n; ++i) sws += (wp ? (long double)wp[i] : 1.0L) * sg[(size_t)i] * sg[(size_t)i];
        for (int64_t i = 0; i < n; ++i) cwc += (wp ? (long double)wp[i] : 1.0L) * cg[(size_t)i] * cg[(size_t)i];
        // (x|x) = |W^(1/2) x projected|^2: at or below rcond^2 x^T W x the column lies in the span of the marginalised
        // model by the rank rule's own threshold, and the pulsar drops out at this frequency (rows of B and m_pg zero)
        if (!(ss > rc_tm * rc_tm * sws) || !(cc > rc_tm * rc_tm * cwc)) {
          double* Bp = plan.B.data() + K * o;
          std::fill(Bp + g * n, Bp + (g + 1) * n, 0.0);
          std::fill(Bp + (G + g) * n, Bp + (G + g + 1) * n, 0.0);
          continue;
        }
        long double* ml = m_ld.data() + (p * G + g) * 3;
        ml[0] = ss;
        ml[1] = sc;
        ml[2] = cc;
        const long double A2[4] = {ss, sc, sc, cc};
        long double inv[4];
        double* md = plan.m.data() + (p * G + g) * 3;
        md[0] = (double)ss;
        md[1] = (double)sc;
        md[2] = (double)cc;
        if (inverse_spd<2>(A2, rc, inv)) {
          double* mi = plan.minv.data() + (p * G + g) * 3;
          mi[0] = (double)inv[0];
          mi[1] = (double)inv[1];
          mi[2] = (double)inv[3];
          counted[(size_t)(p * G + g)] = 1;
        }
      }
    });
    if (no_mem) throw std::bad_alloc();
    for (int64_t g = 0; g < G; ++g)
      for (int64_t p = 0; p < n_psr; ++p) plan.n_eff[(size_t)g] += counted[(size_t)(p * G + g)];
    // the directions: the antenna table, then M and its inverse at every frequency
    const int64_t work_s = S * G * std::max<int64_t>(n_psr, 1) * 16;
    no_mem = fpta_os::run_pool(S, std::min<int64_t>({cap, std::max<int64_t>(work_s >> 22, 1), S}), [&](int64_t s) {
      std::vector<long double> a((size_t)(3 * std::max<int64_t>(n_psr, 1)));  // F+^2, F+ Fx, Fx^2 per pulsar
      bool regular = true;
      for (int64_t p = 0; p < n_psr; ++p) {
        long double fpl, fcr;
        if (!antenna(grid.sky[2 * s], grid.sky[2 * s + 1], grid.pos[3 * p], grid.pos[3 * p + 1], grid.pos[3 * p + 2],
                     fpl, fcr))
          regular = false;
        plan.F[(size_t)((2 * s) * n_psr + p)] = (double)fpl;
        plan.F[(size_t)((2 * s + 1) * n_psr + p)] = (double)fcr;
        a[(size_t)(3 * p)] = fpl * fpl;
        a[(size_t)(3 * p + 1)] = fpl * fcr;
        a[(size_t)(3 * p + 2)] = fcr * fcr;
      }
      const double nan = std::nan("");
      for (int64_t g = 0; g < G; ++g) {
        // M = sum_p [[F+^2, F+ Fx], [F+ Fx, Fx^2]] (x) [[ss, sc], [sc, cc]] in pulsar order
        long double A4[16] = {};
        for (int64_t p = 0; p < n_psr; ++p) {
          const long double* ml = m_ld.data() + (p * G + g) * 3;
          const long double blk[2][2] = {{ml[0], ml[1]}, {ml[1], ml[2]}};
          const long double* ap = a.data() + 3 * p;
          const long double pol[2][2] = {{ap[0], ap[1]}, {ap[1], ap[2]}};
          for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) A4[i * 4 + j] += pol[i >> 1][j >> 1] * blk[i & 1][j & 1];
        }
        long double inv[16];
        const bool ok = regular && inverse_spd<4>(A4, rc, inv);
        double* Md = plan.M.data() + (s * G + g) * 10;
        double* Mi = plan.Minv.data() + (s * G + g) * 10;
        for (int i = 0; i < 4; ++i)
          for (int j = i; j < 4; ++j) {
            Md[tri4(i, j)] = (double)A4[i * 4 + j];
            Mi[tri4(i, j)] = ok ? (double)inv[i * 4 + j] : nan;
          }
      }
    });
    if (no_mem) throw std::bad_alloc();
    for (int64_t p = 0; p < n_psr; ++p) plan.max_rows = std::max(plan.max_rows, plan.rows[(size_t)p]);
  } catch (const std::bad_alloc&) {
    why = "no host memory for the tables of " + std::to_string(bytes) + " bytes (operator 8 K n_toa, K = " +
          std::to_string(K) + ", n_toa = " + std::to_string(n_toa) + ", n_sky = " + std::to_string(S) + ")";
    return 2;
  }
  return 0;
}

}  // namespace fpta_fe
