// Continuous-wave source (circular binary, evolving frequency): per-source constants and input validation of
// fpta_cw_accumulate, on the host in plain C++. No HIP here: cw.hip includes it for the tables its kernels read, and a
// stand-alone CPU program can include it alone (tests/test_cw_host.py builds one under the address sanitizer).
//
// With mc = 10^log10_mc Tsun, w0 = pi 10^log10_fgw, u(x) = 1 - K x and l = log1p(-K x):
//   omega(x) = w0 u^(-3/8)
//   phase(x) = phase0 / 2 + (w0^(-5/3) - omega^(-5/3)) / (32 mc^(5/3)) = phase0 / 2 - C expm1(5/8 l)
//   alpha(x) = mc^(5/3) / (dist omega^(1/3))                           = a0 exp(1/8 l)
// (the expm1 form has no cancellation: the two terms of the literal phase are ~1e7 rad each for a 1e8 Msun, 3 nHz
// source and differ by a few rad). The polarisation and inclination enter only through four coefficients:
//   rplus  = alpha (Ps sin 2 phase + Pc cos 2 phase)     Ps =  (1 + cos_inc^2) cos 2 psi   Pc = 2 cos_inc sin 2 psi
//   rcross = alpha (Xs sin 2 phase + Xc cos 2 phase)     Xs = -(1 + cos_inc^2) sin 2 psi   Xc = 2 cos_inc cos 2 psi
#pragma once
#include <cmath>
#include <cstdint>
#include <string>

namespace fpta_cw {

constexpr int kNPar = 9;  // FPTA_CW_NPAR: cos_gwtheta, gwphi, cos_inc, log10_mc, log10_fgw, log10_h, phase0, psi, psrterm
constexpr long double kPiL = 3.14159265358979323846264338327950288L;
constexpr long double kLog2Of10L = 3.32192809488736234787031942948939018L;
constexpr long double kTsunL = 1.327124400e20L / (299792458.0L * 299792458.0L * 299792458.0L);  // GMsun / c^3, s

// What the main kernel reads per source (block-uniform, 32 bytes).
struct SrcEval {
  double K;      // 256/5 mc^(5/3) w0^(8/3): u(x) = 1 - K x
  double C;      // w0^(-5/3) / (32 mc^(5/3))
  double hp0;    // phase0 / 2
  double pterm;  // 1.0 with the pulsar term, else 0.0
};

// What the prep kernel reads per source: sky angles and the folded coefficients, the amplitude a0 included.
struct SrcGeom {
  double sth, cth, sph, cph;  // sin / cos of gwtheta = arccos(cos_gwtheta) and of gwphi
  double Ps, Pc, Xs, Xc;      // a0 x the coefficients above
};

struct SrcConst {
  SrcEval e;
  SrcGeom g;
  double a0;  // mc^(5/3) / (dist w0^(1/3)) with dist = 2 mc^(5/3) w0^(2/3) / h, i.e. h / (2 w0)
};

// Constants of source `par` [kNPar]. False (and why) for a non-finite parameter or a cosine outside [-1, 1].
inline bool source_constants(const double* par, SrcConst& out, std::string& why) {
  static const char* const names[kNPar] = {"cos_gwtheta", "gwphi", "cos_inc", "log10_mc", "log10_fgw",
                                           "log10_h",     "phase0", "psi",    "psrterm"};
  for (int i = 0; i < kNPar; ++i)
    if (!std::isfinite(par[i])) {
      why = std::string("non-finite ") + names[i];
      return false;
    }
  if (std::fabs(par[0]) > 1.0) {
    why = "|cos_gwtheta| > 1";
    return false;
  }
  if (std::fabs(par[2]) > 1.0) {
    why = "|cos_inc| > 1";
    return false;
  }
  // in long double, rounded once: the fractional powers amplify an fp64 rounding of mc or w0 by their exponents, and
  // the phase is C times a number of order K t, hundreds to 1e4 rad, so a few ulp of K or C would be most of the error
  // (two long double exp2 per source and products: exp2l is ~6x cheaper than powl, and these are most of the call's
  // host time for a large population)
  typedef long double ld;
  static const ld tsun53 = std::pow(kTsunL, (ld)5 / 3), pi13 = std::cbrt(kPiL);
  const ld mc53 = std::exp2((ld)par[3] * 5 / 3 * kLog2Of10L) * tsun53;  // mc^(5/3)
  const ld w13 = pi13 * std::exp2((ld)par[4] / 3 * kLog2Of10L);       // w0^(1/3)
  const ld w23 = w13 * w13, w0 = w23 * w13, w53 = w0 * w23;
  out.e.K = (double)((ld)256 / 5 * mc53 * (w53 * w0));
  out.e.C = (double)(1 / (32 * mc53 * w53));
  out.e.hp0 = 0.5 * par[6];
  out.e.pterm = par[8] != 0.0 ? 1.0 : 0.0;
  out.a0 = (double)(std::pow(10.0, par[5]) / (2 * w0));
  if (!std::isfinite(out.e.K) || !std::isfinite(out.e.C) || !std::isfinite(out.a0)) {
    why = "mass / frequency / strain out of the fp64 range";
    return false;
  }
  const double cth = par[0], ci = par[2];
  out.g.cth = cth;
  out.g.sth = std::sqrt((1.0 - cth) * (1.0 + cth));
  out.g.sph = std::sin(par[1]);
  out.g.cph = std::cos(par[1]);
  const double a = 1.0 + ci * ci, b = 2.0 * ci;
  const double s2 = std::sin(2.0 * par[7]), c2 = std::cos(2.0 * par[7]);
  out.g.Ps = out.a0 * a * c2;
  out.g.Pc = out.a0 * b * s2;
  out.g.Xs = -out.a0 * a * s2;
  out.g.Xc = out.a0 * b * c2;
  return true;
}

// Validates n_src sources against the latest TOA of any pulsar (tmax) and fills ev / gm [n_src]. Returns -1 when all
// are fine, else the index of the first bad source with the reason in `why`. K tmax >= 1: the binary coalesces inside
// the data span, where the waveform is not defined (u <= 0).
inline int64_t validate_sources(int64_t n_src, const double* src, double tmax, SrcEval* ev, SrcGeom* gm,
                                std::string& why) {
  for (int64_t s = 0; s < n_src; ++s) {
    SrcConst k;
    if (!source_constants(src + s * kNPar, k, why)) return s;
    if (!(k.e.K * tmax < 1.0)) {
      why = "coalesces inside the data span (K max(t) >= 1)";
      return s;
    }
    if (ev) ev[s] = k.e;
    if (gm) gm[s] = k.g;
  }
  return -1;
}

// Source splits of one call: a pure function of (n_src, n_toa, option), so identical calls sum in the same order.
// One wave evaluates 64 TOAs; below kFillWaves waves the source range is split until about kTargetWaves waves exist,
// each split keeping at least kMinSrcPerSplit sources.
constexpr int64_t kFillWaves = 2048, kTargetWaves = 4096, kMinSrcPerSplit = 32;
inline int32_t split_count(int64_t n_src, int64_t n_toa, int64_t option) {
  if (n_src <= 0) return 1;
  int64_t n = 1;
  if (option >= 1) {
    n = option;
  } else {
    const int64_t waves = (n_toa + 63) / 64;
    if (waves < kFillWaves) n = (kTargetWaves + waves - 1) / (waves > 0 ? waves : 1);
    const int64_t cap = n_src / kMinSrcPerSplit;
    if (n > cap) n = cap;
  }
  if (n > n_src) n = n_src;
  if (n > 65535) n = 65535;
  return (int32_t)(n < 1 ? 1 : n);
}

}  // namespace fpta_cw
