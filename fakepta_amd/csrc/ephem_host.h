// Solar-system ephemeris (Keplerian orbits with linear elements) and Roemer delay: table layouts, constants and input
// validation of fpta_ephem_kepler / fpta_ephem_orbits / fpta_roemer_accumulate, on the host in plain C++. No HIP here:
// ephem.hip includes it for the tables its kernels read, and a stand-alone CPU program can include it alone
// (tests/test_ephem_host.py builds one under the address sanitizer). The definition is in include/fakepta_amd.h.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>

namespace fpta_ephem {

// A body as the C entry points take it (FPTA_EPHEM_NBODY doubles) and as the kernels read it: the mass, the period in
// days, then (value, rate per Julian century) of six elements; angles in degrees, a in AU.
struct Body {
  double mass, T;
  double inc, inc_rate, Om, Om_rate, omega, omega_rate, a, a_rate, e, e_rate, l0, l0_rate;
};
constexpr int kNBody = 14;  // FPTA_EPHEM_NBODY
constexpr int kNRow = 22;   // FPTA_ROEMER_NPAR: a body, d_mass d_Om d_omega d_inc d_a d_e d_l0, 1 / mass_ss
static_assert(sizeof(Body) == kNBody * sizeof(double), "Body is the ABI row");

// What k_roemer_main reads per row (wave-uniform).
struct RoemerRow {
  Body base;       // the stored elements, a resolved
  Body pert;       // base with the six element deviations added to the values
  double mass_w;   // mass / mass_ss
  double dmass_w;  // d_mass / mass_ss
  double same;     // 1.0 when all six element deviations are exactly 0: one orbit evaluation serves both terms
  double pad;
};

constexpr double kEMax = 0.95;     // FPTA_EPHEM_E_MAX: largest admitted eccentricity
constexpr double kLowE = 0.5;      // Kepler start: M + e sin M below, pi from here on
constexpr double kKeplerTol = 1e-10;
constexpr int kKeplerMaxIter = 12;  // never reached for e <= kEMax: tests/ephem_reference.py kepler_newton, swept on the CPU

constexpr double kPi = 3.14159265358979323846;
constexpr long double kPiL = 3.14159265358979323846264338327950288L;
constexpr double kGMsun = 1.327124400e20;  // m^3 / s^2
constexpr double kG = 6.6743e-11;          // CODATA 2018 / 2022
constexpr double kMsun = kGMsun / kG;      // FPTA_EPHEM_MSUN [kg]
constexpr double kAU = 149597870700.0, kC = 299792458.0, kDay = 86400.0;
constexpr double kObliquityDeg = 23.43928;
constexpr double kMjdJ2000 = 51544.5;

// sine and cosine of the obliquity, rounded once from long double
struct Obliquity {
  double sn, cs;
};
inline Obliquity obliquity() {
  const long double ec = (long double)kObliquityDeg * kPiL / 180.0L;
  return {(double)std::sin(ec), (double)std::cos(ec)};
}

// Julian centuries from J2000 of a TOA in MJD seconds (the validation's copy; the kernels carry the rounding of
// toa / 86400 along, ephem.hip centuries)
inline double centuries(double toa) { return (toa / kDay - kMjdJ2000) / 36525.0; }

// What a = None stands for: the semi-major axis [AU] of period T [days] around the Sun
inline double kepler_a_au(double T) {
  const double ts = T * kDay;
  return std::cbrt(kGMsun * ts * ts / (4.0 * kPi * kPi)) / kAU;
}

// [t0, t1] in centuries of n TOAs; false for a non-finite TOA (its index in bad). n == 0 gives [0, 0].
inline bool toa_span(int64_t n, const double* toas, double& t0, double& t1, int64_t& bad) {
  double lo = 0.0, hi = 0.0;
  for (int64_t i = 0; i < n; ++i) {
    if (!std::isfinite(toas[i])) {
      bad = i;
      return false;
    }
    lo = i ? std::fmin(lo, toas[i]) : toas[i];
    hi = i ? std::fmax(hi, toas[i]) : toas[i];
  }
  t0 = n ? centuries(lo) : 0.0;
  t1 = n ? centuries(hi) : 0.0;
  return true;
}

// The elements are linear in t, so a bound that holds at both ends of the span holds inside.
inline bool check_span(const Body& b, double t0, double t1, std::string& why) {
  for (const double t : {t0, t1}) {
    const double e = b.e + b.e_rate * t, a = b.a + b.a_rate * t;
    if (!(e >= 0.0 && e <= kEMax)) {
      why = "eccentricity " + std::to_string(e) + " outside [0, " + std::to_string(kEMax) + "] inside the TOA span";
      return false;
    }
    if (!(a > 0.0)) {
      why = "semi-major axis <= 0 inside the TOA span";
      return false;
    }
  }
  return true;
}

// Body `in` [kNBody] -> out with a = None (value 0 and rate 0) resolved. False (and why) for a non-finite value or an
// a = None body without a positive period.
inline bool resolve_body(const double* in, Body& out, std::string& why) {
  static const char* const names[kNBody] = {"mass", "T", "inc", "inc rate", "Om", "Om rate", "omega", "omega rate",
                                            "a", "a rate", "e", "e rate", "l0", "l0 rate"};
  for (int i = 0; i < kNBody; ++i)
    if (!std::isfinite(in[i])) {
      why = std::string("non-finite ") + names[i];
      return false;
    }
  out = {in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7], in[8], in[9], in[10], in[11], in[12], in[13]};
  if (out.a == 0.0 && out.a_rate == 0.0) {
    if (!(out.T > 0.0)) {
      why = "a = None needs a period T > 0";
      return false;
    }
    out.a = kepler_a_au(out.T);
  }
  return true;
}

// Validates n bodies over the span [t0, t1] and fills out [n]. Returns -1, or the index of the first bad body.
inline int64_t validate_bodies(int64_t n, const double* bodies, double t0, double t1, Body* out, std::string& why) {
  for (int64_t b = 0; b < n; ++b) {
    Body r;
    if (!resolve_body(bodies + b * kNBody, r, why) || !check_span(r, t0, t1, why)) return b;
    if (out) out[b] = r;
  }
  return -1;
}

// Validates n Roemer rows over the span and fills out [n]. Returns -1, or the index of the first bad row.
inline int64_t validate_rows(int64_t n, const double* rows, double t0, double t1, RoemerRow* out, std::string& why) {
  static const char* const names[7] = {"d_mass", "d_Om", "d_omega", "d_inc", "d_a", "d_e", "d_l0"};
  for (int64_t r = 0; r < n; ++r) {
    const double* row = rows + r * kNRow;
    const double* d = row + kNBody;
    RoemerRow o;
    if (!resolve_body(row, o.base, why)) return r;
    for (int i = 0; i < 7; ++i)
      if (!std::isfinite(d[i])) {
        why = std::string("non-finite ") + names[i];
        return r;
      }
    const double inv = row[kNRow - 1];
    if (!(inv > 0.0) || !std::isfinite(inv)) {
      why = "mass_ss <= 0 (1 / mass_ss must be positive and finite)";
      return r;
    }
    o.pert = o.base;
    o.pert.Om += d[1];
    o.pert.omega += d[2];
    o.pert.inc += d[3];
    o.pert.a += d[4];
    o.pert.e += d[5];
    o.pert.l0 += d[6];
    o.same = (d[1] == 0.0 && d[2] == 0.0 && d[3] == 0.0 && d[4] == 0.0 && d[5] == 0.0 && d[6] == 0.0) ? 1.0 : 0.0;
    if (!check_span(o.base, t0, t1, why)) return r;
    if (o.same == 0.0 && !check_span(o.pert, t0, t1, why)) {
      why = "with its deviations: " + why;
      return r;
    }
    o.mass_w = o.base.mass * inv;
    o.dmass_w = d[0] * inv;
    o.pad = 0.0;
    if (out) out[r] = o;
  }
  return -1;
}

}  // namespace fpta_ephem
