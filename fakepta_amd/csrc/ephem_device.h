// Device arithmetic of a Keplerian orbit with linearly drifting elements, shared by ephem.hip (fpta_ephem_kepler,
// fpta_ephem_orbits, fpta_roemer_accumulate) and roemer_batch.hip (fpta_batch_roemer_accumulate): one definition of
// the Kepler solve, the position in the plane, the century count and the equatorial position, so that both paths
// round every intermediate the same way and a realization of a batch block gets, bit for bit, what the drop-in call
// adds to a zero vector (tests/test_gpu_roemer_batch.py).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "ephem_host.h"

struct fpta_ctx;

namespace __attribute__((visibility("hidden"))) capi {

using fpta_ephem::Body;
using fpta_ephem::RoemerRow;

// One 64-TOA wave of k_roemer_main
struct EphWave {
  int64_t first;  // first TOA (index into the concatenated arrays)
  int32_t psr;
  int32_t count;  // 1 .. 64
};

constexpr int kEphWave = 64;
constexpr double kDegToRad = fpta_ephem::kPi / 180.0;
constexpr double kAuOverC = fpta_ephem::kAU / fpta_ephem::kC;  // light-seconds per AU

struct Vec3 {
  double x, y, z;
};

// E - e sin E = M for M in [0, 2 pi) and 0 <= e <= kEMax: Newton with the analytic derivative. From pi the iterates
// are monotone for every e < 1 (the function is convex below pi and concave above); M + e sin M is closer at low e.
// The cap is never reached: tests/ephem_reference.py kepler_newton is this loop in numpy.
__device__ __forceinline__ double kepler_solve(double M, double e) {
  double E = e < fpta_ephem::kLowE ? M + e * sin(M) : fpta_ephem::kPi;
  for (int it = 0; it < fpta_ephem::kKeplerMaxIter; ++it) {
    double sn, cs;
    sincos(E, &sn, &cs);
    const double dE = ((E - e * sn) - M) / (1.0 - e * cs);
    E -= dE;
    if (fabs(dE) <= fpta_ephem::kKeplerTol) break;
  }
  return E;
}

// Position in the orbital plane. x is the reference's a cos(E - e), not the textbook a (cos E - e): kept so that
// seeded scripts reproduce. This is the one place to change it.
__device__ __forceinline__ void orbit_in_plane(double a_s, double e, double E, double& x, double& y) {
  x = a_s * cos(E - e);
  y = a_s * sqrt((1.0 - e) * (1.0 + e)) * sin(E);
}

// Julian centuries from J2000: (toa / 86400 - 51544.5) / 36525 with the rounding of the first quotient carried along
// (the subtraction of 51544.5 is exact for any MJD of this or the last century)
__device__ __forceinline__ double centuries(double toa) {
  const double d = toa / 86400.0;
  const double r = fma(-d, 86400.0, toa);
  return ((d - fpta_ephem::kMjdJ2000) + r * (1.0 / 86400.0)) / 36525.0;
}

// Equatorial position [light-seconds] of body b at t centuries; (se, ce) the obliquity's sine and cosine.
__device__ __forceinline__ Vec3 orbit_eq(const Body& b, double t, double se, double ce) {
  const double inc = fma(b.inc_rate, t, b.inc), Om = fma(b.Om_rate, t, b.Om), omega = fma(b.omega_rate, t, b.omega);
  const double a_s = fma(b.a_rate, t, b.a) * kAuOverC;
  const double e = fma(b.e_rate, t, b.e), l0 = fma(b.l0_rate, t, b.l0);
  // mean anomaly: reduced in degrees, where the reduction is exact
  double md = l0 - omega;
  md = fma(-floor(md / 360.0), 360.0, md);
  if (md < 0.0) md += 360.0;
  if (md >= 360.0) md -= 360.0;
  const double E = kepler_solve(md * kDegToRad, e);
  double x, y;
  orbit_in_plane(a_s, e, E, x, y);
  // the first two columns of the (Om, omega - Om, inc) rotation: z is 0 in the plane
  double sO, cO, sw, cw, si, ci;
  sincos(Om * kDegToRad, &sO, &cO);
  sincos((omega - Om) * kDegToRad, &sw, &cw);
  sincos(inc * kDegToRad, &si, &ci);
  const double X = (cO * cw - sO * ci * sw) * x + (-cO * sw - sO * ci * cw) * y;
  const double Y = (sO * cw + cO * ci * sw) * x + (-sO * sw + cO * ci * cw) * y;
  const double Z = si * sw * x + si * cw * y;
  return {X, ce * Y - se * Z, se * Y + ce * Z};  // ecliptic -> equatorial
}

// ephem.hip: the device part of a summed fpta_roemer_accumulate on a vector that is on the device already,
// dst [n_toa] += sign * sum of the rows' delays (k_roemer_main<false>). It uploads pos and the rows and fills and
// uploads `waves`, which must live until the stream has run; toas and dst are device pointers. No timer, no sync.
int roemer_sum_launch(fpta_ctx* c, int32_t n_psr, const int64_t* offs, const double* toas, const double* pos,
                      const std::vector<RoemerRow>& rows, double sign, int64_t n_toa, std::vector<EphWave>& waves,
                      double* dst);

}  // namespace capi
