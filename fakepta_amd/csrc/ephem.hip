// Solar-system ephemeris and Roemer delay (fpta_ephem_kepler, fpta_ephem_orbits, fpta_roemer_accumulate): the
// position of a body on a Keplerian orbit with linearly drifting elements, independently per (TOA, body). Each
// evaluation is a Newton solve of Kepler's equation (a sincos per step), a cos, three more sincos and two rotations:
// fp64 VALU work with nothing to share between samples, like k_cw_main.
//
//   k_ephem_kepler  one lane per (M, e) pair: the Kepler solve alone
//   k_ephem_orbits  one lane per TOA, looping over the body table in order: planetssb [n][n_body][6] (columns 3 .. 5
//                   zero) and / or sunssb [n][3] = -sum_b mass_b / Msun orbit_b, summed in a register per component
//   k_roemer_main   one wave per 64 TOAs of one pulsar, looping over the rows in ascending order: the sum of the
//                   delays into the residuals, or every row's delay into its own output row
// The body and row tables are indexed by wave-uniform values only, so they come through the scalar cache. No LDS, no
// atomics. The orbit arithmetic is ephem_device.h, shared with roemer_batch.hip.
#include "capi_host.h"
#include "ephem_device.h"
#include "ephem_host.h"
#include "device_common.h"

namespace __attribute__((visibility("hidden"))) capi {

__global__ __launch_bounds__(256) void k_ephem_kepler(int64_t n, const double* __restrict__ M,
                                                       const double* __restrict__ e, double* __restrict__ E) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  // whole turns are taken off and put back, so any finite M is served: in [0, 2 pi) nothing changes
  const double twopi = 2.0 * fpta_ephem::kPi, twopi_lo = 2.4492935982947064e-16;
  const double m = M[i], k = floor(m / twopi);
  const double mr = k == 0.0 ? m : fma(-k, twopi_lo, fma(-k, twopi, m));
  E[i] = fma(k, twopi, kepler_solve(mr, e[i]));
}

__global__ __launch_bounds__(kEphWave) void k_ephem_orbits(int64_t n, const double* __restrict__ toas,
                                                           int32_t n_body, const Body* __restrict__ bodies,
                                                           double se, double ce, double inv_msun,
                                                           double* __restrict__ pssb, double* __restrict__ sun) {
  const int64_t i = (int64_t)blockIdx.x * kEphWave + threadIdx.x;
  if (i >= n) return;
  const double t = centuries(toas[i]);
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int32_t b = 0; b < n_body; ++b) {
    const Body body = bodies[b];
    const Vec3 o = orbit_eq(body, t, se, ce);
    if (pssb) {
      double* __restrict__ q = pssb + (i * n_body + b) * 6;
      q[0] = o.x;
      q[1] = o.y;
      q[2] = o.z;
      q[3] = 0.0;
      q[4] = 0.0;
      q[5] = 0.0;
    }
    const double w = body.mass * inv_msun;
    sx -= w * o.x;
    sy -= w * o.y;
    sz -= w * o.z;
  }
  if (sun) {
    sun[3 * i] = sx;
    sun[3 * i + 1] = sy;
    sun[3 * i + 2] = sz;
  }
}

// SEPARATE false: dst = the residuals [n_toa], read and written; true: dst = [n_row][n_toa], written
template <bool SEPARATE>
__global__ __launch_bounds__(kEphWave) void k_roemer_main(const EphWave* __restrict__ waves,
                                                          const double* __restrict__ toas,
                                                          const double* __restrict__ pos,
                                                          const RoemerRow* __restrict__ rows, int32_t n_row,
                                                          double se, double ce, double sign, int64_t n_toa,
                                                          double* __restrict__ dst) {
  const EphWave w = waves[blockIdx.x];
  const int32_t lane = min((int32_t)threadIdx.x, w.count - 1);  // spare lanes repeat the last TOA and store nothing
  const bool live = (int32_t)threadIdx.x < w.count;
  const int64_t i = w.first + lane;
  FPTA_DCHECK(i >= 0 && i < n_toa, "k_roemer_main toa", i, n_toa);
  const double t = centuries(toas[i]);
  const double px = pos[3 * w.psr], py = pos[3 * w.psr + 1], pz = pos[3 * w.psr + 2];
  double acc = 0.0;
  for (int32_t r = 0; r < n_row; ++r) {
    const RoemerRow* __restrict__ row = rows + r;
    const Vec3 p = orbit_eq(row->pert, t, se, ce);
    double dx = row->dmass_w * p.x, dy = row->dmass_w * p.y, dz = row->dmass_w * p.z;
    if (row->same == 0.0) {  // wave-uniform
      const Vec3 o = orbit_eq(row->base, t, se, ce);
      const double mw = row->mass_w;
      dx += mw * (p.x - o.x);
      dy += mw * (p.y - o.y);
      dz += mw * (p.z - o.z);
    }
    // explicit fma: the last operation is the same in both modes, whatever the compiler contracts around it
    const double delay = fma(dz, pz, fma(dy, py, dx * px));
    if (SEPARATE) {
      if (live) dst[(int64_t)r * n_toa + i] = sign * delay;
    } else {
      acc += delay;
    }
  }
  if (!SEPARATE && live) dst[i] += sign * acc;
}

// 64-TOA waves of every pulsar, in TOA order; a pulsar without TOAs gets none
static void make_waves(int32_t n_psr, const int64_t* offs, std::vector<EphWave>& waves) {
  waves.clear();
  for (int32_t p = 0; p < n_psr; ++p)
    for (int64_t i = offs[p]; i < offs[p + 1]; i += kEphWave)
      waves.push_back({i, p, (int32_t)std::min<int64_t>(kEphWave, offs[p + 1] - i)});
}

int roemer_sum_launch(fpta_ctx* c, int32_t n_psr, const int64_t* offs, const double* toas, const double* pos,
                      const std::vector<RoemerRow>& rows, double sign, int64_t n_toa, std::vector<EphWave>& waves,
                      double* dst) {
  make_waves(n_psr, offs, waves);
  if (waves.empty() || rows.empty()) return FPTA_OK;
  if (waves.size() > (size_t)0x7FFFFFFF || rows.size() > (size_t)0x7FFFFFFF)
    return fail(c, FPTA_EINVAL, "roemer: too many TOAs or rows");
  const fpta_ephem::Obliquity ob = fpta_ephem::obliquity();
  int rc;
  if ((rc = upload(c, c->eph_pos, pos, sizeof(double) * 3 * (size_t)n_psr, "roemer pos"))) return rc;
  if ((rc = upload(c, c->eph_tab, rows.data(), sizeof(RoemerRow) * rows.size(), "roemer rows"))) return rc;
  if ((rc = upload(c, c->eph_waves, waves.data(), sizeof(EphWave) * waves.size(), "roemer waves"))) return rc;
  k_roemer_main<false><<<dim3((unsigned)waves.size()), dim3(kEphWave), 0, c->stream>>>(
      c->eph_waves.as<EphWave>(), toas, c->eph_pos.as<double>(), c->eph_tab.as<RoemerRow>(), (int32_t)rows.size(),
      ob.sn, ob.cs, sign, n_toa, dst);
  HIPCHK(c, hipGetLastError(), "k_roemer_main launch");
  return FPTA_OK;
}

}  // namespace capi

using namespace capi;

extern "C" int fpta_ephem_kepler(fpta_ctx* c, int64_t n, const double* M, const double* e, double* E_out) {
  if (!c) return fail(nullptr, FPTA_EINVAL, "null ctx");
  if (n < 0 || (n > 0 && (!M || !e || !E_out))) return fail(c, FPTA_EINVAL, "ephem_kepler: bad arguments");
  for (int64_t i = 0; i < n; ++i) {
    if (!std::isfinite(M[i]) || std::fabs(M[i]) > 1e15)
      return fail(c, FPTA_EINVAL, "ephem_kepler: element " + std::to_string(i) + ": M not finite or beyond 1e15");
    if (!(e[i] >= 0.0 && e[i] <= fpta_ephem::kEMax))
      return fail(c, FPTA_EINVAL, "ephem_kepler: element " + std::to_string(i) + ": e outside [0, " +
                                      std::to_string(fpta_ephem::kEMax) + "]");
  }
  if (n == 0) return FPTA_OK;
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  int rc;
  if ((rc = upload(c, c->eph_toas, M, sizeof(double) * n, "kepler M"))) return rc;
  if ((rc = upload(c, c->eph_tab, e, sizeof(double) * n, "kepler e"))) return rc;
  HIPCHK(c, c->eph_out.ensure(sizeof(double) * (size_t)n), "kepler E");
  {
    KTimer kt(c, FPTA_K_EPHEM);
    k_ephem_kepler<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream>>>(
        n, c->eph_toas.as<double>(), c->eph_tab.as<double>(), c->eph_out.as<double>());
    HIPCHK(c, hipGetLastError(), "k_ephem_kepler launch");
  }
  HIPCHK(c, hipMemcpyAsync(E_out, c->eph_out.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream),
         "kepler download");
  HIPCHK(c, hipStreamSynchronize(c->stream), "kepler sync");
  return FPTA_OK;
}

extern "C" int fpta_ephem_orbits(fpta_ctx* c, int64_t n_toa, const double* toas, int32_t n_body,
                                 const double* bodies, double* planetssb_out, double* sunssb_out) {
  if (!c) return fail(nullptr, FPTA_EINVAL, "null ctx");
  if (n_toa < 0 || (n_toa > 0 && !toas) || n_body < 0 || (n_body > 0 && !bodies) ||
      (!planetssb_out && !sunssb_out))
    return fail(c, FPTA_EINVAL, "ephem_orbits: bad arguments");
  if (n_toa > (int64_t)1 << 36) return fail(c, FPTA_EINVAL, "ephem_orbits: too many TOAs");
  // everything is validated here, before anything is uploaded or launched
  double t0, t1;
  int64_t bad = -1;
  if (!fpta_ephem::toa_span(n_toa, toas, t0, t1, bad))
    return fail(c, FPTA_EINVAL, "ephem_orbits: TOA " + std::to_string(bad) + ": not finite");
  std::vector<Body> tab((size_t)n_body);
  std::string why;
  bad = fpta_ephem::validate_bodies(n_body, bodies, t0, t1, tab.data(), why);
  if (bad >= 0) return fail(c, FPTA_EINVAL, "ephem_orbits: body " + std::to_string(bad) + ": " + why);
  if (n_toa == 0) return FPTA_OK;
  if (n_body == 0) {  // no bodies: nothing in planetssb, the Sun at the barycentre
    if (sunssb_out) std::fill(sunssb_out, sunssb_out + 3 * n_toa, 0.0);
    return FPTA_OK;
  }
  const fpta_ephem::Obliquity ob = fpta_ephem::obliquity();
  const size_t n_p = planetssb_out ? (size_t)n_toa * n_body * 6 : 0, n_s = sunssb_out ? (size_t)n_toa * 3 : 0;

  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  int rc;
  if ((rc = upload(c, c->eph_toas, toas, sizeof(double) * n_toa, "ephem toas"))) return rc;
  if ((rc = upload(c, c->eph_tab, tab.data(), sizeof(Body) * tab.size(), "ephem bodies"))) return rc;
  if (n_p) HIPCHK(c, c->eph_out.ensure(sizeof(double) * n_p), "ephem planetssb");
  if (n_s) HIPCHK(c, c->eph_sun.ensure(sizeof(double) * n_s), "ephem sunssb");
  {
    KTimer kt(c, FPTA_K_EPHEM);
    k_ephem_orbits<<<dim3((unsigned)((n_toa + kEphWave - 1) / kEphWave)), dim3(kEphWave), 0, c->stream>>>(
        n_toa, c->eph_toas.as<double>(), n_body, c->eph_tab.as<Body>(), ob.sn, ob.cs, 1.0 / fpta_ephem::kMsun,
        n_p ? c->eph_out.as<double>() : nullptr, n_s ? c->eph_sun.as<double>() : nullptr);
    HIPCHK(c, hipGetLastError(), "k_ephem_orbits launch");
  }
  if (n_p)
    HIPCHK(c, hipMemcpyAsync(planetssb_out, c->eph_out.p, sizeof(double) * n_p, hipMemcpyDeviceToHost, c->stream),
           "ephem planetssb download");
  if (n_s)
    HIPCHK(c, hipMemcpyAsync(sunssb_out, c->eph_sun.p, sizeof(double) * n_s, hipMemcpyDeviceToHost, c->stream),
           "ephem sunssb download");
  HIPCHK(c, hipStreamSynchronize(c->stream), "ephem sync");
  return FPTA_OK;
}

extern "C" int fpta_roemer_accumulate(fpta_ctx* c, int32_t n_psr, const int64_t* offs, const double* toas,
                                      const double* pos, int32_t n_row, const double* rows, double sign,
                                      int32_t separate, double* out) {
  if (!c) return fail(nullptr, FPTA_EINVAL, "null ctx");
  if (n_psr <= 0 || !offs || !pos || n_row < 0 || (n_row > 0 && !rows) || !std::isfinite(sign))
    return fail(c, FPTA_EINVAL, "roemer_accumulate: bad arguments");
  if (offs[0] != 0) return fail(c, FPTA_EINVAL, "roemer_accumulate: offs[0] must be 0");
  for (int32_t p = 0; p < n_psr; ++p) {
    const int64_t n = offs[p + 1] - offs[p];
    if (n < 0) return fail(c, FPTA_EINVAL, "roemer_accumulate: offs must not decrease");
    if (n > (int64_t)1 << 30) return fail(c, FPTA_EINVAL, "roemer_accumulate: too many TOAs in one pulsar");
  }
  const int64_t n_toa = offs[n_psr];
  if (n_toa > 0 && (!toas || (n_row > 0 && !out))) return fail(c, FPTA_EINVAL, "roemer_accumulate: bad arguments");
  // everything is validated here, before anything is uploaded or launched
  double t0, t1;
  int64_t bad = -1;
  if (!fpta_ephem::toa_span(n_toa, toas, t0, t1, bad))
    return fail(c, FPTA_EINVAL, "roemer_accumulate: TOA " + std::to_string(bad) + ": not finite");
  for (int64_t i = 0; i < 3 * (int64_t)n_psr; ++i)
    if (!std::isfinite(pos[i]))
      return fail(c, FPTA_EINVAL, "roemer_accumulate: pulsar " + std::to_string(i / 3) + ": position not finite");
  std::vector<RoemerRow> tab((size_t)n_row);
  std::string why;
  bad = fpta_ephem::validate_rows(n_row, rows, t0, t1, tab.data(), why);
  if (bad >= 0) return fail(c, FPTA_EINVAL, "roemer_accumulate: row " + std::to_string(bad) + ": " + why);
  if (n_row == 0 || n_toa == 0) return FPTA_OK;
  std::vector<EphWave> waves;
  make_waves(n_psr, offs, waves);
  if (waves.size() > (size_t)0x7FFFFFFF) return fail(c, FPTA_EINVAL, "roemer_accumulate: too many TOAs");
  const fpta_ephem::Obliquity ob = fpta_ephem::obliquity();
  const size_t n_out = (size_t)n_toa * (separate ? (size_t)n_row : 1);

  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  int rc;
  if ((rc = upload(c, c->eph_toas, toas, sizeof(double) * n_toa, "roemer toas"))) return rc;
  if ((rc = upload(c, c->eph_pos, pos, sizeof(double) * 3 * n_psr, "roemer pos"))) return rc;
  if ((rc = upload(c, c->eph_tab, tab.data(), sizeof(RoemerRow) * tab.size(), "roemer rows"))) return rc;
  if ((rc = upload(c, c->eph_waves, waves.data(), sizeof(EphWave) * waves.size(), "roemer waves"))) return rc;
  if (separate)
    HIPCHK(c, c->eph_out.ensure(sizeof(double) * n_out), "roemer delays");
  else if ((rc = upload(c, c->eph_out, out, sizeof(double) * n_out, "roemer residuals")))
    return rc;
  {
    KTimer kt(c, FPTA_K_EPHEM);
    const dim3 grid((unsigned)waves.size());
    if (separate)
      k_roemer_main<true><<<grid, dim3(kEphWave), 0, c->stream>>>(
          c->eph_waves.as<EphWave>(), c->eph_toas.as<double>(), c->eph_pos.as<double>(), c->eph_tab.as<RoemerRow>(),
          n_row, ob.sn, ob.cs, sign, n_toa, c->eph_out.as<double>());
    else
      k_roemer_main<false><<<grid, dim3(kEphWave), 0, c->stream>>>(
          c->eph_waves.as<EphWave>(), c->eph_toas.as<double>(), c->eph_pos.as<double>(), c->eph_tab.as<RoemerRow>(),
          n_row, ob.sn, ob.cs, sign, n_toa, c->eph_out.as<double>());
    HIPCHK(c, hipGetLastError(), "k_roemer_main launch");
  }
  HIPCHK(c, hipMemcpyAsync(out, c->eph_out.p, sizeof(double) * n_out, hipMemcpyDeviceToHost, c->stream),
         "roemer download");
  HIPCHK(c, hipStreamSynchronize(c->stream), "roemer sync");
  return FPTA_OK;
}
