// Device arithmetic of a continuous wave, shared by cw.hip (fpta_cw_accumulate) and cw_batch.hip
// (fpta_batch_cw_accumulate): one definition of the (pulsar, source) pair constants and of the delay of one source at
// one TOA, so that both paths round every intermediate the same way and a realization of a batch block gets, bit for
// bit, what the drop-in call adds to a zero vector (tests/test_gpu_cw_batch.py).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "cw_host.h"

struct fpta_ctx;

namespace __attribute__((visibility("hidden"))) capi {

using fpta_cw::SrcEval;
using fpta_cw::SrcGeom;

struct CwPair {
  double Es, Ec;  // sign a0 (F+ Ps + Fx Xs), sign a0 (F+ Pc + Fx Xc)
  double shift;   // L (1 - cos mu): the pulsar term is evaluated at t - shift
  double pad;
};

// {Es, Ec, shift} of source g for the pulsar at unit vector (px, py, pz), L light-seconds away
__device__ __forceinline__ CwPair cw_pair(const SrcGeom& g, double px, double py, double pz, double L, double sign) {
  // m = (sin phi, -cos phi, 0), n = (-cos th cos phi, -cos th sin phi, sin th), omhat = (-sin th cos phi,
  // -sin th sin phi, -cos th)
  const double mp = g.sph * px - g.cph * py;
  const double nq = -g.cth * g.cph * px - g.cth * g.sph * py + g.sth * pz;
  const double op = -g.sth * g.cph * px - g.sth * g.sph * py - g.cth * pz;
  const double fplus = 0.5 * (mp * mp - nq * nq) / (1.0 + op);
  const double fcross = (mp * nq) / (1.0 + op);
  CwPair o;
  o.Es = sign * (fplus * g.Ps + fcross * g.Xs);
  o.Ec = sign * (fplus * g.Pc + fcross * g.Xc);
  o.shift = L * (1.0 + op);  // cos mu = -op
  o.pad = 0.0;
  return o;
}

// alpha(x) (Es sin 2 phase(x) + Ec cos 2 phase(x)) without the amplitude a0 (folded into Es, Ec)
__device__ __forceinline__ double cw_term(const SrcEval& e, double Es, double Ec, double x) {
  const double l = log1p(-e.K * x);
  const double ph2 = 2.0 * (e.hp0 - e.C * expm1(0.625 * l));
  double sn, cs;
  sincos(ph2, &sn, &cs);
  return exp(0.125 * l) * (Es * sn + Ec * cs);
}

// The delay of one source at TOA t: r(t - shift) - r(t) with the pulsar term, -r(t) without. e.pterm must be
// wave-uniform (the branch is a scalar one).
__device__ __forceinline__ double cw_delay(const SrcEval& e, double Es, double Ec, double shift, double t) {
  double d = -cw_term(e, Es, Ec, t);
  if (e.pterm != 0.0) d += cw_term(e, Es, Ec, t - shift);
  return d;
}

// One 64-TOA wave of k_cw_main
struct CwWave {
  int64_t first;  // first TOA (index into the concatenated arrays)
  int32_t psr;
  int32_t count;  // 1 .. 64
};

// cw.hip: the device part of one fpta_cw_accumulate call (cw_prepare fills it, cw_launch runs it)
struct CwRun {
  int32_t n_psr = 0, n_src = 0, per_split = 0, n_used = 0;  // n_used: source pieces in use
  int64_t n_toa = 0;
  std::vector<CwWave> waves;
};
int cw_prepare(fpta_ctx* c, int32_t n_psr, const int64_t* offs, const double* pos, const double* pdist_s,
               const std::vector<SrcEval>& ev, const std::vector<SrcGeom>& gm, CwRun& r);
int cw_launch(fpta_ctx* c, const CwRun& r, const double* toas, double sign, double* res);

// cw_batch.hip: the rows of the block each thread of k_cw_bcast adds its column's value to (bcast_add launches it, for
// roemer_batch.hip too)
constexpr int kCwbRows = 8;

}  // namespace capi
