// Continuous gravitational wave of circular binaries summed into every pulsar of an array (fpta_cw_accumulate):
// S x sum(N_toa) independent fp64 evaluations, each a log1p, an expm1, an exp and a sincos (twice with the pulsar
// term), with nothing a GEMM could reuse. fp64 VALU work, like k_synth_direct.
//
//   k_cw_prep    one thread per (pulsar, source): antenna pattern and light-travel shift, folded with the source's
//                polarisation / inclination / amplitude coefficients (cw_host.h) into {Es, Ec, shift}
//   k_cw_main    one wave per 64 TOAs of one pulsar; each thread sums its sources in ascending order in a register.
//                The source and pair tables are indexed by wave-uniform values only, so they come through the scalar
//                cache, and the pulsar-term branch is uniform. No LDS, no atomics.
//   k_cw_reduce  with n_split > 1 the source range is cut into n_split contiguous pieces (blockIdx.y), each writing
//                its partial sums; this kernel adds them into the residuals in ascending piece order.
// The arithmetic of a pair and of a source at a TOA is cw_device.h's, which cw_batch.hip shares.
#include "capi_host.h"
#include "cw_device.h"
#include "device_common.h"

namespace __attribute__((visibility("hidden"))) capi {

constexpr int kCwWave = 64;

__global__ __launch_bounds__(256) void k_cw_prep(const SrcGeom* __restrict__ gm, const double* __restrict__ pos,
                                                  const double* __restrict__ Ls, int32_t n_psr, int32_t n_src,
                                                  double sign, CwPair* __restrict__ pair) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n_psr * n_src) return;
  const int32_t p = (int32_t)(i / n_src), s = (int32_t)(i - (int64_t)p * n_src);
  FPTA_DCHECK(p < n_psr, "k_cw_prep pulsar", p, n_psr);
  pair[i] = cw_pair(gm[s], pos[3 * p], pos[3 * p + 1], pos[3 * p + 2], Ls[p], sign);
}

// dst: the residuals (SPLIT false: read and written) or the partial sums [gridDim.y][n_toa] (SPLIT true: written)
template <bool SPLIT>
__global__ __launch_bounds__(kCwWave) void k_cw_main(const CwWave* __restrict__ waves,
                                                     const double* __restrict__ toas,
                                                     const SrcEval* __restrict__ ev,
                                                     const CwPair* __restrict__ pair, int32_t n_src,
                                                     int32_t per_split, int64_t n_toa, double* __restrict__ dst) {
  const CwWave w = waves[blockIdx.x];
  const int32_t s0 = (int32_t)blockIdx.y * per_split;
  const int32_t s1 = min(n_src, s0 + per_split);
  const int32_t lane = min((int32_t)threadIdx.x, w.count - 1);  // spare lanes repeat the last TOA and store nothing
  const int64_t i = w.first + lane;
  FPTA_DCHECK(i >= 0 && i < n_toa, "k_cw_main toa", i, n_toa);
  const double t = toas[i];
  const CwPair* __restrict__ pr = pair + (int64_t)w.psr * n_src;
  double acc = 0.0;
  for (int32_t s = s0; s < s1; ++s) {
    const SrcEval e = ev[s];
    const CwPair q = pr[s];
    acc += cw_delay(e, q.Es, q.Ec, q.shift, t);
  }
  if ((int32_t)threadIdx.x < w.count) {
    if (SPLIT)
      dst[(int64_t)blockIdx.y * n_toa + i] = acc;
    else
      dst[i] += acc;
  }
}

__global__ __launch_bounds__(256) void k_cw_reduce(const double* __restrict__ part, int32_t n_split, int64_t n_toa,
                                                    double* __restrict__ res) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_toa) return;
  double acc = 0.0;
  for (int32_t k = 0; k < n_split; ++k) acc += part[(int64_t)k * n_toa + i];
  res[i] += acc;
}

// The device part of a call, shared with fpta_batch_cw_accumulate's one-table mode (cw_batch.hip): cw_prepare makes
// the wave table and the split of (n_src, n_toa, option) and queues every upload but the TOAs and the residuals;
// cw_launch queues k_cw_prep, k_cw_main and, with more than one piece, k_cw_reduce on the ctx stream. Nothing is
// validated here.
int cw_prepare(fpta_ctx* c, int32_t n_psr, const int64_t* offs, const double* pos, const double* pdist_s,
               const std::vector<SrcEval>& ev, const std::vector<SrcGeom>& gm, CwRun& r) {
  const int64_t n_toa = offs[n_psr];
  const int32_t n_src = (int32_t)ev.size();
  std::vector<CwWave>& waves = r.waves;  // the caller keeps it until the stream has taken the upload
  waves.clear();
  for (int32_t p = 0; p < n_psr; ++p)
    for (int64_t i = offs[p]; i < offs[p + 1]; i += kCwWave)
      waves.push_back({i, p, (int32_t)std::min<int64_t>(kCwWave, offs[p + 1] - i)});
  if (waves.size() > (size_t)0x7FFFFFFF) return fail(c, FPTA_EINVAL, "cw_accumulate: too many TOAs");
  const int32_t n_split = fpta_cw::split_count(n_src, n_toa, c->cw_split);
  r.n_psr = n_psr;
  r.n_src = n_src;
  r.n_toa = n_toa;
  r.per_split = (n_src + n_split - 1) / n_split;
  r.n_used = (n_src + r.per_split - 1) / r.per_split;  // no empty trailing piece
  int rc;
  if ((rc = upload(c, c->cw_pos, pos, sizeof(double) * 3 * n_psr, "cw pos"))) return rc;
  if ((rc = upload(c, c->cw_L, pdist_s, sizeof(double) * n_psr, "cw pdist"))) return rc;
  if ((rc = upload(c, c->cw_ev, ev.data(), sizeof(SrcEval) * ev.size(), "cw sources"))) return rc;
  if ((rc = upload(c, c->cw_gm, gm.data(), sizeof(SrcGeom) * gm.size(), "cw source geometry"))) return rc;
  if ((rc = upload(c, c->cw_waves, waves.data(), sizeof(CwWave) * waves.size(), "cw waves"))) return rc;
  HIPCHK(c, c->cw_pair.ensure(sizeof(CwPair) * (size_t)n_psr * (size_t)n_src), "cw pair table");
  if (r.n_used > 1) HIPCHK(c, c->cw_part.ensure(sizeof(double) * (size_t)r.n_used * n_toa), "cw partial sums");
  return FPTA_OK;
}

// toas, res: device [n_toa]; res is read and written (res += sign * the sum over the sources)
int cw_launch(fpta_ctx* c, const CwRun& r, const double* toas, double sign, double* res) {
  const int64_t n_pair = (int64_t)r.n_psr * r.n_src;
  k_cw_prep<<<dim3((unsigned)((n_pair + 255) / 256)), dim3(256), 0, c->stream>>>(
      c->cw_gm.as<SrcGeom>(), c->cw_pos.as<double>(), c->cw_L.as<double>(), r.n_psr, r.n_src, sign,
      c->cw_pair.as<CwPair>());
  HIPCHK(c, hipGetLastError(), "k_cw_prep launch");
  const dim3 grid((unsigned)r.waves.size(), (unsigned)r.n_used);
  if (r.n_used > 1) {
    k_cw_main<true><<<grid, dim3(kCwWave), 0, c->stream>>>(c->cw_waves.as<CwWave>(), toas, c->cw_ev.as<SrcEval>(),
                                                          c->cw_pair.as<CwPair>(), r.n_src, r.per_split, r.n_toa,
                                                          c->cw_part.as<double>());
    HIPCHK(c, hipGetLastError(), "k_cw_main launch");
    k_cw_reduce<<<dim3((unsigned)((r.n_toa + 255) / 256)), dim3(256), 0, c->stream>>>(c->cw_part.as<double>(), r.n_used,
                                                                                     r.n_toa, res);
    HIPCHK(c, hipGetLastError(), "k_cw_reduce launch");
  } else {
    k_cw_main<false><<<grid, dim3(kCwWave), 0, c->stream>>>(c->cw_waves.as<CwWave>(), toas, c->cw_ev.as<SrcEval>(),
                                                           c->cw_pair.as<CwPair>(), r.n_src, r.per_split, r.n_toa,
                                                           res);
    HIPCHK(c, hipGetLastError(), "k_cw_main launch");
  }
  return FPTA_OK;
}

}  // namespace capi

using namespace capi;

extern "C" int fpta_cw_accumulate(fpta_ctx* c, int32_t n_psr, const int64_t* offs, const double* toas,
                                  const double* pos, const double* pdist_s, int32_t n_src, const double* src,
                                  double sign, double* residuals) {
  if (!c) return fail(nullptr, FPTA_EINVAL, "null ctx");
  if (n_psr <= 0 || !offs || !toas || !pos || !pdist_s || n_src < 0 || (n_src > 0 && !src) || !residuals)
    return fail(c, FPTA_EINVAL, "cw_accumulate: bad arguments");
  if (offs[0] != 0) return fail(c, FPTA_EINVAL, "cw_accumulate: offs[0] must be 0");
  for (int32_t p = 0; p < n_psr; ++p) {
    const int64_t n = offs[p + 1] - offs[p];
    if (n <= 0) return fail(c, FPTA_EINVAL, "cw_accumulate: every pulsar needs >= 1 TOA");
    if (n > (int64_t)1 << 30) return fail(c, FPTA_EINVAL, "cw_accumulate: too many TOAs in one pulsar");
  }
  const int64_t n_toa = offs[n_psr];
  if (n_src == 0) return FPTA_OK;
  if ((int64_t)n_psr * n_src > (int64_t)1 << 31)
    return fail(c, FPTA_EINVAL, "cw_accumulate: more than 2^31 (pulsar, source) pairs");
  // everything is validated here, before anything is uploaded or launched
  double tmax = toas[0];
  for (int64_t i = 1; i < n_toa; ++i) tmax = std::max(tmax, toas[i]);
  std::vector<SrcEval> ev((size_t)n_src);
  std::vector<SrcGeom> gm((size_t)n_src);
  std::string why;
  const int64_t bad = fpta_cw::validate_sources(n_src, src, tmax, ev.data(), gm.data(), why);
  if (bad >= 0) return fail(c, FPTA_EINVAL, "cw_accumulate: source " + std::to_string(bad) + ": " + why);
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  int rc;
  CwRun run;
  if ((rc = upload(c, c->cw_toas, toas, sizeof(double) * n_toa, "cw toas"))) return rc;
  if ((rc = cw_prepare(c, n_psr, offs, pos, pdist_s, ev, gm, run))) return rc;
  if ((rc = upload(c, c->scratch_out, residuals, sizeof(double) * n_toa, "cw residuals"))) return rc;
  {
    KTimer kt(c, FPTA_K_CW);
    if ((rc = cw_launch(c, run, c->cw_toas.as<double>(), sign, c->scratch_out.as<double>()))) return rc;
  }
  HIPCHK(c, hipMemcpyAsync(residuals, c->scratch_out.p, sizeof(double) * n_toa, hipMemcpyDeviceToHost, c->stream),
         "cw download");
  HIPCHK(c, hipStreamSynchronize(c->stream), "cw sync");
  return FPTA_OK;
}
