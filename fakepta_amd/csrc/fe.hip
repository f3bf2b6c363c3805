// Continuous-wave F-statistics (fpta_batch_set_fe, fpta_batch_fe_info, fpta_batch_fe, fpta_fe_statistic): per
// realization the Earth-term Fe-statistic on a grid of directions and frequencies with its maxima, and the incoherent
// Fp-statistic per frequency. The definition is in include/fakepta_amd.h; the per-pulsar operator B_p, the antenna
// table, M^-1 and m^-1 are fe_host.h's.
//
//   stage 1  X = B_p r of every realization: k_fit_apply (fit.hip) on this file's operator slot and coefficient buffer
//            [P][K][R_pad], K = 2 G: row g is (r|c_g), row G + g is (r|s_g). The same instances as the Fourier fit, the
//            optimal statistic and the likelihood grid, whose slots are not touched.
//   stage 2  k_fe_sky: a workgroup of 4 waves owns one frequency and 16 realizations. It stages its X tile (pulsars
//            past P as zeros) into LDS once, in the order the MFMA's B operand wants it: [k-step of 4 pulsars][sin,
//            cos][lane].
//            Wave w then takes the tiles w, w + 4, .. of 8 directions. The 16 rows of a tile's antenna operand are
//            ordered (direction & 3, polarisation, direction >> 2), so that with the accumulator map of
//            v_mfma_f64_16x16x4_f64 (column lane & 15, rows (lane >> 4) + 4 q) a lane holds F+ and Fx of the directions
//            lane >> 4 and (lane >> 4) + 4 for its realization; the table is laid out on the host so that a k-step's
//            operand is one 512-byte run. One MFMA chain runs against the sine columns and one against the cosine
//            columns, k = the pulsars in order: the 4-vector N of a (direction, realization) then sits in one lane, and
//            the quadratic form with the 10 numbers of M^-1 is a per-lane epilogue. A lane keeps a running (max,
//            argmax) over its directions in index order; the four lane groups are merged by a butterfly and the four waves
//            through LDS, ties to the lower index, NaN never taken. A fixed order, no atomics, nothing shared between
//            realizations: a realization's numbers are the same whatever R, its position and its neighbours.
//            k_fe_reduce: Fp[g][r] = sum_p x^T m_pg^-1 x / 2 in pulsar order, one thread per (g, r), and the maximum
//            over the frequencies in index order, one thread per realization.
// Padding realizations have X = 0 (the cleared buffer); they are not downloaded.
#include "capi_host.h"
#include "fe_host.h"
#include "device_common.h"

namespace __attribute__((visibility("hidden"))) capi {

constexpr int kFeReal = 16;   // realizations of a workgroup
constexpr int kFeWaves = 4;   // waves of a workgroup
constexpr int kFeDirs = 8;    // directions of a tile
constexpr int kFeRpad = 32;   // k_fit_apply's realization padding: a multiple of kFeReal
static_assert(kFeRpad % kFeReal == 0 && kFeReal == 16 &&
                  2 * 64 * ((fpta_fe::kMaxPsr + 3) / 4) * sizeof(double) <= 65536,
              "k_fe_sky never reads past the padded realizations and its X tile fits 64 KB of LDS");

struct FeArgs {
  const double* X;     // [P][K][R_pad], K = 2 G: the cosine rows, then the sine rows
  const double* Ft;    // [n_tile][KS][64] the antenna operand of every tile and k-step
  const double* Minv;  // [n_sky][G][10]
  double* fef;         // [G][R_pad]
  int32_t* argf;       // [G][R_pad]
  double* map;         // NULL or [n_sky][G][R_pad]
  int32_t P, G, KS, n_sky, n_tile, R_pad;
};

// (v, i) <- the better of (v, i) and (ov, oi): i < 0 marks "nothing yet", the larger value wins, equals go to the lower
// index. Values are never NaN here: a NaN is not taken into a running maximum.
__device__ __forceinline__ void fe_merge(double& v, int& i, double ov, int oi) {
  const bool take = oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i));
  v = take ? ov : v;
  i = take ? oi : i;
}

// Fe = N^T M^-1 N / 2 with the 10 numbers of M^-1's upper triangle (fe_host.h's tri4 order)
__device__ __forceinline__ double fe_form(const double* __restrict__ mi, double n0, double n1, double n2, double n3) {
  const double a00 = mi[0], a01 = mi[1], a02 = mi[2], a03 = mi[3], a11 = mi[4], a12 = mi[5], a13 = mi[6], a22 = mi[7],
               a23 = mi[8], a33 = mi[9];
  const double t0 = fma(a03, n3, fma(a02, n2, fma(a01, n1, a00 * n0)));
  const double t1 = fma(a13, n3, fma(a12, n2, fma(a11, n1, a01 * n0)));
  const double t2 = fma(a23, n3, fma(a22, n2, fma(a12, n1, a02 * n0)));
  const double t3 = fma(a33, n3, fma(a23, n2, fma(a13, n1, a03 * n0)));
  return 0.5 * fma(n3, t3, fma(n2, t2, fma(n1, t1, n0 * t0)));
}

// grid: (R_pad / 16, G); dynamic LDS: KS x 2 x 64 doubles
__global__ __launch_bounds__(64 * kFeWaves) void k_fe_sky(FeArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sFe[];  // [k-step][sin, cos][lane]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lg = lane >> 4;
  const int r0 = (int)blockIdx.x * kFeReal, g = (int)blockIdx.y;
  const int K = 2 * a.G, KS = a.KS;
  FPTA_DCHECK(r0 + kFeReal <= a.R_pad, "k_fe_sky realization", r0 + kFeReal, a.R_pad + 1);

  // the X tile: element (pulsar p, sin / cos, realization rr of the tile), coalesced along the realizations
  for (int i = tid; i < KS * 4 * 2 * kFeReal; i += 64 * kFeWaves) {
    const int rr = i & 15, cs = (i >> 4) & 1, p = i >> 5;
    double x = 0.0;
    if (p < a.P) x = a.X[((int64_t)p * K + (cs ? g : a.G + g)) * a.R_pad + r0 + rr];
    sFe[((p >> 2) * 2 + cs) * 64 + (p & 3) * 16 + rr] = x;
  }
  __syncthreads();

  double best = 0.0;
  int bi = -1;
  for (int tile = wave; tile < a.n_tile; tile += kFeWaves) {  // wave-uniform
    const double* __restrict__ Ft = a.Ft + (int64_t)tile * KS * 64 + lane;
    d4 as = d4{0.0, 0.0, 0.0, 0.0}, ac = d4{0.0, 0.0, 0.0, 0.0};
    for (int ks = 0; ks < KS; ++ks) {
      const double f = Ft[ks * 64];
      const double xs = sFe[(ks * 2) * 64 + lane], xc = sFe[(ks * 2 + 1) * 64 + lane];
      as = __builtin_amdgcn_mfma_f64_16x16x4f64(f, xs, as, 0, 0, 0);
      ac = __builtin_amdgcn_mfma_f64_16x16x4f64(f, xc, ac, 0, 0, 0);
    }
    // the lane's two directions, the lower one first: N = [F+ x_s, F+ x_c, Fx x_s, Fx x_c]
    const int s0 = tile * kFeDirs + lg, s1 = s0 + 4;
    if (s0 < a.n_sky) {
      const double fe = fe_form(a.Minv + ((int64_t)s0 * a.G + g) * 10, as[0], ac[0], as[1], ac[1]);
      if (a.map) a.map[((int64_t)s0 * a.G + g) * a.R_pad + r0 + lr] = fe;
      if (fe == fe && (bi < 0 || fe > best)) {
        best = fe;
        bi = s0;
      }
    }
    if (s1 < a.n_sky) {
      const double fe = fe_form(a.Minv + ((int64_t)s1 * a.G + g) * 10, as[2], ac[2], as[3], ac[3]);
      if (a.map) a.map[((int64_t)s1 * a.G + g) * a.R_pad + r0 + lr] = fe;
      if (fe == fe && (bi < 0 || fe > best)) {
        best = fe;
        bi = s1;
      }
    }
  }
  // the four lane groups of the wave, then the four waves through LDS (the X tile is done with)
  {
    const double ov = __shfl_xor(best, 16, 64);
    const int oi = __shfl_xor(bi, 16, 64);
    fe_merge(best, bi, ov, oi);
  }
  {
    const double ov = __shfl_xor(best, 32, 64);
    const int oi = __shfl_xor(bi, 32, 64);
    fe_merge(best, bi, ov, oi);
  }
  __syncthreads();
  double* sV = sFe;                                        // [waves][16]
  int* sI = (int*)(sFe + kFeWaves * kFeReal);              // [waves][16]
  if (lane < 16) {
    sV[wave * kFeReal + lr] = best;
    sI[wave * kFeReal + lr] = bi;
  }
  __syncthreads();
  if (tid < 16) {
#pragma unroll
    for (int w = 1; w < kFeWaves; ++w) fe_merge(best, bi, sV[w * kFeReal + lr], sI[w * kFeReal + lr]);
    const int64_t o = (int64_t)g * a.R_pad + r0 + lr;
    a.fef[o] = bi < 0 ? __builtin_nan("") : best;
    a.argf[o] = bi;
  }
}

// Fp[g][r] = sum_p x_pg^T m_pg^-1 x_pg / 2 in pulsar order, one thread per (g, r); thread r < R_pad also takes the
// maximum of Fe_f[.][r] over the frequencies in index order (NaN never taken, the first of equals): Fe_max [R_pad] and
// its argmax [2][R_pad] = (direction, frequency), -1 when every value is NaN
__global__ __launch_bounds__(256) void k_fe_reduce(const double* __restrict__ X, const double* __restrict__ pinv,
                                                    const double* __restrict__ fef, const int32_t* __restrict__ argf,
                                                    int32_t P, int32_t G, int32_t R_pad, int64_t n,
                                                    double* __restrict__ fp, double* __restrict__ femax,
                                                    int32_t* __restrict__ argmax) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const int64_t g = e / R_pad, r = e - g * R_pad;
  const int64_t K = 2 * (int64_t)G;
  double s = 0.0;
  for (int32_t p = 0; p < P; ++p) {
    const double xc = X[((int64_t)p * K + g) * R_pad + r], xs = X[((int64_t)p * K + G + g) * R_pad + r];
    const double* __restrict__ mi = pinv + ((int64_t)p * G + g) * 3;
    s += xs * (mi[0] * xs + mi[1] * xc) + xc * (mi[1] * xs + mi[2] * xc);
  }
  fp[e] = 0.5 * s;
  if (e < R_pad) {
    double best = 0.0;
    int bs = -1, bg = -1;
    for (int32_t k = 0; k < G; ++k) {
      const double v = fef[(int64_t)k * R_pad + e];
      if (v == v && (bg < 0 || v > best)) {
        best = v;
        bg = k;
        bs = argf[(int64_t)k * R_pad + e];
      }
    }
    femax[e] = bg < 0 ? __builtin_nan("") : best;
    argmax[e] = bs;
    argmax[R_pad + e] = bg;
  }
}

// Device copies of a plan's tables; the antenna table goes up in k_fe_sky's tile layout
static int fe_upload(fpta_ctx* c, const fpta_fe::Plan& plan, int32_t n_psr, const int64_t* offs, FeSlot& s) {
  int rc;
  if ((rc = fit_upload(c, "fe", s.x, plan.K, plan.B, n_psr, offs, plan.rows))) return rc;
  const int32_t KS = std::max((n_psr + 3) / 4, 1), n_tile = (plan.n_sky + kFeDirs - 1) / kFeDirs;
  std::vector<double> ft;
  try {
    ft.assign((size_t)n_tile * (size_t)KS * 64, 0.0);
  } catch (const std::bad_alloc&) {
    return fail(c, FPTA_ENOMEM, "fe: no host memory for the antenna operand of " +
                                    std::to_string(512.0 * (double)n_tile * (double)KS) + " bytes");
  }
  for (int32_t t = 0; t < n_tile; ++t)
    for (int32_t ks = 0; ks < KS; ++ks)
      for (int32_t lane = 0; lane < 64; ++lane) {
        const int32_t i = lane & 15, p = 4 * ks + (lane >> 4);
        const int32_t sdir = t * kFeDirs + (i & 3) + 4 * (i >> 3), pol = (i >> 2) & 1;
        if (sdir < plan.n_sky && p < n_psr)
          ft[((size_t)t * (size_t)KS + (size_t)ks) * 64 + (size_t)lane] =
              plan.F[(size_t)(2 * sdir + pol) * (size_t)n_psr + (size_t)p];
      }
  const size_t b_f = sizeof(double) * ft.size(), b_m = sizeof(double) * plan.Minv.size();
  const size_t b_p = sizeof(double) * plan.minv.size();
  if (s.f.ensure(b_f) != hipSuccess || s.minv.ensure(b_m) != hipSuccess || s.pinv.ensure(b_p) != hipSuccess)
    return fail(c, FPTA_ENOMEM, "fe: no device memory for the tables of " + std::to_string(b_f + b_m + b_p) +
                                    " bytes (n_sky = " + std::to_string(plan.n_sky) + ", G = " +
                                    std::to_string(plan.G) + ")");
  // ft is this function's own: whatever an upload returns, the stream has run before it goes
  rc = upload(c, s.f, ft.data(), b_f, "fe antenna operand");
  if (!rc) rc = upload(c, s.minv, plan.Minv.data(), b_m, "fe inverses");
  if (!rc) rc = upload(c, s.pinv, plan.minv.data(), b_p, "fe pulsar inverses");
  const hipError_t e = hipStreamSynchronize(c->stream);
  if (rc) return rc;
  if (e != hipSuccess) return hip_fail(c, e, "fe upload sync");
  return FPTA_OK;
}

// Both stages on a block of st.G frequencies and st.n_sky directions; one FPTA_K_DENSE entry. The results stay in the
// slot, padded to st.rpad realizations. want_map: the whole map [n_sky][G][rpad] is written too.
static int fe_launch(fpta_ctx* c, const Block& b, FeSlot& s, FeState& st, bool want_map) {
  const int32_t R = b.R, n_psr = b.n_psr, K = st.K, G = st.G, S = st.n_sky;
  const int32_t R_pad = st.rpad = (R + kFeRpad - 1) / kFeRpad * kFeRpad;
  const size_t b_x = sizeof(double) * (size_t)n_psr * (size_t)K * (size_t)R_pad;
  const size_t b_g = sizeof(double) * (size_t)G * (size_t)R_pad, b_r = sizeof(double) * (size_t)R_pad;
  const size_t b_map = want_map ? sizeof(double) * (size_t)S * (size_t)G * (size_t)R_pad : 0;
  if (s.x.coef.ensure(b_x) != hipSuccess || s.fef.ensure(b_g) != hipSuccess || s.argf.ensure(b_g) != hipSuccess ||
      s.fp.ensure(b_g) != hipSuccess || s.femax.ensure(b_r) != hipSuccess || s.argmax.ensure(b_r) != hipSuccess ||
      (want_map && s.map.ensure(b_map) != hipSuccess))
    return fail(c, FPTA_ENOMEM, "fe: no device memory for " + std::to_string(b_x + 3 * b_g + 2 * b_r + b_map) +
                                    " bytes of results" + (want_map ? " (the map is 8 n_sky G R_pad bytes)" : ""));
  if (R_pad / kFeReal > 0x7FFFFFFF || G > 65535)
    return fail(c, FPTA_EINVAL, "fe: too many realizations or frequencies");
  KTimer kt(c, FPTA_K_DENSE);
  int32_t rp = 0;
  int rc = fit_launch_unbooked(c, b, K, s.x, rp);
  if (rc) return rc;
  if (rp != R_pad) return fail(c, FPTA_EINVAL, "fe: k_fit_apply's realization padding changed");
  if (R == 0) return FPTA_OK;
  FeArgs a;
  a.X = s.x.coef.as<double>();
  a.Ft = s.f.as<double>();
  a.Minv = s.minv.as<double>();
  a.fef = s.fef.as<double>();
  a.argf = s.argf.as<int32_t>();
  a.map = want_map ? s.map.as<double>() : nullptr;
  a.P = n_psr;
  a.G = G;
  a.KS = std::max((n_psr + 3) / 4, 1);
  a.n_sky = S;
  a.n_tile = (S + kFeDirs - 1) / kFeDirs;
  a.R_pad = R_pad;
  const size_t lds = sizeof(double) * 2 * 64 * (size_t)a.KS;
  k_fe_sky<<<dim3((unsigned)(R_pad / kFeReal), (unsigned)G), dim3(64 * kFeWaves), lds, c->stream>>>(a);
  HIPCHK(c, hipGetLastError(), "k_fe_sky launch");
  const int64_t n = (int64_t)G * R_pad;
  k_fe_reduce<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream>>>(
      s.x.coef.as<double>(), s.pinv.as<double>(), s.fef.as<double>(), s.argf.as<int32_t>(), n_psr, G, R_pad, n,
      s.fp.as<double>(), s.femax.as<double>(), s.argmax.as<int32_t>());
  HIPCHK(c, hipGetLastError(), "k_fe_reduce launch");
  return FPTA_OK;
}

// A buffer [rows][R_pad] of int32 as [rows][R]
static int fe_download_i32(fpta_ctx* c, const DevBuf& buf, int64_t rows, int32_t R, int32_t R_pad, int32_t* host) {
  if (rows > 0 && R > 0)
    HIPCHK(c, hipMemcpy2DAsync(host, sizeof(int32_t) * (size_t)R, buf.p, sizeof(int32_t) * (size_t)R_pad,
                               sizeof(int32_t) * (size_t)R, (size_t)rows, hipMemcpyDeviceToHost, c->stream),
           "fe download");
  HIPCHK(c, hipStreamSynchronize(c->stream), "fe sync");
  return FPTA_OK;
}

// The wanted results of fe_launch on that block, unpadded
static int fe_results(fpta_ctx* c, const Block& b, const FeSlot& s, const FeState& st, double* fe_max, int32_t* arg_max,
                      double* fe_f, int32_t* arg_f, double* fp, double* fe_map, double* X) {
  int rc;
  if (fe_max && (rc = fit_download(c, s.femax, 1, b.R, st.rpad, fe_max))) return rc;
  if (arg_max && (rc = fe_download_i32(c, s.argmax, 2, b.R, st.rpad, arg_max))) return rc;
  if (fe_f && (rc = fit_download(c, s.fef, st.G, b.R, st.rpad, fe_f))) return rc;
  if (arg_f && (rc = fe_download_i32(c, s.argf, st.G, b.R, st.rpad, arg_f))) return rc;
  if (fp && (rc = fit_download(c, s.fp, st.G, b.R, st.rpad, fp))) return rc;
  if (fe_map && (rc = fit_download(c, s.map, (int64_t)st.n_sky * st.G, b.R, st.rpad, fe_map))) return rc;
  if (X && (rc = fit_download(c, s.x.coef, (int64_t)b.n_psr * st.K, b.R, st.rpad, X))) return rc;
  return FPTA_OK;
}

// The plan's host tables the caller asked for
static void fe_tables(const fpta_fe::Plan& plan, int32_t* rank_out, double* F_out, double* Minv_out, double* minv_out,
                      int32_t* neff_out) {
  if (rank_out) std::copy(plan.rank.begin(), plan.rank.end(), rank_out);
  if (F_out) std::copy(plan.F.begin(), plan.F.end(), F_out);
  if (Minv_out) std::copy(plan.Minv.begin(), plan.Minv.end(), Minv_out);
  if (minv_out) std::copy(plan.minv.begin(), plan.minv.end(), minv_out);
  if (neff_out) std::copy(plan.n_eff.begin(), plan.n_eff.end(), neff_out);
}

static fpta_fe::Grid fe_grid(int32_t n_fgw, const double* fgw, int32_t n_sky, const double* sky, const double* pos) {
  fpta_fe::Grid g;
  g.n_f = n_fgw;
  g.fgw = fgw;
  g.n_sky = n_sky;
  g.sky = sky;
  g.pos = pos;
  return g;
}

}  // namespace capi

using namespace capi;

extern "C" int fpta_batch_set_fe(fpta_ctx* c, int32_t n_comp, const int32_t* n_modes, const double* f,
                                 int32_t f_is_common, const double* idx, const double* freqf, const double* phi,
                                 const uint8_t* mask, int32_t n_col, const double* M, const int32_t* ncol_psr,
                                 const double* weights, double rcond, int32_t n_fgw, const double* fgw, int32_t n_sky,
                                 const double* sky, const double* pos, double rcond_fe, int32_t* rank_out,
                                 double* F_out, double* Minv_out, double* minv_out, int32_t* neff_out) {
  if (!c) return fail(nullptr, FPTA_EINVAL, "null ctx");
  const Layout& L = c->batch;
  if (L.P <= 0) return fail(c, FPTA_ESTATE, "set_fe: set_toas first");
  if (n_comp == 0) {
    c->fe_st.clear();
    if (rank_out) std::fill(rank_out, rank_out + L.P, 0);
    return FPTA_OK;
  }
  // everything is validated and the tables built here, before anything is uploaded
  std::string why;
  fpta_fe::Plan plan;
  const int made = fpta_fe::make_plan(L.P, L.h_offs.data(), L.h_toas.data(), L.h_nu.data(),
                                      fpta_fit::make_spec(n_comp, n_modes, f, f_is_common, idx, freqf), phi, mask,
                                      fe_grid(n_fgw, fgw, n_sky, sky, pos), n_col, M, ncol_psr, weights, rcond,
                                      rcond_fe, plan, why);
  if (made) return fail(c, made == 2 ? FPTA_ENOMEM : FPTA_EINVAL, "set_fe: " + why);
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  c->fe_st.clear();
  // a statistic with the previous tables may still read them
  HIPCHK(c, hipStreamSynchronize(c->stream), "set_fe sync");
  int rc;
  if ((rc = fe_upload(c, plan, L.P, L.h_offs.data(), c->fe))) return rc;
  c->fe_st = FeState{true, plan.K, plan.G, plan.n_sky};
  fe_tables(plan, rank_out, F_out, Minv_out, minv_out, neff_out);
  return FPTA_OK;
}

extern "C" int fpta_batch_fe_info(fpta_ctx* c, int64_t* info) {
  if (!c || !info) return fail(c, FPTA_EINVAL, "fe_info: bad arguments");
  const FeState& st = c->fe_st;  // all zero while no statistic is set
  const int64_t v[4] = {st.K, st.G, st.n_sky, st.R};
  std::copy(v, v + 4, info);
  return FPTA_OK;
}

extern "C" int fpta_batch_fe(fpta_ctx* c, double* fe_max, int32_t* arg_max, double* fe_f, int32_t* arg_f, double* fp,
                             double* fe_map, double* X) {
  Block b;
  int rc;
  if ((rc = block_check(c, "fe", false, b))) return rc;
  FeState& st = c->fe_st;
  if (!st.set) return fail(c, FPTA_ESTATE, "fe: no F-statistic is set (set_fe first)");
  if ((rc = block_open(c, false))) return rc;
  st.R = 0;
  if ((rc = fe_launch(c, b, c->fe, st, fe_map != nullptr))) return rc;
  st.R = b.R;
  return fe_results(c, b, c->fe, st, fe_max, arg_max, fe_f, arg_f, fp, fe_map, X);
}

extern "C" int fpta_fe_statistic(fpta_ctx* c, int32_t n_psr, const int64_t* offs, const double* toas, const double* nu,
                                 int32_t n_comp, const int32_t* n_modes, const double* f, int32_t f_is_common,
                                 const double* idx, const double* freqf, const double* phi, const uint8_t* mask,
                                 int32_t n_col, const double* M, const int32_t* ncol_psr, const double* weights,
                                 double rcond, int32_t n_fgw, const double* fgw, int32_t n_sky, const double* sky,
                                 const double* pos, double rcond_fe, int32_t n_vec, const double* res, double* fe_max,
                                 int32_t* arg_max, double* fe_f, int32_t* arg_f, double* fp, double* fe_map, double* X,
                                 int32_t* rank_out, double* F_out, double* Minv_out, double* minv_out,
                                 int32_t* neff_out) {
  const OneShot one{c, "fe_statistic", n_psr, offs, n_vec, res};
  int rc;
  if ((rc = one.check())) return rc;
  std::string why;
  fpta_fe::Plan plan;
  const int made = fpta_fe::make_plan(n_psr, offs, toas, nu,
                                      fpta_fit::make_spec(n_comp, n_modes, f, f_is_common, idx, freqf), phi, mask,
                                      fe_grid(n_fgw, fgw, n_sky, sky, pos), n_col, M, ncol_psr, weights, rcond,
                                      rcond_fe, plan, why);
  if ((rc = one.planned(made, why))) return rc;
  fe_tables(plan, rank_out, F_out, Minv_out, minv_out, neff_out);
  if (n_vec == 0) return FPTA_OK;
  if (n_psr == 0 || one.n_toa() == 0) {  // nothing to launch: every X and Fp is zero and every point is singular
    const double nan = std::nan("");
    if (fe_max) std::fill(fe_max, fe_max + n_vec, nan);
    if (arg_max) std::fill(arg_max, arg_max + 2 * (int64_t)n_vec, -1);
    if (fe_f) std::fill(fe_f, fe_f + (int64_t)plan.G * n_vec, nan);
    if (arg_f) std::fill(arg_f, arg_f + (int64_t)plan.G * n_vec, -1);
    if (fp) std::fill(fp, fp + (int64_t)plan.G * n_vec, 0.0);
    if (fe_map) std::fill(fe_map, fe_map + (int64_t)plan.n_sky * plan.G * n_vec, nan);
    if (X) std::fill(X, X + (int64_t)n_psr * plan.K * n_vec, 0.0);
    return FPTA_OK;
  }
  Block b;
  if ((rc = one.upload(b))) return rc;
  if ((rc = fe_upload(c, plan, n_psr, offs, c->fe1))) return rc;
  FeState st{true, plan.K, plan.G, plan.n_sky};
  if ((rc = fe_launch(c, b, c->fe1, st, fe_map != nullptr))) return rc;
  if ((rc = fe_results(c, b, c->fe1, st, fe_max, arg_max, fe_f, arg_f, fp, fe_map, X))) return rc;
  return one.done();
}
