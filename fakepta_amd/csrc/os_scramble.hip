// Sky scrambles of the optimal statistic (fpta_batch_set_os_scrambles, fpta_batch_os_scrambles_info,
// fpta_batch_os_scrambles, fpta_os_scrambles, fpta_os_scramble_match): the statistic of every realization under J
// further pair-weight matrices, the Hellings-Downs matrices of fictitious pulsar positions (or explicit matrices), and
// the rank of the observed S/N among them. The definition is in include/fakepta_amd.h; the pair map and the refusals
// are os_scramble_host.h's. Nothing that depends on the data depends on the matrices except one contraction over the
// pairs a > b (pair e = a (a - 1) / 2 + b, np.tril_indices' order, padded to n_pad = a multiple of 16 with zero rows):
//
//   set      k_scr_orf: Gs[j][e] from the positions of scramble j (x = (1 - p_a . p_b) / 2 with every operation rounded
//            once, G = 1.5 x ln x - x / 4 + 1 / 2), or gathered from explicit matrices; the same kernel gathers the
//            observed matrices of the statistic that is set. k_scr_stats, one workgroup per row: norm = sum G^2 N_ab,
//            sum G^2 and the unweighted products with every observed row, each a strided partial per thread and a
//            tree over the 256 threads.
//   stage 1, 2  the optimal statistic's own (k_fit_apply, k_os_pairs, k_os_reduce): X [P][K][R_pad] and the observed Q.
//   stage 3  k_scr_pairs: Y[e][r] = sum_k phi_hat_k X_a,k X_b,k over the K = 2 N columns. A workgroup of 4 waves owns
//            16 realizations of one lower 16 x 16 tile pair of pulsars; the two X tiles go through LDS in chunks of 8
//            columns, a wave takes 4 realizations and accumulates one v_mfma_f64_16x16x4_f64 per 4 columns. The 256
//            pair sums go back through LDS so that the stores run along the realizations.
//   stage 4  k_scr_gemm: Qs = Gs Y on v_mfma_f64_16x16x4_f64. A workgroup owns a 128 x 64 tile of Qs over the whole
//            pair axis (no split-K), a wave 64 x 32 of it; Gs and Y go through LDS in chunks of 16 pairs.
//   stage 5  k_scr_rank, one thread per realization: S/N of the observed matrices and of every scramble by one device
//            function, the null's mean, standard deviation (two passes in scramble order) and maximum, and the count
//            of scrambles at or above each observed S/N.
// No atomics and a fixed order everywhere: a scramble's row of Qs is the same bits whatever the other scrambles, a
// realization's column the same whatever R, its position and its neighbours. Padding pairs, padding realizations and
// rows past J are exact zeros.
#include <map>
#include <mutex>

#include "capi_host.h"
#include "os_host.h"
#include "os_scramble_host.h"
#include "device_common.h"

namespace __attribute__((visibility("hidden"))) capi {

constexpr int kScrYReal = 16;  // realizations of a k_scr_pairs workgroup
constexpr int kScrYKc = 8;     // columns of X per LDS chunk
constexpr int kScrYLd = kScrYKc * 16 + 1;
constexpr int kScrM = 128, kScrN = 64, kScrK = 16;  // k_scr_gemm's tile of Qs and its chunk of pairs
constexpr int kScrLdA = kScrM + 17, kScrLdB = kScrN + 16;
static_assert(kScrK == fpta_scr::kPairPad, "the pair rows are padded to k_scr_gemm's chunk");
static_assert(kOsRpad % kScrYReal == 0, "k_scr_pairs never reads past the padded realizations");

// x of a pair, every operation rounded once: os_scramble_host.h's pair_x
__device__ inline double scr_pair_x(const double* pa, const double* pb) {
#pragma clang fp contract(off)
  const double dot = (pa[0] * pb[0] + pa[1] * pb[1]) + pa[2] * pb[2];
  return (1.0 - dot) * 0.5;
}

// Gs[j][e] for every pair of the map (padding: 0): from pos [J][P][3], or else from the matrices G [J][P][P].
// grid: (ceil(n_pad / 256), J)
__global__ __launch_bounds__(256) void k_scr_orf(const int32_t* __restrict__ map, const double* __restrict__ pos,
                                                  const double* __restrict__ G, int32_t P, int64_t n_pad,
                                                  double* __restrict__ Gs) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
  if (e >= n_pad) return;
  const int32_t a = map[2 * e], b = map[2 * e + 1];
  double v = 0.0;
  if (a >= 0) {
    if (pos) {
      const double x = scr_pair_x(pos + (j * P + a) * 3, pos + (j * P + b) * 3);
      v = 1.5 * x * log(x) - 0.25 * x + 0.5;
    } else {
      v = G[(j * P + a) * P + b];
    }
  }
  Gs[j * n_pad + e] = v;
}

// Per row j of Gs: norm[j] = sum_e G^2 N_ab, ss[j] = sum_e G^2 and, with n_ref observed rows Go and their sums of
// squares oss, match[j][o] = sum_e Go G / sqrt(oss[o] ss[j]). nab NULL: no norm. grid: (J), 256 threads.
__global__ __launch_bounds__(256) void k_scr_stats(const int32_t* __restrict__ map, const double* __restrict__ Gs,
                                                    const double* __restrict__ nab, int32_t P, int64_t n_pad,
                                                    int32_t n_ref, const double* __restrict__ Go,
                                                    const double* __restrict__ oss, double* __restrict__ norm,
                                                    double* __restrict__ ss, double* __restrict__ match) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const int64_t j = blockIdx.x;
  const double* g = Gs + j * n_pad;
  double ss_j = 0.0;
  for (int what = 0; what < 2 + n_ref; ++what) {  // 0: the sum of squares, 1: the norm, 2 + o: observed row o
    if (what == 1 && !nab) continue;
    double s = 0.0;
    for (int64_t e = tid; e < n_pad; e += 256) {
      const double v = g[e];
      if (what == 0) {
        s = fma(v, v, s);
      } else if (what == 1) {
        const int32_t a = map[2 * e], b = map[2 * e + 1];
        if (a >= 0) s = fma(v * v, nab[(int64_t)a * P + b], s);
      } else {
        s = fma(Go[(int64_t)(what - 2) * n_pad + e], v, s);
      }
    }
    __syncthreads();  // the previous sum's reads of red are done
    red[tid] = s;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
      if (tid < d) red[tid] += red[tid + d];
      __syncthreads();
    }
    const double tot = red[0];
    if (what == 0) ss_j = tot;
    if (tid == 0) {
      if (what == 0)
        ss[j] = tot;
      else if (what == 1)
        norm[j] = tot;
      else
        match[j * n_ref + (what - 2)] = tot / sqrt(oss[what - 2] * ss_j);
    }
  }
}

struct ScrPairArgs {
  const double* X;    // [P][K][R_pad], K = 2 N: the cosine rows, then the sine rows
  const double* phi;  // [N] the template
  double* Y;          // [n_pad][R_pad]
  int32_t P, N, R_pad;
};

// grid: (R_pad / 16, lower tile pairs (ta, tb), tb <= ta, row by row)
__global__ __launch_bounds__(256) void k_scr_pairs(ScrPairArgs a) {
  // sX [row tile, column tile][realization][column of the chunk x 16 + pulsar] while the columns are walked, then sY
  // [pair of the tile pair][realization] in the same memory
  constexpr int kX = 2 * kScrYReal * kScrYLd, kY = 256 * (kScrYReal + 1);
  __shared__ double smem[kX > kY ? kX : kY];
  double(*sX)[kScrYReal][kScrYLd] = reinterpret_cast<double(*)[kScrYReal][kScrYLd]>(smem);
  double(*sY)[kScrYReal + 1] = reinterpret_cast<double(*)[kScrYReal + 1]>(smem);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lg = lane >> 4;
  const int r0 = (int)blockIdx.x * kScrYReal, t = (int)blockIdx.y;
  int ta = 0;
  while ((ta + 1) * (ta + 2) / 2 <= t) ++ta;
  const int tb = t - ta * (ta + 1) / 2;
  const int K = 2 * a.N;
  FPTA_DCHECK(r0 + kScrYReal <= a.R_pad, "k_scr_pairs realization", r0 + kScrYReal, a.R_pad + 1);
  d4 acc[4];
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) acc[rr] = d4{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < K; k0 += kScrYKc) {
    __syncthreads();  // the previous chunk's reads are done
#pragma unroll
    for (int i = 0; i < 2 * 16 * kScrYKc * kScrYReal / 256; ++i) {
      const int idx = tid + 256 * i, rr = idx & 15, p = (idx >> 4) & 15, kk = (idx >> 8) & (kScrYKc - 1),
                tile = idx >> 11;
      const int pp = (tile ? tb : ta) * 16 + p, k = k0 + kk;
      double v = 0.0;
      if (pp < a.P && k < K) v = a.X[((int64_t)pp * K + k) * a.R_pad + r0 + rr];
      sX[tile][rr][kk * 16 + p] = v;
    }
    __syncthreads();
#pragma unroll
    for (int step = 0; step < kScrYKc / 4; ++step) {
      const int kk = step * 4 + lg, k = k0 + kk;
      const double ph = k < K ? a.phi[k < a.N ? k : k - a.N] : 0.0;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int r = wave * 4 + rr;
        const double av = sX[0][r][kk * 16 + lr] * ph, bv = sX[1][r][kk * 16 + lr];
        acc[rr] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[rr], 0, 0, 0);
      }
    }
  }
  __syncthreads();  // the last chunk's reads are done: sY takes sX's place
  // accumulator register q of a lane: row (lane >> 4) + 4 q of the row tile, column lane & 15 of the column tile
#pragma unroll
  for (int rr = 0; rr < 4; ++rr)
#pragma unroll
    for (int q = 0; q < 4; ++q) sY[(lg + 4 * q) * 16 + lr][wave * 4 + rr] = acc[rr][q];
  __syncthreads();
  const int rr = tid & 15;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int pl = (tid >> 4) + 16 * i;
    const int64_t pa = ta * 16 + (pl >> 4), pb = tb * 16 + (pl & 15);
    if (pa < a.P && pb < pa)  // the strict lower triangle: pair pa (pa - 1) / 2 + pb < n_pair
      a.Y[(pa * (pa - 1) / 2 + pb) * a.R_pad + r0 + rr] = sY[pl][rr];
  }
}

// Qs [J][R_pad] = Gs [J][n_pad] Y [n_pad][R_pad]. grid: (ceil(R_pad / 64), ceil(J / 128)), 4 waves as 2 x 2
__global__ __launch_bounds__(256) void k_scr_gemm(const double* __restrict__ Gs, const double* __restrict__ Y,
                                                   double* __restrict__ Qs, int32_t J, int64_t n_pad, int32_t R_pad) {
  __shared__ double sA[kScrK][kScrLdA];  // [pair of the chunk][scramble of the tile]
  __shared__ double sB[kScrK][kScrLdB];  // [pair of the chunk][realization of the tile]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lg = lane >> 4;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 32;
  const int64_t j0 = (int64_t)blockIdx.y * kScrM;
  const int r0 = (int)blockIdx.x * kScrN;
  d4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int n = 0; n < 2; ++n) acc[i][n] = d4{0.0, 0.0, 0.0, 0.0};
  for (int64_t k0 = 0; k0 < n_pad; k0 += kScrK) {
    __syncthreads();  // the previous chunk's reads are done
#pragma unroll
    for (int i = 0; i < kScrM * kScrK / 256; ++i) {
      const int idx = tid + 256 * i, k = idx & (kScrK - 1), j = idx / kScrK;
      sA[k][j] = j0 + j < J ? Gs[(j0 + j) * n_pad + k0 + k] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < kScrK * kScrN / 256; ++i) {
      const int idx = tid + 256 * i, r = idx & (kScrN - 1), k = idx / kScrN;
      sB[k][r] = r0 + r < R_pad ? Y[(k0 + k) * R_pad + r0 + r] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kScrK / 4; ++kk) {
      const int k = kk * 4 + lg;
      double av[4], bv[2];
#pragma unroll
      for (int i = 0; i < 4; ++i) av[i] = sA[k][wm + i * 16 + lr];
#pragma unroll
      for (int n = 0; n < 2; ++n) bv[n] = sB[k][wn + n * 16 + lr];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[i][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[i], bv[n], acc[i][n], 0, 0, 0);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t row = j0 + wm + i * 16 + lg + 4 * q;
        const int col = r0 + wn + n * 16 + lr;
        if (row < J && col < R_pad) Qs[row * R_pad + col] = acc[i][n][q];
      }
}

// The S/N of one matrix and realization: the observed ones and the scrambles' come from here
__device__ inline double scr_snr(double q, double norm) { return q / sqrt(norm); }

// One thread per realization. snr [n_orf][R_pad], cnt [n_orf][R_pad], mom [3][R_pad] (mean, std with ddof = 0, max),
// null NULL or [J][R_pad]. grid: (ceil(R_pad / 64)), 64 threads
__global__ __launch_bounds__(64) void k_scr_rank(const double* __restrict__ Q, const double* __restrict__ onorm,
                                                  int32_t n_orf, const double* __restrict__ Qs,
                                                  const double* __restrict__ norm, int32_t J, int32_t R_pad,
                                                  double* __restrict__ snr, int64_t* __restrict__ cnt,
                                                  double* __restrict__ mom, double* __restrict__ null) {
  const int r = (int)blockIdx.x * 64 + threadIdx.x;
  if (r >= R_pad) return;
  double sum = 0.0, mx = -INFINITY;
  for (int64_t j = 0; j < J; ++j) {
    const double v = scr_snr(Qs[j * R_pad + r], norm[j]);
    sum += v;
    mx = v > mx ? v : mx;
    if (null) null[j * R_pad + r] = v;
  }
  const double mean = sum / (double)J;
  double dev = 0.0;
  for (int64_t j = 0; j < J; ++j) {
    const double d = scr_snr(Qs[j * R_pad + r], norm[j]) - mean;
    dev = fma(d, d, dev);
  }
  mom[r] = mean;
  mom[R_pad + r] = sqrt(dev / (double)J);
  mom[2 * (int64_t)R_pad + r] = mx;
  for (int32_t o = 0; o < n_orf; ++o) {
    const double so = scr_snr(Q[(int64_t)o * R_pad + r], onorm[o]);
    int64_t n = 0;
    for (int64_t j = 0; j < J; ++j) n += scr_snr(Qs[j * R_pad + r], norm[j]) >= so ? 1 : 0;
    snr[(int64_t)o * R_pad + r] = so;
    cnt[(int64_t)o * R_pad + r] = n;
  }
}

// Every scramble through validate_one on up to 16 threads; the refusal of the first bad scramble is the one reported
static bool scr_validate(int64_t P, int64_t n_scr, const double* pos, const double* G, const double* nab,
                         std::string& why) {
  if (!fpta_scr::validate_shape(P, n_scr, pos, G, why)) return false;
  std::mutex mu;
  std::map<int64_t, std::string> bad;
  const unsigned hw = std::thread::hardware_concurrency();
  const int64_t work = n_scr * P * P;
  fpta_os::run_pool(n_scr, std::min<int64_t>({(int64_t)(hw ? hw : 1), 16, work >> 18, n_scr}), [&](int64_t j) {
    {
      std::lock_guard<std::mutex> lk(mu);
      if (!bad.empty() && bad.begin()->first < j) return;
    }
    std::string w;
    if (!fpta_scr::validate_one(P, j, pos, G, nab, w)) {
      std::lock_guard<std::mutex> lk(mu);
      bad[j] = w;
    }
  });
  if (bad.empty()) return true;
  why = bad.begin()->second;
  return false;
}

static int scr_stats_launch(fpta_ctx* c, const ScrSlot& s, const double* rows, int64_t n_rows, const double* nab,
                            int32_t P, int64_t n_pad, int32_t n_ref, double* norm, double* ss, double* match) {
  if (n_rows == 0) return FPTA_OK;
  k_scr_stats<<<dim3((unsigned)n_rows), dim3(256), 0, c->stream>>>(s.map.as<int32_t>(), rows, nab, P, n_pad, n_ref,
                                                                  s.go.as<double>(), s.oss.as<double>(), norm, ss,
                                                                  match);
  HIPCHK(c, hipGetLastError(), "k_scr_stats launch");
  return FPTA_OK;
}

// The pair rows of a validated set on the device with their norms and matches against n_orf observed matrices ref
// [n_orf][P][P] (device); nab (device) NULL: no norms. The stream is idle on return and the inputs are released.
static int scr_build(fpta_ctx* c, const char* who, ScrSlot& s, ScrState& st, int32_t P, int32_t n_scr,
                     const double* pos, const double* G, int32_t n_orf, const double* ref, const double* nab,
                     double* norm_out, double* match_out) {
  const int64_t n_pad = fpta_scr::n_pair_pad(P);
  std::vector<int32_t> map;
  fpta_scr::make_pair_map(P, map);
  st.clear();
  HIPCHK(c, hipStreamSynchronize(c->stream), "scrambles sync");  // a launch with the previous set may still read it
  const size_t b_in = sizeof(double) * (size_t)n_scr * (size_t)P * (pos ? 3 : (size_t)P);
  const size_t b_gs = sizeof(double) * (size_t)n_scr * (size_t)n_pad, b_go = sizeof(double) * (size_t)n_orf * (size_t)n_pad;
  int rc;
  if ((rc = upload(c, s.map, map.data(), sizeof(int32_t) * map.size(), "scrambles pair map"))) return rc;
  if (s.gs.ensure(b_gs) != hipSuccess || s.go.ensure(b_go) != hipSuccess ||
      s.norm.ensure(sizeof(double) * (size_t)n_scr) != hipSuccess ||
      s.ss.ensure(sizeof(double) * (size_t)n_scr) != hipSuccess ||
      s.match.ensure(sizeof(double) * (size_t)n_scr * (size_t)n_orf) != hipSuccess ||
      s.onorm.ensure(sizeof(double) * (size_t)n_orf) != hipSuccess ||
      s.oss.ensure(sizeof(double) * (size_t)n_orf) != hipSuccess || s.in.ensure(b_in) != hipSuccess)
    return fail(c, FPTA_ENOMEM, std::string(who) + ": no device memory for " + std::to_string(b_gs + b_go + b_in) +
                                    " bytes of pair rows and inputs");
  HIPCHK(c, hipMemcpyAsync(s.in.p, pos ? pos : G, b_in, hipMemcpyHostToDevice, c->stream), "scrambles upload");
  const unsigned gx = (unsigned)((n_pad + 255) / 256);
  if (n_orf > 0) {
    k_scr_orf<<<dim3(gx, (unsigned)n_orf), dim3(256), 0, c->stream>>>(s.map.as<int32_t>(), nullptr, ref, P, n_pad,
                                                                     s.go.as<double>());
    HIPCHK(c, hipGetLastError(), "k_scr_orf launch");
    if ((rc = scr_stats_launch(c, s, s.go.as<double>(), n_orf, nab, P, n_pad, 0, s.onorm.as<double>(),
                               s.oss.as<double>(), nullptr)))
      return rc;
  }
  if (n_scr > 0) {
    k_scr_orf<<<dim3(gx, (unsigned)n_scr), dim3(256), 0, c->stream>>>(
        s.map.as<int32_t>(), pos ? s.in.as<double>() : nullptr, pos ? nullptr : s.in.as<double>(), P, n_pad,
        s.gs.as<double>());
    HIPCHK(c, hipGetLastError(), "k_scr_orf launch");
    if ((rc = scr_stats_launch(c, s, s.gs.as<double>(), n_scr, nab, P, n_pad, n_orf, s.norm.as<double>(),
                               s.ss.as<double>(), s.match.as<double>())))
      return rc;
    if (norm_out && nab)
      HIPCHK(c, hipMemcpyAsync(norm_out, s.norm.p, sizeof(double) * (size_t)n_scr, hipMemcpyDeviceToHost, c->stream),
             "scrambles norm download");
    if (match_out && n_orf > 0)
      HIPCHK(c, hipMemcpyAsync(match_out, s.match.p, sizeof(double) * (size_t)n_scr * (size_t)n_orf,
                               hipMemcpyDeviceToHost, c->stream),
             "scrambles match download");
  }
  HIPCHK(c, hipStreamSynchronize(c->stream), "scrambles set sync");
  s.in.release();
  st.set = true;
  st.J = n_scr;
  st.n_orf = n_orf;
  st.n_pair = fpta_scr::n_pair(P);
  st.n_pad = n_pad;
  return FPTA_OK;
}

// The results' device memory for a block padded to R_pad realizations; before the timer entry opens
static int scr_ensure(fpta_ctx* c, const char* who, ScrSlot& s, const ScrState& st, int32_t P, int32_t R_pad,
                      bool want_null) {
  const size_t b_y = sizeof(double) * (size_t)st.n_pad * (size_t)R_pad, b_qs = sizeof(double) * (size_t)st.J * R_pad;
  const size_t b_o = sizeof(double) * (size_t)st.n_orf * (size_t)R_pad;
  if ((P + 15) / 16 > 360) return fail(c, FPTA_EINVAL, std::string(who) + ": too many pulsars");
  if (s.y.ensure(b_y) != hipSuccess || s.qs.ensure(b_qs) != hipSuccess || s.snr.ensure(b_o) != hipSuccess ||
      s.cnt.ensure(b_o) != hipSuccess || s.mom.ensure(sizeof(double) * 3 * (size_t)R_pad) != hipSuccess ||
      (want_null && s.null.ensure(b_qs) != hipSuccess))
    return fail(c, FPTA_ENOMEM, std::string(who) + ": no device memory for " +
                                    std::to_string(b_y + (want_null ? 2 : 1) * b_qs + 2 * b_o) + " bytes of results");
  return FPTA_OK;
}

// Stages 3 to 5 on the coefficients and the observed Q that os_launch_unbooked left in the slot
static int scr_launch(fpta_ctx* c, const OsSlot& os, const OsState& ost, ScrSlot& s, const ScrState& st, int32_t P,
                      bool want_null) {
  const int32_t R_pad = ost.rpad;
  if (st.n_pad > st.n_pair)
    HIPCHK(c, hipMemsetAsync(s.y.as<double>() + st.n_pair * R_pad, 0,
                             sizeof(double) * (size_t)(st.n_pad - st.n_pair) * (size_t)R_pad, c->stream),
           "scrambles pair padding");
  ScrPairArgs a;
  a.X = os.x.coef.as<double>();
  a.phi = os.phi.as<double>();
  a.Y = s.y.as<double>();
  a.P = P;
  a.N = ost.N;
  a.R_pad = R_pad;
  const int n_tile = (P + 15) / 16;
  k_scr_pairs<<<dim3((unsigned)(R_pad / kScrYReal), (unsigned)(n_tile * (n_tile + 1) / 2)), dim3(256), 0, c->stream>>>(a);
  HIPCHK(c, hipGetLastError(), "k_scr_pairs launch");
  k_scr_gemm<<<dim3((unsigned)((R_pad + kScrN - 1) / kScrN), (unsigned)((st.J + kScrM - 1) / kScrM)), dim3(256), 0,
               c->stream>>>(s.gs.as<double>(), s.y.as<double>(), s.qs.as<double>(), st.J, st.n_pad, R_pad);
  HIPCHK(c, hipGetLastError(), "k_scr_gemm launch");
  k_scr_rank<<<dim3((unsigned)((R_pad + 63) / 64)), dim3(64), 0, c->stream>>>(
      os.q.as<double>(), s.onorm.as<double>(), st.n_orf, s.qs.as<double>(), s.norm.as<double>(), st.J, R_pad,
      s.snr.as<double>(), s.cnt.as<int64_t>(), s.mom.as<double>(), want_null ? s.null.as<double>() : nullptr);
  HIPCHK(c, hipGetLastError(), "k_scr_rank launch");
  return FPTA_OK;
}

// The wanted results, unpadded
static int scr_results(fpta_ctx* c, const ScrSlot& s, const ScrState& st, int32_t R, int32_t R_pad, double* snr_obs,
                       int64_t* count_ge, double* mean, double* sd, double* mx, double* snr_null) {
  int rc;
  if (snr_obs && (rc = fit_download(c, s.snr, st.n_orf, R, R_pad, snr_obs))) return rc;
  if (count_ge && (rc = fit_download(c, s.cnt, st.n_orf, R, R_pad, reinterpret_cast<double*>(count_ge)))) return rc;
  if (R > 0) {
    const double* mom = s.mom.as<double>();
    double* const out[3] = {mean, sd, mx};
    for (int i = 0; i < 3; ++i)
      if (out[i])
        HIPCHK(c, hipMemcpyAsync(out[i], mom + (int64_t)i * R_pad, sizeof(double) * (size_t)R, hipMemcpyDeviceToHost,
                                 c->stream),
               "scrambles moments download");
  }
  if (snr_null && (rc = fit_download(c, s.null, st.J, R, R_pad, snr_null))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream), "scrambles sync");
  return FPTA_OK;
}

}  // namespace capi

using namespace capi;

extern "C" int fpta_batch_set_os_scrambles(fpta_ctx* c, int32_t n_scr, const double* pos, const double* G,
                                           double* norm_out, double* match_out) {
  if (!c) return fail(nullptr, FPTA_EINVAL, "null ctx");
  if (!c->os_st.set) return fail(c, FPTA_ESTATE, "set_os_scrambles: no optimal statistic is set (set_os first)");
  if (n_scr == 0) {
    c->scr_st.clear();
    return FPTA_OK;
  }
  const int32_t P = c->batch.P;
  std::string why;
  if (!scr_validate(P, n_scr, pos, G, c->os.h_nab.data(), why)) return fail(c, FPTA_EINVAL, "set_os_scrambles: " + why);
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  return scr_build(c, "set_os_scrambles", c->scr, c->scr_st, P, n_scr, pos, G, c->os_st.J, c->os.g.as<double>(),
                   c->os.nab.as<double>(), norm_out, match_out);
}

extern "C" int fpta_batch_os_scrambles_info(fpta_ctx* c, int64_t* info) {
  if (!c || !info) return fail(c, FPTA_EINVAL, "os_scrambles_info: bad arguments");
  const ScrState& st = c->scr_st;  // all zero while no scrambles are set
  const int64_t v[4] = {st.J, st.n_orf, st.n_pair, st.R};
  std::copy(v, v + 4, info);
  return FPTA_OK;
}

extern "C" int fpta_batch_os_scrambles(fpta_ctx* c, double* snr_obs, int64_t* count_ge, double* mean, double* sd,
                                       double* mx, double* snr_null) {
  Block b;
  int rc;
  if ((rc = block_check(c, "os_scrambles", false, b))) return rc;
  OsState& ost = c->os_st;
  ScrState& st = c->scr_st;
  if (!ost.set) return fail(c, FPTA_ESTATE, "os_scrambles: no optimal statistic is set (set_os first)");
  if (!st.set) return fail(c, FPTA_ESTATE, "os_scrambles: no sky scrambles are set (set_os_scrambles first)");
  if ((rc = block_open(c, false))) return rc;
  ost.R = st.R = 0;
  const int32_t R_pad = (b.R + kOsRpad - 1) / kOsRpad * kOsRpad;
  if ((rc = scr_ensure(c, "os_scrambles", c->scr, st, b.n_psr, R_pad, snr_null != nullptr))) return rc;
  {
    KTimer kt(c, FPTA_K_DENSE);
    if ((rc = os_launch_unbooked(c, b, c->os, ost))) return rc;
    if (ost.rpad != R_pad) return fail(c, FPTA_EINVAL, "os_scrambles: k_fit_apply's realization padding changed");
    if ((rc = scr_launch(c, c->os, ost, c->scr, st, b.n_psr, snr_null != nullptr))) return rc;
  }
  ost.R = st.R = b.R;
  st.rpad = R_pad;
  return scr_results(c, c->scr, st, b.R, R_pad, snr_obs, count_ge, mean, sd, mx, snr_null);
}

extern "C" int fpta_os_scrambles(fpta_ctx* c, int32_t n_psr, const int64_t* offs, const double* toas, const double* nu,
                                 int32_t n_comp, const int32_t* n_modes, const double* f, int32_t f_is_common,
                                 const double* idx, const double* freqf, const double* phi, const uint8_t* mask,
                                 int32_t target, const double* phi_hat, int32_t n_col, const double* M,
                                 const int32_t* ncol_psr, const double* weights, double rcond, int32_t n_g,
                                 const double* G, int32_t n_scr, const double* scr_pos, const double* scr_G,
                                 int32_t n_vec, const double* res, double* Q, double* X, double* norm_out,
                                 double* match_out, double* snr_obs, int64_t* count_ge, double* mean, double* sd,
                                 double* mx, double* snr_null, double* qs, double* nab_out) {
  const OneShot one{c, "os_scrambles", n_psr, offs, n_vec, res};
  int rc;
  if ((rc = one.check())) return rc;
  std::string why;
  fpta_os::Plan plan;
  const fpta_os::Spec sp = fpta_os::make_spec(fpta_fit::make_spec(n_comp, n_modes, f, f_is_common, idx, freqf), phi,
                                              mask, target, phi_hat);
  const int made = fpta_os::make_plan(n_psr, offs, toas, nu, sp, n_col, M, ncol_psr, weights, rcond, n_g, G, plan, why);
  if ((rc = one.planned(made, why))) return rc;
  if (n_scr < 1) return fail(c, FPTA_EINVAL, "os_scrambles: at least one scramble is needed");
  if (!scr_validate(n_psr, n_scr, scr_pos, scr_G, plan.Nab.data(), why))
    return fail(c, FPTA_EINVAL, "os_scrambles: " + why);
  if (nab_out) std::copy(plan.Nab.begin(), plan.Nab.end(), nab_out);
  Block b{nullptr, 0, 0, n_psr};
  if (n_vec > 0 && (rc = one.upload(b))) return rc;
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  if ((rc = os_upload(c, plan, n_psr, offs, phi_hat, n_g, G, c->os1))) return rc;
  ScrState st;
  if ((rc = scr_build(c, "os_scrambles", c->scr1, st, n_psr, n_scr, scr_pos, scr_G, n_g, c->os1.g.as<double>(),
                      c->os1.nab.as<double>(), norm_out, match_out)))
    return rc;
  if (n_vec == 0) return FPTA_OK;
  OsState ost{true, plan.K, plan.N, n_g};
  const int32_t R_pad = (n_vec + kOsRpad - 1) / kOsRpad * kOsRpad;
  if ((rc = scr_ensure(c, "os_scrambles", c->scr1, st, n_psr, R_pad, snr_null != nullptr))) return rc;
  {
    KTimer kt(c, FPTA_K_DENSE);
    if ((rc = os_launch_unbooked(c, b, c->os1, ost))) return rc;
    if (ost.rpad != R_pad) return fail(c, FPTA_EINVAL, "os_scrambles: k_fit_apply's realization padding changed");
    if ((rc = scr_launch(c, c->os1, ost, c->scr1, st, n_psr, snr_null != nullptr))) return rc;
  }
  if ((rc = os_results(c, b, c->os1, ost, Q, nullptr, X))) return rc;
  if ((rc = scr_results(c, c->scr1, st, n_vec, R_pad, snr_obs, count_ge, mean, sd, mx, snr_null))) return rc;
  if (qs && (rc = fit_download(c, c->scr1.qs, st.J, n_vec, R_pad, qs))) return rc;
  return one.done();
}

extern "C" int fpta_os_scramble_match(fpta_ctx* c, int32_t n_psr, int32_t n_scr, const double* pos, int32_t n_ref,
                                      const double* ref, double* match_out, double* rows_out) {
  if (!c) return fail(nullptr, FPTA_EINVAL, "null ctx");
  if (n_ref < 1 || !ref || !match_out) return fail(c, FPTA_EINVAL, "os_scramble_match: bad arguments");
  std::string why;
  if (!scr_validate(n_psr, n_scr, pos, nullptr, nullptr, why)) return fail(c, FPTA_EINVAL, "os_scramble_match: " + why);
  for (int64_t i = 0; i < (int64_t)n_ref * n_psr * n_psr; ++i)
    if (!std::isfinite(ref[i]) && i / n_psr % n_psr != i % n_psr)
      return fail(c, FPTA_EINVAL, "os_scramble_match: reference matrix " + std::to_string(i / ((int64_t)n_psr * n_psr)) +
                                      " is not finite");
  if (n_scr == 0) return FPTA_OK;
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  int rc;
  // the one-shot statistic's slot holds the reference matrices; its own tables are rebuilt by its next call
  if ((rc = upload(c, c->os1.g, ref, sizeof(double) * (size_t)n_ref * (size_t)n_psr * (size_t)n_psr,
                   "os_scramble_match reference")))
    return rc;
  ScrState st;
  if ((rc = scr_build(c, "os_scramble_match", c->scr1, st, n_psr, n_scr, pos, nullptr, n_ref, c->os1.g.as<double>(),
                      nullptr, nullptr, match_out)))
    return rc;
  if (rows_out) {
    HIPCHK(c, hipMemcpy2DAsync(rows_out, sizeof(double) * (size_t)st.n_pair, c->scr1.gs.p,
                               sizeof(double) * (size_t)st.n_pad, sizeof(double) * (size_t)st.n_pair, (size_t)n_scr,
                               hipMemcpyDeviceToHost, c->stream),
           "os_scramble_match rows download");
    HIPCHK(c, hipStreamSynchronize(c->stream), "os_scramble_match sync");
  }
  return FPTA_OK;
}
