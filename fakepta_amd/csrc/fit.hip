// Fourier fit (fpta_batch_set_fit, fpta_batch_fit, fpta_batch_fit_cross, fpta_fit_coefficients): the Fourier
// coefficients a = A_p r of every realization of a block [R][ld], with the per-pulsar operator A_p [K][n_p] of
// fit_host.h, and the cross-spectrum of an array from them, both on v_mfma_f64_16x16x4_f64.
//
//   k_fit_apply<NS>  one pulsar x one tile of 32 realizations per workgroup of 8 waves. The block tile is read from
//                    memory once: per chunk of 64 TOAs wave w loads 16 TOAs (w >> 1) of 16 realizations (w & 1), lane
//                    (lr, lg) two 16-byte runs of its own row (TOAs 2 lg, 2 lg + 1 and 8 + 2 lg, 9 + 2 lg of the 16, as
//                    k_tm_project does), and puts them into LDS lane by lane: [pair of k-steps][half][lane], two
//                    buffers, one barrier per chunk. A k-step's B operand is then what the same lane of the loading
//                    wave held (the reduction index may be any fixed permutation of the TOAs), and its A operand is
//                    A_p[row lr of a 16-row group][that TOA], read from memory (the L2) as 16-byte runs of the row.
//                    NS = 1 (K > 64): wave w owns the row groups w, w + 8, w + 16, w + 24 and takes every k-step, so
//                    no sum across waves is needed. NS = 2, 4, 8 (K <= 64, 32, 16): 8 / NS row groups, and the k-step
//                    pairs of a chunk are dealt to NS waves per group (pair i to slice i mod NS); the slices' partial
//                    sums go through LDS once at the end and are added in slice order.
//   k_fit_cross      X[m][a][b] = sum_r (cos_a cos_b + sin_a sin_b) of mode m: one wave per mode and lower 16 x 16
//                    tile of pulsar pairs, the cosine row first and then the sine row, 8 realizations per load pair;
//                    the tile's lower triangle is stored and mirrored by the same lane.
// No atomics and no dependence on the neighbours: a realization's coefficients are the same whatever R, its position in
// the block and the realizations that share its tile. Rows of the block start at offs[p] and rows of A_p at any
// multiple of n_p: 8-byte aligned only, so their 16-byte accesses are typed 8-byte aligned. The pulsar's last, partial
// chunk reads at clamped indices and zeroes what lies past the end; a lane past the last realization reads the last
// one and stores nothing; the coefficient buffer is cleared before the launch, so rows of dropped columns, pulsars
// without a kept column and the padding realizations are zero.
#include "capi_host.h"
#include "fit_host.h"
#include "device_common.h"

namespace __attribute__((visibility("hidden"))) capi {

constexpr int kFitWaves = 8;    // waves of a workgroup
constexpr int kFitReal = 32;    // realizations of a tile: two MFMA column blocks
constexpr int kFitChunk = 64;   // TOAs of a chunk: four 16-TOA loads x two realization halves = one load per wave
constexpr int kFitPairs = 8;    // k-step pairs of a chunk (a pair: the two TOAs of one 16-byte run)
constexpr int kFitRpad = 32;    // the coefficient buffer's realization padding
static_assert(kFitChunk == 16 * (kFitWaves / 2) && kFitPairs * 8 == kFitChunk && kFitReal == 32,
              "k_fit_apply's loader gives every wave one 16-TOA x 16-realization load per chunk");

typedef double d2u __attribute__((ext_vector_type(2), aligned(8)));  // two doubles at an 8-byte aligned address
typedef double d2 __attribute__((ext_vector_type(2)));

struct FitArgs {
  const double* res;    // [R][ld]
  int64_t ld;
  int32_t R, n_rt;      // realizations, tiles of kFitReal of them
  int32_t K, R_pad;     // rows of every operator; the leading dimension of coef
  const double* A;      // pulsar p's operator [K][n_p] at K offs[p]
  const int64_t* offs;  // [n_psr + 1]
  const int32_t* rank;  // [n_psr] kept Fourier columns
  double* coef;         // [n_psr][K][R_pad]
};

// grid: n_psr x n_rt workgroups, the realization tile fastest (neighbours share a pulsar's operator in the L2)
template <int NS>
__global__ __launch_bounds__(64 * kFitWaves) void k_fit_apply(FitArgs a) {
  constexpr int GP = kFitWaves / NS;      // row groups in flight at once
  constexpr int JMAX = NS == 1 ? 4 : 1;   // row groups of a wave
  __shared__ __attribute__((aligned(16))) double sRaw[2 * kFitPairs * 2 * 64 * 2];  // 32 KB
  d2* sX = (d2*)sRaw;  // [buffer][pair][half][lane]
  const int p = (int)(blockIdx.x / (unsigned)a.n_rt), rt = (int)(blockIdx.x - (unsigned)p * (unsigned)a.n_rt);
  if (a.rank[p] == 0) return;  // no kept column: the cleared buffer is the result
  const int64_t o = a.offs[p];
  const int n = (int)(a.offs[p + 1] - o);
  if (n <= 0) return;
  const int K = a.K, G = (K + 15) >> 4;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lg = lane >> 4;
  FPTA_DCHECK(o + n <= a.ld, "k_fit_apply row", o + n, a.ld + 1);

  // the loader's share: 16 TOAs (sc) of 16 realizations (half)
  const int half = wave & 1, sc = wave >> 1;
  const int lreal = rt * kFitReal + half * 16 + lr;
  const double* __restrict__ row = a.res + (int64_t)(lreal < a.R ? lreal : a.R - 1) * a.ld + o;
  // the worker's share: row groups gw, gw + GP, .. and the pairs slice, slice + NS, ..
  const int gw = wave % GP, slice = wave / GP;
  const int ng = gw < G ? (G - gw + GP - 1) / GP : 0;
  const double* __restrict__ Ap = a.A + (int64_t)K * o;
  const int n_chunks = (n + kFitChunk - 1) / kFitChunk;

  d4 acc[JMAX][2];
#pragma unroll
  for (int j = 0; j < JMAX; ++j) acc[j][0] = acc[j][1] = d4{0.0, 0.0, 0.0, 0.0};

  auto load = [&](int c, d2& x0, d2& x1) {
    const int t0 = c * kFitChunk + sc * 16;
    if (t0 + 16 <= n) {  // wave-uniform
      const d2u u0 = *(const d2u*)(row + t0 + 2 * lg), u1 = *(const d2u*)(row + t0 + 8 + 2 * lg);
      x0 = d2{u0.x, u0.y};
      x1 = d2{u1.x, u1.y};
    } else {
      double v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int t = t0 + ((q >> 1) << 3) + 2 * lg + (q & 1);
        const double x = row[t < n ? t : n - 1];
        v[q] = t < n ? x : 0.0;
      }
      x0 = d2{v[0], v[1]};
      x1 = d2{v[2], v[3]};
    }
  };
  auto put = [&](int buf, const d2& x0, const d2& x1) {
    sX[((buf * kFitPairs + 2 * sc) * 2 + half) * 64 + lane] = x0;
    sX[((buf * kFitPairs + 2 * sc + 1) * 2 + half) * 64 + lane] = x1;
  };
  // one pair of k-steps of chunk c: the TOAs base + 2 lg and base + 2 lg + 1 of lane group lg
  auto pair_step = [&](int c, int buf, int pr, bool full) {
    const int base = c * kFitChunk + (pr >> 1) * 16 + (pr & 1) * 8;
    const d2 b0 = sX[((buf * kFitPairs + pr) * 2 + 0) * 64 + lane];
    const d2 b1 = sX[((buf * kFitPairs + pr) * 2 + 1) * 64 + lane];
#pragma unroll
    for (int j = 0; j < JMAX; ++j)
      if (j < ng) {  // wave-uniform
        const int r = 16 * (gw + j * GP) + lr;
        const double* __restrict__ ar = Ap + (int64_t)(r < K ? r : K - 1) * n;
        double a0, a1;
        if (full) {
          const d2u u = *(const d2u*)(ar + base + 2 * lg);
          a0 = u.x;
          a1 = u.y;
        } else {
          const int t = base + 2 * lg;
          const double v0 = ar[t < n ? t : n - 1], v1 = ar[t + 1 < n ? t + 1 : n - 1];
          a0 = t < n ? v0 : 0.0;
          a1 = t + 1 < n ? v1 : 0.0;
        }
        acc[j][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0.x, acc[j][0], 0, 0, 0);
        acc[j][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1.x, acc[j][1], 0, 0, 0);
        acc[j][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0.y, acc[j][0], 0, 0, 0);
        acc[j][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1.y, acc[j][1], 0, 0, 0);
      }
  };

  {
    d2 x0, x1;
    load(0, x0, x1);
    put(0, x0, x1);
  }
  __syncthreads();
  for (int c = 0; c < n_chunks; ++c) {
    const int buf = c & 1;
    const bool more = c + 1 < n_chunks;
    d2 x0 = d2{0.0, 0.0}, x1 = d2{0.0, 0.0};
    if (more) load(c + 1, x0, x1);  // in flight during this chunk's k-steps
    if ((c + 1) * kFitChunk <= n) {
#pragma unroll
      for (int i = 0; i < kFitPairs / NS; ++i) pair_step(c, buf, slice + i * NS, true);
    } else {
#pragma unroll
      for (int i = 0; i < kFitPairs / NS; ++i) {
        const int pr = slice + i * NS;
        if (c * kFitChunk + pr * 8 < n) pair_step(c, buf, pr, c * kFitChunk + pr * 8 + 8 <= n);
      }
    }
    if (more) put(buf ^ 1, x0, x1);
    __syncthreads();
  }

  if (NS > 1) {
    // the slices' partial sums of a row group, added in slice order by every wave of the group
    double* sRed = sRaw;  // [wave][half x register][lane]; the last barrier above freed the staging buffers
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int q = 0; q < 4; ++q) sRed[(wave * 8 + h * 4 + q) * 64 + lane] = acc[0][h][q];
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        double v = sRed[(gw * 8 + h * 4 + q) * 64 + lane];
#pragma unroll
        for (int s = 1; s < NS; ++s) v += sRed[((gw + s * GP) * 8 + h * 4 + q) * 64 + lane];
        acc[0][h][q] = v;
      }
    if (slice != 0) return;
  }
#pragma unroll
  for (int j = 0; j < JMAX; ++j)
    if (j < ng) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int real = rt * kFitReal + h * 16 + lr;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int r = 16 * (gw + j * GP) + lg + 4 * q;
          if (r < K && real < a.R) a.coef[((int64_t)p * K + r) * a.R_pad + real] = acc[j][h][q];
        }
      }
    }
}

struct CrossArgs {
  const double* coef;   // [P][K][R_pad], zero past the last realization
  int32_t P, K, R_pad, n_tile;
  const int32_t* rows;  // [n_mode][2] the cosine and sine row of every mode
  double* X;            // [n_mode][P][P]
};

// grid: (n_tile^2, n_mode) single-wave workgroups; a tile above the diagonal returns at once
__global__ __launch_bounds__(64) void k_fit_cross(CrossArgs a) {
  const int ta = (int)(blockIdx.x / (unsigned)a.n_tile), tb = (int)(blockIdx.x - (unsigned)ta * (unsigned)a.n_tile);
  if (tb > ta) return;
  const int m = (int)blockIdx.y, lane = threadIdx.x & 63, lr = lane & 15, lg = lane >> 4;
  const int pa = min(ta * 16 + lr, a.P - 1), pb = min(tb * 16 + lr, a.P - 1);
  d4 acc = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int cs = 0; cs < 2; ++cs) {
    const int r = a.rows[2 * m + cs];
    const double* __restrict__ xa = a.coef + ((int64_t)pa * a.K + r) * a.R_pad + 2 * lg;
    const double* __restrict__ xb = a.coef + ((int64_t)pb * a.K + r) * a.R_pad + 2 * lg;
    for (int r0 = 0; r0 < a.R_pad; r0 += 8) {
      const d2 va = *(const d2*)(xa + r0), vb = *(const d2*)(xb + r0);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(va.x, vb.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(va.y, vb.y, acc, 0, 0, 0);
    }
  }
  double* __restrict__ X = a.X + (int64_t)m * a.P * a.P;
  const int ib = tb * 16 + lr;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int ia = ta * 16 + lg + 4 * q;
    if (ia < a.P && ib <= ia) {
      X[(int64_t)ia * a.P + ib] = acc[q];
      X[(int64_t)ib * a.P + ia] = acc[q];
    }
  }
}

// What a launch may allocate or refuse: the slot's coefficient buffer [n_psr][K][R_pad] and the grid bound
static int fit_size(fpta_ctx* c, const Block& b, int32_t K, FitSlot& s, int32_t& R_pad, size_t& bytes) {
  R_pad = (b.R + kFitRpad - 1) / kFitRpad * kFitRpad;
  bytes = sizeof(double) * (size_t)b.n_psr * (size_t)K * (size_t)R_pad;
  if (s.coef.ensure(bytes) != hipSuccess)
    return fail(c, FPTA_ENOMEM, "fit: no device memory for " + std::to_string(bytes) + " bytes of coefficients");
  if ((int64_t)b.n_psr * ((b.R + kFitReal - 1) / kFitReal) > 0x7FFFFFFF)
    return fail(c, FPTA_EINVAL, "fit: too many pulsars x realization tiles");
  return FPTA_OK;
}

// Clears the sized buffer and runs k_fit_apply on the block against the slot's tables
static int fit_run(fpta_ctx* c, const Block& b, int32_t K, const FitSlot& s, int32_t R_pad, size_t bytes) {
  FitArgs a;
  a.res = b.res;
  a.ld = b.ld;
  a.R = b.R;
  a.n_rt = (b.R + kFitReal - 1) / kFitReal;
  a.K = K;
  a.R_pad = R_pad;
  a.A = s.a.as<double>();
  a.offs = s.offs.as<int64_t>();
  a.rank = s.rows.as<int32_t>();
  a.coef = s.coef.as<double>();
  const int64_t blocks = (int64_t)b.n_psr * a.n_rt;
  HIPCHK(c, hipMemsetAsync(s.coef.p, 0, bytes, c->stream), "fit coefficients clear");
  if (blocks == 0) return FPTA_OK;
  const dim3 grid((unsigned)blocks), block(64 * kFitWaves);
  if (K <= 16)
    k_fit_apply<8><<<grid, block, 0, c->stream>>>(a);
  else if (K <= 32)
    k_fit_apply<4><<<grid, block, 0, c->stream>>>(a);
  else if (K <= 64)
    k_fit_apply<2><<<grid, block, 0, c->stream>>>(a);
  else
    k_fit_apply<1><<<grid, block, 0, c->stream>>>(a);
  HIPCHK(c, hipGetLastError(), "k_fit_apply launch");
  return FPTA_OK;
}

int fit_launch_unbooked(fpta_ctx* c, const Block& b, int32_t K, FitSlot& s, int32_t& R_pad) {
  size_t bytes = 0;
  const int rc = fit_size(c, b, K, s, R_pad, bytes);
  return rc ? rc : fit_run(c, b, K, s, R_pad, bytes);
}

// One FPTA_K_DENSE entry around the clear and the launch: the buffer is sized before the entry starts
int fit_launch(fpta_ctx* c, const Block& b, int32_t K, FitSlot& s, int32_t& R_pad) {
  size_t bytes = 0;
  const int rc = fit_size(c, b, K, s, R_pad, bytes);
  if (rc) return rc;
  KTimer kt(c, FPTA_K_DENSE);
  return fit_run(c, b, K, s, R_pad, bytes);
}

// Device copies of an operator slot's tables. The operator is the large one (8 K n_toa bytes): a failed allocation
// says so.
int fit_upload(fpta_ctx* c, const char* who, FitSlot& s, int32_t K, const std::vector<double>& A, int32_t n_psr,
               const int64_t* offs, const std::vector<int32_t>& rows) {
  const std::string w(who);
  const size_t bytes = sizeof(double) * A.size();
  if (s.a.ensure(bytes) != hipSuccess)
    return fail(c, FPTA_ENOMEM, w + ": no device memory for the operator of " + std::to_string(bytes) +
                                    " bytes (8 K n_toa, K = " + std::to_string(K) + ")");
  int rc;
  if ((rc = upload(c, s.a, A.data(), bytes, (w + " operator").c_str()))) return rc;
  if ((rc = upload(c, s.offs, offs, sizeof(int64_t) * ((size_t)n_psr + 1), (w + " offs").c_str()))) return rc;
  if ((rc = upload(c, s.rows, rows.data(), sizeof(int32_t) * (size_t)n_psr, (w + " rows").c_str()))) return rc;
  return FPTA_OK;
}

// coef [n_psr][K][R_pad] on the device -> host [n_psr][K][R]
int fit_download(fpta_ctx* c, const DevBuf& coef, int64_t rows, int32_t R, int32_t R_pad, double* host) {
  if (rows > 0 && R > 0)
    HIPCHK(c, hipMemcpy2DAsync(host, sizeof(double) * (size_t)R, coef.p, sizeof(double) * (size_t)R_pad,
                               sizeof(double) * (size_t)R, (size_t)rows, hipMemcpyDeviceToHost, c->stream),
           "fit download");
  HIPCHK(c, hipStreamSynchronize(c->stream), "fit sync");
  return FPTA_OK;
}

}  // namespace capi

using namespace capi;

extern "C" int fpta_batch_set_fit(fpta_ctx* c, int32_t n_comp, const int32_t* n_modes, const double* f,
                                  int32_t f_is_common, const double* idx, const double* freqf, int32_t n_col,
                                  const double* M, const int32_t* ncol_psr, const double* weights, double rcond,
                                  int32_t* rank_out, uint8_t* kept_out) {
  if (!c) return fail(nullptr, FPTA_EINVAL, "null ctx");
  const Layout& L = c->batch;
  if (L.P <= 0) return fail(c, FPTA_ESTATE, "set_fit: set_toas first");
  if (n_comp == 0) {
    c->fit_st.clear();
    if (rank_out) std::fill(rank_out, rank_out + L.P, 0);
    return FPTA_OK;
  }
  // everything is validated and the operator built here, before anything is uploaded
  std::string why;
  fpta_fit::Plan plan;
  const fpta_fit::Spec sp = fpta_fit::make_spec(n_comp, n_modes, f, f_is_common, idx, freqf);
  const int made = fpta_fit::make_plan(L.P, L.h_offs.data(), L.h_toas.data(), L.h_nu.data(), sp, n_col, M, ncol_psr,
                                       weights, rcond, plan, why);
  if (made) return fail(c, made == 2 ? FPTA_ENOMEM : FPTA_EINVAL, "set_fit: " + why);
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  c->fit_st.clear();
  // a fit with the previous operator may still read the tables (an upload into a buffer that does not grow)
  HIPCHK(c, hipStreamSynchronize(c->stream), "set_fit sync");
  int rc;
  if ((rc = fit_upload(c, "fit", c->fit, plan.K, plan.A, L.P, L.h_offs.data(), plan.rank))) return rc;
  std::vector<int32_t> rows;
  for (int32_t k0 = 0, ci = 0; ci < n_comp; k0 += 2 * n_modes[ci], ++ci)
    for (int32_t k = 0; k < n_modes[ci]; ++k) {
      rows.push_back(k0 + k);
      rows.push_back(k0 + n_modes[ci] + k);
    }
  if ((rc = upload(c, c->cross_rows, rows.data(), sizeof(int32_t) * rows.size(), "fit mode rows"))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream), "set_fit sync");
  c->fit_st = FitState{true, sp.f_is_common, plan.K, (int32_t)(rows.size() / 2)};
  if (rank_out) std::copy(plan.rank.begin(), plan.rank.end(), rank_out);
  if (kept_out) std::copy(plan.kept.begin(), plan.kept.end(), kept_out);
  return FPTA_OK;
}

extern "C" int fpta_batch_fit_info(fpta_ctx* c, int64_t* info) {
  if (!c || !info) return fail(c, FPTA_EINVAL, "fit_info: bad arguments");
  const FitState& st = c->fit_st;  // all zero while no fit is set
  const int64_t v[4] = {st.K, st.modes, st.common ? 1 : 0, st.R};
  std::copy(v, v + 4, info);
  return FPTA_OK;
}

extern "C" int fpta_batch_fit(fpta_ctx* c, double* coef_host) {
  Block b;
  int rc;
  if ((rc = block_check(c, "fit", false, b))) return rc;
  FitState& st = c->fit_st;
  if (!st.set) return fail(c, FPTA_ESTATE, "fit: no fit is set (set_fit first)");
  if ((rc = block_open(c, false))) return rc;
  st.R = 0;
  if ((rc = fit_launch(c, b, st.K, c->fit, st.rpad))) return rc;
  st.R = b.R;
  if (coef_host) return fit_download(c, c->fit.coef, (int64_t)b.n_psr * st.K, st.R, st.rpad, coef_host);
  return FPTA_OK;
}

extern "C" int fpta_batch_fit_cross(fpta_ctx* c, double* out) {
  if (!c) return fail(nullptr, FPTA_EINVAL, "null ctx");
  const FitState& st = c->fit_st;
  if (!st.set || !st.R) return fail(c, FPTA_ESTATE, "fit_cross: no fit result (fpta_batch_fit first)");
  if (!st.common) return fail(c, FPTA_EINVAL, "fit_cross: the fit has per-pulsar frequencies; a common grid is needed");
  if (!out) return fail(c, FPTA_EINVAL, "fit_cross: null output");
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  const int32_t P = c->batch.P, n_tile = (P + 15) / 16;
  const size_t bytes = sizeof(double) * (size_t)st.modes * (size_t)P * (size_t)P;
  if (c->cross_x.ensure(bytes) != hipSuccess)
    return fail(c, FPTA_ENOMEM, "fit_cross: no device memory for " + std::to_string(bytes) + " bytes of cross-spectra");
  CrossArgs a;
  a.coef = c->fit.coef.as<double>();
  a.P = P;
  a.K = st.K;
  a.R_pad = st.rpad;
  a.n_tile = n_tile;
  a.rows = c->cross_rows.as<int32_t>();
  a.X = c->cross_x.as<double>();
  if (st.modes > 65535) return fail(c, FPTA_EINVAL, "fit_cross: too many modes");
  {
    KTimer kt(c, FPTA_K_DENSE);
    k_fit_cross<<<dim3((unsigned)(n_tile * n_tile), (unsigned)st.modes), dim3(64), 0, c->stream>>>(a);
    HIPCHK(c, hipGetLastError(), "k_fit_cross launch");
  }
  HIPCHK(c, hipMemcpyAsync(out, c->cross_x.p, bytes, hipMemcpyDeviceToHost, c->stream), "fit_cross download");
  HIPCHK(c, hipStreamSynchronize(c->stream), "fit_cross sync");
  return FPTA_OK;
}

extern "C" int fpta_fit_coefficients(fpta_ctx* c, int32_t n_psr, const int64_t* offs, const double* toas,
                                     const double* nu, int32_t n_comp, const int32_t* n_modes, const double* f,
                                     int32_t f_is_common, const double* idx, const double* freqf, int32_t n_col,
                                     const double* M, const int32_t* ncol_psr, const double* weights, double rcond,
                                     int32_t n_vec, const double* res, double* coef_out, int32_t* rank_out,
                                     uint8_t* kept_out) {
  const OneShot one{c, "fit_coefficients", n_psr, offs, n_vec, res};
  int rc;
  if ((rc = one.check())) return rc;
  std::string why;
  fpta_fit::Plan plan;
  const fpta_fit::Spec sp = fpta_fit::make_spec(n_comp, n_modes, f, f_is_common, idx, freqf);
  const int made = fpta_fit::make_plan(n_psr, offs, toas, nu, sp, n_col, M, ncol_psr, weights, rcond, plan, why);
  if ((rc = one.planned(made, why))) return rc;
  if (n_vec > 0 && n_psr > 0 && !coef_out) return fail(c, FPTA_EINVAL, "fit_coefficients: coef_out missing");
  if (rank_out) std::copy(plan.rank.begin(), plan.rank.end(), rank_out);
  if (kept_out) std::copy(plan.kept.begin(), plan.kept.end(), kept_out);
  if (n_psr == 0 || n_vec == 0) return FPTA_OK;
  const int64_t rows = (int64_t)n_psr * plan.K;
  if (one.n_toa() == 0 || plan.max_rank == 0) {  // nothing to launch: every coefficient is zero
    std::fill(coef_out, coef_out + rows * n_vec, 0.0);
    return FPTA_OK;
  }
  Block b;
  if ((rc = one.upload(b))) return rc;
  if ((rc = fit_upload(c, "fit", c->fit1, plan.K, plan.A, n_psr, offs, plan.rank))) return rc;
  int32_t R_pad = 0;
  if ((rc = fit_launch(c, b, plan.K, c->fit1, R_pad))) return rc;
  return fit_download(c, c->fit1.coef, rows, n_vec, R_pad, coef_out);  // its sync closes the call
}
