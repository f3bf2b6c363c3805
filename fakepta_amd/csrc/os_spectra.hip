// Optimal statistic under a noise spectrum per realization (fpta_batch_set_os_spectra, fpta_batch_os_spectra). The
// definition is in include/fakepta_amd.h; the per-pulsar plan B0_p = T_p^T P0_p^-1 and A_p = B0_p T_p is
// os_spectra_host.h's, the tables' validation spectra_host.h's.
//
//   tables   k_spectra_amp (spectra.hip, unchanged) turns each table of the call into [P or 1][nm][R_pad] amplitudes,
//            the numbers synth(spectra=...) used; a varied component without a table reads the layout's amplitudes
//   stage 1  z = B0_p r: k_fit_apply (fit.hip) on this file's operator slot, [P][q][R_pad]
//   stage 2  k_oss_solve: per (pulsar, realization) C = I + s A_p s as a packed lower triangle in LDS, beside up to 64
//            right-hand sides s o [A_p's target columns, z] stored as further rows of the same matrix. One pass of q
//            pivot steps factors C = L D L^T and eliminates the right-hand sides with the same rank-one updates (no
//            square root; one barrier per step); D^-1, then the back substitution on the target's trailing block (on
//            all q rows when a target mode of the realization has s = 0). W = C^-1 s [A_t, z] then gives
//            X_k = W_kz / s_k and Z_kj = W_kj / s_k, the form without a subtraction; a target mode with s_k = 0 takes
//            X_k = z_k - sum_i A_ki s_i W_iz and Z_kj = A_kj - sum_i A_ki s_i W_ij. Z' = phi_hat^(1/2) Z phi_hat^(1/2).
//            A workgroup of 256 threads takes kOssRW realizations of one pulsar in turn; A_p is read from global
//            memory (all workgroups of a pulsar read the same 8 q^2 bytes: L2). K + 1 > 64 right-hand sides are
//            split over workgroups, each with its own factorisation.
//   stage 3  k_oss_gram: N_ab[r] = <Z'_a, Z'_b> for a >= b on v_mfma_f64_16x16x4_f64, one wave per (realization, lower
//            16 x 16 pulsar tile pair), k over the K^2 entries in steps of 16 in index order
//   stage 4  k_oss_contract: norm[j][r] = sum_{a>b} G_j[a][b]^2 N_ab[r] and C_jj'[r] = sum_{a>b} G_j G_j' N_ab[r],
//            row-major over a > b, one thread per (result, realization)
//   stage 5  k_os_pairs, k_os_reduce (os.hip, unchanged) on X
// Stages 2 to 4 run per chunk of realizations (Z' is 8 K^2 P bytes per realization). Fixed operation order, no
// atomics, nothing shared between realizations.
#include "capi_host.h"
#include "os_spectra_host.h"
#include "spectra_host.h"
#include "device_common.h"

namespace __attribute__((visibility("hidden"))) capi {

constexpr int kOssRpad = 32;     // k_fit_apply's and k_os_pairs' realization padding
constexpr int kOssCols = 64;     // right-hand sides of a workgroup
constexpr int kOssRW = 4;        // realizations a workgroup takes in turn
constexpr int kOssChunk = 128;   // realizations of a chunk, at most
constexpr size_t kOssZpBytes = (size_t)1 << 30;  // Z' of a chunk, at most (one realization always runs)

// The amplitude of column k of a varied component for (pulsar p, realization r): amp[p pstride + k kstride + r rstride]
struct OssVar {
  const double* amp;
  int64_t pstride;
  int32_t kstride, rstride, n_modes, pad;
};

struct OssArgs {
  const double* A;      // [P][q][q]
  const double* z;      // [P][q][R_pad]
  const double* sph;    // [K] sqrt(phi_hat) over the target's columns
  OssVar v[fpta_oss::kMaxVary];
  double* X;            // [P][K][R_pad]
  double* Zp;           // [n_r][P][K][K] of this chunk
  int32_t n_vary, P, q, K, R_pad, r0, n_r;
};

// grid (ceil(n_r / kOssRW), P, ceil((K + 1) / kOssCols)); dynamic LDS: tri + nc q + 2 q doubles, tri = q (q + 1) / 2
__global__ __launch_bounds__(256) void k_oss_solve(OssArgs a) {
  extern __shared__ double lds[];
  const int q = a.q, K = a.K, tri = q * (q + 1) / 2, t0 = q - K;
  const int c0 = (int)blockIdx.z * kOssCols, nc = min(kOssCols, K + 1 - c0);
  double* Mx = lds;                   // rows i < q: the packed lower triangle; row q + c: right-hand side c [q]
  double* sS = lds + tri + nc * q;    // [q] s
  double* sIp = sS + q;               // [q] 1 / pivot
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, p = blockIdx.y;
  const double* Ap = a.A + (int64_t)p * q * q;
  auto at = [&](int i, int j) -> double& { return Mx[i < q ? i * (i + 1) / 2 + j : tri + (i - q) * q + j]; };
  for (int rr = 0; rr < kOssRW; ++rr) {
    const int rl = (int)blockIdx.x * kOssRW + rr;
    if (rl >= a.n_r) break;
    const int r = a.r0 + rl;
    double* Zp = a.Zp + ((int64_t)rl * a.P + p) * K * K;
    if (tid < q) {
      int j = tid, v = 0;
      while (j >= 2 * a.v[v].n_modes) j -= 2 * a.v[v++].n_modes;
      const OssVar& d = a.v[v];
      const int k = j < d.n_modes ? j : j - d.n_modes;
      sS[tid] = d.amp[(int64_t)p * d.pstride + (int64_t)k * d.kstride + (int64_t)r * d.rstride];
    }
    const int any0 = __syncthreads_or(tid >= t0 && tid < q && sS[tid] == 0.0);
    for (int i = ty; i < q; i += 16) {
      const double si = sS[i];
      for (int j = tx; j <= i; j += 16) at(i, j) = (i == j ? 1.0 : 0.0) + si * Ap[(int64_t)i * q + j] * sS[j];
    }
    for (int c = ty; c < nc; c += 16) {
      const int gc = c0 + c;
      for (int j = tx; j < q; j += 16)
        at(q + c, j) = sS[j] * (gc < K ? Ap[(int64_t)(t0 + gc) * q + j] : a.z[((int64_t)p * q + j) * a.R_pad + r]);
    }
    __syncthreads();
    // pivot step k: every row below (of C and of the right-hand sides) minus its multiple of row k, columns k + 1 ..
    for (int k = 0; k < q; ++k) {
      const double ip = 1.0 / at(k, k);
      if (tid == 0) sIp[k] = ip;
      for (int i = k + 1 + ty; i < q + nc; i += 16) {
        const double li = at(i, k) * ip;
        const int jmax = min(i, q - 1);
        for (int j = k + 1 + tx; j <= jmax; j += 16) at(i, j) -= li * at(j, k);
      }
      __syncthreads();
    }
    for (int c = ty; c < nc; c += 16)
      for (int j = tx; j < q; j += 16) at(q + c, j) *= sIp[j];
    __syncthreads();
    // L^T w = D^-1 L^-1 b on rows lo .. q - 1, from the last row up
    const int lo = any0 ? 0 : t0;
    for (int k = q - 1; k > lo; --k) {
      for (int c = ty; c < nc; c += 16) {
        const double wk = at(q + c, k);
        for (int i = lo + tx; i < k; i += 16) at(q + c, i) -= at(k, i) * sIp[i] * wk;
      }
      __syncthreads();
    }
    for (int c = tx; c < nc; c += 16) {
      const int gc = c0 + c;
      for (int kk = ty; kk < K; kk += 16) {
        const int i = t0 + kk;
        const double sk = sS[i];
        double w;
        if (sk > 0.0) {
          w = at(q + c, i) / sk;
        } else {
          double dot = 0.0;
          for (int j = 0; j < q; ++j) dot += Ap[(int64_t)i * q + j] * sS[j] * at(q + c, j);
          w = (gc < K ? Ap[(int64_t)i * q + t0 + gc] : a.z[((int64_t)p * q + i) * a.R_pad + r]) - dot;
        }
        if (gc < K)
          Zp[(int64_t)kk * K + gc] = a.sph[kk] * w * a.sph[gc];
        else
          a.X[((int64_t)p * K + kk) * a.R_pad + r] = w;
      }
    }
    __syncthreads();  // the next realization reuses the matrix
  }
}

// grid (lower tile pairs, n_r), one wave: N[r][a][b] for the tile pair's a >= b
__global__ __launch_bounds__(64) void k_oss_gram(const double* __restrict__ Zp, int32_t P, int32_t KK, int32_t n_tile,
                                                  double* __restrict__ nab) {
  const int lane = threadIdx.x, pl = lane & 15, kq = lane >> 4, rl = blockIdx.y;
  int ta = 0, tb = (int)blockIdx.x;
  while (tb > ta) tb -= ++ta;  // row by row of the lower triangle
  const int pa = ta * 16 + pl, pb = tb * 16 + pl;
  const double* za = Zp + ((int64_t)rl * P + min(pa, P - 1)) * KK;
  const double* zb = Zp + ((int64_t)rl * P + min(pb, P - 1)) * KK;
  d4 acc = {0.0, 0.0, 0.0, 0.0};
  // the trip count is the wave's (an MFMA needs every lane); K^2 is a multiple of 4, so a lane's four entries are all
  // inside or all outside
  for (int e0 = 0; e0 < KK; e0 += 16) {
    const int e = e0 + 4 * kq;
    double av[4], bv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      av[u] = pa < P && e < KK ? za[e + u] : 0.0;
      bv[u] = pb < P && e < KK ? zb[e + u] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc, 0, 0, 0);
  }
  double* out = nab + (int64_t)rl * P * P;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int ia = ta * 16 + kq + 4 * g, ib = tb * 16 + pl;
    if (ia < P && ib <= ia) out[(int64_t)ia * P + ib] = acc[g];
  }
}

// grid (ceil((J + n_orf^2) / 64), n_r): result `item` < J is norm[item], else C[j][j'] with (j, j') = item - J
__global__ __launch_bounds__(64) void k_oss_contract(const double* __restrict__ nab, const double* __restrict__ G,
                                                      int32_t J, int32_t n_orf, int32_t P, int32_t r0, int32_t R,
                                                      double* __restrict__ out) {
  const int item = blockIdx.x * 64 + threadIdx.x, rl = blockIdx.y;
  if (item >= J + n_orf * n_orf) return;
  const int j1 = item < J ? item : (item - J) / n_orf, j2 = item < J ? item : (item - J) % n_orf;
  const double* g1 = G + (int64_t)j1 * P * P;
  const double* g2 = G + (int64_t)j2 * P * P;
  const double* n = nab + (int64_t)rl * P * P;
  double s = 0.0;
  for (int a = 1; a < P; ++a)
    for (int64_t e = (int64_t)a * P; e < (int64_t)a * P + a; ++e) s += g1[e] * g2[e] * n[e];
  out[(int64_t)item * R + r0 + rl] = s;
}

static size_t oss_lds_bytes(int32_t q, int32_t K) {
  return sizeof(double) * ((size_t)q * (q + 1) / 2 + (size_t)std::min(kOssCols, K + 1) * q + 2 * (size_t)q);
}

// The tables of one call, validated already: uploads and k_spectra_amp per table into the slot, and the descriptors
static int oss_tables(fpta_ctx* c, Layout& L, const OssState& st, OssSlot& s, int32_t n_real, int32_t R_pad,
                      int32_t n_tab, const int32_t* seg, const int32_t* form, const int32_t* per_pulsar,
                      const double* const* tables, OssArgs& a) {
  const int32_t P = L.P;
  size_t raw_n = 0, tab_n = 0;
  for (int32_t t = 0; t < n_tab; ++t) {
    const Seg& sg = *L.segs[(size_t)seg[t]];
    raw_n += (size_t)fpta_spec::table_len({sg.d.kind, sg.nm_orig, sg.d.nm, nullptr}, P, form[t], per_pulsar[t], n_real);
    tab_n += (size_t)(sg.d.kind == 0 ? P : 1) * sg.d.nm * R_pad;
  }
  if (s.raw.ensure(sizeof(double) * raw_n) != hipSuccess || s.tab.ensure(sizeof(double) * tab_n) != hipSuccess)
    return fail(c, FPTA_ENOMEM, "os_spectra: no device memory for " + std::to_string(sizeof(double) * (raw_n + tab_n)) +
                                    " bytes of tables");
  for (int32_t v = 0; v < st.n_vary; ++v) {  // the layout's amplitudes [P or 1][nm]
    const Seg& sg = *L.segs[(size_t)st.seg[v]];
    a.v[v] = OssVar{sg.amp.as<double>(), sg.d.kind == 0 ? (int64_t)sg.d.nm : 0, 1, 0, sg.nm_orig, 0};
  }
  size_t raw_o = 0, tab_o = 0;
  for (int32_t t = 0; t < n_tab; ++t) {
    Seg& sg = *L.segs[(size_t)seg[t]];
    const size_t len =
        (size_t)fpta_spec::table_len({sg.d.kind, sg.nm_orig, sg.d.nm, nullptr}, P, form[t], per_pulsar[t], n_real);
    double* raw = s.raw.as<double>() + raw_o;
    double* tab = s.tab.as<double>() + tab_o;
    HIPCHK(c, hipMemcpyAsync(raw, tables[t], sizeof(double) * len, hipMemcpyHostToDevice, c->stream),
           "os_spectra tables upload");
    const int rc = spectra_table(c, sg, P, form[t], per_pulsar[t], raw, n_real, R_pad, tab, c->stream);
    if (rc) return rc;
    for (int32_t v = 0; v < st.n_vary; ++v)
      if (st.seg[v] == seg[t])
        a.v[v] = OssVar{tab, sg.d.kind == 0 ? (int64_t)sg.d.nm * R_pad : 0, R_pad, 1, sg.nm_orig, 0};
    raw_o += len;
    tab_o += (size_t)(sg.d.kind == 0 ? P : 1) * sg.d.nm * R_pad;
  }
  return FPTA_OK;
}

}  // namespace capi

using namespace capi;

extern "C" int fpta_batch_set_os_spectra(fpta_ctx* c, int32_t n_comp, const int32_t* n_modes, const double* f,
                                         int32_t f_is_common, const double* idx, const double* freqf,
                                         const double* phi, const uint8_t* mask, int32_t target, const double* phi_hat,
                                         int32_t n_vary, const int32_t* vary, const int32_t* vary_seg, int32_t n_col,
                                         const double* M, const int32_t* ncol_psr, const double* weights, double rcond,
                                         int32_t n_g, const double* G, int32_t n_orf, int32_t* rank_out) {
  if (!c) return fail(nullptr, FPTA_EINVAL, "null ctx");
  const Layout& L = c->batch;
  if (L.P <= 0) return fail(c, FPTA_ESTATE, "set_os_spectra: set_toas first");
  if (n_comp == 0) {
    c->oss_st.clear();
    if (rank_out) std::fill(rank_out, rank_out + L.P, 0);
    return FPTA_OK;
  }
  // everything is validated and the plan built here, before anything is uploaded
  std::string why;
  fpta_oss::Plan plan;
  fpta_oss::Spec sp;
  sp.os = fpta_os::make_spec(fpta_fit::make_spec(n_comp, n_modes, f, f_is_common, idx, freqf), phi, mask, target,
                             phi_hat);
  sp.n_vary = n_vary;
  sp.vary = vary;
  if (n_orf < 0 || n_orf > n_g) return fail(c, FPTA_EINVAL, "set_os_spectra: n_orf outside [0, n_g]");
  if (L.P > 65535) return fail(c, FPTA_EINVAL, "set_os_spectra: more than 65535 pulsars");
  if (n_vary >= 1 && n_vary <= fpta_oss::kMaxVary && !vary_seg)
    return fail(c, FPTA_EINVAL, "set_os_spectra: the varied components' layout signals are missing");
  // the cheap checks first: the plan is a second of long-double work. (The varied set itself is fpta_oss::validate's,
  // which runs again inside make_plan.)
  if (!fpta_oss::validate(L.P, L.h_offs.data(), L.h_toas.data(), L.h_nu.data(), sp, n_col, M, ncol_psr, weights, n_g, G,
                          why))
    return fail(c, FPTA_EINVAL, "set_os_spectra: " + why);
  for (int32_t v = 0; v < n_vary; ++v) {
    const std::string who = "set_os_spectra: varied component " + std::to_string(vary[v]) + ": ";
    if (vary_seg[v] < 0 || vary_seg[v] >= (int32_t)L.segs.size())
      return fail(c, FPTA_EINVAL, who + "unknown layout signal " + std::to_string(vary_seg[v]));
    for (int32_t u = 0; u < v; ++u)
      if (vary_seg[u] == vary_seg[v]) return fail(c, FPTA_EINVAL, who + "its layout signal is named twice");
    const Seg& sg = *L.segs[(size_t)vary_seg[v]];
    if (sg.nm_orig != n_modes[vary[v]])
      return fail(c, FPTA_EINVAL, who + std::to_string(n_modes[vary[v]]) + " modes, its layout signal " +
                                      std::to_string(sg.nm_orig));
  }
  const int made = fpta_oss::make_plan(L.P, L.h_offs.data(), L.h_toas.data(), L.h_nu.data(), sp, n_col, M, ncol_psr,
                                       weights, rcond, n_g, G, plan, why);
  if (made) return fail(c, made == 2 ? FPTA_ENOMEM : FPTA_EINVAL, "set_os_spectra: " + why);
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  c->oss_st.clear();
  HIPCHK(c, hipStreamSynchronize(c->stream), "set_os_spectra sync");
  OssSlot& s = c->oss;
  int rc;
  if ((rc = fit_upload(c, "os_spectra", s.x, plan.q, plan.B0, L.P, L.h_offs.data(), plan.rows))) return rc;
  std::vector<double> sph((size_t)plan.K);
  for (int32_t k = 0; k < plan.K; ++k) sph[(size_t)k] = std::sqrt(phi_hat[k < plan.N ? k : k - plan.N]);
  if ((rc = upload(c, s.a, plan.A.data(), sizeof(double) * plan.A.size(), "os_spectra A"))) return rc;
  if ((rc = upload(c, s.phi, phi_hat, sizeof(double) * (size_t)plan.N, "os_spectra template"))) return rc;
  if ((rc = upload(c, s.sph, sph.data(), sizeof(double) * sph.size(), "os_spectra template roots"))) return rc;
  if ((rc = upload(c, s.g, G, sizeof(double) * (size_t)n_g * (size_t)L.P * (size_t)L.P, "os_spectra pair weights")))
    return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream), "os_spectra upload sync");
  OssState st;
  st.set = true;
  st.q = plan.q;
  st.K = plan.K;
  st.N = plan.N;
  st.J = n_g;
  st.n_orf = n_orf;
  st.n_vary = n_vary;
  std::copy(vary_seg, vary_seg + n_vary, st.seg);
  c->oss_st = st;
  if (rank_out) std::copy(plan.rank.begin(), plan.rank.end(), rank_out);
  return FPTA_OK;
}

extern "C" int fpta_batch_os_spectra(fpta_ctx* c, int32_t n_tab, const int32_t* seg, const int32_t* form,
                                     const int32_t* per_pulsar, const int32_t* n_rows, const double* const* tables,
                                     double* Q, double* Q_mode, double* X, double* norm, double* joint, double* nab_out,
                                     double* zp_out) {
  Block b;
  int rc;
  if ((rc = block_check(c, "os_spectra", false, b))) return rc;
  OssState& st = c->oss_st;
  if (!st.set) return fail(c, FPTA_ESTATE, "os_spectra: no statistic is set (set_os_spectra first)");
  Layout& L = c->batch;
  // the tables: everything is refused here, before anything is uploaded or launched
  std::vector<fpta_spec::Signal> sig;
  for (const Seg* sg : L.segs) sig.push_back({sg->d.kind, sg->nm_orig, sg->d.nm, sg->h_amp.data()});
  std::string why;
  if (!fpta_spec::validate(L.P, (int32_t)sig.size(), sig.data(), b.R, n_tab, seg, form, per_pulsar, n_rows, tables, why))
    return fail(c, FPTA_EINVAL, "os_spectra: " + why);
  for (int32_t t = 0; t < n_tab; ++t)
    if (std::find(st.seg, st.seg + st.n_vary, seg[t]) == st.seg + st.n_vary)
      return fail(c, FPTA_EINVAL, "os_spectra: signal " + std::to_string(seg[t]) + ": a table for a signal outside the varied set");
  if ((rc = block_open(c, false))) return rc;
  OssSlot& s = c->oss;
  const int32_t R = b.R, P = b.n_psr, q = st.q, K = st.K, N = st.N, J = st.J, n_orf = st.n_orf;
  const int32_t R_pad = (R + kOssRpad - 1) / kOssRpad * kOssRpad, items = J + n_orf * n_orf;
  st.R = 0;
  st.rpad = R_pad;
  const size_t zp_real = sizeof(double) * (size_t)K * K * P;
  const int32_t n_chunk = (int32_t)std::max<size_t>(1, std::min<size_t>({(size_t)kOssChunk, kOssZpBytes / zp_real, (size_t)R}));
  const size_t b_x = sizeof(double) * (size_t)P * K * R_pad, b_zp = zp_real * (size_t)n_chunk,
               b_nab = sizeof(double) * (size_t)n_chunk * P * P, b_nrm = sizeof(double) * (size_t)std::max(items, 1) * R,
               b_qm = sizeof(double) * (size_t)std::max(J, 1) * N * R_pad, b_q = sizeof(double) * (size_t)std::max(J, 1) * R_pad;
  if (s.xc.ensure(b_x) != hipSuccess || s.zp.ensure(b_zp) != hipSuccess || s.nab.ensure(b_nab) != hipSuccess ||
      s.nrm.ensure(b_nrm) != hipSuccess || s.qm.ensure(b_qm) != hipSuccess || s.q.ensure(b_q) != hipSuccess)
    return fail(c, FPTA_ENOMEM, "os_spectra: no device memory for " + std::to_string(b_x + b_zp + b_nab + b_nrm + b_qm + b_q) +
                                    " bytes of results (Z' of " + std::to_string(n_chunk) + " realizations: " +
                                    std::to_string(b_zp) + ")");
  const size_t lds = oss_lds_bytes(q, K);
  HIPCHK(c, hipFuncSetAttribute((const void*)k_oss_solve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
         "k_oss_solve LDS size");
  OssArgs a{};
  if ((rc = oss_tables(c, L, st, s, R, R_pad, n_tab, seg, form, per_pulsar, tables, a))) return rc;
  a.A = s.a.as<double>();
  a.sph = s.sph.as<double>();
  a.X = s.xc.as<double>();
  a.Zp = s.zp.as<double>();
  a.n_vary = st.n_vary;
  a.P = P;
  a.q = q;
  a.K = K;
  a.R_pad = R_pad;
  {
    KTimer kt(c, FPTA_K_DENSE);
    int32_t rp = 0;
    if ((rc = fit_launch_unbooked(c, b, q, s.x, rp))) return rc;
    if (rp != R_pad) return fail(c, FPTA_EINVAL, "os_spectra: k_fit_apply's realization padding changed");
    a.z = s.x.coef.as<double>();
    HIPCHK(c, hipMemsetAsync(s.xc.p, 0, b_x, c->stream), "os_spectra coefficients clear");
    const int32_t n_tile = (P + 15) / 16;
    for (int32_t r0 = 0; r0 < R; r0 += n_chunk) {
      a.r0 = r0;
      a.n_r = std::min(n_chunk, R - r0);
      const dim3 grid((unsigned)((a.n_r + kOssRW - 1) / kOssRW), (unsigned)P, (unsigned)((K + kOssCols) / kOssCols));
      k_oss_solve<<<grid, dim3(256), lds, c->stream>>>(a);
      HIPCHK(c, hipGetLastError(), "k_oss_solve launch");
      HIPCHK(c, hipMemsetAsync(s.nab.p, 0, sizeof(double) * (size_t)a.n_r * P * P, c->stream), "os_spectra N_ab clear");
      k_oss_gram<<<dim3((unsigned)(n_tile * (n_tile + 1) / 2), (unsigned)a.n_r), dim3(64), 0, c->stream>>>(
          s.zp.as<double>(), P, K * K, n_tile, s.nab.as<double>());
      HIPCHK(c, hipGetLastError(), "k_oss_gram launch");
      if (items > 0) {
        k_oss_contract<<<dim3((unsigned)((items + 63) / 64), (unsigned)a.n_r), dim3(64), 0, c->stream>>>(
            s.nab.as<double>(), s.g.as<double>(), J, n_orf, P, r0, R, s.nrm.as<double>());
        HIPCHK(c, hipGetLastError(), "k_oss_contract launch");
      }
      // a chunk's Z' and N_ab leave before the next chunk overwrites them
      if (zp_out)
        HIPCHK(c, hipMemcpyAsync(zp_out + (size_t)r0 * P * K * K, s.zp.p, zp_real * (size_t)a.n_r, hipMemcpyDeviceToHost,
                                 c->stream), "os_spectra Z' download");
      if (nab_out)
        HIPCHK(c, hipMemcpyAsync(nab_out + (size_t)r0 * P * P, s.nab.p, sizeof(double) * (size_t)a.n_r * P * P,
                                 hipMemcpyDeviceToHost, c->stream), "os_spectra N_ab download");
      if (zp_out || nab_out) HIPCHK(c, hipStreamSynchronize(c->stream), "os_spectra chunk sync");
    }
    if (J > 0 && (rc = os_pairs_launch(c, s.xc.as<double>(), s.phi.as<double>(), s.g.as<double>(), s.qm.as<double>(),
                                       s.q.as<double>(), P, N, R_pad, J)))
      return rc;
  }
  st.R = R;
  if (norm && J > 0)
    HIPCHK(c, hipMemcpyAsync(norm, s.nrm.p, sizeof(double) * (size_t)J * R, hipMemcpyDeviceToHost, c->stream),
           "os_spectra norm download");
  if (joint && n_orf > 0)
    HIPCHK(c, hipMemcpyAsync(joint, s.nrm.as<double>() + (size_t)J * R, sizeof(double) * (size_t)n_orf * n_orf * R,
                             hipMemcpyDeviceToHost, c->stream), "os_spectra joint download");
  if (Q && J > 0 && (rc = fit_download(c, s.q, J, R, R_pad, Q))) return rc;
  if (Q_mode && J > 0 && (rc = fit_download(c, s.qm, (int64_t)J * N, R, R_pad, Q_mode))) return rc;
  if (X && (rc = fit_download(c, s.xc, (int64_t)P * K, R, R_pad, X))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream), "os_spectra sync");  // the tables are the caller's memory
  return FPTA_OK;
}
