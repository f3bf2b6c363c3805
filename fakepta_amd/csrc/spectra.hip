// Per-realization spectra of a batch block: fpta_batch_synth_spectra (include/fakepta_amd.h).
//
//   k_spectra_amp    a call's table of one signal (amplitudes or power-law parameters, realization-major as the host
//                    gives them) -> the device amplitude table [P or 1][nm][R_pad], realization fastest: the
//                    coefficient buffer's order
//   k_spectra_scale  coef[p][col0 + j][r] = tab[p or 0][j / 2][r] * coef[p][col0 + j][r] over a signal's columns
//
// A tabled signal is drawn and mixed by the layout's own kernels (k_gen, k_mix, k_mix_tiled, k_mix_mfma, k_gen_mix:
// their code is untouched) with unit amplitudes: they store 1 * z = z, respectively 1 * sum_q L[p][q] z[q], exactly.
// k_spectra_scale then multiplies by realization r's amplitude, so a coefficient is the same rounded product a * z or
// a * sum L z that the fixed-spectrum route makes with a as the layout's amplitude, bit for bit. Validation is
// spectra_host.h's (no HIP there); routing is run_coefficients' (capi.hip).
#include "capi_host.h"
#include "spectra_host.h"

namespace __attribute__((visibility("hidden"))) capi {

// grid (ceil(R_pad / 256), nm, rows): thread = realization r of (row p, mode k). raw: form 0 [R][rows_tab][N], form 1
// [R][rows_tab][2]; rows_tab = rows, or 1 for a row shared by the pulsars. lay [rows][nm] the layout's amplitudes (an
// exact 0 stays 0), fdf [rows][nm][2] {f, delta f} (form 1). Writes every entry of the table: 0 for the padding mode
// and for r >= R.
__global__ __launch_bounds__(256) void k_spectra_amp(int32_t form, const double* __restrict__ raw, int32_t rows_tab,
                                                     const double* __restrict__ lay, const double* __restrict__ fdf,
                                                     int32_t N, int32_t nm, int32_t R, int32_t R_pad,
                                                     double* __restrict__ tab) {
  const int32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R_pad) return;
  const int32_t k = blockIdx.y, p = blockIdx.z;
  const int64_t e = (int64_t)p * nm + k;
  double a = 0.0;
  if (r < R && k < N && lay[e] != 0.0) {
    const int64_t row = (int64_t)r * rows_tab + (rows_tab > 1 ? p : 0);
    if (form == 0) {
      a = raw[row * N + k];
    } else {
      // fakepta.spectrum.powerlaw in its operation order, times delta f
      const double log10_A = raw[row * 2], gamma = raw[row * 2 + 1];
      const double a10 = pow(10.0, log10_A);
      const double psd = a10 * a10 / (12.0 * (M_PI * M_PI)) * pow(fpta_spec::kFyr, gamma - 3.0) * pow(fdf[2 * e], -gamma);
      a = sqrt(psd * fdf[2 * e + 1]);
    }
  }
  tab[e * R_pad + r] = a;
}

// grid (ceil(R_pad / 512), 2 nm, P): thread = realizations (r, r + 1) of one coefficient column (R_pad is even)
__global__ __launch_bounds__(256) void k_spectra_scale(const double* __restrict__ tab, int64_t tab_pstride, int32_t nm,
                                                       int32_t R_pad, int32_t K, int32_t col0,
                                                       double* __restrict__ coef) {
  const int32_t r = (blockIdx.x * 256 + threadIdx.x) * 2;
  if (r >= R_pad) return;
  const int32_t j = blockIdx.y, p = blockIdx.z;
  const double2 a = *(const double2*)(tab + (int64_t)p * tab_pstride + (int64_t)(j >> 1) * R_pad + r);
  double2* cp = (double2*)(coef + ((int64_t)p * K + col0 + j) * R_pad + r);
  const double2 z = *cp;
  *cp = make_double2(a.x * z.x, a.y * z.y);
}

__global__ __launch_bounds__(256) void k_spectra_ones(double* __restrict__ v, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) v[i] = 1.0;
}

int spectra_scale(fpta_ctx* c, const Layout& L, size_t i, int32_t R_pad, double* coef, hipStream_t st) {
  const SegDesc& d = L.segs[i]->d;
  const double* tab = c->spec.tab[i];
  KTimer kt(c, FPTA_K_GEN, st);
  k_spectra_scale<<<dim3((unsigned)((R_pad / 2 + 255) / 256), (unsigned)(2 * d.nm), (unsigned)L.P), dim3(256), 0, st>>>(
      tab, d.kind == 0 ? (int64_t)d.nm * R_pad : 0, d.nm, R_pad, L.K, d.col0, coef);
  HIPCHK(c, hipGetLastError(), "k_spectra_scale launch");
  return FPTA_OK;
}

int spectra_table(fpta_ctx* c, Seg& s, int32_t P, int32_t form, int32_t per_pulsar, const double* raw, int32_t n_real,
                  int32_t R_pad, double* tab, hipStream_t st) {
  const int32_t rows = s.d.kind == 0 ? P : 1;
  if (form == 1 && !s.fdf.p) {
    HIPCHK(c, s.fdf.ensure(sizeof(double) * s.h_fdf.size()), "spectra frequencies alloc");
    HIPCHK(c, hipMemcpyAsync(s.fdf.p, s.h_fdf.data(), sizeof(double) * s.h_fdf.size(), hipMemcpyHostToDevice, st),
           "spectra frequencies upload");
  }
  k_spectra_amp<<<dim3((unsigned)((R_pad + 255) / 256), (unsigned)s.d.nm, (unsigned)rows), dim3(256), 0, st>>>(
      form, raw, per_pulsar ? P : 1, s.d.amp, s.fdf.as<double>(), s.nm_orig, s.d.nm, n_real, R_pad, tab);
  HIPCHK(c, hipGetLastError(), "k_spectra_amp launch");
  return FPTA_OK;
}

// The tables of one call, validated already, into c->spec: uploads, k_spectra_amp per table, and a host wait for them
// (the tables are the caller's memory, and the draws of the block may be queued on any stream afterwards).
static int spectra_build(fpta_ctx* c, Layout& L, int32_t n_real, int32_t R_pad, int32_t n_tab, const int32_t* seg,
                         const int32_t* form, const int32_t* per_pulsar, const double* const* tables) {
  const int32_t P = L.P;
  if (!c->spec_st) HIPCHK(c, hipStreamCreateWithFlags(&c->spec_st, hipStreamNonBlocking), "spectra stream create");
  hipStream_t st = c->spec_st;
  size_t raw_n = 0, tab_n = 0, ones_n = 0;
  for (int32_t t = 0; t < n_tab; ++t) {
    const Seg& s = *L.segs[(size_t)seg[t]];
    const size_t rows = s.d.kind == 0 ? (size_t)P : 1;
    if (s.d.nm > 32767 || rows > 65535)  // the kernels' grid extents
      return fail(c, FPTA_EINVAL, "batch_synth_spectra: signal too large");
    raw_n += (size_t)fpta_spec::table_len({s.d.kind, s.nm_orig, s.d.nm, nullptr}, P, form[t], per_pulsar[t], n_real);
    tab_n += rows * s.d.nm * R_pad;
    ones_n = std::max(ones_n, rows * s.d.nm);
  }
  // the previous tabled block's scalings may still read the tables (and its draws the unit amplitudes)
  if (c->spec_done_set) {
    if (c->spec_raw.cap < sizeof(double) * raw_n || c->spec_tab.cap < sizeof(double) * tab_n || c->spec_ones_n < ones_n)
      HIPCHK(c, hipEventSynchronize(c->ev_spec_done), "spectra regrow sync");
    else
      HIPCHK(c, hipStreamWaitEvent(st, c->ev_spec_done, 0), "spectra wait");
  }
  HIPCHK(c, c->spec_raw.ensure(sizeof(double) * raw_n), "spectra tables alloc");
  HIPCHK(c, c->spec_tab.ensure(sizeof(double) * tab_n), "spectra amplitudes alloc");
  if (c->spec_ones_n < ones_n) {
    HIPCHK(c, c->spec_ones.ensure(sizeof(double) * ones_n), "spectra unit amplitudes alloc");
    k_spectra_ones<<<dim3((unsigned)((ones_n + 255) / 256)), dim3(256), 0, st>>>(c->spec_ones.as<double>(), (int64_t)ones_n);
    HIPCHK(c, hipGetLastError(), "k_spectra_ones launch");
    c->spec_ones_n = ones_n;
  }
  c->spec.tab.assign(L.segs.size(), nullptr);
  c->spec.per_pulsar = false;
  size_t raw_o = 0, tab_o = 0;
  for (int32_t t = 0; t < n_tab; ++t) {
    Seg& s = *L.segs[(size_t)seg[t]];
    const int32_t rows = s.d.kind == 0 ? P : 1;
    const size_t len =
        (size_t)fpta_spec::table_len({s.d.kind, s.nm_orig, s.d.nm, nullptr}, P, form[t], per_pulsar[t], n_real);
    double* raw = c->spec_raw.as<double>() + raw_o;
    double* tab = c->spec_tab.as<double>() + tab_o;
    HIPCHK(c, hipMemcpyAsync(raw, tables[t], sizeof(double) * len, hipMemcpyHostToDevice, st), "spectra tables upload");
    const int rc = spectra_table(c, s, P, form[t], per_pulsar[t], raw, n_real, R_pad, tab, st);
    if (rc) return rc;
    c->spec.tab[(size_t)seg[t]] = tab;
    c->spec.per_pulsar = c->spec.per_pulsar || s.d.kind == 0;
    raw_o += len;
    tab_o += (size_t)rows * s.d.nm * R_pad;
  }
  HIPCHK(c, hipStreamSynchronize(st), "spectra tables sync");
  c->spec.on = true;
  return FPTA_OK;
}

}  // namespace capi

using namespace capi;

extern "C" int fpta_batch_synth_spectra(fpta_ctx* c, uint64_t seed, int64_t real0, int32_t n_real, int32_t n_tab,
                                        const int32_t* seg, const int32_t* form, const int32_t* per_pulsar,
                                        const int32_t* n_rows, const double* const* tables, double* out,
                                        double* coeffs_out) {
  if (!c) return fail(nullptr, FPTA_EINVAL, "null ctx");
  Layout& L = c->batch;
  if (L.P <= 0) return fail(c, FPTA_ESTATE, "batch_synth_spectra: set_toas first");
  if (n_real <= 0) return fail(c, FPTA_EINVAL, "batch_synth_spectra: n_real must be > 0");
  // everything is validated here, before anything is uploaded or launched
  std::vector<fpta_spec::Signal> sig;
  for (const Seg* s : L.segs) sig.push_back({s->d.kind, s->nm_orig, s->d.nm, s->h_amp.data()});
  std::string why;
  if (!fpta_spec::validate(L.P, (int32_t)sig.size(), sig.data(), n_real, n_tab, seg, form, per_pulsar, n_rows, tables,
                           why))
    return fail(c, FPTA_EINVAL, "batch_synth_spectra: " + why);
  if (n_tab == 0) return batch_common(c, seed, real0, n_real, nullptr, 0, out, coeffs_out, true);
  if (real0 < 0 || real0 + n_real > ((int64_t)1 << 32))
    return fail(c, FPTA_EINVAL, "batch_synth: realization index exceeds the 32-bit Philox counter word");
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  const int32_t R_pad = (n_real + kRealPad - 1) / kRealPad * kRealPad;
  int rc = spectra_build(c, L, n_real, R_pad, n_tab, seg, form, per_pulsar, tables);
  if (!rc) rc = batch_common(c, seed, real0, n_real, nullptr, 0, out, coeffs_out, true);
  c->spec.on = false;
  c->spec.per_pulsar = false;
  return rc;
}
