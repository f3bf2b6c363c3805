/*
 * fakepta_amd.h — C-ABI of libfakepta_amd.so, the MI355X (gfx950) Fourier-basis
 * Gaussian-process residual synthesis for pulsar-timing arrays.
 *
 * The reference (mfalxa/fakepta) has no FFI: its hot path is numpy loops inside
 * Python methods. Each entry point below names the reference code it replaces;
 * the Python host layer (fakepta_amd/fake_pta.py, correlated_noises.py, batch.py)
 * binds them through ctypes (fakepta_amd/_capi.py) behind the reference's own
 * method signatures. INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - Plain pointers + sizes, no torch types. Host buffers are owned by the caller;
 *     the library copies inputs to device buffers owned by the context.
 *   - Every call returns 0 on success or a negative FPTA_E* code; the message is
 *     available from fpta_last_error(ctx) (or fpta_last_error(NULL) for calls
 *     that failed before a context existed). The library never aborts or exits.
 *   - A context owns one device and one HIP stream and is single-threaded; use
 *     one context per GPU (one process per GPU for multi-GPU).
 *   - All arithmetic is IEEE fp64.
 *   - Angular frequencies: the library computes the phase as (2*pi*f_k) * t with
 *     the same operation order as fakepta/fake_pta.py:386, so drop-in results
 *     match the numpy reference to rounding.
 */
#ifndef FAKEPTA_AMD_H
#define FAKEPTA_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FPTA_OK 0
#define FPTA_EINVAL (-22)   /* bad argument / shape */
#define FPTA_ENOMEM (-12)   /* device allocation failed */
#define FPTA_EDEVICE (-19)  /* no device / HIP runtime error */
#define FPTA_ESTATE (-77)   /* call out of order (e.g. synth before set_toas) */

typedef struct fpta_ctx fpta_ctx;

/* ------------------------------------------------------------------ lifetime */
/* 10000 * ABI major + 100 * behaviour revision (FPTA_VERSION): the major changes only if an entry point's signature
 * or buffer size changes; the revision when a call's accepted values or reported codes change. 10100 (round 6):
 * FPTA_OPT_INTERP_WS 0/2/3, DFT_GEN 0, GEN_MIX 0/1/3, ASYNC_SUMS 1 and SIDE_SPLIT 0/1 are refused (FPTA_EINVAL) by
 * the product library (variant builds accept them); FPTA_OPT_INTERP_FUSED takes 0 .. 3; fpta_batch_grid_info_n slot
 * 15 names each k_grid_fused instance (kinds 11 .. 19) instead of kinds 8 / 9. 10200 (round 6): option
 * FPTA_OPT_FUSED_NEXT_MIX; fpta_batch_grid_info_n slots 17 and 18 (FPTA_GRID_INFO_LEN 19). 10300: option key 24 is
 * refused (FPTA_EINVAL); fpta_batch_grid_info_n slot 15 kinds 20 / 21 are gone. */
#define FPTA_VERSION 10300
int fpta_version(void);
int fpta_create(int device, fpta_ctx** out);
int fpta_destroy(fpta_ctx* ctx);
const char* fpta_last_error(const fpta_ctx* ctx);
int fpta_device_count(int* n);

/* ------------------------------------------------------------------ drop-in, one realization
 * These replace the per-call numpy loops of the reference; the host keeps the
 * reference's RNG draws (np.random legacy stream) and bookkeeping, so a seeded
 * script produces the same residuals.
 */

/* Replaces fakepta/fake_pta.py:385-387 (Pulsar.add_time_correlated_noise hot loop)
 * and fakepta/fake_pta.py:538-554 (Pulsar.reconstruct_signal GP branches).
 *   residuals[t] += sign * sum_s m_s(t) (freqf_s/nu_t)^idx_s *
 *                   sum_k ( ccos[k] cos(2 pi f[k] t) + csin[k] sin(2 pi f[k] t) )
 * Segments s are concatenated: seg_nmodes[n_seg]; f/ccos/csin hold sum(seg_nmodes)
 * values. ccos = sqrt(df)*coeffs[0::2] when injecting, df*fourier[0] when reconstructing.
 * mask: NULL, or uint8 [n_seg][n_toa] (1 = TOA belongs to the backend of that segment).
 * residuals: host fp64 [n_toa], read and written. */
int fpta_gp_accumulate(fpta_ctx* ctx, int64_t n_toa, const double* toas, const double* nu,
                       int32_t n_seg, const int32_t* seg_nmodes, const double* f,
                       const double* ccos, const double* csin, const double* seg_idx,
                       const double* seg_freqf, const uint8_t* mask, double sign,
                       double* residuals);

/* Array form of fpta_gp_accumulate (one launch for a whole array): replaces the per-pulsar
 * reconstruct_signal calls of correlated_noises.py:133-134 (replace-on-reinject) and of
 * remove_signal (fake_pta.py:557-567) over many pulsars. n_psr pulsars (CSR offs[n_psr+1]);
 * segment s has seg_nmodes[s] modes and contributes f/ccos/csin blocks of [n_psr][seg_nmodes[s]]
 * (concatenated over segments). mask: NULL or uint8 [n_seg][n_toa_total]. residuals [n_toa_total]. */
int fpta_gp_accumulate_array(fpta_ctx* ctx, int32_t n_psr, const int64_t* offs, const double* toas,
                             const double* nu, int32_t n_seg, const int32_t* seg_nmodes, const double* f,
                             const double* ccos, const double* csin, const double* seg_idx,
                             const double* seg_freqf, const uint8_t* mask, double sign, double* residuals);

/* Replaces fakepta/correlated_noises.py:146-160 (add_common_correlated_noise hot loop).
 * n_psr pulsars, CSR offsets offs[n_psr+1] into toas/nu (seconds / MHz).
 * For mode k: x_sin = L z[k][0], x_cos = L z[k][1] (z in the reference's draw order,
 * [n_modes][2][n_psr], sin vector drawn first), L = [n_psr][n_psr] row-major factor with
 * L L^T = ORF (for exact reference parity pass the transpose of numpy's SVD factor).
 *   residuals[t in p] += (freqf/nu_t)^idx * sum_k amp[k] ( x_cos[p] cos(2 pi f_k t)
 *                                                        + x_sin[p] sin(2 pi f_k t) )
 * with amp[k] = sqrt(df_k) * sqrt(psd_k) (the reference's df**0.5 * coeffs[2k]; cos and sin
 * share it because coeffs = sqrt(repeat(psd, 2)), correlated_noises.py:146-147).
 * x_out (optional, may be NULL): [n_modes][2][n_psr] mixed draws (cos, sin) for the
 * host's signal_model bookkeeping (correlated_noises.py:157-158). */
int fpta_common_accumulate(fpta_ctx* ctx, int32_t n_psr, const int64_t* offs, const double* toas,
                           const double* nu, int32_t n_modes, const double* f, const double* amp,
                           double idx, double freqf, const double* L,
                           const double* z, double* residuals, double* x_out);

/* Replaces the enterprise_extensions cw_delay call of fakepta/fake_pta.py:436-441 (Pulsar.add_cgw) and of the 'cgw'
 * branch of reconstruct_signal, for any number of sources and a whole array in one call (added without a change of
 * FPTA_VERSION: no existing call changes): the continuous wave of circular binaries with evolving frequency
 * (cw_delay with evolve=True, tref=0, p_phase=None), source s in src[s][FPTA_CW_NPAR]. With mc = 10^log10_mc Tsun,
 * w0 = pi 10^log10_fgw, K = 256/5 mc^(5/3) w0^(8/3), omega(x) = w0 (1 - K x)^(-3/8),
 *   phase(x) = phase0/2 + (w0^(-5/3) - omega(x)^(-5/3)) / (32 mc^(5/3)),   alpha(x) = 10^log10_h / (2 w0^(2/3) omega(x)^(1/3)),
 *   r(x) = alpha(x) [ sin 2 phase(x) (1 + cos_inc^2) (F+ cos 2 psi - Fx sin 2 psi)
 *                   + cos 2 phase(x) 2 cos_inc (F+ sin 2 psi + Fx cos 2 psi) ],
 * F+, Fx, cos mu the antenna pattern of pulsar p (unit vector pos[p]) for the source direction:
 *   residuals[t in p] += sign * sum_s ( psrterm_s ? r(t - pdist_s[p] (1 - cos mu)) - r(t) : -r(t) )
 * summed over s in ascending order (in n contiguous pieces when the sources are split, FPTA_OPT_CW_SPLIT). pdist_s:
 * the pulsar distances in light-seconds. Validated on the host before anything is launched (FPTA_EINVAL, the message
 * names the source index, residuals untouched): a non-finite parameter, |cos_gwtheta| > 1 or |cos_inc| > 1, or
 * K max(toas) >= 1 (the binary coalesces inside the data). A source exactly behind a pulsar gives inf / NaN as the
 * reference's antenna pattern does. n_src == 0 is a successful no-op. */
#define FPTA_CW_NPAR 9   /* cos_gwtheta, gwphi, cos_inc, log10_mc, log10_fgw, log10_h, phase0, psi, psrterm (0/1) */
int fpta_cw_accumulate(fpta_ctx* ctx, int32_t n_psr, const int64_t* offs, const double* toas,
                       const double* pos /* [n_psr][3] */, const double* pdist_s /* [n_psr] L in seconds */,
                       int32_t n_src, const double* src /* [n_src][FPTA_CW_NPAR] */,
                       double sign, double* residuals /* host fp64 [n_toa_total], read and written */);
/* The same waves injected into the context's last batch block, in place on the device (added without a change of
 * FPTA_VERSION: no existing call changes): for every realization r of the block and every TOA t of the batch layout,
 *   block[r][t in p] += sign * sum_s delay(t; source s of table r, pulsar p),
 * the delay as above, summed over s in ascending order in one register. n_tab == the block's realization count: table
 * r is the rows src_offs[r] .. src_offs[r + 1] - 1 of src (CSR; a table may be empty), and realization r equals, bit for
 * bit, its samples plus what fpta_cw_accumulate adds to zeros for table r in one piece (FPTA_OPT_CW_SPLIT 1). n_tab == 1:
 * one table for every realization; with pdist_stride == 0 its delay vector is made once with fpta_cw_accumulate's own
 * split rule (it equals that call on zeros bit for bit) and added to every realization. pos [P][3] and pdist_s are the
 * batch layout's pulsars; pdist_stride 0: pdist_s [P] for every realization, P: pdist_s [n_real][P], one distance draw
 * per (realization, pulsar). FPTA_ESTATE without a synthesized block. Validated on the host before anything is uploaded
 * or launched (FPTA_EINVAL, the block untouched): n_tab not 1 or the block's realization count, src_offs not starting
 * at 0 or not monotone, pdist_stride not 0 or P, a non-finite sign, position or distance, and every source as
 * fpta_cw_accumulate validates it against the layout's latest TOA ("realization r, source s: reason"). No sources at
 * all is a successful no-op. It runs on the context's stream and returns when the block is updated;
 * fpta_batch_download, _checksums, _correlations, _project and _fit afterwards see the block with the waves; the next
 * block is not affected. Blocks streamed by fpta_batch_synth_checksums / fpta_multi_synth get no waves. Kernel time is
 * booked under FPTA_K_CW, one entry per call. */
int fpta_batch_cw_accumulate(fpta_ctx* ctx, const double* pos /* [P][3] */, const double* pdist_s,
                             int64_t pdist_stride /* 0: [P] for all, P: [n_real][P] */,
                             int32_t n_tab /* 1: one table for every realization; else == the block's n_real */,
                             const int64_t* src_offs /* [n_tab + 1] */,
                             const double* src /* [src_offs[n_tab]][FPTA_CW_NPAR] */, double sign);

/* Replaces fakepta/ephemeris.py (Ephemeris.solve_kepler_equation, compute_orbit, get_planet_ssb, get_sunssb,
 * roemer_delay: one scipy newton call per (TOA, body) and a Python rotation per sample) for any number of bodies and a
 * whole array in one call (added without a change of FPTA_VERSION: no existing call changes). This text is the
 * specification.
 * A body is FPTA_EPHEM_NBODY doubles: mass, T [days], then (value, rate per Julian century) of inc, Om, omega [deg],
 * a [AU], e, l0 [deg]. a = None of the reference is the pair (0, 0): it stands for the Kepler-law value
 * (GMsun (86400 T)^2 / (4 pi^2))^(1/3) / AU with rate 0 (GMsun = 1.327124400e20), resolved on the host.
 * For a TOA in MJD seconds, t = (toa / 86400 - 51544.5) / 36525 (the reference adds 2400000.5 days first, which costs
 * ~1e-14 century; 51544.5 is exact). Every element is value + rate t. With a_s = a AU / c [s],
 *   M = mod((l0 - omega) pi / 180, 2 pi),   E - e sin E = M,
 *   x = a_s cos(E - e),   y = a_s sqrt(1 - e^2) sin E     (the reference's x, not a_s (cos E - e): kept)
 *   orbit = R_x(eps) R_z(Om) R_x(inc) R_z(omega - Om) (x, y, 0)^T,   eps = 23.43928 deg, angles in radians,
 * i.e. with O = Om, w = omega - Om, i = inc:
 *   X = (cos O cos w - sin O cos i sin w) x + (-cos O sin w - sin O cos i cos w) y
 *   Y = (sin O cos w + cos O cos i sin w) x + (-sin O sin w + cos O cos i cos w) y
 *   Z = sin i sin w x + sin i cos w y,       orbit = (X, cos eps Y - sin eps Z, sin eps Y + cos eps Z)  [light-seconds].
 * Kepler's equation is solved by Newton's method for 0 <= e <= FPTA_EPHEM_E_MAX.
 * Validated on the host before anything is uploaded or launched (FPTA_EINVAL, the message names the TOA, body or row
 * index, the outputs untouched): a non-finite value; e(t) outside [0, FPTA_EPHEM_E_MAX] or a(t) <= 0 at either end of
 * the TOA span (the elements are linear, so the ends suffice); a = None without T > 0; 1 / mass_ss <= 0. */
#define FPTA_EPHEM_NBODY 14
#define FPTA_EPHEM_E_MAX 0.95
#define FPTA_EPHEM_MSUN (1.327124400e20 / 6.6743e-11) /* kg: GMsun / G */
/* E_out[i] with E - e[i] sin E = M[i]; whole turns of M are taken off before the solve and put back after it. */
int fpta_ephem_kepler(fpta_ctx* ctx, int64_t n, const double* M, const double* e, double* E_out);
/* planetssb_out (or NULL): [n_toa][n_body][6], columns 0 .. 2 the orbit of each body in table order, columns 3 .. 5
 * (the velocities, which the reference leaves uninitialised) 0. sunssb_out (or NULL): [n_toa][3] =
 * -sum_b mass_b / FPTA_EPHEM_MSUN orbit_b, summed in table order. At least one output. */
int fpta_ephem_orbits(fpta_ctx* ctx, int64_t n_toa, const double* toas, int32_t n_body,
                      const double* bodies /* [n_body][FPTA_EPHEM_NBODY] */, double* planetssb_out,
                      double* sunssb_out);
/* Roemer delay of ephemeris errors (Ephemeris.roemer_delay, correlated_noises.add_roemer_delay). Row r is a body, then
 * d_mass, d_Om, d_omega, d_inc, d_a, d_e, d_l0, then 1 / mass_ss (mass_ss in the unit of mass and d_mass):
 *   delay_r(t in p) = [ (mass + d_mass) orbit'(t) - mass orbit(t) ] / mass_ss . pos[p]
 * orbit from the row's elements as given, orbit' from the elements with the six deviations added to their values (not
 * to the rates; d_a is added to the resolved a). The reference adds the deviations to its stored table and evaluates
 * both orbits from it, so it returns 0 for element deviations and drifts from call to call; this is the expression it
 * states. When all six element deviations are exactly 0 the orbit is evaluated once.
 *   separate == 0: out[t] += sign * sum_r delay_r(t)   (out: [n_toa_total], read and written; rows summed in
 *                  ascending order in one register per TOA)
 *   separate != 0: out[r][t] = sign * delay_r(t)       (out: [n_row][n_toa_total], written)
 * A pulsar may have no TOAs. n_row == 0 is a successful no-op. */
#define FPTA_ROEMER_NPAR 22
int fpta_roemer_accumulate(fpta_ctx* ctx, int32_t n_psr, const int64_t* offs, const double* toas,
                           const double* pos /* [n_psr][3] */, int32_t n_row,
                           const double* rows /* [n_row][FPTA_ROEMER_NPAR] */, double sign, int32_t separate,
                           double* out);
/* The same delays injected into the context's last batch block, in place on the device (added without a change of
 * FPTA_VERSION: no existing call changes): for every realization r of the block and every TOA t of the batch layout,
 *   block[r][t in p] += sign * sum_k delay_k(t in p),   k over the rows of table r,
 * delay_k as above, summed over k in ascending order in one register, and sign * sum rounded as a product before it is
 * added. n_tab == the block's realization count: table r is the rows row_offs[r] .. row_offs[r + 1] - 1 of rows (CSR; a
 * table may be empty, and its realization is not touched), and realization r equals, bit for bit, its samples plus what
 * fpta_roemer_accumulate (separate == 0) adds to zeros for table r, whatever FPTA_OPT_ROEMER_CHUNK. n_tab == 1: one
 * table for every realization; its delay vector is made once with fpta_roemer_accumulate's own kernel on zeros and
 * added to every realization. pos [P][3]: the batch layout's pulsars. FPTA_ESTATE without a synthesized block.
 * Validated on the host before anything is uploaded or launched (FPTA_EINVAL, the block untouched): n_tab not 1 or the
 * block's realization count, row_offs not starting at 0 or not monotone, a non-finite sign or position, and every row
 * as fpta_roemer_accumulate validates it over the layout's TOA span ("realization r, row k: reason"). No rows at all is
 * a successful no-op. It runs on the context's stream and returns when the block is updated; fpta_batch_download,
 * _checksums, _correlations, _project, _fit, _os and _lnl afterwards see the block with the delays; the next block is
 * not affected. Blocks streamed by fpta_batch_synth_checksums / fpta_multi_synth get no delays. Kernel time is booked
 * under FPTA_K_EPHEM, one entry per call. */
int fpta_batch_roemer_accumulate(fpta_ctx* ctx, const double* pos /* [P][3] */,
                                 int32_t n_tab /* 1: one table for every realization; else == the block's n_real */,
                                 const int64_t* row_offs /* [n_tab + 1] */,
                                 const double* rows /* [row_offs[n_tab]][FPTA_ROEMER_NPAR] */, double sign);

/* Replaces fakepta/correlated_noises.py:73-89 (anisotropic: healpy's pix2ang and one antenna-pattern call per pulsar
 * pair) for any number of maps in one call (added without a change of FPTA_VERSION: no existing call changes). This
 * text is the specification.
 * Pixel centres, HEALPix RING ordering, any nside >= 1 (not only powers of two). With npix = 12 nside^2,
 * ncap = 2 nside (nside - 1) and pixel p in 0 .. npix - 1 (isqrt the integer square root, / on integers truncating):
 *   north cap, p < ncap:             i = (1 + isqrt(1 + 2 p)) >> 1,  j = p + 1 - 2 i (i - 1),
 *                                    z = 1 - 4 i^2 / npix,           phi = (j - 1/2) pi / (2 i)
 *   belt, ncap <= p < npix - ncap:   q = p - ncap,  t = q / (4 nside),  i = t + nside,  j = q - 4 nside t + 1,
 *                                    s = (1 + ((i + nside) & 1)) / 2,
 *                                    z = (2 nside - i) 2 / (3 nside), phi = (j - s) pi / (2 nside)
 *   south cap, otherwise:            q = npix - p,  i = (1 + isqrt(2 q - 1)) >> 1,  j = 4 i + 1 - (q - 2 i (i - 1)),
 *                                    z = -1 + 4 i^2 / npix,          phi = (j - 1/2) pi / (2 i)
 * cos theta = z, sin theta = sqrt((1 - z) (1 + z)); both are rounded once from long double per ring, and phi is a
 * rational multiple of pi ((2 (j - 1) + odd) / n_ring with n_ring the ring's pixel count), so the kernels take its
 * cosine and sine with an exact argument reduction.
 * Antenna pattern of a pulsar with unit vector p for a pixel, the reference's expression (:50-60) kept literally:
 *   m = (sin phi, -cos phi, 0),  n = (-z cos phi, -z sin phi, sin theta),
 *   Omega = (-sin theta cos phi, -sin theta sin phi, -z),  D = 1 + Omega . p,
 *   F+ = 1/2 ((m . p)^2 - (n . p)^2) / D,   Fx = (m . p) (n . p) / D.
 * ORF (:73-89), a weighted Gram matrix of the rows [F+ | Fx]:
 *   ORF[m][a][b] = 1.5 k_ab / npix sum_pix (F+^a F+^b + Fx^a Fx^b) h_m[pix],   k_aa = 2, k_ab = 1 (a != b).
 * The pixel range is cut into contiguous K-splits (FPTA_OPT_ORF_SPLIT); pixels are summed in ascending order within a
 * split and the splits in ascending order, without atomics: a repeated call is bit-identical, the matrix is exactly
 * symmetric, and a map's result does not depend on which other maps share its call.
 * A pulsar exactly on a pixel centre has D = 0 and 0 / 0 terms: its row and column are NaN, as the reference's antenna
 * pattern gives; nothing else is affected. The expression is ill-conditioned near a pixel centre:
 * against 50-digit arithmetic at nside 4 the literal fp64 evaluation is off by 4e-14 / 1.3e-10 / 1.3e-6 of the peak
 * for a pulsar 1e-2 / 1e-4 / 1e-6 rad from a centre. A cancellation-free form in p - pixel direction is no better: the
 * rounding of the pixel direction itself sets the error.
 * Validated on the host before anything is uploaded or launched (FPTA_EINVAL, the message names the index, orf_out
 * untouched): nside < 1 or > 1024; a non-finite map value (map and pixel named); a non-finite position or
 * | |p| - 1 | > 1e-8 (pulsar named); more than 8192 pulsars. n_psr == 0 and n_map == 0 are successful no-ops. */
/* theta = atan2(sin theta, z) and phi of n pixels. Host only, no context: works without a GPU. FPTA_EINVAL (message
 * from fpta_last_error(NULL)) for nside outside [1, 1024] or a pixel outside [0, npix). */
int fpta_healpix_pix2ang_ring(int32_t nside, int64_t n, const int64_t* ipix, double* theta_out, double* phi_out);
int fpta_orf_anisotropic(fpta_ctx* ctx, int32_t n_psr, const double* pos /* [n_psr][3] */, int32_t nside,
                         int32_t n_map, const double* h_maps /* [n_map][npix] */,
                         double* orf_out /* [n_map][n_psr][n_psr] */);
/* The launch plan fpta_orf_anisotropic makes for a shape, a pure function of its arguments (split: the value of
 * FPTA_OPT_ORF_SPLIT). Host only, no context. It also checks the shape: FPTA_EINVAL (message from
 * fpta_last_error(NULL)) for a bad nside, npix != 12 nside^2 or a count out of range. info: pulsars per tile side,
 * pixels per chunk, maps per group, lower-triangle tiles, pixel chunks, K-splits in use, chunks per split, map groups,
 * map groups per launch, workspace bytes. The K-splits do not depend on n_map. */
#define FPTA_ORF_PLAN_LEN 10
int fpta_orf_plan(int32_t n_psr, int32_t nside, int64_t npix, int32_t n_map, int64_t split,
                  int64_t* info /* [FPTA_ORF_PLAN_LEN] */);

/* ------------------------------------------------------------------ timing-model projection
 * The weighted least-squares fit of a pulsar's timing model (the design matrix of fakepta/fake_pta.py make_Mmat; the
 * reference never applies it) removed from residuals (added without a change of FPTA_VERSION: no existing call
 * changes). This text is the specification.
 * For pulsar p with n_p TOAs, design matrix M_p [n_p][m_p], 0 <= m_p <= 16, and weights w > 0, a vector r becomes
 *   r' = r - M_p (M_p^T W M_p)^+ M_p^T W r,   W = diag(w).
 * The normal equations are never formed. On the host, in long double: every column of W^(1/2) M_p is scaled to unit
 * norm, then orthogonalised against the columns kept before it by modified Gram-Schmidt, twice; a column that is all
 * zero, or whose norm after both passes is <= rcond (relative to its scaled norm, 1), is dropped. rcond <= 0 means
 * 1e-10. The kept columns, rounded to fp64, are the basis Q_p [n_p][k_p], k_p the rank. With s = sqrt(w) (fp64) the
 * device computes g = Q_p^T (s o r) and r' = r - (Q_p g) / s on fp64 MFMA (k_tm_project), without atomics: a vector's
 * result is bit-identical whatever the number of vectors of the call, its position among them and its neighbours.
 * A pulsar of rank 0 keeps its samples bit for bit. weights NULL: unit weights. ncol_psr NULL: every pulsar uses all
 * n_col columns; else pulsar p uses the leading ncol_psr[p] <= n_col columns of its rows. rank_out NULL or [n_psr].
 * Validated on the host before anything is uploaded or launched (FPTA_EINVAL, the message names the pulsar, TOA and
 * column): n_col outside [0, 16], a column count outside [0, n_col], a non-finite entry in a column in use, a weight
 * that is not positive and finite. Kernel time is booked under FPTA_K_DENSE, one entry per call.
 *
 * fpta_batch_set_timing_model: the model of the batch layout (after fpta_batch_set_toas, else FPTA_ESTATE); M is
 *   [n_toa_total][n_col] row-major in the layout's TOA order. n_col == 0 clears the model, and so does
 *   fpta_batch_set_toas.
 * fpta_batch_project: projects the context's last block in place on the context's stream (FPTA_ESTATE without a block
 *   or without a model). fpta_batch_download, _checksums and _correlations afterwards see the post-fit block; the next
 *   block is not affected. Blocks streamed by fpta_batch_synth_checksums / fpta_multi_synth are not projected.
 * fpta_tm_project: one call for any array, independent of the batch layout: res [n_vec][offs[n_psr]] in and out. A
 *   pulsar may have no TOAs. */
int fpta_batch_set_timing_model(fpta_ctx* ctx, int32_t n_col, const double* M /* [n_toa_total][n_col] */,
                                const int32_t* ncol_psr, const double* weights, double rcond, int32_t* rank_out);
int fpta_batch_project(fpta_ctx* ctx);
int fpta_tm_project(fpta_ctx* ctx, int32_t n_psr, const int64_t* offs, const double* M /* [n_toa_total][n_col] */,
                    int32_t n_col, const int32_t* ncol_psr, const double* weights, double rcond, int32_t n_vec,
                    double* res /* [n_vec][n_toa_total] */, int32_t* rank_out);

/* ------------------------------------------------------------------ Fourier fit
 * The Fourier coefficients of residuals: the adjoint of the synthesis, residual block -> per-pulsar, per-realization
 * amplitudes, and the cross-spectrum of an array from them (added without a change of FPTA_VERSION: no existing call
 * changes). This text is the specification.
 * For pulsar p with n_p >= 0 TOAs t, radio frequencies nu and weights w > 0 the model is r = M_p b + F_p a:
 *   M_p [n_p][m_p], 0 <= m_p <= 16, a nuisance design (the timing model, say), marginalised and not returned;
 *   F_p [n_p][K], K = sum_c 2 N_c <= 512, the columns of 1 .. 4 components in order. Component c has N_c >= 1
 *   frequencies f_c, all positive and finite, a chromatic index idx_c and a reference frequency freqf_c; its columns
 *   are (freqf_c / nu)^idx_c cos(2 pi f_c[k] t), k = 0 .. N_c - 1, then (freqf_c / nu)^idx_c sin(2 pi f_c[k] t): the
 *   order of signal_model[...]['fourier'] (fakepta/fake_pta.py:385-387). idx_c == 0: the factor is 1 and nu is not
 *   read. f is [sum_c N_c] for the whole array (f_is_common != 0) or [n_psr][sum_c N_c].
 * The fit is the joint weighted least squares min |W^(1/2) (r - M_p b - F_p a)|^2, W = diag(w); the result is
 * a [K], in the units of r. The normal equations are never formed. On the host, in long double (cos / sin of the
 * long-double argument): every column of W^(1/2) [M_p F_p] is scaled to unit norm; the columns are taken in order,
 * M_p's first, and orthogonalised against the kept ones by modified Gram-Schmidt, twice; a column that is all zero,
 * or whose norm after both passes is <= rcond, is dropped. rcond <= 0 means 1e-10. A dropped Fourier column has
 * coefficient exactly 0 and a 0 in the kept mask: a pulsar with fewer TOAs than columns, or a frequency of 1 / yr
 * beside annual nuisance columns, drops columns instead of failing. With W^(1/2) [M_p F_p]_kept = Q R the inverse of R
 * is upper triangular, so a_kept = R_FF^-1 Q_F^T (s o r), s = sqrt(w): the host forms A_p = R_FF^-1 Q_F^T diag(s)
 * (with the column scaling undone), [K][n_p], zero rows for dropped columns, rounds it once to fp64 and uploads it;
 * the device computes a = A_p r on fp64 MFMA (k_fit_apply) and nothing else, without atomics: a vector's coefficients
 * are bit-identical whatever the number of vectors of the call, its position among them and its neighbours. The
 * operator takes 8 K n_toa_total bytes on the host and on the device; an allocation that fails is FPTA_ENOMEM with
 * the size in the message. weights NULL: unit weights. ncol_psr NULL: every pulsar uses all n_col columns of M
 * [n_toa_total][n_col]; else pulsar p the leading ncol_psr[p]. rank_out (NULL or [n_psr]) gets the number of kept
 * Fourier columns, kept_out (NULL or [n_psr][K]) the kept mask.
 * Validated on the host before anything is uploaded or launched (FPTA_EINVAL; the message names the pulsar, TOA,
 * column, component or mode): n_col outside [0, 16], a column count outside [0, n_col], a non-finite entry in a column
 * in use, a weight that is not positive and finite, n_comp outside [1, 4], N_c < 1, K > 512, a frequency that is not
 * positive and finite, a non-finite idx, a non-finite epoch, and with idx_c != 0 a freqf_c or a nu that is not positive
 * and finite. Kernel time is booked under FPTA_K_DENSE, one entry per call.
 *
 * fpta_batch_set_fit: the fit of the batch layout (after fpta_batch_set_toas, else FPTA_ESTATE), with the layout's
 *   TOAs and radio frequencies. n_comp == 0 clears it, and so does fpta_batch_set_toas. Independent of
 *   fpta_batch_set_timing_model.
 * fpta_batch_fit: fits the context's last block on the context's stream (FPTA_ESTATE without a block or without a
 *   fit). The block is read only: what is computed from it, and every later block, is unaffected. The result stays on
 *   the device as [n_psr][K][R_pad], realizations contiguous; coef_host NULL or [n_psr][K][n_real].
 * fpta_batch_fit_cross: from the last fpta_batch_fit result (FPTA_ESTATE without one), for a common grid only
 *   (FPTA_EINVAL otherwise): out [sum_c N_c][n_psr][n_psr],
 *     X[m][a][b] = sum over the block's realizations of (a_cos^a a_cos^b + a_sin^a a_sin^b) of mode m,
 *   modes in component order, as a Gram on fp64 MFMA (k_fit_cross): the lower triangle computed and mirrored, in a
 *   fixed order, bit-symmetric. The caller divides by the realization count and accumulates across blocks.
 * fpta_fit_coefficients: one call for any array, independent of the batch layout: res [n_vec][offs[n_psr]],
 *   coef_out [n_psr][K][n_vec]. A pulsar may have no TOAs: its coefficients are zero. */
int fpta_batch_set_fit(fpta_ctx* ctx, int32_t n_comp, const int32_t* n_modes, const double* f, int32_t f_is_common,
                       const double* idx, const double* freqf, int32_t n_col,
                       const double* M /* [n_toa_total][n_col] */, const int32_t* ncol_psr, const double* weights,
                       double rcond, int32_t* rank_out, uint8_t* kept_out);
/* info[0] = K of the fit that is set (0: none), info[1] = sum_c N_c, info[2] = 1 for a common grid, info[3] = the
 * realizations of the last fpta_batch_fit result (0: none): what sizes coef_host and fpta_batch_fit_cross's out. */
int fpta_batch_fit_info(fpta_ctx* ctx, int64_t* info /* [4] */);
int fpta_batch_fit(fpta_ctx* ctx, double* coef_host);
int fpta_batch_fit_cross(fpta_ctx* ctx, double* out);
int fpta_fit_coefficients(fpta_ctx* ctx, int32_t n_psr, const int64_t* offs, const double* toas, const double* nu,
                          int32_t n_comp, const int32_t* n_modes, const double* f, int32_t f_is_common,
                          const double* idx, const double* freqf, int32_t n_col,
                          const double* M /* [n_toa_total][n_col] */, const int32_t* ncol_psr, const double* weights,
                          double rcond, int32_t n_vec, const double* res /* [n_vec][n_toa_total] */,
                          double* coef_out /* [n_psr][K][n_vec] */, int32_t* rank_out, uint8_t* kept_out);

/* ------------------------------------------------------------------ optimal statistic
 * The noise-weighted optimal cross-correlation statistic of every realization of a block: per realization one number
 * per pair-weight matrix, from which the host derives the amplitude estimate and S/N of an overlap reduction function
 * (ORF), the joint fit of several ORFs and the binned pair correlations (added without a change of FPTA_VERSION: no
 * existing call changes). This text is the specification.
 * A "Fourier column" is (freqf / nu)^idx cos / sin(2 pi f_k t), cosines then sines, as in the Fourier fit above.
 * Per pulsar p (n_p >= 0 TOAs): weights w > 0 (NULL: unit); a nuisance design M_p [n_p][m_p <= 16]; Gaussian-process
 * components c = 0 .. C - 1, 1 <= C <= 8, with q = sum_c 2 N_c <= 1024 Fourier columns in all. Component c has
 * frequencies (f [sum_c N_c] for the whole array, or [n_psr][sum_c N_c]), a chromatic index idx_c, a reference
 * frequency freqf_c, an optional TOA mask (mask NULL, or [C][n_toa_total]: the component's columns are zero where its
 * flag is 0; system noise) and prior variances phi [n_psr][sum_c N_c] >= 0 per pulsar and mode, the same for the
 * cosine and the sine. A mode with phi = 0 is left out of the model for that pulsar.
 * One component is the target (the common process): N modes, K = 2 N <= 512 columns F_p, and a template spectrum
 * phi_hat [N] > 0. Its own phi stays part of P_p.
 *   P_p = W^-1 + sum_c F_c Phi_c F_c^T + M_p inf M_p^T   (the timing model marginalised with infinite variance, so
 *         whether the block was projected does not matter),
 *   X_p = F_p^T P_p^-1 r_p  [K], one per realization,   Z_p = F_p^T P_p^-1 F_p  [K][K];
 * a pulsar without TOAs has X = 0 and Z = 0. Per pair a < b: N_ab = tr(Z_a phi_hat Z_b phi_hat), phi_hat the diagonal
 * over the K columns; rho_ab,r = X_a^T phi_hat X_b / N_ab; sigma_ab^2 = 1 / N_ab; a pair with N_ab = 0 has no rho and
 * carries weight 0 everywhere. For J >= 0 symmetric pair-weight matrices G_j [n_psr][n_psr] (diagonal ignored) the one
 * per-realization device quantity is
 *   Q[j][m][r] = sum_{a<b} G_j[a][b] phi_hat_m (X_a,cos m,r X_b,cos m,r + X_a,sin m,r X_b,sin m,r),
 *   Q[j][r] = sum_m Q[j][m][r], summed in mode order.
 * The host derives the rest from Q and N_ab. A single ORF Gamma (G = Gamma): A2_r = Q_r / sum_{a<b} Gamma_ab^2 N_ab,
 * S/N_r = Q_r / sqrt(sum_{a<b} Gamma_ab^2 N_ab). Several ORFs at once: C A_r = Q_.,r with C_jj' = sum_{a<b} Gamma^j_ab
 * Gamma^j'_ab N_ab. Binned correlations (G = the indicator of the pairs of an angular bin): rho_bin,r = Q_r /
 * sum_{pairs of the bin} N_ab.
 * On the host, in long double, P_p and the normal equations are never formed: the columns of the stacked matrix
 * [W^(1/2) T ; D^(1/2)], T = [M_p, the Fourier columns with phi > 0, the target's last], D = 0 on M_p's columns and
 * 1 / phi on the others, are scaled to unit norm and orthogonalised in order by modified Gram-Schmidt, twice. M_p's
 * columns follow the timing-model projection's rank rule (rcond; a dropped column is not marginalised); a Fourier
 * column cannot drop. With the stacked Q = [Q1 ; Q2] and R, P^-1 T e_j = W^(1/2) Q1 R^-T e_j D_jj for a column of the
 * model, without a subtraction; a target column with phi = 0 takes W^(1/2) (I - Q1 Q1^T) W^(1/2) F_k. B_p = F_p^T
 * P_p^-1 [K][n_p] is rounded once to fp64 and uploaded (8 K n_toa_total bytes on the host and on the device; a failed
 * allocation is FPTA_ENOMEM with the size in the message), Z_p = B_p F_p and N_ab stay on the host. The device
 * computes X = B_p r with the Fourier fit's kernel (k_fit_apply) on an operator slot and a coefficient buffer of its
 * own, so a Fourier fit and an optimal statistic can both be set, and Q on fp64 MFMA (k_os_pairs, k_os_reduce): the
 * pair products of a realization are formed once and contracted with all J matrices, the strict lower triangle only,
 * in a fixed order and without atomics. A realization's X and Q are bit-identical whatever the number of realizations,
 * its position among them and its neighbours. The block is read only.
 * Validated on the host before anything is uploaded or launched (FPTA_EINVAL; the message names the pulsar, component,
 * mode or pair): everything the Fourier fit refuses (with C in [1, 8] and q <= 1024), a target index out of range,
 * K > 512, a phi that is negative or not finite, a phi_hat that is not positive and finite, a G entry that is not
 * finite, a G that is not symmetric (compared exactly). Kernel time is booked under FPTA_K_DENSE, one entry per call.
 *
 * fpta_batch_set_os: the statistic of the batch layout (after fpta_batch_set_toas, else FPTA_ESTATE). rank_out (NULL
 *   or [n_psr]) gets the kept columns of M_p, nab_out (NULL or [n_psr][n_psr]) N_ab (symmetric, zero diagonal).
 *   n_comp == 0 clears it, and so does fpta_batch_set_toas. Independent of fpta_batch_set_timing_model and
 *   fpta_batch_set_fit.
 * fpta_batch_os: the statistic of the context's last block on the context's stream (FPTA_ESTATE without a block or
 *   without a statistic set). Q NULL or [J][n_real], Q_mode NULL or [J][N][n_real], X NULL or [n_psr][K][n_real].
 * fpta_os_statistic: one call for any array and n_vec residual vectors res [n_vec][offs[n_psr]], independent of the
 *   batch layout. A pulsar may have no TOAs. */
int fpta_batch_set_os(fpta_ctx* ctx, int32_t n_comp, const int32_t* n_modes, const double* f, int32_t f_is_common,
                      const double* idx, const double* freqf, const double* phi /* [n_psr][sum_c N_c] */,
                      const uint8_t* mask /* NULL or [n_comp][n_toa_total] */, int32_t target,
                      const double* phi_hat /* [N_target] */, int32_t n_col,
                      const double* M /* [n_toa_total][n_col] */, const int32_t* ncol_psr, const double* weights,
                      double rcond, int32_t n_g, const double* G /* [n_g][n_psr][n_psr] */, int32_t* rank_out,
                      double* nab_out);
/* info[0] = K of the statistic that is set (0: none), info[1] = N, info[2] = J, info[3] = the realizations of the
 * last fpta_batch_os result (0: none): what sizes Q, Q_mode and X. */
int fpta_batch_os_info(fpta_ctx* ctx, int64_t* info /* [4] */);
int fpta_batch_os(fpta_ctx* ctx, double* Q, double* Q_mode, double* X);
int fpta_os_statistic(fpta_ctx* ctx, int32_t n_psr, const int64_t* offs, const double* toas, const double* nu,
                      int32_t n_comp, const int32_t* n_modes, const double* f, int32_t f_is_common,
                      const double* idx, const double* freqf, const double* phi, const uint8_t* mask, int32_t target,
                      const double* phi_hat, int32_t n_col, const double* M, const int32_t* ncol_psr,
                      const double* weights, double rcond, int32_t n_g, const double* G, int32_t n_vec,
                      const double* res /* [n_vec][n_toa_total] */, double* Q, double* Q_mode, double* X,
                      int32_t* rank_out, double* nab_out);

/* ---- sky scrambles of the optimal statistic ----
 * The significance of an optimal-statistic S/N by sky scrambles (Cornish & Sampson 2016; Taylor et al. 2017): the
 * statistic above under n_scr further pair-weight matrices, and the rank of the observed S/N among them (added without
 * a change of FPTA_VERSION: no existing call changes). This text is the specification.
 * A scramble j is a set of fictitious unit position vectors pos[j] [n_psr][3], whose matrix is Hellings-Downs,
 *   x = (1 - p_a . p_b) / 2 (every operation rounded once, the two leading products summed first),
 *   G_ab = 1.5 x ln x - x / 4 + 1 / 2,
 * or an explicit symmetric matrix G[j] [n_psr][n_psr]. Only the pairs a > b enter; they are kept as rows
 * Gs [n_scr][n_pair_pad] in the order of numpy's tril_indices(n_psr, -1), pair e = a (a - 1) / 2 + b, n_pair_pad the
 * next multiple of 16 (zero padding). With X_p, phi_hat and N_ab of the statistic that is set, per realization r:
 *   Y_ab[r] = sum_k phi_hat_k X_a,k X_b,k  over the K = 2 N columns (cosines, then sines), made once per block,
 *   Qs[j][r] = sum_{a>b} Gs[j][ab] Y_ab[r]   (one fp64 MFMA product [n_scr, n_pair] x [n_pair, n_real]),
 *   norm[j] = sum_{a>b} Gs[j][ab]^2 N_ab,   snr_null[j][r] = Qs[j][r] / sqrt(norm[j]),
 *   snr_obs[o][r] = Q[o][r] / sqrt(sum_{a>b} G_o[ab]^2 N_ab) for each of the n_g matrices G_o of the statistic,
 *   count_ge[o][r] = #{j : snr_null[j][r] >= snr_obs[o][r]},
 *   mean, std (ddof = 0, two passes in scramble order) and max of snr_null[.][r],
 *   match[j][o] = sum Gs[j] G_o / sqrt(sum G_o^2 sum Gs[j]^2), unweighted sums over the pairs a > b.
 * snr_obs and snr_null come from one device function. Fixed operation order, no atomics: a scramble's row of Qs is
 * bit-identical whatever the other scrambles, a realization's column whatever the number of realizations, its
 * position among them and its neighbours. The block is read only. An observed matrix without a pair of positive N_ab
 * has snr_obs NaN or infinite and count_ge 0.
 * Validated on the host before anything is uploaded or launched (FPTA_EINVAL with the reason; a refused call leaves
 * the previous set in place): n_scr > 65536, pair rows of more than 8 GiB (8 n_scr n_pair_pad bytes), not exactly one
 * of pos and G, n_psr < 2, a position that is not finite or not of unit length within 1e-12, a matrix that is not
 * symmetric, a pair weight that is not finite (coincident directions; the message names scramble and pair), a scramble
 * whose norm is not positive.
 *
 * fpta_batch_set_os_scrambles: the scrambles of the batch layout's statistic (after fpta_batch_set_os, else
 *   FPTA_ESTATE). n_scr == 0 clears them, and so do fpta_batch_set_os and fpta_batch_set_toas. norm_out NULL or
 *   [n_scr], match_out NULL or [n_scr][n_g].
 * fpta_batch_os_scrambles_info: info[0] = n_scr of the set (0: none), info[1] = n_g, info[2] = n_pair, info[3] = the
 *   realizations of the last fpta_batch_os_scrambles result (0: none).
 * fpta_batch_os_scrambles: on the context's last block and stream (FPTA_ESTATE without a block, a statistic or
 *   scrambles). It runs both stages of fpta_batch_os first, whose results are then those of fpta_batch_os alone, then
 *   k_scr_pairs, k_scr_gemm and k_scr_rank; one FPTA_K_DENSE entry. Each output may be NULL: snr_obs and count_ge
 *   [n_g][n_real], mean, std and max [n_real], snr_null [n_scr][n_real] (kept on the device only when asked for).
 * fpta_os_scrambles: one call for any array and n_vec residual vectors, fpta_os_statistic's arguments and the scramble
 *   inputs; the same kernels. Q NULL or [n_g][n_vec], X NULL or [n_psr][K][n_vec], qs NULL or [n_scr][n_vec] (Qs
 *   itself), nab_out NULL or [n_psr][n_psr].
 * fpta_os_scramble_match: match [n_scr][n_ref] of the Hellings-Downs matrices of pos [n_scr][n_psr][3] against any
 *   reference matrices ref [n_ref][n_psr][n_psr], without a statistic (drawing scrambles of a small match);
 *   rows_out gets the device's pair rows, unpadded. */
int fpta_batch_set_os_scrambles(fpta_ctx* ctx, int32_t n_scr, const double* pos /* NULL or [n_scr][n_psr][3] */,
                                const double* G /* NULL or [n_scr][n_psr][n_psr] */, double* norm_out,
                                double* match_out);
int fpta_batch_os_scrambles_info(fpta_ctx* ctx, int64_t* info /* [4] */);
int fpta_batch_os_scrambles(fpta_ctx* ctx, double* snr_obs, int64_t* count_ge, double* mean, double* std_out,
                            double* max_out, double* snr_null);
int fpta_os_scrambles(fpta_ctx* ctx, int32_t n_psr, const int64_t* offs, const double* toas, const double* nu,
                      int32_t n_comp, const int32_t* n_modes, const double* f, int32_t f_is_common,
                      const double* idx, const double* freqf, const double* phi, const uint8_t* mask, int32_t target,
                      const double* phi_hat, int32_t n_col, const double* M, const int32_t* ncol_psr,
                      const double* weights, double rcond, int32_t n_g, const double* G, int32_t n_scr,
                      const double* scr_pos, const double* scr_G, int32_t n_vec,
                      const double* res /* [n_vec][n_toa_total] */, double* Q, double* X, double* norm_out,
                      double* match_out, double* snr_obs, int64_t* count_ge, double* mean, double* std_out,
                      double* max_out, double* snr_null, double* qs, double* nab_out);
int fpta_os_scramble_match(fpta_ctx* ctx, int32_t n_psr, int32_t n_scr, const double* pos, int32_t n_ref,
                           const double* ref /* [n_ref][n_psr][n_psr] */, double* match_out,
                           double* rows_out /* NULL or [n_scr][n_pair] */);

/* ---- optimal statistic under a noise spectrum per realization ----
 * The statistic above with P_p of realization r built from row r of per-realization spectra, the tables of
 * fpta_batch_synth_spectra: every realization of a block is weighted by its own noise model (a P-P run, a population
 * prior), and one residual block under many draws of the noise parameters gives the noise-marginalised optimal
 * statistic (added without a change of FPTA_VERSION: no existing call changes). This text is the specification.
 * The components, the design, the weights, the target, phi_hat, X_p, Z_p, N_ab and Q are those of the optimal
 * statistic. The components are split into a varied set V (n_vary in [1, 4] distinct component indices, the target
 * the last of them) with q = 2 sum_{c in V} N_c <= 128 Fourier columns T_p, and the fixed rest. vary_seg[v] is the
 * signal of the batch layout (the id fpta_batch_add_signal returned, with as many modes as the component) whose
 * amplitudes a_r, from the call's table or else the layout's, give the varied component its prior variance
 * phi_r = a_r^2 in realization r; the phi argument's entries of the varied components are validated and not used.
 * With P0_p = W^-1 + sum_{c not in V} F_c Phi_c F_c^T + M_p inf M_p^T the host plans once per pulsar, in long double
 * by the route above with the columns of V not part of the model (the projection form of a target column with
 * phi = 0),
 *   B0_p = T_p^T P0_p^-1  [q][n_p], rounded once to fp64, and A_p = B0_p T_p  [q][q] from the unrounded B0_p.
 * The device computes z = B0_p r (k_fit_apply on an operator slot of its own) and per (pulsar, realization), with
 * s = a_r over the q columns and t the target's trailing K columns,
 *   C = I + s A_p s = L D L^T (no pivoting: C is symmetric positive definite with eigenvalues >= 1; a column with
 *       s = 0 decouples),   W = C^-1 (s o [A_p e_t, z]),
 *   X_k = W_kz / s_k,   Z_kj = W_kj / s_k   (from T^T P^-1 = s^-1 C^-1 s B0: no subtraction);
 *   a target mode with s_k = 0 is not part of that realization's model and takes the projection form
 *   X_k = z_k - sum_i A_ki s_i W_iz,   Z_kj = A_kj - sum_i A_ki s_i W_ij.
 * Then N_ab[r] = sum_jk Z'_a,jk Z'_b,jk with Z' = phi_hat^(1/2) Z phi_hat^(1/2) for a >= b (fp64 MFMA, the K^2 entries
 * in index order), norm[j][r] = sum_{a>b} G_j[a][b]^2 N_ab[r] for all n_g matrices and joint[j][j'][r] =
 * sum_{a>b} G_j G_j' N_ab[r] for the first n_orf of them (row-major over a > b), and Q, Q_mode from X by the kernels
 * of the optimal statistic. Z' takes 8 K^2 n_psr bytes per realization: the call runs in chunks of realizations, and a
 * failed allocation is FPTA_ENOMEM with the size. Fixed operation order, no atomics: a realization's results are
 * bit-identical whatever the number of realizations, its position among them and its neighbours. The block is read
 * only. Kernel time is booked under FPTA_K_DENSE, one entry per call.
 *
 * fpta_batch_set_os_spectra: after fpta_batch_set_toas (else FPTA_ESTATE); n_comp == 0 clears it, and so does
 *   fpta_batch_set_toas. Independent of the timing model, the Fourier fit and fpta_batch_set_os. FPTA_EINVAL with the
 *   reason: everything fpta_batch_set_os refuses, a varied set that is empty, larger than 4, repeats a component or
 *   does not end in the target, q > 128 ("more than 128"), an unknown or repeated layout signal or one whose mode
 *   count differs, n_orf outside [0, n_g]. rank_out NULL or [n_psr].
 * fpta_batch_os_spectra: the statistic of the context's last block (FPTA_ESTATE without a block or without a statistic
 *   set). The tables are those of fpta_batch_synth_spectra with n_rows[t] = the block's realizations, validated the
 *   same way before anything is uploaded or launched; a table for a signal outside the varied set is FPTA_EINVAL
 *   naming the signal. n_tab = 0: the layout's amplitudes for every realization. Each output may be NULL: Q
 *   [n_g][n_real], Q_mode [n_g][N][n_real], X [n_psr][K][n_real], norm [n_g][n_real], joint [n_orf][n_orf][n_real],
 *   nab [n_real][n_psr][n_psr] (the entries a >= b; the others are 0), zp [n_real][n_psr][K][K] (Z'). */
int fpta_batch_set_os_spectra(fpta_ctx* ctx, int32_t n_comp, const int32_t* n_modes, const double* f,
                              int32_t f_is_common, const double* idx, const double* freqf,
                              const double* phi /* [n_psr][sum_c N_c] */,
                              const uint8_t* mask /* NULL or [n_comp][n_toa_total] */, int32_t target,
                              const double* phi_hat /* [N_target] */, int32_t n_vary, const int32_t* vary,
                              const int32_t* vary_seg, int32_t n_col, const double* M /* [n_toa_total][n_col] */,
                              const int32_t* ncol_psr, const double* weights, double rcond, int32_t n_g,
                              const double* G /* [n_g][n_psr][n_psr] */, int32_t n_orf, int32_t* rank_out);
int fpta_batch_os_spectra(fpta_ctx* ctx, int32_t n_tab, const int32_t* seg, const int32_t* form,
                          const int32_t* per_pulsar, const int32_t* n_rows, const double* const* tables, double* Q,
                          double* Q_mode, double* X, double* norm, double* joint, double* nab, double* zp);

/* Likelihood ratio of a common process on a spectrum grid: per realization of a block the Gaussian log-likelihood as a
 * function of the target's spectrum, against "no such process", on G grid points (added without a change of
 * FPTA_VERSION: no existing call changes). This text is the specification.
 * The inputs are the optimal statistic's (above) without a template and pair weights: weights, a nuisance design M_p
 * marginalised with infinite variance, C <= 8 components with prior variances phi [n_psr][sum_c N_c], one of them the
 * target with N modes and K = 2 N <= 256 columns F_p. The target's own prior is not part of the base model (its phi
 * entries are validated and otherwise ignored):
 *   P0_p = W^-1 + sum_{c != target} F_c Phi_c F_c^T + M_p inf M_p^T.
 * phi_grid [G][N] >= 0, 1 <= G <= 4096: row g is the target's prior variance per mode, the same for the cosine and the
 * sine and for every pulsar (an uncorrelated common process when the target is a common signal; each pulsar's own noise
 * surface when it is a per-pulsar signal). With X_p = F_p^T P0_p^-1 r_p and Z_p = F_p^T P0_p^-1 F_p:
 *   C_pg = I + phi_g^(1/2) Z_p phi_g^(1/2)   (symmetric, eigenvalues >= 1),   C_pg = L L^T,
 *   U_pg = L^-1 phi_g^(1/2)   (lower triangular; row and column of a mode with phi = 0 are zero),
 *   ld_pg = 2 sum_i ln L_ii,   q[p][g][r] = |U_pg X_p,r|^2,
 *   dlnL[g][r] = sum_p (q[p][g][r] - ld_pg) / 2, summed in pulsar order
 *              = ln p(r | phi_g) - ln p(r | phi = 0) with the timing model marginalised.
 * A pulsar without TOAs contributes exactly 0 and a grid row of zeros gives exactly 0. ECORR is not part of the
 * weights; the other components stay at the values given.
 * On the host, in long double with sums in index order: B_p = F_p^T P0_p^-1 by the optimal statistic's orthogonalisation
 * with the target's phi = 0 (every target row takes the projection form), rounded once to fp64; Z_p = B_p F_p from the
 * unrounded B_p; per grid point the Cholesky factor of C_pg, U_pg by forward substitution, rounded once to fp64, and
 * ld_pg. The device holds B (8 K n_toa_total bytes) and U in 16-row groups with only the columns up to each group's
 * diagonal block (8 * 128 * g (g + 1) bytes per pulsar and grid point, g = ceil(K / 16)); a failed allocation is
 * FPTA_ENOMEM with the size in the message. X = B_p r comes from the Fourier fit's kernel (k_fit_apply) on a third
 * operator slot with its own coefficient buffer, q from fp64 MFMA (k_lnl_quad: per row group only the k-steps up to
 * its diagonal block, the squares summed in a fixed order, no atomics), dlnL from k_lnl_reduce; the per-pulsar terms
 * (q - ld) / 2 added on the host in pulsar order equal dlnL bit for bit. A realization's results are bit-identical
 * whatever the number of realizations, its position among them and its neighbours, and a grid point's whatever G. The
 * block is read only. Validated on the host before anything is uploaded or launched (FPTA_EINVAL): everything the
 * optimal statistic refuses of these inputs, K > 256, G outside [1, 4096], a grid entry that is negative or not finite
 * (the message names the grid row and mode). Kernel time is booked under FPTA_K_DENSE, one entry per call.
 *
 * fpta_batch_set_lnl: the grid of the batch layout (after fpta_batch_set_toas, else FPTA_ESTATE). rank_out (NULL or
 *   [n_psr]) gets the kept columns of M_p, ld_out (NULL or [n_psr][n_grid]) ld_pg. n_comp == 0 clears it, and so does
 *   fpta_batch_set_toas. Independent of the timing model, the Fourier fit and the optimal statistic.
 * fpta_batch_lnl_info: info[0] = K of the grid that is set (0: none), info[1] = N, info[2] = G, info[3] = the
 *   realizations of the last fpta_batch_lnl result (0: none).
 * fpta_batch_lnl: the grid of the context's last block on the context's stream (FPTA_ESTATE without a block or a
 *   grid). dlnl NULL or [G][n_real], q_psr NULL or [n_psr][G][n_real], X NULL or [n_psr][K][n_real].
 * fpta_lnl_grid: one call for any array and n_vec residual vectors res [n_vec][offs[n_psr]], independent of the batch
 *   layout. U_out NULL or [n_psr][G][K][K]: the plan's fp64 U, dense, row-major, zeros above the diagonal. */
int fpta_batch_set_lnl(fpta_ctx* ctx, int32_t n_comp, const int32_t* n_modes, const double* f, int32_t f_is_common,
                       const double* idx, const double* freqf, const double* phi /* [n_psr][sum_c N_c] */,
                       const uint8_t* mask /* NULL or [n_comp][n_toa_total] */, int32_t target, int32_t n_col,
                       const double* M /* [n_toa_total][n_col] */, const int32_t* ncol_psr, const double* weights,
                       double rcond, int32_t n_grid, const double* phi_grid /* [n_grid][N_target] */,
                       int32_t* rank_out, double* ld_out);
int fpta_batch_lnl_info(fpta_ctx* ctx, int64_t* info /* [4] */);
int fpta_batch_lnl(fpta_ctx* ctx, double* dlnl, double* q_psr, double* X);
int fpta_lnl_grid(fpta_ctx* ctx, int32_t n_psr, const int64_t* offs, const double* toas, const double* nu,
                  int32_t n_comp, const int32_t* n_modes, const double* f, int32_t f_is_common, const double* idx,
                  const double* freqf, const double* phi, const uint8_t* mask, int32_t target, int32_t n_col,
                  const double* M, const int32_t* ncol_psr, const double* weights, double rcond, int32_t n_grid,
                  const double* phi_grid, int32_t n_vec, const double* res /* [n_vec][n_toa_total] */, double* dlnl,
                  double* q_psr, double* X, int32_t* rank_out, double* ld_out, double* U_out);

/* Correlated likelihood grid: the likelihood grid above with the target's prior coupled between pulsars by an overlap
 * reduction function (Hellings-Downs, monopole, dipole, any symmetric positive semidefinite Gamma), per realization of
 * a block, per ORF and per grid point (added without a change of FPTA_VERSION: no existing call changes). This text is
 * the specification.
 * The inputs are the likelihood grid's, with the target's frequencies the same for every pulsar, and
 * n_orf factors A [n_orf][n_psr][n_psr], 1 <= n_orf <= 8, each any finite matrix with A A^T = Gamma_o (the lower
 * Cholesky factor, or a factor with zero columns for a singular ORF). The target's prior is
 *   cov(a_pk, a_ql) = Gamma_pq phi_k delta_kl,   both quadratures of a mode sharing phi.
 * K = 2 N, n = n_psr K <= 16384, index (p, k) = p K + k, cosine columns first. With P0_p, X_p and Z_p as above (the
 * target left out of the base model), s_g = phi_g^(1/2) per column and D_g = diag(s_g tiled n_psr times):
 *   T_o[(i,k),(j,l)] = sum_p A_pi A_pj Z_p[k][l]   (symmetric, independent of the grid),
 *   V_o[(j,l)][r]    = sum_p A_pj X_p[l][r]        (independent of the grid),
 *   C_og = I + D_g T_o D_g = L_og L_og^T   (eigenvalues >= 1),   ld[o][g] = 2 sum_i ln L_ii,
 *   q[o][g][r] = |L_og^-1 D_g V_o[:, r]|^2,
 *   dlnL[o][g][r] = (q[o][g][r] - ld[o][g]) / 2 = ln p(r | Gamma_o, phi_g) - ln p(r | phi = 0)
 * with the timing model marginalised: Woodbury's identity and the matrix-determinant lemma in the symmetric form of
 * the likelihood grid. Neither Gamma^-1 nor phi^-1 appears: modes with phi = 0 and singular ORFs need no special case,
 * and a grid row of zeros gives exactly 0. With A = I this is the likelihood grid's dlnL.
 * On the host, in long double with sums in index order: B_p and Z_p as for the likelihood grid; T_o summed in pulsar
 * order from Z_p's lower triangles and rounded once to fp64, stored [n_pad][n_pad] with n_pad = n rounded up to 64 and
 * the padding zero; s_g rounded once. At set time the device writes C_og, factors it in place with the dense path's
 * blocked Cholesky and sums ld in index order; the factors stay cached (8 n_orf G n_pad^2 bytes, at most 32 GiB). Per
 * block X = B_p r comes from k_fit_apply on a fifth operator slot, V from k_clnl_mix (fp64 MFMA), q from k_clnl_solve,
 * a forward substitution blocked by 64 rows with 64 right-hand sides per workgroup on fp64 MFMA, the squares added in
 * row order without atomics, and dlnL from k_clnl_reduce. Nothing is factored per block. A realization's results are
 * bit-identical whatever the number of realizations, its position among them and its neighbours, and a grid point's
 * whatever G. The block is read only. Validated on the host before anything is uploaded or launched (FPTA_EINVAL, the
 * message names the offender): everything the likelihood grid refuses, a target whose frequencies differ between
 * pulsars, n_orf outside [1, 8], a factor entry that is not finite, n > 16384, cached factors beyond 32 GiB (the
 * message states the bytes). A non-positive Cholesky pivot is FPTA_EINVAL naming ORF, grid point and pivot. Beside the
 * cached factors a call on a block of R realizations takes 8 n_orf G n_pad R' bytes of work space for the
 * substitution's Y (R' = R rounded up to 64; 4.9 GB on 100 pulsars with K = 60, G = 100, R = 1024), sized at the call
 * and outside that budget: a failed allocation is FPTA_ENOMEM with the size in the message. The one-shot call frees its
 * factors and work space before it returns; the batch slot keeps them until the grid is set again or cleared. Kernel
 * time is booked under FPTA_K_DENSE, one entry per fpta_batch_clnl call.
 *
 * fpta_batch_set_clnl: the grid of the batch layout (after fpta_batch_set_toas, else FPTA_ESTATE). rank_out (NULL or
 *   [n_psr]) gets the kept columns of M_p, ld_out (NULL or [n_orf][n_grid]) ld. n_comp == 0 clears it, and so does
 *   fpta_batch_set_toas. Independent of the other consumers of the block.
 * fpta_batch_clnl_info: info[0] = K of the grid that is set (0: none), info[1] = G, info[2] = n_orf, info[3] = the
 *   realizations of the last fpta_batch_clnl result (0: none).
 * fpta_batch_clnl: the grid of the context's last block on the context's stream (FPTA_ESTATE without a block or a
 *   grid). dlnl and q NULL or [n_orf][G][n_real], V NULL or [n_orf][n][n_real], X NULL or [n_psr][K][n_real].
 * fpta_clnl_grid: one call for any array and n_vec residual vectors res [n_vec][offs[n_psr]], independent of the batch
 *   layout. T_out NULL or [n_orf][n][n]: the plan's fp64 T, dense, row-major. */
int fpta_batch_set_clnl(fpta_ctx* ctx, int32_t n_comp, const int32_t* n_modes, const double* f, int32_t f_is_common,
                        const double* idx, const double* freqf, const double* phi /* [n_psr][sum_c N_c] */,
                        const uint8_t* mask /* NULL or [n_comp][n_toa_total] */, int32_t target, int32_t n_col,
                        const double* M /* [n_toa_total][n_col] */, const int32_t* ncol_psr, const double* weights,
                        double rcond, int32_t n_grid, const double* phi_grid /* [n_grid][N_target] */, int32_t n_orf,
                        const double* A /* [n_orf][n_psr][n_psr] */, int32_t* rank_out, double* ld_out);
int fpta_batch_clnl_info(fpta_ctx* ctx, int64_t* info /* [4] */);
int fpta_batch_clnl(fpta_ctx* ctx, double* dlnl, double* q, double* V, double* X);
int fpta_clnl_grid(fpta_ctx* ctx, int32_t n_psr, const int64_t* offs, const double* toas, const double* nu,
                   int32_t n_comp, const int32_t* n_modes, const double* f, int32_t f_is_common, const double* idx,
                   const double* freqf, const double* phi, const uint8_t* mask, int32_t target, int32_t n_col,
                   const double* M, const int32_t* ncol_psr, const double* weights, double rcond, int32_t n_grid,
                   const double* phi_grid, int32_t n_orf, const double* A, int32_t n_vec,
                   const double* res /* [n_vec][n_toa_total] */, double* dlnl, double* q, double* V, double* X,
                   int32_t* rank_out, double* ld_out, double* T_out);

/* Continuous-wave F-statistics: per realization of a block the Earth-term Fe-statistic of a circular binary on a grid
 * of directions and frequencies, with its maxima, and the incoherent Fp-statistic per frequency (Babak & Sesana 2012;
 * Ellis, Siemens & Creighton 2012; added without a change of FPTA_VERSION: no existing call changes). This text is the
 * specification.
 * The inputs are the optimal statistic's (above) without a target, a template and pair weights: weights w > 0, a
 * nuisance design M_p [n_p][m_p <= 16] marginalised with infinite variance under the timing-model projection's rank
 * rule, C <= 7 Gaussian-process components with prior variances phi [n_psr][sum_c N_c] >= 0, all of them noise (a
 * common process enters as each pulsar's auto-term):
 *   P_p = W^-1 + sum_c F_c Phi_c F_c^T + M_p inf M_p^T,   (x|y)_p = x^T P_p^-1 y.
 * New inputs: G frequencies fgw [G] > 0, 1 <= G <= 256, neither harmonics nor ordered; n_sky directions sky
 * [n_sky][2] = (cos theta_s, phi_s), 1 <= n_sky <= 12288; the pulsars' unit vectors pos [n_psr][3], n_psr <= 256.
 * With s_g(t) = sin 2 pi f_g t and c_g(t) = cos 2 pi f_g t at the pulsar's TOAs, per pulsar and frequency
 *   x_pg = [(r_p|s_g), (r_p|c_g)] per realization,   m_pg = [[(s|s), (s|c)], [(s|c), (c|c)]].
 * The antenna patterns of pulsar p for direction s are fpta_cw_accumulate's: m = (sin phi, -cos phi, 0), n = (-cos th
 * cos phi, -cos th sin phi, sin th), Om = (-sin th cos phi, -sin th sin phi, -cos th), F+ = ((m.p)^2 - (n.p)^2) / (2 (1
 * + Om.p)), Fx = (m.p)(n.p) / (1 + Om.p), so an injected source and the statistic agree on the convention.
 *   N(s, g) = [sum_p F+ x_s, sum_p F+ x_c, sum_p Fx x_s, sum_p Fx x_c],
 *   M(s, g) = sum_p [[F+^2, F+ Fx], [F+ Fx, Fx^2]] (x) m_pg   (4 x 4),
 *   Fe[s][g][r] = N^T M^-1 N / 2      (the omega^(-1/3) of the literature's basis cancels),
 *   Fp[g][r] = sum_p x_pg^T m_pg^-1 x_pg / 2, summed in pulsar order.
 * 2 Fe is chi^2 with 4 degrees of freedom under the null and has non-centrality (h|h) under a source at (s, g); 2 Fp
 * is chi^2 with 2 n_eff[g] degrees of freedom. The pulsar term, an evolving frequency, the maximum-likelihood
 * amplitudes M^-1 N and ECORR in the weights are out of scope.
 * A pulsar whose column lies in the span of its marginalised model, (s|s) <= rcond^2 s^T W s or the same for c (the
 * timing-model rank rule's threshold; 1 / yr beside annual design columns, say), drops out at that frequency: its two
 * rows of B_p and its m_pg are exactly zero.
 * The inverses are made on the host in long double: the matrix is scaled to unit diagonal and factored by Cholesky;
 * a diagonal entry that is not positive and finite, or a pivot (the diagonal of the scaled Schur complement, before
 * its square root) <= rcond_fe (<= 0: 1e-10), makes the point singular; else the inverse is D^-1/2 L^-T L^-1 D^-1/2
 * with L^-1 by forward substitution, rounded once to fp64. A direction for which 1 + Om.p is exactly zero for some
 * pulsar is singular at every frequency and that pulsar's F+ and Fx read 0 in the table. A singular (s, g) has Fe =
 * NaN (with one pulsar every point is singular). A pulsar whose m_pg is singular (no TOAs, say) adds nothing to Fp,
 * its m^-1 reads 0, and n_eff[g] counts the others.
 * Reductions: Fe_f[g][r] = max_s Fe with its argmax, Fe_max[r] = max_g Fe_f with its (s, g). NaN never wins a maximum,
 * ties go to the lower index (for Fe_max: the lower frequency, then that frequency's direction), all-NaN gives NaN and
 * index -1.
 * On the host (long double, sums in index order): B_p [K = 2 G][n_p] with row g = c_g^T P_p^-1 and row G + g = s_g^T
 * P_p^-1, by the optimal statistic's orthogonalisation with the frequency grid appended as a common achromatic target
 * with phi = 0 (every row takes the projection form), rounded once to fp64; m_pg from the unrounded B_p; the antenna
 * table F [2 n_sky][n_psr] (row 2 s: F+, row 2 s + 1: Fx), M and M^-1 [n_sky][G][10] (the upper triangle row by row:
 * 00 01 02 03 11 12 13 22 23 33) and m^-1 [n_psr][G][3] = (ss, sc, cc), each rounded once. The device computes X [n_psr]
 * [K][n_real] = B_p r with the Fourier fit's kernel (k_fit_apply) on a fourth operator slot with its own coefficient
 * buffer, N on fp64 MFMA with k = the pulsars in order (k_fe_sky: the quadratic form, the map and the maximum over the
 * directions per lane, merged in a fixed order, no atomics) and Fp and the maximum over the frequencies in k_fe_reduce.
 * A realization's numbers are bit-identical whatever the number of realizations, its position among them and its
 * neighbours. The block is read only. Validated on the host before anything is uploaded or launched (FPTA_EINVAL):
 * everything the optimal statistic refuses of these inputs (the frequency grid counts as component C), C > 7, n_psr >
 * 256, G outside [1, 256], n_sky outside [1, 12288], a frequency that is not positive and finite, a cos theta outside
 * [-1, 1], a phi that is not finite, a position that is not a unit vector to 1e-6 (the message names the frequency,
 * direction or pulsar). A failed allocation is FPTA_ENOMEM with the size in the message. Kernel time is booked under
 * FPTA_K_DENSE, one entry per call.
 *
 * fpta_batch_set_fe: the statistics of the batch layout (after fpta_batch_set_toas, else FPTA_ESTATE). rank_out (NULL
 *   or [n_psr]) gets the kept columns of M_p; F_out (NULL or [2 n_sky][n_psr]), Minv_out (NULL or [n_sky][G][10]),
 *   minv_out (NULL or [n_psr][G][3]) and neff_out (NULL or [G]) the host tables. n_comp == 0 clears it (a model without
 *   a process passes one component with phi = 0), and so does fpta_batch_set_toas. Independent of the timing model,
 *   the Fourier fit, the optimal statistic and the likelihood grid.
 * fpta_batch_fe_info: info[0] = K of the statistics that are set (0: none), info[1] = G, info[2] = n_sky, info[3] =
 *   the realizations of the last fpta_batch_fe result (0: none).
 * fpta_batch_fe: the statistics of the context's last block on the context's stream (FPTA_ESTATE without a block or
 *   without statistics set). Each output may be NULL: fe_max [n_real]; arg_max [2][n_real] (row 0 the direction, row
 *   1 the frequency); fe_f and arg_f [G][n_real]; fp [G][n_real]; fe_map [n_sky][G][n_real] (written on the device only
 *   when asked for: 8 n_sky G n_real bytes); X [n_psr][K][n_real].
 * fpta_fe_statistic: one call for any array and n_vec residual vectors res [n_vec][offs[n_psr]], independent of the
 *   batch layout. A pulsar may have no TOAs; n_comp may be 0 (white noise only). */
int fpta_batch_set_fe(fpta_ctx* ctx, int32_t n_comp, const int32_t* n_modes, const double* f, int32_t f_is_common,
                      const double* idx, const double* freqf, const double* phi /* [n_psr][sum_c N_c] */,
                      const uint8_t* mask /* NULL or [n_comp][n_toa_total] */, int32_t n_col,
                      const double* M /* [n_toa_total][n_col] */, const int32_t* ncol_psr, const double* weights,
                      double rcond, int32_t n_fgw, const double* fgw, int32_t n_sky, const double* sky /* [n_sky][2] */,
                      const double* pos /* [n_psr][3] */, double rcond_fe, int32_t* rank_out, double* F_out,
                      double* Minv_out, double* minv_out, int32_t* neff_out);
int fpta_batch_fe_info(fpta_ctx* ctx, int64_t* info /* [4] */);
int fpta_batch_fe(fpta_ctx* ctx, double* fe_max, int32_t* arg_max, double* fe_f, int32_t* arg_f, double* fp,
                  double* fe_map, double* X);
int fpta_fe_statistic(fpta_ctx* ctx, int32_t n_psr, const int64_t* offs, const double* toas, const double* nu,
                      int32_t n_comp, const int32_t* n_modes, const double* f, int32_t f_is_common,
                      const double* idx, const double* freqf, const double* phi, const uint8_t* mask, int32_t n_col,
                      const double* M, const int32_t* ncol_psr, const double* weights, double rcond, int32_t n_fgw,
                      const double* fgw, int32_t n_sky, const double* sky, const double* pos, double rcond_fe,
                      int32_t n_vec, const double* res /* [n_vec][n_toa_total] */, double* fe_max, int32_t* arg_max,
                      double* fe_f, int32_t* arg_f, double* fp, double* fe_map, double* X, int32_t* rank_out,
                      double* F_out, double* Minv_out, double* minv_out, int32_t* neff_out);

/* Replaces fakepta/fake_pta.py:201-230 (add_white_noise), with ECORR fixed (defects D1/D2):
 *   residuals[t] += sigma[t] * z[t]  +  sum over blocks b containing t: ecorr_sigma[b] * zb[b]
 * Blocks are CSR: block_offs[n_blocks+1] into block_idx (TOA indices, any order).
 * n_blocks may be 0 (then block_* / ecorr_sigma / zb may be NULL). */
int fpta_white_accumulate(fpta_ctx* ctx, int64_t n_toa, const double* sigma, const double* z,
                          int64_t n_blocks, const int64_t* block_offs, const int64_t* block_idx,
                          const double* ecorr_sigma, const double* zb, double* residuals);

/* ------------------------------------------------------------------ dense covariance
 * The reference's covariance-matrix route (fakepta/fake_pta.py:389-420, :493-524). Signals are
 * given as segments like fpta_gp_accumulate: seg_nmodes[n_seg]; f and w hold sum(seg_nmodes)
 * values with w = psd * df (the reference's np.repeat(psd * df, 2)); seg_idx / seg_freqf give
 * each segment's chromatic factor (freqf/nu)^idx. For a backend's system noise pass only that
 * backend's TOAs (the reference builds the covariance of the masked TOAs, :398-405).
 * white_var: NULL or [n_toa] white-noise variances, added on the diagonal. */

/* Replaces make_time_correlated_noise_cov (fakepta/fake_pta.py:389-420) and, summed over
 * segments, the red part of make_noise_covariance_matrix (:493-513); with white_var, the
 * total covariance np.diag(white_cov) + red_cov of draw_noise_model (:517):
 *   cov[i][j] = sum_s ch_s(i) ch_s(j) sum_k w[k] (cos(2 pi f_k t_i) cos(2 pi f_k t_j)
 *                                                + sin(2 pi f_k t_i) sin(2 pi f_k t_j))
 *               + (i == j ? white_var[i] : 0)
 * Basis generation + fp64 MFMA Gram (lower tiles, mirrored). cov: host [n_toa][n_toa]. */
int fpta_gp_covariance(fpta_ctx* ctx, int64_t n_toa, const double* toas, const double* nu,
                       int32_t n_seg, const int32_t* seg_nmodes, const double* f, const double* w,
                       const double* seg_idx, const double* seg_freqf, const double* white_var,
                       double* cov);

/* Replaces draw_noise_model(residuals) (fakepta/fake_pta.py:520-523), the Wiener estimate
 *   out = red_cov^T C^-1 residuals,  C = red_cov + diag(white_var),
 * evaluated as residuals - white_var * C^-1 residuals (red_cov is symmetric) through a device
 * Cholesky factorisation of C instead of the reference's explicit inverse. white_var is
 * required. FPTA_EINVAL if C is not positive definite. out may alias residuals. */
int fpta_noise_wiener(fpta_ctx* ctx, int64_t n_toa, const double* toas, const double* nu,
                      int32_t n_seg, const int32_t* seg_nmodes, const double* f, const double* w,
                      const double* seg_idx, const double* seg_freqf, const double* white_var,
                      const double* residuals, double* out);

/* Batched draw_noise_model() (fakepta/fake_pta.py:518-519): n_real realizations of N(0, C),
 * C = red_cov + diag(white_var), as x = L z with L the device Cholesky factor of C and z
 * Philox normals ctr = (toa, 0xFFFFFFFF, 0xFFFFFFF2, g >> 1), pick [g & 1], g = real0 + r.
 * Same distribution as the reference's np.random.multivariate_normal (which factors C by SVD);
 * the draws themselves follow this library's stream. out: host [n_real][n_toa]. */
int fpta_noise_draw(fpta_ctx* ctx, int64_t n_toa, const double* toas, const double* nu,
                    int32_t n_seg, const int32_t* seg_nmodes, const double* f, const double* w,
                    const double* seg_idx, const double* seg_freqf, const double* white_var,
                    uint64_t seed, int64_t real0, int32_t n_real, double* out);

/* ------------------------------------------------------------------ batched realizations
 * Many independent realizations of the whole array on device (north-star steps 1-4):
 * Philox4x32-10 draws -> ORF mixing -> fused basis/contraction -> white/ECORR.
 * Draw streams (invariant to batching and to the number of GPUs):
 *   GP   : ctr = (mode, pulsar, segment, realization), key = seed -> (z_cos, z_sin)
 *   white: ctr = (toa, 0xFFFFFFFF, 0xFFFFFFF0, realization>>1), pick [realization&1]
 *   ECORR: ctr = (block>>1, 0xFFFFFFFF, 0xFFFFFFF1, realization), pick [block&1]
 * Replaces the Python loop of fakepta/fake_pta.py:648-668 + correlated_noises.py:153-160
 * when many realizations of one array are needed. */

/* Array layout: CSR offsets [n_psr+1], toas [s], nu [MHz]. Clears previously added signals. */
int fpta_batch_set_toas(fpta_ctx* ctx, int32_t n_psr, const int64_t* offs, const double* toas,
                        const double* nu);
/* kind 0 = per-pulsar GP: f, amp are [n_psr][n_modes] (amp 0 disables a pulsar);
 * kind 1 = common GP:    f, amp are [n_modes], L is [n_psr][n_psr] (x = L z).
 * amp = sqrt(psd * df). mask: NULL or uint8 [n_toa_total]. Returns the segment id (>= 0). */
int fpta_batch_add_signal(fpta_ctx* ctx, int32_t kind, int32_t n_modes, const double* f,
                          const double* amp, double idx, double freqf, const double* L,
                          const uint8_t* mask);
/* White noise sigma [n_toa_total] (NULL disables) and ECORR blocks (CSR over global TOA
 * indices, ecorr_sigma [n_blocks]; n_blocks 0 disables). */
int fpta_batch_set_white(fpta_ctx* ctx, const double* sigma, int64_t n_blocks,
                         const int64_t* block_offs, const int64_t* block_idx,
                         const double* ecorr_sigma);
int fpta_batch_clear_signals(fpta_ctx* ctx);
/* Synthesize realizations real0 .. real0+n_real-1 into the context's device buffer
 * [n_real][n_toa_total]. If out != NULL the result is also copied to host memory
 * (row-major, same shape). coeffs_out: NULL or host [n_psr][K][n_real] coefficient dump
 * (K = fpta_batch_info column count) for validation. seed: any 64-bit value (the Philox key).
 * 0 <= real0 and real0 + n_real <= 2^32 here, in fpta_batch_synth_checksums and in fpta_multi_synth
 * (FPTA_EINVAL "realization index exceeds the 32-bit Philox counter word" otherwise, the resident
 * block untouched); fpta_noise_draw takes real0 + n_real <= 2^33. */
int fpta_batch_synth(fpta_ctx* ctx, uint64_t seed, int64_t real0, int32_t n_real, double* out,
                     double* coeffs_out);
/* fpta_batch_synth with a spectrum per realization for n_tab of the layout's signals: realization real0 + r takes the
 * same Philox draws, in the same operation order (a z, respectively the rounded product a sum_q L[p][q] z[q]), with
 * a from row r of the signal's table instead of from the layout. Signals without a table keep the layout's
 * amplitudes; the layout is not modified (the next fpta_batch_synth is unchanged), and n_tab = 0 is fpta_batch_synth.
 * Table t belongs to signal seg[t] (the id fpta_batch_add_signal returned; each at most once), holds n_rows[t] =
 * n_real rows and is read from tables[t]:
 *   form[t] 0, amplitudes sqrt(psd * df): [n_real][n_modes] (per_pulsar[t] 0: a common signal, or a per-pulsar signal
 *              whose pulsars share the row) or [n_real][n_psr][n_modes] (per_pulsar[t] 1: a per-pulsar signal only),
 *              n_modes as given to fpta_batch_add_signal;
 *   form[t] 1, power law: (log10_A, gamma) as [n_real][2] or [n_real][n_psr][2]; the device evaluates
 *              sqrt(powerlaw(f_k, log10_A, gamma) (f_k - f_{k-1})), f_{-1} = 0, on the signal's own frequencies
 *              (fakepta/spectrum.py:14-17 with fyr = 1 / Julian year).
 * A mode whose layout amplitude is exactly 0 (a pulsar without the signal, modes past a pulsar's own, the padding
 * mode) stays 0 in every realization: form 1 writes 0 there, and so does a shared row for the pulsars it does not
 * apply to; a form-0 entry that is nonzero where no pulsar it covers has an amplitude is an error.
 * FPTA_EINVAL, naming the signal (and realization, pulsar, mode), with the resident block untouched: a non-finite or
 * negative amplitude, a non-finite parameter, an unknown or repeated signal id, a per-pulsar table for a common
 * signal, n_rows[t] != n_real. The consumers of the block (optimal statistic, likelihood grids, ...) keep the
 * layout's amplitudes as their noise model. fpta_batch_synth_checksums and fpta_multi_synth take no tables. */
int fpta_batch_synth_spectra(fpta_ctx* ctx, uint64_t seed, int64_t real0, int32_t n_real, int32_t n_tab,
                             const int32_t* seg, const int32_t* form, const int32_t* per_pulsar,
                             const int32_t* n_rows, const double* const* tables, double* out, double* coeffs_out);
/* Validation mode: same as fpta_batch_synth but the standard normals come from the host:
 * z [n_real][n_seg][n_psr][n_modes_max][2] (cos, sin); white/ECORR are not added. */
int fpta_batch_synth_from_z(fpta_ctx* ctx, int32_t n_real, int32_t n_modes_max, const double* z,
                            double* out);
/* Copy realizations [r_begin, r_begin + r_count) of the last block to host [r_count][n_toa_total]
 * (the "residual block" gather of SURVEY.md §8(e); the full block can be tens of GB). */
int fpta_batch_download(fpta_ctx* ctx, int32_t r_begin, int32_t r_count, double* host);
/* Device pointer of the last synthesized block and its leading dimension (n_toa_total). */
int fpta_batch_device_out(fpta_ctx* ctx, double** dptr, int64_t* ld, int32_t* n_real);
/* Per-realization sum and sum of squares of the last block, computed on device
 * (deterministic order). sums: host [n_real][2]. */
int fpta_batch_checksums(fpta_ctx* ctx, double* sums);
/* Realizations real0 .. real0 + n_real - 1 streamed through this context in batches of <= batch (the context's
 * block then holds the last batch) with their checksums written to sums [n_real][2] (as fpta_batch_checksums,
 * from the gridded interpolation's partial sums where it runs): batches are queued back to back with no host
 * synchronisation in between (pinned staging, one sync at the end). The single-device form of
 * fpta_multi_synth; fakepta_amd.batch.simulate_sharded uses it when no per-batch consumer is given. */
int fpta_batch_synth_checksums(fpta_ctx* ctx, uint64_t seed, int64_t real0, int64_t n_real, int32_t batch,
                               double* sums);
/* Correlation statistics of the last block, the estimator of
 * fakepta/correlated_noises.py:14-34 (C_r[a][b] = dot(res_a, res_b) / n) for arrays whose pulsars
 * all have n TOAs (FPTA_EINVAL otherwise):
 *   mode 0: host out [n_real][P][P], C_r per realization
 *   mode 1: host out [P][P], sum over realizations of C_r
 *   mode 2: host out [P][P], sum over realizations of C_r[a][b] / sqrt(C_r[a][a] C_r[b][b])
 *   mode 3: host out [n_real][P], auto-correlations C_r[p][p]
 * Sums are formed in a fixed order (bitwise reproducible). */
int fpta_batch_correlations(fpta_ctx* ctx, int32_t mode, double* out);
/* info[0]=n_psr info[1]=n_toa_total info[2]=n_seg info[3]=K columns info[4]=max toas/pulsar */
int fpta_batch_info(fpta_ctx* ctx, int64_t* info);

/* Gridded-path plan of the batch layout and the path the last batch took (for rooflines):
 * out[0] synthesis path of the last batch (1 direct, 2 MFMA, 3 VALU, 4 gridded), out[1] plan usable,
 * out[2] interpolation chunks, out[3] k_grid_dft FMAs per realization, out[4] k_grid_interp FMAs per
 * realization, out[5] direct-contraction FMAs per realization, out[6] grid values per realization,
 * out[7] interpolation-weight bytes, out[8] the FPTA_OPT_GRID_MFMA mask in force, out[9] the exponential-of-
 * semicircle kernel's design estimate exp(-pi w sqrt(1 - 1/sigma)) of the relative aliasing error at the
 * width/oversampling options in force (an estimate, not a bound: a flat spectrum errs by about 4 times as much, a
 * single top mode by up to 2.8e-11 per unit coefficient at the defaults, 18 times; tests/test_grid_modes.py; auto
 * selection takes the gridded path only when the estimate is <= 2e-12), out[10] width w, out[11] oversampling sigma,
 * out[12] grid signals of the plan (signals after FPTA_OPT_GRID_COALESCE), out[13] layout signals, out[14]
 * mean band rows per chunk (all grid signals, padded to 4), out[15] the interpolation kernel of the last gridded
 * block: 0 none, else 1 + 4 kind + 2 (white / ECORR epilogue) + (fused partial checksums), kind 0
 * k_grid_interp_mfma, 1 k_grid_interp_ws, 2 k_grid_interp_ws2, 3 k_grid_interp_lds, 4 k_grid_interp_st, 5
 * k_grid_interp_u, 6 / 7 k_grid_interp_psr with 4 / 8 band steps, 10 k_grid_interp_wr (diagnostic builds only),
 * 11 .. 19 the k_grid_fused<NQ, ODD, GEN, HALF> instances (8 / 12 band steps' operands x no draws / draws / draws
 * from an odd realization, then half-chunk bands x the same three); out[16] (FPTA_VERSION 10100) the interpolation
 * MFMA FMAs per realization of the last gridded block as its kernel ran them (half-chunk bands: both halves' steps;
 * else out[4]); out[17]
 * (FPTA_VERSION 10200) 1 when the last block's k_grid_fused also made the next block's common-signal mix
 * (FPTA_OPT_FUSED_NEXT_MIX), out[18] 1 when the last block took its common-signal mix from the previous block's kernel
 * (no k_gen_mix launch).
 * fpta_batch_grid_info_n writes the first min(n_out, FPTA_GRID_INFO_LEN) values and returns FPTA_GRID_INFO_LEN
 * (negative on error); fpta_batch_grid_info keeps the round-1 contract: out[0..8], host double[9]. */
#define FPTA_GRID_INFO_LEN 19
int fpta_batch_grid_info_n(fpta_ctx* ctx, double* out, int32_t n_out);
int fpta_batch_grid_info(fpta_ctx* ctx, double* out);
/* Why the last batch did not take the gridded path (signal count, non-harmonic grid, error bound, cost,
 * n_real below the threshold, ...); "" when it did. Owned by the context, valid until the next batch. */
const char* fpta_batch_path_reason(const fpta_ctx* ctx);

/* ------------------------------------------------------------------ multi-device (one process)
 * one context per listed device (a device may repeat), the layout replicated on
 * each, realizations [real0, real0 + n_real) sharded contiguously (device g of G owns
 * [real0 + g n/G, real0 + (g+1) n/G)) and streamed in batches of <= batch realizations; only the
 * per-realization checksums (sum, sum of squares; fpta_batch_checksums order) come back, in global
 * realization order: checksums_out host [n_real][2]. The result is bit-identical for every device
 * count and batch size. Replaces running the reference's make_fake_array / add_* loop once per
 * realization (fakepta/fake_pta.py:648-668, fakepta/correlated_noises.py:153-160) over a large
 * ensemble. One-process-per-GPU jobs (torchrun) use fakepta_amd.batch.simulate_sharded instead. */
typedef struct fpta_multi fpta_multi;
int fpta_multi_create(int32_t n_dev, const int32_t* devices, fpta_multi** out);
int fpta_multi_destroy(fpta_multi* m);
const char* fpta_multi_last_error(const fpta_multi* m);
int fpta_multi_size(const fpta_multi* m);
/* The i-th device context (options, kernel statistics, downloads of its last block). */
fpta_ctx* fpta_multi_context(fpta_multi* m, int32_t i);
int fpta_multi_set_toas(fpta_multi* m, int32_t n_psr, const int64_t* offs, const double* toas,
                        const double* nu);
int fpta_multi_add_signal(fpta_multi* m, int32_t kind, int32_t n_modes, const double* f,
                          const double* amp, double idx, double freqf, const double* L,
                          const uint8_t* mask);
int fpta_multi_set_white(fpta_multi* m, const double* sigma, int64_t n_blocks,
                         const int64_t* block_offs, const int64_t* block_idx,
                         const double* ecorr_sigma);
int fpta_multi_set_option(fpta_multi* m, int32_t key, int64_t value);
int fpta_multi_synth(fpta_multi* m, uint64_t seed, int64_t real0, int64_t n_real, int32_t batch,
                     double* checksums_out);
/* How fpta_multi_synth brings the checksums to the host: FPTA_GATHER_RCCL keeps each device's
 * shard on the device and gathers them to device 0 with one ncclGather over xGMI (communicators from
 * ncclCommInitAll over the listed devices, made on first use; the devices must be distinct);
 * FPTA_GATHER_HOST copies each device's checksums into pinned host staging; FPTA_GATHER_AUTO (default) takes
 * RCCL when the devices are distinct. fpta_multi_last_gather: the route the last fpta_multi_synth took. */
#define FPTA_GATHER_AUTO 0
#define FPTA_GATHER_RCCL 1
#define FPTA_GATHER_HOST 2
int fpta_multi_set_gather(fpta_multi* m, int32_t mode);
int fpta_multi_last_gather(const fpta_multi* m);

/* ------------------------------------------------------------------ one process per GPU: RCCL
 * The library's own RCCL (ROCm 7.2, the same HIP runtime as the kernels) for realization-sharded jobs with one
 * process per GPU (fakepta_amd.batch.RcclComm; the reference loop that shards: correlated_noises.py:153-160).
 * Rank 0 makes the 128-byte unique id (fpta_comm_unique_id) and hands it to the other ranks out of band; every
 * rank then calls fpta_comm_init_rank on its context. Collectives run on the context's stream after all work
 * queued there, and return when their result is on the host. Only the job barrier / max of the elapsed time and
 * the checksum gather go through them: the data path has no collective. */
typedef struct fpta_comm fpta_comm;
#define FPTA_COMM_ID_BYTES 128
int fpta_comm_unique_id(void* id);
int fpta_comm_init_rank(fpta_ctx* ctx, int32_t nranks, int32_t rank, const void* id, fpta_comm** out);
int fpta_comm_destroy(fpta_comm* comm);
const char* fpta_comm_last_error(const fpta_comm* comm);
int fpta_comm_size(const fpta_comm* comm, int32_t* nranks, int32_t* rank);
/* *value (host) <- max over ranks of *value. Also the barrier of a timed region. */
int fpta_comm_max(fpta_comm* comm, double* value);
/* Every rank sends `count` doubles (host); rank 0 receives nranks * count, in rank order, into recv (host). */
int fpta_comm_gather(fpta_comm* comm, const double* send, int64_t count, double* recv);

/* ------------------------------------------------------------------ tuning / profiling */
#define FPTA_OPT_SYNTH_PATH 1     /* 0 auto, 1 direct (sincos per basis element), 2 fp64 MFMA, 3 fp64 VALU fused,
                                     4 gridded (real DFT to an oversampled phase grid + banded interpolation,
                                     harmonic grids only; aliasing error <= ~6e-12 relative at the defaults) */
#define FPTA_OPT_MFMA_MIN_REAL 2  /* auto: MFMA path when n_real >= this (default 16) */
#define FPTA_OPT_PROFILE 3        /* 1: time every batch kernel with HIP events on the ctx stream */
#define FPTA_OPT_ANCHOR 4         /* recurrence re-anchor interval in K-steps of 2 modes (0 = once per signal, default) */
#define FPTA_OPT_VALU_VARIANT 5   /* tile variant of the VALU fused kernel (0..5) */
#define FPTA_OPT_FUSE_WHITE 6     /* 1 (default): white/ECORR added in the synthesis epilogue; 0: separate pass */
#define FPTA_OPT_GRID_WIDTH 7     /* gridded path: interpolation kernel width in grid cells (default 15) */
#define FPTA_OPT_GRID_SIGMA 8     /* gridded path: grid oversampling x 100 (default 150) */
#define FPTA_OPT_GRID_MFMA 9      /* gridded path: bit 0 runs the DFT on fp64 MFMA (else fp64 VALU); the
                                     interpolation always runs on fp64 MFMA. Default 1. */
#define FPTA_OPT_FUSE_CHECKSUMS 10 /* 1: the gridded interpolation also writes per-(chunk, realization) partial
                                     sums (sum, sum of squares) of the block it stores, and
                                     fpta_batch_checksums reduces those (in a fixed order: deterministic, batch-
                                     split invariant) instead of re-reading the block. Default 0; other paths
                                     always take the full pass. */
#define FPTA_OPT_MIX_MFMA 11      /* ORF mixing of common signals for P >= 64 pulsars: 1 (default) on fp64 MFMA
                                     (k_mix_mfma), 0 the register-tiled fp64 VALU GEMM (k_mix_tiled) */
#define FPTA_OPT_OVERLAP 12       /* batch synthesis with several signals: 1 (default) draws each signal's
                                     coefficients on a second stream so the gridded DFT of one signal overlaps
                                     the draws of the next; 0 one stream. Results are identical. */
#define FPTA_OPT_INTERP_LDS 13    /* diagnostic builds only (FPTA_BUILD_DIAG; the product library refuses 1):
                                     gridded interpolation: 1 stages each chunk group's grid rows in LDS
                                     (k_grid_interp_lds) where every group fits and no white noise is fused;
                                     0 (default, faster on MI355X) the register-tiled k_grid_interp_mfma.
                                     Results are identical. */
#define FPTA_OPT_GRID_COALESCE 14 /* gridded path: 1 (default) sums, in coefficient space, the signals of a pulsar
                                     that share the base frequency w0 and the chromatic weight on every TOA (e.g.
                                     red noise and a common GWB on the pulsar's own span, or DM noise at a single
                                     radio frequency): they then share one grid and one interpolation band. Exact
                                     algebra (the sum is linear); results agree with 0 to rounding. */
#define FPTA_OPT_INTERP_WS 15     /* gridded interpolation: 1 (default) the warp-specialised k_grid_interp_ws
                                     (producer waves stage the operands in an LDS ring, compute waves only store,
                                     so stores never delay an operand load) for blocks without fused white noise
                                     or fused partial checksums, or k_grid_interp_ws2 (256-realization tiles, two
                                     workgroups per CU) when the padded realization count leaves fewer idle
                                     compute waves in 256- than in 512-realization tiles (C4: R = 256); 2 ws also
                                     for blocks with fused partial checksums; 3 ws2 for every plain block; 0 the
                                     register-pipelined k_grid_interp_mfma; 4 k_grid_interp_st for every block
                                     (compute waves hand their sums to storer waves through LDS; the storers add
                                     white noise / ECORR, store and reduce partial checksums). Results are
                                     identical. Variant builds only (FPTA_BUILD_DIAG): 0, 2, 3 (measured slower)
                                     and 4; the product library refuses them. */
#define FPTA_OPT_SIDE_SPLIT 16    /* pipelined gridded blocks (FPTA_OPT_OVERLAP): 1 the grid signal with the
                                     largest DFT, when it has no common (ORF-mixed) member, is drawn and
                                     transformed on a second side stream, beside the other signals' draws, mixing
                                     and DFT; 2 (default) the same, its DFT started after the common signals'
                                     draws + mixing queued on the first side stream (they get the room beside the
                                     previous block's interpolation first: C2 -1.3 %, C5 -1.4 %); 0 one side
                                     stream for all. Results are identical. 0 and 1 (measured slower): variant
                                     builds only (FPTA_BUILD_DIAG); the product library refuses them. */
#define FPTA_OPT_DFT_GEN 17       /* gridded path: 1 (default) a grid signal with a per-pulsar member draws its
                                     coefficients inside its DFT kernel (k_grid_dft_gen: Philox + Box-Muller into
                                     LDS, same counters and draws as k_gen); 0 k_gen writes them to the coefficient
                                     buffer and k_grid_dft_mfma reads them back. Same draws; sums agree to rounding.
                                     0 (measured slower): variant builds only (FPTA_BUILD_DIAG). */
#define FPTA_OPT_GEN_MIX 18       /* common signals of 64..256 pulsars (fp64 MFMA mixing): 2 (default) draws and ORF
                                     mixing in one kernel (k_gen_mix: normals in LDS, no zbuf round trip), one wave per
                                     16 realizations, 32 realizations per workgroup; 3 the same with 16 realizations
                                     per workgroup (a quarter of the LDS);
                                     1 waves of 32 realizations; 0 k_gen then k_mix_mfma. Same draws and products;
                                     results identical. 0, 1, 3 (equal or slower): variant builds only. */
#define FPTA_OPT_ASYNC_SUMS 19    /* streamed jobs (fpta_batch_synth_checksums, fpta_multi_synth): 1 a block's partial
                                     checksums are reduced on a stream of their own, beside the next block, into one
                                     of two partials buffers; 0 (default) on the context stream. Identical results.
                                     1 (measured slower): variant builds only (FPTA_BUILD_DIAG). */
#define FPTA_OPT_PART_GROUP 20    /* fused partial checksums (FPTA_OPT_FUSE_CHECKSUMS): the interpolation sums the partials
                                     of this many consecutive chunks (1 .. 16, default 16) in registers, in chunk order,
                                     and writes one {sum, sum of squares} row per group; the reduction then sums the
                                     groups in order. Deterministic and batch-split invariant for every value; the
                                     value changes the order of the additions (checksums agree to rounding). */
#define FPTA_OPT_INTERP_PSR 21    /* gridded path with one grid signal of <= 124 grid points whose coefficients the MFMA
                                     DFT would read from the coefficient buffer (e.g. C3's common GWB), <= 32 band
                                     rows and no fused white noise: 1 (default) k_grid_interp_psr (a workgroup makes
                                     one pulsar's grid for 64 realizations in LDS and interpolates the pulsar's chunks
                                     from it: no grid buffer, no separate DFT launch; pipelined blocks alternate two
                                     coefficient buffers); 0 the DFT + interpolation kernels. Results are identical. */
#define FPTA_OPT_INTERP_WR 22     /* diagnostic builds only (FPTA_BUILD_DIAG; the product library refuses 1): gridded
                                     plain blocks of <= 2 grid signals, R_pad a multiple of 256: 1 k_grid_interp_wr
                                     (each grid signal's band rows kept in a ring of LDS rows across consecutive chunks:
                                     only the rows the previous chunk did not hold are loaded; measured slower); 0
                                     (default) the other kernels. Results are identical. */
#define FPTA_OPT_INTERP_FUSED 23  /* gridded plain blocks (no white epilogue, no fused checksums) whose grids for 32
                                     realizations fit in LDS beside the draw ring with at most 4 DFT jobs of 32
                                     quarter-range rows and 2 grid signals (C2: 129 KB of grids): 1 (default)
                                     k_grid_fused (persistent workgroups, one per CU: 4 DFT waves draw and transform
                                     the next pulsar x 32 realizations into LDS while 4 interpolation waves read the
                                     current one: no grid buffer, no DFT launch), its interpolation on half-chunk
                                     bands (TOAs 0..15 and 16..31 of a chunk each with their own band rows) where
                                     that saves at least 3 % of the interpolation's MFMAs (C2: 11 %); 2 k_grid_fused
                                     on whole-chunk bands only; 3 half-chunk bands whenever the plan has them; 0 the
                                     DFT + interpolation kernels. Whole-chunk bands are bit-identical to the DFT +
                                     interpolation kernels; half-chunk bands group the band rows differently (sums
                                     agree to rounding). A layout k_grid_interp_psr serves keeps it. */
/* key 24 is retired (it was FPTA_OPT_FUSED_WHITE in 10100 .. 10200) and is never to be reused */
#define FPTA_OPT_FUSED_NEXT_MIX 25 /* (FPTA_VERSION 10200) pipelined gridded blocks on k_grid_fused (FPTA_OPT_OVERLAP 1)
                                     with one ORF-mixed common signal of 64 .. 256 pulsars drawn by k_gen_mix (C2's
                                     GWB): 1 (default) the kernel's waves with nothing left of their block draw and
                                     mix that signal for the next block of the same seed and size (first realization
                                     real0 + the stride from the block before when that is a whole number of blocks,
                                     else real0 + n_real) into the coefficient buffer that block reads; a batch_synth
                                     with that key then launches no k_gen_mix; after any other call the side streams
                                     wait for the kernel.
                                     0: every block runs k_gen_mix. Results are identical. */
#define FPTA_OPT_CW_SPLIT 26       /* fpta_cw_accumulate: 0 (default) auto: the source range is split over blocks when
                                     the TOAs alone leave the device mostly empty (a pure function of n_src and the
                                     total TOA count); n >= 1 forces n source splits (clamped to n_src). */
#define FPTA_OPT_ORF_SPLIT 27      /* fpta_orf_anisotropic: 0 (default) auto: the pixel range is cut into K-splits
                                     until the tiles fill the device (a pure function of n_psr and nside,
                                     fpta_orf_plan); n >= 1 forces n K-splits (clamped to the chunk count). */
#define FPTA_OPT_ROEMER_CHUNK 28   /* fpta_batch_roemer_accumulate with one table per realization: consecutive
                                     realizations that one k_roemer_block workgroup serves with one evaluation of the
                                     base orbits. 0 (default) auto: n_slab n_real / 1024 (n_slab the 256-TOA slabs of
                                     the layout), within 1 .. 32; n >= 1 forces n (clamped to 32). Results are
                                     identical. */
int fpta_set_option(fpta_ctx* ctx, int32_t key, int64_t value);
/* Current value of option `key` (same keys as fpta_set_option). */
int fpta_get_option(fpta_ctx* ctx, int32_t key, int64_t* value);
/* Build flags of the loaded library: FPTA_BUILD_DEBUG when built with -DFPTA_DEBUG (make debug: per-launch
 * synchronisation and device-side bounds checks; never used for measurements); FPTA_BUILD_DIAG when built with
 * -DFPTA_DIAG_KERNELS (make variant: the measured-and-not-adopted diagnostic kernels, e.g. FPTA_OPT_INTERP_LDS). */
#define FPTA_BUILD_DEBUG 1
#define FPTA_BUILD_DIAG 2
int fpta_build_flags(void);
/* Kernel ids for fpta_kernel_stats */
#define FPTA_K_GEN 0
#define FPTA_K_MIX 1
#define FPTA_K_SYNTH 2
#define FPTA_K_WHITE 3
#define FPTA_K_DENSE 4 /* dense covariance: basis + Gram, Cholesky, solves, draws; k_tm_project: one entry per call
                        * (fpta_batch_project, fpta_tm_project); k_fit_apply and k_fit_cross: one entry per call
                        * (fpta_batch_fit, fpta_fit_coefficients, fpta_batch_fit_cross); fpta_orf_anisotropic: one entry per
                          launch batch (k_orf_aniso + k_orf_reduce); fpta_batch_os, fpta_os_statistic: one entry per
                          call (k_fit_apply + k_os_pairs + k_os_reduce); fpta_batch_lnl, fpta_lnl_grid: one entry per
                          call (k_fit_apply + k_lnl_quad + k_lnl_reduce); fpta_batch_fe, fpta_fe_statistic: one entry per
                          call (k_fit_apply + k_fe_sky + k_fe_reduce) */
#define FPTA_K_GRID 5  /* gridded path: real-DFT grid values (k_grid_dft); its interpolation counts as SYNTH */
#define FPTA_K_CW 6    /* fpta_cw_accumulate: one entry per call (k_cw_prep + k_cw_main [+ k_cw_reduce]);
                        * fpta_batch_cw_accumulate: one entry per call (k_cw_block, or those kernels + k_cw_bcast) */
#define FPTA_K_EPHEM 7 /* fpta_ephem_kepler / fpta_ephem_orbits / fpta_roemer_accumulate: one entry per call;
                        * fpta_batch_roemer_accumulate: one entry per call (k_roemer_block, or k_roemer_main +
                        * k_cw_bcast) */
#define FPTA_K_N 8
/* Accumulated launches and HIP-event milliseconds of kernel `which` since the last reset. */
int fpta_kernel_stats(fpta_ctx* ctx, int32_t which, int64_t* count, double* total_ms);
int fpta_reset_stats(fpta_ctx* ctx);
int fpta_synchronize(fpta_ctx* ctx);

/* ------------------------------------------------------------------ test hooks */
/* Philox4x32-10 on device: ctr [n][4], key [2] -> out [n][4]. */
int fpta_debug_philox(fpta_ctx* ctx, int64_t n, const uint32_t* ctr, const uint32_t* key,
                      uint32_t* out);
/* The uniform -> normal map of every device draw (philox.h normals4) on n given Philox outputs: out[4 i + k] for the
 * words words[4 i .. 4 i + 3] (validation of the map on chosen words, e.g. its end points; oracle normals4). */
int fpta_debug_normals(fpta_ctx* ctx, int64_t n, const uint32_t* words, double* out);
/* Fill the last synthesized device block with `value` (tests: a later batch must overwrite every sample). */
int fpta_debug_fill_out(fpta_ctx* ctx, double value);
/* Which variant of the reported k_grid_fused instance the last gridded block ran (the name fpta_batch_grid_info_n
 * slot 15 reports is the same for both): *shape = 1 or 2, the instance specialised for the layout's term pattern
 * (1: grid signal 0 = a per-pulsar + a common member and signal 1 = a per-pulsar member; 2: one grid signal of one
 * common member); 0, the general instance; -1, the block ran no k_grid_fused. Additive (tests). */
int fpta_debug_fused_shape(fpta_ctx* ctx, int32_t* shape);
/* The intermediates the last dense call (fpta_gp_covariance / fpta_noise_wiener / fpta_noise_draw) of this context
 * left on the device, row-major into out [rows][cols], n = that call's n_toa: what = 0 the matrix [n][n] as it stands
 * (the covariance after fpta_gp_covariance; after the other two the Cholesky factor in the lower triangle, zeros above
 * the diagonal inside each 64 x 64 diagonal block and the covariance's untouched upper blocks elsewhere); what = 1
 * the solve's y = C^-1 residuals [n][1], after fpta_noise_wiener only; what = 2 the normals [n][n_real] (TOA-major)
 * of the last fpta_noise_draw. FPTA_ESTATE when the last dense call failed, did not produce the item, or left other
 * extents than rows x cols. Additive (tests). */
int fpta_debug_dense(fpta_ctx* ctx, int32_t what, int64_t rows, int64_t cols, double* out);

#ifdef __cplusplus
}
#endif
#endif /* FAKEPTA_AMD_H */
