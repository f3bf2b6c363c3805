"""Batched realizations: many independent draws of an array's noise model on one MI355X.

The reference produces one realization per Python call (make_fake_array / add_* /
add_common_correlated_noise, a loop over pulsars and modes). BatchSimulator takes the noise
model an array already carries (each Pulsar's signal_model and noisedict, as left by
make_fake_array or the add_* injectors) and re-draws it R times on the device:

    Philox4x32-10 draws -> ORF mixing -> fused basis/contraction -> white/ECORR

Realization r of seed s is the same whatever the batch split or number of GPUs (the Philox
counter carries the global realization index), so realizations shard across ranks with no
data-path collective. The draws are not numpy's MT19937 stream (SURVEY.md §7 'RNG parity');
the oracle (oracle/fakepta_oracle.py: batch_synth) restates the exact semantics.
"""
import numpy as np

from . import _capi
from . import fit as _fit
from . import lnl as _lnl
from . import clnl as _clnl
from . import fe as _fe
from . import os as _os
from . import tm as _tm
from fakepta.correlated_noises import orf_factor, orf_matrix

GP_NAMES = ("red_noise", "dm_gp", "chrom_gp")


def _df(f):
    return np.diff(np.append(0.0, f))


def _n_modes(sm):
    """Modes a stored signal carries: its coefficient pairs, at most len(f) (reconstruct_signal's zip,
    fake_pta.py:543; a common signal stores `components` pairs on a longer f_psd, correlated_noises.py:140-143)."""
    n = len(sm["f"])
    return min(n, np.shape(sm["fourier"])[1]) if "fourier" in sm else n


def batch_factor(orf_mat):
    """Square root of the ORF for batched draws: the lower Cholesky factor when the ORF is
    positive definite (HD, curn: triangular mixing on device, half the FLOPs), otherwise the SVD
    factor numpy's multivariate_normal uses (singular monopole / dipole ORFs). Any L with
    L L^T = ORF gives the reference's distribution; the drop-in path keeps numpy's exact factor."""
    try:
        return np.ascontiguousarray(np.linalg.cholesky(orf_mat))
    except np.linalg.LinAlgError:
        # singular ORF (monopole: rank 1, dipole: rank 3): the SVD factor with the directions of numerically zero
        # variance (singular values <= 1e-12 of the largest, i.e. rounding noise of a rank-r matrix) set to exact
        # zeros, so the device mixes (and draws normals for) only the first r columns; L L^T changes by <= 1e-12
        # relative
        _, s, _ = np.linalg.svd(orf_mat)
        L = orf_factor(orf_mat)
        L[:, s <= 1e-12 * s[0]] = 0.0
        return np.ascontiguousarray(L)


class BatchSimulator:
    """Device-resident noise model of an array of Pulsar objects.

    signals: names to include (default: every GP signal found in the pulsars' signal_model:
             red_noise, dm_gp, chrom_gp, '*system_noise*' and '*common*').
    white:   include EFAC/EQUAD white noise from each pulsar's noisedict.
    ecorr:   include ECORR epochs (ENTERPRISE convention 10^(2 log10_ecorr)).
    """

    def __init__(self, psrs, signals=None, white=True, ecorr=False, device=None, ctx=None):
        self.psrs = psrs
        self.ctx = ctx if ctx is not None else _capi.get_context(device)
        self.offs = np.concatenate([[0], np.cumsum([len(p.toas) for p in psrs])]).astype(np.int64)
        self.toas = np.concatenate([p.toas for p in psrs])
        self.freqs = np.concatenate([p.freqs for p in psrs])
        self.ctx.batch_set_toas(self.offs, self.toas, self.freqs)
        self._has_tm = False  # set_timing_model
        self._fit = None  # set_fourier_fit: dict(n_modes, f, idx, freqf, common)
        self._os = None  # set_optimal_statistic: dict(G, nab, n_orf, centres, counts, target, template)
        self._scr = None  # set_sky_scrambles: dict(J, positions)
        self._oss = None  # set_optimal_statistic_spectra: dict(G, n_orf, centres, counts, target, template, seg, names, K)
        self._lnl = None  # set_likelihood_grid: dict(phi, axes, ld, target)
        self._fe = None  # set_fe_statistic: dict(fgw, sky, n_eff)
        self._clnl = None  # set_correlated_likelihood: dict(phi, axes, ld, names, target)
        self.segments = []  # (name, kind, f, amp, idx, L, mask) — host copy for checking/reporting
        names = signals
        if names is None:
            names = []
            for p in psrs:
                for s in p.signal_model:
                    if s not in names and (s in GP_NAMES or "common" in s or "system_noise" in s):
                        names.append(s)
        for name in names:
            self._add_named(name)
        if white or ecorr:
            self._set_white(white, ecorr)

    # ------------------------------------------------------------------ layout building
    def _add_named(self, name):
        P = len(self.psrs)
        have = [p for p in self.psrs if name in p.signal_model]
        if not have:
            raise KeyError(f"no pulsar carries signal {name!r}")
        sm0 = have[0].signal_model[name]
        if "common" in name:
            n = _n_modes(sm0)
            f = np.asarray(sm0["f"], float)
            amp = np.sqrt(np.asarray(sm0["psd"], float) * _df(f))[:n]
            f = f[:n]
            L = batch_factor(orf_matrix(self.psrs, sm0["orf"], sm0.get("hmap")))
            self.add_signal(name, 1, f, amp, idx=float(sm0["idx"]), L=L)
            return
        nm = max(_n_modes(p.signal_model[name]) for p in have)
        f = np.zeros((P, nm))
        amp = np.zeros((P, nm))
        mask = None
        for i, p in enumerate(self.psrs):
            if name in p.signal_model:
                sm = p.signal_model[name]
                n = _n_modes(sm)
                fi = np.asarray(sm["f"], float)
                amp[i, :n] = np.sqrt(np.asarray(sm["psd"], float) * _df(fi))[:n]
                fi = fi[:n]
                f[i, :n] = fi
                if len(fi) < nm:  # continue the grid with zero-amplitude modes
                    step = fi[0] if len(fi) else 1.0
                    f[i, len(fi):] = fi[-1] + step * np.arange(1, nm - len(fi) + 1)
            else:
                f[i] = np.arange(1, nm + 1) / max(np.ptp(p.toas), 1.0)
        idx = float(sm0["idx"])
        if "system_noise" in name:
            backend = name.split("system_noise_")[1]
            mask = np.concatenate([p.backend_flags == backend for p in self.psrs]).astype(np.uint8)
            idx = 0.0
        self.add_signal(name, 0, f, amp, idx=idx, mask=mask)

    def add_signal(self, name, kind, f, amp, idx=0.0, freqf=1400.0, L=None, mask=None):
        """Add one GP: kind 0 per-pulsar (f, amp [P, N]) or kind 1 common (f, amp [N], L [P, P])."""
        sid = self.ctx.batch_add_signal(kind, f, amp, idx=idx, freqf=freqf, L=L, mask=mask)
        self.segments.append(dict(name=name, kind=kind, f=np.asarray(f, float), amp=np.asarray(amp, float),
                                  idx=float(idx), freqf=float(freqf), L=L, mask=mask, id=sid))
        return sid

    def _set_white(self, white, ecorr):
        sigma = np.concatenate([p._white_sigma2() ** 0.5 for p in self.psrs]) if white else None
        blocks, esig = [], []
        if ecorr:
            for i, p in enumerate(self.psrs):
                for b in p.backends:
                    key = f"{p.name}_{b}_log10_ecorr"
                    if key not in p.noisedict:
                        continue
                    for q in p.ecorr_blocks(backends=[b]):
                        blocks.append(q + self.offs[i])
                        esig.append(10 ** p.noisedict[key])
        self.sigma = sigma
        self.blocks = blocks
        self.ecorr_sigma = np.array(esig)
        self.ctx.batch_set_white(sigma, blocks if blocks else None, self.ecorr_sigma if blocks else None)

    # ------------------------------------------------------------------ running
    @property
    def n_toa(self):
        return int(self.offs[-1])

    def synth(self, n_real, seed=0, real0=0, to_host=True, coeffs=False, fit=False, spectra=None):
        """Realizations real0 .. real0+n_real-1: returns [n_real, n_toa] (host) or None (device only). fit=True removes
        the timing-model fit (set_timing_model) from the block on the device before the download: the returned array
        and the resident block are post-fit.

        spectra: None, or {signal name: dict(psd=...) | dict(amp=...) | dict(log10_A=..., gamma=...)} with one row per
        realization of this block (fakepta_amd.spectra.spectrum_tables has the shapes): realization real0 + r is drawn
        from row r's spectrum, with the Philox draws and the operation order of the fixed-spectrum block, so a row
        equal to the layout's amplitudes gives that block bit for bit. Signals that are not named keep the layout's
        spectrum, and the layout itself is not modified: the next plain synth() is unchanged, and
        set_optimal_statistic, set_likelihood_grid and the other consumers keep the layout's values as their noise
        model whatever spectrum a block was drawn from."""
        def run(to_host):
            if spectra is None:
                return self.ctx.batch_synth(seed, real0, n_real, to_host=to_host, coeffs=coeffs)
            from . import spectra as _spectra
            seg, form, per, tables = _spectra.spectrum_tables(self, spectra, n_real)
            return self.ctx.batch_synth_spectra(seed, real0, n_real, seg, form, per, tables, to_host=to_host,
                                                coeffs=coeffs)
        if not fit:
            return run(to_host)
        if not self._has_tm:
            raise ValueError("synth(fit=True): no timing model is set; call set_timing_model() first")
        got = run(False)
        self.ctx.batch_project()
        out = self.ctx.batch_download(0, n_real) if to_host else None
        return (out, got[1]) if coeffs else out

    def set_timing_model(self, Mmats=None, weights="white", rcond=None):
        """Set the timing model that project() and synth(fit=True) remove from a block: for every pulsar the weighted
        least-squares fit r - M (M^T W M)^+ M^T W r of its design matrix. Returns the ranks [P].

        Mmats:   list of per-pulsar design matrices [n_p, m_p <= 16] (default: each pulsar's Mmat); an empty list or
                 matrices without columns clear the model.
        weights: "white" (default) 1 / (EFAC^2 toaerr^2 + EQUAD^2) from each pulsar's noisedict, None for unit
                 weights, or an array [n_toa] (or a list of per-pulsar arrays).
        rcond:   a column whose orthogonalised norm is <= rcond of its own norm is dropped (default 1e-10).

        The weights are diagonal: ECORR is not part of them, and a generalised least-squares fit against a dense
        covariance is out of scope."""
        # this call's own defaults: None is each pulsar's Mmat, an empty list no column at all
        Mmats = "tm" if Mmats is None else list(Mmats) or None
        M, ncol = _tm.design_of(self.psrs, Mmats, "set_timing_model")
        w = _tm.weights_of(self.psrs, weights, self.n_toa)
        self._has_tm = False
        rank = self.ctx.batch_set_timing_model(M, ncol_psr=ncol, weights=w, rcond=rcond)
        self._has_tm = M.shape[1] > 0
        return rank

    def project(self):
        """Remove the timing-model fit from the last block, in place on the device: checksums(), correlations(),
        hd_curve() and downloads afterwards see post-fit residuals. The next synth() is not affected."""
        self.ctx.batch_project()

    # ------------------------------------------------------------------ continuous waves
    def add_cgw(self, sources, sign=1.0, p_dist=None):
        """Add continuous waves of circular binaries (fakepta_amd.cw, the signal of Pulsar.add_cgw) to every
        realization of the last block, in place on the device: downloads, checksums(), correlations(), hd_curve(),
        project() and fourier_fit() afterwards see the block with the waves. The next synth() is not affected.

        sources: one table for every realization ([S, 9] rows of cw.COLUMNS, or a dict keyed by Pulsar.add_cgw's
                 argument names), or one population per realization: an [R, S, 9] array or a list of R tables
                 [S_r, 9] (cw.population_tables); a table may be empty.
        sign:    -1.0 takes the same waves out again (to rounding).
        p_dist:  None: every pulsar at L = light_seconds(p.pdist). An array [P] or [R, P]: L =
                 light_seconds(p.pdist, p_dist), the distance draws (in units of the distance's sigma) of a pulsar-term
                 study, one per pulsar or one per (realization, pulsar).

        Every pulsar needs pos and pdist. A bad source (named by realization and index) or a missing block raises the
        library's error and leaves the block as it was."""
        from . import cw as _cw
        P = len(self.psrs)
        try:
            pos = np.array([np.asarray(p.pos, dtype=np.float64) for p in self.psrs]).reshape(P, 3)
            pdist = [p.pdist for p in self.psrs]
        except AttributeError as e:
            raise ValueError(f"add_cgw: every pulsar needs pos and pdist ({e})") from None
        _, _, R = self.ctx.batch_device_out()  # the library's state error without a block
        n_tab, src_offs, src = _cw.population_tables(sources, R)
        if p_dist is None:
            L = np.array([_cw.light_seconds(d) for d in pdist], dtype=np.float64)
        else:
            p_dist = np.asarray(p_dist, dtype=np.float64)
            if p_dist.shape not in ((P,), (R, P)):
                raise ValueError(f"add_cgw: p_dist must be [{P}] or [{R}, {P}], got {p_dist.shape}")
            L = np.stack([np.broadcast_to(_cw.light_seconds(d, p_dist[..., i]), p_dist.shape[:-1])
                          for i, d in enumerate(pdist)], axis=-1)
        self.ctx.batch_cw_accumulate(pos, L, n_tab, src_offs, src, sign=sign)

    # ------------------------------------------------------------------ ephemeris errors
    def add_roemer_delay(self, perturbations, sign=1.0, ephem=None):
        """Add the Roemer delays of solar-system-ephemeris errors (fakepta_amd.ephem, the signal of
        correlated_noises.add_roemer_delay) to every realization of the last block, in place on the device: downloads,
        checksums(), correlations(), hd_curve(), project(), fourier_fit(), optimal_statistic() and likelihood_grid()
        afterwards see the block with the delays. The next synth() is not affected.

        perturbations: one table for every realization (an [n, 22] array of ephem.ROW_COLUMNS rows, or a list of
                 (planet, deviations) as add_roemer_delay_array takes), or one table per realization: an [R, n, 22]
                 array or a list of R tables of either form (ephem.perturbation_tables); a table may be empty.
        sign:    -1.0 takes the same delays out again (to rounding).
        ephem:   the Ephemeris that resolves planets given by name; default the native one every pulsar shares.
                 Tables of rows need none.

        Every pulsar needs pos. A bad row (named by realization and index) or a missing block raises the library's
        error and leaves the block as it was. Realization r gets what add_roemer_delay_array adds for its table. In a
        sharded run the injection goes into the consumer:
            simulate_sharded(sim, n_real, on_batch=lambda sim, first, n: (sim.add_roemer_delay(pert[first:first + n]),
                                                                           sim.project()))"""
        from . import ephem as _ephem
        from fakepta.correlated_noises import _native_ephem
        P = len(self.psrs)
        try:
            pos = np.array([np.asarray(p.pos, dtype=np.float64) for p in self.psrs]).reshape(P, 3)
        except AttributeError as e:
            raise ValueError(f"add_roemer_delay: every pulsar needs pos ({e})") from None
        _, _, R = self.ctx.batch_device_out()  # the library's state error without a block
        if ephem is None and all(hasattr(p, "ephem") for p in self.psrs):
            ephem = _native_ephem(self.psrs)
        n_tab, row_offs, rows = _ephem.perturbation_tables(perturbations, R, ephem=ephem)
        self.ctx.batch_roemer_accumulate(pos, n_tab, row_offs, rows, sign=sign)

    # ------------------------------------------------------------------ Fourier fit
    def set_fourier_fit(self, components=None, Mmats="tm", weights="white", rcond=None, common=None):
        """Set the Fourier fit that fourier_fit(), power_spectrum(), cross_spectrum() and hd_curve(domain="fourier")
        apply to a block: for every pulsar the joint weighted least squares of a nuisance design and Fourier columns,
        of which the Fourier amplitudes come back. Returns (kept Fourier columns [P], kept mask [P, K]).

        components: a list of 1 .. 4 entries, each a signal name of this layout (its f and idx), (n_modes, idx) for
                 the grid k / Tspan of the array, or (f, idx) with f [N] or [P, N]. Default: one achromatic component
                 of 30 modes at k / Tspan. A component's columns are (freqf / nu)^idx cos(2 pi f_k t), k = 0 .. N - 1,
                 then the sines: the order of signal_model[...]['fourier'].
        Mmats:   "tm" (default) marginalises each pulsar's Mmat, None nothing, or a list of per-pulsar matrices
                 [n_p, m_p <= 16].
        weights: as set_timing_model. rcond: a column whose orthogonalised norm is <= rcond is dropped, its
                 coefficient 0 (default 1e-10).
        common:  None keeps one frequency grid for the array when every component has one; True insists on it;
                 False gives every pulsar its own copy (cross_spectrum() then refuses)."""
        tspan = float(np.ptp(self.toas)) if len(self.toas) else 0.0
        n_modes, f, idx, freqf = _fit.resolve_components(components, len(self.psrs), tspan, self.segments, common)
        M, ncol = _tm.design_of(self.psrs, Mmats, "set_fourier_fit")
        w = _tm.weights_of(self.psrs, weights, self.n_toa)
        self._fit = None
        rank, kept = self.ctx.batch_set_fit(n_modes, f, idx, freqf, M=M, ncol_psr=ncol, weights=w, rcond=rcond)
        self._fit = dict(n_modes=n_modes, f=f, idx=idx, freqf=freqf, common=f.ndim == 1)
        return rank, kept

    def _need_fit(self, what):
        if self._fit is None:
            raise ValueError(f"{what}: no Fourier fit is set; call set_fourier_fit() first")
        return self._fit

    def fourier_fit(self, to_host=True):
        """The Fourier coefficients of the last block, [P, K, R] in the units of the residuals (None with
        to_host=False: the result stays on the device for cross_spectrum()). The block is untouched."""
        fit = self._need_fit("fourier_fit")
        return self.ctx.batch_fit(2 * int(fit["n_modes"].sum()), to_host=to_host)

    def power_spectrum(self):
        """Per component [P, N_c]: the mean over the last block's realizations of (a_cos^2 + a_sin^2) / (2 df), df =
        diff(append(0, f)): the units of signal_model[...]['psd'], so it compares with spectrum.powerlaw directly."""
        fit = self._need_fit("power_spectrum")
        return _fit.power_spectrum(self.fourier_fit(), fit["n_modes"], fit["f"])

    def cross_spectrum(self, psd=True):
        """[sum N_c, P, P]: per mode the mean over the last block's realizations of a_cos^a a_cos^b + a_sin^a a_sin^b,
        divided by 2 df (power_spectrum's units; its diagonal is power_spectrum()) unless psd=False. Fitted and
        contracted on the device; a common frequency grid only."""
        fit = self._need_fit("cross_spectrum")
        if not fit["common"]:
            raise ValueError("cross_spectrum: the fit has per-pulsar frequencies; a common grid is needed")
        self.ctx.batch_fit(2 * int(fit["n_modes"].sum()), to_host=False)
        _, _, R = self.ctx.batch_device_out()
        X = self.ctx.batch_fit_cross(int(fit["n_modes"].sum())) / R
        return X / (2.0 * _fit.mode_delta_f(fit["n_modes"], fit["f"]))[:, None, None] if psd else X

    # ------------------------------------------------------------------ optimal statistic
    def set_optimal_statistic(self, target=None, orfs=("hd",), bins=None, template=None, noise="layout", Mmats="tm",
                              weights="white", rcond=None):
        """Set the optimal statistic that optimal_statistic() applies to a block: per realization the noise-weighted
        cross-correlation of every pulsar pair (X_a^T phi_hat X_b with X_p = F_p^T P_p^-1 r_p, the definition of
        include/fakepta_amd.h) against the pair weights of ORFs and angular bins. Returns (kept design columns [P],
        N_ab [P, P]).

        target:   the common process: a signal name of the noise model or its index; None picks the layout's only
                  common signal (ValueError with none or several).
        orfs:     names fakepta's orf_matrix knows ("hd", "monopole", "dipole", "curn") or explicit [P, P] arrays.
        bins:     None, or a number of angular bins (open, edges linspace(0, pi, bins + 1), as hd_curve).
        template: phi_hat [N]; default the target's own amp^2, so A2 is in units of the injected power.
        noise:    "layout": every signal of this layout (f, amp^2, idx, mask) makes P_p; or a list of such segments.
        Mmats, weights, rcond: as set_fourier_fit; the design is marginalised with infinite variance, so project()
                  before optimal_statistic() changes nothing but rounding.

        The weights are diagonal: ECORR is not part of them."""
        segs = self.segments if isinstance(noise, str) and noise == "layout" else noise
        if isinstance(segs, str):
            raise ValueError(f"set_optimal_statistic: noise must be 'layout' or a list of segments, got {noise!r}")
        t = _os.pick_target(segs, target)
        model = _os.noise_model(segs, len(self.psrs))
        phi_hat = _os.template_of(model, t, template)
        G, n_orf, centres, counts = _os.pair_matrices(self.psrs, orfs, bins)
        M, ncol = _os.design_of(self.psrs, Mmats, "set_optimal_statistic")
        w = _tm.weights_of(self.psrs, weights, self.n_toa)
        self._os = None
        self._scr = None  # the library clears the scrambles with the statistic they belong to
        rank, nab = self.ctx.batch_set_os(model["n_modes"], model["f"], model["idx"], model["freqf"], model["phi"], t,
                                          phi_hat, G, masks=model["masks"], M=M, ncol_psr=ncol, weights=w, rcond=rcond)
        self._os = dict(G=G, nab=nab, n_orf=n_orf, centres=centres, counts=counts, target=t, template=phi_hat)
        return rank, nab

    def optimal_statistic(self, per_mode=False):
        """The optimal statistic of every realization of the last block, computed on the device; the block is
        untouched. A dict: A2 and snr [n_orf, R] (each ORF on its own), A2_joint [n_orf, R] when more than one ORF is
        set (the joint fit C A = Q), rho_bins [bins, R] with bin_centres and bin_counts (NaN for a bin without pairs),
        Q [J, R] and norm [J] (the raw device numbers and their denominators, ORFs first, then bins), and Q_mode
        [J, N, R] with per_mode=True. Per batch of a sharded job: simulate_sharded(..., on_batch=lambda sim, first, n:
        ...sim.optimal_statistic()...)."""
        if getattr(self, "_os", None) is None:
            raise ValueError("optimal_statistic: no optimal statistic is set; call set_optimal_statistic() first")
        o = self._os
        Q, Qm, _ = self.ctx.batch_os(per_mode=per_mode)
        return _os.derive(Q, o["G"], o["nab"], o["n_orf"], o["centres"], o["counts"], Qm)

    def set_sky_scrambles(self, n=1000, seed=0, max_match=0.1, positions=None, matrices=None):
        """Set the sky scrambles that sky_scrambles() ranks the optimal statistic against (after
        set_optimal_statistic, which also clears them; fpta_batch_set_os_scrambles). By default n fictitious skies from
        fakepta_amd.os.sky_scrambles(seed=seed) whose Hellings-Downs matrices have |match| <= max_match with the first
        ORF of the statistic; or positions [J, P, 3] (unit vectors), or explicit symmetric matrices [J, P, P] (any
        other ORF scrambled by the caller). n = 0 clears them. Returns (match [J, n_orf], norm [J]): the match with
        every ORF of the statistic and the denominators sum_{a<b} G_j^2 N_ab."""
        o = getattr(self, "_os", None)
        if o is None:
            raise ValueError("set_sky_scrambles: no optimal statistic is set; call set_optimal_statistic() first")
        if positions is not None and matrices is not None:
            raise ValueError("set_sky_scrambles: give positions or matrices, not both")
        if positions is None and matrices is None:
            if int(n) == 0:
                self.ctx.batch_set_os_scrambles()
                self._scr = None
                return np.zeros((0, o["n_orf"])), np.zeros(0)
            positions, _ = _os.sky_scrambles(self.ctx, self.psrs, n, seed=seed, max_match=max_match, ref=o["G"][:1])
        # a refused call leaves the library's scrambles, and this record of them, as they were
        norm, match = self.ctx.batch_set_os_scrambles(pos=positions, G=matrices)
        self._scr = dict(J=len(norm), positions=None if positions is None else np.asarray(positions, dtype=np.float64))
        return match[:, :o["n_orf"]], norm

    def sky_scrambles(self, full=False):
        """The sky-scramble significance of the optimal statistic of every realization of the last block, computed on
        the device; the block is untouched. A dict: p_value = (1 + count_ge) / (1 + J), snr and count_ge [n_orf, R]
        (the observed S/N of each ORF and the scrambles at or above it), null_mean, null_std and null_max [R] of the
        scrambled S/N, and snr_null [J, R] with full=True. Per batch of a sharded job: simulate_sharded(...,
        on_batch=lambda sim, first, n: ...sim.sky_scrambles()["p_value"]...)."""
        o = getattr(self, "_os", None)
        if o is None:
            raise ValueError("sky_scrambles: no optimal statistic is set; call set_optimal_statistic() first")
        got = self.ctx.batch_os_scrambles(full=full)
        J = self.ctx.batch_os_scrambles_info()["n_scr"]
        return _os.derive_scrambles(got["snr_obs"], got["count_ge"], J, got["mean"], got["std"], got["max"],
                                    o["n_orf"], got["snr_null"])

    def set_optimal_statistic_spectra(self, vary, target=None, orfs=("hd",), bins=None, template=None, noise="layout",
                                      Mmats="tm", weights="white", rcond=None):
        """Set the optimal statistic that optimal_statistic_spectra() applies to a block under a noise spectrum per
        realization (fpta_batch_set_os_spectra): the statistic of set_optimal_statistic, with the prior variances of
        the signals in `vary` taken per realization from the spectra of the call, the tables of synth(spectra=...).
        Returns the kept design columns [P].

        vary:    signal names of this layout (at most 4, at most 128 Fourier columns together); the target is added
                 when it is not named. Every other signal of the noise model keeps its values for every realization.
        The other arguments are set_optimal_statistic's. Independent of set_optimal_statistic, the timing model and
        the Fourier fit: all can be set together."""
        segs = self.segments if isinstance(noise, str) and noise == "layout" else noise
        if isinstance(segs, str):
            raise ValueError(f"set_optimal_statistic_spectra: noise must be 'layout' or a list of segments, got "
                             f"{noise!r}")
        segs = list(segs)
        t = _os.pick_target(segs, target)
        vary = [vary] if isinstance(vary, str) else list(vary)
        comp, sid = [], []
        for name in vary + [segs[t].get("name")]:
            hit = [i for i, s in enumerate(segs) if s.get("name") == name]
            lay = [s for s in self.segments if s["name"] == name]
            if len(hit) != 1 or len(lay) != 1:
                raise ValueError(f"set_optimal_statistic_spectra: {name!r} must name one signal of the layout and of "
                                 f"the noise model (the layout has {[s['name'] for s in self.segments]})")
            if hit[0] not in comp:
                comp.append(hit[0])
                sid.append(lay[0]["id"])
        k = comp.index(t)  # the target last
        comp.append(comp.pop(k))
        sid.append(sid.pop(k))
        if len(comp) > _capi.OSS_MAX_VARY:
            raise ValueError(f"set_optimal_statistic_spectra: {len(comp)} varied signals, more than "
                             f"{_capi.OSS_MAX_VARY}")
        model = _os.noise_model(segs, len(self.psrs))
        q = 2 * int(sum(model["n_modes"][c] for c in comp))
        if q > _capi.OSS_MAX_COL:
            raise ValueError(f"set_optimal_statistic_spectra: the varied signals have {q} Fourier columns, more than "
                             f"{_capi.OSS_MAX_COL}")
        phi_hat = _os.template_of(model, t, template)
        G, n_orf, centres, counts = _os.pair_matrices(self.psrs, orfs, bins)
        M, ncol = _os.design_of(self.psrs, Mmats, "set_optimal_statistic_spectra")
        w = _tm.weights_of(self.psrs, weights, self.n_toa)
        # a refused call leaves the library's statistic, and this record of it, as they were
        rank = self.ctx.batch_set_os_spectra(model["n_modes"], model["f"], model["idx"], model["freqf"], model["phi"],
                                             t, phi_hat, comp, sid, G, n_orf, masks=model["masks"], M=M, ncol_psr=ncol,
                                             weights=w, rcond=rcond)
        self._oss = dict(G=G, n_orf=n_orf, centres=centres, counts=counts, target=t, template=phi_hat, seg=sid,
                         names=[segs[c].get("name") for c in comp], K=2 * len(phi_hat))
        return rank

    def optimal_statistic_spectra(self, spectra=None, per_mode=False, pair_norms=False):
        """The optimal statistic of every realization of the last block, each under its own noise spectrum; the block
        is untouched. spectra: the dict synth(spectra=...) takes (spectra.spectrum_tables), one row per realization of
        the block, for signals of the varied set only (ValueError naming any other); a varied signal without an entry
        takes the layout's values, None the layout's for every row. A dict: A2, snr and A2_joint [n_orf, R] (the
        joint fit solved per realization), rho_bins [bins, R], bin_centres, bin_counts, Q [J, R], norm [J, R] and joint
        [n_orf, n_orf, R] (the per-realization denominators), Q_mode [J, N, R] with per_mode=True and N_ab [R, P, P]
        with pair_norms=True. An ORF or bin whose denominator is 0 in a realization is NaN there. Per batch of a
        sharded job: on_batch=lambda sim, first, n: sim.optimal_statistic_spectra(slice_spectra(spectra, first, n))."""
        o = getattr(self, "_oss", None)
        if o is None:
            raise ValueError("optimal_statistic_spectra: no statistic is set; call set_optimal_statistic_spectra() "
                             "first")
        seg, form, per, tables = [], [], [], []
        if spectra:
            from . import spectra as _spectra
            _, _, R = self.ctx.batch_device_out()  # the library's state error without a block
            seg, form, per, tables = _spectra.spectrum_tables(self, spectra, R)
            for s in seg:
                if s not in o["seg"]:
                    name = next(g["name"] for g in self.segments if g["id"] == s)
                    raise ValueError(f"optimal_statistic_spectra: spectra[{name!r}]: the signal is not in the varied "
                                     f"set {o['names']}")
        got = self.ctx.batch_os_spectra(seg, form, per, tables, o["K"], len(o["G"]), o["n_orf"], per_mode=per_mode,
                                        pair_norms=pair_norms)
        return _os.derive_per_realization(got["Q"], got["norm"], got["joint"], o["n_orf"], o["centres"], o["counts"],
                                          got["Q_mode"], got["N_ab"])

    # ------------------------------------------------------------------ likelihood grid
    def set_likelihood_grid(self, target=None, phi=None, log10_A=None, gamma=None, noise="layout", Mmats="tm",
                            weights="white", rcond=None):
        """Set the spectrum grid that likelihood_grid() applies to a block: per realization and grid point the Gaussian
        log-likelihood ratio ln p(r | phi_g) - ln p(r | phi = 0) of the target process with the timing model
        marginalised (the definition of include/fakepta_amd.h). Returns the kept design columns [P].

        target:   a signal name of the noise model or its index; None picks the layout's only common signal
                  (ValueError with none or several). Its own spectrum is not part of the base model: the grid replaces
                  it. A common target is taken as uncorrelated between pulsars; a per-pulsar target gets the same
                  spectrum for every pulsar.
        phi:      the grid [G, N], the target's prior variance per grid point and mode (>= 0), or
        log10_A, gamma: the axes of a power-law grid, phi = spectrum.powerlaw(f, A, gamma) * delta f, amplitude slowest.
        noise:    "layout": every signal of this layout (f, amp^2, idx, mask); or a list of such segments. The other
                  components stay at these values.
        Mmats, weights, rcond: as set_fourier_fit; project() before likelihood_grid() changes nothing but rounding.

        The weights are diagonal: ECORR is not part of them."""
        segs = self.segments if isinstance(noise, str) and noise == "layout" else noise
        if isinstance(segs, str):
            raise ValueError(f"set_likelihood_grid: noise must be 'layout' or a list of segments, got {noise!r}")
        t = _os.pick_target(segs, target)
        model = _os.noise_model(segs, len(self.psrs))
        grid, axes = _lnl.make_grid(_lnl.target_frequencies(model, t), phi, log10_A, gamma)
        M, ncol = _os.design_of(self.psrs, Mmats, "set_likelihood_grid")
        w = _tm.weights_of(self.psrs, weights, self.n_toa)
        self._lnl = None
        rank, ld = self.ctx.batch_set_lnl(model["n_modes"], model["f"], model["idx"], model["freqf"], model["phi"], t,
                                          grid, masks=model["masks"], M=M, ncol_psr=ncol, weights=w, rcond=rcond)
        self._lnl = dict(phi=grid, axes=axes, ld=ld, target=t)
        return rank

    def likelihood_grid(self, per_pulsar=False, posterior=False):
        """The likelihood grid of every realization of the last block, computed on the device; the block is untouched.
        A dict: dlnL [G, R] (or [nA, ngamma, R] for a grid built from axes), argmax (the maximum-likelihood grid point
        per realization; with axes a tuple of index arrays, and log10_A_ml, gamma_ml [R]), lnB [R] = logsumexp_g(dlnL)
        - ln G (the evidence ratio against "no process" under a uniform prior over the grid points), the axes log10_A
        and gamma (None for an explicit grid), the normalised posterior with posterior=True, and q_psr, dlnL_psr
        [P, G, R] with per_pulsar=True. Per batch of a sharded job: simulate_sharded(..., on_batch=lambda sim, first, n:
        ...sim.likelihood_grid()...)."""
        if getattr(self, "_lnl", None) is None:
            raise ValueError("likelihood_grid: no likelihood grid is set; call set_likelihood_grid() first")
        o = self._lnl
        d, q, _ = self.ctx.batch_lnl(per_pulsar=per_pulsar)
        return _lnl.derive(d, o["axes"], o["ld"], q, posterior)

    # ------------------------------------------------------------------ correlated likelihood grid
    def set_correlated_likelihood(self, target=None, orfs=("hd", "curn"), phi=None, log10_A=None, gamma=None,
                                  noise="layout", Mmats="tm", weights="white", rcond=None):
        """Set the ORFs and the spectrum grid that correlated_likelihood() applies to a block: per realization, ORF and
        grid point ln p(r | Gamma_o, phi_g) - ln p(r | phi = 0) of the target process with the prior cov(a_pk, a_ql) =
        Gamma_pq phi_k delta_kl coupling the pulsars and the timing model marginalised (the definition of
        include/fakepta_amd.h). The device factors the coupled P K system once per (ORF, grid point) here and keeps the
        factors (8 n_orf G (P K)^2 bytes, at most 32 GiB); a block then costs one triangular solve each. Returns the
        kept design columns [P].

        target:   as set_likelihood_grid; it needs one frequency grid for the whole array.
        orfs:     names fakepta's orf_matrix knows ("hd", "monopole", "dipole", "curn") or explicit [P, P] arrays,
                  symmetric positive semidefinite (ValueError otherwise); singular ORFs are fine.
        phi, log10_A, gamma, noise, Mmats, weights, rcond: as set_likelihood_grid.

        The weights are diagonal: ECORR is not part of them."""
        segs = self.segments if isinstance(noise, str) and noise == "layout" else noise
        if isinstance(segs, str):
            raise ValueError(f"set_correlated_likelihood: noise must be 'layout' or a list of segments, got {noise!r}")
        t = _os.pick_target(segs, target)
        model = _os.noise_model(segs, len(self.psrs))
        grid, axes = _lnl.make_grid(_lnl.target_frequencies(model, t), phi, log10_A, gamma)
        names, _, A = _clnl.orf_factors(self.psrs, orfs, "set_correlated_likelihood")
        M, ncol = _os.design_of(self.psrs, Mmats, "set_correlated_likelihood")
        w = _tm.weights_of(self.psrs, weights, self.n_toa)
        self._clnl = None
        rank, ld = self.ctx.batch_set_clnl(model["n_modes"], model["f"], model["idx"], model["freqf"], model["phi"], t,
                                           grid, A, masks=model["masks"], M=M, ncol_psr=ncol, weights=w, rcond=rcond)
        self._clnl = dict(phi=grid, axes=axes, ld=ld, names=names, target=t)
        return rank

    def correlated_likelihood(self, posterior=False):
        """The correlated likelihood grid of every realization of the last block, computed on the device; the block is
        untouched. A dict: dlnL [n_orf, G, R] (or [n_orf, nA, ngamma, R] for a grid built from axes), per ORF argmax
        (with axes a tuple of index arrays, and log10_A_ml, gamma_ml [n_orf, R]), lnB [n_orf, R] = logsumexp_g(dlnL) -
        ln G, lnB_vs_curn [n_orf, R] when "curn" is among the ORFs (the row of "hd" is the Hellings-Downs versus CURN
        Bayes factor under a uniform prior over the grid points), orfs (the names), the axes, and the normalised
        posterior with posterior=True. Per batch of a sharded job: simulate_sharded(..., on_batch=lambda sim, first, n:
        ...sim.correlated_likelihood()...)."""
        if getattr(self, "_clnl", None) is None:
            raise ValueError("correlated_likelihood: no correlated likelihood is set; call "
                             "set_correlated_likelihood() first")
        o = self._clnl
        d, _, _, _ = self.ctx.batch_clnl()
        return _clnl.derive(d, o["names"], o["axes"], o["ld"], posterior)

    # ------------------------------------------------------------------ continuous-wave F-statistics
    def set_fe_statistic(self, fgw, nside=None, sky=None, noise="layout", Mmats="tm", weights="white", rcond=None,
                         rcond_fe=None):
        """Set the continuous-wave detection statistics that fe_statistic() applies to a block: per realization the
        Earth-term Fe-statistic on a grid of sky directions and frequencies, Fe = N^T M^-1 N / 2 (2 Fe is chi^2 with 4
        degrees of freedom under the null), and the incoherent Fp-statistic per frequency (the definition of
        include/fakepta_amd.h; the antenna patterns are add_cgw's). Returns the kept design columns [P].

        fgw:      the gravitational-wave frequencies [G <= 256] in Hz, neither harmonics nor ordered.
        nside:    the directions are the pixel centres of a HEALPix RING map (12 nside^2 <= 12288), or
        sky:      an explicit array [n, 2] of (cos_gwtheta, gwphi), add_cgw's keywords.
        noise:    "layout": every signal of this layout (f, amp^2, idx, mask) makes P_p, a common process as each
                  pulsar's auto-term; or a list of such segments. A layout without a Gaussian process is white noise.
        Mmats, weights, rcond: as set_fourier_fit; the design is marginalised with infinite variance.
        rcond_fe: a (direction, frequency) whose scaled M has a Cholesky pivot <= rcond_fe (default 1e-10) is singular
                  and reads NaN.

        Every pulsar needs pos. The weights are diagonal: ECORR is not part of them. The pulsar term and an evolving
        frequency are not modelled."""
        segs = self.segments if isinstance(noise, str) and noise == "layout" else noise
        if isinstance(segs, str):
            raise ValueError(f"set_fe_statistic: noise must be 'layout' or a list of segments, got {noise!r}")
        fgw, sky = _fe.check_frequencies(fgw), _fe.sky_grid(nside, sky)
        model = _fe.model_of(segs, len(self.psrs))
        pos = _fe.positions_of(self.psrs, "set_fe_statistic")
        M, ncol = _os.design_of(self.psrs, Mmats, "set_fe_statistic")
        w = _tm.weights_of(self.psrs, weights, self.n_toa)
        self._fe = None
        rank, tab = self.ctx.batch_set_fe(model["n_modes"], model["f"], model["idx"], model["freqf"], model["phi"], fgw,
                                          sky, pos, masks=model["masks"], M=M, ncol_psr=ncol, weights=w, rcond=rcond,
                                          rcond_fe=rcond_fe, tables=True)
        self._fe = dict(fgw=fgw, sky=sky, n_eff=tab["n_eff"])
        return rank

    def fe_statistic(self, per_frequency=True, full=False):
        """The F-statistics of every realization of the last block, computed on the device; the block is untouched. A
        dict: Fe_max [R] with argmax [2, R] (direction, frequency; -1 where every point is singular) and
        cos_gwtheta_ml, gwphi_ml, fgw_ml [R]; Fe_f and argmax_f [G, R] (the maximum over the directions per frequency;
        None with per_frequency=False); Fp [G, R] with n_eff [G] (2 Fp is chi^2 with 2 n_eff degrees of freedom); Fe
        [n_sky, G, R], the whole map, with full=True; fap_max = fe.false_alarm(Fe_max); the grids fgw and sky. Per batch
        of a sharded job: simulate_sharded(..., on_batch=lambda sim, first, n: (sim.add_cgw(src),
        ...sim.fe_statistic()...))."""
        if getattr(self, "_fe", None) is None:
            raise ValueError("fe_statistic: no F-statistic is set; call set_fe_statistic() first")
        o = self._fe
        out = _fe.derive(self.ctx.batch_fe(per_frequency=per_frequency, full=full), o["fgw"], o["sky"])
        out["n_eff"] = o["n_eff"]
        return out

    def synth_from_z(self, z):
        """Validation mode: z [n_real, n_seg, P, N_max, 2] standard normals (cos, sin)."""
        return self.ctx.batch_synth_from_z(z)

    def correlations(self, normalized=True):
        """Mean over the last block's realizations of the zero-lag cross-correlation matrix
        dot(res_a, res_b)/n (correlated_noises.py:14-19), normalized per realization by the
        auto-correlations if `normalized`. Computed on device; pulsars must share the TOA count."""
        _, _, R = self.ctx.batch_device_out()
        return self.ctx.batch_correlations(2 if normalized else 1) / R

    def hd_curve(self, bins=10, estimator="ratio", return_counts=False, domain="time"):
        """(mean, std, bin centres) of the pairwise correlations against angular separation
        (correlated_noises.py:21-47) for the last block. estimator "ratio": mean cross-power over
        sqrt(mean auto-powers) (consistent); "per_realization": mean of per-realization normalized
        correlations (biased toward 0 by O(1/n_eff) for red processes). A bin with no pulsar pair is NaN,
        as the reference's bin_curve gives, but without NumPy's empty-slice warnings; return_counts=True
        appends the number of pairs per bin so callers can mask the empty ones. domain "fourier" (estimator "ratio"
        only) takes the correlations from the Fourier fit (set_fourier_fit) instead of the zero-lag dot product: S =
        the sum over modes of cross_spectrum(psd=False), binned as S[a][b] / sqrt(S[a][a] S[b][b]); it needs no
        common TOA count, so it works for ragged arrays."""
        if domain not in ("time", "fourier"):
            raise ValueError(f"hd_curve: domain must be 'time' or 'fourier', got {domain!r}")
        if domain == "fourier":
            if estimator != "ratio":
                raise ValueError("hd_curve: domain 'fourier' has the 'ratio' estimator only")
            S = self.cross_spectrum(psd=False).sum(axis=0)
            d = np.sqrt(np.diag(S))
            C = S / np.outer(d, d)
        elif estimator == "ratio":
            C = self.correlations(normalized=False)
            d = np.sqrt(np.diag(C))
            C = C / np.outer(d, d)
        else:
            C = self.correlations(normalized=True)
        pos = np.array([p.pos for p in self.psrs])
        iu = np.triu_indices(len(self.psrs), 1)
        angles = np.arccos(np.clip(pos @ pos.T, -1.0, 1.0))[iu]
        corrs = C[iu]
        edges = np.linspace(0., np.pi, bins + 1)
        centres = edges[:-1] + 0.5 * (edges[1] - edges[0])
        mean, std, counts = np.full(bins, np.nan), np.full(bins, np.nan), np.zeros(bins, dtype=np.int64)
        for b, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
            sel = corrs[(angles > lo) & (angles < hi)]  # open bins, as correlated_noises.py:36-47
            counts[b] = len(sel)
            if len(sel):
                mean[b], std[b] = np.mean(sel), np.std(sel)
        return (mean, std, centres, counts) if return_counts else (mean, std, centres)

    def checksums(self):
        """Per-realization (sum, sum of squares) of the last block, computed on device."""
        return self.ctx.batch_checksums()

    def split(self, block):
        """[n_real, n_toa] -> list of per-pulsar [n_real, n_p] views."""
        return [block[..., self.offs[i]:self.offs[i + 1]] for i in range(len(self.psrs))]


def simulate_batch(psrs, n_real, seed=0, real0=0, signals=None, white=True, ecorr=False, device=None):
    """One-call convenience: [n_real, n_toa_total] residual realizations of the array's noise model."""
    return BatchSimulator(psrs, signals=signals, white=white, ecorr=ecorr, device=device).synth(
        n_real, seed=seed, real0=real0)


# ----------------------------------------------------------------------------- multi-GPU (one process per GPU)
def shard_bounds(n_real, rank, world):
    """Realizations [start, end) of rank `rank` of `world` for a job of n_real (rank g owns
    [g R / G, (g + 1) R / G)); contiguous, disjoint, covering, sizes differing by at most one."""
    return rank * n_real // world, (rank + 1) * n_real // world


class RealizationComm:
    """torch.distributed plumbing of a realization-sharded job: one process per rank launched by torchrun
    (WORLD_SIZE / RANK / LOCAL_RANK from the environment), backend "gloo" (CPU tests, rehearsals of several ranks
    on one card) or "nccl". GPU jobs use RcclComm instead: torch's "nccl" backend would bring torch's own HIP
    runtime and RCCL (ROCm 7.0) into a process whose kernels run on the library's (ROCm 7.2). The data path has no
    collective: only the timing barrier, a max-reduce of the elapsed time and the gather of per-realization
    checksums to rank 0 go through it."""

    def __init__(self, backend="nccl", world=None, rank=None, local_rank=None):
        import os
        self.world = int(os.environ.get("WORLD_SIZE", "1")) if world is None else int(world)
        self.rank = int(os.environ.get("RANK", "0")) if rank is None else int(rank)
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0")) if local_rank is None else int(local_rank)
        self.backend = backend
        self.dist = None
        if self.world > 1:
            import torch
            import torch.distributed as dist
            self.torch = torch
            if backend == "nccl":
                ndev = torch.cuda.device_count()
                torch.cuda.set_device(self.local_rank % max(ndev, 1))
                self.device = torch.device("cuda", torch.cuda.current_device())
            else:
                self.device = torch.device("cpu")
            if not dist.is_initialized():
                dist.init_process_group(backend=backend)
            self.dist = dist

    def barrier(self):
        if self.dist:
            self.dist.barrier()

    def max(self, x):
        """max over ranks of a float (the job time is the slowest rank's)."""
        if not self.dist:
            return float(x)
        t = self.torch.tensor([float(x)], dtype=self.torch.float64, device=self.device)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def gather_to_root(self, arr, rows_per_rank=None):
        """Rank 0 receives every rank's `arr` ([n_g, ...] float64; n_g may differ by rank) concatenated in
        rank order; other ranks get None. rows_per_rank: list of n_g (known to every rank); arrays are padded
        to the largest n_g for the collective and trimmed on rank 0."""
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        if not self.dist:
            return arr.copy()
        if rows_per_rank is None:
            rows_per_rank = [arr.shape[0]] * self.world
        n_max = max(rows_per_rank)
        pad = np.zeros((n_max,) + arr.shape[1:])
        pad[:arr.shape[0]] = arr
        t = self.torch.from_numpy(pad).to(self.device)
        bufs = [self.torch.empty_like(t) for _ in range(self.world)] if self.rank == 0 else None
        self.dist.gather(t, gather_list=bufs, dst=0)
        if self.rank != 0:
            return None
        return np.concatenate([b.cpu().numpy()[:n] for b, n in zip(bufs, rows_per_rank)])

    def close(self):
        if self.dist and self.dist.is_initialized():
            self.dist.destroy_process_group()
        self.dist = None


_RDZV_MAGIC = b"FPTA"


def _recv_exact(conn, n):
    buf = b""
    while len(buf) < n:
        chunk = conn.recv(n - len(buf))
        if not chunk:
            raise ConnectionError("rendezvous connection closed early")
        buf += chunk
    return buf


def _exchange_unique_id(rank, world, addr, port, make_id, timeout, n_bytes=None):
    """Rank 0 makes the RCCL unique id and serves it to ranks 1 .. world - 1 over one TCP socket at (addr, port);
    the other ranks connect (retrying until `timeout`) and read its bytes. Plain sockets: no torch import, so the
    rank process maps one HIP runtime (the library's).

    Protocol: a rank sends b"FPTA" + its rank (uint32 little-endian), reads the id, answers b"A" and returns only once
    rank 0 has confirmed with b"K". Rank 0 counts a rank as served after reading its b"A" and sending b"K", and keeps
    accepting until every rank 1 .. world - 1 is served: a peer with a wrong magic or rank, or one that drops the
    connection before its acknowledgement, uses up no slot; a rank whose acknowledgement rank 0 did not read (timeout,
    reset) gets no confirmation, connects again and is served again. Either side raises TimeoutError past `timeout`
    seconds."""
    import socket
    import struct
    import time as _time
    n = _capi.COMM_ID_BYTES if n_bytes is None else int(n_bytes)
    deadline = _time.monotonic() + timeout
    if rank == 0:
        uid = make_id()
        if len(uid) != n:
            raise ValueError(f"unique id of {len(uid)} bytes, expected {n}")
        pending = set(range(1, world))
        with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as srv:
            srv.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
            srv.bind((addr, port))
            srv.listen(max(world, 8))
            while pending:
                left = deadline - _time.monotonic()
                if left <= 0:
                    raise TimeoutError(f"rank 0: RCCL rendezvous at {addr}:{port}: ranks {sorted(pending)} did not "
                                       f"check in within {timeout} s")
                srv.settimeout(left)
                try:
                    conn, _ = srv.accept()
                except socket.timeout:
                    continue
                with conn:
                    try:
                        conn.settimeout(min(5.0, max(deadline - _time.monotonic(), 0.1)))
                        hello = _recv_exact(conn, 8)
                        peer = struct.unpack("<I", hello[4:])[0]
                        if hello[:4] != _RDZV_MAGIC or not 1 <= peer < world:
                            continue  # a stray or foreign connection: no slot used
                        conn.sendall(uid)
                        if _recv_exact(conn, 1) == b"A":
                            conn.sendall(b"K")
                            pending.discard(peer)
                    except OSError:
                        continue  # no confirmation sent: the peer connects again
        return uid
    hello = _RDZV_MAGIC + struct.pack("<I", rank)
    while True:
        try:
            with socket.create_connection((addr, port), timeout=5.0) as conn:
                conn.sendall(hello)
                buf = _recv_exact(conn, n)
                conn.sendall(b"A")
                if _recv_exact(conn, 1) == b"K":  # rank 0 recorded this rank
                    return buf
        except OSError:
            pass  # no rank 0 yet, or no confirmation: connect again
        if _time.monotonic() > deadline:
            raise TimeoutError(f"rank {rank}: no RCCL rendezvous at {addr}:{port} within {timeout} s")
        _time.sleep(0.2)


class RcclComm:
    """RCCL over xGMI for a realization-sharded job with one process per GPU, launched by
    torchrun (WORLD_SIZE / RANK / MASTER_ADDR / MASTER_PORT from the environment). The communicator is the
    library's own (fpta_comm_*: the system RCCL on the kernels' HIP runtime), on the rank's context and stream;
    torch is never imported, so each rank maps one HIP runtime. Rank 0's 128-byte unique id reaches the others
    over a TCP socket at (MASTER_ADDR, MASTER_PORT + 1) (torchrun's own store listens on MASTER_PORT;
    FAKEPTA_AMD_RDZV_PORT overrides). Same interface as RealizationComm: barrier, max, gather_to_root, close."""

    backend = "rccl"

    def __init__(self, ctx, world=None, rank=None, addr=None, port=None, timeout=120.0):
        import os
        self.world = int(os.environ.get("WORLD_SIZE", "1")) if world is None else int(world)
        self.rank = int(os.environ.get("RANK", "0")) if rank is None else int(rank)
        self.local_rank = ctx.device
        self.ctx = ctx
        addr = addr or os.environ.get("MASTER_ADDR", "127.0.0.1")
        if port is None:
            port = int(os.environ.get("FAKEPTA_AMD_RDZV_PORT", int(os.environ.get("MASTER_PORT", "29500")) + 1))
        uid = _exchange_unique_id(self.rank, self.world, addr, int(port), _capi.Comm.unique_id, timeout)
        self.comm = _capi.Comm(ctx, self.world, self.rank, uid)

    def barrier(self):
        self.comm.max(0.0)

    def max(self, x):
        """max over ranks of a float (the job time is the slowest rank's)."""
        return self.comm.max(x)

    def gather_to_root(self, arr, rows_per_rank=None):
        """As RealizationComm.gather_to_root: rank 0 gets every rank's rows in rank order (padded to the largest
        count for the collective, trimmed here), the other ranks None."""
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        if rows_per_rank is None:
            rows_per_rank = [arr.shape[0]] * self.world
        n_max = max(rows_per_rank)
        pad = np.zeros((n_max,) + arr.shape[1:])
        pad[:arr.shape[0]] = arr
        got = self.comm.gather(pad)
        if got is None:
            return None
        return np.concatenate([got[g, :n] for g, n in enumerate(rows_per_rank)])

    def close(self):
        if getattr(self, "comm", None) is not None:
            self.comm.close()
            self.comm = None


def simulate_sharded(sim, n_real, seed=0, real0=0, batch=4096, comm=None, on_batch=None, spectra=None):
    """Realizations real0 .. real0 + n_real - 1 of `sim`'s noise model over every rank of `comm`.

    Rank g of G synthesizes its shard [real0 + g n / G, real0 + (g + 1) n / G) (shard_bounds) in batches of
    <= `batch` realizations on its own GPU, keeps each batch resident on the device (on_batch(sim, first, n)
    may consume it there: correlations, downloads) and computes per-realization checksums on the device.
    Rank 0 receives all checksums, in global realization order: returns [n_real, 2] (sum, sum of squares)
    on rank 0 and None on the other ranks. TOAs, tables and the ORF factor are replicated (each rank builds
    its own BatchSimulator); realization r is bit-identical whatever G and `batch` are (Philox counters carry
    the global index), which tests/test_dist_gloo.py and tests/test_gpu_c3.py check.

    spectra: None, or the per-realization spectra of BatchSimulator.synth(spectra=...) for the whole job: a dict of
    arrays whose leading axis holds the n_real realizations (row g - real0 is realization g's), or a callable
    (first, n) -> such a dict for realizations first .. first + n - 1. Every batch takes its own rows, through the
    per-batch loop (the library's streamed job takes no tables), so a realization is the same whatever the batch size
    and the number of ranks.

    sim: BatchSimulator (or any object with synth(n, seed=, real0=, to_host=False) and checksums()).
    comm: RcclComm (GPU ranks) or RealizationComm (gloo; default: a single-rank job)."""
    comm = comm if comm is not None else RealizationComm(world=1, rank=0, local_rank=0)
    G = comm.world
    lo, hi = shard_bounds(n_real, comm.rank, G)
    sums = np.empty((hi - lo, 2))
    # checksums from the gridded interpolation's partial sums (FPTA_OPT_FUSE_CHECKSUMS): no second pass over
    # each resident block;
    # each rank's context's own settings are restored afterwards. The synthesis path is chosen once for the job
    # (FPTA_OPT_MFMA_MIN_REAL 1): a tail batch below the default threshold would otherwise take the direct path, and
    # its realizations would depend on the batch split and the number of ranks
    ctx = getattr(sim, "ctx", None)
    fuse = min_real = None
    if ctx is not None:
        from fakepta_amd import _capi
        fuse = ctx.get_option(_capi.OPT_FUSE_CHECKSUMS)
        min_real = ctx.get_option(_capi.OPT_MFMA_MIN_REAL)
        ctx.set_option(_capi.OPT_FUSE_CHECKSUMS, 1)
        ctx.set_option(_capi.OPT_MFMA_MIN_REAL, 1)
    try:
        looped = ctx is None or on_batch is not None or spectra is not None
        if not looped and hi > lo:
            # no per-batch consumer: the whole shard streams inside the library, batches back to back
            sums[:] = ctx.batch_synth_checksums(seed, real0 + lo, hi - lo, batch)
        for first in range(lo, hi, batch) if looped else ():
            n = min(batch, hi - first)
            if spectra is None:
                sim.synth(n, seed=seed, real0=real0 + first, to_host=False)
            else:
                from .spectra import slice_spectra
                part = spectra(real0 + first, n) if callable(spectra) else slice_spectra(spectra, first, n)
                sim.synth(n, seed=seed, real0=real0 + first, to_host=False, spectra=part)
            if on_batch is not None:
                on_batch(sim, real0 + first, n)
            sums[first - lo:first - lo + n] = sim.checksums()
    finally:
        if fuse is not None:
            ctx.set_option(_capi.OPT_FUSE_CHECKSUMS, fuse)
            ctx.set_option(_capi.OPT_MFMA_MIN_REAL, min_real)
    sizes = [shard_bounds(n_real, g, G)[1] - shard_bounds(n_real, g, G)[0] for g in range(G)]
    return comm.gather_to_root(sums, sizes)
