"""Optimal statistic: the noise-weighted cross-correlation statistic of every realization on the device
(fpta_batch_set_os, fpta_batch_os, fpta_os_statistic; the definition is in include/fakepta_amd.h). The device returns
one number per pair-weight matrix and realization, Q[j][r], and the host gets the pair normalisations N_ab with the
plan. The helpers here are the host algebra around them: pair-weight matrices of named overlap reduction functions
(ORFs) and angular bins, the noise model of a layout as the library's tables, and N_ab -> denominators, the joint fit of
several ORFs and the binned correlations. BatchSimulator.set_optimal_statistic / optimal_statistic and the drop-in
fake_pta.optimal_statistic_array share them. Nothing here needs a device except statistic_array's one call."""
import numpy as np

from . import _capi
from . import tm as _tm

MAX_COMP, MAX_COL, MAX_COEF = _capi.OS_MAX_COMP, _capi.OS_MAX_COL, _capi.OS_MAX_COEF


def angular_bins(pos, bins):
    """The pairs of every angular bin as pair-weight matrices: (G [bins, P, P] of 0 / 1, symmetric, zero diagonal; bin
    centres; pairs per bin). Edges linspace(0, pi, bins + 1), open bins, as BatchSimulator.hd_curve: a pair exactly on
    an edge is in no bin."""
    bins = int(bins)
    if bins < 1:
        raise ValueError(f"bins must be a positive count, got {bins}")
    pos = np.asarray(pos, dtype=np.float64)
    if pos.ndim != 2 or pos.shape[1] != 3:
        raise ValueError(f"pulsar positions must be [P, 3], got {pos.shape}")
    P = len(pos)
    ang = np.arccos(np.clip(pos @ pos.T, -1.0, 1.0))
    edges = np.linspace(0.0, np.pi, bins + 1)
    off = ~np.eye(P, dtype=bool)
    G = np.stack([((ang > lo) & (ang < hi) & off).astype(np.float64) for lo, hi in zip(edges[:-1], edges[1:])])
    G = np.maximum(G, G.transpose(0, 2, 1))  # arccos of a symmetric matrix is symmetric; make the flags exactly so
    return G, edges[:-1] + 0.5 * (edges[1] - edges[0]), (G.sum(axis=(1, 2)) / 2).astype(np.int64)


def check_pair_matrices(G, P):
    """G as [J, P, P] float64: finite and exactly symmetric, else ValueError naming the matrix and the pair."""
    G = np.asarray(G, dtype=np.float64)
    if G.ndim == 2:
        G = G[None]
    if G.ndim != 3 or G.shape[1:] != (P, P):
        raise ValueError(f"pair-weight matrices must be [J, {P}, {P}], got {G.shape}")
    off = ~np.eye(P, dtype=bool)
    for j, g in enumerate(G):
        bad = np.argwhere(~np.isfinite(g) & off)
        if len(bad):
            raise ValueError(f"pair-weight matrix {j}, pair ({bad[0][0]}, {bad[0][1]}): not finite")
        bad = np.argwhere(g != g.T)
        if len(bad):
            raise ValueError(f"pair-weight matrix {j}, pair ({bad[0][0]}, {bad[0][1]}): not symmetric")
    return np.ascontiguousarray(G)


def pair_matrices(psrs, orfs=("hd",), bins=None):
    """(G [n_orf + bins, P, P], n_orf, bin centres, pairs per bin): one matrix per ORF (a name fakepta's orf_matrix
    knows, or an explicit [P, P] array), then one per angular bin. The diagonal is ignored by the statistic and set to
    zero here."""
    from fakepta.correlated_noises import orf_matrix
    P = len(psrs)
    if isinstance(orfs, (str, np.ndarray)):
        orfs = [orfs]
    mats = []
    for i, orf in enumerate(orfs):
        if isinstance(orf, str):
            g = np.array(orf_matrix(psrs, orf), dtype=np.float64)
        else:
            g = np.array(orf, dtype=np.float64)
            if g.shape != (P, P):
                raise ValueError(f"ORF {i} must be a name or a [{P}, {P}] array, got shape {g.shape}")
        np.fill_diagonal(g, 0.0)
        mats.append(g)
    centres, counts = np.zeros(0), np.zeros(0, dtype=np.int64)
    if bins is not None:
        Gb, centres, counts = angular_bins(np.array([np.asarray(p.pos, dtype=np.float64) for p in psrs]), bins)
        mats += list(Gb)
    if not mats:
        raise ValueError("the optimal statistic needs at least one ORF or angular bin")
    return check_pair_matrices(np.stack(mats), P), len(orfs), centres, counts


def _lower(P):
    return np.tril_indices(P, -1)


def norms(G, nab):
    """[J]: sum_{a<b} G_j[a][b]^2 N_ab, the denominator of A2 (and, for a 0 / 1 matrix, of the binned rho)."""
    il = _lower(nab.shape[0])
    return np.array([np.sum(g[il] ** 2 * nab[il]) for g in G])


def joint_matrix(G, nab):
    """[J, J]: C_jj' = sum_{a<b} G_j[a][b] G_j'[a][b] N_ab, the normal matrix of the multi-ORF fit."""
    il = _lower(nab.shape[0])
    rows = np.array([g[il] for g in G])
    return (rows * nab[il]) @ rows.T


def derive(Q, G, nab, n_orf, centres=None, counts=None, Q_mode=None):
    """Everything the host derives from Q [J, R] and N_ab: A2 and snr [n_orf, R], A2_joint [n_orf, R] for more than
    one ORF (C A = Q), rho_bins [bins, R] (NaN for a bin without a pair of positive N_ab), bin_centres, bin_counts, Q,
    norm [J] and, when given, Q_mode [J, N, R]."""
    Q = np.asarray(Q, dtype=np.float64)
    norm = norms(G, nab)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(norm[:, None] > 0, Q / norm[:, None], np.nan)
        snr = np.where(norm[:n_orf, None] > 0, Q[:n_orf] / np.sqrt(norm[:n_orf, None]), np.nan)
    out = dict(A2=ratio[:n_orf], snr=snr, rho_bins=ratio[n_orf:], Q=Q, norm=norm,
               bin_centres=np.zeros(0) if centres is None else centres,
               bin_counts=np.zeros(0, dtype=np.int64) if counts is None else counts)
    if n_orf > 1:
        out["A2_joint"] = np.linalg.solve(joint_matrix(G[:n_orf], nab), Q[:n_orf])
    if Q_mode is not None:
        out["Q_mode"] = Q_mode
    return out


def symmetric_pair_norms(nab):
    """N_ab [R, P, P] as fpta_batch_os_spectra leaves it (the entries a >= b) -> symmetric with a zero diagonal, the
    form of set_optimal_statistic's N_ab."""
    nab = np.asarray(nab, dtype=np.float64)
    low = np.tril(nab, -1)
    return low + low.transpose(0, 2, 1)


def norms_per_realization(G, nab):
    """[J, R]: norms() of every realization's N_ab [R, P, P], row-major over the pairs a > b."""
    il = _lower(nab.shape[1])
    return np.array([np.sum(g[il] ** 2 * nab[:, il[0], il[1]], axis=1) for g in G]).reshape(len(G), len(nab))


def joint_matrix_per_realization(G, nab):
    """[J, J, R]: joint_matrix() of every realization's N_ab [R, P, P]."""
    il = _lower(nab.shape[1])
    rows = np.array([g[il] for g in G]).reshape(len(G), -1)
    return np.einsum("ip,jp,rp->ijr", rows, rows, nab[:, il[0], il[1]])


def derive_per_realization(Q, norm, joint, n_orf, centres=None, counts=None, Q_mode=None, nab=None):
    """derive() with a denominator per realization: Q and norm [J, R], joint [n_orf, n_orf, R] (the device's, or
    norms_per_realization / joint_matrix_per_realization). A2, snr and A2_joint [n_orf, R] (one solve per realization;
    for one ORF it is A2), rho_bins [bins, R]; an ORF or a bin whose denominator is 0 in a realization, and a joint fit
    whose matrix is singular there, is NaN there. Q_mode and N_ab (made symmetric) are passed through when given."""
    Q, norm, joint = (np.asarray(v, dtype=np.float64) for v in (Q, norm, joint))
    R = Q.shape[1]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(norm > 0, Q / norm, np.nan)
        snr = np.where(norm[:n_orf] > 0, Q[:n_orf] / np.sqrt(norm[:n_orf]), np.nan)
    joint_a2 = np.full((n_orf, R), np.nan)
    for r in range(R if n_orf else 0):
        C = joint[:, :, r]
        if np.all(np.diag(C) > 0) and np.linalg.matrix_rank(C) == n_orf:
            joint_a2[:, r] = np.linalg.solve(C, Q[:n_orf, r])
    out = dict(A2=ratio[:n_orf], snr=snr, A2_joint=joint_a2, rho_bins=ratio[n_orf:], Q=Q, norm=norm, joint=joint,
               bin_centres=np.zeros(0) if centres is None else centres,
               bin_counts=np.zeros(0, dtype=np.int64) if counts is None else counts)
    if Q_mode is not None:
        out["Q_mode"] = Q_mode
    if nab is not None:
        out["N_ab"] = symmetric_pair_norms(nab)
    return out


# ----------------------------------------------------------------------------- sky scrambles
def scramble_positions(n, P, seed=0):
    """n sets of P directions, uniform on the sphere: unit vectors [n, P, 3] from np.random.default_rng(seed). Drawn on
    the host, like the continuous-wave populations: the seed fixes them whatever the device."""
    n, P = int(n), int(P)
    if n < 0 or P < 1:
        raise ValueError(f"scramble_positions: n must be >= 0 and P >= 1, got {n} and {P}")
    rng = np.random.default_rng(seed)
    z = rng.uniform(-1.0, 1.0, (n, P))
    lon = rng.uniform(0.0, 2.0 * np.pi, (n, P))
    s = np.sqrt(1.0 - z * z)
    pos = np.stack([s * np.cos(lon), s * np.sin(lon), z], axis=-1)
    return np.ascontiguousarray(pos / np.linalg.norm(pos, axis=-1, keepdims=True))


def _positions_of(psrs_or_pos):
    """[P, 3] float64 from an array of positions or from pulsars with a pos attribute."""
    if isinstance(psrs_or_pos, np.ndarray) or not hasattr(psrs_or_pos[0], "pos"):
        pos = np.asarray(psrs_or_pos, dtype=np.float64)
    else:
        pos = np.array([np.asarray(p.pos, dtype=np.float64) for p in psrs_or_pos])
    if pos.ndim != 2 or pos.shape[1] != 3 or len(pos) < 2:
        raise ValueError(f"sky_scrambles: the true positions must be [P >= 2, 3], got {pos.shape}")
    return pos


def hd_matrix(pos):
    """Hellings-Downs [P, P] of unit positions [P, 3], fakepta.correlated_noises.hd's formula, zero diagonal."""
    pos = np.asarray(pos, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        x = (1 - pos @ pos.T) / 2
        g = 1.5 * x * np.log(x) - 0.25 * x + 0.5
    np.fill_diagonal(g, 0.0)
    return g


def sky_scrambles(ctx, psrs_or_pos, n, seed=0, max_match=0.1, ref="hd", max_tries=20):
    """n sky scrambles of a small match with the true sky: candidates from scramble_positions (batches of max(2 n,
    256), batch b seeded [seed, b]), their match with the reference computed on the device (fpta_os_scramble_match),
    the first n with |match| <= max_match kept in the order drawn. ref: "hd", the Hellings-Downs matrix of the true
    positions, or explicit matrices [n_ref, P, P] (every one of them has to be matched that little). Returns
    (positions [n, P, 3], match [n, n_ref]). ValueError with the acceptance rate when max_tries batches do not give
    n."""
    n = int(n)
    if n < 0:
        raise ValueError(f"sky_scrambles: n must be >= 0, got {n}")
    if isinstance(ref, str):
        if ref != "hd":
            raise ValueError(f"sky_scrambles: ref must be 'hd' or explicit matrices, got {ref!r}")
        ref_m = hd_matrix(_positions_of(psrs_or_pos))[None]
    else:
        ref_m = np.asarray(ref, dtype=np.float64)
        ref_m = ref_m[None] if ref_m.ndim == 2 else ref_m
    P = ref_m.shape[-1]
    kept, matches, have, drawn = [], [], 0, 0
    batch = max(2 * n, 256)
    for b in range(int(max_tries)):
        if have >= n:
            break
        cand = scramble_positions(batch, P, [int(seed), b])
        m = ctx.os_scramble_match(cand, ref_m)
        ok = np.all(np.abs(m) <= max_match, axis=1)
        kept.append(cand[ok])
        matches.append(m[ok])
        have += int(ok.sum())
        drawn += batch
    if have < n:
        raise ValueError(f"sky_scrambles: {have} of {drawn} candidates have |match| <= {max_match} (acceptance rate "
                         f"{have / max(drawn, 1):.3g}), fewer than the {n} asked for; raise max_match or max_tries")
    pos = np.concatenate(kept)[:n] if kept else np.zeros((0, P, 3))
    return np.ascontiguousarray(pos), np.concatenate(matches)[:n] if matches else np.zeros((0, len(ref_m)))


def derive_scrambles(snr_obs, count_ge, n_scr, mean=None, std=None, mx=None, n_orf=None, snr_null=None):
    """What the host derives from the device's ranks: p_value = (1 + count_ge) / (1 + J) (the observed sky counts as
    one of its own scrambles, so no p-value is 0), snr and count_ge [n_orf, R] (the first n_orf rows; None: all), and
    the null's moments null_mean, null_std, null_max [R] and snr_null [J, R] passed through when given."""
    snr_obs = np.asarray(snr_obs, dtype=np.float64)
    count_ge = np.asarray(count_ge)
    if not np.issubdtype(count_ge.dtype, np.integer):
        raise ValueError("derive_scrambles: count_ge must be integer counts")
    n_scr = int(n_scr)
    if n_scr < 1 or np.any(count_ge < 0) or np.any(count_ge > n_scr):
        raise ValueError(f"derive_scrambles: counts outside [0, {n_scr}]")
    k = len(snr_obs) if n_orf is None else int(n_orf)
    out = dict(p_value=(1.0 + count_ge[:k]) / (1.0 + n_scr), snr=snr_obs[:k], count_ge=count_ge[:k])
    for key, v in (("null_mean", mean), ("null_std", std), ("null_max", mx), ("snr_null", snr_null)):
        if v is not None:
            out[key] = v
    return out


def scrambles_array(psrs, n=1000, seed=0, max_match=0.1, target=None, orfs=("hd",), template=None, signals=None,
                    Mmats="tm", weights="white", rcond=None, positions=None, matrices=None, full=False, ctx=None):
    """The sky-scramble null distribution of the optimal statistic of psr.residuals for a whole array in one device
    call (fpta_os_scrambles): derive_scrambles' dict for one residual vector (R = 1) plus match [J, n_orf], norm [J]
    and positions (when they were drawn here or given). The noise model is statistic_array's. The scrambles are
    sky_scrambles(ctx, psrs, n, seed, max_match) against the first ORF, or the given positions / matrices."""
    segs = segments_of(psrs, signals)
    t = pick_target(segs, target)
    model = noise_model(segs, len(psrs))
    phi_hat = template_of(model, t, template)
    G, n_orf, _, _ = pair_matrices(psrs, orfs, None)
    M, ncol = design_of(psrs, Mmats, "optimal_statistic_scrambles_array")
    offs = np.concatenate([[0], np.cumsum([len(p.toas) for p in psrs])]).astype(np.int64)
    toas = np.concatenate([np.asarray(p.toas, dtype=np.float64) for p in psrs])
    nu = np.concatenate([np.asarray(p.freqs, dtype=np.float64) for p in psrs])
    res = np.concatenate([np.asarray(p.residuals, dtype=np.float64) for p in psrs])
    ctx = ctx if ctx is not None else _capi.get_context()
    if positions is None and matrices is None:
        positions, _ = sky_scrambles(ctx, psrs, n, seed=seed, max_match=max_match, ref=G[:1])
    got = ctx.os_scrambles(offs, toas, nu, model["n_modes"], model["f"], model["idx"], model["freqf"], model["phi"], t,
                           phi_hat, G, res, pos=positions, matrices=matrices, masks=model["masks"], M=M, ncol_psr=ncol,
                           weights=_tm.weights_of(psrs, weights, int(offs[-1])), rcond=rcond, full=full)
    out = derive_scrambles(got["snr_obs"], got["count_ge"], len(got["norm"]), got["mean"], got["std"], got["max"],
                           n_orf, got["snr_null"])
    out.update(match=got["match"][:, :n_orf], norm=got["norm"], Q=got["Q"])
    if positions is not None:
        out["positions"] = np.asarray(positions, dtype=np.float64)
    return out


def noise_model(segments, n_psr):
    """BatchSimulator-style segments (dicts with name, kind 0 per-pulsar f, amp [P, N] / 1 common f, amp [N], idx,
    freqf, mask) -> dict(names, n_modes [C] int32, f [sum N] or [P, sum N], idx, freqf, phi [P, sum N] = amp^2, masks).
    One grid for the array when every segment is common, else per-pulsar rows."""
    segments = list(segments)
    if not 1 <= len(segments) <= MAX_COMP:
        raise ValueError(f"the noise model takes 1 .. {MAX_COMP} components, got {len(segments)}")
    per_psr = any(np.ndim(s["f"]) == 2 for s in segments)
    fs, phis = [], []
    for i, s in enumerate(segments):
        f, amp = np.asarray(s["f"], dtype=np.float64), np.asarray(s["amp"], dtype=np.float64)
        if f.shape != amp.shape or f.ndim not in (1, 2) or f.shape[-1] < 1 or (f.ndim == 2 and f.shape[0] != n_psr):
            raise ValueError(f"component {i}: f and amp must both be [N] or [{n_psr}, N], got {f.shape} and "
                             f"{amp.shape}")
        if not np.all(np.isfinite(amp)):
            raise ValueError(f"component {i}: an amplitude is not finite")
        fs.append(np.tile(f, (n_psr, 1)) if per_psr and f.ndim == 1 else f)
        phis.append(np.tile(amp ** 2, (n_psr, 1)) if amp.ndim == 1 else amp ** 2)
    n_modes = np.array([f.shape[-1] for f in fs], dtype=np.int32)
    if 2 * int(n_modes.sum()) > MAX_COL:
        raise ValueError(f"{2 * int(n_modes.sum())} Fourier columns, more than {MAX_COL}")
    return dict(names=[s.get("name") for s in segments], n_modes=n_modes,
                f=np.ascontiguousarray(np.concatenate(fs, axis=-1)),
                idx=np.array([float(s.get("idx", 0.0)) for s in segments]),
                freqf=np.array([float(s.get("freqf", 1400.0)) for s in segments]),
                phi=np.ascontiguousarray(np.concatenate(phis, axis=-1)), masks=[s.get("mask") for s in segments])


def pick_target(segments, target=None):
    """The index of the target component: a name, an index, or None for the only common (kind 1) segment."""
    segments = list(segments)
    if target is None:
        common = [i for i, s in enumerate(segments) if s.get("kind") == 1]
        if len(common) != 1:
            raise ValueError(f"the layout has {len(common)} common signals: name the target of the optimal statistic")
        return common[0]
    if isinstance(target, str):
        hit = [i for i, s in enumerate(segments) if s.get("name") == target]
        if not hit:
            raise KeyError(f"the noise model has no signal {target!r}")
        return hit[0]
    t = int(target)
    if t != target or not 0 <= t < len(segments):
        raise ValueError(f"target {target!r} is not a component index in [0, {len(segments)})")
    return t


def template_of(model, target, template=None):
    """phi_hat [N]: the given template, or the target's own amp^2 (it is common, so every pulsar's row is the same and
    A2 comes out in units of the injected power)."""
    n0 = int(model["n_modes"][:target].sum())
    N = int(model["n_modes"][target])
    if template is None:
        template = model["phi"][0, n0:n0 + N] if len(model["phi"]) else np.ones(N)
    template = np.asarray(template, dtype=np.float64)
    if template.shape != (N,):
        raise ValueError(f"the template must hold the target's {N} modes, got shape {template.shape}")
    if not np.all(np.isfinite(template) & (template > 0)):
        raise ValueError("every template value must be positive and finite")
    return template


def segments_of(psrs, names=None):
    """The noise model an array of Pulsar objects carries (signal_model and noisedict), as BatchSimulator lays it
    out, without a device: per-pulsar signals on [P, N] grids (a pulsar without the signal, or with fewer modes, gets
    zero amplitudes there), common signals on their own grid."""
    from .batch import GP_NAMES, _df, _n_modes
    P = len(psrs)
    if names is None:
        names = []
        for p in psrs:
            for s in p.signal_model:
                if s not in names and (s in GP_NAMES or "common" in s or "system_noise" in s):
                    names.append(s)
    out = []
    for name in names:
        have = [p for p in psrs if name in p.signal_model]
        if not have:
            raise KeyError(f"no pulsar carries signal {name!r}")
        sm0 = have[0].signal_model[name]
        if "common" in name:
            n = _n_modes(sm0)
            f = np.asarray(sm0["f"], float)
            out.append(dict(name=name, kind=1, f=f[:n], amp=np.sqrt(np.asarray(sm0["psd"], float) * _df(f))[:n],
                            idx=float(sm0["idx"]), freqf=1400.0, mask=None))
            continue
        nm = max(_n_modes(p.signal_model[name]) for p in have)
        f, amp = np.zeros((P, nm)), np.zeros((P, nm))
        for i, p in enumerate(psrs):
            if name in p.signal_model:
                sm = p.signal_model[name]
                n = _n_modes(sm)
                fi = np.asarray(sm["f"], float)
                amp[i, :n] = np.sqrt(np.asarray(sm["psd"], float) * _df(fi))[:n]
                fi = fi[:n]
                f[i, :n] = fi
                if len(fi) < nm:
                    step = fi[0] if len(fi) else 1.0
                    f[i, len(fi):] = (fi[-1] if len(fi) else 0.0) + step * np.arange(1, nm - len(fi) + 1)
            else:
                f[i] = np.arange(1, nm + 1) / max(np.ptp(p.toas), 1.0)
        idx, mask = float(sm0["idx"]), None
        if "system_noise" in name:
            backend = name.split("system_noise_")[1]
            mask = np.concatenate([p.backend_flags == backend for p in psrs]).astype(np.uint8)
            idx = 0.0
        out.append(dict(name=name, kind=0, f=f, amp=amp, idx=idx, freqf=1400.0, mask=mask))
    return out


design_of = _tm.design_of  # (lnl.py takes it from here)


def statistic_array(psrs, target=None, orfs=("hd",), bins=None, template=None, signals=None, Mmats="tm",
                    weights="white", rcond=None, per_mode=False, ctx=None):
    """The optimal statistic of psr.residuals for a whole array in one device call (fpta_os_statistic): the dict of
    derive() for one residual vector (R = 1). The noise model is what the pulsars carry: signal_model (every GP, or
    `signals`) and the white noise of the noisedict as weights. ECORR is not part of the weights."""
    segs = segments_of(psrs, signals)
    t = pick_target(segs, target)
    model = noise_model(segs, len(psrs))
    phi_hat = template_of(model, t, template)
    G, n_orf, centres, counts = pair_matrices(psrs, orfs, bins)
    M, ncol = design_of(psrs, Mmats, "optimal_statistic_array")
    offs = np.concatenate([[0], np.cumsum([len(p.toas) for p in psrs])]).astype(np.int64)
    toas = np.concatenate([np.asarray(p.toas, dtype=np.float64) for p in psrs])
    nu = np.concatenate([np.asarray(p.freqs, dtype=np.float64) for p in psrs])
    res = np.concatenate([np.asarray(p.residuals, dtype=np.float64) for p in psrs])
    ctx = ctx if ctx is not None else _capi.get_context()
    Q, Qm, _, _, nab = ctx.os_statistic(offs, toas, nu, model["n_modes"], model["f"], model["idx"], model["freqf"],
                                        model["phi"], t, phi_hat, G, res, masks=model["masks"], M=M, ncol_psr=ncol,
                                        weights=_tm.weights_of(psrs, weights, int(offs[-1])), rcond=rcond)
    return derive(Q, G, nab, n_orf, centres, counts, Qm if per_mode else None)
