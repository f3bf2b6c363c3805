"""Correlated likelihood grid: the likelihood grid of fakepta_amd.lnl with the common process correlated between the
pulsars by an overlap reduction function, computed on the device (fpta_batch_set_clnl, fpta_batch_clnl, fpta_clnl_grid;
the definition is in include/fakepta_amd.h). The device returns dlnL [n_orf, G, R] = ln p(r | Gamma_o, phi_g) -
ln p(r | phi = 0) with the timing model marginalised. The helpers here turn ORF names and matrices into factors and hold
the host algebra around dlnL: per ORF the maximum-likelihood grid point and the evidence ratio against "no process"
under a uniform prior over the grid points, and the ratio of every ORF's evidence to CURN's: the Hellings-Downs versus
CURN Bayes factor. BatchSimulator.set_correlated_likelihood / correlated_likelihood and the drop-in
fake_pta.correlated_likelihood_array share them. Nothing here needs a device except grid_array's one call."""
import numpy as np

from . import _capi
from . import lnl as _lnl
from . import os as _os
from . import tm as _tm

MAX_ORF, MAX_N = _capi.CLNL_MAX_ORF, _capi.CLNL_MAX_N


def check_orf(g, P, what="orf"):
    """g as a symmetric positive semidefinite [P, P] float64 matrix, else ValueError: symmetric within 1e-12 of its
    largest entry, no eigenvalue below -1e-10 of the largest."""
    g = np.array(g, dtype=np.float64)
    if g.shape != (P, P):
        raise ValueError(f"{what}: an ORF must be [{P}, {P}], got {g.shape}")
    if not np.all(np.isfinite(g)):
        raise ValueError(f"{what}: an ORF entry is not finite")
    scale = float(np.max(np.abs(g))) if g.size else 0.0
    if np.max(np.abs(g - g.T), initial=0.0) > 1e-12 * scale:
        raise ValueError(f"{what}: the ORF is not symmetric")
    g = 0.5 * (g + g.T)
    w = np.linalg.eigvalsh(g)
    if len(w) and (w[0] < -1e-10 * abs(w[-1]) or w[-1] < 0):
        raise ValueError(f"{what}: the ORF is not positive semidefinite (smallest eigenvalue {w[0]:.3e})")
    return g


def orf_factors(psrs, orfs=("hd", "curn"), what="orf"):
    """(names [J], Gamma [J, P, P], A [J, P, P]) of ORFs given as names fakepta's orf_matrix knows ("hd", "monopole",
    "dipole", "curn") or as [P, P] arrays (named "orf<i>"): A is batch_factor's, the lower Cholesky factor or the
    zero-truncated SVD factor of a singular ORF, A A^T = Gamma."""
    from fakepta.correlated_noises import orf_matrix
    from .batch import batch_factor
    P = len(psrs)
    if isinstance(orfs, (str, np.ndarray)):
        orfs = [orfs]
    orfs = list(orfs)
    if not 1 <= len(orfs) <= MAX_ORF:
        raise ValueError(f"{what}: {len(orfs)} ORFs outside [1, {MAX_ORF}]")
    names, gammas = [], []
    for i, orf in enumerate(orfs):
        if isinstance(orf, str):
            names.append(orf)
            gammas.append(check_orf(orf_matrix(psrs, orf), P, what))
        else:
            names.append(f"orf{i}")
            gammas.append(check_orf(orf, P, what))
    A = np.stack([batch_factor(g) for g in gammas]) if P else np.zeros((len(orfs), 0, 0))
    return names, np.stack(gammas), np.ascontiguousarray(A)


def derive(dlnL, names, axes=None, ld=None, want_posterior=False):
    """Everything the host derives from dlnL [n_orf, G, R]: dlnL (shaped [n_orf, nA, ngamma, R] when the grid came from
    axes), per ORF argmax [n_orf, R] (with axes: a tuple of two such index arrays, plus log10_A_ml and gamma_ml
    [n_orf, R]), lnB [n_orf, R] = logsumexp_g - ln G, lnB_vs_curn [n_orf, R] = lnB - lnB of "curn" when it is among the
    ORFs, orfs (the names), the axes, ld [n_orf, G], and on request the posterior (shaped like dlnL)."""
    dlnL = np.asarray(dlnL, dtype=np.float64)
    if dlnL.ndim != 3 or dlnL.shape[0] != len(names):
        raise ValueError(f"dlnL must be [{len(names)}, G, R], got {dlnL.shape}")
    J, G, R = dlnL.shape
    per = [_lnl.derive(dlnL[o], axes, want_posterior=want_posterior) for o in range(J)]
    out = dict(orfs=list(names), ld=ld, log10_A=per[0]["log10_A"], gamma=per[0]["gamma"],
               dlnL=np.stack([p["dlnL"] for p in per]), lnB=np.stack([p["lnB"] for p in per]))
    if axes is None:
        out["argmax"] = np.stack([p["argmax"] for p in per])
    else:
        out["argmax"] = tuple(np.stack([p["argmax"][a] for p in per]) for a in range(2))
        out["log10_A_ml"] = np.stack([p["log10_A_ml"] for p in per])
        out["gamma_ml"] = np.stack([p["gamma_ml"] for p in per])
    if "curn" in names:
        out["lnB_vs_curn"] = out["lnB"] - out["lnB"][list(names).index("curn")]
    if want_posterior:
        out["posterior"] = np.stack([p["posterior"] for p in per])
    return out


def grid_array(psrs, target=None, orfs=("hd", "curn"), phi=None, log10_A=None, gamma=None, signals=None, Mmats="tm",
               weights="white", rcond=None, want_posterior=False, ctx=None):
    """The correlated likelihood grid of psr.residuals for a whole array in one device call (fpta_clnl_grid): the dict
    of derive() for one residual vector (R = 1). The noise model is what the pulsars carry, as lnl.grid_array takes it;
    the target's own spectrum and ORF are replaced by the grid's and `orfs`."""
    segs = _os.segments_of(psrs, signals)
    t = _os.pick_target(segs, target)
    model = _os.noise_model(segs, len(psrs))
    grid, axes = _lnl.make_grid(_lnl.target_frequencies(model, t), phi, log10_A, gamma)
    names, _, A = orf_factors(psrs, orfs, "correlated_likelihood_array")
    M, ncol = _os.design_of(psrs, Mmats, "correlated_likelihood_array")
    offs = np.concatenate([[0], np.cumsum([len(p.toas) for p in psrs])]).astype(np.int64)
    toas = np.concatenate([np.asarray(p.toas, dtype=np.float64) for p in psrs])
    nu = np.concatenate([np.asarray(p.freqs, dtype=np.float64) for p in psrs])
    res = np.concatenate([np.asarray(p.residuals, dtype=np.float64) for p in psrs])
    ctx = ctx if ctx is not None else _capi.get_context()
    d, _, _, _, _, ld, _ = ctx.clnl_grid(offs, toas, nu, model["n_modes"], model["f"], model["idx"], model["freqf"],
                                         model["phi"], t, grid, A, res, masks=model["masks"], M=M, ncol_psr=ncol,
                                         weights=_tm.weights_of(psrs, weights, int(offs[-1])), rcond=rcond)
    return derive(d, names, axes, ld, want_posterior)
