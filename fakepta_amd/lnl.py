"""Likelihood grid: per realization the Gaussian log-likelihood ratio of a common (or per-pulsar) process as a function
of its spectrum, on a grid of spectra, computed on the device (fpta_batch_set_lnl, fpta_batch_lnl, fpta_lnl_grid; the
definition is in include/fakepta_amd.h). The device returns dlnL [G, R] = ln p(r | phi_g) - ln p(r | phi = 0) with the
timing model marginalised. The helpers here build grids and hold the host algebra around dlnL: the maximum-likelihood
grid point, the evidence ratio against "no process" under a uniform prior over the grid points, and the normalised
posterior. BatchSimulator.set_likelihood_grid / likelihood_grid and the drop-in fake_pta.likelihood_grid_array share
them, and the layout-to-components code is fakepta_amd.os's. Nothing here needs a device except grid_array's one call."""
import numpy as np

from . import _capi
from . import os as _os
from . import tm as _tm

MAX_COEF, MAX_GRID = _capi.LNL_MAX_COEF, _capi.LNL_MAX_GRID


def powerlaw_grid(f, log10_A, gamma):
    """phi [len(log10_A) * len(gamma), N]: spectrum.powerlaw(f, A, gamma) * delta f for every pair of the two axes, the
    amplitude axis slowest (row i * len(gamma) + j is (log10_A[i], gamma[j]))."""
    from fakepta.spectrum import powerlaw
    f = np.asarray(f, dtype=np.float64)
    log10_A, gamma = np.atleast_1d(np.asarray(log10_A, dtype=np.float64)), np.atleast_1d(
        np.asarray(gamma, dtype=np.float64))
    if f.ndim != 1 or len(f) < 1 or not np.all(np.isfinite(f) & (f > 0)):
        raise ValueError("powerlaw_grid: f must be [N] positive frequencies")
    if log10_A.ndim != 1 or gamma.ndim != 1 or len(log10_A) < 1 or len(gamma) < 1:
        raise ValueError("powerlaw_grid: log10_A and gamma must be non-empty one-dimensional axes")
    if not (np.all(np.isfinite(log10_A)) and np.all(np.isfinite(gamma))):
        raise ValueError("powerlaw_grid: an axis value is not finite")
    df = np.diff(np.append(0.0, f))
    return np.stack([powerlaw(f, a, g) * df for a in log10_A for g in gamma])


def check_grid(phi, N):
    """phi as [G, N] float64: finite, >= 0, 1 <= G <= MAX_GRID, else ValueError naming the row and mode."""
    phi = np.asarray(phi, dtype=np.float64)
    if phi.ndim == 1:
        phi = phi[None]
    if phi.ndim != 2 or phi.shape[1] != N:
        raise ValueError(f"the grid must hold the target's {N} modes per row, got shape {phi.shape}")
    if not 1 <= len(phi) <= MAX_GRID:
        raise ValueError(f"{len(phi)} grid points outside [1, {MAX_GRID}]")
    bad = np.argwhere(~(np.isfinite(phi) & (phi >= 0)))
    if len(bad):
        raise ValueError(f"grid row {bad[0][0]}, mode {bad[0][1]}: prior variance is negative or not finite")
    return np.ascontiguousarray(phi)


def make_grid(f, phi=None, log10_A=None, gamma=None):
    """(phi [G, N], axes): either an explicit grid (axes None) or the power-law grid of the two axes (axes = (log10_A,
    gamma) as arrays); ValueError when both or neither are given."""
    axes = log10_A is not None or gamma is not None
    if (phi is not None) == axes:
        raise ValueError("the likelihood grid takes either phi [G, N] or the axes log10_A and gamma")
    if phi is not None:
        return check_grid(phi, len(f)), None
    if log10_A is None or gamma is None:
        raise ValueError("the likelihood grid needs both axes, log10_A and gamma")
    log10_A, gamma = np.atleast_1d(np.asarray(log10_A, dtype=np.float64)), np.atleast_1d(
        np.asarray(gamma, dtype=np.float64))
    return check_grid(powerlaw_grid(f, log10_A, gamma), len(f)), (log10_A, gamma)


def argmax(dlnL):
    """[R]: the grid point of the largest dlnL per realization (the first of equals)."""
    dlnL = np.asarray(dlnL, dtype=np.float64)
    if dlnL.ndim != 2 or dlnL.shape[0] < 1:
        raise ValueError(f"dlnL must be [G, R], got {dlnL.shape}")
    return np.argmax(dlnL, axis=0)


def log_bayes(dlnL):
    """lnB [R] = logsumexp_g(dlnL) - ln G: the evidence ratio against "no process" under a uniform prior over the
    grid points."""
    dlnL = np.asarray(dlnL, dtype=np.float64)
    if dlnL.ndim != 2 or dlnL.shape[0] < 1:
        raise ValueError(f"dlnL must be [G, R], got {dlnL.shape}")
    top = np.max(dlnL, axis=0)
    return top + np.log(np.sum(np.exp(dlnL - top), axis=0)) - np.log(dlnL.shape[0])


def posterior(dlnL):
    """[G, R]: exp(dlnL) normalised over the grid points per realization (a uniform prior over them)."""
    dlnL = np.asarray(dlnL, dtype=np.float64)
    if dlnL.ndim != 2 or dlnL.shape[0] < 1:
        raise ValueError(f"dlnL must be [G, R], got {dlnL.shape}")
    w = np.exp(dlnL - np.max(dlnL, axis=0))
    return w / np.sum(w, axis=0)


def derive(dlnL, axes=None, ld=None, q_psr=None, want_posterior=False):
    """Everything the host derives from dlnL [G, R]: dlnL (shaped [nA, ngamma, R] when the grid came from axes), argmax
    [R] (with axes: a tuple of index arrays (i_A, i_gamma), plus log10_A_ml and gamma_ml [R]), lnB [R], the axes, on
    request the posterior (shaped like dlnL), and with q_psr [P, G, R] and ld [P, G] the per-pulsar q_psr and dlnL_psr =
    (q_psr - ld) / 2, whose sum over the pulsars in order is dlnL bit for bit."""
    dlnL = np.asarray(dlnL, dtype=np.float64)
    G, R = dlnL.shape
    am = argmax(dlnL)
    out = dict(dlnL=dlnL, argmax=am, lnB=log_bayes(dlnL), log10_A=None, gamma=None)
    shape = (G,)
    if axes is not None:
        shape = (len(axes[0]), len(axes[1]))
        out.update(log10_A=axes[0], gamma=axes[1], argmax=np.unravel_index(am, shape))
        out["log10_A_ml"], out["gamma_ml"] = axes[0][out["argmax"][0]], axes[1][out["argmax"][1]]
        out["dlnL"] = dlnL.reshape(shape + (R,))
    if want_posterior:
        out["posterior"] = posterior(dlnL).reshape(shape + (R,))
    if q_psr is not None:
        out["q_psr"] = q_psr
        out["dlnL_psr"] = 0.5 * (q_psr - np.asarray(ld)[:, :, None])
    return out


def target_frequencies(model, target):
    """The target's frequencies [N] of a noise_model() (the first pulsar's row of a per-pulsar grid)."""
    n0, N = int(model["n_modes"][:target].sum()), int(model["n_modes"][target])
    f = model["f"]
    return (f if f.ndim == 1 else f[0])[n0:n0 + N]


def grid_array(psrs, target=None, phi=None, log10_A=None, gamma=None, signals=None, Mmats="tm", weights="white",
               rcond=None, per_pulsar=False, want_posterior=False, ctx=None):
    """The likelihood grid of psr.residuals for a whole array in one device call (fpta_lnl_grid): the dict of derive()
    for one residual vector (R = 1). The noise model is what the pulsars carry: signal_model (every GP, or `signals`)
    and the white noise of the noisedict as weights; the target's own spectrum is replaced by the grid's. ECORR is not
    part of the weights."""
    segs = _os.segments_of(psrs, signals)
    t = _os.pick_target(segs, target)
    model = _os.noise_model(segs, len(psrs))
    grid, axes = make_grid(target_frequencies(model, t), phi, log10_A, gamma)
    M, ncol = _os.design_of(psrs, Mmats, "likelihood_grid_array")
    offs = np.concatenate([[0], np.cumsum([len(p.toas) for p in psrs])]).astype(np.int64)
    toas = np.concatenate([np.asarray(p.toas, dtype=np.float64) for p in psrs])
    nu = np.concatenate([np.asarray(p.freqs, dtype=np.float64) for p in psrs])
    res = np.concatenate([np.asarray(p.residuals, dtype=np.float64) for p in psrs])
    ctx = ctx if ctx is not None else _capi.get_context()
    d, q, _, _, ld, _ = ctx.lnl_grid(offs, toas, nu, model["n_modes"], model["f"], model["idx"], model["freqf"],
                                     model["phi"], t, grid, res, masks=model["masks"], M=M, ncol_psr=ncol,
                                     weights=_tm.weights_of(psrs, weights, int(offs[-1])), rcond=rcond)
    return derive(d, axes, ld, q if per_pulsar else None, want_posterior)
