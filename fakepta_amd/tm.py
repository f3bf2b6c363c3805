"""Timing-model projection: the weighted least-squares fit of each pulsar's design matrix removed from residuals on
the device (fpta_tm_project, fpta_batch_set_timing_model; the definition is in include/fakepta_amd.h). The helpers
here lay an array's design matrices and weights out as the library reads them; BatchSimulator.set_timing_model and the
drop-in Pulsar.fit_timing_model / fit_timing_model_array share them."""
import numpy as np

from . import _capi

MAX_COL = _capi.TM_MAX_COL


def stack_design(Mmats):
    """Per-pulsar design matrices [n_p, m_p] (m_p may differ, 0 allowed) -> (M [n_toa, max m_p] with zero padding
    columns, ncol_psr [P] int32)."""
    mats = [np.asarray(m, dtype=np.float64) for m in Mmats]
    for i, m in enumerate(mats):
        if m.ndim != 2:
            raise ValueError(f"design matrix of pulsar {i} must be [n_toa, n_col], got shape {m.shape}")
        if m.shape[1] > MAX_COL:
            raise ValueError(f"design matrix of pulsar {i} has {m.shape[1]} columns; at most {MAX_COL} are supported")
    ncol = np.array([m.shape[1] for m in mats], dtype=np.int32)
    M = np.zeros((sum(len(m) for m in mats), int(ncol.max()) if len(mats) else 0))
    o = 0
    for m in mats:
        M[o:o + len(m), :m.shape[1]] = m
        o += len(m)
    return M, ncol


def design_of(psrs, Mmats, what):
    """Mmats "tm" (each pulsar's Mmat), None (nothing marginalised) or a list of [n_p, m_p <= 16] -> (M, ncol_psr)."""
    if isinstance(Mmats, str):
        if Mmats != "tm":
            raise ValueError(f"{what}: Mmats must be 'tm', None or a list of matrices, got {Mmats!r}")
        Mmats = [p.Mmat for p in psrs]
    if Mmats is None:
        Mmats = [np.zeros((len(p.toas), 0)) for p in psrs]
    Mmats = list(Mmats)
    if len(Mmats) != len(psrs):
        raise ValueError(f"{what}: {len(Mmats)} design matrices for {len(psrs)} pulsars")
    for i, (m, p) in enumerate(zip(Mmats, psrs)):
        if np.ndim(m) != 2 or np.shape(m)[0] != len(p.toas):
            raise ValueError(f"{what}: design matrix of pulsar {i} must be [{len(p.toas)}, n_col], got shape "
                             f"{np.shape(m)}")
    return stack_design(Mmats)


def weights_of(psrs, weights, n_toa):
    """weights "white": 1 / (EFAC^2 toaerr^2 + EQUAD^2) of each pulsar's noisedict; None: unit weights; else an array
    [n_toa] or a list of per-pulsar arrays. ECORR is not part of the weights."""
    if weights is None:
        return None
    if isinstance(weights, str):
        if weights != "white":
            raise ValueError(f"weights must be 'white', None or an array, got {weights!r}")
        return np.concatenate([1.0 / np.asarray(p._white_sigma2(), dtype=np.float64) for p in psrs])
    if isinstance(weights, (list, tuple)) and len(weights) and np.ndim(weights[0]) == 1:
        weights = np.concatenate([np.asarray(w, dtype=np.float64) for w in weights])
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.shape != (n_toa,):
        raise ValueError(f"weights must hold {n_toa} values, got shape {w.shape}")
    return w


def project(offs, Mmats, res, weights=None, rcond=None, ctx=None):
    """The fit of Mmats (list of [n_p, m_p]) removed from res [n_vec, n_toa] or [n_toa], in place. Returns the ranks."""
    M, ncol = stack_design(Mmats)
    ctx = ctx if ctx is not None else _capi.get_context()
    return ctx.tm_project(offs, M, res, ncol_psr=ncol, weights=weights, rcond=rcond)
