"""Continuous gravitational wave of a circular supermassive black-hole binary, evaluated on the GPU
(fpta_cw_accumulate, csrc/cw.hip): the signal of enterprise_extensions.deterministic.cw_delay with evolve=True,
tref=0 and p_phase=None, with that function's keyword names, and an array form that sums any number of sources into
every pulsar of an array in one call. No third-party dependency; parity with enterprise_extensions itself is
unpinned: the definition is restated in include/fakepta_amd.h."""
import numpy as np

from fakepta import constants as const
from . import _capi

COLUMNS = ("cos_gwtheta", "gwphi", "cos_inc", "log10_mc", "log10_fgw", "log10_h", "phase0", "psi", "psrterm")
# Pulsar.add_cgw's argument names (the keys of signal_model['cgw'] entries), in COLUMNS order
ADD_CGW_KEYS = ("costheta", "phi", "cosinc", "log10_mc", "log10_fgw", "log10_h", "phase0", "psi", "psrterm")


def light_seconds(pdist, p_dist=1.0):
    """L = (pdist[0] + pdist[1] p_dist) kpc / c in seconds; a scalar pdist is a distance without uncertainty."""
    if np.ndim(pdist) == 0:
        return float(pdist) * const.kpc / const.c
    return (pdist[0] + pdist[1] * p_dist) * const.kpc / const.c


def source_table(sources):
    """[S, 9] float64 rows of COLUMNS from an [S, 9] array (or one row), or from a dict of scalars / equal-length
    arrays keyed by Pulsar.add_cgw's argument names (psrterm optional, default False)."""
    if isinstance(sources, dict):
        unknown = set(sources) - set(ADD_CGW_KEYS)
        if unknown:
            raise TypeError(f"unknown continuous-wave parameters {sorted(unknown)}; expected {ADD_CGW_KEYS}")
        missing = [k for k in ADD_CGW_KEYS[:-1] if k not in sources]
        if missing:
            raise TypeError(f"missing continuous-wave parameters {missing}")
        cols = [np.atleast_1d(np.asarray(sources[k], dtype=np.float64)) for k in ADD_CGW_KEYS[:-1]]
        cols.append(np.atleast_1d(np.asarray(sources.get("psrterm", False), dtype=bool)).astype(np.float64))
        n = max(len(c) for c in cols)
        if any(c.ndim != 1 or len(c) not in (1, n) for c in cols):
            raise ValueError("continuous-wave parameters must be scalars or arrays of one length")
        return np.ascontiguousarray(np.stack([np.broadcast_to(c, (n,)) for c in cols], axis=1))
    tab = np.asarray(sources, dtype=np.float64)
    if tab.ndim == 1 and tab.size == len(COLUMNS):
        tab = tab[None, :]
    if tab.ndim != 2 or tab.shape[1] != len(COLUMNS):
        raise ValueError(f"sources must be [S, {len(COLUMNS)}] ({', '.join(COLUMNS)})")
    return np.ascontiguousarray(tab)


def population_tables(sources, n_real):
    """(n_tab, src_offs [n_tab + 1] int64, src [total, 9] float64): the source tables of a block of n_real
    realizations in the CSR form fpta_batch_cw_accumulate takes. sources is one table for every realization ([S, 9],
    one row, or a dict as for source_table: n_tab 1), an [n_real, S, 9] array, or a list of n_real tables [S_r, 9] of
    any lengths (an empty one included). Needs no device."""
    n_real = int(n_real)
    if n_real < 1:
        raise ValueError(f"population_tables: n_real must be >= 1, got {n_real}")
    ncol = len(COLUMNS)
    per_real = None
    if isinstance(sources, dict):
        tab = source_table(sources)
    elif isinstance(sources, (list, tuple)) and len(sources) and all(
            np.ndim(t) == 2 or np.size(t) == 0 for t in sources):
        per_real = [np.zeros((0, ncol)) if np.size(t) == 0 else source_table(t) for t in sources]
    else:
        arr = np.asarray(sources, dtype=np.float64)
        if arr.ndim == 3:
            if arr.shape[2] != ncol:
                raise ValueError(f"population_tables: sources [R, S, {ncol}] expected, got {arr.shape}")
            per_real = list(arr)
        else:
            tab = source_table(arr)
    if per_real is None:
        return 1, np.array([0, len(tab)], dtype=np.int64), tab
    if len(per_real) != n_real:
        raise ValueError(f"population_tables: {len(per_real)} source tables for {n_real} realizations")
    offs = np.concatenate([[0], np.cumsum([len(t) for t in per_real])]).astype(np.int64)
    src = np.concatenate(per_real, axis=0) if offs[-1] else np.zeros((0, ncol))
    return n_real, offs, np.ascontiguousarray(src, dtype=np.float64)


def accumulate(toas_list, pos_list, L_list, sources, residuals, sign=1.0):
    """residuals (concatenated over the pulsars, float64, in place) += sign * sum over sources of the delay."""
    offs = np.concatenate([[0], np.cumsum([len(t) for t in toas_list])]).astype(np.int64)
    toas = np.concatenate([np.asarray(t, dtype=np.float64) for t in toas_list])
    pos = np.array([np.asarray(p, dtype=np.float64) for p in pos_list]).reshape(-1, 3)
    _capi.get_context().cw_accumulate(offs, toas, pos, np.asarray(L_list, dtype=np.float64), source_table(sources),
                                      residuals, sign=sign)
    return offs


def cw_delay(toas, pos, pdist, cos_gwtheta=0, gwphi=0, cos_inc=0, log10_mc=9, log10_fgw=-8, log10_dist=None,
             log10_h=None, phase0=0, psi=0, psrTerm=False, p_dist=1, evolve=True):
    """Delay [s] of one source at `toas` [s] for the pulsar at unit vector `pos`, distance pdist = (mean, sigma) kpc.
    Give the amplitude as log10_h (strain) or log10_dist (luminosity distance in Mpc). Returns a new array."""
    if not evolve:
        raise NotImplementedError("cw_delay: only evolve=True (the form Pulsar.add_cgw injects) is implemented")
    if (log10_h is None) == (log10_dist is None):
        raise ValueError("cw_delay: give exactly one of log10_h and log10_dist")
    if log10_h is None:
        # dist = 2 mc^(5/3) w0^(2/3) / h  ->  h for the given distance
        mc = 10 ** log10_mc * const.Tsun
        w0 = np.pi * 10 ** log10_fgw
        dist = 10 ** log10_dist * const.Mpc / const.c
        log10_h = np.log10(2 * mc ** (5 / 3) * w0 ** (2 / 3) / dist)
    toas = np.asarray(toas, dtype=np.float64)
    out = np.zeros(len(toas))
    row = [cos_gwtheta, gwphi, cos_inc, log10_mc, log10_fgw, log10_h, phase0, psi, float(bool(psrTerm))]
    accumulate([toas], [pos], [light_seconds(pdist, p_dist)], row, out)
    return out


def cw_delay_array(psrs, sources, sign=1.0):
    """sign * (sum over `sources` of the delay) for every pulsar of `psrs` (objects with toas, pos, pdist) in one
    call; sources as for source_table. Returns the list of per-pulsar arrays."""
    tab = source_table(sources)
    out = np.zeros(sum(len(p.toas) for p in psrs))
    offs = accumulate([p.toas for p in psrs], [p.pos for p in psrs], [light_seconds(p.pdist) for p in psrs], tab,
                      out, sign=sign)
    return [out[offs[i]:offs[i + 1]].copy() for i in range(len(psrs))]
