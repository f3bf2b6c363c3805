"""Fourier fit: the Fourier coefficients of residuals on the device (fpta_batch_set_fit, fpta_batch_fit,
fpta_batch_fit_cross, fpta_fit_coefficients; the definition is in include/fakepta_amd.h). The helpers here turn a
component list into the tables the library reads and coefficients into spectra; BatchSimulator.set_fourier_fit /
fourier_fit / power_spectrum / cross_spectrum and the drop-in Pulsar.fit_fourier / fit_fourier_array share them."""
import numpy as np

from . import _capi
from . import tm as _tm

MAX_COMP, MAX_COEF = _capi.FIT_MAX_COMP, _capi.FIT_MAX_COEF


def delta_f(f):
    """diff(append(0, f)) along the last axis: the bin widths of signal_model[...]['psd']."""
    f = np.asarray(f, dtype=np.float64)
    return np.diff(np.concatenate([np.zeros(f.shape[:-1] + (1,)), f], axis=-1), axis=-1)


def resolve_components(components, n_psr, tspan, segments=(), common=None, freqf=1400.0):
    """A component list -> (n_modes [C] int32, f [sum N] or [P, sum N], idx [C], freqf [C]).

    components: None (one achromatic component of 30 modes), or a list whose entries are a signal name of `segments`
    (BatchSimulator.segments: its f, idx and freqf), or (n_modes, idx) for the grid k / tspan, k = 1 .. n_modes, or
    (f, idx) with f [N] for the whole array or [P, N]. common: None keeps one grid for the array when every component
    has one, True insists on it, False gives every pulsar its own copy."""
    if components is None:
        components = [(30, 0.0)]
    if isinstance(components, (str, tuple)):
        components = [components]
    components = list(components)
    if not 1 <= len(components) <= MAX_COMP:
        raise ValueError(f"a Fourier fit takes 1 .. {MAX_COMP} components, got {len(components)}")
    fs, idxs, refs = [], [], []
    for i, comp in enumerate(components):
        if isinstance(comp, str):
            seg = [s for s in segments if s["name"] == comp]
            if not seg:
                raise KeyError(f"component {i}: the layout has no signal {comp!r}")
            f, idx, ref = np.asarray(seg[0]["f"], dtype=np.float64), float(seg[0]["idx"]), float(seg[0]["freqf"])
        else:
            try:
                spec, idx = comp
            except (TypeError, ValueError):
                raise ValueError(f"component {i} must be a signal name or (n_modes or f, idx), got {comp!r}") from None
            idx, ref = float(idx), float(freqf)
            if np.ndim(spec) == 0:
                n = int(spec)
                if n != spec or n < 1:
                    raise ValueError(f"component {i}: the mode count must be a positive integer, got {spec!r}")
                if not tspan > 0:
                    raise ValueError(f"component {i}: the grid k / Tspan needs a positive span, got {tspan}")
                f = np.arange(1, n + 1) / float(tspan)
            else:
                f = np.asarray(spec, dtype=np.float64)
        if f.ndim not in (1, 2) or f.shape[-1] < 1 or (f.ndim == 2 and f.shape[0] != n_psr):
            raise ValueError(f"component {i}: f must be [N] or [{n_psr}, N], got shape {f.shape}")
        if not np.all(np.isfinite(f) & (f > 0)):
            raise ValueError(f"component {i}: every frequency must be positive and finite")
        if not np.isfinite(idx):
            raise ValueError(f"component {i}: the chromatic index must be finite")
        fs.append(f)
        idxs.append(idx)
        refs.append(ref)
    per_psr = any(f.ndim == 2 for f in fs)
    if common and per_psr:
        raise ValueError("common=True, but a component has per-pulsar frequencies")
    if per_psr or common is False:
        fs = [f if f.ndim == 2 else np.tile(f, (n_psr, 1)) for f in fs]
    n_modes = np.array([f.shape[-1] for f in fs], dtype=np.int32)
    if 2 * int(n_modes.sum()) > MAX_COEF:
        raise ValueError(f"{2 * int(n_modes.sum())} Fourier columns, more than {MAX_COEF}")
    return n_modes, np.ascontiguousarray(np.concatenate(fs, axis=-1)), np.array(idxs), np.array(refs)


def split_components(n_modes):
    """Per component (first cosine row, first sine row, N) of the K = sum 2 N coefficient rows."""
    out, k0 = [], 0
    for n in n_modes:
        out.append((k0, k0 + int(n), int(n)))
        k0 += 2 * int(n)
    return out


def power_spectrum(coef, n_modes, f):
    """coef [P, K, R] -> per component [P, N_c]: the mean over realizations of (a_cos^2 + a_sin^2) / (2 df), df =
    diff(append(0, f)) of the component's own frequencies: the units of signal_model[...]['psd']. f: [sum N] or
    [P, sum N]."""
    coef = np.asarray(coef, dtype=np.float64)
    f = np.asarray(f, dtype=np.float64)
    out, m0 = [], 0
    for c0, s0, n in split_components(n_modes):
        df = delta_f(f[..., m0:m0 + n])
        p2 = np.mean(coef[:, c0:c0 + n] ** 2 + coef[:, s0:s0 + n] ** 2, axis=2)
        out.append(p2 / (2.0 * df))
        m0 += n
    return out


def mode_delta_f(n_modes, f):
    """df of every mode of a common grid f [sum N], component by component."""
    f = np.asarray(f, dtype=np.float64)
    out, m0 = [], 0
    for n in n_modes:
        out.append(delta_f(f[m0:m0 + int(n)]))
        m0 += int(n)
    return np.concatenate(out)


def coefficients(offs, toas, nu, components, res, Mmats=None, weights=None, rcond=None, tspan=None, common=None,
                 freqf=1400.0, ctx=None):
    """One call for any array: the Fourier coefficients of res [n_vec, n_toa] or [n_toa]. Returns (n_modes, f, coef
    [P, K, n_vec], kept Fourier columns [P], kept mask [P, K]). freqf: the reference radio frequency of the
    components given as (n_modes or f, idx)."""
    offs = np.asarray(offs, dtype=np.int64)
    toas = np.asarray(toas, dtype=np.float64)
    if tspan is None:
        tspan = float(np.ptp(toas)) if len(toas) else 0.0
    n_modes, f, idx, freqf = resolve_components(components, len(offs) - 1, tspan, common=common, freqf=freqf)
    M, ncol = _tm.stack_design(Mmats) if Mmats is not None else (None, None)
    ctx = ctx if ctx is not None else _capi.get_context()
    coef, rank, kept = ctx.fit_coefficients(offs, toas, nu, n_modes, f, idx, freqf, res, M=M, ncol_psr=ncol,
                                            weights=weights, rcond=rcond)
    return n_modes, f, coef, rank, kept
