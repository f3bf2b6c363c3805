"""Per-realization spectra of a batch block, host side: spectrum_tables() turns what a user says about the signals'
spectra ({name: dict(psd=...) | dict(amp=...) | dict(log10_A=..., gamma=...)}) into the flat arrays of
fpta_batch_synth_spectra (include/fakepta_amd.h). Nothing here touches a device: the layout is read from the
simulator's host copy (BatchSimulator.segments), and every shape, the zero rule and every bad entry is refused here
by name before the library sees the call (it checks again, by signal id)."""
import numpy as np

FORM_AMP, FORM_POWERLAW = 0, 1


def _df(f):
    return np.diff(np.concatenate([np.zeros(f.shape[:-1] + (1,)), f], axis=-1), axis=-1)


def _first(mask):
    return tuple(int(i) for i in np.argwhere(mask)[0])


def _where(idx, per_pulsar, mode=True):
    """'realization r, pulsar p, mode k' of an index into [R, N], [R, P, N], [R] or [R, P]."""
    parts = [f"realization {idx[0]}"]
    if per_pulsar:
        parts.append(f"pulsar {idx[1]}")
    if mode:
        parts.append(f"mode {idx[-1]}")
    return ", ".join(parts)


def _amp_table(who, seg, spec, key, n_real, P):
    kind, N = seg["kind"], seg["f"].shape[-1]
    lay = np.asarray(seg["amp"], dtype=np.float64)  # [N] or [P, N]
    v = np.asarray(spec[key], dtype=np.float64)
    if v.ndim == 0 or v.shape[-1] != N:
        raise ValueError(f"{who}: {key} must end in the signal's {N} modes, got shape {v.shape}")
    if v.ndim > 3:
        raise ValueError(f"{who}: {key} has too many axes {v.shape}")
    if v.ndim == 3 and kind == 1:
        raise ValueError(f"{who}: a per-pulsar table [R, P, N] for a common signal")
    if v.ndim == 3 and v.shape[1] != P:
        raise ValueError(f"{who}: {key} has {v.shape[1]} pulsars, the layout {P}")
    if v.ndim >= 2 and v.shape[0] != n_real:
        raise ValueError(f"{who}: {v.shape[0]} rows for {n_real} realizations")
    per = v.ndim == 3
    if v.ndim == 1:
        v = np.broadcast_to(v, (n_real, N))
    what = "amplitude" if key == "amp" else "psd"
    if not np.all(np.isfinite(v)):
        raise ValueError(f"{who}: {_where(_first(~np.isfinite(v)), per)}: non-finite {what}")
    if np.any(v < 0):
        raise ValueError(f"{who}: {_where(_first(v < 0), per)}: negative {what}")
    if key == "psd":
        # the units of signal_model[...]['psd']: amp = sqrt(psd * df) on the signal's own frequencies; a row shared by
        # the pulsars of a per-pulsar signal takes each pulsar's own df
        df = _df(np.asarray(seg["f"], dtype=np.float64))
        shared = kind == 0 and not per
        if shared:
            v, per = v[:, None, :], True
        v = np.sqrt(v * df)
        if shared:
            v = np.where(lay == 0.0, 0.0, v)  # a shared row does not reach the pulsars that lack the signal
    zero = lay == 0.0 if (per or kind == 1) else np.all(lay == 0.0, axis=0)
    bad = (v != 0.0) & zero
    if np.any(bad):
        raise ValueError(f"{who}: {_where(_first(bad), per)}: nonzero amplitude where the layout's is 0")
    return FORM_AMP, int(per), np.ascontiguousarray(v, dtype=np.float64)


def _powerlaw_table(who, seg, spec, n_real, P):
    kind = seg["kind"]
    a, g = (np.asarray(spec[k], dtype=np.float64) for k in ("log10_A", "gamma"))
    for k, v in (("log10_A", a), ("gamma", g)):
        if v.ndim > 2:
            raise ValueError(f"{who}: {k} must be a scalar, [R] or [R, P], got shape {v.shape}")
        if v.ndim == 2 and kind == 1:
            raise ValueError(f"{who}: a per-pulsar table [R, P] for a common signal")
        if v.ndim >= 1 and v.shape[0] != n_real:
            raise ValueError(f"{who}: {v.shape[0]} rows for {n_real} realizations")
        if v.ndim == 2 and v.shape[1] != P:
            raise ValueError(f"{who}: {k} has {v.shape[1]} pulsars, the layout {P}")
    per = a.ndim == 2 or g.ndim == 2
    shape = (n_real, P) if per else (n_real,)
    a, g = (np.broadcast_to(v[:, None] if (per and v.ndim == 1) else v, shape) for v in (a, g))
    for k, v in (("log10_A", a), ("gamma", g)):
        if not np.all(np.isfinite(v)):
            raise ValueError(f"{who}: {_where(_first(~np.isfinite(v)), per, mode=False)}: non-finite {k}")
    return FORM_POWERLAW, int(per), np.ascontiguousarray(np.stack([a, g], axis=-1), dtype=np.float64)


def spectrum_tables(sim, spectra, n_real):
    """(seg, form, per_pulsar, tables) of fpta_batch_synth_spectra for a block of n_real realizations.

    sim:     a BatchSimulator (only its host copy of the layout, sim.segments and sim.psrs, is read).
    spectra: {signal: spec} with signal a name of the layout (or its id) and spec one of
             dict(amp=a)    coefficient standard deviations sqrt(psd * df): [N] (every realization), [R, N] (a common
                            signal, or a per-pulsar signal whose pulsars share the row) or [R, P, N] (a per-pulsar
                            signal only); N is the signal's mode count;
             dict(psd=s)    the same shapes in the units of signal_model[...]['psd']: amp = sqrt(psd * df) on the
                            signal's own frequencies, so any PSD model of fakepta.spectrum serves;
             dict(log10_A=, gamma=)  power-law parameters, each a scalar, [R] or (per-pulsar signals) [R, P]: the
                            device evaluates sqrt(spectrum.powerlaw(f, log10_A, gamma) * df).
    A mode whose layout amplitude is exactly 0 stays 0: a shared row simply does not reach it, an explicit [R, P, N]
    entry there must be 0. ValueError names the signal and the first bad entry."""
    n_real = int(n_real)
    if n_real <= 0:
        raise ValueError("spectrum_tables: n_real must be > 0")
    if not hasattr(spectra, "items"):
        raise TypeError("spectrum_tables: spectra must be a dict {signal: dict(...)}")
    P = len(sim.psrs)
    segs = sim.segments
    out, seen = [], set()
    for name, spec in spectra.items():
        who = f"spectra[{name!r}]"
        if isinstance(name, (int, np.integer)):
            hit = [s for s in segs if s["id"] == int(name)]
        else:
            hit = [s for s in segs if s["name"] == name]
        if not hit:
            raise ValueError(f"{who}: unknown signal (the layout has {[s['name'] for s in segs]})")
        if len(hit) > 1:
            raise ValueError(f"{who}: the layout has {len(hit)} signals of that name; give the id")
        seg = hit[0]
        if seg["id"] in seen:
            raise ValueError(f"{who}: more than one table for signal {seg['name']!r}")
        seen.add(seg["id"])
        if not hasattr(spec, "keys"):
            raise TypeError(f"{who}: expected dict(psd=...), dict(amp=...) or dict(log10_A=..., gamma=...)")
        keys = set(spec.keys())
        if keys == {"amp"} or keys == {"psd"}:
            form, per, tab = _amp_table(who, seg, spec, next(iter(keys)), n_real, P)
        elif keys == {"log10_A", "gamma"}:
            form, per, tab = _powerlaw_table(who, seg, spec, n_real, P)
        else:
            raise ValueError(f"{who}: expected psd, amp or (log10_A, gamma), got {sorted(keys)}")
        out.append((seg["id"], form, per, tab))
    out.sort(key=lambda t: t[0])
    return ([t[0] for t in out], [t[1] for t in out], [t[2] for t in out], [t[3] for t in out])


def slice_spectra(spectra, lo, n):
    """Rows [lo, lo + n) of every array of a spectra dict that has a realization axis (more than one axis for psd / amp,
    at least one for log10_A / gamma); the rest is kept."""
    out = {}
    for name, spec in spectra.items():
        part = {}
        for k, v in spec.items():
            v = np.asarray(v)
            has_r = v.ndim >= (2 if k in ("amp", "psd") else 1)
            part[k] = v[lo:lo + n] if has_r else v
        out[name] = part
    return out
