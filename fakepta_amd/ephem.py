"""Solar-system ephemeris and Roemer delay on the GPU (fpta_ephem_kepler, fpta_ephem_orbits,
fpta_roemer_accumulate, csrc/ephem.hip): Keplerian orbits with linearly drifting elements for any number of bodies,
and the Roemer delay of ephemeris errors for a whole array in one call. fakepta.ephemeris.Ephemeris is the
reference's class on top of this module. perturbation_tables makes the per-realization row tables that
BatchSimulator.add_roemer_delay (fpta_batch_roemer_accumulate, csrc/roemer_batch.hip) injects into a resident block.
The definition is restated in include/fakepta_amd.h."""
import numpy as np

from . import _capi

# a body row of the C entry points: the keys of an Ephemeris.planets entry, value then rate per century
ELEMENTS = ("inc", "Om", "omega", "a", "e", "l0")
BODY_COLUMNS = ("mass", "T") + tuple(c for k in ELEMENTS for c in (k, k + "_rate"))
DEVIATIONS = ("d_mass", "d_Om", "d_omega", "d_inc", "d_a", "d_e", "d_l0")
ROW_COLUMNS = BODY_COLUMNS + DEVIATIONS + ("inv_mass_ss",)
assert len(BODY_COLUMNS) == _capi.EPHEM_NBODY and len(ROW_COLUMNS) == _capi.ROEMER_NPAR


def body_row(planet):
    """[14] float64 row from an Ephemeris.planets entry (a dict with mass, T and a (value, rate) pair per element).
    a = None becomes (0, 0), which the library resolves to the Kepler-law value of T."""
    row = [float(planet["mass"]), float(planet["T"])]
    for k in ELEMENTS:
        v = planet[k]
        if v is None:
            if k != "a":
                raise ValueError(f"only the semi-major axis may be None, not {k!r}")
            v = (0.0, 0.0)
        if len(v) != 2:
            raise ValueError(f"element {k!r} must be a (value, rate per century) pair")
        row += [float(v[0]), float(v[1])]
    return np.array(row, dtype=np.float64)


def body_table(bodies):
    """[B, 14] float64 table from a dict of planets (in its order), a list of planet dicts or rows, or an array."""
    if isinstance(bodies, dict):
        bodies = list(bodies.values())
    if isinstance(bodies, np.ndarray):
        tab = np.asarray(bodies, dtype=np.float64)
        if tab.ndim == 1 and tab.size == len(BODY_COLUMNS):
            tab = tab[None, :]
    else:
        rows = [body_row(b) if isinstance(b, dict) else np.asarray(b, dtype=np.float64) for b in bodies]
        tab = np.array(rows, dtype=np.float64).reshape(len(rows), -1) if rows else np.zeros((0, len(BODY_COLUMNS)))
    if tab.ndim != 2 or tab.shape[1] != len(BODY_COLUMNS):
        raise ValueError(f"bodies must be [B, {len(BODY_COLUMNS)}] ({', '.join(BODY_COLUMNS)})")
    return np.ascontiguousarray(tab)


def roemer_row(body, mass_ss, d_mass=0., d_Om=0., d_omega=0., d_inc=0., d_a=0., d_e=0., d_l0=0.):
    """[22] float64 row: the body (a planet dict or a 14-row), the seven deviations, 1 / mass_ss."""
    b = body_row(body) if isinstance(body, dict) else np.asarray(body, dtype=np.float64)
    if b.shape != (len(BODY_COLUMNS),):
        raise ValueError(f"a body is {len(BODY_COLUMNS)} values")
    dev = [float(d_mass), float(d_Om), float(d_omega), float(d_inc), float(d_a), float(d_e), float(d_l0)]
    return np.concatenate([b, dev, [1.0 / float(mass_ss)]])


def row_table(rows):
    tab = np.asarray(rows, dtype=np.float64)
    if tab.ndim == 1 and tab.size == len(ROW_COLUMNS):
        tab = tab[None, :]
    if tab.ndim != 2 or tab.shape[1] != len(ROW_COLUMNS):
        raise ValueError(f"rows must be [R, {len(ROW_COLUMNS)}] ({', '.join(ROW_COLUMNS)})")
    return np.ascontiguousarray(tab)


def _is_perturbation(x):
    return isinstance(x, (tuple, list)) and len(x) == 2 and isinstance(x[1], dict)


def _one_table(tab, ephem):
    """[n, 22] from rows or from a list of (planet, deviations); anything empty is the empty table."""
    if isinstance(tab, (list, tuple)) and len(tab) and all(_is_perturbation(x) for x in tab):
        if ephem is None:
            raise ValueError("perturbation_tables: planets given by name need an Ephemeris (ephem=)")
        return row_table([ephem.roemer_row(planet, **dev) for planet, dev in tab])
    if np.size(tab) == 0:
        return np.zeros((0, len(ROW_COLUMNS)))
    return row_table(tab)


def _is_table(x):
    if isinstance(x, (list, tuple)) and len(x) and all(_is_perturbation(p) for p in x):
        return True
    return np.size(x) == 0 or np.ndim(x) == 2


def perturbation_tables(perts, R, ephem=None):
    """(n_tab, row_offs [n_tab + 1] int64, rows [total, 22] float64): the row tables of a block of R realizations in the
    CSR form fpta_batch_roemer_accumulate takes. perts is one table for every realization (an [n, 22] array of
    ROW_COLUMNS rows, one row, or a list of (planet, deviations) as add_roemer_delay_array takes, resolved through
    ephem.roemer_row: n_tab 1), an [R, n, 22] array, or a list of R tables of either form and any lengths (an empty
    one included). Needs no device."""
    R = int(R)
    if R < 1:
        raise ValueError(f"perturbation_tables: R must be >= 1, got {R}")
    ncol = len(ROW_COLUMNS)
    per_real = None
    if isinstance(perts, (list, tuple)) and len(perts) and all(_is_perturbation(x) for x in perts):
        tab = _one_table(perts, ephem)
    elif isinstance(perts, (list, tuple)) and len(perts) and all(_is_table(t) for t in perts):
        per_real = [_one_table(t, ephem) for t in perts]
    else:
        arr = np.asarray(perts, dtype=np.float64)
        if arr.ndim == 3:
            if arr.shape[2] != ncol:
                raise ValueError(f"perturbation_tables: rows [R, n, {ncol}] expected, got {arr.shape}")
            per_real = list(arr)
        elif arr.ndim > 3:
            raise ValueError(f"perturbation_tables: rows [n, {ncol}] or [R, n, {ncol}] expected, got {arr.shape}")
        else:
            tab = _one_table(arr, ephem)
    if per_real is None:
        return 1, np.array([0, len(tab)], dtype=np.int64), tab
    if len(per_real) != R:
        raise ValueError(f"perturbation_tables: {len(per_real)} tables for {R} realizations")
    offs = np.concatenate([[0], np.cumsum([len(t) for t in per_real])]).astype(np.int64)
    rows = np.concatenate(per_real, axis=0) if offs[-1] else np.zeros((0, ncol))
    return R, offs, np.ascontiguousarray(rows, dtype=np.float64)


def kepler(M, e):
    """Eccentric anomaly E with E - e sin E = M, elementwise (0 <= e <= _capi.EPHEM_E_MAX)."""
    return _capi.get_context().ephem_kepler(M, e)


def planet_ssb(toas, bodies):
    """[n, B, 6]: position [light-seconds, equatorial] of every body in columns 0 .. 2, zeros in 3 .. 5."""
    return _capi.get_context().ephem_orbits(toas, body_table(bodies), planets=True, sun=False)[0]


def sun_ssb(toas, bodies):
    """[n, 3]: -sum over the bodies of mass / Msun x position, summed in table order."""
    return _capi.get_context().ephem_orbits(toas, body_table(bodies), planets=False, sun=True)[1]


def accumulate(toas_list, pos_list, rows, out, sign=1.0, separate=False):
    """out (concatenated over the pulsars, float64, in place) += sign * sum over rows of the delay; with separate,
    out [R, n] = sign * each row's delay. Returns the pulsars' offsets into out."""
    offs = np.concatenate([[0], np.cumsum([len(t) for t in toas_list])]).astype(np.int64)
    toas = np.concatenate([np.asarray(t, dtype=np.float64) for t in toas_list]) if len(toas_list) else np.zeros(0)
    pos = np.array([np.asarray(p, dtype=np.float64) for p in pos_list]).reshape(-1, 3)
    _capi.get_context().roemer_accumulate(offs, toas, pos, row_table(rows), out, sign=sign, separate=separate)
    return offs


def roemer_delay_array(psrs, rows, sign=1.0, separate=False):
    """sign * (sum over `rows` of the Roemer delay) for every pulsar of `psrs` (objects with toas and pos) in one call:
    the list of per-pulsar arrays. With separate=True every row's own delay: per pulsar an [R, n_toa] array, so N
    draws of the deviations give N delay vectors from one launch."""
    tab = row_table(rows)
    n = sum(len(p.toas) for p in psrs)
    out = np.zeros((len(tab), n) if separate else n)
    offs = accumulate([p.toas for p in psrs], [p.pos for p in psrs], tab, out, sign=sign, separate=separate)
    return [out[..., offs[i]:offs[i + 1]].copy() for i in range(len(psrs))]
