"""Solar-system ephemeris and Roemer delay on the GPU (fpta_ephem_kepler, fpta_ephem_orbits,
fpta_roemer_accumulate, csrc/ephem.hip): Keplerian orbits with linearly drifting elements for any number of bodies,
and the Roemer delay of ephemeris errors for a whole array in one call. fakepta.ephemeris.Ephemeris is the
reference's class on top of this module. The definition is restated in include/fakepta_amd.h."""
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
