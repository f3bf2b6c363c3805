"""Reference evaluations of the solar-system ephemeris and Roemer delay of fpta_ephem_* / fpta_roemer_accumulate,
restated from the definition in include/fakepta_amd.h:

  kepler_newton    numpy model of the device's Kepler solve, iteration for iteration (same start, same stopping
                   rule, same cap): the CPU tests sweep it over (M, e) to prove the cap is never reached
  orbit_numpy      the literal fp64 numpy evaluation of the definition, term by term (the yardstick of what fp64
  roemer_numpy     achieves, not a target); the Kepler solve inside is kepler_newton
  kepler_mp        the same definition in mpmath at 50 digits, rounded to fp64 at the end: the truth of the fixture
  orbit_mp         tests/golden/g11_ephem.npz (tools/gen_ephem_golden.py)
  roemer_mp

All take the fp64 inputs exactly as given. A body is a row of BODY_COLUMNS, a Roemer row a row of ROW_COLUMNS, the
layouts of the C entry points."""
import numpy as np

from fakepta import constants as const

BODY_COLUMNS = ("mass", "T", "inc", "inc_rate", "Om", "Om_rate", "omega", "omega_rate", "a", "a_rate", "e", "e_rate",
                "l0", "l0_rate")
DEVIATIONS = ("d_mass", "d_Om", "d_omega", "d_inc", "d_a", "d_e", "d_l0")
ROW_COLUMNS = BODY_COLUMNS + DEVIATIONS + ("inv_mass_ss",)
N_BODY_COL, N_ROW_COL = len(BODY_COLUMNS), len(ROW_COLUMNS)  # FPTA_EPHEM_NBODY, FPTA_ROEMER_NPAR
I_MASS, I_T, I_INC, I_OM, I_OMEGA, I_A, I_E, I_L0 = 0, 1, 2, 4, 6, 8, 10, 12
# column of the element value each deviation is added to (d_mass: the mass)
DEVIATION_COLUMN = dict(d_mass=I_MASS, d_Om=I_OM, d_omega=I_OMEGA, d_inc=I_INC, d_a=I_A, d_e=I_E, d_l0=I_L0)

OBLIQUITY_DEG = 23.43928
MJD_J2000 = 51544.5
# the device's Kepler solve (csrc/ephem.hip kepler_solve), mirrored by kepler_newton below
E_MAX = 0.95            # FPTA_EPHEM_E_MAX: the largest admitted eccentricity
KEPLER_LOW_E = 0.5      # below: start at M + e sin M; from there on: start at pi (monotone for every e < 1)
KEPLER_TOL = 1e-10      # stop after the first step no longer than this: the next one would be < 4 tol^2
KEPLER_MAX_ITER = 12    # the cap; tests/test_ephem_host.py proves the model needs fewer for every admitted (M, e)


def centuries(toas):
    """Julian centuries from J2000 of TOAs in MJD seconds."""
    return (np.asarray(toas, dtype=np.float64) / 86400.0 - MJD_J2000) / 36525.0


def kepler_a_au(T_days):
    """Semi-major axis [AU] of period T [days] around the Sun: what a = None stands for."""
    return (const.GMsun * (T_days * const.day) ** 2 / (4 * np.pi ** 2)) ** (1 / 3) / const.AU


def resolve_bodies(bodies):
    """Copy of a body table [B, 14] with every a = None entry (value 0 and rate 0) replaced by kepler_a_au(T)."""
    tab = np.array(bodies, dtype=np.float64).reshape(-1, N_BODY_COL)
    none = (tab[:, I_A] == 0.0) & (tab[:, I_A + 1] == 0.0)
    tab[none, I_A] = kepler_a_au(tab[none, I_T])
    return tab


def kepler_newton(M, e, max_iter=KEPLER_MAX_ITER, return_iterations=False):
    """E with E - e sin E = M for M in [0, 2 pi), by the device's iteration. With return_iterations also the number
    of Newton steps each element took; max_iter + 1 marks an element that never met the stopping rule."""
    M, e = np.broadcast_arrays(np.asarray(M, dtype=np.float64), np.asarray(e, dtype=np.float64))
    E = np.where(e < KEPLER_LOW_E, M + e * np.sin(M), np.pi)
    live = np.ones(M.shape, dtype=bool)
    iters = np.zeros(M.shape, dtype=np.int64)
    for _ in range(max_iter):
        s, c = np.sin(E), np.cos(E)
        dE = ((E - e * s) - M) / (1.0 - e * c)
        E = np.where(live, E - dE, E)
        iters += live
        live &= ~(np.abs(dE) <= KEPLER_TOL)
        if not live.any():
            break
    iters[live] = max_iter + 1
    return (E, iters) if return_iterations else E


def _rotate(x, y, Om_deg, w_deg, inc_deg, cos, sin, pi):
    Om, w, inc, ec = Om_deg * (pi / 180), w_deg * (pi / 180), inc_deg * (pi / 180), OBLIQUITY_DEG * pi / 180
    X = (cos(Om) * cos(w) - sin(Om) * cos(inc) * sin(w)) * x + (-cos(Om) * sin(w) - sin(Om) * cos(inc) * cos(w)) * y
    Y = (sin(Om) * cos(w) + cos(Om) * cos(inc) * sin(w)) * x + (-sin(Om) * sin(w) + cos(Om) * cos(inc) * cos(w)) * y
    Z = sin(inc) * sin(w) * x + sin(inc) * cos(w) * y
    return X, cos(ec) * Y - sin(ec) * Z, sin(ec) * Y + cos(ec) * Z


def orbit_numpy(toas, body):
    """[n, 3] position [light-seconds, equatorial] of one resolved body row at the TOAs, in plain fp64."""
    b = np.asarray(body, dtype=np.float64)
    t = centuries(toas)
    inc, Om, omega = b[I_INC] + b[I_INC + 1] * t, b[I_OM] + b[I_OM + 1] * t, b[I_OMEGA] + b[I_OMEGA + 1] * t
    a = (b[I_A] + b[I_A + 1] * t) * const.AU / const.c
    e = b[I_E] + b[I_E + 1] * t
    l0 = b[I_L0] + b[I_L0 + 1] * t
    M = np.mod((l0 - omega) * np.pi / 180, 2 * np.pi)
    E = kepler_newton(M, e)
    x = a * np.cos(E - e)
    y = a * np.sqrt(1 - e ** 2) * np.sin(E)
    return np.stack(_rotate(x, y, Om, omega - Om, inc, np.cos, np.sin, np.pi), axis=-1)


def sun_numpy(toas, bodies):
    out = np.zeros((len(toas), 3))
    for b in resolve_bodies(bodies):
        out -= b[I_MASS] / const.Msun * orbit_numpy(toas, b)
    return out


def perturbed(row):
    """The body of a Roemer row with its six element deviations added to the element values."""
    row = np.asarray(row, dtype=np.float64)
    b = row[:N_BODY_COL].copy()
    for k, name in enumerate(DEVIATIONS):
        if name != "d_mass":
            b[DEVIATION_COLUMN[name]] += row[N_BODY_COL + k]
    return b


def roemer_numpy(toas, pos, row):
    row = np.asarray(row, dtype=np.float64)
    base = resolve_bodies(row[:N_BODY_COL])[0]
    full = row.copy()
    full[:N_BODY_COL] = base
    mass, d_mass = row[I_MASS], row[N_BODY_COL]
    d_ssb = ((mass + d_mass) * orbit_numpy(toas, perturbed(full)) - mass * orbit_numpy(toas, base)) * row[-1]
    return d_ssb @ np.asarray(pos, dtype=np.float64)


# ----------------------------------------------------------------------------- mpmath truth
def _mp():
    import mpmath as mp
    return mp


def kepler_mp(M, e, dps=50):
    """E - e sin E = M in mpmath (Newton from pi, monotone, then to the working precision); fp64 out."""
    mp = _mp()
    out = np.empty(len(M))
    with mp.workdps(dps):
        for i, (m, ee) in enumerate(zip(np.asarray(M, float), np.broadcast_to(np.asarray(e, float), len(M)))):
            out[i] = float(_kepler_mp(mp, mp.mpf(float(m)), mp.mpf(float(ee))))
    return out


def _kepler_mp(mp, M, e):
    E = mp.pi
    tol = mp.mpf(10) ** (-(mp.mp.dps - 5))
    for _ in range(200):
        dE = (E - e * mp.sin(E) - M) / (1 - e * mp.cos(E))
        E -= dE
        if abs(dE) < tol:
            return E
    raise RuntimeError("kepler_mp did not converge")


def _kepler_a_mp(mp, T_days):
    f = mp.mpf
    return mp.cbrt(f(const.GMsun) * (f(float(T_days)) * f(const.day)) ** 2 / (4 * mp.pi ** 2)) / f(const.AU)


def _orbit_mp(mp, toa, b, a_none):
    """Equatorial position of the fp64 body row b; an a = None row gets its Kepler-law value in mpmath too."""
    m = [mp.mpf(float(v)) for v in b]
    if a_none:
        m[I_A] = _kepler_a_mp(mp, b[I_T])
    return _orbit_mp_exact(mp, toa, m)


def _is_none(b):
    return float(b[I_A]) == 0.0 and float(b[I_A + 1]) == 0.0


def orbit_mp(toas, body, dps=50):
    """[n, 3] of one body row (a = None rows unresolved: the Kepler-law value is made in mpmath too)."""
    mp = _mp()
    out = np.empty((len(toas), 3))
    with mp.workdps(dps):
        for i, toa in enumerate(toas):
            out[i] = [float(v) for v in _orbit_mp(mp, toa, body, _is_none(body))]
    return out


def sun_mp(toas, bodies, dps=50):
    mp = _mp()
    out = np.empty((len(toas), 3))
    bodies = np.asarray(bodies, dtype=np.float64).reshape(-1, N_BODY_COL)
    with mp.workdps(dps):
        msun = mp.mpf(const.GMsun) / mp.mpf(const.G)
        for i, toa in enumerate(toas):
            acc = [mp.mpf(0)] * 3
            for b in bodies:
                o = _orbit_mp(mp, toa, b, _is_none(b))
                acc = [s - mp.mpf(float(b[I_MASS])) / msun * v for s, v in zip(acc, o)]
            out[i] = [float(v) for v in acc]
    return out


def roemer_mp(toas, pos, row, dps=50):
    mp = _mp()
    row = np.asarray(row, dtype=np.float64)
    base = row[:N_BODY_COL]
    none = _is_none(base)
    out = np.empty(len(toas))
    with mp.workdps(dps):
        f = mp.mpf
        pert = [f(float(v)) for v in base]
        if none:  # the deviation d_a is added to the Kepler-law value
            pert[I_A] = _kepler_a_mp(mp, base[I_T])
        for k, name in enumerate(DEVIATIONS):
            if name != "d_mass":
                pert[DEVIATION_COLUMN[name]] += f(float(row[N_BODY_COL + k]))
        mass, d_mass, inv = f(float(row[I_MASS])), f(float(row[N_BODY_COL])), f(float(row[-1]))
        p = [f(float(v)) for v in pos]
        for i, toa in enumerate(toas):
            o1 = _orbit_mp_exact(mp, toa, pert)
            o0 = _orbit_mp(mp, toa, base, none)
            out[i] = float(sum(((mass + d_mass) * u - mass * v) * inv * q for u, v, q in zip(o1, o0, p)))
    return out


def _orbit_mp_exact(mp, toa, b):
    """Equatorial position of a body row held as mpf values (a resolved)."""
    f = mp.mpf
    t = (f(float(toa)) / 86400 - f(MJD_J2000)) / 36525
    lin = lambda i: b[i] + b[i + 1] * t  # noqa: E731
    inc, Om, omega, e, l0 = lin(I_INC), lin(I_OM), lin(I_OMEGA), lin(I_E), lin(I_L0)
    a = lin(I_A) * f(const.AU) / f(const.c)
    M = (l0 - omega) * mp.pi / 180
    M -= 2 * mp.pi * mp.floor(M / (2 * mp.pi))
    E = _kepler_mp(mp, M, e)
    return _rotate(a * mp.cos(E - e), a * mp.sqrt(1 - e * e) * mp.sin(E), Om, omega - Om, inc, mp.cos, mp.sin, mp.pi)
