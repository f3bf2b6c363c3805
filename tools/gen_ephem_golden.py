"""Writes tests/golden/g11_ephem.npz, the fixture of the ephemeris tests (tests/test_ephem_host.py,
tests/test_gpu_ephem.py). Container-only, CPU only: it runs the reference's own Ephemeris (tools/ref_shim.py, with
matplotlib on the Agg backend) and needs mpmath and scipy.

  python tools/gen_ephem_golden.py

Geometry: five pulsars of 1, 63, 64, 65 and 130 TOAs (every side of a 64-TOA wave), sorted uniform draws over MJD
48000 - 60500, one of them replaced by J2000 exactly (51544.5 x 86400 s); many lie before it (negative t). Bodies:
the reference's eight planets, then three added with add_planet: body9 with a = None (T = 1500 d, e = 0.3), body10
with e = 0.6 + 0.01 t, body11 with e = 0.9. Stored, besides the inputs:
  truth            the definition of include/fakepta_amd.h in 50-digit mpmath, rounded to fp64 (tests/ephem_reference.py):
                   planet_truth [n, 11, 3], sun_truth [n, 3] (all eleven bodies), sun8_truth (the planets alone),
                   kepler_truth [7, 26], roemer_truth [12, n]
  err_ref64        max |literal fp64 numpy evaluation - truth|: err_planet [11], err_sun, err_sun8, err_kepler [7],
                   err_roemer [12]; a zero is floored at one ulp of its group's largest |truth|. The tests' yardstick.
  reference output ref_planet [n, 11, 3] (get_orbit_planet), ref_sun8 / ref_sun (get_sunssb without / with the added
                   bodies), ref_roemer [4, n] (roemer_delay of the four d_mass-only rows), each from a fresh Ephemeris
                   per call and per pulsar, and the reference's planet table ref_table [8, 14], ref_names, ref_mass_ss.
The generator fails if any reference output is further than 2.5e-11 max |truth| from the truth: it never widens."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))

N_TOA = (1, 63, 64, 65, 130)
MJD0, MJD1 = 48000.0, 60500.0
J2000_S = 51544.5 * 86400.0
REF_TOL = 2.5e-11
ELEMENTS = ("inc", "Om", "omega", "a", "e", "l0")
EXTRA = (  # name, mass, T, inc, Om, omega, a, e, l0
    ("body9", 1.0e22, 1500.0, [11.2, 0.003], [80.1, -0.04], [211.3, 0.09], None, [0.3, 0.0], [17.5, 8765.4321]),
    ("body10", 5.0e24, 2000.0, [5.5, -0.002], [201.7, 0.11], [-40.2, 0.3], [3.1, 0.00002], [0.6, 0.01],
     [300.25, 6574.123]),
    ("body11", 1.0e23, 1200.0, [17.1, 0.001], [10.4, -0.2], [123.4, 0.05], [2.2, -0.00001], [0.9, 0.0],
     [45.6, 10957.5]),
)


def load_reference_ephemeris():
    """The reference's fakepta.ephemeris module; afterwards `fakepta` resolves to this repository's package again."""
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, HERE)
    import ref_shim
    ref_shim.load_reference()
    from fakepta import ephemeris as ref_eph
    for name in [m for m in sys.modules if m == "fakepta" or m.startswith("fakepta.")]:
        del sys.modules[name]
    sys.path[:] = [p for p in sys.path if p not in (ref_shim.REF, HERE)]
    sys.path.insert(0, ROOT)
    return ref_eph


def fresh(ref_eph, extras=True):
    e = ref_eph.Ephemeris()
    if extras:
        for name, mass, T, inc, Om, omega, a, ecc, l0 in EXTRA:
            e.add_planet(name, mass, T, list(inc), list(Om), list(omega), None if a is None else list(a), list(ecc),
                         list(l0))
    return e


def table_of(planets):
    rows = []
    for p in planets.values():
        row = [p["mass"], p["T"]]
        for k in ELEMENTS:
            row += [0.0, 0.0] if p[k] is None else [p[k][0], p[k][1]]
        rows.append(row)
    return np.array(rows, dtype=np.float64)


def main():
    ref_eph = load_reference_ephemeris()
    from tests import ephem_reference as R

    rng = np.random.default_rng(20261019)
    toas = [np.sort(rng.uniform(MJD0, MJD1, n)) * 86400.0 for n in N_TOA]
    toas[2][np.argmin(np.abs(toas[2] - J2000_S))] = J2000_S
    toas[2].sort()
    offs = np.concatenate([[0], np.cumsum(N_TOA)]).astype(np.int64)
    all_toas = np.concatenate(toas)
    assert J2000_S in all_toas and np.sum(all_toas < J2000_S) > 20
    theta = np.arccos(rng.uniform(-1, 1, len(N_TOA)))
    phi = rng.uniform(0, 2 * np.pi, len(N_TOA))
    pos = np.array([[np.cos(p) * np.sin(t), np.sin(p) * np.sin(t), np.cos(t)] for t, p in zip(theta, phi)])

    full = fresh(ref_eph)
    names = list(full.planets)
    bodies = table_of(full.planets)
    ref_table = table_of(fresh(ref_eph, extras=False).planets)
    mass_ss = float(full.mass_ss)
    assert bodies.shape == (11, R.N_BODY_COL)
    resolved = R.resolve_bodies(bodies)

    def per_pulsar(fn):
        return np.concatenate([fn(p, toas[p]) for p in range(len(N_TOA))], axis=0)

    # ---- orbits
    planet_truth = np.stack([R.orbit_mp(all_toas, b) for b in bodies], axis=1)
    planet_ref64 = np.stack([R.orbit_numpy(all_toas, b) for b in resolved], axis=1)
    err_planet = np.max(np.abs(planet_ref64 - planet_truth), axis=(0, 2))
    ref_planet = np.stack([per_pulsar(lambda p, t, nm=nm: fresh(ref_eph).get_orbit_planet(t, nm)) for nm in names],
                          axis=1)
    for b, nm in enumerate(names):
        peak = np.max(np.abs(planet_truth[:, b]))
        dev = np.max(np.abs(ref_planet[:, b] - planet_truth[:, b]))
        print(f"{nm:8s} peak {peak:.3e} s  fp64 error {err_planet[b]:.2e} ({err_planet[b] / peak:.1e})  "
              f"reference {dev / peak:.2e} of peak")
        assert dev <= REF_TOL * peak, (nm, dev / peak)
    sun_truth, sun8_truth = R.sun_mp(all_toas, bodies), R.sun_mp(all_toas, bodies[:8])
    err_sun = np.max(np.abs(R.sun_numpy(all_toas, bodies) - sun_truth))
    err_sun8 = np.max(np.abs(R.sun_numpy(all_toas, bodies[:8]) - sun8_truth))
    ref_sun = per_pulsar(lambda p, t: fresh(ref_eph).get_sunssb(t))
    ref_sun8 = per_pulsar(lambda p, t: fresh(ref_eph, extras=False).get_sunssb(t))
    for tag, ref, truth in (("sun", ref_sun, sun_truth), ("sun8", ref_sun8, sun8_truth)):
        dev, peak = np.max(np.abs(ref - truth)), np.max(np.abs(truth))
        print(f"{tag}: peak {peak:.3e} s, reference {dev / peak:.2e} of peak")
        assert dev <= REF_TOL * peak, (tag, dev / peak)

    # ---- Kepler sweep
    kepler_M = np.concatenate([[0.0, 1e-12, 1e-3, np.pi / 2, np.pi, 2 * np.pi - 1e-9],
                               np.sort(rng.uniform(0, 2 * np.pi, 20))])
    kepler_e = np.array([0.0, 1e-8, 0.0167, 0.2056, 0.6, 0.9, R.E_MAX])
    kepler_truth = np.stack([R.kepler_mp(kepler_M, e) for e in kepler_e])
    err_kepler = np.max(np.abs(np.stack([R.kepler_newton(kepler_M, e) for e in kepler_e]) - kepler_truth), axis=1)
    floor = np.spacing(np.max(np.abs(kepler_truth), axis=1))
    err_kepler = np.where(err_kepler == 0.0, floor, err_kepler)
    print("kepler fp64 error per e:", err_kepler)

    # ---- Roemer rows
    ib = {nm: i for i, nm in enumerate(names)}
    m = lambda nm: bodies[ib[nm], 0]  # noqa: E731
    specs = [("jupiter", dict(d_mass=1e-4 * m("jupiter"))), ("saturn", dict(d_mass=3e-5 * m("saturn"))),
             ("earth", dict(d_mass=2e-4 * m("earth"))), ("body11", dict(d_mass=1e-3 * m("body11"))),
             ("jupiter", dict(d_Om=1e-6)), ("jupiter", dict(d_omega=1e-6)), ("jupiter", dict(d_inc=1e-6)),
             ("jupiter", dict(d_a=1e-7)), ("jupiter", dict(d_e=1e-8)), ("jupiter", dict(d_l0=1e-6)),
             ("saturn", dict(d_mass=2e-5 * m("saturn"), d_Om=2e-6, d_omega=-1e-6, d_inc=5e-7, d_a=-3e-7, d_e=2e-8,
                             d_l0=-2e-6)),
             ("body9", dict(d_mass=-1e-3 * m("body9"), d_Om=-1e-6, d_omega=3e-6, d_inc=-2e-6, d_a=1e-7, d_e=-1e-8,
                            d_l0=1e-6))]
    rows = np.zeros((len(specs), R.N_ROW_COL))
    for r, (nm, dev) in enumerate(specs):
        rows[r, :R.N_BODY_COL] = bodies[ib[nm]]
        for k, key in enumerate(R.DEVIATIONS):
            rows[r, R.N_BODY_COL + k] = dev.get(key, 0.0)
        rows[r, -1] = 1.0 / mass_ss
    row_body = np.array([ib[nm] for nm, _ in specs], dtype=np.int64)
    roemer_truth = np.stack([per_pulsar(lambda p, t, row=row: R.roemer_mp(t, pos[p], row)) for row in rows])
    roemer_ref64 = np.stack([per_pulsar(lambda p, t, row=row: R.roemer_numpy(t, pos[p], row)) for row in rows])
    err_roemer = np.max(np.abs(roemer_ref64 - roemer_truth), axis=1)
    assert np.all(err_roemer > 0) and np.all(err_planet > 0) and err_sun > 0 and err_sun8 > 0
    ref_roemer = np.stack([per_pulsar(lambda p, t, nm=nm, dev=dev: fresh(ref_eph).roemer_delay(t, pos[p], nm, **dev))
                           for nm, dev in specs[:4]])
    for r in range(len(specs)):
        peak = np.max(np.abs(roemer_truth[r]))
        line = f"row {r:2d} ({specs[r][0]}): peak {peak:.3e} s  fp64 error {err_roemer[r]:.2e} ({err_roemer[r] / peak:.1e})"
        if r < 4:
            dev = np.max(np.abs(ref_roemer[r] - roemer_truth[r]))
            line += f"  reference {dev / peak:.2e} of peak"
            assert dev <= REF_TOL * peak, (r, dev / peak)
        print(line)
        assert peak > 0

    path = os.path.join(ROOT, "tests", "golden", "g11_ephem.npz")
    np.savez(path, offs=offs, toas=all_toas, theta=theta, phi=phi, pos=pos, bodies=bodies, names=np.array(names),
             mass_ss=mass_ss, planet_truth=planet_truth, sun_truth=sun_truth, sun8_truth=sun8_truth,
             err_planet=err_planet, err_sun=err_sun, err_sun8=err_sun8, kepler_M=kepler_M, kepler_e=kepler_e,
             kepler_truth=kepler_truth, err_kepler=err_kepler, rows=rows, row_body=row_body,
             roemer_truth=roemer_truth, err_roemer=err_roemer, ref_planet=ref_planet, ref_sun=ref_sun,
             ref_sun8=ref_sun8, ref_roemer=ref_roemer, ref_table=ref_table,
             ref_names=np.array(names[:8]), ref_mass_ss=float(fresh(ref_eph, extras=False).mass_ss))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
