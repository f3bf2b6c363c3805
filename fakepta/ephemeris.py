"""Drop-in for fakepta/ephemeris.py: Keplerian solar-system ephemeris and the Roemer delay of ephemeris errors.

Same class, methods and signatures as the reference; the orbits are evaluated on the GPU (libfakepta_amd:
fpta_ephem_kepler, fpta_ephem_orbits, fpta_roemer_accumulate through fakepta_amd.ephem), every body and every TOA
in one call instead of one scipy root find per (TOA, planet). Differences from the reference, each a defect of it
(DESIGN.md section 8):
  * roemer_delay leaves `planets` untouched and evaluates the unperturbed orbit from the stored elements, so element
    deviations give a non-zero delay and calls do not accumulate;
  * get_planet_ssb sets the velocity columns to 0 and covers every body of `planet_names`, added ones included.
The in-plane x = a cos(E - e) of the reference is kept.
"""
import numpy as np

from fakepta_amd import ephem as _ephem
from . import constants as const

# Keplerian elements and rates of the planets, J2000 ecliptic, valid 1800 - 2050 AD (E. M. Standish, JPL Solar System
# Dynamics, "Approximate positions of the planets", https://ssd.jpl.nasa.gov/planets/approx_pos.html):
# name, mass [kg], period [days], then (value, rate per Julian century) of the inclination [deg], the longitude of
# the ascending node [deg], the longitude of perihelion [deg], the semi-major axis [AU], the eccentricity and the mean
# longitude [deg]
_JPL = (
    ("mercury", 3.301 * 1e23, 87.9691, (7.00497902, -0.00594749), (48.33076593, -0.12534081),
     (77.45779628, 0.16047689), (0.38709927, 0.00000037), (0.20563661, 0.00001906), (252.25032350, 149472.67411175)),
    ("venus", 4.867 * 1e24, 224.7, (3.39467605, -0.00078890), (76.67984255, -0.27769418),
     (131.60246718, 0.00268329), (0.72333566, 0.00000390), (0.00676399, -0.00004107), (181.97909950, 58517.81538729)),
    ("earth", 5.972 * 1e24, 365.25636, (-0.00001531, -0.01294668), (0., 0.),
     (102.93768193, 0.32327364), (1.00000261, 0.00000562), (0.01673163, -0.00004392), (100.46457166, 35999.37244981)),
    ("mars", 6.417 * 1e23, 687.0, (1.84969142, -0.00813131), (49.55953891, -0.29257343),
     (-23.94362959, 0.44441088), (1.52371034, 0.00001847), (0.09336511, 0.00007882), (-4.55343205, 19140.30268499)),
    ("jupiter", 1.899 * 1e27, 4331, (1.30439695, -0.00183714), (100.47390909, 0.20469106),
     (14.72847983, 0.21252668), (5.20288700, -0.00011607), (0.04853590, -0.00013253), (34.39644051, 3034.74612775)),
    ("saturn", 5.685 * 1e26, 10747, (2.48599187, 0.00193609), (113.66242448, -0.28867794),
     (92.59887831, -0.41897216), (9.53667594, -0.00125060), (0.05550825, -0.00050991), (49.95424423, 1222.49362201)),
    ("uranus", 8.683 * 1e25, 30589, (0.77263783, -0.00242939), (74.01692503, 0.04240589),
     (170.95427630, 0.40805281), (19.18916464, -0.00196176), (0.04685740, -0.00004397), (313.23810451, 428.48202785)),
    ("neptune", 1.024 * 1e26, 59800, (1.77004347, 0.00035372), (131.78422574, -0.00508664),
     (44.96476227, -0.32241464), (30.06992276, 0.00026291), (0.00895439, 0.00005105), (-55.12002969, 218.45945325)),
)

OBLIQUITY_DEG = 23.43928


class Ephemeris:

    def __init__(self):
        self.planets = {}
        for name, mass, T, inc, Om, omega, a, e, l0 in _JPL:
            self.planets[name] = {'mass': mass, 'T': T, 'inc': list(inc), 'Om': list(Om), 'omega': list(omega),
                                  'a': list(a), 'e': list(e), 'l0': list(l0)}
        self._update()

    def _update(self):
        self.planet_names = [*self.planets]
        self.mass_ss = const.Msun + np.sum([self.planets[planet]['mass'] for planet in self.planet_names])

    def add_planet(self, name, mass, T, inc, Om, omega, a, e, l0):
        """Adds (or replaces) a body; `a` may be None: the semi-major axis then follows from T by Kepler's law."""
        self.planets[name] = {'mass': mass, 'T': T, 'inc': inc, 'Om': Om, 'omega': omega, 'a': a, 'e': e, 'l0': l0}
        self._update()

    def do_rotation_op_to_eq(self, vec, Om, omega, inc):
        """Orbital plane -> equatorial frame of `vec` [3] for angles in degrees (host numpy; the kernels apply the
        same two rotations). `omega` is the argument of periapsis measured from the node."""
        ec, inc, Om, omega = np.deg2rad([OBLIQUITY_DEG, inc, Om, omega])
        cO, sO, cw, sw, ci, si = np.cos(Om), np.sin(Om), np.cos(omega), np.sin(omega), np.cos(inc), np.sin(inc)
        rot = np.array([[cO * cw - sO * ci * sw, -cO * sw - sO * ci * cw, 0.],
                        [sO * cw + cO * ci * sw, -sO * sw + cO * ci * cw, 0.],
                        [si * sw, si * cw, 0.]])
        rot_ec = np.array([[1., 0., 0.],
                           [0., np.cos(ec), -np.sin(ec)],
                           [0., np.sin(ec), np.cos(ec)]])
        return rot_ec @ (rot @ np.asarray(vec, dtype=float))

    def solve_kepler_equation(self, M, e):
        """Eccentric anomaly of mean anomaly M [rad] and eccentricity e, elementwise."""
        return _ephem.kepler(M, e)

    def compute_orbit(self, times, T, Om, omega, inc, a, e, l0, mass=None):
        """[n, 3] position [light-seconds, equatorial] at `times` [MJD seconds] of the orbit with these elements."""
        body = {'mass': 0. if mass is None else mass, 'T': T, 'inc': inc, 'Om': Om, 'omega': omega, 'a': a, 'e': e,
                'l0': l0}
        return _ephem.planet_ssb(times, [body])[:, 0, :3]

    def get_orbit_planet(self, times, planet):
        return self.compute_orbit(times, **self.planets[planet])

    def get_planet_ssb(self, times):
        """[n, len(planet_names), 6]: positions in columns 0 .. 2, zeros in the velocity columns."""
        return _ephem.planet_ssb(times, [self.planets[planet] for planet in self.planet_names])

    def get_sunssb(self, times):
        return _ephem.sun_ssb(times, [self.planets[planet] for planet in self.planet_names])

    def roemer_row(self, planet, d_mass=0., d_Om=0., d_omega=0., d_inc=0., d_a=0., d_e=0., d_l0=0.):
        """The row of fakepta_amd.ephem.roemer_delay_array for a deviation of `planet`'s mass and elements."""
        return _ephem.roemer_row(self.planets[planet], self.mass_ss, d_mass, d_Om, d_omega, d_inc, d_a, d_e, d_l0)

    def roemer_delay(self, toas, psr_pos, planet, d_mass=0., d_Om=0., d_omega=0., d_inc=0., d_a=0., d_e=0., d_l0=0.):
        """Delay [s] at `toas` for a pulsar at unit vector `psr_pos` when `planet`'s mass and elements deviate from
        the stored ones. `planets` is not modified."""
        out = np.zeros(len(toas))
        _ephem.accumulate([toas], [psr_pos], self.roemer_row(planet, d_mass, d_Om, d_omega, d_inc, d_a, d_e, d_l0),
                          out)
        return out
