"""Ephemeris and Roemer delay, host side (no GPU): the drop-in fakepta.ephemeris module, the C-ABI surface, the
numpy model of the device's Kepler solve, the integrity of the fixture tests/golden/g11_ephem.npz
(tools/gen_ephem_golden.py), the host validation of csrc/ephem_host.h in a stand-alone C++ program built with the
address and undefined-behaviour sanitizers, and add_roemer_delay's choice between the native and a user's ephemeris."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from tests import ephem_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fakepta_amd.h")
LIB = os.path.join(ROOT, "fakepta_amd", "lib", "libfakepta_amd.so")
CSRC = os.path.join(ROOT, "fakepta_amd", "csrc")
ENTRY_POINTS = ("fpta_ephem_kepler", "fpta_ephem_orbits", "fpta_roemer_accumulate")


@pytest.fixture(scope="module")
def g(golden):
    return golden("g11_ephem.npz")


def no_context(*a, **k):
    raise AssertionError("a device context was requested")


# ----------------------------------------------------------------------------- the drop-in module
def test_ephemeris_imports_without_matplotlib():
    code = ("import sys; from fakepta.ephemeris import Ephemeris; e = Ephemeris(); "
            "assert 'matplotlib' not in sys.modules, 'matplotlib was imported'; print(len(e.planets))")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "8", r.stderr


def test_planet_table_is_the_references(g):
    from fakepta import constants as const
    from fakepta.ephemeris import Ephemeris
    from fakepta_amd import ephem
    e = Ephemeris()
    assert list(e.planets) == list(g["ref_names"]) == e.planet_names
    assert all(list(p) == ["mass", "T", "inc", "Om", "omega", "a", "e", "l0"] for p in e.planets.values())
    np.testing.assert_array_equal(ephem.body_table(e.planets), g["ref_table"])  # bit for bit
    assert e.mass_ss == float(g["ref_mass_ss"])
    assert ephem.BODY_COLUMNS == R.BODY_COLUMNS and ephem.ROW_COLUMNS == R.ROW_COLUMNS
    assert const.Msun == R.const.Msun


def test_add_planet_updates_names_and_mass(g):
    from fakepta.ephemeris import Ephemeris
    from fakepta_amd import ephem
    e = Ephemeris()
    before = e.mass_ss
    e.add_planet("body9", 1.0e22, 1500.0, [11.2, 0.003], [80.1, -0.04], [211.3, 0.09], None, [0.3, 0.0],
                 [17.5, 8765.4321])
    assert e.planet_names[-1] == "body9" and len(e.planet_names) == 9
    assert e.mass_ss > before and abs(e.mass_ss - before - 1.0e22) <= 8 * np.spacing(e.mass_ss)
    tab = ephem.body_table(e.planets)
    np.testing.assert_array_equal(tab[8], g["bodies"][8])
    assert tab[8, R.I_A] == 0.0 and tab[8, R.I_A + 1] == 0.0  # a = None travels as (0, 0) ...
    a = R.resolve_bodies(tab)[8, R.I_A]                        # ... and stands for Kepler's third law
    assert abs(a - (1500.0 / 365.25) ** (2 / 3)) < 1e-4 * a
    with pytest.raises(ValueError):
        ephem.body_row(dict(e.planets["earth"], e=None))


def test_rotation_matches_the_definition():
    from fakepta.ephemeris import Ephemeris
    got = Ephemeris().do_rotation_op_to_eq(np.array([1.5, -0.5, 0.0]), 100.47, -85.7, 1.3)
    want = R._rotate(1.5, -0.5, 100.47, -85.7, 1.3, np.cos, np.sin, np.pi)
    np.testing.assert_allclose(got, want, rtol=0, atol=4 * np.finfo(float).eps)


# ----------------------------------------------------------------------------- C ABI
def test_abi_declares_and_exports_the_entry_points():
    text = open(HEADER).read()
    lib = ctypes.CDLL(LIB)
    from fakepta_amd import _capi
    for name in ENTRY_POINTS:
        assert re.search(rf"^int\s+{name}\s*\(", text, flags=re.M), name
        assert hasattr(lib, name) and name in _capi.EXPORTED
    npar = int(re.search(r"^#define\s+FPTA_ROEMER_NPAR\s+(\d+)\b", text, flags=re.M).group(1))
    nbody = int(re.search(r"^#define\s+FPTA_EPHEM_NBODY\s+(\d+)\b", text, flags=re.M).group(1))
    assert npar == _capi.ROEMER_NPAR == R.N_ROW_COL and nbody == _capi.EPHEM_NBODY == R.N_BODY_COL
    assert npar == nbody + 7 + 1
    assert re.search(r"^#define\s+FPTA_K_EPHEM\s+7\b", text, flags=re.M) and _capi.K_EPHEM == 7
    assert re.search(r"^#define\s+FPTA_K_N\s+8\b", text, flags=re.M)
    assert float(re.search(r"^#define\s+FPTA_EPHEM_E_MAX\s+([\d.]+)", text, flags=re.M).group(1)) == R.E_MAX
    assert _capi.EPHEM_E_MAX == R.E_MAX and _capi.EPHEM_MSUN == R.const.Msun
    host = open(os.path.join(CSRC, "ephem_host.h")).read()
    for pat, want in ((r"kEMax = ([\d.e-]+);", R.E_MAX), (r"kLowE = ([\d.e-]+);", R.KEPLER_LOW_E),
                      (r"kKeplerTol = ([\d.e-]+);", R.KEPLER_TOL), (r"kKeplerMaxIter = (\d+);", R.KEPLER_MAX_ITER)):
        assert float(re.search(pat, host).group(1)) == want, pat


# ----------------------------------------------------------------------------- the Kepler model
def test_newton_model_converges_within_the_cap():
    """Dense sweep of the device's iteration in numpy: every (M, e) meets the stopping rule before the shipped cap, and
    what it returns solves the equation to rounding."""
    M = np.linspace(0.0, 2 * np.pi, 1200, endpoint=False)
    e = np.concatenate([np.linspace(0.0, R.E_MAX, 600), [np.nextafter(R.KEPLER_LOW_E, 0), R.KEPLER_LOW_E, 1e-8]])
    corners = np.array([0.0, 1e-300, 1e-12, 1e-3, np.pi / 2, np.pi, np.nextafter(np.pi, 0), np.nextafter(np.pi, 4),
                        2 * np.pi - 1e-9, np.nextafter(2 * np.pi, 0), 2 * np.pi])
    worst = 0
    for Ms in (M, corners):
        E, it = R.kepler_newton(Ms[:, None], e[None, :], return_iterations=True)
        worst = max(worst, int(it.max()))
        assert it.max() < R.KEPLER_MAX_ITER, (it.max(), np.argwhere(it == it.max())[0])
        resid = np.abs((E - e[None, :] * np.sin(E)) - Ms[:, None])
        # the residual of the fp64 closest to the root: a few ulp of the terms, which are <= 2 pi
        assert resid.max() <= 4 * np.spacing(2 * np.pi), resid.max()
        assert np.all(E >= -1e-15) and np.all(E <= 2 * np.pi + 4 * np.spacing(2 * np.pi))
    print(f"most Newton steps over the sweep: {worst} (cap {R.KEPLER_MAX_ITER})")


def test_model_matches_the_truth_of_the_fixture(g):
    for k, e in enumerate(g["kepler_e"]):
        err = np.max(np.abs(R.kepler_newton(g["kepler_M"], e) - g["kepler_truth"][k]))
        print(f"e = {e}: model error {err:.3e}, stored {g['err_kepler'][k]:.3e}")
        assert err <= 2.0 * g["err_kepler"][k]


# ----------------------------------------------------------------------------- fixture
def test_fixture_integrity(g):
    offs, n = g["offs"], int(g["offs"][-1])
    assert list(np.diff(offs)) == [1, 63, 64, 65, 130]
    assert g["toas"].shape == (n,) and g["pos"].shape == (5, 3)
    np.testing.assert_allclose(np.linalg.norm(g["pos"], axis=1), 1.0, rtol=0, atol=1e-15)
    assert 51544.5 * 86400.0 in g["toas"] and np.sum(g["toas"] < 51544.5 * 86400.0) > 20
    assert g["toas"].min() >= 48000 * 86400.0 and g["toas"].max() <= 60500 * 86400.0
    assert g["bodies"].shape == (11, 14) and g["rows"].shape == (12, 22)
    np.testing.assert_array_equal(g["bodies"][:8], g["ref_table"])
    b = g["bodies"]
    assert (b[8, R.I_A], b[8, R.I_A + 1], b[8, R.I_T], b[8, R.I_E]) == (0.0, 0.0, 1500.0, 0.3)
    assert (b[9, R.I_E], b[9, R.I_E + 1]) == (0.6, 0.01) and b[10, R.I_E] == 0.9
    assert g["planet_truth"].shape == (n, 11, 3) and g["sun_truth"].shape == (n, 3)
    assert g["kepler_truth"].shape == (7, 26) and g["roemer_truth"].shape == (12, n)
    assert list(g["kepler_e"]) == [0.0, 1e-8, 0.0167, 0.2056, 0.6, 0.9, R.E_MAX]
    assert list(g["kepler_M"][:6]) == [0.0, 1e-12, 1e-3, np.pi / 2, np.pi, 2 * np.pi - 1e-9]
    for key in ("err_planet", "err_sun", "err_sun8", "err_kepler", "err_roemer"):
        assert np.all(g[key] >= 0) and np.all(np.isfinite(g[key])), key
    dev = g["rows"][:, 14:21]
    assert np.all(dev[:4, 0] != 0) and not dev[:4, 1:].any()  # four d_mass-only rows
    assert not dev[4:10, 0].any() and np.all(np.count_nonzero(dev[4:10, 1:], axis=1) == 1)
    assert sorted(np.nonzero(dev[4:10, 1:])[1]) == list(range(6))  # each element once
    assert np.all(dev[10:] != 0)
    np.testing.assert_array_equal(g["rows"][:, :14], g["bodies"][g["row_body"]])
    np.testing.assert_array_equal(g["rows"][:, 21], 1.0 / float(g["mass_ss"]))


def test_reference_output_is_within_its_share_of_the_parity_tolerance(g):
    """The generator's condition, re-checked: the reference's own output lies within 2.5e-11 max |truth| of the
    truth, which leaves three quarters of the 1e-10 parity tolerance to the device."""
    for b in range(11):
        peak = np.max(np.abs(g["planet_truth"][:, b]))
        assert np.max(np.abs(g["ref_planet"][:, b] - g["planet_truth"][:, b])) <= 2.5e-11 * peak, b
    for ref, truth in (("ref_sun", "sun_truth"), ("ref_sun8", "sun8_truth")):
        assert np.max(np.abs(g[ref] - g[truth])) <= 2.5e-11 * np.max(np.abs(g[truth]))
    for r in range(4):
        peak = np.max(np.abs(g["roemer_truth"][r]))
        assert np.max(np.abs(g["ref_roemer"][r] - g["roemer_truth"][r])) <= 2.5e-11 * peak, r


def test_fp64_evaluation_reproduces_err_ref64(g):
    offs, toas = g["offs"], g["toas"]
    resolved = R.resolve_bodies(g["bodies"])
    for b in range(11):
        err = np.max(np.abs(R.orbit_numpy(toas, resolved[b]) - g["planet_truth"][:, b]))
        print(f"body {b}: literal fp64 error {err:.3e}, stored {g['err_planet'][b]:.3e}")
        assert err <= 2.0 * g["err_planet"][b]  # 1.0 x with the generator's libm; another host's may differ by an ulp
    assert np.max(np.abs(R.sun_numpy(toas, g["bodies"]) - g["sun_truth"])) <= 2.0 * g["err_sun"]
    assert np.max(np.abs(R.sun_numpy(toas, g["bodies"][:8]) - g["sun8_truth"])) <= 2.0 * g["err_sun8"]
    for r, row in enumerate(g["rows"]):
        ref = np.concatenate([R.roemer_numpy(toas[offs[p]:offs[p + 1]], g["pos"][p], row) for p in range(5)])
        err = np.max(np.abs(ref - g["roemer_truth"][r]))
        print(f"row {r}: literal fp64 error {err:.3e}, stored {g['err_roemer'][r]:.3e}")
        assert err <= 2.0 * g["err_roemer"][r]


def test_fixture_truth_reevaluates_bitwise(g):
    pytest.importorskip("mpmath")
    offs, toas = g["offs"], g["toas"]
    for b in (0, 8, 10):
        for i in (0, 1, 200):
            assert np.array_equal(R.orbit_mp(toas[i:i + 1], g["bodies"][b])[0], g["planet_truth"][i, b]), (b, i)
    np.testing.assert_array_equal(R.sun_mp(toas[5:6], g["bodies"]), g["sun_truth"][5:6])
    for r in (0, 7, 11):
        i = offs[3] + 2
        assert R.roemer_mp(toas[i:i + 1], g["pos"][3], g["rows"][r])[0] == g["roemer_truth"][r, i], r
    np.testing.assert_array_equal(R.kepler_mp(g["kepler_M"][:8], 0.9), g["kepler_truth"][5, :8])


# ----------------------------------------------------------------------------- ephem_host.h under the sanitizers
_MAIN = r"""
#include <cstdio>
#include <vector>
#include "ephem_host.h"
using namespace fpta_ephem;
// stdin: mode ("bodies" | "rows"), n, toa_min, toa_max, then n rows. stdout: per accepted entry "ok i a e0 e1" (the
// resolved a, e at both ends) and for the first refused one "bad i reason" (validation stops there, as the entry
// points do); then the constants.
int main() {
  char mode[16];
  long n = 0;
  double span[2];
  if (std::scanf("%15s %ld %lf %lf", mode, &n, &span[0], &span[1]) != 4 || n < 0) return 2;
  const bool rows = mode[0] == 'r';
  const int width = rows ? kNRow : kNBody;
  std::vector<double> tab((size_t)n * width);
  for (double& v : tab)
    if (std::scanf("%lf", &v) != 1) return 2;
  double t0, t1;
  int64_t bad_toa = -1;
  if (!toa_span(2, span, t0, t1, bad_toa)) {
    std::printf("badtoa %ld\n", (long)bad_toa);
    return 0;
  }
  std::string why;
  std::vector<Body> bodies((size_t)n);
  std::vector<RoemerRow> rr((size_t)n);
  const long bad = rows ? (long)validate_rows(n, tab.data(), t0, t1, rr.data(), why)
                        : (long)validate_bodies(n, tab.data(), t0, t1, bodies.data(), why);
  for (long i = 0; i < (bad < 0 ? n : bad); ++i) {
    const Body& b = rows ? rr[(size_t)i].base : bodies[(size_t)i];
    std::printf("ok %ld %.17g %.17g %.17g", i, b.a, b.e + b.e_rate * t0, b.e + b.e_rate * t1);
    if (rows) {
      const RoemerRow& r = rr[(size_t)i];
      std::printf(" %.17g %.17g %.17g %.17g %.17g", r.pert.a, r.pert.l0, r.mass_w, r.dmass_w, r.same);
    }
    std::printf("\n");
  }
  if (bad >= 0) std::printf("bad %ld %s\n", bad, why.c_str());
  const Obliquity ob = obliquity();
  double e0, e1;
  int64_t none = -1;
  toa_span(0, nullptr, e0, e1, none);
  std::printf("const %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", ob.sn, ob.cs, t0, t1, kMsun, e0, e1);
  return 0;
}
"""


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("ephem_host")
    (d / "main.cpp").write_text(_MAIN)
    exe = str(d / "ephem_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, str(d / "main.cpp"), "-o", exe], check=True)

    def run(mode, tab, toa_min, toa_max):
        text = f"{mode} {len(tab)} {toa_min!r} {toa_max!r}\n" + \
            "\n".join(" ".join(repr(float(v)) for v in row) for row in tab) + "\n"
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return r.stdout.splitlines()
    return run


def test_host_resolution_and_constants(g, host_program):
    toas = g["toas"]
    lines = host_program("bodies", g["bodies"], float(toas.min()), float(toas.max()))
    assert len(lines) == 12 and all(ln.startswith("ok") for ln in lines[:11])
    resolved = R.resolve_bodies(g["bodies"])
    t0, t1 = R.centuries(toas.min()), R.centuries(toas.max())
    for b, line in enumerate(lines[:11]):
        _, idx, a, e0, e1 = line.split()
        assert int(idx) == b
        # a = None (body 8) resolves to the Kepler-law value; every other a passes through. The host takes a cube
        # root; numpy's x ** (1 / 3) rounds the exponent, which costs ln(x) ulp(1/3) / 2 = 1.5e-15 at x = 5.6e34
        np.testing.assert_allclose(float(a), resolved[b, R.I_A], rtol=4e-15 if b == 8 else 0, atol=0)
        np.testing.assert_allclose([float(e0), float(e1)], resolved[b, R.I_E] + resolved[b, R.I_E + 1] * np.array([t0, t1]),
                                   rtol=1e-15, atol=1e-18)
    sn, cs, ht0, ht1, msun, z0, z1 = map(float, lines[-1].split()[1:])
    ec = np.deg2rad(R.OBLIQUITY_DEG)
    np.testing.assert_allclose([sn, cs], [np.sin(ec), np.cos(ec)], rtol=2e-16, atol=0)
    assert (ht0, ht1) == (t0, t1) and t0 < 0 < t1 and (z0, z1) == (0.0, 0.0)
    assert msun == R.const.Msun


def test_host_roemer_rows(g, host_program):
    toas = g["toas"]
    lines = host_program("rows", g["rows"], float(toas.min()), float(toas.max()))
    assert len(lines) == 13 and all(ln.startswith("ok") for ln in lines[:12])
    resolved = R.resolve_bodies(g["rows"][:, :14])
    for r, line in enumerate(lines[:12]):
        f = line.split()
        a, pa, pl0, mw, dmw, same = float(f[2]), *map(float, f[5:])
        row = g["rows"][r]
        assert a == pytest.approx(resolved[r, R.I_A], rel=4e-15 if r == 11 else 0, abs=0)
        assert pa == a + row[14 + 4] and pl0 == row[R.I_L0] + row[14 + 6]
        assert mw == row[0] * row[21] and dmw == row[14] * row[21]
        assert same == (1.0 if r < 4 else 0.0)


def _bad_body(g, col, value):
    tab = g["bodies"].copy()
    tab[6, col] = value
    return tab


@pytest.mark.parametrize("col,value,reason", [(R.I_L0, float("nan"), "non-finite l0"),
                                              (R.I_OM + 1, float("inf"), "non-finite Om rate"),
                                              (R.I_E, 0.951, "eccentricity"),
                                              (R.I_E, -1e-3, "eccentricity"),
                                              (R.I_E + 1, 8.0, "eccentricity"),   # 0.047 + 8 t leaves [0, 0.95] at both ends
                                              (R.I_E + 1, -0.5, "eccentricity"),  # and drops below 0 there with -0.5 t
                                              (R.I_A, -19.0, "semi-major axis"),
                                              (R.I_A + 1, 250.0, "semi-major axis")])  # 19.2 + 250 t < 0 at the early end
def test_host_validation_names_the_body(g, host_program, col, value, reason):
    toas = g["toas"]
    lines = host_program("bodies", _bad_body(g, col, value), float(toas.min()), float(toas.max()))
    assert [ln.split()[0] for ln in lines[:-1]] == ["ok"] * 6 + ["bad"]
    tag, idx, why = lines[-2].split(None, 2)
    assert int(idx) == 6 and reason in why


def test_host_span_ends_decide(g, host_program):
    """e = 0.047 + 8 t is inside [0, 0.95] at t = 0 and over a short span around it, and outside at the fixture's
    late end only: the check looks at the ends of the span, not at the epoch."""
    tab = _bad_body(g, R.I_E + 1, 8.0)
    j2000 = 51544.5 * 86400.0
    assert all(ln.startswith("ok") for ln in host_program("bodies", tab, j2000 - 1e7, j2000 + 1e7)[:-1])
    early_only = host_program("bodies", tab, float(g["toas"].min()), j2000)  # e < 0 at the early end
    assert early_only[-2].startswith("bad 6")
    tab = _bad_body(g, R.I_E + 1, 3.0)  # fine at the early end and at J2000, outside only after 2030
    assert all(ln.startswith("ok") for ln in host_program("bodies", tab, j2000, j2000 + 1e8)[:-1])
    assert host_program("bodies", tab, j2000, j2000 + 1e9)[-2].startswith("bad 6")
    assert host_program("bodies", g["bodies"], float("nan"), 1.0)[0] == "badtoa 0"
    none_without_period = g["bodies"].copy()
    none_without_period[8, R.I_T] = 0.0
    assert "a = None" in host_program("bodies", none_without_period, j2000, j2000 + 1.0)[-2]


@pytest.mark.parametrize("col,value,reason", [(14 + 2, float("nan"), "non-finite d_omega"),
                                              (21, 0.0, "mass_ss"),
                                              (21, -1e-30, "mass_ss"),
                                              (21, float("inf"), "mass_ss"),
                                              (14 + 5, 0.95, "with its deviations: eccentricity"),
                                              (14 + 4, -6.0, "with its deviations: semi-major axis"),
                                              (R.I_INC, float("nan"), "non-finite inc")])
def test_host_validation_names_the_row(g, host_program, col, value, reason):
    rows = g["rows"].copy()
    rows[5, col] = value  # row 5 is a Jupiter row (a = 5.2 AU, e = 0.0485)
    toas = g["toas"]
    lines = host_program("rows", rows, float(toas.min()), float(toas.max()))
    assert [ln.split()[0] for ln in lines[:-1]] == ["ok"] * 5 + ["bad"]
    tag, idx, why = lines[-2].split(None, 2)
    assert int(idx) == 5 and reason in why


# ----------------------------------------------------------------------------- add_roemer_delay without a GPU
class ForeignEphem:
    """A user's own ephemeris class: anything with roemer_delay()."""

    def __init__(self):
        self.calls = []

    def roemer_delay(self, toas, psr_pos, planet, d_mass=0., d_Om=0., d_omega=0., d_inc=0., d_a=0., d_e=0., d_l0=0.):
        self.calls.append((len(toas), planet, d_mass, d_Om, d_omega, d_inc, d_a, d_e, d_l0))
        return np.full(len(toas), d_mass + d_l0)


def _plain_pulsars(ephems):
    return [SimpleNamespace(name=f"J{i:04d}", toas=np.arange(3.0 + i), pos=np.array([1.0, 0, 0]),
                            residuals=np.zeros(3 + i), **({} if e is None else {"ephem": e}))
            for i, e in enumerate(ephems)]


def test_add_roemer_delay_prints_and_returns_without_ephem(monkeypatch, capsys):
    from fakepta import correlated_noises as cn
    from fakepta_amd import _capi
    monkeypatch.setattr(_capi, "get_context", no_context)
    eph = ForeignEphem()
    for fn, args in ((cn.add_roemer_delay, ("jupiter", 1.0)), (cn.add_roemer_delay_array, ([("jupiter", {})],))):
        psrs = _plain_pulsars([eph, None, eph])
        fn(psrs, *args)
        assert '"ephem" not found in pulsar J0001' in capsys.readouterr().out
        assert not eph.calls and not any(p.residuals.any() for p in psrs)


def test_add_roemer_delay_uses_a_foreign_ephem_per_pulsar(monkeypatch):
    from fakepta import correlated_noises as cn
    from fakepta_amd import _capi
    monkeypatch.setattr(_capi, "get_context", no_context)
    a, b = ForeignEphem(), ForeignEphem()
    psrs = _plain_pulsars([a, b, a])
    cn.add_roemer_delay(psrs, "saturn", d_mass=2.0, d_l0=0.5)
    assert a.calls == [(3, "saturn", 2.0, 0., 0., 0., 0., 0., 0.5), (5, "saturn", 2.0, 0., 0., 0., 0., 0., 0.5)]
    assert b.calls == [(4, "saturn", 2.0, 0., 0., 0., 0., 0., 0.5)]
    assert all(np.all(p.residuals == 2.5) for p in psrs)
    cn.add_roemer_delay_array(psrs, [("earth", dict(d_mass=1.0)), ("mars", dict(d_l0=-0.25))])
    assert len(a.calls) == 6 and len(b.calls) == 3 and b.calls[-1][1] == "mars"
    assert all(np.all(p.residuals == 2.5 + 1.0 - 0.25) for p in psrs)


def test_native_ephem_shared_by_all_is_detected():
    from fakepta import correlated_noises as cn
    from fakepta.ephemeris import Ephemeris
    e1, e2 = Ephemeris(), Ephemeris()
    assert cn._native_ephem(_plain_pulsars([e1, e1])) is e1
    assert cn._native_ephem(_plain_pulsars([e1, e2])) is None        # two objects may hold different planets
    assert cn._native_ephem(_plain_pulsars([e1, ForeignEphem()])) is None
    row = e1.roemer_row("jupiter", d_mass=1e23, d_e=1e-8)
    assert row.shape == (22,) and row[14] == 1e23 and row[14 + 5] == 1e-8 and row[21] == 1.0 / e1.mass_ss
