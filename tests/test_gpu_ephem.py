"""Ephemeris and Roemer delay on the GPU (fpta_ephem_kepler, fpta_ephem_orbits, fpta_roemer_accumulate,
csrc/ephem.hip) against tests/golden/g11_ephem.npz.

The yardstick of every accuracy check is stored in the fixture: err_*, the measured max-abs error of the literal
fp64 numpy evaluation of the definition against the 50-digit truth (tools/gen_ephem_golden.py). The device may be
4 x that: its sincos / sqrt are a few ulp where the host libm is <= 1. Parity with the reference's own stored output
is the project's 1e-10 max |ref|."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_PSR = 5
D_KEYS = ("d_mass", "d_Om", "d_omega", "d_inc", "d_a", "d_e", "d_l0")


@pytest.fixture(scope="module")
def g(golden):
    return golden("g11_ephem.npz")


@pytest.fixture(scope="module")
def capi():
    from fakepta_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def ephem():
    from fakepta_amd import ephem
    return ephem


@pytest.fixture()
def ctx(capi):
    return capi.get_context()  # the context the Ephemeris methods and fakepta_amd.ephem use


def planet_dict(row):
    d = {"mass": float(row[0]), "T": float(row[1])}
    for k, key in enumerate(("inc", "Om", "omega", "a", "e", "l0")):
        v = [float(row[2 + 2 * k]), float(row[3 + 2 * k])]
        d[key] = None if key == "a" and v == [0.0, 0.0] else v
    return d


def full_ephemeris(g):
    """The native Ephemeris with the fixture's three added bodies."""
    from fakepta.ephemeris import Ephemeris
    e = Ephemeris()
    for b in range(8, 11):
        p = planet_dict(g["bodies"][b])
        e.add_planet(str(g["names"][b]), p["mass"], p["T"], p["inc"], p["Om"], p["omega"], p["a"], p["e"], p["l0"])
    assert e.mass_ss == float(g["mass_ss"])
    return e


def make_pulsars(g, ephem_obj, which=range(N_PSR)):
    from fakepta.fake_pta import Pulsar
    np.random.seed(7)
    offs = g["offs"]
    out = []
    for p in which:
        psr = Pulsar(g["toas"][offs[p]:offs[p + 1]], 1e-6, g["theta"][p], g["phi"][p], ephem=ephem_obj)
        psr.pos = g["pos"][p].copy()  # the fixture's doubles, whatever this host's sin / cos round to
        np.testing.assert_array_equal(psr.toas, g["toas"][offs[p]:offs[p + 1]])
        out.append(psr)
    return out


def deviations(row):
    return {k: float(v) for k, v in zip(D_KEYS, row[14:21])}


@pytest.fixture(scope="module")
def separate(g, capi):
    """Every row's delay over the whole array, from one separate-mode call: shared, never modified."""
    out = np.full((12, g["offs"][-1]), np.nan)
    capi.get_context().roemer_accumulate(g["offs"], g["toas"], g["pos"], g["rows"], out, separate=True)
    out.setflags(write=False)
    return out


# ----------------------------------------------------------------------------- Kepler
def test_kepler_sweep(g, ephem, ctx):
    got = ephem.kepler(g["kepler_M"][None, :], g["kepler_e"][:, None])
    assert got.shape == (7, 26)
    for k, e in enumerate(g["kepler_e"]):
        err = np.max(np.abs(got[k] - g["kepler_truth"][k]))
        print(f"e = {e}: device error {err:.3e} = {err / g['err_kepler'][k]:.3g} x the fp64 model's")
        assert err <= 4 * g["err_kepler"][k]
    # whole turns are taken off and put back; the class method is the same call
    from fakepta.ephemeris import Ephemeris
    M = g["kepler_M"][6:16]
    turned = Ephemeris().solve_kepler_equation(M + 6 * np.pi, np.full(10, 0.2056))
    np.testing.assert_allclose(turned - 6 * np.pi, got[3, 6:16], rtol=0, atol=8 * np.spacing(8 * np.pi))


# ----------------------------------------------------------------------------- orbits
def test_planet_ssb_and_sun(g, ctx):
    e = full_ephemeris(g)
    toas = g["toas"]
    pssb = e.get_planet_ssb(toas)
    assert pssb.shape == (len(toas), 11, 6) and not pssb[:, :, 3:].any()
    for b in range(11):
        err = np.max(np.abs(pssb[:, b, :3] - g["planet_truth"][:, b]))
        dev = np.max(np.abs(pssb[:, b, :3] - g["ref_planet"][:, b])) / np.max(np.abs(g["ref_planet"][:, b]))
        print(f"{g['names'][b]}: device error {err:.3e} = {err / g['err_planet'][b]:.3g} x the literal fp64 error; "
              f"{dev:.2e} of peak from the reference")
        assert err <= 4 * g["err_planet"][b]
        assert dev <= 1e-10
        np.testing.assert_array_equal(e.get_orbit_planet(toas, str(g["names"][b])), pssb[:, b, :3])
    sun = e.get_sunssb(toas)
    assert sun.shape == (len(toas), 3)
    err = np.max(np.abs(sun - g["sun_truth"]))
    print(f"sun (11 bodies): device error {err:.3e} = {err / g['err_sun']:.3g} x")
    assert err <= 4 * g["err_sun"]
    assert np.max(np.abs(sun - g["ref_sun"])) <= 1e-10 * np.max(np.abs(g["ref_sun"]))


def test_default_ephemeris_and_one_toa(g, ctx):
    from fakepta.ephemeris import Ephemeris
    e = Ephemeris()
    before = copy.deepcopy(e.planets)
    toas = g["toas"]
    pssb = e.get_planet_ssb(toas)
    assert pssb.shape == (len(toas), 8, 6) and not pssb[:, :, 3:].any()
    for b in range(8):
        assert np.max(np.abs(pssb[:, b, :3] - g["planet_truth"][:, b])) <= 4 * g["err_planet"][b]
    sun8 = e.get_sunssb(toas)
    assert np.max(np.abs(sun8 - g["sun8_truth"])) <= 4 * g["err_sun8"]
    assert np.max(np.abs(sun8 - g["ref_sun8"])) <= 1e-10 * np.max(np.abs(g["ref_sun8"]))
    one = e.get_planet_ssb(toas[:1])  # the 1-TOA pulsar
    assert one.shape == (1, 8, 6)
    np.testing.assert_array_equal(one, pssb[:1])
    np.testing.assert_array_equal(e.get_sunssb(toas[:1]), sun8[:1])
    assert e.get_planet_ssb(toas[:0]).shape == (0, 8, 6)
    assert e.planets == before


# ----------------------------------------------------------------------------- Roemer delay
@pytest.mark.parametrize("r", range(12))
def test_roemer_accuracy_per_row(g, separate, r):
    err = np.max(np.abs(separate[r] - g["roemer_truth"][r]))
    peak = np.max(np.abs(g["roemer_truth"][r]))
    print(f"row {r}: device error {err:.3e} = {err / g['err_roemer'][r]:.3g} x the literal fp64 error "
          f"({err / peak:.1e} of peak)")
    assert err <= 4 * g["err_roemer"][r]
    if r < 4:  # d_mass only: the one case in which the reference's roemer_delay is right
        assert np.max(np.abs(separate[r] - g["ref_roemer"][r])) <= 1e-10 * np.max(np.abs(g["ref_roemer"][r]))
    elif r < 10:  # one element deviation: the reference returns exactly 0
        assert np.max(np.abs(separate[r])) >= 0.5 * peak > 0


def test_class_roemer_delay_leaves_planets_unchanged(g, separate, ctx):
    e = full_ephemeris(g)
    before = copy.deepcopy(e.planets)
    offs, p = g["offs"], 3
    sl = slice(offs[p], offs[p + 1])
    for r in (0, 7, 10, 11):
        planet = str(g["names"][g["row_body"][r]])
        np.testing.assert_array_equal(e.roemer_row(planet, **deviations(g["rows"][r])), g["rows"][r])
        first = e.roemer_delay(g["toas"][sl], g["pos"][p], planet, **deviations(g["rows"][r]))
        again = e.roemer_delay(g["toas"][sl], g["pos"][p], planet, **deviations(g["rows"][r]))
        np.testing.assert_array_equal(first, again)  # bitwise: nothing accumulates between calls
        np.testing.assert_array_equal(first, separate[r, sl])
        assert e.planets == before


def test_accumulate_is_the_ordered_sum_of_the_separate_rows(g, separate, ctx):
    offs, n = g["offs"], int(g["offs"][-1])
    want = np.zeros(n)
    for r in range(12):
        want = want + separate[r]
    got = np.zeros(n)
    ctx.roemer_accumulate(offs, g["toas"], g["pos"], g["rows"], got)
    np.testing.assert_array_equal(got, want)
    neg = np.zeros(n)
    ctx.roemer_accumulate(offs, g["toas"], g["pos"], g["rows"], neg, sign=-1.0)
    np.testing.assert_array_equal(neg, -got)
    for r in range(12):  # separate mode = twelve one-row calls
        one = np.zeros(n)
        ctx.roemer_accumulate(offs, g["toas"], g["pos"], g["rows"][r:r + 1], one)
        np.testing.assert_array_equal(one, separate[r])
    sep_neg = np.empty((12, n))
    ctx.roemer_accumulate(offs, g["toas"], g["pos"], g["rows"], sep_neg, sign=-1.0, separate=True)
    np.testing.assert_array_equal(sep_neg, -separate)


def test_guards_stay_nan_and_every_sample_is_written(g, separate, ctx):
    offs, n = g["offs"], int(g["offs"][-1])
    pad = 96
    buf = np.full(pad + 12 * n + pad, np.nan)
    ctx.roemer_accumulate(offs, g["toas"], g["pos"], g["rows"], buf[pad:pad + 12 * n].reshape(12, n), separate=True)
    assert np.isnan(buf[:pad]).all() and np.isnan(buf[-pad:]).all()
    np.testing.assert_array_equal(buf[pad:-pad].reshape(12, n), separate)  # no NaN left
    buf = np.full(pad + n + pad, np.nan)
    buf[pad:pad + n] = 0.0
    ctx.roemer_accumulate(offs, g["toas"], g["pos"], g["rows"][:3], buf[pad:pad + n])
    assert np.isnan(buf[:pad]).all() and np.isnan(buf[-pad:]).all()
    np.testing.assert_array_equal(buf[pad:-pad], (separate[0] + separate[1]) + separate[2])


def test_empty_pulsar_in_the_middle(g, separate, ctx, ephem):
    offs = g["offs"]
    with_empty = np.concatenate([offs[:3], offs[2:]])  # a 0-TOA pulsar after the second
    pos = np.concatenate([g["pos"][:2], [[0.0, 0.0, 1.0]], g["pos"][2:]])
    out = np.full((12, offs[-1]), np.nan)
    ctx.roemer_accumulate(with_empty, g["toas"], pos, g["rows"], out, separate=True)
    np.testing.assert_array_equal(out, separate)
    views = [type("P", (), dict(toas=g["toas"][with_empty[p]:with_empty[p + 1]], pos=pos[p])) for p in range(6)]
    per_psr = ephem.roemer_delay_array(views, g["rows"], separate=True)
    assert [d.shape for d in per_psr] == [(12, k) for k in (1, 63, 0, 64, 65, 130)]
    np.testing.assert_array_equal(np.concatenate(per_psr, axis=1), separate)
    summed = ephem.roemer_delay_array(views, g["rows"][:2])
    np.testing.assert_array_equal(np.concatenate(summed), separate[0] + separate[1])


def test_kernel_stats_count_the_calls(g, capi, ctx):
    ctx.set_option(capi.OPT_PROFILE, 1)
    try:
        ctx.reset_stats()
        ctx.roemer_accumulate(g["offs"], g["toas"], g["pos"], g["rows"], np.zeros(g["offs"][-1]))
        ctx.ephem_orbits(g["toas"], g["bodies"], planets=True, sun=True)
        n, ms = ctx.kernel_stats(capi.K_EPHEM)
        assert n == 2 and ms > 0
    finally:
        ctx.set_option(capi.OPT_PROFILE, 0)


# ----------------------------------------------------------------------------- drop-in
def test_pulsar_and_array_carry_planetssb(g, ctx):
    from fakepta.ephemeris import Ephemeris
    from fakepta.fake_pta import make_fake_array
    e = Ephemeris()
    psr, = make_pulsars(g, e, [4])
    assert psr.ephem is e and psr.planetssb.shape == (130, 8, 6)
    np.testing.assert_array_equal(psr.planetssb, e.get_planet_ssb(psr.toas))
    np.random.seed(3)
    psrs = make_fake_array(npsrs=3, ntoas=40, ephem=e)
    assert len(psrs) == 3
    for p in psrs:
        assert p.ephem is e and p.planetssb.shape == (len(p.toas), 8, 6) and np.isfinite(p.planetssb).all()
        np.testing.assert_array_equal(p.planetssb, e.get_planet_ssb(p.toas))


def test_add_roemer_delay_on_fixture_pulsars(g, separate, ctx):
    from fakepta.correlated_noises import add_roemer_delay, add_roemer_delay_array
    e = full_ephemeris(g)
    before = copy.deepcopy(e.planets)
    offs = g["offs"]
    psrs = make_pulsars(g, e)
    assert not any(p.residuals.any() for p in psrs)
    add_roemer_delay(psrs, "jupiter", d_mass=float(g["rows"][0, 14]))
    for p, psr in enumerate(psrs):
        sl = slice(offs[p], offs[p + 1])
        np.testing.assert_array_equal(psr.residuals, separate[0, sl])
        assert np.max(np.abs(psr.residuals - g["roemer_truth"][0, sl])) <= 4 * g["err_roemer"][0]
    # two perturbations in one call against two single calls: each sum rounds once more
    single = make_pulsars(g, e)
    for r in (1, 10):
        add_roemer_delay(single, str(g["names"][g["row_body"][r]]), **deviations(g["rows"][r]))
    both = make_pulsars(g, e)
    add_roemer_delay_array(both, [(str(g["names"][g["row_body"][r]]), deviations(g["rows"][r])) for r in (1, 10)])
    larger = max(np.max(np.abs(separate[1])), np.max(np.abs(separate[10])))
    for x, y in zip(both, single):
        assert np.max(np.abs(x.residuals - y.residuals)) <= 2 * np.spacing(larger)
    assert e.planets == before


# ----------------------------------------------------------------------------- validation
@pytest.mark.parametrize("col,value", [(12, float("nan")), (10, 0.96), (11, 8.0), (8, -5.2), (21, 0.0), (19, 0.95)])
def test_row_validation_leaves_the_output_untouched(g, capi, ctx, col, value):
    rows = g["rows"].copy()
    rows[5, col] = value
    r = np.random.default_rng(1).normal(size=g["offs"][-1])
    before = r.copy()
    with pytest.raises(capi.FptaError, match="row 5"):
        ctx.roemer_accumulate(g["offs"], g["toas"], g["pos"], rows, r)
    np.testing.assert_array_equal(r, before)
    sep = np.full((12, g["offs"][-1]), 7.0)
    with pytest.raises(capi.FptaError, match="row 5"):
        ctx.roemer_accumulate(g["offs"], g["toas"], g["pos"], rows, sep, separate=True)
    assert np.all(sep == 7.0)


def test_body_and_kepler_validation(g, capi, ctx):
    bodies = g["bodies"].copy()
    bodies[9, 11] = 2.0  # body10: e = 0.6 + 2 t passes 0.95 inside the span
    with pytest.raises(capi.FptaError, match="body 9"):
        ctx.ephem_orbits(g["toas"], bodies)
    bodies = g["bodies"].copy()
    bodies[2, 4] = np.inf
    with pytest.raises(capi.FptaError, match="body 2"):
        ctx.ephem_orbits(g["toas"], bodies, planets=False, sun=True)
    toas = g["toas"].copy()
    toas[17] = np.nan
    with pytest.raises(capi.FptaError, match="TOA 17"):
        ctx.ephem_orbits(toas, g["bodies"])
    with pytest.raises(capi.FptaError, match="element 1"):
        ctx.ephem_kepler(np.array([1.0, 2.0]), np.array([0.5, 0.951]))
    with pytest.raises(capi.FptaError, match="element 0"):
        ctx.ephem_kepler(np.array([np.nan, 2.0]), np.array([0.5, 0.5]))
    # straight at the C entry point: both outputs stay as they were
    bad = g["bodies"].copy()
    bad[9, 10] = -0.1
    n = len(g["toas"])
    pssb, sun = np.full((n, 11, 6), 5.0), np.full((n, 3), 5.0)
    rc = capi._lib.fpta_ephem_orbits(ctx._h, n, capi._ptr(g["toas"]), 11, capi._ptr(bad), capi._ptr(pssb),
                                     capi._ptr(sun))
    assert rc == -22 and b"body 9" in capi._lib.fpta_last_error(ctx._h)
    assert np.all(pssb == 5.0) and np.all(sun == 5.0)


def test_bad_arrays_raise_value_error(g, ctx):
    n = int(g["offs"][-1])
    for bad in (np.zeros(n, dtype=np.float32), np.zeros(2 * n)[::2], np.zeros(n - 1), np.zeros((12, n))):
        with pytest.raises(ValueError):
            ctx.roemer_accumulate(g["offs"], g["toas"], g["pos"], g["rows"], bad)
    with pytest.raises(ValueError):
        ctx.roemer_accumulate(g["offs"], g["toas"], g["pos"], g["rows"], np.zeros(n), separate=True)
    with pytest.raises(ValueError):
        ctx.roemer_accumulate(g["offs"], g["toas"], g["pos"][:4], g["rows"], np.zeros(n))
    r = np.random.default_rng(2).normal(size=n)
    before = r.copy()
    ctx.roemer_accumulate(g["offs"], g["toas"], g["pos"], np.zeros((0, 22)), r)  # no rows: a no-op
    np.testing.assert_array_equal(r, before)
