"""Continuous-wave source on the GPU (fpta_cw_accumulate, csrc/cw.hip) against tests/golden/g10_cw.npz.

The yardstick of every accuracy check is stored in the fixture: err_ref64[s], the measured max-abs error of the
literal fp64 numpy evaluation of the definition against the 60-digit truth (tools/gen_cw_golden.py). The device may
be 4 x that: its sincos / log1p / expm1 are a few ulp where the host libm is <= 1."""
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def g(golden):
    return golden("g10_cw.npz")


@pytest.fixture(scope="module")
def capi():
    from fakepta_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def cw():
    from fakepta_amd import cw
    return cw


@pytest.fixture()
def ctx(capi):
    c = capi.get_context()  # the context the Pulsar methods and fakepta_amd.cw use
    yield c
    c.set_option(capi.OPT_CW_SPLIT, 0)


def psr_views(g):
    offs = g["offs"]
    return [SimpleNamespace(toas=g["toas"][offs[p]:offs[p + 1]], pos=g["pos"][p], pdist=g["pdist"][p])
            for p in range(len(offs) - 1)]


def make_pulsars(g, which=range(4)):
    from fakepta.fake_pta import Pulsar
    np.random.seed(5)
    offs = g["offs"]
    out = []
    for p in which:
        psr = Pulsar(g["toas"][offs[p]:offs[p + 1]], 1e-6, g["theta"][p], g["phi"][p], pdist=tuple(g["pdist"][p]))
        psr.pos = g["pos"][p].copy()  # the fixture's doubles, whatever this host's sin / cos round to
        np.testing.assert_array_equal(psr.toas, g["toas"][offs[p]:offs[p + 1]])
        out.append(psr)
    return out


def add_cgw_args(row):
    return dict(costheta=float(row[0]), phi=float(row[1]), cosinc=float(row[2]), log10_mc=float(row[3]),
                log10_fgw=float(row[4]), log10_h=float(row[5]), phase0=float(row[6]), psi=float(row[7]),
                psrterm=bool(row[8]))


def array_args(g):
    from fakepta_amd import cw
    offs = g["offs"]
    L = np.array([cw.light_seconds(g["pdist"][p]) for p in range(len(offs) - 1)])
    return offs, g["toas"], g["pos"], L


@pytest.mark.parametrize("s", range(10))
def test_accuracy_per_source(g, cw, ctx, s):
    got = np.concatenate(cw.cw_delay_array(psr_views(g), g["src"][s]))
    err = np.max(np.abs(got - g["truth"][s]))
    print(f"source {s}: device error {err:.3e} = {err / g['err_ref64'][s]:.3g} x the literal fp64 error "
          f"({err / g['peak'][s]:.1e} of peak)")
    assert err <= 4 * g["err_ref64"][s]


def test_cw_delay_keywords(g, cw, ctx):
    """The enterprise_extensions keyword form: one pulsar, one source; log10_dist gives the same delay as the
    equivalent log10_h; toas is not modified."""
    from fakepta import constants as const
    offs, s = g["offs"], 6
    row = g["src"][s]
    toas = g["toas"][offs[2]:offs[3]].copy()
    kw = dict(cos_gwtheta=row[0], gwphi=row[1], cos_inc=row[2], log10_mc=row[3], log10_fgw=row[4], phase0=row[6],
              psi=row[7], psrTerm=True)
    got = cw.cw_delay(toas, g["pos"][2], g["pdist"][2], log10_h=row[5], **kw)
    np.testing.assert_array_equal(toas, g["toas"][offs[2]:offs[3]])
    assert np.max(np.abs(got - g["truth"][s, offs[2]:offs[3]])) <= 4 * g["err_ref64"][s]
    mc, w0 = 10 ** row[3] * const.Tsun, np.pi * 10 ** row[4]
    log10_dist = np.log10(2 * mc ** (5 / 3) * w0 ** (2 / 3) / 10 ** row[5] * const.c / const.Mpc)
    via_dist = cw.cw_delay(toas, g["pos"][2], g["pdist"][2], log10_dist=log10_dist, **kw)
    # log10 and 10** round the amplitude: ~ln(10) |log10_h| eps relative
    np.testing.assert_allclose(via_dist, got, rtol=0, atol=64 * EPS * g["peak"][s])


@pytest.mark.parametrize("split", [0, 1, 3, 10])
def test_all_sources_at_once(g, capi, ctx, split):
    offs, toas, pos, L = array_args(g)
    ctx.set_option(capi.OPT_CW_SPLIT, split)
    assert ctx.get_option(capi.OPT_CW_SPLIT) == split
    got = np.zeros(offs[-1])
    ctx.cw_accumulate(offs, toas, pos, L, g["src"], got)
    again = np.zeros(offs[-1])
    ctx.cw_accumulate(offs, toas, pos, L, g["src"], again)
    np.testing.assert_array_equal(got, again)  # bitwise: the summation order is fixed by (S, n_toa, option)
    want = g["truth"].sum(axis=0)
    bound = 4 * g["err_ref64"].sum()
    for p in range(4):  # the 1-, 63-, 257- and 70-TOA pulsars each: the partial-wave guards
        err = np.max(np.abs(got[offs[p]:offs[p + 1]] - want[offs[p]:offs[p + 1]]))
        print(f"split {split}, pulsar {p}: error {err:.3e}, bound {bound:.3e}")
        assert err <= bound


def test_kernel_stats_count_the_call(g, capi, ctx):
    offs, toas, pos, L = array_args(g)
    ctx.set_option(capi.OPT_PROFILE, 1)
    try:
        ctx.reset_stats()
        ctx.cw_accumulate(offs, toas, pos, L, g["src"], np.zeros(offs[-1]))
        n, ms = ctx.kernel_stats(capi.K_CW)
        assert n == 1 and ms > 0
    finally:
        ctx.set_option(capi.OPT_PROFILE, 0)


@pytest.mark.parametrize("col,value", [(4, float("nan")), (0, 1.0000001), (2, -1.5), (4, -6.0)])
def test_validation_leaves_residuals_unchanged(g, capi, ctx, col, value):
    offs, toas, pos, L = array_args(g)
    src = g["src"].copy()
    src[7, col] = value  # (4, -6.0): source 7 (log10_mc 8) coalesces inside the data span
    r = np.random.default_rng(1).normal(size=offs[-1])
    before = r.copy()
    with pytest.raises(capi.FptaError, match="source 7"):
        ctx.cw_accumulate(offs, toas, pos, L, src, r)
    np.testing.assert_array_equal(r, before)


def test_bad_arrays_raise_value_error(g, ctx):
    offs, toas, pos, L = array_args(g)
    for bad in (np.zeros(offs[-1], dtype=np.float32), np.zeros(2 * offs[-1])[::2], np.zeros(offs[-1] - 1)):
        with pytest.raises(ValueError):
            ctx.cw_accumulate(offs, toas, pos, L, g["src"], bad)
    with pytest.raises(ValueError):
        ctx.cw_accumulate(offs, toas, pos[:3], L, g["src"], np.zeros(offs[-1]))


def test_no_sources_is_a_no_op(g, ctx):
    offs, toas, pos, L = array_args(g)
    r = np.random.default_rng(2).normal(size=offs[-1])
    before = r.copy()
    ctx.cw_accumulate(offs, toas, pos, L, np.zeros((0, 9)), r)
    np.testing.assert_array_equal(r, before)


@pytest.mark.parametrize("split", [0, 3])
def test_add_then_subtract(g, capi, ctx, split):
    offs, toas, pos, L = array_args(g)
    ctx.set_option(capi.OPT_CW_SPLIT, split)
    delay = np.zeros(offs[-1])
    ctx.cw_accumulate(offs, toas, pos, L, g["src"], delay)
    peak = np.max(np.abs(delay))
    before = np.random.default_rng(3).uniform(-peak, peak, offs[-1])
    r = before.copy()
    ctx.cw_accumulate(offs, toas, pos, L, g["src"], r, sign=1.0)
    np.testing.assert_allclose(r, before + delay, rtol=0, atol=4 * EPS * peak)
    ctx.cw_accumulate(offs, toas, pos, L, g["src"], r, sign=-1.0)
    # (r + d) - d: two roundings of numbers below 2 peak
    assert np.max(np.abs(r - before)) <= 4 * EPS * peak


def test_drop_in_add_reconstruct_remove(g, ctx):
    offs = g["offs"]
    psr, = make_pulsars(g, [2])
    sl = slice(offs[2], offs[3])
    a, b = 1, 6  # log10_mc 9, log10_fgw -8: without and with the pulsar term
    want = g["truth"][a, sl] + g["truth"][b, sl]
    bound = 4 * (g["err_ref64"][a] + g["err_ref64"][b])
    assert not psr.residuals.any()
    psr.add_cgw(**add_cgw_args(g["src"][a]))
    psr.add_cgw(**add_cgw_args(g["src"][b]))
    assert np.max(np.abs(psr.residuals - want)) <= bound
    assert list(psr.signal_model["cgw"]) == ["0", "1"]
    for key, row in (("0", g["src"][a]), ("1", g["src"][b])):
        assert psr.signal_model["cgw"][key] == add_cgw_args(row)
        assert list(psr.signal_model["cgw"][key]) == ["costheta", "phi", "cosinc", "log10_mc", "log10_fgw", "log10_h",
                                                      "phase0", "psi", "psrterm"]
    rec = psr.reconstruct_signal(["cgw"])
    assert np.max(np.abs(rec - want)) <= bound
    assert np.max(np.abs(rec - psr.residuals)) <= bound
    # something else in the residuals besides the wave, so that removing it has to round
    start = np.random.default_rng(4).uniform(-0.1, 0.1, len(psr.toas)) * np.max(np.abs(rec))
    psr.residuals += start
    psr.remove_signal(["cgw"])
    assert "cgw" not in psr.signal_model
    assert np.max(np.abs(psr.residuals - start)) <= 4 * EPS * np.max(np.abs(rec))


def test_add_cgw_array(g, ctx):
    from fakepta.fake_pta import add_cgw_array, reconstruct_array
    offs, src = g["offs"], g["src"]
    one_by_one = make_pulsars(g)
    for psr in one_by_one:
        for row in src:
            psr.add_cgw(**add_cgw_args(row))
    psrs = make_pulsars(g)
    add_cgw_array(psrs, src, record=True)
    bound = 4 * g["err_ref64"].sum()
    want = g["truth"].sum(axis=0)
    for p, (x, y) in enumerate(zip(psrs, one_by_one)):
        assert np.max(np.abs(x.residuals - y.residuals)) <= bound
        assert np.max(np.abs(x.residuals - want[offs[p]:offs[p + 1]])) <= bound
        assert x.signal_model == y.signal_model and list(x.signal_model["cgw"]) == [str(i) for i in range(10)]
    # the array reconstruction takes 'cgw' too, and the dict form of the sources gives the same injection
    for x, rec in zip(psrs, reconstruct_array(psrs, ["cgw"])):
        assert np.max(np.abs(rec - x.residuals)) <= bound
    quiet = make_pulsars(g)
    add_cgw_array(quiet, {k: src[:, i] for i, k in enumerate(("costheta", "phi", "cosinc", "log10_mc", "log10_fgw",
                                                               "log10_h", "phase0", "psi", "psrterm"))},
                  record=False)
    for x, q in zip(psrs, quiet):
        np.testing.assert_array_equal(q.residuals, x.residuals)
        assert q.signal_model == {}
