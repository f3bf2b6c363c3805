"""Continuous-wave F-statistics on the device (fpta_fe_statistic, fpta_batch_set_fe, fpta_batch_fe: k_fit_apply on its
fourth operator slot, k_fe_sky, k_fe_reduce) and the Python surface above it, against the np.longdouble definition of
tests/fe_reference.py.

Stage 1, X = B_p r, per pulsar and row: |got - truth| <= max(4 e_lit, (n_p + 2) eps sum_t |B_kt| |r_t|), DESIGN.md
section 5i's rule. Stage 2 is held to the definition applied in longdouble to the device's own X and the host's own fp64
tables: |dFe| <= (P + 16) eps sum_ij S_i |Minv_ij| S_j with S_i = sum_p |F_ip| |x_p| (an MFMA dot product of length P in
any order with once-rounded F, the <= 28 roundings of the quadratic form and the rounding of Minv), |dFp| <= (3 P + 6) eps
sum |terms|. Maxima, argmax, NaN and bit identities are compared exactly."""
import numpy as np
import pytest

from tests import fe_reference as FE
from tests import os_reference as OS
from tests import tm_reference as T
from tests import test_fe_host as FH
from tests import test_gpu_os as GO

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
LD = np.longdouble
YEAR = 365.25 * 86400.0
SPAN = 15 * YEAR


@pytest.fixture(scope="module")
def capi():
    from fakepta_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def ctx(capi):
    c = capi.Context(0)
    yield c
    c.close()


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


# ----------------------------------------------------------------------------- stage 1: X against the truth
N_PSR = (0, 1, 5, 16, 17, 33, 250)
M_PSR = (3, 0, 3, 0, 3, 16, 8)
N_VEC = 17
_RAGGED = {}


def ragged(G):
    """The ragged array (0, 1, 5, 16, 17, 33 and 250 TOAs; 0, 3, 8 and 16 design columns) under a red process of 6 modes
    and G frequencies drawn log-uniformly in [1, 60] / span, unordered; the truth and the literal form, made once."""
    if G not in _RAGGED:
        from fakepta_amd import tm
        rng = np.random.default_rng(4000 + G)
        psrs = []
        for n, m in zip(N_PSR, M_PSR):
            t = np.sort(rng.uniform(0.0, SPAN, n))
            nu = T.three_band(rng, n)
            full = np.concatenate([T.mmat(t, nu), T.smooth_columns(rng, t, 8) if n else np.zeros((0, 8))], axis=1)
            psrs.append((t, nu, np.ascontiguousarray(full[:, :m]), 1 / rng.uniform(1e-7, 1e-6, n) ** 2))
        P = len(psrs)
        offs = np.concatenate([[0], np.cumsum(N_PSR)]).astype(np.int64)
        red = np.arange(1, 7) / SPAN
        phi = np.stack([10.0 * (2.0 / np.sum(p[3]) if len(p[0]) else 1e-14) * np.arange(1, 7) ** -3.0 for p in psrs])
        fgw = np.exp(rng.uniform(np.log(1.0), np.log(60.0), G)) / SPAN
        pos = unit(rng.normal(size=(P, 3)))
        sky = np.array([[0.2, 1.0]])
        tr = FE.plan_ld(psrs, lambda p: [(red, 0.0, 1400.0)], lambda p: [phi[p]], lambda p: None, fgw, sky, pos)
        res = rng.normal(0.0, 1e-6, (N_VEC, int(offs[-1])))
        truth, bound = OS.x_truth(tr["B"], offs, res)
        lits = []
        for p, (t, nu, M, w) in enumerate(psrs):
            if len(t) == 0:
                lits.append(np.zeros((2 * G, 0)))
                continue
            T.assert_clear_rank(tr["norms"][p], tr["keep"][p], M)
            lit = OS.operator_literal(t, nu, M, w, [(red, 0.0, 1400.0), (fgw, 0.0, 1400.0)], [phi[p], np.zeros(G)], 1,
                                      tr["keep"][p])
            lit[np.concatenate([tr["dropped"][p], tr["dropped"][p]])] = 0.0
            lits.append(lit)
        literal = np.stack([lits[p] @ res[:, int(offs[p]):int(offs[p + 1])].T for p in range(P)])
        M, ncol = tm.stack_design([p[2] for p in psrs])
        _RAGGED[G] = dict(offs=offs, toas=np.concatenate([p[0] for p in psrs]), nu=np.concatenate([p[1] for p in psrs]),
                          w=np.concatenate([p[3] for p in psrs]), M=M, ncol=ncol, n_modes=np.array([6], dtype=np.int32),
                          f=red, idx=np.zeros(1), freqf=np.full(1, 1400.0), phi=phi, fgw=fgw, sky=sky, pos=pos, res=res,
                          truth=truth, bound=bound, literal=literal, tr=tr)
    return _RAGGED[G]


def one_shot(ctx, c, res, **kw):
    return ctx.fe_statistic(c["offs"], c["toas"], c["nu"], c["n_modes"], c["f"], c["idx"], c["freqf"], c["phi"],
                            c["fgw"], c["sky"], c["pos"], res, M=c.get("M"), ncol_psr=c.get("ncol"), weights=c["w"], **kw)


# K = 2 G = 2, 16, 18, 60, 208 and 512 cross k_fit_apply's instances
@pytest.mark.parametrize("G", [1, 8, 9, 30, 104, 256])
def test_one_shot_x_matches_the_truth(ctx, G):
    c = ragged(G)
    out, rank, tab = one_shot(ctx, c, c["res"], coefficients=True, tables=True)
    P = len(N_PSR)
    assert out["X"].shape == (P, 2 * G, N_VEC) and list(rank) == [int(k.sum()) for k in c["tr"]["keep"]]
    GO.check_x(f"G {G}", out["X"], c["truth"], c["literal"], c["bound"], N_PSR)
    assert np.array_equal(tab["n_eff"], c["tr"]["n_eff"])
    # one direction, every pulsar's TOAs few against K: whatever is regular is the definition applied to X
    check_stage2(f"ragged G {G}", out, tab, full=False)


# ----------------------------------------------------------------------------- stage 2: k_fe_sky, k_fe_reduce
SHAPES, sky_case, shape_inputs = FH.SHAPES, FH.sky_case, FH.shape_inputs  # the inputs: tests/test_fe_host.py


def check_stage2(label, out, tab, full=True):
    """Fe (the map, or the maxima when the map was not asked for), Fp against the definition applied to the device's X
    and the host's tables within the derived bounds; the maxima and argmax bit for bit the definition's reductions of
    the device's own map; the argmax equal to the truth's wherever the truth's top-two gap exceeds twice the bound.
    Returns (worst Fe ratio, worst Fp ratio, (g, r) cases skipped for a smaller gap, (g, r) cases with a maximum)."""
    st = FE.statistics_ld(out["X"], tab["F"], tab["Minv"], tab["minv"])
    efp = np.abs(out["Fp"].astype(LD) - st["Fp"]).astype(np.float64)
    r_fp = float(np.max(efp / np.maximum(st["Fp_bound"], 1e-300), initial=0.0))
    assert np.all(efp <= st["Fp_bound"]), (label, r_fp)
    tru = st["Fe"].astype(np.float64)
    sing = np.isnan(tab["Minv"]).any(axis=2)
    r_fe, n_skip, n_dec = 0.0, 0, 0
    if full:
        fe = out["Fe"]
        assert np.array_equal(np.isnan(fe), np.broadcast_to(sing[:, :, None], fe.shape)), label
        err = np.where(np.isnan(fe), 0.0, np.abs(fe.astype(LD) - st["Fe"]).astype(np.float64))
        r_fe = float(np.max(err / np.maximum(st["Fe_bound"], 1e-300), initial=0.0))
        assert np.all(err <= st["Fe_bound"]), (label, r_fe)
        fef, af, fem, am = FE.reduce_map(fe)
        np.testing.assert_array_equal(out["Fe_f"], fef)
        np.testing.assert_array_equal(out["argmax_f"], af)
        np.testing.assert_array_equal(out["Fe_max"], fem)
        np.testing.assert_array_equal(out["argmax"], am)
        # against the truth's own argmax where its top two are further apart than twice the bound
        tf, taf = FE.nanmax_first(tru, axis=0)
        bnd = np.where(sing[:, :, None], 0.0, st["Fe_bound"])
        second = np.where(np.arange(tru.shape[0])[:, None, None] == taf[None], -np.inf, np.where(np.isnan(tru), -np.inf, tru))
        gap = tf - np.max(second, axis=0)
        clear = (taf >= 0) & (gap > 2 * np.max(bnd, axis=0))
        decided = taf >= 0
        n_skip, n_dec = int(np.sum(decided & ~clear)), int(np.sum(decided))
        assert np.array_equal(out["argmax_f"][clear], taf[clear]), label
        assert np.array_equal(out["argmax_f"] < 0, ~decided)
    else:
        # the per-frequency maxima are the truth's at the device's own argmax, within the bound there
        a = out["argmax_f"]
        ok = a >= 0
        g_i, r_i = np.nonzero(ok)
        got = out["Fe_f"][ok]
        want, bd = st["Fe"][a[ok], g_i, r_i], st["Fe_bound"][a[ok], g_i, r_i]
        err = np.abs(got.astype(LD) - want).astype(np.float64)
        r_fe = float(np.max(err / np.maximum(bd, 1e-300), initial=0.0))
        assert np.all(err <= bd), (label, r_fe)
        assert np.all(np.isnan(out["Fe_f"][~ok])) and np.array_equal(~ok, np.broadcast_to(sing.all(axis=0)[:, None], ok.shape))
    print(f"{label}: Fe error / bound {r_fe:.4f}, Fp error / bound {r_fp:.4f}, argmax cases skipped for a small gap "
          f"{n_skip} of {n_dec}")
    return r_fe, r_fp, n_skip, n_dec


_ARGMAX = {}  # shape -> ((g, r) cases skipped for a small gap, cases with a maximum), filled by run_shape


def run_shape(ctx, P, S, G, R):
    c, res = shape_inputs(P, S, G, R)
    out, _, tab = one_shot(ctx, c, res, full=True, coefficients=True, tables=True)
    assert out["Fe"].shape == (S, G, R) and out["Fp"].shape == (G, R) and out["argmax"].shape == (2, R)
    sing = np.isnan(tab["Minv"]).any(axis=2)
    if P == 1:
        assert sing.all() and np.isnan(out["Fe"]).all() and np.isnan(out["Fe_max"]).all() and np.isnan(out["Fe_f"]).all()
        assert np.all(out["argmax"] == -1) and np.all(out["argmax_f"] == -1)
    else:
        pole = (np.arange(S) == 3) & (S >= 7)  # the deliberately singular direction in the middle of the first tile
        assert np.array_equal(sing.all(axis=1), pole) and not sing[~pole].any()
        assert np.all(out["argmax_f"] != 3) or S < 7
        assert np.all(out["Fe_max"] > 0)
    assert list(tab["n_eff"]) == [P] * G and np.all(out["Fp"] > 0)
    got = check_stage2(f"P {P} n_sky {S} G {G} R {R}", out, tab)
    _ARGMAX[(P, S, G, R)] = got[2:]
    return got


@pytest.mark.parametrize("P,S,G,R", SHAPES)
def test_stage_2_is_the_definition_applied_to_the_device_x(ctx, P, S, G, R):
    run_shape(ctx, P, S, G, R)


def test_device_argmax_is_the_truths_in_all_but_a_few_cases(ctx):
    """Over all shapes together, at most 5 % of the (g, r) cases have a top-two gap of the truth within twice the bound
    and are left out of the argmax comparison (P = 2 always is: every regular direction gives the same Fe). The counts
    are those of the parametrized runs above; a shape that has not run yet (this test selected alone) runs here."""
    for shape in SHAPES:
        if shape not in _ARGMAX:
            run_shape(ctx, *shape)
    n_skip, n_dec = (sum(_ARGMAX[shape][i] for shape in SHAPES) for i in (0, 1))
    print(f"argmax: {n_skip} of {n_dec} (g, r) cases skipped for a small gap ({100 * n_skip / n_dec:.2f} %)")
    assert n_skip <= 0.05 * n_dec and n_dec == FH.argmax_gap_counts()[1]


def test_blocks_and_order_do_not_change_a_bit(ctx):
    """A realization's numbers are the same bits alone, among the first 16, among all 33 and in reversed order."""
    c = sky_case(17, 12, 5, 7)
    res = np.random.default_rng(3).normal(0.0, 3e-7, (33, int(c["offs"][-1])))
    full, _, _ = one_shot(ctx, c, res, full=True, coefficients=True)
    for sel in ([0], [32], list(range(16)), list(range(32, -1, -1)), [5, 31, 6]):
        got, _, _ = one_shot(ctx, c, np.ascontiguousarray(res[sel]), full=True, coefficients=True)
        for key in ("Fe_max", "argmax", "Fe_f", "argmax_f", "Fp", "Fe", "X"):
            np.testing.assert_array_equal(got[key], full[key][..., sel], err_msg=key)


# ----------------------------------------------------------------------------- batch path and end to end
class _Psr:
    """What BatchSimulator, add_cgw and the drop-in call read of a pulsar."""

    def __init__(self, toas, freqs, sigma2, pos, Mmat, signal_model):
        self.toas, self.freqs, self.sigma2, self.pos, self.Mmat = toas, freqs, sigma2, pos, Mmat
        self.signal_model, self.pdist = signal_model, (1.0, 0.2)
        self.residuals = np.zeros(len(toas))

    def _white_sigma2(self):
        return self.sigma2


NSIDE, PIX, G_INJ = 2, 21, 3


FGW12 = np.array([4.3e-9, 2.9e-8, 7.7e-9, 1e-8, 1.7e-8, 5.1e-8])


def pulsars12():
    """12 pulsars of 128 .. 200 TOAs over 15 yr with a weak red process of 4 modes each, a weak uncorrelated common
    process of 4 modes, white noise and a 3-column design."""
    rng = np.random.default_rng(2027)
    P = 12
    counts = rng.integers(128, 201, size=P)
    pos = unit(rng.normal(size=(P, 3)))
    f4 = np.arange(1, 5) / SPAN
    psrs = []
    for i, n in enumerate(counts):
        t = np.sort(rng.uniform(0.0, SPAN, n))
        sm = {"red_noise": dict(f=f4, psd=1e-30 * np.arange(1, 5) ** -3.0 * SPAN * rng.uniform(0.5, 2.0), idx=0.0),
              "gw_common": dict(f=f4, psd=3e-31 * np.arange(1, 5) ** -4.33 * SPAN, idx=0.0, orf="curn")}
        psrs.append(_Psr(t, np.full(n, 1400.0), rng.uniform(2e-7, 5e-7, n) ** 2, pos[i],
                         np.stack([np.ones(n), t / SPAN, (t / SPAN) ** 2], axis=1), sm))
    return psrs


@pytest.fixture(scope="module")
def array12(ctx):
    """pulsars12() as a BatchSimulator; 6 frequencies with 1e-8 Hz among them; the nside-2 sky."""
    from fakepta_amd.batch import BatchSimulator
    from fakepta_amd import fe as fem
    psrs = pulsars12()
    f4 = psrs[0].signal_model["gw_common"]["f"]
    sim = BatchSimulator(psrs, signals=[], white=True, ctx=ctx)
    sim._add_named("red_noise")
    sm0 = psrs[0].signal_model["gw_common"]
    sim.add_signal("gw_common", 1, f4, np.sqrt(sm0["psd"] * np.diff(np.append(0.0, f4))), L=np.eye(len(psrs)))
    return sim, psrs, FGW12, fem.sky_grid(nside=NSIDE)


def source(sky, fgw, log10_h):
    return np.array([[sky[PIX, 0], sky[PIX, 1], 0.3, 8.5, np.log10(fgw[G_INJ]), log10_h, 1.1, 0.4, 0.0]])


_E2E = {}


def truth12(psrs, fgw, sky):
    if "plan" not in _E2E:
        tabs = [(p.toas, p.freqs, p.Mmat, 1 / p.sigma2) for p in psrs]

        def comps_of(p):
            return [(psrs[p].signal_model[k]["f"], 0.0, 1400.0) for k in ("red_noise", "gw_common")]

        def phis_of(p):
            return [psrs[p].signal_model[k]["psd"] * np.diff(np.append(0.0, psrs[p].signal_model[k]["f"]))
                    for k in ("red_noise", "gw_common")]

        tr = FE.plan_ld(tabs, comps_of, phis_of, lambda p: None, fgw, sky, np.array([p.pos for p in psrs]))
        lits = []
        for p, (t, nu, M, w) in enumerate(tabs):
            T.assert_clear_rank(tr["norms"][p], tr["keep"][p], M)
            lits.append(OS.operator_literal(t, nu, M, w, comps_of(p) + [(fgw, 0.0, 1400.0)],
                                            phis_of(p) + [np.zeros(len(fgw))], 2, tr["keep"][p]))
        assert not tr["dropped"].any()
        _E2E["plan"] = (tr, lits)
    return _E2E["plan"]


def composed(psrs, fgw, sky, block, s, g):
    """(Fe truth [R] at (s, g) from the truth's B and tables, the bound a device result is held to): X within its
    stage-1 tolerance dX, F within 1 eps of its scale, Minv within the host test's bound, then the stage-2 bound."""
    tr, lits = truth12(psrs, fgw, sky)
    offs = np.concatenate([[0], np.cumsum([len(p.toas) for p in psrs])]).astype(np.int64)
    P, G = len(psrs), len(fgw)
    Xt, xb = OS.x_truth(tr["B"], offs, block)
    lit = np.stack([lits[p] @ block[:, offs[p]:offs[p + 1]].T for p in range(P)])
    dX = OS.x_tolerance(Xt, lit, xb)[0]
    F2 = tr["F"][2 * s:2 * s + 2]  # [2, P]
    dF = EPS * tr["F_scale"][2 * s:2 * s + 2].astype(np.float64)
    rows = [(0, G + g), (0, g), (1, G + g), (1, g)]  # N = [F+ x_s, F+ x_c, Fx x_s, Fx x_c]
    N = np.stack([F2[a] @ Xt[:, k, :] for a, k in rows])
    aF = np.abs(F2).astype(np.float64)
    aX = np.abs(Xt).astype(np.float64)
    S = np.stack([(aF[a] + dF[a]) @ (aX[:, k, :] + dX[:, k, :]) for a, k in rows])
    e = np.stack([aF[a] @ dX[:, k, :] + dF[a] @ (aX[:, k, :] + dX[:, k, :]) for a, k in rows])
    Mi = np.zeros((4, 4), dtype=LD)
    for k, (i, j) in enumerate(FE.TRI4):
        Mi[i, j] = Mi[j, i] = tr["Minv"][s, g, k]
    aM = np.abs(Mi).astype(np.float64)
    dM = FE.inverse_bound(tr["kappa_M"][s, g]) * float(np.max(aM)) + EPS * aM
    fe = LD(0.5) * np.einsum("ir,ij,jr->r", N, Mi, N)
    aN = np.abs(N).astype(np.float64)
    bound = 0.5 * np.einsum("ir,ij,jr->r", aN, aM, e) * 2 + 0.5 * np.einsum("ir,ij,jr->r", e, aM, e) \
        + 0.5 * np.einsum("ir,ij,jr->r", aN + e, dM, aN + e) + (P + 16) * EPS * np.einsum("ir,ij,jr->r", S, aM + dM, S)
    return fe.astype(np.float64), bound, tr


def test_batch_statistic_end_to_end(ctx, capi, array12):
    sim, psrs, fgw, sky = array12
    rank = sim.set_fe_statistic(fgw, nside=NSIDE)
    assert list(rank) == [3] * 12 and ctx.batch_fe_info() == dict(K=12, G=6, n_sky=48, n_real=0)
    tr, _ = truth12(psrs, fgw, sky)
    # the amplitude that gives (h|h) = 400: Fe of the noise-free signal at its own grid point is (h|h) / 2
    offs = sim.offs
    h0 = np.zeros((1, sim.n_toa))
    from fakepta_amd import cw
    h0[0] = np.concatenate(cw.cw_delay_array(psrs, source(sky, fgw, -14.0)))
    fe0, _, _ = composed(psrs, fgw, sky, h0, PIX, G_INJ)
    log10_h = -14.0 + 0.5 * np.log10(400.0 / (2 * fe0[0]))
    R = 16
    sim.synth(R, seed=11, to_host=False)
    null = sim.fe_statistic()
    sim.add_cgw(source(sky, fgw, log10_h))
    before = sim.checksums()
    out = sim.fe_statistic(full=True)
    np.testing.assert_array_equal(sim.checksums(), before)  # the block is untouched
    assert ctx.batch_fe_info()["n_real"] == R and out["Fe"].shape == (48, 6, R) and list(out["n_eff"]) == [12] * 6
    block = ctx.batch_download(0, R)
    want, bound, _ = composed(psrs, fgw, sky, block, PIX, G_INJ)
    err = np.abs(out["Fe"][PIX, G_INJ] - want)
    print(f"end to end: log10_h {log10_h:.3f} for (h|h) = 400; Fe at the injected point {want.min():.1f} .. "
          f"{want.max():.1f} (null block there: {null['Fe_f'][G_INJ].mean():.2f} on average over the sky maximum); "
          f"largest error / composed bound {float(np.max(err / bound)):.3e}")
    assert np.all(err <= bound)
    # the truth's argmax is the injected (pixel, frequency) in every realization, and so is the device's
    Xt, _ = OS.x_truth(tr["B"], offs, block)
    st = FE.statistics_ld(Xt.astype(np.float64), tr["F"].astype(np.float64), tr["Minv"].astype(np.float64),
                          tr["minv"].astype(np.float64))
    _, _, _, am = FE.reduce_map(st["Fe"].astype(np.float64))
    assert np.all(am[0] == PIX) and np.all(am[1] == G_INJ)
    np.testing.assert_array_equal(out["argmax"], am)
    assert np.all(out["fgw_ml"] == fgw[G_INJ]) and np.all(out["cos_gwtheta_ml"] == sky[PIX, 0])
    assert np.all(out["gwphi_ml"] == sky[PIX, 1]) and np.all(out["fap_max"] < 1e-30)
    fef, af, fmax, amax = FE.reduce_map(out["Fe"])
    for a, b in ((out["Fe_f"], fef), (out["argmax_f"], af), (out["Fe_max"], fmax), (out["argmax"], amax)):
        np.testing.assert_array_equal(a, b)
    # the drop-in form on a downloaded realization gives the same bits
    from fakepta import fake_pta as fp
    for r in (0, R - 1):
        for p, o0, o1 in zip(psrs, offs[:-1], offs[1:]):
            p.residuals = block[r, o0:o1].copy()
        one = fp.fe_statistic_array(psrs, fgw, nside=NSIDE, full=True)
        for key in ("Fe_max", "argmax", "Fe_f", "argmax_f", "Fp", "Fe", "fgw_ml", "cos_gwtheta_ml", "gwphi_ml"):
            np.testing.assert_array_equal(one[key][..., 0], out[key][..., r], err_msg=key)


def test_null_block_has_the_chi_square_mean(ctx, array12):
    sim, psrs, fgw, sky = array12
    sim.set_fe_statistic(fgw, nside=NSIDE)
    R = 48
    sim.synth(R, seed=23, to_host=False)
    out = sim.fe_statistic(full=True)
    m = float(np.mean(2 * out["Fe"][PIX, G_INJ]))
    z = (m - 4.0) / np.sqrt(8.0 / R)
    zp = (np.mean(2 * out["Fp"], axis=1) - 24.0) / np.sqrt(4.0 * 12 / R)
    print(f"null block: mean 2 Fe at the point = {m:.3f} against 4 +- {np.sqrt(8.0 / R):.3f} ({z:+.2f} sigma); mean 2 Fp "
          f"against 24: {np.array2string(zp, precision=2)} sigma")
    assert abs(z) <= 4


def test_white_noise_only_layout_batch_and_drop_in_agree(capi):
    """A layout without a Gaussian process: set_fe_statistic and fe_statistic_array both pass one component with phi =
    0, and the library gives the bits of a call without any component. On a context of its own: a new BatchSimulator
    replaces the context's layout."""
    from fakepta import fake_pta as fp
    from fakepta_amd.batch import BatchSimulator
    from fakepta_amd import fe as fem, tm
    psrs = pulsars12()[:4]
    for p in psrs:
        p.signal_model = {}
    c = capi.Context(0)
    try:
        sim = BatchSimulator(psrs, signals=[], white=True, ctx=c)
        fgw, sky = FGW12[:3], fem.sky_grid(nside=1)
        assert list(sim.set_fe_statistic(fgw, sky=sky)) == [3] * 4
        sim.synth(5, seed=3, to_host=False)
        out = sim.fe_statistic(full=True)
        assert not np.isnan(out["Fe"]).any() and list(out["n_eff"]) == [4] * 3
        block = c.batch_download(0, 5)
        for p, o0, o1 in zip(psrs, sim.offs[:-1], sim.offs[1:]):
            p.residuals = block[2, o0:o1].copy()
        one = fp.fe_statistic_array(psrs, fgw, sky=sky, full=True)
        M, ncol = tm.stack_design([p.Mmat for p in psrs])
        bare, _, _ = c.fe_statistic(sim.offs, sim.toas, sim.freqs, None, None, None, None, None, fgw, sky,
                                    np.array([p.pos for p in psrs]), block[2], M=M, ncol_psr=ncol,
                                    weights=np.concatenate([1 / p.sigma2 for p in psrs]), full=True)
        for key in ("Fe_max", "argmax", "Fe_f", "argmax_f", "Fp", "Fe"):
            np.testing.assert_array_equal(one[key][..., 0], out[key][..., 2], err_msg=key)
            np.testing.assert_array_equal(bare[key][..., 0], out[key][..., 2], err_msg=key)
    finally:
        c.close()


def test_the_other_consumers_keep_their_bits_and_set_toas_clears(ctx, capi, array12):
    sim, psrs, fgw, sky = array12
    ctx.batch_set_fe(None, None, None, None, None, None, None, None, clear=True)
    with pytest.raises(capi.FptaError, match=r"\(-77\).*no F-statistic is set"):
        sim.synth(20, seed=9, to_host=False)
        ctx.batch_fe()
    sim.set_fourier_fit([(4, 0.0)])
    sim.set_optimal_statistic()
    sim.set_likelihood_grid(phi=np.stack([sim.segments[1]["amp"] ** 2, 3.0 * sim.segments[1]["amp"] ** 2]))
    coef0, (Q0, _, XO0), (d0, q0, XL0) = (sim.fourier_fit(), ctx.batch_os(coefficients=True),
                                          ctx.batch_lnl(per_pulsar=True, coefficients=True))
    sim.set_fe_statistic(fgw[:3], sky=sky[:9])
    fe0 = ctx.batch_fe(full=True, coefficients=True)
    for _ in range(2):  # all four set, in turn, twice
        np.testing.assert_array_equal(sim.fourier_fit(), coef0)
        fe1 = ctx.batch_fe(full=True, coefficients=True)
        Q1, _, XO1 = ctx.batch_os(coefficients=True)
        d1, q1, XL1 = ctx.batch_lnl(per_pulsar=True, coefficients=True)
        for a, b in ((Q1, Q0), (XO1, XO0), (d1, d0), (q1, q0), (XL1, XL0)):
            np.testing.assert_array_equal(a, b)
        for key in fe0:
            np.testing.assert_array_equal(fe1[key], fe0[key], err_msg=key)
    assert fe0["X"].shape == (12, 6, 20) and np.any(fe0["X"] != 0) and not np.isnan(fe0["Fe"]).any()
    ctx.set_option(capi.OPT_PROFILE, 1)  # one FPTA_K_DENSE entry per call, both stages
    ctx.reset_stats()
    ctx.batch_fe()
    ctx.synchronize()
    assert ctx.kernel_stats(capi.K_DENSE)[0] == 1
    ctx.set_option(capi.OPT_PROFILE, 0)
    for clear in (lambda: ctx.batch_set_fit(None, None, None, None),
                  lambda: ctx.batch_set_os(None, None, None, None, None, 0, None, None),
                  lambda: ctx.batch_set_lnl(None, None, None, None, None, 0, None)):
        clear()
    np.testing.assert_array_equal(ctx.batch_fe()["Fe_max"], fe0["Fe_max"])  # clearing the others leaves it
    # a refused call leaves what was set; a new layout clears it
    with pytest.raises(capi.FptaError, match=r"\(-22\).*frequency 1: not positive and finite"):
        ctx.batch_set_fe([1], [1e-8], [0.0], [1400.0], np.zeros(1), [1e-8, -1.0], sky[:2], np.array([p.pos for p in psrs]))
    np.testing.assert_array_equal(ctx.batch_fe()["Fe_max"], fe0["Fe_max"])
    c = capi.Context(0)
    try:
        q = sky_case(3, 7, 2, 372)
        with pytest.raises(capi.FptaError, match="set_toas first"):
            c.batch_set_fe(None, None, None, None, None, None, None, None, clear=True)
        c.batch_set_toas(q["offs"], q["toas"], q["nu"])
        c.batch_add_signal(1, q["f"], np.sqrt(q["phi"]), L=np.eye(3))
        with pytest.raises(capi.FptaError, match=r"\(-77\).*nothing synthesized"):
            c.batch_fe()
        c.batch_synth(1, 0, 20, to_host=False)
        c.batch_set_fe(q["n_modes"], q["f"], q["idx"], q["freqf"], q["phi"], q["fgw"], q["sky"], q["pos"], weights=q["w"])
        assert c.batch_fe_info() == dict(K=4, G=2, n_sky=7, n_real=0) and c.batch_fe()["Fp"].shape == (2, 20)
        assert c.batch_fe_info()["n_real"] == 20
        c.batch_set_toas(q["offs"], q["toas"], q["nu"])  # a new layout: the statistic is gone
        c.batch_add_signal(1, q["f"], np.sqrt(q["phi"]), L=np.eye(3))
        c.batch_synth(1, 0, 20, to_host=False)
        with pytest.raises(capi.FptaError, match=r"\(-77\).*no F-statistic is set"):
            c.batch_fe()
    finally:
        c.close()
