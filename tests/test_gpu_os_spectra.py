"""The optimal statistic under a spectrum per realization on the GPU (k_spectra_amp's tables, k_fit_apply on its sixth
operator slot, k_oss_solve, k_oss_gram, k_oss_contract, then k_os_pairs and k_os_reduce, behind
fpta_batch_set_os_spectra and fpta_batch_os_spectra) and the Python surface above it, against the np.longdouble
definition of tests/os_spectra_reference.py: os_reference.operator_ld evaluated once per realization with that
realization's prior variances.

X and Z' per (pulsar, realization): |got - truth| <= os_reference.x_tolerance(truth, literal, bound) with bound =
(q + 2) eps cond_1(C) max |.|, C = I + s A s, and literal the fp64 solve on Phi^-1 + A. N_ab, norm and joint are held to
longdouble sums of the device's own Z', (K^2 + 3) eps sum |.| |.|. Each test prints the measured ratios (DESIGN.md
section 5p)."""
import numpy as np
import pytest

from tests import os_reference as OS
from tests import os_spectra_reference as SR
from tests import tm_reference as T
from tests import test_os_host as H

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
LD = np.longdouble
YEAR = 365.25 * 86400.0
SPAN = 15 * YEAR
# the batch layout takes no pulsar without TOAs (fpta_batch_set_toas refuses it): that case is the host planner's
# (tests/test_os_spectra_host.py)
N_PSR = (1, 5, 16, 17, 33, 250)
M_PSR = (0, 3, 0, 3, 16, 16)
ZERO_PSR = 2  # its layout amplitude of the varied red process is 0
# comps: (modes, chromatic index, per-pulsar grid, masked); vary: component indices, the target last. q = 2, 16, 18, 34,
# 128 and K = 2, 16, 2, 18, 60
CONFIGS = {
    "q2": dict(seed=21, comps=[(1, 0.0, False, False)], vary=[0], R=1),
    "q16": dict(seed=22, comps=[(4, 2.0, True, False), (8, 0.0, False, False)], vary=[1], R=16),
    "q18": dict(seed=23, comps=[(8, 0.0, True, False), (1, 0.0, False, False)], vary=[0, 1], R=17),
    "q34": dict(seed=24, comps=[(3, 0.0, True, True), (8, 0.0, True, False), (9, 0.0, False, False)], vary=[1, 2], R=33),
    "q128": dict(seed=25, comps=[(30, 0.0, True, False), (5, 2.0, True, False), (4, 0.0, True, False),
                                 (30, 0.0, False, False)], vary=[0, 2, 3], R=17),
    # the target alone at K = 128: 129 right-hand sides, three column slices of k_oss_solve (64 + 64 + 1), the last
    # of which holds z and writes X
    "q128t": dict(seed=26, comps=[(5, 2.0, True, False), (64, 0.0, False, False)], vary=[1], R=5),
}
# the distinct spectra of a block, as multiples of the white level per mode (red process, target); the last row also
# leaves one target mode out of the realization's model. Row r of a block is spectrum r mod 4.
ROWS = ((1e4, 3.0), (1e-4, 3.0), (10.0, 1e-6), (30.0, 1.0))


@pytest.fixture(scope="module")
def capi():
    from fakepta_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def ctx(capi):
    c = capi.Context(0)
    yield c
    c.close()


_CASES = {}


def case(name):
    """A configuration's inputs, made once and never changed."""
    if name in _CASES:
        return _CASES[name]
    from fakepta_amd import tm
    cfg = CONFIGS[name]
    rng = np.random.default_rng(cfg["seed"])
    P, R, vary = len(N_PSR), cfg["R"], cfg["vary"]
    offs = np.concatenate([[0], np.cumsum(N_PSR)]).astype(np.int64)
    n_toa = int(offs[-1])
    toas, nu, mats = [], [], []
    for n, m in zip(N_PSR, M_PSR):
        t = np.sort(rng.uniform(0.0, SPAN, n))
        v = T.three_band(rng, n)
        full = np.concatenate([T.mmat(t, v), (rng.uniform(size=(n, 8)) < 0.5).astype(np.float64)], axis=1)
        toas.append(t)
        nu.append(v)
        mats.append(full[:, :m].copy())
    toas, nu = np.concatenate(toas), np.concatenate(nu)
    sigma = rng.uniform(1e-7, 1e-6, n_toa)
    w = 1 / sigma ** 2
    level = np.array([2.0 / np.sum(w[offs[p]:offs[p + 1]]) if N_PSR[p] else 1e-14 for p in range(P)])
    common_level = level[-1]
    n_modes = np.array([c[0] for c in cfg["comps"]], dtype=np.int32)
    edges = np.concatenate([[0], np.cumsum(n_modes)])
    f_rows, phi, masks = [], [], []
    for p in range(P):
        sl = slice(int(offs[p]), int(offs[p + 1]))
        span_p = max(float(np.ptp(toas[sl])) if N_PSR[p] else 0.0, YEAR)
        f_rows.append(np.concatenate([np.arange(1, N + 1) / (span_p if own else SPAN) for N, _, own, _ in cfg["comps"]]))
        phi.append(np.concatenate([(10.0 * level[p] if own else 3.0 * common_level) * np.arange(1, N + 1) ** -3.0
                                   for N, _, own, _ in cfg["comps"]]))
    f_rows, phi = np.stack(f_rows), np.stack(phi)
    for _, _, _, masked in cfg["comps"]:
        masks.append((rng.uniform(size=n_toa) < 0.4).astype(np.uint8) if masked else None)
    tgt = vary[-1]
    N = int(n_modes[tgt])
    shape = np.arange(1, N + 1) ** -3.0
    phi_hat = 3.0 * common_level * shape
    # the layout: the varied signals only, in the order of vary; a per-pulsar one missing from pulsar ZERO_PSR
    lay, tables, phi_rows = [], [], []
    for c in vary:
        Nc, own = int(n_modes[c]), cfg["comps"][c][2]
        sh = np.arange(1, Nc + 1) ** -3.0
        f = f_rows[:, edges[c]:edges[c + 1]] if own else f_rows[0, edges[c]:edges[c + 1]]
        amp = np.sqrt(phi[:, edges[c]:edges[c + 1]] if own else phi[0, edges[c]:edges[c + 1]]).copy()
        mult = np.array([ROWS[r % 4][1 if c == tgt else 0] for r in range(R)])
        if own:
            amp[ZERO_PSR] = 0.0
            tab = np.sqrt(mult[:, None, None] * level[None, :, None] * sh[None, None, :])  # [R, P, N]
            tab[:, ZERO_PSR] = 0.0
        else:
            tab = np.sqrt(mult[:, None] * common_level * sh[None, :])  # [R, N]
            if c == tgt:
                tab[3::4, min(1, Nc - 1)] = 0.0
        lay.append(dict(kind=0 if own else 1, f=np.ascontiguousarray(f), amp=amp, idx=cfg["comps"][c][1],
                        mask=masks[c]))
        tables.append(np.ascontiguousarray(tab))
        phi_rows.append(tab ** 2)
    M, ncol = tm.stack_design(mats)
    G = rng.normal(size=(3, P, P))
    G = G + G.transpose(0, 2, 1)
    c = dict(name=name, offs=offs, toas=toas, nu=nu, mats=mats, M=M, ncol=ncol, w=w, sigma=sigma, n_modes=n_modes,
             f=f_rows, idx=np.array([c[1] for c in cfg["comps"]]), freqf=np.full(len(n_modes), 1400.0), phi=phi,
             masks=masks, vary=vary, target=tgt, phi_hat=phi_hat, lay=lay, tables=tables, phi_rows=phi_rows, G=G, R=R,
             K=2 * N, q=2 * int(sum(n_modes[v] for v in vary)), edges=edges)
    _CASES[name] = c
    return c


def comps_of(c, p):
    return [(c["f"][p, c["edges"][k]:c["edges"][k + 1]], c["idx"][k], c["freqf"][k]) for k in range(len(c["n_modes"]))]


def phis_of(c, p):
    return [c["phi"][p, c["edges"][k]:c["edges"][k + 1]] for k in range(len(c["n_modes"]))]


def masks_of(c, p):
    if all(m is None for m in c["masks"]):
        return None
    return [None if m is None else m[c["offs"][p]:c["offs"][p + 1]] for m in c["masks"]]


def row_phi(c, p, r):
    """The prior variances of the varied components for (pulsar, realization)."""
    return [t[r, p] if t.ndim == 3 else t[r] for t in c["phi_rows"]]


def set_layout(ctx, capi, c, n_orf=1, G=None):
    ctx.batch_set_toas(c["offs"], c["toas"], c["nu"])
    ids = [ctx.batch_add_signal(s["kind"], s["f"], s["amp"], idx=s["idx"], L=None if s["kind"] == 0 else
                                np.eye(len(N_PSR)), mask=s["mask"]) for s in c["lay"]]
    ctx.batch_set_white(c["sigma"], None, None)
    ctx.set_option(capi.OPT_SYNTH_PATH, 1)
    G = c["G"] if G is None else G
    rank = ctx.batch_set_os_spectra(c["n_modes"], c["f"], c["idx"], c["freqf"], c["phi"], c["target"], c["phi_hat"],
                                    c["vary"], ids, G, n_orf, masks=c["masks"], M=c["M"], ncol_psr=c["ncol"],
                                    weights=c["w"])
    return ids, rank


def run(ctx, c, ids, R, tables=None, n_orf=1, J=3, **kw):
    tables = c["tables"] if tables is None else tables
    per = [int(t.ndim == 3) for t in tables]
    return ctx.batch_os_spectra(ids, [0] * len(ids), per, [t[:R] for t in tables], c["K"], J, n_orf, **kw)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_x_and_z_match_the_truth_of_every_realization(ctx, capi, name):
    """Stage 2 on the ragged array (1, 5, 16, 17, 33, 250 TOAs; 0, 3 and 16 design columns): a red process 1e4 x
    and 1e-4 x the white level, a target 1e-6 x it, a target mode with phi_r = 0, a pulsar without the red process;
    tables [R, N] and [R, P, N]. The four distinct spectra are checked against the truth; the realizations that repeat
    one differ only in their residuals, which the same operator meets."""
    c = case(name)
    try:
        ids, rank = set_layout(ctx, capi, c)
        R, K, q, P = c["R"], c["K"], c["q"], len(N_PSR)
        ctx.batch_synth(31, 0, R, to_host=False)
        block = ctx.batch_download(0, R)
        sums = ctx.batch_checksums()
        out = run(ctx, c, ids, R, coefficients=True, zp=True, pair_norms=True, per_mode=True)
        np.testing.assert_array_equal(ctx.batch_checksums(), sums)  # read only
        np.testing.assert_array_equal(ctx.batch_download(0, R), block)
        X, Zp = out["X"], out["Zp"]
        assert X.shape == (P, K, R) and Zp.shape == (R, P, K, K)
        worst = dict(X=0.0, Z=0.0, N=0.0)
        h = np.sqrt(np.concatenate([c["phi_hat"], c["phi_hat"]]))
        Zt_all, Zl_all, cond_all = {}, {}, {}
        for p in range(P):
            sl = slice(int(c["offs"][p]), int(c["offs"][p + 1]))
            t, nu, w, Mp = c["toas"][sl], c["nu"][sl], c["w"][sl], c["mats"][p]
            B0, A, norms, keep = SR.plan_ld(t, nu, Mp, w, comps_of(c, p), phis_of(c, p), c["vary"], masks_of(c, p))
            T.assert_clear_rank(norms, keep, Mp)
            assert rank[p] == int(keep.sum())
            A64, B064 = A.astype(np.float64), B0.astype(np.float64)
            for r in range(min(R, 4)):
                pr = row_phi(c, p, r)
                Bt, Zt = SR.realization_truth(t, nu, Mp, w, comps_of(c, p), phis_of(c, p), c["vary"], pr,
                                              masks_of(c, p))
                phi_q = SR.columns_phi(pr)
                cond = SR.cond1(A64, phi_q)
                rows = [rr for rr in range(r, R, 4)]
                res = block[rows][:, sl]
                Xt = Bt @ res.T.astype(LD)  # [K, vectors]
                Xl, Zl = SR.literal(A64, B064 @ res.T, phi_q, K)
                bound = (q + 2) * EPS * cond * float(np.max(np.abs(Xt))) if Xt.size else 0.0
                tol, _ = OS.x_tolerance(Xt[None], Xl[None], np.full((1, K, len(rows)), bound))
                err = np.abs(X[p][:, rows].astype(LD) - Xt).astype(np.float64)
                worst["X"] = max(worst["X"], float(np.max(err / tol[0])))
                assert np.all(err <= tol[0]), (name, p, r, float(np.max(err / tol[0])), cond)
                Zpt = SR.scaled(Zt, c["phi_hat"])
                Zpl = h[:, None] * Zl * h[None, :]
                zb = (q + 2) * EPS * cond * float(np.max(np.abs(Zpt)))
                ztol, _ = OS.x_tolerance(Zpt[None], Zpl[None], np.full((1, K, K), zb))
                for rr in rows:  # the same spectrum: the same Z', bit for bit
                    np.testing.assert_array_equal(Zp[rr, p], Zp[r, p])
                zerr = np.abs(Zp[r, p].astype(LD) - Zpt).astype(np.float64)
                worst["Z"] = max(worst["Z"], float(np.max(zerr / ztol[0])))
                assert np.all(zerr <= ztol[0]), (name, p, r, float(np.max(zerr / ztol[0])), cond)
                Zt_all[p, r], Zl_all[p, r], cond_all[p, r] = Zpt, Zpl, cond
        # N_ab by the same rule, x_tolerance(truth, literal, (q + 2) eps cond_1(C) max |.|): the truth's and the literal
        # form's pair sums of a realization as [P, P], cond_1 the largest of the realization's pulsars, the literal
        # form's error taken per row a over its pairs
        nab = out["N_ab"]
        il = np.tril_indices(P, -1)
        for r in range(min(R, 4)):
            Nt, Nl = np.zeros((P, P), dtype=LD), np.zeros((P, P))
            for a, b in zip(*il):
                Nt[a, b] = np.sum(Zt_all[a, r] * Zt_all[b, r])
                Nl[a, b] = np.sum(Zl_all[a, r] * Zl_all[b, r])
            nb = (q + 2) * EPS * max(cond_all[p, r] for p in range(P)) * float(np.max(np.abs(Nt)))
            ntol, _ = OS.x_tolerance(Nt[None], Nl[None], np.full((1, P, P), nb))
            nerr = np.abs(nab[r].astype(LD) - Nt).astype(np.float64)
            worst["N"] = max(worst["N"], float(np.max(nerr[il] / ntol[0][il])))
            assert np.all(nerr[il] <= ntol[0][il]), (name, r, float(np.max(nerr[il] / ntol[0][il])))
        print(f"{name}: largest error / tolerance: X {worst['X']:.3g}, Z' {worst['Z']:.3g}, N_ab {worst['N']:.3g}; "
              f"largest cond_1(C) {max(cond_all.values()):.3g}")
    finally:
        ctx.set_option(capi.OPT_SYNTH_PATH, 0)


def small_case(P, seed):
    """P pulsars of 9 .. 20 TOAs, a red process of 2 modes and a target of 2 (q = 8, K = 4), no design."""
    rng = np.random.default_rng(seed)
    n_p = [int(rng.integers(9, 21)) for p in range(P)]
    offs = np.concatenate([[0], np.cumsum(n_p)]).astype(np.int64)
    toas = np.concatenate([np.sort(rng.uniform(0.0, SPAN, n)) for n in n_p])
    nu = np.full(len(toas), 1400.0)
    sigma = rng.uniform(1e-7, 1e-6, len(toas))
    f = np.arange(1, 3) / SPAN
    lvl = 2.0 / (15 / 5e-7 ** 2)
    a_rn = np.sqrt(10.0 * lvl * np.arange(1, 3) ** -3.0)
    a_gw = np.sqrt(3.0 * lvl * np.arange(1, 3) ** -3.0)
    return dict(offs=offs, toas=toas, nu=nu, sigma=sigma, f=f, a_rn=a_rn, a_gw=a_gw, P=P)


def pair_weights(rng, P, J):
    G = rng.normal(size=(J, P, P))
    G = G + G.transpose(0, 2, 1)
    if P > 1:
        G[0] = 0.0
        G[0, P - 1, 0] = G[0, 0, P - 1] = 1.5  # one nonzero pair
    if J > 1:
        G[1] = 0.0
        G[1, :min(P, 16), :min(P, 16)] = 1.0  # all ones on the first diagonal tile
    return G


@pytest.mark.parametrize("P,J", [(1, 1), (2, 3), (3, 17), (16, 3), (17, 1), (33, 17)])
def test_gram_and_contractions_are_the_sums_of_the_device_z(ctx, capi, P, J):
    """Stages 3 and 4 against longdouble sums of the device's own Z': N_ab to (K^2 + 3) eps sum |.| |.|, norm and joint
    to the same bound over their own terms (on top of N_ab's); one pulsar: no pair, norm exactly 0 and the statistics
    NaN."""
    from fakepta_amd import os as osm
    s = small_case(P, 40 + P)
    rng = np.random.default_rng(P)
    R, K, n_orf = 3, 4, min(J, 2)
    G = pair_weights(rng, P, J)
    ctx.batch_set_toas(s["offs"], s["toas"], s["nu"])
    i_rn = ctx.batch_add_signal(0, np.tile(s["f"], (P, 1)), np.tile(s["a_rn"], (P, 1)))
    i_gw = ctx.batch_add_signal(1, s["f"], s["a_gw"], L=np.eye(P))
    ctx.batch_set_white(s["sigma"], None, None)
    phi = np.tile(np.concatenate([s["a_rn"] ** 2, s["a_gw"] ** 2]), (P, 1))
    ctx.batch_set_os_spectra([2, 2], np.tile(np.concatenate([s["f"], s["f"]]), (P, 1)), [0.0, 0.0], [1400.0, 1400.0], phi,
                             1, s["a_gw"] ** 2, [0, 1], [i_rn, i_gw], G, n_orf, weights=1 / s["sigma"] ** 2)
    ctx.batch_synth(3, 0, R, to_host=False)
    tab = np.sqrt(np.array([1.0, 30.0, 0.01])[:, None]) * s["a_rn"][None, :]
    out = ctx.batch_os_spectra([i_rn], [0], [0], [tab], K, J, n_orf, pair_norms=True, zp=True)
    worst = 0.0
    for r in range(R):
        nt, mag = SR.gram_ld(out["Zp"][r])
        tol = (K * K + 3) * EPS * mag.astype(np.float64)
        il = np.tril_indices(P)
        err = np.abs(out["N_ab"][r].astype(LD) - nt).astype(np.float64)
        assert np.all(err[il] <= tol[il])
        assert np.all(out["N_ab"][r][np.triu_indices(P, 1)] == 0)
        worst = max(worst, float(np.max(err[il] / np.maximum(tol[il], 1e-300))))
        norm_t, norm_m, joint_t, joint_m = SR.contractions_ld(G, out["N_ab"][r], n_orf)
        n_pairs = P * (P - 1) // 2
        assert np.all(np.abs(out["norm"][:, r] - norm_t) <= (n_pairs + 3) * EPS * norm_m)
        assert np.all(np.abs(out["joint"][:, :, r] - joint_t) <= (n_pairs + 3) * EPS * joint_m)
    if P == 1:
        assert np.all(out["norm"] == 0) and np.all(out["Q"] == 0)
        d = osm.derive_per_realization(out["Q"], out["norm"], out["joint"], n_orf)
        assert np.all(np.isnan(d["A2"])) and np.all(np.isnan(d["snr"])) and np.all(np.isnan(d["A2_joint"]))
    else:
        assert np.all(out["norm"][0] > 0)
        np.testing.assert_array_equal(out["norm"][0], 1.5 ** 2 * out["N_ab"][:, P - 1, 0])
    print(f"P = {P}, J = {J}: N_ab largest error / bound {worst:.3g}")


def test_a_realization_does_not_depend_on_the_block_around_it(ctx, capi):
    """X, Q and norm of a realization are bit-identical whatever R, its position and its neighbours: blocks of 33, 16
    and 1 rows made from the same host normals (fpta_batch_synth_from_z), and the 33 in reversed order."""
    c = case("q34")
    try:
        ids, _ = set_layout(ctx, capi, c, n_orf=2)
        rng = np.random.default_rng(9)
        P, nm = len(N_PSR), max(int(c["n_modes"][v]) for v in c["vary"])
        z = rng.normal(size=(33, len(ids), P, nm + nm % 2, 2))
        tabs = [np.concatenate([t, t])[:33] if len(t) < 33 else t[:33] for t in c["tables"]]
        assert all(len(t) == 33 for t in tabs)

        def block(rows):
            got = ctx.batch_synth_from_z(np.ascontiguousarray(z[rows]))
            out = run(ctx, c, ids, len(rows), tables=[np.ascontiguousarray(t[rows]) for t in tabs], n_orf=2,
                      coefficients=True)
            return got, out

        full_rows = np.arange(33)
        res, full = block(full_rows)
        assert np.any(full["X"] != 0) and np.all(np.isfinite(full["Q"]))
        for rows in (np.arange(16), np.array([7]), full_rows[::-1].copy()):
            got, out = block(rows)
            np.testing.assert_array_equal(got, res[rows])  # the premise: the rows of the block are the same bits
            np.testing.assert_array_equal(out["X"], full["X"][:, :, rows])
            np.testing.assert_array_equal(out["Q"], full["Q"][:, rows])
            np.testing.assert_array_equal(out["norm"], full["norm"][:, rows])
            np.testing.assert_array_equal(out["joint"], full["joint"][:, :, rows])
    finally:
        ctx.set_option(capi.OPT_SYNTH_PATH, 0)


class _Psr:
    """The attributes BatchSimulator, design_of and weights_of read."""

    def __init__(self, toas, freqs, sigma2, pos, M):
        self.toas, self.freqs, self.sigma2, self.pos, self.Mmat = toas, freqs, sigma2, pos, M
        self.signal_model = {}

    def _white_sigma2(self):
        return self.sigma2


@pytest.fixture(scope="module")
def small(ctx):
    """The unbiasedness layout of tests/test_os_host.py as a BatchSimulator."""
    from fakepta_amd.batch import BatchSimulator
    lay = H.unbiased_layout()
    o = lay["offs"]
    psrs = [_Psr(lay["toas"][o[i]:o[i + 1]], lay["nu"][o[i]:o[i + 1]], lay["sigma"][o[i]:o[i + 1]] ** 2, lay["pos"][i],
                 lay["Mmats"][i]) for i in range(len(o) - 1)]
    sim = BatchSimulator(psrs, signals=[], white=True, ctx=ctx)
    sim.add_signal("red_noise", 0, lay["f_rn"], lay["amp_rn"])
    sim.add_signal("gw_common", 1, lay["f_gw"], lay["amp_gw"], L=lay["L"])
    return sim, psrs, lay


def own_bounds(lay, block, G, n_orf, X_dev, nab_dev):
    """What this route may differ from the shared truth by, for A2, snr, A2_joint and the binned rho of a block under
    the layout's spectrum: X and N_ab within this module's rule (x_tolerance(truth, literal, (q + 2) eps cond_1(C)
    max |.|), asserted here on the device's X and N_ab), carried through Q, the denominators and the joint solve by
    the algebra of test_gpu_os.composed."""
    per, nab_t = H.unbiased_truth()
    offs = lay["offs"]
    P, K = len(per), per[0][0].shape[0]
    q = K + 2 * lay["f_rn"].shape[1]
    phi_hat = lay["amp_gw"] ** 2
    Xt, _ = OS.x_truth([b[0] for b in per], offs, block)
    dX, Zl, conds = np.zeros(Xt.shape), [], []
    for p in range(P):
        sl = slice(int(offs[p]), int(offs[p + 1]))
        B0, A, _, _ = SR.plan_ld(lay["toas"][sl], lay["nu"][sl], lay["Mmats"][p], 1 / lay["sigma"][sl] ** 2,
                                 lay["comps_of"](p), lay["phis_of"](p), [0, 1])
        phi_q = SR.columns_phi(lay["phis_of"](p))
        cond = SR.cond1(A.astype(np.float64), phi_q)
        Xl, Z = SR.literal(A.astype(np.float64), B0.astype(np.float64) @ block[:, sl].T, phi_q, K)
        bound = (q + 2) * EPS * cond * float(np.max(np.abs(Xt[p])))
        dX[p] = OS.x_tolerance(Xt[p][None], Xl[None], np.full((1,) + Xl.shape, bound))[0][0]
        Zl.append(Z.astype(LD))
        conds.append(cond)
    assert np.all(np.abs(X_dev.astype(LD) - Xt) <= dX)
    nl = OS.pair_norms(Zl, phi_hat)[0]
    nb = (q + 2) * EPS * max(conds) * float(np.max(np.abs(nab_t)))
    dnab = OS.x_tolerance(nab_t[None], nl.astype(np.float64)[None], np.full((1, P, P), nb))[0][0]
    dnab = np.maximum(dnab, dnab.T)
    il = np.tril_indices(P, -1)
    assert np.all(np.abs(nab_dev.astype(LD) - nab_t)[il] <= dnab[il])
    X64 = Xt.astype(np.float64)
    Qm_t, _, bq = OS.q_truth(X64, phi_hat, G)
    Qt = Qm_t.sum(axis=1).astype(np.float64)
    ph2 = np.concatenate([phi_hat, phi_hat])[None, :, None]
    aX = np.abs(X64) + dX
    cross = ((dX[il[0]] * aX[il[1]] + aX[il[0]] * dX[il[1]]) * ph2).sum(axis=1)  # [pairs, R]
    dQ = np.abs(G[:, il[0], il[1]]) @ cross + 2 * bq
    norm_t = np.array([np.sum(g[il].astype(LD) ** 2 * nab_t[il]) for g in G]).astype(np.float64)
    dnorm = np.array([np.sum(g[il] ** 2 * dnab[il]) for g in G]) + 8 * EPS * np.abs(norm_t)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = Qt / norm_t[:, None]
        d_ratio = (dQ + np.abs(ratio) * dnorm[:, None]) / norm_t[:, None] + 8 * EPS * np.abs(ratio)
        snr = Qt[:n_orf] / np.sqrt(norm_t[:n_orf, None])
        d_snr = (dQ[:n_orf] + np.abs(snr) * dnorm[:n_orf, None] / np.sqrt(norm_t[:n_orf, None])) / \
            np.sqrt(norm_t[:n_orf, None]) + 8 * EPS * np.abs(snr)
    rows = np.array([g[il] for g in G[:n_orf]])
    C = (rows * nab_t[il].astype(np.float64)) @ rows.T
    dC = (np.abs(rows) * dnab[il]) @ np.abs(rows).T + 8 * EPS * np.abs(C)
    Ci = np.linalg.inv(C)
    joint = Ci @ Qt[:n_orf]
    d_joint = np.abs(Ci) @ (dQ[:n_orf] + dC @ np.abs(joint)) + 64 * EPS * np.linalg.cond(C) * np.abs(joint).max(axis=0)
    return dict(A2=d_ratio[:n_orf], snr=d_snr, rho_bins=d_ratio[n_orf:], A2_joint=d_joint)


def test_every_row_equal_to_the_layout_agrees_with_the_fixed_statistic(ctx, small):
    """With the layout's spectrum in every row, A2, snr, A2_joint and rho_bins agree with optimal_statistic() on the same
    block. Not bit for bit: the fixed route applies B = F^T P^-1 planned in long double, this one solves C in fp64 on
    z = B0 r. Each is within its own tolerance of the shared truth (test_gpu_os.composed's bound for the fixed route,
    own_bounds for this one, from its own X and N_ab tolerances), so they differ by at most the sum.
    norm[:, r] is the same for every r, bit for bit."""
    from tests.test_gpu_os import composed
    sim, psrs, lay = small
    orfs, R = ("hd", "monopole", "dipole"), 40
    rank, nab = sim.set_optimal_statistic(orfs=orfs, bins=5)
    rank2 = sim.set_optimal_statistic_spectra(["red_noise"], orfs=orfs, bins=5)
    np.testing.assert_array_equal(rank, rank2)
    sim.synth(R, seed=5, to_host=False)
    before = sim.checksums()
    fixed = sim.optimal_statistic()
    out = sim.optimal_statistic_spectra(pair_norms=True)
    np.testing.assert_array_equal(sim.checksums(), before)
    again = sim.optimal_statistic_spectra({"gw_common": dict(amp=np.tile(lay["amp_gw"], (R, 1))),
                                           "red_noise": dict(amp=np.tile(lay["amp_rn"], (R, 1, 1)))})
    for key in ("Q", "norm", "joint", "A2"):
        np.testing.assert_array_equal(again[key], out[key])  # a row equal to the layout is the layout
    assert np.all(out["norm"] == out["norm"][:, :1]) and np.all(out["N_ab"] == out["N_ab"][:1])
    block, G = ctx.batch_download(0, R), sim._os["G"]
    want = composed(lay, block, G, nab, 3)
    X_dev = ctx.batch_os_spectra([], [], [], [], 10, len(G), 3, coefficients=True)["X"]
    own = own_bounds(lay, block, G, 3, X_dev, out["N_ab"][0])
    live = out["bin_counts"] > 0
    worst = {}
    for key in ("A2", "snr", "A2_joint", "rho_bins"):
        d = want[key][1] + own[key]
        a, b = out[key], fixed[key]
        if key == "rho_bins":
            a, b, d = a[live], b[live], d[live]
            assert np.all(np.isnan(out[key][~live]))
        worst[key] = float(np.max(np.abs(a - b) / d))
        assert np.all(np.abs(a - b) <= d), (key, worst[key])
    print("per-realization route against the fixed one, largest difference / summed tolerance:",
          {k: f"{v:.2e}" for k, v in worst.items()})


def test_the_other_consumers_and_the_next_block_do_not_see_the_feature(ctx, capi, small):
    """A Fourier fit and the fixed statistic give the same bits with and without this feature set and run; the block
    after a call is the block after an untouched one."""
    sim, psrs, lay = small
    R = 24
    sim.ctx.batch_set_os_spectra(None, None, None, None, None, 0, None, None, None, None, 0)  # cleared
    sim.set_optimal_statistic()
    sim.set_fourier_fit([(4, 0.0)])
    sim.synth(R, seed=11, to_host=False)
    Q0, _, X0 = ctx.batch_os(coefficients=True)
    coef0 = sim.fourier_fit()
    nxt0 = sim.synth(R, seed=11, real0=R)
    sim.set_optimal_statistic_spectra(["red_noise"])
    sim.synth(R, seed=11, to_host=False)
    out = sim.optimal_statistic_spectra()
    assert np.all(np.isfinite(out["A2"]))
    Q1, _, X1 = ctx.batch_os(coefficients=True)
    np.testing.assert_array_equal(Q1, Q0)
    np.testing.assert_array_equal(X1, X0)
    np.testing.assert_array_equal(sim.fourier_fit(), coef0)
    np.testing.assert_array_equal(sim.synth(R, seed=11, real0=R), nxt0)
    sim.set_optimal_statistic_spectra([])  # the target alone
    with pytest.raises(ValueError, match="not in the varied set"):
        sim.optimal_statistic_spectra({"red_noise": dict(amp=np.tile(lay["amp_rn"], (R, 1, 1)))})
    with pytest.raises(capi.FptaError, match="signal 0: a table for a signal outside the varied set"):
        ctx.batch_os_spectra([0], [0], [1], [np.tile(lay["amp_rn"], (R, 1, 1))], 10, 1, 1)
    assert np.all(np.isfinite(sim.optimal_statistic_spectra()["A2"]))  # a refused call leaves the state as it was
    sim.ctx.batch_set_fit(None, None, None, None)


E2E_SEED, E2E_R = 3, 256


def e2e_spectra(lay, R):
    """log10_A of the red noise (per pulsar) and of the common process drawn per realization over one decade."""
    rng = np.random.default_rng(E2E_SEED)
    P = len(lay["offs"]) - 1
    return dict(red_noise=dict(log10_A=rng.uniform(-13.8, -12.8, (R, P)), gamma=3.0),
                gw_common=dict(log10_A=rng.uniform(-14.1, -13.1, R), gamma=13 / 3))


def test_each_realization_under_its_own_truth_is_unbiased(ctx, small):
    """synth(spectra=...) with log10_A of both processes drawn per realization over one decade, then the statistic
    with the same tables: the mean over realizations of A2_r phi_hat / phi_r is within 4 of its standard errors of 1
    (tests/test_os_spectra_host.py shows the seed passes with the reference alone), and the fixed statistic on the same
    block gives other numbers."""
    sim, psrs, lay = small
    spec = e2e_spectra(lay, E2E_R)
    sim.set_optimal_statistic()
    sim.set_optimal_statistic_spectra(["red_noise"])
    sim.synth(E2E_R, seed=E2E_SEED, to_host=False, spectra=spec)
    out = sim.optimal_statistic_spectra(spec)
    fixed = sim.optimal_statistic()
    ratio = 10.0 ** (2 * (-13.6 - spec["gw_common"]["log10_A"]))  # phi_hat / phi_r: the template is the layout's -13.6
    y = out["A2"][0] * ratio
    se = np.std(y) / np.sqrt(E2E_R)
    print(f"mean A2_r phi_hat / phi_r = {np.mean(y):.4f}, standard error {se:.4f}: {(np.mean(y) - 1) / se:.2f} of them "
          f"from 1; the fixed statistic's mean of the same {np.mean(fixed['A2'][0] * ratio):.4f}")
    assert abs(np.mean(y) - 1.0) <= 4 * se
    assert not np.allclose(fixed["A2"][0], out["A2"][0], rtol=1e-3)


@pytest.fixture(scope="module")
def shared_span(capi):
    """tests/test_gpu_os.py's layout of the same name (C2's signal mix on 64 ragged pulsars over one common span, whose
    pipelined k_grid_fused blocks also make the next block's common-signal mix), with this statistic set: red noise
    and the common process varied (q = 120), the 100-mode DM process fixed."""
    from fakepta_amd.batch import batch_factor
    from oracle import fakepta_oracle as O
    c = capi.Context(0)
    rng = np.random.default_rng(17)
    P = 64
    counts = rng.integers(40, 120, size=P)
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    t0, t1 = 0.0, 3.15e8
    toas = np.concatenate([np.concatenate([[t0], np.sort(rng.uniform(t0, t1, k - 2)), [t1]]) for k in counts])
    nu = rng.choice([800.0, 1400.0, 2500.0], size=offs[-1])
    c.batch_set_toas(offs, toas, nu)
    fs, phis, ids = [], [], []
    for nm, idx in ((30, 0.0), (100, 2.0)):
        f = np.tile(np.arange(1, nm + 1) / (t1 - t0), (P, 1))
        amp = np.sqrt(O.powerlaw(f, rng.uniform(-14.5, -13.5, (P, 1)), 3.0) / (t1 - t0))
        ids.append(c.batch_add_signal(0, f, amp, idx=idx))
        fs.append(f)
        phis.append(amp ** 2)
    fc = np.arange(1, 31) / (t1 - t0)
    ac = np.sqrt(O.powerlaw(fc, -14.0, 13 / 3) / (t1 - t0))
    v = rng.normal(size=(P, 3))
    hd = O.orf_hd(v / np.linalg.norm(v, axis=1)[:, None])
    ids.append(c.batch_add_signal(1, fc, ac, L=batch_factor(hd)))
    c.set_option(capi.OPT_SYNTH_PATH, 4)
    np.fill_diagonal(hd, 0.0)
    rank = c.batch_set_os_spectra([30, 100, 30], np.concatenate(fs + [np.tile(fc, (P, 1))], axis=1), [0.0, 2.0, 0.0],
                                  [1400.0] * 3, np.concatenate(phis + [np.tile(ac ** 2, (P, 1))], axis=1), 2, ac ** 2,
                                  [0, 2], [ids[0], ids[2]], hd[None], 1, weights=np.full(int(offs[-1]), 1e13))
    assert list(rank) == [0] * P
    tabs = [np.stack([rng.uniform(-14.5, -13.5, (128, P)), np.full((128, P), 3.0)], axis=-1),
            np.stack([rng.uniform(-14.5, -13.5, 128), np.full(128, 13 / 3)], axis=-1)]
    yield c, [ids[0], ids[2]], tabs
    c.close()


@pytest.mark.parametrize("next_real0,hit", [(384, True), (1000, False)])
def test_statistic_leaves_the_block_and_the_next_block_alone(shared_span, next_real0, hit):
    """The block is bit for bit what it was, and the block after one whose statistic was taken (tables uploaded,
    k_spectra_amp, k_fit_apply and the new kernels on the context stream) is bit for bit the block after an untouched
    one, for a next-mix hit and for a miss."""
    c, ids, tabs = shared_span
    outs = []
    for stat in (False, True):
        for real0 in (0, 128, 256):  # hits start at the third block of a pipelined run
            c.batch_synth(7, real0, 128, to_host=False)
        assert c.batch_grid_info()["interp_kernel"].startswith("k_grid_fused<")
        if stat:
            sums, pre = c.batch_checksums(), c.batch_download(0, 128)
            out = c.batch_os_spectra(ids, [1, 1], [1, 0], tabs, 60, 1, 1)
            assert out["Q"].shape == (1, 128) and np.all(np.isfinite(out["Q"])) and np.any(out["Q"] != 0)
            assert np.all(out["norm"] > 0)
            np.testing.assert_array_equal(c.batch_download(0, 128), pre)
            np.testing.assert_array_equal(c.batch_checksums(), sums)
        outs.append(c.batch_synth(7, next_real0, 128))
        assert c.batch_grid_info()["next_mix_used"] == hit
    np.testing.assert_array_equal(outs[1], outs[0])


def test_state_errors_and_set_toas_clears_the_statistic(capi):
    """FPTA_ESTATE without a layout, without a block and without a statistic; fpta_batch_set_toas clears the statistic;
    a refused set call leaves the one that was set."""
    s = small_case(3, 5)
    P = 3
    c = capi.Context(0)
    try:
        with pytest.raises(capi.FptaError, match="set_os_spectra: set_toas first"):
            c.batch_set_os_spectra(None, None, None, None, None, 0, None, None, None, None, 0)

        def layout():
            c.batch_set_toas(s["offs"], s["toas"], s["nu"])
            return c.batch_add_signal(1, s["f"], s["a_gw"], L=np.eye(P))

        def set_it(weights):
            return c.batch_set_os_spectra([2], s["f"], [0.0], [1400.0], np.tile(s["a_gw"] ** 2, (P, 1)), 0,
                                          s["a_gw"] ** 2, [0], [gw], np.ones((1, P, P)), 1, weights=weights)

        gw = layout()
        w = 1 / s["sigma"] ** 2
        with pytest.raises(capi.FptaError, match="os_spectra: nothing synthesized yet"):
            c.batch_os_spectra([], [], [], [], 4, 1, 1)
        c.batch_synth(1, 0, 5, to_host=False)
        with pytest.raises(capi.FptaError, match="os_spectra: no statistic is set"):
            c.batch_os_spectra([], [], [], [], 4, 1, 1)
        set_it(w)
        first = c.batch_os_spectra([], [], [], [], 4, 1, 1)
        bad = w.copy()
        bad[2] = 0.0
        with pytest.raises(capi.FptaError, match="weight"):
            set_it(bad)
        with pytest.raises(capi.FptaError, match="unknown layout signal 7"):
            c.batch_set_os_spectra([2], s["f"], [0.0], [1400.0], np.tile(s["a_gw"] ** 2, (P, 1)), 0, s["a_gw"] ** 2, [0],
                                   [7], np.ones((1, P, P)), 1, weights=w)
        again = c.batch_os_spectra([], [], [], [], 4, 1, 1)  # the refused calls left the statistic that was set
        for key in ("Q", "norm", "joint"):
            np.testing.assert_array_equal(again[key], first[key])
        gw = layout()  # a new layout: the statistic is gone
        c.batch_synth(1, 0, 5, to_host=False)
        with pytest.raises(capi.FptaError, match="os_spectra: no statistic is set"):
            c.batch_os_spectra([], [], [], [], 4, 1, 1)
    finally:
        c.close()
