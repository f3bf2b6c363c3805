"""The optimal statistic on the GPU (k_fit_apply on its second operator slot, k_os_pairs and k_os_reduce behind
fpta_os_statistic, fpta_batch_set_os and fpta_batch_os) and the Python surface above it, against the np.longdouble
definition of tests/os_reference.py.

X = B_p r, per pulsar and row: |got - truth| <= max(4 e_lit, (n_p + 2) eps sum_t |B_kt| |r_t|), DESIGN.md section 5i's
rule: e_lit is the error of the literal fp64 Woodbury form, the second term the rigorous bound of a length-n_p fp64 dot
product in any order with a once-rounded operator, from the truth's B. Q is held to the definition applied to the
device's own X, downloaded: the dot-product bound (n_terms + 3) eps sum |G| |phi_hat| |X_a| |X_b|, n_terms = K P (P - 1)
/ 2. End to end the two compose. Every truth asserts the conditioning of its own inputs (kept design columns >= 1e-4,
dropped ones <= 1e-13). Each test prints the measured ratios."""
import numpy as np
import pytest

from tests import os_reference as OS
from tests import tm_reference as T
from tests import test_os_host as H
from tests.helpers import random_layout

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
LD = np.longdouble
YEAR = 365.25 * 86400.0
SPAN = 15 * YEAR
# one ragged array: 0 TOAs, fewer TOAs than columns, one chunk of 64 TOAs and its partial forms, several chunks with a
# tail; design columns per pulsar 0, 3 and 16 (make_Mmat's eight and eight offsets between random halves)
N_PSR = (0, 1, 5, 16, 17, 33, 250, 600)
M_PSR = (3, 0, 3, 0, 3, 16, 16, 3)
N_VEC = 33
# K = 2, 16, 18, 60, 208: k_fit_apply's instances (8, 8, 4, 2 slices per row group, and a wave that owns two groups).
# comps: (modes, chromatic index, white-noise multiples of the first mode's prior variance, per-pulsar grid)
CONFIGS = {
    "k2": dict(seed=11, comps=[(3, 0.0, 30.0, True), (1, 0.0, 3.0, False)], target=1, weighted=True),
    "k16": dict(seed=12, comps=[(8, 0.0, 10.0, False)], target=0, weighted=False),
    "k18": dict(seed=13, comps=[(5, 0.0, 1e3, True), (4, 2.0, 5.0, False), (9, 0.0, 3.0, False)], target=2,
                weighted=True),
    "k60": dict(seed=14, comps=[(30, 0.0, 100.0, False), (30, 0.0, 10.0, False)], target=1, weighted=True),
    "k208": dict(seed=15, comps=[(104, 0.0, 10.0, False), (4, 0.0, 100.0, True)], target=0, weighted=False),
}


@pytest.fixture(scope="module")
def capi():
    from fakepta_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def ctx(capi):
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def restore_options(ctx):
    shipped = ctx.options()
    yield
    ctx.set_options(shipped)


_CASES = {}


def case(name):
    """A configuration's inputs, truth and literal form, made once and never changed."""
    if name not in _CASES:
        from fakepta_amd import tm
        cfg = CONFIGS[name]
        rng = np.random.default_rng(cfg["seed"])
        P = len(N_PSR)
        offs = np.concatenate([[0], np.cumsum(N_PSR)]).astype(np.int64)
        toas, nu, mats = [], [], []
        for n, m in zip(N_PSR, M_PSR):
            t = np.sort(rng.uniform(0.0, SPAN, n))
            v = T.three_band(rng, n)
            full = np.concatenate([T.mmat(t, v), (rng.uniform(size=(n, 8)) < 0.5).astype(np.float64)], axis=1)
            toas.append(t)
            nu.append(v)
            mats.append(full[:, :m].copy())
        toas, nu = np.concatenate(toas), np.concatenate(nu)
        w = 1 / rng.uniform(1e-7, 1e-6, int(offs[-1])) ** 2 if cfg["weighted"] else np.full(int(offs[-1]), 1e12)
        n_modes = np.array([c[0] for c in cfg["comps"]], dtype=np.int32)
        idx = np.array([c[1] for c in cfg["comps"]])
        freqf = np.full(len(idx), 1400.0)
        f_rows, phi = [], []
        for p in range(P):
            sl = slice(int(offs[p]), int(offs[p + 1]))
            span_p = max(float(np.ptp(toas[sl])) if N_PSR[p] else 0.0, YEAR)
            level = 2.0 / np.sum(w[sl]) if N_PSR[p] else 1e-14
            f_rows.append(np.concatenate([np.arange(1, N + 1) / (span_p if own else SPAN)
                                          for N, _, _, own in cfg["comps"]]))
            phi.append(np.concatenate([(lv * level if own else lv * 2e-14 / 300) * np.arange(1, N + 1) ** -3.0
                                       for N, _, lv, own in cfg["comps"]]))
        f_rows, phi = np.stack(f_rows), np.stack(phi)
        edges = np.concatenate([[0], np.cumsum(n_modes)])
        tgt = cfg["target"]
        phi_hat = phi[0, edges[tgt]:edges[tgt + 1]].copy()

        def comps_of(p):
            return [(f_rows[p, edges[c]:edges[c + 1]], idx[c], freqf[c]) for c in range(len(n_modes))]

        def phis_of(p):
            return [phi[p, edges[c]:edges[c + 1]] for c in range(len(n_modes))]

        M, ncol = tm.stack_design(mats)
        res = rng.normal(0.0, 1e-6, (N_VEC, int(offs[-1])))
        Bs, lits = [], []
        for p in range(P):
            sl = slice(int(offs[p]), int(offs[p + 1]))
            B, _, norms, keep = OS.operator_ld(toas[sl], nu[sl], mats[p], w[sl], comps_of(p), phis_of(p), tgt,
                                               need_z=False)
            T.assert_clear_rank(norms, keep, mats[p])
            Bs.append(B)
            lits.append(OS.operator_literal(toas[sl], nu[sl], mats[p], w[sl], comps_of(p), phis_of(p), tgt, keep)
                        if N_PSR[p] else np.zeros(B.shape))
        truth, bound = OS.x_truth(Bs, offs, res)
        literal = np.stack([lits[p] @ res[:, int(offs[p]):int(offs[p + 1])].T for p in range(P)])
        K = 2 * int(n_modes[tgt])
        G = rng.normal(size=(3, P, P))
        G = G + G.transpose(0, 2, 1)
        c = dict(offs=offs, toas=toas, nu=nu, mats=mats, M=M, ncol=ncol, w=w, res=res, n_modes=n_modes, f=f_rows,
                 idx=idx, freqf=freqf, phi=phi, target=tgt, phi_hat=phi_hat, truth=truth, bound=bound,
                 literal=literal, K=K, G=G)
        for a in (M, ncol, res, toas, nu, f_rows, phi, G, w):
            a.flags.writeable = False
        _CASES[name] = c
    return _CASES[name]


def one_shot(ctx, c, res, G=None):
    return ctx.os_statistic(c["offs"], c["toas"], c["nu"], c["n_modes"], c["f"], c["idx"], c["freqf"], c["phi"],
                            c["target"], c["phi_hat"], c["G"] if G is None else G, res, M=c["M"], ncol_psr=c["ncol"],
                            weights=c["w"])


def check_x(label, got, truth, literal, bound, n_psr):
    """The module's tolerance per pulsar and row; prints the measured ratios."""
    tol, e_lit = OS.x_tolerance(truth, literal, bound)
    err = np.abs(got.astype(LD) - truth).astype(np.float64)
    for p in range(got.shape[0]):
        if n_psr[p] == 0:
            assert np.all(got[p] == 0.0), (label, p)  # a pulsar without TOAs has X = 0 exactly
            continue
        ratio = err[p] / np.maximum(tol[p], 1e-300)
        rb = err[p] / np.maximum(bound[p], 1e-300)
        print(f"{label} pulsar {p} (n {n_psr[p]}): error / tolerance {ratio.max():.3f}, error / dot-product bound "
              f"{rb.max():.3f}, literal error / bound "
              f"{float(np.max(e_lit[p] / np.maximum(bound[p].max(axis=1, keepdims=True), 1e-300))):.3g}")
        assert np.all(err[p] <= tol[p]), (label, p, float(ratio.max()))


def check_q(label, X, phi_hat, G, Q, Qm):
    """Q and Q_mode are the definition applied to X within the dot-product bound; Q is the sum of Q_mode in mode order,
    bit for bit. Returns the largest error / bound."""
    Qm_t, bm, bq = OS.q_truth(X, phi_hat, G)
    assert Qm.shape == Qm_t.shape and Q.shape == bq.shape
    em = np.abs(Qm.astype(LD) - Qm_t).astype(np.float64)
    eq = np.abs(Q.astype(LD) - Qm_t.sum(axis=1)).astype(np.float64)
    assert np.all(em <= bm), (label, float(np.max(em / np.maximum(bm, 1e-300))))
    assert np.all(eq <= bq), (label, float(np.max(eq / np.maximum(bq, 1e-300))))
    acc = np.zeros(Q.shape)
    for m in range(Qm.shape[1]):
        acc = acc + Qm[:, m]
    np.testing.assert_array_equal(acc, Q)
    worst = max(float(np.max(em / np.maximum(bm, 1e-300), initial=0)), float(np.max(eq / np.maximum(bq, 1e-300), initial=0)))
    print(f"{label}: largest Q error / bound {worst:.4f}")
    return worst


@pytest.mark.parametrize("n_vec", [1, 16, 33])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_one_shot_x_matches_the_truth(ctx, name, n_vec):
    c = case(name)
    Q, Qm, X, rank, nab = one_shot(ctx, c, c["res"][:n_vec])
    assert X.shape == (len(N_PSR), c["K"], n_vec) and Q.shape == (3, n_vec)
    check_x(f"{name} n_vec {n_vec}", X, c["truth"][:, :, :n_vec], c["literal"][:, :, :n_vec], c["bound"][:, :, :n_vec],
            N_PSR)
    check_q(f"{name} n_vec {n_vec}", X, c["phi_hat"], c["G"], Q, Qm)
    assert np.all(nab[0] == 0) and np.all(nab == nab.T) and np.all(nab[1:, 1:][~np.eye(len(N_PSR) - 1, dtype=bool)] > 0)


# ----------------------------------------------------------------------------- k_os_pairs
def pair_case(P, N, seed):
    """P pulsars of 20 .. 30 TOAs under white noise and one common process of N modes: the cheapest inputs that give
    k_os_pairs a full X."""
    rng = np.random.default_rng(seed)
    offs, toas, nu = random_layout(rng, P, (20, 31))
    f = np.arange(1, N + 1) / np.ptp(toas)
    phi = 1e-13 * np.arange(1, N + 1) ** -2.0
    return dict(offs=offs, toas=toas, nu=nu, n_modes=np.array([N], dtype=np.int32), f=f, idx=np.zeros(1),
                freqf=np.full(1, 1400.0), phi=phi, target=0, phi_hat=rng.uniform(0.5, 2.0, N) * phi,
                M=None, ncol=None, w=np.full(int(offs[-1]), 1e13), G=None)


def pair_weights(rng, P, J):
    """J symmetric matrices: a dense random one, then (J >= 3) one with a single nonzero pair and one of all ones on
    the first diagonal 16 x 16 tile, its diagonal included (an a <= b leak shows there), then random sparse ones."""
    G = rng.normal(size=(J, P, P))
    G = G + G.transpose(0, 2, 1)
    if J >= 3 and P >= 2:
        G[1] = 0.0
        a, b = (P - 1, P // 2) if P > 2 else (1, 0)
        G[1, a, b] = G[1, b, a] = 1.5
        G[2] = 0.0
        G[2, :16, :16] = 1.0
    for j in range(3, J):
        G[j] *= rng.uniform(size=(P, P)) < 0.3
        G[j] = np.triu(G[j], 1) + np.triu(G[j], 1).T
    return G


@pytest.mark.parametrize("P,N,R,J", [(1, 1, 1, 1), (2, 5, 16, 3), (3, 30, 17, 1), (16, 5, 33, 17), (17, 1, 16, 3),
                                     (17, 30, 1, 17), (33, 5, 17, 17), (33, 1, 33, 1), (100, 5, 17, 3),
                                     (100, 30, 33, 1), (100, 1, 1, 17)])
def test_pairs_are_the_definition_applied_to_the_device_x(ctx, P, N, R, J):
    c = pair_case(P, N, 1000 * P + 10 * N + R)
    rng = np.random.default_rng(J)
    G = pair_weights(rng, P, J)
    res = rng.normal(0.0, 1e-6, (R, int(c["offs"][-1])))
    Q, Qm, X, _, _ = one_shot(ctx, c, res, G)
    assert Q.shape == (J, R) and Qm.shape == (J, N, R) and X.shape == (P, 2 * N, R)
    if P == 1:
        assert np.all(Q == 0) and np.all(Qm == 0)  # no pair: exactly zero
        return
    assert np.any(Q != 0)
    check_q(f"P {P} N {N} R {R} J {J}", X, c["phi_hat"], G, Q, Qm)
    if J >= 3:
        a, b = (P - 1, P // 2) if P > 2 else (1, 0)
        one = 1.5 * c["phi_hat"][:, None] * (X[a, :N] * X[b, :N] + X[a, N:] * X[b, N:])
        mag = 1.5 * c["phi_hat"][:, None] * (np.abs(X[a, :N] * X[b, :N]) + np.abs(X[a, N:] * X[b, N:]))
        assert np.all(np.abs(Qm[1] - one) <= 8 * EPS * mag)  # the single pair, nothing else


def test_a_matrix_gives_the_same_bits_whatever_the_other_matrices(ctx):
    """k_os_pairs has instances for 1, 2, 4 and 8 matrices per workgroup and slices a longer list: a matrix's Q is the
    same bits alone, among 2, 3, 8, 9 and 17, first or last."""
    P, N, R = 33, 5, 17
    c = pair_case(P, N, 77)
    rng = np.random.default_rng(9)
    G = pair_weights(rng, P, 17)
    res = rng.normal(0.0, 1e-6, (R, int(c["offs"][-1])))
    Q, Qm, _, _, _ = one_shot(ctx, c, res, G)
    for sel in ([0], [16], [3, 0], [0, 1, 16], list(range(8)), list(range(9)), list(range(16, -1, -1))):
        q, qm, _, _, _ = one_shot(ctx, c, res, np.ascontiguousarray(G[sel]))
        np.testing.assert_array_equal(q, Q[sel])
        np.testing.assert_array_equal(qm, Qm[sel])


@pytest.mark.parametrize("name", ["k2", "k18", "k60"])
def test_blocks_and_order_do_not_change_a_bit(ctx, name):
    """A realization's X and Q are the same bits alone, among the first 16, among all 33 and in reversed order."""
    c = case(name)
    Q, Qm, X, _, _ = one_shot(ctx, c, c["res"])
    for sel in ([0], [32], list(range(16)), list(range(32, -1, -1)), [5, 31, 6]):
        q, qm, x, _, _ = one_shot(ctx, c, np.ascontiguousarray(c["res"][sel]))
        np.testing.assert_array_equal(x, X[:, :, sel])
        np.testing.assert_array_equal(q, Q[:, sel])
        np.testing.assert_array_equal(qm, Qm[:, :, sel])


# ----------------------------------------------------------------------------- batch path
class _Psr:
    """What BatchSimulator reads of a pulsar."""

    def __init__(self, toas, freqs, sigma2, pos, Mmat):
        self.toas, self.freqs, self.sigma2, self.pos, self.Mmat = toas, freqs, sigma2, pos, Mmat
        self.signal_model = {}

    def _white_sigma2(self):
        return self.sigma2


@pytest.fixture(scope="module")
def small(ctx):
    """The unbiasedness layout of tests/test_os_host.py as a BatchSimulator: 8 ragged pulsars, red noise and an HD
    background of 5 modes each, white noise, a design of 3 columns."""
    from fakepta_amd.batch import BatchSimulator
    lay = H.unbiased_layout()
    o = lay["offs"]
    psrs = [_Psr(lay["toas"][o[i]:o[i + 1]], lay["nu"][o[i]:o[i + 1]], lay["sigma"][o[i]:o[i + 1]] ** 2, lay["pos"][i],
                 lay["Mmats"][i]) for i in range(len(o) - 1)]
    sim = BatchSimulator(psrs, signals=[], white=True, ctx=ctx)
    sim.add_signal("red_noise", 0, lay["f_rn"], lay["amp_rn"])
    sim.add_signal("gw_common", 1, lay["f_gw"], lay["amp_gw"], L=lay["L"])
    sim.set_timing_model()
    return sim, psrs, lay


def composed(lay, block, G, nab_dev, n_orf, X_dev=None):
    """The truth of A2, snr, A2_joint and the binned rho for a block [R, n_toa], and the bound a device result is held
    to: X within its tolerance (the truth's B), Q within the dot-product bound on top of the X errors it inherits, the
    denominators within (K^2 + 3) eps of their terms' magnitudes."""
    per, nab_t = H.unbiased_truth()
    offs = lay["offs"]
    P, K = len(per), per[0][0].shape[0]
    N = K // 2
    phi_hat = lay["amp_gw"] ** 2
    Xt, xb = OS.x_truth([q[0] for q in per], offs, block)
    lit = np.stack([OS.operator_literal(lay["toas"][offs[p]:offs[p + 1]], lay["nu"][offs[p]:offs[p + 1]],
                                        lay["Mmats"][p], 1 / lay["sigma"][offs[p]:offs[p + 1]] ** 2, lay["comps_of"](p),
                                        lay["phis_of"](p), 1, np.ones(3, dtype=bool)) @ block[:, offs[p]:offs[p + 1]].T
                    for p in range(P)])
    dX = OS.x_tolerance(Xt, lit, xb)[0]
    if X_dev is not None:  # the batch path's X against the truth, the module's rule
        check_x("batch", X_dev, Xt, lit, xb, np.diff(offs))
    X64 = Xt.astype(np.float64)
    Qm_t, _, bq = OS.q_truth(X64, phi_hat, G)
    Qt = Qm_t.sum(axis=1)
    # what the X errors do to Q: sum |G| phi_hat (|dX_a| |X_b| + |X_a| |dX_b| + |dX_a| |dX_b|), cosine and sine
    ia, ib = np.tril_indices(P, -1)
    ph2 = np.concatenate([phi_hat, phi_hat])[None, :, None]
    aX = np.abs(X64) + dX
    cross = ((dX[ia] * aX[ib] + aX[ia] * dX[ib]) * ph2).sum(axis=1)  # [pairs, R]
    dQ = np.abs(G[:, ia, ib]) @ cross + 2 * bq
    il = np.tril_indices(P, -1)
    _, mag = OS.pair_norms([q[1] for q in per], phi_hat)
    dnab = (K * K + 3) * EPS * mag.astype(np.float64)
    norm_t = np.array([np.sum(g[il].astype(LD) ** 2 * nab_t[il]) for g in G]).astype(np.float64)
    dnorm = np.array([np.sum(g[il] ** 2 * dnab[il]) for g in G]) + 8 * EPS * np.abs(norm_t)
    assert np.all(np.abs(nab_dev.astype(LD) - nab_t) <= dnab)
    Qt = Qt.astype(np.float64)
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
    return dict(A2=(ratio[:n_orf], d_ratio[:n_orf]), snr=(snr, d_snr), rho_bins=(ratio[n_orf:], d_ratio[n_orf:]),
                A2_joint=(joint, d_joint))


def test_batch_statistic_end_to_end_and_after_project(ctx, small):
    sim, psrs, lay = small
    rank, nab = sim.set_optimal_statistic(orfs=("hd", "monopole", "dipole"), bins=5)
    assert list(rank) == [3] * 8 and nab.shape == (8, 8)
    R = 48
    sim.synth(R, seed=5, to_host=False)
    before = sim.checksums()
    out = sim.optimal_statistic(per_mode=True)
    np.testing.assert_array_equal(sim.checksums(), before)  # the block is untouched
    assert list(out["bin_counts"][-1:]) == [0] and out["bin_counts"].sum() == 28
    assert np.all(np.isnan(out["rho_bins"][-1])) and np.all(np.isfinite(out["rho_bins"][:-1]))
    assert out["Q"].shape == (8, R) and out["Q_mode"].shape == (8, 5, R) and out["norm"].shape == (8,)
    G = sim._os["G"]
    block = ctx.batch_download(0, R)
    _, _, X_dev = ctx.batch_os(coefficients=True)
    assert X_dev.shape == (8, 10, R)
    want = composed(lay, block, G, nab, 3, X_dev)
    live = out["bin_counts"] > 0
    worst = {}
    for key in ("A2", "snr", "A2_joint", "rho_bins"):
        t, d = want[key]
        got = out[key]
        if key == "rho_bins":
            t, d, got = t[live], d[live], got[live]
        err = np.abs(got - t)
        worst[key] = float(np.max(err / d))
        assert np.all(err <= d), (key, worst[key])
    print("end to end, largest error / composed bound:", {k: f"{v:.2e}" for k, v in worst.items()})
    print(f"A2 (HD) over {R} realizations: mean {out['A2'][0].mean():.3f}, std {out['A2'][0].std():.3f}")
    # the timing model is marginalised: projecting the block first changes A2 by rounding only
    sim.project()
    out_p = sim.optimal_statistic()
    want_p = composed(lay, ctx.batch_download(0, R), G, nab, 3)
    for key in ("A2", "snr", "A2_joint"):
        assert np.all(np.abs(out_p[key] - want_p[key][0]) <= want_p[key][1]), key
        assert np.all(np.abs(want_p[key][0] - want[key][0]) <= want[key][1]), key  # the definition does not see it
        assert np.all(np.abs(out_p[key] - out[key]) <= want_p[key][1] + want[key][1]), key
    sim.set_optimal_statistic()  # hd alone again, after the joint one
    assert "A2_joint" not in sim.optimal_statistic()


def test_fit_and_statistic_set_together_give_their_own_results(ctx, small):
    sim, psrs, lay = small
    sim.set_optimal_statistic()
    sim.ctx.batch_set_fit(None, None, None, None)
    sim.synth(20, seed=9, to_host=False)
    Q0, Qm0, X0 = ctx.batch_os(per_mode=True, coefficients=True)
    sim.set_fourier_fit([(4, 0.0), (3, 2.0)])
    coef0 = sim.fourier_fit()
    Q1, Qm1, X1 = ctx.batch_os(per_mode=True, coefficients=True)
    coef1 = sim.fourier_fit()
    np.testing.assert_array_equal(Q1, Q0)
    np.testing.assert_array_equal(Qm1, Qm0)
    np.testing.assert_array_equal(X1, X0)
    np.testing.assert_array_equal(coef1, coef0)
    assert coef0.shape == (8, 14, 20) and X0.shape == (8, 10, 20) and np.any(coef0 != 0) and np.any(X0 != 0)
    sim.ctx.batch_set_os(None, None, None, None, None, 0, None, None)  # clearing one leaves the other
    np.testing.assert_array_equal(sim.fourier_fit(), coef0)
    sim.set_optimal_statistic()
    sim.ctx.batch_set_fit(None, None, None, None)
    np.testing.assert_array_equal(ctx.batch_os()[0], Q0)


@pytest.fixture(scope="module")
def shared_span(capi):
    """C2's signal mix on 64 ragged pulsars over one common span (tests/test_gpu_next_mix.py): the layout whose
    pipelined k_grid_fused blocks also make the next block's common-signal mix (FPTA_OPT_FUSED_NEXT_MIX), with an
    optimal statistic of the whole model set (q = 320 Fourier columns)."""
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
    fs, phis = [], []
    for nm, idx in ((30, 0.0), (100, 2.0)):
        f = np.tile(np.arange(1, nm + 1) / (t1 - t0), (P, 1))
        amp = np.sqrt(O.powerlaw(f, rng.uniform(-14.5, -13.5, (P, 1)), 3.0) / (t1 - t0))
        c.batch_add_signal(0, f, amp, idx=idx)
        fs.append(f)
        phis.append(amp ** 2)
    fc = np.arange(1, 31) / (t1 - t0)
    ac = np.sqrt(O.powerlaw(fc, -14.0, 13 / 3) / (t1 - t0))
    v = rng.normal(size=(P, 3))
    hd = O.orf_hd(v / np.linalg.norm(v, axis=1)[:, None])
    c.batch_add_signal(1, fc, ac, L=batch_factor(hd))
    c.set_option(capi.OPT_SYNTH_PATH, 4)
    np.fill_diagonal(hd, 0.0)
    rank, nab = c.batch_set_os([30, 100, 30], np.concatenate(fs + [np.tile(fc, (P, 1))], axis=1), [0.0, 2.0, 0.0],
                               [1400.0] * 3, np.concatenate(phis + [np.tile(ac ** 2, (P, 1))], axis=1), 2, ac ** 2,
                               hd[None], weights=np.full(int(offs[-1]), 1e13))
    assert list(rank) == [0] * P and np.all(nab[~np.eye(P, dtype=bool)] > 0)
    yield c
    c.close()


@pytest.mark.parametrize("next_real0,hit", [(384, True), (1000, False)])
def test_statistic_leaves_the_block_and_the_next_block_alone(shared_span, next_real0, hit):
    """The block is bit for bit what it was, and the block after one whose statistic was taken is bit for bit the
    block after an untouched one, for a next-mix hit and for a miss."""
    c = shared_span
    outs = []
    for stat in (False, True):
        for real0 in (0, 128, 256):  # hits start at the third block of a pipelined run
            c.batch_synth(7, real0, 128, to_host=False)
        assert c.batch_grid_info()["interp_kernel"].startswith("k_grid_fused<")
        if stat:
            sums, pre = c.batch_checksums(), c.batch_download(0, 128)
            Q, _, _ = c.batch_os()
            assert Q.shape == (1, 128) and np.all(np.isfinite(Q)) and np.any(Q != 0)
            np.testing.assert_array_equal(c.batch_download(0, 128), pre)
            np.testing.assert_array_equal(c.batch_checksums(), sums)
        outs.append(c.batch_synth(7, next_real0, 128))
        assert c.batch_grid_info()["next_mix_used"] == hit
    np.testing.assert_array_equal(outs[1], outs[0])


# ----------------------------------------------------------------------------- state
def test_state_errors_and_set_toas_clears_the_statistic(capi):
    from fakepta_amd.batch import BatchSimulator
    c = capi.Context(0)
    try:
        p = pair_case(3, 2, 3)
        G = np.ones((1, 3, 3))
        args = (p["n_modes"], p["f"], p["idx"], p["freqf"], p["phi"], 0, p["phi_hat"], G)
        with pytest.raises(capi.FptaError, match="set_toas first"):
            c.batch_set_os(None, None, None, None, None, 0, None, None)
        c.batch_set_toas(p["offs"], p["toas"], p["nu"])
        c.batch_add_signal(1, p["f"], np.sqrt(p["phi"]), L=np.eye(3))
        with pytest.raises(capi.FptaError, match=r"\(-77\).*nothing synthesized"):
            c.batch_os()
        c.batch_synth(1, 0, 20, to_host=False)
        with pytest.raises(capi.FptaError, match=r"\(-77\).*no optimal statistic is set"):
            c.batch_os()
        rank, nab = c.batch_set_os(*args, weights=p["w"])
        assert list(rank) == [0, 0, 0] and nab.shape == (3, 3)
        assert c.batch_os_info() == dict(K=4, N=2, J=1, n_real=0)
        Q, Qm, X = c.batch_os(per_mode=True, coefficients=True)
        assert Q.shape == (1, 20) and Qm.shape == (1, 2, 20) and X.shape == (3, 4, 20)
        assert c.batch_os_info()["n_real"] == 20
        for bad, msg in ((dict(phi=-p["phi"]), r"\(-22\).*pulsar 0, component 0, mode 0: prior variance"),
                         (dict(phi_hat=p["phi_hat"] * [1.0, 0.0]), r"\(-22\).*target mode 1: template"),
                         (dict(G=np.triu(np.ones((1, 3, 3)))), r"\(-22\).*pair \(0, 1\): not symmetric"),
                         (dict(G=np.full((1, 3, 3), np.nan)), r"\(-22\).*pair \(0, 1\): not finite")):
            a = dict(zip(("n_modes", "f", "idx", "freqf", "phi", "target", "phi_hat", "G"), args))
            a.update(bad)
            with pytest.raises(capi.FptaError, match=msg):
                c.batch_set_os(*a.values(), weights=p["w"])
            np.testing.assert_array_equal(c.batch_os()[0], Q)  # a refused call leaves the statistic that was set
        rank, _ = c.batch_set_os(None, None, None, None, None, 0, None, None)  # cleared
        assert list(rank) == [0, 0, 0]
        with pytest.raises(capi.FptaError, match="no optimal statistic is set"):
            c.batch_os()
        c.batch_set_os(*args, weights=p["w"])
        c.batch_set_toas(p["offs"], p["toas"], p["nu"])  # a new layout: the statistic is gone
        c.batch_add_signal(1, p["f"], np.sqrt(p["phi"]), L=np.eye(3))
        c.batch_synth(1, 0, 20, to_host=False)
        with pytest.raises(capi.FptaError, match="no optimal statistic is set"):
            c.batch_os()
        c.set_option(capi.OPT_PROFILE, 1)  # one FPTA_K_DENSE entry per call, both stages
        c.batch_set_os(*args, weights=p["w"])
        c.reset_stats()
        c.batch_os()
        c.synchronize()
        assert c.kernel_stats(capi.K_DENSE)[0] == 1
        # the target of a layout with no common signal, or with several, has to be named
        psrs = [_Psr(p["toas"][p["offs"][i]:p["offs"][i + 1]], p["nu"][p["offs"][i]:p["offs"][i + 1]],
                     np.full(p["offs"][i + 1] - p["offs"][i], 1e-13), np.eye(3)[i], np.zeros((p["offs"][i + 1] - p["offs"][i], 0)))
                for i in range(3)]
        sim = BatchSimulator(psrs, signals=[], white=False, ctx=c)
        with pytest.raises(ValueError, match="0 common signals"):
            sim.set_optimal_statistic()
        sim.add_signal("gw_common", 1, p["f"], np.sqrt(p["phi"]), L=np.eye(3))
        sim.add_signal("clock_common", 1, p["f"], np.sqrt(p["phi"]), L=np.ones((3, 3)))
        with pytest.raises(ValueError, match="2 common signals"):
            sim.set_optimal_statistic()
        sim.set_optimal_statistic(target="gw_common", orfs=("monopole",))
        sim.synth(4, seed=1, to_host=False)
        assert sim.optimal_statistic()["A2"].shape == (1, 4)
    finally:
        c.close()


# ----------------------------------------------------------------------------- drop-in
def test_drop_in_equals_the_one_shot_call(ctx):
    from fakepta import correlated_noises as cn
    from fakepta import fake_pta as fp
    from fakepta_amd import os as osm
    np.random.seed(12)
    psrs = fp.make_fake_array(npsrs=4, Tobs=10, ntoas=90, gaps=True, toaerr=1e-7, pdist=1.0,
                              freqs=[800, 1400, 2500], backends=["A", "B"],
                              custom_model={"RN": 10, "DM": 10, "Sv": None})
    cn.add_common_correlated_noise(psrs, orf="hd", spectrum="powerlaw", name="gw", components=6, log10_A=-13.5,
                                   gamma=13 / 3)
    keep = [p.residuals.copy() for p in psrs]
    out = fp.optimal_statistic_array(psrs, orfs=("hd", "monopole"), bins=3, per_mode=True)
    for p, k in zip(psrs, keep):
        np.testing.assert_array_equal(p.residuals, k)
    segs = osm.segments_of(psrs)
    assert [s["name"] for s in segs] == ["red_noise", "dm_gp", "gw_common"] and osm.pick_target(segs) == 2
    model = osm.noise_model(segs, 4)
    G, n_orf, centres, counts = osm.pair_matrices(psrs, ("hd", "monopole"), 3)
    offs = np.concatenate([[0], np.cumsum([len(p.toas) for p in psrs])]).astype(np.int64)
    assert len(set(np.diff(offs))) > 1  # ragged
    from fakepta_amd import tm
    M, ncol = tm.stack_design([p.Mmat for p in psrs])
    phi_hat = model["phi"][0, 20:26]
    Q, Qm, X, rank, nab = ctx.os_statistic(
        offs, np.concatenate([p.toas for p in psrs]), np.concatenate([p.freqs for p in psrs]), model["n_modes"],
        model["f"], model["idx"], model["freqf"], model["phi"], 2, phi_hat, G,
        np.concatenate([p.residuals for p in psrs]), M=M, ncol_psr=ncol,
        weights=np.concatenate([1 / p._white_sigma2() for p in psrs]))
    np.testing.assert_array_equal(out["Q"], Q)
    np.testing.assert_array_equal(out["Q_mode"], Qm)
    want = osm.derive(Q, G, nab, 2, centres, counts)
    for key in ("A2", "snr", "A2_joint", "rho_bins", "norm", "bin_counts"):
        np.testing.assert_array_equal(out[key], want[key])
    assert out["A2"].shape == (2, 1) and np.all(np.isfinite(out["A2"])) and np.all(out["norm"][:2] > 0)
    # the statistic is the definition applied to X here too
    check_q("drop-in", X, phi_hat, G, Q, Qm)
