"""Correlated likelihood grid on the device (fpta_clnl_grid, fpta_batch_set_clnl, fpta_batch_clnl: k_fit_apply on its
fifth operator slot, k_clnl_fill, dense.hip's blocked Cholesky, k_clnl_logdet, k_clnl_mix, k_clnl_solve, k_clnl_reduce)
and the Python surface above it, against the np.longdouble definition of tests/clnl_reference.py.

Each stage is held to the definition applied to the device's own inputs: V to the dot-product bound from the device's
X; q and ld to the plan's fp64 T and s, in units of n eps cond_2(C_g) q and n eps cond_2(C_g) max(1, |ld|): the
backward error of a Cholesky factorisation and a triangular solve is a modest multiple of n eps, and it reaches q and
ld through cond(C). Exact zeros and bit identities are compared exactly.

The cases of tests/launch_axes.py run k_clnl_mix and k_clnl_solve on three realization tiles (R = 130: vld = 192, the
last tile with 32 padded and 32 dead columns) under the same checkers: every stage, the bit identity of the
realizations at the tiles' edges, and a second batch block against the composed truth."""
import numpy as np
import pytest

from tests import clnl_reference as CR
from tests import launch_axes as AX
from tests import lnl_reference as LR
from tests import os_reference as OS
from tests import test_clnl_host as CH
from tests import test_gpu_os as GO
from tests import test_lnl_host as LH
from tests import test_os_host as H

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
LD = np.longdouble

# Measured on the stage shapes below, the largest over ORFs, grid points and realizations: |q - q_ld| = 0.0024 units of
# n eps cond_2(C) q and |ld - ld_ld| = 0.0022 units of n eps cond_2(C) max(1, |ld|), both on P 17, K 8 (cond_2(C) = 2.0e8
# at the row 1e6 x the intrinsic level; the other shapes stay below 0.0003 and 0.0001): the errors are backward errors
# of a few n eps and do not grow with cond(C) on these inputs. Asserted at 4 x.
Q_MEASURED_UNITS, LD_MEASURED_UNITS = 0.0024, 0.0022
Q_BOUND_UNITS, LD_BOUND_UNITS = 4 * Q_MEASURED_UNITS, 4 * LD_MEASURED_UNITS


@pytest.fixture(scope="module")
def capi():
    from fakepta_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def ctx(capi):
    c = capi.Context(0)
    yield c
    c.close()


# ----------------------------------------------------------------------------- stage by stage
_STAGE = {}
_FACTORS = {}


def stage_case(P, K, G, empty=True):
    """P pulsars of 20 .. 30 TOAs, the second one without TOAs when `empty`, under white noise and one common process of
    K / 2 modes; a grid [G, N] within a factor 10 of the process's level with a third of its modes zero, for G >= 3 an
    all-zero row and a last row 1e6 x the intrinsic level (for G = 1 the one row is 1e6 x it on every third mode); the
    Hellings-Downs ORF of random positions and the rank-1 monopole."""
    key = (P, K, G, empty)
    if key not in _STAGE:
        rng = np.random.default_rng(1000 * P + 10 * K + G)
        N = K // 2
        counts = rng.integers(20, 31, size=P)
        if empty:
            counts[1] = 0
        offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        toas = np.concatenate([np.sort(rng.uniform(0.0, 3e8, k)) for k in counts])
        nu = rng.choice([800.0, 1400.0, 2500.0], size=int(offs[-1]))
        phi = 1e-13 * np.arange(1, N + 1) ** -2.0
        grid = phi[None, :] * 10.0 ** rng.uniform(-1, 1, (G, N)) * (rng.uniform(size=(G, N)) > 1 / 3)
        if G >= 3:
            grid[1] = 0.0
            grid[-1] = 1e6 * phi
        else:
            grid[0, ::3] = 1e6 * phi[::3]
        orfs = CR.orfs_of(P, seed=P)
        A = np.stack([CR.factor_of(orfs["hd"]), CR.factor_of(orfs["monopole"])])
        _STAGE[key] = dict(offs=offs, toas=toas, nu=nu, n_modes=np.array([N], dtype=np.int32),
                           f=np.arange(1, N + 1) / 3e8, idx=np.zeros(1), freqf=np.full(1, 1400.0), phi=phi, target=0,
                           grid=grid, A=A, w=np.full(int(offs[-1]), 1e13), counts=counts)
    return _STAGE[key]


def one_shot(ctx, c, res, grid=None, A=None, tables=False):
    return ctx.clnl_grid(c["offs"], c["toas"], c["nu"], c["n_modes"], c["f"], c["idx"], c["freqf"], c["phi"],
                         c["target"], c["grid"] if grid is None else grid, c["A"] if A is None else A, res,
                         weights=c["w"], tables=tables)


def factors_of(key, T, grid, P):
    """Per (ORF, grid point) the longdouble (L, ld, cond, s) of the plan's fp64 T and s, once per case (the plan is the
    same for every number of realizations: T is compared with the cached one)."""
    if key not in _FACTORS:
        out = []
        for o in range(len(T)):
            row = []
            for g in range(len(grid)):
                s = CR.scale_of(grid[g], P).astype(np.float64)  # the plan's s, rounded once
                row.append(CR.factor(T[o], s) + (s,))
            out.append(row)
        _FACTORS[key] = (T.copy(), out)
    np.testing.assert_array_equal(_FACTORS[key][0], T)
    return _FACTORS[key][1]


def check_stages(label, key, c, d, q, V, X, ld, T):
    """V from the device's X within the dot-product bound; q and ld from the plan's T and s and the device's V within
    the bound units; dlnL = (q - ld) / 2 bit for bit. Returns the largest q and ld errors in units."""
    J, G, R = q.shape
    P, K = X.shape[:2]
    n = P * K
    worst_v = worst_q = worst_ld = worst_c = 0.0
    fac = factors_of(key, T, c["grid"], P)
    for o in range(J):
        Vt, vb = CR.mix(c["A"][o], list(X))
        ev = np.abs(V[o].astype(LD) - Vt).astype(np.float64)
        worst_v = max(worst_v, float(np.max(ev / np.maximum(vb, 1e-300))))
        assert np.all(ev <= vb), (label, "V", o)
        for g in range(G):
            L, ldt, cond, s = fac[o][g]
            qt = CR.quad(L, s, V[o])
            unit_q = n * EPS * cond * qt.astype(np.float64)
            unit_ld = n * EPS * cond * max(1.0, abs(float(ldt)))
            eq = np.abs(q[o, g].astype(LD) - qt).astype(np.float64)
            eld = abs(float(LD(ld[o, g]) - ldt))
            if np.any(qt > 0):
                worst_q = max(worst_q, float(np.max(eq[qt > 0] / unit_q[qt > 0])))
            assert np.all(eq[qt == 0] == 0)
            worst_ld = max(worst_ld, eld / unit_ld)
            worst_c = max(worst_c, cond)
    print(f"{label}: V error / bound {worst_v:.3f}; q error {worst_q:.4f} units of n eps cond q, ld error "
          f"{worst_ld:.4f} units of n eps cond max(1, |ld|); cond_2(C) <= {worst_c:.3g}")
    np.testing.assert_array_equal(d, 0.5 * (q - ld[:, :, None]))
    return worst_q, worst_ld


# (P, K, G): n = 12 (one ragged block), 70 (two blocks, the second ragged), 136 (three blocks), 256 (exactly four);
# R = 1, 16, 33 (one realization tile) on each, and launch_axes.py's R = 130 (three tiles) on n = 12 and n = 70
@pytest.mark.parametrize("P,K,G,R", [(P, K, G, R) for P, K, G in [(3, 4, 1), (5, 14, 3), (17, 8, 3), (4, 64, 1)]
                                     for R in (1, 16, 33)] + [s + (AX.CLNL_R,) for s in AX.CLNL_STAGES])
def test_every_stage_is_the_definition_applied_to_the_device_inputs(ctx, P, K, G, R):
    c = stage_case(P, K, G)
    res = np.random.default_rng(R).normal(0.0, 1e-6, (R, int(c["offs"][-1])))
    d, q, V, X, rank, ld, T = one_shot(ctx, c, res, tables=True)
    n = P * K
    assert d.shape == (2, G, R) and q.shape == (2, G, R) and V.shape == (2, n, R) and X.shape == (P, K, R)
    assert ld.shape == (2, G) and T.shape == (2, n, n) and list(rank) == [0] * P
    assert np.any(q != 0) and np.all(np.isfinite(d)) and np.all(X[1] == 0)  # the pulsar without TOAs
    for o in range(2):
        np.testing.assert_array_equal(T[o], T[o].T)
    wq, wld = check_stages(f"P {P} K {K} G {G} R {R}", (P, K, G), c, d, q, V, X, ld, T)
    assert wq <= Q_BOUND_UNITS and wld <= LD_BOUND_UNITS, (wq, wld)
    if G >= 3:  # the all-zero row: exactly 0 for every ORF and realization
        assert np.all(d[:, 1] == 0.0) and np.all(q[:, 1] == 0.0) and np.all(ld[:, 1] == 0.0)
        assert np.all(ld[:, [0, 2]] > 0)


def test_blocks_order_and_grid_size_do_not_change_a_bit(ctx):
    """A realization's column is the same bits alone, among the first 16, among all 33 and in reversed order; a grid
    point's row is the same alone and inside G = 3; an ORF's results are the same alone and beside another."""
    c = stage_case(5, 14, 3)
    res = np.random.default_rng(3).normal(0.0, 1e-6, (33, int(c["offs"][-1])))
    d, q, V, X, _, ld, _ = one_shot(ctx, c, res)
    for sel in ([0], [32], list(range(16)), list(range(32, -1, -1)), [5, 31, 6]):
        d1, q1, v1, x1, _, _, _ = one_shot(ctx, c, np.ascontiguousarray(res[sel]))
        np.testing.assert_array_equal(x1, X[:, :, sel])
        np.testing.assert_array_equal(v1, V[:, :, sel])
        np.testing.assert_array_equal(q1, q[:, :, sel])
        np.testing.assert_array_equal(d1, d[:, :, sel])
    for g in range(3):
        d1, q1, _, _, _, ld1, _ = one_shot(ctx, c, res, grid=c["grid"][g:g + 1])
        np.testing.assert_array_equal(d1[:, 0], d[:, g])
        np.testing.assert_array_equal(q1[:, 0], q[:, g])
        np.testing.assert_array_equal(ld1[:, 0], ld[:, g])
    d1, _, v1, _, _, ld1, _ = one_shot(ctx, c, res, A=c["A"][1:])
    np.testing.assert_array_equal(d1[0], d[1])
    np.testing.assert_array_equal(v1[0], V[1])
    np.testing.assert_array_equal(ld1[0], ld[1])


def test_tiles_past_the_first_do_not_change_a_bit(ctx):
    """R = 130 on n = 70 (three realization tiles, two block rows): the realizations at the tiles' edges are the same
    bits alone (tile 0 of a block of one) as inside the block, in X, V, q and dlnL."""
    c = stage_case(5, 14, 3)
    R = AX.CLNL_R
    res = np.random.default_rng(3).normal(0.0, 1e-6, (R, int(c["offs"][-1])))
    d, q, V, X, _, ld, _ = one_shot(ctx, c, res)
    assert d.shape == (2, 3, R) and V.shape == (2, 70, R) and np.all(np.isfinite(d)) and np.all(q[:, [0, 2]] > 0)
    for r in AX.CLNL_REALS:
        d1, q1, v1, x1, _, ld1, _ = one_shot(ctx, c, np.ascontiguousarray(res[[r]]))
        np.testing.assert_array_equal(ld1, ld)
        np.testing.assert_array_equal(x1, X[:, :, [r]], err_msg=f"realization {r}")
        np.testing.assert_array_equal(v1, V[:, :, [r]], err_msg=f"realization {r}")
        np.testing.assert_array_equal(q1, q[:, :, [r]], err_msg=f"realization {r}")
        np.testing.assert_array_equal(d1, d[:, :, [r]], err_msg=f"realization {r}")


# ----------------------------------------------------------------------------- batch path
@pytest.fixture(scope="module")
def small(ctx):
    """The unbiasedness layout of tests/test_os_host.py as a BatchSimulator, the common process drawn HD-correlated,
    with one block of 48 realizations on the device."""
    from fakepta_amd.batch import BatchSimulator
    lay = H.unbiased_layout()
    o = lay["offs"]
    psrs = [GO._Psr(lay["toas"][o[i]:o[i + 1]], lay["nu"][o[i]:o[i + 1]], lay["sigma"][o[i]:o[i + 1]] ** 2,
                    lay["pos"][i], lay["Mmats"][i]) for i in range(len(o) - 1)]
    sim = BatchSimulator(psrs, signals=[], white=True, ctx=ctx)
    sim.add_signal("red_noise", 0, lay["f_rn"], lay["amp_rn"])
    sim.add_signal("gw_common", 1, lay["f_gw"], lay["amp_gw"], L=lay["L"])
    sim.set_timing_model()
    sim.synth(48, seed=5, to_host=False)
    return sim, psrs, lay


def small_grid(lay):
    """A 2 x 2 grid around the injected spectrum."""
    from fakepta_amd import lnl
    return lnl.powerlaw_grid(lay["f_gw"], [-13.6, -13.3], [13 / 3, 3.0])


_SMALL = {}


def small_truth(lay):
    """Per pulsar (B0, Z, the literal operator) of the layout with the common process left out, once."""
    if "per" not in _SMALL:
        per = []
        for p in range(len(lay["offs"]) - 1):
            sl = slice(int(lay["offs"][p]), int(lay["offs"][p + 1]))
            args = (lay["toas"][sl], lay["nu"][sl], lay["Mmats"][p], 1 / lay["sigma"][sl] ** 2, lay["comps_of"](p))
            B, Z, norms, keep = LR.base_operator(*args, lay["phis_of"](p), 1)
            lit = OS.operator_literal(*args, [lay["phis_of"](p)[0], np.zeros(len(lay["f_gw"]))], 1, keep)
            per.append((B, Z, lit))
        _SMALL["per"] = per
    return _SMALL["per"]


def x_of(lay, P, block):
    """(X truth [P, K, R] longdouble, its tolerance on the device) of the first P pulsars."""
    per, offs = small_truth(lay)[:P], lay["offs"]
    Xt, xb = OS.x_truth([q[0] for q in per], offs[:P + 1], block)
    lit = np.stack([per[p][2] @ block[:, offs[p]:offs[p + 1]].T for p in range(P)])
    return Xt, OS.x_tolerance(Xt, lit, xb)[0]


def composed_clnl(lay, P, block, grid, As):
    """(dlnL truth [n_orf, G, R] as fp64, the bound a device result is held to) of the first P pulsars. The device's X is
    within dX of the truth (the truth's B0 and the literal form), so V is within dV = |A|^T dX + (P + 2) eps |A|^T (|X|
    + dX); the plan's T and s are within the host test's bounds, so C is within dC, |dC_ij| <= eps (T_BOUND s_i s_j
    rowmax_i |T| + 2 S_BOUND |s_i T_ij s_j|). To first order, with b = |D dV|_2 and every eigenvalue of C >= 1: |dq| <=
    2 sqrt(q) b + b^2 + q |dC|_F and |d ld| = |tr(C^-1 dC)| <= sqrt(n) |dC|_F; the stages add their bound units, the
    reduction one rounding."""
    Xt, dX = x_of(lay, P, block)
    per = small_truth(lay)[:P]
    K, R = Xt.shape[1], Xt.shape[2]
    n = P * K
    d, bound = np.zeros((len(As), len(grid), R)), np.zeros((len(As), len(grid), R))
    for o, A in enumerate(As):
        aA = np.abs(np.asarray(A, dtype=np.float64))
        Tm = CR.t_matrix([q[1] for q in per], A)
        V, _ = CR.mix(A, list(Xt))
        aX = np.abs(Xt).astype(np.float64)
        dV = np.concatenate([np.tensordot(aA[:, j], dX + (P + 2) * EPS * (aX + dX), axes=(0, 0)) for j in range(P)])
        rowmax = np.max(np.abs(Tm), axis=1).astype(np.float64)
        for g in range(len(grid)):
            s = CR.scale_of(grid[g], P)
            L, ld, cond = CR.factor(Tm, s)
            q = CR.quad(L, s, V).astype(np.float64)
            s64 = s.astype(np.float64)
            off = np.abs(s64[:, None] * Tm.astype(np.float64) * s64[None, :])
            dC = EPS * (CH.T_BOUND_EPS * s64[:, None] * s64[None, :] * rowmax[:, None] + 2 * CH.S_BOUND_EPS * off)
            dCn = float(np.sqrt(np.sum(dC * dC)))
            b = np.sqrt(np.sum((s64[:, None] * dV) ** 2, axis=0))
            dq = 2 * np.sqrt(q) * b + b * b + q * dCn + Q_BOUND_UNITS * n * EPS * cond * q
            dld = np.sqrt(n) * dCn + LD_BOUND_UNITS * n * EPS * cond * max(1.0, abs(float(ld)))
            d[o, g] = ((CR.quad(L, s, V) - ld) / 2).astype(np.float64)
            bound[o, g] = (dq + dld) / 2 + EPS * np.abs(d[o, g])
    return d, bound


def composed_lnl(lay, P, block, grid):
    """(dlnL truth [G, R] as fp64, the bound) of likelihood_grid() on the first P pulsars: tests/test_gpu_lnl.py's
    composed bound (X within its tolerance, U and ld within the host test's measured bounds, lnl_reference's stage-2
    allowance on top)."""
    Xt, dX = x_of(lay, P, block)
    per = small_truth(lay)[:P]
    G, R, K = len(grid), block.shape[0], Xt.shape[1]
    d, bound, mag = np.zeros((G, R), dtype=LD), np.zeros((G, R)), np.zeros((G, R))
    for p in range(P):
        Us, lds, _ = LR.grid_truth(per[p][1], grid)
        aX = np.abs(Xt[p]).astype(np.float64)
        for g in range(G):
            U, ld = Us[g], lds[g]
            aU = np.abs(U).astype(np.float64)
            dU = LH.U_BOUND_EPS * EPS * np.max(aU, axis=1, keepdims=True)
            y = U @ Xt[p]
            e = aU @ dX[p] + dU * np.sum(aX + dX[p], axis=0, keepdims=True) + (K + 2) * EPS * (aU @ aX)
            q = np.sum(y * y, axis=0)
            ay = np.abs(y).astype(np.float64)
            dq = np.sum(2 * ay * e + e * e, axis=0) + (K + 3) * EPS * q.astype(np.float64)
            dld = LH.LD_BOUND_EPS * EPS * max(1.0, abs(float(ld)))
            d[g] = d[g] + (q - ld) / 2
            bound[g] += (dq + dld) / 2
            mag[g] += (np.abs(q).astype(np.float64) + abs(float(ld))) / 2
    return d.astype(np.float64), bound + (P + 3) * EPS * mag + EPS * np.abs(d).astype(np.float64)


def test_batch_grid_end_to_end(ctx, small):
    sim, psrs, lay = small
    rank = sim.set_correlated_likelihood(log10_A=[-13.6, -13.3], gamma=[13 / 3, 3.0])
    assert list(rank) == [3] * 8 and ctx.batch_clnl_info() == dict(K=10, G=4, n_orf=2, n_real=0)
    grid = sim._clnl["phi"]
    np.testing.assert_array_equal(grid, small_grid(lay))
    before = sim.checksums()
    out = sim.correlated_likelihood(posterior=True)
    np.testing.assert_array_equal(sim.checksums(), before)  # the block is untouched
    R = 48
    assert ctx.batch_clnl_info()["n_real"] == R and out["orfs"] == ["hd", "curn"]
    assert out["dlnL"].shape == (2, 2, 2, R) and out["lnB"].shape == (2, R) and out["lnB_vs_curn"].shape == (2, R)
    assert np.all(out["lnB_vs_curn"][1] == 0) and np.allclose(out["posterior"].sum(axis=(1, 2)), 1.0)
    flat = out["dlnL"].reshape(2, 4, R)
    for o in range(2):
        np.testing.assert_array_equal(np.ravel_multi_index((out["argmax"][0][o], out["argmax"][1][o]), (2, 2)),
                                      np.argmax(flat[o], axis=0))
    from fakepta_amd import clnl
    As = clnl.orf_factors(psrs, ("hd", "curn"))[2]  # the factors the simulator handed to the device
    want, bound = composed_clnl(lay, 8, ctx.batch_download(0, R), grid, As)
    err = np.abs(flat - want)
    print(f"end to end: largest error / composed bound {float(np.max(err / bound)):.3e}; mean dlnL_hd - dlnL_curn at "
          f"the injected point {float(np.mean(flat[0, 0] - flat[1, 0])):.3f}, mean lnB_vs_curn "
          f"{float(out['lnB_vs_curn'][0].mean()):.3f}")
    assert np.all(err <= bound)
    # a second block of 130 realizations: three tiles of k_clnl_mix and k_clnl_solve on the cached factors
    R2 = AX.CLNL_R
    try:
        sim.synth(R2, seed=6, real0=48, to_host=False)
        before = sim.checksums()
        out = sim.correlated_likelihood()
        np.testing.assert_array_equal(sim.checksums(), before)
        assert ctx.batch_clnl_info()["n_real"] == R2 and out["dlnL"].shape == (2, 2, 2, R2)
        flat = out["dlnL"].reshape(2, 4, R2)
        for o in range(2):
            np.testing.assert_array_equal(np.ravel_multi_index((out["argmax"][0][o], out["argmax"][1][o]), (2, 2)),
                                          np.argmax(flat[o], axis=0))
        want, bound = composed_clnl(lay, 8, ctx.batch_download(0, R2), grid, As)
        err = np.abs(flat - want)
        print(f"second block, R {R2}: largest error / composed bound {float(np.max(err / bound)):.3e}")
        assert np.all(err <= bound)
    finally:
        sim.synth(48, seed=5, to_host=False)  # the fixture's block, for the tests after this one

def test_identity_orf_is_the_likelihood_grid(ctx, small):
    """Gamma = I against likelihood_grid() of the same model on the same block, inside the sum of both paths' bounds."""
    sim, psrs, lay = small
    grid = small_grid(lay)
    R = 48
    block = ctx.batch_download(0, R)
    sim.set_likelihood_grid(phi=grid)
    sim.set_correlated_likelihood(orfs=["curn"], phi=grid)
    dl = sim.likelihood_grid()["dlnL"]
    dc = sim.correlated_likelihood()["dlnL"][0]
    tc, bc = composed_clnl(lay, 8, block, grid, [np.eye(8)])
    tl, bl = composed_lnl(lay, 8, block, grid)
    slack = np.abs(tc[0] - tl)
    print(f"Gamma = I: largest |clnl - lnl| / (sum of the bounds) {float(np.max(np.abs(dc - dl) / (bc[0] + bl))):.3e}; "
          f"the two truths differ by <= {float(np.max(slack)):.2e}")
    assert np.all(np.abs(dc - dl) <= bc[0] + bl)
    sim.ctx.batch_set_lnl(None, None, None, None, None, 0, None)


def test_one_pulsar_is_the_likelihood_grid_of_the_scaled_spectrum(ctx, small):
    """P = 1: Gamma = [[gamma]] scales into phi. The one-shot calls on the first pulsar's part of the block."""
    from fakepta_amd import tm
    sim, psrs, lay = small
    grid, gam = small_grid(lay), 2.5
    n1 = int(lay["offs"][1])
    block = np.ascontiguousarray(ctx.batch_download(0, 48)[:, :n1])
    M, ncol = tm.stack_design(lay["Mmats"][:1])
    args = (lay["offs"][:2], lay["toas"][:n1], lay["nu"][:n1], [5, 5], np.concatenate([lay["f_rn"][0], lay["f_gw"]])[None],
            [0.0, 0.0], [1400.0, 1400.0], np.concatenate([lay["amp_rn"][0] ** 2, lay["amp_gw"] ** 2])[None], 1)
    kw = dict(M=M, ncol_psr=ncol, weights=1 / lay["sigma"][:n1] ** 2)
    A = np.array([[[np.sqrt(gam)]]])
    dc, _, _, Xc, _, _, _ = ctx.clnl_grid(*args, grid, A, block, **kw)
    dl, _, Xl, _, _, _ = ctx.lnl_grid(*args, gam * grid, block, **kw)
    np.testing.assert_array_equal(Xc, Xl)  # the same operator on the same kernel
    tc, bc = composed_clnl(lay, 1, block, grid, A)
    tl, bl = composed_lnl(lay, 1, block, gam * grid)
    slack = np.abs(tc[0] - tl)
    print(f"P = 1: largest |clnl - lnl| / (sum of the bounds) {float(np.max(np.abs(dc[0] - dl) / (bc[0] + bl))):.3e}; "
          f"the two truths differ by <= {float(np.max(slack)):.2e}")
    assert np.all(np.abs(dc[0] - dl) <= bc[0] + bl)
    assert np.any(np.abs(dc[0]) > 1e-3)


def _arrays(out):
    return {k: v for k, v in out.items() if isinstance(v, np.ndarray)}


def test_the_other_slots_and_the_block_are_left_alone(ctx, capi, small):
    """With the Fourier fit, the optimal statistic, the likelihood grid, the F-statistic and the correlated grid all set,
    every result is bitwise what it is with its feature set alone, before and after a correlated call; the block's
    checksums are unchanged by the call; one FPTA_K_DENSE entry per call."""
    sim, psrs, lay = small
    c = sim.ctx
    grid = small_grid(lay)

    def clear():
        c.batch_set_fit(None, None, None, None)
        c.batch_set_os(None, None, None, None, None, 0, None, None)
        c.batch_set_lnl(None, None, None, None, None, 0, None)
        c.batch_set_clnl(None, None, None, None, None, 0, None, None)

    clear()
    sim.set_correlated_likelihood(phi=grid)
    alone = dict(clnl=c.batch_clnl(quadratic=True, mixed=True, coefficients=True))
    clear()
    sim.set_fourier_fit([(4, 0.0), (3, 2.0)])
    alone["fit"] = sim.fourier_fit()
    clear()
    sim.set_optimal_statistic()
    alone["os"] = c.batch_os(per_mode=True, coefficients=True)
    clear()
    sim.set_likelihood_grid(phi=grid)
    alone["lnl"] = c.batch_lnl(per_pulsar=True, coefficients=True)
    clear()
    sim.set_fe_statistic(np.array([2e-8, 5e-8]), nside=1)
    alone["fe"] = _arrays(sim.fe_statistic(full=True))
    sim.set_fourier_fit([(4, 0.0), (3, 2.0)])
    sim.set_optimal_statistic()
    sim.set_likelihood_grid(phi=grid)
    sim.set_correlated_likelihood(phi=grid)
    sums = sim.checksums()
    for _ in range(2):
        got = c.batch_clnl(quadratic=True, mixed=True, coefficients=True)
        for a, b in zip(got, alone["clnl"]):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(sim.checksums(), sums)
        np.testing.assert_array_equal(sim.fourier_fit(), alone["fit"])
        for a, b in zip(c.batch_os(per_mode=True, coefficients=True), alone["os"]):
            np.testing.assert_array_equal(a, b)
        for a, b in zip(c.batch_lnl(per_pulsar=True, coefficients=True), alone["lnl"]):
            np.testing.assert_array_equal(a, b)
        fe = _arrays(sim.fe_statistic(full=True))
        assert fe.keys() == alone["fe"].keys()
        for k in fe:
            np.testing.assert_array_equal(fe[k], alone["fe"][k])
    assert np.any(alone["clnl"][0] != 0) and alone["clnl"][2].shape == (2, 80, 48)
    c.set_option(capi.OPT_PROFILE, 1)
    try:
        c.reset_stats()
        c.batch_clnl()
        c.synchronize()
        assert c.kernel_stats(capi.K_DENSE)[0] == 1
    finally:
        c.set_option(capi.OPT_PROFILE, 0)
    clear()
    with pytest.raises(capi.FptaError, match="no correlated likelihood grid is set"):
        c.batch_clnl()


# ----------------------------------------------------------------------------- errors and state
def test_errors_and_state(capi):
    c = capi.Context(0)
    try:
        p = stage_case(3, 4, 1, empty=False)  # a batch layout needs a TOA per pulsar
        args = (p["n_modes"], p["f"], p["idx"], p["freqf"], p["phi"], 0, p["grid"], p["A"])
        with pytest.raises(capi.FptaError, match="set_toas first"):
            c.batch_set_clnl(None, None, None, None, None, 0, None, None)
        c.batch_set_toas(p["offs"], p["toas"], p["nu"])
        c.batch_add_signal(1, p["f"], np.sqrt(p["phi"]), L=np.eye(3))
        with pytest.raises(capi.FptaError, match=r"\(-77\).*nothing synthesized"):  # no block
            c.batch_clnl()
        c.batch_synth(1, 0, 20, to_host=False)
        with pytest.raises(capi.FptaError, match=r"\(-77\).*no correlated likelihood grid is set"):  # before setting
            c.batch_clnl()
        rank, ld = c.batch_set_clnl(*args, weights=p["w"])
        assert list(rank) == [0, 0, 0] and ld.shape == (2, 1) and np.all(ld > 0)
        assert c.batch_clnl_info() == dict(K=4, G=1, n_orf=2, n_real=0)
        d, q, V, X = c.batch_clnl(quadratic=True, mixed=True, coefficients=True)
        assert d.shape == (2, 1, 20) and q.shape == (2, 1, 20) and V.shape == (2, 12, 20) and X.shape == (3, 4, 20)
        assert c.batch_clnl_info()["n_real"] == 20
        # a target whose frequencies differ between pulsars
        f2 = np.tile(p["f"], (3, 1))
        f2[2, 1] *= 1.01
        with pytest.raises(capi.FptaError,
                           match=r"\(-22\).*target component 0: pulsar 2, mode 1 has its own frequency"):
            c.batch_set_clnl(p["n_modes"], f2, *args[2:], weights=p["w"])
        np.testing.assert_array_equal(c.batch_clnl()[0], d)  # a refused call leaves the grid that was set
        bad = p["A"].copy()
        bad[1, 2, 0] = np.nan
        with pytest.raises(capi.FptaError, match=r"\(-22\).*ORF 1, factor entry \(2, 0\) is not finite"):
            c.batch_set_clnl(*args[:7], bad, weights=p["w"])
        with pytest.raises(ValueError, match="ORFs outside"):
            c.batch_set_clnl(*args[:7], np.zeros((9, 3, 3)), weights=p["w"])
        rank, _ = c.batch_set_clnl(None, None, None, None, None, 0, None, None)  # cleared
        assert list(rank) == [0, 0, 0]
        with pytest.raises(capi.FptaError, match="no correlated likelihood grid is set"):
            c.batch_clnl()
        c.batch_set_clnl(*args, weights=p["w"])
        c.batch_set_toas(p["offs"], p["toas"], p["nu"])  # a new layout: the grid is gone
        c.batch_add_signal(1, p["f"], np.sqrt(p["phi"]), L=np.eye(3))
        c.batch_synth(1, 0, 20, to_host=False)
        with pytest.raises(capi.FptaError, match="no correlated likelihood grid is set"):
            c.batch_clnl()
    finally:
        c.close()


def test_the_budget_cap_names_the_bytes(ctx):
    """64 pulsars with K = 256 are n = 16384; 17 grid points of it are 36507222016 bytes of factors, beyond 32 GiB. The
    refusal comes from the validation, before any table is built."""
    rng = np.random.default_rng(8)
    P, N, G = 64, 128, 17
    offs = (np.arange(P + 1) * 8).astype(np.int64)
    toas = np.concatenate([np.sort(rng.uniform(0.0, 3e8, 8)) for _ in range(P)])
    nu = np.full(8 * P, 1400.0)
    res = np.zeros((1, 8 * P))
    with pytest.raises(Exception, match=r"\(-22\).*the cached factors need 36507222016 bytes"):
        ctx.clnl_grid(offs, toas, nu, np.array([N], dtype=np.int32), np.arange(1, N + 1) / 3e8, np.zeros(1),
                      np.full(1, 1400.0), np.full(N, 1e-13), 0, np.full((G, N), 1e-13), np.eye(P)[None], res,
                      weights=np.full(8 * P, 1e13))


def test_a_non_psd_orf_is_refused(ctx, small):
    sim, psrs, lay = small
    bad = np.eye(8)
    bad[0, 1] = bad[1, 0] = 2.0
    with pytest.raises(ValueError, match="not positive semidefinite"):
        sim.set_correlated_likelihood(orfs=["hd", bad], phi=small_grid(lay))
    with pytest.raises(Exception, match="has its own frequency"):  # the red noise sits on per-pulsar grids
        sim.set_correlated_likelihood(target="red_noise", phi=np.ones((1, 5)) * 1e-14)


# ----------------------------------------------------------------------------- a statement of the definition
# Measured with clnl_reference on the CPU, mean of dlnL_hd - dlnL_curn over 1024 realizations / its standard error:
#   drawn HD-correlated, seeds 1 .. 5:  0.743 / 0.037, 0.759 / 0.038, 0.761 / 0.037, 0.730 / 0.038, 0.712 / 0.038
#   drawn uncorrelated,  seeds 1 .. 5: -0.775 / 0.042, -0.798 / 0.042, -0.807 / 0.041, -0.840 / 0.043, -0.860 / 0.043
# i.e. at least 18 standard errors from zero for every seed (the common process at 3 x the unbiasedness layout's
# amplitude).
@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("identity", [False, True])
def test_the_mean_hd_minus_curn_has_the_sign_of_the_injection(ctx, identity, seed):
    """Gibbs' inequality in expectation: over 1024 oracle realizations of the 6-pulsar layout the realization mean of
    dlnL_hd - dlnL_curn at the injected spectrum is > 0 with the process drawn HD-correlated and < 0 with it drawn
    uncorrelated."""
    from fakepta_amd import tm
    from oracle import fakepta_oracle as O
    lay = CH.statement_layout(identity)
    P = CH.STATEMENT_P
    res = O.batch_synth(lay["offs"], lay["toas"], lay["nu"], lay["segs"], seed, 0, CH.STATEMENT_R, sigma=lay["sigma"])
    M, ncol = tm.stack_design(lay["Mmats"])
    f = np.concatenate([lay["f_rn"], np.tile(lay["f_gw"], (P, 1))], axis=1)
    phi = np.concatenate([lay["amp_rn"] ** 2, np.tile(lay["amp_gw"] ** 2, (P, 1))], axis=1)
    A = np.stack([np.linalg.cholesky(lay["hd"]), np.eye(P)])
    d = ctx.clnl_grid(lay["offs"], lay["toas"], lay["nu"], [5, 5], f, [0.0, 0.0], [1400.0, 1400.0], phi, 1,
                      (lay["amp_gw"] ** 2)[None], A, res, M=M, ncol_psr=ncol, weights=1 / lay["sigma"] ** 2)[0]
    diff = d[0, 0] - d[1, 0]
    mean, se = float(np.mean(diff)), float(np.std(diff) / np.sqrt(len(diff)))
    print(f"identity {identity} seed {seed}: mean dlnL_hd - dlnL_curn = {mean:.4f} +- {se:.4f}")
    assert d.shape == (2, 1, CH.STATEMENT_R) and ((mean < 0) if identity else (mean > 0))


# ----------------------------------------------------------------------------- drop-in
def test_drop_in_equals_the_batch_call(ctx):
    """correlated_likelihood_array on psr.residuals equals BatchSimulator.correlated_likelihood on a block of one
    realization holding the same residuals."""
    from fakepta import correlated_noises as cn
    from fakepta import fake_pta as fp
    from fakepta_amd.batch import BatchSimulator
    np.random.seed(12)
    psrs = fp.make_fake_array(npsrs=4, Tobs=10, ntoas=90, gaps=True, toaerr=1e-7, pdist=1.0,
                              freqs=[800, 1400, 2500], backends=["A", "B"],
                              custom_model={"RN": 10, "DM": 10, "Sv": None})
    cn.add_common_correlated_noise(psrs, orf="hd", spectrum="powerlaw", name="gw", components=6, log10_A=-13.5,
                                   gamma=13 / 3)
    A, gam = np.array([-14.0, -13.5, -13.0]), np.array([3.0, 13 / 3])
    sim = BatchSimulator(psrs, ctx=ctx)
    block = sim.synth(1, seed=3)
    offs = sim.offs
    for i, p in enumerate(psrs):
        p.residuals = block[0, offs[i]:offs[i + 1]].copy()
    keep = [p.residuals.copy() for p in psrs]
    out = fp.correlated_likelihood_array(psrs, orfs=("hd", "curn", "monopole"), log10_A=A, gamma=gam, posterior=True)
    for p, k in zip(psrs, keep):
        np.testing.assert_array_equal(p.residuals, k)
    sim.set_correlated_likelihood(orfs=("hd", "curn", "monopole"), log10_A=A, gamma=gam)
    ref = sim.correlated_likelihood(posterior=True)
    assert out["dlnL"].shape == (3, 3, 2, 1) and np.all(np.isfinite(out["dlnL"])) and out["orfs"] == ref["orfs"]
    for k in ("dlnL", "lnB", "lnB_vs_curn", "posterior", "ld", "log10_A_ml", "gamma_ml"):
        np.testing.assert_array_equal(out[k], ref[k])
    assert np.any(out["lnB_vs_curn"][0] != 0) and np.all(out["lnB_vs_curn"][1] == 0)
