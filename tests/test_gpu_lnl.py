"""Likelihood grid on the device (fpta_lnl_grid, fpta_batch_set_lnl, fpta_batch_lnl: k_fit_apply on its third operator
slot, k_lnl_quad, k_lnl_reduce) and the Python surface above it, against the np.longdouble definition of
tests/lnl_reference.py.

X0 = B0_p r, per pulsar and row: |got - truth| <= max(4 e_lit, (n_p + 2) eps sum_t |B_kt| |r_t|), DESIGN.md section 5i's
rule. Stage 2 is held to the definition applied to the device's own X and the plan's own fp64 U, with the derived
allowance of lnl_reference.quad / dlnl; exact zeros and bit identities are compared exactly.

The cases of tests/launch_axes.py take k_lnl_quad past its first workgroup on every launch axis (three realization
tiles, three grid chunks, the K = 128 and K = 130 instances at their edge) under the same checkers: stage 2, the bit
identities of realizations and grid rows at the tile and chunk edges, and a batch block of 130 realizations on a 9 x 8
grid."""
import numpy as np
import pytest

from tests import launch_axes as AX
from tests import lnl_reference as LR
from tests import os_reference as OS
from tests import tm_reference as T
from tests import test_gpu_os as GO
from tests import test_lnl_host as LH
from tests import test_os_host as H

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
LD = np.longdouble


@pytest.fixture(scope="module")
def capi():
    from fakepta_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def ctx(capi):
    c = capi.Context(0)
    yield c
    c.close()


# ----------------------------------------------------------------------------- stage 1: X0 against the truth
_BASE = {}


def base_case(name):
    """test_gpu_os's ragged array (0, 1, 5, 16, 17, 33, 250 and 600 TOAs; 0, 3 and 16 design columns) with the truth
    and the literal form of the base operator (the target left out of the model), made once."""
    if name not in _BASE:
        c = GO.case(name)
        offs, n_modes = c["offs"], c["n_modes"]
        edges = np.concatenate([[0], np.cumsum(n_modes)])
        tgt = c["target"]
        Bs, lits = [], []
        for p in range(len(offs) - 1):
            sl = slice(int(offs[p]), int(offs[p + 1]))
            comps = [(c["f"][p, edges[i]:edges[i + 1]], c["idx"][i], c["freqf"][i]) for i in range(len(n_modes))]
            phis = [np.zeros(n_modes[i]) if i == tgt else c["phi"][p, edges[i]:edges[i + 1]] for i in range(len(n_modes))]
            B, _, norms, keep = OS.operator_ld(c["toas"][sl], c["nu"][sl], c["mats"][p], c["w"][sl], comps, phis, tgt,
                                               need_z=False)
            T.assert_clear_rank(norms, keep, c["mats"][p])
            Bs.append(B)
            lits.append(OS.operator_literal(c["toas"][sl], c["nu"][sl], c["mats"][p], c["w"][sl], comps, phis, tgt, keep)
                        if GO.N_PSR[p] else np.zeros(B.shape))
        truth, bound = OS.x_truth(Bs, offs, c["res"])
        literal = np.stack([lits[p] @ c["res"][:, int(offs[p]):int(offs[p + 1])].T for p in range(len(offs) - 1)])
        grid = np.stack([c["phi_hat"], np.zeros_like(c["phi_hat"])])
        _BASE[name] = dict(c, truth=truth, bound=bound, literal=literal, grid=grid)
    return _BASE[name]


def one_shot(ctx, c, res, grid=None, factors=False):
    return ctx.lnl_grid(c["offs"], c["toas"], c["nu"], c["n_modes"], c["f"], c["idx"], c["freqf"], c["phi"],
                        c["target"], c["grid"] if grid is None else grid, res, M=c["M"], ncol_psr=c["ncol"],
                        weights=c["w"], factors=factors)


def check_stage2(label, d, q, X, ld, U, n_psr):
    """dlnL and q against the definition applied to X and U in longdouble, within the derived allowance; the per-pulsar
    terms summed in pulsar order are dlnL bit for bit; a pulsar without TOAs has q = 0 and ld = 0. Returns the largest
    error / allowance."""
    P, G, R = q.shape
    dt, qt, db, qb = LR.dlnl(list(U), list(ld), list(X))
    eq, ed = np.abs(q.astype(LD) - qt).astype(np.float64), np.abs(d.astype(LD) - dt).astype(np.float64)
    worst = max(float(np.max(eq / np.maximum(qb, 1e-300))), float(np.max(ed / np.maximum(db, 1e-300))))
    print(f"{label}: largest stage-2 error / allowance {worst:.4f}")
    assert np.all(eq <= qb) and np.all(ed <= db), (label, worst)
    acc = np.zeros((G, R))
    for p in range(P):
        acc = acc + 0.5 * (q[p] - ld[p][:, None])
    np.testing.assert_array_equal(acc, d)
    for p in range(P):
        if n_psr[p] == 0:
            assert np.all(q[p] == 0.0) and np.all(ld[p] == 0.0) and np.all(X[p] == 0.0)
    return worst


@pytest.mark.parametrize("n_vec", [1, 16, 33])
@pytest.mark.parametrize("name", ["k2", "k16", "k18", "k60"])
def test_one_shot_x_matches_the_truth(ctx, name, n_vec):
    c = base_case(name)
    d, q, X, rank, ld, U = one_shot(ctx, c, c["res"][:n_vec], factors=True)
    P = len(GO.N_PSR)
    assert X.shape == (P, c["K"], n_vec) and d.shape == (2, n_vec) and q.shape == (P, 2, n_vec) and ld.shape == (P, 2)
    GO.check_x(f"{name} n_vec {n_vec}", X, c["truth"][:, :, :n_vec], c["literal"][:, :, :n_vec],
               c["bound"][:, :, :n_vec], GO.N_PSR)
    check_stage2(f"{name} n_vec {n_vec}", d, q, X, ld, U, GO.N_PSR)
    assert np.all(d[1] == 0.0) and np.all(q[:, 1] == 0.0) and np.all(ld[:, 1] == 0.0)  # the zero grid row


# ----------------------------------------------------------------------------- stage 2: k_lnl_quad, k_lnl_reduce
_QUAD = {}


def quad_case(P, N, G, seed, empty):
    """P pulsars of 20 .. 30 TOAs (the second one without TOAs when `empty`) under white noise and one process of N
    modes, and a random grid [G, N] within a factor 10 of the process's level with a third of its modes zero and, for
    G >= 3, an all-zero row: the cheapest inputs that give k_lnl_quad a full X."""
    key = (P, N, G, seed, empty)
    if key not in _QUAD:
        rng = np.random.default_rng(seed)
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
        _QUAD[key] = dict(offs=offs, toas=toas, nu=nu, n_modes=np.array([N], dtype=np.int32),
                          f=np.arange(1, N + 1) / 3e8, idx=np.zeros(1), freqf=np.full(1, 1400.0), phi=phi, target=0,
                          grid=grid, M=None, ncol=None, w=np.full(int(offs[-1]), 1e13), counts=counts)
    return _QUAD[key]


# K = 2 (one partial row group, half a block of 8 columns), 16, 18 (the second row group's diagonal block), 60, 62
# (K % 4 = 2), 256 (16 row groups, the instance of 32 realizations); G = 1, 3, 17; R = 1, 16, 17, 33; P = 1, 2, 17
@pytest.mark.parametrize("P,N,G,R,empty", [(1, 1, 1, 1, False), (2, 8, 3, 16, True), (17, 9, 17, 17, True),
                                           (2, 30, 3, 33, False), (2, 31, 1, 17, True), (2, 128, 3, 33, False),
                                           (17, 1, 3, 33, True), (1, 30, 17, 1, False), (2, 128, 1, 1, False)]
                         + AX.LNL_STAGE2)  # past one workgroup on the realization and the grid axis: launch_axes.py
def test_stage_2_is_the_definition_applied_to_the_device_x(ctx, P, N, G, R, empty):
    c = quad_case(P, N, G, 1000 * P + 10 * N + G, empty)
    rng = np.random.default_rng(R)
    res = rng.normal(0.0, 1e-6, (R, int(c["offs"][-1])))
    d, q, X, _, ld, U = one_shot(ctx, c, res, factors=True)
    assert d.shape == (G, R) and q.shape == (P, G, R) and X.shape == (P, 2 * N, R) and U.shape == (P, G, 2 * N, 2 * N)
    assert np.any(q != 0) and np.all(np.isfinite(d))
    check_stage2(f"P {P} K {2 * N} G {G} R {R}", d, q, X, ld, U, c["counts"])
    if G >= 3:
        assert np.all(d[1] == 0.0) and np.all(q[:, 1] == 0.0)  # the all-zero row: exactly 0 for every realization


@pytest.mark.parametrize("N", [9, 30, 128])
def test_blocks_order_and_grid_size_do_not_change_a_bit(ctx, N):
    """A realization's column is the same bits alone, among the first 16, among all 33 and in reversed order; a grid
    point's row is the same alone and inside G = 17."""
    c = quad_case(2, N, 17, 5 + N, False)
    res = np.random.default_rng(3).normal(0.0, 1e-6, (33, int(c["offs"][-1])))
    d, q, X, _, ld, _ = one_shot(ctx, c, res)
    for sel in ([0], [32], list(range(16)), list(range(32, -1, -1)), [5, 31, 6]):
        d1, q1, x1, _, _, _ = one_shot(ctx, c, np.ascontiguousarray(res[sel]))
        np.testing.assert_array_equal(x1, X[:, :, sel])
        np.testing.assert_array_equal(q1, q[:, :, sel])
        np.testing.assert_array_equal(d1, d[:, sel])
    for g in (0, 7, 16):
        d1, q1, _, _, ld1, _ = one_shot(ctx, c, res, grid=c["grid"][g:g + 1])
        np.testing.assert_array_equal(d1[0], d[g])
        np.testing.assert_array_equal(q1[:, 0], q[:, g])
        np.testing.assert_array_equal(ld1[:, 0], ld[:, g])


def test_tiles_and_chunks_past_the_first_do_not_change_a_bit(ctx):
    """N = 9, G = 70, R = 130 (three realization tiles, three grid chunks): the realizations at the tiles' edges are
    the same bits alone (tile 0 of a block of one) as inside the block, the grid rows at the chunks' edges the same
    alone (chunk 0, wave 0) as inside the grid."""
    b = AX.LNL_BITWISE
    c = quad_case(2, b["N"], b["G"], 5 + b["N"], False)
    res = np.random.default_rng(3).normal(0.0, 1e-6, (b["R"], int(c["offs"][-1])))
    d, q, X, _, ld, _ = one_shot(ctx, c, res)
    assert d.shape == (b["G"], b["R"]) and np.all(np.isfinite(d)) and np.all(q[:, [0, b["G"] - 1]] > 0)
    for r in b["reals"]:
        d1, q1, x1, _, _, _ = one_shot(ctx, c, np.ascontiguousarray(res[[r]]))
        np.testing.assert_array_equal(x1, X[:, :, [r]], err_msg=f"realization {r}")
        np.testing.assert_array_equal(q1, q[:, :, [r]], err_msg=f"realization {r}")
        np.testing.assert_array_equal(d1, d[:, [r]], err_msg=f"realization {r}")
    for g in b["rows"]:
        d1, q1, _, _, ld1, _ = one_shot(ctx, c, res, grid=c["grid"][g:g + 1])
        np.testing.assert_array_equal(d1[0], d[g], err_msg=f"grid row {g}")
        np.testing.assert_array_equal(q1[:, 0], q[:, g], err_msg=f"grid row {g}")
        np.testing.assert_array_equal(ld1[:, 0], ld[:, g], err_msg=f"grid row {g}")


# ----------------------------------------------------------------------------- batch path
@pytest.fixture(scope="module")
def small(ctx):
    """The unbiasedness layout of tests/test_os_host.py as a BatchSimulator, the common process drawn uncorrelated."""
    from fakepta_amd.batch import BatchSimulator
    lay = H.unbiased_layout(identity=True)
    o = lay["offs"]
    psrs = [GO._Psr(lay["toas"][o[i]:o[i + 1]], lay["nu"][o[i]:o[i + 1]], lay["sigma"][o[i]:o[i + 1]] ** 2,
                    lay["pos"][i], lay["Mmats"][i]) for i in range(len(o) - 1)]
    sim = BatchSimulator(psrs, signals=[], white=True, ctx=ctx)
    sim.add_signal("red_noise", 0, lay["f_rn"], lay["amp_rn"])
    sim.add_signal("gw_common", 1, lay["f_gw"], lay["amp_gw"], L=lay["L"])
    sim.set_timing_model()
    return sim, psrs, lay


_SMALL_TRUTH = {}


def composed(lay, block, grid):
    """(dlnL truth [G, R] as fp64, the bound a device result is held to): X within its tolerance (the truth's B0 and the
    literal form), U and ld within the host test's measured bounds, then lnl_reference's stage-2 allowance on top of
    the errors y = U X inherits: e_i = sum_k (|U_ik| dX_k + dU_i (|X_k| + dX_k)) + (K + 2) eps sum_k |U_ik| |X_k|."""
    offs = lay["offs"]
    P = len(offs) - 1
    if "base" not in _SMALL_TRUTH:
        base = []
        for p in range(P):
            sl = slice(int(offs[p]), int(offs[p + 1]))
            args = (lay["toas"][sl], lay["nu"][sl], lay["Mmats"][p], 1 / lay["sigma"][sl] ** 2, lay["comps_of"](p))
            B, Z, norms, keep = LR.base_operator(*args, lay["phis_of"](p), 1)
            phis0 = [lay["phis_of"](p)[0], np.zeros(len(lay["f_gw"]))]
            base.append((B, OS.operator_literal(*args, phis0, 1, keep), Z))
        _SMALL_TRUTH["base"] = base
    key = np.asarray(grid, dtype=np.float64).tobytes()  # the factors are a grid's own: one entry per grid
    if key not in _SMALL_TRUTH:
        _SMALL_TRUTH[key] = [(B, lit) + LR.grid_truth(Z, grid)[:2] for B, lit, Z in _SMALL_TRUTH["base"]]
    per = _SMALL_TRUTH[key]
    Xt, xb = OS.x_truth([q[0] for q in per], offs, block)
    lit = np.stack([per[p][1] @ block[:, offs[p]:offs[p + 1]].T for p in range(P)])
    dX = OS.x_tolerance(Xt, lit, xb)[0]
    G, R, K = len(grid), block.shape[0], Xt.shape[1]
    d, bound, mag = np.zeros((G, R), dtype=LD), np.zeros((G, R)), np.zeros((G, R))
    for p in range(P):
        aX = np.abs(Xt[p]).astype(np.float64)
        for g in range(G):
            U, ld = per[p][2][g], per[p][3][g]
            aU = np.abs(U).astype(np.float64)
            dU = LH.U_BOUND_EPS * EPS * np.max(aU, axis=1, keepdims=True)
            y = (U @ Xt[p])
            e = aU @ dX[p] + dU * np.sum(aX + dX[p], axis=0, keepdims=True) + (K + 2) * EPS * (aU @ aX)
            q = np.sum(y * y, axis=0)
            ay = np.abs(y).astype(np.float64)
            dq = np.sum(2 * ay * e + e * e, axis=0) + (K + 3) * EPS * q.astype(np.float64)
            dld = LH.LD_BOUND_EPS * EPS * max(1.0, abs(float(ld)))
            d[g] = d[g] + (q - ld) / 2
            bound[g] += (dq + dld) / 2
            mag[g] += (np.abs(q).astype(np.float64) + abs(float(ld))) / 2
    return d.astype(np.float64), bound + (P + 3) * EPS * mag + EPS * np.abs(d).astype(np.float64)


def test_batch_grid_end_to_end_and_after_project(ctx, small):
    sim, psrs, lay = small
    A = -13.6 + 0.15 * np.arange(-1, 2)
    gam = 13 / 3 + 1.0 * np.arange(-1, 2)
    rank = sim.set_likelihood_grid(log10_A=A, gamma=gam)
    assert list(rank) == [3] * 8
    grid = sim._lnl["phi"]
    assert grid.shape == (9, 5) and ctx.batch_lnl_info() == dict(K=10, N=5, G=9, n_real=0)
    R = 48
    sim.synth(R, seed=5, to_host=False)
    before = sim.checksums()
    out = sim.likelihood_grid(per_pulsar=True, posterior=True)
    np.testing.assert_array_equal(sim.checksums(), before)  # the block is untouched
    assert ctx.batch_lnl_info()["n_real"] == R
    assert out["dlnL"].shape == (3, 3, R) and out["lnB"].shape == (R,) and out["dlnL_psr"].shape == (8, 9, R)
    assert out["posterior"].shape == (3, 3, R) and np.allclose(out["posterior"].sum(axis=(0, 1)), 1.0)
    flat = out["dlnL"].reshape(9, R)
    np.testing.assert_array_equal(np.ravel_multi_index(out["argmax"], (3, 3)), np.argmax(flat, axis=0))
    acc = np.zeros((9, R))
    for p in range(8):
        acc = acc + out["dlnL_psr"][p]
    np.testing.assert_array_equal(acc, flat)
    block = ctx.batch_download(0, R)
    want, bound = composed(lay, block, grid)
    err = np.abs(flat - want)
    print(f"end to end: largest error / composed bound {float(np.max(err / bound)):.3e}; mean dlnL at the injected "
          f"point {flat[4].mean():.2f}, lnB mean {out['lnB'].mean():.2f}")
    assert np.all(err <= bound)
    # the timing model is marginalised: projecting the block first changes dlnL by rounding only
    sim.project()
    flat_p = sim.likelihood_grid()["dlnL"].reshape(9, R)
    want_p, bound_p = composed(lay, ctx.batch_download(0, R), grid)
    assert np.all(np.abs(flat_p - want_p) <= bound_p)
    assert np.all(np.abs(want_p - want) <= bound)  # the definition does not see the projection
    assert np.all(np.abs(flat_p - flat) <= bound_p + bound)


def test_batch_grid_second_block_past_one_tile_and_one_chunk(ctx, small):
    """A second block of 130 realizations on a 9 x 8 (log10_A, gamma) grid: three realization tiles and three grid
    chunks of k_lnl_quad<4> on the batch path, against the composed truth; the [nA, ngamma, R] result and its argmax
    are the flat [G, R] result, amplitude slowest."""
    from fakepta_amd import lnl
    sim, psrs, lay = small
    b = AX.LNL_BATCH
    nA, ng, R = b["nA"], b["ngamma"], b["R"]
    A = -13.6 + 0.1 * (np.arange(nA) - nA // 2)
    gam = 13 / 3 + 0.5 * (np.arange(ng) - ng // 2)
    rank = sim.set_likelihood_grid(log10_A=A, gamma=gam)
    grid = sim._lnl["phi"]
    assert list(rank) == [3] * 8 and grid.shape == (nA * ng, 5)
    assert ctx.batch_lnl_info() == dict(K=b["K"], N=5, G=nA * ng, n_real=0)
    for i, j in ((0, 0), (3, 7), (8, 0), (8, 7)):  # row i ngamma + j is the point (A_i, gamma_j)
        np.testing.assert_array_equal(grid[i * ng + j], lnl.powerlaw_grid(lay["f_gw"], A[i:i + 1], gam[j:j + 1])[0])
    sim.synth(R, seed=6, real0=48, to_host=False)
    before = sim.checksums()
    out = sim.likelihood_grid(per_pulsar=True)
    np.testing.assert_array_equal(sim.checksums(), before)
    assert ctx.batch_lnl_info()["n_real"] == R
    assert out["dlnL"].shape == (nA, ng, R) and out["dlnL_psr"].shape == (8, nA * ng, R)
    flat, _, _ = ctx.batch_lnl()  # the device's [G, R], as it stands
    assert flat.shape == (nA * ng, R)
    for i in range(nA):
        for j in range(ng):
            np.testing.assert_array_equal(out["dlnL"][i, j], flat[i * ng + j])
    np.testing.assert_array_equal(np.ravel_multi_index(out["argmax"], (nA, ng)), np.argmax(flat, axis=0))
    np.testing.assert_array_equal(out["log10_A_ml"], A[np.argmax(flat, axis=0) // ng])
    np.testing.assert_array_equal(out["gamma_ml"], gam[np.argmax(flat, axis=0) % ng])
    acc = np.zeros((nA * ng, R))
    for p in range(8):
        acc = acc + out["dlnL_psr"][p]
    np.testing.assert_array_equal(acc, flat)
    want, bound = composed(lay, ctx.batch_download(0, R), grid)
    err = np.abs(flat - want)
    print(f"second block, R {R} G {nA * ng}: largest error / composed bound {float(np.max(err / bound)):.3e}")
    assert np.all(err <= bound)


def test_fit_statistic_and_grid_set_together_give_their_own_results(ctx, small):
    sim, psrs, lay = small
    grid = np.stack([lay["amp_gw"] ** 2, 3.0 * lay["amp_gw"] ** 2])
    sim.ctx.batch_set_fit(None, None, None, None)
    sim.ctx.batch_set_os(None, None, None, None, None, 0, None, None)
    sim.set_likelihood_grid(phi=grid)
    sim.synth(20, seed=9, to_host=False)
    d0, q0, X0 = ctx.batch_lnl(per_pulsar=True, coefficients=True)
    sim.ctx.batch_set_lnl(None, None, None, None, None, 0, None)
    sim.set_optimal_statistic()
    Q0, _, XO0 = ctx.batch_os(coefficients=True)
    sim.ctx.batch_set_os(None, None, None, None, None, 0, None, None)
    sim.set_fourier_fit([(4, 0.0), (3, 2.0)])
    coef0 = sim.fourier_fit()
    sim.set_optimal_statistic()
    sim.set_likelihood_grid(phi=grid)
    for _ in range(2):  # all three set, in turn, twice
        np.testing.assert_array_equal(sim.fourier_fit(), coef0)
        d1, q1, X1 = ctx.batch_lnl(per_pulsar=True, coefficients=True)
        Q1, _, XO1 = ctx.batch_os(coefficients=True)
        for a, b in ((d1, d0), (q1, q0), (X1, X0), (Q1, Q0), (XO1, XO0)):
            np.testing.assert_array_equal(a, b)
    assert d0.shape == (2, 20) and X0.shape == (8, 10, 20) and np.any(d0 != 0) and np.any(X0 != XO0)
    sim.ctx.batch_set_lnl(None, None, None, None, None, 0, None)  # clearing one leaves the others
    np.testing.assert_array_equal(ctx.batch_os()[0], Q0)
    np.testing.assert_array_equal(sim.fourier_fit(), coef0)
    sim.ctx.batch_set_fit(None, None, None, None)
    sim.ctx.batch_set_os(None, None, None, None, None, 0, None, None)


@pytest.fixture(scope="module")
def shared_span(capi):
    """test_gpu_os's shared-span layout (C2's signal mix on 64 ragged pulsars, pipelined k_grid_fused blocks that also
    make the next block's common-signal mix) with a likelihood grid of 3 points on the common process."""
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
    grid = np.stack([ac ** 2, np.zeros(30), 4.0 * ac ** 2])
    rank, ld = c.batch_set_lnl([30, 100, 30], np.concatenate(fs + [np.tile(fc, (P, 1))], axis=1), [0.0, 2.0, 0.0],
                               [1400.0] * 3, np.concatenate(phis + [np.tile(ac ** 2, (P, 1))], axis=1), 2, grid,
                               weights=np.full(int(offs[-1]), 1e13))
    assert list(rank) == [0] * P and np.all(ld[:, [0, 2]] > 0) and np.all(ld[:, 1] == 0)
    yield c
    c.close()


@pytest.mark.parametrize("next_real0,hit", [(384, True), (1000, False)])
def test_grid_leaves_the_block_and_the_next_block_alone(shared_span, next_real0, hit):
    """The block is bit for bit what it was, and the block after one whose grid was taken is bit for bit the block
    after an untouched one, for a next-mix hit and for a miss."""
    c = shared_span
    outs = []
    for stat in (False, True):
        for real0 in (0, 128, 256):  # hits start at the third block of a pipelined run
            c.batch_synth(7, real0, 128, to_host=False)
        assert c.batch_grid_info()["interp_kernel"].startswith("k_grid_fused<")
        if stat:
            sums, pre = c.batch_checksums(), c.batch_download(0, 128)
            d, _, _ = c.batch_lnl()
            assert d.shape == (3, 128) and np.all(np.isfinite(d)) and np.any(d[0] != 0) and np.all(d[1] == 0.0)
            np.testing.assert_array_equal(c.batch_download(0, 128), pre)
            np.testing.assert_array_equal(c.batch_checksums(), sums)
        outs.append(c.batch_synth(7, next_real0, 128))
        assert c.batch_grid_info()["next_mix_used"] == hit
    np.testing.assert_array_equal(outs[1], outs[0])


# ----------------------------------------------------------------------------- state
def test_state_errors_and_set_toas_clears_the_grid(capi):
    c = capi.Context(0)
    try:
        p = quad_case(3, 2, 3, 3, False)
        args = (p["n_modes"], p["f"], p["idx"], p["freqf"], p["phi"], 0, p["grid"])
        with pytest.raises(capi.FptaError, match="set_toas first"):
            c.batch_set_lnl(None, None, None, None, None, 0, None)
        c.batch_set_toas(p["offs"], p["toas"], p["nu"])
        c.batch_add_signal(1, p["f"], np.sqrt(p["phi"]), L=np.eye(3))
        with pytest.raises(capi.FptaError, match=r"\(-77\).*nothing synthesized"):
            c.batch_lnl()
        c.batch_synth(1, 0, 20, to_host=False)
        with pytest.raises(capi.FptaError, match=r"\(-77\).*no likelihood grid is set"):
            c.batch_lnl()
        rank, ld = c.batch_set_lnl(*args, weights=p["w"])
        assert list(rank) == [0, 0, 0] and ld.shape == (3, 3)
        assert c.batch_lnl_info() == dict(K=4, N=2, G=3, n_real=0)
        d, q, X = c.batch_lnl(per_pulsar=True, coefficients=True)
        assert d.shape == (3, 20) and q.shape == (3, 3, 20) and X.shape == (3, 4, 20)
        assert c.batch_lnl_info()["n_real"] == 20
        bad = p["grid"].copy()
        bad[2, 1] = -1.0
        for grid, msg in ((bad, r"\(-22\).*grid row 2, mode 1: prior variance"),
                          (np.where(bad < 0, np.nan, bad), r"\(-22\).*grid row 2, mode 1: prior variance")):
            with pytest.raises(capi.FptaError, match=msg):
                c.batch_set_lnl(*args[:6], grid, weights=p["w"])
            np.testing.assert_array_equal(c.batch_lnl()[0], d)  # a refused call leaves the grid that was set
        with pytest.raises(ValueError, match="grid points outside"):
            c.batch_set_lnl(*args[:6], np.ones((4097, 2)), weights=p["w"])
        rank, _ = c.batch_set_lnl(None, None, None, None, None, 0, None)  # cleared
        assert list(rank) == [0, 0, 0]
        with pytest.raises(capi.FptaError, match="no likelihood grid is set"):
            c.batch_lnl()
        c.batch_set_lnl(*args, weights=p["w"])
        c.batch_set_toas(p["offs"], p["toas"], p["nu"])  # a new layout: the grid is gone
        c.batch_add_signal(1, p["f"], np.sqrt(p["phi"]), L=np.eye(3))
        c.batch_synth(1, 0, 20, to_host=False)
        with pytest.raises(capi.FptaError, match="no likelihood grid is set"):
            c.batch_lnl()
        c.set_option(capi.OPT_PROFILE, 1)  # one FPTA_K_DENSE entry per call, every stage
        c.batch_set_lnl(*args, weights=p["w"])
        c.reset_stats()
        c.batch_lnl()
        c.synchronize()
        assert c.kernel_stats(capi.K_DENSE)[0] == 1
    finally:
        c.close()


# ----------------------------------------------------------------------------- drop-in
def test_drop_in_equals_the_one_shot_call(ctx):
    from fakepta import correlated_noises as cn
    from fakepta import fake_pta as fp
    from fakepta_amd import lnl, os as osm, tm
    np.random.seed(12)
    psrs = fp.make_fake_array(npsrs=4, Tobs=10, ntoas=90, gaps=True, toaerr=1e-7, pdist=1.0,
                              freqs=[800, 1400, 2500], backends=["A", "B"],
                              custom_model={"RN": 10, "DM": 10, "Sv": None})
    cn.add_common_correlated_noise(psrs, orf="hd", spectrum="powerlaw", name="gw", components=6, log10_A=-13.5,
                                   gamma=13 / 3)
    keep = [p.residuals.copy() for p in psrs]
    A, gam = np.array([-14.0, -13.5, -13.0]), np.array([3.0, 13 / 3])
    out = fp.likelihood_grid_array(psrs, log10_A=A, gamma=gam, per_pulsar=True)
    for p, k in zip(psrs, keep):
        np.testing.assert_array_equal(p.residuals, k)
    segs = osm.segments_of(psrs)
    assert [s["name"] for s in segs] == ["red_noise", "dm_gp", "gw_common"]
    model = osm.noise_model(segs, 4)
    grid = lnl.powerlaw_grid(lnl.target_frequencies(model, 2), A, gam)
    offs = np.concatenate([[0], np.cumsum([len(p.toas) for p in psrs])]).astype(np.int64)
    M, ncol = tm.stack_design([p.Mmat for p in psrs])
    d, q, X, rank, ld, _ = ctx.lnl_grid(
        offs, np.concatenate([p.toas for p in psrs]), np.concatenate([p.freqs for p in psrs]), model["n_modes"],
        model["f"], model["idx"], model["freqf"], model["phi"], 2, grid, np.concatenate([p.residuals for p in psrs]),
        M=M, ncol_psr=ncol, weights=np.concatenate([1 / p._white_sigma2() for p in psrs]))
    assert out["dlnL"].shape == (3, 2, 1) and np.all(np.isfinite(d))
    np.testing.assert_array_equal(out["dlnL"].reshape(6, 1), d)
    np.testing.assert_array_equal(out["q_psr"], q)
    np.testing.assert_array_equal(out["dlnL_psr"], 0.5 * (q - ld[:, :, None]))
    np.testing.assert_array_equal(out["lnB"], lnl.log_bayes(d))
    np.testing.assert_array_equal(np.ravel_multi_index(out["argmax"], (3, 2)), np.argmax(d, axis=0))
