"""The timing-model projection on the GPU (k_tm_project behind fpta_tm_project, fpta_batch_set_timing_model and
fpta_batch_project) and the Python surface above it, against the np.longdouble definition of tests/tm_reference.py.

Tolerance of every comparison with the truth, per pulsar: max |got - truth| <= max(4 e_lit, 64 eps max|r_in|), e_lit
the error of the literal fp64 numpy evaluation of the same definition (column-scaled lstsq with the same rcond) and
the scale the peak of the input (the output of a short pulsar is about 0). Every truth asserts on its own inputs that
each kept column's orthogonalised norm is >= 1e-4 and each dropped one's <= 1e-13 (tm_reference.assert_clear_rank),
so the rank decision is never what a test measures. Each test prints the measured ratios."""
import numpy as np
import pytest

from tests import ld_reference as LDR
from tests import tm_reference as T
from tests.helpers import common_signal, per_psr_signal, random_layout

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
LD = np.longdouble
YEAR = 365.25 * 86400.0
N_PSR = (1, 3, 15, 16, 17, 33, 250)  # ragged: most rows start at odd offsets
# the kernel's 16 waves take a pulsar's 16-TOA chunks in turn: from 272 TOAs on a wave has more than one chunk. 600 (37
# chunks and a tail of 8, at an odd offset), 309 (19 and 5), 2000 (125, no tail: the C2 pulsar) and 545 (34 and 1) give
# every wave two to eight chunks, with the tail's wave holding whole chunks too (600, 545) or a single one (309)
N_LONG = (3, 600, 309, 2000, 545)
N_VEC = 49
# columns per pulsar; "s" marks the single-frequency pulsar (8 columns, rank 5). Ranks: n_p < m gives n_p.
CONFIGS = {
    "unit": dict(seed=77, n=N_PSR, m=(8, 8, 16, 0, 1, "s", 16), rank=(1, 3, 15, 0, 1, 5, 16), weighted=False),
    "weighted": dict(seed=78, n=N_PSR, m=(1, 0, 8, 16, "s", 16, 8), rank=(1, 0, 8, 16, 5, 16, 8), weighted=True),
    "long": dict(seed=79, n=N_LONG, m=(8, 8, 16, 8, "s"), rank=(3, 8, 16, 8, 5), weighted=True),
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
    """(offs, Mmats, stacked M, ncol, weights, res [49, n_toa], truth, literal, ranks) of a configuration, made once
    and never changed."""
    if name not in _CASES:
        cfg = CONFIGS[name]
        rng = np.random.default_rng(cfg["seed"])
        offs = np.concatenate([[0], np.cumsum(cfg["n"])]).astype(np.int64)
        mats = []
        for n, m in zip(cfg["n"], cfg["m"]):
            t = np.sort(rng.uniform(0.0, 15 * YEAR, n))
            nu = np.full(n, 1400.0) if m == "s" else T.three_band(rng, n)
            full = np.concatenate([T.mmat(t, nu), T.smooth_columns(rng, t, 8)], axis=1)
            mats.append(full[:, :8 if m == "s" else m].copy())
        from fakepta_amd import tm
        M, ncol = tm.stack_design(mats)
        w = 1 / rng.uniform(1e-7, 1e-6, int(offs[-1])) ** 2 if cfg["weighted"] else None
        res = rng.normal(0.0, 1e-6, (N_VEC, int(offs[-1])))
        for p, A in enumerate(mats):  # plus something the model absorbs, of the same size
            if A.shape[1]:
                a = rng.normal(0.0, 1e-6, (N_VEC, A.shape[1])) / np.max(np.abs(A), axis=0)
                res[:, offs[p]:offs[p + 1]] += a @ A.T
        truth, ranks = T.project_truth(offs, mats, w, res)
        assert tuple(ranks) == cfg["rank"], ranks
        literal = T.project_literal(offs, mats, w, res)
        for a in (M, ncol, res, truth, literal):
            a.flags.writeable = False
        _CASES[name] = (offs, mats, M, ncol, w, res, truth, literal, ranks)
    return _CASES[name]


def check_against_truth(label, offs, got, truth, literal, res_in):
    """The module's tolerance, per pulsar; prints the measured ratios and returns the largest error in eps x peak."""
    worst = 0.0
    for p in range(len(offs) - 1):
        sl = slice(int(offs[p]), int(offs[p + 1]))
        tol, e_lit, peak = T.tolerance(truth, literal, res_in, sl)
        err = float(np.max(np.abs(np.atleast_2d(got)[:, sl].astype(LD) - np.atleast_2d(truth)[:, sl]), initial=0))
        if peak == 0.0:  # an all-zero input stays all zero
            assert err == 0.0, (label, p, err)
            continue
        print(f"{label} pulsar {p} (n {offs[p + 1] - offs[p]}): error {err / (EPS * peak):.2f} eps x peak, literal "
              f"{e_lit / (EPS * peak):.2f}, error / tolerance {err / tol:.3f}")
        assert err <= tol, (label, p, err, tol)
        worst = max(worst, err / (EPS * peak))
    return worst


# ----------------------------------------------------------------------------- one-shot
@pytest.mark.parametrize("n_vec", [1, 15, 16, 17, 49])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_one_shot_matches_the_truth(ctx, name, n_vec):
    offs, mats, M, ncol, w, res, truth, literal, ranks = case(name)
    got = res[:n_vec].copy()
    rank = ctx.tm_project(offs, M, got, ncol_psr=ncol, weights=w)
    np.testing.assert_array_equal(rank, ranks)
    check_against_truth(f"{name} n_vec {n_vec}", offs, got, truth[:n_vec], literal[:n_vec], res[:n_vec])
    for p, (n, k) in enumerate(zip(np.diff(offs), ranks)):
        sl = slice(int(offs[p]), int(offs[p + 1]))
        if k == 0:  # nothing to remove: bit for bit the input
            np.testing.assert_array_equal(got[:, sl], res[:n_vec, sl])
        else:
            assert not np.array_equal(got[:, sl], res[:n_vec, sl])
        if k == n:  # the model spans everything: 0 to tolerance
            assert np.max(np.abs(got[:, sl])) <= T.tolerance(truth[:n_vec], literal[:n_vec], res[:n_vec], sl)[0]
    # a one-dimensional residual vector is one realization
    one = res[0].copy()
    ctx.tm_project(offs, M, one, ncol_psr=ncol, weights=w)
    np.testing.assert_array_equal(one, got[0])


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_annihilation_and_idempotence(ctx, name):
    offs, mats, M, ncol, w, res, truth, literal, ranks = case(name)
    rng = np.random.default_rng(5)
    r = np.zeros((16, int(offs[-1])))
    for p, A in enumerate(mats):
        if A.shape[1]:
            r[:, offs[p]:offs[p + 1]] = (rng.normal(0.0, 1e-6, (16, A.shape[1])) / np.max(np.abs(A), axis=0)) @ A.T
    t_r, _ = T.project_truth(offs, mats, w, r)
    l_r = T.project_literal(offs, mats, w, r)
    got = r.copy()
    ctx.tm_project(offs, M, got, ncol_psr=ncol, weights=w)
    check_against_truth(f"{name} r = M a", offs, got, t_r, l_r, r)
    for p, k in enumerate(ranks):  # and M a itself comes back as 0, to the same tolerance
        sl = slice(int(offs[p]), int(offs[p + 1]))
        if k:
            assert np.max(np.abs(got[:, sl])) <= T.tolerance(t_r, l_r, r, sl)[0]
    once = res[:16].copy()
    ctx.tm_project(offs, M, once, ncol_psr=ncol, weights=w)
    twice = once.copy()
    ctx.tm_project(offs, M, twice, ncol_psr=ncol, weights=w)
    for p in range(len(ranks)):
        sl = slice(int(offs[p]), int(offs[p + 1]))
        tol = T.tolerance(truth[:16], literal[:16], res[:16], sl)[0]
        d = float(np.max(np.abs(twice[:, sl] - once[:, sl]), initial=0))
        print(f"{name} pulsar {p}: second projection moves the result by {d / tol:.3f} of the tolerance")
        assert d <= tol


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_split_invariance_bit_for_bit(ctx, name):
    """A realization's result does not depend on the number of rows, its position or its neighbours."""
    offs, mats, M, ncol, w, res, truth, literal, ranks = case(name)
    whole = res.copy()
    ctx.tm_project(offs, M, whole, ncol_psr=ncol, weights=w)
    for lo, hi in ((0, 1), (1, 17), (16, 49), (48, 49)):  # groups of 1, 16 and 33 rows
        part = res[lo:hi].copy()
        ctx.tm_project(offs, M, part, ncol_psr=ncol, weights=w)
        np.testing.assert_array_equal(part, whole[lo:hi])
    back = res[::-1].copy()
    ctx.tm_project(offs, M, back, ncol_psr=ncol, weights=w)
    np.testing.assert_array_equal(back[::-1], whole)
    again = res.copy()
    ctx.tm_project(offs, M, again, ncol_psr=ncol, weights=w)
    np.testing.assert_array_equal(again, whole)


def test_one_shot_refusals_leave_the_residuals(ctx, capi):
    offs, mats, M, ncol, w, res, truth, literal, ranks = case("weighted")
    got = res[:2].copy()
    bad = np.array(M)
    bad[int(offs[6]) + 3, 5] = np.nan
    with pytest.raises(capi.FptaError, match="pulsar 6, TOA 3, column 5"):
        ctx.tm_project(offs, bad, got, ncol_psr=ncol, weights=w)
    wb = w.copy()
    wb[int(offs[2]) + 1] = 0.0
    with pytest.raises(capi.FptaError, match="pulsar 2, TOA 1: weight"):
        ctx.tm_project(offs, M, got, ncol_psr=ncol, weights=wb)
    with pytest.raises(ValueError):
        ctx.tm_project(offs, np.zeros((int(offs[-1]), 17)), got)
    with pytest.raises(ValueError):
        ctx.tm_project(offs, M, got[:, :-1].copy())
    np.testing.assert_array_equal(got, res[:2])
    # no columns at all: a successful no-op
    rank = ctx.tm_project(offs, np.zeros((int(offs[-1]), 0)), got)
    assert not rank.any()
    np.testing.assert_array_equal(got, res[:2])


# ----------------------------------------------------------------------------- batch path
class _Psr:
    """What BatchSimulator reads of a pulsar."""

    def __init__(self, toas, freqs, sigma2):
        self.toas, self.freqs, self.sigma2 = toas, freqs, sigma2
        self.Mmat = T.mmat(toas, freqs)
        self.signal_model = {}

    def _white_sigma2(self):
        return self.sigma2


P_B, N_B = 6, 567  # 35 whole chunks and a tail of 7: two or three chunks per wave of k_tm_project


@pytest.fixture(scope="module")
def batch(ctx, capi):
    """A small gridded layout: red noise and a Hellings-Downs common signal on 6 pulsars of 567 TOAs."""
    from fakepta_amd.batch import BatchSimulator
    rng = np.random.default_rng(31)
    offs, toas, nu = random_layout(rng, P_B, (40, N_B), ragged=False)
    sig2 = rng.uniform(1e-7, 1e-6, int(offs[-1])) ** 2
    psrs = [_Psr(toas[offs[i]:offs[i + 1]], nu[offs[i]:offs[i + 1]], sig2[offs[i]:offs[i + 1]]) for i in range(P_B)]
    sim = BatchSimulator(psrs, signals=[], white=False, ctx=ctx)
    f, a = per_psr_signal(rng, offs, toas, 30)
    sim.add_signal("red_noise", 0, f, a)
    f, a, L, _ = common_signal(rng, offs, toas, 20)
    sim.add_signal("gw_common", 1, f, a, L=L)
    return sim, psrs, offs, 1 / sig2


@pytest.fixture()
def gridded(ctx, capi, batch):
    ctx.set_option(capi.OPT_SYNTH_PATH, 4)
    rank = batch[0].set_timing_model()
    assert list(rank) == [8] * P_B
    return batch


def _checksum_bound(block):
    """tests/test_gpu_reductions.py: n_toa additions of the values (or their squares)."""
    return (block.shape[1] + 2) * EPS * np.stack([np.abs(block).sum(axis=1), (block * block).sum(axis=1)], axis=1)


@pytest.mark.parametrize("R,real0", [(48, 0), (33, 101)])
def test_synth_fit_is_synth_then_the_one_shot_projection(ctx, gridded, R, real0):
    sim, psrs, offs, w = gridded
    pre = sim.synth(R, seed=4, real0=real0)
    assert ctx.batch_grid_info()["last_path"] == 4
    post = sim.synth(R, seed=4, real0=real0, fit=True)
    assert post.shape == pre.shape and not np.array_equal(post, pre)
    np.testing.assert_array_equal(ctx.batch_download(0, R), post)  # the resident block is the post-fit one
    want = pre.copy()
    from fakepta_amd import tm
    rank = tm.project(offs, [p.Mmat for p in psrs], want, weights=w, ctx=ctx)
    assert list(rank) == [8] * P_B
    np.testing.assert_array_equal(post, want)
    truth, _ = T.project_truth(offs, [p.Mmat for p in psrs], w, pre)
    literal = T.project_literal(offs, [p.Mmat for p in psrs], w, pre)
    check_against_truth(f"batch R {R}", offs, post, truth, literal, pre)
    # device only, with the coefficients: the block is projected, the coefficients are the block's own
    none, co = sim.synth(R, seed=4, real0=real0, to_host=False, coeffs=True, fit=True)
    assert none is None and co.shape[2] == R
    np.testing.assert_array_equal(ctx.batch_download(0, R), post)


@pytest.mark.parametrize("R,real0", [(48, 0), (33, 101)])
def test_checksums_and_correlations_see_the_projected_block(ctx, capi, gridded, R, real0):
    """With FPTA_OPT_FUSE_CHECKSUMS the interpolation leaves partial checksums of the block as it wrote it: a
    projection makes them stale, and checksums() must not use them."""
    sim, psrs, offs, w = gridded
    ctx.set_option(capi.OPT_FUSE_CHECKSUMS, 1)
    sim.synth(R, seed=4, real0=real0, to_host=False)
    pre_sums = sim.checksums()
    sim.project()
    sums = sim.checksums()
    block = ctx.batch_download(0, R)
    want = LDR.checksum_truth(block)
    es, cb = np.abs(sums.astype(LD) - want), _checksum_bound(block)
    print(f"R {R}: checksum error / bound {float(np.max(es / cb)):.3g}; sum of squares fell to "
          f"{float(np.max(sums[:, 1] / pre_sums[:, 1])):.3g} of the pre-fit one at most")
    assert np.all(es <= cb) and np.all(sums[:, 1] < pre_sums[:, 1])
    np.testing.assert_array_equal(sim.checksums(), sums)
    # correlations: the estimator on the downloaded post-fit block
    C, sum_c, sum_norm, _ = LDR.correlation_truth(block, P_B, N_B)
    a = np.abs(block).reshape(R, P_B, N_B)
    bound0 = (N_B + 2) * EPS * (a @ a.transpose(0, 2, 1)) / N_B
    bound1 = bound0.sum(axis=0) + R * EPS * np.abs(C).astype(np.float64).sum(axis=0)
    bound2 = R * (N_B + R + 8) * EPS
    plain, normed = sim.correlations(normalized=False), sim.correlations(normalized=True)
    assert np.all(np.abs(plain.astype(LD) - sum_c / R) <= bound1 / R + EPS * np.abs(plain))
    assert np.all(np.abs(normed.astype(LD) - sum_norm / R) <= bound2 / R + EPS * np.abs(normed))


def test_simulate_sharded_with_project_as_the_consumer(ctx, capi, gridded):
    from fakepta_amd.batch import simulate_sharded
    sim, psrs, offs, w = gridded
    n_real, batch_size = 48 + 33, 48
    got = simulate_sharded(sim, n_real, seed=4, real0=7, batch=batch_size, on_batch=lambda s, first, n: s.project())
    assert got.shape == (n_real, 2)
    ctx.set_option(capi.OPT_MFMA_MIN_REAL, 1)  # as the job sets it
    for first in range(0, n_real, batch_size):
        n = min(batch_size, n_real - first)
        block = sim.synth(n, seed=4, real0=7 + first, fit=True)
        es = np.abs(got[first:first + n].astype(LD) - LDR.checksum_truth(block))
        assert np.all(es <= _checksum_bound(block))


@pytest.fixture(scope="module")
def shared_span(capi):
    """C2's signal mix on 64 ragged pulsars over one common span (tests/test_gpu_next_mix.py): the layout whose
    pipelined k_grid_fused blocks also make the next block's common-signal mix (FPTA_OPT_FUSED_NEXT_MIX)."""
    from fakepta_amd.batch import batch_factor
    from oracle import fakepta_oracle as O
    c = capi.Context(0)
    rng = np.random.default_rng(17)
    P = 64  # the fewest pulsars whose mix the fused kernel makes; blocks of a multiple of 128 realizations
    counts = rng.integers(40, 120, size=P)
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    t0, t1 = 0.0, 3.15e8
    toas = np.concatenate([np.concatenate([[t0], np.sort(rng.uniform(t0, t1, k - 2)), [t1]]) for k in counts])
    nu = rng.choice([800.0, 1400.0, 2500.0], size=offs[-1])
    c.batch_set_toas(offs, toas, nu)
    for nm, idx in ((30, 0.0), (100, 2.0)):
        f = np.tile(np.arange(1, nm + 1) / (t1 - t0), (P, 1))
        c.batch_add_signal(0, f, np.sqrt(O.powerlaw(f, rng.uniform(-14.5, -13.5, (P, 1)), 3.0) / (t1 - t0)), idx=idx)
    fc = np.arange(1, 31) / (t1 - t0)
    v = rng.normal(size=(P, 3))
    c.batch_add_signal(1, fc, np.sqrt(O.powerlaw(fc, -14.0, 13 / 3) / (t1 - t0)),
                       L=batch_factor(O.orf_hd(v / np.linalg.norm(v, axis=1)[:, None])))
    c.set_option(capi.OPT_SYNTH_PATH, 4)
    M = np.concatenate([T.mmat(toas[offs[i]:offs[i + 1]], nu[offs[i]:offs[i + 1]]) for i in range(P)])
    assert list(c.batch_set_timing_model(M)) == [8] * P
    yield c
    c.close()


@pytest.mark.parametrize("next_real0,hit", [(384, True), (1000, False)])
def test_projection_leaves_the_next_block_alone(shared_span, next_real0, hit):
    """The block after a projected one is bit for bit the block after an unprojected one, whether the projected
    block's kernel had already made its common-signal mix (the next realizations: a next-mix hit) or not (a jump: a
    miss, the mix is drawn again)."""
    c = shared_span
    outs = []
    for project in (False, True):
        for real0 in (0, 128, 256):  # hits start at the third block of a pipelined run
            c.batch_synth(7, real0, 128, to_host=False)
        assert c.batch_grid_info()["interp_kernel"].startswith("k_grid_fused<")
        if project:
            pre = c.batch_download(0, 128)
            c.batch_project()
            assert not np.array_equal(c.batch_download(0, 128), pre)
        outs.append(c.batch_synth(7, next_real0, 128))
        assert c.batch_grid_info()["next_mix_used"] == hit
    np.testing.assert_array_equal(outs[1], outs[0])


def test_state_errors_and_set_toas_clears_the_model(capi):
    c = capi.Context(0)
    try:
        rng = np.random.default_rng(3)
        offs, toas, nu = random_layout(rng, 3, (40, 60))
        with pytest.raises(capi.FptaError, match="set_toas first"):
            c.batch_set_timing_model(np.ones((int(offs[-1]), 1)))
        c.batch_set_toas(offs, toas, nu)
        f, a = per_psr_signal(rng, offs, toas, 10)
        c.batch_add_signal(0, f, a)
        M = np.concatenate([T.mmat(toas[offs[i]:offs[i + 1]], nu[offs[i]:offs[i + 1]]) for i in range(3)])
        assert list(c.batch_set_timing_model(M)) == [8, 8, 8]
        with pytest.raises(capi.FptaError, match="nothing synthesized"):
            c.batch_project()
        pre = c.batch_synth(1, 0, 20)
        c.batch_project()
        post = c.batch_download(0, 20)
        assert not np.array_equal(pre, post)
        assert list(c.batch_set_timing_model(None)) == [0, 0, 0]  # cleared
        with pytest.raises(capi.FptaError, match="no timing model"):
            c.batch_project()
        c.batch_set_timing_model(M, ncol_psr=[8, 0, 3])
        c.batch_synth(1, 0, 20, to_host=False)
        c.batch_project()
        part = c.batch_download(0, 20)
        np.testing.assert_array_equal(part[:, offs[1]:offs[2]], pre[:, offs[1]:offs[2]])  # rank 0: untouched
        np.testing.assert_array_equal(part[:, :offs[1]], post[:, :offs[1]])
        c.batch_set_toas(offs, toas, nu)  # a new layout: the model is gone
        c.batch_add_signal(0, f, a)
        c.batch_synth(1, 0, 20, to_host=False)
        with pytest.raises(capi.FptaError, match="no timing model"):
            c.batch_project()
        c.set_option(capi.OPT_PROFILE, 1)  # one FPTA_K_DENSE entry per projection
        c.batch_set_timing_model(M)
        c.reset_stats()
        c.batch_project()
        c.synchronize()
        assert c.kernel_stats(capi.K_DENSE)[0] == 1
    finally:
        c.close()


# ----------------------------------------------------------------------------- drop-in
def test_drop_in_fit_timing_model(ctx):
    from fakepta import fake_pta as fp
    np.random.seed(11)
    psrs = fp.make_fake_array(npsrs=3, Tobs=10, ntoas=90, gaps=True, toaerr=1e-7, pdist=1.0,
                              freqs=[800, 1400, 2500], backends=["A", "B"],
                              custom_model={"RN": 10, "DM": 10, "Sv": None})
    offs = np.concatenate([[0], np.cumsum([len(p.toas) for p in psrs])]).astype(np.int64)
    res = np.concatenate([p.residuals for p in psrs])
    mats = [p.Mmat.copy() for p in psrs]
    w = np.concatenate([1 / p._white_sigma2() for p in psrs])
    truth, ranks = T.project_truth(offs, mats, w, res)
    literal = T.project_literal(offs, mats, w, res)
    models = [{k: {kk: np.copy(vv) if isinstance(vv, np.ndarray) else vv for kk, vv in v.items()}
               for k, v in p.signal_model.items()} for p in psrs]
    signal0 = psrs[0].reconstruct_signal()
    # one pulsar
    one = psrs[0]
    keep = one.residuals.copy()
    assert one.fit_timing_model() == ranks[0] == 8
    check_against_truth("Pulsar.fit_timing_model", offs[:2], one.residuals, truth[:offs[1]], literal[:offs[1]],
                        res[:offs[1]])
    first = one.residuals.copy()
    one.residuals = keep
    # the whole array in one call
    got_ranks = fp.fit_timing_model_array(psrs)
    np.testing.assert_array_equal(got_ranks, ranks)
    got = np.concatenate([p.residuals for p in psrs])
    check_against_truth("fit_timing_model_array", offs, got, truth, literal, res)
    np.testing.assert_array_equal(psrs[0].residuals, first)
    for p, sm in zip(psrs, models):  # the stored signals are the pre-fit ones
        assert list(p.signal_model) == list(sm)
        for k in sm:
            for kk, vv in sm[k].items():
                np.testing.assert_array_equal(p.signal_model[k][kk], vv)
    np.testing.assert_array_equal(psrs[0].reconstruct_signal(), signal0)
    # unit weights are another fit
    two = psrs[1]
    two.residuals = res[offs[1]:offs[2]].copy()
    two.fit_timing_model(weights=None)
    t1, _ = T.project_truth(offs[1:3] - offs[1], mats[1:2], None, res[offs[1]:offs[2]])
    l1 = T.project_literal(offs[1:3] - offs[1], mats[1:2], None, res[offs[1]:offs[2]])
    check_against_truth("unit weights", offs[1:3] - offs[1], two.residuals, t1, l1, res[offs[1]:offs[2]])
