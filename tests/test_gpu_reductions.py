"""fpta_batch_correlations and fpta_batch_checksums against longdouble sums of the downloaded block
(tests/ld_reference.py), at realization counts on both sides of the 256 partial sums of modes 1 and 2 (one
realization per part up to 256, then rper = ceil(R / 256) per part with empty trailing parts when R is no
multiple of rper) and pulsar counts on both sides of the 64-pulsar tile.

Derived bounds (eps = 2^-52; a dot product of m fp64 products, summed in any order, fused or not, errs by at most
gamma_m sum |a_i b_i|, gamma_m ~ m eps / 2; the bounds take m eps, a factor 2 of slack):
  * mode 0, C_r[a][b] = (sum_t x_a x_b) / n: n products and the division, (n + 2) eps sum_t |x_a x_b| / n.
  * mode 3, C_r[p][p]: the same with positive terms, (n + 2) eps C_r[p][p].
  * mode 1, sum_r C_r: the mode-0 errors of its terms plus an R-term sum, sum_r bound0_r + R eps sum_r |C_r[a][b]|.
  * mode 2, sum_r C_r[a][b] / sqrt(C_r[a][a] C_r[b][b]): by Cauchy-Schwarz sum_t |x_a x_b| / n <= sqrt(C_aa C_bb),
    so a term's numerator contributes at most (n + 2) eps / 2, the two auto-correlations under the square root
    (n + 2) eps / 2 together, and the product, the square root and the quotient 3 eps / 2 more: (n + 8) eps per
    term with the slack, each term at most 1 in magnitude; summing R of them adds R eps R. In all R (n + R + 8) eps,
    absolute.
  * checksums: n_toa additions of the values (or of their squares), (n_toa + 2) eps sum |v| (or sum v^2)."""
import numpy as np
import pytest

from oracle import fakepta_oracle as O
from tests import ld_reference as T

pytestmark = pytest.mark.gpu

EPS = T.EPS
LD = np.longdouble
T0, SPAN = 4.5e9, 3.15e8
SHAPES = [(1, 1, 1), (2, 31, 255), (64, 32, 256), (65, 33, 257), (130, 150, 300), (70, 64, 1000)]


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


def unit_vectors(rng, P):
    v = rng.normal(size=(P, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def set_layout(ctx, rng, n_per_psr):
    """One common HD signal of 10 modes plus white noise, as test_device_correlations_match_numpy."""
    n_per_psr = np.asarray(n_per_psr)
    P = len(n_per_psr)
    offs = np.concatenate([[0], np.cumsum(n_per_psr)]).astype(np.int64)
    epochs = np.sort(T0 + rng.uniform(0.0, SPAN, int(n_per_psr.max())))
    toas = np.concatenate([epochs[:k] for k in n_per_psr])
    ctx.batch_set_toas(offs, toas, np.full(int(offs[-1]), 1400.0))
    f = O.freq_grid(10, SPAN)
    ctx.batch_add_signal(1, f, np.sqrt(O.powerlaw(f, -14.0, 4.0) * O.delta_f(f)),
                         L=O.mvn_factor(O.orf_hd(unit_vectors(rng, P))))
    ctx.batch_set_white(np.full(int(offs[-1]), 1e-7))


def bounds(block, P, n, C):
    """(bound0 [R][P][P], bound1 [P][P], bound2 scalar, bound3 [R][P]) of the module docstring."""
    R = block.shape[0]
    a = np.abs(block).reshape(R, P, n)
    bound0 = (n + 2) * EPS * (a @ a.transpose(0, 2, 1)) / n
    absC = np.abs(C).astype(np.float64)
    bound1 = bound0.sum(axis=0) + R * EPS * absC.sum(axis=0)
    bound3 = (n + 2) * EPS * np.einsum("raa->ra", absC)
    return bound0, bound1, R * (n + R + 8) * EPS, bound3


@pytest.mark.parametrize("P,n,R", SHAPES)
def test_correlations_and_checksums_vs_longdouble(ctx, P, n, R):
    rng = np.random.default_rng([P, n, R])
    set_layout(ctx, rng, np.full(P, n))
    assert ctx.batch_synth(9, 0, R, to_host=False) is None
    block = ctx.batch_download(0, R)
    assert block.shape == (R, P * n) and np.all(np.isfinite(block)) and block.any()
    C, sum_c, sum_norm, autos = T.correlation_truth(block, P, n)
    bound0, bound1, bound2, bound3 = bounds(block, P, n, C)
    ratio = lambda err, bound: float(np.max(err / bound))  # noqa: E731

    m0 = ctx.batch_correlations(0)
    e0 = np.abs(m0.astype(LD) - C)
    m3 = ctx.batch_correlations(3)
    e3 = np.abs(m3.astype(LD) - autos)
    m1 = ctx.batch_correlations(1)
    e1 = np.abs(m1.astype(LD) - sum_c)
    e10 = np.abs(m1.astype(LD) - m0.astype(LD).sum(axis=0))
    m2 = ctx.batch_correlations(2)
    e2 = np.abs(m2.astype(LD) - sum_norm)
    print(f"P {P} n {n} R {R}: error / bound: mode 0 {ratio(e0, bound0):.3g}, mode 1 {ratio(e1, bound1):.3g} "
          f"(against the sum of mode 0: {ratio(e10, bound1):.3g}), mode 2 {ratio(e2, bound2):.3g}, "
          f"mode 3 {ratio(e3, bound3):.3g}")
    assert np.all(e0 <= bound0)
    assert np.all(e3 <= bound3)
    assert np.all(e1 <= bound1)
    assert np.all(e10 <= bound1)  # mode 1 is the sum of mode 0 over the realizations
    assert np.all(e2 <= bound2)
    for m in (m0, m1, m2):
        np.testing.assert_array_equal(m, np.swapaxes(m, -1, -2))  # both triangles are written from one value
    np.testing.assert_array_equal(ctx.batch_correlations(1), m1)  # bitwise repeatable
    np.testing.assert_array_equal(ctx.batch_correlations(2), m2)

    sums = ctx.batch_checksums()
    want = T.checksum_truth(block)
    n_toa = P * n
    cb = (n_toa + 2) * EPS * np.stack([np.abs(block).sum(axis=1), (block * block).sum(axis=1)], axis=1)
    es = np.abs(sums.astype(LD) - want)
    print(f"P {P} n {n} R {R}: checksum error / bound {ratio(es, cb):.3g}")
    assert sums.shape == (R, 2) and np.all(es <= cb)


def test_batch_simulator_statistics_are_exact():
    """BatchSimulator.correlations and hd_curve(estimator="per_realization") on a (65, 33, 257) block equal the
    same quantities computed from the longdouble truth of the downloaded block: the mode-1 / mode-2 bounds over R,
    plus eps for the host's division by R; a bin's mean and standard deviation move by at most the largest error of
    its members (both are 1-Lipschitz in the sup norm), plus the rounding of numpy's own mean / std (8 eps)."""
    from fakepta import correlated_noises as cn
    from fakepta import fake_pta as fp
    from fakepta_amd import _capi
    from fakepta_amd.batch import BatchSimulator
    P, n, R, bins = 65, 33, 257, 8
    np.random.seed(65)
    psrs = fp.make_fake_array(npsrs=P, Tobs=10, ntoas=n, gaps=False, isotropic=True, toaerr=1e-7,
                              backends="X.1400", custom_model={"RN": None, "DM": None, "Sv": None})
    cn.add_common_correlated_noise(psrs, orf="hd", log10_A=-14, gamma=13 / 3, components=10)
    ctx = _capi.Context(0)
    try:
        sim = BatchSimulator(psrs, white=True, ctx=ctx)
        assert sim.synth(R, seed=12, to_host=False) is None
        block = ctx.batch_download(0, R)
        C, sum_c, sum_norm, _ = T.correlation_truth(block, P, n)
        _, bound1, bound2, _ = bounds(block, P, n, C)
        plain, normed = sim.correlations(normalized=False), sim.correlations(normalized=True)
        mean, std, centres, counts = sim.hd_curve(bins=bins, estimator="per_realization", return_counts=True)
    finally:
        ctx.close()
    assert np.all(np.abs(plain.astype(LD) - sum_c / R) <= bound1 / R + EPS * np.abs(plain))
    assert np.all(np.abs(normed.astype(LD) - sum_norm / R) <= bound2 / R + EPS * np.abs(normed))
    pos = np.array([p.pos for p in psrs])
    iu = np.triu_indices(P, 1)
    angles = np.arccos(np.clip(pos @ pos.T, -1.0, 1.0))[iu]
    corrs = (sum_norm / R)[iu]
    edges = np.linspace(0.0, np.pi, bins + 1)
    np.testing.assert_array_equal(centres, edges[:-1] + 0.5 * (edges[1] - edges[0]))
    assert counts.sum() == P * (P - 1) // 2 and np.count_nonzero(counts) >= bins - 1
    tol = bound2 / R + 8 * EPS
    for b in range(bins):
        sel = corrs[(angles > edges[b]) & (angles < edges[b + 1])]
        assert len(sel) == counts[b]
        if len(sel) == 0:  # no pair this close on a 65-pulsar lattice: NaN, as the reference's bin_curve gives
            assert np.isnan(mean[b]) and np.isnan(std[b])
            continue
        mu = sel.sum() / len(sel)
        sd = np.sqrt(((sel - mu) ** 2).sum() / len(sel))
        assert abs(mean[b] - mu) <= tol and abs(std[b] - sd) <= tol


def test_ragged_array_is_refused(ctx, capi):
    rng = np.random.default_rng(3)
    set_layout(ctx, rng, [33, 33, 32, 33])
    ctx.batch_synth(1, 0, 4, to_host=False)
    for mode in range(4):
        with pytest.raises(capi.FptaError, match="same number of TOAs"):
            ctx.batch_correlations(mode)
    assert ctx.batch_checksums().shape == (4, 2)  # the checksums need no common TOA count
