"""The dense-covariance kernels (csrc/dense.hip, dense_build / dense_cholesky in csrc/capi.hip) stage by stage against
longdouble, element by element: tests/dense_reference.py holds the truths and the allowances, none of them measured on
the code under test, and tests/test_dense_reference.py shows on the CPU that numpy's fp64 stays inside them and that
deliberate defects do not. tests/test_gpu_dense.py keeps the norm-wise comparison with the reference's recorded
matrices; on its red spectra a wrong top mode or one bad element of the factor passes.

Inputs (dense_reference.make_case): real-MJD epochs (T0 = 4.5e9 s, span 3.15e8 s), sorted random TOAs, nu from {800,
1400, 2500}, every signal on f_k = k / span with the flat weight w = (1e-7)^2 so that no mode hides behind another,
white = (1e-7 U(0.5, 2))^2. Mode sets: one (1 mode, idx 0), idx1 (3 modes, idx 1), m15 ((7, idx 0) + (5, idx 2) + (3,
idx 4): 2 M % 4 == 2, so the padded basis rows take part), m12 ((8, idx 0) + (4, idx 2.5): pow). Sizes: m15 at n = 1,
2, 63, 64, 65, 128, 256, 257, 321 (a one-row last panel, a one-row second k_trsm_panel workgroup, six tile rows), 384
(an exact last panel); the others at 1, 65, 321.

Stages. The intermediates come through the test hook fpta_debug_dense (Context.debug_dense):
  covariance  |gp_covariance - cov_truth| <= cov_bound, with and without white_var; bitwise symmetric, bitwise equal on
              a repeat; one mode also against the closed form w cos(phi_i - phi_j) of the exact phase.
  factor      Lhat = debug_dense(0) after noise_wiener, C_dev = gp_covariance on the same inputs (the matrix as the
              device built it): |tril(Lhat) tril(Lhat)^T - C_dev| <= factor_bound; positive diagonal; exact zeros above
              the diagonal inside each 64-block; the blocks above those still hold C_dev (the factorisation writes the
              lower triangle only). Also without white_var through noise_draw (n = 20, full rank on 30 columns).
  solve       yhat = debug_dense(1): |r - C_dev yhat| <= solve_bound; |out - (r - white yhat)| <= eps (|r| + |white
              yhat|).
  draws       (n, real0, R) in (1, 0, 1), (2, 1, 2), (63, 7, 37), (256, 0, 256), (321, 3, 257), straddling ldz = 256:
              Zhat = debug_dense(2): |X - Zhat Lhat^T| <= draw_bound; Zhat within 16 eps x the Box-Muller pair's radius
              of the oracle's DENSE_STREAM normals (the rule of test_device_normals4_edge_words; the pair partner of
              realization g at a TOA is realization g ^ 1); any other split of the realizations bitwise equal.
  pivot       white_var[j] = -10 x the diagonal: noise_draw names pivot j exactly, j in 0, 63, 64, 200, 320 at n = 321.
  reuse       n = 384, then n = 63 and 65 on the same context: bitwise what a fresh context gives (dn_PT, dn_Z and
              dn_GT are reused without clearing).
  drop-in     Pulsar.make_time_correlated_noise_cov(signal="system_noise_<backend>") and draw_noise_model_batch against
              the context calls on the same arrays, bitwise, and the former inside cov_bound.

Worst error / allowance per stage as printed on an MI355X (the allowance is 1):

  stage                        m15 (n = 1 .. 384)  one               idx1              m12
  covariance (same with white) 7.1e-4 .. 0.230     0.0089 .. 0.242   0.0036 .. 0.240   0.0010 .. 0.239
  one mode, closed form                            0.0089 .. 0.242
  factor                       0.108 .. 0.209      0.073 .. 0.196    0.063 .. 0.187    0.110 .. 0.158
  solve, residual              4.1e-4 .. 0.034     6.5e-4 .. 0.070   3.6e-4 .. 0.0039  3.6e-4 .. 0.071
  solve, output                0.113 .. 0.476      0.093 .. 0.468    0.068 .. 0.386    0.085 .. 0.451
  no white, n = 20: factor 0.110, draws 0.092
  draws, the five cases in order: product 0.053, 0.097, 0.134, 0.156, 0.173; normals 0, 0, 0.055, 0.060, 0.061
  drop-in system noise, both backends: 0.242

The covariance's largest figures are at the large n and equal numpy's own on the same inputs (0.24: the literal fp64
evaluation, whose distance from the truth enters the allowance four times, so the phase rounding dominates); the
smallest n show the floor 4 eps a. The solve's residual is far inside its worst-case allowance, as for numpy (about
half an eps of |L| |L|^T |y|).

That the allowances bite on the device, not only in tests/test_dense_reference.py: a copy of the library with the last
mode's sin row of k_cov_basis scaled by 1 + 1e-9 read 25 (m15, n = 1) .. 7e5 (one, n = 321) in every covariance case and
2.8e4 in the drop-in case, and one with x[0] of k_trsm_panel's second workgroup scaled by 1 + 1e-12 read 1126 = 1e-12
/ (4 eps) in the factor at n = 321 and 384 and left every other size passing.
"""
import re

import numpy as np
import pytest

from oracle import fakepta_oracle as O
from tests import dense_reference as D

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = D.EPS
DRAW_CASES = [(1, 0, 1), (2, 1, 2), (63, 7, 37), (256, 0, 256), (321, 3, 257)]
SEED = 20240229


@pytest.fixture(scope="module")
def capi():
    from fakepta_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def ctx(capi):
    c = capi.Context(0)
    yield c
    c.close()


def blocks_mask(n):
    """(inside a 64 x 64 diagonal block and above the diagonal, in a block above the diagonal blocks) [n, n]."""
    i = np.arange(n)
    same = (i[:, None] // 64) == (i[None, :] // 64)
    return same & (i[:, None] < i[None, :]), (i[:, None] // 64) < (i[None, :] // 64)


# --------------------------------------------------------------------------- covariance
@pytest.mark.parametrize("name,n", D.CASES)
def test_covariance(ctx, name, n):
    toas, nu, segs, white, _ = D.make_case(name, n)
    ref = D.case_reference(name, n)
    cov0 = ctx.gp_covariance(toas, nu, segs)
    cov = ctx.gp_covariance(toas, nu, segs, white_var=white)
    assert cov0.shape == cov.shape == (n, n) and np.all(np.isfinite(cov0)) and np.all(np.isfinite(cov))
    r0, r1 = D.worst(cov0.astype(LD) - ref.truth0, ref.bound0), D.worst(cov.astype(LD) - ref.truth, ref.bound)
    print(f"covariance {name} n = {n}: {r0:.3g} (with white {r1:.3g})")
    assert r0 < 1 and r1 < 1
    np.testing.assert_array_equal(cov0, cov0.T)
    np.testing.assert_array_equal(cov, cov.T)
    np.testing.assert_array_equal(ctx.gp_covariance(toas, nu, segs), cov0)
    np.testing.assert_array_equal(ctx.gp_covariance(toas, nu, segs, white_var=white), cov)
    off = ~np.eye(n, dtype=bool)
    np.testing.assert_array_equal(cov[off], cov0[off])  # the white variances touch the diagonal alone
    if name == "one":
        ph = D.T.phase(segs[0][0], toas)[:, 0]
        closed = LD(segs[0][1][0]) * np.cos(ph[:, None] - ph[None, :])
        rc = D.worst(cov0.astype(LD) - closed, ref.bound0)
        print(f"covariance one n = {n} against the closed form: {rc:.3g}")
        assert rc < 1


# --------------------------------------------------------------------------- factor and solve
def check_factor(Lhat, C_dev, label):
    n = len(C_dev)
    assert Lhat.shape == (n, n) and np.all(np.isfinite(Lhat))
    assert np.all(np.diag(Lhat) > 0)
    above, upper_blocks = blocks_mask(n)
    assert np.all(Lhat[above] == 0.0)
    np.testing.assert_array_equal(Lhat[upper_blocks], C_dev[upper_blocks])
    low = np.tril(np.ones((n, n), dtype=bool))
    ratio = D.worst((D.factor_product(Lhat) - C_dev.astype(LD))[low], D.factor_bound(Lhat)[low])
    print(f"factor {label}: {ratio:.3g}")
    assert ratio < 1
    return ratio


@pytest.mark.parametrize("name,n", D.CASES)
def test_factor_and_solve(ctx, name, n):
    toas, nu, segs, white, r = D.make_case(name, n)
    out = ctx.noise_wiener(toas, nu, segs, white, r)
    Lhat, yhat = ctx.debug_dense(0), ctx.debug_dense(1)
    C_dev = ctx.gp_covariance(toas, nu, segs, white_var=white)
    check_factor(Lhat, C_dev, f"{name} n = {n}")
    assert yhat.shape == (n,) and np.all(np.isfinite(yhat)) and np.all(np.isfinite(out))
    res = r.astype(LD) - C_dev.astype(LD) @ yhat.astype(LD)
    rs = D.worst(res, D.solve_bound(Lhat, yhat))
    wy = white.astype(LD) * yhat.astype(LD)
    ro = D.worst(out.astype(LD) - (r.astype(LD) - wy), LD(EPS) * (np.abs(r).astype(LD) + np.abs(wy)))
    print(f"solve {name} n = {n}: residual {rs:.3g}, output {ro:.3g}")
    assert rs < 1 and ro < 1


def test_factor_without_white(ctx):
    """white_var == NULL through the factorisation: n = 20 on the 30 basis columns of m15 is positive definite."""
    toas, nu, segs, _, _ = D.make_case("m15", 20)
    x = ctx.noise_draw(toas, nu, segs, None, SEED, 0, 3)
    Lhat, Z = ctx.debug_dense(0), ctx.debug_dense(2).T
    C_dev = ctx.gp_covariance(toas, nu, segs)
    check_factor(Lhat, C_dev, "m15 n = 20, no white")
    rd = D.worst(x.astype(LD) - D.draw_product(Z, Lhat), D.draw_bound(Z, Lhat))
    print(f"draws m15 n = 20, no white: {rd:.3g}")
    assert rd < 1


# --------------------------------------------------------------------------- draws
@pytest.mark.parametrize("n,real0,R", DRAW_CASES)
def test_draws(ctx, n, real0, R):
    toas, nu, segs, white, _ = D.make_case("m15", n)
    x = ctx.noise_draw(toas, nu, segs, white, SEED, real0, R)
    Lhat, Z = ctx.debug_dense(0), ctx.debug_dense(2).T  # [R, n]
    assert x.shape == Z.shape == (R, n) and np.all(np.isfinite(x)) and np.all(np.isfinite(Z))
    rd = D.worst(x.astype(LD) - D.draw_product(Z, Lhat), D.draw_bound(Z, Lhat))
    # the oracle's normals on the even-aligned range: realizations 2 h and 2 h + 1 are one Box-Muller pair per TOA
    lo, hi = real0 & ~1, (real0 + R + 1) & ~1
    want = O.quad_normals(SEED, np.arange(lo, hi), n, O.DENSE_STREAM)
    radius = np.repeat(np.hypot(want[0::2], want[1::2]), 2, axis=0)[real0 - lo:real0 - lo + R]
    want = want[real0 - lo:real0 - lo + R]
    rz = float(np.max(np.abs(Z - want) / (16 * EPS * np.maximum(radius, np.finfo(np.float64).tiny))))
    print(f"draws n = {n}, real0 = {real0}, R = {R}: product {rd:.3g}, normals {rz:.3g}")
    assert rd < 1 and rz <= 1
    # any other split of the realizations gives the same bits: a longer call, and one starting one realization later
    np.testing.assert_array_equal(ctx.noise_draw(toas, nu, segs, white, SEED, real0, R + 3)[:R], x)
    if R > 1:
        np.testing.assert_array_equal(ctx.noise_draw(toas, nu, segs, white, SEED, real0 + 1, R - 1), x[1:])


# --------------------------------------------------------------------------- the pivot report
@pytest.mark.parametrize("j", [0, 63, 64, 200, 320])
def test_pivot_report(ctx, capi, j):
    """An error return, not a fault: every leading block before j is positive definite, pivot j is not."""
    n = 321
    toas, nu, segs, white, _ = D.make_case("m15", n)
    bad = white.copy()
    bad[j] = -10.0 * float(D.case_reference("m15", n).truth0[j, j])
    with pytest.raises(capi.FptaError, match=rf"not positive definite \(pivot {j}\)"):
        ctx.noise_draw(toas, nu, segs, bad, SEED, 0, 4)
    with pytest.raises(capi.FptaError, match="debug_dense"):  # a failed call leaves nothing to read
        ctx.debug_dense(0)
    ctx.noise_draw(toas, nu, segs, white, SEED, 0, 4)  # and the context works on


# --------------------------------------------------------------------------- a small problem after a larger one
def test_reuse_after_a_larger_problem(ctx, capi):
    big = D.make_case("m15", 384)
    ctx.noise_wiener(*big[:4], big[4])
    ctx.noise_draw(*big[:4], SEED, 0, 300)
    fresh = capi.Context(0)
    try:
        for n in (63, 65):
            toas, nu, segs, white, r = D.make_case("m15", n)
            got = []
            for c in (ctx, fresh):  # ctx first: its buffers hold the larger problem
                g = {"wiener": c.noise_wiener(toas, nu, segs, white, r)}
                g["factor (wiener)"], g["y"] = c.debug_dense(0), c.debug_dense(1)
                g["draws"] = c.noise_draw(toas, nu, segs, white, SEED, 5, 9)
                g["factor (draws)"], g["normals"] = c.debug_dense(0), c.debug_dense(2)
                g["covariance"] = c.gp_covariance(toas, nu, segs, white_var=white)
                got.append(g)
            for item in got[0]:
                np.testing.assert_array_equal(got[0][item], got[1][item], err_msg=f"n = {n}: {item}")
    finally:
        fresh.close()


# --------------------------------------------------------------------------- the hook itself
def test_debug_dense_reports_what_the_last_call_left(capi):
    c = capi.Context(0)
    try:
        with pytest.raises(capi.FptaError, match="no dense call"):
            c.debug_dense(0)
        toas, nu, segs, white, r = D.make_case("m12", 65)
        cov = c.gp_covariance(toas, nu, segs, white_var=white)
        np.testing.assert_array_equal(c.debug_dense(0), cov)
        for what in (1, 2):
            with pytest.raises(capi.FptaError, match="was not fpta_noise_"):
                c.debug_dense(what)
        c.noise_wiener(toas, nu, segs, white, r)
        with pytest.raises(capi.FptaError, match="was not fpta_noise_draw"):
            c.debug_dense(2)
        buf = np.empty((66, 66))
        rc = capi._lib.fpta_debug_dense(c._h, 0, 66, 66, buf.ctypes.data_as(capi._vp))
        assert rc == -77 and re.search(r"65 x 65, not 66 x 66", capi._lib.fpta_last_error(c._h).decode())  # FPTA_ESTATE
        c.noise_draw(toas, nu, segs, white, SEED, 0, 5)
        assert c.debug_dense(2).shape == (65, 5)
        with pytest.raises(capi.FptaError, match="was not fpta_noise_wiener"):
            c.debug_dense(1)
    finally:
        c.close()


# --------------------------------------------------------------------------- the drop-in
@pytest.fixture(scope="module")
def pulsar():
    """Two backends on 40 real-MJD epochs (80 TOAs), flat custom spectra of 7 / 5 / 3 modes (idx 0 / 2 / 4) and a
    4-mode system noise on each backend."""
    from fakepta import fake_pta as fp
    rng = np.random.default_rng(77)
    epochs = np.sort(D.T0 + D.SPAN * rng.random(40))
    np.random.seed(31)
    psr = fp.Pulsar(epochs, 1e-7, 0.9, 1.7, freqs=[1400], backends=["A.1400", "B.800"],
                    custom_model={"RN": 7, "DM": 5, "Sv": 3})

    def flat(nm):
        f = np.arange(1, nm + 1) / D.SPAN
        return dict(spectrum="custom", f_psd=f, custom_psd=D.AMP ** 2 / O.delta_f(f))

    psr.add_red_noise(**flat(7))
    psr.add_dm_noise(**flat(5))
    psr.add_chromatic_noise(**flat(3))
    for b in psr.backends:
        psr.add_system_noise(backend=b, components=4, **flat(4))
    return psr


def test_dropin_system_noise_covariance(ctx, pulsar):
    for b in pulsar.backends:
        mask = pulsar.backend_flags == b
        assert 0 < mask.sum() < len(mask)
        seg = pulsar._dense_segment(f"{b}_system_noise_{b}", 1400)
        toas, nu = pulsar.toas[mask], pulsar.freqs[mask]
        cov = pulsar.make_time_correlated_noise_cov(signal=f"system_noise_{b}")
        assert cov.shape == (mask.sum(), mask.sum())
        np.testing.assert_array_equal(cov, ctx.gp_covariance(toas, nu, [seg]))
        ratio = D.worst(cov.astype(LD) - D.cov_truth(toas, nu, [seg]), D.cov_bound(toas, nu, [seg]))
        print(f"drop-in system noise {b}: {ratio:.3g}")
        assert ratio < 1


def test_dropin_draw_noise_model_batch(ctx, pulsar):
    segs, white = pulsar._red_segments(), pulsar._white_sigma2()
    assert len(segs) == 3
    for R, seed, real0 in ((1, 5, 0), (9, 2 ** 40 + 3, 6)):
        got = pulsar.draw_noise_model_batch(R, seed=seed, real0=real0)
        assert got.shape == (R, len(pulsar.toas))
        np.testing.assert_array_equal(got, ctx.noise_draw(pulsar.toas, pulsar.freqs, segs, white, seed, real0, R))
