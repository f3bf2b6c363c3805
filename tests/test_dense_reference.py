"""tests/dense_reference.py checked on the CPU: the longdouble truth against the reference's recorded matrices, numpy's
fp64 evaluation of every stage inside every allowance on the inputs tests/test_gpu_dense_kernels.py gives the device,
and deliberate defects (on the numpy side only) outside them.

What the defects show, as printed here (error / allowance; the allowance is 1):

  numpy fp64 on the GPU test's inputs: covariance 7e-4 (n = 1) .. 0.24 (with and without the white diagonal), factor
    0.06 .. 0.21, solve 3.5e-4 .. 0.07, draws 0.07 .. 0.19.  Fixture G6 against the truth: 0.02 .. 0.09.
  (a) the top mode's sin column scaled by 1 + 1e-9, 30 modes:
      - red spectrum (gamma = 4.5): assert_parity at 1e-10 passes (3e-16). So does cov_bound (0.23 with and without the
        defect), and no sound allowance on the covariance could refuse it: the defect moves an element by 1e-9 w_30 =
        1e-9 30^-4.5 w_1 = 1.02 eps w_1, one rounding of the first mode's own term and 1 / 60 of the dot product's
        allowance. A red covariance cannot show
        this defect at all, which is why the device is tested on flat weights;
      - the flat weights of the GPU test: cov_bound refuses it at 376.
  (b) the last mode's sin row dropped (the padded-row case, 2 M % 4 == 2), gamma = 4.5:
      - M = 15: cov_bound refuses it at 5e8. assert_parity at 1e-10 refuses it too (3.6e-6 = 0.7 x 15^-4.5): the old
        check is blind to a lost top row only where w_M / w_1 < 1e-10;
      - M = 171 (the same padding): assert_parity passes (6.0e-11), cov_bound refuses it at 3e3.
  (c) one element of the factor's last, ragged row (n = 65 and 321, its first column) off by 1e-12 relative:
      factor_bound refuses it at 1e-12 / (4 eps) = 1126, whatever the matrix.
  (d) one term left out of one row's forward substitution: solve_bound refuses it at 1.5e5 (n = 321) and 4e8 (n = 65).
"""
import functools

import numpy as np
import pytest

from oracle import fakepta_oracle as O
from tests import dense_reference as D
from tests.conftest import assert_parity, rel_err

LD = np.longdouble
EPS = D.EPS


# --------------------------------------------------------------------------- the truth against the fixture
def _g6_segs(g, labs):
    return [(g[f"{lab}_f"], g[f"{lab}_psd"] * O.delta_f(g[f"{lab}_f"]), float(g[f"{lab}_idx"]), 1400.0)
            for lab in labs]


@pytest.mark.parametrize("labs", [("rn",), ("dm",), ("sv",), ("rn", "dm", "sv")], ids=["rn", "dm", "sv", "red"])
def test_cov_truth_matches_the_recorded_covariances(golden, labs):
    """Fixture G6 holds the reference's own fp64 matrices (basis diag(psd df) basis^T on the literal phase): they are
    within the allowance of an fp64 evaluation of the truth, and far inside the suite's 1e-10."""
    g = golden("g6_dense_cov.npz")
    segs = _g6_segs(g, labs)
    want = g["red_cov"] if len(labs) > 1 else g[f"{labs[0]}_cov"]
    truth = D.cov_truth(g["toas"], g["freqs"], segs)
    ratio = D.worst(want.astype(LD) - truth, D.cov_bound(g["toas"], g["freqs"], segs))
    print(f"G6 {'+'.join(labs)}: |fixture - truth| / allowance {ratio:.3g}, norm-wise "
          f"{rel_err(truth.astype(np.float64), want):.3g}")
    assert ratio < 1
    assert_parity(truth.astype(np.float64), want, 1e-13)
    d = D.cov_truth(g["toas"], g["freqs"], segs, g["white_cov"]) - truth  # the white variances: the diagonal alone
    assert np.all(d[~np.eye(len(d), dtype=bool)] == 0)
    assert np.all(np.abs(np.diag(d) - g["white_cov"]) <= 2.0 ** -62 * (np.diag(truth) + g["white_cov"]))


# --------------------------------------------------------------------------- numpy fp64 inside every allowance
def forward(L, r, skip=None):
    """L u = r by rows in fp64; skip = (i, k) leaves the term L[i][k] u[k] out of row i (defect (d))."""
    u = np.zeros(len(r))
    for i in range(len(r)):
        row = L[i, :i].copy()
        if skip is not None and skip[0] == i:
            row[skip[1]] = 0.0
        u[i] = (r[i] - row @ u[:i]) / L[i, i]
    return u


def backward(L, u):
    """L^T y = u by rows in fp64."""
    y = np.zeros(len(u))
    for i in range(len(u) - 1, -1, -1):
        y[i] = (u[i] - L[i + 1:, i] @ y[i + 1:]) / L[i, i]
    return y


@functools.lru_cache(maxsize=None)
def numpy_stages(name, n):
    """numpy's fp64 run of the whole path on one case: (C without white, C, L, y)."""
    toas, nu, segs, white, r = D.make_case(name, n)
    G = D.basis_literal(toas, nu, segs)
    C0 = G @ G.T
    C = C0 + np.diag(white)
    L = np.linalg.cholesky(C)
    y = backward(L, forward(L, r))
    return C0, C, L, y


@pytest.mark.parametrize("name,n", D.CASES)
def test_numpy_fp64_stays_inside_every_allowance(name, n):
    toas, nu, segs, white, r = D.make_case(name, n)
    C0, C, L, y = numpy_stages(name, n)
    ref = D.case_reference(name, n)
    cov0 = D.worst(C0.astype(LD) - ref.truth0, ref.bound0)
    cov = D.worst(C.astype(LD) - ref.truth, ref.bound)
    fac = D.worst(D.factor_product(L) - C.astype(LD), D.factor_bound(L))
    res = r.astype(LD) - C.astype(LD) @ y.astype(LD)
    sol = D.worst(res, D.solve_bound(L, y))
    z = np.random.default_rng(n).standard_normal((5, n))
    drw = D.worst((z @ L.T).astype(LD) - D.draw_product(z, L), D.draw_bound(z, L))
    print(f"numpy {name} n = {n}: covariance {cov0:.3g} (white {cov:.3g}), factor {fac:.3g}, solve {sol:.3g}, "
          f"draws {drw:.3g}")
    assert max(cov0, cov, fac, sol, drw) < 1


def test_numpy_fp64_full_rank_without_white():
    """n = 20 on the 30 columns of M = 15: positive definite with no white diagonal (the GPU test's noise_draw case)."""
    toas, nu, segs, _, _ = D.make_case("m15", 20)
    G = D.basis_literal(toas, nu, segs)
    C = G @ G.T
    L = np.linalg.cholesky(C)
    fac = D.worst(D.factor_product(L) - C.astype(LD), D.factor_bound(L))
    print(f"numpy m15 n = 20, no white: cond {np.linalg.cond(C):.3g}, factor {fac:.3g}")
    assert fac < 1


def test_single_mode_closed_form():
    """One achromatic mode: C_ij = w cos(phi_i - phi_j) from the exact phase is cov_truth to longdouble rounding."""
    toas, nu, segs, _, _ = D.make_case("one", 65)
    ph = D.T.phase(segs[0][0], toas)[:, 0]
    closed = LD(segs[0][1][0]) * np.cos(ph[:, None] - ph[None, :])
    assert np.max(np.abs(closed - D.cov_truth(toas, nu, segs))) <= 8 * 2.0 ** -64 * segs[0][1][0]


# --------------------------------------------------------------------------- deliberate defects
def _spectrum_case(M, flat, n=100, seed=5):
    rng = np.random.default_rng(seed)
    toas = np.sort(D.T0 + D.SPAN * rng.random(n))
    nu = rng.choice(D.NUS, n)
    f = np.arange(1, M + 1) / D.SPAN
    w = np.full(M, D.AMP ** 2) if flat else O.powerlaw(f, -14.0, 4.5) * O.delta_f(f)
    segs = [(f, w, 0.0, D.FREQF)]
    return toas, nu, segs, D.basis_literal(toas, nu, segs)


def _cov_ratios(toas, nu, segs, G, Gd):
    truth, bound = D.cov_truth(toas, nu, segs), D.cov_bound(toas, nu, segs)
    return D.worst((G @ G.T).astype(LD) - truth, bound), D.worst((Gd @ Gd.T).astype(LD) - truth, bound)


def test_defect_a_scaled_top_sin_column():
    """The top mode's sin column times 1 + 1e-9, 30 modes (module docstring)."""
    toas, nu, segs, G = _spectrum_case(30, flat=False)
    Gd = G.copy()
    Gd[:, -1] *= 1 + 1e-9
    assert_parity(Gd @ Gd.T, G @ G.T, 1e-10)  # the old check passes it on the red spectrum
    good, bad = _cov_ratios(toas, nu, segs, G, Gd)
    print(f"(a) red: parity {rel_err(Gd @ Gd.T, G @ G.T):.3g}, cov_bound {good:.3g} -> {bad:.3g}; the defect is "
          f"{1e-9 * segs[0][1][-1] / (EPS * segs[0][1][0]):.3g} eps of the first mode's term")
    assert good < 1
    # on the red spectrum the defect is a rounding of the first mode's term, 1 / 60 of what a 60-term dot product is
    # allowed: nothing sound can see it there, and numpy's own rounding (good) is ten times larger
    assert 1e-9 * segs[0][1][-1] < 0.02 * 62 * EPS * segs[0][1][0] and abs(bad - good) < 0.05
    toas, nu, segs, G = _spectrum_case(30, flat=True)
    Gd = G.copy()
    Gd[:, -1] *= 1 + 1e-9
    good, bad = _cov_ratios(toas, nu, segs, G, Gd)
    print(f"(a) flat: parity {rel_err(Gd @ Gd.T, G @ G.T):.3g}, cov_bound {good:.3g} -> {bad:.3g}")
    assert good < 1 < 100 < bad


@pytest.mark.parametrize("M", [15, 171])
def test_defect_b_dropped_last_sin_row(M):
    """The last mode's sin row lost, 2 M % 4 == 2 (the row next to k_cov_basis's padded pair), gamma = 4.5."""
    assert 2 * M % 4 == 2
    toas, nu, segs, G = _spectrum_case(M, flat=False)
    Gd = G.copy()
    Gd[:, -1] = 0.0
    good, bad = _cov_ratios(toas, nu, segs, G, Gd)
    par = rel_err(Gd @ Gd.T, G @ G.T)
    print(f"(b) M = {M}: parity {par:.3g} (w_M / w_1 = {segs[0][1][-1] / segs[0][1][0]:.3g}), cov_bound {good:.3g} "
          f"-> {bad:.3g}")
    assert good < 1 < 100 < bad
    if M == 171:
        assert_parity(Gd @ Gd.T, G @ G.T, 1e-10)  # the old check passes it
    else:
        assert par > 1e-10  # at 15 modes the old check does see it: w_15 / w_1 = 5e-6


@pytest.mark.parametrize("n", [65, 321])
def test_defect_c_one_factor_element(n):
    """L[n - 1][0] off by 1e-12 relative moves (L L^T)[n - 1][0] by 1e-12 |L[n - 1][0] L[0][0]|, and the allowance
    there is 4 eps of the same product."""
    _, C, L, _ = numpy_stages("m15", n)
    Ld = L.copy()
    Ld[n - 1, 0] *= 1 + 1e-12
    assert Ld[n - 1, 0] != L[n - 1, 0]
    good = D.worst(D.factor_product(L) - C.astype(LD), D.factor_bound(L))
    bad = D.worst(D.factor_product(Ld) - C.astype(LD), D.factor_bound(Ld))
    Lk = L.copy()
    Lk[n - 1, n - 1] *= 1 + 1e-12
    diag = D.worst(D.factor_product(Lk) - C.astype(LD), D.factor_bound(Lk))
    print(f"(c) n = {n}: factor_bound {good:.3g} -> {bad:.3g} (the last diagonal element instead: {diag:.3g})")
    assert good < 1 < 1000 < bad


@pytest.mark.parametrize("n", [65, 321])
def test_defect_d_one_substitution_term(n):
    toas, nu, segs, white, r = D.make_case("m15", n)
    _, C, L, y = numpy_stages("m15", n)
    yd = backward(L, forward(L, r, skip=(n - 1, n // 2)))
    res = lambda v: r.astype(LD) - C.astype(LD) @ v.astype(LD)  # noqa: E731
    good, bad = D.worst(res(y), D.solve_bound(L, y)), D.worst(res(yd), D.solve_bound(L, yd))
    print(f"(d) n = {n}: solve_bound {good:.3g} -> {bad:.3g}")
    assert good < 1 < 100 < bad
