"""Longdouble truths and allowances for the dense-covariance path (csrc/dense.hip, dense_build / dense_cholesky in
csrc/capi.hip), stage by stage. Test infrastructure only, like tests/ld_reference.py: not a test and not a conftest.

Every function takes the fp64 inputs exactly as the C ABI receives them: toas [n], nu [n], segments = list of (f [N],
w = psd df [N], idx, freqf) in the order of Context.gp_covariance, white [n] or None. Column 2 m of the basis is mode
m's cosine, column 2 m + 1 its sine, modes numbered through the segments in order (k_cov_basis's rows).

None of the allowances is measured on the code under test. eps = 2^-52 throughout (the unit roundoff is eps / 2, so a
bound written `k eps` is twice Higham's gamma_k: the factor-2 slack of tests/test_gpu_reductions.py).

  basis element: |device - truth| <= E = 4 |literal - truth| + 4 eps a, a = ch sqrt(w): the project's rule for one
    basis element (tests/test_gpu_mode_response.py "exact", tests/test_gpu_dropin_shapes.py). The kernel forms the
    literal's phase fl(fl(2 pi f) t); its sincos, pow and square root are a few ulp.
  covariance (cov_bound): with Ghat = G + dG, |dG| <= E, fl(Ghat Ghat^T) - G G^T = dG Ghat^T + G dG^T + the rounding of
    a dot product of 2 M terms in any order, (2 M + 2) eps |G| |G|^T, + eps white_i for the diagonal's one addition.
  factor (factor_bound): |C - Lhat Lhat^T|_ij <= (min(i, j) + 4) eps (|Lhat| |Lhat|^T)_ij, i and j from 0: Higham,
    Accuracy and Stability of Numerical Algorithms, theorem 10.3 in its componentwise form, where element (i, j) is a
    sum of min(i, j) + 1 products whatever the order (64-wide panels, MFMA trailing update). + 4 for the square root,
    k_trsm_panel's reciprocal and its product, and one subtraction per panel.
  solve (solve_bound): |r - C yhat| <= 2 (n + 2) eps |Lhat| |Lhat|^T |yhat|: (Lhat + d1) u = r, (Lhat^T + d2) yhat = u
    with |d| <= gamma_n |Lhat| each (Higham theorem 8.5), and C = Lhat Lhat^T + the factor's backward error.
  draws (draw_bound): X[r][t] = sum_{k <= t} Z[r][k] L[t][k], t + 1 products: (t + 3) eps sum_k |Z[r][k] L[t][k]|.

tests/test_dense_reference.py pins cov_truth to the reference's recorded matrices (fixture G6), keeps numpy's fp64
evaluation inside every allowance and shows that deliberate defects fall outside."""
import functools
from types import SimpleNamespace

import numpy as np

from tests import ld_reference as T

LD = np.longdouble
EPS = T.EPS


def _segments(segments):
    out = []
    for f, w, idx, freqf in segments:
        f, w = T._f64(np.asarray(f)), T._f64(np.asarray(w))
        assert f.ndim == 1 and f.shape == w.shape and np.all(w >= 0.0)
        out.append((f, w, float(idx), float(freqf)))
    return out


def amplitude(nu, segments):
    """a = ch sqrt(w) [n, 2 M] in longdouble, ch = (freqf / nu)^idx."""
    cols = []
    for f, w, idx, freqf in _segments(segments):
        a = T.chromatic(freqf, nu, idx)[:, None] * np.sqrt(w.astype(LD))[None, :]
        cols.append(np.repeat(a, 2, axis=1))
    return np.concatenate(cols, axis=1)


def basis_truth(toas, nu, segments):
    """G [n, 2 M] in longdouble: ld_reference.mode_truth (exact phase) times sqrt(w)."""
    cols = []
    for f, w, idx, freqf in _segments(segments):
        m = T.mode_truth(f, toas, nu, idx, freqf)  # [n, N, 2]
        cols.append((m * np.sqrt(w.astype(LD))[None, :, None]).reshape(len(toas), 2 * len(f)))
    return np.concatenate(cols, axis=1)


def basis_literal(toas, nu, segments):
    """The fp64 evaluation fl(ch sqrt(w)) cos / sin(fl(fl(2 pi f) t)) [n, 2 M], every operation rounded to fp64."""
    toas, nu = T._f64(toas), T._f64(nu)
    cols = []
    for f, w, idx, freqf in _segments(segments):
        ch = np.ones_like(nu) if idx == 0.0 else (freqf / nu) ** idx
        a = ch[:, None] * np.sqrt(w)[None, :]
        ph = toas[:, None] * (2.0 * np.pi * f)[None, :]
        cols.append(np.stack([a * np.cos(ph), a * np.sin(ph)], axis=2).reshape(len(toas), 2 * len(f)))
    return np.concatenate(cols, axis=1)


def cov_truth(toas, nu, segments, white=None):
    """G G^T (+ diag white) [n, n] in longdouble."""
    G = basis_truth(toas, nu, segments)
    C = G @ G.T
    if white is not None:
        C[np.diag_indices(len(C))] += T._f64(white).astype(LD)
    return C


def element_bound(toas, nu, segments):
    """E [n, 2 M]: the allowance of one basis element, 4 |literal - truth| + 4 eps a."""
    G = basis_truth(toas, nu, segments)
    lit = basis_literal(toas, nu, segments).astype(LD)
    return 4 * np.abs(lit - G) + 4 * LD(EPS) * amplitude(nu, segments)


def cov_bound(toas, nu, segments, white=None):
    """Element-wise allowance [n, n] of |device covariance - cov_truth| (module docstring)."""
    Ga = np.abs(basis_truth(toas, nu, segments))
    E = element_bound(toas, nu, segments)
    EG = E @ Ga.T
    B = EG + EG.T + LD((Ga.shape[1] + 2) * EPS) * (Ga @ Ga.T)
    if white is not None:
        B[np.diag_indices(len(B))] += LD(EPS) * np.abs(T._f64(white).astype(LD))
    return B


def _lower(Lhat):
    L = np.tril(T._f64(Lhat)).astype(LD)
    assert L.ndim == 2 and L.shape[0] == L.shape[1]
    return L


def factor_product(Lhat):
    """tril(Lhat) tril(Lhat)^T in longdouble."""
    L = _lower(Lhat)
    return L @ L.T


def factor_bound(Lhat):
    """Element-wise allowance [n, n] of |C - Lhat Lhat^T| for the computed Cholesky factor of C."""
    La = np.abs(_lower(Lhat))
    i = np.arange(len(La))
    return (np.minimum(i[:, None], i[None, :]) + 4).astype(LD) * LD(EPS) * (La @ La.T)


def solve_bound(Lhat, yhat):
    """Allowance [n] of |r - C yhat| for yhat from two substitutions on the computed factor."""
    La = np.abs(_lower(Lhat))
    n = len(La)
    return LD(2 * (n + 2) * EPS) * (La @ (La.T @ np.abs(T._f64(yhat).astype(LD))))


def draw_product(Zhat, Lhat):
    """Z tril(Lhat)^T [R, n] in longdouble, Zhat [R, n]."""
    return T._f64(Zhat).astype(LD) @ _lower(Lhat).T


def draw_bound(Zhat, Lhat):
    """Allowance [R, n] of |X - Zhat Lhat^T|, Zhat [R, n]."""
    La = np.abs(_lower(Lhat))
    t = np.arange(len(La))
    return (t + 3).astype(LD)[None, :] * LD(EPS) * (np.abs(T._f64(Zhat).astype(LD)) @ La.T)


def worst(err, bound):
    """max err / bound over the elements (0 / 0 counts as 0; anything over a zero allowance as inf)."""
    err, bound = np.abs(np.asarray(err, dtype=LD)), np.asarray(bound, dtype=LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, LD(0), err / bound)
    return float(np.max(ratio)) if ratio.size else 0.0


# --------------------------------------------------------------------------- the GPU test's inputs
# (tests/test_gpu_dense_kernels.py; tests/test_dense_reference.py runs numpy's fp64 on the same ones)
T0, SPAN = 4.5e9, 3.15e8  # real-MJD-like epochs [s]
NUS = (800.0, 1400.0, 2500.0)
FREQF = 1400.0
AMP = 1e-7
MODE_SETS = {
    "one": ((1, 0.0),),
    "idx1": ((3, 1.0),),
    "m15": ((7, 0.0), (5, 2.0), (3, 4.0)),  # 2 M % 4 == 2: one padded basis row pair
    "m12": ((8, 0.0), (4, 2.5)),
}
SIZES = (1, 2, 63, 64, 65, 128, 256, 257, 321, 384)
CASES = [("m15", n) for n in SIZES] + [(name, n) for name in ("one", "idx1", "m12") for n in (1, 65, 321)]


def segments_of(modes):
    """Signals on f_k = k / SPAN with the flat weight w = AMP^2, so that no mode hides behind another."""
    return [(np.arange(1, nm + 1) / SPAN, np.full(nm, AMP ** 2), float(idx), FREQF) for nm, idx in modes]


def _frozen(a):
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def make_case(name, n):
    """(toas, nu, segments, white, r) of one (mode set, size): computed once, shared and read-only."""
    rng = np.random.default_rng([n, sorted(MODE_SETS).index(name)])
    toas = np.sort(T0 + SPAN * rng.random(n))
    nu = rng.choice(NUS, n)
    white = (AMP * rng.uniform(0.5, 2.0, n)) ** 2
    r = AMP * rng.standard_normal(n)
    segs = [tuple(_frozen(x) if isinstance(x, np.ndarray) else x for x in s) for s in segments_of(MODE_SETS[name])]
    return _frozen(toas), _frozen(nu), segs, _frozen(white), _frozen(r)


@functools.lru_cache(maxsize=None)
def case_reference(name, n):
    """The covariance truth and allowance of make_case(name, n), without (truth0, bound0) and with the white diagonal
    (truth, bound): computed once, shared and read-only."""
    toas, nu, segs, white, _ = make_case(name, n)
    truth0, bound0 = cov_truth(toas, nu, segs), cov_bound(toas, nu, segs)
    return SimpleNamespace(truth0=_frozen(truth0), bound0=_frozen(bound0),
                           truth=_frozen(cov_truth(toas, nu, segs, white)),
                           bound=_frozen(cov_bound(toas, nu, segs, white)))
