"""The correlated likelihood grid's definition (include/fakepta_amd.h) in np.longdouble with index-order sums, for the
tests of csrc/clnl_host.h and csrc/clnl.hip, in two forms: the formula (T, V, C_g = I + D_g T D_g, a Cholesky factor and
a forward substitution) and the literal form (the dense stacked covariance blockdiag(P0_p) + F (Gamma (x) phi) F^T on
the null space of the designs, a Cholesky factor and the difference of the log densities). B0 and Z come from
tests/lnl_reference.py (the target left out of the base model)."""
import numpy as np

from tests.ld_reference import LD, EPS
from tests.fit_reference import _sum
from tests import lnl_reference as LR
from tests import os_reference as OS
from tests import test_os_host as H
from tests import tm_reference as T
from tests.tm_reference import basis_ld

YEAR = H.YEAR


def arrays():
    """The arrays of the CPU tests, in tests/test_os_host.arrays()'s format with every component on one grid for the
    array: 3 pulsars of 17 / 33 / 40 TOAs with a target of N = 2 and of N = 3 modes, and 5 pulsars of 0, 12, 25, 40
    and 60 TOAs with N = 7 (n = 70: two 64-row blocks, the second ragged). A red process of 3 modes per pulsar and a
    design of 3 columns beside the target."""
    rng = np.random.default_rng(20262)
    span = 15 * YEAR
    out = {}
    for name, counts, N in (("P3N2", (17, 33, 40), 2), ("P3N3", (17, 33, 40), 3), ("P5N7", (0, 12, 25, 40, 60), 7)):
        ps = []
        for n in counts:
            t, nu, M, w = H._pulsar(rng, n)
            ps.append((t, nu, M[:, :3].copy() if n else np.zeros((0, 3)), w))
        ref = ps[-1][3]
        phi_rn = np.stack([H._spectrum(30.0, p[3], 3, 3.0) if len(p[0]) else np.ones(3) for p in ps])
        phi_gw = np.stack([H._spectrum(5.0, ref, N)] * len(ps))
        out[name] = dict(psrs=ps, comps=[(np.arange(1, 4) / span, 0.0, 1400.0), (np.arange(1, N + 1) / span, 0.0, 1400.0)],
                         phis=[phi_rn, phi_gw], masks=None, target=1)
    return out


def grid_of(arr):
    """[4, N]: the target's own spectrum, an all-zero row, 10 x it with every third mode zero, and a steeper one."""
    base = np.asarray(arr["phis"][arr["target"]])[-1].copy()
    N = len(base)
    g = np.stack([base, np.zeros(N), 10.0 * base, 0.1 * base * np.arange(1, N + 1) ** 1.5])
    g[2, ::3] = 0.0
    return g


def positions(P, seed=5):
    v = np.random.default_rng(seed).normal(size=(P, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def orfs_of(P, seed=5):
    """name -> Gamma [P, P]: Hellings-Downs of random positions, the monopole (rank 1), a random SPD matrix and the
    identity."""
    from oracle import fakepta_oracle as O
    rng = np.random.default_rng(seed + 1)
    B = rng.normal(size=(P, P))
    return dict(hd=np.asarray(O.orf_hd(positions(P, seed)), dtype=np.float64), monopole=np.ones((P, P)),
                spd=B @ B.T / P + 0.1 * np.eye(P), identity=np.eye(P))


def factor_of(gamma):
    """A with A A^T = Gamma as the package makes it (batch.batch_factor)."""
    from fakepta_amd.batch import batch_factor
    return np.ascontiguousarray(batch_factor(np.asarray(gamma, dtype=np.float64)))


_BASE = {}


def base_of(name):
    """Per pulsar (B0, Z, keep) of the longdouble definition with the target left out, once per array."""
    if name not in _BASE:
        arr = arrays()[name]
        offs, toas, nu, Mmats, w, comps_of, phis_of, masks_of = H.array_tables(arr)
        per = []
        for p in range(len(offs) - 1):
            sl = slice(int(offs[p]), int(offs[p + 1]))
            B, Z, norms, keep = LR.base_operator(toas[sl], nu[sl], Mmats[p], w[sl], comps_of(p), phis_of(p),
                                                 arr["target"], masks_of(p))
            T.assert_clear_rank(norms, keep, Mmats[p])
            per.append((B, Z, keep))
        _BASE[name] = per
    return _BASE[name]


def residuals_of(arr, R, seed=3):
    """[R, n_toa]: white draws at three times each TOA's noise level."""
    w = np.concatenate([p[3] for p in arr["psrs"]])
    return 3.0 * np.random.default_rng(seed).normal(size=(R, len(w))) / np.sqrt(w)


def t_matrix(Zs, A):
    """T [n, n] longdouble, T[(i,k),(j,l)] = sum_p A_pi A_pj Z_p[k,l] in pulsar order; Z_p's lower triangle is read."""
    P, K = len(Zs), len(Zs[0])
    A = np.asarray(A, dtype=np.float64).astype(LD)
    Zs = [np.tril(np.asarray(Z)) + np.tril(np.asarray(Z), -1).T for Z in Zs]
    Tm = np.zeros((P * K, P * K), dtype=LD)
    for i in range(P):
        for j in range(P):
            acc = np.zeros((K, K), dtype=LD)
            for p in range(P):
                acc = acc + (A[p, i] * A[p, j]) * Zs[p]
            Tm[i * K:(i + 1) * K, j * K:(j + 1) * K] = acc
    return Tm


def scale_of(phi_g, P):
    """s [n] longdouble: sqrt(phi) per column (cosines then sines), tiled over the pulsars."""
    ph = np.asarray(phi_g, dtype=np.float64)
    return np.tile(np.sqrt(np.concatenate([ph, ph]).astype(LD)), P)


def mix(A, Xs):
    """V [n, R] longdouble, V[(j,l)] = sum_p A_pj X_p[l] in pulsar order, and the dot-product bound of an fp64
    evaluation, (P + 2) eps sum_p |A_pj| |X_p[l]|."""
    P, K = len(Xs), len(Xs[0])
    A = np.asarray(A, dtype=np.float64).astype(LD)
    X = np.stack([np.asarray(x).astype(LD) for x in Xs])  # [P, K, R]
    V = np.zeros((P * K,) + X.shape[2:], dtype=LD)
    mag = np.zeros(V.shape, dtype=LD)
    for j in range(P):
        for p in range(P):
            V[j * K:(j + 1) * K] += A[p, j] * X[p]
            mag[j * K:(j + 1) * K] += np.abs(A[p, j]) * np.abs(X[p])
    return V, ((P + 2) * EPS * mag).astype(np.float64)


def solve_lower(L, b):
    y = np.zeros_like(b)
    for i in range(len(L)):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    return y


def factor(Tm, s):
    """(L longdouble, ld longdouble, cond_2(C) as float) of one ORF and grid point: C = I + D T D = L L^T, ld = 2 sum
    ln L_ii; the condition number from numpy's eigenvalues of C."""
    s = np.asarray(s).astype(LD)
    C = s[:, None] * np.asarray(Tm).astype(LD) * s[None, :] + np.eye(len(s), dtype=LD)
    L = LR.cholesky_ld(C)
    w = np.linalg.eigvalsh(C.astype(np.float64))
    return L, 2 * _sum(np.log(np.diag(L))), float(w[-1] / w[0])


def quad(L, s, V):
    """q [R] longdouble = |L^-1 D V|^2, the squares added in row order."""
    y = solve_lower(L, np.asarray(s).astype(LD)[:, None] * np.asarray(V).astype(LD))
    q = np.zeros(y.shape[1], dtype=LD)
    for i in range(len(y)):
        q = q + y[i] * y[i]
    return q


def point(Tm, s, V):
    """(q [R] longdouble, ld longdouble, cond_2(C) as float) of one ORF and grid point."""
    L, ld, cond = factor(Tm, s)
    return quad(L, s, V), ld, cond


def dlnl_formula(Zs, Xs, A, grid):
    """dlnL [G, R] longdouble of one ORF factor A by the formula."""
    Tm, (V, _) = t_matrix(Zs, A), mix(A, Xs)
    out = []
    for row in np.atleast_2d(grid):
        q, ld, _ = point(Tm, scale_of(row, len(Zs)), V)
        out.append((q - ld) / 2)
    return np.stack(out)


def null_basis(M, keep):
    """N [n, n - m] longdouble, orthonormal, N^T M = 0 for M's kept columns (lnl_reference.literal_dlnl's)."""
    n = len(M)
    if M is None or not np.any(keep):
        return np.eye(n, dtype=LD)
    Mk = np.asarray(M, dtype=np.float64)[:, keep]
    Qm, _, kq = basis_ld(Mk)
    assert np.all(kq)
    u, _, _ = np.linalg.svd(Mk / np.linalg.norm(Mk, axis=0), full_matrices=True)
    cols = []
    for v in u[:, Mk.shape[1]:].T.astype(LD):
        for _ in range(2):
            for q in list(Qm.T) + cols:
                v = v - _sum(q * v) * q
        cols.append(v / np.sqrt(_sum(v * v)))
    return np.stack(cols, axis=1)


def dlnl_literal(arr, keeps, A, grid, r):
    """ln p(r | Gamma, phi_g) - ln p(r | phi = 0) [G, R] by the literal dense form in longdouble, Gamma = A A^T formed
    in longdouble: S(phi) = blockdiag(P0_p) + F (Gamma (x) diag(phi, phi)) F^T with F = blockdiag(F_p), restricted to
    the null space of blockdiag(M_p)'s kept columns, a Cholesky factor, and -(r^T S^-1 r + ln det S) / 2."""
    offs, toas, nu, Mmats, w, comps_of, phis_of, masks_of = H.array_tables(arr)
    P, n_toa, tgt = len(offs) - 1, int(offs[-1]), arr["target"]
    A = np.asarray(A, dtype=np.float64).astype(LD)
    gam = A @ A.T
    N = len(comps_of(0)[tgt][0])
    K = 2 * N
    S0 = np.zeros((n_toa, n_toa), dtype=LD)
    F = np.zeros((n_toa, P * K), dtype=LD)
    Nn = np.zeros((n_toa, 0), dtype=LD)
    for p in range(P):
        sl = slice(int(offs[p]), int(offs[p + 1]))
        t, v, n = toas[sl], nu[sl], int(offs[p + 1] - offs[p])
        comps, phis = comps_of(p), phis_of(p)
        masks = masks_of(p) or [None] * len(comps)
        blk = np.diag(1 / w[sl].astype(LD))
        for c in range(len(comps)):
            f = np.asarray(comps[c][0], dtype=np.float64)
            Fc = np.stack([OS.column_ld(t, v, f, comps[c][1], comps[c][2], k, len(f), masks[c])
                           for k in range(2 * len(f))], axis=1) if n else np.zeros((0, 2 * len(f)), dtype=LD)
            if c == tgt:
                F[sl, p * K:(p + 1) * K] = Fc
            else:
                ph = np.concatenate([phis[c], phis[c]]).astype(np.float64).astype(LD)
                blk = blk + (Fc * ph[None, :]) @ Fc.T
        S0[sl, sl] = blk
        Np = null_basis(Mmats[p], keeps[p]) if n else np.zeros((0, 0), dtype=LD)
        full = np.zeros((n_toa, Np.shape[1]), dtype=LD)
        full[sl] = Np
        Nn = np.concatenate([Nn, full], axis=1)
    rn = np.atleast_2d(np.asarray(r, dtype=np.float64)).astype(LD) @ Nn

    def lnp(S):
        L = LR.cholesky_ld(Nn.T @ S @ Nn)
        y = solve_lower(L, rn.T)
        return -(np.sum(y * y, axis=0) + 2 * _sum(np.log(np.diag(L)))) / 2

    base = lnp(S0)
    out = []
    for row in np.atleast_2d(grid):
        ph = np.asarray(row, dtype=np.float64).astype(LD)
        prior = np.kron(gam, np.diag(np.concatenate([ph, ph])))
        out.append(lnp(S0 + F @ prior @ F.T) - base)
    return np.stack(out)
