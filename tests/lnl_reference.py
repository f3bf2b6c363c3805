"""The likelihood grid's definition (include/fakepta_amd.h) in np.longdouble with index-order sums, for the tests of
csrc/lnl_host.h and csrc/lnl.hip. B0 = F^T P0^-1 and Z come from tests/os_reference.py with the target's phi set to 0
(the target is not part of the base model); this file adds the per-grid-point factor, the quadratic form, the bounds of
the device's fp64 evaluation, and the literal dense form for tiny pulsars."""
import numpy as np

from tests.ld_reference import LD, EPS
from tests.fit_reference import _sum
from tests import os_reference as OS
from tests.tm_reference import basis_ld


def base_operator(t, nu, M, w, comps, phis, target, masks=None, rcond=None):
    """(B0 [K, n], Z [K, K], norms, keep) of one pulsar in longdouble: os_reference.operator_ld with the target's prior
    variances zeroed."""
    phis0 = [np.zeros_like(np.asarray(ph, dtype=np.float64)) if c == target else ph for c, ph in enumerate(phis)]
    return OS.operator_ld(t, nu, M, w, comps, phis0, target, masks, rcond)


def cholesky_ld(C):
    """L (lower, longdouble) with C = L L^T, sums in index order, from C's lower triangle."""
    n = len(C)
    L = np.zeros((n, n), dtype=LD)
    for i in range(n):
        for j in range(i + 1):
            a = C[i, j] - _sum(L[i, :j] * L[j, :j])
            L[i, j] = np.sqrt(a) if i == j else a / L[j, j]
    return L


def factor_ld(Z, phi_g):
    """(U [K, K] longdouble lower triangular, ld, cond(C) as float) of one pulsar and grid point: C = I + s Z s with
    s = sqrt(phi) per column (cosines then sines), C = L L^T, U = L^-1 diag(s), ld = 2 sum ln L_ii."""
    K = len(Z)
    ph = np.asarray(phi_g, dtype=np.float64)
    assert ph.shape == (K // 2,)
    s = np.sqrt(np.concatenate([ph, ph]).astype(LD))
    C = s[:, None] * Z * s[None, :] + np.eye(K, dtype=LD)
    L = cholesky_ld(C)
    U = np.zeros((K, K), dtype=LD)
    for j in range(K):
        if s[j] == 0:
            continue
        U[j, j] = s[j] / L[j, j]
        for i in range(j + 1, K):
            U[i, j] = -_sum(L[i, j:i] * U[j:i, j]) / L[i, i]
    ld = 2 * _sum(np.log(np.diag(L)))
    return U, ld, float(np.linalg.cond(C.astype(np.float64)))


def grid_truth(Z, phi_grid):
    """(U [G, K, K], ld [G], cond [G]) of one pulsar."""
    out = [factor_ld(Z, row) for row in np.atleast_2d(phi_grid)]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out], dtype=LD), np.array([o[2] for o in out])


def quad(U, X):
    """(q [R] longdouble, allowance [R] of the device's fp64 evaluation) of one pulsar and grid point for U [K, K] and
    X [K, R]: with y_i = sum_k U_ik X_k and e_i = (K + 2) eps sum_k |U_ik| |X_k|, the allowance is
    sum_i (2 |y_i| e_i + e_i^2) + (K + 3) eps sum_i y_i^2."""
    U, X = np.asarray(U).astype(LD), np.asarray(X).astype(LD)
    K = len(U)
    y = U @ X
    e = (K + 2) * EPS * (np.abs(U) @ np.abs(X))
    q = np.sum(y * y, axis=0)
    return q, (np.sum(2 * np.abs(y) * e + e * e, axis=0) + (K + 3) * EPS * q).astype(np.float64)


def dlnl(Us, lds, Xs):
    """(dlnL [G, R] longdouble, q [P, G, R] longdouble, allowance of dlnL [G, R], allowance of q [P, G, R]) from per
    pulsar U [G, K, K], ld [G] and X [K, R]: dlnL = sum_p (q - ld) / 2 in pulsar order; the allowance is half the sum
    of q's over the pulsars plus (P + 3) eps sum_p (|q| + |ld|) / 2."""
    P, G, R = len(Us), len(Us[0]), np.shape(Xs[0])[1]
    q, qb = np.zeros((P, G, R), dtype=LD), np.zeros((P, G, R))
    for p in range(P):
        for g in range(G):
            q[p, g], qb[p, g] = quad(Us[p][g], Xs[p])
    ld = np.stack([np.asarray(v).astype(LD) for v in lds])  # [P, G]
    d = np.zeros((G, R), dtype=LD)
    for p in range(P):
        d = d + (q[p] - ld[p][:, None]) / 2
    mag = np.sum(np.abs(q) + np.abs(ld)[:, :, None], axis=0) / 2
    return d, q, (np.sum(qb, axis=0) / 2 + (P + 3) * EPS * mag).astype(np.float64), qb


def literal_dlnl(t, nu, M, w, comps, phis, target, phi_g, keep, r, masks=None):
    """ln p(r | phi_g) - ln p(r | phi = 0) of one (tiny) pulsar by the literal dense form, in longdouble: P(phi) = W^-1 +
    sum_{c != target} F_c Phi_c F_c^T + F Phi F^T restricted to the null space of M's kept columns (an orthonormal
    complement N from numpy's SVD, re-orthogonalised against M in longdouble), a Cholesky factor, and the difference
    of -(r^T N (N^T P N)^-1 N^T r + ln det N^T P N) / 2. r [R, n] or [n]. Returns [R]."""
    n = len(t)
    masks = [None] * len(comps) if masks is None else masks
    r = np.atleast_2d(np.asarray(r, dtype=np.float64)).astype(LD)
    wl = np.ones(n, dtype=LD) if w is None else np.asarray(w, dtype=np.float64).astype(LD)

    def block(c):
        f = np.asarray(comps[c][0], dtype=np.float64)
        return np.stack([OS.column_ld(t, nu, f, comps[c][1], comps[c][2], k, len(f), masks[c])
                         for k in range(2 * len(f))], axis=1)

    P0 = np.diag(1 / wl)
    for c in range(len(comps)):
        if c == target:
            continue
        ph = np.concatenate([phis[c], phis[c]]).astype(np.float64).astype(LD)
        F = block(c)
        P0 = P0 + (F * ph[None, :]) @ F.T
    Ft = block(target)
    pg = np.concatenate([phi_g, phi_g]).astype(np.float64).astype(LD)
    Pg = P0 + (Ft * pg[None, :]) @ Ft.T
    Nn = np.eye(n, dtype=LD)
    if M is not None and np.any(keep):
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
        Nn = np.stack(cols, axis=1)
    rn = r @ Nn  # [R, n - m]

    def lnp(Pm):
        L = cholesky_ld(Nn.T @ Pm @ Nn)
        y = np.zeros_like(rn.T)
        for i in range(len(L)):
            y[i] = (rn.T[i] - L[i, :i] @ y[:i]) / L[i, i]
        return -(np.sum(y * y, axis=0) + 2 * _sum(np.log(np.diag(L)))) / 2

    return lnp(Pg) - lnp(P0)
