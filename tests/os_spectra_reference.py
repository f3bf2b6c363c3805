"""Truth and yardstick of the optimal statistic under a spectrum per realization (include/fakepta_amd.h), for
tests/test_os_spectra_host.py and tests/test_gpu_os_spectra.py. Test infrastructure only; not a test and not a
conftest.

The truth of a realization is tests/os_reference.py's operator_ld, the np.longdouble definition of the fixed
statistic, evaluated with that realization's prior variances: B_p^(r), X = B r, Z and pair_norms, every sum in index
order. plan_ld is the definition of what the host plans once per pulsar, B0 = T^T P0^-1 and A = B0 T: operator_ld with
every varied mode's prior variance set to 0 (the projection form), once per varied component as its target.
literal is the literal fp64 evaluation of the coefficient-space route, np.linalg.solve on Phi^-1 + A over the columns
with phi > 0: X = Phi^-1 (Phi^-1 + A)^-1 z and Z = A - A (Phi^-1 + A)^-1 A. Its distance from the truth is one term of
a tolerance (os_reference.x_tolerance), the other is (q + 2) eps cond_1(C) max |.| with C = I + s A s."""
import numpy as np

from tests import os_reference as OS
from tests.ld_reference import LD, EPS  # noqa: F401
from tests.fit_reference import _sum


def zeroed(phis, vary):
    """The prior variances with every mode of the varied components set to 0."""
    return [np.zeros_like(np.asarray(ph, dtype=np.float64)) if c in vary else np.asarray(ph, dtype=np.float64)
            for c, ph in enumerate(phis)]


def varied_columns(t, nu, comps, vary, masks=None):
    """T [n, q] longdouble: the Fourier columns of the varied components in the order of `vary`."""
    masks = [None] * len(comps) if masks is None else masks
    cols = []
    for c in vary:
        f, idx, freqf = comps[c]
        f = np.asarray(f, dtype=np.float64)
        cols += [OS.column_ld(t, nu, f, idx, freqf, k, len(f), masks[c]) for k in range(2 * len(f))]
    return np.stack(cols, axis=1) if cols else np.zeros((len(t), 0), dtype=LD)


def plan_ld(t, nu, M, w, comps, phis, vary, masks=None):
    """(B0 [q, n] longdouble, A [q, q] longdouble, orthogonalised norms of M's columns, kept) of one pulsar."""
    ph0 = zeroed(phis, vary)
    rows, norms, keep = [], None, None
    for c in vary:
        B, _, norms, keep = OS.operator_ld(t, nu, M, w, comps, ph0, c, masks, need_z=False)
        rows.append(B)
    B0 = np.concatenate(rows, axis=0)
    Tm = varied_columns(t, nu, comps, vary, masks)
    q = len(B0)
    A = np.zeros((q, q), dtype=LD)
    for j in range(q):
        for i in range(j, q):
            A[i, j] = A[j, i] = _sum(B0[i] * Tm[:, j])
    return B0, A, norms, keep


def with_rows(phis, vary, phi_r):
    """The prior variances of one realization: phi_r[v] [N_c] replaces component vary[v]'s."""
    out = [np.asarray(ph, dtype=np.float64) for ph in phis]
    for v, c in enumerate(vary):
        out[c] = np.asarray(phi_r[v], dtype=np.float64)
    return out


def realization_truth(t, nu, M, w, comps, phis, vary, phi_r, masks=None, need_z=True):
    """(B [K, n], Z [K, K]) longdouble of one realization: operator_ld under its own prior variances (the target is
    the last of vary)."""
    B, Z, _, _ = OS.operator_ld(t, nu, M, w, comps, with_rows(phis, vary, phi_r), vary[-1], masks, need_z=need_z)
    return B, Z


def columns_phi(phi_r):
    """[q]: the prior variance of every column of the varied set (cosines, then sines, per component)."""
    return np.concatenate([np.concatenate([np.asarray(p, dtype=np.float64)] * 2) for p in phi_r])


def literal(A, z, phi_q, K):
    """(X [K, n_vec], Z [K, K]) in fp64 from A [q, q], z [q, n_vec] and the columns' prior variances: the solve on
    Phi^-1 + A over the columns with phi > 0; a target column with phi = 0 takes z - A Phi (..) z and A - A (..) A."""
    A = np.asarray(A, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64).reshape(len(A), -1)
    q = len(A)
    on = phi_q > 0
    S = np.diag(1.0 / phi_q[on]) + A[np.ix_(on, on)]
    sol_z = np.linalg.solve(S, z[on]) if on.any() else np.zeros((0, z.shape[1]))
    sol_A = np.linalg.solve(S, A[on][:, q - K:]) if on.any() else np.zeros((0, K))
    X = z[q - K:] - A[q - K:][:, on] @ sol_z
    Z = A[q - K:, q - K:] - A[q - K:][:, on] @ sol_A
    return X, Z


def cond1(A, phi_q):
    """cond_1 of C = I + s A s, s = sqrt(phi), in fp64."""
    s = np.sqrt(np.asarray(phi_q, dtype=np.float64))
    C = np.eye(len(s)) + s[:, None] * np.asarray(A, dtype=np.float64) * s[None, :]
    return float(np.linalg.cond(C, 1))


def scaled(Z, phi_hat):
    """Z' = phi_hat^(1/2) Z phi_hat^(1/2) over the K columns."""
    h = np.sqrt(np.concatenate([phi_hat, phi_hat]).astype(np.float64).astype(LD))
    return h[:, None] * Z * h[None, :]


def gram_ld(Zp):
    """(N [P, P] longdouble for a >= b, the sum of the absolute terms) of Z' [P, K, K]: sum_jk Z'_a,jk Z'_b,jk."""
    Zl = np.asarray(Zp).astype(LD).reshape(len(Zp), -1)
    P = len(Zl)
    nab, mag = np.zeros((P, P), dtype=LD), np.zeros((P, P), dtype=LD)
    for a in range(P):
        for b in range(a + 1):
            nab[a, b] = _sum(Zl[a] * Zl[b])
            mag[a, b] = _sum(np.abs(Zl[a] * Zl[b]))
    return nab, mag


def contractions_ld(G, nab, n_orf):
    """(norm [J], joint [n_orf, n_orf], and the sums of the absolute terms of each) from N [P, P] (a > b read), row-major
    over the pairs a > b, longdouble."""
    P = nab.shape[0]
    ia, ib = np.tril_indices(P, -1)
    g = np.asarray(G, dtype=np.float64)[:, ia, ib].astype(LD)
    n = np.asarray(nab)[ia, ib].astype(LD)
    norm = np.array([_sum(gj * gj * n) for gj in g], dtype=LD)
    norm_mag = np.array([_sum(np.abs(gj * gj * n)) for gj in g], dtype=LD)
    joint = np.array([[_sum(g[i] * g[j] * n) for j in range(n_orf)] for i in range(n_orf)], dtype=LD).reshape(n_orf, n_orf)
    joint_mag = np.array([[_sum(np.abs(g[i] * g[j] * n)) for j in range(n_orf)] for i in range(n_orf)],
                         dtype=LD).reshape(n_orf, n_orf)
    return norm, norm_mag, joint, joint_mag
