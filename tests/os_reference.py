"""Truth and yardstick of the optimal statistic (include/fakepta_amd.h, 'optimal statistic'), for
tests/test_os_host.py and tests/test_gpu_os.py. Test infrastructure only; not a test and not a conftest.

operator_ld is the header's definition in np.longdouble: per pulsar the stacked matrix [W^(1/2) T ; D^(1/2)], T = [M,
the Fourier columns with phi > 0, the target's last], D = 0 on M's columns and 1 / phi on the others, its columns
scaled to unit norm and orthogonalised in order by modified Gram-Schmidt with one re-orthogonalisation; M's columns
follow the timing-model rank rule; then B = F^T P^-1 row by row from P^-1 T e_j = W^(1/2) Q1 R^-T e_j D_jj (a target
column with phi = 0: W^(1/2) (I - Q1 Q1^T) W^(1/2) F_k) and Z = B F. Every sum is taken in index order and every update
in the order written here, which is also how csrc/os_host.h works (tests/fit_reference.py says why that matters).
operator_literal is the literal fp64 numpy evaluation: P = W^-1 + F Phi F^T + 1e40 M M^T (M's kept columns scaled to
unit weighted norm) inverted through the Woodbury identity with np.linalg.solve. Its distance from the truth is one
term of the tolerance of X; the other is the rigorous bound of a length-n fp64 dot product in any order with a
once-rounded operator, (n + 2) eps sum_t |B_kt| |r_t|. q_truth is the pair sum Q of the
definition applied to given X, with the dot-product bound (n_terms + 3) eps sum |G| |phi_hat| |X_a| |X_b|."""
import numpy as np

from tests.ld_reference import LD, EPS  # noqa: F401  (the extended-precision assertion of ld_reference applies)
from tests.fit_reference import TWO_PI, _sum
from tests.tm_reference import RCOND, assert_clear_rank  # noqa: F401

TM_PRIOR = 1e40  # the literal form's prior variance of the timing model


def column_ld(t, nu, f, idx, freqf, k, N, mask=None):
    """Fourier column k (k < N: cosine of mode k, else sine of mode k - N) on TOAs t, longdouble, 0 off the mask."""
    t = np.asarray(t, dtype=np.float64).astype(LD)
    chrom = np.ones(len(t), dtype=LD) if idx == 0 else \
        (LD(np.float64(freqf)) / np.asarray(nu, dtype=np.float64).astype(LD)) ** LD(np.float64(idx))
    arg = TWO_PI * LD(np.float64(f[k if k < N else k - N])) * t
    col = chrom * (np.cos(arg) if k < N else np.sin(arg))
    if mask is not None:
        col = np.where(np.asarray(mask) != 0, col, LD(0))
    return col


def operator_ld(t, nu, M, w, comps, phis, target, masks=None, rcond=None, need_z=True):
    """(B [K, n] longdouble, Z [K, K] longdouble, orthogonalised norms of M's columns [m], kept [m] bool) of one
    pulsar. comps: list of (f [N_c], idx, freqf); phis: list of [N_c] prior variances; masks: None or a list of None /
    flags [n]; target: the index of the target component. need_z=False leaves Z zero (the GPU tests of X and Q do not
    read it)."""
    M = np.zeros((len(t), 0)) if M is None else np.asarray(M)
    assert M.dtype == np.float64 and M.ndim == 2 and M.shape[0] == len(t)
    n, m = M.shape
    masks = [None] * len(comps) if masks is None else masks
    rc = LD(RCOND if rcond is None or rcond <= 0 else rcond)
    s = np.ones(n, dtype=LD) if w is None else np.sqrt(np.asarray(w, dtype=np.float64).astype(LD))
    Nt = len(comps[target][0])
    K = 2 * Nt

    def col(c, k):
        f, idx, freqf = comps[c]
        return column_ld(t, nu, np.asarray(f, dtype=np.float64), idx, freqf, k, len(f), masks[c])

    cols = []  # the model's Fourier columns (component, column), the target's last
    for last in (False, True):
        for c, (f, _, _) in enumerate(comps):
            if (c == target) != last:
                continue
            Nc = len(f)
            cols += [(c, k) for k in range(2 * Nc) if np.float64(phis[c][k if k < Nc else k - Nc]) > 0]
    qa = len(cols)
    nc, L = m + qa, n + qa
    Q = np.zeros((nc, L), dtype=LD)
    R = np.zeros((nc, nc), dtype=LD)
    scale = np.zeros(nc, dtype=LD)
    kept_of = -np.ones(qa, dtype=np.int64)
    norms, keep = np.zeros(m, dtype=LD), np.zeros(m, dtype=bool)
    nk = 0

    def passes(v, proj):
        for _ in range(2):
            for q in range(nk):
                d = _sum(Q[q] * v)
                v = v - d * Q[q]
                if proj is not None:
                    proj[q] += d
        return v

    for j in range(nc):
        v = np.zeros(L, dtype=LD)
        if j < m:
            v[:n] = s * M[:, j].astype(LD)
        else:
            c, k = cols[j - m]
            Nc = len(comps[c][0])
            v[:n] = col(c, k) * s
            v[n + j - m] = LD(1) / np.sqrt(LD(np.float64(phis[c][k if k < Nc else k - Nc])))
        nrm2 = _sum(v * v)
        if not nrm2 > 0:
            continue
        cn = np.sqrt(nrm2)
        v = v * (LD(1) / cn)
        proj = np.zeros(nk, dtype=LD)
        v = passes(v, proj)
        nrm = np.sqrt(_sum(v * v))
        if j < m:
            norms[j] = nrm
            if not nrm > rc:
                continue
            keep[j] = True
        else:
            kept_of[j - m] = nk
        Q[nk] = v / nrm
        R[:nk, nk] = proj
        R[nk, nk] = nrm
        scale[nk] = cn
        nk += 1
    B = np.zeros((K, n), dtype=LD)
    a = sum(1 for c, _ in cols if c != target)
    ft = comps[target][0]
    for k in range(K):
        ph = np.float64(phis[target][k if k < Nt else k - Nt])
        if ph > 0:
            jj = int(kept_of[a])
            a += 1
            y = np.zeros(nk, dtype=LD)
            y[jj] = LD(1) / R[jj, jj]
            for i in range(jj + 1, nk):
                y[i] = -_sum(R[jj:i, i] * y[jj:i]) / R[i, i]
            acc = np.zeros(n, dtype=LD)
            for i in range(jj, nk):
                acc = acc + y[i] * Q[i, :n]
            B[k] = s * acc * ((LD(1) / LD(ph)) / scale[jj])
        else:
            v = np.zeros(L, dtype=LD)
            v[:n] = col(target, k) * s
            v = passes(v, None)
            B[k] = s * v[:n]
    Z = np.zeros((K, K), dtype=LD)
    for j in range(K if need_z else 0):
        Fj = col(target, j)
        for k in range(K):
            Z[k, j] = _sum(B[k] * Fj)
    assert len(ft) == Nt
    return B, Z, norms, keep


def operator_literal(t, nu, M, w, comps, phis, target, keep, masks=None):
    """B [K, n] in fp64: F^T P^-1 through the Woodbury identity, P^-1 = W - W T (Phi_T^-1 + T^T W T)^-1 T^T W with
    np.linalg.solve, T = [M's kept columns scaled to unit weighted norm (prior variance 1e40), the Fourier columns with
    phi > 0]."""
    n = len(t)
    t = np.asarray(t, dtype=np.float64)
    w = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    masks = [None] * len(comps) if masks is None else masks

    def block(c):
        f, idx, freqf = comps[c]
        chrom = np.ones(n) if idx == 0 else (freqf / np.asarray(nu, dtype=np.float64)) ** idx
        arg = 2 * np.pi * np.asarray(f, dtype=np.float64)[None, :] * t[:, None]
        F = np.concatenate([np.cos(arg), np.sin(arg)], axis=1) * chrom[:, None]
        return F if masks[c] is None else F * (np.asarray(masks[c]) != 0)[:, None]

    cols, prior = [], []
    if M is not None and np.any(keep):
        Mk = np.asarray(M, dtype=np.float64)[:, keep]
        cols.append(Mk / np.sqrt(np.sum(w[:, None] * Mk ** 2, axis=0)))
        prior.append(np.full(Mk.shape[1], TM_PRIOR))
    for c in range(len(comps)):
        ph2 = np.concatenate([phis[c], phis[c]]).astype(np.float64)
        cols.append(block(c)[:, ph2 > 0])
        prior.append(ph2[ph2 > 0])
    T = np.concatenate(cols, axis=1)
    Ft = block(target)
    WT = w[:, None] * T
    S = np.diag(1.0 / np.concatenate(prior)) + T.T @ WT
    return (Ft * w[:, None]).T - (Ft.T @ WT) @ np.linalg.solve(S, WT.T)


def definition_residual(t, nu, M, w, comps, phis, target, keep, B, masks=None):
    """How far a longdouble B [K, n] is from the definition B = F^T P^-1, without inverting anything: with P0 = W^-1 +
    sum_c F_c Phi_c F_c^T, marginalising M with infinite variance means B M = 0 and B P0 = F^T + C M^T for some C. Returns
    (max |B M^| , max |(B P0 - F^T) (I - Qm Qm^T)|), M^ the kept columns scaled to unit norm and Qm an orthonormal basis
    of them, both relative to the largest |F| |B| row product scale (max |F| = 1 for an unmasked achromatic target).
    Every product in longdouble: this does not suffer the cancellation of the fp64 literal form."""
    from tests.tm_reference import basis_ld
    n = len(t)
    masks = [None] * len(comps) if masks is None else masks
    wl = np.ones(n, dtype=LD) if w is None else np.asarray(w, dtype=np.float64).astype(LD)

    def block(c):
        f = np.asarray(comps[c][0], dtype=np.float64)
        return np.stack([column_ld(t, nu, f, comps[c][1], comps[c][2], k, len(f), masks[c]) for k in range(2 * len(f))],
                        axis=1)

    BP = B / wl[None, :]
    for c in range(len(comps)):
        F = block(c)
        ph = np.concatenate([phis[c], phis[c]]).astype(np.float64).astype(LD)
        BP = BP + ((B @ F) * ph[None, :]) @ F.T
    D = BP - block(target).T
    scale = np.max(np.abs(block(target)))
    bm = LD(0)
    if M is not None and np.any(keep):
        Mk = np.asarray(M, dtype=np.float64)[:, keep]
        Qm, _, kq = basis_ld(Mk)
        assert np.all(kq)
        D = D - (D @ Qm) @ Qm.T
        bm = np.max(np.abs(B @ (Mk.astype(LD) / np.sqrt(np.sum(Mk.astype(LD) ** 2, axis=0)))) /
                    np.sqrt(np.sum(B * B, axis=1))[:, None])
    return float(bm), float(np.max(np.abs(D)) / scale)


def pair_norms(Zs, phi_hat):
    """(N_ab [P, P] longdouble, symmetric with zero diagonal, and the sum of the absolute terms of every pair) with
    N_ab = tr(Z_a phi_hat Z_b phi_hat), phi_hat over the K columns."""
    P = len(Zs)
    ph = np.concatenate([phi_hat, phi_hat]).astype(np.float64).astype(LD)
    nab, mag = np.zeros((P, P), dtype=LD), np.zeros((P, P), dtype=LD)
    for a in range(P):
        A = Zs[a] * ph[None, :]
        for b in range(a):
            terms = A * (Zs[b].T * ph[:, None])  # [j, k]: Za[j, k] ph_k Zb[k, j] ph_j
            nab[a, b] = nab[b, a] = np.sum(terms)
            mag[a, b] = mag[b, a] = np.sum(np.abs(terms))
    return nab, mag


def x_truth(Bs, offs, res):
    """(X [P, K, n_vec] longdouble, bound [P, K, n_vec] = (n_p + 2) eps sum_t |B_kt| |r_t|) from the truth's B."""
    res = np.atleast_2d(np.asarray(res))
    assert res.dtype == np.float64
    X, bound = [], []
    for p, B in enumerate(Bs):
        r = res[:, int(offs[p]):int(offs[p + 1])].astype(LD)
        X.append(B @ r.T)
        bound.append((B.shape[1] + 2) * EPS * (np.abs(B) @ np.abs(r.T)).astype(np.float64))
    return np.stack(X), np.stack(bound)


def x_tolerance(truth, literal, bound):
    """Per pulsar and row: max(4 e_lit, bound), e_lit the literal form's largest error over the vectors of the row."""
    e_lit = np.max(np.abs(literal.astype(LD) - truth), axis=2, keepdims=True).astype(np.float64)
    return np.maximum(4 * e_lit, bound), e_lit


def q_truth(X, phi_hat, G):
    """(Q_mode [J, N, R] longdouble, its bound [J, N, R], the bound of Q = sum_m Q_mode [J, R]) of the definition
    applied to X [P, K, R]: Q[j][m][r] = sum_{a<b} G_j[a][b] phi_hat_m (X_a,cos X_b,cos + X_a,sin X_b,sin). The bounds
    are the dot-product bound (n_terms + 3) eps sum |G| |phi_hat| |X_a| |X_b| with n_terms = K P (P - 1) / 2, over the
    terms of the mode and over all terms."""
    X = np.asarray(X)
    assert X.dtype == np.float64
    P, K, R = X.shape
    N = K // 2
    G = np.asarray(G, dtype=np.float64)
    J = len(G)
    ia, ib = np.tril_indices(P, -1)
    Gp = G[:, ia, ib].astype(LD)  # [J, pairs]
    Xl = X.astype(LD)
    Qm, mag = np.zeros((J, N, R), dtype=LD), np.zeros((J, N, R), dtype=LD)
    for m in range(N):
        c, s = Xl[:, m, :], Xl[:, N + m, :]
        pc, ps = c[ia] * c[ib], s[ia] * s[ib]  # [pairs, R]
        ph = LD(np.float64(phi_hat[m]))
        for j in range(J):
            g = Gp[j][:, None]
            Qm[j, m] = ph * np.sum(g * (pc + ps), axis=0)
            mag[j, m] = abs(ph) * np.sum(np.abs(g) * (np.abs(pc) + np.abs(ps)), axis=0)
    n_terms = K * P * (P - 1) // 2
    return Qm, ((n_terms + 3) * EPS * mag).astype(np.float64), ((n_terms + 3) * EPS * mag.sum(axis=1)).astype(np.float64)
