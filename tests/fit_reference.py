"""Truth and yardstick of the Fourier fit (include/fakepta_amd.h, 'Fourier fit'), for tests/test_fit_host.py and
tests/test_gpu_fit.py. Test infrastructure only; not a test and not a conftest.

operator_ld / fit_truth are the header's definition in np.longdouble: the columns of W^(1/2) [M F] (cos / sin of the
longdouble argument) scaled to unit norm, modified Gram-Schmidt with one re-orthogonalisation in column order, the rank
rule (a column is dropped when its norm after both passes is <= rcond, or when it is all zero), then A = D_F R_FF^-1
Q_F^T diag(s) with zero rows for dropped columns and a = A r, every sum in longdouble. fit_literal is the literal fp64
numpy evaluation: column-scaled np.linalg.lstsq on the kept columns of [M F] with the same rcond, Fourier part. Its
distance from the truth is one term of the tolerance; the other is the rigorous bound of a length-n fp64 dot product
in any order with a once-rounded operator, (n + 2) eps sum_t |A_kt| |r_t|."""
import numpy as np

from tests.ld_reference import LD, EPS  # noqa: F401  (the extended-precision assertion of ld_reference applies)
from tests.tm_reference import RCOND, KEEP_MIN, DROP_MAX, assert_clear_rank  # noqa: F401

TWO_PI = LD("6.283185307179586476925286766559005768")


def _sum(x):
    """The sum of a longdouble vector in index order. The kept columns of make_Mmat's design come out of the
    Gram-Schmidt passes with norms down to 1e-4, and a small Fourier norm multiplies that again: two longdouble
    evaluations of the definition that differ only in their summation order (numpy's pairwise blocks against a plain
    loop) differ by up to 100 eps of fp64 in A for 33 TOAs, 8 + 18 columns. So the truth fixes the order: every sum is
    taken in index order, every update in the order written here, which is also how csrc/fit_host.h works."""
    return np.cumsum(x)[-1] if len(x) else LD(0)


def columns_ld(t, nu, comps):
    """F [n, K] longdouble: per component (f [N], idx, freqf) the N cosine columns, then the N sine columns."""
    t = np.asarray(t, dtype=np.float64).astype(LD)
    cols = []
    for f, idx, freqf in comps:
        f = np.asarray(f, dtype=np.float64).astype(LD)
        chrom = np.ones(len(t), dtype=LD) if idx == 0 else \
            (LD(np.float64(freqf)) / np.asarray(nu, dtype=np.float64).astype(LD)) ** LD(np.float64(idx))
        arg = TWO_PI * f[None, :] * t[:, None]
        cols += [chrom[:, None] * np.cos(arg), chrom[:, None] * np.sin(arg)]
    return np.concatenate(cols, axis=1) if cols else np.zeros((len(t), 0), dtype=LD)


def operator_ld(t, nu, M, w, comps, rcond=None):
    """(A [K, n] longdouble, kept [K] bool, orthogonalised norms [m + K], kept [m + K]) of one pulsar."""
    M = np.zeros((len(t), 0)) if M is None else np.asarray(M)
    assert M.dtype == np.float64 and M.ndim == 2 and M.shape[0] == len(t)
    n, m = M.shape
    rc = LD(RCOND if rcond is None or rcond <= 0 else rcond)
    s = np.ones(n, dtype=LD) if w is None else np.sqrt(np.asarray(w, dtype=np.float64).astype(LD))
    C = np.concatenate([M.astype(LD), columns_ld(t, nu, comps)], axis=1) * s[:, None]
    nc = C.shape[1]
    K = nc - m
    Q = np.zeros((nc, n), dtype=LD)     # kept basis vectors, by kept order
    Rm = np.zeros((nc, nc), dtype=LD)   # R of the kept, scaled columns
    col_of, scale = [], []
    norms, keep = np.zeros(nc, dtype=LD), np.zeros(nc, dtype=bool)
    for j in range(nc):
        v = C[:, j].copy()
        nrm2 = _sum(v * v)
        if not nrm2 > 0:
            continue
        cn = np.sqrt(nrm2)
        v = v * (LD(1) / cn)
        k = len(col_of)
        proj = np.zeros(k, dtype=LD)
        for _ in range(2):
            for q in range(k):
                d = _sum(Q[q] * v)
                v = v - d * Q[q]
                proj[q] += d
        norms[j] = np.sqrt(_sum(v * v))
        if norms[j] > rc:
            Q[k] = v / norms[j]
            Rm[:k, k] = proj
            Rm[k, k] = norms[j]
            col_of.append(j)
            scale.append(cn)
            keep[j] = True
    k = len(col_of)
    A = np.zeros((K, n), dtype=LD)
    first = next((q for q in range(k) if col_of[q] >= m), k)
    X = Q[:k].copy()
    for j in range(k - 1, first - 1, -1):  # back substitution over the Fourier block
        for i in range(j + 1, k):
            X[j] = X[j] - Rm[j, i] * X[i]
        X[j] = X[j] * (LD(1) / Rm[j, j])
    for j in range(first, k):
        A[col_of[j] - m] = X[j] * (LD(1) / scale[j]) * s
    return A, keep[m:], norms, keep


def fit_truth(offs, toas, nu, Mmats, weights, comps_of, res, rcond=None):
    """(coef [P, K, n_vec] longdouble, kept [P, K], A per pulsar, bound [P, K, n_vec] = (n_p + 2) eps sum_t |A_kt|
    |r_t| with the truth's A). comps_of(p): the component list of pulsar p. Asserts the conditioning of its inputs."""
    res = np.atleast_2d(np.asarray(res))
    assert res.dtype == np.float64
    P = len(offs) - 1
    coef, kept, As, bound = [], [], [], []
    for p in range(P):
        sl = slice(int(offs[p]), int(offs[p + 1]))
        M = None if Mmats is None else Mmats[p]
        w = None if weights is None else np.asarray(weights, dtype=np.float64)[sl]
        A, kp, norms, keep = operator_ld(toas[sl], nu[sl], M, w, comps_of(p), rcond)
        assert_clear_rank(norms, keep, M)
        r = res[:, sl].astype(LD)
        coef.append(A @ r.T)
        kept.append(kp)
        As.append(A)
        bound.append((sl.stop - sl.start + 2) * EPS * (np.abs(A) @ np.abs(r.T)).astype(np.float64))
    return np.stack(coef), np.stack(kept), As, np.stack(bound)


def fit_literal(offs, toas, nu, Mmats, weights, comps_of, res, kept, rcond=None):
    """The same fit in fp64 numpy: per pulsar, lstsq of the unit-norm kept columns of W^(1/2) [M F] against s o r; the
    nuisance columns the truth drops are found by lstsq's own rcond. [P, K, n_vec] fp64."""
    res = np.atleast_2d(np.asarray(res, dtype=np.float64))
    rc = RCOND if rcond is None or rcond <= 0 else rcond
    out = np.zeros((len(offs) - 1, kept.shape[1], res.shape[0]))
    for p in range(len(offs) - 1):
        sl = slice(int(offs[p]), int(offs[p + 1]))
        if sl.stop == sl.start or not kept[p].any():
            continue
        t, v = toas[sl], nu[sl]
        cols = []
        for f, idx, freqf in comps_of(p):
            chrom = 1.0 if idx == 0 else (freqf / v) ** idx
            arg = 2 * np.pi * np.asarray(f)[None, :] * t[:, None]
            cols += [np.cos(arg) * np.reshape(chrom, (-1, 1) if np.ndim(chrom) else ()),
                     np.sin(arg) * np.reshape(chrom, (-1, 1) if np.ndim(chrom) else ())]
        F = np.concatenate(cols, axis=1)[:, kept[p]]
        M = np.zeros((len(t), 0)) if Mmats is None else np.asarray(Mmats[p], dtype=np.float64)
        s = np.ones(len(t)) if weights is None else np.sqrt(np.asarray(weights, dtype=np.float64)[sl])
        C = s[:, None] * np.concatenate([M, F], axis=1)
        nrm = np.linalg.norm(C, axis=0)
        ok = nrm > 0
        x = np.linalg.lstsq(C[:, ok] / nrm[ok], (res[:, sl] * s).T, rcond=rc)[0] / nrm[ok][:, None]
        full = np.zeros((C.shape[1], res.shape[0]))
        full[ok] = x
        out[p, kept[p]] = full[M.shape[1]:]
    return out


def tolerance(truth, literal, bound):
    """Per pulsar and row: max(4 e_lit, bound), e_lit the literal form's largest error over the vectors of that row.
    [P, K, n_vec]."""
    e_lit = np.max(np.abs(literal.astype(LD) - truth), axis=2, keepdims=True).astype(np.float64)
    return np.maximum(4 * e_lit, bound), e_lit
