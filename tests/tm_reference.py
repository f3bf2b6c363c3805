"""Truth and yardstick of the timing-model projection (include/fakepta_amd.h, 'timing-model projection'), for
tests/test_tm_host.py and tests/test_gpu_tm.py. Test infrastructure only; not a test and not a conftest.

basis_ld / project_truth are the header's definition in np.longdouble: every column of W^(1/2) M scaled to unit norm,
modified Gram-Schmidt with one re-orthogonalisation, the rank rule (a column is dropped when its norm after both passes
is <= rcond, or when it is all zero), then r' = r - (Q Q^T (s o r)) / s, with every sum in longdouble.
project_literal is the literal fp64 numpy evaluation of the same definition, column-scaled np.linalg.lstsq with the
same rcond: its distance from the truth is the yardstick of the tolerance."""
import numpy as np

from tests.ld_reference import LD, EPS  # noqa: F401  (the extended-precision assertion of ld_reference applies)

RCOND = 1e-10
KEEP_MIN, DROP_MAX = 1e-4, 1e-13  # a test's own inputs keep every orthogonalised norm outside (DROP_MAX, KEEP_MIN)


def basis_ld(M, w=None, rcond=None):
    """(Q [n, k] longdouble, orthogonalised norms [m] longdouble, kept [m] bool) of one pulsar's M [n, m] (fp64)."""
    M = np.asarray(M)
    assert M.dtype == np.float64 and M.ndim == 2
    n, m = M.shape
    rc = LD(RCOND if rcond is None or rcond <= 0 else rcond)
    s = np.ones(n, dtype=LD) if w is None else np.sqrt(np.asarray(w, dtype=np.float64).astype(LD))
    kept, norms, keep = [], np.zeros(m, dtype=LD), np.zeros(m, dtype=bool)
    for j in range(m):
        v = s * M[:, j].astype(LD)
        nrm2 = np.sum(v * v)
        if not nrm2 > 0:
            continue
        v = v * (LD(1) / np.sqrt(nrm2))
        for _ in range(2):
            for q in kept:
                v = v - np.sum(q * v) * q
        norms[j] = np.sqrt(np.sum(v * v))
        if norms[j] > rc:
            kept.append(v / norms[j])
            keep[j] = True
    Q = np.stack(kept, axis=1) if kept else np.zeros((n, 0), dtype=LD)
    return Q, norms, keep


def assert_clear_rank(norms, keep, M):
    """The rank decision of these inputs is never what a test measures: kept columns >= 1e-4, dropped ones <= 1e-13."""
    for j in range(len(norms)):
        if keep[j]:
            assert norms[j] >= KEEP_MIN, (j, float(norms[j]))
        else:
            assert norms[j] <= DROP_MAX, (j, float(norms[j]))


def project_truth(offs, Mmats, weights, res, rcond=None):
    """(post-fit res [n_vec, n_toa] longdouble, ranks [P]). Mmats: per-pulsar [n_p, m_p]; weights None or [n_toa]."""
    res = np.asarray(res)
    assert res.dtype == np.float64
    r2 = np.atleast_2d(res)
    out = r2.astype(LD)
    ranks = np.zeros(len(Mmats), dtype=np.int64)
    for p, M in enumerate(Mmats):
        sl = slice(int(offs[p]), int(offs[p + 1]))
        w = None if weights is None else np.asarray(weights, dtype=np.float64)[sl]
        Q, norms, keep = basis_ld(M, w, rcond)
        assert_clear_rank(norms, keep, M)
        ranks[p] = Q.shape[1]
        if Q.shape[1] == 0:
            continue
        s = np.ones(len(M), dtype=LD) if w is None else np.sqrt(w.astype(LD))
        x = out[:, sl]
        g = (x * s) @ Q          # [n_vec, k]
        out[:, sl] = x - (g @ Q.T) / s
    return out.reshape(res.shape), ranks


def project_literal(offs, Mmats, weights, res, rcond=None):
    """The same definition in fp64 numpy: per pulsar, lstsq of the unit-norm columns of W^(1/2) M against s o r."""
    r2 = np.atleast_2d(np.asarray(res, dtype=np.float64))
    out = r2.copy()
    rc = RCOND if rcond is None or rcond <= 0 else rcond
    for p, M in enumerate(Mmats):
        sl = slice(int(offs[p]), int(offs[p + 1]))
        M = np.asarray(M, dtype=np.float64)
        if M.shape[1] == 0 or M.shape[0] == 0:
            continue
        s = np.ones(len(M)) if weights is None else np.sqrt(np.asarray(weights, dtype=np.float64)[sl])
        A = s[:, None] * M
        nrm = np.linalg.norm(A, axis=0)
        A = A[:, nrm > 0] / nrm[nrm > 0]
        if A.shape[1] == 0:
            continue
        y = (out[:, sl] * s).T
        x = np.linalg.lstsq(A, y, rcond=rc)[0]
        out[:, sl] = out[:, sl] - (A @ x).T / s
    return out.reshape(np.shape(res))


def tolerance(truth, literal, res_in, sl=slice(None)):
    """max(4 e_lit, 64 eps max|r_in|) over the samples sl: e_lit the literal fp64 evaluation's own error."""
    e_lit = float(np.max(np.abs(np.atleast_2d(literal)[:, sl].astype(LD) - np.atleast_2d(truth)[:, sl]), initial=0))
    peak = float(np.max(np.abs(np.atleast_2d(res_in)[:, sl]), initial=0))
    return max(4 * e_lit, 64 * EPS * peak), e_lit, peak


# ----------------------------------------------------------------------------- inputs
def mmat(toas, freqs, f0=200.0, t0=0.0, year=365.25 * 86400.0):
    """make_Mmat's eight columns: offset, F0, F1, DM, DM1, DM2, annual cos / sin."""
    dt = np.asarray(toas, dtype=np.float64) - t0
    nu = np.asarray(freqs, dtype=np.float64)
    M = np.zeros((len(dt), 8))
    M[:, 0] = 1.0
    M[:, 1] = -dt / f0
    M[:, 2] = -0.5 * dt ** 2 / f0
    M[:, 3] = 1 / nu ** 2
    M[:, 4] = dt / nu ** 2 / f0
    M[:, 5] = 0.5 * dt ** 2 / nu ** 2 / f0
    M[:, 6] = np.cos(2 * np.pi / year * dt)
    M[:, 7] = np.sin(2 * np.pi / year * dt)
    return M


def three_band(rng, n):
    """Observing frequencies on three bands, each TOA's band drawn at random (every band present for n >= 3)."""
    nu = rng.choice([800.0, 1400.0, 2500.0], size=n) + rng.normal(0, 10, n)
    if n >= 3:
        nu[:3] = np.array([800.0, 1400.0, 2500.0]) + rng.normal(0, 10, 3)
    return np.abs(nu)


def smooth_columns(rng, toas, k):
    """k smooth random columns: sinusoids of 1.5 .. 6 cycles over the span with random phases."""
    t = (np.asarray(toas) - np.min(toas)) / max(np.ptp(toas), 1.0)
    cyc = rng.uniform(1.5, 6.0, k)
    return np.sin(2 * np.pi * (cyc[None, :] * t[:, None] + rng.uniform(0, 1, k)[None, :]))
