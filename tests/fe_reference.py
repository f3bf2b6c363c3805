"""Truth and yardstick of the continuous-wave F-statistics (include/fakepta_amd.h, 'Continuous-wave F-statistics'), for
tests/test_fe_host.py and tests/test_gpu_fe.py. Test infrastructure only; not a test and not a conftest.

Everything is the header's definition in np.longdouble with sums in index order. operator_ld is tests/os_reference.py's
operator with the frequency grid appended to the noise model as an achromatic target with phi = 0 (every row takes the
projection form): rows g = c_g^T P^-1, rows G + g = s_g^T P^-1. antenna_ld is cw_device.h's cw_pair. inverse_ld is the
definition's inverse: scale to unit diagonal, Cholesky, pivot rule, L^-1 by forward substitution, D^-1/2 L^-T L^-1
D^-1/2. plan_ld makes the tables of an array; statistics_ld applies the definition to given fp64 X and fp64 tables
(what the device is held to) and returns the derived rounding bounds with it.

The bound of the host's inverses (INV_C). The host and this file both run the same algorithm in the 80-bit format on
inputs that agree to a few eps_ld, so their difference is the sum of both sides' rounding errors, which the standard
analyses bound (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.): for an n x n matrix A scaled to unit
diagonal, the computed Cholesky factor satisfies L L^T = A + dA with |dA| <= gamma_(n+1) |L||L^T| (Thm 10.3), and
|| |L||L^T| ||_2 <= n ||A||_2 (eq. 10.7), which moves the inverse by <= n (n + 1) u kappa(A) relative to ||A^-1||_2;
the forward substitutions for L^-1 add <= n u cond(L) <= n u kappa(A)^(1/2) per triangular factor (Thm 8.5), twice in
the product; the product L^-T L^-1 adds n u, and the scaling by D^-1/2 on both sides of A and of the inverse 4 u. With
kappa >= 1: <= (n (n + 1) + 2 n + n + 4) u kappa = 36 u kappa for n = 4 (18 u kappa for n = 2). Measuring the entries
against the largest entry instead of the 2-norm costs at most a factor n (max |a_ij| >= ||A||_2 / n), and the two sides
each have that error: INV_C = 2 * 4 * 36 = 288, taken for n = 2 as well. The rounding to fp64 adds half an eps of the
entry itself; its floor is 2 eps of the largest entry."""
import numpy as np

from tests.ld_reference import LD, EPS  # noqa: F401  (the extended-precision assertion of ld_reference applies)
from tests.fit_reference import _sum
from tests import os_reference as OS

EPS_LD = np.finfo(LD).eps
INV_C = 288
RCOND_FE = 1e-10
TRI4 = [(i, j) for i in range(4) for j in range(i, 4)]  # the 10 numbers of a symmetric 4 x 4 matrix


def inverse_bound(kappa):
    """The asserted bound of |host inverse - truth| relative to the truth's largest entry."""
    return max(2 * EPS, INV_C * float(kappa) * float(EPS_LD))


def operator_ld(t, nu, M, w, comps, phis, fgw, masks=None):
    """(B [2 G, n] longdouble, norms of M's columns, kept [m]) of one pulsar: comps / phis / masks the noise model as
    os_reference.operator_ld takes it; the frequency grid is appended as the target."""
    fgw = np.asarray(fgw, dtype=np.float64)
    comps2 = list(comps) + [(fgw, 0.0, 1400.0)]
    phis2 = list(phis) + [np.zeros(len(fgw))]
    masks2 = None if masks is None else list(masks) + [None]
    B, _, norms, keep = OS.operator_ld(t, nu, M, w, comps2, phis2, len(comps), masks2, need_z=False)
    return B, norms, keep


def m_ld(t, B, fgw):
    """m [G, 3] = (s|s), (s|c), (c|c) longdouble from the truth's B."""
    G = len(fgw)
    out = np.zeros((G, 3), dtype=LD)
    nu = np.ones(len(t))
    for g in range(G):
        c = OS.column_ld(t, nu, fgw, 0.0, 1400.0, g, G)
        s = OS.column_ld(t, nu, fgw, 0.0, 1400.0, G + g, G)
        out[g] = [_sum(B[G + g] * s), _sum(B[G + g] * c), _sum(B[g] * c)]
    return out


def antenna_ld(sky, pos):
    """(F [2 n_sky, P] longdouble: row 2 s F+, row 2 s + 1 Fx, 0 where 1 + Om.p == 0; scale [2 n_sky, P]: the largest
    of |F| and the numerator's terms over |1 + Om.p|, the yardstick of F's rounding; regular [n_sky] bool)."""
    sky, pos = np.asarray(sky, dtype=np.float64), np.asarray(pos, dtype=np.float64)
    S, P = len(sky), len(pos)
    F, scale, regular = np.zeros((2 * S, P), dtype=LD), np.zeros((2 * S, P), dtype=LD), np.ones(S, dtype=bool)
    x, y, z = (pos[:, i].astype(LD) for i in range(3))
    for s in range(S):
        cth, ph = LD(sky[s, 0]), LD(sky[s, 1])
        sth = np.sqrt(LD(1) - cth * cth)
        cph, sph = np.cos(ph), np.sin(ph)
        mp = sph * x - cph * y
        nq = -cth * cph * x - cth * sph * y + sth * z
        op = -sth * cph * x - sth * sph * y - cth * z
        den = LD(1) + op
        ok = den != 0
        regular[s] = bool(np.all(ok))
        d = np.where(ok, den, LD(1))
        F[2 * s] = np.where(ok, LD(0.5) * (mp * mp - nq * nq) / d, LD(0))
        F[2 * s + 1] = np.where(ok, mp * nq / d, LD(0))
        scale[2 * s] = np.where(ok, LD(0.5) * np.maximum(mp * mp, nq * nq) / np.abs(d), LD(0))
        scale[2 * s + 1] = np.abs(F[2 * s + 1])
    return F, np.maximum(scale, np.abs(F)), regular


def inverse_ld(A, rcond_fe=RCOND_FE):
    """(the inverse of the symmetric matrix A [n, n] by the definition's rule, or None for a singular point; kappa_2 of
    the scaled matrix, inf when singular)."""
    A = np.asarray(A, dtype=LD)
    n = len(A)
    dg = np.diag(A)
    if not np.all(np.isfinite(A)) or not np.all(dg > 0):
        return None, np.inf
    d = LD(1) / np.sqrt(dg)
    S = d[:, None] * A * d[None, :]
    S[np.arange(n), np.arange(n)] = LD(1)
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        piv = S[j, j]
        for l in range(j):
            piv = piv - L[j, l] * L[j, l]
        if not piv > LD(rcond_fe):
            return None, np.inf
        L[j, j] = np.sqrt(piv)
        for i in range(j + 1, n):
            a = S[i, j]
            for l in range(j):
                a = a - L[i, l] * L[j, l]
            L[i, j] = a / L[j, j]
    Li = np.zeros((n, n), dtype=LD)
    for j in range(n):
        Li[j, j] = LD(1) / L[j, j]
        for i in range(j + 1, n):
            a = LD(0)
            for l in range(j, i):
                a = a + L[i, l] * Li[l, j]
            Li[i, j] = -a / L[i, i]
    inv = np.zeros((n, n), dtype=LD)
    for i in range(n):
        for j in range(n):
            a = LD(0)
            for l in range(max(i, j), n):
                a = a + Li[l, i] * Li[l, j]
            inv[i, j] = d[i] * a * d[j]
    return inv, float(np.linalg.cond(S.astype(np.float64)))


def m_matrix(F, m, s, g):
    """M(s, g) [4, 4] longdouble = sum_p [[F+^2, F+ Fx], [F+ Fx, Fx^2]] (x) m_pg in pulsar order; m [P, G, 3]."""
    A = np.zeros((4, 4), dtype=LD)
    for p in range(F.shape[1]):
        fp, fc = F[2 * s, p], F[2 * s + 1, p]
        pol = np.array([[fp * fp, fp * fc], [fp * fc, fc * fc]], dtype=LD)
        blk = np.array([[m[p, g, 0], m[p, g, 1]], [m[p, g, 1], m[p, g, 2]]], dtype=LD)
        A = A + np.kron(pol, blk)
    return A


def plan_ld(psrs, comps_of, phis_of, masks_of, fgw, sky, pos, rcond_fe=RCOND_FE):
    """The tables of an array in longdouble: dict(B [P] of [2 G, n_p], keep, norms, m [P, G, 3], minv [P, G, 3] (0 where
    singular), kappa_m [P, G], counted [P, G] bool, dropped [P, G] bool (the column lies in the span of the marginalised
    model: (x|x) <= rcond^2 x^T W x), n_eff [G], F, F_scale, regular, M [n_sky, G, 10], Minv [n_sky, G, 10] (NaN where
    singular), kappa_M [n_sky, G]). psrs: [(t, nu, Mmat, w)]."""
    fgw = np.asarray(fgw, dtype=np.float64)
    P, G, S = len(psrs), len(fgw), len(sky)
    out = dict(B=[], keep=[], norms=[], m=np.zeros((P, G, 3), dtype=LD), minv=np.zeros((P, G, 3), dtype=LD),
               kappa_m=np.full((P, G), np.inf), counted=np.zeros((P, G), dtype=bool),
               dropped=np.zeros((P, G), dtype=bool))
    for p, (t, nu, M, w) in enumerate(psrs):
        if len(t) == 0:
            out["B"].append(np.zeros((2 * G, 0), dtype=LD))
            out["keep"].append(np.zeros(0 if M is None else M.shape[1], dtype=bool))
            out["norms"].append(np.zeros(0 if M is None else M.shape[1], dtype=LD))
            continue
        B, norms, keep = operator_ld(t, nu, M, w, comps_of(p), phis_of(p), fgw, masks_of(p))
        out["B"].append(B)
        out["keep"].append(keep)
        out["norms"].append(norms)
        out["m"][p] = m_ld(t, B, fgw)
        wl = np.ones(len(t), dtype=LD) if w is None else np.asarray(w, dtype=np.float64).astype(LD)
        for g in range(G):
            ss, sc, cc = out["m"][p, g]
            c = OS.column_ld(t, np.ones(len(t)), fgw, 0.0, 1400.0, g, G)
            sn = OS.column_ld(t, np.ones(len(t)), fgw, 0.0, 1400.0, G + g, G)
            rc2 = LD(OS.RCOND) ** 2
            if not ss > rc2 * _sum(wl * sn * sn) or not cc > rc2 * _sum(wl * c * c):
                # the column lies in the span of the marginalised model: the pulsar drops out at this frequency
                B[g] = 0
                B[G + g] = 0
                out["m"][p, g] = 0
                out["dropped"][p, g] = True
                continue
            inv, kap = inverse_ld(np.array([[ss, sc], [sc, cc]], dtype=LD), rcond_fe)
            if inv is not None:
                out["minv"][p, g] = [inv[0, 0], inv[0, 1], inv[1, 1]]
                out["kappa_m"][p, g] = kap
                out["counted"][p, g] = True
    out["n_eff"] = out["counted"].sum(axis=0)
    F, Fs, regular = antenna_ld(sky, pos)
    out.update(F=F, F_scale=Fs, regular=regular, M=np.zeros((S, G, 10), dtype=LD),
               Minv=np.full((S, G, 10), np.nan, dtype=LD), kappa_M=np.full((S, G), np.inf))
    for s in range(S):
        for g in range(G):
            A = m_matrix(F, out["m"], s, g)
            out["M"][s, g] = [A[i, j] for i, j in TRI4]
            inv, kap = inverse_ld(A, rcond_fe) if regular[s] else (None, np.inf)
            if inv is not None:
                out["Minv"][s, g] = [inv[i, j] for i, j in TRI4]
                out["kappa_M"][s, g] = kap
    return out


def nanmax_first(a, axis=0):
    """(max, argmax) along an axis with the definition's rules: NaN never wins, ties go to the lower index, all-NaN
    gives NaN and -1."""
    a = np.moveaxis(np.asarray(a), axis, 0)
    filled = np.where(np.isnan(a), -np.inf, a)
    arg = np.argmax(filled, axis=0)  # the first of equals
    none = np.all(np.isnan(a), axis=0)
    val = np.take_along_axis(a, arg[None], axis=0)[0]
    return np.where(none, np.nan, val), np.where(none, -1, arg)


def reduce_map(fe):
    """The definition's reductions of a map Fe [n_sky, G, R]: (Fe_f [G, R], argmax_f [G, R], Fe_max [R], argmax
    [2, R])."""
    fef, af = nanmax_first(fe, axis=0)
    fem, ag = nanmax_first(fef, axis=0)
    a_s = np.where(ag >= 0, np.take_along_axis(af, np.maximum(ag, 0)[None], axis=0)[0], -1)
    return fef, af, fem, np.stack([a_s, ag])


def statistics_ld(X, F, Minv, minv):
    """The definition applied in longdouble to fp64 X [P, 2 G, R] (rows g cosine, G + g sine) and the fp64 tables F
    [2 n_sky, P], Minv [n_sky, G, 10], minv [P, G, 3]: dict(Fe [n_sky, G, R] (NaN where Minv is), Fe_bound = (P + 16) eps
    sum_ij S_i |Minv_ij| S_j with S_i = sum_p |F_ip| |x_p|, Fp [G, R], Fp_bound = (3 P + 6) eps sum |terms|)."""
    X, F, Minv, minv = (np.asarray(a) for a in (X, F, Minv, minv))
    assert X.dtype == F.dtype == Minv.dtype == minv.dtype == np.float64
    P, K, R = X.shape
    G, S = K // 2, len(Minv)
    Xl, Fl = X.astype(LD), F.astype(LD)
    xs, xc = Xl[:, G:, :], Xl[:, :G, :]  # [P, G, R]
    Fp_, Fc_ = Fl[0::2], Fl[1::2]  # [S, P]
    N = np.stack([np.einsum("sp,pgr->sgr", Fp_, xs), np.einsum("sp,pgr->sgr", Fp_, xc),
                  np.einsum("sp,pgr->sgr", Fc_, xs), np.einsum("sp,pgr->sgr", Fc_, xc)])  # [4, S, G, R]
    Sa = np.stack([np.einsum("sp,pgr->sgr", np.abs(Fp_), np.abs(xs)), np.einsum("sp,pgr->sgr", np.abs(Fp_), np.abs(xc)),
                   np.einsum("sp,pgr->sgr", np.abs(Fc_), np.abs(xs)), np.einsum("sp,pgr->sgr", np.abs(Fc_), np.abs(xc))])
    fe, mag = np.zeros((S, G, R), dtype=LD), np.zeros((S, G, R), dtype=LD)
    Ml = Minv.astype(LD)
    for k, (i, j) in enumerate(TRI4):
        wgt = LD(1) if i == j else LD(2)
        a = np.where(np.isnan(Ml[:, :, k]), LD(0), Ml[:, :, k])[:, :, None]
        fe = fe + wgt * a * N[i] * N[j]
        mag = mag + wgt * np.abs(a) * Sa[i] * Sa[j]
    sing = np.isnan(Minv).any(axis=2)
    fe = np.where(sing[:, :, None], LD(np.nan), LD(0.5) * fe)
    ml = minv.astype(LD)[:, :, :, None]  # [P, G, 3, 1]
    terms = np.stack([ml[:, :, 0] * xs * xs, 2 * ml[:, :, 1] * xs * xc, ml[:, :, 2] * xc * xc])  # [3, P, G, R]
    fp = LD(0.5) * terms.sum(axis=(0, 1))
    fp_mag = LD(0.5) * np.abs(terms).sum(axis=(0, 1))
    return dict(Fe=fe, Fe_bound=((P + 16) * EPS * mag).astype(np.float64), Fp=fp,
                Fp_bound=((3 * P + 6) * EPS * fp_mag).astype(np.float64))


def hh_ld(B, r):
    """(r|r) = r^T P^-1 r is not available from B alone; for a signal in the span of the grid's columns, r = sum_k a_k
    F_k, (r|r) = a^T (B r): returns B r [2 G] longdouble."""
    return np.asarray(B, dtype=LD) @ np.asarray(r, dtype=np.float64).astype(LD)
