"""High-precision truths for the drop-in and statistics calls of include/fakepta_amd.h, in numpy's np.longdouble
(the x87 80-bit format: 64-bit significand). Test infrastructure only; not a test and not a conftest.

Every function takes the fp64 inputs exactly as the C ABI receives them and evaluates the header's definition with
no rounding that matters at fp64: sums in longdouble (eps 2^-64 x the number of terms), the phase of a basis element
reduced as 2 pi frac(f_k t) with the product f_k t formed exactly (both factors split into 26 / 27-bit halves, so
every partial product is exact in longdouble and the whole cycles drop out before anything is rounded). The tests
use these as the truth and the literal fp64 evaluation's own distance from them as the yardstick (tests/test_gpu_cw.py
does the same with a stored 60-digit truth).

tests/test_ld_reference.py pins common_truth and gp_truth to the reference's recorded outputs (fixtures G2, G3).

mode_truth is the batch paths' basis itself, one mode at a time; grid_q, grid_values and grid_mode_model are the gridded
path's algorithm in longdouble, with the deconvolution factors from an mpmath quadrature (tests/test_grid_modes.py,
tests/test_gpu_mode_response.py)."""
import functools

import numpy as np

LD = np.longdouble
# the hosts are x86-64: np.longdouble is the 80-bit extended format. Anywhere else (longdouble == double) the truths
# below would be no better than the code under test, so this fails loudly instead of skipping.
assert np.finfo(LD).eps <= 2.0 ** -63, (
    f"tests/ld_reference.py needs an extended-precision np.longdouble (eps <= 2^-63); this one has eps = "
    f"{np.finfo(LD).eps!r}")

EPS = np.finfo(np.float64).eps
TWO_PI = 8 * np.arctan(LD(1))


def _f64(a):
    a = np.asarray(a)
    assert a.dtype == np.float64, a.dtype  # the truths take the library's inputs, not a re-rounded copy
    return a


def _split(a):
    """Veltkamp split of fp64 a = hi + lo, hi of <= 26 significant bits, lo of <= 27 (exact, in fp64)."""
    a = _f64(a)
    c = a * (2.0 ** 27 + 1.0)
    hi = c - (c - a)
    return hi.astype(LD), (a - hi).astype(LD)


def _frac(x):
    return x - np.floor(x)


def phase(f, t):
    """2 pi frac(f_k t) [len(t), len(f)] in longdouble; f_k t is formed exactly (see the module docstring)."""
    fh, fl = _split(np.asarray(f, dtype=np.float64).ravel())
    th, tl = _split(np.asarray(t, dtype=np.float64).ravel())
    hh = _frac(th[:, None] * fh[None, :])  # 52-bit product: exact, and so is its fraction
    mid = _frac(th[:, None] * fl[None, :]) + _frac(tl[:, None] * fh[None, :])
    return TWO_PI * _frac(hh + mid + tl[:, None] * fl[None, :])


def chromatic(freqf, nu, idx):
    """(freqf / nu)^idx in longdouble."""
    return (LD(freqf) / _f64(nu).astype(LD)) ** LD(idx)


def mix_truth(L, z):
    """x[k][c][p] = sum_q L[p][q] z[k][c'][q] in the header's (cos, sin) output order: z holds the reference's draws
    [n_modes][2][P] with the sin vector first, so x[:, 0] = L z[:, 1] (cos) and x[:, 1] = L z[:, 0] (sin)."""
    L, z = _f64(L).astype(LD), _f64(z).astype(LD)
    x = np.einsum("pq,kcq->kcp", L, z)
    return x[:, ::-1, :]


def common_truth(offs, toas, nu, f, amp, idx, freqf, L, z):
    """fpta_common_accumulate: (residual delta [n_toa_total], x [n_modes][2][P]) in longdouble.
    delta[t in p] = (freqf / nu_t)^idx sum_k amp_k (x_cos[k][p] cos + x_sin[k][p] sin)(2 pi f_k t)."""
    offs = np.asarray(offs, dtype=np.int64)
    toas, nu, f, amp = _f64(toas), _f64(nu), _f64(f), _f64(amp)
    x = mix_truth(L, z)
    a = amp.astype(LD)
    delta = np.zeros(int(offs[-1]), dtype=LD)
    for p in range(len(offs) - 1):
        sl = slice(int(offs[p]), int(offs[p + 1]))
        ph = phase(f, toas[sl])
        delta[sl] = chromatic(freqf, nu[sl], idx) * (np.cos(ph) @ (a * x[:, 0, p]) + np.sin(ph) @ (a * x[:, 1, p]))
    return delta, x


def gp_truth(offs, toas, nu, segments, masks, sign):
    """fpta_gp_accumulate_array: the residual delta [n_toa_total] in longdouble.
    segments: list of (f [P, N], ccos [P, N], csin [P, N], idx, freqf); masks: None or a list (per segment) of None /
    bool [n_toa_total]; delta[t in p] = sign sum_s m_s(t) (freqf_s / nu_t)^idx_s sum_k (ccos cos + csin sin)."""
    offs = np.asarray(offs, dtype=np.int64)
    toas, nu = _f64(toas), _f64(nu)
    delta = np.zeros(int(offs[-1]), dtype=LD)
    for s, (f, ccos, csin, idx, freqf) in enumerate(segments):
        f, ccos, csin = _f64(f), _f64(ccos), _f64(csin)
        m = None if masks is None or masks[s] is None else np.asarray(masks[s], dtype=bool)
        for p in range(len(offs) - 1):
            sl = slice(int(offs[p]), int(offs[p + 1]))
            ph = phase(f[p], toas[sl])
            v = chromatic(freqf, nu[sl], idx) * (np.cos(ph) @ ccos[p].astype(LD) + np.sin(ph) @ csin[p].astype(LD))
            if m is not None:
                v = np.where(m[sl], v, LD(0))
            delta[sl] += v
    return LD(sign) * delta


def correlation_truth(block, P, n):
    """fpta_batch_correlations on a downloaded block [R][P n]: (C [R][P][P], sum_r C_r [P][P],
    sum_r C_r[a][b] / sqrt(C_r[a][a] C_r[b][b]) [P][P], autos C_r[p][p] [R][P]), summed in longdouble."""
    block = _f64(block)
    R = block.shape[0]
    assert block.shape == (R, P * n)
    C = np.empty((R, P, P), dtype=LD)
    for r in range(R):  # one realization at a time: the longdouble copy of the whole block is not needed
        x = block[r].reshape(P, n).astype(LD)
        C[r] = (x @ x.T) / LD(n)
    autos = np.einsum("raa->ra", C).copy()
    d = np.sqrt(autos)
    norm = (C / (d[:, :, None] * d[:, None, :])).sum(axis=0)
    return C, C.sum(axis=0), norm, autos


def checksum_truth(block):
    """fpta_batch_checksums: per-realization (sum, sum of squares) [R][2] in longdouble."""
    x = _f64(block).astype(LD)
    return np.stack([x.sum(axis=1), (x * x).sum(axis=1)], axis=1)


def mode_truth(f, toas, nu, idx, freqf, mask=None):
    """The basis itself, [n_toa, N, 2] in longdouble: ch(t) cos(2 pi f_k t) and ch(t) sin(2 pi f_k t) with
    ch = (freqf / nu)^idx, 0 where mask (None: no mask) is 0. One pulsar's TOAs and frequencies f [N]."""
    ph = phase(f, toas)
    ch = chromatic(freqf, nu, idx)
    if mask is not None:
        ch = np.where(np.asarray(mask) != 0, ch, LD(0))
    return np.stack([np.cos(ph), np.sin(ph)], axis=2) * ch[:, None, None]


# --------------------------------------------------------------------------- the gridded algorithm in longdouble
# The type-2 non-uniform FFT of csrc/grid_plan.h and DESIGN.md section 5b, evaluated with no rounding that matters
# at fp64: it differs from mode_truth by the algorithm's aliasing alone, so a device that differs from it by more than
# fp64 rounding has a defect, whatever the aliasing allows.
def _to_ld(x):
    """An mpmath number as longdouble: its two leading fp64 pieces (106 bits before the sum is rounded to 64)."""
    hi = float(x)
    return LD(hi) + LD(float(x - hi))


@functools.lru_cache(maxsize=None)
def grid_q(nm, nf, w, beta):
    """q_k = (2 pi / nf) / phi_hat(k), k = 1 .. nm, in longdouble: phi_hat(k) = alpha int_{-1}^{1} exp(beta (sqrt(1 -
    z^2) - 1)) cos(k alpha z) dz, alpha = pi w / nf, by mpmath at 30 digits with z = sin(theta), which makes the
    integrand analytic on [0, pi / 2] (the kernel's square-root end point would cost a Gauss rule its accuracy)."""
    import mpmath as mp
    with mp.workdps(30):
        alpha, b = mp.pi * w / nf, mp.mpf(beta)
        out = []
        for k in range(1, nm + 1):
            ka = k * alpha
            val, err = mp.quad(lambda th: mp.exp(b * (mp.cos(th) - 1)) * mp.cos(ka * mp.sin(th)) * mp.cos(th),
                               [0, mp.pi / 2], error=True)
            assert err <= mp.mpf(10) ** -22 * abs(val), (k, err, val)  # mpmath's own estimate: far below 2^-64
            out.append(_to_ld((2 * mp.pi / nf) / (alpha * 2 * val)))
    q = np.array(out, dtype=LD)
    q.flags.writeable = False
    return q


def grid_values(nm, nf, w, beta, q=None):
    """(C, S) [nm][nf] in longdouble: q_k cos / sin(2 pi ((k j) mod nf) / nf). q: other deconvolution factors than
    grid_q's (tests of the tests)."""
    q = grid_q(nm, nf, w, float(beta)) if q is None else np.asarray(q, dtype=LD)
    k = np.arange(1, nm + 1, dtype=np.int64)
    ang = TWO_PI * ((k[:, None] * np.arange(nf, dtype=np.int64)[None, :]) % nf).astype(LD) / LD(nf)
    return q[:, None] * np.cos(ang), q[:, None] * np.sin(ang)


def grid_mode_model(f1, toas, nu, idx, freqf, mask, J, nm, nf, w, beta, values=None):
    """The gridded algorithm's answer for mode_truth's entries with f_k = k f_1, [n_toa, nm, 2] in longdouble (the
    second value: sum over the w terms of |term|). u = nf (f_1 t) from the exact product as phase forms it; J [n_toa]
    the first interpolation rows the planner takes (its fp64 expression, tests/grid_model.py first_rows), so model
    and device interpolate over the same rows; d = u - J in longdouble; weights phi((d - i) / (w / 2)) as es_weight
    defines them, phi(z) = exp(beta (sqrt(1 - z^2) - 1)) on |z| < 1, else 0."""
    toas = _f64(toas)
    C, S = grid_values(nm, nf, w, beta) if values is None else values
    J = np.asarray(J, dtype=np.int64)
    um = LD(nf) * (phase([f1], toas)[:, 0] / TWO_PI)  # u mod nf
    d = um - (J % nf).astype(LD)
    d = d - LD(nf) * np.round((d - LD(w) / 2) / LD(nf))  # the representative next to J: w / 2 - 1 < d <= w / 2
    ch = chromatic(freqf, nu, idx)
    if mask is not None:
        ch = np.where(np.asarray(mask) != 0, ch, LD(0))
    val = np.zeros((len(toas), nm, 2), dtype=LD)
    tot = np.zeros((len(toas), nm, 2), dtype=LD)
    for i in range(w):
        z = (d - LD(i)) / (LD(w) / 2)
        s = 1 - z * z
        wt = np.where(s > 0, ch * np.exp(LD(beta) * (np.sqrt(np.maximum(s, LD(0))) - 1)), LD(0))
        r = (J + i) % nf
        for c, tab in enumerate((C, S)):
            term = wt[:, None] * tab[:, r].T
            val[:, :, c] += term
            tot[:, :, c] += np.abs(term)
    return val, tot
