"""High-precision truths for the drop-in and statistics calls of include/fakepta_amd.h, in numpy's np.longdouble
(the x87 80-bit format: 64-bit significand). Test infrastructure only; not a test and not a conftest.

Every function takes the fp64 inputs exactly as the C ABI receives them and evaluates the header's definition with
no rounding that matters at fp64: sums in longdouble (eps 2^-64 x the number of terms), the phase of a basis element
reduced as 2 pi frac(f_k t) with the product f_k t formed exactly (both factors split into 26 / 27-bit halves, so
every partial product is exact in longdouble and the whole cycles drop out before anything is rounded). The tests
use these as the truth and the literal fp64 evaluation's own distance from them as the yardstick (tests/test_gpu_cw.py
does the same with a stored 60-digit truth).

tests/test_ld_reference.py pins common_truth and gp_truth to the reference's recorded outputs (fixtures G2, G3)."""
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
