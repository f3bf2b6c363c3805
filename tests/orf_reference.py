"""Reference models of the anisotropic ORF (include/fakepta_amd.h, fpta_orf_anisotropic): the HEALPix RING pixel
centres, the reference's antenna pattern and the weighted Gram sum, restated in numpy (fp64 and np.longdouble) and in
50-digit mpmath. tools/gen_orf_golden.py writes the mpmath values to tests/golden/g12_orf.npz; nothing here comes from
a HEALPix library."""
import math

import numpy as np

MP_DIGITS = 50


# ----------------------------------------------------------------------------- pixel centres (integers are exact)
def ring_index(nside, p):
    """(i, j, kind) of pixel p: the header's three cases; kind 0 north cap, 1 belt, 2 south cap."""
    npix, ncap = 12 * nside * nside, 2 * nside * (nside - 1)
    if p < ncap:
        i = (1 + math.isqrt(1 + 2 * p)) >> 1
        return i, p + 1 - 2 * i * (i - 1), 0
    if p < npix - ncap:
        q = p - ncap
        t = q // (4 * nside)
        return t + nside, q - 4 * nside * t + 1, 1
    q = npix - p
    i = (1 + math.isqrt(2 * q - 1)) >> 1
    return i, 4 * i + 1 - (q - 2 * i * (i - 1)), 2


def _centre(nside, p, num, pi):
    """(z, phi) of pixel p in the arithmetic of `num` (a constructor of exact integers)."""
    npix = 12 * nside * nside
    i, j, kind = ring_index(nside, p)
    if kind == 1:
        s = num(1 + ((i + nside) & 1)) / num(2)
        return num(2 * nside - i) * num(2) / num(3 * nside), (num(j) - s) * pi / num(2 * nside)
    z = num(1) - num(4 * i * i) / num(npix)
    return (z if kind == 0 else -z), (num(j) - num(1) / num(2)) * pi / num(2 * i)


def centres(nside, dtype=np.float64):
    """(z, sin theta, phi) of every pixel in dtype arithmetic (np.float64 or np.longdouble)."""
    pi = dtype(np.pi) if dtype is np.float64 else np.longdouble("3.14159265358979323846264338327950288")
    zs, phis = zip(*(_centre(nside, p, dtype, pi) for p in range(12 * nside * nside)))
    z, phi = np.array(zs, dtype=dtype), np.array(phis, dtype=dtype)
    return z, np.sqrt((1 - z) * (1 + z)), phi


def centres_mp(nside):
    """[(z, sin theta, theta, phi)] per pixel as mpmath numbers."""
    import mpmath as mp
    mp.mp.dps = MP_DIGITS
    out = []
    for p in range(12 * nside * nside):
        z, phi = _centre(nside, p, mp.mpf, mp.pi)
        out.append((z, mp.sqrt((1 - z) * (1 + z)), mp.acos(z), phi))
    return out


def pix2ang_mp(nside):
    """(theta, phi) of every pixel rounded once from mpmath."""
    c = centres_mp(nside)
    return np.array([float(t[2]) for t in c]), np.array([float(t[3]) for t in c])


# ----------------------------------------------------------------------------- antenna pattern and ORF
def antenna(pos, z, st, phi):
    """F+, Fx [P, npix] and D [P, npix]: the reference's expression (correlated_noises.py:50-60), literally."""
    cp, sp, zero = np.cos(phi), np.sin(phi), np.zeros_like(phi)
    m = np.array([sp, -cp, zero]).T
    n = np.array([-z * cp, -z * sp, st]).T
    om = np.array([-st * cp, -st * sp, -z]).T
    pos = np.asarray(pos, dtype=z.dtype)
    mp_, nq, op = m @ pos.T, n @ pos.T, om @ pos.T
    with np.errstate(divide="ignore", invalid="ignore"):
        return (0.5 * (mp_ ** 2 - nq ** 2) / (1 + op)).T, ((mp_ * nq) / (1 + op)).T, (1 + op).T


def orf_numpy(pos, h_maps, dtype=np.float64):
    """ORF [M, P, P] (or [P, P] for one 1-D map): the reference's body (:73-89) on the model's pixel centres."""
    h = np.asarray(h_maps, dtype=dtype)
    one = h.ndim == 1
    h = np.atleast_2d(h)
    npix = h.shape[1]
    nside = math.isqrt(npix // 12)
    assert 12 * nside * nside == npix
    fp, fc, _ = antenna(np.asarray(pos, dtype=dtype), *centres(nside, dtype))
    out = []
    with np.errstate(invalid="ignore"):
        for hm in h:
            orf = dtype(1.5) * ((fp * hm) @ fp.T + (fc * hm) @ fc.T) / dtype(npix)
            orf[np.diag_indices_from(orf)] *= dtype(2.0)
            out.append(orf)
    out = np.array(out)
    return out[0] if one else out


def orf_longdouble(pos, h_maps):
    """The truth where the fixture has none: np.longdouble arithmetic, rounded once. [M, P, P] float64. The matrix
    products of longdouble arrays are plain loops in numpy, so keep P x npix small."""
    return np.asarray(orf_numpy(pos, h_maps, np.longdouble), dtype=np.float64)


def orf_mp(pos, h_maps):
    """ORF [M, P, P] in 50-digit arithmetic from the float64 inputs, rounded once."""
    import mpmath as mp
    mp.mp.dps = MP_DIGITS
    h = np.atleast_2d(np.asarray(h_maps, dtype=np.float64))
    npix = h.shape[1]
    nside = math.isqrt(npix // 12)
    cen = centres_mp(nside)
    P = len(pos)
    fp = [[None] * npix for _ in range(P)]
    fc = [[None] * npix for _ in range(P)]
    for a in range(P):
        px, py, pz = (mp.mpf(float(v)) for v in pos[a])
        for k, (z, st, _, phi) in enumerate(cen):
            cp, sp = mp.cos(phi), mp.sin(phi)
            m_p = sp * px - cp * py
            n_p = -z * cp * px - z * sp * py + st * pz
            d = 1 - st * cp * px - st * sp * py - z * pz
            fp[a][k] = (m_p ** 2 - n_p ** 2) / (2 * d)
            fc[a][k] = m_p * n_p / d
    out = np.empty((len(h), P, P))
    for m, hm in enumerate(h):
        w = [mp.mpf(float(v)) for v in hm]
        for a in range(P):
            for b in range(a + 1):
                s = mp.fsum((fp[a][k] * fp[b][k] + fc[a][k] * fc[b][k]) * w[k] for k in range(npix))
                v = mp.mpf(3) / 2 * s / npix * (2 if a == b else 1)
                out[m, a, b] = out[m, b, a] = float(v)
    return out


def hd_matrix(pos):
    """Hellings-Downs with unit diagonal (correlated_noises.py:62-71)."""
    pos = np.asarray(pos, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        x = (1 - pos @ pos.T) / 2
        orf = 1.5 * x * np.log(x) - 0.25 * x + 0.5
    np.fill_diagonal(orf, 1.0)
    return orf


# ----------------------------------------------------------------------------- test inputs
D_MIN = 1e-3  # every (pulsar, pixel) of a test has D >= this: the literal fp64 error then stays near 1e-15 of peak


def min_d(pos, nside):
    """min over (pulsar, pixel) of D = 1 + Omega . p."""
    return float(antenna(pos, *centres(nside))[2].min())


def draw_positions(rng, n_psr, nside, d_min=D_MIN):
    """n_psr unit vectors, uniform on the sphere, drawn by rejection so that min over pixels of D >= d_min. The
    excluded caps (radius sqrt(2 d_min)) cover the sphere from nside ~ 12 on at d_min = 1e-3: nside <= 8 only."""
    assert nside <= 8, "rejection at D >= 1e-3 leaves no room between the pixel centres of a finer map"
    cen = centres(nside)
    out = []
    while len(out) < n_psr:
        v = rng.normal(size=3)
        v /= np.linalg.norm(v)
        if antenna(v[None, :], *cen)[2].min() >= d_min:
            out.append(v)
    return np.array(out)


def random_positions(rng, n_psr):
    """n_psr unit vectors, uniform on the sphere."""
    v = rng.normal(size=(n_psr, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def draw_maps(rng, n_map, nside):
    """Maps with values in [0.2, 2]."""
    return rng.uniform(0.2, 2.0, size=(n_map, 12 * nside * nside))
