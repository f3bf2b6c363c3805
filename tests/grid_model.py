"""The naive numpy model of the gridded path's planner (csrc/grid_plan.h), written from the definitions in the
header's comments, and the literal fp64 evaluation of the gridded algorithm on that plan. Test infrastructure only; not
a test and not a conftest.

tests/test_grid_plan.py compares the planner's own tables with chrom_weight .. model_tables. The mode-response tests
(tests/test_grid_modes.py, tests/test_gpu_mode_response.py) take every grid signal's (nf, w, beta), the coalescing
groups, the interpolation rows and the deconvolution tables from here, never from the library under test.

A layout is a dict: P, offs [P + 1], toas, nu [n_toa], sigs (a list of dicts: kind, nm, idx, freqf, harmonic, w0 ([P]
for kind 0, [1] for kind 1: the first angular frequency as the library forms it, (2 pi) * f_1), mask (None or uint8
[n_toa])), and the options w, sigma, coalesce, grid_mfma."""
import math

import numpy as np

# the planning constants of grid_plan.h that the model needs (tests/test_grid_plan.py compares them with the header's)
TT, MAX_SEG, DFT_ROWS = 32, 16, 32


def chrom_weight(L, s):
    """Chromatic factor (freqf / nu)^idx times the mask, per TOA."""
    ch = np.ones(len(L["toas"])) if s["idx"] == 0.0 else (s["freqf"] / L["nu"]) ** s["idx"]
    return ch if s["mask"] is None else np.where(s["mask"] != 0, ch, 0.0)


def w0_rows(L, s):
    return s["w0"] if s["kind"] == 0 else np.full(L["P"], s["w0"][0])


def model_groups(L):
    """A signal joins the first earlier grid signal with the same w0 on every pulsar and the same weight per TOA."""
    members = []
    for i, s in enumerate(L["sigs"]):
        for m in members:
            f = L["sigs"][m[0]]
            if (L["coalesce"] and len(m) <= MAX_SEG and np.array_equal(w0_rows(L, s), w0_rows(L, f))
                    and np.array_equal(chrom_weight(L, s), chrom_weight(L, f))):
                m.append(i)
                break
        else:
            members.append([i])
    anchor = [max(m, key=lambda i: (L["sigs"][i]["nm"], -i)) for m in members]  # most modes, the first of equals
    return members, anchor, [m[-1] for m in members]


def bound(w, sigma):
    return math.exp(-math.pi * w * math.sqrt(1.0 - 1.0 / sigma))


def model_sizes(L, s):
    """(nf, w, took the fill, the fill inequality's two sides) of a grid signal anchored at layout signal s."""
    nm, w = s["nm"], L["w"]
    n0 = -(-max(math.ceil(L["sigma"] * (2.0 * nm + 1.0)), 2 * w + 2) // 4) * 4
    rho, w0p = 0.0, w0_rows(L, s)
    for p in range(L["P"]):
        t = L["toas"][L["offs"][p]:L["offs"][p + 1]]
        if len(t) > 1:
            rho += w0p[p] * (t.max() - t.min()) / float(len(t) - 1) / (2.0 * math.pi)
    rho /= L["P"]
    n1 = 4 * (-(-(n0 // 4 + 1) // DFT_ROWS) * DFT_ROWS - 1)
    w1 = w  # the narrowest kernel (>= 4) that keeps the options' bound at the larger oversampling
    while w1 > 4 and bound(w1 - 1, n1 / (2.0 * nm + 1.0)) <= bound(w, L["sigma"]):
        w1 -= 1
    lhs, rhs = w1 + TT * n1 * rho, w + TT * n0 * rho - 0.25
    fill = n1 > n0 and 2 * w1 + 2 <= n1 and lhs < rhs
    return (n1, w1, True, lhs, rhs) if fill else (n0, w, False, lhs, rhs)


_GL = np.polynomial.legendre.leggauss(256)


def model_tables(nm, nf, w, beta):
    """ecos / esin [ntab][lde] = q_k cos / sin(2 pi k j / nf), j <= nf / 2, k = m + 1; q_k = (2 pi / nf) / phi_hat(k),
    phi_hat(k) = alpha int phi(z) cos(k alpha z) dz, phi(z) = exp(beta (sqrt(1 - z^2) - 1)), alpha = pi w / nf; tq
    [4][ntq][ldq]: j <= nf / 4, [0] cos / [1] sin of odd k, [2] / [3] of even k."""
    x, wt = _GL
    half, alpha = nf // 2, math.pi * w / nf
    lde, ntab = (half // DFT_ROWS + 1) * DFT_ROWS, -(-nm // 8) * 8
    ldq, ntq = (nf // 4 // DFT_ROWS + 1) * DFT_ROWS, -(-((nm + 1) // 2) // 8) * 8
    k = np.arange(1, nm + 1)
    phi = np.exp(beta * (np.sqrt(1.0 - x * x) - 1.0))
    q = (2.0 * math.pi / nf) / (alpha * (wt * phi * np.cos(np.outer(k, alpha * x))).sum(axis=1))
    ang = 2.0 * math.pi * (np.outer(k, np.arange(half + 1)) % nf) / nf
    ec, es = np.zeros((ntab, lde)), np.zeros((ntab, lde))
    ec[:nm, :half + 1] = q[:, None] * np.cos(ang)
    es[:nm, :half + 1] = q[:, None] * np.sin(ang)
    tq = np.zeros((4, ntq, ldq))
    for m in range(nm):
        tq[2 * (m & 1), m >> 1, :nf // 4 + 1] = ec[m, :nf // 4 + 1]
        tq[2 * (m & 1) + 1, m >> 1, :nf // 4 + 1] = es[m, :nf // 4 + 1]
    return dict(half=half, lde=lde, ntab=ntab, ldq=ldq, ntq=ntq, ecos=ec.ravel(), esin=es.ravel(), tq=tq.ravel())


# ------------------------------------------------------------------------------------- the literal fp64 evaluation
def deconv_terms(nm, nf, w, beta):
    """The 256 terms [nm][256] whose sum model_tables (and plan_deconv_tables) divides by: wt_q phi(x_q) cos(k alpha
    x_q), in the recipe's own fp64 operations."""
    x, wt = _GL
    alpha = math.pi * w / nf
    phi = np.exp(beta * (np.sqrt(1.0 - x * x) - 1.0))
    return wt * phi * np.cos(np.outer(np.arange(1, nm + 1), alpha * x))


def deconv_q(nm, nf, w, beta):
    """q_k [nm] of the fp64 recipe: model_tables' table at grid row 0 (cos 0 = 1 exactly)."""
    T = model_tables(nm, nf, w, beta)
    return T["ecos"].reshape(T["ntab"], T["lde"])[:nm, 0].copy()


def grid_signals(L):
    """The plan's grid signals: a list of dicts with members, anchor (layout signal indices), nm (the anchor's), nf,
    w, fill, beta and err_bound, as plan_coalesce and plan_grid_sizes make them."""
    members, anchor, _ = model_groups(L)
    out = []
    for m, a in zip(members, anchor):
        s = L["sigs"][a]
        nf, w, fill, _, _ = model_sizes(L, s)
        sig = nf / (2.0 * s["nm"] + 1.0)
        out.append(dict(members=m, anchor=a, nm=s["nm"], nf=nf, w=w, fill=fill,
                        beta=0.98 * math.pi * w * (1.0 - 0.5 / sig), err_bound=bound(w, sig)))
    return out


def first_rows(L, s, g, p):
    """(J, d) of pulsar p's TOAs for grid signal g anchored at layout signal s, in plan_grid_sizes' fp64 operations:
    u = (w0 t) / h, h = 2 pi / nf, J = floor(u - w / 2) + 1 (unwrapped), d = u - J."""
    t = L["toas"][L["offs"][p]:L["offs"][p + 1]]
    u = (w0_rows(L, s)[p] * t) / (2.0 * math.pi / g["nf"])
    J = (np.floor(u - 0.5 * g["w"]) + 1).astype(np.int64)
    return J, u - J


def es_weights(d, w, beta, ch):
    """es_weight (csrc/device_common.h) [n_toa][w] in its fp64 operations: z = (d - i) / (w / 2), s = 1 - z z, ch
    exp(beta (sqrt(s) - 1)) where s > 0, else 0."""
    z = (d[:, None] - np.arange(w, dtype=np.float64)[None, :]) / (0.5 * w)
    s = 1.0 - z * z
    return np.where(s > 0.0, ch[:, None] * np.exp(beta * (np.sqrt(np.maximum(s, 0.0)) - 1.0)), 0.0)


def full_tables(nm, nf, w, beta):
    """(C, S) [nm][nf]: q_k cos / sin(2 pi k j / nf) for every grid row j, the rows past nf / 2 by the symmetry the
    DFT kernels use (g_{nf - j}: cos even, sin odd in j)."""
    T = model_tables(nm, nf, w, beta)
    half = T["half"]
    ec = T["ecos"].reshape(T["ntab"], T["lde"])[:nm, :half + 1]
    es = T["esin"].reshape(T["ntab"], T["lde"])[:nm, :half + 1]
    C, S = np.empty((nm, nf)), np.empty((nm, nf))
    C[:, :half + 1], S[:, :half + 1] = ec, es
    j = np.arange(half + 1, nf)
    C[:, j], S[:, j] = ec[:, nf - j], -es[:, nf - j]
    return C, S


def literal_response(L, s, g, p, coef, tables=None):
    """The literal fp64 evaluation of the gridded algorithm for one coefficient `coef` on mode k (cos or sin) of grid
    signal g, at pulsar p's TOAs: (value, sum of |terms|), each [n_toa_p][nm][2].
    value = sum_{i < w} fl(ch phi_i) fl(coef table[k][(J + i) mod nf]), summed in fp64 in the order of i."""
    nm, nf, w = g["nm"], g["nf"], g["w"]
    C, S = full_tables(nm, nf, w, g["beta"]) if tables is None else tables
    J, d = first_rows(L, s, g, p)
    ch = chrom_weight(L, s)[L["offs"][p]:L["offs"][p + 1]]
    W = es_weights(d, w, g["beta"], ch)
    val = np.zeros((len(J), nm, 2))
    tot = np.zeros((len(J), nm, 2))
    for i in range(w):
        r = (J + i) % nf
        for c, tab in enumerate((C, S)):
            term = W[:, i, None] * (coef * tab[:, r]).T
            val[:, :, c] += term
            tot[:, :, c] += np.abs(term)
    return val, tot
