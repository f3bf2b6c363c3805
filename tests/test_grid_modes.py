"""The gridded path's algorithm, mode by mode, on the CPU: what its deconvolution recipe and its aliasing really are.

1. The fp64 recipe of plan_deconv_tables (256-node Gauss-Legendre on the kernel with its square-root end points,
   tests/grid_model.py model_tables restates it) against an mpmath quadrature of the same integral
   (tests/ld_reference.py grid_q), for every k of N = 1, 30, 100, 257 at the planner's (nf, w, beta) of the shipped
   options, with and without the fill. Allowance: 256 eps sum |terms| / |sum terms|, the dot-product bound of the
   recipe's own 256-term sum computed from the terms (<= 3.4e-12 here). Seen: <= 7.3e-15.

2. The aliasing of one mode. exp(-pi w sqrt(1 - 1 / sigma)) (grid_info "err_bound", 1.5e-12 at the shipped w = 15,
   sigma = 1.5) is the exponential-of-semicircle kernel's design estimate, not a bound on a mode's error: the top
   modes, next to the edge of the oversampled band, are off by up to 18 times as much. Per unit coefficient, sup over
   6000 random TOAs of a 10-year span at real-MJD epochs (one pulsar: the fill taken; 40 pulsars of 150: not taken),
   longdouble model of the algorithm against the longdouble basis (f_k = fl(k / T) as the library receives it), and
   the largest normwise error of eight flat-spectrum draws. "own": over the estimate at the grid signal's own (w, nf /
   (2 N + 1)), "1.5e-12": over the estimate of the options:

      N    nf   w  fill  worst mode  its error       / own  / 1.5e-12   median mode  normwise
      1    32  15  no       1        2.1e-18            13   1.4e-06     2.1e-18     1.1e-18
      1   124   9  yes      1        2.2e-11            24        15     2.2e-11     1.8e-11
      7    32  15  no       7        1.1e-13            11     0.071     1.6e-14     4.9e-14
      7   124  10  yes      6        5.2e-12            24       3.4     3.7e-12     3.2e-12
     30    92  15  no      30        1.4e-11            11       9.4     3.8e-13     6.3e-12
     30   124  13  yes     29        5.3e-12            23       3.4     5.0e-13     1.7e-12
    100   304  15  no      98        2.2e-11            18        15     5.0e-13     6.8e-12
    100   380  13  yes    100        1.8e-11            27        12     1.0e-12     5.0e-12
    257   776  15  no     251        2.8e-11            18        18     7.8e-13     6.4e-12
    257   892  14  yes    248        9.6e-12            23       6.3     7.1e-13     2.2e-12

   (printed by the test; run with -s. The library plans with the padded mode count N + (N & 1), so 1, 7 and 257 modes
   get the grid and the kernel shape of 2, 8 and 258. The 1e-13 of 7 modes without the fill is not aliasing: the
   model runs on k f_1, the basis on fl(k / T), a phase apart by up to eps |2 pi f_k t|.) Every mode is within the
   suite's 1e-10, the normwise figure within the gridded tests' GRID_TOL = 2e-11: both are
   asserted. The worst single mode, 2.8e-11 per unit coefficient, is what the headers and DESIGN.md section 5b quote.

   The fill narrows the kernel until the estimate, not the error, meets the options': a single mode, which the floor
   of 32 grid points alone would leave at 2e-18, ends at 2.2e-11 on 124 points with w = 9 (normwise 1.8e-11, a tenth
   under GRID_TOL). Every mode stays 11 to 27 times its own estimate; none is worse than the options' own top modes.
"""
import functools

import numpy as np
import pytest

from tests import grid_model as G
from tests import ld_reference as T

LD = np.longdouble
EPS = T.EPS
T0, SPAN = 4.5e9, 3.15e8  # real-MJD-like epochs [s], ten years
SHIPPED_W, SHIPPED_SIGMA = 15, 1.5  # fpta_ctx defaults (tests/test_gpu_grid.py asserts them on the library)
TOL, GRID_TOL = 1e-10, 2e-11  # SURVEY.md section 8(c); tests/test_gpu_grid.py
DENSE, SPARSE = 6000, 150  # TOAs per pulsar, 1 or 40 pulsars (6000 TOAs each way): the fill rule takes the larger grid
                            # for the dense pulsar only


@functools.lru_cache(maxsize=None)
def case(N, n_toa):
    """6000 TOAs as one pulsar or as 40 of 150, N flat modes on f_k = k / SPAN, and the planner model's grid signal.
    The library plans with the padded mode count N + (N & 1) (SegDesc::nm), so the model does too."""
    rng = np.random.default_rng([N, n_toa])
    P = DENSE // n_toa
    toas = np.concatenate([np.sort(T0 + SPAN * rng.random(n_toa)) for _ in range(P)])
    f = np.arange(1, N + 1) / SPAN
    sig = dict(kind=0, nm=N + (N & 1), idx=0.0, freqf=1400.0, harmonic=1, w0=np.full(P, (2.0 * np.pi) * f[0]),
               mask=None)
    L = dict(P=P, offs=n_toa * np.arange(P + 1), toas=toas, nu=np.full(P * n_toa, 1400.0), sigs=[sig], w=SHIPPED_W,
             sigma=SHIPPED_SIGMA, coalesce=1, grid_mfma=1)
    (g,) = G.grid_signals(L)
    return L, f, g


@pytest.mark.parametrize("n_toa", [SPARSE, DENSE])
@pytest.mark.parametrize("N", [1, 30, 100, 257])
def test_deconvolution_recipe_against_mpmath(N, n_toa):
    L, f, g = case(N, n_toa)
    assert g["fill"] == (n_toa == DENSE)
    q64 = G.deconv_q(N, g["nf"], g["w"], g["beta"])
    q = T.grid_q(g["nm"], g["nf"], g["w"], g["beta"])[:N]
    dev = np.abs(q64.astype(LD) / q - 1)
    terms = G.deconv_terms(N, g["nf"], g["w"], g["beta"])
    allow = 256 * EPS * np.abs(terms).sum(axis=1) / np.abs(terms.sum(axis=1))
    k = int(np.argmax(dev / allow))
    print(f"N {N} nf {g['nf']} w {g['w']}: largest relative deviation of q_k {float(dev.max()):.2e} (k = "
          f"{int(np.argmax(dev)) + 1}); allowance {allow.min():.2e} .. {allow.max():.2e}; worst ratio "
          f"{float(dev[k] / allow[k]):.2e} at k = {k + 1}")
    assert np.all(dev <= allow)


@pytest.mark.parametrize("n_toa", [SPARSE, DENSE])
@pytest.mark.parametrize("N", [1, 7, 30, 100, 257])
def test_per_mode_aliasing(N, n_toa):
    L, f, g = case(N, n_toa)
    assert g["fill"] == (n_toa == DENSE)  # both size choices of the planner
    J = np.concatenate([G.first_rows(L, L["sigs"][0], g, p)[0] for p in range(L["P"])])
    model, _ = T.grid_mode_model(f[0], L["toas"], L["nu"], 0.0, 1400.0, None, J, g["nm"], g["nf"], g["w"], g["beta"])
    model = model[:, :N, :]
    truth = T.mode_truth(f, L["toas"], L["nu"], 0.0, 1400.0)
    err = np.abs(model - truth).max(axis=(0, 2))  # per mode: sup over TOAs, cos and sin
    rng = np.random.default_rng(N)
    c = rng.standard_normal((8, N, 2)).astype(LD)  # flat spectrum: every mode weighs the same
    diff, want = np.einsum("rkc,tkc->rt", c, model - truth), np.einsum("rkc,tkc->rt", c, truth)
    normwise = float((np.sqrt((diff * diff).sum(axis=1)) / np.sqrt((want * want).sum(axis=1))).max())
    k = int(np.argmax(err))
    print(f"{N:4d} {g['nf']:5d} {g['w']:3d}  {'yes' if g['fill'] else 'no ':3s} {k + 1:6d}     {float(err[k]):.1e}   "
          f"{float(err[k]) / g['err_bound']:8.2g}  {float(err[k]) / G.bound(SHIPPED_W, SHIPPED_SIGMA):8.2g}    "
          f"{float(np.median(err)):.1e}   {normwise:.1e}")
    assert g["err_bound"] <= G.bound(SHIPPED_W, SHIPPED_SIGMA) * (1 + 1e-12)
    assert np.all(err <= TOL)
    assert normwise <= GRID_TOL
