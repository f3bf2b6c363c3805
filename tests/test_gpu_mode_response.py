"""Every batch synthesis path, one coefficient at a time, against a longdouble truth.

The device is linear in the coefficients and fpta_batch_synth_from_z lets a test set them. Realization r of a block sets
exactly one (signal, mode, cos / sin) to 1 on all pulsars at once, or for a common signal exactly one (signal, pulsar
q, mode, cos / sin): then x = L z is the column L[:, q] exactly in any summation order, so the mix kernels' data
movement is checked element by element (a response where L[p][q] == 0 must be exactly 0). With the flat amplitude 1e-7
every realization, pulsar by pulsar, must be amp (L[p][q]) ch(t) cos or sin(2 pi f_k t): tests/ld_reference.py
mode_truth. A relative error of 1e-7 in mode 30 of a red spectrum, invisible to assert_parity at 1e-10, is 1e4 times
the allowances below. The block is NaN before each call and must come back finite; the shipped options are restored
after each test. test_drawn_* does the same for the kernels that draw inside themselves, which from_z cannot reach,
through the coefficient dump.

Layouts: real-MJD epochs (T0 = 4.5e9 s, span 3.15e8 s), ragged sorted TOAs, nu from {800, 1400, 2500}, every signal on
f_k = k / span. per_psr: 5 pulsars of 1, 17, 64, 150, 300 TOAs, 30 modes idx 0 + 41 modes idx 2 (the nm + (nm & 1)
padding mode) + 7 modes idx 4 behind a random mask (three grid signals). top_modes / top_modes_257: 4 pulsars of 100
.. 300 TOAs, 100 / 257 modes idx 2. coalesced: 4 pulsars, two idx-0 signals of 30 and 12 modes (one grid signal, the
12-mode member must answer with its own modes and leave 13 .. 30 alone) + 100 modes idx 2. dense_one: 3 pulsars of 300
.. 400 TOAs, 30 modes idx 0 (bands of <= 32 rows: k_grid_interp_psr). common_chol / common_svd / common_two: 70
pulsars of 8 .. 40 TOAs, a common signal of 4 modes with L the Cholesky factor of the HD ORF or numpy's SVD factor,
or both of them as two signals (idx 0 and idx 2); at FPTA_OPT_MIX_MFMA 1 and 0.

Allowances. None is measured on the code under test; all are computed at run time per (signal, mode, cos / sin,
pulsar), eps = 2^-52, k0 = k - 1 the mode's index from 0:

  exact (path 1, k_synth_direct): |device - truth| <= 4 lit + 4 eps amp max ch. lit = max over the pulsar's TOAs of
    |fl(amp ch cos(fl(fl(2 pi f_k) t))) - truth|, the literal fp64 evaluation's own error; the kernel forms the same
    phase, its sincos and pow are a few ulp (the factor 4 of tests/test_gpu_dropin_shapes.py); the floor covers TOAs
    where the phase rounding happens to vanish (one-TOA pulsars).

  recurrences (path 2 k_synth_mfma, path 3 k_synth_valu_seeded on harmonic grids at anchor 0, path 3 k_synth_valu at
    an anchor): the same, plus amp max_t(ch 2 eps |w_k t|) + amp max ch eps C, and nothing where the mode is itself an
    anchor. Derivation, from the kernels' arithmetic:
    - the phasor of mode k is the anchor mode a's, sincos(fl(w_a t)), turned n times by a step phasor of angle
      fl(w_s t) (k_synth_valu: s = mode 1, n = k0 mod 2 A modes since the anchor, k0 at anchor 0; k_synth_mfma: two
      modes per step, s = mode 2 or twice mode 1's angle, n = (k0 div 2) mod A; seeded: the three-term recurrence with
      2 cos(fl(w_1 t)), whose exact solution is ch exp(i k fl(w_1 t)), so a = none, n = k).
      |fl(fl(2 pi f) t) - 2 pi f t| <= eps |w t| (two roundings), so the angle is off by eps (|w_a t| + n |w_s t|);
      the truth runs on the given f_k = fl(k / T), which is up to eps f_k from f_a + n f_s: eps |w_k t| more. With
      w_a + n w_s = w_k that is 2 eps |w_k t| of angle, times amp ch of value.
    - arithmetic: a complex multiply (two products, two FMAs) errs by <= sqrt(2) eps |z|, and the step phasor's own
      value error (a sincos ulp each; the square cn^2 - sn^2, 2 cn sn of k_synth_mfma's even lanes doubles it and adds
      a rounding) turns every step by <= 3 eps more: C = 6 n, not amplified because |step| = 1 + O(eps).
      The issue expected n (eps / 2 |2 w_1 t| + 4 eps): the product's rounding alone. Rounding 2 pi f and the
      f_k / k f_1 mismatch double the phase part, the step phasor's own error raises 4 to 6.
    - seeded: a local error (the FMA's rounding, eps / 2 |z|, and 2 cos's ulp, eps |z|: <= 2 eps ch) made at step j
      reaches step k times U_{k - j - 1}(cos), |U_n| <= n + 1 (the kernel's comment), the seed's rounding (eps ch per
      component) times U_k0: C = 2 sum_{j <= k0} j + 2 (k0 + 1) = (k0 + 1) (k0 + 2).

  gridded (path 4): the device against the longdouble model M of the algorithm itself (tests/ld_reference.py
    grid_mode_model on the planner model's (nf, w, beta), groups and first rows: tests/grid_model.py), so aliasing
    drops out: |device - M| <= 4 max_t |literal fp64 algorithm - M| + (w + 8) eps amp ch sum_i |phi_i g_{J + i}|. The
    first term is the rounding of u = (w_1 t) / h, which the planner and the literal share; the second the dot-product
    bound of the w-term interpolation (gamma_w = w eps / 2, a factor 2 of slack as in tests/test_gpu_reductions.py),
    needed because the MFMA sums in another order than the literal, + 8 eps for the roundings of the table entry, the
    coefficient (amp L[p][q]), their product, the weight's exp and the quarter-range symmetry. Separately |device -
    truth| <= 1e-10 amp max ch per mode, the suite's tolerance.

  common signals: the above times |L[p][q]|.

  drawn blocks (test_drawn_*): |out - sum_k c_k M_k| <= sum_k |c_k| Y_k with M_k and Y_k the unit-coefficient model
    and gridded allowance, c the block's own coefficient dump; |out - truth| <= 1e-10 sum_k |c_k| max ch.

A deliberately wrong model fails every gridded layout (test_a_wrong_model_fails_where_parity_passes, on the CPU model
side only: q_k taken one mode off, or the top mode's table row scaled by 1 + 1e-9 in the literal and the longdouble
model alike, which assert_parity at 1e-10 passes on a red spectrum of 30 modes and more).

Worst device error over allowance per layout and path, as printed on an MI355X (the bound is 1):

  layout          direct  mfma   seeded (0 .. 5)  grid, MFMA DFT  its kernel                   grid, VALU DFT (.._ws)
  per_psr         0.250   0.298  0.280            0.273 (0.243)   k_grid_interp_ws<false>      0.266 (0.243)
  top_modes       0.250   0.270  0.256            0.252 (0.223)   k_grid_fused<8, f, f, true>  0.250 (0.223)
  coalesced       0.250   0.271  0.256            0.251 (0.226)   k_grid_fused<8, f, f, true>  0.250 (0.226)
  dense_one                                       0.250 (0.144)   k_grid_interp_psr<false, 8>  0.249 (0.144)
  top_modes_257           0.284  0.254            0.251 (0.298)   k_grid_interp_ws<false>      0.251 (0.298)
  common_chol     0.249   0.249  0.137            0.261 (6.3e-4)  k_grid_fused<8, f, f, true>  0.253 (6.3e-4)
  common_svd      0.250   0.250  0.131            0.257 (6.2e-4)  k_grid_fused<8, f, f, true>  0.252 (6.2e-4)
  common_two      0.252   0.250  0.142            0.259 (6.3e-4)  k_grid_fused<8, f, f, true>  0.259 (6.3e-4)
  top_modes at FPTA_OPT_ANCHOR 1 / 8: k_synth_mfma 0.250 / 0.339, k_synth_valu (every variant) 0.435 / 0.326
  drawn_c2: 0.059 (0.0084), k_grid_fused<12, false, true, false> on its shaped instance and k_grid_dft_gen +
    k_grid_interp_ws<false> alike; drawn_dm: 0.065 (0.0096), the same two
  wrong models, every gridded layout: q_k one mode off 4e9 .. 7e12, the top row scaled by 1 + 1e-9 102 (257 modes) ..
    3e4 (4 modes); the right model 0.25 .. 0.27

In brackets: device - truth over 1e-10 amp max ch. The six seeded variants gave the same figure to three digits in
every layout, and so did FPTA_OPT_MIX_MFMA 1 and 0. A figure of 0.25 is a device that errs exactly as the literal fp64
evaluation does, whose own error enters the allowance four times: the rounding of the phase, or of u, dominates
everywhere. The recurrence terms are needed: against the exact paths' allowance alone (the second figure each
recurrence case prints) the seeded kernel and k_synth_mfma read 6.7 on per_psr, k_synth_valu 1.31 and 1.01 at anchors
1 and 8, k_synth_mfma 1.04 at anchor 8, and the 100- and 257-mode layouts 0.84 .. 0.97. With the planner model run on
the unpadded mode count (41 instead of 42: the same nf, beta 1.2 % apart) per_psr read 117 and top_modes_257 1.37: a
kernel shape that differs in the third digit does not pass.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import fakepta_oracle as O
from tests import grid_model as G
from tests import ld_reference as T

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = T.EPS
T0, SPAN = 4.5e9, 3.15e8  # real-MJD-like epochs [s]
NUS = (800.0, 1400.0, 2500.0)
FREQF = 1400.0
AMP = 1e-7
TOL = 1e-10
SHIPPED_WIDTH, SHIPPED_SIGMA100 = 15, 150
GEN_LOAD = 1  # draw shape of C2's pattern (csrc/fused_sched.h)


@pytest.fixture(scope="module")
def capi():
    from fakepta_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def ctx(capi):
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def restore_options(ctx, capi):
    shipped = ctx.options()
    assert shipped[capi.OPT_GRID_WIDTH] == SHIPPED_WIDTH and shipped[capi.OPT_GRID_SIGMA] == SHIPPED_SIGMA100
    assert shipped[capi.OPT_GRID_COALESCE] == 1 and shipped[capi.OPT_ANCHOR] == 0
    yield
    ctx.batch_clear()
    ctx.set_options(shipped)


def set_or_skip(ctx, capi, key, value):
    """Option values that only a variant build accepts skip on the product build, as elsewhere."""
    try:
        ctx.set_option(key, value)
    except capi.FptaError as e:
        if "variant" in str(e) or "diagnostic" in str(e):
            pytest.skip(str(e))
        raise


# ------------------------------------------------------------------------------------------------ layouts
def _sig(kind, nm, idx, P, mask=None, L=None):
    f = np.arange(1, nm + 1) / SPAN
    return dict(kind=kind, nm=nm, idx=idx, mask=mask, L=L, f=f if kind == 1 else np.tile(f, (P, 1)),
                amp=np.full(nm if kind == 1 else (P, nm), AMP))


def _hd_factor(rng, P, how):
    v = rng.normal(size=(P, 3))
    gam = O.orf_hd(v / np.linalg.norm(v, axis=1)[:, None])
    return np.ascontiguousarray(np.linalg.cholesky(gam) if how == "chol" else O.mvn_factor(gam))


@functools.lru_cache(maxsize=None)
def layout(name):
    rng = np.random.default_rng([len(name), sum(map(ord, name))])
    if name == "per_psr":
        n = np.array([1, 17, 64, 150, 300])
    elif name.startswith("common"):
        n = rng.integers(8, 41, size=70)
    elif name == "dense_one":
        n = rng.integers(300, 401, size=3)
    elif name.startswith("drawn"):
        n = rng.integers(40, 101, size=3)
    else:
        n = rng.integers(100, 301, size=4)
    P, N = len(n), int(n.sum())
    offs = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    toas = np.concatenate([np.sort(T0 + rng.uniform(0.0, SPAN, k)) for k in n])
    nu = rng.choice(NUS, size=N)
    if name == "per_psr":
        mask = (rng.random(N) < 0.6).astype(np.uint8)
        sigs = [_sig(0, 30, 0.0, P), _sig(0, 41, 2.0, P), _sig(0, 7, 4.0, P, mask=mask)]
    elif name == "top_modes":
        sigs = [_sig(0, 100, 2.0, P)]
    elif name == "top_modes_257":
        sigs = [_sig(0, 257, 2.0, P)]
    elif name == "coalesced":
        sigs = [_sig(0, 30, 0.0, P), _sig(0, 12, 0.0, P), _sig(0, 100, 2.0, P)]
    elif name == "dense_one":
        sigs = [_sig(0, 30, 0.0, P)]
    elif name in ("common_chol", "common_svd"):
        sigs = [_sig(1, 4, 0.0, P, L=_hd_factor(rng, P, name[7:]))]
    elif name == "common_two":
        sigs = [_sig(1, 4, 0.0, P, L=_hd_factor(rng, P, "chol")), _sig(1, 4, 2.0, P, L=_hd_factor(rng, P, "svd"))]
    elif name == "drawn_c2":  # RN30 + DM100 + HD30: C2's draw shape
        sigs = [_sig(0, 30, 0.0, P), _sig(0, 100, 2.0, P), _sig(1, 30, 0.0, P, L=_hd_factor(rng, P, "svd"))]
    elif name == "drawn_dm":
        sigs = [_sig(0, 100, 2.0, P)]
    else:
        raise KeyError(name)
    for a in (offs, toas, nu):
        a.flags.writeable = False  # shared between tests: nobody changes it
    # the same layout as the planner model reads it (tests/grid_model.py): w0 as the library forms it, and the mode
    # count the planner is given, which is the padded one, nm + (nm & 1) (SegDesc::nm): 41 modes get the grid size and
    # the kernel shape beta of 42
    plan = dict(P=P, offs=offs, toas=toas, nu=nu, w=SHIPPED_WIDTH, sigma=SHIPPED_SIGMA100 / 100.0, coalesce=1,
                grid_mfma=1,
                sigs=[dict(kind=s["kind"], nm=s["nm"] + (s["nm"] & 1), idx=s["idx"], freqf=FREQF, harmonic=1,
                           mask=s["mask"],
                           w0=np.full(P if s["kind"] == 0 else 1, (2.0 * np.pi) * (1.0 / SPAN))) for s in sigs])
    # realizations: one (signal, mode, cos / sin), or one (signal, pulsar q, mode, cos / sin) of a common signal
    r0, R = [], 0
    for s in sigs:
        r0.append(R)
        R += (P if s["kind"] == 1 else 1) * 2 * s["nm"]
    return SimpleNamespace(name=name, P=P, N=N, n=n, offs=offs, toas=toas, nu=nu, sigs=sigs, plan=plan, r0=r0, R=R,
                           nmax=max(s["nm"] + (s["nm"] & 1) for s in sigs))


def psr(lay, p):
    return slice(int(lay.offs[p]), int(lay.offs[p + 1]))


def upload(ctx, lay):
    ctx.batch_set_toas(lay.offs, lay.toas, lay.nu)
    for s in lay.sigs:
        ctx.batch_add_signal(s["kind"], s["f"], s["amp"], idx=s["idx"], freqf=FREQF, L=s["L"], mask=s["mask"])


def one_hot(lay):
    z = np.zeros((lay.R, len(lay.sigs), lay.P, lay.nmax, 2))
    for si, s in enumerate(lay.sigs):
        nm = s["nm"]
        if s["kind"] == 0:
            r = lay.r0[si] + np.arange(2 * nm).reshape(nm, 2)
            for c in range(2):
                z[r[:, c], si, :, np.arange(nm), c] = 1.0
        else:
            r = lay.r0[si] + np.arange(lay.P * 2 * nm).reshape(lay.P, nm, 2)
            for q in range(lay.P):
                for c in range(2):
                    z[r[q, :, c], si, q, np.arange(nm), c] = 1.0
    return z


# ------------------------------------------------------------------------------------------------ truths and yardsticks
def _ch64(s, nu, mask):
    """chrom_factor (csrc/device_common.h) in its fp64 operations, times the mask."""
    x = FREQF / nu
    ch = np.ones(len(nu)) if s["idx"] == 0.0 else x * x if s["idx"] == 2.0 else x if s["idx"] == 1.0 else x ** s["idx"]
    return ch if mask is None else np.where(mask != 0, ch, 0.0)


@functools.lru_cache(maxsize=None)
def direct_yardsticks(name, coef=AMP):
    """Per (signal, pulsar): truth coef ch cos / sin [nm][2][n_p] in longdouble, the literal fp64 evaluation's error
    lit [nm][2] (max over the pulsar's TOAs), max ch, and max_t ch |w_k t| [nm]."""
    lay = layout(name)
    out = []
    for s in lay.sigs:
        f = s["f"] if s["kind"] == 1 else s["f"][0]
        w = (2.0 * np.pi) * f  # the library's operation order
        per = []
        for p in range(lay.P):
            sl = psr(lay, p)
            t, nu, m = lay.toas[sl], lay.nu[sl], None if s["mask"] is None else s["mask"][sl]
            truth = np.transpose(LD(coef) * T.mode_truth(f, t, nu, s["idx"], FREQF, m), (1, 2, 0))
            ch = _ch64(s, nu, m)
            ph = w[:, None] * t[None, :]
            lit64 = np.stack([coef * (ch * np.cos(ph)), coef * (ch * np.sin(ph))], axis=1)
            per.append(SimpleNamespace(truth=truth, lit=np.abs(lit64.astype(LD) - truth).max(axis=2).astype(float),
                                       chmax=float(ch.max()), tw=(ch[None, :] * np.abs(ph)).max(axis=1)))
        out.append(per)
    return out


def recurrence_term(kernel, anchor, nm, y, coef=AMP):
    """The recurrence paths' extra allowance [nm][1][1] (module docstring)."""
    k0 = np.arange(nm)
    if kernel == "seeded":
        n, C = k0 + 1, (k0 + 1.0) * (k0 + 2.0)
    elif kernel == "mfma":
        n = (k0 // 2) % anchor if anchor else k0 // 2
        C = 6.0 * n
    else:  # k_synth_valu
        n = k0 % (2 * anchor) if anchor else k0
        C = 6.0 * n
    term = coef * (2.0 * EPS * y.tw + y.chmax * EPS * C)
    return np.where(n > 0, term, 0.0)[:, None, None]


@functools.lru_cache(maxsize=None)
def grid_yardsticks(name, coef=AMP, wrong=None):
    """(grid signals of the planner model, per layout signal its grid signal's index, per (grid signal, pulsar): the
    longdouble model M [nm][2][n_p], max_t |literal fp64 algorithm - M| [nm][2][1], sum |terms| [nm][2][n_p]).
    wrong: a deliberately wrong model, for the test of the tests."""
    lay = layout(name)
    gs = G.grid_signals(lay.plan)
    of = {i: gi for gi, g in enumerate(gs) for i in g["members"]}
    out = []
    for g in gs:
        s = lay.plan["sigs"][g["anchor"]]
        nm, nf, w, beta = g["nm"], g["nf"], g["w"], g["beta"]
        values = T.grid_values(nm, nf, w, beta)
        tables = G.full_tables(nm, nf, w, beta)
        if wrong == "q_off_by_one":  # mode k deconvolved with q_{k + 1}, in the longdouble model and the literal alike
            q = T.grid_q(nm + 1, nf, w, beta)
            values = T.grid_values(nm, nf, w, beta, q[1:])
            tables = tuple(v * (q[1:] / q[:-1]).astype(float)[:, None] for v in tables)
        if wrong == "row_scaled":  # the top mode the layout has (the row after it may be the padding mode's)
            top = lay.sigs[g["anchor"]]["nm"] - 1
            values = tuple(np.where(np.arange(nm)[:, None] == top, v * (1 + LD(1e-9)), v) for v in values)
            tables = tuple(np.where(np.arange(nm)[:, None] == top, v * (1 + 1e-9), v) for v in tables)
        per = []
        for p in range(lay.P):
            sl = psr(lay, p)
            J, _ = G.first_rows(lay.plan, s, g, p)
            M, _ = T.grid_mode_model(1.0 / SPAN, lay.toas[sl], lay.nu[sl], s["idx"], FREQF,
                                     None if s["mask"] is None else s["mask"][sl], J, nm, nf, w, beta, values)
            lit, tot = G.literal_response(lay.plan, s, g, p, coef, tables)
            M = np.transpose(LD(coef) * M, (1, 2, 0))
            lit, tot = np.transpose(lit, (1, 2, 0)), np.transpose(tot, (1, 2, 0))
            per.append(SimpleNamespace(M=M, lit=np.abs(lit.astype(LD) - M).max(axis=2, keepdims=True).astype(float),
                                       tot=tot, w=w))
        out.append(per)
    return gs, of, out


# ------------------------------------------------------------------------------------------------ the comparison
def responses(lay, out, si, p):
    """The block's rows that excite signal si, at pulsar p's TOAs: [(P,) nm, 2, n_p]."""
    s = lay.sigs[si]
    rows = (lay.P if s["kind"] == 1 else 1) * 2 * s["nm"]
    blk = out[lay.r0[si]:lay.r0[si] + rows, psr(lay, p)]
    return blk.reshape(((lay.P,) if s["kind"] == 1 else ()) + (s["nm"], 2, blk.shape[1]))


def compare(dev, ref, allow, scale=None):
    """Worst |dev - scale ref| / (|scale| allow); where the allowance is 0 the device must be exact. dev [(P,) nm, 2,
    n_p], scale None or L[p, :]."""
    if scale is not None:
        ref = LD(1) * scale.astype(LD)[:, None, None, None] * ref[None]
        allow = np.abs(scale)[:, None, None, None] * np.broadcast_to(allow, ref.shape[1:])[None]
    err = np.abs(dev.astype(LD) - ref).astype(float)
    allow = np.broadcast_to(allow, err.shape)
    assert np.all(err[allow == 0.0] == 0.0), "a response that must be exactly 0 is not"
    return float((err[allow > 0.0] / allow[allow > 0.0]).max(initial=0.0))


def check_block(lay, out, kind, anchor=0, wrong=None):
    """Worst ratio of a one-hot block against its allowance. kind: direct, mfma, valu, seeded or grid."""
    assert out.shape == (lay.R, lay.N) and np.all(np.isfinite(out))
    Y = direct_yardsticks(lay.name)
    worst, worst_truth = 0.0, 0.0
    if kind == "grid":
        gs, of, GY = grid_yardsticks(lay.name, AMP, wrong)
    for si, s in enumerate(lay.sigs):
        nm = s["nm"]
        for p in range(lay.P):
            dev, y = responses(lay, out, si, p), Y[si][p]
            scale = None if s["kind"] == 0 else s["L"][p, :]
            if kind == "grid":
                gy = GY[of[si]][p]
                allow = 4.0 * gy.lit[:nm] + (gy.w + 8) * EPS * gy.tot[:nm]
                worst = max(worst, compare(dev, gy.M[:nm], allow, scale))
                worst_truth = max(worst_truth, compare(dev, y.truth, np.full((nm, 2, 1), TOL * AMP * y.chmax), scale))
            else:
                allow = 4.0 * y.lit[:, :, None] + 4.0 * EPS * AMP * y.chmax
                if kind != "direct":  # second figure: against the exact paths' allowance, for the record only
                    worst_truth = max(worst_truth, compare(dev, y.truth, allow, scale))
                    allow = allow + recurrence_term(kind, anchor, nm, y)
                worst = max(worst, compare(dev, y.truth, allow, scale))
    return worst, worst_truth


def run_from_z(ctx, lay):
    z = one_hot(lay)
    ctx.batch_synth_from_z(z)  # sizes the block
    ctx.debug_fill_out(np.nan)
    return ctx.batch_synth_from_z(z)


# (id, FPTA_OPT_SYNTH_PATH, FPTA_OPT_VALU_VARIANT, FPTA_OPT_GRID_MFMA)
PATHS = ([("direct", 1, 0, None), ("mfma", 2, 0, None)] + [(f"valu{v}", 3, v, None) for v in range(6)]
         + [("grid_mfma1", 4, 0, 1), ("grid_mfma0", 4, 0, 0)])
# the interpolation kernel of a from_z block (no in-kernel draws, not pipelined) on the product build, by
# psr_layout / fused_layout (csrc/capi.hip): one grid signal of <= 124 points with bands of <= 32 rows on the MFMA
# DFT: k_grid_interp_psr; else <= 2 grid signals whose grids fit in LDS, on the MFMA DFT: k_grid_fused without draws;
# else (three grid signals, 776 grid points, or the VALU DFT of FPTA_OPT_GRID_MFMA 0): k_grid_interp_ws
GRID_KERNEL = {"per_psr": "k_grid_interp_ws<", "top_modes": "k_grid_fused<", "top_modes_257": "k_grid_interp_ws<",
               "coalesced": "k_grid_fused<", "dense_one": "k_grid_interp_psr<", "common_chol": "k_grid_fused<",
               "common_svd": "k_grid_fused<", "common_two": "k_grid_fused<"}


def run_case(ctx, capi, name, path_id, anchor=0, mix_mfma=None):
    lay = layout(name)
    pid, path, variant, grid_mfma = next(p for p in PATHS if p[0] == path_id)
    ctx.set_option(capi.OPT_SYNTH_PATH, path)
    set_or_skip(ctx, capi, capi.OPT_VALU_VARIANT, variant)
    set_or_skip(ctx, capi, capi.OPT_ANCHOR, anchor)
    if grid_mfma is not None:
        set_or_skip(ctx, capi, capi.OPT_GRID_MFMA, grid_mfma)
    if mix_mfma is not None:
        set_or_skip(ctx, capi, capi.OPT_MIX_MFMA, mix_mfma)
    upload(ctx, lay)
    out = run_from_z(ctx, lay)
    gi = ctx.batch_grid_info()
    assert gi["last_path"] == path, gi
    label = f"{name} {pid} anchor {anchor}" + ("" if mix_mfma is None else f" mix_mfma {mix_mfma}")
    if path == 4:
        # the aggregate of the planner model against the library's own plan
        gs = G.grid_signals(lay.plan)
        assert gi["grid_signals"] == len(gs) and gi["signals"] == len(lay.sigs), gi
        # err_bound: the design estimate at the options' (w, sigma); each grid signal's own (w, nf / (2 N + 1)) within
        est = G.bound(SHIPPED_WIDTH, SHIPPED_SIGMA100 / 100.0)
        assert gi["width"] == SHIPPED_WIDTH and abs(gi["err_bound"] / est - 1) < 1e-12, gi
        assert max(g["err_bound"] for g in gs) <= est * (1 + 1e-12), gs
        want = GRID_KERNEL[name] if grid_mfma else "k_grid_interp_ws<"
        kernel = gi["interp_kernel"]
        print(f"{label}: {kernel}")
        if not capi.build_flags() & capi.BUILD_DIAG:  # a variant build pads the bands: other kernels may serve
            assert kernel.startswith(want), (kernel, want)
            if want == "k_grid_fused<":
                assert _fused_instance(kernel)[1:3] == (False, False), kernel  # the instance without draws
        worst, worst_truth = check_block(lay, out, "grid")
        print(f"{label}: device - model over allowance {worst:.3g}; device - truth over 1e-10 amp ch {worst_truth:.3g}")
        assert worst <= 1.0 and worst_truth <= 1.0
    else:
        kind = "direct" if path == 1 else "mfma" if path == 2 else "seeded" if anchor == 0 else "valu"
        worst, exact = check_block(lay, out, kind, anchor)
        print(f"{label}: device - truth over allowance {worst:.3g} ({kind}"
              + (")" if kind == "direct" else f"; over the exact paths' allowance {exact:.3g})"))
        assert worst <= 1.0
    return out


# ------------------------------------------------------------------------------------------------ C. one-hot responses
@pytest.mark.parametrize("path_id", [p[0] for p in PATHS])
@pytest.mark.parametrize("name", ["per_psr", "top_modes", "coalesced"])
def test_per_pulsar_mode_responses(ctx, capi, name, path_id):
    run_case(ctx, capi, name, path_id)


@pytest.mark.parametrize("path_id", ["grid_mfma1", "grid_mfma0"])
def test_dense_one_signal_reaches_the_per_pulsar_kernel(ctx, capi, path_id):
    run_case(ctx, capi, "dense_one", path_id)


@pytest.mark.parametrize("anchor", [1, 8])
@pytest.mark.parametrize("path_id", ["mfma"] + [f"valu{v}" for v in range(6)])
def test_top_modes_anchored_recurrences(ctx, capi, path_id, anchor):
    """FPTA_OPT_ANCHOR 1 and 8 (0: test_per_pulsar_mode_responses): k_synth_mfma re-anchors every `anchor` K-steps,
    path 3 takes k_synth_valu, which re-anchors every 2 `anchor` modes."""
    run_case(ctx, capi, "top_modes", path_id, anchor=anchor)


@pytest.mark.parametrize("path_id", ["mfma"] + [f"valu{v}" for v in range(6)] + ["grid_mfma1", "grid_mfma0"])
def test_257_mode_responses(ctx, capi, path_id):
    run_case(ctx, capi, "top_modes_257", path_id)


@pytest.mark.parametrize("mix_mfma", [1, 0])
@pytest.mark.parametrize("path_id", [p[0] for p in PATHS])
@pytest.mark.parametrize("name", ["common_chol", "common_svd", "common_two"])
def test_common_signal_mode_responses(ctx, capi, name, path_id, mix_mfma):
    out = run_case(ctx, capi, name, path_id, mix_mfma=mix_mfma)
    lay = layout(name)
    L = lay.sigs[0]["L"]  # the Cholesky factor of common_chol and common_two: its upper triangle answers exactly 0
    if name != "common_svd":
        assert np.all(np.triu(L, 1) == 0) and np.all(np.diag(L) != 0)
        for p in range(lay.P - 1):
            assert np.all(responses(lay, out, 0, p)[p + 1:] == 0.0), p


def test_coalesced_member_keeps_to_its_modes(ctx, capi):
    """The 12-mode member of the coalesced grid signal answers with modes 1 .. 12 of its own truth and nothing of modes
    13 .. 30 (test_per_pulsar_mode_responses holds it to the allowances): its coefficient lands in the 30-mode
    anchor's column of the same mode, so its block equals the anchor's first 12 modes bit for bit."""
    lay = layout("coalesced")
    gs = G.grid_signals(lay.plan)
    assert [g["members"] for g in gs] == [[0, 1], [2]] and [g["anchor"] for g in gs] == [0, 2]
    ctx.set_option(capi.OPT_SYNTH_PATH, 4)
    upload(ctx, lay)
    out = run_from_z(ctx, lay)
    Y = direct_yardsticks("coalesced")
    for p in range(lay.P):
        anchor, member = responses(lay, out, 0, p), responses(lay, out, 1, p)
        np.testing.assert_array_equal(member, anchor[:12])  # the same grid, the same coefficient column values
        assert compare(member, Y[0][p].truth[:12], np.full((12, 2, 1), TOL * AMP * Y[0][p].chmax)) <= 1.0


# ------------------------------------------------------------------------------------------------ D. drawing kernels
def _fused_instance(name):
    assert name.startswith("k_grid_fused<") and name.endswith(">"), name
    nq, odd, gen, half = name[len("k_grid_fused<"):-1].split(", ")
    return int(nq), odd == "true", gen == "true", half == "true"


@pytest.mark.parametrize("fused", ["shipped", 0])
@pytest.mark.parametrize("name", ["drawn_c2", "drawn_dm"])
def test_drawn_blocks_against_their_coefficients(ctx, capi, name, fused):
    """The kernels that draw inside themselves (k_grid_fused<.., GEN>, C2's shaped instance among them, and with
    FPTA_OPT_INTERP_FUSED 0 k_grid_dft_gen): a plain block against the model driven by the same block's coefficient
    dump. Flat spectrum, 64 realizations."""
    lay, R, seed = layout(name), 64, 20240611
    ctx.set_option(capi.OPT_SYNTH_PATH, 4)
    if fused != "shipped":
        set_or_skip(ctx, capi, capi.OPT_INTERP_FUSED, fused)
    upload(ctx, lay)
    _, co = ctx.batch_synth(seed, 0, R, coeffs=True)
    ctx.debug_fill_out(np.nan)
    out = ctx.batch_synth(seed, 0, R)
    gi, shape = ctx.batch_grid_info(), ctx.debug_fused_shape()
    print(f"{name} INTERP_FUSED {fused}: {gi['interp_kernel']} shape {shape}")
    assert gi["last_path"] == 4 and np.all(np.isfinite(out))
    if fused == "shipped":  # draws in the kernel, from an even realization; C2's pattern on its shaped instance
        nq, odd, gen, half = _fused_instance(gi["interp_kernel"])
        assert (odd, gen) == (False, True), gi
        assert shape == (GEN_LOAD if name == "drawn_c2" else 0), shape
        if not capi.build_flags() & capi.BUILD_DIAG:
            assert gi["interp_kernel"] == "k_grid_fused<12, false, true, false>", gi
    else:  # k_grid_dft_gen draws, the warp-specialised kernel interpolates
        assert shape == -1, shape
        if not capi.build_flags() & capi.BUILD_DIAG:
            assert gi["interp_kernel"] == "k_grid_interp_ws<false>", gi
    gs, of, GY = grid_yardsticks(name, 1.0)
    assert gi["grid_signals"] == len(gs)
    Y = direct_yardsticks(name, 1.0)
    col0 = np.concatenate([[0], np.cumsum([2 * (s["nm"] + (s["nm"] & 1)) for s in lay.sigs])])
    assert co.shape == (lay.P, col0[-1], R)
    worst = worst_truth = 0.0
    for p in range(lay.P):
        n_p = int(lay.n[p])
        pred, bound, truth, tbound = (np.zeros((R, n_p), dtype=LD) for _ in range(4))
        for si, s in enumerate(lay.sigs):
            nm, gy = s["nm"], GY[of[si]][p]
            c = co[p, col0[si]:col0[si] + 2 * nm, :].reshape(nm, 2, R).astype(LD)
            Yk = (4.0 * gy.lit[:nm] + (gy.w + 8) * EPS * gy.tot[:nm]).astype(LD)
            pred += np.einsum("kcr,kct->rt", c, gy.M[:nm])
            bound += np.einsum("kcr,kct->rt", np.abs(c), Yk)
            truth += np.einsum("kcr,kct->rt", c, Y[si][p].truth)
            tbound += (TOL * Y[si][p].chmax * np.abs(c).sum(axis=(0, 1)))[:, None]
        blk = out[:, psr(lay, p)].astype(LD)
        worst = max(worst, float((np.abs(blk - pred) / bound).max()))
        worst_truth = max(worst_truth, float((np.abs(blk - truth) / tbound).max()))
    print(f"{name} INTERP_FUSED {fused}: block - model over allowance {worst:.3g}; block - truth over 1e-10 sum |c| ch "
          f"{worst_truth:.3g}")
    assert worst <= 1.0 and worst_truth <= 1.0


# ------------------------------------------------------------------------------------------------ the test of the tests
@pytest.mark.parametrize("wrong", ["q_off_by_one", "row_scaled"])
@pytest.mark.parametrize("name", ["per_psr", "top_modes", "coalesced", "dense_one", "top_modes_257", "common_chol",
                                  "common_two"])
def test_a_wrong_model_fails_where_parity_passes(ctx, capi, name, wrong):
    """A model with q_k taken one mode off, or with the top mode's table row of every grid signal scaled by 1 + 1e-9, is
    rejected by the gridded allowance in every gridded layout (worst ratio above 10), while assert_parity at 1e-10
    passes the scaled row on a red spectrum of 30 modes and more: the scaled and the right model's blocks are compared
    that way here. CPU model side only: the device block is the correct one."""
    from tests.conftest import assert_parity
    lay = layout(name)
    ctx.set_option(capi.OPT_SYNTH_PATH, 4)
    upload(ctx, lay)
    out = run_from_z(ctx, lay)
    good, _ = check_block(lay, out, "grid")
    bad, _ = check_block(lay, out, "grid", wrong=wrong)
    print(f"{name} {wrong}: worst ratio {bad:.3g} against the wrong model, {good:.3g} against the right one")
    assert good <= 1.0 and bad > 10.0
    if wrong == "row_scaled":  # what the suite's own comparison makes of the same defect, gamma = 3 amplitudes
        _, _, right = grid_yardsticks(name, AMP)
        _, _, scaled = grid_yardsticks(name, AMP, wrong)
        for gr, gs in zip(right, scaled):
            if gr[0].M.shape[0] < 30:  # 4 or 8 modes: the top one is no weak mode, parity would see it
                continue
            a = np.arange(1, gr[0].M.shape[0] + 1, dtype=np.float64) ** -1.5
            for p in range(lay.P):
                assert_parity(np.einsum("k,kct->t", a, gs[p].M.astype(float)),
                              np.einsum("k,kct->t", a, gr[p].M.astype(float)), TOL)
