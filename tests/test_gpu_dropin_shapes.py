"""The one-realization drop-in calls of the C ABI (fpta_common_accumulate, fpta_gp_accumulate[_array],
fpta_white_accumulate: what Pulsar.add_*, add_common_correlated_noise and reconstruct_array run) at the shapes the
golden fixtures never reach: the ORF mix on either side of the k_mix / k_mix_mfma / k_mix_tiled switch at 64 pulsars
with its x_out stores and their host unpacking, ragged arrays with one-TOA pulsars, odd mode counts, ECORR block
layouts that are not contiguous runs, and the Python surface at 100 pulsars.

Truth: tests/ld_reference.py (longdouble evaluation of the header's definitions on the fp64 inputs as given).

Tolerances, none of them measured on the code under test:
  * Residuals: the yardstick of tests/test_gpu_cw.py, computed here at run time. err_ref64 = max over the whole
    array of |literal fp64 oracle - truth| (oracle.common_synth_loop / gp_synth_loop / reconstruct_loop on the same
    inputs, added to the same starting residuals); every pulsar's device error must be <= 4 err_ref64. The device
    forms the phase (2 pi f_k) t in the reference's operation order, so it shares the oracle's dominant error (the
    rounding of a phase of ~10^2 .. 10^4 rad at t ~ 4.5e9 s); its sincos and pow are a few ulp where libm is <= 1.
  * Mixed draws x_out = L z: a dot product of m fp64 products, summed in any order, fused or not, errs by at most
    gamma_m sum |a_i b_i| with gamma_m ~ m eps / 2 (Higham, Accuracy and Stability of Numerical Algorithms, section
    3.1); the bound used is P eps (|L| @ |z|), elementwise: a factor 2 of slack.
  * White noise: out = fl(r + fma(e, zb, fl(sigma z))): three roundings, each at most eps / 2 of a partial sum that
    is itself at most |r| + |sigma z| + |e zb|, so |error| <= 3 eps (|r| + |sigma z| + |e zb|) per TOA.

Device / literal ratios (max over pulsars of the device error, over err_ref64) seen on an MI355X; the bound is 4.
FPTA_OPT_MIX_MFMA 1 and 0 gave the same figures to three digits in every case:

  common_accumulate, 30 red modes     hd_svd    eye   monopole_svd   hd_chol
    P   1                              1.02    0.995     0.967        1.00
    P   2                              1.07    0.997     0.963        0.991
    P  63                              0.977   0.968     0.982        0.991
    P  64                              0.985   0.996     1.00         1.00
    P  65                              1.02    0.993     0.988        0.991
    P 150                              1.01    1.00      1.01         1.03
    P 257                              1.02    1.02      1.03         0.99
    P 300                              1.03    1.00      1.04         1.00
  common_accumulate, 101 flat modes   P 63: 1.00, P 65: 1.00
  gp_accumulate_array                 per pulsar (1, 1, 63, 64, 257 TOAs): 0.011, 0.20, 1.00, 0.83, 0.77
  add_common_correlated_noise, P 100  hd 1.59, curn 1.00, monopole 1.41
  reconstruct_array, P 100            hd 1.00, curn 0.94, monopole 1.00

err_ref64 itself was 6e-15 .. 1.2e-14 of the peak for the red spectrum (one-TOA arrays: 7e-16 .. 2.4e-13) and
4e-13 .. 5e-13 for the flat ones. No case came near 4, so no further term is added to the yardstick: the derived
allowance for the mix, ch sum_k amp_k (bound_cos + bound_sin) with the x_out bounds, would be 2 .. 70 x err_ref64 at
64 pulsars and more and is not needed (x_out itself was within 0.1 of its bound everywhere, and exact for the identity).
"""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import fakepta_oracle as O
from tests import ld_reference as T

pytestmark = pytest.mark.gpu

EPS = T.EPS
LD = np.longdouble
T0, SPAN = 4.5e9, 3.15e8  # real-MJD-like epochs [s]
NUS = (800.0, 1400.0, 2500.0)
FREQF = 1400.0
MIX_P = (1, 2, 63, 64, 65, 150, 257, 300)  # k_mix below 64 pulsars; k_mix_mfma / k_mix_tiled from 64 up
FACTORS = ("hd_svd", "eye", "monopole_svd", "hd_chol")


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
def restore_options(ctx):
    shipped = ctx.options()
    yield
    ctx.set_options(shipped)


def frozen(**kw):
    for v in kw.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False  # shared between tests: nobody changes it
    return SimpleNamespace(**kw)


def ragged_layout(rng, n):
    n = np.asarray(n)
    offs = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    toas = np.concatenate([np.sort(T0 + rng.uniform(0.0, SPAN, k)) for k in n])
    nu = rng.choice(NUS, size=int(offs[-1]))
    return offs, toas, nu


def per_pulsar_max(err, offs):
    return np.array([err[offs[p]:offs[p + 1]].max() for p in range(len(offs) - 1)])


def orf_factor(kind, pos):
    """The factors the drop-in path really receives, plus the batch path's Cholesky factor."""
    if kind == "hd_svd":  # numpy's dense SVD factor (add_common_correlated_noise's orf_factor)
        return O.mvn_factor(O.orf_hd(pos))
    if kind == "eye":  # curn: detected as lower-triangular by the host, the q loop stops at the tile
        return np.eye(len(pos))
    if kind == "monopole_svd":  # rank 1 plus rounding noise in the other columns
        return O.mvn_factor(O.orf_monopole(pos))
    return np.linalg.cholesky(O.orf_hd(pos))  # lower-triangular, dense below the diagonal


@functools.lru_cache(maxsize=None)
def mix_case(P, factor, spectrum):
    """Inputs, truth and yardstick of one fpta_common_accumulate call; computed once, shared by the option values."""
    rng = np.random.default_rng([P, FACTORS.index(factor), len(spectrum)])
    n = rng.integers(1, 41, size=P)
    n[0] = 1  # a one-TOA pulsar first: the partial-wave guards
    offs, toas, nu = ragged_layout(rng, n)
    v = rng.normal(size=(P, 3))
    L = np.ascontiguousarray(orf_factor(factor, v / np.linalg.norm(v, axis=1)[:, None]))
    nm, idx = (30, 2.0) if spectrum == "red" else (101, 0.0)  # 101: the nm + (nm & 1) padding mode
    f = np.arange(1, nm + 1) / SPAN
    df = O.delta_f(f)
    psd = O.powerlaw(f, -14.5, 13 / 3) if spectrum == "red" else 1e-14 / df  # flat: amp = 1e-7
    amp = df ** 0.5 * np.sqrt(psd)  # as add_common_correlated_noise forms it
    z = rng.standard_normal((nm, 2, P))
    delta, x = T.common_truth(offs, toas, nu, f, amp, idx, FREQF, L, z)
    peak = float(np.abs(delta).max())
    r0 = rng.uniform(-0.1, 0.1, int(offs[-1])) * peak  # non-zero starting residuals
    want = r0.astype(LD) + delta
    tl = [toas[offs[p]:offs[p + 1]] for p in range(P)]
    fl = [nu[offs[p]:offs[p + 1]] for p in range(P)]
    res, _ = O.common_synth_loop(tl, fl, f, psd, z, L, idx, FREQF)
    err_ref64 = float(np.abs((r0 + np.concatenate(res)).astype(LD) - want).max())
    x_bound = P * EPS * (np.abs(L) @ np.abs(z[:, ::-1, :])[..., None])[..., 0]  # [nm][2 (cos, sin)][P]
    # what an x in error by x_bound moves the residuals by: ch sum_k amp_k (bound_cos + bound_sin)
    ch = (FREQF / nu) ** idx
    psr_of = np.repeat(np.arange(P), n)
    mix_term = ch * (amp[:, None] * (x_bound[:, 0, :] + x_bound[:, 1, :])).sum(axis=0)[psr_of]
    return frozen(P=P, offs=offs, toas=toas, nu=nu, L=L, f=f, amp=amp, idx=idx, z=z, r0=r0, want=want, x=x,
                  x_bound=x_bound, err_ref64=err_ref64, peak=peak, mix_term=mix_term)


def check_common(ctx, capi, c, mfma, label):
    ctx.set_option(capi.OPT_MIX_MFMA, mfma)
    assert ctx.get_option(capi.OPT_MIX_MFMA) == mfma
    args = (c.offs, c.toas, c.nu, c.f, c.amp, c.idx, FREQF, c.L, c.z)
    # the negated draws first: whatever an earlier call left in the context's x_out buffer is overwritten with
    # something else than this call's answer, and L (-z) = -(L z) bit for bit (every product and sum changes sign)
    x_neg = ctx.common_accumulate(*args[:-1], -c.z, c.r0.copy())
    r = c.r0.copy()
    x = ctx.common_accumulate(*args, r)
    np.testing.assert_array_equal(x_neg, -x)
    xerr = np.abs(x.astype(LD) - c.x)
    print(f"{label}: x_out error / bound {float((xerr / c.x_bound).max()):.3g}")
    assert np.all(xerr <= c.x_bound)
    err = np.abs(r.astype(LD) - c.want)
    worst = per_pulsar_max(err, c.offs)
    print(f"{label}: device error {float(worst.max()):.3e} = {float(worst.max()) / c.err_ref64:.3g} x the literal "
          f"fp64 error {c.err_ref64:.3e} ({c.err_ref64 / c.peak:.1e} of peak); the x_out bound alone would move the "
          f"residuals by {float(c.mix_term.max()) / c.err_ref64:.3g} x")
    assert np.all(worst <= 4 * c.err_ref64)
    again = c.r0.copy()
    np.testing.assert_array_equal(ctx.common_accumulate(*args, again), x)
    np.testing.assert_array_equal(again, r)  # a second identical call: bit-identical
    plain = c.r0.copy()
    assert ctx.common_accumulate(*args, plain, want_x=False) is None
    np.testing.assert_array_equal(plain, r)  # the x_out stores change nothing else


# ----------------------------------------------------------------------------- a. common_accumulate
@pytest.mark.parametrize("mfma", [1, 0])
@pytest.mark.parametrize("factor", FACTORS)
@pytest.mark.parametrize("P", MIX_P)
def test_common_accumulate_across_mix_kernels(ctx, capi, P, factor, mfma):
    """30 modes of a gamma = 13/3 spectrum, chromatic index 2, on ragged pulsars of 1 .. 40 TOAs: x_out within
    P eps (|L| @ |z|) of the longdouble product, every pulsar's residuals within 4 x the literal fp64 oracle's own
    error (module docstring), want_x=False and a repeated call bit-identical."""
    check_common(ctx, capi, mix_case(P, factor, "red"), mfma, f"P {P} {factor} mfma {mfma}")


@pytest.mark.parametrize("mfma", [1, 0])
@pytest.mark.parametrize("P", [63, 65])
def test_common_accumulate_flat_odd_mode_count(ctx, capi, P, mfma):
    """101 modes (padded to 102 on the device) of a flat spectrum, amp 1e-7, no chromatic factor: every mode
    weighs the same, so a wrong column of the padded coefficient layout shows at full size."""
    check_common(ctx, capi, mix_case(P, "hd_svd", "flat"), mfma, f"P {P} flat 101 modes mfma {mfma}")


# ----------------------------------------------------------------------------- b. gp_accumulate_array
@functools.lru_cache(maxsize=None)
def gp_case():
    rng = np.random.default_rng(20)
    n = np.array([1, 1, 63, 64, 257])
    P = len(n)
    offs, toas, nu = ragged_layout(rng, n)
    ntot = int(offs[-1])
    tspan = SPAN * (0.6 + 0.1 * np.arange(P))  # every pulsar its own frequency grid
    half = np.arange(ntot) % 2 == 0
    segs, coeffs, masks = [], [], [None, half, None]
    for nm, idx, kind in ((1, 0.0, "one"), (7, 2.0, "red"), (100, 4.0, "flat")):
        f = np.arange(1, nm + 1)[None, :] / tspan[:, None]
        df = np.stack([O.delta_f(fp) for fp in f])
        psd = {"one": 1e-12 / df, "red": O.powerlaw(f, -13.5, 3.0), "flat": 1e-14 / df}[kind]
        c = np.stack([O.gp_coeffs_from_z(psd[p], rng.standard_normal(2 * nm)) for p in range(P)])
        coeffs.append(c)
        segs.append((f, df ** 0.5 * c[:, 0::2], df ** 0.5 * c[:, 1::2], idx, FREQF))
    delta = T.gp_truth(offs, toas, nu, segs, masks, 1.0)
    peak = float(np.abs(delta).max())
    r0 = rng.uniform(-0.1, 0.1, ntot) * peak
    lit = np.zeros(ntot)
    for s, (f, _, _, idx, _) in enumerate(segs):
        for p in range(P):
            sl = slice(offs[p], offs[p + 1])
            acc = lit[sl]  # a view: gp_synth_loop accumulates in place
            O.gp_synth_loop(toas[sl], nu[sl], f[p], coeffs[s][p], idx, FREQF,
                            mask=None if masks[s] is None else masks[s][sl], residuals=acc)
    want = r0.astype(LD) + delta
    err_ref64 = float(np.abs((r0 + lit).astype(LD) - want).max())
    for sg in segs:
        for a in sg[:3]:
            a.flags.writeable = False
    return frozen(P=P, offs=offs, toas=toas, nu=nu, segs=segs, masks=masks, half=half, r0=r0, want=want, peak=peak,
                  err_ref64=err_ref64)


def test_gp_accumulate_array_ragged(ctx):
    """Pulsars of 1, 1, 63, 64 and 257 TOAs; segments of 1 mode (idx 0), 7 modes (idx 2, masked on every other
    TOA) and 100 flat modes (idx 4). sign = +1 within 4 x the literal fp64 error of the truth for every pulsar;
    sign = -1 then returns to the start: (r + d) - d with the same d, two roundings of numbers below 1.1 peak, so
    within 4 eps peak."""
    c = gp_case()
    r = c.r0.copy()
    ctx.gp_accumulate_array(c.offs, c.toas, c.nu, c.segs, r, sign=1.0, masks=c.masks)
    worst = per_pulsar_max(np.abs(r.astype(LD) - c.want), c.offs)
    print(f"gp_accumulate_array: device error per pulsar / literal fp64 error {c.err_ref64:.3e} "
          f"({c.err_ref64 / c.peak:.1e} of peak): {[f'{float(w) / c.err_ref64:.3g}' for w in worst]}")
    assert np.all(worst <= 4 * c.err_ref64)
    ctx.gp_accumulate_array(c.offs, c.toas, c.nu, c.segs, r, sign=-1.0, masks=c.masks)
    assert np.max(np.abs(r - c.r0)) <= 4 * EPS * c.peak


def test_gp_accumulate_mask_leaves_other_toas_untouched(ctx):
    c = gp_case()
    r = c.r0.copy()
    ctx.gp_accumulate_array(c.offs, c.toas, c.nu, [c.segs[1]], r, masks=[c.half])
    np.testing.assert_array_equal(r[~c.half], c.r0[~c.half])  # bit for bit
    assert np.all(r[c.half] != c.r0[c.half])


def test_gp_accumulate_one_pulsar_equals_array_form(ctx):
    c = gp_case()
    r = c.r0.copy()
    ctx.gp_accumulate_array(c.offs, c.toas, c.nu, c.segs, r, masks=c.masks)
    for p in range(c.P):
        sl = slice(c.offs[p], c.offs[p + 1])
        one = c.r0[sl].copy()
        ctx.gp_accumulate(c.toas[sl], c.nu[sl], [(f[p], cc[p], cs[p], idx, ff) for f, cc, cs, idx, ff in c.segs], one,
                          masks=[None if m is None else m[sl] for m in c.masks])
        np.testing.assert_array_equal(one, r[sl])


# ----------------------------------------------------------------------------- c. white_accumulate
def white_blocks(layout, n):
    if layout == "none":
        return None
    if layout == "singletons":
        return [[t] for t in range(n)]
    if layout == "interleaved":  # members interleaved between blocks, listed in descending order; every fifth TOA
        nb = 3 if n >= 3 else 1  # (t % 5 == 4) in no block
        members = [t for t in range(n) if t % 5 != 4]
        return [sorted((t for t in members if t % nb == b), reverse=True) for b in range(nb)]
    runs = [list(range(s, min(s + 4, n))) for s in range(0, n, 4)]  # "empty": an empty block inside the CSR
    runs.insert(max(1, len(runs) // 2), [])
    return runs


def white_inputs(n, blocks, seed=0):
    rng = np.random.default_rng([n, seed])
    nb = len(blocks) if blocks else 0
    return frozen(sigma=rng.uniform(1e-7, 1e-6, n), z=rng.standard_normal(n), r0=rng.normal(0.0, 5e-7, n),
                  esig=rng.uniform(1e-7, 1e-6, nb), zb=rng.standard_normal(nb))


@pytest.mark.parametrize("layout", ["none", "singletons", "interleaved", "empty"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_white_accumulate_edges(ctx, n, layout):
    """r + sigma z + (ECORR of the block that holds the TOA) against the longdouble sum, within
    3 eps (|r| + |sigma z| + |e zb|) per TOA (module docstring), on either side of the 256-thread block."""
    blocks = white_blocks(layout, n)
    w = white_inputs(n, blocks)
    want = w.r0.astype(LD) + w.sigma.astype(LD) * w.z.astype(LD)
    bound = np.abs(w.r0) + np.abs(w.sigma * w.z)
    for b, members in enumerate(blocks or []):
        m = np.asarray(members, dtype=np.int64)
        want[m] += LD(w.esig[b]) * LD(w.zb[b])
        bound[m] += abs(w.esig[b] * w.zb[b])
    r = w.r0.copy()
    ctx.white_accumulate(w.sigma, w.z, r, blocks, w.esig if blocks else None, w.zb if blocks else None)
    err = np.abs(r.astype(LD) - want)
    print(f"white n {n} {layout}: error / bound {float((err / (3 * EPS * bound)).max()):.3g}")
    assert np.all(err <= 3 * EPS * bound)


def raw_white(ctx, capi, n, sigma, z, boffs, bidx, esig, zb, r):
    boffs, bidx = np.asarray(boffs, dtype=np.int64), np.asarray(bidx, dtype=np.int64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    return capi._lib.fpta_white_accumulate(ctx._h, n, p(sigma), p(z), len(boffs) - 1, p(boffs), p(bidx), p(esig),
                                           p(zb), p(r))


@pytest.mark.parametrize("what,boffs,bidx,message", [
    ("a TOA in two blocks", [0, 3, 6], [0, 1, 2, 5, 2, 7], "two ECORR blocks"),
    ("an index >= n", [0, 3, 6], [0, 1, 2, 5, 257, 7], "out of range"),
    ("a negative index", [0, 3, 6], [0, 1, 2, 5, -1, 7], "out of range"),
    ("boffs[0] != 0", [1, 3, 6], [0, 1, 2, 5, 6, 7], "bad ECORR block CSR"),
])
def test_white_accumulate_refuses_bad_blocks(ctx, capi, what, boffs, bidx, message):
    """Loud failure (FPTA_EINVAL and a message), residuals unchanged bit for bit."""
    n = 257
    w = white_inputs(n, [[], []], seed=1)
    r = w.r0.copy()
    rc = raw_white(ctx, capi, n, w.sigma, w.z, boffs, bidx, w.esig, w.zb, r)
    assert rc == -22, what
    assert message in capi._lib.fpta_last_error(ctx._h).decode()
    np.testing.assert_array_equal(r, w.r0)
    if what == "a TOA in two blocks":  # and through the wrapper: the same refusal as an exception
        with pytest.raises(capi.FptaError, match=message):
            ctx.white_accumulate(w.sigma, w.z, r, [[0, 1, 2], [5, 2, 7]], w.esig, w.zb)
        np.testing.assert_array_equal(r, w.r0)


# ----------------------------------------------------------------------------- d. Python surface, 100 pulsars
@pytest.mark.parametrize("orf", ["hd", "curn", "monopole"])
def test_add_common_correlated_noise_100_pulsars(orf):
    """add_common_correlated_noise on 100 pulsars (k_mix_mfma behind the Python layer): the residuals against the
    truth on the re-drawn normals within the yardstick; every pulsar's stored fourier against x amp0 / sqrt(df)
    (the x_out bound scaled, plus the two roundings of the host's multiply and divide: 2 eps); reconstruct_array
    against its own truth within its own yardstick, and against the injected residuals within both yardsticks
    plus the re-rounding of the coefficients (amp x against df (x amp0 / sqrt(df)): the product, the quotient, the
    square root and df = sqrt(df)^2 (1 + 2 delta) make at most 4 eps relative per coefficient) and the rounding of
    after - before (eps (|after| + |before|))."""
    from fakepta import correlated_noises as cn
    from fakepta import fake_pta as fp
    P, nm = 100, 30
    np.random.seed(100)
    psrs = fp.make_fake_array(npsrs=P, Tobs=10, ntoas=40, gaps=False, isotropic=True, toaerr=1e-7,
                              backends="X.1400", custom_model={"RN": None, "DM": None, "Sv": None})
    assert all(not p.signal_model for p in psrs)  # no per-pulsar signals
    before = np.concatenate([p.residuals for p in psrs])
    assert before.any()
    state = np.random.get_state()
    cn.add_common_correlated_noise(psrs, orf=orf, log10_A=-14.0, gamma=13 / 3, components=nm)
    np.random.set_state(state)
    z = np.empty((nm, 2, P))
    for k in range(nm):
        z[k, 0] = np.random.standard_normal(P)
        z[k, 1] = np.random.standard_normal(P)
    after = np.concatenate([p.residuals for p in psrs])
    offs = np.concatenate([[0], np.cumsum([len(p.toas) for p in psrs])]).astype(np.int64)
    toas, nu = np.concatenate([p.toas for p in psrs]), np.concatenate([p.freqs for p in psrs])
    sm = psrs[0].signal_model["gw_common"]
    f, psd = sm["f"], sm["psd"]
    df = O.delta_f(f)
    amp0, sq_df = np.sqrt(psd), df ** 0.5
    L = np.ascontiguousarray(O.mvn_factor(O.ORFS[orf](np.array([p.pos for p in psrs]))))
    delta, x = T.common_truth(offs, toas, nu, f, sq_df * amp0, 0.0, FREQF, L, z)
    want = before.astype(LD) + delta
    tl, fl = [p.toas for p in psrs], [p.freqs for p in psrs]
    res, _ = O.common_synth_loop(tl, fl, f, psd, z, L, 0.0, FREQF)
    err_inj = float(np.abs((before + np.concatenate(res)).astype(LD) - want).max())
    worst = per_pulsar_max(np.abs(after.astype(LD) - want), offs)
    print(f"add_common_correlated_noise {orf}: device error {float(worst.max()):.3e} = "
          f"{float(worst.max()) / err_inj:.3g} x the literal fp64 error {err_inj:.3e}")
    assert np.all(worst <= 4 * err_inj)
    # stored coefficients
    x_bound = P * EPS * (np.abs(L) @ np.abs(z[:, ::-1, :])[..., None])[..., 0]
    scale = (amp0.astype(LD) / sq_df.astype(LD))[:, None, None]
    four = x * scale  # [nm][2][P]
    got = np.stack([p.signal_model["gw_common"]["fourier"] for p in psrs], axis=-1).transpose(1, 0, 2)
    assert got.shape == four.shape
    assert np.all(np.abs(got.astype(LD) - four) <= x_bound * scale + 2 * EPS * np.abs(four))
    # reconstruction from the stored coefficients: one fpta_gp_accumulate_array call
    rec = np.concatenate(fp.reconstruct_array(psrs, ["gw_common"]))
    stored = got.transpose(2, 1, 0)  # [P][2][nm]
    seg = (np.tile(f, (P, 1)), df * stored[:, 0, :], df * stored[:, 1, :], 0.0, FREQF)
    rec_truth = T.gp_truth(offs, toas, nu, [seg], None, 1.0)
    lit = np.concatenate([O.reconstruct_loop(tl[p], fl[p], f, stored[p], 0.0, FREQF) for p in range(P)])
    err_rec = float(np.abs(lit.astype(LD) - rec_truth).max())
    worst = per_pulsar_max(np.abs(rec.astype(LD) - rec_truth), offs)
    print(f"reconstruct_array {orf}: device error {float(worst.max()):.3e} = {float(worst.max()) / err_rec:.3g} x "
          f"the literal fp64 error {err_rec:.3e}")
    assert np.all(worst <= 4 * err_rec)
    psr_of = np.repeat(np.arange(P), np.diff(offs))
    coef_term = 4 * EPS * ((sq_df * amp0)[:, None] * np.abs(x.astype(np.float64)).sum(axis=1)).sum(axis=0)[psr_of]
    tol = 4 * (err_inj + err_rec) + coef_term + EPS * (np.abs(after) + np.abs(before))
    assert np.all(np.abs(rec - (after - before)) <= tol)
