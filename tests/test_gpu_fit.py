"""The Fourier fit on the GPU (k_fit_apply and k_fit_cross behind fpta_fit_coefficients, fpta_batch_set_fit,
fpta_batch_fit and fpta_batch_fit_cross) and the Python surface above it, against the np.longdouble definition of
tests/fit_reference.py.

Tolerance of every comparison with the truth, per pulsar and row: |got - truth| <= max(4 e_lit, (n_p + 2) eps sum_t
|A_kt| |r_t|). e_lit is the error of the literal fp64 numpy evaluation (column-scaled lstsq, same rcond); the second
term is the rigorous bound of a length-n_p fp64 dot product in any order with a once-rounded operator, from the truth's
A. Every truth asserts on its own inputs that each kept column's orthogonalised norm is >= 1e-4 and each dropped one's
<= 1e-13, so the rank decision is never what a test measures. Each test prints the measured ratios (DESIGN.md section
5i)."""
import numpy as np
import pytest

from tests import fit_reference as F
from tests import ld_reference as LDR
from tests import tm_reference as T
from tests.helpers import common_signal, per_psr_signal, random_layout

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
LD = np.longdouble
YEAR = 365.25 * 86400.0
SPAN = 15 * YEAR
# one ragged array: rows of the block start at odd offsets; 0 TOAs, fewer TOAs than columns, one chunk of 64 TOAs and
# its partial forms (1 .. 33), several chunks with a tail (250, 309, 600) and without one (2000 = 31 chunks + 16)
N_PSR = (0, 1, 5, 15, 16, 17, 33, 250, 309, 600, 2000)
M_PSR = (8, 0, 8, 16, 0, 8, 16, 8, 16, 0, 8)  # nuisance columns per pulsar: none, make_Mmat's 8, 8 offsets more
N_VEC = 33
# K = 2, 16, 18, 60, 208, 512: one row (8 TOA slices per row group), exactly one group, one group + 2 (4 slices), four
# groups (2 slices), 13 groups (a wave owns two) and the limit, 32 groups (a wave owns four)
CONFIGS = {
    "k2": dict(seed=11, comps=[(1, 0.0)], weighted=False, per_psr=False),
    "k16": dict(seed=12, comps=[(8, 0.0)], weighted=True, per_psr=False),
    "k18": dict(seed=11, comps=[(5, 0.0), (4, 2.0)], weighted=True, per_psr=True),
    "k60": dict(seed=14, comps=[(30, 0.0)], weighted=True, per_psr=False),
    "k208": dict(seed=11, comps=[(100, 0.0), (4, 2.0)], weighted=False, per_psr=False),
    # at the limit the pulsars of 250, 309 and 600 TOAs are left out: with fewer TOAs than about 2 K the
    # last columns a pulsar keeps come out of the Gram-Schmidt passes at 1e-10 .. 1e-5 for every seed tried (389), and
    # the truth's own conditioning assertion refuses them; k208 has those pulsars on the same kernel instance
    "k512": dict(seed=11, comps=[(256, 0.0)], weighted=False, per_psr=False,
                 n=(0, 1, 5, 15, 16, 17, 33, 2000), m=(8, 0, 8, 16, 16, 8, 16, 8)),
}
# the seeds are the first from 11 on whose inputs pass the conditioning assertion (a 16-TOA pulsar that keeps its
# sixteenth column, or a 33-TOA one its thirty-third, does so at an arbitrary norm)


def shape_of(name):
    cfg = CONFIGS[name]
    return cfg.get("n", N_PSR), cfg.get("m", M_PSR)


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


def jumps(rng, n, k):
    """k offset columns between random halves of the TOAs (what a backend or an epoch flag selects). The smooth
    columns of tests/test_gpu_tm.py are sinusoids of 1.5 .. 6 cycles, nearly in the span of the Fourier columns that
    follow them: those then come out of the Gram-Schmidt passes at 1e-10 .. 1e-5, inside the band a truth must avoid."""
    return (rng.uniform(size=(n, k)) < 0.5).astype(np.float64)


_CASES = {}


def case(name):
    """A configuration's inputs, truth and literal form, made once and never changed."""
    if name not in _CASES:
        from fakepta_amd import tm
        cfg = CONFIGS[name]
        rng = np.random.default_rng(cfg["seed"])
        n_psr, m_psr = shape_of(name)
        P = len(n_psr)
        offs = np.concatenate([[0], np.cumsum(n_psr)]).astype(np.int64)
        toas, nu, mats = [], [], []
        for n, m in zip(n_psr, m_psr):
            t = np.sort(rng.uniform(0.0, SPAN, n))
            v = T.three_band(rng, n)
            full = np.concatenate([T.mmat(t, v), jumps(rng, n, 8)], axis=1) if n else np.zeros((0, 16))
            toas.append(t)
            nu.append(v)
            mats.append(full[:, :m].copy())
        toas, nu = np.concatenate(toas), np.concatenate(nu)
        n_modes = np.array([c[0] for c in cfg["comps"]], dtype=np.int32)
        idx = np.array([c[1] for c in cfg["comps"]])
        freqf = np.full(len(idx), 1400.0)
        spans = [max(float(np.ptp(toas[offs[p]:offs[p + 1]])) if n_psr[p] else 0.0, YEAR) if cfg["per_psr"] else SPAN
                 for p in range(P)]
        f_rows = np.stack([np.concatenate([np.arange(1, N + 1) / spans[p] for N in n_modes]) for p in range(P)])
        f = f_rows if cfg["per_psr"] else f_rows[0].copy()
        edges = np.concatenate([[0], np.cumsum(n_modes)])

        def comps_of(p):
            return [(f_rows[p, edges[c]:edges[c + 1]], idx[c], freqf[c]) for c in range(len(n_modes))]

        M, ncol = tm.stack_design(mats)
        w = 1 / rng.uniform(1e-7, 1e-6, int(offs[-1])) ** 2 if cfg["weighted"] else None
        res = rng.normal(0.0, 1e-6, (N_VEC, int(offs[-1])))
        truth, kept, As, bound = F.fit_truth(offs, toas, nu, mats, w, comps_of, res)
        literal = F.fit_literal(offs, toas, nu, mats, w, comps_of, res, kept)
        c = dict(offs=offs, toas=toas, nu=nu, mats=mats, M=M, ncol=ncol, w=w, res=res, n_modes=n_modes, f=f, idx=idx,
                 freqf=freqf, comps_of=comps_of, truth=truth, kept=kept, As=As, bound=bound, literal=literal,
                 K=2 * int(n_modes.sum()), n_psr=n_psr)
        for a in (M, ncol, res, toas, nu, f):
            a.flags.writeable = False
        _CASES[name] = c
    return _CASES[name]


def check_against_truth(label, got, truth, literal, bound, kept, n_psr=None):
    """The module's tolerance per pulsar and row; prints the measured ratios, returns the largest error / tolerance."""
    tol, e_lit = F.tolerance(truth, literal, bound)
    err = np.abs(got.astype(LD) - truth).astype(np.float64)
    worst = 0.0
    for p in range(got.shape[0]):
        assert np.all(got[p][~kept[p]] == 0.0), (label, p)  # dropped rows are exact zeros
        if not kept[p].any():
            continue
        ratio = np.where(tol[p] > 0, err[p] / np.where(tol[p] > 0, tol[p], 1.0), np.where(err[p] > 0, np.inf, 0.0))
        rb = np.where(bound[p] > 0, err[p] / np.where(bound[p] > 0, bound[p], 1.0), 0.0)
        n = "" if n_psr is None else f" (n {n_psr[p]})"
        print(f"{label} pulsar {p}{n}: kept {int(kept[p].sum())}, error / tolerance {ratio.max():.3f}, error / "
              f"dot-product bound {rb.max():.3f}, literal error / bound "
              f"{float(np.max(e_lit[p] / np.maximum(bound[p].max(axis=1, keepdims=True), 1e-300))):.2f}")
        assert np.all(err[p] <= tol[p]), (label, p, float(ratio.max()))
        worst = max(worst, float(ratio.max()))
    return worst


def one_shot(ctx, c, res, mats="case", w="case"):
    M, ncol = (c["M"], c["ncol"]) if mats == "case" else (None, None)
    return ctx.fit_coefficients(c["offs"], c["toas"], c["nu"], c["n_modes"], c["f"], c["idx"], c["freqf"], res, M=M,
                                ncol_psr=ncol, weights=c["w"] if w == "case" else w)


# ----------------------------------------------------------------------------- one-shot
@pytest.mark.parametrize("n_vec", [1, 16, 33])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_one_shot_matches_the_truth(ctx, name, n_vec):
    c = case(name)
    coef, rank, kept = one_shot(ctx, c, c["res"][:n_vec])
    assert coef.shape == (len(c["n_psr"]), c["K"], n_vec)
    np.testing.assert_array_equal(kept, c["kept"])
    np.testing.assert_array_equal(rank, c["kept"].sum(axis=1))
    assert rank[0] == 0 and np.all(coef[0] == 0.0)  # the pulsar without TOAs
    worst = check_against_truth(f"{name} n_vec {n_vec}", coef, c["truth"][:, :, :n_vec], c["literal"][:, :, :n_vec],
                                c["bound"][:, :, :n_vec], c["kept"], c["n_psr"])
    print(f"{name} n_vec {n_vec}: largest error / tolerance {worst:.3f}")
    if n_vec == 1:  # a one-dimensional residual vector is one realization
        one, _, _ = one_shot(ctx, c, c["res"][0])
        np.testing.assert_array_equal(one, coef)


@pytest.mark.parametrize("name", ["k18", "k60"])
def test_exactness(ctx, name):
    """r = F a0 with nothing marginalised returns a0 (0 in the rows the rank rule drops), and r = M b with M
    marginalised returns 0, both under the module's bound."""
    c = case(name)
    rng = np.random.default_rng(5)
    offs, P, K = c["offs"], len(c["n_psr"]), c["K"]
    r = np.zeros((16, int(offs[-1])))
    a0 = rng.normal(0.0, 1e-7, (P, K, 16))
    for p in range(P):
        sl = slice(int(offs[p]), int(offs[p + 1]))
        r[:, sl] = (F.columns_ld(c["toas"][sl], c["nu"][sl], c["comps_of"](p)) @ a0[p].astype(LD)).T.astype(np.float64)
    truth, kept, _, bound = F.fit_truth(offs, c["toas"], c["nu"], None, c["w"], c["comps_of"], r)
    literal = F.fit_literal(offs, c["toas"], c["nu"], None, c["w"], c["comps_of"], r, kept)
    coef, _, got_kept = one_shot(ctx, c, r, mats=None)
    np.testing.assert_array_equal(got_kept, kept)
    check_against_truth(f"{name} r = F a0", coef, truth, literal, bound, kept, c["n_psr"])
    for p in range(P):
        if kept[p].all():  # every column kept: the amplitudes themselves come back, to the rounding of F a0 and the fit
            tol = F.tolerance(truth[p:p + 1], literal[p:p + 1], bound[p:p + 1])[0][0]
            assert np.all(np.abs(coef[p] - a0[p]) <= 2 * tol), p  # the truth is a0 within eps / 2 sum |A| |r| itself
    rb = np.zeros((16, int(offs[-1])))
    for p, A in enumerate(c["mats"]):
        if A.shape[1] and A.shape[0]:
            rb[:, offs[p]:offs[p + 1]] = (rng.normal(0.0, 1e-6, (16, A.shape[1])) / np.max(np.abs(A), axis=0)) @ A.T
    truth, kept, _, bound = F.fit_truth(offs, c["toas"], c["nu"], c["mats"], c["w"], c["comps_of"], rb)
    literal = F.fit_literal(offs, c["toas"], c["nu"], c["mats"], c["w"], c["comps_of"], rb, kept)
    coef, _, _ = one_shot(ctx, c, rb)
    check_against_truth(f"{name} r = M b", coef, truth, literal, bound, kept, c["n_psr"])
    tol = F.tolerance(truth, literal, bound)[0]
    assert np.all(np.abs(coef) <= 2 * tol)  # the truth itself is 0 to its own rounding of M b


@pytest.mark.parametrize("name", ["k2", "k16", "k18", "k60", "k208", "k512"])
def test_blocks_and_order_do_not_change_a_bit(ctx, name):
    c = case(name)
    res = c["res"]
    whole, _, _ = one_shot(ctx, c, res)
    # every one-shot call plans its operator again: a second at K = 208, three at K = 512. Those two (the same kernel
    # instance, two and four row groups per wave) take fewer calls: blocks of 16 rows, and at K = 512 only the last 17
    # rows as a block of their own; the reversed order below moves every row to another tile position in all cases
    if name == "k512":
        np.testing.assert_array_equal(one_shot(ctx, c, res[16:])[0], whole[:, :, 16:])
    for size in (() if name == "k512" else (16,) if name == "k208" else (1, 16)):
        parts = [one_shot(ctx, c, res[i:i + size])[0] for i in range(0, N_VEC, size)]
        np.testing.assert_array_equal(np.concatenate(parts, axis=2), whole)
    rev, _, _ = one_shot(ctx, c, res[::-1].copy())
    np.testing.assert_array_equal(rev[:, :, ::-1], whole)


# ----------------------------------------------------------------------------- batch path
class _Psr:
    """What BatchSimulator reads of a pulsar."""

    def __init__(self, toas, freqs, sigma2, pos):
        self.toas, self.freqs, self.sigma2, self.pos = toas, freqs, sigma2, pos
        self.Mmat = T.mmat(toas, freqs)
        self.signal_model = {}

    def _white_sigma2(self):
        return self.sigma2


P_B = 12


@pytest.fixture(scope="module")
def batch(ctx, capi):
    """Red noise (30 modes) and a Hellings-Downs background (30 modes) on 12 ragged pulsars of 200 .. 600 TOAs."""
    from fakepta_amd.batch import BatchSimulator
    rng = np.random.default_rng(41)
    offs, toas, nu = random_layout(rng, P_B, (200, 600))
    sig2 = rng.uniform(1e-7, 1e-6, int(offs[-1])) ** 2
    f, a, L, pos = common_signal(rng, offs, toas, 30)
    psrs = [_Psr(toas[offs[i]:offs[i + 1]], nu[offs[i]:offs[i + 1]], sig2[offs[i]:offs[i + 1]], pos[i])
            for i in range(P_B)]
    sim = BatchSimulator(psrs, signals=[], white=False, ctx=ctx)
    fr, ar = per_psr_signal(rng, offs, toas, 30)
    sim.add_signal("red_noise", 0, fr, ar)
    sim.add_signal("gw_common", 1, f, a, L=L)
    sim.set_timing_model()
    return sim, psrs, offs, toas, nu, 1 / sig2


def test_batch_fit_of_a_synthesised_block(ctx, batch):
    sim, psrs, offs, toas, nu, w = batch
    rank, kept = sim.set_fourier_fit(["gw_common"])
    assert kept.shape == (P_B, 60) and np.all(rank == kept.sum(axis=1))
    sim.synth(64, seed=3, to_host=False)
    sim.project()
    before = sim.checksums()
    coef = sim.fourier_fit()
    np.testing.assert_array_equal(sim.checksums(), before)  # the block is untouched
    block = ctx.batch_download(0, 64)
    fg = sim.segments[1]["f"]
    mats = [p.Mmat for p in psrs]
    truth, kept_t, _, bound = F.fit_truth(offs, toas, nu, mats, w, lambda p: [(fg, 0.0, 1400.0)], block)
    literal = F.fit_literal(offs, toas, nu, mats, w, lambda p: [(fg, 0.0, 1400.0)], block, kept_t)
    np.testing.assert_array_equal(kept, kept_t)
    assert coef.shape == (P_B, 60, 64)
    check_against_truth("batch", coef, truth, literal, bound, kept_t, np.diff(offs))
    assert sim.fourier_fit(to_host=False) is None
    ps = sim.power_spectrum()
    assert len(ps) == 1 and ps[0].shape == (P_B, 30) and np.all(np.isfinite(ps[0])) and np.all(ps[0] > 0)
    np.testing.assert_array_equal(sim.checksums(), before)


@pytest.fixture(scope="module")
def shared_span(capi):
    """C2's signal mix on 64 ragged pulsars over one common span (tests/test_gpu_next_mix.py): the layout whose
    pipelined k_grid_fused blocks also make the next block's common-signal mix (FPTA_OPT_FUSED_NEXT_MIX)."""
    from fakepta_amd.batch import batch_factor
    from oracle import fakepta_oracle as O
    c = capi.Context(0)
    rng = np.random.default_rng(17)
    P = 64
    counts = rng.integers(40, 120, size=P)
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    t0, t1 = 0.0, 3.15e8
    toas = np.concatenate([np.concatenate([[t0], np.sort(rng.uniform(t0, t1, k - 2)), [t1]]) for k in counts])
    nu = rng.choice([800.0, 1400.0, 2500.0], size=offs[-1])
    c.batch_set_toas(offs, toas, nu)
    for nm, idx in ((30, 0.0), (100, 2.0)):
        f = np.tile(np.arange(1, nm + 1) / (t1 - t0), (P, 1))
        c.batch_add_signal(0, f, np.sqrt(O.powerlaw(f, rng.uniform(-14.5, -13.5, (P, 1)), 3.0) / (t1 - t0)), idx=idx)
    fc = np.arange(1, 31) / (t1 - t0)
    v = rng.normal(size=(P, 3))
    c.batch_add_signal(1, fc, np.sqrt(O.powerlaw(fc, -14.0, 13 / 3) / (t1 - t0)),
                       L=batch_factor(O.orf_hd(v / np.linalg.norm(v, axis=1)[:, None])))
    c.set_option(capi.OPT_SYNTH_PATH, 4)
    rank, _ = c.batch_set_fit([10], np.arange(1, 11) / (t1 - t0), [0.0], [1400.0])
    assert list(rank) == [20] * P
    yield c
    c.close()


@pytest.mark.parametrize("next_real0,hit", [(384, True), (1000, False)])
def test_fit_leaves_the_block_and_the_next_block_alone(shared_span, next_real0, hit):
    """The block is bit for bit what it was, and the block after a fitted one is bit for bit the block after an
    unfitted one, whether the fitted block's kernel had already made its common-signal mix (the next realizations: a
    next-mix hit) or not (a jump: a miss, the mix is drawn again)."""
    c = shared_span
    outs = []
    for fit in (False, True):
        for real0 in (0, 128, 256):  # hits start at the third block of a pipelined run
            c.batch_synth(7, real0, 128, to_host=False)
        assert c.batch_grid_info()["interp_kernel"].startswith("k_grid_fused<")
        if fit:
            sums, pre = c.batch_checksums(), c.batch_download(0, 128)
            coef = c.batch_fit(20)
            assert coef.shape == (64, 20, 128) and np.all(np.isfinite(coef)) and np.any(coef != 0)
            np.testing.assert_array_equal(c.batch_download(0, 128), pre)
            np.testing.assert_array_equal(c.batch_checksums(), sums)
        outs.append(c.batch_synth(7, next_real0, 128))
        assert c.batch_grid_info()["next_mix_used"] == hit
    np.testing.assert_array_equal(outs[1], outs[0])


# ----------------------------------------------------------------------------- cross-spectrum
@pytest.mark.parametrize("R", [1, 33])
@pytest.mark.parametrize("N", [1, 30])
@pytest.mark.parametrize("P", [1, 3, 16, 17, 100])
def test_cross_spectrum_is_the_gram_of_the_coefficients(capi, P, N, R):
    c = capi.Context(0)
    try:
        rng = np.random.default_rng(100 * P + N + R)
        offs, toas, nu = random_layout(rng, P, (70, 90))
        c.batch_set_toas(offs, toas, nu)
        f, a = per_psr_signal(rng, offs, toas, 8)
        c.batch_add_signal(0, f, a)
        fg = np.arange(1, N + 1) / np.ptp(toas)
        # two components when there is room, so that the cosine and sine rows of a mode are not neighbours
        n_modes = [N, 2] if N > 1 else [N]
        ff = np.concatenate([fg, fg[:2]]) if N > 1 else fg
        rank, _ = c.batch_set_fit(n_modes, ff, [0.0, 2.0][:len(n_modes)], [1400.0] * len(n_modes))
        K, n_mode = 2 * sum(n_modes), sum(n_modes)
        c.batch_synth(5, 0, R, to_host=False)
        coef = c.batch_fit(K)
        X = c.batch_fit_cross(n_mode)
        assert X.shape == (n_mode, P, P)
        np.testing.assert_array_equal(X, X.transpose(0, 2, 1))  # symmetric bit for bit
        cl = coef.astype(LD)
        worst, m0, k0 = 0.0, 0, 0
        for n in n_modes:
            co, si = cl[:, k0:k0 + n], cl[:, k0 + n:k0 + 2 * n]
            want = np.einsum("akr,bkr->kab", co, co) + np.einsum("akr,bkr->kab", si, si)
            mag = np.einsum("akr,bkr->kab", np.abs(co), np.abs(co)) + np.einsum("akr,bkr->kab", np.abs(si), np.abs(si))
            bound = (2 * R + 2) * EPS * mag.astype(np.float64)
            err = np.abs(X[m0:m0 + n].astype(LD) - want).astype(np.float64)
            assert np.all(err <= bound), (P, N, R, float(np.max(err / np.maximum(bound, 1e-300))))
            worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
            m0, k0 = m0 + n, k0 + 2 * n
        print(f"P {P} N {N} R {R}: largest cross-spectrum error / bound {worst:.3f}")
    finally:
        c.close()


def test_cross_spectrum_needs_a_common_grid(capi, ctx, batch):
    sim = batch[0]
    sim.set_fourier_fit(["red_noise"])
    sim.synth(8, seed=3, to_host=False)
    sim.fourier_fit(to_host=False)
    with pytest.raises(capi.FptaError, match=r"\(-22\).*common grid"):
        ctx.batch_fit_cross(30)
    with pytest.raises(ValueError, match="per-pulsar"):
        sim.cross_spectrum()


def test_hd_curve_in_the_fourier_domain_on_a_ragged_array(capi, ctx, batch):
    sim, psrs = batch[0], batch[1]
    sim.set_fourier_fit(["gw_common"])
    sim.synth(48, seed=9, to_host=False)
    X = sim.cross_spectrum(psd=False)
    Xp = sim.cross_spectrum()
    df = np.diff(np.append(0.0, sim.segments[1]["f"]))
    np.testing.assert_array_equal(Xp, X / (2.0 * df)[:, None, None])
    ps = sim.power_spectrum()[0]
    # the same 2 x 48 non-negative terms summed in another order, then the divisions by R and 2 df
    np.testing.assert_allclose(np.diagonal(Xp, axis1=1, axis2=2).T, ps, rtol=(2 * 48 + 8) * EPS)
    mean, std, centres, counts = sim.hd_curve(bins=6, domain="fourier", return_counts=True)
    S = X.sum(axis=0)
    d = np.sqrt(np.diag(S))
    C = S / np.outer(d, d)
    pos = np.array([p.pos for p in psrs])
    iu = np.triu_indices(P_B, 1)
    ang, cor = np.arccos(np.clip(pos @ pos.T, -1.0, 1.0))[iu], C[iu]
    edges = np.linspace(0.0, np.pi, 7)
    assert counts.sum() == len(cor)
    for b in range(6):
        sel = cor[(ang > edges[b]) & (ang < edges[b + 1])]
        assert counts[b] == len(sel)
        if len(sel):
            assert mean[b] == np.mean(sel) and std[b] == np.std(sel)
        else:
            assert np.isnan(mean[b]) and np.isnan(std[b])
    assert np.all(np.abs(np.diag(C) - 1) <= 4 * EPS)
    with pytest.raises(capi.FptaError):  # the time-domain estimator still needs equal TOA counts
        sim.correlations()
    with pytest.raises(ValueError, match="ratio"):
        sim.hd_curve(domain="fourier", estimator="per_realization")


# ----------------------------------------------------------------------------- state
def test_state_errors_and_set_toas_clears_the_fit(capi):
    c = capi.Context(0)
    try:
        rng = np.random.default_rng(3)
        offs, toas, nu = random_layout(rng, 3, (40, 60))
        fg = np.arange(1, 4) / np.ptp(toas)
        with pytest.raises(capi.FptaError, match="set_toas first"):
            c.batch_set_fit([3], fg, [0.0], [1400.0])
        c.batch_set_toas(offs, toas, nu)
        f, a = per_psr_signal(rng, offs, toas, 10)
        c.batch_add_signal(0, f, a)
        with pytest.raises(capi.FptaError, match=r"\(-77\).*nothing synthesized"):
            c.batch_fit(6)
        c.batch_synth(1, 0, 20, to_host=False)
        with pytest.raises(capi.FptaError, match=r"\(-77\).*no fit is set"):
            c.batch_fit(6)
        rank, kept = c.batch_set_fit([3], fg, [0.0], [1400.0])
        assert list(rank) == [6, 6, 6] and kept.all()
        with pytest.raises(capi.FptaError, match=r"\(-77\).*no fit result"):
            c.batch_fit_cross(3)
        assert c.batch_fit_info() == dict(K=6, n_mode=3, common=True, n_real=0)
        coef = c.batch_fit(6)
        assert coef.shape == (3, 6, 20) and c.batch_fit_cross(3).shape == (3, 3, 3)
        assert c.batch_fit_info()["n_real"] == 20
        np.testing.assert_array_equal(c.batch_fit(), coef)  # the buffers are sized from the library's own counts
        assert c.batch_fit_cross().shape == (3, 3, 3)
        with pytest.raises(ValueError, match="6 Fourier columns, not 4"):  # a wrong count is refused, not written past
            c.batch_fit(4)
        with pytest.raises(ValueError, match="3 modes, not 2"):
            c.batch_fit_cross(2)
        # independent of the timing model: setting or clearing one leaves the fit, and the other way round
        M = np.concatenate([T.mmat(toas[offs[i]:offs[i + 1]], nu[offs[i]:offs[i + 1]]) for i in range(3)])
        assert list(c.batch_set_timing_model(M)) == [8, 8, 8]
        np.testing.assert_array_equal(c.batch_fit(6), coef)
        with pytest.raises(capi.FptaError, match=r"\(-22\).*component 0, mode 1"):
            c.batch_set_fit([3], [fg[0], -1.0, fg[2]], [0.0], [1400.0])
        np.testing.assert_array_equal(c.batch_fit(6), coef)  # a refused call leaves the fit that was set
        rank, kept = c.batch_set_fit(None, None, None, None)  # cleared
        assert list(rank) == [0, 0, 0]
        with pytest.raises(capi.FptaError, match="no fit is set"):
            c.batch_fit(6)
        c.batch_project()  # the timing model is still there
        c.batch_set_fit([3], fg, [0.0], [1400.0])
        c.batch_set_toas(offs, toas, nu)  # a new layout: the fit is gone
        c.batch_add_signal(0, f, a)
        c.batch_synth(1, 0, 20, to_host=False)
        with pytest.raises(capi.FptaError, match="no fit is set"):
            c.batch_fit(6)
        c.set_option(capi.OPT_PROFILE, 1)  # one FPTA_K_DENSE entry per fit and per cross-spectrum
        c.batch_set_fit([3], fg, [0.0], [1400.0])
        c.reset_stats()
        c.batch_fit(6, to_host=False)
        c.synchronize()
        assert c.kernel_stats(capi.K_DENSE)[0] == 1
        c.batch_fit_cross(3)
        assert c.kernel_stats(capi.K_DENSE)[0] == 2
    finally:
        c.close()


# ----------------------------------------------------------------------------- drop-in
def test_drop_in_fit_fourier(ctx):
    from fakepta import fake_pta as fp
    np.random.seed(12)
    psrs = fp.make_fake_array(npsrs=3, Tobs=10, ntoas=90, gaps=True, toaerr=1e-7, pdist=1.0,
                              freqs=[800, 1400, 2500], backends=["A", "B"],
                              custom_model={"RN": 10, "DM": 10, "Sv": None})
    offs = np.concatenate([[0], np.cumsum([len(p.toas) for p in psrs])]).astype(np.int64)
    assert len(set(np.diff(offs))) > 1  # ragged
    toas, nu = np.concatenate([p.toas for p in psrs]), np.concatenate([p.freqs for p in psrs])
    res = np.concatenate([p.residuals for p in psrs])
    keep = [p.residuals.copy() for p in psrs]
    w = np.concatenate([1 / p._white_sigma2() for p in psrs])
    mats = [p.Mmat.copy() for p in psrs]

    def comps_of(p):
        return [(np.arange(1, 7) / psrs[p].Tspan, 0.0, 1400.0)]

    truth, kept, _, bound = F.fit_truth(offs, toas, nu, mats, w, comps_of, res)
    literal = F.fit_literal(offs, toas, nu, mats, w, comps_of, res, kept)
    got = fp.fit_fourier_array(psrs, components=6)
    coef = np.zeros((3, 12, 1))
    for i, (f, co) in enumerate(got):
        np.testing.assert_array_equal(f, np.arange(1, 7) / psrs[i].Tspan)
        assert co.shape == (2, 6)
        df = np.diff(np.append(0.0, f))
        coef[i, :, 0] = np.concatenate([co[0] * df, co[1] * df])  # back to amplitudes, one rounding each way
        np.testing.assert_array_equal(psrs[i].residuals, keep[i])
    tol = F.tolerance(truth, literal, bound)[0]
    assert np.all(np.abs(coef.astype(LD) - truth) <= tol + 2 * EPS * np.abs(coef))
    f0, c0 = psrs[0].fit_fourier(components=6)
    np.testing.assert_array_equal(c0, got[0][1])
    # a chromatic component at another reference frequency: columns (1000 / nu)^2 cos / sin
    def chrom_of(p):
        return [(np.arange(1, 6) / psrs[p].Tspan, 2.0, 1000.0)]

    tc, kc, _, bc = F.fit_truth(offs, toas, nu, None, w, chrom_of, res)
    lc = F.fit_literal(offs, toas, nu, None, w, chrom_of, res, kc)
    gc = fp.fit_fourier_array(psrs, components=5, idx=2., marginalize_tm=False, freqf=1000)
    g14 = fp.fit_fourier_array(psrs, components=5, idx=2., marginalize_tm=False)
    cc = np.zeros((3, 10, 1))
    for i, (f, co) in enumerate(gc):
        df = np.diff(np.append(0.0, f))
        cc[i, :, 0] = np.concatenate([co[0] * df, co[1] * df])
        # the columns at 1400 MHz are 1.96 times these: the amplitudes differ by that factor, far outside rounding
        np.testing.assert_allclose(co, g14[i][1] * 1.4 ** 2, rtol=0, atol=1e-9 * np.max(np.abs(co)))
        assert not np.allclose(co, g14[i][1], rtol=0.5)
    assert np.all(np.abs(cc.astype(LD) - tc) <= F.tolerance(tc, lc, bc)[0] + 2 * EPS * np.abs(cc))
    # the convention: the fit of a reconstructed signal alone, nothing marginalised, unit weights, is its stored
    # 'fourier' table. The device is held to the truth by the module's tolerance; that the truth is the table is a
    # property of the definition (rows, order, the division by df), where a mistake is an error of order 1: 1e-6.
    p = psrs[1]
    sm = p.signal_model["red_noise"]
    fs = np.asarray(sm["f"], dtype=np.float64)
    p.residuals = p.reconstruct_signal(["red_noise"])
    o1 = np.array([0, len(p.toas)])
    t1, k1, _, b1 = F.fit_truth(o1, p.toas, p.freqs, None, None, lambda q: [(fs, 0.0, 1400.0)], p.residuals)
    l1 = F.fit_literal(o1, p.toas, p.freqs, None, None, lambda q: [(fs, 0.0, 1400.0)], p.residuals, k1)
    f1, c1 = p.fit_fourier(components=fs, weights=None, marginalize_tm=False)
    df = np.diff(np.append(0.0, fs))
    a1 = np.concatenate([c1[0] * df, c1[1] * df])[None, :, None]
    assert np.all(np.abs(a1.astype(LD) - t1) <= F.tolerance(t1, l1, b1)[0] + 2 * EPS * np.abs(a1))
    stored = np.asarray(sm["fourier"], dtype=np.float64)
    table = (t1[0, :, 0].astype(np.float64).reshape(2, -1) / df)
    assert np.max(np.abs(table - stored)) <= 1e-6 * np.max(np.abs(stored))
    p.residuals = keep[1]
