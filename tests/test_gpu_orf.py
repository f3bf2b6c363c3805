"""fpta_orf_anisotropic on the GPU (k_orf_aniso + k_orf_reduce) and the Python surface above it, against the 50-digit
truths of tests/golden/g12_orf.npz where they exist and the np.longdouble model of tests/orf_reference.py elsewhere.

Tolerance of every comparison with a truth: the GPU's max error may be at most 4 x the fp64 numpy model's max error
against the same truth (the chunked MFMA accumulation order differs from numpy's pairwise sums), with the floor
64 eps max|ORF|. Every case asserts min over (pulsar, pixel) of D >= 1e-3 on its own inputs, where the literal fp64
error stays near 1e-15 of the peak."""
import numpy as np
import pytest

from tests import orf_reference as R

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


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
def auto_split(ctx, capi):
    ctx.set_option(capi.OPT_ORF_SPLIT, 0)
    yield
    ctx.set_option(capi.OPT_ORF_SPLIT, 0)


@pytest.fixture(scope="module")
def g(golden):
    return golden("g12_orf.npz")


_CASES = {}


def case(g, n_psr, nside):
    """(pos, maps, truth, fp64 model) of a shape, made once: the fixture's where it has the shape, else drawn here
    (rejection at D >= 1e-3) with the np.longdouble truth."""
    key = (n_psr, nside)
    if key not in _CASES:
        name = f"p{n_psr}n{nside}"
        if f"{name}_truth" in g:
            pos, maps, truth = g[f"{name}_pos"], g[f"{name}_maps"], g[f"{name}_truth"]
        else:
            rng = np.random.default_rng(1000 * n_psr + nside)
            pos, maps = R.draw_positions(rng, n_psr, nside), R.draw_maps(rng, 1, nside)
            truth = R.orf_longdouble(pos, maps)
        assert R.min_d(pos, nside) >= R.D_MIN
        _CASES[key] = (pos, maps, truth, R.orf_numpy(pos, maps))
    return _CASES[key]


def check(got, truth, model, what=""):
    """The tolerance of the module docstring; prints the figures before it asserts."""
    peak = np.max(np.abs(truth))
    e_gpu, e_np = np.max(np.abs(got - truth)), np.max(np.abs(model - truth))
    bound = max(4.0 * e_np, 64.0 * EPS * peak)
    print(f"{what}: GPU error {e_gpu:.3e} ({e_gpu / peak:.2e} of peak), numpy model {e_np:.3e}, "
          f"ratio {e_gpu / e_np if e_np else float('inf'):.2f}, bound {bound:.3e}")
    assert e_gpu <= bound, (what, e_gpu, bound)


# ----------------------------------------------------------------------------- truth
@pytest.mark.parametrize("n_psr,nside", [(1, 1), (5, 2), (16, 3), (5, 4), (65, 4), (17, 8), (130, 8)])
def test_matches_the_truth(ctx, g, n_psr, nside):
    """One tile / two tile rows with an off-diagonal tile (130), ragged 16- and 64-edges, a non-power-of-two nside,
    a single chunk that is not full (nside 1: 12 pixels) and the fixture's three maps (P 5, nside 2)."""
    pos, maps, truth, model = case(g, n_psr, nside)
    got = ctx.orf_anisotropic(pos, nside, maps)
    assert got.shape == truth.shape == (len(maps), n_psr, n_psr)
    for m in range(len(maps)):
        np.testing.assert_array_equal(got[m], got[m].T)
        check(got[m], truth[m], model[m], f"P {n_psr} nside {nside} map {m}")


# ----------------------------------------------------------------------------- K-splits
@pytest.mark.parametrize("n_psr", [17, 130])
def test_k_splits(ctx, capi, g, n_psr):
    pos, maps, truth, model = case(g, n_psr, 8)
    auto = ctx.orf_anisotropic(pos, 8, maps)
    plan = capi.orf_plan(n_psr, 8)
    assert plan["n_chunks"] == 48 and 1 <= plan["n_split"] <= 48
    seen = {}
    for split in (1, 2, 3, 7):
        ctx.set_option(capi.OPT_ORF_SPLIT, split)
        assert ctx.get_option(capi.OPT_ORF_SPLIT) == split
        assert capi.orf_plan(n_psr, 8, split=split)["n_split"] == split
        got = ctx.orf_anisotropic(pos, 8, maps)
        check(got[0], truth[0], model[0], f"P {n_psr} split {split}")
        np.testing.assert_array_equal(got, ctx.orf_anisotropic(pos, 8, maps))  # a repeated call: bit for bit
        seen[split] = got
    ctx.set_option(capi.OPT_ORF_SPLIT, plan["n_split"])
    np.testing.assert_array_equal(ctx.orf_anisotropic(pos, 8, maps), auto)  # auto is the split count it reports
    if plan["n_split"] in seen:
        np.testing.assert_array_equal(seen[plan["n_split"]], auto)
    ctx.set_option(capi.OPT_ORF_SPLIT, 1000)  # clamped to the chunk count
    assert capi.orf_plan(n_psr, 8, split=1000)["n_split"] == 48
    check(ctx.orf_anisotropic(pos, 8, maps)[0], truth[0], model[0], f"P {n_psr} split 1000 -> 48")


# ----------------------------------------------------------------------------- maps
@pytest.mark.parametrize("n_map", [1, 3, 9])
def test_maps_share_a_call_without_changing(ctx, capi, g, n_map):
    """Map m of a batched call is the single-map call bit for bit (9 maps cross a map group of 4), and the ORF is
    linear in the map within the tolerance."""
    pos = case(g, 17, 8)[0]
    maps = R.draw_maps(np.random.default_rng(77), 9, 8)[:n_map]
    assert capi.orf_plan(17, 8, n_map)["n_groups"] == (n_map + 3) // 4
    batched = ctx.orf_anisotropic(pos, 8, maps)
    for m in range(n_map):
        np.testing.assert_array_equal(batched[m], ctx.orf_anisotropic(pos, 8, maps[m:m + 1])[0])
    if n_map >= 3:
        combo = 2.0 * maps[0] + maps[1]
        truth = R.orf_longdouble(pos, combo[None, :])[0]
        model = R.orf_numpy(pos, combo)
        check(2.0 * batched[0] + batched[1], truth, model, f"linearity, {n_map} maps")
        check(ctx.orf_anisotropic(pos, 8, combo[None, :])[0], truth, model, "the combined map")


# ----------------------------------------------------------------------------- structure
def test_output_is_fully_overwritten_and_zero_map_gives_zeros(ctx, g):
    pos, maps, truth, model = case(g, 130, 8)
    out = np.full((1, 130, 130), np.nan)
    assert ctx.orf_anisotropic(pos, 8, maps, out=out) is out
    assert np.all(np.isfinite(out))
    np.testing.assert_array_equal(out[0], out[0].T)
    check(out[0], truth[0], model[0], "NaN-poisoned output")
    zeros = ctx.orf_anisotropic(pos, 8, np.zeros_like(maps))
    assert np.all(zeros == 0.0)
    assert ctx.orf_anisotropic(np.zeros((0, 3)), 8, maps).shape == (1, 0, 0)  # no pulsars: a no-op


def test_uniform_map_is_hellings_downs(ctx):
    """h = 1 at nside 16 against hd(): the GPU may deviate by the numpy model's own quadrature error on these positions
    plus 1e-9 (20 random pulsars: no rejection is possible between the pixel centres of nside 16)."""
    pos = R.random_positions(np.random.default_rng(16), 20)
    h = np.ones((1, 12 * 16 * 16))
    hd = R.hd_matrix(pos)
    quad = np.max(np.abs(R.orf_numpy(pos, h)[0] - hd))
    dev = np.max(np.abs(ctx.orf_anisotropic(pos, 16, h)[0] - hd))
    print(f"nside 16: GPU deviation from hd() {dev:.3e}, numpy model {quad:.3e}")
    assert quad < 2e-3 and dev <= quad + 1e-9


# ----------------------------------------------------------------------------- a pulsar on a pixel centre
def test_pulsar_on_a_pixel_centre_gives_a_nan_row_and_column(ctx, capi):
    theta, phi = capi.pix2ang_ring(3, [48])
    assert phi[0] == 0.0 and abs(theta[0] - np.pi / 2) <= EPS  # pixel 48 of nside 3: z = 0, phi = 0 exactly
    rng = np.random.default_rng(3)
    others, maps = R.draw_positions(rng, 5, 3), R.draw_maps(rng, 2, 3)
    pos = np.insert(others, 2, [1.0, 0.0, 0.0], axis=0)
    got = ctx.orf_anisotropic(pos, 3, maps)
    keep = np.array([0, 1, 3, 4, 5])
    assert np.all(np.isnan(got[:, 2, :])) and np.all(np.isnan(got[:, :, 2]))
    rest = got[:, keep][:, :, keep]
    assert np.all(np.isfinite(rest))
    truth, model = R.orf_longdouble(others, maps), R.orf_numpy(others, maps)
    for m in range(2):
        check(rest[m], truth[m], model[m], f"beside the coincident pulsar, map {m}")


# ----------------------------------------------------------------------------- validation
def test_validation_names_the_index_and_leaves_the_output(ctx, capi, g):
    pos, maps = g["p5n2_pos"], g["p5n2_maps"]
    out = np.full((3, 5, 5), -7.0)

    def refused(match, pos=pos, nside=2, maps=maps):
        with pytest.raises(capi.FptaError, match=match):
            ctx.orf_anisotropic(pos, nside, maps, out=out)
        assert np.all(out == -7.0)
    refused("nside 0", nside=0)
    refused("nside 1025", nside=1025)
    refused("npix 48 is not 12 nside", nside=3)           # maps of nside 2 handed over as nside 3
    refused("npix 47 is not 12 nside", maps=maps[:, :47])
    bad = maps.copy()
    bad[1, 17] = np.nan
    refused("map 1, pixel 17", maps=bad)
    bad[1, 17] = np.inf
    refused("map 1, pixel 17", maps=bad)
    far = pos.copy()
    far[3] *= 1.0 + 1e-6
    refused("pulsar 3: position is not a unit vector", pos=far)
    far[3, 1] = np.nan
    refused("pulsar 3: position not finite", pos=far)
    ctx.orf_anisotropic(pos * (1.0 + 5e-9), 2, maps, out=out)  # within 1e-8 of unit length: accepted
    assert np.all(out != -7.0)


# ----------------------------------------------------------------------------- the Python surface
def _array(n_psr, nside, seed):
    from fakepta import fake_pta as fp
    np.random.seed(seed)
    psrs = fp.make_fake_array(npsrs=n_psr, Tobs=10, ntoas=60, gaps=False, isotropic=True, toaerr=1e-7,
                              backends="X.1400", custom_model={"RN": None, "DM": None, "Sv": None})
    rng = np.random.default_rng(seed)
    for p, v in zip(psrs, R.draw_positions(rng, n_psr, nside)):
        p.pos = v
    pos = np.array([p.pos for p in psrs])
    assert R.min_d(pos, nside) >= R.D_MIN
    return psrs, pos, R.draw_maps(rng, 3, nside)


def test_drop_in_functions(ctx):
    from fakepta import correlated_noises as cn
    from fakepta_amd import orf
    psrs, pos, maps = _array(6, 4, 21)
    one = cn.anisotropic(psrs, maps[0])
    np.testing.assert_array_equal(one, orf.anisotropic_orf(pos, maps[0]))
    np.testing.assert_array_equal(one, cn.orf_matrix(psrs, "anisotropic", maps[0]))
    assert one.shape == (6, 6)
    check(one, R.orf_longdouble(pos, maps[0]), R.orf_numpy(pos, maps[0]), "anisotropic(psrs, h_map)")
    many = cn.anisotropic_array(psrs, maps)
    assert many.shape == (3, 6, 6)
    np.testing.assert_array_equal(many[0], one)
    assert orf.npix2nside(192) == 4
    with pytest.raises(ValueError):
        orf.npix2nside(191)
    with pytest.raises(ValueError):
        cn.anisotropic(psrs, maps[0][:-1])


def test_add_common_correlated_noise_anisotropic(ctx):
    """The injection with orf='anisotropic' against host numpy built from the truth ORF: the same draws, orf_factor,
    residuals and fourier to 1e-10; hmap is stored; reconstruct_signal gives the injected signal back; BatchSimulator
    replays the signal_model and matches the oracle given the same ORF matrix."""
    from fakepta import correlated_noises as cn
    from fakepta_amd.batch import BatchSimulator
    from oracle import fakepta_oracle as O
    from tests.conftest import assert_parity
    from tests.helpers import oracle_segments
    psrs, pos, maps = _array(6, 4, 22)
    h, nm = maps[1], 12
    before = [p.residuals.copy() for p in psrs]
    state = np.random.get_state()
    cn.add_common_correlated_noise(psrs, orf="anisotropic", h_map=h, log10_A=-14.0, gamma=13 / 3, components=nm)
    np.random.set_state(state)
    z = np.empty((nm, 2, 6))
    for k in range(nm):
        z[k, 0] = np.random.standard_normal(6)
        z[k, 1] = np.random.standard_normal(6)
    sm = psrs[0].signal_model["gw_common"]
    assert sm["orf"] == "anisotropic" and sm["hmap"] is h
    truth = R.orf_longdouble(pos, h)
    L = cn.orf_factor(truth)
    res, fourier = O.common_synth_loop([p.toas for p in psrs], [p.freqs for p in psrs], sm["f"], sm["psd"], z, L, 0.0)
    delta = np.concatenate([p.residuals - b for p, b in zip(psrs, before)])
    assert_parity(delta, np.concatenate(res), 1e-10)
    got = np.array([p.signal_model["gw_common"]["fourier"] for p in psrs])
    want = np.array(fourier)
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-10 * np.abs(want).max())
    for p, b in zip(psrs, before):
        assert_parity(p.reconstruct_signal(["gw_common"]), p.residuals - b, 1e-10)
    sim = BatchSimulator(psrs, white=False, ctx=ctx)
    np.testing.assert_allclose(sim.segments[0]["L"] @ sim.segments[0]["L"].T, truth, rtol=0, atol=1e-12)
    offs = np.concatenate([[0], np.cumsum([len(p.toas) for p in psrs])])
    want = O.batch_synth(offs, np.concatenate([p.toas for p in psrs]), np.concatenate([p.freqs for p in psrs]),
                         oracle_segments(sim), 5, 0, 32)
    assert_parity(sim.synth(32, seed=5), want, 1e-10)
