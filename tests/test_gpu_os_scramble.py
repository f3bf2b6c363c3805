"""Sky scrambles of the optimal statistic on the GPU (k_scr_orf, k_scr_stats, k_scr_pairs, k_scr_gemm and k_scr_rank
behind fpta_os_scrambles, fpta_batch_set_os_scrambles, fpta_batch_os_scrambles and fpta_os_scramble_match) and the
Python surface above them, against the np.longdouble definition.

Qs is held to the definition applied to the device's own X, contracted as Y and then Q: |Qs - truth| <= (K + n_pair + 5)
eps sum_{a<b} |G_ab| sum_m phi_hat_m (|c_a c_b| + |s_a s_b|), a K-term and then an n_pair-term dot product; a matrix
with one nonzero pair to 8 eps of its one term's magnitude. The Hellings-Downs rows are held to the formula in long
double from the same fp64 positions: 4 eps |G'(x)| for the rounding of x and 6 eps of the evaluation's terms. norm,
match and the null's moments are held to the dot-product bounds of their sums. The counts are integers and exact.
Each test prints its largest error / bound."""
import numpy as np
import pytest

from tests.test_gpu_os import _Psr, pair_case, pair_weights

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
LD = np.longdouble


@pytest.fixture(scope="module")
def capi():
    from fakepta_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def ctx(capi):
    c = capi.Context(0)
    yield c
    c.close()


def one_shot(ctx, c, res, G_obs, **kw):
    return ctx.os_scrambles(c["offs"], c["toas"], c["nu"], c["n_modes"], c["f"], c["idx"], c["freqf"], c["phi"],
                            c["target"], c["phi_hat"], G_obs, res, weights=c["w"], full=True, **kw)


def observed(rng, P, n=2):
    G = rng.normal(size=(n, P, P))
    return G + G.transpose(0, 2, 1)


def scramble_weights(rng, P, J):
    """pair_weights' matrices as scrambles: a sparse one that came out without any pair has no norm and would be
    refused, so it gets its first pair."""
    G = pair_weights(rng, P, J)
    for g in G:
        if not np.any(np.tril(g, -1)):
            g[1, 0] = g[0, 1] = 1.0
    return G


def y_truth(X, phi_hat):
    """(Y [n_pair, R] longdouble, its magnitude sum_m phi_hat_m (|c_a c_b| + |s_a s_b|)) from X [P, K, R]."""
    P, K, R = X.shape
    ia, ib = np.tril_indices(P, -1)
    ph = np.concatenate([phi_hat, phi_hat]).astype(LD)[None, :, None]
    Xl = X.astype(LD)
    prod = Xl[ia] * Xl[ib] * ph  # [pairs, K, R]
    return prod.sum(axis=1), np.abs(prod).sum(axis=1)


# (P, N, R, J): the issue's shapes, and one more than k_scr_gemm's tile on its three axes (128 scrambles, 64
# realizations, a chunk of 16 pairs: 7 pulsars have 21)
SHAPES = [(2, 1, 1, 1), (3, 5, 17, 17), (17, 30, 16, 3), (33, 5, 33, 257), (33, 1, 1, 17), (100, 5, 17, 65),
          (7, 2, 65, 129)]


@pytest.mark.parametrize("P,N,R,J", SHAPES)
def test_scrambled_q_is_the_definition_applied_to_the_device_x(ctx, P, N, R, J):
    from fakepta_amd import os as osm
    c = pair_case(P, N, 1000 * P + 10 * N + R)
    rng = np.random.default_rng(J)
    G = scramble_weights(rng, P, J)
    G_obs = observed(rng, P)
    res = rng.normal(0.0, 1e-6, (R, int(c["offs"][-1])))
    out = one_shot(ctx, c, res, G_obs, matrices=G)
    X, Qs, nab = out["X"], out["Qs"], out["N_ab"]
    assert Qs.shape == (J, R) and X.shape == (P, 2 * N, R) and out["snr_null"].shape == (J, R)
    assert np.any(Qs != 0)
    ia, ib = np.tril_indices(P, -1)
    n_pair, K = len(ia), 2 * N
    Y, mag = y_truth(X, c["phi_hat"])
    Gp = G[:, ia, ib]
    truth = Gp.astype(LD) @ Y
    bound = ((K + n_pair + 5) * EPS * (np.abs(Gp).astype(LD) @ mag)).astype(np.float64)
    err = np.abs(Qs.astype(LD) - truth).astype(np.float64)
    print(f"P {P} N {N} R {R} J {J}: largest Qs error / bound {float(np.max(err / np.maximum(bound, 1e-300))):.4f}")
    assert np.all(err <= bound)
    if J >= 3:
        a, b = (P - 1, P // 2) if P > 2 else (1, 0)
        e = a * (a - 1) // 2 + b
        one = (LD(1.5) * Y[e]).astype(np.float64)
        lim = 8 * EPS * 1.5 * mag[e].astype(np.float64)
        print(f"  the single pair: largest error / (8 eps term) {float(np.max(np.abs(Qs[1] - one) / lim)):.4f}")
        assert np.all(np.abs(Qs[1] - one) <= lim)  # the single pair, nothing else
    # the explicit matrices' norms are os.norms', and the S/N is Qs / sqrt(norm) to 2 eps
    want = osm.norms(G, nab)
    assert np.all(np.abs(out["norm"] - want) <= (n_pair + 3) * EPS * want)
    snr = Qs / np.sqrt(out["norm"])[:, None]
    assert np.all(np.abs(out["snr_null"] - snr) <= 2 * EPS * np.abs(snr))


def hd_long_double(pos):
    """(G, x, the issue's bound) of every pair a > b of pos [J, P, 3], in long double from the fp64 positions."""
    P = pos.shape[1]
    ia, ib = np.tril_indices(P, -1)
    pl = pos.astype(LD)
    x = (1 - np.sum(pl[:, ia] * pl[:, ib], axis=-1)) / 2
    lx = np.log(x)
    G = LD(1.5) * x * lx - x / 4 + LD(0.5)
    bound = 4 * EPS * np.abs(LD(1.5) * (lx + 1) - LD(0.25)) + 6 * EPS * (np.abs(LD(1.5) * x * lx) + x / 4 + LD(0.5))
    return G, x, bound


@pytest.mark.parametrize("P,J", [(2, 1), (17, 33), (100, 65)])
def test_hellings_downs_rows_norm_and_match_from_positions(ctx, P, J):
    from fakepta_amd import os as osm
    pos = osm.scramble_positions(J, P, seed=100 * P + J)
    G, x, bound = hd_long_double(pos)
    assert float(x.min()) > 1e-9  # the first-order term of x's rounding is the whole story
    rng = np.random.default_rng(P)
    ref = observed(rng, P, 3)
    ref[0] = osm.hd_matrix(osm.scramble_positions(1, P, seed=1)[0])
    match, rows = ctx.os_scramble_match(pos, ref, rows=True)
    err = np.abs(rows.astype(LD) - G)
    print(f"P {P} J {J}: largest HD row error / bound {float(np.max(err / bound)):.4f}, min x {float(x.min()):.3g}")
    assert np.all(err <= bound)
    # match: the dot products' bounds on top of the row errors
    ia, ib = np.tril_indices(P, -1)
    n = len(ia)
    Gr = ref[:, ia, ib].astype(LD)  # [n_ref, pairs]
    num = G @ Gr.T  # [J, n_ref]
    d_num = bound @ np.abs(Gr).T + (n + 3) * EPS * (np.abs(G) @ np.abs(Gr).T)
    A = np.sum(Gr * Gr, axis=1)[None, :]
    B = np.sum(G * G, axis=1)[:, None]
    dA = (n + 3) * EPS * A
    dB = np.sum((2 * np.abs(G) + bound) * bound, axis=1)[:, None] + (n + 3) * EPS * B
    want = num / np.sqrt(A * B)
    # first order the two sums under the root count half; they are taken whole, which covers the higher orders
    d_match = d_num / np.sqrt(A * B) + np.abs(want) * (dA / A + dB / B) + 8 * EPS * np.abs(want)
    em = np.abs(match.astype(LD) - want)
    print(f"  largest match error / bound {float(np.max(em / d_match)):.4f}")
    assert np.all(em <= d_match) and np.all(np.abs(match) <= 1 + 1e-12)
    # norm, through the one-shot call on the same positions: sum G^2 N_ab with the device's N_ab
    c = pair_case(P, 2, 7 * P)
    res = rng.normal(0.0, 1e-6, (1, int(c["offs"][-1])))
    out = one_shot(ctx, c, res, ref, pos=pos)
    nab = out["N_ab"][ia, ib].astype(LD)[None, :]
    norm_t = np.sum(G * G * nab, axis=1)
    d_norm = np.sum((2 * np.abs(G) + bound) * bound * nab, axis=1) + (n + 3) * EPS * norm_t
    en = np.abs(out["norm"].astype(LD) - norm_t)
    print(f"  largest norm error / bound {float(np.max(en / d_norm)):.4f}")
    assert np.all(en <= d_norm)
    np.testing.assert_array_equal(out["match"], match)  # the same kernels, the same bits


def test_ranks_are_exact_and_the_moments_within_their_bounds(ctx):
    from fakepta_amd import os as osm
    P, N, R, J = 12, 4, 33, 257
    c = pair_case(P, N, 4242)
    rng = np.random.default_rng(5)
    G_obs = observed(rng, P, 3)
    pos = osm.scramble_positions(J, P, seed=9)
    res = rng.normal(0.0, 1e-6, (R, int(c["offs"][-1])))
    out = one_shot(ctx, c, res, G_obs, pos=pos)
    null, obs = out["snr_null"], out["snr_obs"]
    assert null.shape == (J, R) and obs.shape == (3, R) and out["count_ge"].dtype == np.int64
    want = np.array([[np.sum(null[:, r] >= obs[o, r]) for r in range(R)] for o in range(3)])
    np.testing.assert_array_equal(out["count_ge"], want)  # integers: exactly the count of the downloaded numbers
    assert 0 < want.min() or want.max() < J  # not all at one end
    snr = osm.derive(out["Q"], G_obs, out["N_ab"], 3)["snr"]
    rel = np.abs(obs - snr) / np.abs(snr)
    print(f"snr_obs against derive(): largest relative difference {float(rel.max() / EPS):.2f} eps")
    assert np.all(rel <= 4 * EPS)
    nl = null.astype(LD)
    mean_t = nl.sum(axis=0) / J
    d_mean = (J + 2) * EPS * np.abs(nl).sum(axis=0) / J
    dev = nl - mean_t
    var_t = np.sum(dev * dev, axis=0) / J
    std_t = np.sqrt(var_t)
    d_std = ((J + 4) * EPS * var_t + 2 * np.abs(dev).sum(axis=0) / J * d_mean) / (2 * std_t) + 2 * EPS * std_t
    e_mean, e_std = np.abs(out["mean"] - mean_t), np.abs(out["std"] - std_t)
    print(f"null moments: largest mean error / bound {float(np.max(e_mean / d_mean)):.4f}, std "
          f"{float(np.max(e_std / d_std)):.4f}")
    assert np.all(e_mean <= d_mean) and np.all(e_std <= d_std)
    np.testing.assert_array_equal(out["max"], null.max(axis=0))
    d = osm.derive_scrambles(obs, out["count_ge"], J, out["mean"], out["std"], out["max"], n_orf=1)
    np.testing.assert_array_equal(d["p_value"], (1.0 + want[:1]) / (1.0 + J))


def test_a_scramble_gives_the_same_bits_whatever_the_other_scrambles(ctx):
    P, N, R = 33, 5, 17
    c = pair_case(P, N, 77)
    rng = np.random.default_rng(9)
    G = scramble_weights(rng, P, 258)
    G_obs = observed(rng, P, 1)
    res = rng.normal(0.0, 1e-6, (R, int(c["offs"][-1])))
    full = one_shot(ctx, c, res, G_obs, matrices=G)
    # alone, first, last, among 2, 9, 65 and 257 others
    for sel in ([7], [7, 0], [0, 7], [3, 7, 1], list(range(10)), list(range(66)), [257] + list(range(257)),
                list(range(257, -1, -1))):
        got = one_shot(ctx, c, res, G_obs, matrices=np.ascontiguousarray(G[sel]))
        np.testing.assert_array_equal(got["Qs"], full["Qs"][sel])
        np.testing.assert_array_equal(got["snr_null"], full["snr_null"][sel])
        np.testing.assert_array_equal(got["norm"], full["norm"][sel])
        np.testing.assert_array_equal(got["snr_obs"], full["snr_obs"])


def test_a_realization_gives_the_same_bits_whatever_the_block(ctx):
    from fakepta_amd import os as osm
    P, N, J = 17, 5, 20
    c = pair_case(P, N, 78)
    rng = np.random.default_rng(10)
    G_obs = observed(rng, P, 2)
    pos = osm.scramble_positions(J, P, seed=4)
    res = rng.normal(0.0, 1e-6, (33, int(c["offs"][-1])))
    full = one_shot(ctx, c, res, G_obs, pos=pos)
    # blocks of 1, 16, 17 and 33, at any position
    for sel in ([0], [32], list(range(16)), list(range(16, 33)), list(range(32, -1, -1)), [5, 31, 6]):
        got = one_shot(ctx, c, np.ascontiguousarray(res[sel]), G_obs, pos=pos)
        for key in ("Qs", "snr_null", "snr_obs", "count_ge"):
            np.testing.assert_array_equal(got[key], full[key][:, sel], err_msg=key)
        for key in ("mean", "std", "max"):
            np.testing.assert_array_equal(got[key], full[key][sel], err_msg=key)


# ----------------------------------------------------------------------------- batch path
@pytest.fixture(scope="module")
def small(ctx):
    """12 pulsars of 40 TOAs, red noise and an HD-correlated common process of 4 modes each, white noise, a design of 3
    columns, as a BatchSimulator."""
    from fakepta_amd.batch import BatchSimulator, batch_factor
    from oracle import fakepta_oracle as O
    rng = np.random.default_rng(31)
    P, n = 12, 40
    span = 3.0e8
    pos = rng.normal(size=(P, 3))
    pos /= np.linalg.norm(pos, axis=1)[:, None]
    psrs = []
    for p in range(P):
        t = np.sort(rng.uniform(0.0, span, n))
        psrs.append(_Psr(t, rng.choice([800.0, 1400.0, 2500.0], n), rng.uniform(2e-7, 6e-7, n) ** 2, pos[p],
                         np.stack([np.ones(n), t / span, (t / span) ** 2], axis=1)))
    f = np.arange(1, 5) / span
    f_rn = np.tile(f, (P, 1))
    amp_rn = np.sqrt(O.powerlaw(f_rn, rng.uniform(-13.6, -13.2, (P, 1)), 3.0) / span)
    amp_gw = np.sqrt(O.powerlaw(f, -13.5, 13 / 3) / span)
    sim = BatchSimulator(psrs, signals=[], white=True, ctx=ctx)
    sim.add_signal("red_noise", 0, f_rn, amp_rn)
    sim.add_signal("gw_common", 1, f, amp_gw, L=batch_factor(O.orf_hd(pos)))
    sim.set_timing_model()
    return sim, psrs


def one_shot_of(sim, psrs, block, positions):
    """The one-shot call with the tables set_optimal_statistic and set_sky_scrambles gave the library."""
    from fakepta_amd import os as osm
    from fakepta_amd import tm
    model = osm.noise_model(sim.segments, len(psrs))
    t = osm.pick_target(sim.segments)
    M, ncol = osm.design_of(psrs, "tm", "test")
    offs = np.concatenate([[0], np.cumsum([len(p.toas) for p in psrs])]).astype(np.int64)
    return sim.ctx.os_scrambles(offs, np.concatenate([p.toas for p in psrs]), np.concatenate([p.freqs for p in psrs]),
                                model["n_modes"], model["f"], model["idx"], model["freqf"], model["phi"], t,
                                osm.template_of(model, t), sim._os["G"], block, pos=positions, masks=model["masks"],
                                M=M, ncol_psr=ncol, weights=tm.weights_of(psrs, "white", int(offs[-1])), full=True)


def test_batch_scrambles_end_to_end(ctx, small):
    from fakepta_amd import os as osm
    sim, psrs = small
    P, R, J = 12, 33, 65
    sim.set_optimal_statistic(orfs=("hd", "monopole"))
    match, norm = sim.set_sky_scrambles(n=J, seed=3, max_match=0.1)
    assert match.shape == (J, 2) and norm.shape == (J,) and np.all(norm > 0)
    assert np.all(np.abs(match[:, 0]) <= 0.1)  # only scrambles of a small match with the true sky are kept
    raw = ctx.os_scramble_match(osm.scramble_positions(256, P, [3, 0]), sim._os["G"][:1])
    assert np.any(np.abs(raw) > 0.1)  # and the rule does reject candidates at this size
    pos = sim._scr["positions"]
    assert pos.shape == (J, P, 3)
    keep = np.abs(raw[:, 0]) <= 0.1
    np.testing.assert_array_equal(pos, osm.scramble_positions(256, P, [3, 0])[keep][:J])  # the first J, in order
    np.testing.assert_array_equal(match[:, 0], raw[keep, 0][:J])
    assert ctx.batch_os_scrambles_info() == dict(n_scr=J, n_g=2, n_pair=66, n_real=0)
    sim.synth(R, seed=5, to_host=False)
    sums = sim.checksums()
    before = sim.optimal_statistic()
    out = sim.sky_scrambles(full=True)
    np.testing.assert_array_equal(sim.checksums(), sums)  # the block is untouched
    after = sim.optimal_statistic()
    for key in ("Q", "A2", "snr"):
        np.testing.assert_array_equal(after[key], before[key])
    assert ctx.batch_os_scrambles_info()["n_real"] == R
    assert out["p_value"].shape == (2, R) and out["snr_null"].shape == (J, R) and out["null_max"].shape == (R,)
    assert np.all(out["p_value"] >= 1 / (J + 1)) and np.all(out["p_value"] <= 1)
    np.testing.assert_array_equal(out["p_value"], (1.0 + out["count_ge"]) / (1.0 + J))
    rel = np.abs(out["snr"] - before["snr"]) / np.abs(before["snr"])
    assert np.all(rel <= 4 * EPS)
    # the one-shot call on the downloaded block: the same kernels, the same bits
    one = one_shot_of(sim, psrs, ctx.batch_download(0, R), pos)
    np.testing.assert_array_equal(one["norm"], norm)
    np.testing.assert_array_equal(one["match"], match)
    np.testing.assert_array_equal(one["Q"], before["Q"])
    for key, other in (("snr", "snr_obs"), ("count_ge", "count_ge"), ("null_mean", "mean"), ("null_std", "std"),
                       ("null_max", "max"), ("snr_null", "snr_null")):
        np.testing.assert_array_equal(out[key], one[other], err_msg=key)
    lean = sim.sky_scrambles()
    assert "snr_null" not in lean
    np.testing.assert_array_equal(lean["p_value"], out["p_value"])
    # an HD background on the sky it was drawn for: the observed S/N sits high in the null of most realizations
    print(f"HD p-values over {R} realizations: median {float(np.median(out['p_value'][0])):.3f}, "
          f"null mean {float(out['null_mean'].mean()):.3f}, null std {float(out['null_std'].mean()):.3f}")


def test_scrambles_leave_the_next_block_alone(ctx, small):
    sim, psrs = small
    sim.set_optimal_statistic()
    sim.set_sky_scrambles(n=20, seed=1)
    outs = []
    for stat in (False, True):
        for real0 in (0, 48):
            ctx.batch_synth(11, real0, 48, to_host=False)
        if stat:
            pre = ctx.batch_download(0, 48)
            assert sim.sky_scrambles()["p_value"].shape == (1, 48)
            np.testing.assert_array_equal(ctx.batch_download(0, 48), pre)
        outs.append(ctx.batch_synth(11, 96, 48))
    np.testing.assert_array_equal(outs[1], outs[0])


def test_state_errors_and_what_clears_the_scrambles(capi, ctx, small):
    from fakepta_amd import os as osm
    sim, psrs = small
    P = 12
    sim.set_optimal_statistic()
    sim.synth(8, seed=2, to_host=False)
    pos = osm.scramble_positions(9, P, seed=8)
    with pytest.raises(capi.FptaError, match=r"\(-77\).*no sky scrambles are set"):
        sim.sky_scrambles()
    match, norm = sim.set_sky_scrambles(positions=pos)
    assert match.shape == (9, 1) and ctx.batch_os_scrambles_info()["n_scr"] == 9
    ref = sim.sky_scrambles(full=True)
    # a refused set keeps the scrambles that were set
    bad = pos.copy()
    bad[4, 2] *= 1.001
    same = pos.copy()
    same[3, 1] = same[3, 0]  # coincident directions
    for kw, msg in ((dict(positions=bad), r"\(-22\).*scramble 4, pulsar 2: position is not of unit length"),
                    (dict(positions=same), r"\(-22\).*scramble 3, pair \(0, 1\): pair weight is not finite"),
                    (dict(matrices=np.triu(np.ones((2, P, P)), 1)), r"\(-22\).*scramble 0, pair \(0, 1\): not symmetric"),
                    (dict(matrices=np.zeros((1, P, P))), r"\(-22\).*scramble 0: norm is not positive")):
        with pytest.raises(capi.FptaError, match=msg):
            sim.set_sky_scrambles(**kw)
        got = sim.sky_scrambles(full=True)
        for key in ref:
            np.testing.assert_array_equal(got[key], ref[key], err_msg=key)
    with pytest.raises(ValueError, match="not both"):
        sim.set_sky_scrambles(positions=pos, matrices=np.zeros((1, P, P)))
    # explicit matrices: the scrambles' own Hellings-Downs matrices made in numpy differ from the device's rows by
    # d, and the norms then by at most sum d (|G1| + |G2|) N_ab and the two sums' own bounds
    mats = np.array([osm.hd_matrix(p) for p in pos])
    _, rows = ctx.os_scramble_match(pos, mats[:1], rows=True)
    il = np.tril_indices(P, -1)
    m2, n2 = sim.set_sky_scrambles(matrices=mats)
    g2 = mats[:, il[0], il[1]]
    nab = sim._os["nab"][il]
    lim = np.sum(np.abs(g2 - rows) * (np.abs(g2) + np.abs(rows)) * nab, axis=1) + (66 + 3) * EPS * (n2 + norm)
    assert m2.shape == match.shape and np.all(np.abs(n2 - norm) <= lim)
    # one FPTA_K_DENSE entry per call
    ctx.set_option(capi.OPT_PROFILE, 1)
    try:
        ctx.reset_stats()
        sim.sky_scrambles()
        ctx.synchronize()
        assert ctx.kernel_stats(capi.K_DENSE)[0] == 1
    finally:
        ctx.set_option(capi.OPT_PROFILE, 0)
    # n = 0 clears them; set_optimal_statistic clears them; so does a new layout
    sim.set_sky_scrambles(n=0)
    assert ctx.batch_os_scrambles_info()["n_scr"] == 0
    sim.set_sky_scrambles(positions=pos)
    sim.set_optimal_statistic()
    assert ctx.batch_os_scrambles_info()["n_scr"] == 0 and sim._scr is None
    with pytest.raises(capi.FptaError, match="no sky scrambles are set"):
        sim.sky_scrambles()
    c = capi.Context(0)
    try:
        p = pair_case(3, 2, 3)
        with pytest.raises(capi.FptaError, match=r"\(-77\).*no optimal statistic is set"):
            c.batch_set_os_scrambles(pos=osm.scramble_positions(2, 3, seed=1))
        c.batch_set_toas(p["offs"], p["toas"], p["nu"])
        c.batch_add_signal(1, p["f"], np.sqrt(p["phi"]), L=np.eye(3))
        with pytest.raises(capi.FptaError, match=r"\(-77\).*no optimal statistic is set"):
            c.batch_set_os_scrambles(pos=osm.scramble_positions(2, 3, seed=1))
        c.batch_set_os(p["n_modes"], p["f"], p["idx"], p["freqf"], p["phi"], 0, p["phi_hat"], np.ones((1, 3, 3)),
                       weights=p["w"])
        c.batch_set_os_scrambles(pos=osm.scramble_positions(2, 3, seed=1))
        with pytest.raises(capi.FptaError, match=r"\(-77\).*nothing synthesized"):
            c.batch_os_scrambles()
        assert c.batch_os_scrambles_info()["n_scr"] == 2
        c.batch_set_toas(p["offs"], p["toas"], p["nu"])
        assert c.batch_os_scrambles_info()["n_scr"] == 0
    finally:
        c.close()
    from fakepta_amd.batch import BatchSimulator
    fresh = BatchSimulator(psrs, signals=[], white=True, ctx=capi.Context(0))
    try:
        with pytest.raises(ValueError, match="no optimal statistic is set"):
            fresh.set_sky_scrambles(n=4)
        with pytest.raises(ValueError, match="no optimal statistic is set"):
            fresh.sky_scrambles()
    finally:
        fresh.ctx.close()


def test_sky_scrambles_reports_the_acceptance_rate_when_it_cannot_reach_n(ctx):
    from fakepta_amd import os as osm
    true = osm.scramble_positions(1, 12, seed=2)[0]
    with pytest.raises(ValueError, match=r"acceptance rate"):
        osm.sky_scrambles(ctx, true, 50, seed=1, max_match=1e-6, max_tries=2)
    pos, match = osm.sky_scrambles(ctx, true, 50, seed=1, max_match=0.2)
    assert pos.shape == (50, 12, 3) and match.shape == (50, 1) and np.all(np.abs(match) <= 0.2)
    again, _ = osm.sky_scrambles(ctx, true, 50, seed=1, max_match=0.2)
    np.testing.assert_array_equal(again, pos)


# ----------------------------------------------------------------------------- drop-in
def test_drop_in_equals_the_one_shot_call(ctx):
    from fakepta import correlated_noises as cn
    from fakepta import fake_pta as fp
    from fakepta_amd import os as osm
    from fakepta_amd import tm
    np.random.seed(12)
    psrs = fp.make_fake_array(npsrs=6, Tobs=10, ntoas=60, gaps=True, toaerr=1e-7, pdist=1.0,
                              freqs=[800, 1400, 2500], backends=["A", "B"],
                              custom_model={"RN": 10, "DM": 10, "Sv": None})
    cn.add_common_correlated_noise(psrs, orf="hd", spectrum="powerlaw", name="gw", components=6, log10_A=-13.5,
                                   gamma=13 / 3)
    keep = [p.residuals.copy() for p in psrs]
    out = fp.optimal_statistic_scrambles_array(psrs, n=40, seed=2, max_match=0.3, orfs=("hd", "monopole"), full=True)
    for p, k in zip(psrs, keep):
        np.testing.assert_array_equal(p.residuals, k)
    assert out["p_value"].shape == (2, 1) and out["snr_null"].shape == (40, 1) and out["match"].shape == (40, 2)
    assert np.all(np.abs(out["match"][:, 0]) <= 0.3)
    segs = osm.segments_of(psrs)
    model = osm.noise_model(segs, 6)
    G, n_orf, _, _ = osm.pair_matrices(psrs, ("hd", "monopole"), None)
    offs = np.concatenate([[0], np.cumsum([len(p.toas) for p in psrs])]).astype(np.int64)
    M, ncol = tm.stack_design([p.Mmat for p in psrs])
    one = ctx.os_scrambles(offs, np.concatenate([p.toas for p in psrs]), np.concatenate([p.freqs for p in psrs]),
                           model["n_modes"], model["f"], model["idx"], model["freqf"], model["phi"], 2,
                           model["phi"][0, 20:26], G, np.concatenate([p.residuals for p in psrs]),
                           pos=out["positions"], M=M, ncol_psr=ncol,
                           weights=np.concatenate([1 / p._white_sigma2() for p in psrs]), full=True)
    for key, other in (("snr", "snr_obs"), ("count_ge", "count_ge"), ("null_mean", "mean"), ("null_std", "std"),
                       ("null_max", "max"), ("snr_null", "snr_null"), ("norm", "norm"), ("match", "match"), ("Q", "Q")):
        np.testing.assert_array_equal(out[key], one[other], err_msg=key)
    np.testing.assert_array_equal(out["p_value"], (1.0 + one["count_ge"]) / 41.0)
