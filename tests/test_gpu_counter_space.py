"""Every drawing kernel at 64-bit seeds and high realization indices, against the numpy oracle (uint64 throughout,
pinned by the Random123 vectors and, at these very points, by tests/test_counter_space_host.py).

Every output is a function of (seed, global realization g): Philox key (k0, k1) = (seed & 0xFFFFFFFF, seed >> 32),
counter word 3 = g >> 1, with real0 + n_real <= 2^32 on the batch and streamed paths and <= 2^33 for fpta_noise_draw.
The rest of the GPU suite stays at seeds below 2^13 and realizations below 2^13, where k1 == 0 and bit 31 of g is
clear: a kernel or a host call that dropped k1, passed k0 twice, kept g in 32 signed bits or formed g >> 1 after
cutting g would pass it. Here each site that assembles a counter and key of its own runs at

  seeds         S_HI = 0x9E3779B97F4A7C15 (both words nonzero, top bit set), S_K1 = 2^32 (k0 == 0), -1 == 2^64 - 1
  realizations  blocks across bit 31 from 2^31 - 17 (odd) and 2^31 - 16 (even), blocks ending exactly at 2^32 with an
                odd and an even count, and for the dense draws 2^32 - 5 (g >> 1 reaches 2^31) and a block ending at 2^33

on the small layouts the suite already uses for that kernel, with the tolerance of that kernel's existing test (blocks
1e-10 through assert_parity, downloaded coefficients 1e-13 element-wise, dense draws 1e-9; device against device bit
for bit), and asserts the kernel or instance that ran. The calls past the limits are refused and leave the resident
block as it was. tests/counter_space.py holds the points and the comparison helpers; the CPU module shows that every
helper rejects the oracle's own answer under each of those wrong conventions.

k_white is not among the sites: the library only launches it with normals handed in (fpta_white_accumulate), never
with a counter of its own.

Reference loops: the reference's fakepta/fake_pta.py:201-253 (white / ECORR), 372-387 (per-pulsar GP), 518-519 (dense
draws), correlated_noises.py:153-160 (ORF-mixed common signals).
"""
import numpy as np
import pytest

from oracle import fakepta_oracle as O
from tests import counter_space as S
from tests.conftest import assert_parity
from tests.helpers import common_signal, oracle_segments, per_psr_signal, random_layout
from tests.test_gpu_dense import _random_case
from tests.test_gpu_fused_shapes import GEN_LOAD, _CASES, _instance, _layout as fused_layout, _run as fused_run
from tests.test_gpu_next_mix import _layout as c2_layout
from tests.test_gpu_white_grid import _c5_like, _run as white_run

pytestmark = pytest.mark.gpu

PHILOX_MSG = "32-bit Philox counter word"


@pytest.fixture(scope="module")
def capi():
    from fakepta_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def ctx(capi):
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def shipped(ctx, capi):
    opts = ctx.options()
    assert opts[capi.OPT_INTERP_FUSED] == 1 and opts[capi.OPT_FUSED_NEXT_MIX] == 1 and opts[capi.OPT_OVERLAP] == 1
    assert opts[capi.OPT_FUSE_WHITE] == 1 and opts[capi.OPT_GEN_MIX] == 2 and opts[capi.OPT_DFT_GEN] == 1
    return opts


def _counted(ctx, capi, call):
    """call() with the launch records on: (its result, launches per kind of kernel_stats)."""
    ctx.set_option(capi.OPT_PROFILE, 1)
    try:
        ctx.reset_stats()
        res = call()
        n = {k: ctx.kernel_stats(getattr(capi, k))[0] for k in ("K_GEN", "K_MIX", "K_SYNTH", "K_WHITE", "K_GRID")}
    finally:
        ctx.set_option(capi.OPT_PROFILE, 0)
        ctx.reset_stats()
    return res, n


# ----------------------------------------------------------------------------- 1. k_gen
@pytest.mark.parametrize("seed", [S.S_HI, S.S_K1], ids=["S_HI", "S_K1"])
def test_k_gen_coefficients(ctx, capi, shipped, seed):
    """The layout and bound of test_device_normals_match_oracle (3 pulsars, 12 modes, 9 realizations): amp * z of
    k_gen's counters, element by element, below and across bit 31 from odd and even starts and up to 2^32 - 1."""
    rng = np.random.default_rng(5)
    offs, toas, nu = random_layout(rng, 3, (30, 60))
    ctx.batch_set_toas(offs, toas, nu)
    f, a = per_psr_signal(rng, offs, toas, 12)
    ctx.batch_add_signal(0, f, a)
    segs = [O.Segment(0, 2 * np.pi * f, a)]
    try:
        for real0 in (S.BIT31_ODD, S.BIT31_EVEN, S.B31 - 5, S.B31 - 4, S.B32 - 9):  # 9 from 2^31 - 5 cross bit 31
            (out, co), n = _counted(ctx, capi, lambda: ctx.batch_synth(seed, real0, 9, coeffs=True))
            assert n["K_GEN"] >= 1 and n["K_MIX"] == 0, n
            S.check_coeffs(co, S.oracle_coeffs(segs, 3, seed, real0, 9))
            for p in range(3):  # the oracle's normals themselves, as that test takes them
                z = O.gp_normals(seed, np.arange(real0, real0 + 9), p, 0, 12)
                want = np.transpose(a[p][None, :, None] * z, (1, 2, 0)).reshape(24, 9)
                np.testing.assert_allclose(co[p], want, rtol=S.COEF_TOL, atol=S.COEF_TOL * np.abs(want).max())
            S.check_block(out, O.batch_synth(offs, toas, nu, segs, seed, real0, 9))
    finally:
        ctx.batch_clear()
        ctx.set_options(shipped)


def test_negative_seed_is_its_64_bit_pattern(ctx, shipped):
    """seed = -1 draws the bits of seed = 2^64 - 1 (k0 == k1 == 0xFFFFFFFF), in the batch path and the dense draws."""
    rng = np.random.default_rng(6)
    offs, toas, nu = random_layout(rng, 3, (30, 60))
    ctx.batch_set_toas(offs, toas, nu)
    f, a = per_psr_signal(rng, offs, toas, 12)
    ctx.batch_add_signal(0, f, a)
    try:
        got = ctx.batch_synth(-1, S.BIT31_ODD, 33)
        np.testing.assert_array_equal(got, ctx.batch_synth(2 ** 64 - 1, S.BIT31_ODD, 33))
        S.check_block(got, O.batch_synth(offs, toas, nu, [O.Segment(0, 2 * np.pi * f, a)], 2 ** 64 - 1, S.BIT31_ODD, 33))
        toas, nu, segs, osigs, white = _random_case(264, 64, white_scale=1e-6)
        got = ctx.noise_draw(toas, nu, segs, white, -1, S.B32 - 5, 9)
        np.testing.assert_array_equal(got, ctx.noise_draw(toas, nu, segs, white, 2 ** 64 - 1, S.B32 - 5, 9))
    finally:
        ctx.batch_clear()
        ctx.set_options(shipped)


# ----------------------------------------------------------------------------- 2. k_gen + k_mix / k_mix_tiled
@pytest.mark.parametrize("P,mix_mfma", [(7, 1), (66, 0)], ids=["k_mix", "k_mix_tiled"])
def test_k_gen_and_mix(ctx, capi, shipped, P, mix_mfma):
    """A common signal drawn by k_gen and mixed by k_mix (fewer than 64 pulsars) or by k_mix_tiled (FPTA_OPT_MIX_MFMA 0
    from 64 pulsars up, where k_gen_mix would otherwise draw): the layouts of test_batch_vs_oracle and
    test_tiled_mix_vs_oracle."""
    rng = np.random.default_rng(21 + P)
    offs, toas, nu = random_layout(rng, P, (20, 100) if P < 64 else (5, 40))
    ctx.batch_set_toas(offs, toas, nu)
    f1, a1 = per_psr_signal(rng, offs, toas, 30 if P < 64 else 6)
    fc, ac, L, _ = common_signal(rng, offs, toas, 18)  # even mode counts: the download has no padding column
    ctx.batch_add_signal(0, f1, a1, idx=2.0)
    ctx.batch_add_signal(1, fc, ac, idx=0.0, L=L)
    segs = [O.Segment(0, 2 * np.pi * f1, a1, 2.0), O.Segment(1, 2 * np.pi * fc, ac, 0.0, L=L)]
    try:
        ctx.set_option(capi.OPT_MIX_MFMA, mix_mfma)
        ctx.set_option(capi.OPT_SYNTH_PATH, 3)
        for seed, (real0, R) in zip((S.S_HI, S.S_K1, S.S_HI, S.S_HI), S.windows(33, 34)):
            (out, co), n = _counted(ctx, capi, lambda: ctx.batch_synth(seed, real0, R, coeffs=True))
            assert n["K_GEN"] >= 2 and n["K_MIX"] == 1, n  # both signals on k_gen, one mix
            S.check_coeffs(co, S.oracle_coeffs(segs, P, seed, real0, R))
            S.check_block(out, O.batch_synth(offs, toas, nu, segs, seed, real0, R))
    finally:
        ctx.batch_clear()
        ctx.set_options(shipped)


# ----------------------------------------------------------------------------- 3. k_gen_mix
@pytest.mark.parametrize("factor,wins", [("svd", (0, 3)), ("monopole", (1, 2))], ids=["full_rank", "monopole"])
def test_k_gen_mix(ctx, capi, shipped, factor, wins):
    """64 pulsars (test_gpu_next_mix's layout): the common signal drawn and mixed by k_gen_mix. A plain block launches
    it alone (one K_MIX record, no k_gen: the per-pulsar draws are k_grid_fused's); a coefficient download also runs
    k_gen for the per-pulsar signals."""
    rng = np.random.default_rng(64)
    offs, toas, nu, segs = c2_layout(ctx, rng, 64, factor, n=(40, 80))
    try:
        for w in wins:
            real0, R = S.windows(33, 34)[w]
            got, n = _counted(ctx, capi, lambda: ctx.batch_synth(S.S_HI, real0, R))
            gi = ctx.batch_grid_info()
            assert n["K_MIX"] == 1 and n["K_GEN"] == 0, n
            assert _instance(gi["interp_kernel"])[1:3] == (real0 % 2 == 1, True), gi["interp_kernel"]
            print(f"k_gen_mix {factor} real0 {real0}: {n}, {gi['interp_kernel']}")
            want = O.batch_synth(offs, toas, nu, segs, S.S_HI, real0, R)
            S.check_block(got, want)
            (out, co), n = _counted(ctx, capi, lambda: ctx.batch_synth(S.S_HI, real0, R, coeffs=True))
            assert n["K_MIX"] == 1 and n["K_GEN"] >= 2, n
            S.check_coeffs(co, S.oracle_coeffs(segs, 64, S.S_HI, real0, R))
            S.check_block(out, want)
    finally:
        ctx.batch_clear()
        ctx.set_options(shipped)


# ----------------------------------------------------------------------------- 4, 5. k_grid_dft_gen, k_grid_fused
@pytest.mark.parametrize("case,seed", [("gen_load_1_1", S.S_HI), ("gen_load_1_1", S.S_K1), ("gen_load_2_7", S.S_HI),
                                       ("gen_only_1_1", S.S_HI)],
                         ids=["gen_load_1_1-S_HI", "gen_load_1_1-S_K1", "gen_load_2_7-S_HI", "gen_only_1_1-S_HI"])
def test_fused_and_dft_gen_draws(ctx, capi, shipped, case, seed):
    """test_fused_shapes_bitwise_and_oracle's checks at the high points. FPTA_OPT_INTERP_FUSED 0: k_grid_dft_gen draws
    (grid_term_coefs; no k_gen launch) and another kernel interpolates; 2 and 3: k_grid_fused draws in its ring, on the
    shaped instance (gen_load_*) or the fallback (gen_only_*), whole and half bands, its ODD flag the start's parity.
    Whole bands equal the two-kernel path bit for bit; all three match the oracle."""
    rn, dm, gw, nu_const, n_grid, gen, shape = _CASES[case]
    assert gen
    rng = np.random.default_rng(4200 + sorted(_CASES).index(case))
    offs, toas, nu, segs = fused_layout(ctx, rng, int(rng.integers(3, 6)), rn, dm, gw, nu_const)
    try:
        ctx.set_option(capi.OPT_SYNTH_PATH, 4)
        for real0, R in S.windows(33, 64):
            (ref, k0, s0), n = _counted(ctx, capi, lambda: fused_run(ctx, capi, 0, seed, real0, R))
            # two blocks (fused_run's warm-up and the block): k_gen and k_mix for the common signal at the most, never
            # k_gen for the two per-pulsar signals
            assert n["K_GEN"] <= (2 if gw else 0) and n["K_MIX"] <= (2 if gw else 0) and n["K_GRID"] >= 1, n
            got, k2, s2 = fused_run(ctx, capi, 2, seed, real0, R)
            half, k3, s3 = fused_run(ctx, capi, 3, seed, real0, R)
            assert (s0, s2, s3) == (-1, shape, shape), (case, s0, s2, s3)
            assert ctx.batch_grid_info()["grid_signals"] == n_grid
            assert not k0.startswith("k_grid_fused"), k0
            for k, is_half in ((k2, False), (k3, True)):
                nq, odd, kgen, khalf = _instance(k)
                assert (odd, kgen, khalf) == (real0 % 2 == 1, True, is_half), (case, real0, k)
            print(f"{case} real0 {real0}: {k0} {n}, {k2} and {k3} shape {s2}")
            np.testing.assert_array_equal(ref, got)
            want = O.batch_synth(offs, toas, nu, segs, seed, real0, R)
            S.check_block(ref, want)
            S.check_block(half, want)
            S.check_block(got, want)
    finally:
        ctx.batch_clear()
        ctx.set_options(shipped)


# ----------------------------------------------------------------------------- 6. the successor's mix
@pytest.mark.parametrize("first,made", [(S.B32 - 3 * 128, [True, True, False]), (S.B31 - 129, [True, True, True])],
                         ids=["up_to_2^32", "across_bit_31_odd"])
def test_successor_mix_at_the_top_of_the_range(ctx, capi, shipped, first, made):
    """Three pipelined 128-realization blocks of test_fused_shapes_pipelined_next_mix's 64-pulsar layout with
    FPTA_OPT_FUSED_NEXT_MIX 1: the second and third take the mix the block before made (fused_mix_tile: the paired
    DPP form from an even start, the two-call form from an odd one). The block that ends at 2^32 makes none, since its
    successor would pass the limit, and returns success. Every block equals the option-off run bit for bit, the last
    one the oracle."""
    rng = np.random.default_rng(4100)
    offs, toas, nu, segs = fused_layout(ctx, rng, 64, 30, 100, 30, n=(40, 60))
    R = 128

    def run(on):
        ctx.set_option(capi.OPT_FUSED_NEXT_MIX, on)
        res = []
        for b in range(3):
            out = ctx.batch_synth(S.S_HI, first + R * b, R)
            gi = ctx.batch_grid_info()
            assert _instance(gi["interp_kernel"])[1:3] == (first % 2 == 1, True), gi["interp_kernel"]
            assert ctx.debug_fused_shape() == GEN_LOAD
            res.append((out, gi["next_mix_used"], gi["next_mix_made"]))
        return res

    try:
        ctx.set_option(capi.OPT_SYNTH_PATH, 4)
        ref = run(0)  # also grows the second coefficient buffer, so the option-on run's first block can make a mix
        got = run(1)
        assert [(u, m) for _, u, m in ref] == [(False, False)] * 3
        assert [u for _, u, _ in got] == [False, True, True], got
        assert [m for _, _, m in got] == made, got
        print(f"successor mix from {first}: {ctx.batch_grid_info()['interp_kernel']}, used / made "
              f"{[(u, m) for _, u, m in got]}")
        for b in range(3):
            assert np.all(np.isfinite(got[b][0]))
            np.testing.assert_array_equal(got[b][0], ref[b][0], err_msg=f"block {b}")
        S.check_block(got[2][0], O.batch_synth(offs, toas, nu, segs, S.S_HI, first + 2 * R, R))
    finally:
        ctx.batch_clear()
        ctx.set_options(shipped)


# ----------------------------------------------------------------------------- 7. white noise and ECORR
@pytest.mark.parametrize("fuse_white", [1, 0], ids=["epilogue", "k_white_pairs"])
def test_white_and_ecorr(ctx, capi, shipped, fuse_white):
    """A shrunk C5-like layout with white noise and ECORR epochs of 1, 2 and 3 TOAs on the gridded path. FPTA_OPT_FUSE_WHITE
    1: k_epoch_normals + the interpolation epilogue's white_quad (k_grid_interp_mfma<true, ..>); 0: k_epoch_normals + the
    separate k_white_pairs pass. An odd start leaves the first realization pair half outside the block."""
    rng = np.random.default_rng(405)
    offs, toas, nu, segs, sigma, block_of, esig = _c5_like(ctx, rng, P=5, n=(40, 120), commons=("hd",))
    blocks = [np.flatnonzero(block_of == b) for b in range(len(esig))]
    # pulsar 2 has 6 TOAs, three per backend: one backend's epochs of 2 + 1 TOAs become one epoch of 3
    mine = [b for b, q in enumerate(blocks) if offs[2] <= q[0] < offs[3]]
    sizes = sorted(len(blocks[b]) for b in mine)
    assert sizes == [1, 1, 2, 2], sizes
    b2, b1 = mine[0], mine[1]
    assert (len(blocks[b2]), len(blocks[b1])) == (2, 1)
    blocks[b2] = np.concatenate([blocks[b2], blocks[b1]])
    del blocks[b1]
    esig = np.delete(esig, b1)
    block_of = -np.ones(offs[-1], dtype=np.int64)
    for b, q in enumerate(blocks):
        block_of[q] = b
    assert sorted(set(len(q) for q in blocks)) == [1, 2, 3]
    ctx.batch_set_white(sigma, blocks, esig)
    try:
        ctx.set_option(capi.OPT_SYNTH_PATH, 4)
        ctx.set_option(capi.OPT_FUSE_WHITE, fuse_white)
        for seed, (real0, R) in zip((S.S_HI, S.S_K1, S.S_HI, S.S_HI), S.windows(33, 34)):
            (got, k), n = _counted(ctx, capi, lambda: white_run(ctx, seed, real0, R))
            # two blocks ran (white_run's warm-up and the block): k_epoch_normals each, k_white_pairs each if separate
            assert n["K_WHITE"] == (2 if fuse_white else 4), n
            print(f"white + ECORR fuse_white {fuse_white} real0 {real0}: {k} {n}")
            assert k.startswith("k_grid_interp_"), k
            assert k.startswith("k_grid_interp_mfma<true,") == bool(fuse_white), k
            want = O.batch_synth(offs, toas, nu, segs, seed, real0, R, sigma=sigma, block_of=block_of, ecorr_sigma=esig)
            S.check_block(got, want)
    finally:
        ctx.batch_set_white()
        ctx.batch_clear()
        ctx.set_options(shipped)


# ----------------------------------------------------------------------------- 8. streamed jobs
@pytest.fixture(scope="module")
def c3s(capi):
    """A C3-like job (test_gpu_c3) of 8 pulsars x 100 TOAs: one HD common signal of 30 modes, on a context of its own."""
    from fakepta import correlated_noises as cn
    from fakepta import fake_pta as fp
    from fakepta_amd.batch import BatchSimulator
    c = capi.Context(0)
    np.random.seed(3)
    psrs = fp.make_fake_array(npsrs=8, Tobs=10, ntoas=100, gaps=False, isotropic=True, toaerr=1e-7,
                              backends="NUPPI.1400", custom_model={"RN": None, "DM": None, "Sv": None})
    cn.add_common_correlated_noise(psrs, orf="hd", log10_A=-15, gamma=13 / 3, components=30)
    sim = BatchSimulator(psrs, white=False, ctx=c)
    assert c.batch_info()["K"] == 60 and sim.n_toa == 800
    yield sim, c
    c.close()


def _multi(capi, sim):
    m = capi.MultiContext([0, 0])
    m.set_toas(sim.offs, sim.toas, sim.freqs)
    for s in sim.segments:
        m.add_signal(s["kind"], s["f"], s["amp"], idx=s["idx"], L=s["L"], mask=s["mask"])
    return m


def test_streamed_jobs_up_to_the_limit(c3s, capi):
    """The last 300 realizations below 2^32 through fpta_batch_synth_checksums, the two-context driver and
    simulate_sharded (in the library and block by block), in batches of 128 and 77: one set of checksums, bit for bit.
    Picked realizations as test_c3_streamed_checksums_and_picks takes them: the resident row against the oracle's, the
    checksums against the row, and within the same bounds against the oracle's row itself (measured: 1e-16 relative on
    the sum of squares, 3e-21 absolute on the sum)."""
    from fakepta_amd.batch import simulate_sharded
    sim, ctx = c3s
    n, real0 = 300, S.B32 - 300
    picks = {0: None, 127: None, 128: None, 153: None, 299: None}

    def grab(s, first, k):
        for r in picks:
            if first <= real0 + r < first + k:
                picks[r] = ctx.batch_download(real0 + r - first, 1)[0]

    sums = simulate_sharded(sim, n, seed=S.S_HI, real0=real0, batch=128, on_batch=grab)
    path = ctx.batch_grid_info()["last_path"]
    print(f"streamed job: path {path}, {ctx.batch_grid_info()['interp_kernel']}")
    assert sums.shape == (n, 2) and np.all(np.isfinite(sums))
    for batch in (128, 77):
        np.testing.assert_array_equal(ctx.batch_synth_checksums(S.S_HI, real0, n, batch=batch), sums)
        np.testing.assert_array_equal(simulate_sharded(sim, n, seed=S.S_HI, real0=real0, batch=batch), sums)
    assert ctx.batch_grid_info()["last_path"] == path  # one path for the job, whoever streams it
    m = _multi(capi, sim)
    try:
        for batch in (128, 77):
            np.testing.assert_array_equal(m.synth_checksums(S.S_HI, real0, n, batch=batch), sums)
        assert m.context(1).batch_grid_info()["last_path"] == path
    finally:
        m.close()
    segs = oracle_segments(sim)
    for r, row in picks.items():
        want = O.batch_synth(sim.offs, sim.toas, sim.freqs, segs, S.S_HI, real0 + r, 1)[0]
        print(f"realization 2^32 - {n - r}: sum of squares {sums[r, 1]:.17g} (oracle row {(want ** 2).sum():.17g}), "
              f"sum {sums[r, 0]:.17g} (oracle row {want.sum():.17g})")
        assert_parity(row, want, S.TOL)
        S.check_sums(sums[r], row)
        S.check_sums(sums[r], want)


# ----------------------------------------------------------------------------- 9. dense draws
@pytest.mark.parametrize("n", [64, 333])
def test_dense_draws(ctx, n):
    """k_dense_normals at test_draws_vs_oracle_and_split_invariance's layouts and bound: a block across 2^32, where
    g >> 1 reaches 2^31, and one ending exactly at 2^33; the split invariance of that test across the 2^32 point."""
    toas, nu, segs, osigs, white = _random_case(200 + n, n, white_scale=1e-6)
    cov = O.dense_cov(toas, nu, osigs) + np.diag(white)
    for seed in (S.S_HI, S.S_K1):
        for real0, R in S.DENSE_STARTS:
            got = ctx.noise_draw(toas, nu, segs, white, seed, real0, R)
            S.check_draws(got, O.dense_draws(cov, seed, real0, R))
    whole = ctx.noise_draw(toas, nu, segs, white, S.S_HI, S.B32 - 5, 9)
    np.testing.assert_array_equal(ctx.noise_draw(toas, nu, segs, white, S.S_HI, S.B32 - 2, 4), whole[3:7])
    np.testing.assert_array_equal(ctx.noise_draw(toas, nu, segs, white, S.S_HI, S.B32, 4), whole[5:9])
    np.testing.assert_array_equal(ctx.noise_draw(toas, nu, segs, white, S.S_HI, S.B32 - 5, 5), whole[:5])


def test_dense_draws_dropin(ctx, golden):
    """Pulsar.draw_noise_model_batch on fixture G6's pulsar (test_dropin_pulsar_covariance_replay's construction; its
    covariance has condition number 1.6e3) against the oracle's draws of the fixture's covariance."""
    from fakepta import fake_pta as fp
    g = golden("g6_dense_cov.npz")
    rng = np.random.default_rng(17)
    yr = 365.25 * 24 * 3600
    keep = rng.random(80) < 0.75
    epochs = 0.2 * yr + np.arange(1, 81)[keep] * (30.1 * 24 * 3600)
    np.random.seed(23)
    psr = fp.Pulsar(epochs, 2e-7, 0.4, 2.2, pdist=(1.0, 0.2), freqs=[1400], backends=["A.1400", "B.800"],
                    custom_model={"RN": 30, "DM": 100, "Sv": 30})
    np.testing.assert_array_equal(psr.toas, g["toas"])
    for b in psr.backends:
        psr.noisedict[f"{psr.name}_{b}_efac"] = {"A.1400": 1.2, "B.800": 0.9}[b]
        psr.noisedict[f"{psr.name}_{b}_log10_tnequad"] = {"A.1400": -6.8, "B.800": -7.1}[b]
    psr.add_red_noise(spectrum="powerlaw", log10_A=-13.9, gamma=3.1)
    psr.add_dm_noise(spectrum="powerlaw", log10_A=-13.5, gamma=2.2)
    psr.add_chromatic_noise(spectrum="powerlaw", log10_A=-13.8, gamma=1.8)
    cov = g["red_cov"] + np.diag(g["white_cov"])
    for real0, R in S.DENSE_STARTS:
        got = psr.draw_noise_model_batch(R, seed=S.S_HI, real0=real0)
        S.check_draws(got, O.dense_draws(cov, S.S_HI, real0, R))
        np.testing.assert_array_equal(
            got, ctx.noise_draw(psr.toas, psr.freqs, psr._red_segments(), psr._white_sigma2(), S.S_HI, real0, R))


# ----------------------------------------------------------------------------- 10. BatchSimulator.synth
def test_batch_simulator_synth(ctx, capi, shipped, golden):
    """BatchSimulator.synth(seed=S_HI, real0 high) on the first four pulsars of fixture G8's array (ragged mode counts,
    multi-backend white noise, an HD common signal), as test_example_workflow_batch_vs_oracle checks it."""
    from fakepta.correlated_noises import add_common_correlated_noise
    from fakepta.fake_pta import copy_array
    from fakepta_amd.batch import BatchSimulator
    from tests.helpers import g8_inputs
    psrs_0, nd, cm, g = g8_inputs(golden)
    np.random.seed(int(g["seed"]))
    psrs = copy_array(psrs_0[:4], nd, cm)
    for psr in psrs:
        psr.make_ideal()
        psr.add_white_noise()
        psr.add_red_noise()
        psr.add_dm_noise()
        psr.add_chromatic_noise()
    add_common_correlated_noise(psrs, log10_A=-15., gamma=13 / 3, orf='hd')
    sim = BatchSimulator(psrs, white=True, ctx=ctx)
    try:
        segs = oracle_segments(sim)
        assert len(segs) >= 3 and sim.sigma is not None
        for real0, R in ((S.BIT31_ODD, 24), (S.B32 - 5, 5)):
            got = sim.synth(R, seed=S.S_HI, real0=real0)
            want = O.batch_synth(sim.offs, sim.toas, sim.freqs, segs, S.S_HI, real0, R, sigma=sim.sigma)
            S.check_block(got, want)
    finally:
        ctx.batch_set_white()
        ctx.batch_clear()
        ctx.set_options(shipped)


# ----------------------------------------------------------------------------- refusals
def test_calls_past_the_limits_are_refused(c3s, capi):
    """real0 + n_real == 2^32 + 1 and real0 == -1 are refused by batch_synth, batch_synth_checksums and
    MultiContext.synth_checksums with the counter-word message, noise_draw refuses 2^33 + 1; the resident block then
    downloads unchanged and the same call one realization lower succeeds."""
    sim, ctx = c3s
    segs = oracle_segments(sim)
    held = ctx.batch_synth(S.S_HI, S.BIT31_ODD, 20)
    m = _multi(capi, sim)
    try:
        for real0, n in ((S.B32 - 8, 9), (-1, 9), (S.B32, 1)):
            with pytest.raises(capi.FptaError, match=PHILOX_MSG):
                ctx.batch_synth(S.S_HI, real0, n)
            with pytest.raises(capi.FptaError, match=PHILOX_MSG):
                ctx.batch_synth_checksums(S.S_HI, real0, n, batch=4)
            with pytest.raises(capi.FptaError, match=PHILOX_MSG):
                m.synth_checksums(S.S_HI, real0, n, batch=4)
            np.testing.assert_array_equal(ctx.batch_download(0, 20), held)
        want = O.batch_synth(sim.offs, sim.toas, sim.freqs, segs, S.S_HI, S.B32 - 9, 9)
        got = ctx.batch_synth(S.S_HI, S.B32 - 9, 9)
        S.check_block(got, want)
        sums = ctx.batch_synth_checksums(S.S_HI, S.B32 - 9, 9, batch=4)
        np.testing.assert_array_equal(m.synth_checksums(S.S_HI, S.B32 - 9, 9, batch=4), sums)
        np.testing.assert_array_equal(ctx.batch_synth_checksums(S.S_HI, S.B32 - 300, 300, batch=128)[-9:], sums)
    finally:
        m.close()
    toas, nu, dsegs, osigs, white = _random_case(264, 64, white_scale=1e-6)
    with pytest.raises(capi.FptaError, match="realization index"):
        ctx.noise_draw(toas, nu, dsegs, white, S.S_HI, S.B33 - 8, 9)
    cov = O.dense_cov(toas, nu, osigs) + np.diag(white)
    S.check_draws(ctx.noise_draw(toas, nu, dsegs, white, S.S_HI, S.B33 - 9, 9), O.dense_draws(cov, S.S_HI, S.B33 - 9, 9))
