"""Continuous-wave populations injected into a resident batch block (k_cw_block / k_cw_bcast behind
fpta_batch_cw_accumulate, BatchSimulator.add_cgw) against tests/golden/g10_cw.npz and against the drop-in call.

Accuracy has the rule and the margin of tests/test_gpu_cw.py: the device may be 4 x err_ref64[s], the measured error of
the literal fp64 numpy evaluation against the 60-digit truth. Everything else is bit for bit: realization r of the
block equals its samples plus what fpta_cw_accumulate adds to zeros for table r (in one piece for per-realization
tables, with the default split for one shared table). The main layout is the fixture's four pulsars of 1, 63, 257 and
70 TOAs: a one-lane slab, a partial wave, two slabs of one pulsar (256 + 1) and a slab of two waves. The shared table
runs at 3 and at 17 realizations: k_cw_bcast's groups of 8 rows, one group and 8 + 8 + 1."""
import numpy as np
import pytest

from tests import ld_reference as LDR
from tests import tm_reference as T
from tests.helpers import common_signal, per_psr_signal, random_layout
from tests.test_gpu_tm import _checksum_bound

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
LD = np.longdouble


@pytest.fixture(scope="module")
def g(golden):
    return golden("g10_cw.npz")


@pytest.fixture(scope="module")
def capi():
    from fakepta_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def cw():
    from fakepta_amd import cw
    return cw


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


class _Psr:
    """What BatchSimulator and add_cgw read of a pulsar."""

    def __init__(self, toas, freqs, sigma2, pos, pdist):
        self.toas, self.freqs, self.sigma2, self.pos, self.pdist = toas, freqs, sigma2, pos, pdist
        self.Mmat = T.mmat(toas, freqs)
        self.signal_model = {}

    def _white_sigma2(self):
        return self.sigma2


@pytest.fixture(scope="module")
def sim(ctx, g):
    """The fixture's four pulsars with one 5-mode red-noise signal, so that a block is not zero. Its amplitude keeps
    the samples below the loudest fixture source's peak (asserted where a test's bound relies on it)."""
    from fakepta_amd.batch import BatchSimulator
    offs, toas = g["offs"], g["toas"]
    psrs = [_Psr(toas[offs[p]:offs[p + 1]], np.full(offs[p + 1] - offs[p], 1400.0), np.full(offs[p + 1] - offs[p], 1e-14),
                 g["pos"][p], tuple(g["pdist"][p])) for p in range(4)]
    s = BatchSimulator(psrs, signals=[], white=False, ctx=ctx)
    f, a = per_psr_signal(np.random.default_rng(41), offs, toas, 5, log10_A=-14.5)
    s.add_signal("red_noise", 0, f, a)
    return s


def layout_args(g, cw, p_dist_row=None):
    """The drop-in call's arguments; p_dist_row None: L = light_seconds(pdist), as add_cgw(p_dist=None) takes it."""
    offs = g["offs"]
    if p_dist_row is None:
        L = np.array([cw.light_seconds(g["pdist"][p]) for p in range(4)])
    else:
        L = np.array([cw.light_seconds(g["pdist"][p], p_dist_row[p]) for p in range(4)])
    return offs, g["toas"], g["pos"], L


def drop_in_delay(ctx, capi, g, cw, table, split, p_dist_row=None):
    """fpta_cw_accumulate on zeros."""
    offs, toas, pos, L = layout_args(g, cw, p_dist_row)
    ctx.set_option(capi.OPT_CW_SPLIT, split)
    out = np.zeros(offs[-1])
    ctx.cw_accumulate(offs, toas, pos, L, table, out)
    ctx.set_option(capi.OPT_CW_SPLIT, 0)
    return out


def many_sources(g, n=300):
    """The fixture's rows cycled, phase0 and psi shifted row by row: K depends on neither, so every row passes the
    coalescence rule as the fixture's rows do."""
    k = np.arange(n)
    rows = g["src"][k % 10].copy()
    rows[:, 6] += 0.1 * k
    rows[:, 7] += 0.01 * k
    return rows


def test_accuracy_against_the_truth(ctx, g, sim):
    R, src = 10, g["src"]
    sim.synth(R, seed=3, to_host=False)
    ctx.debug_fill_out(0.0)
    sim.add_cgw([src[s:s + 1] for s in range(R)])
    got = ctx.batch_download(0, R)
    for s in range(R):
        err = np.max(np.abs(got[s] - g["truth"][s]))
        print(f"source {s}: device error {err:.3e} = {err / g['err_ref64'][s]:.3g} x the literal fp64 error "
              f"({err / g['peak'][s]:.1e} of peak)")
        assert err <= 4 * g["err_ref64"][s]
    # one realization gets all ten, the others none
    sim.synth(R, seed=3, to_host=False)
    ctx.debug_fill_out(0.0)
    sim.add_cgw([src[:0]] * 4 + [src] + [src[:0]] * 5)
    got = ctx.batch_download(0, R)
    want, bound = g["truth"].sum(axis=0), 4 * g["err_ref64"].sum()
    offs = g["offs"]
    for p in range(4):
        err = np.max(np.abs(got[4, offs[p]:offs[p + 1]] - want[offs[p]:offs[p + 1]]))
        print(f"all ten, pulsar {p}: error {err:.3e}, bound {bound:.3e} ({err / bound:.3g})")
        assert err <= bound
    assert not got[:4].any() and not got[5:].any()


def test_ragged_tables_bit_identical_to_the_drop_in_call(ctx, capi, g, cw, sim):
    src = g["src"]
    tables = [src[:0], src[9:10], src[7:10], src, many_sources(g)]  # 300: two LDS tiles and a partial one
    assert [len(t) for t in tables] == [0, 1, 3, 10, 300]
    R = len(tables)
    base = sim.synth(R, seed=11)
    assert np.all(np.ptp(base, axis=1) > 0)
    sim.add_cgw(tables)
    got = ctx.batch_download(0, R)
    delays = [drop_in_delay(ctx, capi, g, cw, t, 1) for t in tables]
    for r in range(R):
        np.testing.assert_array_equal(got[r], base[r] + delays[r], err_msg=f"realization {r}")
    np.testing.assert_array_equal(got[0], base[0])
    assert not np.array_equal(got[1:], base[1:])
    sim.add_cgw(tables, sign=-1.0)
    back = ctx.batch_download(0, R)
    np.testing.assert_array_equal(back[0], base[0])
    for r in range(1, R):
        peak = np.max(np.abs(delays[r]))
        assert np.max(np.abs(base[r])) <= peak  # (b + d) - d: two roundings of numbers below 2 peak
        err = np.max(np.abs(back[r] - base[r]))
        print(f"realization {r} ({len(tables[r])} sources): add then subtract leaves {err / (EPS * peak):.3g} eps x peak")
        assert err <= 4 * EPS * peak


@pytest.mark.parametrize("n_src", [10, 300])
def test_shared_table(ctx, capi, g, cw, sim, n_src):
    """One table for every realization: the delay vector is made once with the drop-in call's own split rule (300
    sources on 391 TOAs: 9 pieces and k_cw_reduce)."""
    table = g["src"] if n_src == 10 else many_sources(g)
    R = 3
    base = sim.synth(R, seed=12)
    sim.add_cgw(table)
    got = ctx.batch_download(0, R)
    delay = drop_in_delay(ctx, capi, g, cw, table, 0)
    np.testing.assert_array_equal(got, base + delay[None, :])
    assert not np.array_equal(got, base)
    # the dict form of the same table
    sim.synth(R, seed=12, to_host=False)
    keys = ("costheta", "phi", "cosinc", "log10_mc", "log10_fgw", "log10_h", "phase0", "psi", "psrterm")
    sim.add_cgw({k: table[:, i] for i, k in enumerate(keys)})
    np.testing.assert_array_equal(ctx.batch_download(0, R), got)
    # 17 realizations: k_cw_bcast's groups of 8 rows, two full ones and one of a single row, on two column chunks
    R = 17
    base = sim.synth(R, seed=12)
    sim.add_cgw(table)
    np.testing.assert_array_equal(ctx.batch_download(0, R), base + delay[None, :])


def test_per_realization_distances(ctx, capi, g, cw, sim):
    R, table = 5, g["src"][5:]  # the five sources with the pulsar term
    assert table[:, 8].all()
    p_dist = np.random.default_rng(6).normal(size=(R, 4))
    base = sim.synth(R, seed=13)
    sim.add_cgw(table, p_dist=p_dist)
    got = ctx.batch_download(0, R)
    for r in range(R):
        delay = drop_in_delay(ctx, capi, g, cw, table, 1, p_dist_row=p_dist[r])
        np.testing.assert_array_equal(got[r], base[r] + delay, err_msg=f"realization {r}")
    assert not np.array_equal(got[0] - base[0], got[1] - base[1])  # the draws matter
    # [P]: one draw per pulsar for every realization, the same as [R, P] with equal rows
    sim.synth(R, seed=13, to_host=False)
    sim.add_cgw(table, p_dist=p_dist[2])
    one = ctx.batch_download(0, R)
    sim.synth(R, seed=13, to_host=False)
    sim.add_cgw(table, p_dist=np.tile(p_dist[2], (R, 1)))
    np.testing.assert_array_equal(ctx.batch_download(0, R), one)
    np.testing.assert_array_equal(one[2], got[2])
    for bad in (np.zeros(3), np.zeros((R + 1, 4)), np.zeros((R, 3))):
        with pytest.raises(ValueError):
            sim.add_cgw(table, p_dist=bad)
    np.testing.assert_array_equal(ctx.batch_download(0, R), one)


def test_refusals_leave_the_block_unchanged(ctx, capi, g, cw, sim):
    src = g["src"]
    R = 5
    sim.synth(R, seed=14, to_host=False)
    before = ctx.batch_download(0, R)
    offs, toas, pos, L = layout_args(g, cw)
    tables = [src[:2], src[2:5], src[5:8], src[:1], src[9:]]
    # R + 1 tables: the Python surface refuses the shape, the library the call
    with pytest.raises(ValueError):
        sim.add_cgw(tables + [src[:1]])
    n_tab, so, rows = cw.population_tables(tables + [src[:1]], R + 1)
    with pytest.raises(capi.FptaError, match="6 source tables for a block of 5 realizations"):
        ctx.batch_cw_accumulate(pos, L, n_tab, so, rows)
    np.testing.assert_array_equal(ctx.batch_download(0, R), before)
    bad = [t.copy() for t in tables]
    bad[2][1, 4] = np.nan
    with pytest.raises(capi.FptaError, match="realization 2, source 1: non-finite log10_fgw"):
        sim.add_cgw(bad)
    np.testing.assert_array_equal(ctx.batch_download(0, R), before)
    bad = [t.copy() for t in tables]
    bad[4][0, 3:5] = 8.0, -6.0  # log10_mc 8 at log10_fgw -6: K max(t) ~ 16
    with pytest.raises(capi.FptaError, match="realization 4, source 0: coalesces"):
        sim.add_cgw(bad)
    np.testing.assert_array_equal(ctx.batch_download(0, R), before)
    bad = src.copy()
    bad[7, 2] = -1.5  # one table for all
    with pytest.raises(capi.FptaError, match="realization 0, source 7"):
        sim.add_cgw(bad)
    with pytest.raises(capi.FptaError, match="non-finite sign"):
        sim.add_cgw(src, sign=np.inf)
    np.testing.assert_array_equal(ctx.batch_download(0, R), before)
    # no sources at all: a successful no-op
    sim.add_cgw([src[:0]] * R)
    sim.add_cgw(src[:0])
    np.testing.assert_array_equal(ctx.batch_download(0, R), before)


def test_no_block_is_a_state_error(capi, g, cw):
    from fakepta_amd.batch import BatchSimulator
    c = capi.Context(0)
    try:
        offs, toas, pos, L = layout_args(g, cw)
        so = np.array([0, 10], dtype=np.int64)
        with pytest.raises(capi.FptaError, match="set_toas first"):
            c.batch_cw_accumulate(pos, L, 1, so, g["src"])
        psrs = [_Psr(toas[offs[p]:offs[p + 1]], np.full(offs[p + 1] - offs[p], 1400.0), None, pos[p],
                     tuple(g["pdist"][p])) for p in range(4)]
        s = BatchSimulator(psrs, signals=[], white=False, ctx=c)
        f, a = per_psr_signal(np.random.default_rng(1), offs, toas, 5)
        s.add_signal("red_noise", 0, f, a)
        with pytest.raises(capi.FptaError, match=r"\(-77\).*nothing synthesized"):
            c.batch_cw_accumulate(pos, L, 1, so, g["src"])
        with pytest.raises(capi.FptaError, match=r"\(-77\)"):
            s.add_cgw(g["src"])
        base = s.synth(2, seed=1)
        s.add_cgw(g["src"])  # and with a block it goes through
        assert not np.array_equal(c.batch_download(0, 2), base)
    finally:
        c.close()


def test_kernel_stats_count_the_call(ctx, capi, g, sim):
    ctx.set_option(capi.OPT_PROFILE, 1)
    sim.synth(4, seed=15, to_host=False)
    for sources in ([g["src"]] * 4, g["src"]):  # k_cw_block; the drop-in kernels and k_cw_bcast
        ctx.reset_stats()
        sim.add_cgw(sources)
        ctx.synchronize()
        n, ms = ctx.kernel_stats(capi.K_CW)
        assert n == 1 and ms > 0


# ----------------------------------------------------------------------------- consumers (tests/test_gpu_tm.py's layouts)
P_B, N_B = 6, 567


@pytest.fixture(scope="module")
def gridded_sim(ctx):
    """tests/test_gpu_tm.py's `gridded` shape: red noise and a Hellings-Downs common signal on 6 pulsars of 567 TOAs,
    with pos and pdist added."""
    from fakepta_amd.batch import BatchSimulator
    rng = np.random.default_rng(31)
    offs, toas, nu = random_layout(rng, P_B, (40, N_B), ragged=False)
    sig2 = rng.uniform(1e-7, 1e-6, int(offs[-1])) ** 2
    v = rng.normal(size=(P_B, 3))
    pos = v / np.linalg.norm(v, axis=1)[:, None]
    psrs = [_Psr(toas[offs[i]:offs[i + 1]], nu[offs[i]:offs[i + 1]], sig2[offs[i]:offs[i + 1]], pos[i], (1.0, 0.2))
            for i in range(P_B)]
    s = BatchSimulator(psrs, signals=[], white=False, ctx=ctx)
    f, a = per_psr_signal(rng, offs, toas, 30)
    s.add_signal("red_noise", 0, f, a)
    f, a, L, _ = common_signal(rng, offs, toas, 20)
    s.add_signal("gw_common", 1, f, a, L=L)
    return s, psrs, offs, 1 / sig2


@pytest.fixture()
def gridded(ctx, capi, gridded_sim):
    ctx.set_option(capi.OPT_SYNTH_PATH, 4)
    assert list(gridded_sim[0].set_timing_model()) == [8] * P_B
    return gridded_sim


def population(g, n_real):
    """Realization r: two or three of the fixture's sources, a different set and phase in each."""
    pop = []
    for r in range(n_real):
        t = g["src"][[r % 10, (r + 3) % 10, (r + 7) % 10][:2 + r % 2]].copy()
        t[:, 6] += 0.05 * r
        pop.append(t)
    return pop


def test_consumers_see_the_waves(ctx, capi, g, gridded):
    s, psrs, offs, w = gridded
    R = 33
    ctx.set_option(capi.OPT_FUSE_CHECKSUMS, 1)
    s.synth(R, seed=4, real0=101, to_host=False)
    assert ctx.batch_grid_info()["last_path"] == 4
    pre_sums = s.checksums()
    s.add_cgw(population(g, R))
    sums = s.checksums()
    block = ctx.batch_download(0, R)
    es, cb = np.abs(sums.astype(LD) - LDR.checksum_truth(block)), _checksum_bound(block)
    print(f"checksum error / bound {float(np.max(es / cb)):.3g}")
    assert np.all(es <= cb)
    assert np.all(sums[:, 0] != pre_sums[:, 0]) and np.all(sums[:, 1] != pre_sums[:, 1])  # not the stale partial sums
    np.testing.assert_array_equal(s.checksums(), sums)
    s.project()
    from fakepta_amd import tm
    want = block.copy()
    assert list(tm.project(offs, [p.Mmat for p in psrs], want, weights=w, ctx=ctx)) == [8] * P_B
    np.testing.assert_array_equal(ctx.batch_download(0, R), want)


def test_simulate_sharded_with_add_cgw_as_the_consumer(ctx, capi, g, gridded):
    from fakepta_amd.batch import simulate_sharded
    s, psrs, offs, w = gridded
    n_real, batch_size = 48 + 33, 48
    pop = population(g, n_real)
    got = simulate_sharded(s, n_real, seed=4, batch=batch_size,
                           on_batch=lambda sim, first, n: (sim.add_cgw(pop[first:first + n]), sim.project()))
    assert got.shape == (n_real, 2)
    ctx.set_option(capi.OPT_MFMA_MIN_REAL, 1)  # as the job sets it
    for first in range(0, n_real, batch_size):
        n = min(batch_size, n_real - first)
        plain = s.synth(n, seed=4, real0=first, fit=True)
        s.synth(n, seed=4, real0=first, to_host=False)
        s.add_cgw(pop[first:first + n])
        s.project()
        block = ctx.batch_download(0, n)
        assert not np.array_equal(block, plain)
        es = np.abs(got[first:first + n].astype(LD) - LDR.checksum_truth(block))
        assert np.all(es <= _checksum_bound(block))


@pytest.fixture(scope="module")
def shared_span(capi):
    """tests/test_gpu_tm.py's `shared_span` layout: C2's signal mix on 64 ragged pulsars over one common span, whose
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
    pos = v / np.linalg.norm(v, axis=1)[:, None]
    c.batch_add_signal(1, fc, np.sqrt(O.powerlaw(fc, -14.0, 13 / 3) / (t1 - t0)), L=batch_factor(O.orf_hd(pos)))
    c.set_option(capi.OPT_SYNTH_PATH, 4)
    yield c, pos
    c.close()


@pytest.mark.parametrize("next_real0,hit", [(384, True), (1000, False)])
def test_injection_leaves_the_next_block_alone(shared_span, g, cw, next_real0, hit):
    """The block after an injected one is bit for bit the block after an untouched one, whether the earlier block's
    kernel had already made its common-signal mix (a next-mix hit) or not (a jump: a miss)."""
    c, pos = shared_span
    n_tab, so, rows = cw.population_tables(population(g, 128), 128)
    L = np.full(64, cw.light_seconds((1.0, 0.2)))
    outs = []
    for inject in (False, True):
        for real0 in (0, 128, 256):  # hits start at the third block of a pipelined run
            c.batch_synth(7, real0, 128, to_host=False)
        assert c.batch_grid_info()["interp_kernel"].startswith("k_grid_fused<")
        if inject:
            pre = c.batch_download(0, 128)
            c.batch_cw_accumulate(pos, L, n_tab, so, rows)
            assert not np.array_equal(c.batch_download(0, 128), pre)
        outs.append(c.batch_synth(7, next_real0, 128))
        assert c.batch_grid_info()["next_mix_used"] == hit
    np.testing.assert_array_equal(outs[1], outs[0])
