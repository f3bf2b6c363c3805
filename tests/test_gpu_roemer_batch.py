"""Roemer delays of ephemeris errors injected into a resident batch block (k_roemer_block, or k_roemer_main and
k_cw_bcast, behind fpta_batch_roemer_accumulate and BatchSimulator.add_roemer_delay) against
tests/golden/g11_ephem.npz and against the drop-in call.

Accuracy has the rule and the margin of tests/test_gpu_ephem.py: the device may be 4 x err_roemer[r], the measured
error of the literal fp64 numpy evaluation against the 50-digit truth. Everything else is bit for bit: realization r
of the block equals its samples plus what fpta_roemer_accumulate adds to zeros for table r. Two layouts: the fixture's
five pulsars (1, 63, 64, 65 and 130 TOAs) for accuracy, and four pulsars of 1, 63, 257 and 70 TOAs inside the
fixture's span: a one-lane slab, a partial wave, two slabs of one pulsar (256 + 1) and a slab of two waves."""
import numpy as np
import pytest

from tests import ld_reference as LDR
from tests.helpers import per_psr_signal
from tests.test_gpu_cw_batch import P_B, _Psr, gridded, gridded_sim, shared_span  # noqa: F401 (fixtures)
from tests.test_gpu_tm import _checksum_bound

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
LD = np.longdouble
D_KEYS = ("d_mass", "d_Om", "d_omega", "d_inc", "d_a", "d_e", "d_l0")


@pytest.fixture(scope="module")
def g(golden):
    return golden("g11_ephem.npz")


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


def _simulator(ctx, offs, toas, pos, seed):
    """Pulsars with pos and one 5-mode red-noise signal, so that a block is not zero."""
    from fakepta_amd.batch import BatchSimulator
    P = len(offs) - 1
    psrs = [_Psr(toas[offs[p]:offs[p + 1]], np.full(offs[p + 1] - offs[p], 1400.0),
                 np.full(offs[p + 1] - offs[p], 1e-14), pos[p], (1.0, 0.2)) for p in range(P)]
    s = BatchSimulator(psrs, signals=[], white=False, ctx=ctx)
    f, a = per_psr_signal(np.random.default_rng(seed), offs, toas, 5, log10_A=-14.5)
    s.add_signal("red_noise", 0, f, a)
    return s


@pytest.fixture(scope="module")
def lay(g):
    """The synthetic layout: (offs, toas, pos)."""
    rng = np.random.default_rng(23)
    counts = [1, 63, 257, 70]
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    toas = np.concatenate([np.sort(rng.uniform(g["toas"].min(), g["toas"].max(), k)) for k in counts])
    v = rng.normal(size=(4, 3))
    return offs, toas, v / np.linalg.norm(v, axis=1)[:, None]


@pytest.fixture()
def sim(ctx, lay):
    return _simulator(ctx, *lay, seed=41)


@pytest.fixture()
def fixture_sim(ctx, g):
    return _simulator(ctx, g["offs"], g["toas"], g["pos"], seed=42)


def drop_in_delay(ctx, lay, table, sign=1.0):
    """fpta_roemer_accumulate on zeros."""
    offs, toas, pos = lay
    out = np.zeros(offs[-1])
    ctx.roemer_accumulate(offs, toas, pos, table, out, sign=sign)
    return out


def cycled_rows(g, n, first=0):
    """Row k: fixture body k mod 11 with the deviations of fixture row 7 k mod 12, so that the eleven distinct bases
    meet mass-only (fixture rows 0 .. 3) and element deviations alike; d_mass moves row by row."""
    k = np.arange(first, first + n)
    rows = np.concatenate([g["bodies"][k % 11], g["rows"][(7 * k) % 12, 14:]], axis=1)
    rows[:, 14] += 1e19 * k
    return rows


def slots_of(rows):
    """The planner's rule on the host: the first eight distinct bases in order of appearance, -1 beyond."""
    seen, out = [], []
    for row in rows:
        key = row[:14].tobytes()
        if key not in seen and len(seen) < 8:
            seen.append(key)
        out.append(seen.index(key) if key in seen else -1)
    return np.array(out)


# ----------------------------------------------------------------------------- 1. accuracy
def test_accuracy_against_the_truth(ctx, g, fixture_sim):
    R, rows = 12, g["rows"]
    fixture_sim.synth(R, seed=3, to_host=False)
    ctx.debug_fill_out(0.0)
    fixture_sim.add_roemer_delay([rows[r:r + 1] for r in range(R)])
    got = ctx.batch_download(0, R)
    for r in range(R):
        err = np.max(np.abs(got[r] - g["roemer_truth"][r]))
        print(f"row {r}: device error {err:.3e} = {err / g['err_roemer'][r]:.3g} x the literal fp64 error")
        assert err <= 4 * g["err_roemer"][r]
    # one realization gets all twelve, the others none
    fixture_sim.synth(R, seed=3, to_host=False)
    ctx.debug_fill_out(0.0)
    fixture_sim.add_roemer_delay([rows[:0]] * 4 + [rows] + [rows[:0]] * 7)
    got = ctx.batch_download(0, R)
    want, bound = g["roemer_truth"].sum(axis=0), 4 * g["err_roemer"].sum()
    err = np.max(np.abs(got[4] - want))
    print(f"all twelve: error {err:.3e}, bound {bound:.3e} ({err / bound:.3g})")
    assert err <= bound
    assert np.max(np.abs(got[4])) > 0.5 * np.max(np.abs(want))
    assert not got[:4].any() and not got[5:].any()


# ----------------------------------------------------------------------------- 2. ragged tables
@pytest.mark.parametrize("sign", [1.0, -0.37])
def test_ragged_tables_bit_identical_to_the_drop_in_call(ctx, g, lay, sim, sign):
    rows = g["rows"]
    tables = [rows[:0], rows[10:11], rows[[1, 6, 11]], rows, cycled_rows(g, 40)]
    assert [len(t) for t in tables] == [0, 1, 3, 12, 40]
    # the call's slots: every combination of (slotted, beyond the slots) x (mass-only, element deviations) occurs
    every = np.concatenate(tables)
    slot, same = slots_of(every), ~every[:, 15:21].any(axis=1)
    assert len(set(r[:14].tobytes() for r in tables[4])) >= 9
    for slotted in (True, False):
        for mass_only in (True, False):
            assert np.any(((slot >= 0) == slotted) & (same == mass_only)), (slotted, mass_only)
    R = len(tables)
    base = sim.synth(R, seed=11)
    assert np.all(np.ptp(base, axis=1) > 0)
    sim.add_roemer_delay(tables, sign=sign)
    got = ctx.batch_download(0, R)
    delays = [drop_in_delay(ctx, lay, t, sign) for t in tables]
    for r in range(R):
        np.testing.assert_array_equal(got[r], base[r] + delays[r], err_msg=f"realization {r}")
    np.testing.assert_array_equal(got[0], base[0])
    assert not np.array_equal(got[1:], base[1:])
    sim.add_roemer_delay(tables, sign=-sign)
    back = ctx.batch_download(0, R)
    np.testing.assert_array_equal(back[0], base[0])
    for r in range(1, R):
        # fl(fl(b + d) - d), -d exact: two roundings of numbers below 2 peak
        peak = max(np.max(np.abs(delays[r])), np.max(np.abs(base[r])))
        err = np.max(np.abs(back[r] - base[r]))
        print(f"realization {r} ({len(tables[r])} rows): add then subtract leaves {err / (EPS * peak):.3g} eps x peak")
        assert err <= 4 * EPS * peak


# ----------------------------------------------------------------------------- 3. chunks
def test_chunk_independence(ctx, capi, g, sim):
    R = 37
    tables, first = [], 0
    for r in range(R):  # 0 .. 4 rows each, the empty ones spread over the chunks
        n = (3 * r + 1) % 5
        tables.append(cycled_rows(g, n, first))
        first += n
    assert min(len(t) for t in tables) == 0 and (slots_of(np.concatenate(tables)) < 0).any()
    blocks = []
    for chunk in (0, 1, 5, 32):
        ctx.set_option(capi.OPT_ROEMER_CHUNK, chunk)
        assert ctx.get_option(capi.OPT_ROEMER_CHUNK) == chunk
        base = sim.synth(R, seed=21)
        sim.add_roemer_delay(tables)
        blocks.append(ctx.batch_download(0, R))
        assert not np.array_equal(blocks[-1], base)
    for b in blocks[1:]:
        np.testing.assert_array_equal(b, blocks[0])


# ----------------------------------------------------------------------------- 4. one table for all
def test_shared_table(ctx, g, lay, sim):
    from fakepta.ephemeris import Ephemeris
    R, table = 3, g["rows"]
    base = sim.synth(R, seed=12)
    sim.add_roemer_delay(table)
    got = ctx.batch_download(0, R)
    delay = drop_in_delay(ctx, lay, table)
    np.testing.assert_array_equal(got, base + delay[None, :])
    assert not np.array_equal(got, base)
    # the (planet, deviations) list with a native Ephemeris against the rows it stands for
    e = Ephemeris()
    perts = [(p, {k: float(v) for k, v in zip(D_KEYS, table[r, 14:21])}) for p, r in (("jupiter", 0), ("saturn", 10))]
    sim.synth(R, seed=12, to_host=False)
    sim.add_roemer_delay(perts, ephem=e)
    by_name = ctx.batch_download(0, R)
    sim.synth(R, seed=12, to_host=False)
    sim.add_roemer_delay(np.array([e.roemer_row(p, **d) for p, d in perts]))
    np.testing.assert_array_equal(by_name, ctx.batch_download(0, R))
    assert not np.array_equal(by_name, base)
    with pytest.raises(ValueError, match="Ephemeris"):
        sim.add_roemer_delay(perts)  # these pulsars carry no ephemeris
    np.testing.assert_array_equal(ctx.batch_download(0, R), by_name)


# ----------------------------------------------------------------------------- 5. refusals
def test_refusals_leave_the_block_unchanged(ctx, capi, g, lay, sim):
    from fakepta_amd import ephem
    rows = g["rows"]
    R = 5
    sim.synth(R, seed=14, to_host=False)
    before = ctx.batch_download(0, R)
    tables = [rows[:2], rows[2:5], rows[5:8], rows[:1], rows[9:]]
    # R + 1 tables: the Python surface refuses the shape, the library the call
    with pytest.raises(ValueError):
        sim.add_roemer_delay(tables + [rows[:1]])
    n_tab, ro, tab = ephem.perturbation_tables(tables + [rows[:1]], R + 1)
    with pytest.raises(capi.FptaError, match="6 row tables for a block of 5 realizations"):
        ctx.batch_roemer_accumulate(lay[2], n_tab, ro, tab)
    np.testing.assert_array_equal(ctx.batch_download(0, R), before)
    bad = [t.copy() for t in tables]
    bad[2][1, 17] = np.nan
    with pytest.raises(capi.FptaError, match="realization 2, row 1: non-finite d_inc"):
        sim.add_roemer_delay(bad)
    np.testing.assert_array_equal(ctx.batch_download(0, R), before)
    bad = [t.copy() for t in tables]
    bad[4][0, 11] = 8.0  # e + 8 t leaves [0, 0.95] inside the span
    with pytest.raises(capi.FptaError, match="realization 4, row 0: eccentricity"):
        sim.add_roemer_delay(bad)
    np.testing.assert_array_equal(ctx.batch_download(0, R), before)
    bad = rows.copy()
    bad[7, 21] = 0.0  # one table for all: 1 / mass_ss
    with pytest.raises(capi.FptaError, match="realization 0, row 7: mass_ss"):
        sim.add_roemer_delay(bad)
    bad = [t.copy() for t in tables]
    bad[1][2, 21] = 0.0
    with pytest.raises(capi.FptaError, match="realization 1, row 2: mass_ss"):
        sim.add_roemer_delay(bad)
    for sign in (np.inf, np.nan):
        with pytest.raises(capi.FptaError, match="non-finite sign"):
            sim.add_roemer_delay(tables, sign=sign)
    np.testing.assert_array_equal(ctx.batch_download(0, R), before)
    # no rows at all: a successful no-op
    sim.add_roemer_delay([rows[:0]] * R)
    sim.add_roemer_delay(rows[:0])
    np.testing.assert_array_equal(ctx.batch_download(0, R), before)


def test_no_block_is_a_state_error(capi, g, lay):
    c = capi.Context(0)
    try:
        ro = np.array([0, 12], dtype=np.int64)
        with pytest.raises(capi.FptaError, match="set_toas first"):
            c.batch_roemer_accumulate(lay[2], 1, ro, g["rows"])
        s = _simulator(c, *lay, seed=1)
        with pytest.raises(capi.FptaError, match=r"\(-77\).*nothing synthesized"):
            c.batch_roemer_accumulate(lay[2], 1, ro, g["rows"])
        with pytest.raises(capi.FptaError, match=r"\(-77\)"):
            s.add_roemer_delay(g["rows"])
        base = s.synth(2, seed=1)
        s.add_roemer_delay(g["rows"])  # and with a block it goes through
        assert not np.array_equal(c.batch_download(0, 2), base)
    finally:
        c.close()


# ----------------------------------------------------------------------------- 7. kernel stats
def test_kernel_stats_count_the_call(ctx, capi, g, sim):
    ctx.set_option(capi.OPT_PROFILE, 1)
    sim.synth(4, seed=15, to_host=False)
    for tables in ([g["rows"]] * 4, g["rows"]):  # k_roemer_block; k_roemer_main and k_cw_bcast
        ctx.reset_stats()
        sim.add_roemer_delay(tables)
        ctx.synchronize()
        n, ms = ctx.kernel_stats(capi.K_EPHEM)
        assert n == 1 and ms > 0


# ----------------------------------------------------------------------------- 6. consumers (tests/test_gpu_cw_batch.py's layouts)
def population(g, n_real):
    """Realization r: two or three of the fixture's rows, a different set and mass error in each."""
    pop = []
    for r in range(n_real):
        t = g["rows"][[r % 12, (r + 5) % 12, (r + 7) % 12][:2 + r % 2]].copy()
        t[:, 14] += 1e20 * (r + 1)
        pop.append(t)
    return pop


def test_consumers_see_the_delays(ctx, capi, g, gridded):
    s, psrs, offs, w = gridded
    R = 33
    ctx.set_option(capi.OPT_FUSE_CHECKSUMS, 1)
    s.synth(R, seed=4, real0=101, to_host=False)
    assert ctx.batch_grid_info()["last_path"] == 4
    pre_sums = s.checksums()
    s.add_roemer_delay(population(g, R))
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


def test_simulate_sharded_with_add_roemer_delay_as_the_consumer(ctx, capi, g, gridded):
    from fakepta_amd.batch import simulate_sharded
    s, psrs, offs, w = gridded
    n_real, batch_size = 48 + 33, 48
    pop = population(g, n_real)
    got = simulate_sharded(s, n_real, seed=4, batch=batch_size,
                           on_batch=lambda sim, first, n: (sim.add_roemer_delay(pop[first:first + n]), sim.project()))
    assert got.shape == (n_real, 2)
    ctx.set_option(capi.OPT_MFMA_MIN_REAL, 1)  # as the job sets it
    for first in range(0, n_real, batch_size):
        n = min(batch_size, n_real - first)
        plain = s.synth(n, seed=4, real0=first, fit=True)
        s.synth(n, seed=4, real0=first, to_host=False)
        s.add_roemer_delay(pop[first:first + n])
        s.project()
        block = ctx.batch_download(0, n)
        assert not np.array_equal(block, plain)
        es = np.abs(got[first:first + n].astype(LD) - LDR.checksum_truth(block))
        assert np.all(es <= _checksum_bound(block))


@pytest.mark.parametrize("next_real0,hit", [(384, True), (1000, False)])
def test_injection_leaves_the_next_block_alone(shared_span, g, next_real0, hit):
    """The block after an injected one is bit for bit the block after an untouched one, whether the earlier block's
    kernel had already made its common-signal mix (a next-mix hit) or not (a jump: a miss)."""
    from fakepta_amd import ephem
    c, pos = shared_span
    n_tab, ro, rows = ephem.perturbation_tables(population(g, 128), 128)
    outs = []
    for inject in (False, True):
        for real0 in (0, 128, 256):  # hits start at the third block of a pipelined run
            c.batch_synth(7, real0, 128, to_host=False)
        assert c.batch_grid_info()["interp_kernel"].startswith("k_grid_fused<")
        if inject:
            pre = c.batch_download(0, 128)
            c.batch_roemer_accumulate(pos, n_tab, ro, rows)
            assert not np.array_equal(c.batch_download(0, 128), pre)
        outs.append(c.batch_synth(7, next_real0, 128))
        assert c.batch_grid_info()["next_mix_used"] == hit
    np.testing.assert_array_equal(outs[1], outs[0])
