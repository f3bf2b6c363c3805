"""k_grid_fused's draw shapes (csrc/fused_sched.h): a shaped instance issues only the draw and table loads an
iteration of the DFT waves' ring loop reads, every other layout takes the fallback with all loads in place. Small layouts
at the edges of that schedule: group counts (ng0, ng1) of the two grid signals from (1, 1), where one iteration is
both first and last, to C2's (2, 7) and its mirror, and every term pattern. The reported kernel is the instance the
layout always had, whichever variant of it ran; which one did is asserted through fpta_debug_fused_shape.

Each case: whole-chunk bands (FPTA_OPT_INTERP_FUSED 2) equal the two-kernel path (0) bit for bit, half-chunk bands
(3) match the oracle at the project's tolerance, every sample is written (NaN-poisoned block), with 33 realizations
from an odd first one (the ODD instances, padding realizations) and 64 from an even one.
"""
import numpy as np
import pytest

from oracle import fakepta_oracle as O
from tests.conftest import assert_parity

pytestmark = pytest.mark.gpu

TOL = 1e-10  # the project's parity tolerance


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
def shipped(ctx):
    return ctx.options()


def _layout(ctx, rng, P, rn, dm, gw, nu_const=False, n=(40, 101)):
    """P pulsars of 40 to 100 TOAs on one common span T, every signal on f_k = k / T: red noise of rn modes (idx 0), DM
    of dm modes (idx 2) and a common HD signal of gw modes (0: none of that kind). Signals of one chromatic weight
    coalesce into one grid signal, the one of most modes its anchor: RN and the common signal always, DM too at a single
    radio frequency (nu_const)."""
    counts = rng.integers(n[0], n[1], size=P)
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    t0, t1 = 4.4e9, 4.4e9 + 3.15e8
    toas = np.concatenate([np.concatenate([[t0], np.sort(rng.uniform(t0, t1, k - 2)), [t1]]) for k in counts])
    nu = np.full(offs[-1], 1400.0) if nu_const else rng.choice([800.0, 1400.0, 2500.0], size=offs[-1])
    T = t1 - t0
    ctx.batch_set_toas(offs, toas, nu)
    segs = []
    for nm, idx in ((rn, 0.0), (dm, 2.0)):
        if nm:
            f = np.tile(np.arange(1, nm + 1) / T, (P, 1))
            a = np.sqrt(O.powerlaw(f, rng.uniform(-14.5, -13.5, (P, 1)), 3.0) / T)
            ctx.batch_add_signal(0, f, a, idx=idx)
            segs.append(O.Segment(0, 2 * np.pi * f, a, idx))
    if gw:
        fc = np.arange(1, gw + 1) / T
        ac = np.sqrt(O.powerlaw(fc, -14.0, 13 / 3) / T)
        v = rng.normal(size=(P, 3))
        L = O.mvn_factor(O.orf_hd(v / np.linalg.norm(v, axis=1)[:, None]))
        ctx.batch_add_signal(1, fc, ac, L=L)
        segs.append(O.Segment(1, 2 * np.pi * fc, ac, 0.0, L=L))
    return offs, toas, nu, segs


def _run(ctx, capi, fused, seed, real0, R):
    ctx.set_option(capi.OPT_INTERP_FUSED, fused)
    ctx.batch_synth(seed, 0, R, to_host=False)
    ctx.debug_fill_out(np.nan)
    out = ctx.batch_synth(seed, real0, R)
    return out, ctx.batch_grid_info()["interp_kernel"], ctx.debug_fused_shape()


def _instance(name):
    """(NQ, ODD, GEN, HALF) of a reported k_grid_fused<...> name."""
    assert name.startswith("k_grid_fused<") and name.endswith(">"), name
    nq, odd, gen, half = name[len("k_grid_fused<"):-1].split(", ")
    return int(nq), odd == "true", gen == "true", half == "true"


# draw shapes (csrc/fused_sched.h)
ANY, GEN_LOAD, LOAD = 0, 1, 2

# (rn, dm, gw modes, one radio frequency, grid signals, draws in the kernel, the variant that must run): the terms of
# grid signal 0 / 1 and their group counts (fused_groups: 2 and 16 modes are 1 group, 18 and 30 are 2, 100 are 7)
_CASES = {
    "gen_load_2_7": (30, 100, 30, False, 2, True, GEN_LOAD),   # {RN, GWB} / {DM}: C2, (2, 7)
    "gen_load_7_2": (100, 30, 18, False, 2, True, GEN_LOAD),   # the mirror: signal 0 draws alone for five iterations
    "gen_load_1_1": (2, 16, 2, False, 2, True, GEN_LOAD),      # one iteration, first and last at once
    "gen_load_1_2": (16, 18, 2, False, 2, True, GEN_LOAD),
    "gen_load_2_1": (18, 2, 16, False, 2, True, GEN_LOAD),
    "gen_only_2_7": (30, 100, 0, False, 2, True, ANY),         # {RN} / {DM}: no loaded term
    "gen_only_1_1": (16, 2, 0, False, 2, True, ANY),
    "load_anchor_2_7": (18, 100, 30, False, 2, True, ANY),     # {GWB, RN}: the common signal is the anchor
    "load_only_7": (0, 0, 100, False, 1, False, LOAD),         # one mixed common signal: the instance without draws (C4)
    "load_only_1": (0, 0, 16, False, 1, False, LOAD),
    "three_members": (30, 100, 18, True, 1, True, ANY),        # RN + DM + GWB in one grid signal: a member past the
}                                                              # prefetched slots, which only the fallback draws


@pytest.mark.parametrize("case", sorted(_CASES))
def test_fused_shapes_bitwise_and_oracle(ctx, capi, shipped, case):
    rn, dm, gw, nu_const, n_grid, gen, shape = _CASES[case]
    rng = np.random.default_rng(4000 + sorted(_CASES).index(case))
    offs, toas, nu, segs = _layout(ctx, rng, int(rng.integers(3, 6)), rn, dm, gw, nu_const)
    try:
        ctx.set_option(capi.OPT_SYNTH_PATH, 4)
        for R, real0 in ((33, 5), (64, 0)):
            ref, k0, s0 = _run(ctx, capi, 0, 17, real0, R)
            got, k2, s2 = _run(ctx, capi, 2, 17, real0, R)
            half, k3, s3 = _run(ctx, capi, 3, 17, real0, R)
            # the path that ran: the two-kernel path, then the shape's instance or the fallback as the layout demands
            assert (s0, s2, s3) == (-1, shape, shape), (case, s0, s2, s3)
            assert ctx.batch_grid_info()["grid_signals"] == n_grid, ctx.batch_grid_info()
            assert not k0.startswith("k_grid_fused"), k0
            # the instance this layout has always had: draws in the kernel iff a per-pulsar member, the ODD one iff
            # they start from an odd realization, bands as the option says
            for k, is_half in ((k2, False), (k3, True)):
                nq, odd, kgen, khalf = _instance(k)
                assert (odd, kgen, khalf) == (gen and real0 % 2 == 1, gen, is_half), (case, k)
                assert nq in (8, 12), k
            assert np.all(np.isfinite(got)) and np.all(np.isfinite(half))
            np.testing.assert_array_equal(ref, got)
            want = O.batch_synth(offs, toas, nu, segs, 17, real0, R)
            assert_parity(half, want, TOL)
            assert_parity(got, want, TOL)
    finally:
        ctx.batch_clear()
        ctx.set_options(shipped)


def test_fused_shapes_pipelined_next_mix(ctx, capi, shipped):
    """Pipelined blocks of C2's pattern at 64 pulsars (the fewest whose mix the fused kernel makes for its successor):
    the third block takes its mix from the second block's kernel and equals the same block on the two-kernel path
    without that mix, bit for bit."""
    rng = np.random.default_rng(4100)
    _layout(ctx, rng, 64, 30, 100, 30, n=(40, 60))
    try:
        ctx.set_option(capi.OPT_SYNTH_PATH, 4)
        ctx.set_option(capi.OPT_INTERP_FUSED, 2)
        ctx.set_option(capi.OPT_OVERLAP, 1)
        ctx.set_option(capi.OPT_FUSED_NEXT_MIX, 1)
        for b in range(2):
            ctx.batch_synth(23, 128 * b, 128, to_host=False)
        got = ctx.batch_synth(23, 256, 128)
        gi = ctx.batch_grid_info()
        assert gi["next_mix_used"], gi
        assert _instance(gi["interp_kernel"])[1:] == (False, True, False), gi
        assert ctx.debug_fused_shape() == GEN_LOAD
        ctx.set_option(capi.OPT_FUSED_NEXT_MIX, 0)
        ctx.set_option(capi.OPT_INTERP_FUSED, 0)
        ref = ctx.batch_synth(23, 256, 128)
        assert not ctx.batch_grid_info()["next_mix_used"] and ctx.debug_fused_shape() == -1
        assert np.all(np.isfinite(got))
        np.testing.assert_array_equal(ref, got)
    finally:
        ctx.batch_clear()
        ctx.set_options(shipped)
