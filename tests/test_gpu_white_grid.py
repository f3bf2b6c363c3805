"""Gridded white / ECORR blocks and three-grid-signal blocks on the kernels that ship for them (k_grid_dft_gen +
k_grid_interp_mfma<true, ..>; plain blocks of such layouts on k_grid_interp_ws), on a ragged C5-like layout: RN + HD /
monopole / dipole common signals in one grid signal, DM and Sv in two more, white noise + 2-TOA ECORR epochs. Against
the oracle, pipelined against one-stream, and the kernel choice. (The opt-in fused kernel these layouts once had,
option key 24, is removed: DESIGN.md §9.)

Reference loops: /root/reference/fakepta/fake_pta.py:201-253 (white / ECORR), 372-387 (per-pulsar GP),
correlated_noises.py:153-160 (ORF-mixed common signals).
"""
import numpy as np
import pytest

from oracle import fakepta_oracle as O
from tests.conftest import assert_parity, rel_err
from tests.test_gpu_grid import GRID_TOL, TOL

pytestmark = pytest.mark.gpu


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
    assert opts[capi.OPT_INTERP_FUSED] == 1
    return opts


def _c5_like(ctx, rng, P=17, n=(40, 500), white=True, ecorr=True, sv=True, commons=("hd", "monopole", "dipole")):
    """C5's signal mix on ragged pulsars over one common span: every epoch observed by two backends (np.repeat, as
    fake_pta.Pulsar), RN30, DM100 (idx 2), Sv60 (idx 4), the common signals on f_k = k / T (ORF factors of rank P,
    1 and 3), per-TOA white sigma and one 2-TOA ECORR block per (backend, epoch pair); one pulsar of 7 TOAs, one of 33.
    Returns the oracle's segments and white parameters."""
    counts = rng.integers(n[0], n[1], size=P) // 2 * 2
    counts[2], counts[3] = 6, 34
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    t0, t1 = 4.4e9, 4.4e9 + 3.15e8
    toas, nu = [], []
    for k in counts:
        ep = np.concatenate([[t0], np.sort(rng.uniform(t0, t1, k // 2 - 2)), [t1]]) if k >= 4 else np.array([t0, t1])
        toas.append(np.repeat(ep, 2))
        nu.append(np.abs(np.tile([1400.0, 800.0], k // 2) + rng.normal(0, 10, k)))
    toas, nu = np.concatenate(toas), np.concatenate(nu)
    T = t1 - t0
    ctx.batch_set_toas(offs, toas, nu)
    segs = []
    for nm, idx in ((30, 0.0), (100, 2.0)) + (((60, 4.0),) if sv else ()):
        f = np.tile(np.arange(1, nm + 1) / T, (P, 1))
        a = np.sqrt(O.powerlaw(f, rng.uniform(-14.5, -13.5, (P, 1)), 3.0) / T)
        ctx.batch_add_signal(0, f, a, idx=idx)
        segs.append(O.Segment(0, 2 * np.pi * f, a, idx))
    v = rng.normal(size=(P, 3))
    pos = v / np.linalg.norm(v, axis=1)[:, None]
    orfs = {"hd": O.orf_hd, "monopole": O.orf_monopole, "dipole": O.orf_dipole}
    from fakepta_amd.batch import batch_factor
    for name in commons:
        fc = np.arange(1, 31) / T
        ac = np.sqrt(O.powerlaw(fc, -14.5, 13 / 3) / T)
        L = batch_factor(orfs[name](pos))
        ctx.batch_add_signal(1, fc, ac, L=L)
        segs.append(O.Segment(1, 2 * np.pi * fc, ac, 0.0, L=L))
    sigma = rng.uniform(0.5e-7, 2e-7, offs[-1]) if white else None
    blocks, esig, block_of = [], [], -np.ones(offs[-1], dtype=np.int64)
    if ecorr:
        for p in range(P):
            idx = np.arange(offs[p], offs[p + 1])
            for b in (0, 1):  # backend b: TOAs of the backend, epochs of two consecutive times
                tb = idx[b::2]
                for j in range(0, len(tb), 2):
                    blocks.append(tb[j:j + 2])
        esig = rng.uniform(0.5e-7, 1.5e-7, len(blocks))
        for i, q in enumerate(blocks):
            block_of[q] = i
    ctx.batch_set_white(sigma, blocks if ecorr else [], esig if ecorr else [])
    return offs, toas, nu, segs, sigma, (block_of if ecorr else None), (np.asarray(esig) if ecorr else None)


def _run(ctx, seed, real0, R):
    ctx.batch_synth(seed, 0, R, to_host=False)
    ctx.debug_fill_out(np.nan)
    out = ctx.batch_synth(seed, real0, R)
    return out, ctx.batch_grid_info()["interp_kernel"]


@pytest.mark.parametrize("case", ["white_ecorr", "white", "ecorr", "plain", "two_grid_white"])
def test_c5_like_layouts_match_oracle(ctx, capi, shipped, case):
    """The shipped options (+ FPTA_OPT_SYNTH_PATH 4) against the oracle at the gridded tolerance: realization counts off
    the realization tiles (R_pad padding), odd first realizations (the white stream's misaligned quads), every sample
    written (NaN-poisoned block), no k_grid_fused instance. R = 333 and 100: the whole block; R = 16 and 1024: the
    first, a middle and the last realization, each against the oracle's one-realization range."""
    rng = np.random.default_rng(401 + len(case))
    kw = dict(white=case in ("white_ecorr", "white", "two_grid_white"), ecorr=case in ("white_ecorr", "ecorr"),
              sv=case != "two_grid_white")
    offs, toas, nu, segs, sigma, block_of, esig = _c5_like(ctx, rng, **kw)
    try:
        ctx.set_option(capi.OPT_SYNTH_PATH, 4)
        for R, real0 in ((333, 5), (16, 0), (100, 77), (1024, 3)):
            got, k = _run(ctx, 13, real0, R)
            assert np.all(np.isfinite(got))
            assert not k.startswith("k_grid_fused"), k
            if R in (333, 100):
                want = O.batch_synth(offs, toas, nu, segs, 13, real0, R, sigma=sigma, block_of=block_of,
                                     ecorr_sigma=esig)
            else:
                rows = [0, R // 2 - 1, R - 1]
                want = np.concatenate([O.batch_synth(offs, toas, nu, segs, 13, real0 + r, 1, sigma=sigma,
                                                     block_of=block_of, ecorr_sigma=esig) for r in rows])
                got = got[rows]
            assert rel_err(got, want) <= GRID_TOL, (R, real0, rel_err(got, want))
            assert_parity(got, want, TOL)
    finally:
        ctx.batch_set_white()
        ctx.batch_clear()
        ctx.set_options(shipped)


def test_pipelined_blocks_and_determinism(ctx, capi, shipped):
    """Pipelined blocks (FPTA_OPT_OVERLAP 1: the next block's common draws into the other coefficient buffer on the
    side stream while this block's kernels read their own) equal one-stream blocks bit for bit, run to run, with their
    checksums; batch-split invariance (a realization's samples do not depend on the block it is drawn in)."""
    rng = np.random.default_rng(433)
    _c5_like(ctx, rng, P=20, n=(200, 700))
    try:
        ctx.set_option(capi.OPT_SYNTH_PATH, 4)
        res = {}
        for ov in (0, 1):
            ctx.set_option(capi.OPT_OVERLAP, ov)
            for b in range(3):
                ctx.batch_synth(29, 256 * b, 256, to_host=False)
            res[ov, "last"] = ctx.batch_synth(29, 256 * 3, 256)
            assert not ctx.batch_grid_info()["interp_kernel"].startswith("k_grid_fused")
            res[ov, "each"] = [(ctx.batch_synth(29, 300 * b + 1, 300), ctx.batch_checksums()) for b in range(3)]
        np.testing.assert_array_equal(res[0, "last"], res[1, "last"])
        for (x, xs), (y, ys) in zip(res[0, "each"], res[1, "each"]):
            np.testing.assert_array_equal(x, y)
            np.testing.assert_array_equal(xs, ys)
        whole = ctx.batch_synth(29, 100, 64)
        split = np.concatenate([ctx.batch_synth(29, 100, 17), ctx.batch_synth(29, 117, 47)])
        np.testing.assert_array_equal(whole, split)
    finally:
        ctx.batch_set_white()
        ctx.batch_clear()
        ctx.set_options(shipped)


def test_kernel_choice_and_retired_key(ctx, capi, shipped):
    """A plain block of a two-grid-signal layout runs on k_grid_fused; the same layout with white noise takes the DFT +
    interpolation kernels. Option key 24 (the removed kernel's) is refused by set_option and get_option."""
    rng = np.random.default_rng(439)
    try:
        offs = _c5_like(ctx, rng, P=6, n=(100, 300), white=False, ecorr=False, sv=False)[0]
        ctx.set_option(capi.OPT_SYNTH_PATH, 4)
        ctx.batch_synth(3, 0, 256, to_host=False)
        k = ctx.batch_grid_info()["interp_kernel"]
        assert k.startswith("k_grid_fused<"), k
        ctx.batch_set_white(rng.uniform(0.5e-7, 2e-7, offs[-1]), [], [])
        ctx.batch_synth(3, 0, 256, to_host=False)
        k = ctx.batch_grid_info()["interp_kernel"]
        assert not k.startswith("k_grid_fused"), k
        with pytest.raises(capi.FptaError):
            ctx.set_option(24, 1)
        with pytest.raises(capi.FptaError):
            ctx.get_option(24)
    finally:
        ctx.batch_set_white()
        ctx.batch_clear()
        ctx.set_options(shipped)


def test_coeffs_after_pipelined_ecorr_blocks(ctx, capi, shipped):
    """A coefficient download after pipelined ECORR blocks (FPTA_OPT_OVERLAP 1) succeeds and changes no sample: the
    block reads its epoch normals realization-major whichever way its coefficients are drawn. (With the removed
    kernel's option on, this call failed with FPTA_ESTATE.)"""
    rng = np.random.default_rng(443)
    _c5_like(ctx, rng, P=8, n=(100, 300))
    try:
        ctx.set_option(capi.OPT_SYNTH_PATH, 4)
        ctx.set_option(capi.OPT_OVERLAP, 1)
        for b in range(2):
            ctx.batch_synth(7, 256 * b, 256, to_host=False)
        out, co = ctx.batch_synth(7, 512, 64, coeffs=True)
        assert np.all(np.isfinite(out)) and np.all(np.isfinite(co))
        np.testing.assert_array_equal(out, ctx.batch_synth(7, 512, 64))
    finally:
        ctx.batch_set_white()
        ctx.batch_clear()
        ctx.set_options(shipped)
