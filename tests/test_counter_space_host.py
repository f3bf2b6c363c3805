"""CPU half of tests/test_gpu_counter_space.py (tests/counter_space.py holds what the two share).

(a) The oracle's counter assembly (numpy casts of uint64 realizations and of the 64-bit seed) against a restatement in
    Python integers, at the seeds and realizations the GPU tests visit: 64-bit seeds, realizations around bit 31, at
    the batch limit 2^32 and, for the indexed streams, up to the dense limit 2^33.
(b) A test of the tests: every comparison helper of the GPU tests rejects the oracle's own answer under each wrong
    counter convention a kernel or its host plumbing could have (the high key word dropped, k0 used for both words, the
    realization reduced modulo 2^31, and, in the dense range, g >> 1 taken after g was cut to 32 bits), on the layouts
    the GPU tests run, and accepts the right answer.
"""
import numpy as np
import pytest

from oracle import fakepta_oracle as O
from tests import counter_space as S
from tests.test_gpu_dense import _random_case
from tests.test_gpu_fused_shapes import _CASES, _layout as fused_layout
from tests.test_gpu_white_grid import _c5_like

SEEDS = (S.S_HI, S.S_K1, -1, 0x80000000, 7)
GP_REALS = (0, 1, S.BIT31_ODD, S.BIT31_EVEN, S.B31 - 2, S.B31 - 1, S.B31, S.B31 + 1, S.B32 - 40, S.B32 - 9, S.B32 - 2,
            S.B32 - 1)
QUAD_REALS = GP_REALS + (S.B32, S.B32 + 1, S.B32 + 3, S.B33 - 9, S.B33 - 2, S.B33 - 1)


# ----------------------------------------------------------------------------- (a) the oracle's counters
def test_seed_key_words():
    for seed in SEEDS + (2 ** 64 - 1, 2 ** 63, 0):
        assert tuple(int(w) for w in O.seed_key(seed)) == S.key_py(seed)
    assert S.key_py(S.S_HI) == (0x7F4A7C15, 0x9E3779B9) and S.key_py(S.S_K1) == (0, 1)
    np.testing.assert_array_equal(O.seed_key(-1), O.seed_key(2 ** 64 - 1))
    np.testing.assert_array_equal(O.seed_key(-1), [0xFFFFFFFF, 0xFFFFFFFF])


@pytest.mark.parametrize("seed", SEEDS)
def test_gp_normals_counters(seed):
    """O.gp_normals of realization g = normals (2 (g & 1), 2 (g & 1) + 1) of the call ctr = (k, p, seg, g >> 1)."""
    n_modes = 5
    for p, seg in ((0, 0), (63, 2)):
        got = O.gp_normals(seed, np.array(GP_REALS), p, seg, n_modes)  # [R, N, 2]
        for i, g in enumerate(GP_REALS):
            for k in (0, n_modes - 1):
                ctr, pick = S.gp_counter_py(k, p, seg, g)
                z = S.normals_of_counter(ctr, seed)
                np.testing.assert_array_equal(got[i, k], z[pick:pick + 2], err_msg=f"g={g} k={k}")


@pytest.mark.parametrize("stream", [O.WHITE_STREAM, O.ECORR_STREAM, O.DENSE_STREAM])
@pytest.mark.parametrize("seed", SEEDS)
def test_quad_normals_counters(seed, stream):
    """O.quad_normals of (index i, realization g) = normal 2 (i & 1) + (g & 1) of ctr = (i >> 1, 0xFFFFFFFF, stream,
    g >> 1), up to g = 2^33 - 1 (g >> 1 fills the counter word)."""
    n = 7
    got = O.quad_normals(seed, np.array(QUAD_REALS, dtype=np.uint64), n, stream)
    for j, g in enumerate(QUAD_REALS):
        for i in range(n):
            ctr, pick = S.quad_counter_py(i, stream, g)
            assert got[j, i] == S.normals_of_counter(ctr, seed)[pick], (g, i)


def test_block_entry_points_take_the_same_counters():
    """O.batch_coefficients, the white / ECORR part of O.batch_synth and O.dense_draws are gp_normals / quad_normals of
    the global realization: a window at the limit, row by row."""
    f = np.arange(1, 4) / 3e8
    a = np.full((2, 3), 1e-7)
    segs = [O.Segment(0, 2 * np.pi * np.tile(f, (2, 1)), a)]
    co = O.batch_coefficients(segs, 2, S.S_HI, S.B32 - 3, 3)[0]  # [R, P, N, 2]
    for r in range(3):
        for p in range(2):
            for k in range(3):
                ctr, pick = S.gp_counter_py(k, p, 0, S.B32 - 3 + r)
                np.testing.assert_array_equal(co[r, p, k], 1e-7 * S.normals_of_counter(ctr, S.S_HI)[pick:pick + 2])
    offs, toas, nu = np.array([0, 3]), np.array([1e8, 2e8, 3e8]), np.full(3, 1400.0)
    sigma, block_of, esig = np.array([1.0, 2.0, 3.0]), np.array([0, 0, -1]), np.array([5.0])
    out = O.batch_synth(offs, toas, nu, [], S.S_K1, S.B32 - 2, 2, sigma=sigma, block_of=block_of, ecorr_sigma=esig)
    for r in range(2):
        g = S.B32 - 2 + r
        for t in range(3):
            ctr, pick = S.quad_counter_py(t, O.WHITE_STREAM, g)
            want = sigma[t] * S.normals_of_counter(ctr, S.S_K1)[pick]
            if block_of[t] >= 0:
                ctr, pick = S.quad_counter_py(0, O.ECORR_STREAM, g)
                want += esig[0] * S.normals_of_counter(ctr, S.S_K1)[pick]
            assert out[r, t] == want
    d = O.dense_draws(np.eye(3), S.S_HI, S.B33 - 2, 2)
    for r in range(2):
        for t in range(3):
            ctr, pick = S.quad_counter_py(t, O.DENSE_STREAM, S.B33 - 2 + r)
            assert d[r, t] == S.normals_of_counter(ctr, S.S_HI)[pick]


def test_oracle_rows_restates_the_conventions():
    fn = lambda seed, real0, n: np.array([[seed, g] for g in range(real0, real0 + n)], dtype=object)  # noqa: E731
    rows = S.oracle_rows(fn, S.S_HI, S.B31 - 2, 4, "g_mod_2_31")
    assert rows.tolist() == [[S.S_HI, S.B31 - 2], [S.S_HI, S.B31 - 1], [S.S_HI, 0], [S.S_HI, 1]]
    rows = S.oracle_rows(fn, S.S_HI, S.B32 - 1, 3, "g_trunc_32")
    assert rows.tolist() == [[S.S_HI, S.B32 - 1], [S.S_HI, 0], [S.S_HI, 1]]
    assert S.oracle_rows(fn, S.S_HI, 5, 2, "k1_dropped").tolist() == [[0x7F4A7C15, 5], [0x7F4A7C15, 6]]
    assert S.oracle_rows(fn, S.S_HI, 5, 1, "k0_twice").tolist() == [[0x7F4A7C157F4A7C15, 5]]
    assert S.oracle_rows(fn, -1, 5, 1, "k1_dropped").tolist() == [[0xFFFFFFFF, 5]]
    assert S.oracle_rows(fn, 9, 5, 2).tolist() == [[9, 5], [9, 6]]


# ----------------------------------------------------------------------------- (b) a test of the tests
BATCH_WRONG = ("k1_dropped", "k0_twice", "g_mod_2_31")


def _rejects(check, wrong_answer, right_answer):
    check(right_answer, right_answer)
    with pytest.raises(AssertionError):
        check(wrong_answer, right_answer)


@pytest.fixture(scope="module")
def plain():
    """The fused kernel's smallest shaped layout (test_gpu_fused_shapes gen_load_1_1)."""
    rn, dm, gw, nu_const = _CASES["gen_load_1_1"][:4]
    offs, toas, nu, segs = fused_layout(S.RecordingCtx(), np.random.default_rng(1), 3, rn, dm, gw, nu_const)
    return offs, toas, nu, segs


@pytest.mark.parametrize("seed", [S.S_HI, S.S_K1])
@pytest.mark.parametrize("wrong", BATCH_WRONG)
def test_block_and_checksum_helpers_reject(plain, wrong, seed):
    offs, toas, nu, segs = plain
    fn = lambda s, r0, n: O.batch_synth(offs, toas, nu, segs, s, r0, n)  # noqa: E731
    for real0, R in S.windows(33, 34):
        right = fn(seed, real0, R)
        bad = S.oracle_rows(fn, seed, real0, R, wrong)
        with pytest.raises(AssertionError):
            S.check_block(bad, right)
        # the realizations the convention moves: every one for a key defect, those with bit 31 set for g mod 2^31
        moved = [r for r in range(R) if wrong != "g_mod_2_31" or real0 + r >= S.B31]
        assert moved
        for r in (moved[0], moved[-1]):
            S.check_sums((right[r].sum(), (right[r] ** 2).sum()), right[r])
            with pytest.raises(AssertionError):
                S.check_sums((bad[r].sum(), (bad[r] ** 2).sum()), right[r])
    S.check_block(right, right)


@pytest.mark.parametrize("wrong", BATCH_WRONG)
def test_block_helper_rejects_on_the_white_streams(wrong):
    """White noise and ECORR alone (no GP signal): the indexed streams' counters."""
    offs, toas, nu, segs, sigma, block_of, esig = _c5_like(S.RecordingCtx(), np.random.default_rng(2), P=4, n=(40, 60),
                                                           sv=False, commons=())
    fn = lambda s, r0, n: O.batch_synth(offs, toas, nu, [], s, r0, n, sigma=sigma, block_of=block_of,  # noqa: E731
                                        ecorr_sigma=esig)
    only_ecorr = lambda s, r0, n: O.batch_synth(offs, toas, nu, [], s, r0, n, block_of=block_of,  # noqa: E731
                                                ecorr_sigma=esig)
    for f in (fn, only_ecorr):
        for real0, R in ((S.BIT31_ODD, 33), (S.B32 - 33, 33)):
            right = f(S.S_HI, real0, R)
            bad = S.oracle_rows(f, S.S_HI, real0, R, wrong)
            with pytest.raises(AssertionError):
                S.check_block(bad, right)


@pytest.mark.parametrize("wrong", BATCH_WRONG)
def test_coefficient_helper_rejects(plain, wrong):
    offs, toas, nu, segs = plain
    P = len(offs) - 1
    fn = lambda s, r0, n: np.transpose(S.oracle_coeffs(segs, P, s, r0, n), (2, 0, 1))  # noqa: E731
    for seed in (S.S_HI, S.S_K1):
        for real0, R in ((S.BIT31_ODD, 19), (S.B32 - 9, 9)):
            right = np.transpose(fn(seed, real0, R), (1, 2, 0))
            bad = np.transpose(S.oracle_rows(fn, seed, real0, R, wrong), (1, 2, 0))
            assert right.shape == (P, 2 * sum(s.n_modes for s in segs), R)
            _rejects(S.check_coeffs, bad, right)


@pytest.mark.parametrize("wrong", sorted(S.WRONG))
def test_dense_helper_rejects(wrong):
    toas, nu, segs, osigs, white = _random_case(264, 64, white_scale=1e-6)
    cov = O.dense_cov(toas, nu, osigs) + np.diag(white)
    fn = lambda s, r0, n: O.dense_draws(cov, s, r0, n)  # noqa: E731
    for real0, R in S.DENSE_STARTS:
        right = fn(S.S_HI, real0, R)
        _rejects(S.check_draws, S.oracle_rows(fn, S.S_HI, real0, R, wrong), right)
