"""The (seed, realization) points and the comparison helpers of tests/test_gpu_counter_space.py, importable without a
GPU so that tests/test_counter_space_host.py can test them: the oracle's counters against a restatement in Python
integers, and every helper against the oracle's own answer under a deliberately wrong counter convention.

Every draw is a function of (seed, global realization g): key (k0, k1) = (seed & 0xFFFFFFFF, seed >> 32), counter word 3
= g >> 1, normal picked by g & 1 (oracle gp_normals / quad_normals; philox.h gp_normal2 / quad_normal). The batch paths
take real0 + n_real <= 2^32, fpta_noise_draw <= 2^33.
"""
import numpy as np

from oracle import fakepta_oracle as O
from tests.conftest import assert_parity

TOL = 1e-10        # blocks: the project's parity tolerance
COEF_TOL = 1e-13   # downloaded coefficients: test_device_normals_match_oracle's element-wise bound
DENSE_TOL = 1e-9   # dense draws: test_draws_vs_oracle_and_split_invariance's bound

S_HI = 0x9E3779B97F4A7C15  # both key words nonzero, the top bit set
S_K1 = 1 << 32             # k0 == 0, k1 == 1
B31, B32, B33 = 1 << 31, 1 << 32, 1 << 33
BIT31_ODD, BIT31_EVEN = B31 - 17, B31 - 16  # blocks of >= 18 realizations from here straddle bit 31 of g
DENSE_STARTS = ((B32 - 5, 9), (B33 - 9, 9))  # (real0, n_real): g >> 1 reaches 2^31 inside; ends exactly at 2^33


def windows(R_odd, R_even):
    """(real0, n_real) of a batch kernel's cases: across bit 31 from an odd and an even start, and ending exactly at
    2^32 with an odd count (an odd start: the ODD instances) and an even one."""
    assert R_odd % 2 == 1 and R_even % 2 == 0 and min(R_odd, R_even) >= 18
    return ((BIT31_ODD, R_odd), (BIT31_EVEN, R_even), (B32 - R_odd, R_odd), (B32 - R_even, R_even))


# ----------------------------------------------------------------------------- counters in Python integers
def key_py(seed):
    seed = seed % (1 << 64)
    return seed % B32, seed // B32


def gp_counter_py(k, p, seg, g):
    """((c0, c1, c2, c3), first normal of the call's four that realization g takes as (cos, sin))."""
    return (k, p, seg, g // 2), 2 * (g % 2)


def quad_counter_py(i, stream, g):
    """((c0, c1, c2, c3), the normal of the call's four that (index i, realization g) takes)."""
    return (i // 2, 0xFFFFFFFF, stream, g // 2), 2 * (i % 2) + g % 2


def normals_of_counter(ctr, seed):
    """The four normals of one Philox call, its counter and key handed over as Python integers."""
    assert all(0 <= int(w) < B32 for w in ctr), ctr
    k0, k1 = key_py(seed)
    words = O.philox4x32_10(np.array([ctr], dtype=np.uint32), np.array([k0, k1], dtype=np.uint32))
    return O.normals4(words)[0]


# ----------------------------------------------------------------------------- wrong conventions
# Each maps (seed, g) to the (seed, g) whose right draws are the wrong convention's draws of the original pair.
def _drop_k1(seed, g):
    return seed % B32, g


def _k0_twice(seed, g):
    return (seed % B32) * (B32 + 1), g


def _g_mod_2_31(seed, g):
    return seed, g % B31


def _g_trunc_32(seed, g):  # g >> 1 taken after g was cut to 32 bits: the parity survives, bit 32 is lost
    return seed, g % B32


WRONG = {"k1_dropped": _drop_k1, "k0_twice": _k0_twice, "g_mod_2_31": _g_mod_2_31, "g_trunc_32": _g_trunc_32}


def oracle_rows(fn, seed, real0, n_real, wrong=None):
    """fn(seed, real0, n_real) -> array whose leading axis is the realization, evaluated for realizations
    real0 .. real0 + n_real - 1 under a wrong convention (None: the right one): the mapped realizations, run by run of
    consecutive ones."""
    if wrong is None:
        return fn(seed, real0, n_real)
    mapped = [WRONG[wrong](seed % (1 << 64), g) for g in range(real0, real0 + n_real)]
    out, i = [], 0
    while i < n_real:
        j = i + 1
        while j < n_real and mapped[j] == (mapped[i][0], mapped[j - 1][1] + 1):
            j += 1
        out.append(fn(mapped[i][0], mapped[i][1], j - i))
        i = j
    return np.concatenate(out, axis=0)


# ----------------------------------------------------------------------------- comparison helpers
def check_block(got, want):
    """A synthesized block [R, n_toa] against the oracle's."""
    assert np.all(np.isfinite(got))
    assert_parity(got, want, TOL)


def check_coeffs(co, want):
    """Downloaded coefficients [P][K][R] against the oracle's, pulsar by pulsar and element by element."""
    assert co.shape == want.shape, (co.shape, want.shape)
    for p in range(co.shape[0]):
        np.testing.assert_allclose(co[p], want[p], rtol=COEF_TOL, atol=COEF_TOL * np.abs(want[p]).max())


def check_draws(got, want):
    """Dense draws [R, n] against the oracle's."""
    assert np.all(np.isfinite(got))
    assert_parity(got, want, DENSE_TOL)


def check_sums(sums, row):
    """One realization's checksums (sum, sum of squares) against a row [n_toa] of that realization
    (test_c3_streamed_checksums_and_picks' bounds)."""
    np.testing.assert_allclose(sums[1], (row ** 2).sum(), rtol=1e-12)
    np.testing.assert_allclose(sums[0], row.sum(), rtol=1e-9, atol=1e-12 * np.abs(row).sum())


def oracle_coeffs(segs, P, seed, real0, n_real):
    """O.batch_coefficients in the download's layout [P][K][R]: per signal, mode by mode, cos then sin; an odd mode
    count is followed by the zero-amplitude mode the library pads it with."""
    a = O.batch_coefficients(segs, P, seed, real0, n_real)  # per signal [R, P, N, 2]
    a = [np.pad(x, ((0, 0), (0, 0), (0, x.shape[2] % 2), (0, 0))) for x in a]
    return np.concatenate([np.transpose(x, (1, 2, 3, 0)).reshape(P, -1, n_real) for x in a], axis=1)


class RecordingCtx:
    """Stands in for a Context in the suite's layout builders where only the layout is wanted (no device)."""

    def __getattr__(self, name):
        if name.startswith("batch_") or name in ("set_option", "set_options"):
            return lambda *a, **k: 0
        raise AttributeError(name)
