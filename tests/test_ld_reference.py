"""Pin the longdouble truths of tests/ld_reference.py to the reference's own recorded outputs (fixtures G2 and G3),
so that the GPU tests which measure against them measure against the reference's semantics. CPU only."""
import numpy as np
import pytest

from oracle import fakepta_oracle as O
from tests import ld_reference as T
from tests.conftest import assert_parity


@pytest.mark.parametrize("orf", ["hd", "monopole", "dipole", "curn"])
def test_common_truth_reproduces_g3(golden, orf):
    g = golden("g3_common.npz")
    f, psd, z, idx = g[f"{orf}_f"], g[f"{orf}_psd"], g[f"{orf}_z"], float(g[f"{orf}_idx"])
    df = O.delta_f(f)
    amp = df ** 0.5 * np.sqrt(psd)  # what add_common_correlated_noise hands to fpta_common_accumulate
    L = np.ascontiguousarray(g[f"{orf}_svdM"].T)
    delta, x = T.common_truth(g["offs"], g["toas"], g["freqs"], f, amp, idx, 1400.0, L, z)
    assert delta.dtype == np.longdouble and x.dtype == np.longdouble and x.shape == z.shape
    assert_parity(delta.astype(np.float64), g[f"{orf}_residuals"], 1e-12)
    # fourier[p][0 = cos, 1 = sin][k] = x sqrt(psd_k) / sqrt(df_k) (correlated_noises.py:157-158)
    fourier = (x * (np.sqrt(psd.astype(np.longdouble)) / np.sqrt(df.astype(np.longdouble)))[:, None, None])
    fourier = fourier.transpose(2, 1, 0).astype(np.float64)
    want = g[f"{orf}_fourier"]
    np.testing.assert_allclose(fourier, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())


@pytest.mark.parametrize("lab", ["rn", "dm", "sv"])
def test_gp_truth_reproduces_g2(golden, lab):
    g = golden("g2_single_psr.npz")
    toas, freqs = g["toas"], g["freqs"]
    f, idx = g[f"{lab}_f"], float(g[f"{lab}_idx"])
    coeffs = O.gp_coeffs_from_z(g[f"{lab}_psd"], g[f"{lab}_z"])
    sq_df = O.delta_f(f) ** 0.5
    seg = (f[None, :], (sq_df * coeffs[0::2])[None, :], (sq_df * coeffs[1::2])[None, :], idx, 1400.0)
    offs = np.array([0, len(toas)])
    delta = T.gp_truth(offs, toas, freqs, [seg], None, 1.0)
    assert delta.dtype == np.longdouble
    assert_parity(delta.astype(np.float64), g[f"{lab}_delta"], 1e-12)
    # the sign and the mask of the header's formula
    mask = np.arange(len(toas)) % 2 == 0
    half = T.gp_truth(offs, toas, freqs, [seg], [mask], -1.0)
    np.testing.assert_array_equal(half[mask], -delta[mask])
    assert not half[~mask].any()


def test_phase_is_exact_where_fp64_is_not():
    """2 pi frac(f t) at a real-MJD epoch: a whole number of cycles gives a zero phase exactly, and binary fractions
    of a cycle come out to fp64 rounding, where the fp64 product (2 pi f) t is already off by ~1e-13 rad."""
    t = np.array([4.5e9])
    f = np.array([2.0 ** -20, 3.0 * 2.0 ** -21])  # f t = 4291.5..., exact binary fractions
    want = 2 * np.pi * np.mod(f * t, 1.0)  # f t is exact in fp64 here (few significant bits)
    got = T.phase(f, t)[0]
    assert np.max(np.abs(got.astype(np.float64) - want)) <= 4 * T.EPS
    assert T.phase(np.array([1.0 / 1024.0]), np.array([1024.0 * 4394531.0]))[0, 0] == 0


def test_statistics_truths_small_case():
    rng = np.random.default_rng(0)
    R, P, n = 3, 2, 5
    block = rng.normal(size=(R, P * n))
    C, s1, s2, autos = T.correlation_truth(block, P, n)
    x = block.reshape(R, P, n)
    ref = np.einsum("rat,rbt->rab", x, x) / n
    np.testing.assert_allclose(C.astype(float), ref, rtol=1e-14)
    np.testing.assert_allclose(s1.astype(float), ref.sum(0), rtol=1e-14)
    np.testing.assert_allclose(autos.astype(float), np.einsum("raa->ra", ref), rtol=1e-14)
    d = np.sqrt(np.einsum("raa->ra", ref))
    np.testing.assert_allclose(s2.astype(float), (ref / (d[:, :, None] * d[:, None, :])).sum(0), rtol=1e-14)
    np.testing.assert_allclose(np.diag(s2.astype(float)), R, rtol=1e-15)
    cs = T.checksum_truth(block)
    np.testing.assert_allclose(cs.astype(float), np.stack([block.sum(1), (block ** 2).sum(1)], 1), rtol=1e-14)
