"""fpta_batch_synth_spectra / BatchSimulator.synth(spectra=...): every realization of a block drawn from its own
spectrum, with the Philox draws and the operation order of the fixed-spectrum block.

Bit-for-bit reference: the fixed-spectrum synth on a layout rebuilt with row r as its amplitudes (code this feature
does not touch), whose realization r must equal realization r of the tabled block. Truth: tests/spectra_reference.py
(the oracle's normals, amplitudes per realization) at the project's tolerances (counter_space.COEF_TOL for downloaded
coefficients, TOL / GRID_TOL of tests/test_gpu_grid.py for blocks). test_table_kernels_past_their_first_block runs
tests/launch_axes.py's R = 520 (three k_spectra_amp blocks, two k_spectra_scale blocks) under both.

Reference semantics of one realization: /root/reference/fakepta/fake_pta.py:372-387 (per-pulsar GP),
correlated_noises.py:153-160 (common GP), spectrum.py:12-15 (powerlaw).
"""
import numpy as np
import pytest

from oracle import fakepta_oracle as O
from tests import counter_space as S
from tests import launch_axes as AX
from tests import spectra_reference as SR
from tests.conftest import assert_parity, rel_err
from tests.test_gpu_grid import GRID_TOL, TOL

pytestmark = pytest.mark.gpu

T0, T1 = 4.4e9, 4.4e9 + 3.15e8
T = T1 - T0
N_RN, N_DM, N_GW = 30, 100, 30
RN, DM, GW = 0, 1, 2  # signal ids


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
    return ctx.options()


def _make(seed, P, factor="cholesky", n=(40, 260), n_rn=N_RN, ragged_rn=False):
    """test_gpu_next_mix._layout's layout as host arrays: P ragged pulsars over one span carrying RN, DM100 and a
    common GWB30. ragged_rn: pulsar 1 carries 7 modes fewer of RN, pulsar 2 none."""
    from fakepta_amd.batch import batch_factor
    rng = np.random.default_rng(seed)
    counts = rng.integers(n[0], n[1], size=P)
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    toas = np.concatenate([np.concatenate([[T0], np.sort(rng.uniform(T0, T1, k - 2)), [T1]]) for k in counts])
    nu = rng.choice([800.0, 1400.0, 2500.0], size=offs[-1])
    f, amp = [], []
    for nm in (n_rn, N_DM):
        f.append(np.tile(np.arange(1, nm + 1) / T, (P, 1)))
        amp.append(np.sqrt(O.powerlaw(f[-1], rng.uniform(-14.5, -13.5, (P, 1)), 3.0) / T))
    if ragged_rn:
        amp[0][1, n_rn - 7:] = 0.0
        amp[0][2, :] = 0.0
    f.append(np.arange(1, N_GW + 1) / T)
    amp.append(np.sqrt(O.powerlaw(f[-1], -14.0, 13 / 3) / T))
    v = rng.normal(size=(P, 3))
    pos = v / np.linalg.norm(v, axis=1)[:, None]
    if factor == "cholesky":
        L = batch_factor(O.orf_hd(pos))
    elif factor == "svd":
        L = O.mvn_factor(O.orf_hd(pos))
    else:
        L = batch_factor(O.orf_monopole(pos))
    return dict(P=P, offs=offs, toas=toas, nu=nu, f=f, amp=amp, L=L, idx=(0.0, 2.0, 0.0))


def _build(ctx, lay, amp=None, path=4):
    """Set the layout on the context, with amp {signal id: amplitudes} replacing the layout's; the oracle's segments."""
    amp = amp or {}
    ctx.batch_clear()
    ctx.batch_set_toas(lay["offs"], lay["toas"], lay["nu"])
    segs = []
    for s in (RN, DM, GW):
        a = np.ascontiguousarray(amp.get(s, lay["amp"][s]))
        ctx.batch_add_signal(int(s == GW), lay["f"][s], a, idx=lay["idx"][s], L=lay["L"] if s == GW else None)
        segs.append(O.Segment(int(s == GW), 2 * np.pi * lay["f"][s], a, lay["idx"][s], L=lay["L"] if s == GW else None))
    ctx.set_option(1, path)  # FPTA_OPT_SYNTH_PATH
    return segs


def _tabled(ctx, seed, real0, R, tabs, **kw):
    """tabs: {signal id: (form, per_pulsar, table)}"""
    ids = sorted(tabs)
    return ctx.batch_synth_spectra(seed, real0, R, ids, [tabs[i][0] for i in ids], [tabs[i][1] for i in ids],
                                   [tabs[i][2] for i in ids], **kw)


def _gw_rows(rng, R):
    """[R, N_GW] power-law amplitudes, log10_A over a decade and gamma over 2 .. 6."""
    f = np.arange(1, N_GW + 1) / T
    return np.sqrt(O.powerlaw(f[None, :], rng.uniform(-14.5, -13.5, (R, 1)), rng.uniform(2.0, 6.0, (R, 1))) / T)


def _picks(R):
    return (0, R // 2 - 1 + (R // 2) % 2, R - 1)  # the first, an odd one, the last


def _check_rows_bitwise(ctx, lay, got, seed, real0, R, rows, path=4, picks=None):
    """Realization r of `got` against the fixed-spectrum block of the layout rebuilt with rows {signal id: [R, ...]}[r],
    for r in picks (_picks(R) by default)."""
    for r in _picks(R) if picks is None else picks:
        _build(ctx, lay, {s: v[r] for s, v in rows.items()}, path)
        want = ctx.batch_synth(seed, real0, R)
        assert np.all(np.isfinite(got[r]))
        np.testing.assert_array_equal(got[r], want[r], err_msg=f"realization {r}")


# ----------------------------------------------------------------------------- 1. equal rows
@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("which", ["common", "all"])
def test_equal_rows_are_the_plain_block(ctx, capi, shipped, white, which):
    """Tables whose every row is the layout's amplitude: the block and the coefficient download are those of plain
    synth bit for bit, on k_grid_fused for plain blocks; with white noise and ECORR on as well."""
    lay = _make(801, 66)
    R = 256
    try:
        _build(ctx, lay)
        if white:
            rng = np.random.default_rng(5)
            n = int(lay["offs"][-1])
            blocks = [np.arange(i, min(i + 2, n)) for i in range(0, n - 1, 2)]
            ctx.batch_set_white(rng.uniform(0.5e-7, 2e-7, n), blocks, rng.uniform(0.5e-7, 1.5e-7, len(blocks)))
        tabs = {GW: (0, 0, np.tile(lay["amp"][GW], (R, 1)))}
        if which == "all":
            tabs[RN] = (0, 1, np.tile(lay["amp"][RN], (R, 1, 1)))
            tabs[DM] = (0, 1, np.tile(lay["amp"][DM], (R, 1, 1)))
        for coeffs in (False, True):
            want = ctx.batch_synth(3, 512, R, coeffs=coeffs)
            k0 = ctx.batch_grid_info()["interp_kernel"]
            got = _tabled(ctx, 3, 512, R, tabs, coeffs=coeffs)
            k1 = ctx.batch_grid_info()["interp_kernel"]
            if not white and not coeffs:  # (a coefficient download takes the block off the fused kernel)
                assert k0.startswith("k_grid_fused<") and k1.startswith("k_grid_fused<"), (k0, k1)
            if coeffs:
                np.testing.assert_array_equal(got[1], want[1])
                got, want = got[0], want[0]
            assert np.all(np.isfinite(got))
            np.testing.assert_array_equal(got, want)
    finally:
        ctx.batch_set_white()
        ctx.batch_clear()
        ctx.set_options(shipped)


# ----------------------------------------------------------------------------- 2. distinct rows
@pytest.mark.parametrize("path,fused,R", [(4, 1, 256), (4, 0, 256), (3, 1, 256), (2, 1, 256), (1, 1, 5)])
def test_common_rows_bitwise(ctx, capi, shipped, path, fused, R):
    lay = _make(811, 66)
    rows = _gw_rows(np.random.default_rng(812), R)
    try:
        _build(ctx, lay, path=path)
        ctx.set_option(capi.OPT_INTERP_FUSED, shipped[capi.OPT_INTERP_FUSED] if fused else 0)
        got = _tabled(ctx, 11, 1001, R, {GW: (0, 0, rows)})
        assert ctx.batch_grid_info()["last_path"] == path
        _check_rows_bitwise(ctx, lay, got, 11, 1001, R, {GW: rows}, path)
    finally:
        ctx.batch_clear()
        ctx.set_options(shipped)


def test_per_pulsar_rows(ctx, capi, shipped):
    """[R, P, N] on red noise with an odd N, a pulsar with fewer modes and one without the signal: three realizations
    bit for bit, the whole download and block against the reference."""
    P, R, n_rn = 66, 256, 29
    lay = _make(821, P, n_rn=n_rn, ragged_rn=True)
    rng = np.random.default_rng(822)
    rows = np.sqrt(O.powerlaw(lay["f"][RN][None], rng.uniform(-14.5, -13.0, (R, P, 1)), rng.uniform(1.0, 5.0, (R, P, 1))) / T)
    rows = np.where(lay["amp"][RN][None] == 0.0, 0.0, rows)
    try:
        segs = _build(ctx, lay)
        got, co = _tabled(ctx, 13, 77, R, {RN: (0, 1, rows)}, coeffs=True)
        want_co = SR.coefficients(segs, P, 13, 77, R, {RN: rows})
        S.check_coeffs(co, SR.download(want_co, P, R))
        assert np.all(co[2, :2 * (n_rn + 1)] == 0.0) and np.all(co[1, 2 * (n_rn - 7):2 * (n_rn + 1)] == 0.0)
        assert np.all(co[:, 2 * n_rn:2 * (n_rn + 1)] == 0.0)  # the padding mode
        want = SR.synth(lay["offs"], lay["toas"], lay["nu"], segs, 13, 77, R, {RN: rows})
        got2 = _tabled(ctx, 13, 77, R, {RN: (0, 1, rows)})  # without the download: the block's own route
        for g in (got, got2):
            assert rel_err(g, want) <= GRID_TOL
            assert_parity(g, want, TOL)
        _check_rows_bitwise(ctx, lay, got2, 13, 77, R, {RN: rows})
    finally:
        ctx.batch_clear()
        ctx.set_options(shipped)


def _first_signal(co, nm, rows):
    """[len(rows), P, nm, 2] (cos, sin) of the first signal's nm modes in a coefficient download [P][K][R]."""
    P = co.shape[0]
    return np.transpose(co[:, :2 * nm][:, :, list(rows)].reshape(P, nm, 2, len(rows)), (3, 0, 1, 2))


def _device_amplitudes(z, co, radius=4):
    """The amplitudes the device evaluated from power-law parameters agree with numpy's to COEF_TOL, not to the bit
    (the device's pow and numpy's differ by tens of ulp), so a fixed-spectrum layout that is to give the same bits has
    to carry the device's own. They are recovered from the tabled block's coefficients co [..., 2] = fl(a z) and the
    unit-amplitude draws z [..., 2]: fl(co / z) is within two roundings of a, and per entry the neighbour of it within
    `radius` ulp is taken whose products with both draws are the coefficients bit for bit (0 where the draws are 0:
    the layout has no amplitude there). A layout that carries them stores those coefficients."""
    live = z[..., 0] != 0.0
    est = np.where(live, co[..., 0] / np.where(live, z[..., 0], 1.0), 0.0)
    out, found = est.copy(), np.zeros(est.shape, dtype=bool)
    up = dn = est
    for _ in range(radius + 1):
        for cand in (up, dn):
            ok = ~found & np.all(cand[..., None] * z == co, axis=-1)
            out[ok] = cand[ok]
            found |= ok
        up, dn = np.nextafter(up, np.inf), np.nextafter(dn, -np.inf)
    assert np.all(found), f"{int(np.sum(~found))} amplitudes do not reproduce their coefficients"
    return out


@pytest.mark.parametrize("path", AX.SPECTRA["paths"])
def test_table_kernels_past_their_first_block(ctx, capi, shipped, path):
    """R = 520 from an odd real0 (R_pad = 640: three k_spectra_amp blocks, two k_spectra_scale blocks, the second a
    quarter full) with all three signals tabled: red noise of 3 modes as per-pulsar power-law parameters (the padding
    mode takes k_spectra_amp's k < N branch), DM as an amplitude row the pulsars share, the common signal as amplitude
    rows. The realizations at the blocks' edges are the rebuilt fixed-spectrum layout's bit for bit, and the downloaded
    coefficients the reference's."""
    from fakepta import spectrum
    c = AX.SPECTRA
    P, R, real0, n_rn, picks = c["P"], c["R"], c["real0"], c["n_rn"], list(c["picks"])
    lay = _make(881, P, n=c["n"], n_rn=n_rn, ragged_rn=True)
    rng = np.random.default_rng(882)
    rn = np.stack([rng.uniform(-14.5, -13.0, (R, P)), rng.uniform(1.0, 5.0, (R, P))], axis=2)
    dm = np.sqrt(O.powerlaw(lay["f"][DM][:1], rng.uniform(-14.5, -13.5, (R, 1)), rng.uniform(1.0, 4.0, (R, 1))) / T)
    gw = _gw_rows(rng, R)
    df_rn = np.stack([O.delta_f(f) for f in lay["f"][RN]])
    a_rn = np.sqrt(spectrum.powerlaw(lay["f"][RN][None], rn[..., :1], rn[..., 1:]) * df_rn)
    a_rn = np.where(lay["amp"][RN][None] == 0.0, 0.0, a_rn)
    tabs = {RN: (1, 1, rn), DM: (0, 0, dm), GW: (0, 0, gw)}
    try:
        segs = _build(ctx, lay, path=path)
        got, co = _tabled(ctx, 41, real0, R, tabs, coeffs=True)
        assert ctx.batch_grid_info()["last_path"] == path
        want = SR.download(SR.coefficients(segs, P, 41, real0, R, {RN: a_rn, DM: dm, GW: gw}), P, R)
        S.check_coeffs(co[:, :, picks], want[:, :, picks])
        S.check_coeffs(co, want)  # and every realization in between
        assert np.all(co[1:3, :2 * (n_rn + 1)] == 0.0) and np.all(co[:, 2 * n_rn:2 * (n_rn + 1)] == 0.0)
        assert np.all(co[0, :2 * n_rn] != 0.0)
        got2 = _tabled(ctx, 41, real0, R, tabs)  # without the download: the block's own route
        assert ctx.batch_grid_info()["last_path"] == path and np.all(np.isfinite(got)) and np.all(np.isfinite(got2))
        # the draws, from the layout with unit red-noise amplitudes (1 z = z), then the device's own amplitudes
        _build(ctx, lay, {RN: (lay["amp"][RN] != 0.0).astype(np.float64)}, path)
        _, unit = ctx.batch_synth(41, real0, R, coeffs=True)
        a_dev = _device_amplitudes(_first_signal(unit, n_rn + 1, picks)[:, :, :n_rn],
                                   _first_signal(co, n_rn + 1, picks)[:, :, :n_rn])
        assert np.all((a_dev == 0.0) == (a_rn[picks] == 0.0))
        far = np.abs(a_dev - a_rn[picks]) / np.spacing(np.maximum(a_rn[picks], 1e-300))
        print(f"path {path}: the device's power-law amplitudes differ from numpy's by up to {far.max():.0f} ulp")
        rows_rn = a_rn.copy()
        rows_rn[picks] = a_dev
        rows = {RN: rows_rn, DM: np.broadcast_to(dm[:, None, :], (R, P, N_DM)), GW: gw}
        _check_rows_bitwise(ctx, lay, got2, 41, real0, R, rows, path, picks=picks)
    finally:
        ctx.batch_clear()
        ctx.set_options(shipped)


# ----------------------------------------------------------------------------- 3. mix routes
@pytest.mark.parametrize("P,factor,R", [(5, "cholesky", 100), (66, "cholesky", 256), (66, "svd", 100),
                                        (66, "monopole", 256)])
def test_mix_routes_bitwise(ctx, capi, shipped, P, factor, R):
    """k_mix (P = 5), and at P = 66 the Cholesky, full and rank-1 factors, each with FPTA_OPT_MIX_MFMA and
    FPTA_OPT_GEN_MIX at every value the library accepts; R = 100 leaves rows past R in the 128-realization padding."""
    lay = _make(831 + P, P, factor)
    rows = _gw_rows(np.random.default_rng(832), R)
    ran = 0
    try:
        for key, values in ((capi.OPT_MIX_MFMA, (0, 1)), (capi.OPT_GEN_MIX, (0, 1, 2, 3))):
            for v in values:
                _build(ctx, lay)
                ctx.set_options(shipped)
                ctx.set_option(1, 4)
                try:
                    ctx.set_option(key, v)
                except capi.FptaError:
                    continue  # a value of variant builds only
                got = _tabled(ctx, 17, 300, R, {GW: (0, 0, rows)})
                _check_rows_bitwise(ctx, lay, got, 17, 300, R, {GW: rows})
                ran += 1
        assert ran >= 3  # MIX_MFMA 0 and 1, GEN_MIX 2
    finally:
        ctx.batch_clear()
        ctx.set_options(shipped)


# ----------------------------------------------------------------------------- 4. next-mix sequence
def test_next_mix_sequence(ctx, capi, shipped):
    """plain, plain, plain, tabled, plain, tabled, tabled, plain at consecutive real0: identical with
    FPTA_OPT_FUSED_NEXT_MIX on and off, no tabled block takes a precomputed mix, the third plain block does."""
    lay = _make(841, 66)
    R = 256
    rows = _gw_rows(np.random.default_rng(842), R)
    rn_rows = np.tile(lay["amp"][RN], (R, 1, 1)) * np.random.default_rng(843).uniform(0.5, 2.0, (R, 1, 1))
    kinds = "pppTpTTp"
    fetch = (True, False, True, True, False, False, True, True)
    try:
        _build(ctx, lay)

        def seq(on, tabs):
            ctx.set_option(capi.OPT_FUSED_NEXT_MIX, on)
            outs, used = [], []
            for i, (k, dl) in enumerate(zip(kinds, fetch)):
                if k == "p":
                    out = ctx.batch_synth(19, i * R, R, to_host=dl)
                else:
                    out = _tabled(ctx, 19, i * R, R, tabs, to_host=dl)
                gi = ctx.batch_grid_info()
                assert gi["interp_kernel"].startswith("k_grid_fused<"), gi["interp_kernel"]
                outs.append(out if dl else None)
                used.append(bool(gi["next_mix_used"]))
            ctx.synchronize()
            return outs, used

        for tabs in ({GW: (0, 0, rows)}, {RN: (0, 1, rn_rows)}):
            ref, used0 = seq(0, tabs)
            got, used1 = seq(1, tabs)
            assert not any(used0)
            for i, (x, y) in enumerate(zip(ref, got)):
                if x is not None:
                    assert np.all(np.isfinite(y))
                    np.testing.assert_array_equal(y, x, err_msg=f"block {i} ({kinds[i]})")
            assert not any(u for u, k in zip(used1, kinds) if k == "T"), used1
            assert used1[2], used1
        # the tabled blocks of the sequence are right, not only equal: block 3 against the rebuilt layout
        ctx.set_option(capi.OPT_FUSED_NEXT_MIX, 1)
        _build(ctx, lay)
        for i in range(3):
            ctx.batch_synth(19, i * R, R, to_host=False)
        got = _tabled(ctx, 19, 3 * R, R, {GW: (0, 0, rows)})
        _check_rows_bitwise(ctx, lay, got, 19, 3 * R, R, {GW: rows})
    finally:
        ctx.batch_clear()
        ctx.set_options(shipped)


# ----------------------------------------------------------------------------- 5. batching
@pytest.mark.parametrize("real0", [4321, S.windows(19, 18)[0][0] - 60])
def test_batch_split_invariance(ctx, capi, shipped, real0):
    """R = 100 from an odd first realization in one call and as 37 + 63 with the tables sliced; the second window
    straddles bit 31 of the realization index."""
    lay = _make(851, 66)
    R = 100
    rng = np.random.default_rng(852)
    rows = _gw_rows(rng, R)
    rn = np.tile(lay["amp"][RN], (R, 1, 1)) * rng.uniform(0.5, 2.0, (R, lay["P"], 1))
    assert real0 % 2 == 1
    try:
        _build(ctx, lay)
        ctx.set_option(capi.OPT_MFMA_MIN_REAL, 1)
        one = _tabled(ctx, S.S_HI, real0, R, {GW: (0, 0, rows), RN: (0, 1, rn)})
        a = _tabled(ctx, S.S_HI, real0, 37, {GW: (0, 0, rows[:37]), RN: (0, 1, rn[:37])})
        b = _tabled(ctx, S.S_HI, real0 + 37, 63, {GW: (0, 0, rows[37:]), RN: (0, 1, rn[37:])})
        np.testing.assert_array_equal(np.concatenate([a, b]), one)
    finally:
        ctx.batch_clear()
        ctx.set_options(shipped)


# ----------------------------------------------------------------------------- 6. power-law form
def test_powerlaw_form(ctx, capi, shipped):
    """[R, 2] on the common signal and [R, P, 2] on red noise, evaluated on the device: the coefficients are the
    reference's with numpy's sqrt(spectrum.powerlaw * df), exact zeros where the layout's amplitude is 0."""
    from fakepta import spectrum
    P, R, n_rn = 12, 40, 29
    lay = _make(861, P, n_rn=n_rn, ragged_rn=True)
    rng = np.random.default_rng(862)
    gw = np.stack([rng.uniform(-15.0, -13.0, R), rng.uniform(2.0, 6.0, R)], axis=1)
    gw[0], gw[1], gw[2] = (-14.0, 0.0), (-14.0, 7.0), (-18.0, 13 / 3)
    rn = np.stack([rng.uniform(-15.0, -13.0, (R, P)), rng.uniform(1.0, 6.0, (R, P))], axis=2)
    rn[3, 0], rn[3, 1], rn[4, 5] = (-13.5, 0.0), (-14.5, 7.0), (-18.0, 3.0)
    a_gw = np.sqrt(spectrum.powerlaw(lay["f"][GW][None, :], gw[:, :1], gw[:, 1:]) * O.delta_f(lay["f"][GW]))
    df_rn = np.stack([O.delta_f(f) for f in lay["f"][RN]])
    a_rn = np.sqrt(spectrum.powerlaw(lay["f"][RN][None], rn[..., :1], rn[..., 1:]) * df_rn)
    a_rn = np.where(lay["amp"][RN][None] == 0.0, 0.0, a_rn)
    try:
        segs = _build(ctx, lay)
        got, co = _tabled(ctx, 23, 9, R, {GW: (1, 0, gw), RN: (1, 1, rn)}, coeffs=True)
        want = SR.coefficients(segs, P, 23, 9, R, {GW: a_gw, RN: a_rn})
        S.check_coeffs(co, SR.download(want, P, R))
        assert np.all(co[2, :2 * (n_rn + 1)] == 0.0) and np.all(co[1, 2 * (n_rn - 7):2 * (n_rn + 1)] == 0.0)
        assert np.all(co[:, 2 * n_rn:2 * (n_rn + 1)] == 0.0)
        assert np.all(co[0, :2 * n_rn] != 0.0)
        block = SR.synth(lay["offs"], lay["toas"], lay["nu"], segs, 23, 9, R, {GW: a_gw, RN: a_rn})
        assert_parity(got, block, TOL)
    finally:
        ctx.batch_clear()
        ctx.set_options(shipped)


def test_shared_rows_on_a_per_pulsar_signal(ctx, capi, shipped):
    """[R, N] amplitudes and [R, 2] parameters on red noise: every pulsar takes the row, except where the layout's
    amplitude is 0 (fewer modes, no signal), which stays 0."""
    from fakepta import spectrum
    P, R, n_rn = 12, 40, 29
    lay = _make(865, P, n_rn=n_rn, ragged_rn=True)
    rng = np.random.default_rng(866)
    rows = rng.uniform(1e-8, 1e-6, (R, n_rn))
    par = np.stack([rng.uniform(-15.0, -13.0, R), rng.uniform(1.0, 6.0, R)], axis=1)
    df = np.stack([O.delta_f(f) for f in lay["f"][RN]])
    a_par = np.sqrt(spectrum.powerlaw(lay["f"][RN][None], par[:, None, :1], par[:, None, 1:]) * df)
    a_par = np.where(lay["amp"][RN][None] == 0.0, 0.0, a_par)
    try:
        segs = _build(ctx, lay)
        for tab, amps in (((0, 0, rows), rows), ((1, 0, par), a_par)):
            got, co = _tabled(ctx, 27, 3, R, {RN: tab}, coeffs=True)
            want = SR.coefficients(segs, P, 27, 3, R, {RN: amps})
            S.check_coeffs(co, SR.download(want, P, R))
            assert np.all(co[2, :2 * (n_rn + 1)] == 0.0) and np.all(co[1, 2 * (n_rn - 7):2 * (n_rn + 1)] == 0.0)
            assert np.all(co[0, :2 * n_rn] != 0.0)
            assert_parity(got, SR.synth(lay["offs"], lay["toas"], lay["nu"], segs, 27, 3, R, {RN: amps}), TOL)
    finally:
        ctx.batch_clear()
        ctx.set_options(shipped)


# ----------------------------------------------------------------------------- 7. errors
def test_errors_leave_the_block(ctx, capi, shipped):
    P, R = 6, 8
    lay = _make(871, P, n=(40, 80), n_rn=29, ragged_rn=True)
    ok_gw = np.tile(lay["amp"][GW], (R, 1))
    ok_rn = np.tile(lay["amp"][RN], (R, 1, 1))

    def bad(tab, r, *at, value):
        tab = tab.copy()
        tab[(r,) + at] = value
        return tab
    cases = [
        ({GW: (0, 0, bad(ok_gw, 3, 4, value=np.nan))}, ("signal 2", "realization 3", "mode 4", "non-finite")),
        ({GW: (0, 0, bad(ok_gw, 7, 0, value=-1e-9))}, ("signal 2", "realization 7", "mode 0", "negative")),
        ({RN: (0, 1, bad(ok_rn, 2, 5, 1, value=np.inf))}, ("signal 0", "realization 2", "pulsar 5", "mode 1", "non-finite")),
        ({RN: (0, 1, bad(ok_rn, 1, 2, 3, value=1e-8))}, ("signal 0", "realization 1", "pulsar 2", "mode 3", "layout's is 0")),
        ({RN: (0, 1, bad(ok_rn, 1, 1, 28, value=1e-8))}, ("signal 0", "pulsar 1", "mode 28", "layout's is 0")),
        ({GW: (1, 0, bad(np.tile([-14.0, 3.0], (R, 1)), 5, 1, value=np.nan))}, ("signal 2", "realization 5", "gamma")),
        ({RN: (1, 1, bad(np.tile([-14.0, 3.0], (R, P, 1)), 6, 4, 0, value=np.inf))},
         ("signal 0", "realization 6", "pulsar 4", "log10_A")),
        ({7: (0, 0, ok_gw)}, ("signal 7", "unknown")),
        ({GW: (0, 1, np.tile(ok_gw[:, None, :], (1, P, 1)))}, ("signal 2", "per-pulsar", "common")),
        ({GW: (0, 0, ok_gw[:5])}, ("signal 2", "5 table rows", f"{R} realizations")),
    ]
    try:
        _build(ctx, lay)
        ctx.batch_synth(29, 10, R, to_host=False)
        before = ctx.batch_checksums()
        for tabs, words in cases:
            with pytest.raises(capi.FptaError) as e:
                _tabled(ctx, 29, 50, R, tabs)
            assert all(w in str(e.value) for w in words), (str(e.value), words)
            np.testing.assert_array_equal(ctx.batch_checksums(), before)
        with pytest.raises(capi.FptaError) as e:  # a repeated id
            ctx.batch_synth_spectra(29, 50, R, [GW, GW], [0, 0], [0, 0], [ok_gw, ok_gw])
        assert "signal 2" in str(e.value) and "more than one" in str(e.value)
        np.testing.assert_array_equal(ctx.batch_checksums(), before)
        # last_blk untouched too: the resident block is still the one of real0 = 10
        np.testing.assert_array_equal(ctx.batch_download(0, R), ctx.batch_synth(29, 10, R))
    finally:
        ctx.batch_clear()
        ctx.set_options(shipped)


# ----------------------------------------------------------------------------- 8. surface
@pytest.fixture(scope="module")
def sim(ctx):
    from fakepta import correlated_noises as cn
    from fakepta import fake_pta as fp
    from fakepta_amd.batch import BatchSimulator
    np.random.seed(31)
    psrs = fp.make_fake_array(npsrs=8, Tobs=10, ntoas=120, gaps=False, toaerr=1e-7, backends="NUPPI.1400",
                              custom_model={"RN": 10, "DM": 12, "Sv": None})
    cn.add_common_correlated_noise(psrs, orf="hd", components=6, log10_A=-14.0, gamma=13 / 3)
    s = BatchSimulator(psrs, white=True, ctx=ctx)
    yield s
    ctx.batch_clear()


def test_synth_errors_by_name(sim, ctx):
    R = 6
    sim.synth(R, seed=1, to_host=False)
    before = sim.checksums()
    gw = [s for s in sim.segments if s["kind"] == 1][0]
    N = len(gw["f"])
    for spectra, words in (
            ({gw["name"]: dict(amp=np.full((R, N), -1.0))}, (gw["name"], "realization 0", "mode 0", "negative")),
            ({gw["name"]: dict(log10_A=np.r_[np.full(R - 1, -14.0), np.nan], gamma=3.0)}, ("realization 5", "log10_A")),
            ({"nope": dict(log10_A=-14.0, gamma=3.0)}, ("nope", "unknown")),
            ({gw["name"]: dict(log10_A=np.full((R, 8), -14.0), gamma=3.0)}, ("per-pulsar", "common")),
            ({gw["name"]: dict(amp=np.ones((R + 1, N)))}, (f"{R + 1} rows", f"{R} realizations")),
            ({gw["name"]: dict(amp=np.ones((R, N))), gw["id"]: dict(amp=np.ones((R, N)))}, ("more than one",))):
        with pytest.raises(ValueError) as e:
            sim.synth(R, seed=1, spectra=spectra)
        assert all(w in str(e.value) for w in words), (str(e.value), words)
        np.testing.assert_array_equal(sim.checksums(), before)


def test_sharded_and_consumers(sim, ctx, capi, shipped):
    from fakepta_amd.batch import simulate_sharded
    from fakepta_amd.spectra import slice_spectra
    n, rng = 300, np.random.default_rng(33)
    gw = [s for s in sim.segments if s["kind"] == 1][0]["name"]
    spectra = {gw: dict(log10_A=rng.uniform(-14.5, -13.5, n), gamma=rng.uniform(2.0, 6.0, n)),
               "red_noise": dict(log10_A=rng.uniform(-14.5, -13.5, (n, 8)), gamma=3.0)}
    try:
        sim.set_timing_model()
        sim.set_likelihood_grid(log10_A=np.linspace(-15, -13, 5), gamma=np.linspace(2, 6, 5))
        ctx.set_option(capi.OPT_MFMA_MIN_REAL, 1)
        block = sim.synth(n, seed=37, real0=1, spectra=spectra)
        sums = sim.checksums()
        for r in range(n):
            S.check_sums(sums[r], block[r])
        seen = []

        def same(got):  # the checksums of the one block, at check_sums' bounds (the batches' sums may come from the
            for r in range(n):  # interpolation's partials, in another order)
                S.check_sums(got[r], block[r])

        def on_batch(s, first, m):
            seen.append((first, m, s.likelihood_grid(posterior=True)["posterior"].shape[-1]))
        got = simulate_sharded(sim, n, seed=37, real0=1, batch=128, spectra=spectra, on_batch=on_batch)
        same(got)
        assert seen == [(1, 128, 128), (129, 128, 128), (257, 44, 44)]
        got = simulate_sharded(sim, n, seed=37, real0=1, batch=128, on_batch=lambda *a: None,
                               spectra=lambda first, m: slice_spectra(spectra, first - 1, m))
        same(got)
        got2 = simulate_sharded(sim, n, seed=37, real0=1, batch=128, spectra=spectra)  # no consumer: still the loop
        np.testing.assert_array_equal(got2, got)
        # project() and likelihood_grid() on a tabled block
        sim.synth(64, seed=37, real0=1, to_host=False, spectra=slice_spectra(spectra, 0, 64))
        lg = sim.likelihood_grid()
        assert np.all(np.isfinite(lg["dlnL"])) and lg["dlnL"].shape[-1] == 64
        sim.project()
        assert np.all(np.isfinite(sim.checksums()))
    finally:
        ctx.set_options(shipped)
