"""Times the injection of ephemeris-error Roemer delays into a resident batch block (k_roemer_block,
fpta_batch_roemer_accumulate) on the GPU against the drop-in kernel (fpta_roemer_accumulate) and a copy of the block.

  python tools/bench_roemer_batch.py [--calls 7] [--warmup 2] [--out profiles/roemer_batch_bench.json]

Shape: the C2 TOA layout (100 pulsars x 2000 TOAs), a block of R = 128 realizations, four rows per realization (the
four giant planets of the native Ephemeris, a different draw of the deviations in each): 128 x 4 x 200000 = 1.02e8
(row, sample) pairs. Kernel time is the HIP-event time fpta_kernel_stats books under FPTA_K_EPHEM, one entry per call;
the candidates alternate call by call on the same card, --calls timed calls after --warmup of each. Figures are
medians, the spread is max - min.

  element_deviations  every row has element deviations. Yardstick: fpta_roemer_accumulate with the same 512 rows on
                      the same layout, the same pairs with two orbit evaluations each where k_roemer_block makes one
                      (the base orbits come from LDS). Expectation: faster than the yardstick by more than both spreads.
  mass_only           every row has a mass deviation only: no orbit evaluation in the loop. Yardstick: a
                      device-to-device copy of the block (it reads and writes the block once, as the kernel does). No
                      bound is set: the ratio is reported.
  shared_table        one table of four element rows for every realization (k_roemer_main on zeros, then k_cw_bcast)
                      beside the drop-in call on the same four rows plus the copy.
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from fakepta.ephemeris import Ephemeris  # noqa: E402
from fakepta_amd import _capi  # noqa: E402
from tools.bench_tm_project import Hip, stats  # noqa: E402

DAY = 86400.0
N_PSR, N_TOA, R = 100, 2000, 128
PLANETS = ("jupiter", "saturn", "uranus", "neptune")


def draw_rows(rng, ephem, n_tables, elements):
    """n_tables x 4 rows: a BayesEphem-like draw of the mass error of every giant planet and, with `elements`, of its
    six orbital elements."""
    rows = []
    for _ in range(n_tables):
        for planet in PLANETS:
            dev = dict(d_mass=rng.normal(0.0, 1e-4) * ephem.planets[planet]["mass"])
            if elements:
                dev.update(d_Om=rng.normal(0, 1e-6), d_omega=rng.normal(0, 1e-6), d_inc=rng.normal(0, 1e-6),
                           d_a=rng.normal(0, 1e-7), d_e=rng.normal(0, 1e-8), d_l0=rng.normal(0, 1e-6))
            rows.append(ephem.roemer_row(planet, **dev))
    return np.array(rows)


def timed(ctx, call):
    ctx.reset_stats()
    call()
    ctx.synchronize()
    n, ms = ctx.kernel_stats(_capi.K_EPHEM)
    assert n == 1, n
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roemer_batch_bench.json"))
    a = ap.parse_args()
    if a.calls < 5 or a.warmup < 2:
        ap.error("--calls must be >= 5 and --warmup >= 2 for a measurement")
    if _capi.build_flags() & _capi.BUILD_DEBUG:
        sys.exit("bench_roemer_batch: the debug build is not for measurements")
    ctx = _capi.get_context()
    ctx.set_option(_capi.OPT_PROFILE, 1)
    rng = np.random.default_rng(2)
    ephem = Ephemeris()
    offs = np.arange(N_PSR + 1, dtype=np.int64) * N_TOA
    t0, t1 = 53000.0 * DAY, (53000.0 + 15 * 365.25) * DAY
    toas = np.concatenate([np.sort(rng.uniform(t0, t1, N_TOA)) for _ in range(N_PSR)])
    nu = np.full(N_PSR * N_TOA, 1400.0)
    v = rng.normal(size=(N_PSR, 3))
    pos = v / np.linalg.norm(v, axis=1)[:, None]
    ctx.batch_set_toas(offs, toas, nu)
    f = np.tile(np.arange(1, 11) / (t1 - t0), (N_PSR, 1))
    ctx.batch_add_signal(0, f, np.full(f.shape, 1e-7))
    ctx.batch_synth(1, 0, R, to_host=False)
    ptr, ld, nr = ctx.batch_device_out()
    assert (ld, nr) == (N_PSR * N_TOA, R)
    n_rows = len(PLANETS)
    ro = np.arange(R + 1, dtype=np.int64) * n_rows
    one = np.array([0, n_rows], dtype=np.int64)
    res = np.zeros(N_PSR * N_TOA)
    hip = Hip()
    dst = hip.malloc(8 * ld * nr)
    ea, eb = hip.event(), hip.event()
    result = dict(shape=dict(n_psr=N_PSR, n_toa_per_psr=N_TOA, realizations=R, rows_per_realization=n_rows,
                             drop_in_rows=R * n_rows, row_sample_pairs=R * n_rows * N_PSR * N_TOA,
                             block_bytes=8 * ld * nr, chunk_option=ctx.get_option(_capi.OPT_ROEMER_CHUNK)),
                  calls=a.calls, warmup=a.warmup)

    # (a) element deviations in every row against the drop-in call with the same rows
    rows = draw_rows(rng, ephem, R, True)
    block, drop = [], []
    for i in range(a.warmup + a.calls):  # alternating, call by call
        b = timed(ctx, lambda: ctx.batch_roemer_accumulate(pos, R, ro, rows))
        d = timed(ctx, lambda: ctx.roemer_accumulate(offs, toas, pos, rows, res))
        if i >= a.warmup:
            block.append(b)
            drop.append(d)
    r = dict(k_roemer_block=stats(block), drop_in_kernel_same_rows=stats(drop))
    r["ratio_block_over_drop_in"] = r["k_roemer_block"]["ms_median"] / r["drop_in_kernel_same_rows"]["ms_median"]
    gain = r["drop_in_kernel_same_rows"]["ms_median"] - r["k_roemer_block"]["ms_median"]
    r["faster_by_more_than_both_spreads"] = bool(
        gain > r["k_roemer_block"]["ms_spread"] + r["drop_in_kernel_same_rows"]["ms_spread"])
    result["element_deviations"] = r
    print("element_deviations", json.dumps(r), flush=True)

    # (b) mass-only rows against a device-to-device copy of the block
    rows = draw_rows(rng, ephem, R, False)
    block, copy = [], []
    for i in range(a.warmup + a.calls):
        b = timed(ctx, lambda: ctx.batch_roemer_accumulate(pos, R, ro, rows))
        c = hip.copy_ms(dst, ptr, 8 * ld * nr, ea, eb)
        if i >= a.warmup:
            block.append(b)
            copy.append(c)
    r = dict(k_roemer_block=stats(block), device_to_device_copy=stats(copy))
    r["ratio_block_over_copy"] = r["k_roemer_block"]["ms_median"] / r["device_to_device_copy"]["ms_median"]
    result["mass_only"] = r
    print("mass_only", json.dumps(r), flush=True)

    # (c) one table for every realization against the drop-in call on the same rows plus the copy
    rows = draw_rows(rng, ephem, 1, True)
    shared, drop, copy = [], [], []
    for i in range(a.warmup + a.calls):
        s = timed(ctx, lambda: ctx.batch_roemer_accumulate(pos, 1, one, rows))
        d = timed(ctx, lambda: ctx.roemer_accumulate(offs, toas, pos, rows, res))
        c = hip.copy_ms(dst, ptr, 8 * ld * nr, ea, eb)
        if i >= a.warmup:
            shared.append(s)
            drop.append(d)
            copy.append(c)
    hip.free(dst)
    r = dict(rows=n_rows, shared_table_call=stats(shared), drop_in_kernel_same_rows=stats(drop),
             device_to_device_copy=stats(copy))
    r["ratio_shared_over_drop_in_plus_copy"] = r["shared_table_call"]["ms_median"] / (
        r["drop_in_kernel_same_rows"]["ms_median"] + r["device_to_device_copy"]["ms_median"])
    result["shared_table"] = r
    print("shared_table", json.dumps(r), flush=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
