"""Times the ephemeris kernels (fpta_ephem_orbits, fpta_roemer_accumulate) on the GPU.

  python tools/bench_ephem.py [--calls 12] [--warmup 3] [--out profiles/ephem_bench.json] [--skip-c4]

(a) planetssb of the eight planets for the C2 layout (100 pulsars x 2000 TOAs) and the C4 layout (1000 x 10^4), all
    TOAs in one call: what the Pulsar constructors of such an array ask for
(b) Roemer delays summed into the residuals of the same layouts, 12 rows (four of them mass-only: one orbit each) and
    1024 rows (every element deviated: two orbits each)

Kernel time is the HIP-event time of the call's kernel on the context stream (fpta_kernel_stats, FPTA_K_EPHEM); call
time is the host clock around the whole call (validation, uploads, kernel, download, synchronise). Every case is
warmed up, then timed --calls times; the figures are medians, the spread is max - min over the timed calls. The
baseline is the vectorised fp64 numpy model of tests/ephem_reference.py on this host, timed on a subset of the TOAs
and scaled. Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from fakepta.ephemeris import Ephemeris  # noqa: E402
from fakepta_amd import _capi, ephem  # noqa: E402
from tests import ephem_reference as R  # noqa: E402


def make_layout(rng, n_psr, n_toa):
    toas = np.concatenate([np.sort(rng.uniform(53000.0, 58500.0, n_toa)) for _ in range(n_psr)]) * 86400.0
    offs = np.arange(n_psr + 1, dtype=np.int64) * n_toa
    th, ph = np.arccos(rng.uniform(-1, 1, n_psr)), rng.uniform(0, 2 * np.pi, n_psr)
    pos = np.stack([np.cos(ph) * np.sin(th), np.sin(ph) * np.sin(th), np.cos(th)], axis=1)
    return dict(offs=offs, toas=toas, pos=pos)


def make_rows(rng, eph, n_row):
    """The first four rows deviate a mass only; every other row deviates all six elements of a planet drawn in turn."""
    rows = []
    for r in range(n_row):
        planet = eph.planet_names[r % len(eph.planet_names)]
        mass = eph.planets[planet]["mass"]
        if r < 4:
            rows.append(eph.roemer_row(planet, d_mass=1e-4 * mass))
        else:
            d = rng.normal(size=7)
            rows.append(eph.roemer_row(planet, d_mass=1e-5 * mass * d[0], d_Om=1e-6 * d[1], d_omega=1e-6 * d[2],
                                       d_inc=1e-6 * d[3], d_a=1e-7 * d[4], d_e=1e-8 * d[5], d_l0=1e-6 * d[6]))
    return np.array(rows)


def summarise(ker, wall, orbit_evals, calls):
    k = np.array(ker)
    return dict(kernel_ms_median=float(np.median(k)), kernel_ms_min=float(k.min()), kernel_ms_max=float(k.max()),
                kernel_ms_spread=float(k.max() - k.min()), call_ms_median=float(np.median(wall)),
                call_ms_spread=float(np.max(wall) - np.min(wall)), orbit_evaluations=int(orbit_evals),
                orbit_evaluations_per_s=orbit_evals / (np.median(k) * 1e-3), calls=calls)


def measure(ctx, call, orbit_evals, calls, warmup):
    for _ in range(warmup):
        call()
    ker, wall = [], []
    for _ in range(calls):
        ctx.reset_stats()
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        n, ms = ctx.kernel_stats(_capi.K_EPHEM)
        assert n == 1
        ker.append(ms)
    return summarise(ker, wall, orbit_evals, calls)


def numpy_orbit_seconds(toas, bodies, n_sub):
    """Seconds the fp64 numpy model takes for every TOA and body, scaled from the first n_sub TOAs."""
    sub = toas[:n_sub]
    resolved = R.resolve_bodies(bodies)
    t0 = time.perf_counter()
    for b in resolved:
        R.orbit_numpy(sub, b)
    return (time.perf_counter() - t0) * len(toas) / len(sub)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--numpy-toas", type=int, default=20000)
    ap.add_argument("--skip-c4", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ephem_bench.json"))
    a = ap.parse_args()
    if a.calls < 10:
        ap.error("--calls must be >= 10")
    if _capi.build_flags() & _capi.BUILD_DEBUG:
        sys.exit("bench_ephem: the debug build is not for measurements")
    ctx = _capi.get_context()
    ctx.set_option(_capi.OPT_PROFILE, 1)
    rng = np.random.default_rng(12)
    eph = Ephemeris()
    bodies = ephem.body_table(eph.planets)
    rows = {12: make_rows(rng, eph, 12), 1024: make_rows(rng, eph, 1024)}
    result = {"calls": a.calls, "warmup": a.warmup}
    layouts = [("c2_100x2000", 100, 2000)] + ([] if a.skip_c4 else [("c4_1000x10000", 1000, 10000)])
    for name, n_psr, n_toa in layouts:
        lay = make_layout(rng, n_psr, n_toa)
        n = len(lay["toas"])
        res = measure(ctx, lambda: ctx.ephem_orbits(lay["toas"], bodies), n * len(bodies), a.calls, a.warmup)
        numpy_s = numpy_orbit_seconds(lay["toas"], bodies, a.numpy_toas)
        res["numpy_s_scaled"] = numpy_s
        res["numpy_orbit_evaluations_per_s"] = n * len(bodies) / numpy_s
        result[f"planetssb_{name}_8bodies"] = res
        print(name, "planetssb", json.dumps(res), flush=True)
        for n_row, tab in rows.items():
            out = np.zeros(n)
            evals = n * int(np.sum(np.where(np.any(tab[:, 15:21] != 0, axis=1), 2, 1)))
            res = measure(ctx, lambda: ctx.roemer_accumulate(lay["offs"], lay["toas"], lay["pos"], tab, out), evals,
                          a.calls, a.warmup)
            res["numpy_s_scaled"] = numpy_s / (n * len(bodies)) * evals
            result[f"roemer_{name}_{n_row}rows"] = res
            print(name, "roemer", n_row, json.dumps(res), flush=True)
    ctx.set_option(_capi.OPT_PROFILE, 0)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
