"""Times the Fourier-fit kernel (k_fit_apply, fpta_batch_fit) on the GPU against the existing read-once pass over the
same block, a full-pass fpta_batch_checksums, and against the fp64 MFMA floor.

  python tools/bench_fourier_fit.py [--calls 20] [--warmup 3] [--out profiles/fourier_fit_bench.json] [--skip-c4]
                                    [--only c2_k60|c2_k200|c4_k200]

Shapes: C2 (100 pulsars x 2000 TOAs, 1024 realizations, 1.6 GB) with K = 60 (30 modes) and K = 200 (100 modes), and
the per-GPU share of C4 (1000 x 10^4 TOAs, 256 realizations, 20 GB) with K = 200; make_Mmat's eight columns
marginalised, three-band frequencies, white-noise weights, one common grid k / 15 yr. The block is white noise (the
fit's traffic and arithmetic do not depend on what the block holds). The operator of C4 is 16 GB on the host and on
the device and its long-double build takes minutes on 16 cores: --skip-c4 leaves it out.

The fit's time is the HIP-event time on the context stream (fpta_kernel_stats, FPTA_K_DENSE: the clear of the
coefficient buffer and the kernel, one entry per call). The library books no entry for the checksum pass, so that one
is host wall-clock time around fpta_batch_checksums from an idle stream (launch, kernel, the download of [R][2] sums,
synchronisation); the fit is timed that way too (fit_wall), and the ratio to the read-once pass is taken between the
two wall-clock figures. --calls launches after --warmup, medians, spread = max - min. The MFMA floor is 2 K samples /
50 TF (DESIGN.md section 5b's measured fp64 MFMA ceiling). Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from fakepta_amd import _capi  # noqa: E402
from tests import tm_reference as T  # noqa: E402

YEAR = 365.25 * 86400.0
MFMA_TF = 50.0
SHAPES = {"c2_k60": ("c2_100x2000_r1024_k60", 100, 2000, 1024, 30),
          "c2_k200": ("c2_100x2000_r1024_k200", 100, 2000, 1024, 100),
          "c4_k200": ("c4_per_gpu_1000x10000_r256_k200", 1000, 10000, 256, 100)}


def stats(v):
    v = np.array(v)
    return dict(ms_median=float(np.median(v)), ms_min=float(v.min()), ms_max=float(v.max()),
                ms_spread=float(v.max() - v.min()))


def timed(ctx, call, calls, warmup):
    """(HIP-event time booked under FPTA_K_DENSE, host wall-clock time from an idle stream) per call."""
    for _ in range(warmup):
        call()
    ctx.synchronize()
    ev, wall = [], []
    for _ in range(calls):
        ctx.reset_stats()
        t0 = time.perf_counter()
        call()
        ctx.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(ctx.kernel_stats(_capi.K_DENSE)[1])
    return stats(ev), stats(wall)


def run_shape(ctx, name, n_psr, n_toa, R, n_modes, calls, warmup):
    rng = np.random.default_rng(n_psr)
    offs = np.arange(n_psr + 1, dtype=np.int64) * n_toa
    toas = np.concatenate([np.sort(rng.uniform(0.0, 15 * YEAR, n_toa)) for _ in range(n_psr)])
    nu = np.abs(rng.choice([800.0, 1400.0, 2500.0], size=n_psr * n_toa) + rng.normal(0, 10, n_psr * n_toa))
    sigma = rng.uniform(1e-7, 1e-6, n_psr * n_toa)
    M = np.concatenate([T.mmat(toas[offs[p]:offs[p + 1]], nu[offs[p]:offs[p + 1]]) for p in range(n_psr)])
    ctx.batch_set_toas(offs, toas, nu)
    ctx.batch_set_white(sigma)
    t0 = time.time()
    rank, _ = ctx.batch_set_fit([n_modes], np.arange(1, n_modes + 1) / (15 * YEAR), [0.0], [1400.0], M=M,
                                weights=1 / sigma ** 2)
    plan_s = time.time() - t0
    K = 2 * n_modes
    ctx.set_option(_capi.OPT_FUSE_CHECKSUMS, 0)  # the checksums take the full pass over the block
    ctx.batch_synth(1, 0, R, to_host=False)
    _, ld, nr = ctx.batch_device_out()
    n_bytes = 8 * ld * nr
    res = dict(n_psr=n_psr, n_toa_per_psr=n_toa, realizations=R, K=K, kept_min=int(rank.min()),
               block_bytes=int(n_bytes), operator_bytes=int(8 * K * ld), host_plan_seconds=plan_s, calls=calls,
               warmup=warmup)
    res["fit"], res["fit_wall"] = timed(ctx, lambda: ctx.batch_fit(K, to_host=False), calls, warmup)
    _, res["checksums_full_pass_wall"] = timed(ctx, ctx.batch_checksums, calls, warmup)
    res["mfma_floor_ms"] = 2.0 * K * ld * nr / (MFMA_TF * 1e12) * 1e3
    fit, read = res["fit"]["ms_median"], res["checksums_full_pass_wall"]["ms_median"]
    res["fit_over_read_once_pass"] = res["fit_wall"]["ms_median"] / read
    res["fit_over_mfma_floor"] = fit / res["mfma_floor_ms"]
    res["bound_by"] = "mfma" if res["mfma_floor_ms"] > read else "read"
    res["fit_over_larger_bound"] = fit / res["mfma_floor_ms"] if res["bound_by"] == "mfma" \
        else res["fit_over_read_once_pass"]
    res["fit_tflops"] = 2.0 * K * ld * nr / (fit * 1e-3) / 1e12
    res["fit_block_gb_per_s"] = n_bytes / (fit * 1e-3) / 1e9
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-c4", action="store_true")
    ap.add_argument("--only", choices=sorted(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fourier_fit_bench.json"))
    a = ap.parse_args()
    if a.calls < 20:
        ap.error("--calls must be >= 20 for a measurement")
    if _capi.build_flags() & _capi.BUILD_DEBUG:
        sys.exit("bench_fourier_fit: the debug build is not for measurements")
    ctx = _capi.get_context()
    ctx.set_option(_capi.OPT_PROFILE, 1)
    keys = [a.only] if a.only else ["c2_k60", "c2_k200"] + ([] if a.skip_c4 else ["c4_k200"])
    result = {}
    for key in keys:
        name, n_psr, n_toa, R, n_modes = SHAPES[key]
        result[name] = run_shape(ctx, name, n_psr, n_toa, R, n_modes, a.calls, a.warmup)
        with open(a.out, "w") as fh:  # after every shape: the long one comes last
            json.dump(result, fh, indent=1)
            fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
