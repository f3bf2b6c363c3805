"""Times fpta_orf_anisotropic (the anisotropic ORF as a weighted antenna-pattern Gram matrix on fp64 MFMA) on the GPU.

  python tools/bench_orf.py [--calls 12] [--warmup 3] [--out profiles/orf_bench.json]

  A  P = 100, nside 32, one map     the drop-in call (latency)
  B  P = 1000, nside 64, one map
  C  P = 100, nside 32, 81 maps     one ORF per map of a spherical-harmonic basis (l <= 8)

Kernel time is the HIP-event time of the call's kernels on the context stream (fpta_kernel_stats, FPTA_K_DENSE:
k_orf_aniso + k_orf_reduce of every launch batch); call time is the host clock around the whole call (validation,
uploads, kernels, download, synchronise). Every shape is warmed up, then timed --calls times: median, min and max.
FLOP/s counts the Gram matrix alone, 2 P^2 (2 npix) per map over the kernel time, against the 50 TF fp64 MFMA ceiling
of DESIGN.md section 5b; the kernels compute the lower-triangle tiles only (about half of it) and the ~30 flops of
geometry per (pulsar, pixel) are not counted. The numpy time is the parent's body
(fp * h) @ fp.T + (fc * h) @ fc.T on the same inputs (antenna patterns made once per shape and timed apart; the pixel
centres from fpta_healpix_pix2ang_ring), on this host at the BLAS thread count in force. No ratio is a condition: the
figures are recorded as measured. --numpy-repeats 0 skips the numpy side (A/B runs of a variant library loaded through
FAKEPTA_AMD_LIB). Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from fakepta.correlated_noises import create_gw_antenna_pattern  # noqa: E402
from fakepta_amd import _capi  # noqa: E402

MFMA_CEILING = 50e12  # fp64 MFMA FLOP/s
SHAPES = (("A_p100_nside32_1map", 100, 32, 1), ("B_p1000_nside64_1map", 1000, 64, 1),
          ("C_p100_nside32_81maps", 100, 32, 81))


def numpy_body(pos, nside, maps, repeats):
    """(seconds to make the antenna patterns, median seconds of the Gram body over all maps, the ORFs)."""
    theta, phi = _capi.pix2ang_ring(nside)
    npix = len(theta)
    t0 = time.perf_counter()
    pats = [create_gw_antenna_pattern(p, theta, phi) for p in pos]
    fp, fc = np.array([a for a, _, _ in pats]), np.array([b for _, b, _ in pats])
    t_pat = time.perf_counter() - t0
    times, out = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = []
        for h in maps:
            orf = 1.5 * ((fp * h) @ fp.T + (fc * h) @ fc.T) / npix
            orf[np.diag_indices_from(orf)] *= 2.0
            out.append(orf)
        times.append(time.perf_counter() - t0)
    return t_pat, float(np.median(times)), np.array(out)


def measure(ctx, pos, nside, maps, calls, warmup):
    out = np.empty((len(maps), len(pos), len(pos)))
    for _ in range(warmup):
        ctx.orf_anisotropic(pos, nside, maps, out=out)
    ker, wall = [], []
    for _ in range(calls):
        ctx.reset_stats()
        t0 = time.perf_counter()
        ctx.orf_anisotropic(pos, nside, maps, out=out)
        wall.append((time.perf_counter() - t0) * 1e3)
        n, ms = ctx.kernel_stats(_capi.K_DENSE)
        assert n >= 1
        ker.append(ms)
    return np.array(ker), np.array(wall), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--numpy-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orf_bench.json"))
    a = ap.parse_args()
    if a.calls < 10:
        ap.error("--calls must be >= 10")
    if _capi.build_flags() & _capi.BUILD_DEBUG:
        sys.exit("bench_orf: the debug build is not for measurements")
    ctx = _capi.Context(0)
    ctx.set_option(_capi.OPT_PROFILE, 1)
    rng = np.random.default_rng(12)
    result = {"calls": a.calls, "warmup": a.warmup, "mfma_ceiling_flops": MFMA_CEILING,
              "blas_threads_env": os.environ.get("OMP_NUM_THREADS")}
    for name, n_psr, nside, n_map in SHAPES:
        v = rng.normal(size=(n_psr, 3))
        pos = v / np.linalg.norm(v, axis=1)[:, None]
        maps = rng.uniform(0.2, 2.0, size=(n_map, 12 * nside * nside))
        ker, wall, got = measure(ctx, pos, nside, maps, a.calls, a.warmup)
        if a.numpy_repeats > 0:
            t_pat, t_body, want = numpy_body(pos, nside, maps, a.numpy_repeats)
        else:  # a variant library timed against another: the kernels only
            t_pat, t_body, want = float("nan"), float("nan"), got
        flop = 2.0 * n_psr * n_psr * 2 * maps.shape[1] * n_map
        plan = _capi.orf_plan(n_psr, nside, n_map)
        result[name] = dict(
            n_psr=n_psr, nside=nside, n_map=n_map, plan=plan,
            kernel_ms_median=float(np.median(ker)), kernel_ms_min=float(ker.min()), kernel_ms_max=float(ker.max()),
            call_ms_median=float(np.median(wall)), call_ms_min=float(wall.min()), call_ms_max=float(wall.max()),
            gram_flop=flop, flops_achieved=flop / (np.median(ker) * 1e-3),
            fraction_of_mfma_ceiling=flop / (np.median(ker) * 1e-3) / MFMA_CEILING,
            numpy_antenna_patterns_s=t_pat, numpy_body_s=t_body,
            numpy_body_over_call=t_body / (np.median(wall) * 1e-3),
            max_abs_diff_vs_numpy_over_peak=float(np.nanmax(np.abs(got - want)) / np.nanmax(np.abs(want))))
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
