"""Times the sky scrambles of the optimal statistic (fpta_batch_os_scrambles: k_fit_apply, k_os_pairs + k_os_reduce,
then k_scr_pairs, k_scr_gemm and k_scr_rank) on the GPU, beside a device copy of the block, the GEMM's model and the
capability that existed before: optimal_statistic() given the scrambles' matrices as ORFs.

  python tools/bench_os_scrambles.py [--calls 20] [--warmup 3] [--out profiles/os_scrambles_bench.json]

Shape: C2 (100 pulsars x 2000 TOAs, 1024 realizations, 1.6 GB), a red process of 30 modes per pulsar and a common
process of 30 modes (K = 60), make_Mmat's eight columns marginalised, three-band frequencies, white-noise weights, the
Hellings-Downs ORF observed; J = 1, 256, 1000 and 10000 scrambles from fakepta_amd.os.sky_scrambles.

fpta_batch_os_scrambles books one FPTA_K_DENSE entry per call, so its parts are separated by differences of medians in
the same run: fpta_batch_os alone is stages 1 and 2; the call with J = 1 adds k_scr_pairs (and a GEMM and a rank of one
row); J = 1000 and 10000 add k_scr_gemm and k_scr_rank, reported together against the model 2 J n_pair R FLOP at 50 TF
(DESIGN.md section 5b's measured fp64 MFMA ceiling) plus one read of Gs at 8 TB/s. At J = 256 the same matrices go
through set_optimal_statistic(orfs=...) -> fpta_batch_os, alternated with the new path. Times are HIP-event times on
the context stream (fpta_kernel_stats); --calls launches after --warmup, medians, spread = max - min. The set's time
(candidates, match, validation, upload, rows, norms) is wall time. Needs a GPU: there is no fallback."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from fakepta_amd import _capi  # noqa: E402
from fakepta_amd import os as _os  # noqa: E402
from tests import tm_reference as T  # noqa: E402

YEAR = 365.25 * 86400.0
MFMA_TF, HBM_TBS = 50.0, 8.0


def stats(v):
    v = np.array(v)
    return dict(ms_median=float(np.median(v)), ms_min=float(v.min()), ms_max=float(v.max()),
                ms_spread=float(v.max() - v.min()))


def timed(ctx, call, calls, warmup):
    """HIP-event time booked under FPTA_K_DENSE per call."""
    for _ in range(warmup):
        call()
    ctx.synchronize()
    ev = []
    for _ in range(calls):
        ctx.reset_stats()
        call()
        ctx.synchronize()
        ev.append(ctx.kernel_stats(_capi.K_DENSE)[1])
    return stats(ev)


def timed_wall(ctx, call, calls, warmup):
    """Wall time per call with the stream idle before and after (the device copy books no kernel entry)."""
    for _ in range(warmup):
        call()
    ctx.synchronize()
    ev = []
    for _ in range(calls):
        t0 = time.perf_counter()
        call()
        ctx.synchronize()
        ev.append((time.perf_counter() - t0) * 1e3)
    return stats(ev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "os_scrambles_bench.json"))
    a = ap.parse_args()
    if a.calls < 20:
        ap.error("--calls must be >= 20 for a measurement")
    if _capi.build_flags() & _capi.BUILD_DEBUG:
        sys.exit("bench_os_scrambles: the debug build is not for measurements")
    ctx = _capi.get_context()
    ctx.set_option(_capi.OPT_PROFILE, 1)
    P, n_toa, R, N = 100, 2000, 1024, 30
    rng = np.random.default_rng(P)
    offs = np.arange(P + 1, dtype=np.int64) * n_toa
    toas = np.concatenate([np.sort(rng.uniform(0.0, 15 * YEAR, n_toa)) for _ in range(P)])
    nu = np.abs(rng.choice([800.0, 1400.0, 2500.0], size=P * n_toa) + rng.normal(0, 10, P * n_toa))
    sigma = rng.uniform(1e-7, 1e-6, P * n_toa)
    M = np.concatenate([T.mmat(toas[offs[p]:offs[p + 1]], nu[offs[p]:offs[p + 1]]) for p in range(P)])
    v = rng.normal(size=(P, 3))
    pos = v / np.linalg.norm(v, axis=1)[:, None]
    f = np.arange(1, N + 1) / (15 * YEAR)
    white = 2.0 / np.array([np.sum(1 / sigma[offs[p]:offs[p + 1]] ** 2) for p in range(P)])
    phi = np.concatenate([100.0 * white[:, None] * np.arange(1, N + 1)[None, :] ** -3.0,
                          np.tile(10.0 * white.mean() * np.arange(1, N + 1) ** (-13 / 3), (P, 1))], axis=1)
    hd = _os.hd_matrix(pos)
    ctx.batch_set_toas(offs, toas, nu)
    ctx.batch_add_signal(0, np.tile(f, (P, 1)), np.sqrt(phi[:, :N]))
    ctx.batch_add_signal(1, f, np.sqrt(phi[0, N:]), L=np.eye(P))
    ctx.batch_set_white(sigma)
    ctx.batch_synth(1, 0, R, to_host=False)
    dptr, ld, nr = ctx.batch_device_out()
    n_pair = P * (P - 1) // 2
    res = dict(n_psr=P, n_toa_per_psr=n_toa, realizations=R, K=2 * N, n_pair=n_pair, block_bytes=int(8 * ld * nr),
               calls=a.calls, warmup=a.warmup)
    n_modes, ff, w = [N, N], np.concatenate([f, f]), 1 / sigma ** 2

    def set_os(G):
        ctx.batch_set_os(n_modes, ff, [0.0, 0.0], [1400.0, 1400.0], phi, 1, phi[0, N:], G, M=M, weights=w)

    def os_call():
        ctx._check(_capi._lib.fpta_batch_os(ctx._h, None, None, None), "fpta_batch_os")

    def scr_call():
        ctx._check(_capi._lib.fpta_batch_os_scrambles(ctx._h, None, None, None, None, None, None),
                   "fpta_batch_os_scrambles")

    # (a) the device copy of the block, the traffic yardstick, on the library's own HIP runtime
    hip = ctypes.CDLL("libamdhip64.so")
    n_bytes = int(8 * ld * nr)
    dst = ctypes.c_void_p()

    def hip_ok(rc, what):
        if rc != 0:
            sys.exit(f"bench_os_scrambles: {what} failed with HIP error {rc}")

    hip_ok(hip.hipMalloc(ctypes.byref(dst), ctypes.c_size_t(n_bytes)), "hipMalloc of the copy's target")

    def copy_block():
        hip_ok(hip.hipMemcpy(dst, ctypes.c_void_p(dptr), ctypes.c_size_t(n_bytes), 3), "hipMemcpy device to device")
        hip_ok(hip.hipDeviceSynchronize(), "hipDeviceSynchronize")

    res["block_copy"] = timed_wall(ctx, copy_block, a.calls, a.warmup)
    res["block_copy_GBps_read_plus_write"] = 2 * n_bytes / (res["block_copy"]["ms_median"] * 1e-3) / 1e9
    hip_ok(hip.hipFree(dst), "hipFree")

    set_os(hd[None])
    res["os_j1"] = timed(ctx, os_call, a.calls, a.warmup)
    for J in (1, 256, 1000, 10000):
        t0 = time.perf_counter()
        cand, _ = _os.sky_scrambles(ctx, pos, J, seed=J, max_match=0.1, ref=hd[None])
        t1 = time.perf_counter()
        norm, match = ctx.batch_set_os_scrambles(pos=cand)
        t2 = time.perf_counter()
        res[f"set_seconds_j{J}"] = dict(draw_and_match=t1 - t0, validate_upload_rows_norms=t2 - t1, total=t2 - t0)
        res[f"max_abs_match_j{J}"] = float(np.abs(match).max())
        res[f"scr_j{J}"] = timed(ctx, scr_call, a.calls, a.warmup)
        extra = res[f"scr_j{J}"]["ms_median"] - res["os_j1"]["ms_median"]
        res[f"scr_minus_os_ms_j{J}"] = extra
        if J == 256:
            # (c) what existed before: the same 256 matrices as the ORFs of the statistic, alternated with the new path
            mats = np.array([_os.hd_matrix(p) for p in cand])
            old, new = [], []
            for _ in range(2):
                set_os(mats)
                old.append(timed(ctx, os_call, a.calls // 2, a.warmup))
                set_os(hd[None])
                ctx.batch_set_os_scrambles(pos=cand)
                new.append(timed(ctx, scr_call, a.calls // 2, a.warmup))
            for key, runs in (("os_orfs_j256", old), ("scr_j256_alternated", new)):
                res[key] = dict(ms_median=float(np.median([r["ms_median"] for r in runs])),
                                ms_min=min(r["ms_min"] for r in runs), ms_max=max(r["ms_max"] for r in runs))
                res[key]["ms_spread"] = res[key]["ms_max"] - res[key]["ms_min"]
            res["scr_over_os_orfs_j256"] = res["scr_j256_alternated"]["ms_median"] / res["os_orfs_j256"]["ms_median"]
            res["scr_not_slower_than_os_orfs_j256"] = bool(
                res["scr_j256_alternated"]["ms_median"] <= res["os_orfs_j256"]["ms_median"] +
                res["os_orfs_j256"]["ms_spread"])
    pairs = res["scr_minus_os_ms_j1"]
    res["k_scr_pairs_ms_estimate"] = pairs
    for J in (1000, 10000):
        # (b) the GEMM's model: 2 J n_pair R FLOP at 50 TF plus one read of Gs at 8 TB/s
        model = 2.0 * J * n_pair * R / (MFMA_TF * 1e12) + 8.0 * J * n_pair / (HBM_TBS * 1e12)
        got = res[f"scr_minus_os_ms_j{J}"] - pairs
        res[f"gemm_rank_ms_j{J}"] = got
        res[f"gemm_model_ms_j{J}"] = model * 1e3
        res[f"gemm_rank_over_model_j{J}"] = got / (model * 1e3)
        res[f"scr_over_block_copy_j{J}"] = res[f"scr_j{J}"]["ms_median"] / res["block_copy"]["ms_median"]
    print(json.dumps(res), flush=True)
    with open(a.out, "w") as fh:
        json.dump({"c2_100x2000_r1024": res}, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
