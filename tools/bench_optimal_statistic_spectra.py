"""Times the optimal statistic under a spectrum per realization (fpta_batch_os_spectra: k_spectra_amp's tables,
k_fit_apply on its sixth operator slot, k_oss_solve, k_oss_gram, k_oss_contract, k_os_pairs + k_os_reduce) on the GPU,
beside the fixed optimal statistic (fpta_batch_os) and a device copy of the block in the same run.

  python tools/bench_optimal_statistic_spectra.py [--calls 20] [--warmup 3] [--out profiles/os_spectra_bench.json]

Shape: C2 (100 pulsars x 2000 TOAs, 1024 realizations, 1.6 GB), a red process of 30 modes per pulsar and a common
process of 30 modes, make_Mmat's eight columns marginalised, three-band frequencies, white-noise weights. q = 120
varies both processes (K = 60), q = 60 the common process alone (the red process is then part of the fixed model). The
tables are power laws, log10_A drawn per realization over a decade. J = 1 is the Hellings-Downs ORF, J = 13 is HD +
monopole + dipole + ten angular bins (n_orf = 3).

fpta_batch_os_spectra books one FPTA_K_DENSE entry per call, so the stages are separated by differences of medians
in the same run: stage 1 is a Fourier fit of the same q columns (the same kernel on another operator); the call with
J = 0 adds the tables, the solve and the Gram; J = 1 and J = 13 add the contraction and the pair sums. The solve and
the Gram are reported together against the sum of their models: q^3 / 3 FLOP per matrix and 2 (P^2 / 2) K^2 R FLOP at
50 TF (DESIGN.md section 5b's measured fp64 MFMA ceiling) plus one read of Z' at 8 TB/s. Times are HIP-event times
on the context stream (fpta_kernel_stats); --calls launches after --warmup, medians, spread = max - min. Needs a GPU:
there is no fallback."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "os_spectra_bench.json"))
    a = ap.parse_args()
    if a.calls < 20:
        ap.error("--calls must be >= 20 for a measurement")
    if _capi.build_flags() & _capi.BUILD_DEBUG:
        sys.exit("bench_optimal_statistic_spectra: the debug build is not for measurements")
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
    x = (1 - pos @ pos.T) / 2
    with np.errstate(divide="ignore", invalid="ignore"):
        hd = 1.5 * x * np.log(x) - 0.25 * x + 0.5
    dip = pos @ pos.T
    for g in (hd, dip):
        np.fill_diagonal(g, 0.0)
    G13 = np.concatenate([np.stack([hd, np.ones((P, P)) - np.eye(P), dip]), _os.angular_bins(pos, 10)[0]])
    ctx.batch_set_toas(offs, toas, nu)
    i_rn = ctx.batch_add_signal(0, np.tile(f, (P, 1)), np.sqrt(phi[:, :N]))
    i_gw = ctx.batch_add_signal(1, f, np.sqrt(phi[0, N:]), L=np.eye(P))
    ctx.batch_set_white(sigma)
    ctx.batch_synth(1, 0, R, to_host=False)
    dptr, ld, nr = ctx.batch_device_out()
    res = dict(n_psr=P, n_toa_per_psr=n_toa, realizations=R, block_bytes=int(8 * ld * nr), calls=a.calls,
               warmup=a.warmup)
    tabs = {i_rn: np.stack([rng.uniform(-14.5, -13.5, (R, P)), np.full((R, P), 3.0)], axis=-1),
            i_gw: np.stack([rng.uniform(-15.0, -14.0, R), np.full(R, 13 / 3)], axis=-1)}
    n_modes, ff, w = [N, N], np.concatenate([f, f]), 1 / sigma ** 2

    def spectra_call(ids, K, J, n_orf):
        seg = np.array(ids, dtype=np.int32)
        form = np.ones(len(ids), dtype=np.int32)
        per = np.array([int(tabs[i].ndim == 3) for i in ids], dtype=np.int32)
        rows = np.full(len(ids), R, dtype=np.int32)
        keep = [np.ascontiguousarray(tabs[i]) for i in ids]
        ptrs = (ctypes.c_void_p * len(ids))(*[t.ctypes.data for t in keep])
        return lambda: ctx._check(_capi._lib.fpta_batch_os_spectra(
            ctx._h, len(ids), _capi._ptr(seg), _capi._ptr(form), _capi._ptr(per), _capi._ptr(rows),
            ctypes.cast(ptrs, ctypes.c_void_p), None, None, None, None, None, None, None), "fpta_batch_os_spectra")

    # the device copy of the block, the traffic yardstick: hipMemcpy device to device of the resident block on the
    # library's own HIP runtime, timed with the device idle before and after. A failure ends the run.
    hip = ctypes.CDLL("libamdhip64.so")
    n_bytes = int(8 * ld * nr)
    dst = ctypes.c_void_p()

    def hip_ok(rc, what):
        if rc != 0:
            sys.exit(f"bench_optimal_statistic_spectra: {what} failed with HIP error {rc}")

    hip_ok(hip.hipMalloc(ctypes.byref(dst), ctypes.c_size_t(n_bytes)), "hipMalloc of the copy's target")

    def copy_block():
        hip_ok(hip.hipMemcpy(dst, ctypes.c_void_p(dptr), ctypes.c_size_t(n_bytes), 3), "hipMemcpy device to device")
        hip_ok(hip.hipDeviceSynchronize(), "hipDeviceSynchronize")

    res["block_copy"] = timed_wall(ctx, copy_block, a.calls, a.warmup)
    res["block_copy_GBps_read_plus_write"] = 2 * n_bytes / (res["block_copy"]["ms_median"] * 1e-3) / 1e9
    hip_ok(hip.hipFree(dst), "hipFree")
    for q, vary, ids in ((120, [0, 1], [i_rn, i_gw]), (60, [1], [i_gw])):
        K = 2 * N
        ctx.batch_set_fit(n_modes if q == 120 else [N], ff if q == 120 else f, [0.0] * (q // 60), [1400.0] * (q // 60),
                          M=M, weights=w)
        res[f"fit_q{q}"] = timed(ctx, lambda: ctx.batch_fit(q, to_host=False), a.calls, a.warmup)
        for J, G, n_orf in ((0, None, 0), (1, G13[:1], 1), (13, G13, 3)):
            t0 = time.time()
            ctx.batch_set_os_spectra(n_modes, ff, [0.0, 0.0], [1400.0, 1400.0], phi, 1, phi[0, N:], vary, ids, G, n_orf,
                                     M=M, weights=w)
            res[f"host_plan_seconds_q{q}_j{J}"] = time.time() - t0
            res[f"oss_q{q}_j{J}"] = timed(ctx, spectra_call(ids, K, J, n_orf), a.calls, a.warmup)
            if J == 1:  # the fixed statistic, interleaved
                ctx.batch_set_os(n_modes, ff, [0.0, 0.0], [1400.0, 1400.0], phi, 1, phi[0, N:], G, M=M, weights=w)
                res[f"os_fixed_q{q}_j1"] = timed(ctx, lambda: _capi._lib.fpta_batch_os(ctx._h, None, None, None), a.calls,
                                                a.warmup)
        s1 = res[f"fit_q{q}"]["ms_median"]
        mid = res[f"oss_q{q}_j0"]["ms_median"] - s1
        model = (P * R * q ** 3 / 3.0 + 2.0 * (P * P / 2.0) * K * K * R) / (MFMA_TF * 1e12) + \
            8.0 * K * K * P * R / (HBM_TBS * 1e12)
        res[f"solve_gram_ms_q{q}"] = mid
        res[f"solve_gram_model_ms_q{q}"] = model * 1e3
        res[f"solve_gram_over_model_q{q}"] = mid / (model * 1e3)
        for J in (1, 13):
            res[f"contract_pairs_ms_q{q}_j{J}"] = res[f"oss_q{q}_j{J}"]["ms_median"] - res[f"oss_q{q}_j0"]["ms_median"]
        res[f"oss_over_fixed_q{q}_j1"] = res[f"oss_q{q}_j1"]["ms_median"] / res[f"os_fixed_q{q}_j1"]["ms_median"]
    print(json.dumps(res), flush=True)
    with open(a.out, "w") as fh:
        json.dump({"c2_100x2000_r1024": res}, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
