"""Times the optimal statistic (fpta_batch_os: k_fit_apply on its second operator slot, then k_os_pairs + k_os_reduce) on
the GPU, split into its two stages, beside a Fourier fit (fpta_batch_fit) of the same K on the same block in the same
run.

  python tools/bench_optimal_statistic.py [--calls 20] [--warmup 3] [--out profiles/os_bench.json]

Shape: C2 (100 pulsars x 2000 TOAs, 1024 realizations, 1.6 GB), a red process of 30 modes per pulsar and a common
process of 30 modes (K = 60) as the noise model, make_Mmat's eight columns marginalised, three-band frequencies,
white-noise weights. The block is white noise (neither stage's traffic or arithmetic depends on what the block holds).
J = 1 is the Hellings-Downs ORF, J = 13 is HD + monopole + dipole + ten angular bins.

fpta_batch_os books one FPTA_K_DENSE entry per call for both stages, so the stages are separated by setting the same
statistic with J = 0 (stage 1 alone: the clear of the coefficient buffer and k_fit_apply), J = 1 and J = 13: stage 2
(k_os_pairs + k_os_reduce) is the difference of the medians. Times are HIP-event times on the context stream
(fpta_kernel_stats); --calls launches after --warmup, medians, spread = max - min. Stage 1 is reported as a ratio to
the Fourier fit (the same kernel on another operator). Stage 2 is reported against its model: one read of the
coefficient buffer [P][K][R_pad] at 8 TB/s plus 2 P^2 K R FLOP at 50 TF (DESIGN.md section 5b's measured fp64 MFMA
ceiling). Needs a GPU: there is no fallback."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "os_bench.json"))
    a = ap.parse_args()
    if a.calls < 20:
        ap.error("--calls must be >= 20 for a measurement")
    if _capi.build_flags() & _capi.BUILD_DEBUG:
        sys.exit("bench_optimal_statistic: the debug build is not for measurements")
    ctx = _capi.get_context()
    ctx.set_option(_capi.OPT_PROFILE, 1)
    P, n_toa, R, N = 100, 2000, 1024, 30
    K = 2 * N
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
    ctx.batch_set_white(sigma)
    ctx.batch_synth(1, 0, R, to_host=False)
    _, ld, nr = ctx.batch_device_out()
    res = dict(n_psr=P, n_toa_per_psr=n_toa, realizations=R, K=K, block_bytes=int(8 * ld * nr),
               operator_bytes=int(8 * K * ld), coefficient_bytes=int(8 * P * K * R), calls=a.calls, warmup=a.warmup)
    ctx.batch_set_fit([N], f, [0.0], [1400.0], M=M, weights=1 / sigma ** 2)
    res["fit"] = timed(ctx, lambda: ctx.batch_fit(K, to_host=False), a.calls, a.warmup)
    for J, G in ((0, None), (1, G13[:1]), (13, G13)):
        t0 = time.time()
        ctx.batch_set_os([N, N], np.concatenate([f, f]), [0.0, 0.0], [1400.0, 1400.0], phi, 1, phi[0, N:], G, M=M,
                         weights=1 / sigma ** 2)
        res[f"host_plan_seconds_j{J}"] = time.time() - t0
        res[f"os_j{J}"] = timed(ctx, lambda: _capi._lib.fpta_batch_os(ctx._h, None, None, None), a.calls, a.warmup)
    res["fit_again"] = timed(ctx, lambda: ctx.batch_fit(K, to_host=False), a.calls, a.warmup)
    s1 = res["os_j0"]["ms_median"]
    res["stage1_ms"] = s1
    res["stage1_over_fit"] = s1 / res["fit"]["ms_median"]
    res["fit_run_spread_ratio"] = max(res["fit"]["ms_max"], res["fit_again"]["ms_max"]) / \
        min(res["fit"]["ms_min"], res["fit_again"]["ms_min"])
    res["pairs_model_ms"] = (8.0 * P * K * R / (HBM_TBS * 1e12) + 2.0 * P * P * K * R / (MFMA_TF * 1e12)) * 1e3
    for J in (1, 13):
        s2 = res[f"os_j{J}"]["ms_median"] - s1
        res[f"stage2_ms_j{J}"] = s2
        res[f"stage2_over_model_j{J}"] = s2 / res["pairs_model_ms"]
        res[f"stage2_over_stage1_j{J}"] = s2 / s1
    print(json.dumps(res), flush=True)
    with open(a.out, "w") as fh:
        json.dump({"c2_100x2000_r1024_k60": res}, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
