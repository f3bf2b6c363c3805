"""Times the likelihood grid (fpta_batch_lnl: k_fit_apply on its third operator slot, then k_lnl_quad + k_lnl_reduce) on
the GPU, split into its two stages, beside a Fourier fit (fpta_batch_fit) of the same K on the same block in the same
run.

  python tools/bench_likelihood_grid.py [--calls 20] [--warmup 3] [--out profiles/lnl_grid_bench.json]

Shape: C2 (100 pulsars x 2000 TOAs, 1024 realizations, 1.6 GB), a red process of 30 modes per pulsar as the base model
and a common process of 30 modes (K = 60) as the target, make_Mmat's eight columns marginalised, three-band
frequencies, white-noise weights. The block is white noise (neither stage's traffic or arithmetic depends on what the
block holds). The grids are power laws around the target's level, G = 1, 100 (10 x 10) and 400 (20 x 20).

fpta_batch_lnl books one FPTA_K_DENSE entry per call for every stage, so stage 2 (k_lnl_quad + k_lnl_reduce) is the
difference of the medians to a run of stage 1 alone in the same run: the optimal statistic of the same model with no
pair-weight matrix (J = 0: the clear of the coefficient buffer and k_fit_apply on an operator of the same shape).
Times are HIP-event times on the context stream (fpta_kernel_stats); --calls launches after --warmup, medians, spread =
max - min. Stage 2 is reported against its model, the larger of P G R sum_groups (16 x columns up to the group's
diagonal block) x 2 FLOP at 50 TF (DESIGN.md section 5b's measured fp64 MFMA ceiling) and one read of U at 8 TB/s, and
against stage 1 and the Fourier fit. Needs a GPU: there is no fallback."""
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
from fakepta_amd import lnl as _lnl  # noqa: E402
from tests import tm_reference as T  # noqa: E402
from tools.bench_optimal_statistic import stats, timed  # noqa: E402,F401

YEAR = 365.25 * 86400.0
MFMA_TF, HBM_TBS = 50.0, 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lnl_grid_bench.json"))
    a = ap.parse_args()
    if a.calls < 20:
        ap.error("--calls must be >= 20 for a measurement")
    if _capi.build_flags() & _capi.BUILD_DEBUG:
        sys.exit("bench_likelihood_grid: the debug build is not for measurements")
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
    f = np.arange(1, N + 1) / (15 * YEAR)
    white = 2.0 / np.array([np.sum(1 / sigma[offs[p]:offs[p + 1]] ** 2) for p in range(P)])
    phi = np.concatenate([100.0 * white[:, None] * np.arange(1, N + 1)[None, :] ** -3.0,
                          np.tile(10.0 * white.mean() * np.arange(1, N + 1) ** (-13 / 3), (P, 1))], axis=1)
    ctx.batch_set_toas(offs, toas, nu)
    ctx.batch_set_white(sigma)
    ctx.batch_synth(1, 0, R, to_host=False)
    _, ld, nr = ctx.batch_device_out()
    groups = (K + 15) // 16
    u_doubles = 128 * groups * (groups + 1)
    flop_pg = 2.0 * sum(16 * 16 * (j + 1) for j in range(groups))  # per pulsar, grid point and realization
    res = dict(n_psr=P, n_toa_per_psr=n_toa, realizations=R, K=K, block_bytes=int(8 * ld * nr),
               operator_bytes=int(8 * K * ld), coefficient_bytes=int(8 * P * K * R), calls=a.calls, warmup=a.warmup)
    model = ([N, N], np.concatenate([f, f]), [0.0, 0.0], [1400.0, 1400.0], phi, 1)
    ctx.batch_set_fit([N], f, [0.0], [1400.0], M=M, weights=1 / sigma ** 2)
    res["fit"] = timed(ctx, lambda: ctx.batch_fit(K, to_host=False), a.calls, a.warmup)
    ctx.batch_set_os(*model, phi[0, N:], None, M=M, weights=1 / sigma ** 2)
    res["stage1"] = timed(ctx, lambda: _capi._lib.fpta_batch_os(ctx._h, None, None, None), a.calls, a.warmup)
    s1 = res["stage1"]["ms_median"]
    res["stage1_ms"] = s1
    res["stage1_over_fit"] = s1 / res["fit"]["ms_median"]
    # the log10_A whose gamma = 13 / 3 power law has the target's first-mode variance
    level = 0.5 * np.log10(phi[0, N] / _lnl.powerlaw_grid(f, [0.0], [13 / 3])[0, 0])
    for n_a, n_g in ((1, 1), (10, 10), (20, 20)):
        G = n_a * n_g
        grid = _lnl.powerlaw_grid(f, level + np.linspace(-0.5, 0.5, n_a) if n_a > 1 else [level],
                                  np.linspace(2.0, 6.0, n_g) if n_g > 1 else [13 / 3])
        t0 = time.time()
        ctx.batch_set_lnl(*model, grid, M=M, weights=1 / sigma ** 2)
        res[f"host_plan_seconds_g{G}"] = time.time() - t0
        res[f"lnl_g{G}"] = timed(ctx, lambda: _capi._lib.fpta_batch_lnl(ctx._h, None, None, None), a.calls, a.warmup)
        s2 = res[f"lnl_g{G}"]["ms_median"] - s1
        mfma_ms = P * G * R * flop_pg / (MFMA_TF * 1e12) * 1e3
        read_ms = 8.0 * P * G * u_doubles / (HBM_TBS * 1e12) * 1e3
        res[f"factor_bytes_g{G}"] = int(8 * P * G * u_doubles)
        res[f"stage2_ms_g{G}"] = s2
        res[f"stage2_model_ms_g{G}"] = max(mfma_ms, read_ms)
        res[f"stage2_over_model_g{G}"] = s2 / max(mfma_ms, read_ms)
        res[f"stage2_over_stage1_g{G}"] = s2 / s1
        res[f"stage2_over_fit_g{G}"] = s2 / res["fit"]["ms_median"]
    res["fit_again"] = timed(ctx, lambda: ctx.batch_fit(K, to_host=False), a.calls, a.warmup)
    res["fit_run_spread_ratio"] = max(res["fit"]["ms_max"], res["fit_again"]["ms_max"]) / \
        min(res["fit"]["ms_min"], res["fit_again"]["ms_min"])
    print(json.dumps(res), flush=True)
    with open(a.out, "w") as fh:
        json.dump({"c2_100x2000_r1024_k60": res}, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
