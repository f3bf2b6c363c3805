"""Times the correlated likelihood grid (fpta_batch_set_clnl, fpta_batch_clnl: k_fit_apply on its fifth operator slot,
then k_clnl_mix + k_clnl_solve + k_clnl_reduce) on the GPU: the set time, host and device apart, and the per-block time
split into its stages.

  python tools/bench_correlated_likelihood.py [--calls 20] [--warmup 3] [--grids 1,10,100]
                                              [--out profiles/clnl_bench.json]

Shape: C2 (100 pulsars x 2000 TOAs, 1024 realizations, 1.6 GB), bench_likelihood_grid.py's model: a red process of 30
modes per pulsar as the base model and a common process of 30 modes (K = 60, n = P K = 6000) as the target, make_Mmat's
eight columns marginalised, three-band frequencies, white-noise weights, a white-noise block. One ORF, Hellings-Downs of
random positions; power-law grids around the target's level with G = 1, 10 and 100 points (100 points cache 29 GB of
factors).

Set time: the wall time of fpta_batch_set_clnl; its device part is what the call books under FPTA_K_DENSE (k_clnl_fill,
the blocked Cholesky of every grid point, k_clnl_logdet), the rest is the host (the operators, T in long double, uploads
and the per-matrix synchronisation). Per block: fpta_batch_clnl books one FPTA_K_DENSE entry per call, so stage 2 (mix,
solve, reduce) is the difference of the medians to a run of stage 1 alone in the same run: the optimal statistic of the
same model with no pair-weight matrix. HIP-event times on the context stream; --calls launches after --warmup, medians.
Stage 2 is reported against its model, the larger of n^2 R G FLOP at 50 TF (DESIGN.md section 5b's measured fp64 MFMA
ceiling) and one read of the factors' lower triangles per 64-realization tile at 8 TB/s. Needs a GPU: there is no
fallback."""
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
from tools.bench_optimal_statistic import timed  # noqa: E402

YEAR = 365.25 * 86400.0
MFMA_TF, HBM_TBS = 50.0, 8.0


def hd_matrix(pos):
    """The Hellings-Downs ORF of unit vectors pos [P, 3] (1 on the diagonal)."""
    x = np.clip((1.0 - pos @ pos.T) / 2.0, 1e-300, None)
    g = 1.5 * x * np.log(x) - 0.25 * x + 0.5
    np.fill_diagonal(g, 1.0)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--grids", default="1,10,100")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clnl_bench.json"))
    a = ap.parse_args()
    if a.calls < 20:
        ap.error("--calls must be >= 20 for a measurement")
    if _capi.build_flags() & _capi.BUILD_DEBUG:
        sys.exit("bench_correlated_likelihood: the debug build is not for measurements")
    ctx = _capi.get_context()
    ctx.set_option(_capi.OPT_PROFILE, 1)
    P, n_toa, R, N = 100, 2000, 1024, 30
    K = 2 * N
    n = P * K
    n_pad = (n + 63) // 64 * 64
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
    v = rng.normal(size=(P, 3))
    A = np.linalg.cholesky(hd_matrix(v / np.linalg.norm(v, axis=1)[:, None]))
    ctx.batch_set_toas(offs, toas, nu)
    ctx.batch_set_white(sigma)
    ctx.batch_synth(1, 0, R, to_host=False)
    _, ld, nr = ctx.batch_device_out()
    res = dict(n_psr=P, n_toa_per_psr=n_toa, realizations=R, K=K, n=n, n_pad=n_pad, n_orf=1, block_bytes=int(8 * ld * nr),
               operator_bytes=int(8 * K * ld), calls=a.calls, warmup=a.warmup)
    model = ([N, N], np.concatenate([f, f]), [0.0, 0.0], [1400.0, 1400.0], phi, 1)
    ctx.batch_set_os(*model, phi[0, N:], None, M=M, weights=1 / sigma ** 2)
    res["stage1"] = timed(ctx, lambda: _capi._lib.fpta_batch_os(ctx._h, None, None, None), a.calls, a.warmup)
    s1 = res["stage1_ms"] = res["stage1"]["ms_median"]
    level = 0.5 * np.log10(phi[0, N] / _lnl.powerlaw_grid(f, [0.0], [13 / 3])[0, 0])
    tiles = (R + 63) // 64
    for G in [int(g) for g in a.grids.split(",")]:
        grid = _lnl.powerlaw_grid(f, level + np.linspace(-0.5, 0.5, G) if G > 1 else [level], [13 / 3])
        ctx.synchronize()
        ctx.reset_stats()
        t0 = time.time()
        ctx.batch_set_clnl(*model, grid, A, M=M, weights=1 / sigma ** 2)
        ctx.synchronize()
        wall = time.time() - t0
        dev = ctx.kernel_stats(_capi.K_DENSE)[1] * 1e-3
        res[f"set_seconds_g{G}"] = wall
        res[f"set_device_seconds_g{G}"] = dev
        res[f"set_host_seconds_g{G}"] = wall - dev
        res[f"clnl_g{G}"] = timed(ctx, lambda: _capi._lib.fpta_batch_clnl(ctx._h, None, None, None, None), a.calls,
                                  a.warmup)
        s2 = res[f"clnl_g{G}"]["ms_median"] - s1
        mfma_ms = float(n) * n * R * G / (MFMA_TF * 1e12) * 1e3
        read_ms = 8.0 * 0.5 * n * n * G * tiles / (HBM_TBS * 1e12) * 1e3
        res[f"factor_bytes_g{G}"] = int(8 * G * n_pad * n_pad)
        res[f"stage2_ms_g{G}"] = s2
        res[f"stage2_model_ms_g{G}"] = max(mfma_ms, read_ms)
        res[f"stage2_model_mfma_ms_g{G}"] = mfma_ms
        res[f"stage2_model_read_ms_g{G}"] = read_ms
        res[f"stage2_over_model_g{G}"] = s2 / max(mfma_ms, read_ms)
        res[f"stage2_over_stage1_g{G}"] = s2 / s1
        print(json.dumps({k: res[k] for k in res if k.endswith(f"_g{G}")}), flush=True)
    res["stage1_again"] = timed(ctx, lambda: _capi._lib.fpta_batch_os(ctx._h, None, None, None), a.calls, a.warmup)
    print(json.dumps(res), flush=True)
    with open(a.out, "w") as fh:
        json.dump({"c2_100x2000_r1024_k60": res}, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
