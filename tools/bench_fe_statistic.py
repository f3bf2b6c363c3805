"""Times the continuous-wave F-statistics (fpta_batch_fe: k_fit_apply on its fourth operator slot, then k_fe_sky +
k_fe_reduce) on the GPU, split into its two stages.

  python tools/bench_fe_statistic.py [--calls 20] [--warmup 3] [--out profiles/fe_bench.json]

Shape: C2 (100 pulsars x 2000 TOAs, 1024 realizations, 1.6 GB), a red process of 30 modes per pulsar as the noise model,
make_Mmat's eight columns marginalised, three-band frequencies, white-noise weights, G = 60 frequencies k / (15 yr)
(K = 120) and the HEALPix skies of nside 2, 4 and 8 (48, 192 and 768 directions). The block is white noise (neither
stage's traffic or arithmetic depends on what the block holds).

fpta_batch_fe books one FPTA_K_DENSE entry per call for both stages, so the stages are separated by setting the same
statistic with one direction (stage 1: the clear of the coefficient buffer and k_fit_apply, plus a stage 2 of one tile)
against the full sky: stage 2 (k_fe_sky + k_fe_reduce) is the difference of the medians. Times are HIP-event times on
the context stream (fpta_kernel_stats); --calls launches after --warmup, medians, spread = max - min. Stage 2 is reported
against its model, one read of the coefficient buffer [P][K][R_pad] at 8 TB/s plus 8 n_sky P G R FLOP at 50 TF (DESIGN.md
section 5b's measured fp64 MFMA ceiling), and against stage 1 of the same run. Needs a GPU: there is no fallback."""
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
from fakepta_amd import fe as _fe  # noqa: E402
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fe_bench.json"))
    a = ap.parse_args()
    if a.calls < 20:
        ap.error("--calls must be >= 20 for a measurement")
    if _capi.build_flags() & _capi.BUILD_DEBUG:
        sys.exit("bench_fe_statistic: the debug build is not for measurements")
    ctx = _capi.get_context()
    ctx.set_option(_capi.OPT_PROFILE, 1)
    P, n_toa, R, N, G = 100, 2000, 1024, 30, 60
    K = 2 * G
    rng = np.random.default_rng(P)
    offs = np.arange(P + 1, dtype=np.int64) * n_toa
    toas = np.concatenate([np.sort(rng.uniform(0.0, 15 * YEAR, n_toa)) for _ in range(P)])
    nu = np.abs(rng.choice([800.0, 1400.0, 2500.0], size=P * n_toa) + rng.normal(0, 10, P * n_toa))
    sigma = rng.uniform(1e-7, 1e-6, P * n_toa)
    M = np.concatenate([T.mmat(toas[offs[p]:offs[p + 1]], nu[offs[p]:offs[p + 1]]) for p in range(P)])
    v = rng.normal(size=(P, 3))
    pos = v / np.linalg.norm(v, axis=1)[:, None]
    f = np.arange(1, N + 1) / (15 * YEAR)
    fgw = np.arange(1, G + 1) / (15 * YEAR)
    white = 2.0 / np.array([np.sum(1 / sigma[offs[p]:offs[p + 1]] ** 2) for p in range(P)])
    phi = 100.0 * white[:, None] * np.arange(1, N + 1)[None, :] ** -3.0
    ctx.batch_set_toas(offs, toas, nu)
    ctx.batch_set_white(sigma)
    ctx.batch_synth(1, 0, R, to_host=False)
    _, ld, nr = ctx.batch_device_out()
    res = dict(n_psr=P, n_toa_per_psr=n_toa, realizations=R, K=K, G=G, block_bytes=int(8 * ld * nr),
               operator_bytes=int(8 * K * ld), coefficient_bytes=int(8 * P * K * R), calls=a.calls, warmup=a.warmup)

    def run(label, sky):
        t0 = time.time()
        ctx.batch_set_fe([N], f, [0.0], [1400.0], phi, fgw, sky, pos, M=M, weights=1 / sigma ** 2)
        res[f"host_plan_seconds_{label}"] = time.time() - t0
        res[f"fe_{label}"] = timed(
            ctx, lambda: _capi._lib.fpta_batch_fe(ctx._h, None, None, None, None, None, None, None), a.calls, a.warmup)
        return res[f"fe_{label}"]["ms_median"]

    s1 = run("one_direction", _fe.sky_grid(nside=1)[:1])
    res["stage1_ms"] = s1
    for nside in (2, 4, 8):
        sky = _fe.sky_grid(nside=nside)
        s2 = run(f"nside{nside}", sky) - s1
        model = (8.0 * P * K * R / (HBM_TBS * 1e12) + 8.0 * len(sky) * P * G * R / (MFMA_TF * 1e12)) * 1e3
        res[f"stage2_ms_nside{nside}"] = s2
        res[f"stage2_model_ms_nside{nside}"] = model
        res[f"stage2_over_model_nside{nside}"] = s2 / model
        res[f"stage2_over_stage1_nside{nside}"] = s2 / s1
    res["stage1_again_ms"] = run("one_direction_again", _fe.sky_grid(nside=1)[:1])
    print(json.dumps(res), flush=True)
    with open(a.out, "w") as fh:
        json.dump({"c2_100x2000_r1024_g60": res}, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
