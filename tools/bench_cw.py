"""Times fpta_cw_accumulate (continuous waves of a binary population summed into a whole array) on the GPU.

  python tools/bench_cw.py [--calls 12] [--warmup 3] [--out profiles/cw_bench.json]

(a) the C2 layout, 100 pulsars x 2000 TOAs, 4096 sources: once all without and once all with the pulsar term
(b) 25 pulsars x 100 TOAs, 10^4 sources (half with the pulsar term): source split auto (FPTA_OPT_CW_SPLIT 0) and
    forced to 1, alternating call by call in the same process

Kernel time is the HIP-event time of the call's kernels on the context stream (fpta_kernel_stats, FPTA_K_CW: prep +
main + reduce); call time is the host clock around the whole call (uploads, kernels, download, synchronise). Every
variant is warmed up, then timed --calls times; the figures are medians, the spread is max - min over the timed
calls. The one condition: in (b) auto must not be slower than forced-1 by more than that spread (exit status 1).
The literal numpy evaluation (tests/cw_reference.py) is timed on this host for the same pulsars on a subset of the
sources and scaled to all of them. Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from fakepta import constants as const  # noqa: E402
from fakepta_amd import _capi  # noqa: E402
from tests import cw_reference as R  # noqa: E402


def make_case(rng, n_psr, n_toa, n_src, psrterm):
    span = 15 * const.yr
    toas = np.concatenate([np.sort(rng.uniform(0, span, n_toa)) for _ in range(n_psr)])
    offs = np.arange(n_psr + 1, dtype=np.int64) * n_toa
    th, ph = np.arccos(rng.uniform(-1, 1, n_psr)), rng.uniform(0, 2 * np.pi, n_psr)
    pos = np.stack([np.cos(ph) * np.sin(th), np.sin(ph) * np.sin(th), np.cos(th)], axis=1)
    pdist = np.stack([rng.uniform(0.5, 1.5, n_psr), np.full(n_psr, 0.1)], axis=1)
    L = (pdist[:, 0] + pdist[:, 1]) * const.kpc / const.c
    # a population: chirp masses 10^8 .. 10^9.3 Msun at 2 .. 50 nHz (none coalesces within 15 yr)
    src = np.stack([rng.uniform(-1, 1, n_src), rng.uniform(0, 2 * np.pi, n_src), rng.uniform(-1, 1, n_src),
                    rng.uniform(8, 9.3, n_src), rng.uniform(-8.7, -7.3, n_src), rng.uniform(-16, -14, n_src),
                    rng.uniform(0, 2 * np.pi, n_src), rng.uniform(0, np.pi, n_src),
                    np.broadcast_to(np.asarray(psrterm, dtype=float), (n_src,))], axis=1)
    K = 256 / 5 * (10 ** src[:, 3] * const.Tsun) ** (5 / 3) * (np.pi * 10 ** src[:, 4]) ** (8 / 3)
    assert np.all(K * toas.max() < 1)
    return dict(offs=offs, toas=toas, pos=pos, pdist=pdist, L=L, src=np.ascontiguousarray(src))


def one_call(ctx, case, split):
    ctx.set_option(_capi.OPT_CW_SPLIT, split)
    out = np.zeros(case["offs"][-1])
    ctx.reset_stats()
    t0 = time.perf_counter()
    ctx.cw_accumulate(case["offs"], case["toas"], case["pos"], case["L"], case["src"], out)
    wall = time.perf_counter() - t0
    n, ms = ctx.kernel_stats(_capi.K_CW)
    assert n == 1
    return ms, wall * 1e3, out


def measure(ctx, case, splits, calls, warmup):
    """Alternates the variants call by call; {split: figures}."""
    for _ in range(warmup):
        for s in splits:
            one_call(ctx, case, s)
    ker = {s: [] for s in splits}
    wall = {s: [] for s in splits}
    outs = {}
    for _ in range(calls):
        for s in splits:
            k, w, outs[s] = one_call(ctx, case, s)
            ker[s].append(k)
            wall[s].append(w)
    pairs = len(case["src"]) * int(case["offs"][-1])
    evals = int(case["offs"][-1]) * int(np.sum(1 + (case["src"][:, 8] != 0)))
    res = {}
    for s in splits:
        k = np.array(ker[s])
        res[s] = dict(kernel_ms_median=float(np.median(k)), kernel_ms_min=float(k.min()), kernel_ms_max=float(k.max()),
                      kernel_ms_spread=float(k.max() - k.min()), call_ms_median=float(np.median(wall[s])),
                      source_toa_pairs=pairs, waveform_evaluations=evals,
                      pairs_per_s=pairs / (np.median(k) * 1e-3), evaluations_per_s=evals / (np.median(k) * 1e-3),
                      calls=calls)
    return res, outs


def numpy_time(case, n_sub):
    """Seconds the literal numpy evaluation takes for every pulsar and all sources, scaled from the first n_sub."""
    offs = case["offs"]
    t0 = time.perf_counter()
    for s in case["src"][:n_sub]:
        kw = dict(zip(R.COLUMNS, s))
        for p in range(len(offs) - 1):
            R.cw_delay_numpy(case["toas"][offs[p]:offs[p + 1]], case["pos"][p], case["pdist"][p], **kw)
    return (time.perf_counter() - t0) * len(case["src"]) / n_sub


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--numpy-sources", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cw_bench.json"))
    a = ap.parse_args()
    if a.calls < 10:
        ap.error("--calls must be >= 10")
    if _capi.build_flags() & _capi.BUILD_DEBUG:
        sys.exit("bench_cw: the debug build is not for measurements")
    ctx = _capi.Context(0)
    ctx.set_option(_capi.OPT_PROFILE, 1)
    rng = np.random.default_rng(11)
    result = {"calls": a.calls, "warmup": a.warmup}
    case = make_case(rng, 100, 2000, 4096, 0.0)  # one set of pulsars, TOAs and sources: only the pulsar term switches
    for name, psrterm in (("a_c2_4096src_earth_term", 0.0), ("a_c2_4096src_pulsar_term", 1.0)):
        case["src"][:, 8] = psrterm
        res, _ = measure(ctx, case, [0], a.calls, a.warmup)
        res[0]["numpy_s_scaled"] = numpy_time(case, a.numpy_sources)
        result[name] = res[0]
    case = make_case(rng, 25, 100, 10000, np.arange(10000) % 2)
    res, outs = measure(ctx, case, [0, 1], a.calls, a.warmup)
    scale = np.max(np.abs(outs[1]))
    result["b_25x100_10000src"] = {
        "auto": res[0], "forced_1": res[1], "numpy_s_scaled": numpy_time(case, a.numpy_sources),
        "auto_vs_forced_1_max_abs_diff_over_peak": float(np.max(np.abs(outs[0] - outs[1])) / scale)}
    spread = max(res[0]["kernel_ms_spread"], res[1]["kernel_ms_spread"])
    ok = res[0]["kernel_ms_median"] <= res[1]["kernel_ms_median"] + spread
    result["b_auto_not_slower_than_forced_1"] = bool(ok)
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result, indent=1))
    if not ok:
        sys.exit("bench_cw: the auto split is slower than one split by more than the run-to-run spread")


if __name__ == "__main__":
    main()
