"""Times the continuous-wave injection into a resident batch block (k_cw_block, fpta_batch_cw_accumulate) on the GPU
against the drop-in kernels (fpta_cw_accumulate) doing the same number of waveform evaluations.

  python tools/bench_cw_batch.py [--calls 7] [--warmup 2] [--out profiles/cw_batch_bench.json]

Shape: the C2 TOA layout (100 pulsars x 2000 TOAs), a block of R = 128 realizations, S = 64 sources per realization
(a different population in each): 128 x 64 x 200000 = 1.64e9 source x TOA pairs. The yardstick is fpta_cw_accumulate on
the same layout with 8192 sources of the same kind: the same 1.64e9 pairs, in one piece (3125 waves). Both are run
once with Earth terms only (one waveform evaluation per pair) and once with the pulsar term (two), alternating call by
call on the same card; kernel time is the HIP-event time fpta_kernel_stats books under FPTA_K_CW, one entry per
call, --calls timed calls after --warmup of each. Figures are medians, the spread is max - min. The expectation is a
ratio <= 1.10: on top of the evaluations the new kernel reads and writes the block once (0.4 GB) and makes the
(pulsar, source) pair constants once per (slab, source).

Also recorded: the host time of the validation and per-source constants of the R x S sources (a call whose last
source is refused runs exactly that and nothing else), the one-table mode (the drop-in kernels on 64 sources into a
vector, then k_cw_bcast) beside the drop-in call on the same 64 sources and a device-to-device copy of the block, and
the share of the fp64 vector pipe: evaluations/s x the fp64 VALU instructions per evaluation (counted in the gfx950 ISA
of the shipped kernel, --fp64-per-pair for both terms of one source) x 2 FLOP over 70 TFLOP/s. Needs a GPU: there is no
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

from fakepta_amd import _capi, cw  # noqa: E402
from tools.bench_tm_project import Hip, stats  # noqa: E402

YEAR = 365.25 * 86400.0
N_PSR, N_TOA, R, S = 100, 2000, 128, 64
FMA_CEILING = 70e12  # fp64 vector FMA, FLOP/s


def population(rng, n, psrterm):
    """n sources a PTA might see: 10^8 .. 10^9.5 Msun at 1.6 .. 16 nHz, far from coalescence over 15 years."""
    return np.stack([rng.uniform(-1, 1, n), rng.uniform(0, 2 * np.pi, n), rng.uniform(-1, 1, n), rng.uniform(8, 9.5, n),
                     rng.uniform(-8.8, -7.8, n), rng.uniform(-15, -14, n), rng.uniform(0, 2 * np.pi, n),
                     rng.uniform(0, np.pi, n), np.full(n, float(psrterm))], axis=1)


def timed(ctx, call):
    ctx.reset_stats()
    call()
    ctx.synchronize()
    n, ms = ctx.kernel_stats(_capi.K_CW)
    assert n == 1, n
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--fp64-per-pair", type=int, default=539,
                    help="fp64 VALU instructions of one trip of k_cw_block's source loop, both terms (gfx950 ISA)")
    ap.add_argument("--insts-per-pair", type=int, default=764, help="all instructions of that trip")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cw_batch_bench.json"))
    a = ap.parse_args()
    if a.calls < 5 or a.warmup < 2:
        ap.error("--calls must be >= 5 and --warmup >= 2 for a measurement")
    if _capi.build_flags() & _capi.BUILD_DEBUG:
        sys.exit("bench_cw_batch: the debug build is not for measurements")
    ctx = _capi.get_context()
    ctx.set_option(_capi.OPT_PROFILE, 1)
    rng = np.random.default_rng(2)
    offs = np.arange(N_PSR + 1, dtype=np.int64) * N_TOA
    toas = np.concatenate([np.sort(rng.uniform(0.0, 15 * YEAR, N_TOA)) for _ in range(N_PSR)])
    nu = np.full(N_PSR * N_TOA, 1400.0)
    v = rng.normal(size=(N_PSR, 3))
    pos = v / np.linalg.norm(v, axis=1)[:, None]
    L = np.array([cw.light_seconds((d, 0.0)) for d in rng.uniform(0.5, 2.0, N_PSR)])
    ctx.batch_set_toas(offs, toas, nu)
    f = np.tile(np.arange(1, 11) / (15 * YEAR), (N_PSR, 1))
    ctx.batch_add_signal(0, f, np.full(f.shape, 1e-7))
    ctx.batch_synth(1, 0, R, to_host=False)
    ptr, ld, nr = ctx.batch_device_out()
    assert (ld, nr) == (N_PSR * N_TOA, R)
    n_pairs = R * S * N_PSR * N_TOA
    so = np.arange(R + 1, dtype=np.int64) * S
    res = np.zeros(N_PSR * N_TOA)
    result = dict(shape=dict(n_psr=N_PSR, n_toa_per_psr=N_TOA, realizations=R, sources_per_realization=S,
                             drop_in_sources=R * S, source_toa_pairs=n_pairs, block_bytes=8 * ld * nr),
                  calls=a.calls, warmup=a.warmup,
                  isa=dict(fp64_valu_per_pair_both_terms=a.fp64_per_pair, instructions_per_pair_both_terms=a.insts_per_pair))
    for name, psrterm in (("earth_term", 0), ("pulsar_term", 1)):
        src = population(rng, R * S, psrterm)
        block, drop = [], []
        for i in range(a.warmup + a.calls):  # alternating, call by call
            b = timed(ctx, lambda: ctx.batch_cw_accumulate(pos, L, R, so, src))
            d = timed(ctx, lambda: ctx.cw_accumulate(offs, toas, pos, L, src, res))
            if i >= a.warmup:
                block.append(b)
                drop.append(d)
        evals = n_pairs * (1 + psrterm)
        r = dict(k_cw_block=stats(block), drop_in_kernels=stats(drop))
        r["ratio_block_over_drop_in"] = r["k_cw_block"]["ms_median"] / r["drop_in_kernels"]["ms_median"]
        r["evaluations_per_s"] = evals / (r["k_cw_block"]["ms_median"] * 1e-3)
        r["drop_in_evaluations_per_s"] = evals / (r["drop_in_kernels"]["ms_median"] * 1e-3)
        # fp64 instructions per evaluation: half of a both-terms trip; every one counted as an FMA issue slot (2 FLOP)
        r["fp64_valu_per_s"] = r["evaluations_per_s"] * (a.fp64_per_pair / 2)
        r["fp64_issue_share_of_70tf_fma_ceiling"] = r["fp64_valu_per_s"] * 2 / FMA_CEILING
        bad = src.copy()
        bad[-1, 4] = np.nan  # refused at the very last source: validation and constants of all R x S, nothing else
        host = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            try:
                ctx.batch_cw_accumulate(pos, L, R, so, bad)
            except _capi.FptaError:
                host.append((time.perf_counter() - t0) * 1e3)
        assert len(host) == a.calls
        r["host_validation_and_constants"] = stats(host)
        result[name] = r
        print(name, json.dumps(r), flush=True)
    # one table for every realization: the drop-in kernels on S sources into a vector, then k_cw_bcast over the block
    src = population(rng, S, 1)
    one = np.array([0, S], dtype=np.int64)
    hip = Hip()
    dst = hip.malloc(8 * ld * nr)
    ea, eb = hip.event(), hip.event()
    shared, drop, copy = [], [], []
    for i in range(a.warmup + a.calls):
        s = timed(ctx, lambda: ctx.batch_cw_accumulate(pos, L, 1, one, src))
        d = timed(ctx, lambda: ctx.cw_accumulate(offs, toas, pos, L, src, res))
        c = hip.copy_ms(dst, ptr, 8 * ld * nr, ea, eb)
        if i >= a.warmup:
            shared.append(s)
            drop.append(d)
            copy.append(c)
    hip.free(dst)
    r = dict(sources=S, shared_table_call=stats(shared), drop_in_kernels_same_sources=stats(drop),
             device_to_device_copy=stats(copy))
    r["bcast_ms_by_difference"] = r["shared_table_call"]["ms_median"] - r["drop_in_kernels_same_sources"]["ms_median"]
    r["bcast_over_copy"] = r["bcast_ms_by_difference"] / r["device_to_device_copy"]["ms_median"]
    result["shared_table"] = r
    print("shared_table", json.dumps(r), flush=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
