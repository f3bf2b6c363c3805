"""Times a C2 block drawn from per-realization spectra (fpta_batch_synth_spectra) against the fixed-spectrum block.

  python tools/bench_spectra.py [--rounds 7] [--steps 12] [--warmup 3] [--out profiles/spectra_bench.json]

Shape: bench.py's C2 array (100 pulsars x 2000 TOAs, RN30 + DM100 + HD GWB30), R = 1024 realizations per step, the
shipped options. Five variants alternate in one process, round by round:

  (a) plain synth                                   (b) power-law parameters [R, 2] on gw_common
  (c) amplitudes [R, N] on gw_common                (d) power-law parameters [R, P, 2] on red_noise
  (e) amplitudes [R, P, N] on red_noise

A round of a variant is bench.py's own measurement: --steps consecutive blocks queued back to back (consecutive
realizations, device-resident), one synchronisation at the end, wall time / steps; every variant is warmed with
--warmup steps first, as bench.py warms its steps. Steps are timed this way and not with one pair of events per
block because a block's work spans the context's streams and overlaps its neighbours' (FPTA_OPT_OVERLAP): only a
queue of steps shows what a step costs. Figures are medians over --rounds, the spread is max - min; (b) - (e) are
given as multiples of (a). The tables are made once (spectrum_tables' host time is reported on its own); host_ms is
the time a call keeps the host before it returns, which for a tabled block holds the upload of its tables, and
k_spectra_amp: their difference to (a)'s is the host-side cost of a tabled step. The route of each variant's last
block is reported: the interpolation kernel (the third template argument of k_grid_fused says whether it draws the
per-pulsar signals itself, gen_fused) and next_mix_used. Needs a GPU: there is no fallback."""
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
from fakepta_amd.batch import BatchSimulator  # noqa: E402
from fakepta_amd.spectra import spectrum_tables  # noqa: E402
from tools.bench_tm_project import stats  # noqa: E402

R, SEED = 1024, 1234


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectra_bench.json"))
    a = ap.parse_args()
    if a.rounds < 5 or a.warmup < 2 or a.steps < 4:
        ap.error("--rounds must be >= 5, --warmup >= 2 and --steps >= 4 for a measurement")
    if _capi.build_flags() & _capi.BUILD_DEBUG:
        sys.exit("bench_spectra: the debug build is not for measurements")
    import bench
    ctx = _capi.get_context()
    sim = BatchSimulator(bench.build_array(100, 2000, "c2"), white=False, ctx=ctx)
    P = len(sim.psrs)
    gw = [s for s in sim.segments if s["kind"] == 1][0]
    rn = [s for s in sim.segments if s["name"] == "red_noise"][0]
    rng = np.random.default_rng(3)
    f_gw, f_rn = np.asarray(gw["f"]), np.asarray(rn["f"])
    from fakepta.spectrum import powerlaw
    prior = dict(b={gw["name"]: dict(log10_A=rng.uniform(-15.5, -14.5, R), gamma=rng.uniform(2.0, 6.0, R))},
                 d={"red_noise": dict(log10_A=rng.uniform(-14.5, -13.5, (R, P)), gamma=rng.uniform(1.0, 5.0, (R, P)))})
    pb, pd = prior["b"][gw["name"]], prior["d"]["red_noise"]
    prior["c"] = {gw["name"]: dict(psd=powerlaw(f_gw[None, :], pb["log10_A"][:, None], pb["gamma"][:, None]))}
    prior["e"] = {"red_noise": dict(psd=powerlaw(f_rn[None], pd["log10_A"][..., None], pd["gamma"][..., None]))}
    tables, host_tables = {}, {}
    for v in "bcde":
        t0 = time.perf_counter()
        tables[v] = spectrum_tables(sim, prior[v], R)
        host_tables[v] = (time.perf_counter() - t0) * 1e3
    upload_bytes = {v: int(sum(t.nbytes for t in tables[v][3])) for v in "bcde"}
    state = dict(real0=0)

    def step(v):
        r0 = state["real0"]
        state["real0"] += R
        t0 = time.perf_counter()
        if v == "a":
            ctx.batch_synth(SEED, r0, R, to_host=False)
        else:
            ctx.batch_synth_spectra(SEED, r0, R, *tables[v], to_host=False)
        return (time.perf_counter() - t0) * 1e3

    def run(v, n):
        ctx.synchronize()
        t0 = time.perf_counter()
        host = [step(v) for _ in range(n)]
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n, float(np.median(host))

    ms = {v: [] for v in "abcde"}
    host = {v: [] for v in "abcde"}
    route = {}
    for v in "abcde":
        run(v, a.warmup)
    for _ in range(a.rounds):
        for v in "abcde":  # alternating, round by round
            run(v, 2)  # into the variant's own steady state (the pipeline's first block after another variant)
            m, h = run(v, a.steps)
            ms[v].append(m)
            host[v].append(h)
            gi = ctx.batch_grid_info()
            kern = gi["interp_kernel"]
            gen = kern.split(",")[2].strip() == "true" if kern.startswith("k_grid_fused<") else None
            route[v] = dict(interp_kernel=kern, gen_fused=gen, next_mix_used=bool(gi["next_mix_used"]),
                            next_mix_made=bool(gi["next_mix_made"]), path=int(gi["last_path"]))
    result = dict(shape=dict(n_psr=P, n_toa=int(sim.n_toa), realizations=R, signals=[s["name"] for s in sim.segments]),
                  rounds=a.rounds, steps=a.steps, warmup=a.warmup, variants={})
    base = stats(ms["a"])
    names = dict(a="plain synth", b="power law [R, 2] on the common signal", c="amplitudes [R, N] on the common signal",
                 d="power law [R, P, 2] on red noise", e="amplitudes [R, P, N] on red noise")
    for v in "abcde":
        r = dict(what=names[v], step=stats(ms[v]), host_per_call=stats(host[v]), route=route[v])
        r["step_over_plain"] = r["step"]["ms_median"] / base["ms_median"]
        if v != "a":
            r["upload_bytes"] = upload_bytes[v]
            r["spectrum_tables_host_ms"] = host_tables[v]
            r["host_per_call_minus_plain_ms"] = r["host_per_call"]["ms_median"] - stats(host["a"])["ms_median"]
        result["variants"][v] = r
        print(v, json.dumps(r), flush=True)
    result["plain_spread_over_median"] = base["ms_spread"] / base["ms_median"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
