"""Times the timing-model projection kernel (k_tm_project, fpta_batch_project) on the GPU against a device-to-device
copy of the same block.

  python tools/bench_tm_project.py [--calls 20] [--warmup 3] [--out profiles/tm_project_bench.json] [--skip-c4]
                                   [--only c2|c4] [--no-copy]

Shapes: C2 (100 pulsars x 2000 TOAs, 1024 realizations, 1.6 GB) and the per-GPU share of C4 (1000 x 10^4 TOAs, 256
realizations, 20 GB), make_Mmat's eight columns on three-band frequencies, white-noise weights. The block is white
noise (the projection's traffic does not depend on what the block holds).

Kernel time is the HIP-event time of the launch on the context stream (fpta_kernel_stats, FPTA_K_DENSE), one launch
per call, --calls launches after --warmup. The copy is hipMemcpyAsync device to device of the whole block into a
second buffer, timed by HIP events in the same process, on the same card and in the same run: the practical
one-read-one-write roof. The figures are medians; the spread is max - min. The aim is a ratio <= 1.5: a two-sweep
kernel whose re-read missed every cache would move three block sizes against the copy's two. --only and --no-copy run
one shape without the copy (for a counter collection of the kernel alone). Needs a GPU: there is no fallback."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from fakepta_amd import _capi  # noqa: E402
from tests import tm_reference as T  # noqa: E402

YEAR = 365.25 * 86400.0
SHAPES = {"c2": ("c2_100x2000_r1024", 100, 2000, 1024), "c4": ("c4_per_gpu_1000x10000_r256", 1000, 10000, 256)}


class Hip:
    """The few calls of the HIP runtime the copy needs, on the runtime the library itself maps."""

    def __init__(self):
        # the runtime libfakepta_amd.so has mapped into this process, whatever its version; else the loader's choice
        path = "libamdhip64.so"
        with open("/proc/self/maps") as fh:
            for line in fh:
                if "libamdhip64.so" in line:
                    path = line.split()[-1]
                    break
        self.lib = ctypes.CDLL(path)
        self.lib.hipGetErrorString.restype = ctypes.c_char_p

    def check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: {self.lib.hipGetErrorString(rc).decode()}")

    def malloc(self, n_bytes):
        p = ctypes.c_void_p()
        self.check(self.lib.hipMalloc(ctypes.byref(p), ctypes.c_size_t(n_bytes)), "hipMalloc")
        return p

    def free(self, p):
        self.check(self.lib.hipFree(p), "hipFree")

    def event(self):
        e = ctypes.c_void_p()
        self.check(self.lib.hipEventCreate(ctypes.byref(e)), "hipEventCreate")
        return e

    def copy_ms(self, dst, src, n_bytes, a, b):
        """One device-to-device copy on the null stream between two events."""
        self.check(self.lib.hipEventRecord(a, None), "hipEventRecord")
        self.check(self.lib.hipMemcpyAsync(dst, ctypes.c_void_p(src), ctypes.c_size_t(n_bytes), 3, None),
                   "hipMemcpyAsync")  # 3: hipMemcpyDeviceToDevice
        self.check(self.lib.hipEventRecord(b, None), "hipEventRecord")
        self.check(self.lib.hipEventSynchronize(b), "hipEventSynchronize")
        ms = ctypes.c_float()
        self.check(self.lib.hipEventElapsedTime(ctypes.byref(ms), a, b), "hipEventElapsedTime")
        return float(ms.value)


def stats(v):
    v = np.array(v)
    return dict(ms_median=float(np.median(v)), ms_min=float(v.min()), ms_max=float(v.max()),
                ms_spread=float(v.max() - v.min()))


def run_shape(ctx, hip, name, n_psr, n_toa, R, calls, warmup, copy):
    rng = np.random.default_rng(n_psr)
    offs = np.arange(n_psr + 1, dtype=np.int64) * n_toa
    toas = np.concatenate([np.sort(rng.uniform(0.0, 15 * YEAR, n_toa)) for _ in range(n_psr)])
    nu = np.abs(rng.choice([800.0, 1400.0, 2500.0], size=n_psr * n_toa) + rng.normal(0, 10, n_psr * n_toa))
    sigma = rng.uniform(1e-7, 1e-6, n_psr * n_toa)
    M = np.concatenate([T.mmat(toas[offs[p]:offs[p + 1]], nu[offs[p]:offs[p + 1]]) for p in range(n_psr)])
    ctx.batch_set_toas(offs, toas, nu)
    ctx.batch_set_white(sigma)
    rank = ctx.batch_set_timing_model(M, weights=1 / sigma ** 2)
    assert np.all(rank == 8), rank
    ctx.batch_synth(1, 0, R, to_host=False)
    ptr, ld, nr = ctx.batch_device_out()
    n_bytes = 8 * ld * nr
    for _ in range(warmup):
        ctx.batch_project()
    ctx.synchronize()
    ker = []
    for _ in range(calls):
        ctx.reset_stats()
        ctx.batch_project()
        ctx.synchronize()
        n, ms = ctx.kernel_stats(_capi.K_DENSE)
        assert n == 1
        ker.append(ms)
    res = dict(n_psr=n_psr, n_toa_per_psr=n_toa, realizations=R, columns=8, block_bytes=int(n_bytes), calls=calls,
               warmup=warmup, kernel=stats(ker))
    res["kernel_gb_per_s_of_two_block_sizes"] = 2 * n_bytes / (res["kernel"]["ms_median"] * 1e-3) / 1e9
    if copy:
        dst = hip.malloc(n_bytes)
        a, b = hip.event(), hip.event()
        for _ in range(warmup):
            hip.copy_ms(dst, ptr, n_bytes, a, b)
        res["copy"] = stats([hip.copy_ms(dst, ptr, n_bytes, a, b) for _ in range(calls)])
        res["copy_gb_per_s"] = 2 * n_bytes / (res["copy"]["ms_median"] * 1e-3) / 1e9
        res["kernel_over_copy"] = res["kernel"]["ms_median"] / res["copy"]["ms_median"]
        hip.free(dst)
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-c4", action="store_true")
    ap.add_argument("--only", choices=sorted(SHAPES))
    ap.add_argument("--no-copy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tm_project_bench.json"))
    a = ap.parse_args()
    if a.calls < 1 or (a.calls < 20 and not a.no_copy):
        ap.error("--calls must be >= 20 for a measurement")
    if _capi.build_flags() & _capi.BUILD_DEBUG:
        sys.exit("bench_tm_project: the debug build is not for measurements")
    ctx = _capi.get_context()
    ctx.set_option(_capi.OPT_PROFILE, 1)
    hip = Hip()
    keys = [a.only] if a.only else ["c2"] + ([] if a.skip_c4 else ["c4"])
    result = {}
    for key in keys:
        name, n_psr, n_toa, R = SHAPES[key]
        result[name] = run_shape(ctx, hip, name, n_psr, n_toa, R, a.calls, a.warmup, not a.no_copy)
    if not a.no_copy:
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
        print("wrote", a.out)


if __name__ == "__main__":
    main()
