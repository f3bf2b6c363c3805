"""Writes tests/golden/g10_cw.npz, the fixture of the continuous-wave tests (tests/test_cw_host.py,
tests/test_gpu_cw.py). CPU only; needs mpmath.

  python tools/gen_cw_golden.py

Geometry: four pulsars of 1, 63, 257 and 70 TOAs (sorted uniform draws over 15 yr; the second pulsar's TOAs start at
MJD 53000 in seconds, so large epochs are covered), distinct distances. Ten sources from a fixed seed: five
(log10_mc, log10_fgw) pairs, each once without and once with the pulsar term. Stored: the inputs, truth[s] (the
definition in 60-digit mpmath, rounded to fp64), err_ref64[s] = max |literal fp64 numpy evaluation - truth[s]| (what
a plain fp64 implementation of the definition achieves: the tests' yardstick) and peak[s] = max |truth[s]|."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from fakepta import constants as const  # noqa: E402
from tests import cw_reference as R  # noqa: E402

N_TOA = (1, 63, 257, 70)
OFFSET_PSR, OFFSET_S = 1, 53000 * 86400.0
PAIRS = ((9.5, -7.5), (9.0, -8.0), (8.0, -8.5), (7.5, -7.0), (10.0, -8.8))


def main():
    rng = np.random.default_rng(20260410)
    span = 15 * const.yr
    toas = [np.sort(rng.uniform(0.0, span, n)) for n in N_TOA]
    toas[OFFSET_PSR] = toas[OFFSET_PSR] + OFFSET_S
    offs = np.concatenate([[0], np.cumsum(N_TOA)]).astype(np.int64)
    theta = np.arccos(rng.uniform(-1, 1, len(N_TOA)))
    phi = rng.uniform(0, 2 * np.pi, len(N_TOA))
    pos = np.array([[np.cos(p) * np.sin(t), np.sin(p) * np.sin(t), np.cos(t)] for t, p in zip(theta, phi)])
    pdist = np.array([[1.0, 0.2], [0.55, 0.11], [1.37, 0.05], [2.1, 0.4]])
    src = []
    for psrterm in (0.0, 1.0):
        for log10_mc, log10_fgw in PAIRS:
            src.append([rng.uniform(-1, 1), rng.uniform(0, 2 * np.pi), rng.uniform(-1, 1), log10_mc, log10_fgw,
                        rng.uniform(-14.5, -13.5), rng.uniform(0, 2 * np.pi), rng.uniform(0, np.pi), psrterm])
    src = np.array(src)
    tmax = max(t.max() for t in toas)
    for s in src:
        mc = 10 ** s[3] * const.Tsun
        K = 256 / 5 * mc ** (5 / 3) * (np.pi * 10 ** s[4]) ** (8 / 3)
        assert K * tmax < 1, (s, K * tmax)
    n = int(offs[-1])
    truth = np.empty((len(src), n))
    err = np.empty(len(src))
    for i, s in enumerate(src):
        kw = dict(zip(R.COLUMNS, s))
        ref = np.empty(n)
        for p in range(len(N_TOA)):
            sl = slice(offs[p], offs[p + 1])
            truth[i, sl] = R.cw_delay_mp(toas[p], pos[p], pdist[p], **kw)
            ref[sl] = R.cw_delay_numpy(toas[p], pos[p], pdist[p], **kw)
        err[i] = np.max(np.abs(ref - truth[i]))
        print(f"source {i}: peak {np.max(np.abs(truth[i])):.3e}  literal fp64 error {err[i]:.3e} "
              f"({err[i] / np.max(np.abs(truth[i])):.1e} of peak)")
    assert np.all(err > 0) and np.all(np.isfinite(truth))
    path = os.path.join(ROOT, "tests", "golden", "g10_cw.npz")
    np.savez(path, offs=offs, toas=np.concatenate(toas), theta=theta, phi=phi, pos=pos, pdist=pdist, src=src,
             truth=truth, err_ref64=err, peak=np.max(np.abs(truth), axis=1))
    print("wrote", path)


if __name__ == "__main__":
    main()
