"""Writes tests/golden/g12_orf.npz: 50-digit mpmath truths of the anisotropic ORF (tests/orf_reference.py).

  python tools/gen_orf_golden.py [--out tests/golden/g12_orf.npz]

  theta_<nside>, phi_<nside>   pixel centres of nside 1, 2, 3, 4 and 8, rounded once from mpmath
  <case>_pos, _maps, _truth    pulsar positions [P, 3], maps [M, npix] with values in [0.2, 2], ORFs [M, P, P] for the
                               cases p5n2 (P = 5, nside 2, 3 maps), p5n4 (P = 5, nside 4) and p17n8 (P = 17, nside 8)
  <case>_err64                 max |fp64 numpy model - truth| per map, on the generating host
The positions are drawn by rejection so that min over (pulsar, pixel) of D >= 1e-3 (orf_reference.draw_positions).
Data only: every number comes from the definition in include/fakepta_amd.h, none from a HEALPix library."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import orf_reference as R  # noqa: E402

NSIDES = (1, 2, 3, 4, 8)
CASES = (("p5n2", 5, 2, 3), ("p5n4", 5, 4, 1), ("p17n8", 17, 8, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g12_orf.npz"))
    a = ap.parse_args()
    data = {"nsides": np.array(NSIDES), "case_names": np.array([c[0] for c in CASES])}
    for nside in NSIDES:
        data[f"theta_{nside}"], data[f"phi_{nside}"] = R.pix2ang_mp(nside)
    rng = np.random.default_rng(20261019)
    for name, n_psr, nside, n_map in CASES:
        pos = R.draw_positions(rng, n_psr, nside)
        maps = R.draw_maps(rng, n_map, nside)
        truth = R.orf_mp(pos, maps)
        err = np.max(np.abs(R.orf_numpy(pos, maps) - truth), axis=(1, 2))
        print(f"{name}: min D {R.min_d(pos, nside):.3e}, fp64 model error / peak "
              f"{np.max(err) / np.max(np.abs(truth)):.2e}")
        data.update({f"{name}_pos": pos, f"{name}_maps": maps, f"{name}_truth": truth, f"{name}_err64": err})
    np.savez_compressed(a.out, **data)
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
