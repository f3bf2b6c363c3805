"""bench.py --dump-outputs on a small C2 / C3 array: the files hold what the last timed step computed (the dumped
realizations' own sums equal the device checksums of the same step, which the line's `checksum` totals), two runs
with the same arguments write identical files, and --steps sets the number of timed steps (the last step's block
moves with it)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--npsr", "12", "--ntoa", "300", "--real", "192", "--warmup", "1"]


def _run(args, out_dir):
    env = {k: v for k, v in os.environ.items() if not k.startswith("FPTA_") and k not in ("WORLD_SIZE", "RANK",
                                                                                         "LOCAL_RANK")}
    res = subprocess.run([sys.executable, "bench.py"] + args + ["--dump-outputs", str(out_dir)], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=110)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0]), {f: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


@pytest.fixture(scope="module")
def c2_runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump")
    return [_run(SMALL + ["--steps", s], d / name) for s, name in (("2", "a"), ("2", "b"), ("3", "c"))]


def test_c2_dump_holds_the_last_step(c2_runs):
    line, out = c2_runs[0]
    assert line["steps"] == 2 and not line["full"] and line["ms_per_step"] > 0
    assert line["roofline_exact"] is None and line["pcie_inclusive"] is None and line["cpu_baseline"] is None
    assert not {"c3", "c5", "c4_per_gpu"} & set(line)
    assert sorted(out) == ["checksums.npy", "residual_cols.npy", "residual_rows.npy", "residuals.npy"]
    assert all(a.dtype == np.float64 for a in out.values())
    res, sums = out["residuals.npy"], out["checksums.npy"]
    assert res.shape == (192, 12 * 300) and sums.shape == (192, 2)  # 5.5 MB: the whole block
    np.testing.assert_array_equal(out["residual_rows.npy"], np.arange(192))
    assert np.all(np.isfinite(res)) and np.all(res.std(axis=1) > 0)
    # fp64 sums of 3600 terms in another order: 3600 eps relative to the sum of magnitudes bounds the difference
    tol = 3600 * np.finfo(float).eps
    np.testing.assert_allclose(res.sum(axis=1), sums[:, 0], rtol=0, atol=tol * np.abs(res).sum(axis=1).max())
    np.testing.assert_allclose((res ** 2).sum(axis=1), sums[:, 1], rtol=tol)
    assert line["n_checksums"] == 192
    np.testing.assert_allclose(line["checksum"], sums[:, 1].sum(), rtol=1e-13)


def test_c2_dump_repeats_and_follows_steps(c2_runs):
    (_, a), (_, b), (line_c, c) = c2_runs
    for f in a:
        np.testing.assert_array_equal(a[f], b[f])
    # one more timed step: its block holds the next 192 realizations, not the same ones again
    assert line_c["steps"] == 3
    assert not np.array_equal(a["residuals.npy"], c["residuals.npy"])
    assert c["residuals.npy"].shape == a["residuals.npy"].shape


def test_c3_dump_is_the_jobs_checksums(tmp_path):
    line, out = _run(["--gpus", "1", "--config", "c3", "--npsr", "12", "--ntoa", "300", "--c3-real", "700",
                      "--c3-batch", "256", "--steps", "1", "--warmup", "1"], tmp_path / "c3")
    assert sorted(out) == ["checksums.npy"]
    sums = out["checksums.npy"]
    assert sums.dtype == np.float64 and sums.shape == (700, 2) and np.all(sums[:, 1] > 0)
    assert line["n_checksums"] == 700
    np.testing.assert_allclose(line["checksum"], sums[:, 1].sum(), rtol=1e-13)
