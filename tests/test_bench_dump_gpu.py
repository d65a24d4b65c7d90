"""bench.py --dump-outputs on the device: the last timed step's alignment results as DIR/<field>.npy, float64, one row per
frame pair; two runs with the same arguments give the same inputs and therefore the same outputs, bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 64


def _bench(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--problems", str(B), "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_dump_outputs_writes_the_last_step_and_repeats_bit_for_bit(tmp_path):
    d1, d2 = tmp_path / "a", tmp_path / "b"
    line = _bench(d1)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["config"]["frame_pairs_per_gpu"] == B
    for k in ("cpu_baseline", "secondary", "step_of_1024"):   # --full only
        assert k not in line, k
    _bench(d2)
    names = sorted(os.listdir(d1))
    assert names == sorted(os.listdir(d2))
    assert {"T_icur_iref.npy", "status.npy", "n_fts_to_track.npy", "iters.npy", "chi2.npy"} <= set(names)
    total = 0
    for n in names:
        a, b = np.load(d1 / n), np.load(d2 / n)
        assert a.dtype == np.float64 and a.shape[0] == B, n
        assert np.array_equal(a, b), n
        total += a.nbytes
    assert total <= 64 << 20
    T = np.load(d1 / "T_icur_iref.npy")
    assert T.shape == (B, 7) and np.allclose(np.linalg.norm(T[:, :4], axis=1), 1.0)
    # the dumped results are the ones the line's figures were computed from
    n_fts = np.load(d1 / "n_fts_to_track.npy")
    assert (n_fts > 0).all()
    assert np.load(d1 / "n_patch_iters.npy").sum() == line["patch_iterations_per_step"]
    assert int((np.load(d1 / "status.npy") != 0).sum()) == line["solver_failures"]
    patches_per_step = line["value"] * line["ms_per_step"] * 1e-3    # value = patches x steps / elapsed, ms_per_step = elapsed / steps
    assert abs(n_fts.sum() - patches_per_step) <= 1e-6 * patches_per_step
