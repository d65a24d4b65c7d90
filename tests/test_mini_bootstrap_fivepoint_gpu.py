"""Integration: the mono chain started from images alone by the default initialiser (tools/svoh_mini_frontend.cpp,
SVOH_MINI_BOOTSTRAP=2 with a parameter file that names no init_method, which is FivePoint): FivePointInitHip
(host/svo_hip_init.h, essential_ransac_kernel in csrc/essential.hip) in front of the per-frame chain, on the rendered
one-plane sequence of tests/test_mini_bootstrap_gpu.py.  The bars are those of test_bootstrap_from_images_alone there."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_mini_bootstrap_gpu import dataset, N_FRAMES, INIT_MIN_INLIERS   # noqa: F401 (dataset: the module's fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def run(cmd, level):
    return subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, SVOH_MINI_BOOTSTRAP=level), timeout=300)


@pytest.fixture(scope="module")
def first_run(dataset):
    cmd, out_dir = dataset["command"]("out_fivepoint_a", params="params_fivepoint.yaml")
    return run(cmd, "2"), out_dir


def test_bootstrap_from_images_alone_with_the_default_method(dataset, first_run):
    import ate
    r, out_dir = first_run
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [line.split(",") for line in (out_dir / "bootstrap.csv").read_text().splitlines()]
    assert rows[0] == ["frame", "result", "n_tracked", "disparity", "n_inliers", "n_triangulated", "scale", "ms_ransac"]
    rows = rows[1:]
    print("\n".join(",".join(r_) for r_ in rows))
    results = [r_[1] for r_ in rows]
    assert results[-1] == "kSuccess" and results.count("kSuccess") == 1 and len(rows) >= 2
    assert [int(r_[0]) for r_ in rows] == list(range(len(rows)))      # one line per initialiser call, from frame 0 on
    k_success = int(rows[-1][0])
    assert k_success <= 15
    assert int(rows[-1][5]) >= INIT_MIN_INLIERS and int(rows[-1][4]) >= INIT_MIN_INLIERS
    assert float(rows[-1][7]) > 0.0                                   # the estimator's kernel time was read

    # trajectory: the reference frame, then every frame from the success on
    est = ate.load_tum(str(out_dir / "trajectory.txt"))
    stamps, poses = dataset["stamps"], dataset["poses"]
    want = [stamps[0] * 1e-9] + [stamps[k] * 1e-9 for k in range(k_success, N_FRAMES)]
    assert len(est) == len(want) and np.abs(est[:, 0] - np.array(want)).max() < 1e-3
    gt = np.array([[stamps[k] * 1e-9] + list(T.t) + [T.q[1], T.q[2], T.q[3], T.q[0]] for k, T in enumerate(poses)])
    res = ate.ate(est, gt, with_scale=True, max_dt=1e-3)
    keep = [0] + list(range(k_success, N_FRAMES))
    path_len = float(np.linalg.norm(np.diff(gt[keep, 1:4], axis=0), axis=1).sum())
    fc = np.loadtxt(str(out_dir / "frontend.csv"), delimiter=",", skiprows=1)
    assert [int(v) for v in fc[:, 0]] == list(range(k_success, N_FRAMES))
    late = fc[fc[:, 0] >= k_success + 5]
    print("success at frame %d with %s inliers, %s triangulated points, scale %s, kernel %s ms; ATE rmse %.4f m over a %.3f m path (scale %.3f); from "
          "frame %d on: reprojected median %d, landmarks median %d, structure-optimised median %d; converged seeds at the end %d"
          % (k_success, rows[-1][4], rows[-1][5], rows[-1][6], rows[-1][7], res["rmse"], path_len, res["scale"], k_success + 5,
             int(np.median(late[:, 3])), int(np.median(late[:, 15])), int(np.median(late[:, 14])), int(fc[-1, 6])))
    assert res["n"] == len(want)
    assert res["rmse"] < 0.03 * path_len + 0.003
    assert 0.8 < res["scale"] < 1.25
    # the later frames track: the floors of the chain test, from five frames after the success on
    assert (late[:, 2] > 0).all()
    assert np.median(late[:, 3]) > 80
    assert np.median(late[:, 15]) > 40 and np.median(late[:, 14]) > 20
    assert fc[-1, 6] > 100


def test_two_runs_are_byte_identical(dataset, first_run):
    r1, out_a = first_run
    cmd, out_b = dataset["command"]("out_fivepoint_b", params="params_fivepoint.yaml")
    r2 = run(cmd, "2")
    assert r1.returncode == 0 and r2.returncode == 0, r1.stderr + r2.stderr
    assert (out_a / "trajectory.txt").read_bytes() == (out_b / "trajectory.txt").read_bytes() and (out_a / "trajectory.txt").stat().st_size > 0

    def untimed(path):   # bootstrap.csv without its last column, the kernel's time
        return [line.rsplit(",", 1)[0] for line in path.read_text().splitlines()]
    assert untimed(out_a / "bootstrap.csv") == untimed(out_b / "bootstrap.csv")


def test_under_the_value_one_the_refusal_is_unchanged_and_names_the_value_that_runs_it(dataset):
    cmd, out_dir = dataset["command"]("out_fivepoint_refused", params="params_fivepoint.yaml")
    r = run(cmd, "1")
    assert r.returncode == 1 and "FivePoint" in r.stderr and "SVOH_MINI_BOOTSTRAP=2" in r.stderr, r.stdout + r.stderr
    assert not (out_dir / "bootstrap.csv").exists()


def test_one_shot_stays_refused_under_either_value(dataset):
    cmd, out_dir = dataset["command"]("out_oneshot_refused", params="params_oneshot.yaml")
    params = cmd[3]
    with open(params, "w") as f:
        f.write(open(cmd[3].replace("params_oneshot.yaml", "params_fivepoint.yaml")).read() + "init_method: OneShot\n")
    for level in ("1", "2"):
        r = run(cmd, level)
        assert r.returncode == 1 and "OneShot" in r.stderr, r.stdout + r.stderr
    assert not (out_dir / "bootstrap.csv").exists()
