"""Integration: the mono chain started from images alone (tools/svoh_mini_frontend.cpp, SVOH_MINI_BOOTSTRAP=1): the
homography initialiser (host/svo_hip_init.h, csrc/init.hip) in front of the per-frame chain, on a rendered one-plane
EuRoC-layout sequence of its own whose steps are sideways and large enough for the initialiser's disparity threshold.
The bars on the trajectory and the counters are those of tests/test_mini_frontend_gpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from svo_pro_universal_amd import synth
from test_io_cpu import write_png

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
TOOL = os.path.join(ROOT, "svo_pro_universal_amd", "host", "svoh_mini_frontend")
COUNTER_COLS = [0, 1, 2, 3, 4, 5, 6, 14, 15]   # frontend.csv without its timing columns
N_FRAMES = 30
INIT_MIN_INLIERS = 70                            # the factory's default, which the parameter file leaves alone


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """30 frames of 752x480: the camera slides sideways along a plane about 5.6 m away, 5 cm a frame (about 4 px of
    disparity a frame: the default init_min_disparity of 40 px is reached around the tenth frame)."""
    root = tmp_path_factory.mktemp("bootstrap")
    cam = synth.Camera.euroc_like(752, 480)
    sc = synth.make_align_scene(160, n_features=8, cam=cam, rot_deg=(0.3, 0.5), trans_m=(0.015, 0.025))
    step = synth.SE3(synth.quat_from_axis_angle([0.3, 1.0, 0.2], np.deg2rad(0.08)), (0.048, 0.012, 0.004))
    poses = [sc.T_w_ref]
    for k in range(1, N_FRAMES):
        poses.append(poses[-1] * step)
    data = root / "ds" / "mav0" / "cam0" / "data"
    data.mkdir(parents=True)
    stamps = [1403636579763555584 + 50000000 * k for k in range(N_FRAMES)]
    for k, T in enumerate(poses):
        write_png(str(data / ("%d.png" % stamps[k])), synth.render(cam, T, sc.plane, sc.tex), chunk=65536)
    (root / "ds" / "mav0" / "cam0" / "data.csv").write_text("#timestamp [ns],filename\n" + "".join("%d,%d.png\n" % (t, t) for t in stamps))
    (root / "calib.yaml").write_text("""cameras:
- camera:
    label: cam0
    image_height: %d
    image_width: %d
    type: pinhole
    intrinsics:
      data: [%.17g, %.17g, %.17g, %.17g]
    distortion:
      type: radial-tangential
      parameters:
        data: [%.17g, %.17g, %.17g, %.17g]
  T_B_C:
    data: [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]
""" % ((cam.height, cam.width, cam.fx, cam.fy, cam.cx, cam.cy) + tuple(cam.dist)))
    base = ("max_fts: 180\ngrid_size: 30\nn_pyr_levels: 3\ndetector_threshold_secondary: 100\n"
            "use_threaded_depthfilter: False\nimg_align_max_level: 4\nimg_align_min_level: 2\n")
    (root / "params.yaml").write_text(base + "init_method: Homography\n")
    (root / "params_fivepoint.yaml").write_text(base)
    d = float(np.mean(sc.depth))          # the scene's true mean depth: the depth prior
    T0 = poses[0].inverse().as7()

    def command(out_name, params="params.yaml", extra=()):
        out_dir = root / out_name
        out_dir.mkdir(exist_ok=True)
        return ([TOOL, str(root / "ds"), str(root / "calib.yaml"), str(root / params), str(out_dir)]
                + ["%.17g" % v for v in T0] + ["%.6f" % (0.5 * d), "%.6f" % d, "%.6f" % (2.0 * d)] + list(extra)), out_dir
    return dict(command=command, poses=poses, stamps=stamps, depth=d)


def run(cmd, bootstrap):
    env = dict(os.environ)
    env.pop("SVOH_MINI_BOOTSTRAP", None)
    if bootstrap:
        env["SVOH_MINI_BOOTSTRAP"] = "1"
    return subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)


def test_bootstrap_from_images_alone(dataset):
    import ate
    cmd, out_dir = dataset["command"]("out_bootstrap")
    r = run(cmd, True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [line.split(",") for line in (out_dir / "bootstrap.csv").read_text().splitlines()]
    assert rows[0] == ["frame", "result", "n_tracked", "disparity", "n_inliers", "n_triangulated", "scale", "ms_ransac"]
    rows = rows[1:]
    print("\n".join(",".join(r_) for r_ in rows))
    results = [r_[1] for r_ in rows]
    assert results[-1] == "kSuccess" and results.count("kSuccess") == 1 and len(rows) >= 2
    assert all(x == "kTracking" for x in results[:-1])
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
    print("success at frame %d with %s triangulated points, scale %s; ATE rmse %.4f m over a %.3f m path (scale %.3f); from frame %d on: reprojected "
          "median %d, landmarks median %d, structure-optimised median %d; converged seeds at the end %d"
          % (k_success, rows[-1][5], rows[-1][6], res["rmse"], path_len, res["scale"], k_success + 5, int(np.median(late[:, 3])),
             int(np.median(late[:, 15])), int(np.median(late[:, 14])), int(fc[-1, 6])))
    assert res["n"] == len(want)
    assert res["rmse"] < 0.03 * path_len + 0.003
    assert 0.8 < res["scale"] < 1.25
    # the later frames track: the floors of the chain test, from five frames after the success on
    assert (late[:, 2] > 0).all()
    assert np.median(late[:, 3]) > 80
    assert np.median(late[:, 15]) > 40 and np.median(late[:, 14]) > 20
    assert fc[-1, 6] > 100


def test_without_the_switch_nothing_changes(dataset):
    outs = []
    for name in ("out_plain_a", "out_plain_b"):
        cmd, out_dir = dataset["command"](name)
        r = run(cmd, False)
        assert r.returncode == 0, r.stdout + r.stderr
        assert not (out_dir / "bootstrap.csv").exists()
        fc = np.loadtxt(str(out_dir / "frontend.csv"), delimiter=",", skiprows=1)
        outs.append(((out_dir / "trajectory.txt").read_bytes(), fc[:, COUNTER_COLS], r.stdout.split(",")[0]))
    assert outs[0][0] == outs[1][0] and len(outs[0][0]) > 0
    assert np.array_equal(outs[0][1], outs[1][1])
    assert outs[0][2] == outs[1][2] == "svoh_mini_frontend: %d frames" % N_FRAMES


def test_refusals(dataset):
    cmd, out_dir = dataset["command"]("out_refused", params="params_fivepoint.yaml")
    r = run(cmd, True)
    assert r.returncode == 1 and "FivePoint" in r.stderr and not (out_dir / "bootstrap.csv").exists()
    cmd, out_dir = dataset["command"]("out_refused_lockstep", extra=["30", "8", "2", "lockstep"])
    r = run(cmd, True)
    assert r.returncode == 1 and "lock-step" in r.stderr
