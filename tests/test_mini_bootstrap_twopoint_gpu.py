"""Integration: the mono chain started from images and a gyroscope's rotation alone (tools/svoh_mini_frontend.cpp,
SVOH_MINI_BOOTSTRAP=1 with init_method: TwoPoint): TwoPointInitHip (host/svo_hip_init.h, translation_ransac_kernel in
csrc/init.hip) in front of the per-frame chain, on the rendered sequence of tests/test_mini_bootstrap_gpu.py with the
rotation priors written from the true poses.  The bars are those of test_bootstrap_from_images_alone there."""
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
N_FRAMES = 30
INIT_MIN_INLIERS = 70                            # the factory's default, which the parameter file leaves alone


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """30 frames of 752x480: the camera slides sideways along a plane about 5.6 m away, 5 cm a frame (about 4 px of
    disparity a frame: the default init_min_disparity of 40 px is reached around the tenth frame).  The camera is the
    body (T_B_C = I), so mav0/imu_prior.csv holds R_cam(k)_cam(k-1) of the true poses."""
    root = tmp_path_factory.mktemp("bootstrap_twopoint")
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
    listing = "#timestamp [ns],filename\n" + "".join("%d,%d.png\n" % (t, t) for t in stamps)
    (root / "ds" / "mav0" / "cam0" / "data.csv").write_text(listing)
    rel = [(1.0, 0.0, 0.0, 0.0)] + [tuple((poses[k].inverse() * poses[k - 1]).q) for k in range(1, N_FRAMES)]
    (root / "ds" / "mav0" / "imu_prior.csv").write_text("# qw qx qy qz of R_imu(k)_imu(k-1)\n" + "".join("%.17g %.17g %.17g %.17g\n" % q for q in rel))
    # the same images without any source of a rotation prior
    bare = root / "ds_bare" / "mav0" / "cam0"
    bare.mkdir(parents=True)
    (bare / "data.csv").write_text(listing)
    os.symlink(str(data), str(bare / "data"))
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
    (root / "params.yaml").write_text("max_fts: 180\ngrid_size: 30\nn_pyr_levels: 3\ndetector_threshold_secondary: 100\n"
                                      "use_threaded_depthfilter: False\nimg_align_max_level: 4\nimg_align_min_level: 2\n"
                                      "init_method: TwoPoint\n")
    d = float(np.mean(sc.depth))          # the scene's true mean depth: the depth prior
    T0 = poses[0].inverse().as7()

    def command(out_name, ds="ds"):
        out_dir = root / out_name
        out_dir.mkdir(exist_ok=True)
        return ([TOOL, str(root / ds), str(root / "calib.yaml"), str(root / "params.yaml"), str(out_dir)]
                + ["%.17g" % v for v in T0] + ["%.6f" % (0.5 * d), "%.6f" % d, "%.6f" % (2.0 * d)]), out_dir
    return dict(command=command, poses=poses, stamps=stamps, depth=d)


def run(cmd):
    return subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, SVOH_MINI_BOOTSTRAP="1"), timeout=300)


@pytest.fixture(scope="module")
def first_run(dataset):
    cmd, out_dir = dataset["command"]("out_twopoint_a")
    return run(cmd), out_dir


def test_bootstrap_from_images_and_rotation_priors(dataset, first_run):
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
    cmd, out_b = dataset["command"]("out_twopoint_b")
    r2 = run(cmd)
    assert r1.returncode == 0 and r2.returncode == 0, r1.stderr + r2.stderr
    assert (out_a / "trajectory.txt").read_bytes() == (out_b / "trajectory.txt").read_bytes() and (out_a / "trajectory.txt").stat().st_size > 0

    def untimed(path):   # bootstrap.csv without its last column, the kernel's time
        return [line.rsplit(",", 1)[0] for line in path.read_text().splitlines()]
    assert untimed(out_a / "bootstrap.csv") == untimed(out_b / "bootstrap.csv")


def test_without_a_rotation_prior_the_tool_refuses(dataset):
    cmd, out_dir = dataset["command"]("out_no_prior", ds="ds_bare")
    r = run(cmd)
    assert r.returncode == 1 and "rotation prior" in r.stderr, r.stdout + r.stderr
    assert not (out_dir / "bootstrap.csv").exists()
