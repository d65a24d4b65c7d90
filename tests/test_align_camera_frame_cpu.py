"""The premise of tests/test_align_camera_frame_gpu.py: with the large extrinsics of tests/camera_frame_cases.py a kernel
that hands out its normal equations in the wrong frame CANNOT pass the parity tolerance.  Oracle and NumPy only.

The alignment kernel sums rotation-free camera-frame rows and rotates the sums once per pass (H = Q H' Q^T, g = Q g').  For
each mistake that change invites -- the rotation forgotten, tau left out of X', R_imu_cam and R_cam_imu exchanged -- the
sums such a kernel would produce are W H W^T, W g of the true ones (camera_frame_cases.wrong_frames).  They must differ
from the oracle's H, g by at least 1e3 x TOL_HG of the largest entry, the tolerance the GPU tests compare at."""
import numpy as np
import pytest

from svo_pro_universal_amd import _capi as capi, synth

import camera_frame_cases as cfc
import helpers

MARGIN = 1e3


@pytest.fixture(scope="module")
def problem(oracle_lib):
    sc = cfc.scene(7100, n=300, P=4, border_features=20)
    ref, cur = helpers.scene_pyramids(oracle_lib, sc, 5)
    return sc, oracle_lib.problem_from_scenes([(sc, ref, cur)])


def test_the_extrinsics_are_large_and_consistent(problem):
    sc, _ = problem
    q = sc.T_cam_imu.q
    assert abs(2.0 * np.arccos(abs(q[0])) - 0.6) < 1e-12 and abs(np.linalg.norm(sc.T_cam_imu.t) - 0.3) < 1e-12
    I = sc.T_imu_cam * sc.T_cam_imu
    assert np.abs(I.R() - np.eye(3)).max() < 1e-15 and np.abs(I.t).max() < 1e-15


@pytest.mark.parametrize("level", [4, 0])
@pytest.mark.parametrize("illum", [0, 1])
def test_a_wrong_frame_is_far_outside_the_tolerance(oracle_lib, problem, level, illum):
    sc, opb = problem
    opt = capi.default_align_options(patch_size=4, min_level=0, estimate_illumination_gain=illum, estimate_illumination_offset=illum)
    H, g, chi2, n_meas, vis = oracle_lib.sparse_align_evaluate(opt, opb, level)
    assert n_meas > 0 and np.abs(H).max() > 0 and np.abs(g).max() > 0
    for name, W in sorted(cfc.wrong_frames(sc, 8).items()):
        dH = np.abs(W @ H @ W.T - H).max() / (helpers.TOL_HG * np.abs(H).max())
        dg = np.abs(W @ g - g).max() / (helpers.TOL_HG * np.abs(g).max())
        print("[camera frame] level %d illum %d %-9s: H off by %.3g x TOL_HG, g by %.3g x TOL_HG" % (level, illum, name, dH, dg))
        assert dH >= MARGIN and dg >= MARGIN, (name, dH, dg)


def test_the_rows_are_the_rotated_camera_frame_rows(problem):
    """... and the algebra the kernel rests on, row by row in NumPy: the reference's row [B0, p x B0], B0 = R_imu_cam alpha,
    p = T_imu_cam xyz_ref (frame.h:342-357), is blockdiag(R_imu_cam, R_imu_cam) [alpha, X' x alpha] with X' = xyz_ref + tau,
    tau = R_cam_imu t_imu_cam -- and is none of the three mistakes' rows."""
    sc, _ = problem
    R_ic, t_ic = sc.T_imu_cam.R(), np.asarray(sc.T_imu_cam.t, np.float64)
    tau = R_ic.T @ t_ic
    Q = cfc.blockdiag(R_ic, 6)
    rng = np.random.RandomState(5)
    for _ in range(20):
        X = rng.uniform(-1.0, 1.0, 3) + [0.0, 0.0, 3.0]
        alpha = rng.normal(size=3)
        B0, p = R_ic @ alpha, R_ic @ X + t_ic
        a = np.concatenate([B0, np.cross(p, B0)])
        a_cam = np.concatenate([alpha, np.cross(X + tau, alpha)])
        assert np.abs(Q @ a_cam - a).max() <= 1e-14 * np.abs(a).max()
        for name, W in cfc.wrong_frames(sc, 6).items():
            assert np.abs(W @ a - a).max() > 1e-3 * np.abs(a).max(), name
