"""Scenes with LARGE camera-IMU extrinsics for the tests of the alignment kernel's camera-frame normal equations
(tests/test_align_camera_frame_cpu.py, tests/test_align_camera_frame_gpu.py).

The kernel sums the normal equations of rotation-free Jacobian rows a' = [alpha, X' x alpha], X' = xyz_ref + tau, and
rotates the sums once per pass: H = Q H' Q^T, g = Q g', Q = blockdiag(R_imu_cam, R_imu_cam [, 1, 1]).  The scenes of
synth.make_align_scene turn the camera against the IMU by 0.05 rad and move it by 5 cm; a frame that is off by that
little can hide in a test.  Here: 0.6 rad about a generic axis and 0.3 m."""
import numpy as np

from svo_pro_universal_amd import synth

AXES = ([0.48, -0.62, 0.62], [-0.7, 0.3, 0.65])          # generic: no coordinate axis, no coordinate plane
LEVERS = ([0.2, -0.1, 0.2], [-0.12, 0.25, -0.116])       # 0.3 m each


def with_large_extrinsics(sc, k=0, angle=0.6):
    """Replace the extrinsics of a synth.AlignScene (before a problem is built from it).  The images and features are the
    camera's own and stay; what the alignment estimates, T_icur_iref, is the camera's motion seen from the new IMU."""
    lever = np.asarray(LEVERS[k], np.float64)
    sc.T_cam_imu = synth.SE3(synth.quat_from_axis_angle(AXES[k], angle), lever * (0.3 / np.linalg.norm(lever)))
    sc.T_imu_cam = sc.T_cam_imu.inverse()
    T_imu_world_ref = sc.T_imu_cam * sc.T_ref_f_w
    T_imu_world_cur = sc.T_imu_cam * sc.T_cur_f_w_gt
    sc.T_icur_iref_gt = T_imu_world_cur * T_imu_world_ref.inverse()
    return sc


def scene(seed, n=300, P=4, cam=None, k=0, **kw):
    return with_large_extrinsics(synth.make_align_scene(seed, n_features=n, patch_size=P, cam=cam, **kw), k)


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def blockdiag(R, D):
    Q = np.eye(D)
    Q[0:3, 0:3] = R
    Q[3:6, 3:6] = R
    return Q


def wrong_frames(sc, D):
    """name -> W (D x D): the sums a kernel with that mistake would hand out are W H W^T, W g for the true H, g.
      unrotated: the pass's rotation forgotten (H', g' themselves)                       W = Q^T
      no_tau:    X' = xyz_ref instead of xyz_ref + tau, i.e. a' = N (Q^T a),
                 N = [[I, 0], [-skew(tau), I]]                                              W = Q N Q^T
      exchanged: R_imu_cam and R_cam_imu exchanged in the rotation (Q^T applied to H')     W = Q^T Q^T"""
    R_ic = sc.T_imu_cam.R()
    tau = R_ic.T @ np.asarray(sc.T_imu_cam.t, np.float64)
    Q = blockdiag(R_ic, D)
    N = np.eye(D)
    N[3:6, 0:3] = -skew(tau)
    return {"unrotated": Q.T, "no_tau": Q @ N @ Q.T, "exchanged": Q.T @ Q.T}
