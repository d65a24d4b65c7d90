"""The equidistant and ATAN cameras on the DEVICE: svoh_camera_maths (the camera maths of svoh_math.h as the wide
kernels compile it) against the NumPy restatement on grids that reach the image corners, the reference's held camera
cases, the NaN of the equidistant centre pixel, and the refusal of the Jacobian the reference does not have (ATAN)."""
import math

import numpy as np
import pytest

from svo_pro_universal_amd import _capi as capi, frontend as fe, synth
import np_restatement_cameras as npc
import test_camera_models_cpu as cpu

pytestmark = pytest.mark.gpu

MODEL_NAME = {npc.EQUIDISTANT: "equidistant", npc.ATAN: "atan"}


def synth_cam(cw):
    return synth.Camera(cw.width, cw.height, cw.fx, cw.fy, cw.cx, cw.cy, dist=cw.d, model=MODEL_NAME[cw.model])


@pytest.mark.parametrize("name", ["visensor_flyingroom_mono.yaml", "davis_flyingroom.yaml", "svo_test_pinhole.yaml"])
def test_device_camera_maths_match_the_restatement(gpu_ctx, name):
    cw = cpu.cam_of_file(name)
    pts = cpu.corner_grid(cw)
    want = cpu.restated_maths(cw, pts)
    has_J = cw.model != npc.ATAN
    px, J, fb = gpu_ctx.camera_maths(synth_cam(cw), pts.ravel(), jacobian=has_J)
    got = np.concatenate([px.reshape(-1, 2), J.reshape(-1, 6) if has_J else np.full((len(pts), 6), np.nan),
                          fb.reshape(-1, 3)], axis=1)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert cpu.rel_err(got[ok], want[ok]).max() < 1e-13
    if has_J:   # without the Jacobian: the same projection and back-projection
        px2, J2, fb2 = gpu_ctx.camera_maths(synth_cam(cw), pts.ravel(), jacobian=False)
        assert J2 is None and np.array_equal(px2, px) and np.array_equal(fb2, fb)


def test_atan_jacobian_is_refused(gpu_ctx):
    cam = synth_cam(cpu.cam_of_file("svo_test_pinhole.yaml"))
    with pytest.raises(fe.SvohError) as e:
        gpu_ctx.camera_maths(cam, [0.1, 0.2, 1.0])
    assert e.value.code == capi.SVOH_ERR_UNSUPPORTED


def test_held_cases_on_the_device(gpu_ctx):
    # test_cameras.cpp:34-81 through a unit pinhole (fx = fy = 1, cx = cy = 0): project3 is distort, backProject3 undistort
    atan = synth.Camera(1000, 1000, 1.0, 1.0, 0.0, 0.0, dist=[0.934479], model="atan")
    _, _, fb = gpu_ctx.camera_maths(atan, [0.5, 0.8, 1.0], jacobian=False)
    assert abs(fb[0] - 0.5) < 1e-10 and abs(fb[1] - 0.8) < 1e-10
    eq = synth.Camera(1000, 1000, 1.0, 1.0, 0.0, 0.0, dist=[-0.0027, 0.0241, -0.0430, 0.0311], model="equidistant")
    _, _, fb = gpu_ctx.camera_maths(eq, [0.5, 0.8, 1.0])
    assert abs(fb[0] - 0.5) < 1e-10 and abs(fb[1] - 0.8) < 1e-10
    x, y, step = fb[0], fb[1], 1e-4
    pts = np.array([[x, y, 1.0], [x + step, y, 1.0], [x - step, y, 1.0], [x, y + step, 1.0], [x, y - step, 1.0]])
    p2, J2, _ = gpu_ctx.camera_maths(eq, pts.ravel())
    p2 = p2.reshape(-1, 2)
    num = np.stack([(p2[1] - p2[2]) / (2 * step), (p2[3] - p2[4]) / (2 * step)], axis=1)
    assert np.abs(J2[:6].reshape(2, 3)[:, :2] - num).max() < 1e-4


def test_equidistant_centre_back_projects_to_nan(gpu_ctx):
    cw = cpu.cam_of_file("visensor_flyingroom_mono.yaml")
    px, _, fb = gpu_ctx.camera_maths(synth_cam(cw), [0.0, 0.0, 1.0])
    assert px[0] == cw.cx and px[1] == cw.cy
    assert math.isnan(fb[0]) and math.isnan(fb[1]) and fb[2] == 1.0


def test_narrow_cameras_unchanged(gpu_ctx):
    # radtan through the wide-aware entry still runs the narrow kernel: the old call signature, the old numbers
    cam = synth.Camera.euroc_like(752, 480)
    cn = npc.CamWide.of(cam)
    xyz = np.array([0.3, -0.2, 1.5])
    px, J, fb = gpu_ctx.camera_maths(cam, xyz)
    assert np.abs(px - cn.project3(xyz)).max() < 1e-12
    assert np.abs(J.reshape(2, 3) - cn.project3_jacobian(xyz)).max() < 1e-9


def test_atan_with_zero_s_is_refused(gpu_ctx):
    cam = synth.Camera(752, 480, 383.0, 382.4, 344.7, 244.3, dist=[0.0], model="atan")
    with pytest.raises(fe.SvohError) as e:
        gpu_ctx.camera_maths(cam, [0.1, 0.2, 1.0], jacobian=False)
    assert e.value.code != capi.SVOH_OK and "non-zero" in str(e.value)


def test_alignment_refuses_a_wide_camera_instead_of_treating_it_as_pinhole(gpu_ctx):
    # the alignment kernels are compiled for NONE | RADTAN only: a wide camera is an error, never a pinhole
    sc = synth.make_align_scene(3, n_features=60, patch_size=4, cam=synth.Camera.visensor_like())
    fr = gpu_ctx.build_pyramid(sc.img_ref, 5)
    fc = gpu_ctx.build_pyramid(sc.img_cur, 5)
    pbs, _ = fe.make_align_problems([[(sc, fr, fc)]])
    with pytest.raises(fe.SvohError) as e:
        gpu_ctx.sparse_align(capi.default_align_options(min_level=1), pbs)
    assert "distortion" in str(e.value)
