"""Runs tests/cpp/test_host_align_wide.cpp: SparseImgAlignHip on a bundle with an equidistant or atan camera -- the
blocking overload goes through svoh_sparse_align_wide_batch, the overloads that queue throw."""
import os
import struct
import subprocess

import numpy as np
import pytest

from svo_pro_universal_amd import frontend as fe

import wide_align as wa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def dump_scene(path, sc):
    cam = sc.cam
    with open(path, "wb") as f:
        f.write(struct.pack("4i", cam.width, cam.height, sc.n_features, fe._DISTORTION[cam.model]))
        np.array([cam.fx, cam.fy, cam.cx, cam.cy] + (list(cam.dist) + [0.0, 0.0, 0.0])[:4]).tofile(f)
        sc.T_cam_imu.as7().tofile(f)
        sc.T_ref_f_w.as7().tofile(f)
        # the new frame starts near its true pose (wide_align.MOTION): T_f_w = T_cam_imu * T_icur_iref * T_imu_world(ref)
        (sc.T_cam_imu * wa.start_state(sc) * sc.T_imu_cam * sc.T_ref_f_w).as7().tofile(f)
        np.ascontiguousarray(sc.px, np.float64).tofile(f)
        np.ascontiguousarray(sc.f, np.float64).tofile(f)
        np.ascontiguousarray(sc.pos_world, np.float64).tofile(f)
        np.ascontiguousarray(sc.flags, np.uint8).tofile(f)
        sc.img_ref.tofile(f)
        sc.img_cur.tofile(f)


@pytest.mark.parametrize("kind,seed", [("equidistant", 317), ("atan", 324)])
def test_cpp_host_mirror_runs_a_wide_bundle_through_the_wide_entry(tmp_path, kind, seed):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "svo_pro_universal_amd", "host")])
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "align_wide.mk"])
    sc = wa.scene(kind, seed, 150, 4, 30)[0]
    path = str(tmp_path / "scene.bin")
    dump_scene(path, sc)
    out = subprocess.run([os.path.join(ROOT, "tests", "cpp", "test_host_align_wide"), path], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "PASS" in out.stdout
