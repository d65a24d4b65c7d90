"""The pose optimiser's and the candidate projection's wide twins without a GPU: (1) the built objects carry the twins
under their own names beside the narrow kernels, within their register budgets; (2) the premises of
tests/test_wide_geometry_gpu.py hold on the NumPy reference alone -- that file demands exact equality of discrete outputs
(iteration counts, outlier flags, visibility flags), which is fair only where the reference decides none of them within
rounding of its threshold.  A scene that fails a premise gets another seed in tests/wide_geometry.py; the GPU file's
bars stay."""
import os
import subprocess
import sys

import numpy as np
import pytest

import wide_geometry as wg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svo_pro_universal_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "scripts"))

ET = (0, 1, 2)   # as the kernels' second template argument: svoh_pose_error_type


@pytest.fixture(scope="module")
def built():
    import kernel_resources_built as krb
    if not (os.path.exists(os.path.join(CSRC, "pose.o")) and os.path.exists(os.path.join(CSRC, "matcher.o"))):
        subprocess.check_call(["make", "-s", "-C", CSRC])
    return krb.kernels(os.path.join(CSRC, "pose.o")), krb.kernels(os.path.join(CSRC, "matcher.o"))


def test_pose_twins_exist_beside_the_narrow_kernels(built):
    pose, _ = built
    unit, bearing, image = wg.UNIT, wg.BEARING, wg.IMAGE
    narrow = ["pose_optimize_kernel<%d, %d>" % (nt, et) for nt in (64, 256) for et in ET]
    narrow += ["pose_optimize_kernel<512, %d>" % et for et in (unit, image)]
    assert len(narrow) == 8
    for name in narrow:
        assert name in pose, name
    wide = sorted(k for k in pose if k.startswith("pose_optimize_wide_kernel<"))
    must = sorted("pose_optimize_wide_kernel<%d, %d>" % (nt, et) for nt in (64, 256) for et in (bearing, image))
    may = "pose_optimize_wide_kernel<512, %d>" % image
    assert wide in (must, sorted(must + [may])), wide          # four, or five with the 512-thread image-plane build
    for name in wide:                                          # the unit-plane error never evaluates the camera: no twin
        assert not name.endswith(", %d>" % unit)
        assert pose[name]["vgpr"] <= 512
    if may in pose:                                            # 512 threads are two waves per SIMD
        assert pose[may]["vgpr"] <= 256 and pose[may]["vgpr_spill"] == 0


def test_candidate_twins_exist_and_keep_the_narrow_budget(built):
    _, matcher = built
    for stem in ("project_candidates", "project_candidates_multi", "project_candidates_ranges"):
        narrow, wide = matcher[stem + "_kernel"], matcher[stem + "_wide_kernel"]
        assert wide["lds"] == 0 and wide["vgpr_spill"] <= narrow["vgpr_spill"]


@pytest.mark.parametrize("name,error_type", wg.POSE_CASES)
def test_pose_reference_decides_nothing_within_rounding(name, error_type):
    sc = wg.pose_scene(name)
    g = wg.pose_reference(name, error_type)
    opt = wg.pose_options(name, error_type)
    assert g["status"] == 0
    e0, e1 = wg.pose_error(sc, sc["T_imu_world_init"].as7()), wg.pose_error(sc, g["T7"])
    assert e1[0] < 0.1 * e0[0] and e1[1] < 0.1 * e0[1]
    assert g["n_deleted_edges"] + g["n_deleted_corners"] >= 10
    if wg.POSE_SCENES[name][2] > 0:
        assert g["n_deleted_edges"] >= 1
        assert any(wg.npp.is_edgelet(int(t)) and u for c in sc["cams"] for t, u in zip(c["type"], c["usable"]))
    thr = opt.outlier_threshold
    for c, e in zip(sc["cams"], g["final"]):
        u = c["usable"].astype(bool)
        assert np.abs(np.abs(e[u]) - thr).min() > 1e-6 * thr


@pytest.mark.parametrize("kind", ["equidistant", "atan"])
def test_candidate_reference_decides_little_within_rounding(kind):
    r = wg.candidate_reference(kind)
    n = wg.N_CAND
    assert r["near"].sum() <= 4
    assert 300 < r["ok"].sum() < n - 300
    assert r["cone_alone"].sum() >= 20 and r["margin_alone"].sum() >= 20
