"""The three mono-bootstrap estimators on the motion grid of tests/motion_cases.py, without a GPU: the NumPy restatements
against the planted motions, the premises under which tests/test_motion_grid_gpu.py compares the kernels with them exactly,
and the functions the kernels run (tests/cpp_fivepoint/fivepoint_tool, tests/cpp_twopoint/twopoint_tool) and the host's
homography path (tests/cpp_init/init_tool) against the restatements, plain and under the address and undefined-behaviour
sanitizers, by the rules of tests/test_fivepoint_cpu.py, tests/test_twopoint_cpu.py and tests/test_init_cpu.py."""
import subprocess

import numpy as np
import pytest

import motion_cases as mc
import np_restatement_fivepoint as np5
import np_restatement_init as npi
import np_restatement_twopoint as npt
import test_fivepoint_cpu as t5
import test_init_cpu as ti
import test_twopoint_cpu as t2
from test_fivepoint_cpu import angle_deg, rotation_deg


@pytest.fixture(scope="module", autouse=True)
def tools():
    subprocess.check_call(["make", "-s", "-C", t5.TOOL_DIR, "fivepoint_tool", "fivepoint_tool_san"])
    subprocess.check_call(["make", "-s", "-C", t2.TOOL_DIR, "twopoint_tool", "twopoint_tool_san"])
    subprocess.check_call(["make", "-s", "-C", ti.TOOL_DIR, "init_tool", "init_tool_san"])


# ---------------------------------------------------------------- the restatements against the planted motions
# Measured on the restatements over the three scene seeds 31, 1031, 2031 per case (100 matches, 512 hypotheses); every bar
# is twice the worst of the three.  Degrees off, essential matrix (rotation, direction of t) and translation (direction):
#   forward              0.131 - 0.275, 1.29 - 2.50      0.149 - 0.310
#   backward             0.053 - 0.161, 0.30 - 1.34      0.130 - 0.273
#   identity_y_outliers  0 - 0.140,     0 - 1.91         0 - 0.136
#   rot20                0.103 - 0.264, 0.39 - 1.71      0.175 - 0.334
#   rot45                0.057 - 0.830, 0.33 - 5.23      0.117 - 0.289
#   rot90z_exact         0.099 - 0.527, 0.14 - 2.59      0.261 - 0.742
#   wide                 0.010 - 0.045, 0.09 - 0.79      0.075 - 0.320
# The noise-free cases without outliers (identity_x, identity_z, identity_general) gave R and t of the truth to 2e-15: their
# bar is the 1e-9 of the exact comparisons, on the entries, not an angle (an arc cosine near 1 resolves 1e-6 degrees).
# short_baseline: the direction is not observable (1 cm at 2 - 8 m is 0.5 - 2 px of parallax against 0.3 px of noise): 30 -
# 155 degrees off with the essential matrix, 66 - 103 with the translation, and 0 - 70 of the 70 planted inliers kept; only
# the status, the model's form and the mask's agreement with the model are asserted.
# Every other case kept all 70 planted inliers and at most 2 of the 30 outliers, with both estimators.
ACCURACY_E = {"forward": (2 * 0.2752, 2 * 2.502), "backward": (2 * 0.1613, 2 * 1.338), "identity_y_outliers": (2 * 0.1397, 2 * 1.909),
              "rot20": (2 * 0.264, 2 * 1.714), "rot45": (2 * 0.83, 2 * 5.227), "rot90z_exact": (2 * 0.5265, 2 * 2.591),
              "wide": (2 * 0.04508, 2 * 0.7917)}
ACCURACY_T = {"forward": 2 * 0.3095, "backward": 2 * 0.2733, "identity_y_outliers": 2 * 0.1364, "rot20": 2 * 0.3343, "rot45": 2 * 0.2887,
              "rot90z_exact": 2 * 0.7421, "wide": 2 * 0.3204}
# The homography against H = R + t n^T / d (H[2, 2] = 1), largest entry off: plane_forward 0.94e-3 - 1.80e-3, plane_oblique
# 1.03e-3 - 1.53e-3, plane_identity 0.93e-3 - 1.70e-3: twice the worst.  All 70 planted inliers kept, no outlier.
ACCURACY_H = {"plane_forward": 2 * 1.80e-3, "plane_oblique": 2 * 1.53e-3, "plane_identity": 2 * 1.70e-3}
EXACT_MODEL = 1e-9
NOISE_FREE_ALL_INLIERS = ("identity_x", "identity_z", "identity_general")
SEEDS3 = (31, 1031, 2031)


def check_inliers(c, r, what):
    inl = ~c["is_outlier"]
    assert r["n_inliers"] == int(r["mask"].sum()), what
    assert r["mask"][inl].all(), what                              # every planted inlier: the noise is 7 sigma inside
    assert r["mask"][~inl].sum() <= 0.1 * max(1, (~inl).sum()), what


@pytest.mark.parametrize("seed", SEEDS3)
@pytest.mark.parametrize("name", mc.BEARING_CASES)
def test_essential_restatement_recovers_the_planted_motion(name, seed):
    c = mc.make_scene(seed, mc.N, **mc.GRID[name])
    r = np5.estimate_essential_ransac(c["f_cur"], c["f_ref"], c["thresh"], c["seed"], mc.K)
    assert r["status"] == np5.STATUS_OK
    rot, err = rotation_deg(r["R"], c["R"]), angle_deg(r["t"], c["t"])
    print("%s/%d: rotation %.4g deg off, direction %.4g deg off, %d of %d planted inliers, %d others, %d iterations" % (
        name, seed, rot, err, int(r["mask"][~c["is_outlier"]].sum()), int((~c["is_outlier"]).sum()), int(r["mask"][c["is_outlier"]].sum()), r["refine_iters"]))
    assert abs(np.linalg.norm(r["t"]) - 1.0) < 1e-12 and np.abs(r["R"] @ r["R"].T - np.eye(3)).max() < 1e-12 and np.linalg.det(r["R"]) > 0
    assert np.array_equal(r["mask"], np5.inliers(r["R"][None], r["t"][None], c["f_cur"], c["f_ref"], c["thresh"])[0].astype(np.uint8))
    if name == "short_baseline":
        assert r["n_inliers"] == int(r["mask"].sum())
        return
    check_inliers(c, r, name)
    if name in NOISE_FREE_ALL_INLIERS:
        assert np.abs(r["R"] - c["R"]).max() <= EXACT_MODEL and np.abs(r["t"] - mc.unit(c["t"])).max() <= EXACT_MODEL
    else:
        assert rot < ACCURACY_E[name][0] and err < ACCURACY_E[name][1]


@pytest.mark.parametrize("seed", SEEDS3)
@pytest.mark.parametrize("name", mc.BEARING_CASES)
def test_translation_restatement_recovers_the_planted_direction(name, seed):
    c = mc.make_scene(seed, mc.N, **mc.GRID[name])
    r = npt.estimate_translation_ransac(c["f_cur"], c["f_ref"], c["R"], c["thresh"], c["seed"], mc.K)
    assert r["status"] == npt.STATUS_OK
    err = angle_deg(r["t"], c["t"])
    print("%s/%d: direction %.4g deg off, %d of %d planted inliers, %d others" % (
        name, seed, err, int(r["mask"][~c["is_outlier"]].sum()), int((~c["is_outlier"]).sum()), int(r["mask"][c["is_outlier"]].sum())))
    assert abs(np.linalg.norm(r["t"]) - 1.0) < 1e-12
    g, _, Ainv = npt.stage(c["f_cur"], c["f_ref"], c["R"])
    assert np.array_equal(r["mask"], npt.inlier_test(r["t"], c["f_cur"], g, Ainv, c["thresh"])[0].astype(np.uint8))
    if name == "short_baseline":
        assert r["n_inliers"] == int(r["mask"].sum())
        return
    check_inliers(c, r, name)
    if name in NOISE_FREE_ALL_INLIERS:
        assert np.abs(r["t"] - mc.unit(c["t"])).max() <= EXACT_MODEL
    else:
        assert err < ACCURACY_T[name]


@pytest.mark.parametrize("seed", SEEDS3)
@pytest.mark.parametrize("name", mc.PLANE_CASES)
def test_homography_restatement_recovers_the_planted_homography(name, seed):
    c = mc.make_scene(seed, mc.N, **mc.GRID[name])
    r = npi.estimate_homography_ransac(c["uv_ref"], c["uv_cur"], c["thresh_h"], c["seed"], mc.K)
    assert r["status"] == npi.STATUS_OK
    H = c["R"] + np.outer(c["t"], c["normal"]) / c["d"]
    err = np.abs(r["H"] - H / H[2, 2]).max()
    print("%s/%d: |dH| %.3g, %d of %d planted inliers, %d others" % (
        name, seed, err, int(r["mask"][~c["is_outlier"]].sum()), int((~c["is_outlier"]).sum()), int(r["mask"][c["is_outlier"]].sum())))
    check_inliers(c, r, name)
    assert err < ACCURACY_H[name]


def test_wide_has_bearings_behind_the_image_plane():
    for c in (mc.case_e("wide"), mc.case_t("wide")):
        assert (c["f_ref"][:, 2] <= 0).sum() >= 5 and (c["f_cur"][~c["is_outlier"], 2] <= 0).sum() >= 5
        assert np.abs(np.linalg.norm(c["f_ref"], axis=1) - 1).max() < 1e-15 and np.abs(np.linalg.norm(c["f_cur"], axis=1) - 1).max() < 1e-15


def test_noise_free_bearings_are_the_exact_projection():
    for name in mc.NOISE_FREE:
        if name.startswith("plane_"):
            continue
        c = mc.case_e(name)
        inl = ~c["is_outlier"]
        # R = I: both bearings and t lie in one plane, to rounding
        assert np.abs(np.einsum("ni,ni->n", np.cross(c["f_cur"][inl], c["f_ref"][inl]), mc.unit(c["t"])[None])).max() < 1e-15


# ---------------------------------------------------------------- the premises of the exact comparisons
EXACT_E = tuple(nm for nm in mc.RAGGED_BATCH if nm not in mc.PROPERTY_ONLY_E)
EXACT_T = tuple(nm for nm in mc.RAGGED_BATCH if nm not in mc.PROPERTY_ONLY_T)


def test_the_property_only_cases_are_few_and_named():
    allowed = {"identity_x", "identity_z", "identity_general", "short_baseline"}
    assert set(mc.PROPERTY_ONLY_E) <= allowed and set(mc.PROPERTY_ONLY_T) <= allowed
    assert all(len(reason) > 20 for reason in list(mc.PROPERTY_ONLY_E.values()) + list(mc.PROPERTY_ONLY_T.values()))


@pytest.mark.parametrize("name", EXACT_E)
def test_premises_of_the_exact_comparison_essential(name):
    """fivepoint_cases.premises (tests/test_fivepoint_cpu.py states them) on the restatement's two runs."""
    ok, m = mc.premises_e(name)
    a = mc.restated_e(name)
    print("%s: %s; h %d, %d -> %d inliers, %d degenerate, %d models, %d iterations" % (
        name, m, a["best_hypothesis"], a["n_inliers_hypothesis"], a["n_inliers"], a["n_degenerate"], a["n_models"], a["refine_iters"]))
    assert a["status"] == np5.STATUS_OK and ok
    if name not in mc.MODEL_NOT_UNIQUE:
        assert m["model_diff"] * 100.0 <= t5.fc.MODEL_BAR


@pytest.mark.parametrize("name", sorted(mc.PROPERTY_ONLY_E))
def test_a_property_only_case_meets_the_premises_at_none_of_ten_seeds(name):
    assert not any(mc.premises_e(name, seed)[0] for seed in range(1, 11))


@pytest.mark.parametrize("name", EXACT_T)
def test_premises_of_the_exact_comparison_translation(name):
    r = mc.restated_t(name)
    print("%s: gap_hyp %.2e gap_final %.2e eig_gap %.3g gap_norm %.2e gap_sign %.2e, %d -> %d inliers" % (
        name, r["gap_hyp"], r["gap_final"], r["eig_gap"], r["gap_norm"], r["gap_sign"], r["n_inliers_hypothesis"], r["n_inliers"]))
    assert mc.premises_t(name)


@pytest.mark.parametrize("name", mc.RAGGED_BATCH_PLANE)
def test_premises_of_the_exact_comparison_homography(name):
    r = mc.restated_h(name)
    print("%s: gap_hyp %.2e gap_final %.2e gap_lambda %.2e, %d degenerate" % (name, r["gap_hyp"], r["gap_final"], r["gap_lambda"], r["n_degenerate"]))
    assert mc.premises_h(name)


# ---------------------------------------------------------------- the kernels' functions, serially on the CPU
def check_properties_e(c, a, b, status, n_degenerate, mask, R, t, what):
    """A property-only case of the essential-matrix estimator: noise-free, so the truth is the reference."""
    inl = ~c["is_outlier"]
    assert status == np5.STATUS_OK, what
    assert mask[inl].all(), what
    assert np.abs(R - c["R"]).max() <= EXACT_MODEL and np.abs(t - mc.unit(c["t"])).max() <= EXACT_MODEL, what
    assert n_degenerate <= max(a["n_degenerate"], b["n_degenerate"]), (what, n_degenerate, a["n_degenerate"], b["n_degenerate"])


@pytest.mark.parametrize("exe", [t5.TOOL, t5.TOOL_SAN], ids=["plain", "sanitized"])
@pytest.mark.parametrize("name", mc.RAGGED_BATCH)
def test_fivepoint_tool_equals_restatement(tmp_path, name, exe):
    c = mc.case_e(name)
    path = str(tmp_path / "case.txt")
    t5.write_case(path, c["f_cur"], c["f_ref"], c["thresh"], c["seed"], mc.K)
    out = t5.run_tool(exe, path)
    a, b = mc.restated_e(name), mc.restated_e(name, True)
    print("%s: winner %s (restatement %d), %s degenerate (restatement %d and %d)" % (
        name, out["best_hypothesis"][0], a["best_hypothesis"], out["n_degenerate"][0], a["n_degenerate"], b["n_degenerate"]))
    if name in mc.PROPERTY_ONLY_E:
        check_properties_e(c, a, b, int(out["status"][0]), int(out["n_degenerate"][0]), np.array(out["mask"], int),
                           np.array(out["R"], float).reshape(3, 3), np.array(out["t"], float), name)
    else:
        t5.check_tool(out, a, name, c["f_cur"], c["f_ref"], c["thresh"], mc.K, name not in mc.MODEL_NOT_UNIQUE)
    if name in NOISE_FREE_ALL_INLIERS:
        # every sample is five exact matches of one motion: every hypothesis must find it (a root of even multiplicity, or one
        # of a cluster, is invisible to a root finder that bisects sign changes)
        assert int(out["n_hold_all"][0]) == mc.K, (name, out["n_hold_all"])


@pytest.mark.parametrize("name", NOISE_FREE_ALL_INLIERS)
def test_restatement_finds_the_motion_in_every_all_inlier_hypothesis(name):
    a = mc.restated_e(name, turned=name in mc.PROPERTY_ONLY_E)     # identity_x: the run that calls none degenerate
    best = np.full(mc.K, -1)
    np.maximum.at(best, a["cand_h"], a["cand_count"])
    assert (best == mc.N).all()


@pytest.mark.parametrize("exe", [t2.TOOL, t2.TOOL_SAN], ids=["plain", "sanitized"])
@pytest.mark.parametrize("name", mc.RAGGED_BATCH)
def test_twopoint_tool_equals_restatement(tmp_path, name, exe):
    c = mc.case_t(name)
    path = str(tmp_path / "case.txt")
    t2.write_case(path, c["f_cur"], c["f_ref"], c["R"], c["thresh"], c["seed"], mc.K)
    t2.check_tool(t2.run_tool(exe, path), mc.restated_t(name), name)


@pytest.mark.parametrize("exe", [ti.TOOL, ti.TOOL_SAN], ids=["plain", "sanitized"])
@pytest.mark.parametrize("name", mc.PLANE_CASES)
def test_homography_path_of_the_host_equals_restatement(tmp_path, name, exe):
    """The restated H of a plane case through the host's decomposition and selection (svo_hip_init.cpp behind init_tool), as
    tests/test_init_cpu.py::test_host_maths_equal_the_restatement has it, and the selected motion against the planted one."""
    c, r = mc.case_h(name), mc.restated_h(name)
    path = str(tmp_path / "case.txt")
    ti.write_case(path, r["H"], c, r["mask"], 3.0, np.arctan(2.0 / (2 * c["focal"])) * 2, [1, 0, 0, 0, 0, 0, 0])
    out = ti.run_tool(exe, path)
    ti.close(ti.floats(out["singular_values"][0]), np.linalg.svd(r["H"], compute_uv=False), "singular values")
    motions = npi.decompose_homography(r["H"])
    assert int(out["n_motions"][0][0]) == len(motions) == 4
    for k, (R, t, n) in enumerate(motions):
        ti.close(ti.floats(out["motion_R"][k]).reshape(3, 3), R, "R %d" % k)
        ti.close(ti.floats(out["motion_t"][k]), t, "t %d" % k)
        ti.close(ti.floats(out["motion_n"][k]), n, "n %d" % k)
    s = npi.select_motion(r["H"], c["f_cur"], c["f_ref"], r["mask"], c["thresh_h"])
    assert [float(v) for v in out["cheirality"][0]] == s["cheirality"]
    assert int(out["picked"][0][0]) == s["picked"] and float(out["score"][0][0]) == s["score"]
    ti.close(ti.floats(out["selected_R"][0]).reshape(3, 3), s["R"], "selected R")
    ti.close(ti.floats(out["selected_t"][0]), s["t"], "selected t")
    d = [(rotation_deg(R, c["R"]), angle_deg(t, c["t"])) for (R, t, n) in motions]
    print("%s: picked %d, cheirality %s, the four motions (rotation, direction) off by %s" % (name, s["picked"], s["cheirality"], d))
