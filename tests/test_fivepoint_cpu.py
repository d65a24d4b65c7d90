"""The FivePoint initialiser's estimator without a GPU: the NumPy restatement (tests/np_restatement_fivepoint.py) against
planted geometry, the premises under which tests/test_essential_ransac_gpu.py compares the kernel with it exactly, and the
functions the kernel runs (csrc/svoh_essential.h, serially behind tests/cpp_fivepoint/fivepoint_tool) against the
restatement, plain and under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import np_restatement_fivepoint as np5
import fivepoint_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL_DIR = os.path.join(ROOT, "tests", "cpp_fivepoint")
TOOL, TOOL_SAN = os.path.join(TOOL_DIR, "fivepoint_tool"), os.path.join(TOOL_DIR, "fivepoint_tool_san")


@pytest.fixture(scope="module", autouse=True)
def tools():
    subprocess.check_call(["make", "-s", "-C", TOOL_DIR, "fivepoint_tool", "fivepoint_tool_san"])


def angle_deg(a, b):
    return float(np.degrees(np.arccos(np.clip(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)), -1.0, 1.0))))


def rotation_deg(Ra, Rb):
    return float(np.degrees(np.arccos(np.clip((np.trace(Ra @ Rb.T) - 1.0) / 2.0, -1.0, 1.0))))


# ---------------------------------------------------------------- the restatement against planted geometry
# Measured on the restatement over three seeds per scene (200 matches, 2000 hypotheses, without and with the 30 % of
# outliers), degrees off in (rotation, direction of t): general scenes 0.02 - 0.16 and 0.11 - 1.31, planar scenes
# 0.09 - 1.83 and 0.55 - 14.6 (the worst: a plane with outliers, the one scene that used all ten iterations; the others of
# its class stay below 0.45 and 2.7).  The bars are twice the worst, per scene class.
ACCURACY = {"general": (2 * 0.155, 2 * 1.311), "plane": (2 * 1.825, 2 * 14.52)}
SCENES = [("general", False, 0.0), ("plane", True, 0.0), ("outliers", False, 0.3), ("plane_outliers", True, 0.3)]


@pytest.mark.parametrize("name,plane,outliers", SCENES)
@pytest.mark.parametrize("k", [0, 1, 2])
def test_restatement_recovers_the_planted_motion_and_inliers(name, plane, outliers, k):
    c = fc.make_case(31 + 7 * len(name) + 1000 * k, 200, plane=plane, outlier_fraction=outliers)
    r = np5.estimate_essential_ransac(c["f_cur"], c["f_ref"], c["thresh"], c["seed"])
    assert r["status"] == np5.STATUS_OK
    inl = ~c["is_outlier"]
    rot, rot_win = rotation_deg(r["R"], c["R"]), rotation_deg(r["R_winner"], c["R"])
    err, err_win = angle_deg(r["t"], c["t"]), angle_deg(r["t_winner"], c["t"])
    print("%s/%d: rotation %.3f deg off (winner %.3f), direction %.3f deg off (winner %.3f), %d iterations, %d of %d planted inliers, %d others"
          % (name, k, rot, rot_win, err, err_win, r["refine_iters"], int(r["mask"][inl].sum()), int(inl.sum()), int(r["mask"][~inl].sum())))
    assert abs(np.linalg.norm(r["t"]) - 1.0) < 1e-12 and np.abs(r["R"] @ r["R"].T - np.eye(3)).max() < 1e-12
    bar = ACCURACY["plane" if plane else "general"]
    assert rot < bar[0] and err < bar[1]
    assert r["mask"][inl].sum() >= 0.98 * inl.sum()                # the noise is 7 sigma inside; the model is a fit to it
    assert r["mask"][~inl].sum() <= 0.1 * max(1, (~inl).sum())     # an outlier near the epipolar line passes: a few per cent
    assert r["n_inliers"] == int(r["mask"].sum())


def test_a_nan_match_is_never_an_inlier_and_spoils_only_its_hypotheses():
    f_cur, f_ref, thresh, seed, k = fc.nan_case()
    a = np5.estimate_essential_ransac(f_cur, f_ref, thresh, seed)
    b = np5.estimate_essential_ransac(f_cur, f_ref, thresh, seed, basis_turn=fc.TURN)
    assert a["status"] == np5.STATUS_OK and a["mask"][k] == 0 and a["n_degenerate"] > 0
    ok, m = fc.premises(a, b, f_cur, f_ref, thresh)
    assert ok, m
    c = fc.make_case(fc.SCENE_SEEDS["nan"], 100)
    assert rotation_deg(a["R"], c["R"]) < ACCURACY["general"][0] and angle_deg(a["t"], c["t"]) < ACCURACY["general"][1]


NO_MODEL = ["pure rotation", "identical matches", "n = 4", "n = 0"]


@pytest.mark.parametrize("what", NO_MODEL)
def test_no_model(what):
    f_cur, f_ref = fc.no_model_inputs()[what]
    for turn in (None, fc.TURN):
        r = np5.estimate_essential_ransac(f_cur, f_ref, fc.THRESH, 99, basis_turn=turn)
        assert r["status"] == np5.STATUS_NO_MODEL
        assert not r["R"].any() and not r["t"].any() and not r["mask"].any()
        assert (r["best_hypothesis"], r["best_candidate"], r["n_inliers_hypothesis"], r["n_inliers"], r["n_degenerate"], r["n_models"],
                r["refine_iters"]) == (0, 0, 0, 0, 0, 0, 0)


def test_every_candidate_is_an_essential_matrix_of_its_five():
    c = fc.make_case(77, 50)
    idx, ok = np5.sample_five(5, 64, 50)
    assert ok.all()
    fc5, fr5 = c["f_cur"][idx], c["f_ref"][idx]
    for turn in (None, fc.TURN):
        E, valid, degenerate, _, _ = np5.essential_candidates(fc5, fr5, turn)
        assert not degenerate.any() and valid.any(axis=1).all()
        Ev = E[valid]
        epi = np.einsum("ksi,kcij,ksj->kcs", fc5, E, fr5)[valid]
        cubic = 2.0 * Ev @ np.transpose(Ev, (0, 2, 1)) @ Ev - np.einsum("m,mij->mij", np.einsum("mij,mij->m", Ev, Ev), Ev)
        print("candidates %d, epipolar %.2e, det %.2e, cubic %.2e" % (len(Ev), np.abs(epi).max(), np.abs(np.linalg.det(Ev)).max(), np.abs(cubic).max()))
        assert np.abs(epi).max() < 1e-12
        assert np.median(np.abs(np.linalg.det(Ev))) < 1e-12 and np.median(np.abs(cubic).max(axis=(1, 2))) < 1e-12


# ---------------------------------------------------------------- the premises of the exact comparison on the GPU
def test_the_model_bar_is_a_hundred_times_what_the_two_runs_differ_by():
    worst = max(fc.model_difference(fc.restated(nm), fc.restated(nm, True)) for nm in fc.CASE_NAMES if nm not in fc.MODEL_NOT_UNIQUE)
    print("largest difference of (R, t) between the restatement's two runs: %.2e; bar %.1e" % (worst, fc.MODEL_BAR))
    assert 100.0 * worst <= fc.MODEL_BAR == 1e-9                   # the floor of the other two estimators holds


@pytest.mark.parametrize("name", fc.CASE_NAMES)
def test_premises_of_the_exact_comparison(name):
    """The restatement run twice, with its own null-space basis and with the basis turned.  (a) Both runs give the same
    status, winner, counts and mask.  (b) The winner's count is unique within its hypothesis and tied only with higher h.
    (c) For the winner, the final model and every candidate at h <= the winner's whose count is within one of it: no
    error closer to the threshold than a thousand times what the two runs' models change it by, and never closer than
    1e-7 (relative).  (d) The winner's five sample errors are below thresh / 1000.  Beyond what the issue names: no
    candidate had two motions that hold its five, no refinement step within 1e-13 of the stopping bound, no elimination
    with a smallest singular value between 1e-9 (degenerate) and 1e-8: the pivots the kernel tests are of that order.  At n = 5 and
    n = 6 the model is not unique: (a) without the winner, and (d)."""
    c, _ = fc.case(name)
    a, b = fc.restated(name), fc.restated(name, True)
    ok, m = fc.premises(a, b, c["f_cur"], c["f_ref"], c["thresh"], model_unique=name not in fc.MODEL_NOT_UNIQUE)
    print("%s: %s; h %d, %d -> %d inliers, %d degenerate, %d models, %d iterations" % (
        name, m, a["best_hypothesis"], a["n_inliers_hypothesis"], a["n_inliers"], a["n_degenerate"], a["n_models"], a["refine_iters"]))
    assert a["status"] == np5.STATUS_OK
    assert m["same"] and m["motion_unique"] and m["sample"] < 1e-3 and m["elim"] >= 1e-8
    if name not in fc.MODEL_NOT_UNIQUE:
        assert m["tie_ok"] and m["gap_ok"] and m["gap"] >= 1e-7 and m["steps_ok"]
        assert m["model_diff"] * 100.0 <= fc.MODEL_BAR
    else:
        assert a["mask"].all() and a["n_inliers"] == len(a["mask"])
    assert ok


# ---------------------------------------------------------------- the kernel's functions, serially on the CPU
def write_case(path, f_cur, f_ref, thresh, seed, K):
    with open(path, "w") as f:
        f.write("K %d\nthresh %.17g\nseed %d\n" % (K, thresh, seed))
        for a, b in zip(f_cur, f_ref):
            f.write("match %s %s\n" % (" ".join("%.17g" % v for v in a), " ".join("%.17g" % v for v in b)))


def run_tool(exe, path):
    p = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert p.returncode == 0, (p.returncode, p.stderr.decode()[-2000:])
    assert b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr, p.stderr.decode()[-2000:]
    out = {}
    for line in p.stdout.decode().splitlines():
        key, *vals = line.split()
        out[key] = vals
    return out


def check_tool(out, want, what, f_cur, f_ref, thresh, K, model_unique=True):
    keys = ["status", "n_inliers_hypothesis", "n_inliers", "n_degenerate"] + (["best_hypothesis", "refine_iters"] if model_unique else [])
    for key in keys:
        assert int(out[key][0]) == want[key], (what, key, out[key], want[key])
    assert np.array_equal(np.array(out["mask"], int), want["mask"]), what
    n_models = int(out["n_models"][0])
    R, t = np.array(out["R"], float).reshape(3, 3), np.array(out["t"], float)
    if want["status"] != np5.STATUS_OK:
        assert not R.any() and not t.any() and n_models == 0 and int(out["best_candidate"][0]) == 0
        return
    assert 0 < n_models <= 10 * K and 0 <= int(out["best_candidate"][0]) < 10
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-9 and np.linalg.det(R) > 0 and abs(np.linalg.norm(t) - 1.0) < 1e-9
    if model_unique:
        d = max(np.abs(R - want["R"]).max(), np.abs(t - want["t"]).max())
        Rw, tw = np.array(out["R_winner"], float).reshape(3, 3), np.array(out["t_winner"], float)
        dw = max(np.abs(Rw - want["R_winner"]).max(), np.abs(tw - want["t_winner"]).max())
        print("%s: |d(R, t)| %.2e, winner %.2e, models %d (restatement %d)" % (what, d, dw, n_models, want["n_models"]))
        assert d <= fc.MODEL_BAR, (what, d)
    else:
        assert np5.inliers(R[None], t[None], f_cur, f_ref, thresh)[0].all(), what


@pytest.mark.parametrize("exe", [TOOL, TOOL_SAN], ids=["plain", "sanitized"])
@pytest.mark.parametrize("name", fc.CASE_NAMES)
def test_tool_equals_restatement(tmp_path, name, exe):
    c, K = fc.case(name)
    path = str(tmp_path / "case.txt")
    write_case(path, c["f_cur"], c["f_ref"], c["thresh"], c["seed"], K)
    check_tool(run_tool(exe, path), fc.restated(name), name, c["f_cur"], c["f_ref"], c["thresh"], K, name not in fc.MODEL_NOT_UNIQUE)


@pytest.mark.parametrize("exe", [TOOL, TOOL_SAN], ids=["plain", "sanitized"])
@pytest.mark.parametrize("what", NO_MODEL + ["nan"])
def test_tool_on_degenerate_input(tmp_path, what, exe):
    if what == "nan":
        f_cur, f_ref, thresh, seed, _ = fc.nan_case()
    else:
        (f_cur, f_ref), thresh, seed = fc.no_model_inputs()[what], fc.THRESH, 99
    path = str(tmp_path / "case.txt")
    write_case(path, f_cur, f_ref, thresh, seed, 2000)
    check_tool(run_tool(exe, path), np5.estimate_essential_ransac(f_cur, f_ref, thresh, seed), what, f_cur, f_ref, thresh, 2000)
