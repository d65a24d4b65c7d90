"""The TwoPoint initialiser's estimator without a GPU: the NumPy restatement (tests/np_restatement_twopoint.py) against
planted geometry, the premises under which tests/test_translation_ransac_gpu.py compares the kernel with it exactly, and
the functions the kernel runs (csrc/svoh_translation.h, serially behind tests/cpp_twopoint/twopoint_tool) against the
restatement, plain and under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import np_restatement_twopoint as npt
import twopoint_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL_DIR = os.path.join(ROOT, "tests", "cpp_twopoint")
TOOL, TOOL_SAN = os.path.join(TOOL_DIR, "twopoint_tool"), os.path.join(TOOL_DIR, "twopoint_tool_san")


@pytest.fixture(scope="module", autouse=True)
def tools():
    subprocess.check_call(["make", "-s", "-C", TOOL_DIR, "twopoint_tool", "twopoint_tool_san"])


def angle_deg(a, b):
    return float(np.degrees(np.arccos(np.clip(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)), -1.0, 1.0))))


# ---------------------------------------------------------------- the restatement against planted geometry
# One match bounds the direction to (epipolar noise) / (parallax): 0.3 px in both images is 0.42 px = 1.1e-3 rad at 400 px,
# the parallax of 0.46 m at 2 - 8 m about 0.09 rad, so 0.66 degrees; over N = 140 inliers whose moment matrix has a middle
# eigenvalue of 0.05 - 0.09 of the largest the weak axis keeps 0.66 / sqrt(0.07 N) = 0.21 degrees (one sigma).  The bar
# is 1 degree; a winning hypothesis from one noisy pair is allowed ten times that.
@pytest.mark.parametrize("name,plane,outliers", [("general", False, 0.0), ("plane", True, 0.0), ("outliers", False, 0.3),
                                                 ("plane_outliers", True, 0.3)])
def test_restatement_recovers_the_planted_translation_and_inliers(name, plane, outliers):
    c = tc.make_case(31 + 7 * len(name), 200, plane=plane, outlier_fraction=outliers)
    r = npt.estimate_translation_ransac(c["f_cur"], c["f_ref"], c["R"], c["thresh"], c["seed"])
    assert r["status"] == npt.STATUS_OK
    inl = ~c["is_outlier"]
    err, err_win = angle_deg(r["t"], c["t"]), angle_deg(r["t_winner"], c["t"])
    print("%s: direction %.3f deg off (winner %.3f), %d of %d planted inliers, %d others" %
          (name, err, err_win, int(r["mask"][inl].sum()), int(inl.sum()), int(r["mask"][~inl].sum())))
    assert abs(np.linalg.norm(r["t"]) - 1.0) < 1e-12
    assert err < 1.0 and err_win < 10.0
    assert r["mask"][inl].all()                                    # every planted inlier (the noise is 7 sigma inside)
    assert r["mask"][~inl].sum() <= 0.1 * max(1, (~inl).sum())     # an outlier near the epipolar line passes: a few per cent
    assert r["n_inliers"] == int(r["mask"].sum())


def test_a_nan_match_is_never_an_inlier_and_spoils_only_its_hypotheses():
    f_cur, f_ref, R, thresh, seed, k = tc.nan_case()
    r = npt.estimate_translation_ransac(f_cur, f_ref, R, thresh, seed)
    assert r["status"] == npt.STATUS_OK and r["mask"][k] == 0 and r["n_degenerate"] > 0
    assert tc.premises_hold(r)
    c = tc.make_case(tc.SCENE_SEEDS["nan"], 100)
    assert angle_deg(r["t"], c["t"]) < 1.0


def no_model_inputs():
    c = tc.make_case(55, 40, outlier_fraction=0.0)
    rot = c["f_ref"] @ c["R"].T                                    # the camera only turned
    same = np.tile(c["f_cur"][:1], (40, 1)), np.tile(c["f_ref"][:1], (40, 1))
    return {"pure rotation": (rot, c["f_ref"], c["R"]), "identical matches": (same[0], same[1], c["R"]),
            "n = 1": (c["f_cur"][:1], c["f_ref"][:1], c["R"]), "n = 0": (c["f_cur"][:0], c["f_ref"][:0], c["R"])}


@pytest.mark.parametrize("what", ["pure rotation", "identical matches", "n = 1", "n = 0"])
def test_no_model(what):
    f_cur, f_ref, R = no_model_inputs()[what]
    r = npt.estimate_translation_ransac(f_cur, f_ref, R, tc.THRESH, 99)
    assert r["status"] == npt.STATUS_NO_MODEL
    assert not r["t"].any() and not r["mask"].any()
    assert (r["best_hypothesis"], r["n_inliers_hypothesis"], r["n_inliers"], r["n_degenerate"]) == (0, 0, 0, 0)


def test_jacobi_agrees_with_eigh():
    rng = np.random.RandomState(5)
    for _ in range(50):
        mh = rng.randn(30, 3) * [1.0, 0.3, 0.02]
        Q, _ = np.linalg.qr(rng.randn(3, 3))
        mh = mh @ Q.T
        M = mh.T @ mh
        w, V = np.linalg.eigh(M)
        v = npt.jacobi_smallest_eigenvector(M)
        assert abs(abs(v @ V[:, 0]) - 1.0) < 1e-12 and abs(np.linalg.norm(v) - 1.0) < 1e-15
    assert np.array_equal(npt.jacobi_smallest_eigenvector(np.zeros((3, 3))), [1.0, 0.0, 0.0])
    assert np.isnan(npt.jacobi_smallest_eigenvector(np.full((3, 3), np.nan))).all()


# ---------------------------------------------------------------- the premises of the exact comparison on the GPU
@pytest.mark.parametrize("name", tc.CASE_NAMES)
def test_premises_of_the_exact_comparison(name):
    """No error of any hypothesis, nor of the final model, within 1e-7 (relative) of the threshold; the winner's count
    unique or tied only with higher h; (lambda_mid - lambda_min) / lambda_max >= 1e-2 for M.  Beyond what the issue
    names: no |t| within 1e-3 (relative) of the degeneracy bound, no sign decision within 1e-9 of zero."""
    r = tc.restated(name)
    print("%s: gap_hyp %.2e gap_final %.2e eig_gap %.3g gap_norm %.2e gap_sign %.2e, %d -> %d inliers, %d degenerate" %
          (name, r["gap_hyp"], r["gap_final"], r["eig_gap"], r["gap_norm"], r["gap_sign"], r["n_inliers_hypothesis"], r["n_inliers"],
           r["n_degenerate"]))
    assert r["status"] == npt.STATUS_OK
    assert r["gap_hyp"] >= 1e-7 and r["gap_final"] >= 1e-7
    assert r["tie_ok"]
    assert r["eig_gap"] >= 1e-2
    assert r["gap_norm"] >= 1e-3 and r["gap_sign"] >= 1e-9


# ---------------------------------------------------------------- the kernel's functions, serially on the CPU
def write_case(path, f_cur, f_ref, R, thresh, seed, K):
    with open(path, "w") as f:
        f.write("K %d\nthresh %.17g\nseed %d\nR %s\n" % (K, thresh, seed, " ".join("%.17g" % v for v in np.asarray(R).ravel())))
        for a, b in zip(f_cur, f_ref):
            f.write("match %s %s\n" % (" ".join("%.17g" % v for v in a), " ".join("%.17g" % v for v in b)))


def run_tool(exe, path):
    p = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert p.returncode == 0, (p.returncode, p.stderr.decode()[-2000:])
    assert b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr, p.stderr.decode()[-2000:]
    out = {}
    for line in p.stdout.decode().splitlines():
        key, *vals = line.split()
        out[key] = vals
    return out


def check_tool(out, want, what):
    for key in ("status", "best_hypothesis", "n_inliers_hypothesis", "n_inliers", "n_degenerate"):
        assert int(out[key][0]) == want[key], (what, key, out[key], want[key])
    assert np.array_equal(np.array(out["mask"], int), want["mask"]), what
    d = np.abs(np.array(out["t"], float) - want["t"]).max()
    dw = np.abs(np.array(out["t_winner"], float) - want["t_winner"]).max()
    print("%s: |dt| %.2e, winner %.2e" % (what, d, dw))
    assert d <= 1e-10 and dw <= 1e-10, (what, d, dw)


@pytest.mark.parametrize("exe", [TOOL, TOOL_SAN], ids=["plain", "sanitized"])
@pytest.mark.parametrize("name", tc.CASE_NAMES)
def test_tool_equals_restatement(tmp_path, name, exe):
    c, K = tc.case(name)
    path = str(tmp_path / "case.txt")
    write_case(path, c["f_cur"], c["f_ref"], c["R"], c["thresh"], c["seed"], K)
    check_tool(run_tool(exe, path), tc.restated(name), name)


@pytest.mark.parametrize("exe", [TOOL, TOOL_SAN], ids=["plain", "sanitized"])
@pytest.mark.parametrize("what", ["pure rotation", "identical matches", "n = 1", "n = 0", "nan"])
def test_tool_on_degenerate_input(tmp_path, what, exe):
    if what == "nan":
        f_cur, f_ref, R, thresh, seed, _ = tc.nan_case()
    else:
        (f_cur, f_ref, R), thresh, seed = no_model_inputs()[what], tc.THRESH, 99
    path = str(tmp_path / "case.txt")
    write_case(path, f_cur, f_ref, R, thresh, seed, 2000)
    check_tool(run_tool(exe, path), npt.estimate_translation_ransac(f_cur, f_ref, R, thresh, seed), what)
