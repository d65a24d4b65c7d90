"""The mono bootstrap without a GPU: the NumPy restatement (tests/np_restatement_init.py) against planted geometry and the
case the reference holds, and the C++ host maths (svo_hip_init.cpp behind tests/cpp_init/init_tool) against the
restatement.  The GPU tests compare the kernel with the same restatement on the same cases (tests/init_cases.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import init_cases as ic
import np_restatement_init as npi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL_DIR = os.path.join(ROOT, "tests", "cpp_init")
TOOL, TOOL_SAN = os.path.join(TOOL_DIR, "init_tool"), os.path.join(TOOL_DIR, "init_tool_san")


@pytest.fixture(scope="module", autouse=True)
def tools():
    """The two tools, made here when build() has not left them (they need the compiler only); nothing to do otherwise."""
    subprocess.check_call(["make", "-s", "-C", TOOL_DIR, "init_tool", "init_tool_san"])


# ---------------------------------------------------------------- the estimator's restatement
def test_mix_is_splitmix64():
    # the first three outputs of splitmix64 seeded with 0 (Vigna's reference values)
    x, out = np.uint64(0), []
    for _ in range(3):
        out.append(int(npi.mix(x)))
        with np.errstate(over="ignore"):
            x = x + np.uint64(0x9E3779B97F4A7C15)
    assert out == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]


def test_samples_are_four_different_indices_and_bounded():
    for n in (4, 5, 64, 1024):
        idx, ok = npi.sample_indices(77, 500, n)
        assert ok.all() or n == 4
        good = idx[ok]
        assert ((good >= 0) & (good < n)).all()
        assert all(len(set(row)) == 4 for row in good)
    # the first index of hypothesis h is its draw d = 0
    idx, _ = npi.sample_indices(5, 3, 1000)
    for h in range(3):
        assert idx[h, 0] == int(npi.mix(np.uint64(5) ^ npi.mix(np.uint64(h << 8)))) % 1000


@pytest.mark.parametrize("name", ic.CASE_NAMES)
def test_no_case_of_the_gpu_test_is_a_rounding_tie(name):
    """Both gaps of every case the GPU test compares exactly: no error of any hypothesis, and none under the refined H,
    lies within 1e-9 (relative) of the threshold; no lambda lies that close to its bound either."""
    r = ic.restated(name)
    print("%s: gap_hyp %.2e gap_final %.2e gap_lambda %.2e, %d degenerate" % (name, r["gap_hyp"], r["gap_final"], r["gap_lambda"], r["n_degenerate"]))
    assert r["status"] == npi.STATUS_OK
    assert r["gap_hyp"] >= 1e-9 and r["gap_final"] >= 1e-9 and r["gap_lambda"] >= 1e-9


def test_estimator_finds_the_planted_inliers():
    c, K = ic.case("n255")
    r = ic.restated("n255")
    inl = ~c["is_outlier"]
    # every match the estimator keeps is a planted inlier up to the few outliers that fall near their prediction by chance,
    # and it keeps nearly all of them (0.3 px of noise against a 2 px threshold)
    assert r["mask"][inl].sum() >= 0.95 * inl.sum()
    assert r["mask"][~inl].sum() <= 2
    Ht = c["R"] + np.outer(c["t"], c["normal"]) / c["d"]
    assert np.abs(r["H"] - Ht / Ht[2, 2]).max() < 5e-3


def test_four_matches_are_fitted_exactly():
    r = ic.restated("n4")
    assert (r["n_inliers_hypothesis"], r["n_inliers"], r["best_hypothesis"]) == (4, 4, 0)


# ---------------------------------------------------------------- decomposition and selection
def rot_dist(A, B):
    return np.abs(A - B).max()


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_planted_motion_is_among_the_four(seed):
    c = ic.make_case(seed, 50, noise_px=0.0, outlier_fraction=0.0)
    H = (c["R"] + np.outer(c["t"], c["normal"]) / c["d"]) * (0.3 + seed)   # any scale
    motions = npi.decompose_homography(H)
    assert len(motions) == 4
    err = [max(rot_dist(R, c["R"]), np.abs(t - c["t"] / c["d"]).max(), np.abs(n - c["normal"]).max()) for (R, t, n) in motions]
    assert min(err) <= 1e-9, err


# Two of the four motions put the plane in front of the camera for the points near the optical axis; which of them is the
# planted one is decided by the cheirality scores when the false normal turns some matches away (ratio of the two best
# scores below 0.9), else by the capped Sampson sums.  The Sampson stage is restated as the reference has it (E = R [t]x,
# its own normalisation) and cannot tell the two apart for points ON the plane, which satisfy both epipolar geometries; so
# "the planted motion is selected" is asserted where the cheirality scores decide, and "one of the two" where they do not.
DECISIVE_SEEDS = (2, 3, 8, 9, 10)
AMBIGUOUS_SEEDS = (6, 7, 29)


def planted(seed):
    c = ic.make_case(seed, 50, noise_px=0.0, outlier_fraction=0.0)
    return c, c["R"] + np.outer(c["t"], c["normal"]) / c["d"]


@pytest.mark.parametrize("seed", DECISIVE_SEEDS)
def test_selected_motion_is_the_planted_one(seed):
    c, H = planted(seed)
    s = npi.select_motion(H, c["f_cur"], c["f_ref"], np.ones(50, bool), c["thresh"])
    best = sorted(s["cheirality"], reverse=True)
    assert best[1] / best[0] < 0.9, "not a case the cheirality scores decide"
    assert s["ok"] and s["score"] == 50
    assert rot_dist(s["R"], c["R"]) <= 1e-9
    tn, tp = s["t"] / np.linalg.norm(s["t"]), c["t"] / np.linalg.norm(c["t"])
    assert np.abs(tn - tp).max() <= 1e-9          # t up to scale, same sign
    assert np.abs(s["n"] - c["normal"]).max() <= 1e-9


@pytest.mark.parametrize("seed", AMBIGUOUS_SEEDS)
def test_ambiguous_selection_is_one_of_the_two_motions_in_front(seed):
    c, H = planted(seed)
    s = npi.select_motion(H, c["f_cur"], c["f_ref"], np.ones(50, bool), c["thresh"])
    assert sorted(s["cheirality"]) == [0.0, 0.0, 50.0, 50.0]
    assert s["ok"] and s["cheirality"][s["picked"]] == 50.0


@pytest.mark.parametrize("name", ["n65", "n255"])
def test_selection_after_the_estimator_on_noisy_matches(name):
    """0.3 px of noise and 30 % gross outliers: the estimator's H, its mask and the selection give the motion of the four
    that is nearest to the planted one (cases the cheirality scores decide)."""
    c, _ = ic.case(name)
    r = ic.restated(name)
    s = npi.select_motion(r["H"], c["f_cur"], c["f_ref"], r["mask"], c["thresh"])
    best = sorted(s["cheirality"], reverse=True)
    assert best[1] / best[0] < 0.9, "not a case the cheirality scores decide"
    tp = c["t"] / np.linalg.norm(c["t"])
    d = [rot_dist(R, c["R"]) + np.abs(t / np.linalg.norm(t) - tp).max() for (R, t, n) in npi.decompose_homography(r["H"])]
    assert s["ok"] and s["picked"] == int(np.argmin(d))


def test_pure_rotation_has_no_four_motions_and_scores_zero():
    R = ic.rodrigues([0.02, -0.05, 0.01])
    assert len(npi.decompose_homography(R * 1.7)) == 1
    c = ic.make_case(3, 20)
    s = npi.select_motion(R, c["f_cur"], c["f_ref"], np.ones(20, bool), c["thresh"])
    assert not s["ok"] and s["score"] == 0.0


# ---------------------------------------------------------------- the case the reference holds
def test_held_case_fixture_is_the_reference_data():
    z = np.load(ic.HELD_PATH)
    assert z["f_ref"].shape == z["f_cur"].shape == (70, 3)
    assert float(z["focal_length"]) == 386.711 and int(z["reference_inliers"]) == 69 and float(z["reproj_error_thresh"]) == 2.0
    assert np.abs(np.linalg.norm(z["f_ref"], axis=1) - 1).max() < 1e-5     # unit bearing vectors, six digits
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_homography_held_case as gen
    text = ("f_ref.resize(Eigen::NoChange,70);\n" + "".join("  f_ref.col(i++) = Vector3d(%r, %r, %r);\n" % tuple(float(x) for x in v) for v in z["f_ref"])
            + "  i = 0;\n" + "".join("  f_cur.col(i++) = Vector3d(%r, %r, %r);\n" % tuple(float(x) for x in v) for v in z["f_cur"])
            + "  focal_length = 386.711;\n  double reproj_error_thresh = 2.0;\n  EXPECT_EQ(inliers.size(), 69);\n")
    again = gen.parse(text)
    for k in ("f_ref", "f_cur", "focal_length", "reference_inliers", "reproj_error_thresh"):
        assert np.array_equal(again[k], z[k]), k


def held_selection():
    c, _ = ic.case("held")
    r = ic.restated("held")
    return c, r, npi.select_motion(r["H"], c["f_cur"], c["f_ref"], r["mask"], c["thresh"])


def test_held_case_against_the_reference_count():
    """vk::computeInliers at 2 px for the restatement's motion: within 3 of the 69 the reference asserts with OpenCV's
    estimator.  (Hypothesis 1575 wins with 65 inliers, 64 after the refinement; cheirality 0 / 64 / 0 / 64.)"""
    c, r, s = held_selection()
    assert (r["best_hypothesis"], r["n_inliers_hypothesis"], r["n_inliers"]) == (1575, 65, 64)
    assert s["cheirality"] == [0.0, 64.0, 0.0, 64.0]
    n = len(npi.compute_inliers(c["f_cur"], c["f_ref"], s["R"], s["t"], c["thresh_px"], c["focal"]))
    print("computeInliers at 2 px: %d of 70 (the reference asserts %d)" % (n, c["reference_inliers"]))
    assert abs(n - c["reference_inliers"]) <= 3


def test_one_refinement_round_is_the_fixed_point_on_the_held_case():
    c, r, _ = held_selection()
    H2, _ = npi.refine(r["H"], c["uv_ref"], c["uv_cur"], r["mask"].astype(bool))
    m2, _ = npi.inlier_test(H2, c["uv_ref"], c["uv_cur"], c["thresh"])
    assert np.array_equal(m2.astype(np.uint8), r["mask"])


def test_decomposition_is_well_conditioned_on_the_held_case():
    """A relative change of H of 1e-9 (the GPU test's bound on H) moves the selected motion by less than 1e-6: the bound
    tests/test_homography_ransac_gpu.py::test_held_case_motion_and_count puts on R and t."""
    c, r, s = held_selection()
    rng = np.random.RandomState(0)
    worst = 0.0
    for _ in range(20):
        Hp = r["H"] + 1e-9 * np.abs(r["H"]).max() * rng.uniform(-1, 1, (3, 3))
        sp = npi.select_motion(Hp, c["f_cur"], c["f_ref"], r["mask"], c["thresh"])
        assert sp["picked"] == s["picked"]
        worst = max(worst, np.abs(sp["R"] - s["R"]).max(), np.abs(sp["t"] - s["t"]).max())
    print("largest change of the motion: %.2e" % worst)
    assert worst <= 1e-6


# ---------------------------------------------------------------- triangulation and rescale
def test_triangulation_and_rescale_recover_the_planted_structure():
    c = ic.make_case(11, 60, noise_px=0.0, outlier_fraction=0.0)
    matches = [(i, i) for i in range(60)]
    kept, pts = npi.triangulate_points(c["f_cur"], c["f_ref"], c["R"], c["t"], 1e-3, matches)
    assert kept == matches
    ray = c["f_ref"] / c["f_ref"][:, 2:3]
    X_ref = ray * (c["d"] / (ray @ c["normal"]))[:, None]
    assert np.abs(pts - (X_ref @ c["R"].T + c["t"])).max() < 1e-9
    depth = 7.5
    R_ref_w, t_ref_w = ic.rodrigues([0.1, 0.2, -0.3]), np.array([0.5, -1.0, 2.0])
    scale, R_cw, t_cw, world = npi.rescale_and_initialize_points(pts, c["R"], c["t"], R_ref_w, t_ref_w, depth)
    med = np.sort(np.linalg.norm(pts, axis=1))[30]
    assert abs(scale - depth / med) < 1e-12
    # the points seen from the rescaled current frame are the triangulated ones times the scale
    assert np.abs(world @ R_cw.T + t_cw - pts * scale).max() < 1e-9
    # the baseline is scaled, the reference frame stays
    pos_ref, pos_cur = -R_ref_w.T @ t_ref_w, -R_cw.T @ t_cw
    assert abs(np.linalg.norm(pos_cur - pos_ref) - scale * np.linalg.norm(c["t"])) < 1e-9


# ---------------------------------------------------------------- the C++ host maths against the restatement
def write_case(path, H, c, mask, depth, angle, T_ref_world, ids1=(), ids2=(), disp=(), pivot=0.5, px=2.0):
    with open(path, "w") as f:
        f.write("H " + " ".join(repr(float(v)) for v in np.asarray(H).ravel()) + "\n")
        f.write("thresh %r\ndepth %r\nangle %r\npivot %r\nfocal %r\npx %r\n" % (float(c["thresh"]), float(depth), float(angle), float(pivot), float(c["focal"]), float(px)))
        f.write("T_ref_world " + " ".join(repr(float(v)) for v in T_ref_world) + "\n")
        for i in range(c["f_cur"].shape[0]):
            f.write("match " + " ".join(repr(float(v)) for v in list(c["f_cur"][i]) + list(c["f_ref"][i])) + " %d\n" % int(mask[i]))
        if len(ids1):
            f.write("ids1 " + " ".join(str(int(v)) for v in ids1) + "\n")
        if len(ids2):
            f.write("ids2 " + " ".join(str(int(v)) for v in ids2) + "\n")
        if len(disp):
            f.write("disp " + " ".join(repr(float(v)) for v in disp) + "\n")


def run_tool(exe, path):
    p = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert p.returncode == 0, (p.returncode, p.stderr.decode()[-2000:])
    assert b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr, p.stderr.decode()[-2000:]
    out = {}
    for line in p.stdout.decode().splitlines():
        key, _, rest = line.partition(" ")
        out.setdefault(key, []).append(rest.split())
    return out


def floats(tokens):
    return np.array([float(t) for t in tokens])


def quat_to_R(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def close(a, b, what):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape, what
    scale = max(1.0, np.abs(b).max()) if b.size else 1.0
    assert np.abs(a - b).max() <= 1e-10 * scale if b.size else True, (what, np.abs(a - b).max())


@pytest.mark.parametrize("name", ["held", "n65", "n255"])
def test_host_maths_equal_the_restatement(tmp_path, name):
    c, _ = ic.case(name)
    r = ic.restated(name)
    rng = np.random.RandomState(5)
    depth, angle = 3.25, np.arctan(2.0 / (2 * c["focal"])) * 2
    R_ref_w, t_ref_w = ic.rodrigues([0.3, -0.2, 0.1]), np.array([0.2, 0.4, -0.6])
    # quaternion of R_ref_w (w first), for the tool
    w = np.sqrt(1 + np.trace(R_ref_w)) / 2
    q = np.array([w, (R_ref_w[2, 1] - R_ref_w[1, 2]) / (4 * w), (R_ref_w[0, 2] - R_ref_w[2, 0]) / (4 * w), (R_ref_w[1, 0] - R_ref_w[0, 1]) / (4 * w)])
    ids1 = rng.permutation(60)[:40] - 5            # some negative: no track
    ids2 = rng.permutation(60)[:45] - 5
    disp = rng.uniform(0, 80, 37)
    path = str(tmp_path / "case.txt")
    write_case(path, r["H"] * 1.3, c, r["mask"], depth, angle, list(q) + list(t_ref_w), ids1, ids2, disp, pivot=0.35)
    out = run_tool(TOOL, path)

    close(floats(out["singular_values"][0]), np.linalg.svd(r["H"] * 1.3, compute_uv=False), "singular values")
    motions = npi.decompose_homography(r["H"] * 1.3)
    assert int(out["n_motions"][0][0]) == len(motions) == 4
    for k, (R, t, n) in enumerate(motions):
        close(floats(out["motion_R"][k]).reshape(3, 3), R, "R %d" % k)
        close(floats(out["motion_t"][k]), t, "t %d" % k)
        close(floats(out["motion_n"][k]), n, "n %d" % k)
    s = npi.select_motion(r["H"] * 1.3, c["f_cur"], c["f_ref"], r["mask"], c["thresh"])
    assert [float(v) for v in out["cheirality"][0]] == s["cheirality"]
    assert int(out["picked"][0][0]) == s["picked"] and float(out["score"][0][0]) == s["score"]
    close(floats(out["selected_R"][0]).reshape(3, 3), s["R"], "selected R")
    close(floats(out["selected_t"][0]), s["t"], "selected t")

    matches = [(i, i) for i in range(c["f_cur"].shape[0])]
    kept, pts = npi.triangulate_points(c["f_cur"], c["f_ref"], s["R"], s["t"], angle, matches)
    assert [int(v) for v in out["triangulated"][0]] == [m[0] for m in kept]
    close(floats(out["points_in_cur"][0]).reshape(-1, 3), pts, "points in cur")
    scale, R_cw, t_cw, world = npi.rescale_and_initialize_points(pts, s["R"], s["t"], R_ref_w, t_ref_w, depth)
    close(float(out["scale"][0][0]), scale, "scale")
    T = floats(out["T_cur_world"][0])
    close(quat_to_R(T[:4]), R_cw, "R_cur_world")
    close(T[4:], t_cw, "t_cur_world")
    close(floats(out["points_in_world"][0]).reshape(-1, 3), world, "points in world")
    inl = npi.compute_inliers(c["f_cur"], c["f_ref"], s["R"], s["t"], 2.0, c["focal"])
    assert [int(v) for v in out["compute_inliers"][0]] == inl

    d = np.sort(disp)[::-1]
    assert float(out["disparity_percentile"][0][0]) == d[int(np.floor(0.35 * d.size))]
    slot1 = {int(t): i for i, t in enumerate(ids1) if t >= 0}
    want = ["%d:%d" % (slot1[int(t)], i) for i, t in enumerate(ids2) if t >= 0 and int(t) in slot1]
    assert out["feature_matches"][0] == want


def degenerate_case(kind):
    c = ic.make_case(21, 30)
    H, mask = ic.restated("n65")["H"], np.ones(30, np.uint8)
    if kind == "rotation":
        H = ic.rodrigues([0.03, 0.01, -0.02])
    elif kind in ("n0", "n1", "n2"):
        k = int(kind[1])
        c = dict(c, f_cur=c["f_cur"][:k], f_ref=c["f_ref"][:k])
        mask = mask[:k]
    elif kind == "nan":
        c = dict(c, f_cur=c["f_cur"].copy(), f_ref=c["f_ref"].copy())
        c["f_cur"][3, 0] = np.nan
        c["f_ref"][7] = np.nan
        c["f_cur"][11, 2] = np.inf
    elif kind == "nan_H":
        H = np.full((3, 3), np.nan)
    return H, c, mask


@pytest.mark.parametrize("kind", ["rotation", "n0", "n1", "n2", "nan", "nan_H"])
def test_host_maths_under_sanitizers_on_degenerate_input(tmp_path, kind):
    """tests/cpp_init/init_tool_san (address + undefined behaviour, host code only, run directly): a pure rotation, fewer
    matches than anything needs, bearing vectors that are not numbers.  No report, exit 0, and a refusal where the
    reference would abort."""
    H, c, mask = degenerate_case(kind)
    path = str(tmp_path / "case.txt")
    disp = [] if kind == "n0" else [1.0, np.nan, 3.0] if kind == "nan" else [2.0]
    write_case(path, H, c, mask, 2.0, 0.005, [1, 0, 0, 0, 0, 0, 0], ids1=[0, 1, -1], ids2=[1, 1, 5], disp=disp)
    out = run_tool(TOOL_SAN, path)
    if kind == "rotation":
        assert int(out["n_motions"][0][0]) == 1 and float(out["score"][0][0]) == 0.0 and int(out["picked"][0][0]) == -1
    if kind in ("n0", "n1"):
        assert "rescale_refused" in out or float(out["score"][0][0]) == 0.0
    if kind == "n0":
        assert float(out["disparity_percentile"][0][0]) == 0.0
    assert out["feature_matches"][0] == ["1:0", "1:1"]
