"""Seeded cases of the essential-matrix estimator (the FivePoint initialiser) shared by tests/test_fivepoint_cpu.py and
tests/test_essential_ransac_gpu.py: the scenes of tests/twopoint_cases.py (points at depths of 2 - 8 m or on one plane, a
rotation of 1.5 degrees, a translation of 0.46 m, 0.3 px of noise at a focal length of 400 px, 30 % gross outliers; none
at n = 5 and n = 6).  The restatement's result of every case is computed once per session, and once more with its
null-space basis turned by a fixed orthogonal matrix: what the two runs do not agree on to the last bit is what no other
writing of the estimator can be asked to reproduce."""
import functools

import numpy as np

import np_restatement_fivepoint as np5
import twopoint_cases as tc

THRESH = tc.THRESH
# the sizes at which the kernel takes another path: the smallest problem and one more, one wave +- 1, one pass of the 256
# threads +- 1, the LDS limit, at two passes of the workgroup over the hypotheses; the hypothesis counts: one, one pass of
# the workgroup +- 1, the default
SIZES = (5, 6, 63, 64, 65, 255, 256, 257, 1024)
K_FOR_SIZES = 512
HYPOTHESES = (1, 255, 256, 257, 2000)
N_FOR_HYPOTHESES = 65
# per case its scene seed, chosen so that the premises tests/test_fivepoint_cpu.py asserts hold for it
SCENE_SEEDS = {"n5": 1, "n6": 101, "n63": 201, "n64": 301, "n65": 401, "n255": 501, "n256": 601, "n257": 701, "n1024": 801,
               "plane": 901, "k1": 1001, "k255": 1101, "k256": 1201, "k257": 1301, "k2000": 1401, "nan": 1501}
# the model is not unique at these sizes (several essential matrices fit five matches exactly): no comparison of R and t
MODEL_NOT_UNIQUE = ("n5", "n6")
# R and t of the kernel against the restatement: 100 times the largest difference between the restatement's two runs over
# the cases (tests/test_fivepoint_cpu.py prints and asserts it), never below the 1e-9 of the other two estimators
MODEL_BAR = 1e-9

_q, _r = np.linalg.qr(np.random.RandomState(4242).randn(4, 4))
TURN = _q * np.sign(np.diag(_r))                                       # a fixed orthogonal 4 x 4


def make_case(seed, n, plane=False, outlier_fraction=tc.OUTLIER_FRACTION):
    """twopoint_cases.make_case; no outliers below seven matches."""
    return tc.make_case(seed, n, plane=plane, outlier_fraction=outlier_fraction if n > 6 else 0.0)


def names():
    return tuple("n%d" % n for n in SIZES) + ("plane", ) + tuple("k%d" % k for k in HYPOTHESES)


CASE_NAMES = names()
RAGGED_BATCH = ("n5", "n6", "n63", "n64", "n65", "plane", "n255", "n256", "n257", "n1024")


def shape_of(name):
    """(n, K, plane) of a case name: 'n<size>' (512 hypotheses), 'k<hypotheses>' (65 matches) or 'plane' (200 matches, 2000)."""
    if name == "plane":
        return 200, 2000, True
    if name[0] == "n":
        return int(name[1:]), K_FOR_SIZES, False
    return N_FOR_HYPOTHESES, int(name[1:]), False


@functools.lru_cache(maxsize=None)
def case(name):
    """(case, K)."""
    n, K, plane = shape_of(name)
    return make_case(SCENE_SEEDS[name], n, plane=plane), K


@functools.lru_cache(maxsize=None)
def restated(name, turned=False):
    """The restatement's result of a case (turned: with the null-space basis turned); computed once, shared, never changed."""
    c, K = case(name)
    return np5.estimate_essential_ransac(c["f_cur"], c["f_ref"], c["thresh"], c["seed"], K, basis_turn=TURN if turned else None)


def nan_case():
    """100 matches, one planted inlier made NaN: (f_cur, f_ref, thresh, seed, k)."""
    c = make_case(SCENE_SEEDS["nan"], 100)
    f_cur, f_ref = c["f_cur"].copy(), c["f_ref"].copy()
    k = int(np.flatnonzero(~c["is_outlier"])[3])
    f_cur[k, 0] = np.nan
    f_ref[k, 1] = np.nan
    return f_cur, f_ref, c["thresh"], c["seed"], k


def no_model_inputs():
    c = make_case(55, 40, outlier_fraction=0.0)
    rot = c["f_ref"] @ c["R"].T                                    # the camera only turned
    return {"pure rotation": (rot, c["f_ref"]), "identical matches": (np.tile(c["f_cur"][:1], (40, 1)), np.tile(c["f_ref"][:1], (40, 1))),
            "n = 4": (c["f_cur"][:4], c["f_ref"][:4]), "n = 0": (c["f_cur"][:0], c["f_ref"][:0])}


def model_difference(a, b):
    return float(max(np.abs(a["R"] - b["R"]).max(), np.abs(a["t"] - b["t"]).max()))


def premises(a, b, f_cur, f_ref, thresh, model_unique=True):
    """The premises of an exact comparison from the restatement's two runs a and b (tests/test_fivepoint_cpu.py states
    them).  Returns (ok, what was measured)."""
    m = dict(elim=min(a["elim_smin"], b["elim_smin"]), same=False, tie_ok=False, gap=np.inf, gap_ok=False, sample=np.inf, steps_ok=True, model_diff=np.inf, motion_unique=False)
    keys = ("status", "best_hypothesis", "n_inliers_hypothesis", "n_inliers", "n_degenerate", "refine_iters")
    if not model_unique:
        keys = ("status", "n_inliers_hypothesis", "n_inliers", "n_degenerate")
    m["same"] = all(a[k] == b[k] for k in keys) and np.array_equal(a["mask"], b["mask"])
    if a["status"] != np5.STATUS_OK or not m["same"]:
        return False, m
    m["motion_unique"] = a["motion_unique"] and b["motion_unique"]
    m["sample"] = float(max(np.abs(a["sample_err"]).max(), np.abs(b["sample_err"]).max()) / thresh)
    m["model_diff"] = model_difference(a, b)
    if not model_unique:
        ok = m["motion_unique"] and m["elim"] >= 1e-8
        return ok, m
    h, cnt = a["best_hypothesis"], a["n_inliers_hypothesis"]
    in_h = a["cand_count"][a["cand_h"] == h]
    m["tie_ok"] = int((in_h == cnt).sum()) == 1 and not np.any(a["cand_count"][a["cand_h"] < h] >= cnt)
    gap_ok, gap_min = True, np.inf
    pairs = [(a["R_winner"], a["t_winner"], b["R_winner"], b["t_winner"]), (a["R"], a["t"], b["R"], b["t"])]
    near = np.flatnonzero((a["cand_h"] <= h) & (a["cand_count"] >= cnt - 1))
    for i in near:
        js = np.flatnonzero(b["cand_h"] == a["cand_h"][i])
        if len(js) == 0:
            return False, m
        d = [max(np.abs(b["cand_R"][j] - a["cand_R"][i]).max(), np.abs(b["cand_t"][j] - a["cand_t"][i]).max()) for j in js]
        j = js[int(np.argmin(d))]
        if b["cand_count"][j] != a["cand_count"][i]:
            return False, m
        pairs.append((a["cand_R"][i], a["cand_t"][i], b["cand_R"][j], b["cand_t"][j]))
    for Ra, ta, Rb, tb in pairs:
        ea, _ = np5.errors(Ra[None], ta[None], f_cur, f_ref)
        eb, _ = np5.errors(Rb[None], tb[None], f_cur, f_ref)
        fin = np.isfinite(ea[0]) & np.isfinite(eb[0])
        gap = np.abs(ea[0][fin] - thresh)
        change = np.abs(ea[0][fin] - eb[0][fin])
        gap_ok = gap_ok and bool(np.all(gap >= 1000.0 * change)) and bool(np.all(gap >= 1e-7 * thresh))
        if gap.size:
            gap_min = min(gap_min, float(gap.min() / thresh))
    m["gap"], m["gap_ok"] = gap_min, gap_ok
    m["steps_ok"] = all(abs(s - 1e-10) >= 1e-13 for s in a["steps"] + b["steps"])
    ok = m["tie_ok"] and gap_ok and m["sample"] < 1e-3 and m["steps_ok"] and m["motion_unique"] and m["elim"] >= 1e-8
    return ok, m
