"""Seeded cases of the translation estimator (the TwoPoint initialiser) shared by tests/test_twopoint_cpu.py and
tests/test_translation_ransac_gpu.py: points at depths of 2 - 8 m (or on one plane), a rotation of 1.5 degrees that is
given to the estimator as its prior, a translation of 0.46 m, 0.3 px of noise at a focal length of 400 px, 30 % gross
outliers.  The restatement's result of every case is computed once per session."""
import functools

import numpy as np

import np_restatement_twopoint as npt
from init_cases import rodrigues

FOCAL = 400.0
THRESH_PX = 2.0
NOISE_PX = 0.3
OUTLIER_FRACTION = 0.3
# TwoPointInit's threshold: 1 - cos(getAngleError(reproj_error_thresh)), the angle error of a pinhole projection
ANGLE_ERROR = np.arctan(THRESH_PX / (2.0 * FOCAL)) + np.arctan(THRESH_PX / (2.0 * FOCAL))
THRESH = 1.0 - np.cos(ANGLE_ERROR)

# the sizes at which the kernel takes another path: the smallest problem and one more, one wave +- 1, one pass of the 256
# threads +- 1, the LDS limit; the hypothesis counts: one, one pass of the workgroup +- 1, the default
SIZES = (2, 3, 63, 64, 65, 255, 256, 257, 1024)
HYPOTHESES = (1, 255, 256, 257, 2000)
N_FOR_HYPOTHESES = 65
# per case its scene seed (100 * its position + 1); tests/test_twopoint_cpu.py asserts that the premises of an exact
# comparison hold for every one of them
SCENE_SEEDS = {"n2": 1, "n3": 101, "n63": 201, "n64": 301, "n65": 401, "n255": 501, "n256": 601, "n257": 701, "n1024": 801,
               "plane": 901, "k1": 1001, "k255": 1101, "k256": 1201, "k257": 1301, "k2000": 1401, "nan": 1501}


def make_case(seed, n, plane=False, noise_px=NOISE_PX, outlier_fraction=OUTLIER_FRACTION):
    """dict(f_ref, f_cur [n,3] unit bearings, R (the prior: the true rotation), t (true, t_cur_ref), thresh, seed,
    is_outlier)."""
    rng = np.random.RandomState(seed)
    axis = rng.randn(3)
    R = rodrigues(np.deg2rad(1.5) * axis / np.linalg.norm(axis))
    t = np.array([0.42, 0.15, 0.08]) + 0.04 * rng.randn(3)
    t *= 0.46 / np.linalg.norm(t)
    uv_ref = np.stack([rng.uniform(-0.6, 0.6, n), rng.uniform(-0.45, 0.45, n)], axis=1)
    ray = np.concatenate([uv_ref, np.ones((n, 1))], axis=1)
    if plane:
        normal = np.array([0.15 * rng.randn(), 0.15 * rng.randn(), 1.0])
        normal /= np.linalg.norm(normal)
        X_ref = ray * ((3.0 + rng.rand()) / (ray @ normal))[:, None]
    else:
        X_ref = ray * rng.uniform(2.0, 8.0, n)[:, None]
    X_cur = X_ref @ R.T + t
    uv_cur = X_cur[:, :2] / X_cur[:, 2:3]
    uv_ref = uv_ref + rng.randn(n, 2) * (noise_px / FOCAL)
    uv_cur = uv_cur + rng.randn(n, 2) * (noise_px / FOCAL)
    n_out = int(round(outlier_fraction * n)) if n > 4 else 0
    is_outlier = np.zeros(n, bool)
    is_outlier[rng.permutation(n)[:n_out]] = True
    uv_cur[is_outlier] = np.stack([rng.uniform(-0.6, 0.6, n_out), rng.uniform(-0.45, 0.45, n_out)], axis=1)

    def bearings(uv):
        f = np.concatenate([uv, np.ones((uv.shape[0], 1))], axis=1)
        return f / np.linalg.norm(f, axis=1, keepdims=True)
    return dict(f_ref=bearings(uv_ref), f_cur=bearings(uv_cur), R=R, t=t, thresh=THRESH, seed=1000 + seed, is_outlier=is_outlier)


def premises_hold(r, gap=1e-7, eig=1e-2):
    """The premises of an exact comparison on a restated result (tests/test_twopoint_cpu.py states them)."""
    return (r["status"] == npt.STATUS_OK and min(r["gap_hyp"], r["gap_final"]) >= gap and r["tie_ok"] and r["eig_gap"] >= eig
            and r["gap_norm"] >= 1e-3 and r["gap_sign"] >= 1e-9)


def names():
    return tuple("n%d" % n for n in SIZES) + ("plane", ) + tuple("k%d" % k for k in HYPOTHESES)


CASE_NAMES = names()
RAGGED_BATCH = ("n2", "n3", "n63", "n64", "n65", "plane", "n255", "n256", "n257", "n1024")


def shape_of(name):
    """(n, K, plane) of a case name: 'n<size>' (2000 hypotheses), 'k<hypotheses>' (65 matches) or 'plane' (200 matches)."""
    if name == "plane":
        return 200, 2000, True
    if name[0] == "n":
        return int(name[1:]), 2000, False
    return N_FOR_HYPOTHESES, int(name[1:]), False


@functools.lru_cache(maxsize=None)
def case(name):
    """(case, K)."""
    n, K, plane = shape_of(name)
    return make_case(SCENE_SEEDS[name], n, plane=plane), K


@functools.lru_cache(maxsize=None)
def restated(name):
    """The restatement's result of a case; computed once, shared, never changed."""
    c, K = case(name)
    return npt.estimate_translation_ransac(c["f_cur"], c["f_ref"], c["R"], c["thresh"], c["seed"], K)


def nan_case():
    """100 matches, one planted inlier made NaN: (f_cur, f_ref, R, thresh, seed, k)."""
    c = make_case(SCENE_SEEDS["nan"], 100)
    f_cur, f_ref = c["f_cur"].copy(), c["f_ref"].copy()
    k = int(np.flatnonzero(~c["is_outlier"])[3])
    f_cur[k, 0] = np.nan
    f_ref[k, 1] = np.nan
    return f_cur, f_ref, c["R"], c["thresh"], c["seed"], k
