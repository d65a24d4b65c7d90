"""Seeded cases of the homography initialiser shared by tests/test_init_cpu.py and tests/test_homography_ransac_gpu.py:
a plane, a pose, n matches on the unit plane with 0.3 px of noise, 30 % of them gross outliers; and the case the reference
holds (tests/golden/homography_held_case.npz).  The restatement's result of every case is computed once per session."""
import functools
import os

import numpy as np

import np_restatement_init as npi

FOCAL = 400.0
THRESH_PX = 2.0
NOISE_PX = 0.3
OUTLIER_FRACTION = 0.3
HELD_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "homography_held_case.npz")
HELD_SEED = 12345

# the sizes at which the kernel takes another path: fewer matches than a wave, one wave +- 1, one pass of the 256 threads
# +- 1, the LDS limit; the hypothesis counts: one, one pass of the workgroup +- 1, the default
SIZES = (4, 5, 63, 64, 65, 255, 257, 1024)
HYPOTHESES = (1, 255, 256, 257, 2000)
N_FOR_HYPOTHESES = 65


def rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = npi.skew(np.asarray(w) / th)
    return np.eye(3) + np.sin(th) * k + (1 - np.cos(th)) * (k @ k)


def make_case(seed, n, noise_px=NOISE_PX, outlier_fraction=OUTLIER_FRACTION):
    """dict(uv_ref, uv_cur [n,2], f_ref, f_cur [n,3] unit bearings, thresh, seed, R, t, normal, d, is_outlier)."""
    rng = np.random.RandomState(seed)
    normal = np.array([0.15 * rng.randn(), 0.15 * rng.randn(), 1.0])
    normal /= np.linalg.norm(normal)
    d = 2.0 + rng.rand()
    R = rodrigues(0.08 * rng.randn(3))
    t = np.array([0.35, 0.1, 0.05]) + 0.05 * rng.randn(3)
    uv_ref = np.stack([rng.uniform(-0.6, 0.6, n), rng.uniform(-0.45, 0.45, n)], axis=1)
    ray = np.concatenate([uv_ref, np.ones((n, 1))], axis=1)
    X_ref = ray * (d / (ray @ normal))[:, None]            # on the plane normal . X = d of the ref frame
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
    return dict(uv_ref=uv_ref, uv_cur=uv_cur, f_ref=bearings(uv_ref), f_cur=bearings(uv_cur), thresh=THRESH_PX / FOCAL,
                seed=1000 + seed, R=R, t=t, normal=normal, d=d, is_outlier=is_outlier, focal=FOCAL)


@functools.lru_cache(maxsize=None)
def held_case():
    z = np.load(HELD_PATH)
    f_ref, f_cur = z["f_ref"], z["f_cur"]
    focal = float(z["focal_length"])
    return dict(uv_ref=f_ref[:, :2] / f_ref[:, 2:3], uv_cur=f_cur[:, :2] / f_cur[:, 2:3], f_ref=f_ref, f_cur=f_cur,
                thresh=float(z["reproj_error_thresh"]) / focal, seed=HELD_SEED, focal=focal,
                thresh_px=float(z["reproj_error_thresh"]), reference_inliers=int(z["reference_inliers"]))


@functools.lru_cache(maxsize=None)
def case(name):
    """'n<size>' (2000 hypotheses), 'k<hypotheses>' (65 matches) or 'held': (case, K)."""
    if name == "held":
        return held_case(), 2000
    if name[0] == "n":
        return make_case(int(name[1:]), int(name[1:])), 2000
    return make_case(7000 + int(name[1:]), N_FOR_HYPOTHESES), int(name[1:])


CASE_NAMES = tuple("n%d" % n for n in SIZES) + ("held",) + tuple("k%d" % k for k in HYPOTHESES)
RAGGED_BATCH = ("n4", "n5", "n63", "n64", "n65", "held", "n255", "n257", "n1024")


@functools.lru_cache(maxsize=None)
def restated(name):
    """The restatement's result of a case; computed once, shared, never changed."""
    c, K = case(name)
    return npi.estimate_homography_ransac(c["uv_ref"], c["uv_cur"], c["thresh"], c["seed"], K)
