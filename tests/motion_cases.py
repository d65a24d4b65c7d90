"""A grid of camera motions for the three mono-bootstrap estimators, shared by tests/test_motion_grid_cpu.py and
tests/test_motion_grid_gpu.py.  The cases of tests/twopoint_cases.py, tests/fivepoint_cases.py and tests/init_cases.py all
come from one family (a small rotation, a mostly sideways translation, pinhole bearings, 0.3 px of noise); here the
rotation, the translation, the noise, the share of outliers, the depths, the plane and the field of view are given, not
drawn: forward and backward motion, exactly no rotation, axis-aligned translations, large rotations, a short baseline,
noise-free matches, bearings behind the image plane.  The noise is added after the exact projection, so noise_px = 0 gives
exact bearings.  The restatements' results are computed once per session."""
import functools

import numpy as np

import fivepoint_cases as fc
import init_cases as ic
import np_restatement_fivepoint as np5
import np_restatement_init as npi
import np_restatement_twopoint as npt
import twopoint_cases as tc

FOCAL = tc.FOCAL
THRESH = tc.THRESH                                                     # the two bearing estimators' (1 - cos)
THRESH_H = ic.THRESH_PX / ic.FOCAL                                     # the homography's, on the unit plane
N, K = 100, 512
PINHOLE = (0.6, 0.45)                                                  # |u|, |v| on the unit plane
WIDE_DEG = 100.0                                                       # bearings up to this angle off the optical axis


def rot(axis, deg):
    a = np.asarray(axis, np.float64)
    return ic.rodrigues(np.deg2rad(deg) * a / np.linalg.norm(a))


def rot90z():
    return np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])   # exact: no sine or cosine rounded


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def tangent_noise(f, d):
    """Unit bearings moved by d [n,2] (radians) in their tangent planes; unchanged where d is all zero."""
    if not d.any():
        return f
    a = np.where(np.abs(f[:, :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    b1 = unit(np.cross(f, a))
    b2 = np.cross(f, b1)
    return unit(f + b1 * d[:, :1] + b2 * d[:, 1:])


def make_scene(seed, n, R, t, noise_px=0.0, outlier_fraction=0.0, depth=(2.0, 8.0), plane=None, fov=PINHOLE):
    """dict(f_ref, f_cur [n,3] unit bearings, R, t (t_cur_ref, as given), thresh, seed, is_outlier, and for a pinhole field
    of view uv_ref, uv_cur).  fov: (|u|, |v|) of a pinhole image on the unit plane, or an angle in degrees: bearings drawn
    uniformly on the cap of that half-angle about the optical axis (built from angles, never from uv).  plane: None or
    (normal, d): the points lie on normal . X = d of the reference frame."""
    rng = np.random.RandomState(seed)
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    pinhole = not np.isscalar(fov)
    if pinhole:
        uv = np.stack([rng.uniform(-fov[0], fov[0], n), rng.uniform(-fov[1], fov[1], n)], axis=1)
        ray = unit(np.concatenate([uv, np.ones((n, 1))], axis=1))
    else:
        theta = np.arccos(rng.uniform(np.cos(np.deg2rad(fov)), 1.0, n))
        phi = rng.uniform(-np.pi, np.pi, n)
        ray = np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], axis=1)
    if plane is not None:
        normal, d = unit(plane[0]), float(plane[1])
        X_ref = ray * (d / (ray @ normal))[:, None]
    else:
        X_ref = ray * rng.uniform(depth[0], depth[1], n)[:, None]
    X_cur = X_ref @ R.T + t
    f_ref, f_cur = unit(X_ref), unit(X_cur)                            # the exact projection
    sigma = noise_px / FOCAL
    noise = rng.randn(2, n, 2) * sigma                                 # drawn in the order of twopoint_cases.make_case
    n_out = int(round(outlier_fraction * n)) if n > 6 else 0
    is_outlier = np.zeros(n, bool)
    is_outlier[rng.permutation(n)[:n_out]] = True
    out = dict(R=R, t=t, thresh=THRESH, seed=1000 + seed, is_outlier=is_outlier)
    if pinhole:
        uv_ref, uv_cur = f_ref[:, :2] / f_ref[:, 2:3], f_cur[:, :2] / f_cur[:, 2:3]
        if sigma != 0.0:                                               # noise-free: the bearings stay the exact ones
            uv_ref, uv_cur = uv_ref + noise[0], uv_cur + noise[1]
            f_ref = unit(np.concatenate([uv_ref, np.ones((n, 1))], axis=1))
            f_cur = unit(np.concatenate([uv_cur, np.ones((n, 1))], axis=1))
        uv_out = np.stack([rng.uniform(-fov[0], fov[0], n_out), rng.uniform(-fov[1], fov[1], n_out)], axis=1)
        uv_cur[is_outlier] = uv_out
        f_cur[is_outlier] = unit(np.concatenate([uv_out, np.ones((n_out, 1))], axis=1))
        out.update(uv_ref=uv_ref, uv_cur=uv_cur, thresh_h=THRESH_H, focal=FOCAL)
    else:
        f_ref, f_cur = tangent_noise(f_ref, noise[0]), tangent_noise(f_cur, noise[1])
        theta = np.arccos(rng.uniform(np.cos(np.deg2rad(fov)), 1.0, n_out))
        phi = rng.uniform(-np.pi, np.pi, n_out)
        f_cur[is_outlier] = np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], axis=1)
    if plane is not None:
        out.update(normal=normal, d=d)
    out.update(f_ref=f_ref, f_cur=f_cur)
    return out


_NOISY = dict(noise_px=0.3, outlier_fraction=0.3)
_PLANE_OBLIQUE = (np.sin(np.deg2rad(60.0)), 0.0, np.cos(np.deg2rad(60.0)))
# name -> the arguments of make_scene (without seed and n)
GRID = {
    "forward": dict(R=rot((1.0, -2.0, 0.5), 1.0), t=(0.008, -0.004, 0.45), **_NOISY),
    "backward": dict(R=rot((-1.0, 0.5, 2.0), 1.0), t=(-0.005, 0.007, -0.45), **_NOISY),
    "identity_y_outliers": dict(R=np.eye(3), t=(0.0, 0.4, 0.0), outlier_fraction=0.3),
    "identity_x": dict(R=np.eye(3), t=(0.4, 0.0, 0.0)),
    "identity_z": dict(R=np.eye(3), t=(0.0, 0.0, 0.4)),
    "identity_general": dict(R=np.eye(3), t=(0.4, 0.05, 0.02)),
    "rot20": dict(R=rot((0.3, 1.0, -0.2), 20.0), t=(0.4, 0.1, 0.15), **_NOISY),
    "rot45": dict(R=rot((1.0, 0.4, 0.3), 45.0), t=(-0.2, 0.35, 0.1), **_NOISY),
    "rot90z_exact": dict(R=rot90z(), t=(0.3, -0.25, 0.1), **_NOISY),
    "short_baseline": dict(R=rot((0.2, -1.0, 0.4), 1.0), t=tuple(0.01 * unit((0.8, 0.5, 0.33))), **_NOISY),
    "wide": dict(R=rot((0.5, 1.0, 0.2), 5.0), t=(0.3, 0.1, 0.25), fov=WIDE_DEG, **_NOISY),
    "plane_forward": dict(R=rot((1.0, -2.0, 0.5), 1.0), t=(0.008, -0.004, 0.45), plane=((0.0, 0.0, 1.0), 3.0), **_NOISY),
    "plane_oblique": dict(R=rot((0.3, 1.0, -0.2), 3.0), t=(0.0, 0.4, 0.05), plane=(_PLANE_OBLIQUE, 2.5), **_NOISY),
    # with the noise of the others: on exact matches of a camera that did not turn H^T H - 1 has rank one, and the decomposition
    # the host inherits from the reference takes the roots of minors that are zero up to rounding, of either sign
    "plane_identity": dict(R=np.eye(3), t=(0.4, 0.0, 0.0), plane=((0.0, 0.0, 1.0), 3.0), **_NOISY),
}
BEARING_CASES = tuple(nm for nm in GRID if not nm.startswith("plane_"))
PLANE_CASES = tuple(nm for nm in GRID if nm.startswith("plane_"))
NOISE_FREE = tuple(nm for nm in GRID if GRID[nm].get("noise_px", 0.0) == 0.0)
# the two sizes the ragged batch adds: more than one pass of the 256 threads, and the smallest problem of the five-point
EXTRA = {"n257": ("rot20", 257), "n5": ("identity_general", 5)}
EXTRA_PLANE = {"n257": ("plane_oblique", 257), "n5": ("plane_identity", 5)}
RAGGED_BATCH = BEARING_CASES + ("n257", "n5")
RAGGED_BATCH_PLANE = PLANE_CASES + ("n257", "n5")

# Per case and estimator its scene seed: the first of 1 .. 10 at which the restatement alone meets the premises of an exact
# comparison (fivepoint_cases.premises, twopoint_cases.premises_hold, the three gaps of tests/test_init_cpu.py);
# tests/test_motion_grid_cpu.py asserts that they hold.  Seed 1 where not named: the translation and the homography
# estimators meet theirs at seed 1 everywhere; the essential-matrix estimator's short_baseline at seed 1 has an elimination
# whose smallest singular value (1.3e-9) lies between the degeneracy bound and ten times it.  A case whose restatement meets
# them with none of the ten is a property-only case (seed 1), named here with its reason.
SEEDS_E = {"short_baseline": 2}
SEEDS_T = {}
SEEDS_H = {}
PROPERTY_ONLY_E = {
    "identity_x": "at every seed 1 .. 10 the restatement's own SVD basis calls 11 - 27 of the 512 all-inlier samples degenerate "
                  "and its turned basis none: the two runs do not agree on n_degenerate, so nothing can be asked to equal it"}
PROPERTY_ONLY_T = {}
MODEL_NOT_UNIQUE = ("n5", )                                            # as fivepoint_cases.MODEL_NOT_UNIQUE


def spec_of(name, plane=False):
    """(grid name, n) of a case name."""
    extra = EXTRA_PLANE if plane else EXTRA
    return extra[name] if name in extra else (name, N)


@functools.lru_cache(maxsize=None)
def scene(name, seed, plane=False):
    grid, n = spec_of(name, plane)
    return make_scene(seed, n, **GRID[grid])


def case_e(name):
    return scene(name, SEEDS_E.get(name, 1))


def case_t(name):
    return scene(name, SEEDS_T.get(name, 1))


def case_h(name):
    return scene(name, SEEDS_H.get(name, 1), True)


@functools.lru_cache(maxsize=None)
def restated_e(name, turned=False, seed=None):
    c = scene(name, SEEDS_E.get(name, 1) if seed is None else seed)
    return np5.estimate_essential_ransac(c["f_cur"], c["f_ref"], c["thresh"], c["seed"], K, basis_turn=fc.TURN if turned else None)


@functools.lru_cache(maxsize=None)
def restated_t(name, seed=None):
    c = scene(name, SEEDS_T.get(name, 1) if seed is None else seed)
    return npt.estimate_translation_ransac(c["f_cur"], c["f_ref"], c["R"], c["thresh"], c["seed"], K)


@functools.lru_cache(maxsize=None)
def restated_h(name, seed=None):
    c = scene(name, SEEDS_H.get(name, 1) if seed is None else seed, True)
    return npi.estimate_homography_ransac(c["uv_ref"], c["uv_cur"], c["thresh_h"], c["seed"], K)


def premises_e(name, seed=None):
    c = scene(name, SEEDS_E.get(name, 1) if seed is None else seed)
    a, b = restated_e(name, False, seed), restated_e(name, True, seed)
    return fc.premises(a, b, c["f_cur"], c["f_ref"], c["thresh"], model_unique=name not in MODEL_NOT_UNIQUE)


def premises_t(name, seed=None):
    return tc.premises_hold(restated_t(name, seed))


def premises_h(name, seed=None):
    r = restated_h(name, seed)
    return r["status"] == npi.STATUS_OK and min(r["gap_hyp"], r["gap_final"], r["gap_lambda"]) >= 1e-9
