"""Scenes and NumPy references shared by tests/test_wide_geometry_cpu.py and tests/test_wide_geometry_gpu.py: the pose
optimiser and the candidate projection on EQUIDISTANT and ATAN cameras.  The reference throughout is the NumPy
restatement (np_restatement_pose.optimize_pose, np_restatement_direct.get_candidate) given a CamWide: the C oracle
has no wide camera.  Every reference is computed once per process and handed out unchanged."""
import functools
import os

import numpy as np
import yaml

from svo_pro_universal_amd import _capi as capi, synth
import np_restatement_cameras as npc
import np_restatement_direct as nd
import np_restatement_pose as npp
import pose_helpers as ph

UNIT, BEARING, IMAGE = capi.POSE_ERR_UNIT_PLANE, capi.POSE_ERR_BEARING_DIFF, capi.POSE_ERR_IMAGE_PLANE
CALIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "param", "calib")


@functools.lru_cache(maxsize=None)
def camera(kind):
    if kind == "equidistant":
        return synth.Camera.visensor_like()                       # 752 x 480
    if kind == "atan":
        c = yaml.safe_load(open(os.path.join(CALIB, "svo_test_pinhole.yaml")))["cameras"][0]["camera"]
        assert c["distortion"]["type"] == "fisheye"          # the loader's name of the ATAN model
        fx, fy, cx, cy = [float(v) for v in c["intrinsics"]["data"]]
        d = [float(v) for v in c["distortion"]["parameters"]["data"]]
        return synth.Camera(c["image_width"], c["image_height"], fx, fy, cx, cy, dist=d, model="atan")
    assert kind == "radtan"
    return synth.Camera.euroc_like(752, 480)


# ---- pose scenes -------------------------------------------------------------------------------------------------
# name -> (camera kinds per camera of the rig, seed, edgelet_fraction).  300 features a camera: several rounds per lane
# in the one-wave geometry and, with two cameras, more than one round of 256 lanes.
SEEDS = (71, 74)
POSE_SCENES = {}
for _s in SEEDS:
    POSE_SCENES["eq1_%d" % _s] = (("equidistant",), _s, 0.3)
    POSE_SCENES["eq2_%d" % _s] = (("equidistant", "equidistant"), _s + 10, 0.3)
POSE_SCENES["atan_edges"] = (("atan",), 81, 0.3)
POSE_SCENES["atan_corners"] = (("atan",), 82, 0.0)
POSE_SCENES["mixed"] = (("radtan", "equidistant"), 83, 0.3)
POSE_SCENES["radtan"] = (("radtan",), 84, 0.3)
for _i in range(9):
    POSE_SCENES["batch%d" % _i] = (("equidistant",), 90 + _i, 0.3)

# (scene, error type) pairs the GPU file compares with the restatement; the CPU file holds the premises for each
POSE_CASES = [(n, et) for n in POSE_SCENES if n.startswith("eq") for et in (UNIT, BEARING, IMAGE)]
POSE_CASES += [("atan_edges", UNIT), ("atan_corners", BEARING), ("mixed", IMAGE), ("mixed", BEARING), ("radtan", IMAGE)]


@functools.lru_cache(maxsize=None)
def pose_scene(name):
    kinds, seed, edgelets = POSE_SCENES[name]
    n = 300
    if name.startswith("batch"):
        n = 40 + 37 * int(name[5:])
    sc = ph.make_pose_scene(seed, n=n, cam=camera(kinds[0]), n_cams=len(kinds), edgelet_fraction=edgelets)
    for c, kind in zip(sc["cams"], kinds):
        if kind != kinds[0]:
            # the rig's other model: the same pixels, the bearing vectors of THAT camera (752 x 480 both)
            cam = camera(kind)
            px = c["px"].reshape(-1, 2)
            x, y = cam.undistorted_xy(px[:, 0], px[:, 1])
            f = np.stack([x, y, np.ones(len(x))], 1)
            c["f"] = np.ascontiguousarray(f / np.linalg.norm(f, axis=1, keepdims=True)).ravel()
            # and the points where that camera sees them at those pixels' noise-free places: re-project the old points
            old = npc.CamWide.of(c["cam"])
            T = nd.Tf.from7((c["T_cam_imu"] * sc["T_imu_world_gt"]).as7())
            new = npc.CamWide.of(cam)
            xyz = c["xyz_world"].reshape(-1, 3).copy()
            for i in range(len(xyz)):
                p = T.apply(xyz[i])
                u = old.project3(p)
                fb = np.asarray(new.back_project3(u), np.float64)
                xyz[i] = T.inverse().apply(fb / fb[2] * p[2])
            c["xyz_world"] = np.ascontiguousarray(xyz).ravel()
            c["cam"] = cam
    return sc


def pose_options(name, error_type, **kw):
    return capi.default_pose_options(pose_scene(name)["cams"][0]["cam"], error_type=error_type, **kw)


def np_cams(sc):
    return [dict(cam=npc.CamWide.of(c["cam"]), T_cam_imu=nd.Tf.from7(c["T_cam_imu"].as7()), px=c["px"], f=c["f"], grad=c["grad"],
                 level=c["level"], type=c["type"], xyz_world=c["xyz_world"], usable=c["usable"]) for c in sc["cams"]]


@functools.lru_cache(maxsize=None)
def pose_reference(name, error_type):
    """optimize_pose of the restatement, plus `final`: per camera the final unwhitened error of every feature (0 where
    not usable), as removeOutliers computes it."""
    sc = pose_scene(name)
    opt = pose_options(name, error_type)
    cams = np_cams(sc)
    g = npp.optimize_pose(error_type, cams, nd.Tf.from7(sc["T_imu_world_init"].as7()), opt.outlier_threshold, opt.max_iter, opt.eps)
    final = []
    for c in cams:
        e = np.zeros(len(c["level"]))
        for i in range(len(e)):
            if c["usable"][i]:
                ue = npp.residual(error_type, c["cam"], g["T"], c["T_cam_imu"], c["px"][2 * i:2 * i + 2], c["f"][3 * i:3 * i + 3],
                                  c["grad"][2 * i:2 * i + 2], c["xyz_world"][3 * i:3 * i + 3], npp.is_edgelet(int(c["type"][i])), 0.0, False)[0]
                e[i] = ue * (1.0 / (1 << int(c["level"][i])))
        final.append(e)
    g["final"] = final
    g["T7"] = np.concatenate([g["T"].q, g["T"].t])
    return g


def pose_error(sc, T7):
    return synth.se3_error(synth.SE3.from7(np.asarray(T7, np.float64)), sc["T_imu_world_gt"])


# ---- candidate sets ----------------------------------------------------------------------------------------------
N_CAND = 4000


@functools.lru_cache(maxsize=None)
def candidate_set(seed=17):
    """4 000 points of a local map of two keyframes: half are seeds (bearing vector, inverse depth, keyframe), half are
    landmarks scattered around and BEHIND the current view (the cone of Frame::isVisible is what rejects those)."""
    rng = np.random.RandomState(seed)
    T_w_cur = synth.SE3(synth.quat_from_axis_angle([0.2, 1, -0.1], 0.15), (0.4, -0.1, 0.2))
    T_w_kf = [T_w_cur * synth.SE3(synth.quat_from_axis_angle([0, 1, 0.3], 0.25), (0.3, 0.05, 0.1)),
              T_w_cur * synth.SE3(synth.quat_from_axis_angle([1, 0.2, 0], 0.2), (-0.2, 0.1, 0.05))]
    n = N_CAND
    kind = (rng.uniform(size=n) < 0.5).astype(np.uint8)
    kf = rng.randint(0, 2, n).astype(np.int32)
    v, mu = np.zeros((n, 3)), np.ones(n)
    for i in range(n):
        if kind[i]:
            f = np.array([rng.uniform(-0.9, 0.9), rng.uniform(-0.7, 0.7), 1.0]); v[i] = f / np.linalg.norm(f)
            mu[i] = 1.0 / rng.uniform(0.5, 8.0)
        else:
            v[i] = T_w_cur.transform(np.array([rng.uniform(-6, 6), rng.uniform(-4, 4), rng.uniform(-8.0, 8.0)]))
    return dict(T_f_w=T_w_cur.inverse(), T_w_kf=T_w_kf, kind=kind, kf=kf, v=v, mu=mu, n=n)


def candidate_reference_at(kind_of_cam, T_f_w7, cs):
    """get_candidate for every point, and what decided it.  Returns dict(ok n, px n x 2, near n: the point lies within
    1e-9 of an integer pixel boundary or within 1e-12 of the cone's cosine -- where libm and ocml may disagree --,
    cone_alone n: rejected by the cone although its projection passes the box and the margin, margin_alone n: passes
    the cone and the image box and fails the 8-pixel margin only)."""
    cam = npc.CamWide.of(camera(kind_of_cam))
    T = nd.Tf.from7(np.asarray(T_f_w7, np.float64))
    Tkf = [nd.Tf.from7(t.as7()) for t in cs["T_w_kf"]]
    f_tl = nd.normalized(cam.back_project3(np.zeros(2)))
    n = cs["n"]
    out = dict(ok=np.zeros(n, bool), px=np.zeros((n, 2)), near=np.zeros(n, bool), cone_alone=np.zeros(n, bool), margin_alone=np.zeros(n, bool))
    for i in range(n):
        seed = bool(cs["kind"][i])
        ok, px = nd.get_candidate(cam, T, Tkf[cs["kf"][i]].inverse(), None if seed else cs["v"][i], cs["v"][i], cs["mu"][i])
        out["ok"][i], out["px"][i] = ok, px
        xyz = Tkf[cs["kf"][i]].apply(cs["v"][i] * (1.0 / cs["mu"][i])) if seed else cs["v"][i]
        xf = T.apply(xyz)
        cos = nd.normalized(xf)[2]
        p = cam.project3(xf)
        in_box = bool(cam.is_keypoint_visible(p))
        in_margin = in_box and bool(cam.is_keypoint_visible_with_margin((int(p[0]), int(p[1])), nd.K_REPROJ_PATCH))
        out["near"][i] = abs(cos - f_tl[2]) < 1e-12 or (np.isfinite(p).all() and min(abs(p[0] - round(p[0])), abs(p[1] - round(p[1]))) < 1e-9)
        out["cone_alone"][i] = cos < f_tl[2] and in_margin
        out["margin_alone"][i] = (not cos < f_tl[2]) and in_box and not in_margin
    return out


@functools.lru_cache(maxsize=None)
def candidate_reference(kind_of_cam):
    cs = candidate_set()
    return candidate_reference_at(kind_of_cam, cs["T_f_w"].as7(), cs)
