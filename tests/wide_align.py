"""NumPy reading of sparse image alignment for ANY of the four pinhole camera models (none, radtan, equidistant, atan):
the checker of svoh_sparse_align_wide_batch / _wide_evaluate, and the scenes, option sets and references that
tests/test_wide_align_cpu.py and tests/test_wide_align_gpu.py share.  The C oracle has no wide camera; for radtan this
reading is tied to it in tests/test_wide_align_cpu.py.

Written from the reference's files, like the other restatements:
  precomputeBaseCaches            src/svo_img_align/src/sparse_img_align.cpp:262-317
      every projection here is of type kPinhole whatever its distortion, so without use_distortion_jacobian the rows
      are Frame::jacobian_xyz2uv_imu (frame.h:342-357) times the error multiplier |fx|; with it they are minus
      Frame::jacobian_xyz2image_imu (frame.cpp:274-290), the model's own project3 Jacobian (which the atan model lacks)
  precomputeJacobiansAndRefPatches  :319-403
  computeResidualsOfFrame           :405-498    z < 0 is invisible (kPinhole); project3 of the model
  computeHessianAndGradient         :500-541
  SparseImgAlign::run / evaluateError :34-156   the cameras of a bundle add into one H, g
The projection and its Jacobian are np_restatement_cameras.CamWide's (scalar libm maths); selection, bilinear lookup and
pyramids are np_restatement's; update and solve are np_restatement_gn's, with its Gauss-Newton loop restated around
`evaluate` below (np_restatement_gn.run is bound to np_restatement.evaluate).

Every evaluation also reports how close its inputs came to a decision that libm and the device's maths could take
differently (`Probe`): tests/test_wide_align_cpu.py asserts the distances, so that the GPU tests may demand exact
discrete results."""
import functools

import numpy as np

from svo_pro_universal_amd import _capi as capi, synth

import np_restatement as n0
import np_restatement_cameras as npc
import np_restatement_gn as ngn
import odd_sizes
import wide_geometry as wg
from np_restatement_direct import Tf


class Probe(object):
    """Smallest distances met so far: of a projected patch corner (pixels of the level) to a bound of the visibility
    test, or of a camera-frame depth to zero (`bound`); of max|dx| to eps, relative (`eps`)."""

    def __init__(self):
        self.bound = np.inf
        self.eps = np.inf
        self.vis_level0 = []      # (visible, invisible) features of the bundle, of every evaluation at level 0


def _tf(T):
    return T if isinstance(T, Tf) else Tf.from7(np.asarray(T.as7(), np.float64))


def jacobian_rows(cam, T_cam_imu, T_imu_cam, xyz_ref, dist_jac):
    """frame_jac of precomputeBaseCaches for one feature: 2 x 6."""
    p_imu = T_imu_cam.apply(xyz_ref)
    G = np.zeros((3, 6))
    G[:, :3] = np.eye(3)
    x, y, z = p_imu
    G[:, 3:] = -np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
    p_cam = T_cam_imu.apply(p_imu)
    R_ci = n0.quat_to_R(T_cam_imu.q)
    if not dist_jac:
        J_proj = np.array([[1.0, 0.0, -p_cam[0] / p_cam[2]], [0.0, 1.0, -p_cam[1] / p_cam[2]]])
        return (-1.0 / p_cam[2]) * (J_proj @ R_ci @ G) * abs(cam.fx)
    return -(cam.project3_jacobian(p_cam) @ R_ci @ G)


def evaluate(scene, ref_levels, cur_levels, level, P, T, max_level=4, alpha=0.0, beta=0.0, est_alpha=False, est_beta=False,
             robust=False, weight_scale=10.0, dist_jac=False, probe=None):
    """evaluateError's share of one camera at state (T = T_icur_iref as Tf, alpha, beta): H 8x8, g 8, sum of the weighted
    squared residuals, n_meas, visibility of the selected features, number of selected features."""
    cam = npc.CamWide.of(scene.cam)
    T_ci, T_ic = _tf(scene.T_cam_imu), _tf(scene.T_imu_cam)
    px = scene.px.reshape(-1, 2).T
    idx = n0.select_features(px, scene.flags, ref_levels[max_level], max_level, P)
    n = idx.size
    px = px[:, idx]
    f = scene.f.reshape(-1, 3)[idx]
    pw = scene.pos_world.reshape(-1, 3)[idx]
    depth = np.sqrt(((pw - np.asarray(scene.ref_pos)[None]) ** 2).sum(1))
    xyz_ref = f * depth[:, None]
    scale = 1.0 / (1 << level)
    ref_img, cur_img = ref_levels[level], cur_levels[level]
    h, w = cur_img.shape
    T_cur_ref = T_ci * T * T_ic
    c = (P - 1) / 2.0
    vis = np.zeros(n, bool)
    utl, vtl = np.zeros(n), np.zeros(n)
    Jrows = np.zeros((n, 2, 6))
    for i in range(n):
        xyz_cur = T_cur_ref.apply(xyz_ref[i])
        if probe is not None:
            probe.bound = min(probe.bound, abs(xyz_cur[2]))
        if xyz_cur[2] < 0.0:
            continue
        uv = cam.project3(xyz_cur)
        u, v = uv[0] * scale - c, uv[1] * scale - c
        if probe is not None and np.isfinite(u) and np.isfinite(v):
            probe.bound = min(probe.bound, abs(u), abs(v), abs(u + P + 2.0 - w), abs(v + P + 2.0 - h))
        if u < 0.0 or v < 0.0 or u + P + 2.0 >= w or v + P + 2.0 >= h or not (np.isfinite(u) and np.isfinite(v)):
            continue
        vis[i], utl[i], vtl[i] = True, u, v
        Jrows[i] = jacobian_rows(cam, T_ci, T_ic, xyz_ref[i], dist_jac)
    H, g = np.zeros((8, 8)), np.zeros(8)
    if not vis.any():
        return H, g, 0.0, 0, vis.astype(np.uint8), n
    k = np.nonzero(vis)[0]
    # reference patches with border, central differences (:319-403)
    c_wb = (P + 2 - 1) / 2.0
    gx, gy = np.meshgrid(np.arange(P + 2), np.arange(P + 2))
    patch = n0.bilinear(ref_img, (px[0, k] * scale - c_wb)[:, None, None] + gx[None], (px[1, k] * scale - c_wb)[:, None, None] + gy[None])
    ref_val = patch[:, 1:-1, 1:-1]
    dx = 0.5 * (patch[:, 1:-1, 2:] - patch[:, 1:-1, :-2])
    dy = 0.5 * (patch[:, 2:, 1:-1] - patch[:, :-2, 1:-1])
    J = np.zeros((k.size, P, P, 8))
    J[..., :6] = (dx[..., None] * Jrows[k][:, None, None, 0, :] + dy[..., None] * Jrows[k][:, None, None, 1, :]) * scale
    if est_alpha:
        J[..., 6] = -ref_val
    if est_beta:
        J[..., 7] = -1.0
    gx, gy = np.meshgrid(np.arange(P), np.arange(P))
    Icur = n0.bilinear(cur_img, utl[k][:, None, None] + gx[None], vtl[k][:, None, None] + gy[None])
    res = Icur * (1.0 + float(np.float32(alpha))) + float(np.float32(beta)) - ref_val      # alpha, beta travel as float (:411-412)
    wgt = np.ones_like(res)
    if robust:   # TukeyWeightFunction::weight on float (robust_cost.cpp:48-60)
        e = (res / np.float32(weight_scale)).astype(np.float32)
        b2 = np.float32(4.6851) * np.float32(4.6851)
        x2 = e * e
        t = np.float32(1.0) - x2 / b2
        wgt = np.where(x2 <= b2, t * t, np.float32(0)).astype(np.float64)
    Jm, rm, wm = J.reshape(-1, 8), res.ravel(), wgt.ravel()
    H = (Jm * wm[:, None]).T @ Jm
    g = -(Jm * (rm * wm)[:, None]).sum(0)
    return H, g, float((rm * rm * wm).sum()), int(rm.size), vis.astype(np.uint8), n


def evaluate_bundle(cams, level, P, T, probe=None, **kw):
    """The cameras of a bundle: one H, one g (:138-154).  Returns H, g, chi2 (per measurement), n_meas, visibility of
    the selected features (camera after camera), n_selected."""
    H, g, chi2, nm, vis, nsel = np.zeros((8, 8)), np.zeros(8), 0.0, 0, [], 0
    for scene, ref_levels, cur_levels in cams:
        Hc, gc, c2, n, v, ns = evaluate(scene, ref_levels, cur_levels, level, P, T, probe=probe, **kw)
        H += Hc; g += gc; chi2 += c2; nm += n; nsel += ns
        vis.append(v)
    vis = np.concatenate(vis)
    if probe is not None and level == 0:
        probe.vis_level0.append((int(vis.sum()), int(nsel - vis.sum())))
    return H, g, chi2 / max(1, nm), nm, vis, nsel


def run(cams, opt, T_init, alpha_init=0.0, beta_init=0.0, prior=None, probe=None):
    """SparseImgAlign::run with the options of a svoh_align_options: np_restatement_gn.run's loop around evaluate_bundle.
    Returns dict(T, alpha, beta, iters, n_meas per level, status, n_fts_to_track, n_patch_iters)."""
    P = opt.patch_size
    kw = dict(max_level=opt.max_level, est_alpha=bool(opt.estimate_illumination_gain), est_beta=bool(opt.estimate_illumination_offset),
              robust=bool(opt.robustification), weight_scale=opt.weight_scale, dist_jac=bool(opt.use_distortion_jacobian))
    state = (_tf(T_init), float(alpha_init), float(beta_init))
    iters, n_meas = [0] * capi.SVOH_MAX_LEVELS, [0] * capi.SVOH_MAX_LEVELS
    n_sel = sum(n0.select_features(sc.px.reshape(-1, 2).T, sc.flags, ref[opt.max_level], opt.max_level, P).size for sc, ref, _ in cams)
    out = dict(n_fts_to_track=n_sel, n_patch_iters=0)
    if n_sel == 0:   # SparseImgAlign::run returns before the first level (:60-64)
        out.update(T=state[0], alpha=state[1], beta=state[2], iters=iters, n_meas=n_meas, status=1)
        return out
    stop, status, I_prior = False, 0, np.zeros(8)
    for level in range(opt.max_level, opt.min_level - 1, -1):
        old_state = state
        for it in range(opt.max_iter):
            H, g, _c2, nm, _vis, _ = evaluate_bundle(cams, level, P, state[0], probe=probe, alpha=state[1], beta=state[2], **kw)
            iters[level] += 1
            n_meas[level] = nm
            out["n_patch_iters"] += nm // (P * P)
            if prior is not None:                    # applyPrior (sparse_img_align_base.cpp:77-107)
                if it == 0:
                    I_prior = np.zeros(8)
                    I_prior[0:3] = prior["lambda_trans"] * max(abs(H[j, j]) for j in range(3))
                    I_prior[3:6] = prior["lambda_rot"] * max(abs(H[j, j]) for j in range(3, 6))
                    I_prior[6] = prior["lambda_alpha"] * H[6, 6]
                    I_prior[7] = prior["lambda_beta"] * H[7, 7]
                H = H + np.diag(I_prior)
                g = g.copy()
                g[:6] += I_prior[:6] * ngn.tf_log(prior["T"].inverse() * state[0])
                g[6] += I_prior[6] * (prior["alpha"] - state[1])
                g[7] += I_prior[7] * (prior["beta"] - state[2])
            dx = ngn.solve_ldlt_semantics(H, g)
            if np.isnan(dx[0]):
                stop = True
            if stop:
                state, status = old_state, 2
                break
            old_state, state = state, ngn.update(state, dx)
            x_norm = float(np.max(np.abs(dx)))
            if probe is not None:
                probe.eps = min(probe.eps, abs(x_norm - opt.eps) / opt.eps)
            if x_norm < opt.eps:
                break
    out.update(T=state[0], alpha=state[1], beta=state[2], iters=iters, n_meas=n_meas, status=status)
    return out


# ---- what the CPU and the GPU tests share ---------------------------------------------------------------------------
KINDS = ("equidistant", "atan")
EVAL_SEED = {"equidistant": 313, "atan": 317}
RUN_SEED = {"equidistant": 324, "atan": 317}
EVAL_LEVELS = (4, 2, 0)
N_LEVELS = 5
# A motion large enough that selected features leave the image at level 0: the selection (at level 4) keeps every feature 40 pixels
# (P = 8: 72) inside, and the scenes' default motion, up to 2 degrees and 5 cm, moves a point by 30 pixels at the most.  A run therefore
# starts near the truth (start_state) and not at the identity.  The seeds below are those of 300 .. 344 whose scenes, at the true
# motion, lose at least five and at most 40 % of their selected features at level 0 with 4x4 and with 8x8 patches.
MOTION = dict(rot_deg=(3.0, 5.0), trans_m=(0.8, 1.2))


def option_sets(kind, P):
    """illumination off / on x robust off / on x distortion Jacobian off / on (atan: off -- it has none)."""
    out = []
    for illum in (0, 1):
        for robust in (0, 1):
            for dj in ((0,) if kind == "atan" else (0, 1)):
                out.append(capi.default_align_options(patch_size=P, max_level=4, min_level=0, estimate_illumination_gain=illum,
                                                      estimate_illumination_offset=illum, robustification=robust, use_distortion_jacobian=dj))
    return out


def opt_key(opt):
    return (opt.patch_size, opt.max_level, opt.min_level, opt.estimate_illumination_gain, opt.estimate_illumination_offset, opt.robustification,
            opt.use_distortion_jacobian, opt.max_iter)


def opt_from_key(k):
    return capi.default_align_options(patch_size=k[0], max_level=k[1], min_level=k[2], estimate_illumination_gain=k[3],
                                      estimate_illumination_offset=k[4], robustification=k[5], use_distortion_jacobian=k[6], max_iter=k[7])


@functools.lru_cache(maxsize=None)
def scene(kind, seed, n, P, border):
    """(scene, reference pyramid, current pyramid) on wide_geometry's 752 x 480 camera of that kind."""
    sc = synth.make_align_scene(seed, n_features=n, patch_size=P, cam=wg.camera(kind), border_features=border, **MOTION)
    return sc, n0.create_img_pyramid(sc.img_ref, N_LEVELS), n0.create_img_pyramid(sc.img_cur, N_LEVELS)


def eval_scene(kind, P):
    return scene(kind, EVAL_SEED[kind], 600, P, 60)      # 660 features: a second patch for 148 lanes of the workgroup's 512


def run_scene(kind, P):
    return scene(kind, RUN_SEED[kind], 150, P, 30)


def start_state(sc):
    """Where a run starts (see MOTION)."""
    return eval_state(sc)[0]


def eval_state(sc):
    """Where the evaluations are taken: near the truth but not at it, with illumination terms that are not zero."""
    T = synth.SE3(synth.quat_from_axis_angle([0.2, -1.0, 0.4], 0.003), [0.004, -0.002, 0.003]) * sc.T_icur_iref_gt
    return T, 0.02, -1.5


@functools.lru_cache(maxsize=None)
def eval_reference(kind, key, level):
    opt = opt_from_key(key)
    cam = eval_scene(kind, opt.patch_size)
    T, a, b = eval_state(cam[0])
    probe = Probe()
    r = evaluate_bundle([cam], level, opt.patch_size, _tf(T), probe=probe, max_level=opt.max_level, alpha=a, beta=b,
                        est_alpha=bool(opt.estimate_illumination_gain), est_beta=bool(opt.estimate_illumination_offset),
                        robust=bool(opt.robustification), weight_scale=opt.weight_scale, dist_jac=bool(opt.use_distortion_jacobian))
    return r, probe


def weighted_prior(sc):
    """A prior that acts: (ctypes struct for the entry, dict for the reading)."""
    Tp = synth.SE3(synth.quat_from_axis_angle([0.3, -1, 0.2], 0.004), [0.003, -0.002, 0.001]) * sc.T_icur_iref_gt
    p = capi.svoh_align_prior()
    p.have_prior = 1
    for i in range(4):
        p.T_prior.q[i] = float(Tp.q[i])
    for i in range(3):
        p.T_prior.t[i] = float(Tp.t[i])
    p.alpha_prior, p.beta_prior = 0.01, -0.5
    p.lambda_rot, p.lambda_trans, p.lambda_alpha, p.lambda_beta = 0.5, 0.7, 0.2, 0.3
    d = dict(T=_tf(Tp), alpha=0.01, beta=-0.5, lambda_rot=0.5, lambda_trans=0.7, lambda_alpha=0.2, lambda_beta=0.3)
    return p, d


@functools.lru_cache(maxsize=None)
def run_reference(kind, key, with_prior=False):
    opt = opt_from_key(key)
    cam = run_scene(kind, opt.patch_size)
    probe = Probe()
    prior = weighted_prior(cam[0])[1] if with_prior else None
    return run([cam], opt, start_state(cam[0]), prior=prior, probe=probe), probe


# ---- the ragged launch of seven problems (tests/test_wide_align_gpu.py, item 3) --------------------------------------
RAGGED_OPT = dict(patch_size=4, max_level=4, min_level=0)


@functools.lru_cache(maxsize=None)
def ragged_problems():
    """name -> dict(cams=[(scene, ref, cur), ...], prior=None | (struct, dict)).  The rig's second camera has extrinsics of
    its own (another seed) and looks at a scene of its own, moved by the FIRST camera's body motion."""
    out = {}
    out["equidistant"] = dict(cams=[scene("equidistant", 317, 150, 4, 30)])
    out["atan"] = dict(cams=[scene("atan", 324, 150, 4, 30)])
    out["radtan"] = dict(cams=[scene("radtan", 313, 150, 4, 30)])
    a = scene("radtan", 317, 150, 4, 30)
    b = rig_partner(a[0], "equidistant", 325, 90)
    out["rig"] = dict(cams=[a, b])
    # One patch leaves four directions of the pose free: H is singular, and what Eigen's LDLT makes of a singular matrix is not
    # something a reading with another solver can follow step for step.  Under a weighted prior the system is definite.
    of = scene("equidistant", 326, 1, 4, 0)
    out["one_feature"] = dict(cams=[of], prior=weighted_prior(of[0]))
    sc, ref, cur = scene("equidistant", 327, 40, 4, 0)
    none = synth.AlignScene()
    none.__dict__.update(sc.__dict__)
    none.flags = np.zeros_like(sc.flags)
    out["no_flagged"] = dict(cams=[(none, ref, cur)])
    pc = scene("atan", 317, 150, 4, 30)
    out["prior"] = dict(cams=[pc], prior=weighted_prior(pc[0]))
    return out


RAGGED_ORDER = ("equidistant", "atan", "radtan", "rig", "one_feature", "no_flagged", "prior")


def rig_partner(first, kind, seed, n):
    """A second camera of first's rig: its own intrinsics (kind), its own extrinsics, its own plane and texture, and a
    current image rendered where the BODY motion of `first` puts it."""
    sc = synth.make_align_scene(seed, n_features=n, patch_size=4, cam=wg.camera(kind), border_features=10, render_images=False, **MOTION)
    T_body = first.T_icur_iref_gt                       # T_icur_iref of the bundle
    T_w_ref = sc.T_w_ref                                # this camera's reference pose (world <- camera)
    T_imu_world_ref = sc.T_imu_cam * T_w_ref.inverse()
    T_imu_world_cur = T_body * T_imu_world_ref
    T_w_cur = (sc.T_cam_imu * T_imu_world_cur).inverse()
    sc.img_ref = synth.render(sc.cam, T_w_ref, sc.plane, sc.tex)
    sc.img_cur = synth.render(sc.cam, T_w_cur, sc.plane, sc.tex)
    sc.T_icur_iref_gt = T_body
    return sc, n0.create_img_pyramid(sc.img_ref, N_LEVELS), n0.create_img_pyramid(sc.img_cur, N_LEVELS)


@functools.lru_cache(maxsize=None)
def ragged_reference(name):
    pb = ragged_problems()[name]
    probe = Probe()
    opt = capi.default_align_options(**RAGGED_OPT)
    prior = pb["prior"][1] if pb.get("prior") else None
    return run(pb["cams"], opt, start_state(pb["cams"][0][0]), prior=prior, probe=probe), probe


# ---- the odd size (item 6) ------------------------------------------------------------------------------------------
ODD_SIZE = (413, 309)
assert ODD_SIZE in odd_sizes.SIZES.values()


@functools.lru_cache(maxsize=None)
def odd_scene():
    """The equidistant camera with its principal point and focal lengths scaled to 413 x 309."""
    c = wg.camera("equidistant")
    w, h = ODD_SIZE
    cam = synth.Camera(w, h, c.fx * w / c.width, c.fy * h / c.height, c.cx * w / c.width, c.cy * h / c.height, dist=c.dist, model="equidistant")
    sc = synth.make_align_scene(338, n_features=120, patch_size=4, cam=cam, border_features=25, max_level=3, **MOTION)
    return sc, n0.create_img_pyramid(sc.img_ref, 4), n0.create_img_pyramid(sc.img_cur, 4)


ODD_OPT = dict(patch_size=4, max_level=3, min_level=0)


@functools.lru_cache(maxsize=None)
def odd_reference():
    cam = odd_scene()
    probe = Probe()
    return run([cam], capi.default_align_options(**ODD_OPT), start_state(cam[0]), probe=probe), probe
