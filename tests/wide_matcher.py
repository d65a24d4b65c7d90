"""Cases and NumPy references shared by tests/test_wide_matcher_cpu.py and tests/test_wide_matcher_gpu.py: the blocking
matcher entries (seed update, direct matcher with both warps, stereo seam) on EQUIDISTANT and ATAN cameras.  The
reference throughout is the NumPy reading (np_restatement_direct) given a CamWide: the C oracle has no wide camera.
Every reference is computed once per process and handed out unchanged (callers copy what they change).

Pairs (`name`): "equidistant" / "atan" = both frames on that camera; "mixed" = a radtan reference frame and an
equidistant current frame of the same size (the same scene seed gives the same poses, plane and texture, so the two
renderings show the same world); "radtan" = both frames narrow, for what a twin must not change."""
import functools

import numpy as np

from svo_pro_universal_amd import _capi as capi, synth
import np_restatement as n0
import np_restatement_cameras as npc
import np_restatement_direct as nd
import wide_geometry as wg

CAMERAS = ("equidistant", "atan")
N_UNITS, N_SEAM = 400, 120
# (matcher options, depth filter options) of the seed update, as tests/test_klt_matcher_gpu.py::test_update_seeds_parity
SEED_OPTION_SETS = (
    (dict(), dict()),
    (dict(affine_est_gain=1, max_epi_search_steps=500), dict(check_convergence=1)),
    (dict(subpix_refinement=0, affine_est_offset=0), dict(use_vogiatzis_update=0, check_visibility=0)),
)
PAIRS = {"equidistant": ("equidistant", "equidistant"), "atan": ("atan", "atan"), "mixed": ("radtan", "equidistant"),
         "radtan": ("radtan", "radtan")}
EPS8 = 8.0 * 2.0 ** -52      # the rounding perturbation of tests/test_wide_matcher_cpu.py (test 3)


def camera(kind):
    return wg.camera(kind)          # equidistant: synth.Camera.visensor_like(); all 752 x 480


@functools.lru_cache(maxsize=None)
def _scene(kind, seed, trans_m):
    sc = synth.make_align_scene(seed, n_features=10, cam=camera(kind), rot_deg=(0.5, 1.5), trans_m=trans_m)
    return sc, n0.create_img_pyramid(sc.img_ref, 5), n0.create_img_pyramid(sc.img_cur, 5)


@functools.lru_cache(maxsize=None)
def pair(name, seam=False):
    """(scene of the reference camera, reference pyramid, current pyramid, reference camera, current camera).  seam: the
    stereo seam's scene (baselines as tests/test_klt_matcher_gpu.py::test_epipolar_match_batch_parity_stereo_seam)."""
    kr, kc = PAIRS[name]
    seed, trans = (66, (0.05, 0.15)) if seam else (63, (0.08, 0.2))
    sc, ref, _ = _scene(kr, seed, trans)
    _, _, cur = _scene(kc, seed, trans)
    return sc, ref, cur, camera(kr), camera(kc)


@functools.lru_cache(maxsize=None)
def seed_set(name):
    """400 seeds of the reference frame, a few types overwritten as test_update_seeds_parity does.  Read-only."""
    sd = synth.make_seed_set(pair(name)[0], N_UNITS, margin=3, levels=(0, 1, 2, 3))
    sd["type"][::17] = capi.FT_MAPPOINT_SEED
    sd["type"][5::41] = capi.FT_CORNER        # not a seed: skipped
    sd["type"][7::53] = capi.FT_OUTLIER
    sd["type"][9::59] = capi.FT_EDGELET_SEED_CONVERGED
    for v in sd.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return sd


# ---- cameras of the NumPy reading --------------------------------------------------------------------------------------
def cam_wide(c):
    return npc.CamWide.of(c)


def cam_misread_as_radtan(c):
    """The same numbers read as k1 k2 p1 p2 (equidistant only: four parameters)."""
    return nd.Cam(c.width, c.height, c.fx, c.fy, c.cx, c.cy, c.dist if c.model != "none" else None)


class _CamScaled(npc.CamWide):
    scale = 1.0

    def distort(self, x, y):
        a, b = npc.CamWide.distort(self, x, y)
        return a * self.scale, b * self.scale

    def undistort(self, x, y):
        a, b = npc.CamWide.undistort(self, x, y)
        return a * self.scale, b * self.scale


def _scaled(c, s):
    w = npc.CamWide.of(c)
    w.__class__ = _CamScaled
    w.scale = s
    return w


def cam_rounded_up(c):
    return _scaled(c, 1.0 + EPS8)


def cam_rounded_down(c):
    return _scaled(c, 1.0 - EPS8)


def np_views(name, mu_range, cam_of=cam_wide, seam=False):
    sc, ref, cur, cam_r, cam_c = pair(name, seam)
    return (nd.FrameView(ref, cam_of(cam_r), nd.Tf.from7(sc.T_ref_f_w.as7()), 1, mu_range),
            nd.FrameView(cur, cam_of(cam_c), nd.Tf.from7(sc.T_cur_f_w_gt.as7()), 2, 0.0))


def nd_options(mopt):
    return nd.MatcherOptions(align_max_iter=mopt.align_max_iter, max_epi_search_steps=mopt.max_epi_search_steps,
                             subpix_refinement=bool(mopt.subpix_refinement),
                             epi_search_edgelet_filtering=bool(mopt.epi_search_edgelet_filtering),
                             scan_on_unit_sphere=bool(mopt.scan_on_unit_sphere),
                             epi_search_edgelet_max_angle=mopt.epi_search_edgelet_max_angle,
                             affine_est_offset=bool(mopt.affine_est_offset), affine_est_gain=bool(mopt.affine_est_gain),
                             max_patch_diff_ratio=mopt.max_patch_diff_ratio)


# ---- seed update -------------------------------------------------------------------------------------------------------
def seed_options(name, sphere, option_set):
    mkw, dkw = SEED_OPTION_SETS[option_set]
    return (capi.default_matcher_options(scan_on_unit_sphere=sphere, **mkw),
            capi.default_depth_filter_options(pair(name)[4], **dkw))        # px_error_angle of the current camera


@functools.lru_cache(maxsize=None)
def seeds_reference(name, sphere=0, option_set=0, cam_of=cam_wide, rounds=2):
    """The NumPy reading's rounds, state and types fed back: a list of nd.update_seeds dicts."""
    sd = seed_set(name)
    mopt, dopt = seed_options(name, sphere, option_set)
    nrv, ncv = np_views(name, sd["mu_range"], cam_of)
    state, types, out = sd["state"].copy(), sd["type"].copy(), []
    for _ in range(rounds):
        g = nd.update_seeds(ncv, [nrv], sd["ref_frame_idx"], sd["px"], sd["f"], sd["grad"], sd["level"], types, state, nd_options(mopt),
                            dopt.seed_convergence_sigma2_thresh, dopt.mappoint_convergence_sigma2_thresh, dopt.px_error_angle,
                            bool(dopt.check_visibility), bool(dopt.check_convergence), bool(dopt.use_vogiatzis_update))
        out.append(g)
        state, types = g["state"], g["type"]
    return out


def median_depth_error(name, g):
    """Median relative depth error of the successful seeds of a round against the scene's true depth."""
    sd = seed_set(name)
    ok = g["success"] == 1
    return float(np.median(np.abs(1.0 / g["state"].reshape(-1, 4)[ok, 0] - sd["true_depth"][ok]) / sd["true_depth"][ok]))


# ---- direct matcher ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def direct_inputs(name):
    sc, _, _, cam_r, cam_c = pair(name)
    sd = seed_set(name)
    x = sd["f"].reshape(-1, 3).T * sd["true_depth"]
    xw = sc.T_w_ref.transform(x)
    px_true = cam_c.project(sc.T_w_cur.inverse().transform(xw))
    px_init = np.ascontiguousarray((px_true + np.random.RandomState(1).uniform(-2.0, 2.0, px_true.shape)).T).ravel()
    px_init[:10] += 40.0                                            # hopeless starts: alignment failures / too far
    lm = np.ascontiguousarray(xw.T)
    lm[::97] += 50.0                                                # landmarks far off their pixel (pixelwise warp)
    ftype = np.where(seed_set(name)["type"] == 0, capi.FT_EDGELET, capi.FT_CORNER).astype(np.uint8)
    return dict(px_init=px_init, landmark_xyz=lm, type=ftype, px_true=px_true)


@functools.lru_cache(maxsize=None)
def direct_reference(name, pixelwise=False, gain=0, cam_of=cam_wide):
    sd, di = seed_set(name), direct_inputs(name)
    nrv, ncv = np_views(name, sd["mu_range"], cam_of)
    mopt = capi.default_matcher_options(affine_est_gain=gain)
    return nd.match_direct_batch(ncv, [nrv], sd["ref_frame_idx"], sd["px"], sd["f"], sd["grad"], sd["level"], di["type"],
                                 sd["true_depth"], di["px_init"], nd_options(mopt), landmark_xyz=di["landmark_xyz"] if pixelwise else None)


# ---- stereo seam -------------------------------------------------------------------------------------------------------
def seam_options():
    return capi.default_matcher_options(max_epi_search_steps=500, subpix_refinement=1, scan_on_unit_sphere=1)


@functools.lru_cache(maxsize=None)
def seam_inputs(name):
    sc = pair(name, True)[0]
    sd = synth.make_seed_set(sc, N_SEAM, margin=6, levels=(0, 1, 2))
    ftype = np.where(sd["type"] == 0, capi.FT_EDGELET, capi.FT_CORNER).astype(np.uint8)   # detector output, not seeds
    d_mean = float(np.median(sd["true_depth"]))
    d_inv_common = (1.0 / d_mean, 1.0 / (0.3 * d_mean), 1.0 / (15.0 * d_mean))          # mean / min / max
    d_each = d_mean * np.random.RandomState(5).uniform(0.8, 1.25, N_SEAM)
    d_inv = np.ascontiguousarray(np.stack([1.0 / d_each, 1.0 / (0.3 * d_each), 1.0 / (15.0 * d_each)], 1)).ravel()
    T_f1f0 = (sc.T_cur_f_w_gt * sc.T_ref_f_w.inverse()).as7()
    return dict(sd=sd, type=ftype, d_inv_common=d_inv_common, d_inv=d_inv, T_f1f0=T_f1f0)


@functools.lru_cache(maxsize=None)
def seam_reference(name, per_feature=False, cam_of=cam_wide):
    """dict(result, depth, px_cur): with the common range through nd.stereo_triangulate (every feature visited), with
    per-feature ranges through one nd.Matcher's find_epipolar_match_direct, as that loop calls it."""
    si = seam_inputs(name)
    sd, n = si["sd"], N_SEAM
    f0, f1 = np_views(name, 0.0, cam_of, seam=True)
    T = nd.Tf.from7(si["T_f1f0"])
    px, f, grad = sd["px"].reshape(-1, 2), sd["f"].reshape(-1, 3), sd["grad"].reshape(-1, 2)
    out = dict(result=np.zeros(n, np.int32), depth=np.zeros(n), px_cur=np.zeros((n, 2)))
    if not per_feature:
        matches, results, _ = nd.stereo_triangulate(f0, f1, T, px, f, grad, sd["level"], si["type"], np.arange(n), n + 1, *si["d_inv_common"])
        out["result"][:] = results
        for m in matches:
            out["depth"][m["i_ref"]] = m["depth"]
            out["px_cur"][m["i_ref"]] = m["px"]
        return out
    matcher = nd.Matcher(nd.MatcherOptions(max_epi_search_steps=500, subpix_refinement=True))
    for i in range(n):
        matcher.options.align_1d = nd.is_edgelet(int(si["type"][i]))
        d = si["d_inv"][3 * i:3 * i + 3]
        res, depth = matcher.find_epipolar_match_direct(f0, f1, T, px[i], f[i], grad[i], int(sd["level"][i]), int(si["type"][i]),
                                                        float(d[0]), float(d[1]), float(d[2]))
        out["result"][i] = res
        if res == nd.SUCCESS:
            out["depth"][i], out["px_cur"][i] = depth, matcher.px_cur
    return out
