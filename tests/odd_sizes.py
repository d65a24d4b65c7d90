"""Image sizes whose pyramid levels truncate, shared by tests/test_odd_sizes_cpu.py and tests/test_odd_sizes_gpu.py (no GPU
call, no oracle call at import).

The other parity tests run at 640x480, 752x480 and 320x240: every level is exactly w0/2^k x h0/2^k there.  Here a level is
floor(previous / 2) in at least one dimension at every step (frame_utils::createImgPyramid, frame.cpp:381-384), row lengths
are odd, and almost no level's byte count is a multiple of 16 -- the unit in which the alignment kernel copies a level's
images into LDS and places them there.

  A  413 x 309   levels 206x154, 103x77, 51x38, 25x19
  B  375 x 247   levels 187x123,  93x61, 46x30, 23x15   the smallest size that leaves a band of features inside the
                                                          level-4 margin of a 4x4 patch (synth.make_align_scene: 16 * 7 px)
  C  501 x 397   levels 250x198, 125x99, 62x49, 31x24   for 8x8 patches, whose margin (16 * 11 px) fits neither A nor B
"""
import math

import numpy as np

from svo_pro_universal_amd import synth

import helpers

N_LEVELS = 5
SIZES = {"A": (413, 309), "B": (375, 247), "C": (501, 397)}
PATCH = {"A": 4, "B": 4, "C": 8}


def level_sizes(w, h, n_levels=N_LEVELS):
    """[(w, h)] of every level: each is the integer half of the one before (frame.cpp:381-384)"""
    out = [(w, h)]
    for _ in range(1, n_levels):
        w, h = w // 2, h // 2
        out.append((w, h))
    return out


def check_premises(name):
    """what makes a size worth testing: odd widths and heights among its levels, byte counts with a 16-byte tail, and a
    level whose size is NOT the real-valued w0 / 2^k"""
    w, h = SIZES[name]
    lv = level_sizes(w, h)
    assert any(lw % 2 for lw, lh in lv) and any(lh % 2 for lw, lh in lv), lv
    assert sum((lw * lh) % 16 != 0 for lw, lh in lv[1:]) >= 3, lv
    assert any(lw != w / float(1 << k) or lh != h / float(1 << k) for k, (lw, lh) in enumerate(lv)), lv
    return lv


for _name in SIZES:
    check_premises(_name)


def camera(name, kind):
    """pinhole: f = w/2 like PinholeGeometry::createTestCamera, the principal point off the centre by a non-integer
    amount; radtan: synth.Camera.euroc_like at the size (cx = 367.215 w / 752, cy = 248.375: off-centre as well)"""
    w, h = SIZES[name]
    if kind == "pinhole":
        return synth.Camera(w, h, 0.5 * w, 0.5 * w, 0.5 * w + 3.3, 0.5 * h - 2.7)
    assert kind == "radtan"
    return synth.Camera.euroc_like(w, h)


def align_scene(name, kind, seed, n=300, **kw):
    kw.setdefault("border_features", 60)
    kw.setdefault("invalid_fraction", 0.1)
    return helpers.small_scene(seed, n=n, P=PATCH[name], cam=camera(name, kind), **kw)


# ---------------------------------------------------------------------------------------------------------------------
# extractFeaturesSubset (sparse_img_align.cpp:213-229) at max_level 4 with a 4x4 patch: patch_size_wb = 6,
# u_tl = px / 16 - 2.5, u_tl_i = floor(u_tl); kept iff 0 <= u_tl_i and u_tl_i + 6 < w4 - 2, the same for v with h4.
#   lower bound, both sizes, both axes:  floor(px / 16 - 2.5) >= 0         <=>  px >= 40
#   A, level 4 is 25 x 19:   x: u_tl_i + 6 < 23  <=>  u_tl_i <= 16  <=>  px / 16 - 2.5 < 17  <=>  px < 312
#                            y: v_tl_i + 6 < 17  <=>  v_tl_i <= 10  <=>  py / 16 - 2.5 < 11  <=>  py < 216
#   B, level 4 is 23 x 15:   x: u_tl_i + 6 < 21  <=>  u_tl_i <= 14  <=>  px < 16 * 17.5 = 280
#                            y: v_tl_i + 6 < 13  <=>  v_tl_i <= 6   <=>  py < 16 *  9.5 = 152
# A real-valued level size would move every upper bound: 413 / 16 = 25.8125 gives u_tl_i <= 17, px < 328;
# 309 / 16 = 19.3125 gives py < 232; 375 / 16 = 23.4375 gives px < 296; 247 / 16 = 15.4375 gives py < 168.
# ---------------------------------------------------------------------------------------------------------------------
SELECTION_PX = {
    "A": np.array([[39.99, 120.0], [40.0, 120.0], [311.99, 120.0], [312.0, 120.0],
                   [200.0, 39.99], [200.0, 40.0], [200.0, 215.99], [200.0, 216.0],
                   [327.99, 120.0], [200.0, 231.99]]),     # kept only by a real-valued level size
    "B": np.array([[39.99, 100.0], [40.0, 100.0], [279.99, 100.0], [280.0, 100.0],
                   [150.0, 39.99], [150.0, 40.0], [150.0, 151.99], [150.0, 152.0],
                   [295.99, 100.0], [150.0, 167.99]]),
}
SELECTION_KEPT = [False, True, True, False, False, True, True, False, False, False]


def landmarks_behind(sc, px):
    """bearing vectors (3 x n) through the pixels px (n x 2) of the reference image and the points (3 x n, world) where
    they meet the scene's plane: what synth.make_align_scene puts behind its own features"""
    x, y = sc.cam.undistorted_xy(px[:, 0], px[:, 1])
    ray = np.stack([x, y, np.ones_like(x)])
    f = ray / np.linalg.norm(ray, axis=0, keepdims=True)
    n_cam = sc.T_w_ref.R().T @ sc.plane.n
    h_cam = sc.plane.h - float(sc.plane.n @ sc.T_w_ref.t)
    return f, sc.T_w_ref.transform(f * (h_cam / (n_cam @ f)))


def selection_scene(name, kind="pinhole"):
    """a scene whose features are the crafted pixels, with the scene's own landmarks behind them"""
    px = SELECTION_PX[name]
    sc = helpers.small_scene(61, n=px.shape[0], P=4, cam=camera(name, kind))
    assert sc.n_features == px.shape[0]
    f, pos_world = landmarks_behind(sc, px)
    sc.px = px.ravel().copy()
    sc.f = np.ascontiguousarray(f.T).ravel().copy()
    sc.pos_world = np.ascontiguousarray(pos_world.T).ravel().copy()
    return sc


# ---------------------------------------------------------------------------------------------------------------------
# alignPyr2D at level 0 with a 16x16 patch (feature_alignment.cpp:789-797, 862-868): the template's corner px - 8 must be
# in [1, w - 17)  <=>  9 <= px <= w - 10; the current patch's corner floor(u) must be in [0, w - 16).
#   A: x in [9, 403], y in [9, 299];   B: x in [9, 365], y in [9, 237]
# ---------------------------------------------------------------------------------------------------------------------
def klt_boundary_tracks(name):
    """(px_ref int32 2n, px_cur float64 2n, expected status of the first 8 tracks): reference pixels one step outside /
    inside each bound, and two tracks whose CURRENT corner is exactly w - 16 (lost) and 0.01 inside (tracked)"""
    w, h = SIZES[name]
    mx, my = w // 2, h // 2
    px_ref = np.array([[x, my] for x in (8, 9, w - 10, w - 9)] + [[mx, y] for y in (8, 9, h - 10, h - 9)], np.int32)
    px_cur = px_ref.astype(np.float64)
    extra_ref = np.array([[mx, my], [mx, my]], np.int32)
    extra_cur = np.array([[w - 16 + 8.0, float(my)], [w - 16 + 8.0 - 0.01, float(my)]])
    ok = [0, 1, 1, 0, 0, 1, 1, 0]
    return np.concatenate([px_ref, extra_ref]).ravel(), np.concatenate([px_cur, extra_cur]).ravel(), ok


KLT_BOUNDS = {"A": ((9, 403), (9, 299)), "B": ((9, 365), (9, 237))}
for _name, ((_x0, _x1), (_y0, _y1)) in KLT_BOUNDS.items():
    _r, _c, _ok = klt_boundary_tracks(_name)
    assert list(_r.reshape(-1, 2)[:4, 0]) == [_x0 - 1, _x0, _x1, _x1 + 1]
    assert list(_r.reshape(-1, 2)[4:8, 1]) == [_y0 - 1, _y0, _y1, _y1 + 1]


# ---------------------------------------------------------------------------------------------------------------------
# Per-level visibility of the alignment (computeResidualsOfFrame, sparse_img_align.cpp:447-456): with the landmark projected
# to uv in the current image, u_tl = uv / 2^k - (P - 1) / 2; the patch is skipped iff u_tl < 0 or u_tl + P + 2 >= w_k (the
# same for v and h_k).  The far corner u_tl + P + 2 = uv / 2^k + (P + 5) / 2 reaches the edge at
#       uv = (w_k - (P + 5) / 2) * 2^k                       A, P = 4:  level 1: 403,  level 2: 394,  level 3: 372
# and would reach a real-valued edge w0 / 2^k at               A, P = 4:  level 1: 404,  level 2: 395,  level 3: 377
# ---------------------------------------------------------------------------------------------------------------------
def add_edge_visibility_features(sc, n_extra=40, seed=5):
    """Append n_extra features to a PINHOLE scene whose first projection into the current image (the run starts at
    T_icur_iref = identity, so the landmark projects where its bearing vector points) puts the patch's far corner within +-1
    level pixel of the right or bottom edge of level 1, 2 or 3 -- every second one between the true edge and the
    real-valued one where the two differ.  Their reference pixel is an ordinary, selected one (the selection's upper bound
    lies far inside these positions).  Returns the level-0 target pixels (n_extra x 2)."""
    cam = sc.cam
    assert cam.model == "none"
    P = sc.patch_size
    lv = level_sizes(cam.width, cam.height)
    rng = np.random.RandomState(seed)
    targets = []
    for i in range(n_extra):
        k = 1 + i % 3
        axis = (i // 3) % 2                         # 0: right edge, 1: bottom edge
        dim_k, dim0 = lv[k][axis], (cam.width, cam.height)[axis]
        edge = (dim_k - (P + 5) / 2.0) * (1 << k)    # level-0 coordinate at which the corner touches the level's edge
        edge_real = (dim0 / float(1 << k) - (P + 5) / 2.0) * (1 << k)
        if i % 2 and edge_real - edge >= 1.0:        # visible by a real-valued level size, invisible by the true one
            t = edge + rng.uniform(0.25, edge_real - edge - 0.25)
        else:                                        # within one level pixel of the true edge, never on it
            t = edge + rng.choice([-1.0, 1.0]) * rng.uniform(0.05, 1.0) * (1 << k)
        other = rng.uniform(0.3, 0.6) * (cam.height, cam.width)[axis]
        targets.append((t, other) if axis == 0 else (other, t))
    targets = np.array(targets)
    # bearing vectors through the target pixels, landmarks on the scene's plane
    f, pos_world = landmarks_behind(sc, targets)
    # reference pixels: those of the scene's first usable inner features, a few pixels aside
    px = sc.px.reshape(-1, 2)
    margin = 16 * (P + 3)
    inner = np.nonzero((px[:, 0] >= margin) & (px[:, 0] < cam.width - margin) & (px[:, 1] >= margin) &
                       (px[:, 1] < cam.height - margin) & (sc.flags == 1))[0]
    assert inner.size >= n_extra
    px_new = px[inner[:n_extra]] + rng.uniform(-0.5, 0.5, (n_extra, 2))
    sc.px = np.concatenate([sc.px, px_new.ravel()])
    sc.f = np.concatenate([sc.f, np.ascontiguousarray(f.T).ravel()])
    sc.pos_world = np.concatenate([sc.pos_world, np.ascontiguousarray(pos_world.T).ravel()])
    sc.flags = np.concatenate([sc.flags, np.ones(n_extra, np.uint8)])
    sc.n_features += n_extra
    return targets


# ---------------------------------------------------------------------------------------------------------------------
# Matcher, depth filter, epipolar seam: units whose match lies at the bound of the in-frame test of their level.
#   align1D / align2D (feature_alignment.cpp:108-112, 294-297): floor(u) >= w_L - 4 at the search level L leaves the frame
#   the epipolar scans (Matcher::isPatchWithinImage, matcher.cpp:314-322):  pxi >= w_L - 8 is not compared
#   the reference patch (findMatchDirect, oracle/svo_oracle_matcher.c):     (int)px / 2^l >= w_l - 6 is not visible
# with w_L the level's integer size (the reference divides the camera's integer width by 1 << L).
# ---------------------------------------------------------------------------------------------------------------------
def edge_units(sc, n_units=60, bound=4, levels=(0, 1, 2, 3), seed=9, depth_noise=(0.9, 1.1)):
    """n_units features of the reference frame, in synth.make_seed_set's form, whose TRUE position in the current frame lies
    within 2 level pixels of  w_l - bound  (right edge) or  h_l - bound  (bottom edge) at their own level l: the target in
    the current image is computed from the integer level size, carried to the reference image over the scene's plane and
    truncated to a detector position there."""
    cam = sc.cam
    lv = level_sizes(cam.width, cam.height)
    rng = np.random.RandomState(seed + 31337)
    level = np.array([levels[i % len(levels)] for i in range(n_units)], np.int32)
    cur = np.zeros((n_units, 2))
    for i in range(n_units):
        l, axis = int(level[i]), (i // len(levels)) % 2
        d = -2.0 + 4.0 * ((i * 7) % n_units + 0.5) / n_units          # spread over (-2, 2) level pixels
        t = (lv[l][axis] - bound + d) * (1 << l)
        other = rng.uniform(0.3, 0.7) * (cam.height, cam.width)[axis]
        cur[i] = (t, other) if axis == 0 else (other, t)
    # current pixel -> plane -> reference pixel
    x, y = cam.undistorted_xy(cur[:, 0], cur[:, 1])
    ray_w = sc.T_w_cur.R() @ np.stack([x, y, np.ones_like(x)])
    lam = (sc.plane.h - float(sc.plane.n @ sc.T_w_cur.t)) / (sc.plane.n @ ray_w)
    Xw = sc.T_w_cur.t[:, None] + ray_w * lam
    px = np.floor(cam.project(sc.T_w_ref.inverse().transform(Xw)))      # detector positions
    x, y = cam.undistorted_xy(px[0], px[1])
    ray = np.stack([x, y, np.ones_like(x)])
    f = ray / np.linalg.norm(ray, axis=0, keepdims=True)
    n_cam = sc.T_w_ref.R().T @ sc.plane.n
    h_cam = sc.plane.h - float(sc.plane.n @ sc.T_w_ref.t)
    dist = h_cam / (n_cam @ f)
    ang = rng.uniform(0, 2 * math.pi, n_units)
    grad = np.stack([np.cos(ang), np.sin(ang)])
    ftype = (rng.uniform(size=n_units) >= 0.3).astype(np.uint8)          # kEdgeletSeed = 0 / kCornerSeed = 1
    mu0 = 1.0 / (dist * rng.uniform(depth_noise[0], depth_noise[1], n_units))
    return dict(px=np.ascontiguousarray(px.T).ravel().copy(), f=np.ascontiguousarray(f.T).ravel().copy(),
                grad=np.ascontiguousarray(grad.T).ravel().copy(), level=level, type=ftype, mu0=mu0, true_depth=dist,
                ref_frame_idx=np.zeros(n_units, np.int32))


def seed_set_with_edge_units(sc, n_seeds, margin, levels, n_edge=60, bound=4, seed=0):
    """synth.make_seed_set(sc, n_seeds, ...) with edge_units appended; sd["edge"] marks them"""
    sd = synth.make_seed_set(sc, n_seeds, seed=seed, margin=margin, levels=levels)
    eu = edge_units(sc, n_edge, bound=bound, levels=tuple(l for l in levels))
    s2 = sd["mu_range"] * sd["mu_range"] / 36.0
    state = np.stack([eu["mu0"], np.full(n_edge, s2), np.full(n_edge, 10.0), np.full(n_edge, 10.0)])
    out = dict(sd)
    for k in ("px", "f", "grad", "level", "type", "true_depth", "ref_frame_idx"):
        out[k] = np.concatenate([sd[k], eu[k]]).astype(sd[k].dtype)
    out["state"] = np.concatenate([sd["state"], np.ascontiguousarray(state.T).ravel()])
    out["edge"] = np.concatenate([np.zeros(n_seeds, bool), np.ones(n_edge, bool)])
    return out


def predicted_pixels(sc, sd, noise, seed):
    """the current-frame pixels of the units' true positions (2 x n) and a start value px_true + U(-noise, noise)"""
    x = sd["f"].reshape(-1, 3).T * sd["true_depth"]
    px_true = sc.cam.project(sc.T_w_cur.inverse().transform(sc.T_w_ref.transform(x)))
    px_init = np.ascontiguousarray((px_true + np.random.RandomState(seed).uniform(-noise, noise, px_true.shape)).T).ravel()
    return px_true, px_init
