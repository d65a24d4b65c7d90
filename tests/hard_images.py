"""Degenerate image content for the kernels that read pixels, shared by tests/test_hard_images_cpu.py and
tests/test_hard_images_gpu.py (no GPU call, no oracle call).

Every other parity test renders synth.Texture: 28 sine waves around grey 128 that almost never clip.  No 8x8 patch of it is
flat, none has its gradient in one direction only, no two positions along an epipolar line score exactly the same.  Here the
content is what real frames also hold -- sky, lamps, walls, blinds, tiles, noise -- and what it selects in the code: exact
ZMSSD ties (the scans must keep the FIRST best step), singular and rank-deficient float Hessians (1/0, inf and NaN cascades
that are equal on two sides only in the reference's order of operations), the packed integer paths at 0 / 255, and updates
that run away through (int)floorf(u).

Frame pairs: 320x240, 4 pyramid levels, pinhole f = 160.  Reference pose = identity; the current camera is translated along
+x ("h") or +y ("v") by b = s d / f in front of a fronto-parallel plane at d = 2 m, so both images are crops of ONE canvas, the
current one s = 6 pixels further along: the true match of reference pixel (u, v) is (u - 6, v) resp. (u, v - 6), known by
hand, and epipolar lines are image rows resp. columns.

Families (pure functions of the integer canvas coordinates; seeded where random):
  flat       one grey value: 0, 77, 255                        H = 0: 1/det = inf, NaN positions, every score ties
  stripes    vertical bars 4 px wide, 40 / 200 (period 8 = patch size)   rank-1 H, ties every 8 px along a row ("h": the
             gradient lies along the epipolar line; "v": across it, and the two images are the same picture)
  checker    8x8 squares of 0 / 255                            +-255 differences, ties every 16 px; at level 2 the squares
             are 2x2 and a 16x16 KLT patch has h00 = h11 = 256 * 255^2 = 16 646 400, the largest sum there is
  steps      16x16 blocks of random grey, every fifth block repeated to the right (T-corners)   flat interiors, straight
             edges (rank 1), corners (full rank) side by side
  ramp       (3 x) mod 256                                     constant gradient: the zero-mean score is the same at every
             step between two wraps
  saturated  a smooth pattern with a gain that clips >= 40 % of the pixels to 0 / 255 (asserted)   plateaus and their rims
  noise      independent uniform u8

Units are placed BY CLASS (CLASS_MIX), seeded, from masks computed on the images themselves, and assert_premises() checks
every unit again from its own patch: a "flat" unit's 10x10 patch with border is constant at its level, a "straight edge"
unit's integer Hessian has h00 h11 == h01^2 (and is not zero), a "corner" unit's has full rank.
"""
import math

import numpy as np

from svo_pro_universal_amd import _capi as capi, synth

import np_restatement as n0

W, H, N_LEVELS = 320, 240, 4
CANVAS_W, CANVAS_H = 352, 272
OX, OY = 16, 16            # the reference crop's corner on the canvas (a multiple of 16: blocks and squares stay aligned at every level)
SHIFT = 6
DEPTH = 2.0
CAM = synth.Camera(width=W, height=H, fx=160.0, fy=160.0, cx=160.0, cy=120.0)

# (name, family, variant, pair)
CASES = [("flat0", "flat", 0, "h"), ("flat77", "flat", 77, "h"), ("flat255", "flat", 255, "h"),
         ("stripes_h", "stripes", None, "h"), ("stripes_v", "stripes", None, "v"),
         ("checker", "checker", None, "h"), ("steps", "steps", None, "h"), ("ramp", "ramp", None, "h"),
         ("saturated", "saturated", None, "h"), ("noise", "noise", None, "h")]
CASE_NAMES = [c[0] for c in CASES]
TIE_FAMILIES = ("stripes_h", "checker", "ramp")

# the share of a family's units per class; a class without a candidate at a level (a flat 10x10 patch does not fit into an
# 8x8 block of level 1) leaves its share to the others of that level
CLASS_MIX = {
    "flat": (("flat", 1.0),),
    "stripes": (("edge", 1.0),),                                   # on a stripe: every patch is a straight edge
    "checker": (("block_corner", 0.5), ("corner", 0.5)),
    "steps": (("flat", 0.25), ("edge", 0.35), ("block_corner", 0.4)),
    "ramp": (("wrap", 0.5), ("edge", 0.5)),                        # next to a wrap / between two wraps
    "saturated": (("plateau", 0.4), ("rim", 0.6)),
    "noise": (("corner", 1.0),),
}
FLAT_CLASSES = ("flat", "plateau")
EDGE_CLASSES = ("edge", "wrap")
CORNER_CLASSES = ("corner", "block_corner", "rim")
BLOCK = {"checker": 8, "steps": 16}


def canvas(family, variant=None):
    x, y = np.meshgrid(np.arange(CANVAS_W), np.arange(CANVAS_H))
    if family == "flat":
        img = np.full(x.shape, int(variant))
    elif family == "stripes":
        img = np.where((x // 4) % 2 == 0, 40, 200)
    elif family == "checker":
        img = ((x // 8 + y // 8) % 2) * 255
    elif family == "steps":
        t = np.random.RandomState(1601).randint(0, 256, (CANVAS_H // 16, CANVAS_W // 16))
        by, bx = np.nonzero((np.add.outer(2 * np.arange(t.shape[0]), np.arange(t.shape[1])) % 5 == 0)[:, :-1])
        t[by, bx + 1] = t[by, bx]                                   # two equal neighbours: the corners above and below are T-corners
        img = t[y // 16, x // 16]
    elif family == "ramp":
        img = (3 * x) % 256
    elif family == "saturated":
        v = 0.6 * np.sin(2 * math.pi * x / 37.0 + 0.3) * np.cos(2 * math.pi * y / 29.0) + 0.4 * np.sin(2 * math.pi * (x + y) / 53.0 + 1.1)
        img = np.clip(np.floor(128.0 + 900.0 * v + 0.5), 0, 255)
        assert np.mean((img == 0) | (img == 255)) >= 0.4, np.mean((img == 0) | (img == 255))
    elif family == "noise":
        img = np.random.RandomState(1607).randint(0, 256, x.shape)
    else:
        raise ValueError(family)
    return np.ascontiguousarray(img, dtype=np.uint8)


class Pair(object):
    """One (reference, current) frame pair of a case: images, pyramids (NumPy reading of halfSample; the tests hold the
    oracle's and the device's against them byte for byte), camera, poses (camera <- world) and the shift of the true match."""
    pass


_PAIRS = {}


def pair(name):
    if name in _PAIRS:
        return _PAIRS[name]
    _n, family, variant, axis = CASES[CASE_NAMES.index(name)]
    cv = canvas(family, variant)
    p = Pair()
    p.name, p.family, p.axis, p.cam = name, family, axis, CAM
    sx, sy = (SHIFT, 0) if axis == "h" else (0, SHIFT)
    p.shift = np.array([float(sx), float(sy)])
    p.img_ref = np.ascontiguousarray(cv[OY:OY + H, OX:OX + W])
    p.img_cur = np.ascontiguousarray(cv[OY + sy:OY + sy + H, OX + sx:OX + sx + W])
    b = SHIFT * DEPTH / CAM.fx
    p.T_ref_f_w = synth.SE3()
    p.T_cur_f_w = synth.SE3(t=(-b, 0.0, 0.0) if axis == "h" else (0.0, -b, 0.0))
    p.ref = n0.create_img_pyramid(p.img_ref, N_LEVELS)
    p.cur = n0.create_img_pyramid(p.img_cur, N_LEVELS)
    p.epi_dir = np.array([1.0, 0.0]) if axis == "h" else np.array([0.0, 1.0])
    _PAIRS[name] = p
    return p


# ---------------------------------------------------------------------------------------------------------------------
# classes, from the images
# ---------------------------------------------------------------------------------------------------------------------
def _box(a, half):
    """sum of a over the (2 half)^2 patch [y - half, y + half) x [x - half, x + half) for every centre with the patch inside"""
    h, w = a.shape
    c = np.zeros((h + 1, w + 1), np.int64)
    c[1:, 1:] = a.astype(np.int64).cumsum(0).cumsum(1)
    out = np.zeros((h, w), np.int64)
    n = 2 * half
    out[half:h - half + 1, half:w - half + 1] = c[n:, n:] - c[:-n, n:] - c[n:, :-n] + c[:-n, :-n]
    return out


def int_hessian(img, x, y, half):
    """(h00, h01, h11) of the (2 half)^2 patch centred on (x, y): sums of products of the central differences, as integers"""
    i = img.astype(np.int64)
    ys, xs = slice(y - half, y + half), slice(x - half, x + half)
    dx = i[ys, x - half + 1:x + half + 1] - i[ys, x - half - 1:x + half - 1]
    dy = i[y - half + 1:y + half + 1, xs] - i[y - half - 1:y + half - 1, xs]
    return int((dx * dx).sum()), int((dx * dy).sum()), int((dy * dy).sum())


def class_masks(family, img, half, level):
    """name -> boolean mask over the centres (x, y) of a level image, for the (2 half)^2 patch with its one-pixel border"""
    h, w = img.shape
    i = img.astype(np.int64)
    dx, dy = np.zeros_like(i), np.zeros_like(i)
    dx[:, 1:-1] = i[:, 2:] - i[:, :-2]
    dy[1:-1, :] = i[2:, :] - i[:-2, :]
    h00, h01, h11 = _box(dx * dx, half), _box(dx * dy, half), _box(dy * dy, half)
    valid = np.zeros((h, w), bool)
    valid[half + 1:h - half, half + 1:w - half] = True
    n = 2 * half + 2
    win = np.lib.stride_tricks.sliding_window_view(img, (n, n))
    const = np.zeros((h, w), bool)
    const[half + 1:half + 1 + win.shape[0], half + 1:half + 1 + win.shape[1]] = win.max(axis=(2, 3)) == win.min(axis=(2, 3))
    det = h00 * h11 - h01 * h01
    m = dict(flat=valid & const, edge=valid & ~const & (det == 0) & (h00 + h11 > 0), corner=valid & (det > 0))
    xx, yy = np.meshgrid(np.arange(w), np.arange(h))
    if family in BLOCK:
        b = BLOCK[family] >> level
        m["block_corner"] = m["corner"] & (xx % b == 0) & (yy % b == 0) if b >= 2 else np.zeros((h, w), bool)
    if family == "ramp":
        falls = np.zeros((h, w), bool)
        falls[:, :-1] = i[:, 1:] < i[:, :-1]
        m["wrap"] = m["edge"] & (_box(falls, half) > 0)
        m["edge"] = m["edge"] & ~m["wrap"]
    if family == "saturated":
        sat = (img == 0) | (img == 255)
        m["plateau"] = m["flat"] & sat
        n_sat = _box(sat, half)
        m["rim"] = m["corner"] & (n_sat > 0) & (n_sat < 4 * half * half)
    return m


def place(name, n, seed, half=4, levels=(0, 1), margin=24, moved=()):
    """n units of a case: level-0 pixel (n x 2, multiples of 2^level: detector positions), level, class name.  Per level the
    family's classes share the units by CLASS_MIX; within a class the positions are drawn (seeded) from every centre of that
    class at least `margin` level-0 pixels inside the image.  moved: indices of units whose position is drawn once more, from
    the same class at the same level (MOVED below)."""
    p = pair(name)
    rng = np.random.RandomState(seed)
    px, lv, cls, pool = [], [], [], []
    for k, level in enumerate(levels):
        n_l = n // len(levels) + (n % len(levels) if k == 0 else 0)
        masks = class_masks(p.family, p.ref[level], half, level)
        m = (margin + (1 << level) - 1) >> level
        inside = np.zeros(p.ref[level].shape, bool)
        inside[m:(H - margin) >> level, m:(W - margin) >> level] = True
        cand = [(c, wgt, np.argwhere(masks[c] & inside)) for c, wgt in CLASS_MIX[p.family]]
        cand = [(c, wgt, a) for c, wgt, a in cand if len(a)]
        assert cand, (name, level)
        total = sum(wgt for _c, wgt, _a in cand)
        counts = [int(n_l * wgt / total) for _c, wgt, _a in cand]
        counts[0] += n_l - sum(counts)
        for (c, _w, a), cnt in zip(cand, counts):
            pick = a[rng.choice(len(a), cnt, replace=len(a) < cnt)]
            px.append(pick[:, ::-1].astype(np.float64) * (1 << level))
            lv += [level] * cnt
            cls += [c] * cnt
            pool += [a] * cnt
    px = np.concatenate(px)
    for i in moved:
        a = pool[i]
        px[i] = a[np.random.RandomState(seed * 1000 + i).randint(len(a))][::-1].astype(np.float64) * (1 << lv[i])
    return px, np.array(lv, np.int32), np.array(cls)


def assert_premises(name, px, level, cls, half=4):
    """every unit is the case it claims to be, from its own patch of the reference pyramid"""
    p = pair(name)
    seen = set()
    for (x, y), l, c in zip(px, level, cls):
        img = p.ref[int(l)]
        x, y = int(x) >> int(l), int(y) >> int(l)
        patch = img[y - half - 1:y + half + 1, x - half - 1:x + half + 1]
        assert patch.shape == (2 * half + 2, 2 * half + 2), (name, x, y, l)
        h00, h01, h11 = int_hessian(img, x, y, half)
        if c in FLAT_CLASSES:
            assert patch.min() == patch.max() and h00 == h01 == h11 == 0, (name, x, y, l, c)
            if c == "plateau":
                assert patch[0, 0] in (0, 255)
        elif c in EDGE_CLASSES:
            assert h00 * h11 == h01 * h01 and h00 + h11 > 0, (name, x, y, l, c, h00, h01, h11)
        else:
            assert c in CORNER_CLASSES and h00 * h11 - h01 * h01 > 0, (name, x, y, l, c, h00, h01, h11)
        seen.add(c)
    if half == 4 and 0 in level:                # the matcher's 8x8 patch: at level 0 every class of the family is there
        seen0 = set(cls[level == 0].tolist())
        assert seen0 == set(c for c, _w in CLASS_MIX[p.family]), (name, seen0)
    return seen


# ---------------------------------------------------------------------------------------------------------------------
# unit sets (the forms of synth.make_track_set / make_seed_set)
# ---------------------------------------------------------------------------------------------------------------------
N_TRACKS, N_SEEDS, N_DIRECT, N_STEREO = 64, 256, 128, 128
# Tie counts of the placements below (tests/test_hard_images_cpu.py::test_tie_premise measures them and asserts floors of two
# thirds): of 256 seeds, those whose best ZMSSD below the threshold is reached by more than one scored step of the scan /
# ... by two steps inside one block of 64 consecutive steps / ... by steps of different blocks / ... on both sides of the turn
#                 unit plane              unit sphere
#   stripes_h      65 /  65 / 61 /  65     88 /  88 / 61 /  88
#   checker        67 /  67 / 61 /  66     88 /  87 / 61 /  87
#   ramp          148 / 142 / 43 /  93    134 / 132 / 39 / 133
#   flat*, stripes_v  249 / 249 / 61 / 154   221 / 221 / 61 / 221   (every step scores 0; the match then fails in the alignment)
#   steps         127 / 124 / 33 /  78    134 / 126 / 38 / 133
#   saturated      61 /  59 / 15 /  60     89 /  79 / 23 /  89
#   noise           8 /   6 /  2 /   8     53 /  39 / 14 /  53      (the walk comes back over pixels it has scored)
# The 61 are the wide seeds (WIDE_SIGMA) that pass the edgelet filter: only their search is longer than 64 steps.
# Moved units.  The pixelwise warp (warp::warpPixelwise) carries every patch pixel through backProject3 -> normalized() * depth
# -> T -> project3 in double and takes floor() of the result.  With a pure translation along one image axis and integer
# reference pixels the other coordinate of EVERY patch pixel comes back as an integer give or take one ulp (75.99999999999999
# or 76.0): floor() and the float weights behind it hang on the last bit of a sqrt and a division, a grey level of the patch
# moves by one (255 -> 254 on a flat white image), and on a handful of units that is enough to move the float32 alignment
# past the 1e-4 px bar or across a result code.  Neither reading is wrong; the unit's position is drawn once more:
#   direct flat255 31     pixelwise: oracle and NumPy reading differ in 2 of 100 patch pixels (254 / 255); one converges, one not
#   direct stripes_v 23, 79   pixelwise: 1 of 100 patch pixels differs by one grey level; code 5 against 0
#   direct checker 111    pixelwise: 1 patch pixel differs by one grey level; both succeed, 5.0e-4 px apart
#   direct saturated 26   pixelwise: 1 patch pixel differs by one grey level; both succeed, 1.07e-4 px apart
# (Seen between the oracle and the NumPy reading; the kernels follow the oracle's order of operations and agreed with it on
# every unit they were given.)
MOVED = {("direct", "flat255"): (31,), ("direct", "stripes_v"): (23, 79), ("direct", "checker"): (111,),
         ("direct", "saturated"): (26,)}
WIDE_SIGMA = 12.0           # every fourth seed: an inverse-depth sigma that makes the epipolar line ~150 px (~210 steps)


_SETS = {}


def _once(fn):
    """a unit set is built once per case and handed out as it is: callers copy what they change"""
    def cached(name, *args, **kw):
        key = (fn.__name__, name, args, tuple(sorted(kw.items())))
        if key not in _SETS:
            _SETS[key] = fn(name, *args, **kw)
        return _SETS[key]
    cached.__name__, cached.__doc__ = fn.__name__, fn.__doc__
    return cached


@_once
def klt_tracks(name, n=N_TRACKS, seed=11):
    """integer reference pixels by class for the 16x16 level-0 template, the tracker's start value (the reference pixel) and
    the true position"""
    px, level, cls = place(name, n, seed, half=8, levels=(0,), margin=44, moved=MOVED.get(("klt", name), ()))
    return dict(px_ref=np.ascontiguousarray(px, np.float64).astype(np.int32).ravel().copy(), px_cur_init=px.ravel().copy(),
                px_true=(px - pair(name).shift).ravel().copy(), cls=cls, level=level)


def _bearing(px):
    ray = np.stack([(px[:, 0] - CAM.cx) / CAM.fx, (px[:, 1] - CAM.cy) / CAM.fy, np.ones(len(px))])
    f = ray / np.linalg.norm(ray, axis=0, keepdims=True)
    return f, DEPTH / f[2]


def _gradients(p, rng, n, across_fraction=0.12):
    """edgelet gradients along the epipolar line (within 0.5 rad, inside the filter's cos > 0.7), a few across it"""
    a = math.atan2(p.epi_dir[1], p.epi_dir[0]) + rng.uniform(-0.5, 0.5, n) + math.pi * rng.randint(0, 2, n)
    across = rng.uniform(size=n) < across_fraction
    a = np.where(across, a + 0.5 * math.pi + rng.uniform(-0.3, 0.3, n), a)
    return np.stack([np.cos(a), np.sin(a)])


@_once
def seed_set(name, n=N_SEEDS, seed=23, edgelet_fraction=0.3, depth_noise=(0.7, 1.3)):
    """seeds with priors like depth_filter_utils::initializeSeeds (synth.make_seed_set's form): mu within 0.7-1.3 of the
    truth, sigma2 = mu_range^2 / 36, a = b = 10; every fourth seed with sigma = WIDE_SIGMA, a long search"""
    p = pair(name)
    px, level, cls = place(name, n, seed, moved=MOVED.get(("seeds", name), ()))
    rng = np.random.RandomState(seed + 104729)
    f, dist = _bearing(px)
    mu_range = 1.0 / (0.5 * float(dist.min()))
    mu0 = 1.0 / (dist * rng.uniform(depth_noise[0], depth_noise[1], n))
    sigma2 = np.full(n, mu_range * mu_range / 36.0)
    wide = np.arange(n) % 4 == 3
    sigma2[wide] = WIDE_SIGMA * WIDE_SIGMA
    state = np.stack([mu0, sigma2, np.full(n, 10.0), np.full(n, 10.0)])
    ftype = np.where(rng.uniform(size=n) < edgelet_fraction, 0, 1).astype(np.uint8)       # kEdgeletSeed / kCornerSeed
    grad = _gradients(p, rng, n)
    return dict(px=px.ravel().copy(), f=np.ascontiguousarray(f.T).ravel().copy(), grad=np.ascontiguousarray(grad.T).ravel().copy(),
                level=level, type=ftype, state=np.ascontiguousarray(state.T).ravel().copy(), mu_range=mu_range, true_depth=dist,
                ref_frame_idx=np.zeros(n, np.int32), cls=cls, wide=wide, px_true=(px - p.shift).ravel().copy())


@_once
def direct_set(name, n=N_DIRECT, seed=37):
    """candidates of Matcher::findMatchDirect: detector features with their true depth, a start within +-2 px of the
    truth, ten of them 40 px away; landmarks (world = reference camera) for the pixelwise warp"""
    p = pair(name)
    px, level, cls = place(name, n, seed, moved=MOVED.get(("direct", name), ()))
    rng = np.random.RandomState(seed + 7919)
    f, dist = _bearing(px)
    ftype = np.where(rng.uniform(size=n) < 0.3, capi.FT_EDGELET, capi.FT_CORNER).astype(np.uint8)
    grad = _gradients(p, rng, n)
    px_true = px - p.shift
    px_init = px_true + rng.uniform(-2.0, 2.0, px_true.shape)
    px_init[:10] += 40.0
    return dict(px=px.ravel().copy(), f=np.ascontiguousarray(f.T).ravel().copy(), grad=np.ascontiguousarray(grad.T).ravel().copy(),
                level=level, type=ftype, true_depth=dist, ref_frame_idx=np.zeros(n, np.int32), cls=cls,
                px_true=px_true.ravel().copy(), px_init=px_init.ravel().copy(),
                landmark_xyz=np.ascontiguousarray((f * dist).T).copy())


@_once
def stereo_set(name, n=N_STEREO, seed=41):
    """new features of the left (= reference) image for StereoTriangulation::compute's epipolar matches, 500 steps: the
    depth range [0.04, 15] x the mean makes the epipolar line ~140 px, three rounds of a 64-step scan"""
    p = pair(name)
    px, level, cls = place(name, n, seed, moved=MOVED.get(("stereo", name), ()))
    rng = np.random.RandomState(seed + 31337)
    f, dist = _bearing(px)
    ftype = np.where(rng.uniform(size=n) < 0.3, capi.FT_EDGELET, capi.FT_CORNER).astype(np.uint8)
    grad = _gradients(p, rng, n)
    d_mean = float(np.median(dist))
    return dict(px=px.ravel().copy(), f=np.ascontiguousarray(f.T).ravel().copy(), grad=np.ascontiguousarray(grad.T).ravel().copy(),
                level=level, type=ftype, true_depth=dist, ref_frame_idx=np.zeros(n, np.int32), cls=cls,
                d_inv=[1.0 / d_mean, 1.0 / (0.04 * d_mean), 1.0 / (15.0 * d_mean)],
                T_f1f0=(p.T_cur_f_w * p.T_ref_f_w.inverse()).as7(), px_true=(px - p.shift).ravel().copy())


# ---------------------------------------------------------------------------------------------------------------------
# sparse image alignment on the same frame pairs
# ---------------------------------------------------------------------------------------------------------------------
ALIGN_FAMILIES = ("steps", "saturated", "noise")
ALIGN_LEVELS = (3, 2, 1)          # max_level 3 (four pyramid levels) down to the default min_level 1
N_ALIGN = 60


def align_full_rank(name, x, y, patch_size):
    """the premise of an alignment feature: around (x, y) / 2^L the patch_size^2 patch's integer Hessian has full rank at every
    level used"""
    p = pair(name)
    for level in ALIGN_LEVELS:
        h00, h01, h11 = int_hessian(p.ref[level], int(x) >> level, int(y) >> level, patch_size // 2)
        if h00 * h11 - h01 * h01 <= 0:
            return False
    return True


@_once
def align_scene(name, patch_size, n=N_ALIGN, seed=53):
    """an object with the attributes of synth.AlignScene (what frontend.make_align_problems and the oracle's
    problem_from_scenes read): n features on block corners (steps), plateau rims (saturated) or anywhere (noise), at multiples of
    8 px so that their centre is a pixel of every level used, each of full rank at every level for 4x4 AND 8x8 patches.  No problem
    is flat; the camera is its own IMU frame; the run starts at the identity, the truth is the pair's translation."""
    p = pair(name)
    assert p.family in ALIGN_FAMILIES
    margin = (1 << ALIGN_LEVELS[0]) * (8 + 3)
    sat = (p.ref[0] == 0) | (p.ref[0] == 255)
    n_sat = _box(sat, 4)
    cand = []
    for y in range(margin, H - margin + 1, 8):
        for x in range(margin, W - margin + 1, 8):
            if p.family == "steps" and (x % 16 or y % 16):
                continue                                              # block corners
            if p.family == "saturated" and not 0 < n_sat[y, x] < 64:
                continue                                              # a rim: saturated and unsaturated pixels under the patch
            if align_full_rank(name, x, y, 4) and align_full_rank(name, x, y, 8):
                cand.append((x, y))
    assert len(cand) >= n // 3, (name, len(cand))
    rng = np.random.RandomState(seed)
    px = np.array(cand, np.float64)[rng.choice(len(cand), n, replace=len(cand) < n)]
    f, dist = _bearing(px)
    sc = synth.AlignScene()
    sc.seed, sc.cam, sc.patch_size = seed, CAM, patch_size
    sc.img_ref, sc.img_cur = p.img_ref, p.img_cur
    sc.T_cam_imu, sc.T_imu_cam = synth.SE3(), synth.SE3()
    sc.T_ref_f_w, sc.T_cur_f_w_gt = p.T_ref_f_w, p.T_cur_f_w
    sc.px = px.ravel().copy()
    sc.f = np.ascontiguousarray(f.T).ravel().copy()
    sc.pos_world = np.ascontiguousarray((f * dist).T).ravel().copy()
    sc.flags = np.ones(n, np.uint8)
    sc.n_features, sc.depth = n, dist
    sc.T_icur_iref_gt, sc.T_icur_iref_init = p.T_cur_f_w, synth.SE3()
    sc.ref_pos = np.zeros(3)
    return sc
