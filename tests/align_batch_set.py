"""A seeded, ragged set of alignment problems large enough to run in the BATCH build of the alignment kernel
(sparse_align_kernel<P, 256, ILLUM, false, ROBUST, 1, false, false>: two 256-thread workgroups per compute unit that
take problem after problem from a queue), for tests/test_sparse_align_batch_build_gpu.py.

compose() is pure NumPy: it returns WHAT a launch is made of -- per problem its cameras (camera kind, scene seed,
feature counts, motion, illumination change), prior, initial values, start pose and where its feature arrays live.
BatchSet (GPU) renders the images, builds the pyramids and makes the device and oracle problems.

What the set guarantees (tests/test_align_batch_set_cpu.py asserts every line of it):
  * main set: 5 * num_cus problems that every launch runs + a few 4x4-only rigs; the grid is 2 * num_cus workgroups, so
    >= 3 * num_cus problems run as a workgroup's second or later problem; mid set: num_cus + 17 problems
  * feature counts 12 ... 2000, skewed small, mean near 250, the wave / workspace edges REQUIRED_COUNTS each present
  * cameras: pinhole 640x480, radtan 640x480, radtan 752x480 (level 4 = 1410 bytes: the staging's tail loop; levels
    4..2 do not fit the image area: level 2 is staged over the resident ones)
  * rigs: two cameras (>= 5 %; they take turns in this build), four 640x480 cameras (exactly kMaxStageItems images
    resident), three 320x240 cameras (18 resident images: the table overflows, the workgroup stages level by level;
    4x4 patches only: the feature margin of 8x8 patches does not fit that sensor), a camera without a usable feature
  * priors (>= 5 %), non-zero alpha_init / beta_init, problems with no usable feature (>= 2 %), problems that start
    looking away (>= 2 %), border / invalid features, large motions, host- and device-resident feature arrays
  * adjacency -- the queue hands out consecutive indices, so stale state of problem i meets problem i + 1: consecutive
    problems never share an image (every camera of the set has its own scene seed), never have the same camera kind
    (model and resolution) at the same camera index, never fall in the same feature-count class (SIZE_CLASS_EDGES:
    one wave, one workgroup pass, two passes, more), and a degenerate problem is followed by an ordinary one (one
    camera, every feature usable or nearly, starts at the identity)
"""
import numpy as np

from svo_pro_universal_amd import synth

REQUIRED_COUNTS = (12, 33, 63, 64, 65, 255, 256, 257, 340, 341, 513, 2000)
SIZE_CLASS_EDGES = (64, 256, 512)          # <= 64 | 65..256 | 257..512 | > 512 features (all cameras together)
MONO_KINDS = ("pinhole640", "radtan752", "radtan640")
LARGE_MOTION = dict(rot_deg=(1.5, 3.0), trans_m=(0.05, 0.12))
N_SMALL_RIGS_MAIN, N_SMALL_RIGS_MID = 6, 4
K_MAX_STAGE_ITEMS = 16                     # kMaxStageItems (csrc/sparse_align.hip)
LDS_IMG_REQUEST = 52224                    # what enqueue_align asks for the 256-thread geometry before launch_one trims it
LDS_PER_CU = 163840
# Scenes the ORACLE cannot judge: with the illumination terms estimated, the Gauss-Newton iteration of scene 100634 (97 features)
# diverges at level 4 (alpha = -30.5, beta = 4088, no patch visible from level 3 down), and the oracle's own result moves by
# 2.6e-8 in the pose when nothing but the order of its features -- the order of its sums -- changes: more than the 1e-8 it is asked
# to judge by (every build of the kernel, the ones with parity tests of their own included, lands 1.8e-8 from it, with equal
# iteration counts).  The scene gets another seed; test_oracle_agrees_with_itself_on_the_set (GPU file) holds every problem of
# the set to that criterion, which involves the oracle alone.
REPLACED_SCENE_SEEDS = {100634: 500634}


def camera_of(kind):
    if kind == "pinhole640":
        return synth.Camera.test_camera()
    if kind == "radtan640":
        return synth.Camera.euroc_like()
    if kind == "radtan752":
        return synth.Camera.euroc_like(752, 480)
    if kind == "pinholeB640":              # a second pinhole for the four-camera rigs
        return synth.Camera(640, 480, 400.0, 400.0, 310.0, 250.0)
    if kind == "small320":
        return synth.Camera(320, 240, 160.0, 160.0, 160.0, 120.0)
    raise ValueError(kind)


def size_class(n):
    return int(np.searchsorted(SIZE_CLASS_EDGES, n, side="left"))


class CamSpec(object):
    """One camera of a problem: make_align_scene(seed, n_total - border, cam=camera_of(kind), border_features=border, ...)."""
    FIELDS = ("kind", "seed", "n_total", "border", "invalid", "gain", "offset", "large_motion", "no_flags")

    def __init__(self, kind, seed, n_total, border=0, invalid=0.0, gain=1.0, offset=0.0, large_motion=False, no_flags=False):
        self.kind, self.seed, self.n_total, self.border, self.invalid = kind, int(seed), int(n_total), int(border), float(invalid)
        self.gain, self.offset, self.large_motion, self.no_flags = float(gain), float(offset), bool(large_motion), bool(no_flags)

    def astuple(self):
        return tuple(getattr(self, f) for f in self.FIELDS)

    def scene(self, P):
        kw = dict(LARGE_MOTION) if self.large_motion else {}
        sc = synth.make_align_scene(self.seed, n_features=self.n_total - self.border, patch_size=P, cam=camera_of(self.kind),
                                    border_features=self.border, invalid_fraction=self.invalid, gain=self.gain,
                                    offset=self.offset, render_images=False, **kw)
        assert sc.n_features == self.n_total
        if self.no_flags:
            sc.flags[:] = 0
        return sc


class ProblemSpec(object):
    """kind: mono | stereo | quad | small_rig.  degenerate: None | "no_flags" | "away".  prior: None or
    (axis, angle, t, lambda_rot, lambda_trans, alpha, beta, lambda_alpha, lambda_beta).  mem: "device" | "host"."""

    def __init__(self, kind, cams, prior=None, alpha_init=0.0, beta_init=0.0, degenerate=None, mem="device"):
        self.kind, self.cams, self.prior = kind, cams, prior
        self.alpha_init, self.beta_init, self.degenerate, self.mem = float(alpha_init), float(beta_init), degenerate, mem

    @property
    def n_features(self):
        return sum(c.n_total for c in self.cams)

    @property
    def p8(self):
        """part of the 8x8 launches (the 320x240 sensor has no room for the 8x8 feature margin)"""
        return self.kind != "small_rig"

    @property
    def ordinary(self):
        c = self.cams[0]
        return (self.kind == "mono" and self.degenerate is None and self.prior is None and not c.large_motion
                and c.border == 0 and c.invalid == 0.0 and not c.no_flags)

    def astuple(self):
        return (self.kind, tuple(c.astuple() for c in self.cams), self.prior, self.alpha_init, self.beta_init, self.degenerate, self.mem)


def _draw_count(rng):
    """12 ... 2000, skewed small (log-normal around 150; with the required edges and the rigs the set's mean is near 250)"""
    return int(np.clip(np.exp(rng.normal(np.log(150.0), 0.9)), 12, 2000))


def _count_in_other_class(rng, avoid):
    for _ in range(1000):
        n = _draw_count(rng)
        if size_class(n) not in avoid:
            return n
    raise AssertionError("no feature count outside classes %r" % (avoid,))


def _prior(rng, illum):
    axis = tuple(float(x) for x in rng.normal(size=3))
    t = tuple(float(x) for x in rng.uniform(-0.003, 0.003, 3))
    lam = (0.5, 0.0), (2.0, 3.0), (0.1, 0.1)
    lr, lt = lam[rng.randint(0, 3)]
    if illum:   # test_prior's third case: illumination prior as well
        return (axis, 0.004, t, lr, lt, 0.01, -0.5, 0.5, 0.5)
    return (axis, 0.004, t, lr, lt, 0.0, 0.0, 0.0, 0.0)


def _compose_one(rng, n_problems, n_small_rigs, seed_base, required):
    """One launch's composition, problem by problem; every special kind has its stride, ordinary problems fill the rest."""
    specs = []
    next_seed = [seed_base]

    def seed():
        next_seed[0] += 1
        return REPLACED_SCENE_SEEDS.get(next_seed[0], next_seed[0])

    required = list(required)
    # positions of the special problems: strides chosen so that the shares of the module docstring hold for any size
    kind_at = {}

    def place(name, first, stride, limit=None):
        k, placed = first, 0
        while k < n_problems - 1 and (limit is None or placed < limit):
            while k in kind_at or (k - 1) in kind_at and kind_at[k - 1] in ("no_flags", "away", "small_rig"):
                k += 1
            if k >= n_problems - 1:
                break
            kind_at[k] = name
            placed += 1
            k += stride
    place("no_flags", 7, 40)           # >= 2 %
    place("away", 11, 40)              # >= 2 %
    # (the 8x8 launches leave the small rigs out: the problem behind one is then the neighbour of the one in front of it, so it
    # is a one-camera problem that differs from both -- no special problem is placed there)
    place("small_rig", 23, max(8, (n_problems - 30) // max(1, n_small_rigs)), limit=n_small_rigs)
    place("stereo", 3, 14)             # >= 5 % two-camera rigs (with the 752 and the empty-camera ones below)
    place("stereo752", 19, 90)
    place("stereo_empty", 29, 150)
    place("quad", 37, 160)
    place("prior", 5, 16)              # >= 5 %
    place("prior_illum", 13, 48)
    place("init", 9, 36)               # non-zero alpha_init / beta_init
    place("border", 2, 12)
    place("large_motion", 6, 30)
    assert sum(1 for v in kind_at.values() if v == "small_rig") == n_small_rigs
    for i in range(n_problems):
        what = kind_at.get(i, "plain")
        prev = specs[-1] if specs else None
        prev_kinds = [c.kind for c in prev.cams] if prev else []
        prev_class = size_class(prev.n_features) if prev else -1
        # what a one-camera problem must differ from: its predecessor, and across a small rig the problem in front of that
        around = [p for p in (prev, specs[-2] if prev is not None and prev.kind == "small_rig" and len(specs) > 1 else None) if p is not None]
        avoid_kinds = set(p.cams[0].kind for p in around)
        avoid_classes = set(size_class(p.n_features) for p in around)
        after_degenerate = prev is not None and prev.degenerate is not None

        def mono_kind():
            ks = [k for k in MONO_KINDS if k not in avoid_kinds]
            return ks[rng.randint(0, len(ks))]

        mem = "host" if rng.uniform() < 0.2 else "device"
        if what == "plain" or after_degenerate:
            # an ordinary problem; the required feature counts are used up here, where the class rule allows
            n = None
            for r in required:
                if size_class(r) not in avoid_classes:
                    n = r
                    required.remove(r)
                    break
            if n is None:
                n = _count_in_other_class(rng, avoid_classes)
            specs.append(ProblemSpec("mono", [CamSpec(mono_kind(), seed(), n, gain=1.0 + 0.04 * rng.uniform(), offset=3.0 * rng.uniform())], mem=mem))
            continue
        n = _count_in_other_class(rng, avoid_classes)
        if what in ("no_flags", "away"):
            specs.append(ProblemSpec("mono", [CamSpec(mono_kind(), seed(), n, no_flags=(what == "no_flags"))], degenerate=what, mem=mem))
        elif what in ("stereo", "stereo752", "stereo_empty"):
            # two cameras whose kinds differ from the previous problem's at both indices; the pair's total in another class
            pool = ("radtan752", "pinhole640") if what == "stereo752" else ("pinhole640", "radtan640")
            k0 = [k for k in pool if not prev_kinds or k != prev_kinds[0]][0]
            k1 = [k for k in (pool + ("radtan752", "radtan640")) if k != k0 and (len(prev_kinds) < 2 or k != prev_kinds[1])][0]
            n0 = max(12, n * 5 // 9)
            n1 = max(12, n - n0)
            if size_class(n0 + n1) == prev_class:
                n1 += 64 if size_class(n0 + n1 + 64) != prev_class else 256
            cams = [CamSpec(k0, seed(), n0, border=min(6, n0 // 4), gain=1.02, offset=1.5),
                    CamSpec(k1, seed(), n1, border=min(6, n1 // 4), gain=1.02, offset=1.5, no_flags=(what == "stereo_empty"))]
            specs.append(ProblemSpec("stereo", cams, mem=mem, prior=_prior(rng, False) if rng.uniform() < 0.3 else None))
        elif what == "quad":
            kinds = ["pinhole640", "radtan640", "pinholeB640", "radtan640"]
            if prev_kinds and prev_kinds[0] == "pinhole640":
                kinds = ["radtan640", "pinholeB640", "radtan640", "pinhole640"]
            if len(prev_kinds) > 1 and prev_kinds[1] == kinds[1]:
                kinds[1], kinds[2] = kinds[2], kinds[1]
            per = {0: (14, 15, 16, 17), 1: (40, 45, 50, 55), 2: (90, 100, 110, 120), 3: (150, 170, 130, 160)}[(prev_class + 1) % 4]
            specs.append(ProblemSpec("quad", [CamSpec(k, seed(), m, border=min(4, m // 4)) for k, m in zip(kinds, per)], mem=mem))
        elif what == "small_rig":
            per = (20, 24, 28) if prev_class != 1 else (12, 14, 16)
            specs.append(ProblemSpec("small_rig", [CamSpec("small320", seed(), m) for m in per], mem=mem))
        elif what in ("prior", "prior_illum"):
            specs.append(ProblemSpec("mono", [CamSpec(mono_kind(), seed(), n, gain=1.02, offset=1.0)], prior=_prior(rng, what == "prior_illum"),
                                     alpha_init=0.0 if what == "prior" else 0.005, beta_init=0.0 if what == "prior" else -0.2, mem=mem))
        elif what == "init":
            specs.append(ProblemSpec("mono", [CamSpec(mono_kind(), seed(), n, gain=1.03, offset=2.0)], alpha_init=0.02 * rng.uniform(-1, 1),
                                     beta_init=float(rng.uniform(-2.0, 2.0)), mem=mem))
        elif what == "border":
            b = min(60, max(2, n // 5))
            specs.append(ProblemSpec("mono", [CamSpec(mono_kind(), seed(), n, border=b, invalid=0.1)], mem=mem))
        elif what == "large_motion":
            specs.append(ProblemSpec("mono", [CamSpec(mono_kind(), seed(), n, border=n // 2, large_motion=True)], mem=mem))
        else:
            raise AssertionError(what)
    assert not required, "required feature counts left over: %r" % (required,)
    return specs


class Composition(object):
    def __init__(self, num_cus, seed, main, mid):
        self.num_cus, self.seed, self.main, self.mid = num_cus, seed, main, mid

    def launch(self, which, P):
        """the problems of the main / mid launch for PxP patches"""
        specs = self.main if which == "main" else self.mid
        return [s for s in specs if P == 4 or s.p8]

    def astuple(self):
        return (self.num_cus, self.seed, tuple(s.astuple() for s in self.main), tuple(s.astuple() for s in self.mid))


def compose(num_cus, seed=20240611):
    """The composition of the two launches for a device of num_cus compute units; bit-reproducible from the seed."""
    rng = np.random.RandomState(seed)
    main = _compose_one(rng, 5 * num_cus + N_SMALL_RIGS_MAIN, N_SMALL_RIGS_MAIN, 100000, REQUIRED_COUNTS)
    mid = _compose_one(rng, num_cus + 17, N_SMALL_RIGS_MID, 300000, (2000, 513, 12))
    return Composition(num_cus, seed, main, mid)


# ---- a host-side copy of the kernel's staging arithmetic (csrc/sparse_align.hip: the resident-levels block of the kernel) ----

def staging_plan(cam_sizes, level_hi, level_lo, lds_img_bytes):
    """cam_sizes: [(w, h)] of level 0, one per camera.  Returns (resident levels, images in the table, list_ok):
    which levels stay in LDS for the problem's life, how many images that is, and whether the register-staged list takes them
    (frames built by the library are unpadded and 16-byte aligned, so only the table's size can say no)."""
    def level_bytes(l):
        return sum(2 * ((((w >> l) * (h >> l)) + 15) & ~15) for w, h in cam_sizes)
    off, n_items, room, list_ok, resident = 0, 0, True, True, []
    for l in range(level_hi, level_lo - 1, -1):
        need = level_bytes(l)
        room = room and off + need <= lds_img_bytes
        if not room:
            continue
        for _ in range(2 * len(cam_sizes)):
            list_ok = list_ok and n_items < K_MAX_STAGE_ITEMS
            n_items += 1
        resident.append(l)
        off += need
    return resident, n_items, list_ok


def lds_img_bytes_for(static_lds):
    """launch_one: the image area of a 256-thread workgroup that shares its compute unit with a second one"""
    room = (LDS_PER_CU // 2 - static_lds) & ~15 if LDS_PER_CU // 2 > static_lds else 0
    return min(LDS_IMG_REQUEST & ~15, room)


# ---- GPU side ----------------------------------------------------------------------------------------------------------------

AWAY = synth.SE3(synth.quat_from_axis_angle([0, 1, 0], 2.5), [0, 0, 0])


def make_prior(p):
    import helpers
    axis, angle, t, lr, lt, a, b, la, lb = p
    return helpers.make_prior(synth.SE3(synth.quat_from_axis_angle(list(axis), angle), list(t)), lr, lt, alpha=a, beta=b,
                              lambda_alpha=la, lambda_beta=lb)


class Launch(object):
    """One launch's problems for one patch size: the device problems (ctypes array), the oracle's, and their specs."""
    pass


class BatchSet(object):
    """The rendered set: frames on the device (released by close()), host pyramids for the oracle."""

    N_LEVELS = 5

    def __init__(self, ctx, orc, comp, device="cuda:0"):
        import torch
        from svo_pro_universal_amd import frontend as fe
        self.ctx, self.orc, self.comp, self.fe, self.torch, self.device = ctx, orc, comp, fe, torch, device
        self._frames = []
        self._keep = []
        self.pyr = {}        # camera seed -> (frame_ref, frame_cur, levels_ref, levels_cur)
        by_kind = {}
        for s in comp.main + comp.mid:
            for c in s.cams:
                by_kind.setdefault(c.kind, []).append(c)
        self.n_pairs = {k: len(v) for k, v in by_kind.items()}
        for kind, cams in sorted(by_kind.items()):
            cam = camera_of(kind)
            for c0 in range(0, len(cams), 256):     # 256 pairs at a time: 157 MB of 640x480 images on the device
                part = cams[c0:c0 + 256]
                poses, planes, texs, gains, offsets = [], [], [], [], []
                for c in part:
                    sc = c.scene(4)
                    poses += [sc.T_w_ref, sc.T_w_cur]
                    planes += [sc.plane, sc.plane]
                    texs += [sc.tex, sc.tex]
                    gains += [1.0, c.gain]
                    offsets += [0.0, c.offset]
                imgs = synth.render_batch_torch(cam, poses, planes, texs, device, gains=gains, offsets=offsets)
                torch.cuda.synchronize()
                frames = ctx.build_pyramid_batch_device(imgs.data_ptr(), cam.width * cam.height, len(poses), cam.width, cam.height,
                                                        cam.width, self.N_LEVELS)
                ctx.synchronize()
                self._frames += frames
                host = imgs.cpu().numpy()           # copied back once, for the oracle
                del imgs
                for k, c in enumerate(part):
                    self.pyr[c.seed] = (frames[2 * k], frames[2 * k + 1], orc.create_img_pyramid(host[2 * k], self.N_LEVELS),
                                        orc.create_img_pyramid(host[2 * k + 1], self.N_LEVELS))
        self._launches = {}

    def check_pyramids(self, n=6):
        """the oracle's pyramid equals the device's on a handful of frames of every camera kind (the plumbing, not the pyramid kernel)"""
        seen = {}
        for s in self.comp.main:
            for c in s.cams:
                if seen.setdefault(c.kind, 0) < n:
                    seen[c.kind] += 1
                    fr, fc, lr, lc = self.pyr[c.seed]
                    for frame, levels in ((fr, lr), (fc, lc)):
                        for l in range(self.N_LEVELS):
                            assert np.array_equal(self.ctx.download_level(frame, l), levels[l]), (c.kind, c.seed, l)
        return seen

    def launch(self, which, P):
        if (which, P) in self._launches:
            return self._launches[(which, P)]
        torch, fe = self.torch, self.fe
        specs = self.comp.launch(which, P)
        scenes = [[c.scene(P) for c in s.cams] for s in specs]
        # device-resident feature arrays: one buffer per kind, as the benchmark keeps them
        dev_scs = [sc for s, scs in zip(specs, scenes) if s.mem == "device" for sc in scs]
        bufs = [torch.from_numpy(np.concatenate([getattr(sc, name) for sc in dev_scs])).to(self.device)
                for name in ("px", "f", "pos_world", "flags")]
        torch.cuda.synchronize()
        items, off = [], 0
        for s, scs in zip(specs, scenes):
            cams = []
            for c, sc in zip(s.cams, scs):
                fr, fc = self.pyr[c.seed][:2]
                if s.mem == "device":
                    dp = dict(px=bufs[0].data_ptr() + 16 * off, f=bufs[1].data_ptr() + 24 * off, pos_world=bufs[2].data_ptr() + 24 * off,
                              flags=bufs[3].data_ptr() + off)
                    off += sc.n_features
                    cams.append((sc, fr, fc, dp))
                else:
                    cams.append((sc, fr, fc))
            items.append(cams)
        T_init = [AWAY if s.degenerate == "away" else None for s in specs]
        pbs, keep = fe.make_align_problems(items, T_init=T_init)
        oracle_pbs = []
        for i, (s, scs) in enumerate(zip(specs, scenes)):
            prior = make_prior(s.prior) if s.prior is not None else None
            pbs[i].alpha_init, pbs[i].beta_init = s.alpha_init, s.beta_init
            if prior is not None:
                pbs[i].prior = prior
            cams_o = [(sc, self.pyr[c.seed][2], self.pyr[c.seed][3]) for c, sc in zip(s.cams, scs)]
            oracle_pbs.append(self.orc.problem_from_scenes(cams_o, T_init=T_init[i], prior=prior, alpha_init=s.alpha_init,
                                                           beta_init=s.beta_init))
        # the oracle's problems once more with every camera's features in another order (the order of the oracle's sums)
        permuted = []
        for i, (s, scs) in enumerate(zip(specs, scenes)):
            cams_p = []
            for c, sc in zip(s.cams, scs):
                perm = np.random.RandomState(c.seed).permutation(sc.n_features)
                sp = synth.AlignScene()
                sp.__dict__.update(sc.__dict__)
                sp.px, sp.f = sc.px.reshape(-1, 2)[perm].ravel(), sc.f.reshape(-1, 3)[perm].ravel()
                sp.pos_world, sp.flags = sc.pos_world.reshape(-1, 3)[perm].ravel(), sc.flags[perm]
                cams_p.append((sp, self.pyr[c.seed][2], self.pyr[c.seed][3]))
            prior = make_prior(s.prior) if s.prior is not None else None
            permuted.append(self.orc.problem_from_scenes(cams_p, T_init=T_init[i], prior=prior, alpha_init=s.alpha_init, beta_init=s.beta_init))
        L = Launch()
        L.oracle_problems_permuted = permuted
        L.specs, L.scenes, L.problems, L.oracle_problems, L.keep = specs, scenes, pbs, oracle_pbs, (bufs, keep)
        self._launches[(which, P)] = L
        return L

    def close(self):
        self._launches.clear()
        for f in self._frames:
            self.ctx.release_frame(f)
        self._frames = []
        self.pyr.clear()
