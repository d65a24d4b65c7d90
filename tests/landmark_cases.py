"""An independent reading of the landmark bookkeeping, and the scenarios it is compared on.

The host mirrors decide which observations the structure kernel is given: upgradeSeedsToFeatures, the stereo
triangulation's and the initialiser's point creation, a keyframe leaving the map, optimizeStructure's selection.
This module restates that bookkeeping from the reference's text in plain Python -- frames and points are dicts,
observations are lists of (frame id, feature index) -- and does not call the host library:

    Point::addObservation / removeObservation           svo_common/src/point.cpp:41-66
    FrameHandlerBase::upgradeSeedsToFeatures            svo/src/frame_handler_base.cpp:828-918
    FrameHandlerBase::optimizeStructure (selection)     svo/src/frame_handler_base.cpp:779-825
    StereoTriangulation::compute (point creation)       svo/src/stereo_triangulation.cpp:95-137
    initialization_utils::rescaleAndInitializePoints    svo/src/initialization.cpp:800-840 (and :556-564)
    Map::removeKeyframe (observation removal)           svo/src/map.cpp:64-93

A scenario is a script: one event per line (see `Reading.feed`).  tests/cpp/landmarks_tool.cpp replays the same
script through the real mirrors and writes the same dump; the two are compared as text, every double printed
with 17 significant digits.  Positions are computed with the operation order of svoh_math.h (itself a
restatement of minkindr's quaternion transforms), in Python floats, so that they are the same doubles.

What a dump holds: a line per event that reports something (`upgraded`, `init`, `stereo`, a `step` block per
frame of a structure step, `throw`), and `state` blocks: every point with its live observations, every frame the
scene still holds, and which frames are alive at all.

`Reading(dedupe=False)` is the bookkeeping with a bare append in place of Point::addObservation -- what the
mirrors did before they were corrected; the discrimination test uses it to put the duplicates back.
"""
import math

import numpy as np

from svo_pro_universal_amd import _capi as capi, synth

EDGELET_TYPES = (capi.FT_EDGELET, capi.FT_EDGELET_SEED, capi.FT_EDGELET_SEED_CONVERGED)          # types.h:113-118
CORNER_TYPES = (capi.FT_CORNER, capi.FT_CORNER_SEED, capi.FT_CORNER_SEED_CONVERGED)             # types.h:106-111
MAPPOINT_TYPES = (capi.FT_MAPPOINT, capi.FT_MAPPOINT_SEED, capi.FT_MAPPOINT_SEED_CONVERGED)     # types.h:120-125
FIRST_UPGRADE_ID = 1 << 20        # the harnesses' counter of upgraded points; the triangulation's counts from 0


class Conflict(Exception):
    """Point::addObservation's CHECK_EQ(it->keypoint_index_, feature_index), point.cpp:56."""


# ---- rigid transforms on Python floats, in svoh_math.h's operation order ------------------------------------
def _rotate(q, v):
    w, x, y, z = q
    ux = y * v[2] - z * v[1]
    uy = z * v[0] - x * v[2]
    uz = x * v[1] - y * v[0]
    ux += ux
    uy += uy
    uz += uz
    return (v[0] + w * ux + (y * uz - z * uy), v[1] + w * uy + (z * ux - x * uz), v[2] + w * uz + (x * uy - y * ux))


def _sqnorm(q):
    return q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]


def _inverse_rotate(q, v):
    n2 = _sqnorm(q)
    return _rotate((q[0] / n2, -q[1] / n2, -q[2] / n2, -q[3] / n2), v)


def t_transform(T, p):
    r = _rotate(T[:4], p)
    return (r[0] + T[4], r[1] + T[5], r[2] + T[6])


def t_inverse(T):
    it = _inverse_rotate(T[:4], T[4:])
    return (T[0], -T[1], -T[2], -T[3], -it[0], -it[1], -it[2])


def t_mul(a, b):
    aw, ax, ay, az = a[:4]
    bw, bx, by, bz = b[:4]
    q = (aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
         aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx)
    if abs(_sqnorm(q) - 1.0) > 1.0e-4:      # minkindr renormalises a product only then
        n = math.sqrt(_sqnorm(q))
        q = (q[0] / n, q[1] / n, q[2] / n, q[3] / n)
    rt = _rotate(a[:4], b[4:])
    return q + (a[4] + rt[0], a[5] + rt[1], a[6] + rt[2])


def fmt(x):
    return "%.17g" % x


def _floats(tok):
    return tuple(float(t) for t in tok)


# ---- the reading ---------------------------------------------------------------------------------------------
class Reading:
    """Interprets a script line by line (`feed`) and collects the dump (`out`).  `solver(batch) -> positions`
    stands for Point::optimize in a structure step; without one the step applies the positions the script gives."""

    def __init__(self, dedupe=True, solver=None):
        self.dedupe, self.solver = dedupe, solver
        self.frames, self.held, self.points, self.registered = {}, set(), {}, set()
        self.next_upgrade_id, self.next_stereo_id = FIRST_UPGRADE_ID, 0
        self.out, self.batches, self.stopped = [], [], False
        self.touched = set()      # the points a solver has moved: all others are where they were made

    # -- Point::addObservation / removeObservation (point.cpp:41-66)
    def add_observation(self, pid, fid, idx):
        obs = self.points[pid]["obs"]
        if self.dedupe:
            for o in obs:
                if o[0] == fid:
                    if o[1] != idx:
                        raise Conflict("frame %d: feature %d, then %d" % (fid, o[1], idx))
                    return
        obs.append((fid, idx))

    def remove_observation(self, pid, fid):
        p = self.points[pid]
        p["obs"] = [o for o in p["obs"] if o[0] != fid]

    # -- who is alive: the scene's own pointers, and the keyframes that seed references hold (points hold weak ones)
    def alive(self):
        seen, todo = set(), list(self.held)
        while todo:
            fid = todo.pop()
            if fid in seen:
                continue
            seen.add(fid)
            todo.extend(r[0] for r in self.frames[fid]["seedref"] if r is not None)
        return seen

    def new_point(self, pid, pos, stamp=0):
        assert pid not in self.points
        self.points[pid] = dict(id=pid, pos=tuple(pos), stamp=stamp, obs=[])

    # -- FrameHandlerBase::upgradeSeedsToFeatures (frame_handler_base.cpp:828-918)
    def upgrade(self, fid):
        fr = self.frames[fid]
        count, edgelets = 0, []
        for i in range(fr["n"]):
            if fr["landmark"][i] is not None:
                self.add_observation(fr["landmark"][i], fid, i)                  # :835-848, whatever the type
            elif fr["seedref"][i] is not None:
                kid, sid = fr["seedref"][i]
                kf = self.frames[kid]
                pid = kf["landmark"][sid]
                if pid is None:                                                  # :860-870
                    depth = 1.0 / kf["invmu"][sid]                               # seed.h:110-113, :145-149
                    f = kf["f"][sid]
                    pos = t_transform(t_inverse(kf["T"]), (f[0] * depth, f[1] * depth, f[2] * depth))
                    pid = self.next_upgrade_id
                    self.next_upgrade_id += 1
                    self.new_point(pid, pos)
                    kf["landmark"][sid] = pid
                    kf["track"][sid] = pid
                    self.add_observation(pid, kid, sid)
                fr["landmark"][i] = pid                                          # :873-875
                fr["track"][i] = pid
                self.add_observation(pid, fid, i)
                kt = kf["type"][sid]                                             # :876-902
                if kt in CORNER_TYPES:
                    kf["type"][sid] = fr["type"][i] = capi.FT_CORNER
                elif kt in MAPPOINT_TYPES:
                    kf["type"][sid] = fr["type"][i] = capi.FT_MAPPOINT
                elif kt in EDGELET_TYPES:
                    kf["type"][sid] = fr["type"][i] = capi.FT_EDGELET
                    edgelets.append(i)
                else:
                    raise ValueError("Seed-Type not known")
                count += 1
            fr["seedref"][i] = None                                              # :906-908: every feature
        return count, edgelets

    # -- StereoTriangulation::compute's loop over the match results (stereo_triangulation.cpp:95-137)
    def stereo(self, id0, id1, n_old, n_desired, indices, result, depth, f_cur):
        f0, f1 = self.frames[id0], self.frames[id1]
        T_world_cam0 = t_inverse(f0["T"])
        n_ok = n_failed = 0
        for i_ref in indices:
            k = i_ref - n_old
            if result[k] == capi.MATCH_SUCCESS:
                f, d = f0["f"][i_ref], depth[k]
                pid = self.next_stereo_id
                self.next_stereo_id += 1
                self.new_point(pid, t_transform(T_world_cam0, (f[0] * d, f[1] * d, f[2] * d)))
                f0["landmark"][i_ref] = pid
                f0["track"][i_ref] = pid
                self.add_observation(pid, id0, i_ref)
                i_cur = f1["n"]
                assert i_cur < f1["cap"]
                f1["type"][i_cur] = f0["type"][i_ref]
                f1["f"][i_cur] = f_cur[k]
                f1["landmark"][i_cur] = pid
                f1["track"][i_cur] = pid
                self.add_observation(pid, id1, i_cur)
                f1["n"] += 1
                n_ok += 1
            else:
                n_failed += 1
            if n_ok >= n_desired:
                break
        return n_ok, n_failed

    # -- initialization_utils::rescaleAndInitializePoints (initialization.cpp:800-840)
    def init_points(self, cur_id, ref_id, depth_at_cur, T_cur_ref, matches, points_in_cur):
        cur, ref = self.frames[cur_id], self.frames[ref_id]
        assert len(matches) > 1
        depths = sorted(math.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]) for p in points_in_cur)
        scale = depth_at_cur / depths[len(depths) // 2]                          # vk::getMedian: the upper median
        T = t_mul(T_cur_ref, ref["T"])
        pos_ref, pos_cur = t_inverse(ref["T"])[4:], t_inverse(T)[4:]
        p = tuple(pos_ref[c] + scale * (pos_cur[c] - pos_ref[c]) for c in range(3))
        rp = _rotate(T[:4], p)
        T = T[:4] + (-rp[0], -rp[1], -rp[2])
        cur["T"] = T
        T_world_cur = t_inverse(T)
        for (ic, ir), x in zip(matches, points_in_cur):
            assert cur["track"][ic] == ref["track"][ir]
            pid = cur["track"][ic]
            self.new_point(pid, t_transform(T_world_cur, (x[0] * scale, x[1] * scale, x[2] * scale)))
            cur["landmark"][ic] = pid
            ref["landmark"][ir] = pid
            self.add_observation(pid, ref_id, ir)
            self.add_observation(pid, cur_id, ic)
        return scale

    # -- FrameHandlerBase::optimizeStructure's candidates of one frame (frame_handler_base.cpp:797-814) and what
    #    Point::optimize is given: the observations whose frame is still alive (point.cpp:262-275)
    def gather(self, fid, max_n_pts):
        fr = self.frames[fid]
        pts = [fr["landmark"][i] for i in range(fr["n"]) if fr["landmark"][i] is not None and fr["type"][i] not in EDGELET_TYPES]
        if max_n_pts > 0:
            max_n_pts = min(max_n_pts, len(pts))     # and a partition that the loop over the whole container ignores (:815)
        alive = self.alive()
        view_ids, views, obs_begin, obs_view, obs_f, pos = [], [], [0], [], [], []
        for pid in pts:
            pos.append(self.points[pid]["pos"])
            for ofid, idx in self.points[pid]["obs"]:
                if ofid not in alive:
                    continue
                if ofid not in view_ids:
                    view_ids.append(ofid)
                    views.append(self.frames[ofid]["T"])
                obs_view.append(view_ids.index(ofid))
                obs_f.append(self.frames[ofid]["f"][idx])
            obs_begin.append(len(obs_view))
        return max_n_pts, dict(frame=fid, stamps={p: self.points[p]["stamp"] for p in pts}, pts=pts, views=views, obs_begin=obs_begin, obs_view=obs_view, obs_f=obs_f, pos=pos)

    def structure(self, max_n_pts, bundle, scripted):
        if max_n_pts == 0:                                                       # :785-786
            self.out.append("structure 0")
            return
        n_total = 0
        for k, fid in enumerate(bundle):
            max_in = max_n_pts
            max_n_pts, b = self.gather(fid, max_n_pts)
            b["max_in"] = max_in
            self.batches.append(b)
            if not self.solver:
                self.out.append("step %d %d %d %d %d %d" % (fid, max_in, max_n_pts, len(b["pts"]), len(b["views"]), len(b["obs_view"])))
                if b["pts"]:
                    self.out.append("pts " + " ".join(str(p) for p in b["pts"]))
                    self.out.append("views " + " ".join(fmt(x) for T in b["views"] for x in T))
                    self.out.append("obs_begin " + " ".join(str(x) for x in b["obs_begin"]))
                    self.out.append("obs_view " + " ".join(str(x) for x in b["obs_view"]))
                    self.out.append("obs_f " + " ".join(fmt(x) for f in b["obs_f"] for x in f))
                    self.out.append("pos " + " ".join(fmt(x) for p in b["pos"] for x in p))
            if not b["pts"]:
                continue
            if self.solver:      # Point::optimize returns at once with fewer than two observations (point.cpp:255-259)
                n_obs = np.diff(b["obs_begin"])
                new_pos = [tuple(float(x) for x in p) if n >= 2 else old for p, n, old in zip(self.solver(b), n_obs, b["pos"])]
                self.touched.update(pid for pid, n in zip(b["pts"], n_obs) if n >= 2)
            else:
                new_pos = [scripted.get((k, pid), p) for pid, p in zip(b["pts"], b["pos"])]
            for pid, p in zip(b["pts"], new_pos):                                # :815-819
                self.points[pid]["pos"] = p
                self.points[pid]["stamp"] = fid
            n_total += len(b["pts"])
        self.out.append("structure %d" % n_total)

    def state(self):
        alive = self.alive()
        shown = set(self.registered)
        for fid in alive:
            fr = self.frames[fid]
            shown.update(p for p in fr["landmark"][:fr["n"]] if p is not None)
        self.out.append("state")
        for pid in sorted(shown):
            p = self.points[pid]
            live = [o for o in p["obs"] if o[0] in alive]
            self.out.append("point %d %s %d %d%s" % (pid, " ".join(fmt(x) for x in p["pos"]), p["stamp"], len(live),
                                                     "".join(" %d %d" % o for o in live)))
        for fid in sorted(self.held):
            fr = self.frames[fid]
            n = fr["n"]
            self.out.append("frame %d %d" % (fid, n))
            self.out.append("types " + " ".join(str(t) for t in fr["type"][:n]))
            self.out.append("tracks " + " ".join(str(t) for t in fr["track"][:n]))
            self.out.append("seedrefs " + " ".join("%d %d" % (r if r is not None else (-1, -1)) for r in fr["seedref"][:n]))
        self.out.append("alive " + " ".join("%d %d" % (fid, fid in alive) for fid in sorted(self.frames)))

    # -- one line of a script
    def feed(self, line):
        tok = line.split()
        if not tok or self.stopped:
            return
        ev, a = tok[0], tok[1:]
        try:
            if ev == "frame":            # frame <id> <n> <capacity> <T_f_w: qw qx qy qz tx ty tz>
                fid, n, cap = int(a[0]), int(a[1]), int(a[2])
                self.frames[fid] = dict(id=fid, T=_floats(a[3:10]), n=n, cap=cap, type=[capi.FT_OUTLIER] * cap, f=[(0.0, 0.0, 0.0)] * cap,
                                        invmu=[0.0] * cap, landmark=[None] * cap, track=[-1] * cap, seedref=[None] * cap)
                self.held.add(fid)
            elif ev == "grow":           # grow <id> <n>: more features (the detector's, before a triangulation)
                fr = self.frames[int(a[0])]
                assert fr["n"] <= int(a[1]) <= fr["cap"]
                fr["n"] = int(a[1])
            elif ev == "feat":           # feat <frame> <i> <type> <f: 3> <inverse depth>
                fr, i = self.frames[int(a[0])], int(a[1])
                fr["type"][i], fr["f"][i], fr["invmu"][i] = int(a[2]), _floats(a[3:6]), float(a[6])
            elif ev == "seedref":        # seedref <frame> <i> <keyframe> <seed>
                self.frames[int(a[0])]["seedref"][int(a[1])] = (int(a[2]), int(a[3]))
            elif ev == "track":          # track <frame> <i> <track id>
                self.frames[int(a[0])]["track"][int(a[1])] = int(a[2])
            elif ev == "point":          # point <id> <x y z> <last_structure_optim_>
                self.new_point(int(a[0]), _floats(a[1:4]), int(a[4]))
                self.registered.add(int(a[0]))
            elif ev == "landmark":       # landmark <frame> <i> <point>: the feature carries the landmark (no observation yet)
                self.frames[int(a[0])]["landmark"][int(a[1])] = int(a[2])
            elif ev == "obs":            # obs <point> <frame> <i>: Point::addObservation
                self.add_observation(int(a[0]), int(a[1]), int(a[2]))
            elif ev == "upgrade":        # upgrade <frame>
                count, edgelets = self.upgrade(int(a[0]))
                self.out.append("upgraded %d %d %d%s" % (int(a[0]), count, len(edgelets), "".join(" %d" % e for e in edgelets)))
            elif ev == "stereo":         # stereo <f0> <f1> <n_old> <n_new> <n_desired> <indices> <results> <depths> <f_cur: 3 each>
                id0, id1, n_old, n_new, n_desired = (int(x) for x in a[:5])
                r = a[5:]
                indices, result = [int(x) for x in r[:n_new]], [int(x) for x in r[n_new:2 * n_new]]
                depth, fc = _floats(r[2 * n_new:3 * n_new]), _floats(r[3 * n_new:6 * n_new])
                assert self.frames[id0]["n"] == n_old + n_new
                n_ok, n_failed = self.stereo(id0, id1, n_old, n_desired, indices, result, depth, [fc[3 * k:3 * k + 3] for k in range(n_new)])
                self.out.append("stereo %d %d %d" % (n_ok, n_failed, self.frames[id1]["n"]))
            elif ev == "init":           # init <cur> <ref> <depth> <T_cur_ref: 7> <m> then m times <i_cur> <i_ref> <x y z in cur>
                m = int(a[10])
                r = a[11:]
                matches = [(int(r[5 * k]), int(r[5 * k + 1])) for k in range(m)]
                pts = [_floats(r[5 * k + 2:5 * k + 5]) for k in range(m)]
                scale = self.init_points(int(a[0]), int(a[1]), float(a[2]), _floats(a[3:10]), matches, pts)
                self.out.append("init %s %s" % (fmt(scale), " ".join(fmt(x) for x in self.frames[int(a[0])]["T"])))
            elif ev == "remove":         # remove <frame>: its observations leave its landmarks (Map::removeKeyframe)
                fr = self.frames[int(a[0])]
                for i in range(fr["n"]):
                    if fr["landmark"][i] is not None:
                        self.remove_observation(fr["landmark"][i], fr["id"])
            elif ev == "clearrefs":      # clearrefs <frame>: the keyframe window lets go of the frame's seed references
                fr = self.frames[int(a[0])]
                fr["seedref"] = [None] * fr["cap"]
            elif ev == "drop":           # drop <frame>: the scene's own pointer goes
                self.held.discard(int(a[0]))
            elif ev == "structure":      # structure <max_n_pts> <n frames> <frames> <k> then k times <frame's place> <point> <x y z>
                nf = int(a[1])
                bundle = [int(x) for x in a[2:2 + nf]]
                r = a[3 + nf:]
                scripted = {(int(r[5 * k]), int(r[5 * k + 1])): _floats(r[5 * k + 2:5 * k + 5]) for k in range(int(a[2 + nf]))}
                self.structure(int(a[0]), bundle, scripted)
            elif ev == "state":
                self.state()
            else:
                raise ValueError("unknown event " + ev)
        except Conflict:
            self.out.append("throw " + " ".join(tok[:2]))
            self.stopped = True

    def finish(self):
        self.state()
        return "\n".join(self.out) + "\n"


def read_script(text, dedupe=True, solver=None):
    """The reading's dump of a script, and the Reading (for its batches and points)."""
    r = Reading(dedupe=dedupe, solver=solver)
    for line in text.splitlines():
        r.feed(line)
    return r.finish(), r


# ---- comparing two dumps ----------------------------------------------------------------------------------------
def _blocks(text):
    """A dump as a list of blocks: a `step` line with its six arrays is one block, every other line its own."""
    out, lines, i = [], text.splitlines(), 0
    while i < len(lines):
        t = lines[i].split()
        if t[0] == "step" and int(t[4]) > 0:
            out.append(lines[i:i + 7])
            i += 7
        else:
            out.append([lines[i]])
            i += 1
    return out


def _canonical_step(block, stamps):
    """A step whose candidates std::nth_element reordered: per point (sorted by id) its position and its observations
    as (view pose, bearing vector) in order; and that the first max_out candidates are not younger than the rest."""
    head = block[0].split()
    max_out, n = int(head[3]), int(head[4])
    arr = {b.split()[0]: b.split()[1:] for b in block[1:]}
    pts = [int(x) for x in arr["pts"]]
    ob, ov = [int(x) for x in arr["obs_begin"]], [int(x) for x in arr["obs_view"]]
    rec = []
    for k in range(n):
        obs = [(tuple(arr["views"][7 * ov[o]:7 * ov[o] + 7]), tuple(arr["obs_f"][3 * o:3 * o + 3])) for o in range(ob[k], ob[k + 1])]
        rec.append((pts[k], tuple(arr["pos"][3 * k:3 * k + 3]), tuple(obs)))
    if stamps is not None and 0 < max_out < n:
        assert max(stamps[p] for p in pts[:max_out]) <= min(stamps[p] for p in pts[max_out:]), "not partitioned by last_structure_optim_"
    return head, sorted(rec)


def assert_same_dump(got, want, batches=None):
    """`got` (the tool's) equals `want` (the reading's) line for line; a step in which max_n_pts is positive and below
    the number of candidates is compared point by point, since the order std::nth_element leaves is the library's
    (`batches`: the reading's, for the stamps that order has to respect)."""
    bg, bw = _blocks(got), _blocks(want)
    n_step = 0
    for k, (g, w) in enumerate(zip(bg, bw)):
        head = w[0].split()
        if len(w) == 7 and 0 < int(head[2]) < int(head[4]):
            stamps = batches[n_step]["stamps"] if batches else None
            assert _canonical_step(g, stamps) == _canonical_step(w, None), "block %d: %s" % (k, w[0])
        else:
            assert g == w, "block %d:\n  tool    %s\n  reading %s" % (k, next((a for a, b in zip(g, w) if a != b), g[-1])[:300],
                                                                       next((b for a, b in zip(g, w) if a != b), w[-1])[:300])
        n_step += head[0] == "step"
    assert len(bg) == len(bw), "tool wrote %d blocks, the reading %d" % (len(bg), len(bw))


# ---- scenarios -------------------------------------------------------------------------------------------------
class _Builder:
    """Writes a script and runs the reading beside it, so that a later event can be made from the state so far."""

    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)
        self.lines, self.reading = [], Reading()

    def ev(self, *tok):
        line = " ".join(fmt(t) if isinstance(t, float) else str(t) for t in tok)
        self.lines.append(line)
        self.reading.feed(line)

    def pose(self, centre=(0.0, 0.0, 0.0)):
        """A view as pose_helpers.make_structure_scene makes them: a small rotation, a camera centre within 0.6 m."""
        rng = self.rng
        T_w_f = synth.SE3(synth.quat_from_axis_angle(rng.normal(size=3), rng.uniform(0, 0.25)), rng.uniform(-0.6, 0.6, 3) + np.asarray(centre))
        return tuple(float(x) for x in T_w_f.inverse().as7())

    def cloud(self, n):
        rng = self.rng
        return np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3, 9, n)], 1)

    def bearing(self, T, p, noise=2e-3):
        """(bearing vector with noise, true distance) of world point p in the frame with pose T."""
        q = np.array(t_transform(T, tuple(float(x) for x in p)))
        d = float(np.linalg.norm(q))
        f = q / d + self.rng.normal(0, noise, 3)
        f /= np.linalg.norm(f)
        return tuple(float(x) for x in f), d

    def frame(self, fid, T, n, cap=None):
        self.ev("frame", fid, n, cap if cap is not None else n, *T)

    def feat(self, fid, i, typ, f, invmu=0.0):
        self.ev("feat", fid, i, typ, *f, float(invmu))

    def seed(self, fid, i, typ, p, err=0.08):
        """Feature i of keyframe fid is a seed on world point p, its depth off by err (relative)."""
        f, d = self.bearing(self.reading.frames[fid]["T"], p)
        self.feat(fid, i, typ, f, 1.0 / (d * (1.0 + self.rng.normal(0, err))))

    def observe(self, fid, i, typ, p):
        f, _ = self.bearing(self.reading.frames[fid]["T"], p)
        self.feat(fid, i, typ, f)

    def structure(self, max_n_pts, bundle, gt):
        """A structure step.  The positions it applies stand for the optimiser's: the true point with a small error, per
        frame of the bundle and candidate (`gt`: point id -> true position)."""
        entries = []
        if max_n_pts != 0:
            m = max_n_pts
            for k, fid in enumerate(bundle):
                m, b = self.reading.gather(fid, m)
                for pid in dict.fromkeys(b["pts"]):
                    n_live = b["obs_begin"][b["pts"].index(pid) + 1] - b["obs_begin"][b["pts"].index(pid)]
                    if n_live >= 2 and pid in gt:      # Point::optimize leaves a point with fewer than two observations alone
                        entries += [k, pid] + [float(x) for x in np.asarray(gt[pid]) + self.rng.normal(0, 0.01, 3)]
        self.ev("structure", max_n_pts, len(bundle), *bundle, len(entries) // 5, *entries)

    def text(self):
        return "\n".join(self.lines) + "\n"


SEED_TYPES = (capi.FT_CORNER_SEED, capi.FT_CORNER_SEED_CONVERGED, capi.FT_EDGELET_SEED, capi.FT_EDGELET_SEED_CONVERGED,
              capi.FT_MAPPOINT_SEED, capi.FT_MAPPOINT_SEED_CONVERGED)


def _gt_of(b, frames_points):
    """point id -> true world position, from (frame, feature) -> world point, for every landmark the frames carry."""
    gt = {}
    for fid, world in frames_points.items():
        fr = b.reading.frames.get(fid)
        if fr is None:
            continue
        for i, p in world.items():
            if i < fr["n"] and fr["landmark"][i] is not None:
                gt[fr["landmark"][i]] = p
    return gt


def mono_keyframes(seed=101):
    """a. A keyframe with corner, edgelet and map-point seeds, converged and not; a later frame upgrades some of them; a third
    frame observes the resulting landmarks, upgrades more and becomes a keyframe; the first keyframe leaves the map."""
    b = _Builder(seed)
    n0 = 30
    P = b.cloud(n0)
    b.frame(10, b.pose(), n0)
    for i in range(n0):
        b.seed(10, i, SEED_TYPES[i % 6], P[i])
    world = {10: {i: P[i] for i in range(n0)}, 11: {}, 12: {}}
    # frame 11: 18 features on seeds of 10 (every type), 3 on nothing
    b.frame(11, b.pose(), 21)
    on = list(b.rng.permutation(n0)[:18])
    for i, s in enumerate(on):
        b.observe(11, i, capi.FT_CORNER_SEED, P[s])
        b.ev("seedref", 11, i, 10, int(s))
        world[11][i] = P[s]
    for i in range(18, 21):
        b.feat(11, i, capi.FT_CORNER_SEED, (0.0, 0.0, 1.0))
    b.ev("upgrade", 11)
    b.structure(-1, [11], _gt_of(b, world))
    b.ev("state")
    # frame 12: 14 features on landmarks that frame 11 made (the reprojector's matches), 6 on further seeds of 10, 2 on nothing
    b.frame(12, b.pose(), 22)
    for i, s in enumerate(on[:14]):
        pid = b.reading.frames[10]["landmark"][s]
        b.observe(12, i, b.reading.frames[10]["type"][s], P[s])
        b.ev("landmark", 12, i, pid)
        b.ev("track", 12, i, pid)
        world[12][i] = P[s]
    rest = [s for s in range(n0) if s not in on][:6]
    for i, s in enumerate(rest, 14):
        b.observe(12, i, capi.FT_CORNER_SEED, P[s])
        b.ev("seedref", 12, i, 10, int(s))
        world[12][i] = P[s]
    for i in range(20, 22):
        b.feat(12, i, capi.FT_CORNER_SEED, (0.0, 0.0, 1.0))
    b.ev("upgrade", 12)
    b.structure(-1, [12], _gt_of(b, world))
    b.ev("state")
    # the first keyframe leaves the map (the harnesses' keyframe window: references, observations, the pointer)
    b.ev("clearrefs", 10)
    b.ev("remove", 10)
    b.ev("drop", 10)
    b.structure(-1, [12], _gt_of(b, world))
    return b.text()


def stereo_keyframe_step(seed=203):
    """b. A stereo keyframe step in the harnesses' order -- the frame that is not the keyframe through upgradeSeedsToFeatures,
    the triangulation's loop with successes, failures and the n_desired cut-off, the keyframe through upgradeSeedsToFeatures --
    a structure step over the bundle, then the same keyframe step again with a few more new features."""
    b = _Builder(seed)
    n_seed, n_old, n_new, n_new2, n_r = 10, 8, 30, 6, 6
    S, N = b.cloud(n_seed), b.cloud(n_new + n_new2)
    b.frame(20, b.pose(), n_seed)
    for i in range(n_seed):
        b.seed(20, i, SEED_TYPES[i % 6], S[i])
    n_desired = 20
    T_l = b.pose()
    T_r = b.pose(centre=np.array(t_inverse(T_l)[4:]))       # the right camera: a baseline within 0.6 m of the left one
    b.frame(22, T_l, n_old + n_new, n_old + n_new + n_new2)
    b.frame(23, T_r, n_r, n_r + n_desired + n_new2)
    world = {20: {i: S[i] for i in range(n_seed)}, 22: {}, 23: {}}
    for i in range(n_old):                                   # the left frame hangs on seeds 0..7, the right one on 4..9
        b.observe(22, i, capi.FT_CORNER_SEED, S[i])
        b.ev("seedref", 22, i, 20, i)
        world[22][i] = S[i]
    for i in range(n_r):
        b.observe(23, i, capi.FT_CORNER_SEED, S[4 + i])
        b.ev("seedref", 23, i, 20, 4 + i)
        world[23][i] = S[4 + i]

    def key_step(first, count, want):
        rng = b.rng
        for k in range(count):                               # the detector's new features of the left frame
            typ = capi.FT_CORNER if k % 4 else capi.FT_EDGELET
            b.observe(22, first + k, typ, N[first - n_old + k])
            world[22][first + k] = N[first - n_old + k]
        b.ev("upgrade", 23)
        indices = [first + int(k) for k in rng.permutation(count)]
        result = [0 if rng.uniform() < 0.8 else int(rng.randint(1, 4)) for _ in range(count)]
        depth, f_cur = [], []
        i_cur = b.reading.frames[23]["n"]
        n_ok = 0
        reached = set()
        for i_ref in indices:
            n_ok += result[i_ref - first] == 0
            reached.add(i_ref)
            if n_ok >= want:
                break
        if count > want:      # the first step shows the cut-off, and failures before it
            assert len(reached) < count and any(result[i - first] for i in reached), "choose another seed"
        for k in range(count):
            p = N[first - n_old + k]
            f, _ = b.bearing(T_r, p)
            _, d = b.bearing(T_l, p, noise=0.0)
            depth.append(d * (1.0 + rng.normal(0, 0.08)))
            f_cur += list(f)
        for i_ref in indices:                                # where the right frame's new features will sit
            if i_ref in reached and result[i_ref - first] == 0:
                world[23][i_cur] = N[i_ref - n_old]
                i_cur += 1
        b.ev("stereo", 22, 23, first, count, want, *indices, *result, *depth, *f_cur)
        b.ev("upgrade", 22)

    key_step(n_old, n_new, n_desired)
    b.structure(-1, [22, 23], _gt_of(b, world))
    b.ev("state")
    b.ev("grow", 22, n_old + n_new + n_new2)
    key_step(n_old + n_new, n_new2, n_new2)
    b.structure(-1, [22, 23], _gt_of(b, world))
    return b.text()


def bootstrap(seed=303):
    """c. The initialiser's points on two frames, then both frames through upgradeSeedsToFeatures; a third frame observes most of
    the landmarks, becomes a keyframe and gets a structure step; the second frame is a keyframe once more and gets one.
    (No structure step on the bare pair: with every observation there twice the normal equations are the same ones times two,
    which is exact in binary floating point, so that step could not tell the duplicates from their absence.)"""
    b = _Builder(seed)
    n, m, n3 = 20, 16, 12
    P = b.cloud(n)
    T_ref, T_cur = b.pose(), b.pose()
    b.frame(30, T_ref, n)
    b.frame(31, T_cur, n)
    world = {30: {}, 31: {}, 32: {}}
    for i in range(n):
        b.observe(30, i, capi.FT_CORNER, P[i])
        b.observe(31, (i + 3) % n, capi.FT_CORNER, P[i])
        b.ev("track", 30, i, 100 + i)
        b.ev("track", 31, (i + 3) % n, 100 + i)
        world[30][i], world[31][(i + 3) % n] = P[i], P[i]
    T_cur_ref = t_mul(T_cur, t_inverse(T_ref))
    T_cur_ref = T_cur_ref[:4] + tuple(0.37 * x for x in T_cur_ref[4:])     # the relative pose's translation is known up to scale
    sel = sorted(int(x) for x in b.rng.permutation(n)[:m])
    rows = []
    for i in sel:
        x = np.array(t_transform(T_cur, tuple(float(v) for v in P[i]))) * 0.37 * (1.0 + b.rng.normal(0, 0.03))
        rows += [(i + 3) % n, i] + [float(v) for v in x]
    depth = sorted(float(np.linalg.norm(t_transform(T_cur, tuple(float(v) for v in P[i])))) for i in sel)[m // 2]
    b.ev("init", 31, 30, depth, *T_cur_ref, m, *rows)
    b.ev("upgrade", 30)
    b.ev("upgrade", 31)
    b.ev("state")
    b.frame(32, b.pose(), n3 + 1)
    for k, i in enumerate(sel[:n3]):
        b.observe(32, k, capi.FT_CORNER, P[i])
        b.ev("landmark", 32, k, 100 + i)
        b.ev("track", 32, k, 100 + i)
        world[32][k] = P[i]
    b.feat(32, n3, capi.FT_CORNER_SEED, (0.0, 0.0, 1.0))
    b.ev("upgrade", 32)
    b.structure(-1, [32], _gt_of(b, world))
    b.ev("state")
    b.ev("upgrade", 31)       # a later keyframe step finds the same observations
    b.structure(-1, [31], _gt_of(b, world))
    return b.text()


def multi_camera_bundle(seed=404):
    """d. Seeds reached through both frames of a bundle: one point, three observations; others through one frame only."""
    b = _Builder(seed)
    n = 12
    P = b.cloud(n)
    b.frame(40, b.pose(), n)
    for i in range(n):
        b.seed(40, i, SEED_TYPES[i % 6], P[i])
    world = {40: {i: P[i] for i in range(n)}, 41: {}, 42: {}}
    for fid, seeds in ((41, [0, 1, 2, 3, 4, 5, 6, 7]), (42, [7, 6, 5, 4, 8, 9])):
        b.frame(fid, b.pose(), len(seeds) + 1)
        for i, s in enumerate(seeds):
            b.observe(fid, i, capi.FT_CORNER_SEED, P[s])
            b.ev("seedref", fid, i, 40, s)
            world[fid][i] = P[s]
        b.feat(fid, len(seeds), capi.FT_CORNER_SEED, (0.0, 0.0, 1.0))
    b.ev("upgrade", 41)
    b.ev("upgrade", 42)
    b.structure(-1, [41, 42], _gt_of(b, world))
    return b.text()


def stale_seed_reference(seed=505):
    """e. Features that carry a landmark and a left-over seed reference: the reference goes (frame_handler_base.cpp:906-908),
    and once the scene lets go of the old keyframe nothing holds it."""
    b = _Builder(seed)
    n = 8
    P = b.cloud(n)
    b.frame(50, b.pose(), n)
    for i in range(n):
        b.seed(50, i, SEED_TYPES[i % 6], P[i])
    b.frame(51, b.pose(), 7)
    for i in range(3):                                       # seeds 0..2 become landmarks through this frame
        b.observe(51, i, capi.FT_CORNER_SEED, P[i])
        b.ev("seedref", 51, i, 50, i)
    for i in range(3, 6):                                    # landmarks of their own, and references to seeds 3..5 left over
        b.ev("point", 900 + i, *[float(x) for x in P[i]], 0)
        b.observe(51, i, capi.FT_CORNER, P[i])
        b.ev("landmark", 51, i, 900 + i)
        b.ev("seedref", 51, i, 50, i)
    b.feat(51, 6, capi.FT_CORNER_SEED, (0.0, 0.0, 1.0))
    b.ev("upgrade", 51)
    b.ev("state")
    b.ev("drop", 50)
    return b.text()


def index_conflict(seed=606):
    """f. Two features of one frame reach one seed: the reference's CHECK_EQ fails at the second."""
    b = _Builder(seed)
    n = 4
    P = b.cloud(n)
    b.frame(70, b.pose(), n)
    for i in range(n):
        b.seed(70, i, SEED_TYPES[i % 6], P[i])
    b.frame(71, b.pose(), 5)
    for i, s in enumerate([0, 1, 2, 1, 3]):
        b.observe(71, i, capi.FT_CORNER_SEED, P[s])
        b.ev("seedref", 71, i, 70, s)
    b.ev("upgrade", 71)
    b.ev("state")             # not reached
    return b.text()


def selection(seed=707):
    """g. optimizeStructure's candidates over a two-frame bundle: max_n_pts of 0, of a value below and of one above the number
    of candidates (carried from the first frame to the second) and of -1, landmarks with differing last_structure_optim_, edgelets, a landmark
    with one observation, one that both frames carry."""
    b = _Builder(seed)
    n = 14
    P = b.cloud(n)
    T = {fid: b.pose() for fid in (60, 61, 62)}
    counts = {60: n, 61: 9, 62: 8}
    for fid in (60, 61, 62):
        b.frame(fid, T[fid], counts[fid])
    gt = {}
    for i in range(n):
        pid = 800 + i
        gt[pid] = P[i]
        start = P[i] * (1.0 + b.rng.normal(0, 0.08)) + b.rng.normal(0, 0.02, 3)
        b.ev("point", pid, *[float(x) for x in start], int(b.rng.randint(1, 40)))
        typ = capi.FT_EDGELET if i % 5 == 4 else (capi.FT_MAPPOINT if i % 5 == 3 else capi.FT_CORNER)
        b.observe(60, i, typ, P[i])
        b.ev("landmark", 60, i, pid)
        b.ev("obs", pid, 60, i)
    for i in range(9):        # frame 61 carries landmarks 0..8 (0 is the one with no further view), frame 62 landmarks 6..13
        typ = b.reading.frames[60]["type"][i]
        b.observe(61, i, typ, P[i])
        b.ev("landmark", 61, i, 800 + i)
        if i > 0:
            b.ev("obs", 800 + i, 61, i)
    for i in range(8):
        typ = b.reading.frames[60]["type"][6 + i]
        b.observe(62, i, typ, P[6 + i])
        b.ev("landmark", 62, i, 806 + i)
        b.ev("obs", 806 + i, 62, i)
    b.structure(0, [61, 62], gt)
    b.ev("state")
    b.structure(4, [61, 62], gt)
    b.ev("state")
    b.structure(10, [61, 62], gt)      # above the first frame's candidates: the second frame is handed their number, not 10
    b.ev("state")
    b.structure(-1, [62, 61], gt)
    return b.text()


SCENARIOS = dict(a_mono_keyframes=mono_keyframes, b_stereo_keyframe_step=stereo_keyframe_step, c_bootstrap=bootstrap,
                 d_multi_camera_bundle=multi_camera_bundle, e_stale_seed_reference=stale_seed_reference,
                 f_index_conflict=index_conflict, g_selection=selection)
