"""Every kernel that reads an image, against the oracle, at image sizes whose pyramid levels truncate (tests/odd_sizes.py:
A = 413x309, B = 375x247, C = 501x397): odd row lengths, levels of floor(floor(w / 2) / 2) ... pixels, byte counts that are
no multiple of 16.  The bars are those of the family each test belongs to (tests/test_pyramid_gpu.py,
tests/test_sparse_align_gpu.py, tests/test_boundaries_gpu.py, tests/test_klt_matcher_gpu.py); the premises -- that the
oracle is right at these sizes, and what the crafted pixels do on it -- are in tests/test_odd_sizes_cpu.py.

The alignment kernel decides per problem which levels' images are resident in LDS from the problem's start, which are
staged alone when their turn comes and which are read from global memory (sparse_align.hip).  The alignment tests here KNOW
which way each level went: they ask svoh_sparse_align_last_launch_lds for the image budget of the launch, restate the
kernel's rule (level_paths) and assert that each of the three ways handled a level of truncated size with a 16-byte tail.
With 5 levels, 4..0 (bytes of one camera's reference + current image, each rounded up to 16):
    A  960, 3 904, 15 872,  63 456, 255 264      B  704, 2 784, 11 360, 46 016, 185 280      C (8x8 patches) level 1: 99 008
  * the 256-thread builds (batch, one wave per SIMD; about 51 KB): A and B keep 4..2 resident, B stages level 1 alone, A reads
    level 1 from global memory -- B is the size that reaches "staged alone" there;
  * the 512-thread builds (78 KB, less a small problem's workspace rows): A stages level 1 alone (B keeps it resident), the
    A + B rig (109 472 bytes) and C read level 1 from global memory.
No further size was needed."""
import ctypes as C
import os

import numpy as np
import pytest

from svo_pro_universal_amd import _capi as capi, frontend as fe, synth

import helpers
import np_restatement_direct as nd
import odd_sizes as od
import test_sparse_align_gpu as sa
from test_klt_matcher_gpu import views
from test_sparse_align_batch_build_gpu import assert_batch_build

pytestmark = pytest.mark.gpu

ROUNDINGS = [capi.SVOH_HALFSAMPLE_REFERENCE, capi.SVOH_HALFSAMPLE_SCALAR]


# ---------------------------------------------------------------------------------------------------------------------
# pyramid
# ---------------------------------------------------------------------------------------------------------------------
def _image(name, k=0):
    w, h = od.SIZES[name]
    rng = np.random.RandomState(w * 7 + h + k)
    img = rng.randint(0, 256, (h, w)).astype(np.uint8)
    img[: h // 3] = np.where(rng.uniform(size=(h // 3, w)) < 0.5, 255, 254)     # sums on the rounding edges
    return img


def _check_frame(ctx, frame, want):
    for l, lv in enumerate(want):
        got = ctx.download_level(frame, l)
        assert got.shape == lv.shape and np.array_equal(got, lv), "level %d differs" % l
    ctx.release_frame(frame)


@pytest.mark.parametrize("rounding", ROUNDINGS)
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_pyramid_bit_exact(gpu_ctx, oracle_lib, name, rounding):
    img = _image(name)
    want = oracle_lib.create_img_pyramid(img, od.N_LEVELS, rounding)
    assert [(a.shape[1], a.shape[0]) for a in want] == od.level_sizes(*od.SIZES[name])
    fr, got = gpu_ctx.build_pyramid(img, od.N_LEVELS, rounding, return_levels=True)
    for a, b in zip(got, want):
        assert a.shape == b.shape and np.array_equal(a, b)
    _check_frame(gpu_ctx, fr, want)


def _place(dst_addr, img, pitch):
    """img's rows at dst_addr, pitch bytes apart"""
    h, w = img.shape
    for y in range(h):
        C.memmove(dst_addr + y * pitch, img[y].ctypes.data, w)


def _pitched_block(imgs, pitch, stride):
    """one pageable buffer of noise with image i at an ODD address + i * stride; returns (buffer, address of image 0)"""
    h, w = imgs[0].shape
    buf = np.random.RandomState(99).randint(0, 256, stride * len(imgs) + 64).astype(np.uint8)
    first = buf.ctypes.data + 1 + (buf.ctypes.data % 2)          # odd
    assert first % 2 == 1 and (len(imgs) - 1) * stride + (h - 1) * pitch + w <= buf.size - 2
    for i, im in enumerate(imgs):
        _place(first + i * stride, im, pitch)
    return buf, first


@pytest.mark.parametrize("rounding", ROUNDINGS)
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_pyramid_entries_with_a_pitch(gpu_ctx, oracle_lib, name, rounding):
    """svoh_build_pyramid, _batch and _multi given level 0 with pitch = width + 11 from an odd address (frontend.build_pyramid
    makes its input contiguous first, so only these direct calls pass a pitch): every level bit-equal to the oracle's pyramid
    of the contiguous copy.  _multi from pageable memory (one 2-D copy per image) and from page-locked memory, where
    gather_images_kernel takes its slow arm for a pitch and for a source that is not 16-byte aligned -- and its fast arm's
    byte tail for a tight, aligned image whose size is no multiple of 16."""
    ctx, lib = gpu_ctx, gpu_ctx.lib
    w, h = od.SIZES[name]
    imgs = [_image(name, k) for k in range(3)]
    want = [oracle_lib.create_img_pyramid(im, od.N_LEVELS, rounding) for im in imgs]
    pitch = w + 11
    stride = h * pitch + 7
    if stride % 16 == 0:
        stride += 2
    assert stride % 16 != 0 and (w * h) % 16 != 0
    buf, first = _pitched_block(imgs, pitch, stride)
    # one image
    out = capi.svoh_frame_t()
    lv = [np.zeros((lh, lw), np.uint8) for lw, lh in od.level_sizes(w, h)]
    host = (C.c_void_p * od.N_LEVELS)(*[a.ctypes.data for a in lv])
    ctx._check(lib.svoh_build_pyramid(ctx.h, C.c_void_p(first), w, h, pitch, capi.SVOH_MEM_HOST, od.N_LEVELS, rounding, host, C.byref(out)))
    for a, b in zip(lv, want[0]):
        assert np.array_equal(a, b)
    _check_frame(ctx, out.value, want[0])
    # three images, image_stride no multiple of 16
    outs = (capi.svoh_frame_t * 3)()
    ctx._check(lib.svoh_build_pyramid_batch(ctx.h, C.c_void_p(first), C.c_size_t(stride), 3, w, h, pitch, capi.SVOH_MEM_HOST, od.N_LEVELS,
                                            rounding, outs))
    for i in range(3):
        _check_frame(ctx, outs[i], want[i])
    # images at separate addresses, pageable
    ptrs = (C.c_void_p * 3)(*[first + i * stride for i in range(3)])
    outs = (capi.svoh_frame_t * 3)()
    ctx._check(lib.svoh_build_pyramid_multi(ctx.h, ptrs, 3, w, h, pitch, capi.SVOH_MEM_HOST, od.N_LEVELS, rounding, outs))
    for i in range(3):
        _check_frame(ctx, outs[i], want[i])
    # ... and page-locked: (pitch, first address) = pitched from odd addresses / tight from odd addresses / tight and aligned
    block = C.c_void_p()
    span = h * pitch + 64
    span += span % 2                  # even: every image of a layout starts at an address of the first one's parity
    ctx._check(lib.svoh_host_alloc(ctx.h, C.c_size_t(3 * span + 64), C.byref(block)))
    try:
        assert block.value % 16 == 0
        for p, lead in ((pitch, 1), (w, 1), (w, 0)):
            if lead == 0:
                span16 = (span + 15) & ~15
                addrs = [block.value + i * span16 for i in range(3)]
                assert all(a % 16 == 0 for a in addrs) and addrs[2] + h * p <= block.value + 3 * span + 64
            else:
                addrs = [block.value + lead + i * span for i in range(3)]
                assert all(a % 2 == 1 for a in addrs)
            C.memset(block.value, 0xA5, 3 * span + 64)
            for a, im in zip(addrs, imgs):
                _place(a, im, p)
            ptrs = (C.c_void_p * 3)(*addrs)
            outs = (capi.svoh_frame_t * 3)()
            ctx._check(lib.svoh_build_pyramid_multi(ctx.h, ptrs, 3, w, h, p, capi.SVOH_MEM_HOST_PINNED, od.N_LEVELS, rounding, outs))
            for i in range(3):
                _check_frame(ctx, outs[i], want[i])
    finally:
        ctx._check(lib.svoh_host_free(ctx.h, block))
    del buf


# ---------------------------------------------------------------------------------------------------------------------
# sparse image alignment
# ---------------------------------------------------------------------------------------------------------------------
class CachedOracle(object):
    """The oracle with its alignment answers remembered: the same problems go through every workgroup geometry, the oracle
    computes each answer once.  Everything else is the oracle's."""

    def __init__(self, orc):
        self._orc, self._memo = orc, {}

    def __getattr__(self, name):
        return getattr(self._orc, name)

    def sparse_align_evaluate(self, opt, pb, level):
        key = ("evaluate", id(pb), bytes(opt), level)
        if key not in self._memo:
            self._memo[key] = (pb, self._orc.sparse_align_evaluate(opt, pb, level))
        return self._memo[key][1]

    def sparse_align_run(self, opt, pb, trace_capacity=0):
        if trace_capacity:
            return self._orc.sparse_align_run(opt, pb, trace_capacity=trace_capacity)
        key = ("run", id(pb), bytes(opt))
        if key not in self._memo:
            self._memo[key] = (pb, self._orc.sparse_align_run(opt, pb))
        return self._memo[key][1]


class Case(object):
    def __init__(self, ctx, orc, tag, sizes, scenes, kind="parity"):
        self.tag, self.sizes, self.scenes, self.kind = tag, sizes, scenes, kind
        self.P = scenes[0].patch_size
        self.opb, self.gpb, self.keep = sa.both(ctx, orc, scenes, n_levels=od.N_LEVELS)


def option_sets(P):
    """plain, and illumination gain + offset with robust weights"""
    return [capi.default_align_options(patch_size=P, min_level=0),
            capi.default_align_options(patch_size=P, min_level=0, estimate_illumination_gain=1, estimate_illumination_offset=1,
                                       robustification=1)]


@pytest.fixture(scope="module")
def cases(gpu_ctx, oracle_lib):
    """the problems, built once: oracle problem + device problem on the same pyramids (sa.both asserts those equal)"""
    orc = CachedOracle(oracle_lib)
    out = {}
    seeds = {("A", "pinhole"): 301, ("A", "radtan"): 302, ("B", "pinhole"): 303, ("B", "radtan"): 304, ("C", "pinhole"): 305,
             ("C", "radtan"): 306}
    for (name, kind), seed in seeds.items():
        out["%s_%s" % (name, kind)] = Case(gpu_ctx, orc, "%s_%s" % (name, kind), [name], [od.align_scene(name, kind, seed)])
    for name in ("A", "B"):
        out["selection_" + name] = Case(gpu_ctx, orc, "selection_" + name, [name], [od.selection_scene(name)], kind="selection")
    sc = od.align_scene("A", "pinhole", 74, border_features=0, invalid_fraction=0.0)
    od.add_edge_visibility_features(sc)
    out["visibility_A"] = Case(gpu_ctx, orc, "visibility_A", ["A"], [sc])
    # camera 0 at A, camera 1 at B: the levels' summed bytes, off_cur and every offset behind an image with a tail.  440 features
    # stay below the 512 from which a problem alone is spread over a cluster of workgroups, so the knobs decide its geometry; the
    # second rig (720 features) is the one that runs in cluster mode whatever the knobs say
    out["rig_A_B"] = Case(gpu_ctx, orc, "rig_A_B", ["A", "B"], [od.align_scene("A", "pinhole", 311, n=180, border_features=40),
                                                                od.align_scene("B", "radtan", 311, n=180, border_features=40)])
    out["rig_A_B_cluster"] = Case(gpu_ctx, orc, "rig_A_B_cluster", ["A", "B"], [od.align_scene("A", "pinhole", 312), od.align_scene("B", "radtan", 312)])
    return orc, out


def level_paths(sizes, max_level, min_level, budget):
    """The kernel's rule (sparse_align.hip, "which levels stay resident"), restated: from the coarsest level down a level is
    RESIDENT while it fits beside the coarser ones; once one did not fit no finer one is resident, and such a level is STAGED
    alone at its turn if it fits by itself, else read from GLOBAL memory.  sizes: (w0, h0) per camera."""
    def need(l):
        return sum(2 * ((w * h + 15) & ~15) for w, h in (od.level_sizes(w0, h0)[l] for w0, h0 in sizes))
    paths, off, room = {}, 0, True
    for l in range(max_level, min_level - 1, -1):
        room = room and off + need(l) <= budget
        if room:
            paths[l] = "resident"
            off += need(l)
        else:
            paths[l] = "staged" if need(l) <= budget else "global"
    return paths


def test_level_paths_restates_the_documented_640x480_case():
    """sparse_align.hip: "640x480: levels 4, 3, 2 = 50 400 bytes" fit 51 KB side by side, nothing finer fits even alone"""
    assert level_paths([(640, 480)], 4, 0, 52224) == {4: "resident", 3: "resident", 2: "resident", 1: "global", 0: "global"}
    assert level_paths([(640, 480)], 4, 0, 50399) == {4: "resident", 3: "resident", 2: "staged", 1: "global", 0: "global"}
    assert level_paths([od.SIZES["A"]], 4, 0, 79872)[1] == "staged" and level_paths([od.SIZES["B"]], 4, 0, 79872)[1] == "resident"


class Coverage(object):
    """which way the levels with a truncated size and a 16-byte tail went, over the full-run launches noted"""

    def __init__(self, ctx):
        self.ctx, self.seen, self.launches = ctx, {}, []

    def note(self, case, opt):
        budget, info = self.ctx.last_align_launch_lds(), self.ctx.last_align_launch()
        sizes = [od.SIZES[n] for n in case.sizes]
        paths = level_paths(sizes, opt.max_level, opt.min_level, budget)
        self.launches.append((case.tag, info["nt"], info["rows"], info["latency"], info["rig"], budget, info["cluster_g"], paths))
        for l, path in paths.items():
            lv = [od.level_sizes(w0, h0)[l] for w0, h0 in sizes]
            truncated = any((w, h) != (w0 / float(1 << l), h0 / float(1 << l)) for (w, h), (w0, h0) in zip(lv, sizes))
            if truncated and any((w * h) % 16 for w, h in lv):
                self.seen.setdefault(path, set()).add((case.tag, l))

    def assert_all_three(self):
        print("[residency] " + "; ".join("%s: %s" % (k, sorted(v)[:4]) for k, v in sorted(self.seen.items())))
        assert set(self.seen) == {"resident", "staged", "global"}, (sorted(self.seen), self.launches[:12])


def check_case(ctx, orc, case, coverage=None, after_run=None):
    for opt in option_sets(case.P):
        if case.kind == "selection":
            # the bars of tests/test_boundaries_gpu.py: one visibility byte per selected feature, the selected count, and the
            # first evaluation equal to the oracle's
            kept = sum(od.SELECTION_KEPT)
            H, g, chi2, nm, vis = ctx.sparse_align_evaluate(opt, case.gpb[0], 4)
            assert vis.size == kept
            res = ctx.sparse_align(opt, case.gpb)[0]
            assert res.n_fts_to_track == kept
            Ho, go, c2o, nmo, viso = orc.sparse_align_evaluate(opt, case.opb, 4)
            assert nmo == nm and nm > 0 and np.array_equal(viso, vis)
            assert np.abs(H - Ho).max() <= 1e-10 * np.abs(Ho).max() and np.abs(g - go).max() <= 1e-10 * np.abs(go).max()
        else:
            sa.check_evaluate(ctx, orc, opt, case.opb, case.gpb, (4, 3, 2, 1, 0) if case.tag == "visibility_A" else (4, 3, 1, 0))
            sa.check_run(ctx, orc, opt, case.opb, case.gpb)
        if after_run is not None:
            after_run()
        if coverage is not None:
            coverage.note(case, opt)


def test_crafted_visibility_premise(cases):
    """on the oracle: the visible count differs between levels, is below the selected count at one, and changes inside a level
    during the run (tests/test_odd_sizes_cpu.py checks each crafted pixel against the integer level size)"""
    orc, cs = cases
    case = cs["visibility_A"]
    opt = option_sets(4)[0]
    n_vis = {}
    for level in (4, 3, 2, 1, 0):
        H, g, chi2, nm, vis = orc.sparse_align_evaluate(opt, case.opb, level)
        assert vis.size == case.scenes[0].n_features
        n_vis[level] = int(vis.sum())
    assert len(set(n_vis.values())) >= 2 and min(n_vis.values()) < case.scenes[0].n_features, n_vis
    n, ro, tr = orc.sparse_align_run(opt, case.opb, trace_capacity=80)
    lv, nm = tr["level"], tr["n_meas"]
    assert any(lv[k] == lv[k - 1] and nm[k] != nm[k - 1] for k in range(1, len(lv)))


def test_default_geometry(gpu_ctx, cases):
    """every case in the geometry the library picks for one small problem, each of the three residency paths covered"""
    orc, cs = cases
    cov = Coverage(gpu_ctx)
    for case in cs.values():
        check_case(gpu_ctx, orc, case, cov)
    cov.assert_all_three()


@pytest.mark.parametrize("nt,rows", [("256", "0"), ("512", "0"), ("512", "2"), ("512", "4"), ("512", "8")])
def test_all_workgroup_geometries(gpu_ctx, cases, nt, rows, monkeypatch):
    """the knobs of test_sparse_align_gpu.test_all_workgroup_geometries: threads, lanes per patch, and -- after the pass with
    the geometry's own image budget, whose residency paths are asserted -- the image budget forced to nothing / levels >= 2 /
    everything that fits"""
    orc, cs = cases
    monkeypatch.setenv("SVOH_ALIGN_THREADS", nt)
    monkeypatch.setenv("SVOH_ALIGN_ROWS", rows)
    gpu_ctx.reload_knobs()
    cov = Coverage(gpu_ctx)
    for case in cs.values():
        check_case(gpu_ctx, orc, case, cov)
    print("[geometries] %r" % sorted(set(l[1:5] + (l[6],) for l in cov.launches)))
    assert all(l[1] == int(nt) and l[6] == 0 for l in cov.launches if l[0] != "rig_A_B_cluster"), [l[:7] for l in cov.launches]
    assert all(l[6] >= 2 for l in cov.launches if l[0] == "rig_A_B_cluster")
    cov.assert_all_three()
    for lds in ("0", "38400", "153856"):
        monkeypatch.setenv("SVOH_ALIGN_LDS", lds)
        gpu_ctx.reload_knobs()
        forced = Coverage(gpu_ctx)
        for case in cs.values():
            check_case(gpu_ctx, orc, case, forced)
        assert all(l[5] <= int(lds) for l in forced.launches)
        if lds == "0":
            assert set(forced.seen) == {"global"}


def test_visibility_case_in_a_cluster(gpu_ctx, cases, monkeypatch):
    """the crafted visibility case spread over three workgroups (SVOH_ALIGN_CLUSTER, as
    test_sparse_align_gpu.test_visibility_changes_inside_a_level forces it): every share must notice a patch that comes or goes"""
    orc, cs = cases
    monkeypatch.setenv("SVOH_ALIGN_CLUSTER", "3")
    gpu_ctx.reload_knobs()
    cov = Coverage(gpu_ctx)
    check_case(gpu_ctx, orc, cs["visibility_A"], cov)
    assert all(l[6] == 3 for l in cov.launches), cov.launches


def test_batch_build(gpu_ctx, cases, monkeypatch):
    """the batch build (256 threads, levels staged through registers from a table of 16-byte pieces: stage_item_list) on ONE
    problem, forced the way test_sparse_align_batch_build_gpu.test_batch_build_on_one_problem forces it; that it ran is
    asserted behind every run"""
    orc, cs = cases
    monkeypatch.setenv("SVOH_ALIGN_THREADS", "256")
    monkeypatch.setenv("SVOH_ALIGN_LATENCY_BUILD", "0")
    gpu_ctx.reload_knobs()
    cov = Coverage(gpu_ctx)
    for tag in ("A_pinhole", "A_radtan", "B_radtan", "visibility_A", "rig_A_B"):
        check_case(gpu_ctx, orc, cs[tag], cov, after_run=lambda: assert_batch_build(gpu_ctx.last_align_launch(), 1, 1))
    cov.assert_all_three()


# ---------------------------------------------------------------------------------------------------------------------
# KLT
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_klt_boundary_tracks(gpu_ctx, oracle_lib, name):
    sc = helpers.small_scene(62, n=10, cam=od.camera(name, "pinhole"))
    ref = oracle_lib.create_img_pyramid(sc.img_ref, od.N_LEVELS)
    fr = gpu_ctx.build_pyramid(sc.img_ref, od.N_LEVELS)
    opt = capi.default_klt_options(max_level=0, min_level=0)
    px_ref, px_cur, ok = od.klt_boundary_tracks(name)
    n = px_ref.size // 2
    po, so = oracle_lib.klt_track_batch(opt, [ref] * n, ref, px_ref, px_cur)
    pg, sg = gpu_ctx.klt_track_batch(opt, [fr] * n, fr, px_ref, px_cur)
    assert np.array_equal(sg, so) and np.array_equal(pg, po)
    assert list(sg[:8]) == ok and sg[8] == 0 and sg[9] == 1
    gpu_ctx.release_frame(fr)


@pytest.mark.parametrize("cam_kind", ["pinhole", "radtan"])
def test_klt_bit_identical(gpu_ctx, oracle_lib, cam_kind):
    """test_klt_matcher_gpu.test_klt_bit_identical at A"""
    orc = oracle_lib
    sc = synth.make_align_scene(51, n_features=10, cam=od.camera("A", cam_kind), rot_deg=(0.5, 1.5), trans_m=(0.05, 0.15))
    ref, cur = orc.create_img_pyramid(sc.img_ref, od.N_LEVELS), orc.create_img_pyramid(sc.img_cur, od.N_LEVELS)
    fr, fc = gpu_ctx.build_pyramid(sc.img_ref, od.N_LEVELS), gpu_ctx.build_pyramid(sc.img_cur, od.N_LEVELS)
    tr = synth.make_track_set(sc, 400, margin=6)
    for kw in (dict(), dict(min_level=2), dict(max_iter=3), dict(patch_sizes=[8, 8, 16, 16, 8]), dict(min_update_squared=1e-6)):
        opt = capi.default_klt_options(**kw)
        po, so = orc.klt_track_batch(opt, ref, cur, tr["px_ref"], tr["px_cur_init"])
        pg, sg = gpu_ctx.klt_track_batch(opt, fr, fc, tr["px_ref"], tr["px_cur_init"])
        assert np.array_equal(so, sg)
        assert np.array_equal(po, pg), np.abs(po - pg).max()
        if not kw:
            ok = so == 1
            err = np.linalg.norm((pg - tr["px_true"]).reshape(-1, 2), axis=1)
            assert ok.mean() > 0.9 and np.median(err[ok]) < 0.1
    gpu_ctx.release_frame(fr); gpu_ctx.release_frame(fc)


# ---------------------------------------------------------------------------------------------------------------------
# matcher, depth filter, epipolar seam
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(params=["eight_lanes_per_unit", "one_lane_per_unit", "packed", "one_wave_per_unit"])
def matcher_geometry(request, gpu_ctx):
    """the four SVOH_MATCHER_G8 geometries of tests/test_klt_matcher_gpu.py's fixture of this name (autouse for that whole
    module, so it is restated here for the tests that ask for it)"""
    old = os.environ.get("SVOH_MATCHER_G8")
    os.environ["SVOH_MATCHER_G8"] = {"eight_lanes_per_unit": "1", "one_lane_per_unit": "0", "packed": "2", "one_wave_per_unit": "3"}[request.param]
    gpu_ctx.reload_knobs()
    yield request.param
    if old is None:
        os.environ.pop("SVOH_MATCHER_G8", None)
    else:
        os.environ["SVOH_MATCHER_G8"] = old
    gpu_ctx.reload_knobs()


MATCHER_SCENES = [("A", "pinhole"), ("B", "radtan")]


@pytest.fixture(scope="module")
def matcher_scenes(gpu_ctx, oracle_lib):
    """scene, oracle pyramids, device frames per (size, camera); the motion of seed 162 carries pixels towards the right and
    the bottom edge, so that matches exist there (the premise each test asserts on the oracle)"""
    out = {}
    for name, kind in MATCHER_SCENES:
        sc = synth.make_align_scene(162, n_features=10, cam=od.camera(name, kind), rot_deg=(0.5, 1.5), trans_m=(0.05, 0.15))
        ref, cur = oracle_lib.create_img_pyramid(sc.img_ref, od.N_LEVELS), oracle_lib.create_img_pyramid(sc.img_cur, od.N_LEVELS)
        fr, lv = gpu_ctx.build_pyramid(sc.img_ref, od.N_LEVELS, return_levels=True)
        fc, lvc = gpu_ctx.build_pyramid(sc.img_cur, od.N_LEVELS, return_levels=True)
        for a, b in zip(lv + lvc, ref + cur):
            assert np.array_equal(a, b)
        out[(name, kind)] = (sc, ref, cur, fr, fc)
    return out, {}


def _both_outcomes(result, edge):
    """the premise of the crafted units, on the oracle: some are matched, some are not"""
    r = result[edge]
    assert (r == capi.MATCH_SUCCESS).any() and (r != capi.MATCH_SUCCESS).any(), np.unique(r, return_counts=True)


@pytest.mark.parametrize("name,kind", MATCHER_SCENES)
def test_update_seeds_parity(gpu_ctx, oracle_lib, matcher_scenes, matcher_geometry, name, kind):
    """1000 seeds (margin 3, levels 0..3) and 60 whose match lies within 2 level pixels of w_L - 8 / h_L - 8, the bound of the
    epipolar scans' in-frame test at their level; two rounds, the state fed back"""
    orc = oracle_lib
    packs, memo = matcher_scenes
    sc, ref, cur, fr, fc = packs[(name, kind)]
    sd = od.seed_set_with_edge_units(sc, 1000, margin=3, levels=(0, 1, 2, 3), bound=8)
    ov_r, ov_c, gv_r, gv_c = views(gpu_ctx, orc, sc, ref, cur, fr, fc, sd["mu_range"])
    mopt = capi.default_matcher_options(scan_on_unit_sphere=int(kind == "radtan"))
    dopt = capi.default_depth_filter_options(sc.cam)
    if ("seeds", name) not in memo:      # the oracle's two rounds, once for the four geometries
        fbo, ko = orc.make_feature_batch(sd["ref_frame_idx"], sd["px"], sd["f"], sd["grad"], sd["level"], sd["type"])
        rounds, state = [], sd["state"]
        for rnd in range(2):
            nso, state, so, mro = orc.update_seeds_batch(mopt, dopt, [ov_r], ov_c, fbo, state)
            rounds.append((nso, state, so, mro, ko["type"].copy()))
        memo[("seeds", name)] = rounds
    fbg, kg = fe.make_feature_batch(sd["ref_frame_idx"], sd["px"], sd["f"], sd["grad"], sd["level"], sd["type"])
    state_g = sd["state"]
    for rnd, (nso, state_o, so, mro, type_o) in enumerate(memo[("seeds", name)]):
        nsg, state_g, sg, mrg = gpu_ctx.update_seeds_batch(mopt, dopt, [gv_r], gv_c, fbg, state_g)
        assert nso == nsg and np.array_equal(so, sg)
        assert np.array_equal(mro, mrg), np.nonzero(mro != mrg)
        assert np.array_equal(type_o, kg["type"])
        assert np.allclose(state_g, state_o, rtol=1e-9, atol=0)
        assert len(set(mro.tolist())) >= 4 and nso > 0.5 * 1000
        _both_outcomes(mro, sd["edge"])


@pytest.mark.parametrize("name,kind", MATCHER_SCENES)
def test_match_direct_parity(gpu_ctx, oracle_lib, matcher_scenes, matcher_geometry, name, kind):
    """800 units (margin 3, levels 0..3) and 60 whose predicted pixel lies within 2 level pixels of w_L - 4 / h_L - 4, the bound
    of align1D / align2D's in-frame test at the search level; the affine and the pixelwise warp"""
    orc = oracle_lib
    packs, memo = matcher_scenes
    sc, ref, cur, fr, fc = packs[(name, kind)]
    sd = od.seed_set_with_edge_units(sc, 800, margin=3, levels=(0, 1, 2, 3), bound=4)
    ov_r, ov_c, gv_r, gv_c = views(gpu_ctx, orc, sc, ref, cur, fr, fc, sd["mu_range"])
    px_true, px_init = od.predicted_pixels(sc, sd, 2.0, 1)
    px_init[:20] += 40.0          # some hopeless starts
    lm = np.ascontiguousarray(sc.T_w_ref.transform(sd["f"].reshape(-1, 3).T * sd["true_depth"]).T)
    ftype = np.where(sd["type"] == 0, capi.FT_EDGELET, capi.FT_CORNER)
    for mkw in (dict(), dict(affine_est_gain=1)):
        mopt = capi.default_matcher_options(**mkw)
        for warp, landmarks in (("affine", None), ("pixelwise", lm)):
            key = ("direct", name, warp, tuple(mkw))
            if key not in memo:
                fbo, ko = orc.make_feature_batch(sd["ref_frame_idx"], sd["px"], sd["f"], sd["grad"], sd["level"], ftype)
                memo[key] = orc.match_direct_batch(mopt, [ov_r], ov_c, fbo, sd["true_depth"], px_init, landmark_xyz=landmarks)
            oo = memo[key]
            fbg, kg = fe.make_feature_batch(sd["ref_frame_idx"], sd["px"], sd["f"], sd["grad"], sd["level"], ftype)
            og = gpu_ctx.match_direct_batch(mopt, [gv_r], gv_c, fbg, sd["true_depth"], px_init, landmark_xyz=landmarks)
            assert np.array_equal(oo["result"], og["result"]), np.nonzero(oo["result"] != og["result"])[0][:10]
            assert np.array_equal(oo["search_level"], og["search_level"])
            assert np.abs(oo["px_cur"] - og["px_cur"]).max() <= 1e-4
            ok = oo["result"] == 0
            assert ok.sum() > 0.5 * 800 and len(set(oo["result"].tolist())) >= 3
            assert set(oo["search_level"][ok].tolist()) >= {0, 1, 2, 3}
            assert np.allclose(oo["A"], og["A"], rtol=1e-12, atol=1e-14)
            assert np.abs(oo["f_cur"] - og["f_cur"])[np.repeat(ok, 3)].max() < 1e-6
            if warp == "affine":
                assert np.allclose(oo["h_inv"], og["h_inv"], rtol=1e-6)
            _both_outcomes(oo["result"], sd["edge"])


@pytest.mark.parametrize("sphere", [0, 1])
@pytest.mark.parametrize("name,kind", MATCHER_SCENES)
def test_epipolar_match_parity_stereo_seam(gpu_ctx, oracle_lib, matcher_scenes, matcher_geometry, name, kind, sphere):
    """test_klt_matcher_gpu.test_epipolar_match_batch_parity_stereo_seam: 500 search steps, 300 features (+ 60 at the scans'
    in-frame bound), on the unit plane and on the unit sphere"""
    orc = oracle_lib
    packs, memo = matcher_scenes
    sc, ref, cur, fr, fc = packs[(name, kind)]
    sd = od.seed_set_with_edge_units(sc, 300, margin=6, levels=(0, 1, 2), bound=8)
    ftype = np.where(sd["type"] == 0, capi.FT_EDGELET, capi.FT_CORNER).astype(np.uint8)
    ov_r, ov_c, gv_r, gv_c = views(gpu_ctx, orc, sc, ref, cur, fr, fc, 0.0)
    T_f1f0 = (sc.T_cur_f_w_gt * sc.T_ref_f_w.inverse()).as7()
    d_mean = float(np.median(sd["true_depth"]))
    d_inv = [1.0 / d_mean, 1.0 / (0.3 * d_mean), 1.0 / (15.0 * d_mean)]
    mopt = capi.default_matcher_options(max_epi_search_steps=500, subpix_refinement=1, scan_on_unit_sphere=sphere)
    key = ("epipolar", name, sphere)
    if key not in memo:
        fbo, ko = orc.make_feature_batch(sd["ref_frame_idx"], sd["px"], sd["f"], sd["grad"], sd["level"], ftype)
        memo[key] = orc.epipolar_match_batch(mopt, [ov_r], ov_c, fbo, d_inv_common=d_inv, T_cur_ref=[T_f1f0])
    oo = memo[key]
    fbg, kg = fe.make_feature_batch(sd["ref_frame_idx"], sd["px"], sd["f"], sd["grad"], sd["level"], ftype)
    og = gpu_ctx.epipolar_match_batch(mopt, [gv_r], gv_c, fbg, d_inv_common=d_inv, T_cur_ref=[T_f1f0])
    assert np.array_equal(oo["result"], og["result"]), np.nonzero(oo["result"] != og["result"])
    assert np.array_equal(oo["search_level"], og["search_level"])
    ok = oo["result"] == capi.MATCH_SUCCESS
    assert ok.mean() > 0.5 and len(set(oo["result"].tolist())) >= 3
    assert np.allclose(og["depth"][ok], oo["depth"][ok], rtol=1e-9, atol=0)
    assert np.abs(oo["px_cur"] - og["px_cur"])[np.repeat(ok, 2)].max() <= 1e-4
    assert np.abs(oo["f_cur"] - og["f_cur"])[np.repeat(ok, 3)].max() < 1e-6
    assert np.allclose(oo["A"], og["A"], rtol=1e-12, atol=1e-14)
    _both_outcomes(oo["result"], sd["edge"])


# ---------------------------------------------------------------------------------------------------------------------
# candidate projection
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pinhole", "radtan"])
def test_candidate_projection_at_every_edge(gpu_ctx, kind):
    """svoh_project_candidates at A, 2000 points (landmarks and seeds of two keyframes) whose projections straddle, within
    +-1 px, every bound of projectPointAndCheckVisibility (reprojector.cpp:525-543): the image's edges 0 | w and 0 | h
    (Frame::isVisible) and the 8-pixel margin on the truncated pixel.  Verdicts exact and pixels to 1e-9 against the NumPy
    restatement test_sparse_align_gpu.test_candidate_projection_rides_the_alignment_launch uses (no point is put closer than
    1e-3 px to a bound, so rounding cannot decide)."""
    lib, h = gpu_ctx.lib, gpu_ctx.h
    cam = od.camera("A", kind)
    w, ht = od.SIZES["A"]
    rng = np.random.RandomState(8)
    T_w_cur = synth.SE3(synth.quat_from_axis_angle([0.2, 1, -0.1], 0.15), (0.4, -0.1, 0.2))
    T_w_kf = [T_w_cur * synth.SE3(synth.quat_from_axis_angle([0, 1, 0.3], 0.05), (0.1, 0.05, 0.02)),
              T_w_cur * synth.SE3(synth.quat_from_axis_angle([1, 0, 0.2], -0.08), (-0.2, 0.0, 0.1))]
    n = 2000
    bounds = [(0, 0.0), (0, 8.0), (0, w - 8.0), (0, float(w)), (1, 0.0), (1, 8.0), (1, ht - 8.0), (1, float(ht))]
    target = np.zeros((n, 2))
    for i in range(n):
        axis, b = bounds[i % 8]
        d = rng.choice([-1.0, 1.0]) * rng.uniform(1e-3, 1.0)
        other = rng.uniform(-4.0, (ht, w)[axis] + 4.0)
        target[i] = (b + d, other) if axis == 0 else (other, b + d)
    x, y = cam.undistorted_xy(target[:, 0], target[:, 1])
    for _ in range(40):           # the distortion's inverse to rounding (undistorted_xy stops at 1e-4 px in the far corners)
        p = cam.project(np.stack([x, y, np.ones(n)]))
        x, y = x + (target[:, 0] - p[0]) / cam.fx, y + (target[:, 1] - p[1]) / cam.fy
    X_cur = np.stack([x, y, np.ones(n)]) * rng.uniform(0.5, 8.0, n)
    X_w = T_w_cur.transform(X_cur)
    kind_arr = (rng.uniform(size=n) < 0.5).astype(np.uint8)
    kf = rng.randint(0, 2, n).astype(np.int32)
    v, mu = np.zeros((n, 3)), np.ones(n)
    for i in range(n):
        if kind_arr[i]:       # a seed: bearing vector in its keyframe and inverse depth
            X_kf = T_w_kf[kf[i]].inverse().transform(X_w[:, i])
            v[i] = X_kf / np.linalg.norm(X_kf)
            mu[i] = 1.0 / np.linalg.norm(X_kf)
        else:
            v[i] = X_w[:, i]
    T_f_w = T_w_cur.inverse()
    c, T = fe._camera(cam), fe._se3(T_f_w)
    Tk = (capi.svoh_se3 * 2)(*[fe._se3(t) for t in T_w_kf])
    v_flat = np.ascontiguousarray(v).ravel()
    px, vis = np.zeros(2 * n), np.zeros(n, np.uint8)
    assert lib.svoh_project_candidates(h, C.byref(c), C.byref(T), 2, Tk, n, kind_arr.ctypes.data, kf.ctypes.data, v_flat.ctypes.data,
                                       mu.ctypes.data, px.ctypes.data, vis.ctypes.data) == 0
    ncam, nT = nd.Cam.of(cam), nd.Tf.from7(T_f_w.as7())
    want = np.zeros(n, np.uint8)
    for i in range(n):
        ok, p = nd.get_candidate(ncam, nT, nd.Tf.from7(T_w_kf[kf[i]].as7()).inverse(), v[i] if not kind_arr[i] else None, v[i], mu[i])
        want[i] = ok
        if ok:
            assert np.abs(px[2 * i:2 * i + 2] - p).max() < 1e-9, i
            assert np.abs(p - target[i]).max() < 1e-6, i           # the point is where it was put
    assert np.array_equal(vis, want), np.nonzero(vis != want)[0][:10]
    for k in range(8):            # both verdicts at the margin's bounds; at the image's own edges the margin has already said no
        if bounds[k][1] in (0.0, float(w), float(ht)):
            assert want[k::8].sum() == 0
        else:
            assert 0 < want[k::8].sum() < want[k::8].size, (k, want[k::8].sum())
