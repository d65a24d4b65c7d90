"""The composition of the batch-build parity set (tests/align_batch_set.py) holds every condition the GPU tests of
tests/test_sparse_align_batch_build_gpu.py rely on, and is bit-reproducible from its seed.  No GPU, no images."""
import os
import sys

import numpy as np
import pytest

import align_batch_set as bs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUM_CUS = 256


@pytest.fixture(scope="module")
def comp():
    return bs.compose(NUM_CUS)


def _sets(comp):
    return (("main", comp.main), ("mid", comp.mid))


def test_reproducible_from_the_seed(comp):
    assert bs.compose(NUM_CUS).astuple() == comp.astuple()
    assert bs.compose(NUM_CUS, seed=comp.seed + 1).astuple() != comp.astuple()
    # ... down to the scenes' arrays
    for s in comp.main[:40]:
        for c in s.cams:
            a, b = c.scene(4), c.scene(4)
            for name in ("px", "f", "pos_world", "flags"):
                assert np.array_equal(getattr(a, name), getattr(b, name))


def test_sizes(comp):
    for P in (4, 8):
        main, mid = comp.launch("main", P), comp.launch("mid", P)
        grid = 2 * NUM_CUS
        assert len(main) >= 5 * NUM_CUS and len(main) - grid >= 3 * NUM_CUS   # some workgroup takes at least three
        assert len(mid) >= NUM_CUS and len(mid) < grid                        # the batch build, a workgroup each, an idle tail
    assert len(comp.mid) == NUM_CUS + 17
    assert len(comp.launch("main", 8)) == 5 * NUM_CUS


def test_feature_counts(comp):
    n = np.array([s.n_features for s in comp.main])
    assert n.min() == 12 and n.max() == 2000
    assert 200 <= n.mean() <= 300
    assert np.median(n) < n.mean() and np.median(n) < 200                     # skewed small
    per_cam = set(c.n_total for s in comp.main for c in s.cams)
    for r in bs.REQUIRED_COUNTS:
        assert r in per_cam, r
    for s in comp.main + comp.mid:
        for c in s.cams:
            sc = c.scene(4)
            assert sc.n_features == c.n_total and sc.flags.size == c.n_total
    assert 2000 in set(c.n_total for s in comp.mid for c in s.cams)


def test_cameras_and_rigs(comp):
    for name, specs in _sets(comp):
        kinds = [c.kind for s in specs for c in s.cams]
        for k in ("pinhole640", "radtan640", "radtan752"):
            assert kinds.count(k) >= len(specs) // 10, (name, k)
        n2 = sum(1 for s in specs if len(s.cams) == 2)
        assert n2 >= 0.05 * len(specs), name
        assert sum(1 for s in specs if s.kind == "quad") >= 2, name
        assert sum(1 for s in specs if s.kind == "small_rig") >= 3, name
        assert any(len(s.cams) == 2 and all(c.kind == "radtan752" for c in s.cams) or
                   len(s.cams) == 2 and any(c.kind == "radtan752" for c in s.cams) for s in specs), name
        assert any(len(s.cams) >= 2 and any(c.no_flags for c in s.cams) and not all(c.no_flags for c in s.cams) for s in specs), name
        for s in specs:
            if s.kind == "quad":
                assert len(s.cams) == 4 and all(bs.camera_of(c.kind).width == 640 for c in s.cams)
            if s.kind == "small_rig":
                assert len(s.cams) == 3 and not s.p8
            else:
                assert s.p8
    assert bs.camera_of("radtan752").width == 752 and (752 >> 4) * (480 >> 4) == 1410 and 1410 % 16 != 0
    assert bs.camera_of("pinhole640").dist is None and bs.camera_of("radtan640").dist is not None


def _image_areas():
    """the image area of every batch instantiation as launch_one sizes it, from the static LDS of the built code objects"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources_built as krb
    import subprocess
    csrc = os.path.join(ROOT, "svo_pro_universal_amd", "csrc")
    if not os.path.exists(os.path.join(csrc, "sparse_align.o")):
        subprocess.check_call(["make", "-s", "-C", csrc])
    ks = krb.kernels(os.path.join(csrc, "sparse_align.o"))
    areas = {}
    for P in (4, 8):
        for illum in ("false", "true"):
            for robust in ("false", "true"):
                d = ks["sparse_align_kernel<%d, 256, %s, false, %s, 1, false, false>" % (P, illum, robust)]
                areas[(P, illum, robust)] = bs.lds_img_bytes_for(d["lds"])
    return areas


def test_staging_arithmetic_matches_the_built_kernels(comp):
    """The rigs were sized from the kernel's staging rule; here the rule is applied with the image area the built batch
    instantiations really get: 640x480 mono keeps levels 4..2 (6 images), 752x480 mono keeps 4..3 and stages level 2 over
    them, a two-camera rig does not keep level 2, four 640x480 cameras fill the 16-entry table exactly, three 320x240
    cameras need 18 entries (the list is refused, the workgroup stages level by level)."""
    areas = _image_areas()
    assert len(areas) == 8
    for key, area in areas.items():
        for lo in (0, 2):
            plan = lambda sizes: bs.staging_plan(sizes, 4, lo, area)
            assert plan([(640, 480)]) == ([4, 3, 2], 6, True), (key, area)
            assert plan([(752, 480)]) == ([4, 3], 4, True), (key, area)
            assert plan([(640, 480), (640, 480)]) == ([4, 3], 8, True), (key, area)
            assert plan([(752, 480), (640, 480)]) == ([4, 3], 8, True), (key, area)
            assert plan([(640, 480)] * 4) == ([4, 3], bs.K_MAX_STAGE_ITEMS, True), (key, area)
            if key[0] == 4:
                res, n_items, ok = plan([(320, 240)] * 3)
                assert res == [4, 3, 2] and n_items == 18 and not ok, (key, area)
    # every problem of the set is one of the cases above; the fallback sits BETWEEN two list-staged problems
    for name, specs in _sets(comp):
        for i, s in enumerate(specs):
            sizes = [(bs.camera_of(c.kind).width, bs.camera_of(c.kind).height) for c in s.cams]
            ok = bs.staging_plan(sizes, 4, 0, min(areas.values()))[2]
            assert ok == (s.kind != "small_rig")
            if s.kind == "small_rig":
                assert 0 < i < len(specs) - 1 and specs[i - 1].kind != "small_rig" and specs[i + 1].kind != "small_rig"


def test_priors_initial_values_degenerate_and_hard_problems(comp):
    for name, specs in _sets(comp):
        n = len(specs)
        assert sum(1 for s in specs if s.prior is not None) >= 0.05 * n, name
        assert any(s.prior is not None and s.prior[7] > 0 and s.prior[8] > 0 for s in specs), name          # illumination lambdas
        assert any(s.prior is not None and s.prior[4] == 0.0 for s in specs) and any(s.prior is not None and s.prior[4] > 0 for s in specs), name
        assert sum(1 for s in specs if s.alpha_init != 0.0 and s.beta_init != 0.0) >= 5, name
        assert sum(1 for s in specs if s.degenerate == "no_flags") >= 0.02 * n, name
        assert sum(1 for s in specs if s.degenerate == "away") >= 0.02 * n, name
        for s in specs:
            if s.degenerate == "no_flags":
                assert all(not c.scene(4).flags.any() for c in s.cams)
        assert sum(1 for s in specs if any(c.border > 0 and c.invalid > 0 for c in s.cams)) >= 5, name
        assert sum(1 for s in specs if any(c.large_motion for c in s.cams)) >= 5, name
        mem = [s.mem for s in specs]
        assert mem.count("device") > mem.count("host") >= 0.05 * n, name


def test_adjacency(comp):
    for P in (4, 8):
        for which in ("main", "mid"):
            specs = comp.launch(which, P)
            for a, b in zip(specs[:-1], specs[1:]):
                for ca, cb in zip(a.cams, b.cams):
                    assert ca.kind != cb.kind, (which, P, a.astuple(), b.astuple())
                assert bs.size_class(a.n_features) != bs.size_class(b.n_features), (which, P, a.n_features, b.n_features)
                if a.degenerate is not None:
                    assert b.ordinary
            assert specs[-1].degenerate is None
    # no image is shared by any two cameras of the set: every camera has its own scene seed
    seeds = [c.seed for s in comp.main + comp.mid for c in s.cams]
    assert len(set(seeds)) == len(seeds)
    pairs = {}
    for s in comp.main:
        for c in s.cams:
            cam = bs.camera_of(c.kind)
            pairs[(cam.width, cam.height)] = pairs.get((cam.width, cam.height), 0) + 1
    assert pairs[(640, 480)] >= 256 and pairs[(752, 480)] >= 64 and pairs[(320, 240)] >= 9
