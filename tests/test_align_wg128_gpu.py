"""The 128-thread batch build of the alignment kernel (sparse_align_kernel<P, 128, ILLUM, false, ROBUST>: two waves per
problem, four workgroups per compute unit) against the oracle, forced through the knobs as
tests/test_sparse_align_batch_build_gpu.py forces the 256-thread one: discrete fields equal, pose / alpha / beta within the
project's tolerances (check_run of tests/test_sparse_align_gpu.py, for every problem of a launch).

What is new in this build and what the cases below aim at:
  * two waves: a 40-feature problem leaves wave 1 without a patch, 129 features give the second trip one lane, 300 features
    three trips with a ragged last one;
  * half-level residency: a level whose pair of images does not fit the image area while one image does runs with the
    reference image in LDS and the current one from global memory (the only choice the kernel has; at the default budget
    level 2 of a 640x480 pair; with SVOH_ALIGN_LDS=6000 level 3).  residency_plan below is this file's own copy of the rule, and the launches' image areas
    are checked against it;
  * queue reuse: with one workgroup per compute unit and num_cus + 40 problems some workgroups take a second problem.
The evaluation path (selection and visibility masks, H, g) is checked in both 256-thread builds: the masks are written by
evaluations only.
"""
import numpy as np
import pytest

from svo_pro_universal_amd import _capi as capi, frontend as fe, synth

import helpers
import test_sparse_align_gpu as sa

pytestmark = pytest.mark.gpu

TOL_POSE = sa.TOL_POSE
RAGGED_COUNTS = (40, 129, 300)


def residency_plan(w, h, level_hi, level_lo, lds):
    """level -> "resident" | "alone" | "half" | "global" for one camera of w x h pixels and lds bytes of image area"""
    one = {l: (((w >> l) * (h >> l)) + 15) & ~15 for l in range(level_lo, level_hi + 1)}
    plan, off, room = {}, 0, True
    for l in range(level_hi, level_lo - 1, -1):
        room = room and off + 2 * one[l] <= lds
        if room:
            plan[l] = "resident"
            off += 2 * one[l]
        elif 2 * one[l] <= lds:
            plan[l] = "alone"
        elif one[l] <= lds:
            plan[l] = "half"
        else:
            plan[l] = "global"
    return plan


def mismatches(res, oracle):
    bad, worst = [], 0.0
    for i, (rg, (n, ro)) in enumerate(zip(res, oracle)):
        d_pose = helpers.se3_max_abs_diff(rg.T_icur_iref, ro.T_icur_iref)
        d_alpha, d_beta = abs(rg.alpha - ro.alpha), abs(rg.beta - ro.beta)
        ok = (rg.n_fts_to_track == n and rg.status == ro.status and list(rg.iters) == list(ro.iters) and list(rg.n_meas) == list(ro.n_meas)
              and rg.n_patch_iters == ro.n_patch_iters and d_pose < TOL_POSE and d_alpha < TOL_POSE and d_beta < 1e-6)
        if ok:
            worst = max(worst, d_pose)
        else:
            bad.append(dict(i=i, gpu=(rg.n_fts_to_track, rg.status, list(rg.iters)[:5], list(rg.n_meas)[:5], rg.n_patch_iters),
                            oracle=(n, ro.status, list(ro.iters)[:5], list(ro.n_meas)[:5], ro.n_patch_iters),
                            d_pose=d_pose, d_alpha=d_alpha, d_beta=d_beta))
    print("[wg128] %d problems, %d mismatches, largest pose difference among the rest %.2e" % (len(res), len(bad), worst))
    return bad


class Ragged(object):
    """three 640x480 problems of 40, 129 and 300 features (border and unusable features among the larger two), one launch"""

    def __init__(self, ctx, orc, P):
        self.orc, self.keep, self.opbs, self.singles, items = orc, [], [], [], []
        for k, n in enumerate(RAGGED_COUNTS):
            cam = synth.Camera.euroc_like() if k == 1 else synth.Camera.test_camera()
            border = (0, 9, 20)[k]
            sc = helpers.small_scene(910 + k, n=n - border, P=P, cam=cam, border_features=border, invalid_fraction=(0.0, 0.05, 0.1)[k],
                                     gain=1.02, offset=1.5)
            assert sc.n_features == n
            opb, gpb, keep = sa.both(ctx, orc, [sc])
            self.keep.append((gpb, keep))
            self.opbs.append(opb)
            self.singles.append((opb, gpb))
            items.append([(sc, gpb[0].cams[0].ref_frame, gpb[0].cams[0].cur_frame)])
        self.problems, keep = fe.make_align_problems(items)
        self.keep.append(keep)
        self._oracle = {}

    def oracle(self, opt, key):
        if key not in self._oracle:
            self._oracle[key] = [self.orc.sparse_align_run(opt, opb)[:2] for opb in self.opbs]
        return self._oracle[key]


@pytest.fixture(scope="module")
def ragged4(gpu_ctx, oracle_lib):
    return Ragged(gpu_ctx, oracle_lib, 4)


@pytest.fixture(scope="module")
def ragged8(gpu_ctx, oracle_lib):
    return Ragged(gpu_ctx, oracle_lib, 8)


def run_wg128(ctx, monkeypatch, opt, problems, grid, **env):
    monkeypatch.setenv("SVOH_ALIGN_THREADS", "128")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx.reload_knobs()
    res = ctx.sparse_align(opt, problems)
    info = ctx.last_align_launch()
    assert info["nt"] == 128 and info["rows"] == 1 and info["latency"] is False and info["rig"] is False and info["cluster_g"] == 0, info
    assert info["grid"] == grid and info["n_desc"] == len(problems), info
    return res


def test_ragged_problems(gpu_ctx, ragged4, monkeypatch):
    """(a) levels 4..0 at the default budget: levels 4 and 3 resident, level 2 with one image in LDS, levels 1 and 0 from global memory"""
    opt = capi.default_align_options(patch_size=4, min_level=0)
    res = run_wg128(gpu_ctx, monkeypatch, opt, ragged4.problems, 3)
    lds = gpu_ctx.last_align_launch_lds()
    print("[wg128] image area at four workgroups per compute unit: %d bytes" % lds)
    assert residency_plan(640, 480, 4, 0, lds) == {4: "resident", 3: "resident", 2: "half", 1: "global", 0: "global"}, lds
    assert not mismatches(res, ragged4.oracle(opt, "plain"))


def test_mixed_residency_at_level_3(gpu_ctx, ragged4, monkeypatch):
    """(b) an image area that holds level 4 and ONE image of level 3.  The resident side is the reference image: the kernel has no
    other choice (the current image as the resident one measured the same and was deleted), so the case runs once."""
    opt = capi.default_align_options(patch_size=4, min_level=0)
    res = run_wg128(gpu_ctx, monkeypatch, opt, ragged4.problems, 3, SVOH_ALIGN_LDS="6000")
    lds = gpu_ctx.last_align_launch_lds()
    assert lds == 6000   # (a multiple of 16: handed on as it is)
    assert residency_plan(640, 480, 4, 0, lds) == {4: "resident", 3: "half", 2: "global", 1: "global", 0: "global"}
    assert not mismatches(res, ragged4.oracle(opt, "plain"))


def test_options(gpu_ctx, ragged4, ragged8, monkeypatch):
    """(d) 8x8 patches once, the illumination terms once -- and the robust weights once, with and without the illumination terms:
    the ROBUST instantiations have no gradient-only pass, so every iteration of theirs is a full pass over the half-resident level"""
    opt8 = capi.default_align_options(patch_size=8, min_level=0)
    assert not mismatches(run_wg128(gpu_ctx, monkeypatch, opt8, ragged8.problems, 3), ragged8.oracle(opt8, "plain"))
    opti = capi.default_align_options(patch_size=4, min_level=0, estimate_illumination_gain=1, estimate_illumination_offset=1)
    assert not mismatches(run_wg128(gpu_ctx, monkeypatch, opti, ragged4.problems, 3), ragged4.oracle(opti, "illum"))
    optr = capi.default_align_options(patch_size=4, min_level=0, robustification=1)
    assert not mismatches(run_wg128(gpu_ctx, monkeypatch, optr, ragged4.problems, 3), ragged4.oracle(optr, "robust"))
    optri = capi.default_align_options(patch_size=4, min_level=0, robustification=1, estimate_illumination_gain=1, estimate_illumination_offset=1)
    assert not mismatches(run_wg128(gpu_ctx, monkeypatch, optri, ragged4.problems, 3), ragged4.oracle(optri, "robust_illum"))


def _permuted(sc, seed):
    perm = np.random.RandomState(seed).permutation(sc.n_features)
    sp = synth.AlignScene()
    sp.__dict__.update(sc.__dict__)
    sp.px, sp.f = sc.px.reshape(-1, 2)[perm].ravel(), sc.f.reshape(-1, 3)[perm].ravel()
    sp.pos_world, sp.flags = sc.pos_world.reshape(-1, 3)[perm].ravel(), sc.flags[perm]
    return sp


def test_queue_reuse(gpu_ctx, oracle_lib, monkeypatch):
    """(c) one workgroup per compute unit, num_cus + 40 problems of 12..60 features on 160x120 images (levels 2..0; level 0 runs
    half resident), one of them with nothing selected: 40 workgroups take a second problem (state reset, restaging, the levels'
    offsets).  A few dozen features on so small an image leave some scenes so ill-conditioned that the oracle's own pose moves by
    more than the tolerance when only the order of its features changes; such a seed is passed over (a criterion that involves
    the oracle alone, as in tests/align_batch_set.py)."""
    import torch
    orc, ctx = oracle_lib, gpu_ctx
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_problems = num_cus + 40
    cam = synth.Camera(160, 120, 80.0, 80.0, 80.0, 60.0)
    opt = capi.default_align_options(patch_size=4, max_level=2, min_level=0)
    rng = np.random.RandomState(4128)
    items, oracle, keep, seed, passed_over = [], [], [], 940000, 0
    while len(items) < n_problems:
        seed += 1
        assert seed < 940000 + 3 * n_problems, "too many scenes the oracle cannot judge"
        n = int(rng.randint(12, 61))
        sc = synth.make_align_scene(seed, n_features=n, patch_size=4, cam=cam, max_level=2, gain=1.0 + 0.04 * rng.uniform(), offset=3.0 * rng.uniform())
        empty = len(items) == 17
        if empty:
            sc.flags[:] = 0
        ref, cur = helpers.scene_pyramids(orc, sc, 3)
        n1, r1, _ = orc.sparse_align_run(opt, orc.problem_from_scenes([(sc, ref, cur)]))
        n2, r2, _ = orc.sparse_align_run(opt, orc.problem_from_scenes([(_permuted(sc, seed), ref, cur)]))
        if not (n1 == n2 and r1.status == r2.status and list(r1.iters) == list(r2.iters) and list(r1.n_meas) == list(r2.n_meas)
                and helpers.se3_max_abs_diff(r1.T_icur_iref, r2.T_icur_iref) < TOL_POSE):
            passed_over += 1
            continue
        fr, fc = ctx.build_pyramid(sc.img_ref, 3), ctx.build_pyramid(sc.img_cur, 3)
        keep.append((fr, fc))
        items.append([(sc, fr, fc)])
        oracle.append((n1, r1))
    print("[wg128] %d problems, %d seeds passed over" % (n_problems, passed_over))
    assert oracle[17][0] == 0 and oracle[17][1].status == 1
    problems, k2 = fe.make_align_problems(items)
    try:
        res = run_wg128(ctx, monkeypatch, opt, problems, num_cus, SVOH_ALIGN_WG_PER_CU="1")
        lds = ctx.last_align_launch_lds()
        assert residency_plan(160, 120, 2, 0, lds) == {2: "resident", 1: "resident", 0: "half"}, lds
        assert res[17].status == 1 and res[17].n_fts_to_track == 0
        assert not mismatches(res, oracle)
    finally:
        for fr, fc in keep:
            ctx.release_frame(fr)
            ctx.release_frame(fc)


@pytest.mark.parametrize("latency_build", ["0", "1"])
def test_evaluate_in_the_256_thread_builds(gpu_ctx, oracle_lib, ragged4, latency_build, monkeypatch):
    """(e) the selection and visibility masks an evaluation hands out are written by evaluations only: mask, H and g of the
    300-feature problem at levels 4, 1 and 0 in the batch build and in the latency build of the 256-thread kernel"""
    monkeypatch.setenv("SVOH_ALIGN_THREADS", "256")
    monkeypatch.setenv("SVOH_ALIGN_LATENCY_BUILD", latency_build)
    gpu_ctx.reload_knobs()
    opb, gpb = ragged4.singles[2]
    for kw in (dict(), dict(estimate_illumination_gain=1, estimate_illumination_offset=1)):
        opt = capi.default_align_options(patch_size=4, min_level=0, **kw)
        gpu_ctx.sparse_align(opt, gpb)   # a run in between: it must leave nothing an evaluation reads
        sa.check_evaluate(gpu_ctx, oracle_lib, opt, opb, gpb, (4, 1, 0))
