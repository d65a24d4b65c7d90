"""The BATCH build of the alignment kernel against the oracle.

Every alignment throughput the project quotes is the batch build's: sparse_align_kernel<P, 256, ILLUM, false, ROBUST, 1,
false, false> -- 256 threads, two workgroups per compute unit, workspace rows by LDS-DMA, the levels' images staged through
registers (stage_item_list), every workgroup taking problem after problem from a queue.  decide_geometry hands it out from
num_cus problems per launch on; the other parity tests launch at most 64.  Here a seeded, ragged set of 5 * num_cus
problems (tests/align_batch_set.py; its conditions are asserted by tests/test_align_batch_set_cpu.py) goes through ONE
launch per option set, and every problem of it is compared with the oracle exactly as check_run of
tests/test_sparse_align_gpu.py compares a single one: discrete fields equal, pose / alpha / beta within the project's
tolerances.  The tests assert their own premise through svoh_sparse_align_last_launch_info: which build ran, with how many
workgroups, over how many problems.

A problem's sums stay inside one workgroup and its lane assignment depends on its own feature order only, so its result
must not depend on what ran before it on the same workgroup, nor on where in the launch it sits: the order / repetition /
alone-in-a-launch legs compare BITS.
"""
import ctypes as C
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from svo_pro_universal_amd import _capi as capi, frontend as fe, synth

import align_batch_set as bs
import helpers
import test_sparse_align_gpu as sa

pytestmark = pytest.mark.gpu

TOL_POSE, TOL_HG = sa.TOL_POSE, sa.TOL_HG


def _options(P, illum, robust, **kw):
    kw.setdefault("min_level", 0)
    return capi.default_align_options(patch_size=P, estimate_illumination_gain=illum, estimate_illumination_offset=illum,
                                      robustification=robust, **kw)


# (id, P, options): the option matrix every problem of the set goes through
CASES = [("p%d_illum%d_robust%d" % (P, il, ro), P, dict(illum=il, robust=ro)) for P in (4, 8) for ro in (0, 1) for il in (0, 1)]
CASES += [("p4_handler_levels", 4, dict(illum=0, robust=0, min_level=2)),
          ("p4_max_iter1", 4, dict(illum=0, robust=0, max_iter=1)),
          ("p4_distortion_jacobian", 4, dict(illum=0, robust=0, use_distortion_jacobian=1))]
CASE = {c[0]: c for c in CASES}
NEIGHBOUR_CASES = ("p4_illum0_robust0", "p4_illum1_robust1")


def case_options(case_id):
    _, P, kw = CASE[case_id]
    kw = dict(kw)
    return _options(P, kw.pop("illum"), kw.pop("robust"), **kw)


def result_bytes(res):
    n = len(res)
    return np.frombuffer(bytes(res), dtype=np.uint8).reshape(n, C.sizeof(capi.svoh_align_result)).copy()


class Bench(object):
    """The rendered set and what has been computed on it so far (oracle results and blocking-call results, per launch and case)."""

    def __init__(self, ctx, orc):
        import torch
        self.ctx, self.orc = ctx, orc
        self.num_cus = torch.cuda.get_device_properties(0).multi_processor_count
        t0 = time.perf_counter()
        self.set = bs.BatchSet(ctx, orc, bs.compose(self.num_cus))
        print("[batch set] %d + %d problems, image pairs %r, built in %.1f s" % (len(self.set.comp.main), len(self.set.comp.mid),
                                                                                self.set.n_pairs, time.perf_counter() - t0))
        self._oracle, self._gpu = {}, {}

    def oracle(self, which, case_id):
        key = (which, case_id)
        if key not in self._oracle:
            L = self.set.launch(which, CASE[case_id][1])
            opt = case_options(case_id)
            t0 = time.perf_counter()
            with ThreadPoolExecutor(max_workers=16) as ex:   # a ctypes call: releases the GIL
                self._oracle[key] = list(ex.map(lambda pb: self.orc.sparse_align_run(opt, pb)[:2], L.oracle_problems))
            print("[oracle] %s %s: %d problems in %.1f s" % (which, case_id, len(L.oracle_problems), time.perf_counter() - t0))
        return self._oracle[key]

    def gpu(self, which, case_id):
        """the blocking call's results (bytes, one row per problem) and what the accessor said about the launch"""
        key = (which, case_id)
        if key not in self._gpu:
            L = self.set.launch(which, CASE[case_id][1])
            res = self.ctx.sparse_align(case_options(case_id), L.problems)
            self._gpu[key] = (result_bytes(res), self.ctx.last_align_launch(), res)
        return self._gpu[key]


@pytest.fixture(scope="module")
def bench(gpu_ctx, oracle_lib):
    b = Bench(gpu_ctx, oracle_lib)
    yield b
    b.set.close()


def assert_batch_build(info, grid, n_desc):
    assert info["nt"] == 256 and info["latency"] is False and info["cluster_g"] == 0 and info["rows"] == 1 and info["rig"] is False, info
    assert info["grid"] == grid and info["n_desc"] == n_desc, (info, grid, n_desc)


def compare_with_oracle(specs, res, oracle):
    """check_run of tests/test_sparse_align_gpu.py for every problem of a launch; every mismatch is reported, none is skipped"""
    assert len(specs) == len(res) == len(oracle)
    bad, worst = [], dict(pose=0.0, alpha=0.0, beta=0.0)
    for i, (s, rg, (n, ro)) in enumerate(zip(specs, res, oracle)):
        d_pose = helpers.se3_max_abs_diff(rg.T_icur_iref, ro.T_icur_iref)
        d_alpha, d_beta = abs(rg.alpha - ro.alpha), abs(rg.beta - ro.beta)
        ok = (rg.n_fts_to_track == n and rg.status == ro.status and list(rg.iters) == list(ro.iters) and list(rg.n_meas) == list(ro.n_meas)
              and rg.n_patch_iters == ro.n_patch_iters and d_pose < TOL_POSE and d_alpha < TOL_POSE and d_beta < 1e-6)
        if s.degenerate == "no_flags":
            ok = ok and rg.status == 1 and rg.n_fts_to_track == 0
        if s.degenerate == "away":
            ok = ok and rg.n_fts_to_track > 0 and not any(rg.n_meas)
        if ok:
            worst = dict(pose=max(worst["pose"], d_pose), alpha=max(worst["alpha"], d_alpha), beta=max(worst["beta"], d_beta))
        else:
            bad.append(dict(i=i, kind=s.kind, degenerate=s.degenerate, n=[c.n_total for c in s.cams], cams=[c.kind for c in s.cams],
                            gpu=(rg.n_fts_to_track, rg.status, list(rg.iters)[:5], list(rg.n_meas)[:5], rg.n_patch_iters),
                            oracle=(n, ro.status, list(ro.iters)[:5], list(ro.n_meas)[:5], ro.n_patch_iters),
                            d_pose=d_pose, d_alpha=d_alpha, d_beta=d_beta))
    print("[parity] %d problems, %d mismatches, largest differences among the rest: %r" % (len(specs), len(bad), worst))
    assert not bad, "%d of %d problems differ from the oracle; the first: %r" % (len(bad), len(specs), bad[:5])


def test_set_premises(bench):
    """the plumbing: the oracle's pyramids are the device's; the set on this device has the sizes the legs below count on"""
    seen = bench.set.check_pyramids()
    assert set(seen) >= {"pinhole640", "radtan640", "radtan752", "small320"}
    assert bench.set.n_pairs["pinhole640"] + bench.set.n_pairs["radtan640"] >= 256
    assert len(bench.set.comp.launch("main", 8)) == 5 * bench.num_cus and len(bench.set.comp.mid) == bench.num_cus + 17


@pytest.mark.parametrize("case_id", [c[0] for c in CASES])
def test_oracle_agrees_with_itself_on_the_set(bench, case_id):
    """The premise of the comparison: the tolerances judge a kernel only where the oracle's own result does not move by more than
    them when the order of its sums changes.  Every problem of the set, with its features permuted, through the oracle again: equal
    discrete fields, pose / alpha / beta within the same tolerances.  (A scene that fails this is ill-conditioned -- a diverging
    iteration amplifies the last bit -- and is replaced in tests/align_batch_set.py, REPLACED_SCENE_SEEDS, never skipped here.)"""
    for which in ("main", "mid"):
        L = bench.set.launch(which, CASE[case_id][1])
        opt = case_options(case_id)
        with ThreadPoolExecutor(max_workers=16) as ex:
            again = list(ex.map(lambda pb: bench.orc.sparse_align_run(opt, pb)[:2], L.oracle_problems_permuted))
        bad, worst = [], 0.0
        for i, ((n, ro), (n2, rp)) in enumerate(zip(bench.oracle(which, case_id), again)):
            d = (helpers.se3_max_abs_diff(ro.T_icur_iref, rp.T_icur_iref), abs(ro.alpha - rp.alpha), abs(ro.beta - rp.beta))
            if not (n == n2 and ro.status == rp.status and list(ro.iters) == list(rp.iters) and list(ro.n_meas) == list(rp.n_meas)
                    and d[0] < TOL_POSE and d[1] < TOL_POSE and d[2] < 1e-6):
                bad.append((i, [c.seed for c in L.specs[i].cams], list(ro.iters)[:5], list(rp.iters)[:5], d))
            else:
                worst = max(worst, d[0])
        print("[oracle vs itself] %s %s: %d problems, %d not reproducible, largest pose difference among the rest %.2e" % (which, case_id, len(again), len(bad), worst))
        assert not bad, bad[:5]


@pytest.mark.parametrize("case_id", [c[0] for c in CASES])
def test_batch_against_oracle(bench, case_id):
    """3a: ONE svoh_sparse_align_batch call over the main set (>= 5 * num_cus problems on 2 * num_cus workgroups), every
    problem against the oracle; the same for the mid set (num_cus + 17 problems: the batch build, a workgroup each)."""
    for which in ("main", "mid"):
        L = bench.set.launch(which, CASE[case_id][1])
        _, info, res = bench.gpu(which, case_id)
        n = len(L.problems)
        if which == "main":
            assert n > 2 * bench.num_cus
            assert_batch_build(info, 2 * bench.num_cus, n)
        else:
            assert bench.num_cus <= n < 2 * bench.num_cus
            assert_batch_build(info, n, n)
        compare_with_oracle(L.specs, res, bench.oracle(which, case_id))


def _reordered(problems, order):
    return (capi.svoh_align_problem * len(order))(*[problems[int(i)] for i in order])


@pytest.mark.parametrize("case_id", NEIGHBOUR_CASES)
def test_result_does_not_depend_on_neighbours(bench, case_id, monkeypatch):
    """3b: the same launch twice (the workgroup-to-problem assignment differs from run to run), reversed, in a seeded random
    order, and ~20 problems of every kind each ALONE in a launch of the same build: every problem's result is the same bits."""
    ctx = bench.ctx
    L = bench.set.launch("main", 4)
    opt = case_options(case_id)
    want, info, _ = bench.gpu("main", case_id)
    n = len(L.problems)
    again = result_bytes(ctx.sparse_align(opt, L.problems))
    assert_batch_build(ctx.last_align_launch(), 2 * bench.num_cus, n)
    assert np.array_equal(again, want), np.flatnonzero((again != want).any(1))[:20]
    for order in (np.arange(n)[::-1], np.random.RandomState(77).permutation(n)):
        got = result_bytes(ctx.sparse_align(opt, _reordered(L.problems, order)))
        assert_batch_build(ctx.last_align_launch(), 2 * bench.num_cus, n)
        differ = np.flatnonzero((got != want[order]).any(1))
        assert differ.size == 0, [(int(order[k]), L.specs[int(order[k])].kind) for k in differ[:20]]
    # alone in a launch: SVOH_ALIGN_THREADS=256 + SVOH_ALIGN_LATENCY_BUILD=0 keep the batch build for a small launch; a problem of
    # 512 features or more would otherwise be spread over a cluster of workgroups (another kernel): SVOH_ALIGN_CLUSTER=0 for those
    picks = {}
    for i, s in enumerate(L.specs):
        tags = [s.kind + "/" + s.cams[0].kind if s.kind == "mono" else s.kind, "degenerate:%s" % s.degenerate, "mem:" + s.mem,
                "prior" if s.prior is not None else None, "prior_illum" if s.prior is not None and s.prior[7] > 0 else None,
                "init" if s.alpha_init != 0.0 and s.prior is None else None, "border" if s.cams[0].border and s.cams[0].invalid else None,
                "large_motion" if s.cams[0].large_motion else None, "empty_camera" if len(s.cams) > 1 and any(c.no_flags for c in s.cams) else None,
                "stereo752" if len(s.cams) == 2 and any(c.kind == "radtan752" for c in s.cams) else None]
        tags += ["n=%d" % c.n_total for c in s.cams if c.n_total in (12, 64, 65, 256, 257, 341, 513, 2000)]
        for t in tags:
            if t is not None and t not in picks:
                picks[t] = i
    alone = sorted(set(picks.values()))
    assert 15 <= len(alone) <= 40 and {"quad", "small_rig", "stereo", "degenerate:away", "degenerate:no_flags", "n=2000"} <= set(picks)
    monkeypatch.setenv("SVOH_ALIGN_THREADS", "256")
    monkeypatch.setenv("SVOH_ALIGN_LATENCY_BUILD", "0")
    for i in alone:
        if L.specs[i].n_features >= 512:
            monkeypatch.setenv("SVOH_ALIGN_CLUSTER", "0")
        else:
            monkeypatch.delenv("SVOH_ALIGN_CLUSTER", raising=False)
        ctx.reload_knobs()
        got = result_bytes(ctx.sparse_align(opt, _reordered(L.problems, [i])))
        single = ctx.last_align_launch()
        assert single["key"] == info["key"] and single["grid"] == 1 and single["n_desc"] == 1, (single, info)
        assert np.array_equal(got[0], want[i]), (i, L.specs[i].astuple())


def test_batch_build_on_one_problem(gpu_ctx, oracle_lib, monkeypatch):
    """3c: the batch build on ONE problem (SVOH_ALIGN_THREADS=256 + SVOH_ALIGN_LATENCY_BUILD=0): H and g at levels 4, 1 and 0
    within TOL_HG, the run for the option matrix of test_evaluate_and_run_option_matrix, the stereo bundle of test_stereo_bundle,
    a 752x480 radtan scene, and the committed golden fixtures."""
    orc = oracle_lib
    monkeypatch.setenv("SVOH_ALIGN_THREADS", "256")
    monkeypatch.setenv("SVOH_ALIGN_LATENCY_BUILD", "0")
    gpu_ctx.reload_knobs()

    def premise(opt, gpb):
        gpu_ctx.sparse_align(opt, gpb)
        assert_batch_build(gpu_ctx.last_align_launch(), 1, 1)

    for P in (4, 8):
        for cam in (synth.Camera.test_camera(), synth.Camera.euroc_like()):
            sc = helpers.small_scene(31, n=400, P=P, cam=cam, border_features=60, invalid_fraction=0.1)
            opb, gpb, keep = sa.both(gpu_ctx, orc, [sc])
            for illum in (0, 1):
                for robust in (0, 1):
                    for dj in (0, 1):
                        opt = _options(P, illum, robust, use_distortion_jacobian=dj)
                        premise(opt, gpb)
                        sa.check_evaluate(gpu_ctx, orc, opt, opb, gpb, (4, 1, 0))
                        sa.check_run(gpu_ctx, orc, opt, opb, gpb)
                        assert_batch_build(gpu_ctx.last_align_launch(), 1, 1)
    # the stereo bundle of test_stereo_bundle
    a = helpers.small_scene(34, n=250, border_features=30)
    b = synth.make_align_scene(34, n_features=220, cam=synth.Camera.euroc_like(), border_features=10)
    opb, gpb, keep = sa.both(gpu_ctx, orc, [a, b])
    opt = capi.default_align_options(min_level=1)
    premise(opt, gpb)
    sa.check_evaluate(gpu_ctx, orc, opt, opb, gpb, (4, 2))
    sa.check_run(gpu_ctx, orc, opt, opb, gpb)
    assert_batch_build(gpu_ctx.last_align_launch(), 1, 1)
    # a 752x480 radtan scene: level 4 is 47 x 30 pixels (88 sixteen-byte pieces and two bytes), level 2 is staged over levels 4 and 3
    w = helpers.small_scene(43, n=450, cam=synth.Camera.euroc_like(752, 480), border_features=40, gain=1.03, offset=2.0)
    opb, gpb, keep = sa.both(gpu_ctx, orc, [w])
    for opt in (_options(4, 0, 0), _options(4, 1, 1)):
        premise(opt, gpb)
        sa.check_evaluate(gpu_ctx, orc, opt, opb, gpb, (4, 1, 0))
        sa.check_run(gpu_ctx, orc, opt, opb, gpb)
        assert_batch_build(gpu_ctx.last_align_launch(), 1, 1)
    # the committed fixtures (no oracle call)
    for tag in ("pinhole", "radtan"):
        helpers.check_golden_fixtures(gpu_ctx, tag, after_run=lambda name: assert_batch_build(gpu_ctx.last_align_launch(), 1, 1))


def test_queued_batch_launches(bench):
    """3d: main, mid and main queued back to back, one fetch_all: the queue head and the control block move between launches of
    different descriptor counts; every launch delivers the bits of its blocking call."""
    ctx = bench.ctx
    case_id = "p4_illum0_robust0"
    opt = case_options(case_id)
    main, mid = bench.set.launch("main", 4), bench.set.launch("mid", 4)
    want = np.concatenate([bench.gpu("main", case_id)[0], bench.gpu("mid", case_id)[0], bench.gpu("main", case_id)[0]])
    infos = []
    for L in (main, mid, main):
        ctx.sparse_align_enqueue(opt, L.problems)
        infos.append(ctx.last_align_launch())
    got = result_bytes(ctx.sparse_align_fetch_all(2 * len(main.problems) + len(mid.problems)))
    assert_batch_build(infos[0], 2 * bench.num_cus, len(main.problems))
    assert_batch_build(infos[1], len(mid.problems), len(mid.problems))
    assert_batch_build(infos[2], 2 * bench.num_cus, len(main.problems))
    differ = np.flatnonzero((got != want).any(1))
    assert differ.size == 0, differ[:20]
