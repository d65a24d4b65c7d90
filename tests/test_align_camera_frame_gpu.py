"""The alignment kernel's camera-frame normal equations against the oracle, on scenes whose camera-IMU extrinsics are LARGE
(0.6 rad, 0.3 m: tests/camera_frame_cases.py; tests/test_align_camera_frame_cpu.py shows that a wrong frame is then 1e8 x the
tolerance off).  The kernel sums rotation-free rows and rotates the sums once per pass (rotate_sums in sparse_align.hip);
everything that reads the sums -- the step, the evaluation's H and g, a share's raw sums, a cluster's exchange -- must see
the IMU-frame sums it always saw.

640x480, 40 / 129 / 300 features (an empty second wave, a one-lane trip, a ragged last trip in the 128-thread build), 4x4 and
8x8 patches, in every build of the kernel: 128 threads, the 256-thread batch build, whatever a small launch gets by default,
two lanes per patch, the latency build.  H and g at TOL_HG, a full run at TOL_POSE with every discrete field equal."""
import numpy as np
import pytest

from svo_pro_universal_amd import _capi as capi, frontend as fe, synth

import camera_frame_cases as cfc
import helpers
import test_sparse_align_gpu as sa

pytestmark = pytest.mark.gpu

COUNTS = (40, 129, 300)   # the RAGGED_COUNTS of tests/test_align_wg128_gpu.py
LEVELS = (4, 2, 0)

# build -> (environment, what last_align_launch must say of a single-problem launch)
BUILDS = {
    "wg128": (dict(SVOH_ALIGN_THREADS="128"), dict(nt=128, rows=1, latency=False)),
    "batch256": (dict(SVOH_ALIGN_THREADS="256", SVOH_ALIGN_LATENCY_BUILD="0"), dict(nt=256, rows=1, latency=False)),
    "default": (dict(), dict()),
    "rows2": (dict(SVOH_ALIGN_THREADS="512", SVOH_ALIGN_ROWS="2"), dict(nt=512, rows=2)),
    "latency": (dict(SVOH_ALIGN_THREADS="256", SVOH_ALIGN_LATENCY_BUILD="1"), dict(nt=256, rows=1, latency=True)),
}


def force(ctx, monkeypatch, build, **more):
    env = dict(BUILDS[build][0], **more)
    for k in ("SVOH_ALIGN_THREADS", "SVOH_ALIGN_ROWS", "SVOH_ALIGN_LATENCY_BUILD", "SVOH_ALIGN_CLUSTER", "SVOH_ALIGN_WG_PER_CU"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx.reload_knobs()


def ran_in(ctx, build, **also):
    info = ctx.last_align_launch()
    for k, v in dict(BUILDS[build][1], **also).items():
        assert info[k] == v, (build, k, info)


class Problems(object):
    """the scenes of one patch size with both sides' problems; the oracle's answers are computed once per option set"""

    def __init__(self, ctx, orc, P):
        self.ctx, self.orc, self.P, self.by_name, self._oracle = ctx, orc, P, {}, {}
        for k, n in enumerate(COUNTS):
            border = (0, 9, 20)[k]
            sc = cfc.scene(7200 + 10 * P + k, n=n - border, P=P, k=k % 2, border_features=border, invalid_fraction=(0.0, 0.05, 0.1)[k],
                           gain=1.02, offset=1.5)
            assert sc.n_features == n and (sc.cam.width, sc.cam.height) == (640, 480)
            self.add("n%d" % n, [sc])
        # use_distortion_jacobian wants a camera with distortion
        self.add("radtan", [cfc.scene(7250 + P, n=129, P=P, cam=synth.Camera.euroc_like(), k=1, border_features=9)])
        # a rig of two cameras whose extrinsics differ (and differ from each other by 1 rad and half a metre)
        self.add("rig", [cfc.scene(7260 + P, n=129, P=P, k=0, border_features=9, gain=1.02, offset=1.5),
                         cfc.scene(7261 + P, n=40, P=P, cam=synth.Camera.euroc_like(), k=1, gain=1.02, offset=1.5)])

    def add(self, name, scenes):
        opb, gpb, keep = sa.both(self.ctx, self.orc, scenes)
        self.by_name[name] = (scenes, opb, gpb, keep)

    def oracle_eval(self, name, opt, key, level):
        k = (name, key, "eval", level)
        if k not in self._oracle:
            self._oracle[k] = self.orc.sparse_align_evaluate(opt, self.by_name[name][1], level)
        return self._oracle[k]

    def oracle_run(self, name, opt, key):
        k = (name, key, "run")
        if k not in self._oracle:
            self._oracle[k] = self.orc.sparse_align_run(opt, self.by_name[name][1])[:2]
        return self._oracle[k]

    def check(self, name, opt, key, levels=LEVELS):
        """H, g, visibility at `levels` (sa.check_evaluate's assertions) and a full run (sa.check_run's), against the cached oracle"""
        ctx, (_, opb, gpb, _) = self.ctx, self.by_name[name]
        worst = 0.0
        for level in levels:
            Ho, go, c2o, nmo, viso = self.oracle_eval(name, opt, key, level)
            Hg, gg, c2g, nmg, visg = ctx.sparse_align_evaluate(opt, gpb[0], level)
            assert nmo == nmg and np.array_equal(viso, visg), (name, key, level)
            dH, dg = np.abs(Hg - Ho).max() / np.abs(Ho).max(), np.abs(gg - go).max() / np.abs(go).max()
            worst = max(worst, dH, dg)
            assert dH <= helpers.TOL_HG and dg <= helpers.TOL_HG, (name, key, level, dH, dg)
            assert np.array_equal(Hg, Hg.T)
            assert abs(c2g - c2o) <= 1e-4 * abs(c2o)
        n, ro = self.oracle_run(name, opt, key)
        rg = ctx.sparse_align(opt, gpb)[0]
        d_pose = helpers.se3_max_abs_diff(rg.T_icur_iref, ro.T_icur_iref)
        print("[camera frame] %-7s P=%d %-12s H, g within %.1e of the largest entry, pose within %.1e" % (name, self.P, key, worst, d_pose))
        assert rg.n_fts_to_track == n and rg.status == ro.status
        assert list(rg.iters) == list(ro.iters) and list(rg.n_meas) == list(ro.n_meas) and rg.n_patch_iters == ro.n_patch_iters
        assert d_pose < helpers.TOL_POSE and abs(rg.alpha - ro.alpha) < helpers.TOL_POSE and abs(rg.beta - ro.beta) < 1e-6
        return rg


@pytest.fixture(scope="module")
def problems(gpu_ctx, oracle_lib):
    return {P: Problems(gpu_ctx, oracle_lib, P) for P in (4, 8)}


@pytest.mark.parametrize("P", [4, 8])
@pytest.mark.parametrize("build", sorted(BUILDS))
def test_every_build_against_the_oracle(gpu_ctx, problems, monkeypatch, build, P):
    force(gpu_ctx, monkeypatch, build)
    opt = capi.default_align_options(patch_size=P, min_level=0)
    for n in COUNTS:
        problems[P].check("n%d" % n, opt, "plain")
        ran_in(gpu_ctx, build, rig=False, cluster_g=0)


@pytest.mark.parametrize("build", ["wg128", "batch256", "default"])
def test_illumination_robust_weights_and_distortion_jacobian(gpu_ctx, problems, monkeypatch, build):
    """the illumination rows and columns go through the rotation unchanged (Q has a 2x2 identity for them); the robust
    instantiations have no gradient-only pass; use_distortion_jacobian takes the dense arm of the camera-frame rows"""
    force(gpu_ctx, monkeypatch, build)
    pb = problems[4]
    pb.check("n300", capi.default_align_options(patch_size=4, min_level=0, estimate_illumination_gain=1, estimate_illumination_offset=1), "illum")
    pb.check("n300", capi.default_align_options(patch_size=4, min_level=0, robustification=1), "robust")
    pb.check("radtan", capi.default_align_options(patch_size=4, min_level=0, use_distortion_jacobian=1), "distjac")
    pb.check("radtan", capi.default_align_options(patch_size=4, min_level=0, use_distortion_jacobian=1, estimate_illumination_gain=1,
                                                  estimate_illumination_offset=1), "distjac_illum")
    ran_in(gpu_ctx, build)


@pytest.mark.parametrize("P", [4, 8])
@pytest.mark.parametrize("build", ["default", "batch256", "rows2", "cluster"])
def test_rig_of_two_cameras(gpu_ctx, problems, monkeypatch, build, P):
    """a lane's sums mix the cameras: camera 1's rows are turned into camera 0's frame, the pass's one rotation is camera 0's.
    By default a small launch of a rig runs its cameras side by side (the rig build); the 256-thread batch build takes rigs and
    single cameras alike; in a cluster every share rotates before the shares are added."""
    if build == "cluster":
        force(gpu_ctx, monkeypatch, "default", SVOH_ALIGN_CLUSTER="2")
    else:
        force(gpu_ctx, monkeypatch, build)
    for kw, key in ((dict(), "plain"), (dict(estimate_illumination_gain=1, estimate_illumination_offset=1), "illum")):
        problems[P].check("rig", capi.default_align_options(patch_size=P, min_level=0, **kw), key)
    info = gpu_ctx.last_align_launch()
    if build == "cluster":
        assert info["cluster_g"] == 2, info
    elif build == "default":
        assert info["rig"] is True, info
    elif build == "batch256":
        ran_in(gpu_ctx, build, rig=False, cluster_g=0)
    else:
        ran_in(gpu_ctx, build, cluster_g=0)   # (two lanes per patch: the cameras take turns, whatever the key says of side by side)


@pytest.mark.parametrize("n_workgroups", [1, 3])
def test_rig_patch_split(gpu_ctx, problems, n_workgroups):
    """the raw sums of a share (svoh_sparse_align_partial_sums) are IMU-frame sums: the split iteration over the rig, whole and
    with one camera per participant, ends where the oracle does"""
    from test_split_align_gpu import run_split
    pb = problems[4]
    scenes, opb, gpb, _ = pb.by_name["rig"]
    cams = [(sc, gpb[0].cams[c].ref_frame, gpb[0].cams[c].cur_frame) for c, sc in enumerate(scenes)]
    opt = capi.default_align_options(patch_size=4, min_level=1)
    n, ro = pb.oracle_run("rig", opt, "split")
    for shares in ([cams], [[cams[0]], [cams[1]]]):
        res = run_split(gpu_ctx, opt, shares, n_workgroups=n_workgroups)
        assert res.status == ro.status and res.iters == list(ro.iters) and res.n_meas == list(ro.n_meas)
        assert helpers.se3_max_abs_diff(res.state.T_icur_iref, ro.T_icur_iref) < helpers.TOL_POSE


@pytest.mark.parametrize("kind", ["single_camera", "with_rigs"])
def test_a_workgroups_second_problem(gpu_ctx, problems, monkeypatch, kind):
    """num_cus + 40 problems, one workgroup per compute unit: 40 workgroups take a second problem, whose camera constants
    (R_imu_cam, tau, a rig's camera-to-camera-0 rotation) must be its own.  Problems of two different extrinsics in turn --
    and, in the 256-thread batch build, rigs and single cameras in turn."""
    import torch
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    pb = problems[4]
    names = ["n40", "n129", "n300"] + (["rig"] if kind == "with_rigs" else [])
    opt = capi.default_align_options(patch_size=4, min_level=1)
    items, expect = [], []
    for i in range(num_cus + 40):
        name = names[i % len(names)]
        scenes, _, gpb, _ = pb.by_name[name]
        items.append([(sc, gpb[0].cams[c].ref_frame, gpb[0].cams[c].cur_frame) for c, sc in enumerate(scenes)])
        expect.append(pb.oracle_run(name, opt, "level1"))
    pbs, keep = fe.make_align_problems(items)
    force(gpu_ctx, monkeypatch, "wg128", SVOH_ALIGN_WG_PER_CU="1")   # (a launch with a rig in it cannot take the 128-thread build)
    res = gpu_ctx.sparse_align(opt, pbs)
    info = gpu_ctx.last_align_launch()
    assert info["nt"] == (128 if kind == "single_camera" else 256) and info["latency"] is False and info["rig"] is False, info
    assert info["grid"] == num_cus and info["n_desc"] == num_cus + 40, info
    bad = []
    for i, (rg, (n, ro)) in enumerate(zip(res, expect)):
        d = helpers.se3_max_abs_diff(rg.T_icur_iref, ro.T_icur_iref)
        if not (rg.n_fts_to_track == n and rg.status == ro.status and list(rg.iters) == list(ro.iters) and list(rg.n_meas) == list(ro.n_meas)
                and rg.n_patch_iters == ro.n_patch_iters and d < helpers.TOL_POSE):
            bad.append((i, names[i % len(names)], d, list(rg.iters)[:5], list(ro.iters)[:5]))
    assert not bad, bad[:5]


def _turned(T, angle=0.0, shift=0.0):
    q = synth.quat_mul(synth.quat_from_axis_angle([0.3, 0.5, -0.8], angle), T.q) if angle else T.q
    return synth.SE3(q, np.asarray(T.t, np.float64) + [shift, 0.0, 0.0])


@pytest.mark.parametrize("what", ["rotation", "translation"])
def test_an_inconsistent_extrinsics_pair_is_refused(gpu_ctx, problems, what):
    """ref_T_cam_imu must be the inverse of ref_T_imu_cam (include/svo_hip.h): R_cam_imu turned by 1e-6 rad, or its translation
    off by 1e-6 m, is refused with the invalid-argument status by every entry that takes an alignment problem -- and the same
    problem with the pair put right runs."""
    scenes, opb, gpb, _ = problems[4].by_name["n129"]
    sc = scenes[0]
    opt = capi.default_align_options(patch_size=4, min_level=2)
    good = fe._se3(sc.T_cam_imu)
    gpb[0].cams[0].ref_T_cam_imu = fe._se3(_turned(sc.T_cam_imu, angle=1e-6) if what == "rotation" else _turned(sc.T_cam_imu, shift=1e-6))
    try:
        for call in (lambda: gpu_ctx.sparse_align(opt, gpb), lambda: gpu_ctx.sparse_align_enqueue(opt, gpb),
                     lambda: gpu_ctx.sparse_align_evaluate(opt, gpb[0], 2)):
            with pytest.raises(fe.SvohError) as e:
                call()
            assert e.value.code == capi.SVOH_ERR_INVALID_ARGUMENT
    finally:
        gpb[0].cams[0].ref_T_cam_imu = good
    assert gpu_ctx.sparse_align(opt, gpb)[0].status == 0
