"""Parity tests proper: the HIP path, called through the C ABI, against the CPU
oracle on the same seeded inputs, against the committed golden fixtures, and --
at BASELINE's full size -- through size-independent properties.

Tolerances (fp64 on both sides; only the summation order of the normal
equations and FMA contraction differ):
  H, g            relative 1e-10 of the largest entry
  visibility, n_meas, iteration counts, selection   exact
  final pose / alpha / beta    1e-8 absolute (observed ~1e-15)
  chi2            relative 1e-4 (the reference accumulates it in float; we use fp64)
"""
import ctypes as C

import numpy as np
import pytest

from svo_pro_universal_amd import _capi as capi, frontend as fe, synth

import helpers

pytestmark = pytest.mark.gpu

TOL_HG = helpers.TOL_HG      # 1e-10
TOL_POSE = helpers.TOL_POSE  # 1e-8


def both(gpu_ctx, orc, scenes, n_levels=5, **mk):
    """Build the oracle problem and the device problem for a list of cameras."""
    cams_o, cams_g = [], []
    for sc in scenes:
        ref, cur = helpers.scene_pyramids(orc, sc, n_levels)
        fr, lv = gpu_ctx.build_pyramid(sc.img_ref, n_levels, return_levels=True)
        fc = gpu_ctx.build_pyramid(sc.img_cur, n_levels)
        for a, b in zip(lv, ref):
            assert np.array_equal(a, b)
        cams_o.append((sc, ref, cur))
        cams_g.append((sc, fr, fc))
    opb = orc.problem_from_scenes(cams_o, **mk)
    gpb, keep = fe.make_align_problems([cams_g], **mk)
    return opb, gpb, keep


def check_evaluate(gpu_ctx, orc, opt, opb, gpb, levels):
    for level in levels:
        Ho, go, c2o, nmo, viso = orc.sparse_align_evaluate(opt, opb, level)
        Hg, gg, c2g, nmg, visg = gpu_ctx.sparse_align_evaluate(opt, gpb[0], level)
        assert nmo == nmg and np.array_equal(viso, visg)
        assert np.abs(Hg - Ho).max() <= TOL_HG * np.abs(Ho).max()
        assert np.abs(gg - go).max() <= TOL_HG * np.abs(go).max()
        assert np.array_equal(Hg, Hg.T)
        if nmo:
            assert abs(c2g - c2o) <= 1e-4 * abs(c2o)


def check_run(gpu_ctx, orc, opt, opb, gpb):
    n, ro, _ = orc.sparse_align_run(opt, opb)
    rg = gpu_ctx.sparse_align(opt, gpb)[0]
    assert rg.n_fts_to_track == n and rg.status == ro.status
    assert list(rg.iters) == list(ro.iters) and list(rg.n_meas) == list(ro.n_meas)
    assert rg.n_patch_iters == ro.n_patch_iters
    assert helpers.se3_max_abs_diff(rg.T_icur_iref, ro.T_icur_iref) < TOL_POSE
    assert abs(rg.alpha - ro.alpha) < TOL_POSE and abs(rg.beta - ro.beta) < 1e-6
    return rg, ro


@pytest.mark.parametrize("P", [4, 8])
@pytest.mark.parametrize("cam_kind", ["pinhole", "radtan"])
def test_evaluate_and_run_option_matrix(gpu_ctx, oracle_lib, P, cam_kind):
    orc = oracle_lib
    cam = synth.Camera.test_camera() if cam_kind == "pinhole" else synth.Camera.euroc_like()
    sc = helpers.small_scene(31, n=400, P=P, cam=cam, border_features=60, invalid_fraction=0.1)
    opb, gpb, keep = both(gpu_ctx, orc, [sc])
    for illum in (0, 1):
        for robust in (0, 1):
            for dj in (0, 1):
                opt = capi.default_align_options(patch_size=P, min_level=0, estimate_illumination_gain=illum,
                                                 estimate_illumination_offset=illum, robustification=robust,
                                                 use_distortion_jacobian=dj)
                check_evaluate(gpu_ctx, orc, opt, opb, gpb, (4, 1, 0))
                check_run(gpu_ctx, orc, opt, opb, gpb)


def test_only_gain_or_only_offset(gpu_ctx, oracle_lib):
    orc = oracle_lib
    sc = helpers.small_scene(32, n=300, gain=1.05, offset=3.0)
    opb, gpb, keep = both(gpu_ctx, orc, [sc])
    for ga, of in ((1, 0), (0, 1)):
        opt = capi.default_align_options(min_level=1, estimate_illumination_gain=ga, estimate_illumination_offset=of)
        check_evaluate(gpu_ctx, orc, opt, opb, gpb, (3,))
        check_run(gpu_ctx, orc, opt, opb, gpb)


def test_handler_levels_and_iteration_caps(gpu_ctx, oracle_lib):
    """FrameHandlerBase uses levels 4..2 (svo_factory.cpp:137-138); also max_iter 1 and a huge eps."""
    orc = oracle_lib
    sc = helpers.small_scene(33, n=180)
    opb, gpb, keep = both(gpu_ctx, orc, [sc])
    for kw in (dict(min_level=2), dict(min_level=0, max_iter=1), dict(min_level=3, eps=10.0),
               dict(max_level=2, min_level=2, max_iter=30, eps=1e-9)):
        opt = capi.default_align_options(**kw)
        rg, ro = check_run(gpu_ctx, orc, opt, opb, gpb)
        assert max(rg.iters) <= opt.max_iter


def test_stereo_bundle(gpu_ctx, oracle_lib):
    """Two cameras with different extrinsics and features: one H/g summed over cameras
    (sparse_img_align.cpp:138-154)."""
    orc = oracle_lib
    a = helpers.small_scene(34, n=250, border_features=30)
    b = synth.make_align_scene(34, n_features=220, cam=synth.Camera.euroc_like(), border_features=10)
    # second camera: same motion of the rig, different camera-imu extrinsics
    opb, gpb, keep = both(gpu_ctx, orc, [a, b])
    opt = capi.default_align_options(min_level=1)
    check_evaluate(gpu_ctx, orc, opt, opb, gpb, (4, 2))
    check_run(gpu_ctx, orc, opt, opb, gpb)


@pytest.mark.parametrize("sizes", [(70, 130, 20), (125, 125), (160, 150), (129, 3), (40, 0, 90), (300, 200)])
def test_rig_cameras_side_by_side(gpu_ctx, oracle_lib, sizes):
    """Round 4: in a launch of a few problems the cameras of a rig run side by side, camera c on the waves behind camera
    c-1's, when their patches fit the workgroup together (sparse_align_kernel<..., RIG>: the 256-thread latency build and
    the 512-thread geometry) -- and take turns when they do not (the last case).  Unequal cameras, three cameras, a camera
    without features, gain + offset with a prior: against the oracle, like every other bundle."""
    orc = oracle_lib
    cams = [helpers.small_scene(500 + k, n=max(n, 1), border_features=min(6, n // 4), gain=1.02, offset=1.5) if k != 1 else
            synth.make_align_scene(500 + k, n_features=max(n, 1), cam=synth.Camera.euroc_like(), border_features=min(6, n // 4), gain=1.02, offset=1.5)
            for k, n in enumerate(sizes)]
    for sc, n in zip(cams, sizes):
        if n == 0: sc.flags[:] = 0      # a camera whose every feature is unusable
    Tp = synth.SE3(synth.quat_from_axis_angle([0.2, -1, 0.3], 0.003), [0.002, -0.001, 0.001])
    prior = helpers.make_prior(Tp, 0.5, 0.2)
    opb, gpb, keep = both(gpu_ctx, orc, cams, prior=prior)
    for kw in (dict(min_level=2), dict(min_level=1, estimate_illumination_gain=1, estimate_illumination_offset=1)):
        opt = capi.default_align_options(**kw)
        check_evaluate(gpu_ctx, orc, opt, opb, gpb, (4, 2))
        check_run(gpu_ctx, orc, opt, opb, gpb)


def test_prior(gpu_ctx, oracle_lib):
    orc = oracle_lib
    sc = helpers.small_scene(35, n=300, gain=1.02, offset=1.0)
    Tp = synth.SE3(synth.quat_from_axis_angle([0.3, -1, 0.2], 0.004), [0.003, -0.002, 0.001])
    for lam_r, lam_t, la, lb in ((0.5, 0.0, 0.0, 0.0), (2.0, 3.0, 0.0, 0.0), (0.1, 0.1, 0.5, 0.5)):
        prior = helpers.make_prior(Tp, lam_r, lam_t, alpha=0.01, beta=-0.5, lambda_alpha=la, lambda_beta=lb)
        opb, gpb, keep = both(gpu_ctx, orc, [sc], prior=prior)
        opt = capi.default_align_options(min_level=1, estimate_illumination_gain=int(la > 0),
                                         estimate_illumination_offset=int(la > 0))
        check_run(gpu_ctx, orc, opt, opb, gpb)


def test_no_features_and_all_invisible(gpu_ctx, oracle_lib):
    orc = oracle_lib
    sc = helpers.small_scene(36, n=120)
    sc.flags[:] = 0
    opb, gpb, keep = both(gpu_ctx, orc, [sc])
    opt = capi.default_align_options()
    rg, ro = check_run(gpu_ctx, orc, opt, opb, gpb)
    assert rg.status == 1 and rg.n_fts_to_track == 0
    assert helpers.se3_max_abs_diff(rg.T_icur_iref, gpb[0].T_icur_iref) == 0.0
    # selected but invisible: start from a pose that looks away -> H = 0, zero step, converged
    sc = helpers.small_scene(36, n=120)
    away = synth.SE3(synth.quat_from_axis_angle([0, 1, 0], 2.5), [0, 0, 0])
    opb, gpb, keep = both(gpu_ctx, orc, [sc], T_init=away)
    check_evaluate(gpu_ctx, orc, opt, opb, gpb, (4,))
    rg, ro = check_run(gpu_ctx, orc, opt, opb, gpb)
    assert list(rg.n_meas)[:5] == [0, 0, 0, 0, 0]


def test_ragged_batch_equals_singles(gpu_ctx, oracle_lib):
    """A batch of problems of very different sizes (12 ... 2000 features, mixed cameras)
    gives exactly the per-problem results."""
    orc = oracle_lib
    sizes = [12, 33, 64, 65, 300, 2000, 513]  # (a single patch gives a rank-2 H: ill-posed, no parity to check)
    items, singles = [], []
    opt = capi.default_align_options(min_level=1)
    for k, n in enumerate(sizes):
        cam = synth.Camera.euroc_like() if k % 2 else synth.Camera.test_camera()
        sc = helpers.small_scene(40 + k, n=n, cam=cam)
        opb, gpb, keep = both(gpu_ctx, orc, [sc])
        items.append([(sc, gpb[0].cams[0].ref_frame, gpb[0].cams[0].cur_frame)])
        singles.append(orc.sparse_align_run(opt, opb)[1])
    pbs, keep = fe.make_align_problems(items)
    res = gpu_ctx.sparse_align(opt, pbs)
    for rg, ro in zip(res, singles):
        assert rg.n_fts_to_track == ro.n_fts_to_track and list(rg.iters) == list(ro.iters)
        assert helpers.se3_max_abs_diff(rg.T_icur_iref, ro.T_icur_iref) < TOL_POSE


@pytest.mark.parametrize("nt,rows", [("256", "0"), ("512", "0"), ("512", "2"), ("512", "4"), ("512", "8")])
def test_all_workgroup_geometries(gpu_ctx, oracle_lib, nt, rows, monkeypatch):
    """One lane per patch (256 / 512 threads) and the rows geometry (2, 4 or -- 8x8 patches -- 8 lanes per patch, 512
    threads) against the oracle.  (A small single problem runs in the rows geometry by default, so the other tests of this
    file exercise it too.)"""
    orc = oracle_lib
    monkeypatch.setenv("SVOH_ALIGN_THREADS", nt)
    monkeypatch.setenv("SVOH_ALIGN_ROWS", rows)
    gpu_ctx.reload_knobs()
    sc = helpers.small_scene(37, n=700, border_features=50)
    opb, gpb, keep = both(gpu_ctx, orc, [sc])
    for lds in ("0", "38400", "153856"):  # global gathers only / levels>=2 in LDS / levels>=1 in LDS
        monkeypatch.setenv("SVOH_ALIGN_LDS", lds)
        gpu_ctx.reload_knobs()
        opt = capi.default_align_options(min_level=0)
        check_evaluate(gpu_ctx, orc, opt, opb, gpb, (4, 1, 0))
        check_run(gpu_ctx, orc, opt, opb, gpb)
    # 8x8 patches, illumination terms, stereo and a radtan camera through the same geometry (the 256-thread one
    # brings the workspace rows in by LDS-DMA and reads 11- / 9-pixel footprint rows as 16-byte loads)
    monkeypatch.setenv("SVOH_ALIGN_LDS", "38400")
    gpu_ctx.reload_knobs()
    a = helpers.small_scene(41, n=400, P=8, border_features=30)
    b = synth.make_align_scene(42, n_features=333, patch_size=8, cam=synth.Camera.euroc_like(), border_features=10, gain=1.05, offset=4.0)
    opb2, gpb2, keep2 = both(gpu_ctx, orc, [a, b])
    for kw in (dict(), dict(estimate_illumination_gain=1, estimate_illumination_offset=1), dict(robustification=1)):
        opt = capi.default_align_options(min_level=0, patch_size=8, **kw)
        check_evaluate(gpu_ctx, orc, opt, opb2, gpb2, (3, 0))
        check_run(gpu_ctx, orc, opt, opb2, gpb2)


@pytest.mark.parametrize("rows", [None, "0", "2", "4"])
def test_small_stereo_bundle_with_prior_in_every_lane_geometry(gpu_ctx, oracle_lib, rows, monkeypatch):
    """Round 4's small-problem paths together: a stereo bundle of 2 x ~60 features (the workspace rows of both cameras live
    in LDS, the default geometry gives such a problem two lanes per patch), gain + offset estimated, a rotation /
    translation / illumination prior (the wave-wide Gauss-Newton step with lane 0's prior part, eight parameters, one
    camera pose per lane) -- against the oracle, in the default geometry and with the lanes per patch forced."""
    orc = oracle_lib
    if rows is not None:
        monkeypatch.setenv("SVOH_ALIGN_ROWS", rows)
        gpu_ctx.reload_knobs()
    a = helpers.small_scene(141, n=64, border_features=8, gain=1.03, offset=2.0)
    b = synth.make_align_scene(141, n_features=58, cam=synth.Camera.euroc_like(), border_features=6, gain=1.03, offset=2.0)
    Tp = synth.SE3(synth.quat_from_axis_angle([0.2, -1, 0.3], 0.003), [0.002, -0.001, 0.001])
    prior = helpers.make_prior(Tp, 0.5, 0.2, alpha=0.02, beta=-0.3, lambda_alpha=0.3, lambda_beta=0.3)
    opb, gpb, keep = both(gpu_ctx, orc, [a, b], prior=prior)
    for kw in (dict(min_level=2), dict(min_level=0, robustification=1)):
        opt = capi.default_align_options(estimate_illumination_gain=1, estimate_illumination_offset=1, **kw)
        check_evaluate(gpu_ctx, orc, opt, opb, gpb, (4, 2))
        check_run(gpu_ctx, orc, opt, opb, gpb)
    # the same bundle with 8x8 patches (up to eight lanes per patch)
    a8 = helpers.small_scene(142, n=30, P=8, border_features=4)
    opb8, gpb8, keep8 = both(gpu_ctx, orc, [a8])
    opt8 = capi.default_align_options(patch_size=8, min_level=1)
    check_evaluate(gpu_ctx, orc, opt8, opb8, gpb8, (3, 1))
    check_run(gpu_ctx, orc, opt8, opb8, gpb8)


def test_device_resident_inputs(gpu_ctx, oracle_lib):
    import torch
    orc = oracle_lib
    sc = helpers.small_scene(38, n=256)
    opb, gpb, keep = both(gpu_ctx, orc, [sc])
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (sc.px, sc.f, sc.pos_world, sc.flags)]
    torch.cuda.synchronize()
    dp = dict(px=t[0].data_ptr(), f=t[1].data_ptr(), pos_world=t[2].data_ptr(), flags=t[3].data_ptr())
    pbs, keep2 = fe.make_align_problems([[(sc, gpb[0].cams[0].ref_frame, gpb[0].cams[0].cur_frame, dp)]])
    opt = capi.default_align_options()
    check_run(gpu_ctx, orc, opt, opb, pbs)


@pytest.mark.parametrize("tag", ["pinhole", "radtan"])
def test_golden_fixtures(gpu_ctx, tag):
    """HIP path vs the committed fixtures (no oracle call)."""
    helpers.check_golden_fixtures(gpu_ctx, tag)


def test_full_size_properties(gpu_ctx):
    """BASELINE configs[1] size (2000 patches, 640x480, levels 4..0), 8 frame pairs:
    size-independent properties only -- ground-truth pose recovery, determinism,
    invariance to a permutation of the features, batch == single."""
    cam = synth.Camera.test_camera()
    scenes = [synth.make_align_scene(100 + i, n_features=2000, cam=cam) for i in range(8)]
    items = []
    for sc in scenes:
        items.append([(sc, gpu_ctx.build_pyramid(sc.img_ref, 5), gpu_ctx.build_pyramid(sc.img_cur, 5))])
    opt = capi.default_align_options(min_level=0)
    pbs, keep = fe.make_align_problems(items)
    r1 = gpu_ctx.sparse_align(opt, pbs)
    r2 = gpu_ctx.sparse_align(opt, pbs)
    for a, b, sc in zip(r1, r2, scenes):
        assert a.status == 0 and a.n_fts_to_track == 2000
        assert helpers.se3_max_abs_diff(a.T_icur_iref, b.T_icur_iref) == 0.0  # bitwise repeatable
        e0 = synth.se3_error(sc.T_icur_iref_init, sc.T_icur_iref_gt)
        e1 = synth.se3_error(synth.SE3.from7(fe.se3_to_numpy(a.T_icur_iref)), sc.T_icur_iref_gt)
        assert e1[0] < 0.05 * e0[0] + 1e-4 and e1[1] < 0.05 * e0[1] + 3e-4, (e0, e1)
    # permuting the features changes only the summation order
    sc = scenes[0]
    perm = np.random.RandomState(0).permutation(sc.n_features)
    sp = synth.make_align_scene(100, n_features=2000, cam=cam, render_images=False)
    sp.px = sc.px.reshape(-1, 2)[perm].ravel(); sp.f = sc.f.reshape(-1, 3)[perm].ravel()
    sp.pos_world = sc.pos_world.reshape(-1, 3)[perm].ravel(); sp.flags = sc.flags[perm]
    pp, keep2 = fe.make_align_problems([[(sp, items[0][0][1], items[0][0][2])]])
    rp = gpu_ctx.sparse_align(opt, pp)[0]
    assert list(rp.iters) == list(r1[0].iters)
    assert helpers.se3_max_abs_diff(rp.T_icur_iref, r1[0].T_icur_iref) < 1e-9


def test_normal_equations_are_additive_over_patch_shards(gpu_ctx):
    """The sharding rule of SURVEY.md 8(e): H, g, chi2*n and n_meas of a frame are the sums of the same
    quantities over any partition of its patches (what a patch-split all-reduce would add up), at full size."""
    cam = synth.Camera.test_camera()
    sc = synth.make_align_scene(120, n_features=2000, cam=cam)
    fr, fc = gpu_ctx.build_pyramid(sc.img_ref, 5), gpu_ctx.build_pyramid(sc.img_cur, 5)
    opt = capi.default_align_options(estimate_illumination_gain=1, estimate_illumination_offset=1)
    flags0 = sc.flags.copy()
    rng = np.random.RandomState(5)
    owner = rng.randint(0, 4, sc.n_features)          # 4 "ranks"
    for level in (4, 2, 0):
        pb, keep = fe.make_align_problems([[(sc, fr, fc)]])
        H, g, chi2, nm, vis = gpu_ctx.sparse_align_evaluate(opt, pb[0], level)
        Hs, gs, cs, ns = np.zeros((8, 8)), np.zeros(8), 0.0, 0
        for r in range(4):
            sc.flags = (flags0 * (owner == r)).astype(np.uint8)
            pbr, keepr = fe.make_align_problems([[(sc, fr, fc)]])
            Hr, gr, cr, nr, vr = gpu_ctx.sparse_align_evaluate(opt, pbr[0], level)
            Hs += Hr; gs += gr; cs += cr * nr; ns += nr
        sc.flags = flags0
        assert ns == nm and nm > 0
        assert np.abs(Hs - H).max() <= 1e-11 * np.abs(H).max()
        assert np.abs(gs - g).max() <= 1e-11 * np.abs(g).max()
        assert abs(cs - chi2 * nm) <= 1e-11 * chi2 * nm


def test_error_codes(gpu_ctx):
    sc = helpers.small_scene(39, n=50)
    fr = gpu_ctx.build_pyramid(sc.img_ref, 3)
    gpb, keep = fe.make_align_problems([[(sc, fr, fr)]])
    with pytest.raises(fe.SvohError) as e:  # pyramid too shallow for max_level 4
        gpu_ctx.sparse_align(capi.default_align_options(), gpb)
    assert e.value.code == -1 and "levels" in str(e.value)
    with pytest.raises(fe.SvohError) as e:
        gpu_ctx.sparse_align(capi.default_align_options(patch_size=5, max_level=2, min_level=1), gpb)
    assert e.value.code == -5
    gpb[0].cams[0].ref_frame = 987654321
    with pytest.raises(fe.SvohError) as e:
        gpu_ctx.sparse_align(capi.default_align_options(max_level=2, min_level=1), gpb)
    assert e.value.code == -4
    with pytest.raises(fe.SvohError):
        gpu_ctx.release_frame(987654321)


@pytest.mark.parametrize("n,cluster", [(2000, None), (1500, 3), (700, 2), (4000, 16)])
def test_cluster_mode_single_problem(gpu_ctx, oracle_lib, n, cluster):
    """One problem spread over several co-resident workgroups (device-side barrier per iteration; automatic from
    512 features, SVOH_ALIGN_CLUSTER forces a size): same iteration counts and pose as the oracle and as the
    one-workgroup kernel (summation order differs: 1e-9)."""
    import os
    orc = oracle_lib
    sc = helpers.small_scene(81, n=n, border_features=100, invalid_fraction=0.05)
    opb, gpb, keep = both(gpu_ctx, orc, [sc])
    opt = capi.default_align_options(min_level=0)
    old = os.environ.get("SVOH_ALIGN_CLUSTER")
    try:
        os.environ["SVOH_ALIGN_CLUSTER"] = "0"
        gpu_ctx.reload_knobs()
        single = gpu_ctx.sparse_align(opt, gpb)[0]
        if cluster is None:
            del os.environ["SVOH_ALIGN_CLUSTER"]
            gpu_ctx.reload_knobs()
        else:
            os.environ["SVOH_ALIGN_CLUSTER"] = str(cluster)
            gpu_ctx.reload_knobs()
        rg, ro = check_run(gpu_ctx, orc, opt, opb, gpb)
        assert rg.status == 0 and list(rg.iters) == list(single.iters) and rg.n_fts_to_track == single.n_fts_to_track
        assert rg.n_patch_iters == single.n_patch_iters
        assert helpers.se3_max_abs_diff(rg.T_icur_iref, single.T_icur_iref) < 1e-9
        # illumination terms + prior + stereo through the cluster path
        b = synth.make_align_scene(81, n_features=n // 2, cam=synth.Camera.euroc_like(), border_features=10)
        Tp = synth.SE3(synth.quat_from_axis_angle([0.3, -1, 0.2], 0.004), [0.003, -0.002, 0.001])
        prior = helpers.make_prior(Tp, 0.5, 0.3)
        opb2, gpb2, keep2 = both(gpu_ctx, orc, [sc, b], prior=prior)
        opt2 = capi.default_align_options(min_level=1, estimate_illumination_gain=1, estimate_illumination_offset=1)
        check_run(gpu_ctx, orc, opt2, opb2, gpb2)
    finally:
        if old is None:
            os.environ.pop("SVOH_ALIGN_CLUSTER", None)
            gpu_ctx.reload_knobs()
        else:
            os.environ["SVOH_ALIGN_CLUSTER"] = old
            gpu_ctx.reload_knobs()


def test_cluster_mode_small_batch_of_large_problems(gpu_ctx, oracle_lib):
    """A few large problems in one call: each gets its own cluster of workgroups (own exchange slots and
    arrival counter); the results are those of the one-workgroup kernel problem by problem."""
    import os
    orc = oracle_lib
    scenes = [helpers.small_scene(90 + k, n=n, border_features=40) for k, n in enumerate((900, 1500, 700))]
    items, oracle_pbs = [], []
    for sc in scenes:
        fr, fc = gpu_ctx.build_pyramid(sc.img_ref, 5), gpu_ctx.build_pyramid(sc.img_cur, 5)
        items.append([(sc, fr, fc)])
        ref, cur = helpers.scene_pyramids(orc, sc, 5)
        oracle_pbs.append(orc.problem_from_scenes([(sc, ref, cur)]))
    gpb, keep = fe.make_align_problems(items)
    opt = capi.default_align_options(min_level=1)
    old = os.environ.get("SVOH_ALIGN_CLUSTER")
    try:
        os.environ["SVOH_ALIGN_CLUSTER"] = "0"
        gpu_ctx.reload_knobs()
        single = gpu_ctx.sparse_align(opt, gpb)
        single = [(list(r.iters), r.n_fts_to_track, fe.se3_to_numpy(r.T_icur_iref)) for r in single]
        os.environ.pop("SVOH_ALIGN_CLUSTER")
        gpu_ctx.reload_knobs()
        clustered = gpu_ctx.sparse_align(opt, gpb)
        for r, (it, nf, T), opb in zip(clustered, single, oracle_pbs):
            assert r.status == 0 and list(r.iters) == it and r.n_fts_to_track == nf
            assert np.abs(fe.se3_to_numpy(r.T_icur_iref) - T).max() < 1e-9
            n, ro, _ = orc.sparse_align_run(opt, opb)
            assert n == r.n_fts_to_track and list(ro.iters) == list(r.iters) and list(ro.n_meas) == list(r.n_meas)
            assert helpers.se3_max_abs_diff(r.T_icur_iref, ro.T_icur_iref) < TOL_POSE
    finally:
        if old is None:
            os.environ.pop("SVOH_ALIGN_CLUSTER", None)
            gpu_ctx.reload_knobs()
        else:
            os.environ["SVOH_ALIGN_CLUSTER"] = old
            gpu_ctx.reload_knobs()


@pytest.mark.parametrize("seed", [48, 52, 53, 56])
def test_visibility_changes_inside_a_level(gpu_ctx, oracle_lib, seed):
    """Scenes whose set of visible patches changes between iterations of the same level (the oracle's trace says
    so): the kernel's gradient-only passes must notice, repeat the iteration with a fresh Hessian and end exactly
    where the every-iteration recomputation ends -- with one workgroup and with a cluster of three."""
    import os
    orc = oracle_lib
    sc = helpers.small_scene(seed, n=300, border_features=300, rot_deg=(1.5, 3.0), trans_m=(0.05, 0.12))
    opb, gpb, keep = both(gpu_ctx, orc, [sc])
    opt = capi.default_align_options(min_level=0)
    n, ro, tr = orc.sparse_align_run(opt, opb, trace_capacity=80)
    lv, nm = tr["level"], tr["n_meas"]
    assert any(lv[k] == lv[k - 1] and nm[k] != nm[k - 1] for k in range(1, len(lv)))   # the premise of the test
    old = os.environ.get("SVOH_ALIGN_CLUSTER")
    try:
        for g in ("0", "3"):
            os.environ["SVOH_ALIGN_CLUSTER"] = g
            gpu_ctx.reload_knobs()
            check_run(gpu_ctx, orc, opt, opb, gpb)
    finally:
        if old is None:
            os.environ.pop("SVOH_ALIGN_CLUSTER", None)
            gpu_ctx.reload_knobs()
        else:
            os.environ["SVOH_ALIGN_CLUSTER"] = old
            gpu_ctx.reload_knobs()


def test_kernel_timing_is_a_switch(gpu_ctx):
    """The library's default is no event pair around a launch (svoh_set_kernel_timing, include/svo_hip.h): the *_kernel_ms
    calls then refuse instead of reporting a stale time, results are the same either way."""
    import ctypes as C
    sc = helpers.small_scene(91, n=150)
    gpb, keep = fe.make_align_problems([[(sc, gpu_ctx.build_pyramid(sc.img_ref, 5), gpu_ctx.build_pyramid(sc.img_cur, 5))]])
    opt = capi.default_align_options(min_level=2)
    timed = fe.se3_to_numpy(gpu_ctx.sparse_align(opt, gpb)[0].T_icur_iref)
    ms = C.c_float()
    assert gpu_ctx.lib.svoh_sparse_align_last_kernel_ms(gpu_ctx.h, C.byref(ms)) == 0 and 0.0 < ms.value < 50.0
    fresh = fe.Context(0, kernel_timing=False)
    try:
        gpb2, keep2 = fe.make_align_problems([[(sc, fresh.build_pyramid(sc.img_ref, 5), fresh.build_pyramid(sc.img_cur, 5))]])
        untimed = fe.se3_to_numpy(fresh.sparse_align(opt, gpb2)[0].T_icur_iref)
        assert np.array_equal(untimed, timed)
        assert fresh.lib.svoh_sparse_align_last_kernel_ms(fresh.h, C.byref(ms)) != 0
        assert b"svoh_set_kernel_timing" in fresh.lib.svoh_last_error_string(fresh.h)
        assert fresh.lib.svoh_last_kernel_ms(fresh.h, C.byref(ms)) != 0
        fresh.set_kernel_timing(True)
        fresh.sparse_align(opt, gpb2)
        assert fresh.lib.svoh_sparse_align_last_kernel_ms(fresh.h, C.byref(ms)) == 0 and ms.value > 0.0
    finally:
        fresh.close()


def test_queued_launches_and_kernel_time_history(gpu_ctx):
    """Several enqueue calls before one fetch: the last launch's results are handed out, every launch's device
    time can be read afterwards (the library keeps the last 32 event pairs)."""
    import ctypes as C
    scs = [helpers.small_scene(95 + k, n=200) for k in range(3)]
    items = []
    for sc in scs:
        items.append([(sc, gpu_ctx.build_pyramid(sc.img_ref, 5), gpu_ctx.build_pyramid(sc.img_cur, 5))])
    gpb, keep = fe.make_align_problems(items)
    opt = capi.default_align_options(min_level=1)
    want = gpu_ctx.sparse_align(opt, gpb)
    want = [fe.se3_to_numpy(r.T_icur_iref) for r in want]
    for _ in range(5):
        gpu_ctx.sparse_align_enqueue(opt, gpb)
    got = gpu_ctx.sparse_align_fetch(3)
    for r, T in zip(got, want):
        assert r.status == 0 and np.array_equal(fe.se3_to_numpy(r.T_icur_iref), T)
    ms = (C.c_float * 40)()
    n = C.c_int()
    gpu_ctx._check(gpu_ctx.lib.svoh_sparse_align_kernel_ms_history(gpu_ctx.h, 5, ms, C.byref(n)))
    assert n.value == 5 and all(0.0 < ms[k] < 50.0 for k in range(5))
    gpu_ctx._check(gpu_ctx.lib.svoh_sparse_align_kernel_ms_history(gpu_ctx.h, 40, ms, C.byref(n)))
    assert 6 <= n.value <= 32
    last = C.c_float()
    gpu_ctx._check(gpu_ctx.lib.svoh_sparse_align_last_kernel_ms(gpu_ctx.h, C.byref(last)))
    assert last.value == ms[n.value - 1]


def test_queued_launches_of_different_sizes_each_deliver(gpu_ctx):
    """A large launch queued right behind... a smaller one: the second call's staging (descriptor block,
    zeroed control words, host feature arrays -- all in one reused pinned buffer whose layout moves with the problem
    count) must not touch what the first launch's upload has not read yet.  fetch_all hands out every queued
    launch's results; each must equal the blocking call's, bit for bit."""
    sizes = [700, 40, 333, 512, 90, 260, 1500, 64]
    scs = [helpers.small_scene(140 + k, n=n) for k, n in enumerate(sizes)]
    items = [[(sc, gpu_ctx.build_pyramid(sc.img_ref, 5), gpu_ctx.build_pyramid(sc.img_cur, 5))] for sc in scs]
    big, keep1 = fe.make_align_problems(items)            # host-resident feature arrays: staged per call
    small, keep2 = fe.make_align_problems(items[1:2])
    mid, keep3 = fe.make_align_problems(items[3:6])
    opt = capi.default_align_options(min_level=1)
    # the launch geometry (and with it the summation order) depends on a call's composition: every queued call is
    # compared with the blocking call of the same composition
    want = [fe.se3_to_numpy(r.T_icur_iref) for pbs in (big, small, mid, big) for r in gpu_ctx.sparse_align(opt, pbs)]
    for rounds in range(3):
        gpu_ctx.sparse_align_enqueue(opt, big)
        gpu_ctx.sparse_align_enqueue(opt, small)
        gpu_ctx.sparse_align_enqueue(opt, mid)
        gpu_ctx.sparse_align_enqueue(opt, big)
        got = gpu_ctx.sparse_align_fetch_all(8 + 1 + 3 + 8)
        for k, r in enumerate(got):
            assert r.status == 0 and r.n_fts_to_track > 0
            assert np.array_equal(fe.se3_to_numpy(r.T_icur_iref), want[k]), k
    with pytest.raises(Exception):                        # nothing is queued any more
        gpu_ctx.sparse_align_fetch_all(1)


def test_cluster_that_never_completes_falls_back(gpu_ctx):
    """A workgroup of a cluster that never reaches the device-side barrier (test hook) must not hang the device:
    its partners give up after their bounded wait (status 3 for enqueue / fetch callers) and
    svoh_sparse_align_batch runs the problem again with one workgroup."""
    import os, time
    # the hook (a share that never arrives) exists only in the test build of the library, on a context of its own
    hooks_lib = capi.load(capi.TESTHOOKS_LIB_PATH)
    product_ctx, gpu_ctx = gpu_ctx, fe.Context(0, lib=hooks_lib)
    sc = helpers.small_scene(97, n=1200)
    fr, fc = gpu_ctx.build_pyramid(sc.img_ref, 5), gpu_ctx.build_pyramid(sc.img_cur, 5)
    gpb, keep = fe.make_align_problems([[(sc, fr, fc)]])
    opt = capi.default_align_options(min_level=2)
    old = {k: os.environ.get(k) for k in ("SVOH_ALIGN_CLUSTER", "SVOH_ALIGN_CLUSTER_TEST_ABSENT")}
    try:
        os.environ["SVOH_ALIGN_CLUSTER"] = "0"
        gpu_ctx.reload_knobs()
        want = gpu_ctx.sparse_align(opt, gpb)[0]
        os.environ["SVOH_ALIGN_CLUSTER"] = "4"
        gpu_ctx.reload_knobs()
        os.environ["SVOH_ALIGN_CLUSTER_TEST_ABSENT"] = "1"
        gpu_ctx.reload_knobs()
        gpu_ctx.sparse_align_enqueue(opt, gpb)
        t0 = time.perf_counter()
        gave_up = gpu_ctx.sparse_align_fetch(1)[0]
        assert gave_up.status == 3 and time.perf_counter() - t0 < 30.0
        got = gpu_ctx.sparse_align(opt, gpb)[0]          # the batch entry repeats the launch without the cluster
        assert got.status == 0 and list(got.iters) == list(want.iters)
        assert np.array_equal(fe.se3_to_numpy(got.T_icur_iref), fe.se3_to_numpy(want.T_icur_iref))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
                gpu_ctx.reload_knobs()
            else:
                os.environ[k] = v
                gpu_ctx.reload_knobs()
        gpu_ctx.close()
        product_ctx.reload_knobs()


def test_candidate_projection_rides_the_alignment_launch(gpu_ctx):
    """f-4 on the device: svoh_project_candidates_enqueue queued behind svoh_sparse_align_enqueue with align_result_index = 0
    composes the current frame's pose ON THE DEVICE from the alignment result (T_f_w = T_cam_imu * T_icur_iref *
    T_imu_world_ref, sparse_img_align.cpp:100-107); one fetch delivers both.  Pixels and verdicts against an independent
    NumPy restatement of reprojector.cpp:489-543 / frame.cpp:229-260 (tests/np_restatement_direct.py) at the pose the
    fetch returns: verdicts exact, pixels to rounding."""
    import ctypes as C
    import np_restatement_direct as nd
    lib, h = gpu_ctx.lib, gpu_ctx.h
    cam = synth.Camera.euroc_like()
    sc = helpers.small_scene(131, n=400, cam=cam)
    fr, fc = gpu_ctx.build_pyramid(sc.img_ref, 5), gpu_ctx.build_pyramid(sc.img_cur, 5)
    pbs, keep = fe.make_align_problems([[(sc, fr, fc)]])
    opt = capi.default_align_options(min_level=1)
    rng = np.random.RandomState(4)
    # the "local map": two keyframes; world points all around the current view (many outside it) and seeds of both keyframes
    T_w_kf = [sc.T_w_ref, sc.T_w_ref * synth.SE3(synth.quat_from_axis_angle([0, 1, 0], 0.2), (0.3, 0.0, 0.1))]
    n = 3000
    kind = (rng.uniform(size=n) < 0.5).astype(np.uint8)
    kf = rng.randint(0, 2, n).astype(np.int32)
    v = np.zeros((n, 3)); mu = np.ones(n)
    for i in range(n):
        if kind[i]:
            f = np.array([rng.uniform(-0.9, 0.9), rng.uniform(-0.7, 0.7), 1.0]); v[i] = f / np.linalg.norm(f)
            mu[i] = 1.0 / rng.uniform(0.5, 8.0)
        else:
            v[i] = sc.T_w_cur.transform(np.array([rng.uniform(-6, 6), rng.uniform(-4, 4), rng.uniform(-1.0, 8.0)]))
    T_imu_world_ref = sc.T_imu_cam * sc.T_ref_f_w if hasattr(sc, "T_imu_cam") else sc.T_ref_f_w
    Ta, Tb = fe._se3(sc.T_cam_imu), fe._se3(T_imu_world_ref)
    Tk = (capi.svoh_se3 * 2)(*[fe._se3(t) for t in T_w_kf])
    c = fe._camera(cam)
    v_flat = np.ascontiguousarray(v).ravel()
    gpu_ctx.sparse_align_enqueue(opt, pbs)
    assert lib.svoh_project_candidates_enqueue(h, C.byref(c), C.byref(Ta), C.byref(Tb), 0, 2, Tk, n, kind.ctypes.data, kf.ctypes.data,
                                               v_flat.ctypes.data, mu.ctypes.data) == 0
    res = gpu_ctx.sparse_align_fetch(1)[0]
    px, vis = np.zeros(2 * n), np.zeros(n, np.uint8)
    assert lib.svoh_project_candidates_collect(h, n, px.ctypes.data, vis.ctypes.data) == 0
    # the same at the pose the fetch has returned, in NumPy
    T_icur_iref = nd.Tf.from7(fe.se3_to_numpy(res.T_icur_iref))
    T_f_w = nd.Tf.from7(sc.T_cam_imu.as7()) * T_icur_iref * nd.Tf.from7(T_imu_world_ref.as7())
    ncam = nd.Cam.of(cam)
    f_tl = ncam.back_project3(np.zeros(2)); min_cos = f_tl[2] / np.linalg.norm(f_tl)
    n_vis = 0
    for i in range(n):
        # tests/np_restatement_direct.get_candidate: reprojector.cpp:489-543 (the same function the host mirror is checked
        # against on the CPU, tests/test_np_second_opinion_cpu.py)
        T_kf = nd.Tf.from7(T_w_kf[kf[i]].as7()).inverse()
        ok, p = nd.get_candidate(ncam, T_f_w, T_kf, v[i] if not kind[i] else None, v[i], mu[i])
        if ok != bool(vis[i]):   # a pixel within rounding of an integer boundary, or a point on the cone, may fall on either side
            xyz = v[i] if not kind[i] else nd.Tf.from7(T_w_kf[kf[i]].as7()).apply(v[i] * (1.0 / mu[i]))
            xf = T_f_w.apply(xyz)
            assert min(abs(p[0] - round(p[0])), abs(p[1] - round(p[1]))) < 1e-9 or abs(xf[2] / np.linalg.norm(xf) - min_cos) < 1e-12, i
        elif ok:
            assert np.abs(px[2 * i:2 * i + 2] - p).max() < 1e-9
            n_vis += 1
    assert 200 < n_vis < n - 200
    # without a queued alignment result the composed form is refused, the explicit form works
    T_explicit = fe._se3(synth.SE3.from7(np.concatenate([T_f_w.q, T_f_w.t])))
    px2, vis2 = np.zeros(2 * n), np.zeros(n, np.uint8)
    assert lib.svoh_project_candidates(h, C.byref(c), C.byref(T_explicit), 2, Tk, n, kind.ctypes.data, kf.ctypes.data, v_flat.ctypes.data,
                                       mu.ctypes.data, px2.ctypes.data, vis2.ctypes.data) == 0
    assert np.array_equal(vis, vis2) and np.abs(px - px2)[np.repeat(vis.astype(bool), 2)].max() < 1e-9
