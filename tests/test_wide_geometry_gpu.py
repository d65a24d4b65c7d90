"""The pose optimiser and the candidate projection on EQUIDISTANT and ATAN cameras, on the GPU, against the NumPy
restatement given a CamWide (the C oracle has no wide camera).  Bars as for the narrow pose family
(tests/test_np_second_opinion_cpu.py, tests/test_pose_gpu.py): status, iteration count, n_meas, deleted counts and every
outlier flag exact; pose within 1e-9; per-feature final errors rtol 1e-9 / atol 1e-15; the medians before / after
rel 1e-7.  measurement_sigma is 1.48f * a float median of errors: exact where the error type does not evaluate the
camera (UNIT_PLANE); elsewhere ocml and libm may round one double differently before the cast to float, so it is held
to two float spacings -- derived from the cast, not measured.  tests/test_wide_geometry_cpu.py holds the premises that
make the exact comparisons fair."""
import ctypes as C
import os

import numpy as np
import pytest
import torch  # before the first svoh call of the process: one HIP runtime for both (see _capi._share_hip_runtime_with_torch)

from svo_pro_universal_amd import _capi as capi, frontend as fe, synth

import np_restatement_direct as nd
import wide_geometry as wg

pytestmark = pytest.mark.gpu

THREADS = ("256", "64", "512")   # 512 is silently 256 where it is not instantiated


@pytest.fixture
def pose_threads(gpu_ctx):
    """Set SVOH_POSE_THREADS for a call and restore it, as tests/test_pose_gpu.py's fixture does."""
    old = os.environ.get("SVOH_POSE_THREADS")

    def use(v):
        if v is None:
            os.environ.pop("SVOH_POSE_THREADS", None)
        else:
            os.environ["SVOH_POSE_THREADS"] = v
        gpu_ctx.reload_knobs()
    yield use
    use(old)


def run(ctx, name, error_type):
    sc = wg.pose_scene(name)
    pb, keep = fe.make_pose_problem(sc["cams"], sc["T_imu_world_init"])
    return ctx.optimize_pose(wg.pose_options(name, error_type), [pb])[0], keep


def check(r, keep, name, error_type):
    g = wg.pose_reference(name, error_type)
    sc = wg.pose_scene(name)
    assert r.status == g["status"] == 0 and r.iters == g["iters"] and r.n_meas == g["n_meas"]
    assert (r.n_deleted_edges, r.n_deleted_corners) == (g["n_deleted_edges"], g["n_deleted_corners"])
    if error_type == wg.UNIT:
        assert r.measurement_sigma == g["sigma"]
    else:
        assert abs(r.measurement_sigma - g["sigma"]) <= 2 * float(np.spacing(np.float32(g["sigma"])))
    assert np.abs(fe.se3_to_numpy(r.T_imu_world) - g["T7"]).max() < 1e-9
    assert r.reproj_error_before == pytest.approx(g["err_before"], rel=1e-7)
    assert r.reproj_error_after == pytest.approx(g["err_after"], rel=1e-7)
    for k, o, e in zip(keep, g["outlier"], g["final"]):
        assert np.array_equal(k["outlier"][:len(o)], o)
        assert np.allclose(k["final_error"][:len(e)], e, rtol=1e-9, atol=1e-15)
    e0, e1 = wg.pose_error(sc, sc["T_imu_world_init"].as7()), wg.pose_error(sc, fe.se3_to_numpy(r.T_imu_world))
    assert e1[0] < 0.1 * e0[0] and e1[1] < 0.1 * e0[1]


def narrow_still_works(ctx):
    r, keep = run(ctx, "radtan", wg.IMAGE)
    check(r, keep, "radtan", wg.IMAGE)


# ---- 1. equidistant parity -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("error_type", [wg.UNIT, wg.BEARING, wg.IMAGE])
@pytest.mark.parametrize("n_cams", [1, 2])
def test_equidistant_pose_parity(gpu_ctx, pose_threads, threads, error_type, n_cams):
    pose_threads(threads)
    for seed in wg.SEEDS:
        name = "eq%d_%d" % (n_cams, seed)
        r, keep = run(gpu_ctx, name, error_type)
        check(r, keep, name, error_type)


# ---- 2. ATAN: no Jacobian ------------------------------------------------------------------------------------------
def test_atan_runs_where_no_jacobian_is_evaluated(gpu_ctx):
    for name, et in (("atan_edges", wg.UNIT), ("atan_corners", wg.BEARING)):
        r, keep = run(gpu_ctx, name, et)
        check(r, keep, name, et)


@pytest.mark.parametrize("name,error_type", [("atan_edges", wg.IMAGE), ("atan_corners", wg.IMAGE), ("atan_edges", wg.BEARING)])
def test_atan_is_refused_where_a_jacobian_would_be_evaluated(gpu_ctx, name, error_type):
    with pytest.raises(fe.SvohError) as e:
        run(gpu_ctx, name, error_type)
    assert e.value.code == capi.SVOH_ERR_UNSUPPORTED and "Jacobian" in str(e.value)
    narrow_still_works(gpu_ctx)


def packed_call(ctx, opt, built):
    cat = {k: [] for k in ("px", "f", "grad", "level", "type", "xyz_world", "usable")}
    for pb, keep in built:
        for a in keep:
            for k in cat:
                cat[k].append(a[k].ravel())
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(np.concatenate(v)).to(dev) for k, v in cat.items()}
    n_total = t["level"].numel()
    t["outlier"] = torch.zeros(n_total, dtype=torch.uint8, device=dev)
    t["final_error"] = torch.zeros(n_total, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    arr = capi.svoh_pose_packed_arrays()
    arr.n_features_total = n_total
    for k in ("px", "f", "grad", "level", "type", "xyz_world", "usable", "outlier", "final_error"):
        setattr(arr, k, t[k].data_ptr())
    pbs = (capi.svoh_pose_problem * len(built))(*[b[0] for b in built])
    res = (capi.svoh_pose_result * len(built))()
    ctx._check(ctx.lib.svoh_optimize_pose_batch_packed(ctx.h, C.byref(opt), len(built), pbs, C.byref(arr), res))
    return res, t["outlier"].cpu().numpy(), t["final_error"].cpu().numpy()


def test_atan_bearing_difference_is_refused_by_the_packed_entry(gpu_ctx):
    # even without an edgelet: the types live on the device and cannot be checked
    sc = wg.pose_scene("atan_corners")
    built = [fe.make_pose_problem(sc["cams"], sc["T_imu_world_init"])]
    with pytest.raises(fe.SvohError) as e:
        packed_call(gpu_ctx, wg.pose_options("atan_corners", wg.BEARING), built)
    assert e.value.code == capi.SVOH_ERR_UNSUPPORTED and "Jacobian" in str(e.value)
    narrow_still_works(gpu_ctx)


# ---- 3. a rig of a radtan and an equidistant camera ----------------------------------------------------------------
@pytest.mark.parametrize("error_type", [wg.IMAGE, wg.BEARING])
def test_mixed_rig_pose_parity(gpu_ctx, error_type):
    r, keep = run(gpu_ctx, "mixed", error_type)
    check(r, keep, "mixed", error_type)


# ---- 4. batches ----------------------------------------------------------------------------------------------------
def test_equidistant_batch_equals_singles(gpu_ctx):
    names = ["batch%d" % i for i in range(9)]
    opt = wg.pose_options(names[0], wg.IMAGE)
    built = [fe.make_pose_problem(wg.pose_scene(n)["cams"], wg.pose_scene(n)["T_imu_world_init"]) for n in names]
    batch = gpu_ctx.optimize_pose(opt, [b[0] for b in built])
    flags = [[k["outlier"].copy() for k in b[1]] for b in built]
    errs = [[k["final_error"].copy() for k in b[1]] for b in built]
    for i, n in enumerate(names):
        sc = wg.pose_scene(n)
        pb, keep = fe.make_pose_problem(sc["cams"], sc["T_imu_world_init"])
        r = gpu_ctx.optimize_pose(opt, [pb])[0]
        assert r.status == 0
        assert np.array_equal(fe.se3_to_numpy(r.T_imu_world), fe.se3_to_numpy(batch[i].T_imu_world))
        assert (r.iters, r.n_meas, r.n_deleted_corners, r.n_deleted_edges) == (batch[i].iters, batch[i].n_meas, batch[i].n_deleted_corners, batch[i].n_deleted_edges)
        assert r.measurement_sigma == batch[i].measurement_sigma and r.reproj_error_after == batch[i].reproj_error_after
        assert all(np.array_equal(a, k["outlier"]) for a, k in zip(flags[i], keep))
        assert all(np.array_equal(a, k["final_error"]) for a, k in zip(errs[i], keep))


def test_radtan_problem_beside_an_equidistant_one(gpu_ctx):
    opt = wg.pose_options("radtan", wg.IMAGE)
    sc_r, sc_e = wg.pose_scene("radtan"), wg.pose_scene("eq1_%d" % wg.SEEDS[0])
    pb, keep = fe.make_pose_problem(sc_r["cams"], sc_r["T_imu_world_init"])
    alone = gpu_ctx.optimize_pose(opt, [pb])[0]
    pb2, keep2 = fe.make_pose_problem(sc_r["cams"], sc_r["T_imu_world_init"])
    pbe, _ = fe.make_pose_problem(sc_e["cams"], sc_e["T_imu_world_init"])
    beside = gpu_ctx.optimize_pose(opt, [pbe, pb2])[1]   # the wide twin runs the radtan problem there
    assert (alone.status, alone.iters, alone.n_meas, alone.n_deleted_corners, alone.n_deleted_edges) == \
           (beside.status, beside.iters, beside.n_meas, beside.n_deleted_corners, beside.n_deleted_edges)
    assert np.array_equal(keep[0]["outlier"], keep2[0]["outlier"])
    assert np.abs(fe.se3_to_numpy(alone.T_imu_world) - fe.se3_to_numpy(beside.T_imu_world)).max() < 1e-9


def test_packed_entry_equals_the_host_array_entry_on_an_equidistant_problem(gpu_ctx):
    name = "eq2_%d" % wg.SEEDS[0]
    sc = wg.pose_scene(name)
    opt = wg.pose_options(name, wg.IMAGE)
    built = [fe.make_pose_problem(sc["cams"], sc["T_imu_world_init"])]
    want = gpu_ctx.optimize_pose(opt, [built[0][0]])[0]
    res, out_g, err_g = packed_call(gpu_ctx, opt, built)
    r = res[0]
    assert r.status == want.status == 0 and r.iters == want.iters and r.n_meas == want.n_meas
    assert np.array_equal(fe.se3_to_numpy(r.T_imu_world), fe.se3_to_numpy(want.T_imu_world))
    assert r.measurement_sigma == want.measurement_sigma and r.reproj_error_after == want.reproj_error_after
    off = 0
    for a in built[0][1]:
        n = a["level"].size
        assert np.array_equal(out_g[off:off + n], a["outlier"][:n]) and np.array_equal(err_g[off:off + n], a["final_error"][:n])
        off += n


# ---- 5. candidates, single entry -----------------------------------------------------------------------------------
def compare_candidates(px, vis, ref):
    differ = vis != ref["ok"]
    assert differ.sum() <= 4 and not (differ & ~ref["near"]).any()
    both = vis & ref["ok"]
    assert np.abs(px[both] - ref["px"][both]).max() < 1e-9


@pytest.mark.parametrize("kind", ["equidistant", "atan"])
def test_candidates_on_a_wide_camera(gpu_ctx, kind):
    cs = wg.candidate_set()
    px, vis = gpu_ctx.project_candidates(wg.camera(kind), cs["T_f_w"], cs["T_w_kf"], cs["kind"], cs["kf"], cs["v"], cs["mu"])
    compare_candidates(px, vis, wg.candidate_reference(kind))
    assert 300 < vis.sum() < cs["n"] - 300


# ---- 6. candidates with the pose composed on the device from the alignment queued in front -------------------------
def test_equidistant_candidates_ride_a_radtan_alignment(gpu_ctx):
    cam = synth.Camera.euroc_like()
    sc = synth.make_align_scene(131, n_features=200, patch_size=4, cam=cam)
    fr, fc = gpu_ctx.build_pyramid(sc.img_ref, 5), gpu_ctx.build_pyramid(sc.img_cur, 5)
    pbs, keep = fe.make_align_problems([[(sc, fr, fc)]])
    cs = wg.candidate_set()
    eq = wg.camera("equidistant")
    T_cam_imu = synth.SE3(synth.quat_from_axis_angle([0.1, 0.2, 1.0], 0.05), (0.02, -0.01, 0.03))
    T_imu_world_ref = T_cam_imu.inverse() * cs["T_f_w"]     # with T_icur_iref near the identity the view stays the set's
    gpu_ctx.sparse_align_enqueue(capi.default_align_options(min_level=1), pbs)
    n = gpu_ctx.project_candidates_enqueue(eq, None, cs["T_w_kf"], cs["kind"], cs["kf"], cs["v"], cs["mu"], align_result_index=0,
                                           T_cam_imu=T_cam_imu, T_imu_world_ref=T_imu_world_ref)
    res = gpu_ctx.sparse_align_fetch(1)[0]
    px, vis = gpu_ctx.project_candidates_collect(n)
    T = nd.Tf.from7(T_cam_imu.as7()) * nd.Tf.from7(fe.se3_to_numpy(res.T_icur_iref)) * nd.Tf.from7(T_imu_world_ref.as7())
    T7 = np.concatenate([T.q, T.t])
    px2, vis2 = gpu_ctx.project_candidates(eq, T7, cs["T_w_kf"], cs["kind"], cs["kf"], cs["v"], cs["mu"])
    assert np.array_equal(vis, vis2) and 300 < vis.sum() < n - 300
    assert np.abs(px[vis] - px2[vis]).max() < 1e-9
    gpu_ctx.release_frame(fr); gpu_ctx.release_frame(fc)


# ---- 7. candidates, staged entries: a radtan and an equidistant job in one launch -----------------------------------
# (the per-point form here; the ranges form, with and without inverse depths read from a seed batch in flight, below)
def _view(ptr, dtype, count):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(count * np.dtype(dtype).itemsize,)).view(dtype)


def test_staged_candidates_of_a_radtan_and_an_equidistant_job(gpu_ctx):
    ctx = gpu_ctx
    cs = wg.candidate_set()
    n, cams = cs["n"], [wg.camera("radtan"), wg.camera("equidistant")]
    want = [ctx.project_candidates(c, cs["T_f_w"], cs["T_w_kf"], cs["kind"], cs["kf"], cs["v"], cs["mu"]) for c in cams]
    st = capi.svoh_candidate_stage_t()
    ctx._check(ctx.lib.svoh_project_candidates_stage(ctx.h, 2, 4, 2 * n, C.byref(st)))
    jarr = C.cast(st.jobs, C.POINTER(capi.svoh_candidate_job))
    karr = C.cast(st.T_world_kf, C.POINTER(capi.svoh_se3))
    for j, cam in enumerate(cams):
        jj = capi.svoh_candidate_job()
        jj.cam, jj.T_f_w_or_T_cam_imu, jj.align_result_index = fe._camera(cam), fe._se3(cs["T_f_w"]), -1
        jj.kf_begin, jj.n_kf, jj.point_begin, jj.n_points = 2 * j, 2, j * n, n
        jarr[j] = jj
        for k, T in enumerate(cs["T_w_kf"]):
            karr[2 * j + k] = fe._se3(T)
        _view(st.job, np.int32, 2 * n)[j * n:(j + 1) * n] = j
        _view(st.kind, np.uint8, 2 * n)[j * n:(j + 1) * n] = cs["kind"]
        _view(st.kf, np.int32, 2 * n)[j * n:(j + 1) * n] = cs["kf"]
        _view(st.v, np.float64, 6 * n)[3 * j * n:3 * (j + 1) * n] = cs["v"].ravel()
        _view(st.mu, np.float64, 2 * n)[j * n:(j + 1) * n] = cs["mu"]
    ctx._check(ctx.lib.svoh_project_candidates_enqueue_staged(ctx.h))
    ctx._check(ctx.lib.svoh_project_candidates_wait(ctx.h))
    for j in range(2):
        px = _view(st.px, np.float64, 4 * n)[2 * j * n:2 * (j + 1) * n].reshape(n, 2)
        vis = _view(st.visible, np.uint8, 2 * n)[j * n:(j + 1) * n].astype(bool)
        assert np.array_equal(vis, want[j][1])
        # the radtan job goes through the wide twin here: rounding may differ from the narrow kernel's
        assert np.abs(px[vis] - want[j][0][vis]).max() < 1e-9


def _upload_features(ctx, sets):
    """svoh_features_upload for a list of seed sets (synth.make_seed_set) in one call; returns the handles."""
    m = len(sets)
    keep = [[np.ascontiguousarray(sd[k], dt) for sd in sets] for k, dt in (("px", np.float64), ("f", np.float64), ("grad", np.float64), ("level", np.int32))]
    n = (C.c_int32 * m)(*[a.size for a in keep[3]])
    ptrs = [(C.c_void_p * m)(*[a.ctypes.data for a in col]) for col in keep]
    out = (C.c_uint64 * m)()
    ctx._check(ctx.lib.svoh_features_upload(ctx.h, m, n, ptrs[0], ptrs[1], ptrs[2], ptrs[3], out))
    return [int(h) for h in out]


@pytest.mark.parametrize("with_units", [False, True])
def test_staged_ranges_of_a_radtan_and_an_equidistant_job(gpu_ctx, with_units):
    """svoh_project_candidates_stage_ranges with two jobs over the same seeds of two keyframes (resident f columns), one
    job on a radtan camera and one on an equidistant: project_candidates_ranges_wide_kernel.  with_units: through
    svoh_project_candidates_enqueue_staged_units, the inverse depths read on the device from a depth-filter batch that has
    been sent off and not collected (every ninth point keeps its staged value), as
    tests/test_lockstep_abi_gpu.py::test_candidate_projection_reads_inverse_depths_from_the_seed_batch_in_flight; else
    through svoh_project_candidates_enqueue_staged with the staged inverse depths.  Each job against the single entry on
    its camera with the inverse depths the job must have used: flags exact, pixels within 1e-9 (the radtan job runs the
    wide twin here and the narrow kernel there)."""
    ctx = gpu_ctx
    cam = synth.Camera.euroc_like()          # the frames and the seed update: the image kernels run narrow cameras only
    job_cams = [wg.camera("radtan"), wg.camera("equidistant")]
    pairs = []
    for i in range(2):
        sc = synth.make_align_scene(980 + i, n_features=10, cam=cam, rot_deg=(0.5, 1.5), trans_m=(0.05, 0.15))
        pairs.append((sc, ctx.build_pyramid(sc.img_ref, 5), ctx.build_pyramid(sc.img_cur, 5)))
    sets = [synth.make_seed_set(sc, 300 + 80 * i, seed=40 + i, margin=14) for i, (sc, fr, fc) in enumerate(pairs)]
    n_each = [sd["level"].size for sd in sets]
    n = sum(n_each)
    handles = _upload_features(ctx, sets)
    T_cur = pairs[0][0].T_cur_f_w_gt
    T_world_kf = [sc.T_ref_f_w.inverse() for sc, fr, fc in pairs]
    old_mu = [sd["state"].reshape(-1, 4)[:, 0].copy() for sd in sets]
    units = [np.arange(sum(n_each[:k]), sum(n_each[:k + 1]), dtype=np.int32) for k in range(2)]
    for k in range(2):
        units[k][::9] = -1
    g = None
    if with_units:   # the update, sent off and not collected
        mopt, dopt = capi.default_matcher_options(), capi.default_depth_filter_options(cam)
        refs = (capi.svoh_frame_view * 2)(*[fe.make_frame_view(fr, cam, sc.T_ref_f_w, sd["mu_range"], 0) for (sc, fr, fc), sd in zip(pairs, sets)])
        curs = (capi.svoh_frame_view * 2)(*[fe.make_frame_view(fc, cam, sc.T_cur_f_w_gt, 0.0, 1) for (sc, fr, fc) in pairs])
        ctx._check(ctx.lib.svoh_matcher_begin_deferred(ctx.h))
        g = capi.svoh_matcher_stage_t()
        ctx._check(ctx.lib.svoh_matcher_stage(ctx.h, 1, n, 8, 0, C.byref(g)))
        off = 0
        for k, sd in enumerate(sets):
            m = n_each[k]
            _view(g.ref_frame_idx, np.int32, n)[off:off + m] = k
            _view(g.cur_frame_idx, np.int32, n)[off:off + m] = k
            for name, width, dt in (("px", 2, np.float64), ("f", 3, np.float64), ("grad", 2, np.float64), ("level", 1, np.int32), ("type", 1, np.uint8), ("state", 4, np.float64)):
                _view(getattr(g, name), dt, width * n)[width * off:width * (off + m)] = sd[name]
            off += m
        fb = capi.svoh_feature_batch()
        fb.n, fb.mem_space, fb.n_cur_frames = n, capi.SVOH_MEM_STAGED, 2
        for k in ("ref_frame_idx", "cur_frame_idx", "px", "f", "grad", "level", "type"):
            setattr(fb, k, getattr(g, k))
        ctx._check(ctx.lib.svoh_update_seeds_batch(ctx.h, C.byref(mopt), C.byref(dopt), 2, refs, curs, C.byref(fb), g.state, g.success, g.result, None))
        ctx._check(ctx.lib.svoh_matcher_flush(ctx.h))
    # two jobs, each over both keyframes: four ranges back to back, 2 n points
    cs = capi.svoh_candidate_stage_t()
    ctx._check(ctx.lib.svoh_project_candidates_stage_ranges(ctx.h, 2, 4, 2 * n, C.byref(cs)))
    jarr = C.cast(cs.jobs, C.POINTER(capi.svoh_candidate_job))
    karr = C.cast(cs.T_world_kf, C.POINTER(capi.svoh_se3))
    rarr = C.cast(cs.ranges, C.POINTER(capi.svoh_candidate_range))
    off = 0
    for j, jc in enumerate(job_cams):
        jj = capi.svoh_candidate_job()
        jj.cam, jj.T_f_w_or_T_cam_imu, jj.align_result_index = fe._camera(jc), fe._se3(T_cur), -1
        jj.kf_begin, jj.n_kf, jj.point_begin, jj.n_points = 2 * j, 2, j * n, n
        jarr[j] = jj
        for k in range(2):
            karr[2 * j + k] = fe._se3(T_world_kf[k])
            r = capi.svoh_candidate_range()
            r.features, r.point_begin, r.n_points, r.job = handles[k], off, n_each[k], j
            rarr[2 * j + k] = r
            _view(cs.kind, np.uint8, 2 * n)[off:off + n_each[k]] = 1
            _view(cs.mu, np.float64, 2 * n)[off:off + n_each[k]] = old_mu[k]
            if with_units:
                _view(cs.mu_unit, np.int32, 2 * n)[off:off + n_each[k]] = units[k]
            off += n_each[k]
    ctx._check((ctx.lib.svoh_project_candidates_enqueue_staged_units if with_units else ctx.lib.svoh_project_candidates_enqueue_staged)(ctx.h))
    ctx._check(ctx.lib.svoh_project_candidates_wait(ctx.h))
    px_all, vis_all = _view(cs.px, np.float64, 4 * n).copy(), _view(cs.visible, np.uint8, 2 * n).copy()
    want_mu = np.concatenate(old_mu)
    if with_units:
        ctx._check(ctx.lib.svoh_matcher_collect(ctx.h))
        new_mu = _view(g.state, np.float64, 4 * n).reshape(-1, 4)[:, 0].copy()
        assert (new_mu != want_mu).mean() > 0.3          # the update did move the seeds
        by_unit = np.concatenate(units) >= 0
        want_mu[by_unit] = new_mu[by_unit]
    kf = np.concatenate([np.full(m, k, np.int32) for k, m in enumerate(n_each)])
    v = np.concatenate([np.asarray(sd["f"], np.float64).ravel() for sd in sets])
    for j, jc in enumerate(job_cams):
        px_w, vis_w = ctx.project_candidates(jc, T_cur, T_world_kf, np.ones(n, np.uint8), kf, v, want_mu)
        vis = vis_all[j * n:(j + 1) * n].astype(bool)
        px = px_all[2 * j * n:2 * (j + 1) * n].reshape(n, 2)
        assert np.array_equal(vis, vis_w) and 0.05 < vis.mean() < 1.0
        assert np.abs(px[vis] - px_w[vis]).max() < 1e-9
    for h in handles:
        ctx._check(ctx.lib.svoh_features_release(ctx.h, h))
    for sc, fr, fc in pairs:
        ctx.release_frame(fr); ctx.release_frame(fc)
