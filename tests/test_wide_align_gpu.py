"""Sparse image alignment on equidistant and atan cameras: svoh_sparse_align_wide_batch / _wide_evaluate
(sparse_align_wide_kernel) against the NumPy reading of tests/wide_align.py.  The C oracle has no wide camera; the reading is
tied to it for radtan in tests/test_wide_align_cpu.py, which also asserts the conditions on these inputs (no projected patch
corner within 1e-6 px of a visibility bound, no max|dx| within 1e-6 of eps) under which the discrete results here are exact.

Tolerances: those of tests/test_sparse_align_gpu.py against the oracle (check_evaluate, check_run) --
  H, g            relative 1e-10 of the largest entry (helpers.TOL_HG)
  n_meas, n_selected, visibility, status, iterations, n_patch_iters     exact
  pose, alpha     1e-8 absolute (helpers.TOL_POSE), beta 1e-6
  chi2            relative 1e-4."""
import ctypes as C

import numpy as np
import pytest

from svo_pro_universal_amd import _capi as capi, frontend as fe, synth

import helpers
import wide_align as wa

pytestmark = pytest.mark.gpu

TOL_HG = helpers.TOL_HG
TOL_POSE = helpers.TOL_POSE


@pytest.fixture(scope="module")
def frames(gpu_ctx):
    """(scene, ref levels, cur levels) -> (scene, ref handle, cur handle); the device's pyramid is the reading's."""
    made = {}

    def get(cam):
        key = id(cam[1])
        if key not in made:
            sc, ref, cur = cam
            fr, lv = gpu_ctx.build_pyramid(sc.img_ref, len(ref), return_levels=True)
            fc, lvc = gpu_ctx.build_pyramid(sc.img_cur, len(cur), return_levels=True)
            assert all(np.array_equal(a, b) for a, b in zip(lv, ref)) and all(np.array_equal(a, b) for a, b in zip(lvc, cur))
            made[key] = (fr, fc)
        return (cam[0],) + made[key]
    yield get
    for fr, fc in made.values():
        gpu_ctx.release_frame(fr)
        gpu_ctx.release_frame(fc)


def result_bytes(r):
    """Every field of a result (or of an array of results) as bytes: the struct's padding is nobody's."""
    if not isinstance(r, capi.svoh_align_result):
        return b"".join(result_bytes(x) for x in r)
    ints = np.array([r.status, r.n_fts_to_track, r.n_patch_iters] + list(r.iters) + list(r.n_meas), np.int64)
    dbl = np.array(list(r.T_icur_iref.q) + list(r.T_icur_iref.t) + [r.alpha, r.beta] + list(r.chi2), np.float64)
    return ints.tobytes() + dbl.tobytes()


def check_against_reading(rg, rn):
    assert rg.status == rn["status"] and rg.n_fts_to_track == rn["n_fts_to_track"]
    assert list(rg.iters) == rn["iters"] and list(rg.n_meas) == rn["n_meas"]
    assert rg.n_patch_iters == rn["n_patch_iters"]
    q = np.array([rg.T_icur_iref.q[i] for i in range(4)]); t = np.array([rg.T_icur_iref.t[i] for i in range(3)])
    dq = min(np.abs(q - rn["T"].q).max(), np.abs(q + rn["T"].q).max())
    assert max(dq, np.abs(t - rn["T"].t).max()) < TOL_POSE
    assert abs(rg.alpha - rn["alpha"]) < TOL_POSE and abs(rg.beta - rn["beta"]) < 1e-6


# ---- 1. evaluation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [4, 8])
@pytest.mark.parametrize("kind", wa.KINDS)
def test_evaluation_matches_the_reading(gpu_ctx, frames, kind, P):
    cam = wa.eval_scene(kind, P)
    T, a, b = wa.eval_state(cam[0])
    gpb, keep = fe.make_align_problems([[frames(cam)]], T_init=T, alpha_init=a, beta_init=b)
    for opt in wa.option_sets(kind, P):
        for level in wa.EVAL_LEVELS:
            (Hn, gn, c2n, nmn, visn, nsel), _probe = wa.eval_reference(kind, wa.opt_key(opt), level)
            Hg, gg, c2g, nmg, visg = gpu_ctx.sparse_align_wide_evaluate(opt, gpb[0], level)
            assert nmg == nmn and len(visg) == nsel and np.array_equal(visg, visn)
            assert np.abs(Hg - Hn).max() <= TOL_HG * np.abs(Hn).max()
            assert np.abs(gg - gn).max() <= TOL_HG * np.abs(gn).max()
            assert np.array_equal(Hg, Hg.T)
            assert abs(c2g - c2n) <= 1e-4 * abs(c2n)


# ---- 2. full run ----------------------------------------------------------------------------------------------------
# (kind, P, distortion Jacobian): a case of its own each, so that none takes more than a few seconds (the time is the reading's)
RUN_CASES = [(kind, P, dj) for kind in wa.KINDS for P in (4, 8) for dj in ((0,) if kind == "atan" else (0, 1))]


@pytest.mark.parametrize("kind,P,dj", RUN_CASES)
def test_full_run_matches_the_reading(gpu_ctx, frames, kind, P, dj):
    cam = wa.run_scene(kind, P)
    sc = cam[0]
    for opt in [o for o in wa.option_sets(kind, P) if o.use_distortion_jacobian == dj]:
        for with_prior in ((False, True) if opt.use_distortion_jacobian == 0 and opt.robustification == 0 else (False,)):
            rn, _probe = wa.run_reference(kind, wa.opt_key(opt), with_prior)
            prior = wa.weighted_prior(sc)[0] if with_prior else None
            gpb, keep = fe.make_align_problems([[frames(cam)]], T_init=wa.start_state(sc), prior=prior)
            rg = gpu_ctx.sparse_align_wide(opt, gpb)[0]
            check_against_reading(rg, rn)


# ---- 3. one ragged launch of seven problems ---------------------------------------------------------------------------
def test_ragged_launch_equals_single_launches_bit_for_bit_and_the_reading(gpu_ctx, frames):
    pbs = wa.ragged_problems()
    opt = capi.default_align_options(**wa.RAGGED_OPT)
    items, T_init, priors = [], [], []
    for name in wa.RAGGED_ORDER:
        pb = pbs[name]
        items.append([frames(c) for c in pb["cams"]])
        T_init.append(wa.start_state(pb["cams"][0][0]))
        priors.append(pb["prior"][0] if pb.get("prior") else capi.svoh_align_prior())
    gpb, keep = fe.make_align_problems(items, T_init=T_init, prior=priors)
    together = gpu_ctx.sparse_align_wide(opt, gpb)
    for i, name in enumerate(wa.RAGGED_ORDER):
        one, keep1 = fe.make_align_problems([items[i]], T_init=[T_init[i]], prior=[priors[i]])
        alone = gpu_ctx.sparse_align_wide(opt, one)[0]
        assert result_bytes(alone) == result_bytes(together[i]), name
        check_against_reading(together[i], wa.ragged_reference(name)[0])
    assert together[5].status == 1 and together[5].n_fts_to_track == 0 and together[4].n_fts_to_track == 1


# ---- 4. all-narrow problems through the wide entries ------------------------------------------------------------------
def test_narrow_problems_through_the_wide_entries_are_the_narrow_entries_results(gpu_ctx, frames):
    a, b = wa.scene("radtan", 313, 150, 4, 30), wa.scene("radtan", 317, 150, 4, 30)
    opt = capi.default_align_options(min_level=1, use_distortion_jacobian=1)
    gpb, keep = fe.make_align_problems([[frames(a)], [frames(b)]], T_init=[wa.start_state(a[0]), wa.start_state(b[0])])
    narrow = gpu_ctx.sparse_align(opt, gpb)
    wide = gpu_ctx.sparse_align_wide(opt, gpb)
    assert result_bytes(narrow) == result_bytes(wide) and narrow[0].status == 0 and sum(narrow[0].iters) >= 4
    for level in (4, 1):
        en = gpu_ctx.sparse_align_evaluate(opt, gpb[0], level)
        ew = gpu_ctx.sparse_align_wide_evaluate(opt, gpb[0], level)
        assert all(np.array_equal(x, y) for x, y in zip(en, ew)) and en[3] > 0


# ---- 5. refusals ----------------------------------------------------------------------------------------------------
def _call_wide(ctx, opt, gpb):
    """(rc, results array pre-filled with 0xA5, whether it is untouched)"""
    n = len(gpb)
    res = (capi.svoh_align_result * n)()
    C.memset(res, 0xA5, C.sizeof(res))
    rc = ctx.lib.svoh_sparse_align_wide_batch(ctx.h, C.byref(opt), n, gpb, res)
    return rc, C.string_at(C.addressof(res), C.sizeof(res)) == b"\xa5" * C.sizeof(res)


def _eval_wide(ctx, opt, pb, level):
    H, g = np.full(64, 7.5), np.full(8, 7.5)
    vis = np.full(4096, 0xA5, np.uint8)
    chi2, nm, nsel = C.c_double(7.5), C.c_int32(-7), C.c_int32(-7)
    rc = ctx.lib.svoh_sparse_align_wide_evaluate(ctx.h, C.byref(opt), C.byref(pb), level, H.ctypes.data, g.ctypes.data, C.byref(chi2),
                                                 C.byref(nm), vis.ctypes.data, C.byref(nsel))
    untouched = (H == 7.5).all() and (g == 7.5).all() and (vis == 0xA5).all() and chi2.value == 7.5 and nm.value == -7 and nsel.value == -7
    return rc, untouched


def test_refusals_leave_results_untouched_and_the_context_usable(gpu_ctx, frames):
    ctx = gpu_ctx
    eq, at, rt = wa.scene("equidistant", 317, 150, 4, 30), wa.scene("atan", 324, 150, 4, 30), wa.scene("radtan", 313, 150, 4, 30)
    opt = capi.default_align_options(min_level=1)
    opt_dj = capi.default_align_options(min_level=1, use_distortion_jacobian=1)
    starts = [wa.start_state(c[0]) for c in (eq, at, rt)]
    narrow_pb, keep_n = fe.make_align_problems([[frames(rt)]], T_init=[starts[2]])
    narrow_before = result_bytes(ctx.sparse_align(opt, narrow_pb))

    def fresh():
        return fe.make_align_problems([[frames(eq)], [frames(at)], [frames(rt)]], T_init=starts)

    gpb, keep = fresh()
    ok_rc, _ = _call_wide(ctx, opt, gpb)
    assert ok_rc == 0
    # ATAN with the distortion Jacobian: the reference has none for that model
    assert _call_wide(ctx, opt_dj, gpb) == (capi.SVOH_ERR_UNSUPPORTED, True)
    assert _eval_wide(ctx, opt_dj, gpb[1], 2) == (capi.SVOH_ERR_UNSUPPORTED, True)
    # ATAN with s zero or not finite
    for s in (0.0, float("inf"), float("nan")):
        bad, keep_b = fresh()
        bad[1].cams[0].cam.d[0] = s
        assert _call_wide(ctx, opt, bad) == (capi.SVOH_ERR_INVALID_ARGUMENT, True)
        assert _eval_wide(ctx, opt, bad[1], 2) == (capi.SVOH_ERR_INVALID_ARGUMENT, True)
    # a camera that is not in host memory (the radtan one beside the wide ones as well), or seed positions from a batch in flight
    for which in (0, 2):
        bad, keep_b = fresh()
        bad[which].cams[0].mem_space = capi.SVOH_MEM_DEVICE
        assert _call_wide(ctx, opt, bad) == (capi.SVOH_ERR_UNSUPPORTED, True)
    bad, keep_b = fresh()
    bad[0].cams[0].mem_space = capi.SVOH_MEM_DEVICE
    assert _eval_wide(ctx, opt, bad[0], 2) == (capi.SVOH_ERR_UNSUPPORTED, True)
    units = np.full(eq[0].n_features, -1, np.int32)
    bad, keep_b = fresh()
    bad[0].cams[0].pos_seed_unit = units.ctypes.data
    assert _call_wide(ctx, opt, bad) == (capi.SVOH_ERR_UNSUPPORTED, True)
    assert _eval_wide(ctx, opt, bad[0], 2) == (capi.SVOH_ERR_UNSUPPORTED, True)
    # inside a deferred matcher section
    ctx._check(ctx.lib.svoh_matcher_begin_deferred(ctx.h))
    try:
        assert _call_wide(ctx, opt, gpb) == (capi.SVOH_ERR_INVALID_ARGUMENT, True)
        assert _eval_wide(ctx, opt, gpb[0], 2) == (capi.SVOH_ERR_INVALID_ARGUMENT, True)
    finally:
        ctx._check(ctx.lib.svoh_matcher_collect(ctx.h))
    # between a narrow enqueue and its fetch: refused, and the fetch then delivers the right results
    ctx.sparse_align_enqueue(opt, narrow_pb)
    assert _call_wide(ctx, opt, gpb) == (capi.SVOH_ERR_INVALID_ARGUMENT, True)
    assert _eval_wide(ctx, opt, gpb[0], 2) == (capi.SVOH_ERR_INVALID_ARGUMENT, True)
    assert result_bytes(ctx.sparse_align_fetch(1)) == narrow_before
    # ... and afterwards both kinds of launch give what they gave
    again, _ = _call_wide(ctx, opt, gpb)
    assert again == 0
    assert result_bytes(ctx.sparse_align(opt, narrow_pb)) == narrow_before
    assert result_bytes(ctx.sparse_align_wide(opt, gpb)) == result_bytes(ctx.sparse_align_wide(opt, gpb))


def test_every_other_alignment_entry_still_refuses_an_equidistant_problem(gpu_ctx, frames):
    ctx = gpu_ctx
    eq = wa.scene("equidistant", 317, 150, 4, 30)
    opt = capi.default_align_options(min_level=1)
    gpb, keep = fe.make_align_problems([[frames(eq)]], T_init=[wa.start_state(eq[0])])
    with pytest.raises(fe.SvohError) as e:
        ctx.sparse_align(opt, gpb)
    assert e.value.code == capi.SVOH_ERR_INVALID_ARGUMENT and "distortion" in str(e.value)
    with pytest.raises(fe.SvohError) as e:
        ctx.sparse_align_enqueue(opt, gpb)
    assert "distortion" in str(e.value)
    key = C.c_int32(0)
    assert ctx.lib.svoh_sparse_align_geometry_key(ctx.h, C.byref(opt), C.byref(gpb[0]), C.byref(key)) == capi.SVOH_ERR_INVALID_ARGUMENT
    narrow, keep_n = fe.make_align_problems([[frames(wa.scene("radtan", 313, 150, 4, 30))]])
    ctx._check(ctx.lib.svoh_sparse_align_geometry_key(ctx.h, C.byref(opt), C.byref(narrow[0]), C.byref(key)))
    assert ctx.lib.svoh_sparse_align_enqueue_keyed(ctx.h, C.byref(opt), 1, gpb, key) == capi.SVOH_ERR_INVALID_ARGUMENT
    with pytest.raises(fe.SvohError) as e:
        ctx.sparse_align_evaluate(opt, gpb[0], 2)
    assert "distortion" in str(e.value)
    d_state, d_sums = C.c_void_p(), C.c_void_p()
    ctx._check(ctx.lib.svoh_sparse_align_split_buffers(ctx.h, C.byref(d_state), C.byref(d_sums)))
    with pytest.raises(fe.SvohError) as e:
        ctx.split_init(gpb[0], d_state.value)
    assert "distortion" in str(e.value)
    with pytest.raises(fe.SvohError):
        ctx.sparse_align_fetch(1)          # nothing was queued by any of them
    assert ctx.sparse_align(opt, narrow)[0].status == 0


# ---- 6. an odd size ---------------------------------------------------------------------------------------------------
def test_equidistant_run_at_413x309(gpu_ctx, frames):
    cam = wa.odd_scene()
    gpb, keep = fe.make_align_problems([[frames(cam)]], T_init=[wa.start_state(cam[0])])
    rg = gpu_ctx.sparse_align_wide(capi.default_align_options(**wa.ODD_OPT), gpb)[0]
    check_against_reading(rg, wa.odd_reference()[0])


# ---- bookkeeping of a twin launch -------------------------------------------------------------------------------------
def test_a_twin_launch_is_timed_and_leaves_the_launch_info_alone(gpu_ctx, frames):
    ctx = gpu_ctx
    rt, eq = wa.scene("radtan", 313, 150, 4, 30), wa.scene("equidistant", 317, 150, 4, 30)
    opt = capi.default_align_options(min_level=1)
    narrow, keep_n = fe.make_align_problems([[frames(rt)]], T_init=[wa.start_state(rt[0])])
    wide, keep_w = fe.make_align_problems([[frames(eq)]], T_init=[wa.start_state(eq[0])])
    ctx.sparse_align(opt, narrow)
    info, lds, lane = ctx.last_align_launch(), ctx.last_align_launch_lds(), ctx.last_align_lane()
    ctx.sparse_align_wide(opt, wide)
    ms = C.c_float(-1.0)
    ctx._check(ctx.lib.svoh_sparse_align_last_kernel_ms(ctx.h, C.byref(ms)))
    assert 0.0 < ms.value < 1000.0
    assert (ctx.last_align_launch(), ctx.last_align_launch_lds(), ctx.last_align_lane()) == (info, lds, lane)
