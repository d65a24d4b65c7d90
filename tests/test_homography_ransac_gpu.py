"""svoh_homography_ransac_batch (csrc/init.hip) against its NumPy restatement (tests/np_restatement_init.py).

The winner, both counts, the status and the mask are compared exactly: tests/test_init_cpu.py asserts for every case used
here that no error of any hypothesis lies within 1e-9 (relative) of the threshold, so a difference cannot be a rounding
tie.  H is compared to 1e-9 relative: both sides stop a quadratically converging iteration at steps below 1e-10."""
import ctypes as C

import numpy as np
import pytest

import init_cases as ic
import np_restatement_init as npi
from svo_pro_universal_amd import _capi as capi, frontend as fe

pytestmark = pytest.mark.gpu


def problem_of(name):
    c, K = ic.case(name)
    return (c["uv_ref"], c["uv_cur"], c["thresh"], c["seed"]), K


def check_against(r, mask, want, what):
    assert r.status == want["status"], what
    assert r.best_hypothesis == want["best_hypothesis"], what
    assert r.n_inliers_hypothesis == want["n_inliers_hypothesis"], what
    assert r.n_inliers == want["n_inliers"], what
    assert np.array_equal(mask, want["mask"]), what
    H = np.array(r.H).reshape(3, 3)
    scale = np.abs(want["H"]).max()
    err = np.abs(H - want["H"]).max() / (scale if scale > 0 else 1.0)
    print("%s: best %d, %d -> %d inliers, %d iterations, |dH| %.2e" % (what, r.best_hypothesis, r.n_inliers_hypothesis,
                                                                        r.n_inliers, r.refine_iters, err))
    assert err <= 1e-9, (what, err)
    assert abs(r.refine_iters - want["refine_iters"]) <= 1, (what, r.refine_iters, want["refine_iters"])
    if r.status == capi.SVOH_HOMOGRAPHY_OK:
        assert H[2, 2] == 1.0, what


@pytest.mark.parametrize("name", ic.CASE_NAMES)
def test_single_problem_equals_restatement(gpu_ctx, name):
    pb, K = problem_of(name)
    res, masks = gpu_ctx.homography_ransac([pb], capi.default_init_options(n_hypotheses=K))
    check_against(res[0], masks[0], ic.restated(name), name)


def as_bytes(r):
    return C.string_at(C.addressof(r), C.sizeof(r))


def test_ragged_batch_is_bit_identical_to_single_calls(gpu_ctx):
    pbs = [problem_of(nm)[0] for nm in ic.RAGGED_BATCH]
    opt = capi.default_init_options()
    res, masks = gpu_ctx.homography_ransac(pbs, opt)
    for i, nm in enumerate(ic.RAGGED_BATCH):
        one, m1 = gpu_ctx.homography_ransac([pbs[i]], opt)
        assert as_bytes(res[i]) == as_bytes(one[0]), nm
        assert np.array_equal(masks[i], m1[0]), nm
        check_against(res[i], masks[i], ic.restated(nm), "batch/" + nm)


def no_model(gpu_ctx, uv_ref, uv_cur, what):
    res, masks = gpu_ctx.homography_ransac([(uv_ref, uv_cur, 2.0 / 400.0, 99)])
    r = res[0]
    want = npi.estimate_homography_ransac(uv_ref, uv_cur, 2.0 / 400.0, 99)
    assert want["status"] == npi.STATUS_NO_MODEL, what
    assert r.status == capi.SVOH_HOMOGRAPHY_NO_MODEL, what
    assert list(r.H) == [0.0] * 9 and (r.best_hypothesis, r.n_inliers_hypothesis, r.n_inliers, r.refine_iters) == (0, 0, 0, 0), what
    assert not masks[0].any(), what


def test_collinear_matches_give_no_model(gpu_ctx):
    s = np.linspace(-0.5, 0.5, 40)
    uv = np.stack([s, 0.5 * s + 0.1], axis=1)
    no_model(gpu_ctx, uv, uv + [0.01, 0.0], "collinear")


def test_identical_matches_give_no_model(gpu_ctx):
    uv = np.tile([[0.1, -0.2]], (40, 1))
    no_model(gpu_ctx, uv, uv + 0.01, "identical")


def test_three_matches_give_no_model(gpu_ctx):
    c, _ = ic.case("n5")
    no_model(gpu_ctx, c["uv_ref"][:3], c["uv_cur"][:3], "n = 3")


def test_too_many_matches_is_an_error_and_leaves_the_results_untouched(gpu_ctx):
    uv = np.zeros((1025, 2))
    ok, _ = ic.case("n5")
    pbs = (capi.svoh_homography_problem * 2)()
    arrays = [np.ascontiguousarray(ok["uv_ref"]), np.ascontiguousarray(ok["uv_cur"]), uv]
    pbs[0].n, pbs[0].uv_ref, pbs[0].uv_cur, pbs[0].thresh, pbs[0].seed = 5, arrays[0].ctypes.data, arrays[1].ctypes.data, ok["thresh"], 1
    pbs[1].n, pbs[1].uv_ref, pbs[1].uv_cur, pbs[1].thresh, pbs[1].seed = 1025, uv.ctypes.data, uv.ctypes.data, ok["thresh"], 1
    res = (capi.svoh_homography_result * 2)()
    C.memset(res, 0xAB, C.sizeof(res))
    masks = np.full(5 + 1025, 0xCD, np.uint8)
    opt = capi.default_init_options()
    rc = gpu_ctx.lib.svoh_homography_ransac_batch(gpu_ctx.h, C.byref(opt), 2, pbs, res, masks.ctypes.data)
    assert rc == capi.SVOH_ERR_INVALID_ARGUMENT
    assert b"1024" in gpu_ctx.lib.svoh_last_error_string(gpu_ctx.h)
    assert as_bytes(res) == b"\xab" * C.sizeof(res)
    assert (masks == 0xCD).all()
    with pytest.raises(fe.SvohError):
        gpu_ctx.homography_ransac([(uv, uv, ok["thresh"], 1)])


def test_a_nan_match_is_never_an_inlier(gpu_ctx):
    c = ic.make_case(4242, 100)
    uv_ref, uv_cur = c["uv_ref"].copy(), c["uv_cur"].copy()
    k = int(np.flatnonzero(~c["is_outlier"])[3])
    uv_ref[k, 0] = np.nan
    uv_cur[k, 1] = np.nan
    want = npi.estimate_homography_ransac(uv_ref, uv_cur, c["thresh"], c["seed"])
    assert want["status"] == npi.STATUS_OK and want["n_degenerate"] > 0 and min(want["gap_hyp"], want["gap_final"]) >= 1e-9
    res, masks = gpu_ctx.homography_ransac([(uv_ref, uv_cur, c["thresh"], c["seed"])])
    assert masks[0][k] == 0
    check_against(res[0], masks[0], want, "NaN match")


def test_held_case_motion_and_count(gpu_ctx):
    """The case the reference's test_homography.cpp holds, through the Python face and the restatement's selection
    (homography.cpp:88-135): the motion and the vk::computeInliers count at 2 px are the restatement's."""
    c, K = ic.case("held")
    res, masks = gpu_ctx.homography_ransac([problem_of("held")[0]], capi.default_init_options(n_hypotheses=K))
    want = ic.restated("held")
    got = npi.select_motion(np.array(res[0].H).reshape(3, 3), c["f_cur"], c["f_ref"], masks[0], c["thresh"])
    ref = npi.select_motion(want["H"], c["f_cur"], c["f_ref"], want["mask"], c["thresh"])
    assert got["ok"] and got["picked"] == ref["picked"] and got["cheirality"] == ref["cheirality"] and got["score"] == ref["score"]
    # H agrees to 1e-9; tests/test_init_cpu.py::test_decomposition_is_well_conditioned_on_the_held_case bounds what the
    # decomposition makes of such a difference by 1e-6
    assert np.abs(got["R"] - ref["R"]).max() <= 1e-6 and np.abs(got["t"] - ref["t"]).max() <= 1e-6
    n_got = len(npi.compute_inliers(c["f_cur"], c["f_ref"], got["R"], got["t"], c["thresh_px"], c["focal"]))
    n_ref = len(npi.compute_inliers(c["f_cur"], c["f_ref"], ref["R"], ref["t"], c["thresh_px"], c["focal"]))
    assert n_got == n_ref and abs(n_got - c["reference_inliers"]) <= 3, (n_got, n_ref)


def test_kernel_time_is_reported(gpu_ctx):
    """svoh_last_kernel_ms after the call is this kernel's time (the session's context brackets every launch: frontend.Context)."""
    pb, _ = problem_of("n65")
    gpu_ctx.homography_ransac([pb])
    ms = C.c_float(-1.0)
    assert gpu_ctx.lib.svoh_last_kernel_ms(gpu_ctx.h, C.byref(ms)) == 0
    assert ms.value > 0.0
