"""svoh_translation_ransac_batch (csrc/init.hip) against its NumPy restatement (tests/np_restatement_twopoint.py).

The winner, both counts, the number of degenerate hypotheses, the status and the mask are compared exactly:
tests/test_twopoint_cpu.py asserts for every case used here that no error of any hypothesis lies within 1e-7 (relative) of
the threshold, so a difference cannot be a rounding tie.  t is compared to 1e-9, the bar tests/test_homography_ransac_gpu.py
sets for H: with M's eigenvalue gap of at least 1e-2 both eigen-solvers are far inside it."""
import ctypes as C

import numpy as np
import pytest

import np_restatement_twopoint as npt
import twopoint_cases as tc
from svo_pro_universal_amd import _capi as capi, frontend as fe

pytestmark = pytest.mark.gpu


def problem_of(name):
    c, K = tc.case(name)
    return (c["f_cur"], c["f_ref"], c["R"], c["thresh"], c["seed"]), K


def check_against(r, mask, want, what):
    assert r.status == want["status"], what
    assert r.best_hypothesis == want["best_hypothesis"], what
    assert r.n_inliers_hypothesis == want["n_inliers_hypothesis"], what
    assert r.n_inliers == want["n_inliers"], what
    assert r.n_degenerate == want["n_degenerate"], what
    assert np.array_equal(mask, want["mask"]), what
    err = np.abs(np.array(r.t) - want["t"]).max()
    print("%s: best %d, %d -> %d inliers, %d degenerate, |dt| %.2e" % (what, r.best_hypothesis, r.n_inliers_hypothesis, r.n_inliers,
                                                                      r.n_degenerate, err))
    assert err <= 1e-9, (what, err)
    assert r.reserved == 0


@pytest.mark.parametrize("name", tc.CASE_NAMES)
def test_single_problem_equals_restatement(gpu_ctx, name):
    pb, K = problem_of(name)
    res, masks = gpu_ctx.translation_ransac([pb], capi.default_init_options(n_hypotheses=K))
    check_against(res[0], masks[0], tc.restated(name), name)


def as_bytes(r):
    return C.string_at(C.addressof(r), C.sizeof(r))


def test_ragged_batch_is_bit_identical_to_single_calls(gpu_ctx):
    pbs = [problem_of(nm)[0] for nm in tc.RAGGED_BATCH]
    opt = capi.default_init_options()
    res, masks = gpu_ctx.translation_ransac(pbs, opt)
    for i, nm in enumerate(tc.RAGGED_BATCH):
        one, m1 = gpu_ctx.translation_ransac([pbs[i]], opt)
        assert as_bytes(res[i]) == as_bytes(one[0]), nm
        assert np.array_equal(masks[i], m1[0]), nm
        check_against(res[i], masks[i], tc.restated(nm), "batch/" + nm)


def no_model(gpu_ctx, f_cur, f_ref, R, what):
    want = npt.estimate_translation_ransac(f_cur, f_ref, R, tc.THRESH, 99)
    assert want["status"] == npt.STATUS_NO_MODEL, what
    res, masks = gpu_ctx.translation_ransac([(f_cur, f_ref, R, tc.THRESH, 99)])
    r = res[0]
    assert r.status == capi.SVOH_TRANSLATION_NO_MODEL, what
    assert list(r.t) == [0.0] * 3, what
    assert (r.best_hypothesis, r.n_inliers_hypothesis, r.n_inliers, r.n_degenerate, r.reserved) == (0, 0, 0, 0, 0), what
    assert not masks[0].any(), what


def test_pure_rotation_gives_no_model(gpu_ctx):
    c = tc.make_case(55, 40, outlier_fraction=0.0)
    no_model(gpu_ctx, c["f_ref"] @ c["R"].T, c["f_ref"], c["R"], "pure rotation")


def test_identical_matches_give_no_model(gpu_ctx):
    c = tc.make_case(55, 40, outlier_fraction=0.0)
    no_model(gpu_ctx, np.tile(c["f_cur"][:1], (40, 1)), np.tile(c["f_ref"][:1], (40, 1)), c["R"], "identical")


def test_one_match_gives_no_model(gpu_ctx):
    c = tc.make_case(55, 40, outlier_fraction=0.0)
    no_model(gpu_ctx, c["f_cur"][:1], c["f_ref"][:1], c["R"], "n = 1")


def test_too_many_matches_is_an_error_and_leaves_the_results_untouched(gpu_ctx):
    f = np.zeros((1025, 3))
    ok, _ = tc.case("n3")
    pbs = (capi.svoh_translation_problem * 2)()
    arrays = [np.ascontiguousarray(ok["f_cur"]), np.ascontiguousarray(ok["f_ref"]), f]
    R = (C.c_double * 9)(*np.asarray(ok["R"]).ravel())
    pbs[0].n, pbs[0].f_cur, pbs[0].f_ref, pbs[0].R_cur_ref, pbs[0].thresh, pbs[0].seed = 3, arrays[0].ctypes.data, arrays[1].ctypes.data, R, ok["thresh"], 1
    pbs[1].n, pbs[1].f_cur, pbs[1].f_ref, pbs[1].R_cur_ref, pbs[1].thresh, pbs[1].seed = 1025, f.ctypes.data, f.ctypes.data, R, ok["thresh"], 1
    res = (capi.svoh_translation_result * 2)()
    C.memset(res, 0xAB, C.sizeof(res))
    masks = np.full(3 + 1025, 0xCD, np.uint8)
    opt = capi.default_init_options()
    rc = gpu_ctx.lib.svoh_translation_ransac_batch(gpu_ctx.h, C.byref(opt), 2, pbs, res, masks.ctypes.data)
    assert rc == capi.SVOH_ERR_INVALID_ARGUMENT
    assert b"1024" in gpu_ctx.lib.svoh_last_error_string(gpu_ctx.h)
    assert as_bytes(res) == b"\xab" * C.sizeof(res)
    assert (masks == 0xCD).all()
    with pytest.raises(fe.SvohError):
        gpu_ctx.translation_ransac([(f, f, ok["R"], ok["thresh"], 1)])


def test_a_nan_match_is_never_an_inlier(gpu_ctx):
    f_cur, f_ref, R, thresh, seed, k = tc.nan_case()
    want = npt.estimate_translation_ransac(f_cur, f_ref, R, thresh, seed)
    assert want["status"] == npt.STATUS_OK and want["n_degenerate"] > 0 and tc.premises_hold(want)
    res, masks = gpu_ctx.translation_ransac([(f_cur, f_ref, R, thresh, seed)])
    assert masks[0][k] == 0
    check_against(res[0], masks[0], want, "NaN match")


def test_kernel_time_is_reported(gpu_ctx):
    """svoh_last_kernel_ms after the call is this kernel's time (the session's context brackets every launch: frontend.Context)."""
    pb, _ = problem_of("n65")
    gpu_ctx.translation_ransac([pb])
    ms = C.c_float(-1.0)
    assert gpu_ctx.lib.svoh_last_kernel_ms(gpu_ctx.h, C.byref(ms)) == 0
    assert ms.value > 0.0
    print("translation_ransac_kernel, 65 matches, 2000 hypotheses: %.4f ms" % ms.value)
