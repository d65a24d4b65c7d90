"""svoh_essential_ransac_batch (csrc/essential.hip) against its NumPy restatement (tests/np_restatement_fivepoint.py).

The status, the winning hypothesis, both counts, the number of degenerate hypotheses, the iterations of the refinement
and the mask are compared exactly: tests/test_fivepoint_cpu.py asserts for every case used here that the restatement, run
with two different bases of the null space, decides all of them alike, and that no error that could change one lies
closer to the threshold than a thousand times what the two runs differ by.  best_candidate is a position among roots
whose order depends on the basis of the null space, and n_models counts candidates of ill-conditioned samples too: both are
only bounded.  R and t are compared to fivepoint_cases.MODEL_BAR = 1e-9: a hundred times the largest difference between
the restatement's two runs (4.5e-15) is below the 1e-9 of the other two estimators, which therefore holds.  At n = 5 and
n = 6 several essential matrices fit: the model is checked for what it must be, not compared."""
import ctypes as C

import numpy as np
import pytest

import np_restatement_fivepoint as np5
import fivepoint_cases as fc
from svo_pro_universal_amd import _capi as capi, frontend as fe

pytestmark = pytest.mark.gpu


def problem_of(name):
    c, K = fc.case(name)
    return (c["f_cur"], c["f_ref"], c["thresh"], c["seed"]), K


def check_against(r, mask, want, what, pb, K, model_unique=True):
    f_cur, f_ref, thresh, _ = pb
    R, t = np.array(r.R).reshape(3, 3), np.array(r.t)
    print("%s: best %d/%d, %d -> %d inliers, %d degenerate, %d models (restatement %d), %d iterations" % (
        what, r.best_hypothesis, r.best_candidate, r.n_inliers_hypothesis, r.n_inliers, r.n_degenerate, r.n_models, want["n_models"], r.refine_iters))
    assert r.status == want["status"], what
    assert r.n_inliers_hypothesis == want["n_inliers_hypothesis"], what
    assert r.n_inliers == want["n_inliers"], what
    assert r.n_degenerate == want["n_degenerate"], what
    assert np.array_equal(mask, want["mask"]), what
    assert 0 < r.n_models <= 10 * K and 0 <= r.best_candidate < 10, what
    assert list(r.reserved) == [0, 0]
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-9 and np.linalg.det(R) > 0 and abs(np.linalg.norm(t) - 1.0) < 1e-9, what
    if model_unique:
        assert r.best_hypothesis == want["best_hypothesis"], what
        assert r.refine_iters == want["refine_iters"], what
        err = max(np.abs(R - want["R"]).max(), np.abs(t - want["t"]).max())
        print("%s: |d(R, t)| %.2e" % (what, err))
        assert err <= fc.MODEL_BAR, (what, err)
    else:
        assert 0 <= r.best_hypothesis < K and 1 <= r.refine_iters <= 10, what
        assert np5.inliers(R[None], t[None], np.asarray(f_cur), np.asarray(f_ref), thresh)[0].all(), what


@pytest.mark.parametrize("name", fc.CASE_NAMES)
def test_single_problem_equals_restatement(gpu_ctx, name):
    pb, K = problem_of(name)
    res, masks = gpu_ctx.essential_ransac([pb], capi.default_init_options(n_hypotheses=K))
    check_against(res[0], masks[0], fc.restated(name), name, pb, K, name not in fc.MODEL_NOT_UNIQUE)


def as_bytes(r):
    return C.string_at(C.addressof(r), C.sizeof(r))


def test_ragged_batch_is_bit_identical_to_single_calls(gpu_ctx):
    """One hypothesis count for the whole batch (512, that of the size cases); 'plane' therefore against a restatement at 512
    of its own only for being byte-identical, the others against the shared ones."""
    pbs = [problem_of(nm)[0] for nm in fc.RAGGED_BATCH]
    opt = capi.default_init_options(n_hypotheses=fc.K_FOR_SIZES)
    res, masks = gpu_ctx.essential_ransac(pbs, opt)
    for i, nm in enumerate(fc.RAGGED_BATCH):
        one, m1 = gpu_ctx.essential_ransac([pbs[i]], opt)
        assert as_bytes(res[i]) == as_bytes(one[0]), nm
        assert np.array_equal(masks[i], m1[0]), nm
        if fc.shape_of(nm)[1] == fc.K_FOR_SIZES:
            check_against(res[i], masks[i], fc.restated(nm), "batch/" + nm, pbs[i], fc.K_FOR_SIZES, nm not in fc.MODEL_NOT_UNIQUE)


def no_model(gpu_ctx, f_cur, f_ref, what):
    want = np5.estimate_essential_ransac(f_cur, f_ref, fc.THRESH, 99)
    assert want["status"] == np5.STATUS_NO_MODEL, what
    res, masks = gpu_ctx.essential_ransac([(f_cur, f_ref, fc.THRESH, 99)])
    r = res[0]
    assert r.status == capi.SVOH_ESSENTIAL_NO_MODEL, what
    assert list(r.R) == [0.0] * 9 and list(r.t) == [0.0] * 3, what
    assert (r.best_hypothesis, r.best_candidate, r.n_inliers_hypothesis, r.n_inliers, r.n_degenerate, r.n_models, r.refine_iters) == (0, ) * 7, what
    assert list(r.reserved) == [0, 0], what
    assert not masks[0].any(), what


def test_pure_rotation_gives_no_model(gpu_ctx):
    no_model(gpu_ctx, *fc.no_model_inputs()["pure rotation"], "pure rotation")


def test_identical_matches_give_no_model(gpu_ctx):
    no_model(gpu_ctx, *fc.no_model_inputs()["identical matches"], "identical")


def test_four_matches_give_no_model(gpu_ctx):
    no_model(gpu_ctx, *fc.no_model_inputs()["n = 4"], "n = 4")


def test_too_many_matches_is_an_error_and_leaves_the_results_untouched(gpu_ctx):
    f = np.zeros((1025, 3))
    ok, _ = fc.case("n6")
    pbs = (capi.svoh_essential_problem * 2)()
    arrays = [np.ascontiguousarray(ok["f_cur"]), np.ascontiguousarray(ok["f_ref"]), f]
    pbs[0].n, pbs[0].f_cur, pbs[0].f_ref, pbs[0].thresh, pbs[0].seed = 6, arrays[0].ctypes.data, arrays[1].ctypes.data, ok["thresh"], 1
    pbs[1].n, pbs[1].f_cur, pbs[1].f_ref, pbs[1].thresh, pbs[1].seed = 1025, f.ctypes.data, f.ctypes.data, ok["thresh"], 1
    res = (capi.svoh_essential_result * 2)()
    C.memset(res, 0xAB, C.sizeof(res))
    masks = np.full(6 + 1025, 0xCD, np.uint8)
    opt = capi.default_init_options()
    rc = gpu_ctx.lib.svoh_essential_ransac_batch(gpu_ctx.h, C.byref(opt), 2, pbs, res, masks.ctypes.data)
    assert rc == capi.SVOH_ERR_INVALID_ARGUMENT
    assert b"1024" in gpu_ctx.lib.svoh_last_error_string(gpu_ctx.h)
    assert as_bytes(res) == b"\xab" * C.sizeof(res)
    assert (masks == 0xCD).all()
    with pytest.raises(fe.SvohError):
        gpu_ctx.essential_ransac([(f, f, ok["thresh"], 1)])


def test_a_nan_match_is_never_an_inlier(gpu_ctx):
    f_cur, f_ref, thresh, seed, k = fc.nan_case()
    want = np5.estimate_essential_ransac(f_cur, f_ref, thresh, seed)
    assert want["status"] == np5.STATUS_OK and want["n_degenerate"] > 0
    res, masks = gpu_ctx.essential_ransac([(f_cur, f_ref, thresh, seed)])
    assert masks[0][k] == 0
    check_against(res[0], masks[0], want, "NaN match", (f_cur, f_ref, thresh, seed), 2000)


def test_kernel_time_is_reported(gpu_ctx):
    """svoh_last_kernel_ms after the call is this kernel's time (the session's context brackets every launch: frontend.Context)."""
    pb, _ = problem_of("n65")
    gpu_ctx.essential_ransac([pb])
    ms = C.c_float(-1.0)
    assert gpu_ctx.lib.svoh_last_kernel_ms(gpu_ctx.h, C.byref(ms)) == 0
    assert ms.value > 0.0
    print("essential_ransac_kernel, 65 matches, 2000 hypotheses: %.4f ms" % ms.value)
