"""svoh_essential_ransac_batch, svoh_translation_ransac_batch and svoh_homography_ransac_batch on the motion grid of
tests/motion_cases.py (100 matches, 512 hypotheses): forward and backward motion, exactly no rotation, axis-aligned
translations, rotations of 20, 45 and exactly 90 degrees, a baseline of 1 cm, noise-free matches, bearings behind the image
plane, planes approached and passed.  Every case is checked by check_against of the estimator's own GPU test: status,
winner, both counts, n_degenerate, refine_iters and the mask exactly, R and t (H) to 1e-9; tests/test_motion_grid_cpu.py
asserts the premises of that for every case.  The property-only cases (motion_cases.PROPERTY_ONLY_E, each with its reason)
are checked against the planted motion instead."""
import numpy as np
import pytest

import motion_cases as mc
import test_essential_ransac_gpu as ge
import test_homography_ransac_gpu as gh
import test_translation_ransac_gpu as gt
from svo_pro_universal_amd import _capi as capi
from test_motion_grid_cpu import check_properties_e

pytestmark = pytest.mark.gpu


def problem_e(name):
    c = mc.case_e(name)
    return (c["f_cur"], c["f_ref"], c["thresh"], c["seed"])


def problem_t(name):
    c = mc.case_t(name)
    return (c["f_cur"], c["f_ref"], c["R"], c["thresh"], c["seed"])


def problem_h(name):
    c = mc.case_h(name)
    return (c["uv_ref"], c["uv_cur"], c["thresh_h"], c["seed"])


def options():
    return capi.default_init_options(n_hypotheses=mc.K)


def check_e(r, mask, name, what):
    if name in mc.PROPERTY_ONLY_E:
        a, b = mc.restated_e(name), mc.restated_e(name, True)
        print("%s: best %d, %d degenerate (restatement %d and %d)" % (what, r.best_hypothesis, r.n_degenerate, a["n_degenerate"], b["n_degenerate"]))
        check_properties_e(mc.case_e(name), a, b, r.status, r.n_degenerate, mask, np.array(r.R).reshape(3, 3), np.array(r.t), what)
    else:
        ge.check_against(r, mask, mc.restated_e(name), what, problem_e(name), mc.K, name not in mc.MODEL_NOT_UNIQUE)


@pytest.mark.parametrize("name", mc.BEARING_CASES)
def test_essential_equals_restatement(gpu_ctx, name):
    res, masks = gpu_ctx.essential_ransac([problem_e(name)], options())
    check_e(res[0], masks[0], name, name)


@pytest.mark.parametrize("name", mc.BEARING_CASES)
def test_translation_equals_restatement(gpu_ctx, name):
    assert name not in mc.PROPERTY_ONLY_T
    res, masks = gpu_ctx.translation_ransac([problem_t(name)], options())
    gt.check_against(res[0], masks[0], mc.restated_t(name), name)


@pytest.mark.parametrize("name", mc.PLANE_CASES)
def test_homography_equals_restatement(gpu_ctx, name):
    res, masks = gpu_ctx.homography_ransac([problem_h(name)], options())
    gh.check_against(res[0], masks[0], mc.restated_h(name), name)


def test_essential_ragged_batch_of_mixed_motions_is_bit_identical_to_single_calls(gpu_ctx):
    pbs = [problem_e(nm) for nm in mc.RAGGED_BATCH]
    res, masks = gpu_ctx.essential_ransac(pbs, options())
    for i, nm in enumerate(mc.RAGGED_BATCH):
        one, m1 = gpu_ctx.essential_ransac([pbs[i]], options())
        assert ge.as_bytes(res[i]) == ge.as_bytes(one[0]), nm
        assert np.array_equal(masks[i], m1[0]), nm
        check_e(res[i], masks[i], nm, "batch/" + nm)


def test_translation_ragged_batch_of_mixed_motions_is_bit_identical_to_single_calls(gpu_ctx):
    pbs = [problem_t(nm) for nm in mc.RAGGED_BATCH]
    res, masks = gpu_ctx.translation_ransac(pbs, options())
    for i, nm in enumerate(mc.RAGGED_BATCH):
        one, m1 = gpu_ctx.translation_ransac([pbs[i]], options())
        assert gt.as_bytes(res[i]) == gt.as_bytes(one[0]), nm
        assert np.array_equal(masks[i], m1[0]), nm
        gt.check_against(res[i], masks[i], mc.restated_t(nm), "batch/" + nm)


def test_homography_ragged_batch_of_mixed_motions_is_bit_identical_to_single_calls(gpu_ctx):
    pbs = [problem_h(nm) for nm in mc.RAGGED_BATCH_PLANE]
    res, masks = gpu_ctx.homography_ransac(pbs, options())
    for i, nm in enumerate(mc.RAGGED_BATCH_PLANE):
        one, m1 = gpu_ctx.homography_ransac([pbs[i]], options())
        assert gh.as_bytes(res[i]) == gh.as_bytes(one[0]), nm
        assert np.array_equal(masks[i], m1[0]), nm
        gh.check_against(res[i], masks[i], mc.restated_h(nm), "batch/" + nm)
