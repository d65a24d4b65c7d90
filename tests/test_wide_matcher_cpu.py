"""Premises of tests/test_wide_matcher_gpu.py, held without a GPU: the cases of tests/wide_matcher.py exercise several
outcomes, would notice a camera model read wrongly, and their integer outputs do not hang on the last bits of atan / tan
(the device's are ocml's, the NumPy reading's are libm's) -- which is what lets the GPU tests ask for exact integers.

The ATAN parameter check of the three entries (s zero or not finite) sits behind the frame-handle lookup of a live
context and cannot be reached without a device: it is in the GPU file."""
import numpy as np
import pytest

import np_restatement_direct as nd
import wide_matcher as wm


# ---- 1. outcome variety ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", wm.CAMERAS)
def test_outcome_variety(kind):
    g = wm.seeds_reference(kind)[0]
    codes = set(g["match_result"].tolist())
    print("%s: match results %s, %d of %d succeed" % (kind, sorted(codes), int(g["success"].sum()), wm.N_UNITS))
    assert len(codes) >= 4
    assert g["success"].sum() > wm.N_UNITS // 2
    d = wm.direct_reference(kind)
    assert len(set(d["result"].tolist())) >= 3 and (d["result"] == nd.SUCCESS).sum() > wm.N_UNITS // 2
    s = wm.seam_reference(kind)
    assert len(set(s["result"].tolist())) >= 2 and (s["result"] == nd.SUCCESS).sum() > wm.N_SEAM // 2


# ---- 2. discriminating: the parameters misread as radtan ---------------------------------------------------------------
def test_misreading_the_equidistant_parameters_as_radtan_shows():
    good = wm.seeds_reference("equidistant")[0]
    bad = wm.seeds_reference("equidistant", cam_of=wm.cam_misread_as_radtan)[0]
    a, b = good["state"].reshape(-1, 4), bad["state"].reshape(-1, 4)
    rel = (np.abs(a - b) / np.maximum(np.abs(a), 1e-300)).max(axis=1)
    differ = (good["match_result"] != bad["match_result"]) | (rel > 1e-6)
    print("misread as radtan: %d of %d units differ" % (int(differ.sum()), wm.N_UNITS))
    assert differ.mean() >= 0.1


# ---- 3. rounding stability of the reference ----------------------------------------------------------------------------
def _integers_equal(a, b, keys):
    return all(np.array_equal(a[k], b[k]) for k in keys)


@pytest.mark.parametrize("cam_of", [wm.cam_rounded_up, wm.cam_rounded_down])
@pytest.mark.parametrize("kind", wm.CAMERAS)
def test_reference_integers_do_not_hang_on_the_last_bits_of_the_camera(kind, cam_of):
    """distort / undistort scaled by (1 +- 8 * 2^-52): result codes, success flags, types and search levels identical."""
    worst = 0.0
    for base, moved in zip(wm.seeds_reference(kind), wm.seeds_reference(kind, cam_of=cam_of)):
        assert _integers_equal(base, moved, ("match_result", "success", "type", "search_level"))
        a, b = base["state"].reshape(-1, 4), moved["state"].reshape(-1, 4)
        worst = max(worst, float((np.abs(a - b) / np.maximum(np.abs(a), 1e-300)).max()))
    for pixelwise in (False, True):
        assert _integers_equal(wm.direct_reference(kind, pixelwise), wm.direct_reference(kind, pixelwise, cam_of=cam_of),
                               ("result", "search_level"))
    for per_feature in (False, True):
        assert _integers_equal(wm.seam_reference(kind, per_feature), wm.seam_reference(kind, per_feature, cam_of=cam_of), ("result",))
    print("%s: largest relative state change under the perturbation %.1e" % (kind, worst))
    assert worst < 1e-8 / 10        # an order of magnitude inside the GPU file's state tolerance


@pytest.mark.parametrize("sphere,option_set", [(0, 1), (0, 2), (1, 0), (1, 1), (1, 2)])
@pytest.mark.parametrize("kind", wm.CAMERAS)
def test_seed_reference_integers_are_stable_in_the_other_option_sets(kind, sphere, option_set):
    """The seed update's other scans and option sets of the GPU file, both directions of the perturbation."""
    tol = 1e-5 if wm.SEED_OPTION_SETS[option_set][0].get("affine_est_gain") else 1e-8
    for cam_of in (wm.cam_rounded_up, wm.cam_rounded_down):
        for base, moved in zip(wm.seeds_reference(kind, sphere, option_set), wm.seeds_reference(kind, sphere, option_set, cam_of=cam_of)):
            assert _integers_equal(base, moved, ("match_result", "success", "type", "search_level"))
            a, b = base["state"].reshape(-1, 4), moved["state"].reshape(-1, 4)
            assert (np.abs(a - b) / np.maximum(np.abs(a), 1e-300)).max() < tol / 10


def test_mixed_pair_reference_integers_are_stable_too():
    for cam_of in (wm.cam_rounded_up, wm.cam_rounded_down):
        for base, moved in zip(wm.seeds_reference("mixed"), wm.seeds_reference("mixed", cam_of=cam_of)):
            assert _integers_equal(base, moved, ("match_result", "success", "type", "search_level"))
        assert _integers_equal(wm.direct_reference("mixed"), wm.direct_reference("mixed", cam_of=cam_of), ("result", "search_level"))
        assert _integers_equal(wm.seam_reference("mixed"), wm.seam_reference("mixed", cam_of=cam_of), ("result",))
