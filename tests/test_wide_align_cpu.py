"""tests/wide_align.py, the NumPy reading that checks the alignment on equidistant and atan cameras (no GPU here):
tied to the C oracle where the oracle has the camera (radtan, both Jacobian branches), and the conditions on the inputs
of tests/test_wide_align_gpu.py under which that file may ask for exact discrete results."""
import numpy as np
import pytest

from svo_pro_universal_amd import _capi as capi, synth

import helpers
import wide_align as wa
import wide_geometry as wg


# ---- the reading against the existing yardstick: radtan, where the oracle has the camera -----------------------------
@pytest.mark.parametrize("dist_jac", [0, 1])
@pytest.mark.parametrize("P", [4, 8])
def test_reading_agrees_with_the_oracle_on_radtan(oracle_lib, P, dist_jac):
    """Discrete outputs exact; H, g to 1e-9 of their largest entry (tests/test_oracle_cpu.py's bound between the oracle and
    np_restatement.evaluate), pose / alpha 1e-9 and beta 1e-7 (tests/test_np_second_opinion_cpu.py, _gn_compare)."""
    orc = oracle_lib
    sc = wa.scene("radtan", 313, 220, P, 40)[0]
    ref, cur = helpers.scene_pyramids(orc, sc)
    assert all(np.array_equal(a, b) for a, b in zip(ref, wa.n0.create_img_pyramid(sc.img_ref, 5)))
    cams = [(sc, ref, cur)]
    T, a, b = wa.eval_state(sc)
    for illum, robust in ((0, 0), (1, 0), (1, 1)):
        opt = capi.default_align_options(patch_size=P, min_level=0, estimate_illumination_gain=illum, estimate_illumination_offset=illum,
                                         robustification=robust, use_distortion_jacobian=dist_jac)
        pb = orc.problem_from_scenes(cams, T_init=T, alpha_init=a, beta_init=b)
        for level in wa.EVAL_LEVELS:
            Ho, go, c2o, nmo, viso = orc.sparse_align_evaluate(opt, pb, level)
            Hn, gn, c2n, nmn, visn, nsel = wa.evaluate_bundle(cams, level, P, wa._tf(T), max_level=4, alpha=a, beta=b, est_alpha=bool(illum),
                                                              est_beta=bool(illum), robust=bool(robust), dist_jac=bool(dist_jac))
            assert nmo == nmn and nsel == len(viso) and np.array_equal(viso, visn)
            assert 0 < visn.sum() < len(visn) or level != 0
            assert np.abs(Ho - Hn).max() <= 1e-9 * np.abs(Hn).max()
            assert np.abs(go - gn).max() <= 1e-9 * np.abs(gn).max()
            assert abs(c2o - c2n) <= 1e-4 * c2n
        n, ro, _ = orc.sparse_align_run(opt, orc.problem_from_scenes(cams, T_init=wa.start_state(sc)))
        rn = wa.run(cams, opt, wa.start_state(sc))
        assert n == rn["n_fts_to_track"] and ro.status == rn["status"] and ro.n_patch_iters == rn["n_patch_iters"]
        assert list(ro.iters) == rn["iters"] and list(ro.n_meas) == rn["n_meas"]
        qo = np.array([ro.T_icur_iref.q[i] for i in range(4)]); to = np.array([ro.T_icur_iref.t[i] for i in range(3)])
        dq = min(np.abs(qo - rn["T"].q).max(), np.abs(qo + rn["T"].q).max())
        assert max(dq, np.abs(to - rn["T"].t).max()) < 1e-9
        assert abs(ro.alpha - rn["alpha"]) < 1e-9 and abs(ro.beta - rn["beta"]) < 1e-7


def test_reading_agrees_with_the_oracle_on_a_rig_with_a_prior(oracle_lib):
    """Two cameras with extrinsics of their own add into one H, one g; applyPrior on top."""
    orc = oracle_lib
    a = wa.scene("radtan", 313, 150, 4, 30)
    b = wa.rig_partner(a[0], "radtan", 343, 100)
    cams = [a, b]
    p_c, p_np = wa.weighted_prior(a[0])
    opt = capi.default_align_options(min_level=1, estimate_illumination_gain=1, estimate_illumination_offset=1)
    n, ro, _ = orc.sparse_align_run(opt, orc.problem_from_scenes(cams, prior=p_c, T_init=wa.start_state(a[0])))
    rn = wa.run(cams, opt, wa.start_state(a[0]), prior=p_np)
    assert n == rn["n_fts_to_track"] and ro.status == rn["status"] == 0 and ro.n_patch_iters == rn["n_patch_iters"]
    assert list(ro.iters) == rn["iters"] and list(ro.n_meas) == rn["n_meas"] and sum(rn["iters"]) >= 4
    assert helpers.se3_max_abs_diff(ro.T_icur_iref, orc.to_se3(synth.SE3(rn["T"].q, rn["T"].t))) < 1e-9
    assert abs(ro.alpha - rn["alpha"]) < 1e-9 and abs(ro.beta - rn["beta"]) < 1e-7


# ---- the inputs of the GPU tests -----------------------------------------------------------------------------------
def _conditions(probe, run_to_level0):
    assert probe.bound >= 1e-6, probe.bound          # no projected patch corner (no depth) within 1e-6 of a visibility bound
    assert probe.eps >= 1e-6, probe.eps              # no max|dx| within 1e-6 (relative) of eps
    if run_to_level0:
        assert probe.vis_level0 and all(v > 0 and i > 0 for v, i in probe.vis_level0), probe.vis_level0


@pytest.mark.parametrize("P", [4, 8])
@pytest.mark.parametrize("kind", wa.KINDS)
def test_inputs_of_the_evaluations(kind, P):
    for opt in wa.option_sets(kind, P):
        for level in wa.EVAL_LEVELS:
            (H, g, chi2, nm, vis, nsel), probe = wa.eval_reference(kind, wa.opt_key(opt), level)
            _conditions(probe, level == 0)
            assert nsel > 512 and nsel % 512 != 0      # a second, partial round of the workgroup's 512 lanes
            assert 0 < vis.sum() and nm == int(vis.sum()) * P * P
            assert np.isfinite(H).all() and np.abs(g[:6]).min() > 0
    assert wa.eval_scene(kind, P)[0].n_features > nsel  # border features the selection rejects


@pytest.mark.parametrize("P", [4, 8])
@pytest.mark.parametrize("kind", wa.KINDS)
def test_inputs_of_the_full_runs(kind, P):
    moved = 0
    for opt in wa.option_sets(kind, P):
        for with_prior in ((False, True) if opt.use_distortion_jacobian == 0 and opt.robustification == 0 else (False,)):
            r, probe = wa.run_reference(kind, wa.opt_key(opt), with_prior)
            _conditions(probe, True)
            assert r["status"] == 0 and 100 < r["n_fts_to_track"] < wa.run_scene(kind, P)[0].n_features
            assert all(r["iters"][l] >= 1 for l in range(5))
            moved += sum(r["iters"])
    assert moved > 40


def test_inputs_of_the_ragged_launch_and_the_odd_size():
    pbs = wa.ragged_problems()
    assert tuple(pbs) == wa.RAGGED_ORDER
    for name in wa.RAGGED_ORDER:
        r, probe = wa.ragged_reference(name)
        # both visible and invisible features at level 0: not the problem of one feature, nor the one without a feature
        _conditions(probe, name not in ("one_feature", "no_flagged"))
        assert r["status"] == (1 if name == "no_flagged" else 0)
    assert wa.ragged_reference("one_feature")[0]["n_fts_to_track"] == 1 and wa.ragged_reference("no_flagged")[0]["n_fts_to_track"] == 0
    rig = pbs["rig"]["cams"]
    assert rig[0][0].cam.model == "radtan" and rig[1][0].cam.model == "equidistant"
    assert helpers.se3_max_abs_diff(helpers_se3(rig[0][0].T_cam_imu), helpers_se3(rig[1][0].T_cam_imu)) > 1e-3     # different extrinsics
    r, probe = wa.odd_reference()
    _conditions(probe, True)
    sc = wa.odd_scene()[0]
    assert (sc.cam.width, sc.cam.height) == wa.ODD_SIZE and r["status"] == 0 and r["n_fts_to_track"] > 60
    assert [lv.shape for lv in wa.odd_scene()[1]] == [(309, 413), (154, 206), (77, 103), (38, 51)]   # levels that truncate


def helpers_se3(T):
    from oracle import oracle as orc
    return orc.to_se3(T)
