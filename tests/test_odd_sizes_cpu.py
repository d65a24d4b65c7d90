"""The oracle at image sizes whose pyramid levels truncate (tests/odd_sizes.py): the hand-derived bounds of the selection
and of KLT on the oracle, and the oracle against the NumPy second opinion (tests/np_restatement_direct.py,
tests/np_restatement.py) at 413x309 -- the premise of tests/test_odd_sizes_gpu.py, which holds the kernels against this
oracle at these sizes."""
import ctypes as C

import numpy as np
import pytest

from svo_pro_universal_amd import _capi as capi, synth

import helpers
import np_restatement as n0
import np_restatement_direct as nd
import odd_sizes as od
from test_np_second_opinion_cpu import _nd_options, _views


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_level_sizes_are_the_oracles(oracle_lib, name):
    """every level is the integer half of the one before, on the oracle's pyramid as in odd_sizes.level_sizes"""
    w, h = od.SIZES[name]
    img = np.random.RandomState(w).randint(0, 256, (h, w)).astype(np.uint8)
    lv = oracle_lib.create_img_pyramid(img, od.N_LEVELS)
    assert [(a.shape[1], a.shape[0]) for a in lv] == od.level_sizes(w, h)
    pn = n0.create_img_pyramid(img, od.N_LEVELS)
    for a, b in zip(lv, pn):
        assert a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize("name", ["A", "B"])
def test_selection_boundaries(oracle_lib, name):
    """extractFeaturesSubset at level 4: the bounds of odd_sizes.SELECTION_PX, derived there from the level's integer size"""
    orc = oracle_lib
    sc = od.selection_scene(name)
    ref, cur = helpers.scene_pyramids(orc, sc)
    w4, h4 = od.level_sizes(*od.SIZES[name])[4]
    assert (ref[4].shape[1], ref[4].shape[0]) == (w4, h4)
    pb = orc.problem_from_scenes([(sc, ref, cur)])
    idx = np.zeros(sc.n_features, np.int32)
    n = orc.load().orc_extract_features_subset(C.byref(pb.c.cams[0]), 4, 6, idx.ctypes.data)
    assert sorted(idx[:n]) == [i for i, k in enumerate(od.SELECTION_KEPT) if k]
    # the same bounds from the rule itself, in integers
    for (x, y), kept in zip(od.SELECTION_PX[name], od.SELECTION_KEPT):
        u, v = int(np.floor(x / 16.0 - 2.5)), int(np.floor(y / 16.0 - 2.5))
        assert kept == (u >= 0 and v >= 0 and u + 6 < w4 - 2 and v + 6 < h4 - 2)


@pytest.mark.parametrize("name", ["A", "B"])
def test_klt_template_and_current_boundaries(oracle_lib, name):
    """alignPyr2D at level 0, 16x16 patch: reference pixels 8 | 9 and w - 10 | w - 9 (h likewise), a current corner at
    exactly w - 16 is lost, 0.01 inside it is tracked"""
    orc = oracle_lib
    sc = helpers.small_scene(62, n=10, cam=od.camera(name, "pinhole"))
    ref = orc.create_img_pyramid(sc.img_ref, od.N_LEVELS)
    opt = capi.default_klt_options(max_level=0, min_level=0)
    px_ref, px_cur, ok = od.klt_boundary_tracks(name)
    n = px_ref.size // 2
    po, so = orc.klt_track_batch(opt, [ref] * n, ref, px_ref, px_cur)   # same image on both sides: a track converges where it starts
    assert list(so[:8]) == ok
    assert so[8] == 0 and so[9] == 1
    assert np.array_equal(po.reshape(-1, 2)[[1, 2, 5, 6]], px_cur.reshape(-1, 2)[[1, 2, 5, 6]])


def _scene_a(cam_kind, seed):
    return synth.make_align_scene(seed, n_features=10, cam=od.camera("A", cam_kind), rot_deg=(0.5, 1.5), trans_m=(0.08, 0.2))


@pytest.mark.parametrize("cam_kind", ["pinhole", "radtan"])
def test_update_seeds_oracle_vs_numpy_second_opinion(oracle_lib, cam_kind):
    """test_np_second_opinion_cpu.test_update_seeds_oracle_vs_numpy_second_opinion at 413x309, 500 seeds at levels 0..3, two
    rounds: codes, success flags and types exact, state relative 1e-8; at least 4 result codes, more than half succeed."""
    orc = oracle_lib
    n = 500
    sc = _scene_a(cam_kind, 63)
    sd = synth.make_seed_set(sc, n, margin=3, levels=(0, 1, 2, 3))
    rv, cv, nrv, ncv = _views(orc, sc, sd, cam_kind)
    mopt, dopt = capi.default_matcher_options(scan_on_unit_sphere=int(cam_kind == "radtan")), capi.default_depth_filter_options(sc.cam)
    state = sd["state"].copy(); types = sd["type"].copy()
    for rnd in range(2):
        fb, keep = orc.make_feature_batch(sd["ref_frame_idx"], sd["px"], sd["f"], sd["grad"], sd["level"], types)
        ns, st_o, succ_o, mr_o = orc.update_seeds_batch(mopt, dopt, [rv], cv, fb, state)
        got = nd.update_seeds(ncv, [nrv], sd["ref_frame_idx"], sd["px"], sd["f"], sd["grad"], sd["level"], types, state,
                              _nd_options(mopt), dopt.seed_convergence_sigma2_thresh, dopt.mappoint_convergence_sigma2_thresh,
                              dopt.px_error_angle, bool(dopt.check_visibility), bool(dopt.check_convergence),
                              bool(dopt.use_vogiatzis_update))
        assert np.array_equal(mr_o, got["match_result"]), np.nonzero(mr_o != got["match_result"])[0][:10]
        assert np.array_equal(succ_o, got["success"])
        assert np.array_equal(keep["type"], got["type"])
        assert ns == int(got["success"].sum())
        a, b = st_o.reshape(-1, 4), got["state"].reshape(-1, 4)
        rel = np.abs(a - b) / np.maximum(np.abs(a), 1e-300)
        print("update_seeds %s round %d: %d codes, %d of %d succeed, state rel %.2e" % (cam_kind, rnd, len(set(mr_o.tolist())), succ_o.sum(), n, rel.max()))
        assert rel.max() <= 1e-8, (rel.max(), np.unravel_index(rel.argmax(), rel.shape))
        assert len(set(mr_o.tolist())) >= 4 and succ_o.sum() > 0.5 * n      # several failure kinds beside the successes
        state, types = st_o, keep["type"].copy()


@pytest.mark.parametrize("cam_kind", ["pinhole", "radtan"])
def test_match_direct_oracle_vs_numpy_second_opinion(oracle_lib, cam_kind):
    """test_np_second_opinion_cpu.test_match_direct_oracle_vs_numpy_second_opinion at 413x309, 500 units at levels 0..3:
    result codes exact, px_cur <= 1e-4; at least 3 result codes, more than half succeed, every search level 0..3 occurs."""
    orc = oracle_lib
    n = 500
    sc = synth.make_align_scene(64, n_features=10, cam=od.camera("A", cam_kind), rot_deg=(0.5, 1.5), trans_m=(0.05, 0.15))
    sd = synth.make_seed_set(sc, n, margin=3, levels=(0, 1, 2, 3))
    rv, cv, nrv, ncv = _views(orc, sc, sd, cam_kind)
    px_true, px_init = od.predicted_pixels(sc, sd, 2.0, 1)
    px_init[:20] += 40.0
    ftype = np.where(sd["type"] == 0, capi.FT_EDGELET, capi.FT_CORNER)
    for mkw in (dict(), dict(affine_est_gain=1)):
        mopt = capi.default_matcher_options(**mkw)
        fb, keep = orc.make_feature_batch(sd["ref_frame_idx"], sd["px"], sd["f"], sd["grad"], sd["level"], ftype)
        oo = orc.match_direct_batch(mopt, [rv], cv, fb, sd["true_depth"], px_init)
        gg = nd.match_direct_batch(ncv, [nrv], sd["ref_frame_idx"], sd["px"], sd["f"], sd["grad"], sd["level"], ftype,
                                   sd["true_depth"], px_init, _nd_options(mopt))
        assert np.array_equal(oo["result"], gg["result"]), np.nonzero(oo["result"] != gg["result"])[0][:10]
        ran = oo["result"] != nd.FAIL_VISIBILITY
        assert np.array_equal(oo["search_level"][ran], gg["search_level"][ran])
        ok = oo["result"] == 0
        print("match_direct %s %r: %d codes, %d of %d succeed, px_cur differs by %.2e" % (cam_kind, mkw, len(set(oo["result"].tolist())), ok.sum(), n,
                                                                                       np.abs(oo["px_cur"] - gg["px_cur"]).max()))
        assert ok.sum() > 0.5 * n and len(set(oo["result"].tolist())) >= 3
        assert set(oo["search_level"][ran].tolist()) >= {0, 1, 2, 3}
        assert np.abs(oo["px_cur"] - gg["px_cur"]).max() <= 1e-4
        assert np.allclose(oo["A"][np.repeat(ran, 4)], gg["A"][np.repeat(ran, 4)], rtol=1e-11, atol=1e-13)


@pytest.mark.parametrize("name,cam_kind,level", [("A", "pinhole", 3), ("A", "radtan", 1), ("C", "pinhole", 2)])
def test_evaluate_matches_numpy_restatement(oracle_lib, name, cam_kind, level):
    """The alignment's H / g restatement (np_restatement.evaluate, the per-iteration part of np_restatement_gn) takes the
    scene's camera and the pyramid's arrays, so it runs at any size: test_oracle_cpu.test_evaluate_matches_numpy_restatement
    with its bars (visibility and n_meas exact, H and g relative 1e-9) at A and -- 8x8 patches -- C."""
    orc = oracle_lib
    P = od.PATCH[name]
    sc = od.align_scene(name, cam_kind, 11, n=250, border_features=40)
    ref, cur = helpers.scene_pyramids(orc, sc)
    for illum, robust in ((0, 0), (1, 1)):
        opt = capi.default_align_options(patch_size=P, min_level=0, estimate_illumination_gain=illum,
                                         estimate_illumination_offset=illum, robustification=robust)
        pb = orc.problem_from_scenes([(sc, ref, cur)], alpha_init=0.01 * illum, beta_init=0.5 * illum)
        H, g, chi2, nm, vis = orc.sparse_align_evaluate(opt, pb, level)
        H2, g2, chi22, nm2, vis2 = n0.evaluate(sc, ref, cur, level, P, sc.T_icur_iref_init.q, sc.T_icur_iref_init.t,
                                               alpha=0.01 * illum, beta=0.5 * illum, est_alpha=bool(illum),
                                               est_beta=bool(illum), robust=bool(robust))
        assert nm == nm2 and nm > 0 and np.array_equal(vis, vis2)
        assert np.abs(H - H2).max() <= 1e-9 * np.abs(H2).max()
        assert np.abs(g - g2).max() <= 1e-9 * np.abs(g2).max()
        assert abs(chi2 - chi22) <= 1e-4 * chi22


def test_crafted_visibility_premise(oracle_lib):
    """odd_sizes.add_edge_visibility_features: on the oracle the visible count differs between levels and is below the
    selected count; each crafted feature is visible exactly where the integer level size says."""
    orc = oracle_lib
    sc = od.align_scene("A", "pinhole", 74, border_features=0, invalid_fraction=0.0)
    n0_feat = sc.n_features
    targets = od.add_edge_visibility_features(sc)
    ref, cur = helpers.scene_pyramids(orc, sc)
    pb = orc.problem_from_scenes([(sc, ref, cur)])
    opt = capi.default_align_options(min_level=0)
    lv = od.level_sizes(*od.SIZES["A"])
    n_vis, disagree = {}, 0
    for level in (4, 3, 2, 1, 0):
        H, g, chi2, nm, vis = orc.sparse_align_evaluate(opt, pb, level)
        assert vis.size == sc.n_features          # every feature is selected (the crafted ones sit on selected pixels)
        n_vis[level] = int(vis.sum())
        s = 1.0 / (1 << level)
        for t, v in zip(targets, vis[n0_feat:]):
            want = all(c * s - 1.5 >= 0.0 and c * s - 1.5 + 6.0 < dim for c, dim in zip(t, lv[level]))
            assert bool(v) == want, (level, t)
            real = all(c * s - 1.5 >= 0.0 and c * s - 1.5 + 6.0 < dim0 * s for c, dim0 in zip(t, od.SIZES["A"]))
            disagree += int(real != want)
    assert len(set(n_vis.values())) >= 2 and min(n_vis.values()) < sc.n_features, n_vis
    assert disagree >= 5      # pixels on which a real-valued level size would decide the other way
