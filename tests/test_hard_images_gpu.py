"""The kernels that read pixels against the CPU oracle on degenerate image content (tests/hard_images.py: flat, striped,
checkered, blocky, ramped, saturated and noisy frame pairs with the units placed by class): pyramid, KLT, the depth filter's seed
update with both epipolar scans, the direct matcher with both warps and the stereo seam's epipolar match, in every matcher
geometry and both KLT block sizes.  tests/test_hard_images_cpu.py shows on the CPU that the cases are what they claim, that the
oracle agrees with the NumPy second opinion on them and that the periodic families tie.

Bars: pyramid bytes, KLT status and position (NaN as NaN), result codes, success flags, types and search levels exact; seed
states relative 1e-9; matched pixels 1e-4 px; the stereo seam's bars are those of
test_klt_matcher_gpu.py::test_epipolar_match_batch_parity_stereo_seam.  No unit is left out."""
import contextlib
import os

import numpy as np
import pytest

from svo_pro_universal_amd import _capi as capi, frontend as fe

import hard_images as hi

pytestmark = pytest.mark.gpu

GEOMETRIES = {"eight_lanes_per_unit": "1", "one_lane_per_unit": "0", "packed": "2", "one_wave_per_unit": "3"}
KLT_OPTION_SETS = (dict(), dict(patch_sizes=[8, 8, 16, 16, 8]), dict(max_iter=3))
MATCH_FAIL_ANGLE = 7      # SVOH_MATCH_FAIL_ANGLE (Matcher::MatchResult::kFailAngle): rejected by the edgelet filter


@contextlib.contextmanager
def knob(gpu_ctx, name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    gpu_ctx.reload_knobs()
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old
        gpu_ctx.reload_knobs()


@pytest.fixture(params=list(GEOMETRIES))
def matcher_geometry(request, gpu_ctx):
    with knob(gpu_ctx, "SVOH_MATCHER_G8", GEOMETRIES[request.param]):
        yield request.param


@pytest.fixture(params=["64", "256"])
def klt_block(request, gpu_ctx):
    with knob(gpu_ctx, "SVOH_KLT_BLOCK", request.param):
        yield request.param


_FRAMES, _ORACLE = {}, {}


def frames(gpu_ctx, name):
    """the case's two device pyramids, built once"""
    if name not in _FRAMES:
        p = hi.pair(name)
        _FRAMES[name] = (gpu_ctx.build_pyramid(p.img_ref, hi.N_LEVELS), gpu_ctx.build_pyramid(p.img_cur, hi.N_LEVELS))
    return _FRAMES[name]


def oracle_once(key, fn):
    """the oracle's answer, computed once and shared by the geometries; handed out as it is, never written to"""
    if key not in _ORACLE:
        _ORACLE[key] = fn()
    return _ORACLE[key]


def views(orc, gpu_ctx, name, mu_range):
    p = hi.pair(name)
    fr, fc = frames(gpu_ctx, name)
    return (orc.make_frame_view(p.ref, p.cam, p.T_ref_f_w, mu_range, 1), orc.make_frame_view(p.cur, p.cam, p.T_cur_f_w, 0.0, 2),
            fe.make_frame_view(fr, p.cam, p.T_ref_f_w, mu_range, 1), fe.make_frame_view(fc, p.cam, p.T_cur_f_w, 0.0, 2))


def same_bits(a, b):
    """equal arrays, a NaN equal to a NaN (and an inf only to the inf of its sign)"""
    return np.array_equal(a, b, equal_nan=True)


def test_pyramid_every_byte(gpu_ctx, oracle_lib):
    for name in hi.CASE_NAMES:
        p = hi.pair(name)
        for img, lv_n in ((p.img_ref, p.ref), (p.img_cur, p.cur)):
            _f, lv_g = gpu_ctx.build_pyramid(img, hi.N_LEVELS, return_levels=True)
            lv_o = oracle_lib.create_img_pyramid(img, hi.N_LEVELS)
            assert len(lv_g) == hi.N_LEVELS
            for g, o, n in zip(lv_g, lv_o, lv_n):
                assert g.shape == o.shape and np.array_equal(g, o) and np.array_equal(o, n), name


def run_klt(gpu_ctx, name, kw):
    fr, fc = frames(gpu_ctx, name)
    tr = hi.klt_tracks(name)
    return gpu_ctx.klt_track_batch(capi.default_klt_options(max_level=3, **kw), fr, fc, tr["px_ref"], tr["px_cur_init"])


def test_klt_status_and_position_bits(gpu_ctx, oracle_lib, klt_block):
    for name in hi.CASE_NAMES:
        p = hi.pair(name)
        tr = hi.klt_tracks(name)
        for k, kw in enumerate(KLT_OPTION_SETS):
            po, so = oracle_once(("klt", name, k), lambda: oracle_lib.klt_track_batch(
                capi.default_klt_options(max_level=3, **kw), p.ref, p.cur, tr["px_ref"], tr["px_cur_init"]))
            pg, sg = run_klt(gpu_ctx, name, kw)
            assert np.array_equal(so, sg), (name, kw, np.nonzero(so != sg)[0][:10])
            assert same_bits(po, pg), (name, kw, np.nonzero(~((po == pg) | ((po != po) & (pg != pg))))[0][:10])


def test_klt_block_sizes_bit_identical(gpu_ctx):
    out = {}
    for blk in ("64", "256"):
        with knob(gpu_ctx, "SVOH_KLT_BLOCK", blk):
            out[blk] = [run_klt(gpu_ctx, name, kw) for name in hi.CASE_NAMES for kw in KLT_OPTION_SETS]
    for (pa, sa), (pb, sb) in zip(out["64"], out["256"]):
        assert np.array_equal(sa, sb) and same_bits(pa, pb)


SEED_OPTION_SETS = [(sphere, vog) for sphere in (0, 1) for vog in (1, 0)]


def seed_options(name, sphere, vog):
    return (capi.default_matcher_options(scan_on_unit_sphere=sphere, max_epi_search_steps=500),
            capi.default_depth_filter_options(hi.pair(name).cam, use_vogiatzis_update=vog))


def run_seeds(update, make_batch, ref_view, cur_view, name, sphere, vog):
    """two rounds with the state and the types fed back; per round (n_success, state in, state out, success, codes, types)"""
    sd = hi.seed_set(name)
    mopt, dopt = seed_options(name, sphere, vog)
    state, types, rounds = sd["state"].copy(), sd["type"].copy(), []
    for _rnd in range(2):
        fb, keep = make_batch(sd["ref_frame_idx"], sd["px"], sd["f"], sd["grad"], sd["level"], types)
        ns, st, succ, mr = update(mopt, dopt, [ref_view], cur_view, fb, state)
        rounds.append((int(ns), state.copy(), st.copy(), succ.copy(), mr.copy(), types.copy(), keep["type"].copy()))
        state, types = st.copy(), keep["type"].copy()
    return rounds


def check_untouched(rnd):
    """a seed that was not updated keeps its state bit for bit, apart from the reference's b + 1 behind a failed match that was
    not rejected by the edgelet filter (depth_filter.cpp: seed::increaseOutlierProbability)"""
    _ns, st_in, st_out, succ, mr, t_in, t_out = rnd
    a, b = st_in.reshape(-1, 4), st_out.reshape(-1, 4)
    untouched = (succ == 0) & ((t_out != capi.FT_OUTLIER) | (t_in == capi.FT_OUTLIER))
    assert same_bits(a[untouched, :3], b[untouched, :3])
    inc = np.where((mr == capi.MATCH_NOT_RUN) | (mr == MATCH_FAIL_ANGLE), 0.0, 1.0)
    assert same_bits(a[untouched, 3] + inc[untouched], b[untouched, 3])


def test_update_seeds(gpu_ctx, oracle_lib, matcher_geometry):
    orc = oracle_lib
    for name in hi.CASE_NAMES:
        mu_range = hi.seed_set(name)["mu_range"]
        ov_r, ov_c, gv_r, gv_c = views(orc, gpu_ctx, name, mu_range)
        for sphere, vog in SEED_OPTION_SETS:
            ro = oracle_once(("seeds", name, sphere, vog), lambda: run_seeds(
                orc.update_seeds_batch, orc.make_feature_batch, ov_r, ov_c, name, sphere, vog))
            rg = run_seeds(gpu_ctx.update_seeds_batch, fe.make_feature_batch, gv_r, gv_c, name, sphere, vog)
            for k, (o, g) in enumerate(zip(ro, rg)):
                tag = (name, sphere, vog, k)
                assert o[0] == g[0], tag
                assert np.array_equal(o[3], g[3]), (tag, np.nonzero(o[3] != g[3])[0][:10])
                assert np.array_equal(o[4], g[4]), (tag, np.nonzero(o[4] != g[4])[0][:10], o[4][o[4] != g[4]][:10], g[4][o[4] != g[4]][:10])
                assert np.array_equal(o[6], g[6]), tag
                assert np.allclose(g[2], o[2], rtol=1e-9, atol=0, equal_nan=True), (tag, np.nonzero(~np.isclose(g[2], o[2], rtol=1e-9, atol=0, equal_nan=True))[0][:10])
                check_untouched(g)
                check_untouched(o)


def run_direct(match, make_batch, ref_view, cur_view, name, pixelwise):
    ds = hi.direct_set(name)
    fb, _keep = make_batch(ds["ref_frame_idx"], ds["px"], ds["f"], ds["grad"], ds["level"], ds["type"])
    return match(capi.default_matcher_options(), [ref_view], cur_view, fb, ds["true_depth"], ds["px_init"],
                 landmark_xyz=ds["landmark_xyz"] if pixelwise else None)


def test_match_direct_both_warps(gpu_ctx, oracle_lib, matcher_geometry):
    orc = oracle_lib
    for name in hi.CASE_NAMES:
        ov_r, ov_c, gv_r, gv_c = views(orc, gpu_ctx, name, 0.0)
        for pixelwise in (False, True):
            oo = oracle_once(("direct", name, pixelwise), lambda: run_direct(
                orc.match_direct_batch, orc.make_feature_batch, ov_r, ov_c, name, pixelwise))
            og = run_direct(gpu_ctx.match_direct_batch, fe.make_feature_batch, gv_r, gv_c, name, pixelwise)
            tag = (name, pixelwise)
            bad = np.nonzero(oo["result"] != og["result"])[0]
            assert bad.size == 0, (tag, bad[:10], oo["result"][bad][:10], og["result"][bad][:10])
            assert np.array_equal(oo["search_level"], og["search_level"]), tag
            ok = np.repeat(oo["result"] == capi.MATCH_SUCCESS, 2)
            d = np.abs(oo["px_cur"] - og["px_cur"])
            assert not ok.any() or d[ok].max() <= 1e-4, (tag, d[ok].max(), np.nonzero(ok & (d > 1e-4))[0][:10] // 2)
            # a match that failed leaves the start value where it was, on both sides
            px_init = hi.direct_set(name)["px_init"]
            assert same_bits(og["px_cur"][~ok], px_init[~ok]) and same_bits(oo["px_cur"][~ok], px_init[~ok]), tag


def run_epipolar(match, make_batch, ref_view, cur_view, name):
    ss = hi.stereo_set(name)
    mopt = capi.default_matcher_options(max_epi_search_steps=500, subpix_refinement=1, scan_on_unit_sphere=1)
    fb, _keep = make_batch(ss["ref_frame_idx"], ss["px"], ss["f"], ss["grad"], ss["level"], ss["type"])
    return match(mopt, [ref_view], cur_view, fb, d_inv_common=ss["d_inv"], T_cur_ref=[ss["T_f1f0"]])


def test_stereo_seam_epipolar_match(gpu_ctx, oracle_lib, matcher_geometry):
    orc = oracle_lib
    for name in hi.CASE_NAMES:
        ov_r, ov_c, gv_r, gv_c = views(orc, gpu_ctx, name, 0.0)
        oo = oracle_once(("stereo", name), lambda: run_epipolar(orc.epipolar_match_batch, orc.make_feature_batch, ov_r, ov_c, name))
        og = run_epipolar(gpu_ctx.epipolar_match_batch, fe.make_feature_batch, gv_r, gv_c, name)
        bad = np.nonzero(oo["result"] != og["result"])[0]
        assert bad.size == 0, (name, bad[:10], oo["result"][bad][:10], og["result"][bad][:10])
        assert np.array_equal(oo["search_level"], og["search_level"]), name
        ok = oo["result"] == capi.MATCH_SUCCESS
        assert np.allclose(og["depth"][ok], oo["depth"][ok], rtol=1e-9, atol=0), name
        if ok.any():
            assert np.abs(oo["px_cur"] - og["px_cur"])[np.repeat(ok, 2)].max() <= 1e-4, name
            assert np.abs(oo["f_cur"] - og["f_cur"])[np.repeat(ok, 3)].max() < 1e-6, name
        assert np.allclose(oo["A"], og["A"], rtol=1e-12, atol=1e-14), name


def across_geometries(gpu_ctx, run):
    """run(name, ref view, cur view) -> list of (label, array): the same bit for bit in the four matcher geometries"""
    out = {}
    for geo, val in GEOMETRIES.items():
        with knob(gpu_ctx, "SVOH_MATCHER_G8", val):
            res = []
            for name in hi.CASE_NAMES:
                fr, fc = frames(gpu_ctx, name)
                p = hi.pair(name)
                mu_range = hi.seed_set(name)["mu_range"]
                res += [((name,) + label, a) for label, a in run(name, fe.make_frame_view(fr, p.cam, p.T_ref_f_w, mu_range, 1),
                                                                 fe.make_frame_view(fc, p.cam, p.T_cur_f_w, 0.0, 2))]
            out[geo] = res
    first = out["eight_lanes_per_unit"]
    for geo, res in out.items():
        assert len(res) == len(first)
        for (la, a), (lb, b) in zip(first, res):
            assert la == lb
            assert same_bits(a, b), (geo, la, int(np.sum(~((a == b) | ((a != a) & (b != b))))))


def test_seed_update_geometries_bit_identical(gpu_ctx):
    def run(name, gv_r, gv_c):
        return [(("seeds", sphere, vog, rnd, k), np.asarray(a)) for sphere, vog in SEED_OPTION_SETS
                for rnd, r in enumerate(run_seeds(gpu_ctx.update_seeds_batch, fe.make_feature_batch, gv_r, gv_c, name, sphere, vog))
                for k, a in enumerate(r)]
    across_geometries(gpu_ctx, run)


def test_direct_and_epipolar_geometries_bit_identical(gpu_ctx):
    """every output array: result codes, pixels, bearing vectors, search levels, h_inv, warp matrices, depths"""
    def run(name, gv_r, gv_c):
        res = []
        for pixelwise in (False, True):
            d = run_direct(gpu_ctx.match_direct_batch, fe.make_feature_batch, gv_r, gv_c, name, pixelwise)
            res += [(("direct", pixelwise, k), d[k]) for k in sorted(d)]
        e = run_epipolar(gpu_ctx.epipolar_match_batch, fe.make_feature_batch, gv_r, gv_c, name)
        return res + [(("epipolar", k), e[k]) for k in sorted(e)]
    across_geometries(gpu_ctx, run)


# ---------------------------------------------------------------------------------------------------------------------
# sparse image alignment on hard edges, clipped plateaus and noise: the Tukey weights and the MAD scale meet real outliers
# ---------------------------------------------------------------------------------------------------------------------
ALIGN_OPTION_SETS = (dict(), dict(robustification=1), dict(estimate_illumination_gain=1, estimate_illumination_offset=1))


@pytest.mark.parametrize("patch_size", [4, 8])
def test_sparse_align_on_hard_content(gpu_ctx, oracle_lib, patch_size):
    from test_sparse_align_gpu import check_evaluate, check_run
    for name in hi.ALIGN_FAMILIES:
        p = hi.pair(name)
        fr, fc = frames(gpu_ctx, name)
        sc = hi.align_scene(name, patch_size)
        opb = oracle_lib.problem_from_scenes([(sc, p.ref, p.cur)])
        gpb, _keep = fe.make_align_problems([[(sc, fr, fc)]])
        for kw in ALIGN_OPTION_SETS:
            opt = capi.default_align_options(max_level=3, min_level=1, patch_size=patch_size, **kw)
            check_evaluate(gpu_ctx, oracle_lib, opt, opb, gpb, hi.ALIGN_LEVELS)
            rg, ro = check_run(gpu_ctx, oracle_lib, opt, opb, gpb)
            assert all(rg.n_meas[level] == hi.N_ALIGN * patch_size * patch_size for level in hi.ALIGN_LEVELS)
