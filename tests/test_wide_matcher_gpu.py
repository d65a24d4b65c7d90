"""The blocking matcher entries on EQUIDISTANT and ATAN cameras, on the GPU, against the NumPy reading given a CamWide (the
C oracle has no wide camera): svoh_update_seeds_batch (update_seeds_wide_kernel, eight lanes per unit),
svoh_match_direct_batch / _pixelwise (match_direct_wide_kernel, one lane per unit) and svoh_epipolar_match_batch
(epipolar_match_wide_kernel, one wave per unit).  Cases and references: tests/wide_matcher.py.

Bars.  Integer outputs (result codes, success flags, types, search levels, the success count) exact: tests/
test_wide_matcher_cpu.py shows that they do not move when the camera maths move by 8 ulp.  Seed state 1e-8 relative, 1e-5
with the illumination gain estimated (the bars of tests/test_np_second_opinion_cpu.py for this reading against a C
implementation, which explains the ill-conditioned 4x4 system; two orders above the measured 8-ulp sensitivity).  Direct
matcher: the bars of test_match_direct_oracle_vs_numpy_second_opinion.  Seam depth and pixel 1e-8 relative (doubles computed
from a float32 sub-pixel position).  Each round of the seed update starts from the reference's previous state and types, so
a round compares one step on identical inputs."""
import ctypes as C
import os

import numpy as np
import pytest
import torch  # noqa: F401  -- before the first svoh call of the process (see tests/test_wide_geometry_gpu.py)

from svo_pro_universal_amd import _capi as capi, frontend as fe

import np_restatement_direct as nd
import wide_matcher as wm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def frames(gpu_ctx):
    """(name, seam) -> (reference frame handle, current frame handle), built once."""
    made = {}

    def get(name, seam=False):
        if (name, seam) not in made:
            _, ref, cur, _, _ = wm.pair(name, seam)
            made[(name, seam)] = (gpu_ctx.build_pyramid(ref[0], 5), gpu_ctx.build_pyramid(cur[0], 5))
        return made[(name, seam)]
    yield get
    for fr, fc in made.values():
        gpu_ctx.release_frame(fr); gpu_ctx.release_frame(fc)


@pytest.fixture
def matcher_g8(gpu_ctx):
    """Set SVOH_MATCHER_G8 for a call; the conftest's fixture re-reads the knobs after the test."""
    old = os.environ.get("SVOH_MATCHER_G8")

    def use(v):
        if v is None:
            os.environ.pop("SVOH_MATCHER_G8", None)
        else:
            os.environ["SVOH_MATCHER_G8"] = v
        gpu_ctx.reload_knobs()
    yield use
    use(old)


def views(frames, name, mu_range, seam=False, ids=(1, 2)):
    sc, _, _, cam_r, cam_c = wm.pair(name, seam)
    fr, fc = frames(name, seam)
    return (fe.make_frame_view(fr, cam_r, sc.T_ref_f_w, mu_range, ids[0]), fe.make_frame_view(fc, cam_c, sc.T_cur_f_w_gt, 0.0, ids[1]))


def batch(sd, types, sel=slice(None)):
    k = np.arange(sd["level"].size)[sel]
    fb, keep = fe.make_feature_batch(sd["ref_frame_idx"][k], sd["px"].reshape(-1, 2)[k].ravel(), sd["f"].reshape(-1, 3)[k].ravel(),
                                     sd["grad"].reshape(-1, 2)[k].ravel(), sd["level"][k], np.asarray(types)[k])
    fb.keep = keep          # the batch holds addresses: its arrays live as long as it does
    return fb, keep


def rel_err(a, b):
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-300)


# ---- 1. seed update ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("option_set", [0, 1, 2])
@pytest.mark.parametrize("sphere", [0, 1])
@pytest.mark.parametrize("kind", wm.CAMERAS)
def test_seed_update_parity(gpu_ctx, frames, kind, sphere, option_set):
    sd = wm.seed_set(kind)
    mopt, dopt = wm.seed_options(kind, sphere, option_set)
    rv, cv = views(frames, kind, sd["mu_range"])
    tol = 1e-5 if mopt.affine_est_gain else 1e-8
    state, types = sd["state"], sd["type"]
    for g in wm.seeds_reference(kind, sphere, option_set):
        fb, keep = batch(sd, types)
        ns, st, succ, mr = gpu_ctx.update_seeds_batch(mopt, dopt, [rv], cv, fb, state)
        rel = rel_err(st, g["state"])
        print("%s sphere %d set %d: %d succeed, largest relative state difference %.2e" % (kind, sphere, option_set, ns, rel.max()))
        assert np.array_equal(mr, g["match_result"]), np.nonzero(mr != g["match_result"])[0][:10]
        assert np.array_equal(succ, g["success"]) and np.array_equal(keep["type"], g["type"])
        assert ns == int(g["success"].sum())
        assert rel.max() <= tol, (rel.max(), np.unravel_index(rel.argmax(), (wm.N_UNITS, 4)))
        state, types = g["state"], g["type"]
    # the depths are the scene's: no worse than the reading's own median error on these inputs, plus a tenth of it
    got = dict(state=st, success=succ)
    assert wm.median_depth_error(kind, got) <= 1.1 * wm.median_depth_error(kind, g)


# ---- 2. direct matcher, both warps ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("pixelwise", [False, True])
@pytest.mark.parametrize("kind", wm.CAMERAS)
def test_direct_matcher_parity(gpu_ctx, frames, kind, pixelwise):
    sd, di = wm.seed_set(kind), wm.direct_inputs(kind)
    rv, cv = views(frames, kind, sd["mu_range"])
    for gain in (0, 1):
        g = wm.direct_reference(kind, pixelwise, gain)
        fb, keep = batch(sd, di["type"])
        o = gpu_ctx.match_direct_batch(capi.default_matcher_options(affine_est_gain=gain), [rv], cv, fb, sd["true_depth"], di["px_init"],
                                       landmark_xyz=di["landmark_xyz"] if pixelwise else None)
        assert np.array_equal(o["result"], g["result"]), np.nonzero(o["result"] != g["result"])[0][:10]
        assert np.array_equal(o["search_level"], g["search_level"])
        ran, ok = g["result"] != nd.FAIL_VISIBILITY, g["result"] == nd.SUCCESS
        assert ok.sum() > wm.N_UNITS // 2
        assert np.abs(o["px_cur"] - g["px_cur"]).max() <= 1e-4
        assert np.allclose(o["A"][np.repeat(ran, 4)], g["A"][np.repeat(ran, 4)], rtol=1e-11, atol=1e-13)
        assert np.abs(o["f_cur"] - g["f_cur"])[np.repeat(ok, 3)].max() < 1e-6
        edge_ok = ok & (di["type"] == capi.FT_EDGELET)
        assert np.allclose(o["h_inv"][edge_ok], g["h_inv"][edge_ok], rtol=1e-5)


# ---- 3. stereo seam ------------------------------------------------------------------------------------------------------
def run_seam(ctx, frames, name, per_feature, sel=slice(None)):
    si = wm.seam_inputs(name)
    rv, cv = views(frames, name, 0.0, seam=True)
    fb, keep = batch(si["sd"], si["type"], sel)
    if per_feature:
        return ctx.epipolar_match_batch(wm.seam_options(), [rv], cv, fb, d_inv=si["d_inv"].reshape(-1, 3)[sel].ravel(), T_cur_ref=[si["T_f1f0"]])
    return ctx.epipolar_match_batch(wm.seam_options(), [rv], cv, fb, d_inv_common=list(si["d_inv_common"]), T_cur_ref=[si["T_f1f0"]])


def check_seam(o, g):
    assert np.array_equal(o["result"], g["result"]), np.nonzero(o["result"] != g["result"])[0][:10]
    ok = g["result"] == nd.SUCCESS
    assert ok.sum() > wm.N_SEAM // 2
    assert np.allclose(o["depth"][ok], g["depth"][ok], rtol=1e-8, atol=0)
    assert np.allclose(o["px_cur"].reshape(-1, 2)[ok], g["px_cur"][ok], rtol=1e-8, atol=0)


@pytest.mark.parametrize("per_feature", [False, True])
@pytest.mark.parametrize("kind", wm.CAMERAS)
def test_stereo_seam_parity(gpu_ctx, frames, kind, per_feature):
    o = run_seam(gpu_ctx, frames, kind, per_feature)
    check_seam(o, wm.seam_reference(kind, per_feature))
    # the triangulated depth is the scene's: no worse than the reading's own median error, plus a tenth of it
    g, true_depth = wm.seam_reference(kind, per_feature), wm.seam_inputs(kind)["sd"]["true_depth"]
    ok = g["result"] == nd.SUCCESS
    err = [float(np.median(np.abs(d[ok] - true_depth[ok]) / true_depth[ok])) for d in (o["depth"], g["depth"])]
    assert err[0] <= 1.1 * err[1]


# ---- 4. a radtan view beside an equidistant one --------------------------------------------------------------------------
def test_mixed_launch_against_the_reading(gpu_ctx, frames):
    sd, di = wm.seed_set("mixed"), wm.direct_inputs("mixed")
    rv, cv = views(frames, "mixed", sd["mu_range"])
    mopt, dopt = wm.seed_options("mixed", 0, 0)
    g = wm.seeds_reference("mixed")[0]
    fb, keep = batch(sd, sd["type"])
    ns, st, succ, mr = gpu_ctx.update_seeds_batch(mopt, dopt, [rv], cv, fb, sd["state"])
    assert np.array_equal(mr, g["match_result"]) and np.array_equal(succ, g["success"]) and np.array_equal(keep["type"], g["type"])
    assert ns == int(g["success"].sum()) > wm.N_UNITS // 2 and rel_err(st, g["state"]).max() <= 1e-8
    g = wm.direct_reference("mixed")
    fb, keep = batch(sd, di["type"])
    o = gpu_ctx.match_direct_batch(capi.default_matcher_options(), [rv], cv, fb, sd["true_depth"], di["px_init"])
    assert np.array_equal(o["result"], g["result"]) and np.array_equal(o["search_level"], g["search_level"])
    assert (g["result"] == nd.SUCCESS).sum() > wm.N_UNITS // 2 and np.abs(o["px_cur"] - g["px_cur"]).max() <= 1e-4
    check_seam(run_seam(gpu_ctx, frames, "mixed", False), wm.seam_reference("mixed"))


def two_pair_views(frames, names, mu_range, seam=False):
    """Reference views, then current views, of two pairs in one launch: unit i of pair k carries ref / cur index k."""
    v = [views(frames, n, mu_range, seam, ids=(1 + 2 * k, 2 + 2 * k)) for k, n in enumerate(names)]
    return [a for a, _ in v], [b for _, b in v]


def direct_two_current(ctx, mopt, rvs, cvs, fb, depth, px_init):
    """svoh_match_direct_batch with a list of current views (fe.Context.match_direct_batch passes one)."""
    n = fb.n
    depth = np.ascontiguousarray(depth, np.float64)
    out = dict(px_cur=np.ascontiguousarray(px_init, np.float64).copy(), result=np.zeros(n, np.int32), f_cur=np.zeros(3 * n),
               search_level=np.zeros(n, np.int32), h_inv=np.zeros(n), A=np.zeros(4 * n))
    ctx._check(ctx.lib.svoh_match_direct_batch(ctx.h, C.byref(mopt), len(rvs), (capi.svoh_frame_view * len(rvs))(*rvs),
                                               (capi.svoh_frame_view * len(cvs))(*cvs), C.byref(fb), depth.ctypes.data,
                                               out["px_cur"].ctypes.data, out["result"].ctypes.data, out["f_cur"].ctypes.data,
                                               out["search_level"].ctypes.data, out["h_inv"].ctypes.data, out["A"].ctypes.data))
    return out


def doubled(fb, keep, n):
    """fb's units twice, the second copy on reference / current frame 1."""
    arrs = {k: np.concatenate([a, a]) for k, a in keep.items()}
    arrs["ref_frame_idx"][n:] = 1
    fb2, keep2 = fe.make_feature_batch(arrs["ref_frame_idx"], arrs["px"], arrs["f"], arrs["grad"], arrs["level"], arrs["type"])
    keep2["cur_frame_idx"] = np.ascontiguousarray(arrs["ref_frame_idx"], np.int32)
    fb2.cur_frame_idx, fb2.n_cur_frames = keep2["cur_frame_idx"].ctypes.data, 2
    return fb2, keep2


def test_radtan_units_through_the_twins_keep_their_bits(gpu_ctx, frames, matcher_g8):
    """The same radtan pair once alone (the narrow kernels, SVOH_MATCHER_G8 set to the twin's geometry) and once beside an
    equidistant pair in one launch (the twins): CamModelWide runs the narrow functions for RADTAN, so integers are equal
    and doubles array_equal.  The narrow kernels themselves are the code they were (tests/
    test_kernel_resources_matcher_wide_cpu.py and the disassembly), so these are the bits from before the twins."""
    sd, di = wm.seed_set("radtan"), wm.direct_inputs("radtan")
    n = wm.N_UNITS
    rv, cv = views(frames, "radtan", sd["mu_range"])
    rvs, cvs = two_pair_views(frames, ("radtan", "equidistant"), sd["mu_range"])
    mopt, dopt = wm.seed_options("radtan", 0, 0)
    # seed update: eight lanes per unit
    matcher_g8("1")
    fb, keep = batch(sd, sd["type"])
    alone = gpu_ctx.update_seeds_batch(mopt, dopt, [rv], cv, fb, sd["state"])
    matcher_g8(None)
    fb2, keep2 = doubled(*batch(sd, sd["type"]), n)
    both = gpu_ctx.update_seeds_batch(mopt, dopt, rvs, cvs, fb2, np.concatenate([sd["state"], sd["state"]]))
    assert alone[0] > n // 2 and np.array_equal(alone[1], both[1][:4 * n])
    assert np.array_equal(alone[2], both[2][:n]) and np.array_equal(alone[3], both[3][:n]) and np.array_equal(keep["type"], keep2["type"][:n])
    assert not np.array_equal(both[1][:4 * n], both[1][4 * n:])          # the other half did run another camera
    # direct matcher: one lane per unit
    matcher_g8("0")
    fb, keep = batch(sd, di["type"])
    alone = gpu_ctx.match_direct_batch(capi.default_matcher_options(), [rv], cv, fb, sd["true_depth"], di["px_init"])
    matcher_g8(None)
    fb2, keep2 = doubled(*batch(sd, di["type"]), n)
    both = direct_two_current(gpu_ctx, capi.default_matcher_options(), rvs, cvs, fb2, np.tile(sd["true_depth"], 2), np.tile(di["px_init"], 2))
    for k, a in alone.items():
        w = a.size // n
        assert np.array_equal(a, both[k][:w * n]), k
    # stereo seam: one wave per unit
    si = wm.seam_inputs("radtan")
    matcher_g8("3")
    alone = run_seam(gpu_ctx, frames, "radtan", False)
    matcher_g8(None)
    rvs, cvs = two_pair_views(frames, ("radtan", "equidistant"), 0.0, seam=True)
    fb2, keep2 = doubled(*batch(si["sd"], si["type"]), wm.N_SEAM)
    both = gpu_ctx.epipolar_match_batch(wm.seam_options(), rvs, cvs, fb2, d_inv_common=list(si["d_inv_common"]),
                                        T_cur_ref=[si["T_f1f0"]] * 4)
    for k, a in alone.items():
        w = a.size // wm.N_SEAM
        assert np.array_equal(a, both[k][:w * wm.N_SEAM]), k


# ---- 5. batch properties -------------------------------------------------------------------------------------------------
def test_empty_batch_and_a_batch_of_one(gpu_ctx, frames):
    kind = "equidistant"
    sd, di = wm.seed_set(kind), wm.direct_inputs(kind)
    rv, cv = views(frames, kind, sd["mu_range"])
    mopt, dopt = wm.seed_options(kind, 0, 0)
    none = slice(0, 0)
    ns, st, succ, mr = gpu_ctx.update_seeds_batch(mopt, dopt, [rv], cv, batch(sd, sd["type"], none)[0], np.zeros(0))
    assert ns == 0 and st.size == 0 and succ.size == 0 and mr.size == 0
    o = gpu_ctx.match_direct_batch(mopt, [rv], cv, batch(sd, di["type"], none)[0], np.zeros(0), np.zeros(0))
    assert all(a.size == 0 for a in o.values())
    assert all(a.size == 0 for a in run_seam(gpu_ctx, frames, kind, False, none).values())
    # one unit alone = its row in the whole batch, bit for bit
    fb, keep = batch(sd, sd["type"])
    whole = gpu_ctx.update_seeds_batch(mopt, dopt, [rv], cv, fb, sd["state"])
    i = int(np.nonzero(whole[2])[0][3])                       # a seed that is updated
    one = slice(i, i + 1)
    fb1, keep1 = batch(sd, sd["type"], one)
    ns, st, succ, mr = gpu_ctx.update_seeds_batch(mopt, dopt, [rv], cv, fb1, sd["state"][4 * i:4 * i + 4])
    assert ns == 1 and np.array_equal(st, whole[1][4 * i:4 * i + 4]) and mr[0] == whole[3][i] and keep1["type"][0] == keep["type"][i]
    whole = gpu_ctx.match_direct_batch(mopt, [rv], cv, batch(sd, di["type"])[0], sd["true_depth"], di["px_init"])
    i = int(np.nonzero(whole["result"] == 0)[0][3])
    o = gpu_ctx.match_direct_batch(mopt, [rv], cv, batch(sd, di["type"], slice(i, i + 1))[0], sd["true_depth"][i:i + 1], di["px_init"][2 * i:2 * i + 2])
    for k, a in o.items():
        assert np.array_equal(a, whole[k][a.size * i:a.size * (i + 1)]), k
    whole = run_seam(gpu_ctx, frames, kind, True)
    i = int(np.nonzero(whole["result"] == 0)[0][3])
    o = run_seam(gpu_ctx, frames, kind, True, slice(i, i + 1))
    for k, a in o.items():
        assert np.array_equal(a, whole[k][a.size * i:a.size * (i + 1)]), k


def test_two_reference_frames_with_different_wide_cameras(gpu_ctx, frames):
    """An equidistant pair and an ATAN pair in one launch = the two single-pair launches, bit for bit."""
    names = ("equidistant", "atan")
    sds = [wm.seed_set(k) for k in names]
    n = wm.N_UNITS
    mu = sds[0]["mu_range"]                                   # one value for both reference views, in all three launches
    mopt, dopt = wm.seed_options("equidistant", 0, 0)
    singles = []
    for k, sd in zip(names, sds):
        rv, cv = views(frames, k, mu)
        singles.append(gpu_ctx.update_seeds_batch(mopt, dopt, [rv], cv, batch(sd, sd["type"])[0], sd["state"]))
    rvs, cvs = two_pair_views(frames, names, mu)
    cat = {k: np.concatenate([sd[k] for sd in sds]) for k in ("px", "f", "grad", "level", "type", "state")}
    idx = np.repeat(np.arange(2, dtype=np.int32), n)
    fb, keep = fe.make_feature_batch(idx, cat["px"], cat["f"], cat["grad"], cat["level"], cat["type"])
    fb.cur_frame_idx, fb.n_cur_frames = keep["ref_frame_idx"].ctypes.data, 2
    ns, st, succ, mr = gpu_ctx.update_seeds_batch(mopt, dopt, rvs, cvs, fb, cat["state"])
    assert ns == singles[0][0] + singles[1][0]
    for k in range(2):
        assert np.array_equal(st[4 * n * k:4 * n * (k + 1)], singles[k][1])
        assert np.array_equal(succ[n * k:n * (k + 1)], singles[k][2]) and np.array_equal(mr[n * k:n * (k + 1)], singles[k][3])


# ---- 6. what stays closed ------------------------------------------------------------------------------------------------
def narrow_still_works(ctx, frames):
    sd = wm.seed_set("radtan")
    rv, cv = views(frames, "radtan", sd["mu_range"])
    mopt, dopt = wm.seed_options("radtan", 0, 0)
    ns, st, succ, mr = ctx.update_seeds_batch(mopt, dopt, [rv], cv, batch(sd, sd["type"])[0], sd["state"])
    assert ns > wm.N_UNITS // 2


def raw_seed_call(ctx, entry, rv, cv, fb, mopt, dopt, extra=()):
    n = fb.n
    st = np.full(4 * n, 7.0)
    succ, mr, ns = np.full(n, 9, np.uint8), np.full(n, -77, np.int32), C.c_int32(-5)
    rc = entry(ctx.h, C.byref(mopt), C.byref(dopt), 1, C.byref(rv), C.byref(cv), C.byref(fb), st.ctypes.data, succ.ctypes.data,
               mr.ctypes.data, C.byref(ns), *extra)
    untouched = (st == 7.0).all() and (succ == 9).all() and (mr == -77).all()
    return rc, untouched


@pytest.mark.parametrize("kind", wm.CAMERAS)
def test_ex_entry_and_deferred_section_keep_refusing(gpu_ctx, frames, kind):
    lib = gpu_ctx.lib
    sd = wm.seed_set(kind)
    rv, cv = views(frames, kind, sd["mu_range"])
    mopt, dopt = wm.seed_options(kind, 0, 0)
    fb, keep = batch(sd, sd["type"])
    n = fb.n
    px_cur = np.full(2 * n, 3.0)
    outs = capi.svoh_seed_match_outputs()
    outs.px_cur = px_cur.ctypes.data
    rc, untouched = raw_seed_call(gpu_ctx, lib.svoh_update_seeds_batch_ex, rv, cv, fb, mopt, dopt, (C.byref(outs),))
    assert rc == capi.SVOH_ERR_UNSUPPORTED and untouched and (px_cur == 3.0).all() and np.array_equal(keep["type"], sd["type"])
    narrow_still_works(gpu_ctx, frames)
    assert lib.svoh_matcher_begin_deferred(gpu_ctx.h) == 0
    try:
        rc, untouched = raw_seed_call(gpu_ctx, lib.svoh_update_seeds_batch, rv, cv, fb, mopt, dopt)
        assert rc == capi.SVOH_ERR_UNSUPPORTED and untouched
        di = wm.direct_inputs(kind)
        fbd, keepd = batch(sd, di["type"])
        px, res = di["px_init"].copy(), np.full(n, -77, np.int32)
        depth = np.ascontiguousarray(sd["true_depth"])
        rc = lib.svoh_match_direct_batch(gpu_ctx.h, C.byref(mopt), 1, C.byref(rv), C.byref(cv), C.byref(fbd), depth.ctypes.data,
                                         px.ctypes.data, res.ctypes.data, None, None, None, None)
        assert rc == capi.SVOH_ERR_UNSUPPORTED and (res == -77).all() and np.array_equal(px, di["px_init"])
    finally:
        assert lib.svoh_matcher_collect(gpu_ctx.h) == 0
    narrow_still_works(gpu_ctx, frames)


# ---- 7. hostile views ----------------------------------------------------------------------------------------------------
def test_wide_view_of_another_size_and_bad_atan_parameters_are_refused(gpu_ctx, frames):
    from svo_pro_universal_amd import synth
    sd = wm.seed_set("equidistant")
    rv, cv = views(frames, "equidistant", sd["mu_range"])
    mopt, dopt = wm.seed_options("equidistant", 0, 0)
    fb, keep = batch(sd, sd["type"])
    c = wm.camera("equidistant")
    small = synth.Camera(c.width - 8, c.height, c.fx, c.fy, c.cx, c.cy, dist=c.dist, model="equidistant")
    bad = fe.make_frame_view(frames("equidistant")[1], small, wm.pair("equidistant")[0].T_cur_f_w_gt, 0.0, 2)
    rc, untouched = raw_seed_call(gpu_ctx, gpu_ctx.lib.svoh_update_seeds_batch, rv, bad, fb, mopt, dopt)
    assert rc == capi.SVOH_ERR_INVALID_ARGUMENT and untouched
    # ATAN: s zero or not finite, in each of the three entries, before anything is staged
    a = wm.camera("atan")
    sda, dia, sia = wm.seed_set("atan"), wm.direct_inputs("atan"), wm.seam_inputs("atan")
    rva, cva = views(frames, "atan", sda["mu_range"])
    for s in (0.0, float("nan"), float("inf")):
        cam = synth.Camera(a.width, a.height, a.fx, a.fy, a.cx, a.cy, dist=[s], model="atan")
        bad = fe.make_frame_view(frames("atan")[1], cam, wm.pair("atan")[0].T_cur_f_w_gt, 0.0, 2)
        rc, untouched = raw_seed_call(gpu_ctx, gpu_ctx.lib.svoh_update_seeds_batch, rva, bad, batch(sda, sda["type"])[0], mopt, dopt)
        assert rc == capi.SVOH_ERR_INVALID_ARGUMENT and untouched
        for pixelwise in (False, True):
            with pytest.raises(fe.SvohError) as e:
                gpu_ctx.match_direct_batch(mopt, [rva], bad, batch(sda, dia["type"])[0], sda["true_depth"], dia["px_init"],
                                           landmark_xyz=dia["landmark_xyz"] if pixelwise else None)
            assert e.value.code == capi.SVOH_ERR_INVALID_ARGUMENT
        with pytest.raises(fe.SvohError) as e:
            gpu_ctx.epipolar_match_batch(wm.seam_options(), [rva], bad, batch(sia["sd"], sia["type"])[0], d_inv_common=list(sia["d_inv_common"]))
        assert e.value.code == capi.SVOH_ERR_INVALID_ARGUMENT
    narrow_still_works(gpu_ctx, frames)
