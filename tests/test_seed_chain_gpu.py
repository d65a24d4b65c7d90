"""svoh_update_seeds_chain on the GPU: a new keyframe's seeds against a list of frames in ONE launch, state and type
carried on the device (FrameHandlerMono::processFrame with update_seeds_with_old_keyframes, frame_handler_mono.cpp:218-225).

Bars: the chain call against one svoh_update_seeds_batch call per list position -- the same kernel arithmetic, so raw
bytes (NaNs included); against the CPU oracle -- discrete outputs exact, state rtol 1e-9 (libm vs the device's libm:
the bar test_update_seeds_parity holds over three fed-back rounds).  Every test runs in the three geometries the chain
kernel is built in."""
import ctypes as C
import os

import numpy as np
import pytest

from svo_pro_universal_amd import _capi as capi, frontend as fe

import seed_chain as scn

pytestmark = pytest.mark.gpu

OPTION_SETS = {
    "defaults": (dict(), dict(check_visibility=1, check_convergence=0)),
    "gain_plane_gaussian": (dict(affine_est_gain=1, scan_on_unit_sphere=0), dict(use_vogiatzis_update=0)),
}


@pytest.fixture(params=["eight_lanes_per_unit", "one_lane_per_unit", "one_wave_per_unit"], autouse=True)
def matcher_geometry(request, gpu_ctx):
    old = os.environ.get("SVOH_MATCHER_G8")
    os.environ["SVOH_MATCHER_G8"] = {"eight_lanes_per_unit": "1", "one_lane_per_unit": "0", "one_wave_per_unit": "3"}[request.param]
    gpu_ctx.reload_knobs()
    yield request.param
    if old is None:
        os.environ.pop("SVOH_MATCHER_G8", None)
    else:
        os.environ["SVOH_MATCHER_G8"] = old
    gpu_ctx.reload_knobs()


_packs = {}


def pack(gpu_ctx, cam_kind):
    """Data, frames and views of one camera kind: made once, never changed."""
    if cam_kind not in _packs:
        d = scn.make_data(cam_kind)
        fr = gpu_ctx.build_pyramid(d.sc.img_ref, 5)
        frames = [gpu_ctx.build_pyramid(im, 5) for im in d.imgs[:5]]
        refs, lst = scn.make_views(d, fe.make_frame_view, fr, frames)
        _packs[cam_kind] = (d, refs, lst)
    return _packs[cam_kind]


def options(d, name):
    mkw, dkw = OPTION_SETS[name]
    return capi.default_matcher_options(**mkw), capi.default_depth_filter_options(d.cam, **dkw)


def feature_batch(sd):
    return fe.make_feature_batch(sd["ref_frame_idx"], sd["px"], sd["f"], sd["grad"], sd["level"], sd["type"])


def run_chain(gpu_ctx, d, refs, lst, chains, mopt, dopt, **kw):
    fb, keep = feature_batch(d.sd)
    ns, st, n_ok, res, suc = gpu_ctx.update_seeds_chain(mopt, dopt, refs, fb, d.sd["state"], lst, chains, **kw)
    return ns, st, keep["type"], res, suc, n_ok


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def assert_chain_equals_sequence(got, want):
    ns, st, types, res, suc, n_ok = got
    ns_w, st_w, types_w, res_w, suc_w = want
    assert np.array_equal(res, res_w), np.argwhere(res != res_w)[:10]
    assert np.array_equal(suc, suc_w)
    assert same_bytes(types, types_w)
    assert same_bytes(st, st_w), np.nonzero(st.view(np.uint64) != st_w.view(np.uint64))[0][:10]
    assert ns == ns_w and np.array_equal(n_ok, suc_w.sum(1))


@pytest.mark.parametrize("cam_kind,opts,chains", [
    ("pinhole", "defaults", "CHAINS_4"), ("pinhole", "gain_plane_gaussian", "CHAINS_4"), ("radtan", "defaults", "CHAINS_4"),
    ("pinhole", "defaults", "CHAINS_6"), ("pinhole", "gain_plane_gaussian", "CHAINS_6"),
])
def test_chain_equals_the_sequence_of_single_calls(gpu_ctx, cam_kind, opts, chains):
    d, refs, lst = pack(gpu_ctx, cam_kind)
    chains = getattr(scn, chains)
    mopt, dopt = options(d, opts)
    want = scn.run_sequence(gpu_ctx.update_seeds_batch, fe.make_feature_batch, refs, lst, chains, d.sd, mopt, dopt)
    got = run_chain(gpu_ctx, d, refs, lst, chains, mopt, dopt)
    assert_chain_equals_sequence(got, want)
    ns, st, types, res, suc, n_ok = got
    n0, n1 = scn.N_SEEDS[0], scn.N_SEEDS[0] + scn.N_SEEDS[1]
    # the data does what it was made for: work in the walked chains, nothing beyond them
    assert suc[:n0].sum() > n0 // 2 and suc[n0:n1, 0].sum() > scn.N_SEEDS[1] // 2
    assert np.all(res[n0:n1, 1:] == capi.MATCH_NOT_RUN) and np.all(res[n1:] == capi.MATCH_NOT_RUN) and not suc[n1:].any()
    assert same_bytes(st.reshape(-1, 4)[n1:], d.sd["state"].reshape(-1, 4)[n1:]) and np.array_equal(types[n1:], d.sd["type"][n1:])
    if chains is scn.CHAINS_4:
        # the frame under the reference view's id and the one that looks away: every unit returns before the matcher
        assert np.all(res[:n0, 1] == capi.MATCH_NOT_RUN) and np.all(res[:n0, 2] == capi.MATCH_NOT_RUN)
    # a seed that converged on the way went on as a converged seed
    t0 = d.sd["type"][:n0]
    conv = (t0 < 3) & (types[:n0] >= 3) & (types[:n0] <= 5)
    assert conv.any() and np.all(types[:n0][conv] == t0[conv] + 3)
    # without the step outputs: the same state, types and counts
    fb, keep = feature_batch(d.sd)
    ns2, st2, n_ok2, res2, suc2 = gpu_ctx.update_seeds_chain(mopt, dopt, refs, fb, d.sd["state"], lst, chains, want_steps=False)
    assert res2 is None and suc2 is None and ns2 == ns and same_bytes(st2, st) and same_bytes(keep["type"], types)
    assert np.array_equal(n_ok2, n_ok)


_oracle_run = {}


def test_chain_against_the_oracle(gpu_ctx, oracle_lib):
    orc = oracle_lib
    d, refs, lst = pack(gpu_ctx, "pinhole")
    mopt, dopt = options(d, "defaults")
    if not _oracle_run:   # the reference: computed once, shared by the geometries
        ref = orc.create_img_pyramid(d.sc.img_ref, 5)
        pyr = [orc.create_img_pyramid(im, 5) for im in d.imgs[:5]]
        orefs, olst = scn.make_views(d, orc.make_frame_view, ref, pyr)
        _oracle_run["want"] = scn.run_sequence(orc.update_seeds_batch, orc.make_feature_batch, orefs, olst, scn.CHAINS_3, d.sd, mopt, dopt)
        _oracle_run["after_two"] = scn.run_sequence(orc.update_seeds_batch, orc.make_feature_batch, orefs, olst, ([0, 1], [], []), d.sd, mopt, dopt)[2]
    ns_o, st_o, types_o, res_o, suc_o = _oracle_run["want"]
    n0 = scn.N_SEEDS[0]
    # conditions of the test, on the oracle's run alone
    t0, t2 = d.sd["type"][:n0], _oracle_run["after_two"][:n0]
    assert ((t0 < 3) & (t2 >= 3) & (t2 <= 5)).any(), "no unit converges before its last step"
    ran_and_failed = (res_o[:n0] != capi.MATCH_SUCCESS) & (res_o[:n0] != capi.MATCH_NOT_RUN)
    later_success = np.stack([suc_o[:n0, j + 1:].any(1) for j in range(3)], axis=1)
    assert (ran_and_failed & later_success).any(), "no unit fails a step and succeeds at a later one"
    assert (suc_o[:n0].sum(1) > 0).sum() > n0 // 2
    ns, st, types, res, suc, n_ok = run_chain(gpu_ctx, d, refs, lst, scn.CHAINS_3, mopt, dopt)
    assert np.array_equal(res, res_o), np.argwhere(res != res_o)[:10]
    assert np.array_equal(suc, suc_o) and np.array_equal(types, types_o)
    assert ns == ns_o and np.array_equal(n_ok, suc_o.sum(1))
    assert np.allclose(st, st_o, rtol=1e-9, atol=0)


def raw_chain_call(gpu_ctx, d, refs, lst, begin, idx, max_steps=4, n_chain_frames=None, fb=None, want_steps=True):
    """The C entry with hand-made chain arrays; returns (rc, n_success, state, types, steps_succeeded, step_result, step_success)."""
    if fb is None:
        fb, keep = feature_batch(d.sd)
        n, state = fb.n, d.sd["state"].copy()
    else:
        fb, keep = fb
        n, state = fb.n, np.zeros(4 * fb.n)
    rv = (capi.svoh_frame_view * len(refs))(*refs)
    cv = (capi.svoh_frame_view * max(len(lst), 1))(*lst)
    begin, idx = np.ascontiguousarray(begin, np.int32), np.ascontiguousarray(idx if len(idx) else [0], np.int32)
    n_ok = np.full(max(n, 1), -7, np.int32)
    res = np.full((max(n, 1), max(max_steps, 1)), -7, np.int32)
    suc = np.full((max(n, 1), max(max_steps, 1)), 9, np.uint8)
    ns = C.c_int32(-7)
    mopt, dopt = options(d, "defaults")
    rc = gpu_ctx.lib.svoh_update_seeds_chain(gpu_ctx.h, C.byref(mopt), C.byref(dopt), len(refs), rv, C.byref(fb), state.ctypes.data,
                                             len(lst) if n_chain_frames is None else n_chain_frames, cv, begin.ctypes.data,
                                             idx.ctypes.data, C.byref(ns), n_ok.ctypes.data, res.ctypes.data if want_steps else None,
                                             suc.ctypes.data if want_steps else None, max_steps)
    return rc, ns.value, state, keep["type"], n_ok[:n], res[:n], suc[:n]


def test_refusals_and_empties(gpu_ctx):
    from svo_pro_universal_amd import synth
    d, refs, lst = pack(gpu_ctx, "pinhole")
    mopt, dopt = options(d, "defaults")
    INVALID, BAD_HANDLE, UNSUPPORTED = -1, -4, -5
    begin = [0, 4, 5, 5]
    idx = [k for c in scn.CHAINS_4 for k in c]
    untouched = lambda r: np.array_equal(r[2], d.sd["state"]) and np.array_equal(r[3], d.sd["type"]) and np.all(r[4] == -7)
    for bad_begin in ([1, 4, 5, 5], [0, 4, 3, 5], [0, -1, 5, 5]):
        r = raw_chain_call(gpu_ctx, d, refs, lst, bad_begin, idx)
        assert r[0] == INVALID and untouched(r), bad_begin
    for bad_idx in ([0, 5, 6, 7, 2], [0, 5, -1, 1, 2]):
        r = raw_chain_call(gpu_ctx, d, refs, lst, begin, bad_idx)
        assert r[0] == INVALID and untouched(r), bad_idx
    unknown = list(lst); unknown[3] = fe.make_frame_view(0x7fffffff, d.cam, d.T_f_w[3], 0.0, 13)   # not even in a chain
    r = raw_chain_call(gpu_ctx, d, refs, unknown, begin, idx)
    assert r[0] == BAD_HANDLE and untouched(r)
    small_cam = synth.Camera(width=320, height=240, fx=160.0, fy=160.0, cx=160.0, cy=120.0)
    wrong_size = list(lst); wrong_size[1] = fe.make_frame_view(lst[1].frame, small_cam, d.T_f_w[1], 0.0, 11)
    r = raw_chain_call(gpu_ctx, d, refs, wrong_size, begin, idx)
    assert r[0] == INVALID and untouched(r)
    wide = list(lst); wide[0] = fe.make_frame_view(lst[0].frame, d.cam, d.T_f_w[0], 0.0, 10)
    wide[0].cam.distortion = capi.SVOH_DISTORTION_EQUIDISTANT
    r = raw_chain_call(gpu_ctx, d, refs, wide, begin, idx)
    assert r[0] == UNSUPPORTED and untouched(r)
    wide_ref = list(refs); wide_ref[2] = fe.make_frame_view(refs[2].frame, d.cam, d.sc.T_ref_f_w, d.sd["mu_range"], 3)
    wide_ref[2].cam.distortion = capi.SVOH_DISTORTION_ATAN
    r = raw_chain_call(gpu_ctx, d, wide_ref, lst, begin, idx)
    assert r[0] == UNSUPPORTED and untouched(r)
    r = raw_chain_call(gpu_ctx, d, refs, lst, begin, idx, max_steps=3)                  # the longest chain has four entries
    assert r[0] == INVALID and untouched(r)
    assert raw_chain_call(gpu_ctx, d, refs, lst, begin, idx, max_steps=3, want_steps=False)[0] == 0   # ... which matters only for the step outputs
    with pytest.raises(fe.SvohError):
        gpu_ctx.update_seeds_chain(mopt, dopt, refs, feature_batch(d.sd)[0], d.sd["state"], lst, scn.CHAINS_4, max_steps=2)
    # the context is usable: a correct call gives the bytes of the comparison arm
    want = scn.run_sequence(gpu_ctx.update_seeds_batch, fe.make_feature_batch, refs, lst, scn.CHAINS_4, d.sd, mopt, dopt)
    assert_chain_equals_sequence(run_chain(gpu_ctx, d, refs, lst, scn.CHAINS_4, mopt, dopt), want)
    # a wider table than the longest chain: NOT_RUN / 0 in the columns beyond
    rc, ns, st, types, n_ok, res, suc = raw_chain_call(gpu_ctx, d, refs, lst, begin, idx, max_steps=6)
    assert rc == 0 and np.array_equal(res[:, :4], want[3]) and np.all(res[:, 4:] == capi.MATCH_NOT_RUN) and not suc[:, 4:].any()
    assert same_bytes(st, want[1]) and ns == want[0]
    # all chains empty: success, nothing launched, zeros in the outputs, state and types as they were
    rc, ns, st, types, n_ok, res, suc = raw_chain_call(gpu_ctx, d, refs, lst, [0, 0, 0, 0], [])
    assert rc == 0 and ns == 0 and not n_ok.any() and np.all(res == capi.MATCH_NOT_RUN) and not suc.any()
    assert same_bytes(st, d.sd["state"]) and np.array_equal(types, d.sd["type"])
    # n == 0
    empty = fe.make_feature_batch(np.zeros(0, np.int32), np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0, np.int32), np.zeros(0, np.uint8))
    rc, ns = raw_chain_call(gpu_ctx, d, refs, lst, begin, idx, fb=empty)[:2]
    assert rc == 0 and ns == 0
    ns, st, n_ok, res, suc = gpu_ctx.update_seeds_chain(mopt, dopt, refs, empty[0], np.zeros(0), lst, scn.CHAINS_4)
    assert ns == 0 and st.size == 0 and n_ok.size == 0 and res.shape[0] == 0


def test_chain_inside_a_deferred_section_with_a_flushed_seed_batch(gpu_ctx):
    """The place the host mirror calls it from: a seed batch of OTHER keyframes has been queued and flushed, the section is
    open.  The chain call gives its usual bytes and svoh_matcher_collect the batch's usual results."""
    d, refs, lst = pack(gpu_ctx, "pinhole")
    mopt, dopt = options(d, "defaults")
    lib, h = gpu_ctx.lib, gpu_ctx.h
    sd = d.sd
    fbs, ks = fe.make_feature_batch(np.zeros(len(sd["level"]), np.int32), sd["px"], sd["f"], sd["grad"], sd["level"], sd["type"])
    alone = gpu_ctx.update_seeds_batch(mopt, dopt, [refs[0]], lst[3], fbs, sd["state"])
    alone_types = ks["type"].copy()
    want = run_chain(gpu_ctx, d, refs, lst, scn.CHAINS_4, mopt, dopt)
    fbs, ks = fe.make_feature_batch(np.zeros(len(sd["level"]), np.int32), sd["px"], sd["f"], sd["grad"], sd["level"], sd["type"])
    n = fbs.n
    rva = (capi.svoh_frame_view * 1)(refs[0])
    st = np.ascontiguousarray(sd["state"], np.float64).copy()
    succ, mr, ns = np.zeros(n, np.uint8), np.zeros(n, np.int32), C.c_int32()
    assert lib.svoh_matcher_begin_deferred(h) == 0
    try:
        assert lib.svoh_update_seeds_batch(h, C.byref(mopt), C.byref(dopt), 1, rva, C.byref(lst[3]), C.byref(fbs), st.ctypes.data,
                                           succ.ctypes.data, mr.ctypes.data, C.byref(ns)) == 0
        assert lib.svoh_matcher_flush(h) == 0
        got = run_chain(gpu_ctx, d, refs, lst, scn.CHAINS_4, mopt, dopt)
    finally:
        assert lib.svoh_matcher_collect(h) == 0
    for a, b in zip(got, want):
        assert same_bytes(np.asarray(a), np.asarray(b))
    assert ns.value == alone[0] and same_bytes(st, alone[1]) and np.array_equal(succ, alone[2]) and np.array_equal(mr, alone[3])
    assert np.array_equal(ks["type"], alone_types)
