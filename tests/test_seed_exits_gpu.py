"""Every form of the seed update on the crafted set of tests/seed_exits.py (64 seeds that leave updateSeed through every
exit): svoh_update_seeds_batch_ex in the four geometries, the packed geometry without binning, the whole-sets staged
form, the deferred mixed launch, and svoh_update_seeds_chain with a one-frame list.  Every seed kernel is built from
seed_update_gate / seed_update_apply: state, type, success, result and the
optional outputs are the same bytes in every form; the discrete fields are the oracle's and the state is within the
1e-9 of test_update_seeds_parity."""
import ctypes as C
import os

import numpy as np
import pytest

from svo_pro_universal_amd import _capi as capi, frontend as fe

import seed_exits as sx

pytestmark = pytest.mark.gpu

KNOBS = ("SVOH_MATCHER_G8", "SVOH_SEED_BINNING")
_pack = {}


@pytest.fixture
def knobs(gpu_ctx):
    """set(**values): the matcher's environment knobs for the calls that follow; put back afterwards."""
    old = {k: os.environ.get(k) for k in KNOBS}

    def put(values):
        for k in KNOBS:
            if values.get(k) is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = values[k]
        gpu_ctx.reload_knobs()
    yield lambda **values: put(values)
    put(old)


def pack(gpu_ctx, oracle_lib):
    """Data, frames, views and the oracle's two runs: made once, never changed."""
    if not _pack:
        orc = oracle_lib
        d = sx.make_data()
        refs, cur = sx.make_views(d, fe.make_frame_view, gpu_ctx.build_pyramid(d.sc.img_ref, 5), gpu_ctx.build_pyramid(d.sc.img_cur, 5))
        pyr_ref, pyr_cur = orc.create_img_pyramid(d.sc.img_ref, 5), orc.create_img_pyramid(d.sc.img_cur, 5)
        orefs, ocur = sx.make_views(d, orc.make_frame_view, pyr_ref, pyr_cur)
        want = {}
        for run in sx.RUNS:
            mopt, dopt = sx.options(d, run)
            fb, keep = orc.make_feature_batch(d.sd["ref_frame_idx"], d.sd["px"], d.sd["f"], d.sd["grad"], d.sd["level"], d.sd["type"])
            ns, st, suc, res = orc.update_seeds_batch(mopt, dopt, orefs, ocur, fb, d.sd["state"])
            want[run] = dict(state=st, type=keep["type"], success=suc, result=res)
        _pack.update(d=d, refs=refs, cur=cur, want=want)
    return _pack["d"], _pack["refs"], _pack["cur"], _pack["want"]


def _view(ptr, dtype, count):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), shape=(count,))


def host_call(ctx, d, refs, cur, mopt, dopt, with_direct_batch=False):
    """svoh_update_seeds_batch_ex over host arrays; with_direct_batch: inside a deferred section behind a direct batch of the
    same features, which puts both into one launch where they share a geometry."""
    sd, n = d.sd, sx.N
    fb, keep = fe.make_feature_batch(sd["ref_frame_idx"], sd["px"], sd["f"], sd["grad"], sd["level"], sd["type"])
    rv = (capi.svoh_frame_view * len(refs))(*refs)
    out = dict(state=np.ascontiguousarray(sd["state"], np.float64).copy(), success=np.full(n, 9, np.uint8), result=np.full(n, -7, np.int32),
               px_cur=np.full(2 * n, -7.0), f_cur=np.full(3 * n, -7.0), search_level=np.full(n, -7, np.int32), A=np.full(4 * n, -7.0))
    outs = capi.svoh_seed_match_outputs(out["px_cur"].ctypes.data, out["f_cur"].ctypes.data, out["search_level"].ctypes.data, out["A"].ctypes.data)
    ns = C.c_int32(-7)
    if with_direct_batch:
        fbd, keepd = fe.make_feature_batch(sd["ref_frame_idx"], sd["px"], sd["f"], sd["grad"], sd["level"], sd["type"])
        x, y, _ = sx._project(d, 1.0 / sd["true_depth"])
        dd = dict(depth=np.ascontiguousarray(sd["true_depth"], np.float64), px_cur=np.ascontiguousarray(np.stack([x, y], axis=1).ravel()),
                  result=np.zeros(n, np.int32), f_cur=np.zeros(3 * n), search_level=np.zeros(n, np.int32), h_inv=np.zeros(n), A=np.zeros(4 * n))
        ctx._check(ctx.lib.svoh_matcher_begin_deferred(ctx.h))
        try:
            ctx._check(ctx.lib.svoh_match_direct_batch(ctx.h, C.byref(mopt), len(refs), rv, C.byref(cur), C.byref(fbd), dd["depth"].ctypes.data, dd["px_cur"].ctypes.data,
                                                       dd["result"].ctypes.data, dd["f_cur"].ctypes.data, dd["search_level"].ctypes.data, dd["h_inv"].ctypes.data,
                                                       dd["A"].ctypes.data))
            ctx._check(ctx.lib.svoh_update_seeds_batch_ex(ctx.h, C.byref(mopt), C.byref(dopt), len(refs), rv, C.byref(cur), C.byref(fb), out["state"].ctypes.data,
                                                          out["success"].ctypes.data, out["result"].ctypes.data, C.byref(ns), C.byref(outs)))
        finally:
            ctx._check(ctx.lib.svoh_matcher_collect(ctx.h))
        assert (dd["result"] == capi.MATCH_SUCCESS).sum() > n // 4      # the direct batch did run
    else:
        ctx._check(ctx.lib.svoh_update_seeds_batch_ex(ctx.h, C.byref(mopt), C.byref(dopt), len(refs), rv, C.byref(cur), C.byref(fb), out["state"].ctypes.data,
                                                      out["success"].ctypes.data, out["result"].ctypes.data, C.byref(ns), C.byref(outs)))
    assert ns.value == int(out["success"].sum())
    out["type"] = keep["type"]
    return out


def whole_sets_call(ctx, d, refs, cur, mopt, dopt):
    """The staged form whose units ARE the reference views' resident features, view after view (SVOH_BATCH_WHOLE_SETS)."""
    sd, n = d.sd, sx.N
    sel = [np.nonzero(sd["ref_frame_idx"] == r)[0] for r in range(len(refs))]
    assert np.array_equal(np.concatenate(sel), np.arange(n))       # the set lists its units view after view
    cols = [[np.ascontiguousarray(sd[k].reshape(n, -1)[s].ravel(), dt) for s in sel] for k, dt in (("px", np.float64), ("f", np.float64), ("grad", np.float64), ("level", np.int32))]
    m = len(sel)
    handles = (C.c_uint64 * m)()
    ctx._check(ctx.lib.svoh_features_upload(ctx.h, m, (C.c_int32 * m)(*[s.size for s in sel]), *[(C.c_void_p * m)(*[a.ctypes.data for a in col]) for col in cols], handles))
    try:
        rv = (capi.svoh_frame_view * m)(*refs)
        for k in range(m):
            rv[k].features = handles[k]
        cv = (capi.svoh_frame_view * 1)(cur)
        ctx._check(ctx.lib.svoh_matcher_begin_deferred(ctx.h))
        g = capi.svoh_matcher_stage_t()
        try:
            ctx._check(ctx.lib.svoh_matcher_stage(ctx.h, 1, n, m + 4, capi.SVOH_STAGE_MATCH_OUTPUTS | capi.SVOH_STAGE_RESIDENT_COLUMNS, C.byref(g)))
            _view(g.ref_frame_idx, np.int32, n)[:] = -7            # not read in this layout
            _view(g.feature_index, np.int32, n)[:] = 10 ** 7
            _view(g.cur_frame_idx, np.int32, n)[:] = 0
            _view(g.type, np.uint8, n)[:] = sd["type"]
            _view(g.state, np.float64, 4 * n)[:] = sd["state"]
            fb = capi.svoh_feature_batch()
            fb.n, fb.mem_space, fb.n_cur_frames, fb.layout = n, capi.SVOH_MEM_STAGED, 1, capi.SVOH_BATCH_WHOLE_SETS
            for k in ("ref_frame_idx", "cur_frame_idx", "type", "feature_index"):
                setattr(fb, k, getattr(g, k))
            outs = capi.svoh_seed_match_outputs(g.px_cur, g.f_cur, g.search_level, g.A_cur_ref)
            ctx._check(ctx.lib.svoh_update_seeds_batch_ex(ctx.h, C.byref(mopt), C.byref(dopt), m, rv, cv, C.byref(fb), g.state, g.success, g.result, None, C.byref(outs)))
        finally:
            ctx._check(ctx.lib.svoh_matcher_collect(ctx.h))
        return dict(state=_view(g.state, np.float64, 4 * n).copy(), type=_view(g.type, np.uint8, n).copy(), success=_view(g.success, np.uint8, n).copy(),
                    result=_view(g.result, np.int32, n).copy(), px_cur=_view(g.px_cur, np.float64, 2 * n).copy(), f_cur=_view(g.f_cur, np.float64, 3 * n).copy(),
                    search_level=_view(g.search_level, np.int32, n).copy(), A=_view(g.A_cur_ref, np.float64, 4 * n).copy())
    finally:
        for h in handles:
            ctx._check(ctx.lib.svoh_features_release(ctx.h, h))


def chain_call(ctx, d, refs, cur, mopt, dopt):
    """svoh_update_seeds_chain with the current frame as every reference view's one-frame list."""
    sd = d.sd
    fb, keep = fe.make_feature_batch(sd["ref_frame_idx"], sd["px"], sd["f"], sd["grad"], sd["level"], sd["type"])
    ns, st, n_ok, res, suc = ctx.update_seeds_chain(mopt, dopt, refs, fb, sd["state"], [cur], [[0]] * len(refs))
    assert ns == int(suc.sum()) and np.array_equal(n_ok, suc[:, 0])
    return dict(state=st, type=keep["type"], success=suc[:, 0].copy(), result=res[:, 0].copy())


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("run", sorted(sx.RUNS))
def test_every_form_of_the_seed_update_takes_every_exit_alike(gpu_ctx, oracle_lib, knobs, run):
    d, refs, cur, want = pack(gpu_ctx, oracle_lib)
    mopt, dopt = sx.options(d, run)
    got = {}
    for g in ("0", "1", "3", "2"):
        knobs(SVOH_MATCHER_G8=g)
        got["batch, geometry " + g] = host_call(gpu_ctx, d, refs, cur, mopt, dopt)
    knobs(SVOH_MATCHER_G8="2", SVOH_SEED_BINNING="0")
    got["batch, geometry 2 without binning"] = host_call(gpu_ctx, d, refs, cur, mopt, dopt)
    for g in (None, "2"):       # the launch rule's own choice (eight lanes per unit at this size), and the packed kernel's whole-sets build
        knobs(SVOH_MATCHER_G8=g)
        got["whole sets, geometry %s" % g] = whole_sets_call(gpu_ctx, d, refs, cur, mopt, dopt)
    for g in ("0", "1"):        # the two geometries the mixed kernel is built in
        knobs(SVOH_MATCHER_G8=g)
        got["deferred mixed launch, geometry " + g] = host_call(gpu_ctx, d, refs, cur, mopt, dopt, with_direct_batch=True)
    for g in ("0", "1", "3"):
        knobs(SVOH_MATCHER_G8=g)
        got["chain of one, geometry " + g] = chain_call(gpu_ctx, d, refs, cur, mopt, dopt)
    first = got["batch, geometry 0"]
    for form, out in got.items():
        for name, a in out.items():
            assert same_bytes(a, first[name]), (form, name, np.nonzero(np.asarray(a).ravel() != np.asarray(first[name]).ravel())[0][:10])
    w = want[run]
    for name in ("type", "success", "result"):
        assert np.array_equal(first[name], w[name]), (name, np.nonzero(first[name] != w[name])[0])
    assert np.allclose(first["state"], w["state"], rtol=1e-9, atol=0)
    # the run is the one the CPU test classified: every exit taken (by the GPU's own outputs)
    classes = sx.classify(d, run, first["state"], first["type"], first["success"], first["result"])
    assert not [name for name in sx.EXITS[run] if classes[name].size == 0]
    # units that did not run read back as zeros in the optional outputs
    idle = first["result"] == capi.MATCH_NOT_RUN
    assert not first["px_cur"].reshape(-1, 2)[idle].any() and not first["f_cur"].reshape(-1, 3)[idle].any() and not first["A"].reshape(-1, 4)[idle].any()
    assert not first["search_level"][idle].any() and first["px_cur"].reshape(-1, 2)[first["success"] == 1].all()
