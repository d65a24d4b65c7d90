"""The scenarios of tests/test_align_side_copies_gpu.py, run in a process of their own (the test starts one per setting of
SVOH_ALIGN_SIDE_COPIES): launches of the alignment's batch build queued back to back, whose uploads and downloads travel on the
alignment's copy stream beside the neighbouring kernels (csrc/svoh_internal.h, "side copies").

  python align_side_copies_child.py OUT.json

Every scenario compares bits with the same problem set run ALONE through svoh_sparse_align_batch in this process and writes what it
found -- rows that differ, a SHA-256 of what it fetched, how many launches took the side path (the counter of
libsvo_hip_testhooks.so) -- into OUT.json; the test asserts.  The last scenario destroys the context with launches queued and not
fetched: the process must still end with status 0."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import torch  # noqa: F401  -- before libsvo_hip is loaded: one HIP runtime for both

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from svo_pro_universal_amd import _capi as capi, frontend as fe  # noqa: E402
from oracle import oracle as orc  # noqa: E402  -- BatchSet keeps the oracle's pyramids beside the device's; nothing here asks the oracle

import align_batch_set as bs  # noqa: E402


def result_bytes(res):
    return np.frombuffer(bytes(res), dtype=np.uint8).reshape(len(res), C.sizeof(capi.svoh_align_result)).copy()


def reordered(problems, order):
    return (capi.svoh_align_problem * len(order))(*[problems[int(i)] for i in order])


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def host_arrays(problems):
    """NumPy views of the host-resident feature arrays the problems point at"""
    views = []
    for pb in problems:
        for c in range(pb.n_cams):
            cam = pb.cams[c]
            if cam.mem_space != capi.SVOH_MEM_HOST or cam.n_features == 0:
                continue
            n = cam.n_features
            for ptr, count, ctype in ((cam.px, 2 * n, C.c_double), (cam.f, 3 * n, C.c_double), (cam.pos_world, 3 * n, C.c_double),
                                      (cam.flags, n, C.c_uint8)):
                addr = C.cast(ptr, C.c_void_p).value
                views.append(np.ctypeslib.as_array((ctype * count).from_address(addr)))
    return views


def main(out_path):
    orc.build()
    hooks = capi.load(capi.TESTHOOKS_LIB_PATH)
    hooks.svoh_test_align_side_launches.restype = C.c_ulonglong
    hooks.svoh_test_align_side_launches.argtypes = [C.c_void_p]
    ctx = fe.Context(0, lib=hooks)
    lib, h = ctx.lib, ctx.h
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    full = bs.compose(num_cus)
    S = bs.BatchSet(ctx, orc, bs.Composition(num_cus, full.seed, [], full.mid))   # the mid set alone: num_cus + 17 problems
    L = S.launch("mid", 4)
    n = len(L.problems)
    opt = capi.default_align_options(patch_size=4, min_level=0)
    out = {"n": n, "num_cus": num_cus, "setting": os.environ.get("SVOH_ALIGN_SIDE_COPIES")}

    def side_launches():
        return int(hooks.svoh_test_align_side_launches(h))

    # three sets of different contents: the ragged set, reversed, and its odd problems followed by its even ones
    orders = {"A": np.arange(n), "B": np.arange(n)[::-1], "C": np.concatenate([np.arange(1, n, 2), np.arange(0, n, 2)])}
    sets = {k: reordered(L.problems, o) for k, o in orders.items()}
    alone, builds = {}, {}
    for k in "ABC":
        alone[k] = result_bytes(ctx.sparse_align(opt, sets[k]))
        builds[k] = ctx.last_align_launch()
    out["alone_sha"] = {k: sha(alone[k]) for k in "ABC"}
    out["alone_builds"] = builds
    out["alone_consistent"] = bool(np.array_equal(alone["B"], alone["A"][orders["B"]]) and np.array_equal(alone["C"], alone["A"][orders["C"]]))
    out["side_after_blocking_calls"] = side_launches()

    def queue(names, after_enqueue=None):
        before = side_launches()
        for k in names:
            ctx.sparse_align_enqueue(opt, sets[k])
            if after_enqueue:
                after_enqueue(k)
        return before

    def differing(got, names):
        want = np.concatenate([alone[k] for k in names])
        return [int(i) for i in np.flatnonzero((got != want).any(1))[:20]]

    # 1. five launches back to back, one fetch_all: every device block and every pinned block is used again with other contents
    names = "ABCAB"
    before = queue(names)
    got = result_bytes(ctx.sparse_align_fetch_all(len(names) * n))
    out["five"] = {"differ": differing(got, names), "sha": sha(got), "side": side_launches() - before}

    # 1b. a queue longer than the result blocks were made for: the first launch of a queue reserves room for 32 launches of its
    #     size and the buffers add half of that, so launch 49 finds both the device block and the pinned block of results full
    #     and drains -- with results of the launches before it still held back or on the copy stream -- before it replaces them
    names = "ABC" * 20
    before = queue(names)
    got = result_bytes(ctx.sparse_align_fetch_all(len(names) * n))
    out["grow"] = {"differ": differing(got, names), "sha": sha(got), "side": side_launches() - before, "launches": len(names)}

    # 2. the host-resident feature arrays are overwritten right after each enqueue returns: the staging copy is the launch's own
    views = host_arrays(L.problems)
    saved = [v.copy() for v in views]
    out["host_arrays"] = len(views)

    def garbage(_k):
        for v in views:
            v.view(np.uint8)[:] = 0xA5

    def restore():
        for v, s in zip(views, saved):
            v[:] = s

    names = "ABCA"
    before = side_launches()
    for k in names:
        restore()
        ctx.sparse_align_enqueue(opt, sets[k])
        garbage(k)
    got = result_bytes(ctx.sparse_align_fetch_all(len(names) * n))
    restore()
    out["garbage"] = {"differ": differing(got, names), "sha": sha(got), "side": side_launches() - before}

    # 3. a refused enqueue between two queued launches: set B with an unknown frame handle in its LAST problem, so that the call
    #    fails after it has written nearly all of the staging block it picked
    bad = reordered(L.problems, orders["B"])
    bad[n - 1].cams[0].cur_frame = 987654321
    refused, differ, side = [], [], []
    for _ in range(3):
        before = side_launches()
        ctx.sparse_align_enqueue(opt, sets["A"])
        refused.append(int(lib.svoh_sparse_align_enqueue(h, C.byref(opt), n, bad)))
        ctx.sparse_align_enqueue(opt, sets["B"])
        got = result_bytes(ctx.sparse_align_fetch_all(2 * n))
        differ += differing(got, "AB")
        side.append(side_launches() - before)
    out["refused"] = {"rc": refused, "differ": differ, "side": side, "sha": sha(got)}

    # 4. mixed queue: a small launch (8 problems: the context's stream) between two batch launches, and a candidate projection
    #    behind all three that composes its pose on the device from a result of the LAST launch; against the blocking sequence
    small = reordered(L.problems, [i for i, s in enumerate(L.specs) if s.kind == "mono" and s.n_features < 400][:8])
    pick = [j for j, i in enumerate(orders["C"]) if L.specs[int(i)].ordinary][0]   # an ordinary one-camera problem of set C
    sc = L.scenes[int(orders["C"][pick])][0]
    rng = np.random.RandomState(4)
    m = 1500
    kind = (rng.uniform(size=m) < 0.5).astype(np.uint8)
    kf = rng.randint(0, 2, m).astype(np.int32)
    from svo_pro_universal_amd import synth
    T_w_kf = [sc.T_w_ref, sc.T_w_ref * synth.SE3(synth.quat_from_axis_angle([0, 1, 0], 0.2), (0.3, 0.0, 0.1))]
    v, mu = np.zeros((m, 3)), np.ones(m)
    for i in range(m):
        if kind[i]:
            f = np.array([rng.uniform(-0.9, 0.9), rng.uniform(-0.7, 0.7), 1.0])
            v[i] = f / np.linalg.norm(f)
            mu[i] = 1.0 / rng.uniform(0.5, 8.0)
        else:
            v[i] = sc.T_w_cur.transform(np.array([rng.uniform(-6, 6), rng.uniform(-4, 4), rng.uniform(-1.0, 8.0)]))
    T_imu_world_ref = sc.T_imu_cam * sc.T_ref_f_w if hasattr(sc, "T_imu_cam") else sc.T_ref_f_w
    Ta, Tb = fe._se3(sc.T_cam_imu), fe._se3(T_imu_world_ref)
    Tk = (capi.svoh_se3 * 2)(*[fe._se3(t) for t in T_w_kf])
    cam = fe._camera(sc.cam)
    v_flat = np.ascontiguousarray(v).ravel()

    def project(index):
        rc = lib.svoh_project_candidates_enqueue(h, C.byref(cam), C.byref(Ta), C.byref(Tb), index, 2, Tk, m, kind.ctypes.data, kf.ctypes.data,
                                                 v_flat.ctypes.data, mu.ctypes.data)
        assert rc == 0, lib.svoh_last_error_string(h)

    def collect():
        px, vis = np.zeros(2 * m), np.zeros(m, np.uint8)
        assert lib.svoh_project_candidates_collect(h, m, px.ctypes.data, vis.ctypes.data) == 0, lib.svoh_last_error_string(h)
        return px, vis

    # the blocking sequence
    want_small = result_bytes(ctx.sparse_align(opt, small))
    small_build = ctx.last_align_launch()
    ctx.sparse_align_enqueue(opt, sets["C"])
    project(pick)
    want_c = result_bytes(ctx.sparse_align_fetch(n))
    want_px, want_vis = collect()
    # the queue
    before = side_launches()
    ctx.sparse_align_enqueue(opt, sets["A"])
    ctx.sparse_align_enqueue(opt, small)
    ctx.sparse_align_enqueue(opt, sets["C"])
    project(n + 8 + pick)
    got = result_bytes(ctx.sparse_align_fetch_all(2 * n + 8))
    px, vis = collect()
    want = np.concatenate([alone["A"], want_small, alone["C"]])
    out["mixed"] = {"differ": [int(i) for i in np.flatnonzero((got != want).any(1))[:20]], "sha": sha(got, px, vis),
                    "blocking_c_is_alone_c": bool(np.array_equal(want_c, alone["C"])), "small_build": small_build,
                    "projection_equal": bool(np.array_equal(px.view(np.uint64), want_px.view(np.uint64)) and np.array_equal(vis, want_vis)),
                    "visible": int(vis.sum()), "points": m, "side": side_launches() - before}

    # 5. fetch(n) hands out the LAST launch only and ends the queue; a new queue starts from nothing
    before = queue("ABC")
    last = result_bytes(ctx.sparse_align_fetch(n))
    side_first = side_launches() - before
    before = queue("BA")
    got = result_bytes(ctx.sparse_align_fetch_all(2 * n))
    try:
        ctx.sparse_align_fetch_all(1)
        nothing_left = False
    except fe.SvohError:
        nothing_left = True
    out["fetch_last"] = {"last_differ": differing(last, "C"), "differ": differing(got, "BA"), "sha": sha(last, got), "nothing_left": nothing_left,
                         "side": [side_first, side_launches() - before]}

    # 6. the context destroyed with launches queued and not fetched (their results still on their way)
    before = queue("ABC")
    out["destroy"] = {"side": side_launches() - before}
    with open(out_path, "w") as f:
        json.dump(out, f)
    ctx.close()
    print("align_side_copies_child: done", flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
