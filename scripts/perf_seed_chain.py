"""What the seeds of new keyframes cost against their lists of frames: ONE svoh_update_seeds_chain call against the K
svoh_update_seeds_batch calls (one per list position) that did the same before, on the same inputs.

Cases: one keyframe of 360 seeds with a list of 6 frames (a stream's keyframe step), and 32 keyframes of 360 seeds with ragged
lists of 1 - 6 frames (a lock-step round).  Per arm: the wall time of the C call(s) and the device time of the kernel(s)
(svoh_last_kernel_ms), median of five, the two arms in turns.  Both arms must leave the same bytes.

    python scripts/perf_seed_chain.py [out.json]      (default: profiles/seed_chain.json)"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  first: libsvo_hip must share torch's HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from svo_pro_universal_amd import _capi as capi, frontend as fe, synth  # noqa: E402

PER_KF, N_VIEWS, REPS = 360, 6, 5


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "seed_chain.json")
    ctx = fe.Context(0, kernel_timing=True)
    lib, h = ctx.lib, ctx.h
    cam = synth.Camera.euroc_like(752, 480)
    sc = synth.make_align_scene(11, n_features=8, cam=cam, rot_deg=(0.3, 0.8), trans_m=(0.05, 0.12))
    rng = np.random.RandomState(5)
    fr = ctx.build_pyramid(sc.img_ref, 5)
    views = []
    for k in range(N_VIEWS):
        q = synth.quat_from_axis_angle(rng.normal(size=3), np.deg2rad(rng.uniform(0.3, 0.8)))
        t = rng.normal(size=3)
        T_w_c = sc.T_w_ref * synth.SE3(q, t / np.linalg.norm(t) * rng.uniform(0.05, 0.12))
        views.append(fe.make_frame_view(ctx.build_pyramid(synth.render(cam, T_w_c, sc.plane, sc.tex), 5), cam, T_w_c.inverse(), 0.0, 100 + k))
    mopt, dopt = capi.default_matcher_options(), capi.default_depth_filter_options(cam)
    cva = (capi.svoh_frame_view * N_VIEWS)(*views)
    results = {"per_keyframe_seeds": PER_KF, "reps": REPS, "statistic": "median", "unit": "us", "cases": {}}
    for name, n_kf in (("1_keyframe_x_360_x_chain_6", 1), ("32_keyframes_x_360_x_chains_1_to_6", 32)):
        # longest list first: the units still walking at list position j are then a prefix of the batch
        lens = [6] if n_kf == 1 else sorted((1 + (r * 5) // (n_kf - 1) for r in range(n_kf)), reverse=True)
        chains = [[(r + j) % N_VIEWS for j in range(lens[r])] for r in range(n_kf)]
        n = PER_KF * n_kf
        sd = synth.make_seed_set(sc, n)
        ref_idx = np.repeat(np.arange(n_kf, dtype=np.int32), PER_KF)
        fb, keep = fe.make_feature_batch(ref_idx, sd["px"], sd["f"], sd["grad"], sd["level"], sd["type"])
        rva = (capi.svoh_frame_view * n_kf)(*[fe.make_frame_view(fr, cam, sc.T_ref_f_w, sd["mu_range"], 1 + r) for r in range(n_kf)])
        state0, type0 = np.ascontiguousarray(sd["state"], np.float64), keep["type"].copy()
        begin = np.zeros(n_kf + 1, np.int32); begin[1:] = np.cumsum(lens)
        idx = np.ascontiguousarray([k for c in chains for k in c], np.int32)
        n_ok, ns, kms = np.zeros(n, np.int32), C.c_int32(), C.c_float()
        succ, mr = np.zeros(n, np.uint8), np.zeros(n, np.int32)
        # the K calls: position j takes the units of the keyframes whose list is longer than j, each into its own current frame
        steps = []
        for j in range(max(lens)):
            n_j = PER_KF * sum(1 for ln in lens if ln > j)
            cur_idx = np.ascontiguousarray(np.repeat([chains[r][j] for r in range(n_kf) if lens[r] > j], PER_KF), np.int32)
            steps.append((n_j, cur_idx))

        def chain_arm():
            st = state0.copy(); keep["type"][:] = type0
            fb.n, fb.cur_frame_idx, fb.n_cur_frames = n, None, 0
            t0 = time.perf_counter()
            rc = lib.svoh_update_seeds_chain(h, C.byref(mopt), C.byref(dopt), n_kf, rva, C.byref(fb), st.ctypes.data, N_VIEWS, cva, begin.ctypes.data,
                                             idx.ctypes.data, C.byref(ns), n_ok.ctypes.data, None, None, 0)
            wall = time.perf_counter() - t0
            assert rc == 0, lib.svoh_last_error_string(h)
            lib.svoh_last_kernel_ms(h, C.byref(kms))
            return wall * 1e6, kms.value * 1e3, st, keep["type"].copy(), ns.value

        def calls_arm():
            st = state0.copy(); keep["type"][:] = type0
            wall = kernel = 0.0
            total = 0
            for n_j, cur_idx in steps:
                fb.n, fb.cur_frame_idx, fb.n_cur_frames = n_j, cur_idx.ctypes.data, N_VIEWS
                t0 = time.perf_counter()
                rc = lib.svoh_update_seeds_batch(h, C.byref(mopt), C.byref(dopt), n_kf, rva, cva, C.byref(fb), st.ctypes.data, succ.ctypes.data, mr.ctypes.data, C.byref(ns))
                wall += time.perf_counter() - t0
                assert rc == 0, lib.svoh_last_error_string(h)
                lib.svoh_last_kernel_ms(h, C.byref(kms))
                kernel += kms.value
                total += ns.value
            return wall * 1e6, kernel * 1e3, st, keep["type"].copy(), total

        for _ in range(3):   # code objects, the staging blocks' first allocation
            a, b = chain_arm(), calls_arm()
        assert np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64)) and np.array_equal(a[3], b[3]) and a[4] == b[4], "the two arms differ"
        rows = {"chain": [], "k_calls": []}
        for _ in range(REPS):   # in turns
            rows["chain"].append(chain_arm()[:2])
            rows["k_calls"].append(calls_arm()[:2])
        case = {"n_keyframes": n_kf, "n_units": n, "chain_lengths": lens, "n_single_calls": len(steps), "n_step_successes": a[4]}
        for arm, v in rows.items():
            v = np.array(v)
            case[arm] = {"wall_us": round(float(np.median(v[:, 0])), 1), "kernel_us": round(float(np.median(v[:, 1])), 1),
                         "wall_us_all": [round(float(x), 1) for x in v[:, 0]], "kernel_us_all": [round(float(x), 1) for x in v[:, 1]]}
        results["cases"][name] = case
        print(name, {k: (case[k]["wall_us"], case[k]["kernel_us"]) for k in ("chain", "k_calls")}, "(wall us, kernel us)")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
