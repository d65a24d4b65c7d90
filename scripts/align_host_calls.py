#!/usr/bin/env python3
"""The HIP runtime calls the alignment's host side makes, scenario by scenario, for comparing two builds of the library.

  rocprofv3 --hip-trace --output-format csv -d DIR -o NAME -- python scripts/align_host_calls.py run
      One context, 320x240 images.  In order: four batch launches of num_cus + 17 problems queued back to back and fetched once; a
      keyed launch of 3 problems; an evaluation; a wide (equidistant) batch of 2 problems; a partial-sums + gn-update pair.  The list
      runs twice (the first pass makes the streams and grows every buffer, the second is the steady state), then the four-launch
      queue once more with SVOH_ALIGN_SIDE_COPIES=1 (the copy stream).  Every scenario stands between two hipRuntimeGetVersion calls,
      which nothing else in the process makes.  Prints a digest of every result, so that two builds can be seen to compute the same.

  python scripts/align_host_calls.py compare PARENT_hip_api_trace.csv NEW_hip_api_trace.csv
      Per scenario and thread, the ordered HIP call names of both traces: equal or not, with a digest and the first differences.
      (The CSV trace carries names, threads and times, no arguments: streams and events cannot be numbered from it.)
"""
import csv
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENARIOS = ["four_launch_queue", "keyed_3", "evaluation", "wide_batch_2", "partial_sums_gn_update"]
MARK = "hipRuntimeGetVersion"


def run():
    import numpy as np
    import torch  # noqa: F401  (loads the ROCm runtime the library links against)
    from svo_pro_universal_amd import _capi as capi, frontend as fe, synth

    hip = C.CDLL("libamdhip64.so")

    def mark():
        v = C.c_int()
        hip.hipRuntimeGetVersion(C.byref(v))

    digest = hashlib.sha256()

    def note(name, *arrays):
        h = hashlib.sha256()
        for a in arrays:
            h.update(np.ascontiguousarray(a).tobytes())
        digest.update(h.digest())
        print("%-28s %s" % (name, h.hexdigest()[:16]))

    ctx = fe.Context(0, kernel_timing=False)
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    cam = synth.Camera(320, 240, 160.0, 160.0, 160.0, 120.0)
    wide_cam = synth.Camera(320, 240, 160.0, 160.0, 160.0, 120.0, dist=[0.004, -0.028, 0.12, -0.107], model="equidistant")
    opt = capi.default_align_options(max_level=3, min_level=1)

    def scenes(camera, seeds, n_features):
        items = []
        for s in seeds:
            sc = synth.make_align_scene(s, n_features=n_features, patch_size=4, cam=camera, max_level=3)
            items.append([(sc, ctx.build_pyramid(sc.img_ref, 4), ctx.build_pyramid(sc.img_cur, 4))])
        return fe.make_align_problems(items)

    base, keep0 = scenes(cam, range(700, 708), 60)
    n_batch = num_cus + 17
    batch = (capi.svoh_align_problem * n_batch)(*[base[i % 8] for i in range(n_batch)])
    three = (capi.svoh_align_problem * 3)(*[base[i] for i in range(3)])
    wide, keep1 = scenes(wide_cam, range(720, 722), 60)
    d_state, d_sums = C.c_void_p(), C.c_void_p()
    ctx._check(ctx.lib.svoh_sparse_align_split_buffers(ctx.h, C.byref(d_state), C.byref(d_sums)))

    def four_launch_queue(tag):
        for _ in range(4):
            ctx.sparse_align_enqueue(opt, batch)
        note(tag, bytes(ctx.sparse_align_fetch_all(4 * n_batch)))

    def keyed_3(tag):
        k = C.c_int32()
        ctx._check(ctx.lib.svoh_sparse_align_geometry_key(ctx.h, C.byref(opt), C.byref(three[0]), C.byref(k)))
        ctx._check(ctx.lib.svoh_sparse_align_enqueue_keyed(ctx.h, C.byref(opt), 3, three, k.value))
        note(tag, bytes(ctx.sparse_align_fetch_all(3)))

    def evaluation(tag):
        H, g, chi2, nm, vis = ctx.sparse_align_evaluate(opt, base[1], 1)
        note(tag, H, g, np.array([chi2, nm]), vis)

    def wide_batch_2(tag):
        note(tag, bytes(ctx.sparse_align_wide(opt, wide)))

    def partial_sums_gn_update(tag):
        ctx.split_init(base[2], d_state.value)
        ctx.partial_sums(opt, base[2], 2, d_state.value, d_sums.value)
        st = ctx.gn_update(opt, base[2], 2, 0, d_sums.value, d_state.value)
        note(tag, bytes(st))

    steps = [four_launch_queue, keyed_3, evaluation, wide_batch_2, partial_sums_gn_update]
    for pass_ in ("cold", "warm"):
        for f in steps:
            mark()
            f("%s %s" % (pass_, f.__name__))
            mark()
    os.environ["SVOH_ALIGN_SIDE_COPIES"] = "1"
    ctx.reload_knobs()
    for pass_ in ("side cold", "side warm"):
        mark()
        four_launch_queue("%s four_launch_queue" % pass_)
        mark()
    print("all results %s" % digest.hexdigest()[:16])
    ctx.close()


def scenario_lists(path):
    """[(scenario index, {thread: [call names]})] from a rocprofv3 hip_api_trace.csv"""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), r["Thread_Id"], r["Function"]))
    rows.sort()
    marks = [i for i, r in enumerate(rows) if r[2] == MARK]
    assert len(marks) % 2 == 0 and marks, "%s: %d markers" % (path, len(marks))
    main_thread = rows[marks[0]][1]
    out = []
    for a, b in zip(marks[0::2], marks[1::2]):
        per_thread = {}
        for t, thread, fn in rows[a + 1:b]:
            per_thread.setdefault("main" if thread == main_thread else "other", []).append(fn)
        out.append(per_thread)
    return out


def compare(parent_csv, new_csv):
    names = ["cold " + s for s in SCENARIOS] + ["warm " + s for s in SCENARIOS] + ["side cold four_launch_queue", "side warm four_launch_queue"]
    A, B = scenario_lists(parent_csv), scenario_lists(new_csv)
    assert len(A) == len(B) == len(names), (len(A), len(B), len(names))
    differ = 0
    for name, a, b in zip(names, A, B):
        for thread in sorted(set(a) | set(b)):
            la, lb = a.get(thread, []), b.get(thread, [])
            da, db = (hashlib.sha256("\n".join(x).encode()).hexdigest()[:16] for x in (la, lb))
            same = la == lb
            differ += not same
            print("%-32s thread %-5s parent %4d calls %s | new %4d calls %s  %s" % (name, thread, len(la), da, len(lb), db, "equal" if same else "DIFFERENT"))
            if not same:
                for i, (x, y) in enumerate(zip(la + [None] * len(lb), lb + [None] * len(la))):
                    if x != y:
                        print("    first difference at call %d: parent %s | new %s" % (i, x, y))
                        print("    parent: %s" % " ".join(map(str, la[max(0, i - 3):i + 6])))
                        print("    new:    %s" % " ".join(map(str, lb[max(0, i - 3):i + 6])))
                        break
    print("%d scenario/thread list(s) differ" % differ)
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
