"""The scenarios of tests/test_align_overlap_gpu.py, run in a process of their own (the test starts one per setting of
SVOH_ALIGN_OVERLAP / SVOH_ALIGN_SIDE_COPIES): launches of the alignment's batch build queued back to back, every second one of which
runs on the alignment's second launch lane, beside the tail of the launch before it (csrc/svoh_internal.h, "launch lanes").

  python align_overlap_child.py OUT.json

Shapes: 320x240 images, levels 2..0, 4x4 patches, six parameters, 12..64 features per problem; set A has num_cus + 17 problems --
the smallest launch that takes the batch build and gives workgroups a second problem -- sets B, C and D are larger, so that both
lanes' workspaces have to grow.  Every scenario compares bits with the same set run ALONE through svoh_sparse_align_batch (a
blocking call is never overlapped; the test compares the SHA-256 with the child that ran under SVOH_ALIGN_OVERLAP=0), and the sets
run alone are held against the oracle at the bars of tests/test_sparse_align_batch_build_gpu.py.

Every step runs under a time limit of its own (SIGALRM ends the process: the test sees the status and stops).  The last scenario
destroys the context with two launches queued and not fetched, then runs set A on a second context."""
import ctypes as C
import hashlib
import json
import os
import signal
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch  # noqa: F401  -- before libsvo_hip is loaded: one HIP runtime for both

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from svo_pro_universal_amd import _capi as capi, frontend as fe  # noqa: E402
from oracle import oracle as orc  # noqa: E402

import align_batch_set as bs  # noqa: E402
import helpers  # noqa: E402

STEP_SECONDS = 120
GROWTH_QUEUES = ("ABC", "ACD", "BD", "AB", "CD", "AD")


def step(name):
    """the step that begins here has STEP_SECONDS to finish"""
    signal.alarm(STEP_SECONDS)
    print("align_overlap_child: " + name, flush=True)


def result_bytes(res):
    return np.frombuffer(bytes(res), dtype=np.uint8).reshape(len(res), C.sizeof(capi.svoh_align_result)).copy()


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# Scenes the ORACLE cannot judge (as REPLACED_SCENE_SEEDS of align_batch_set.py): a few dozen features on a 320x240 image leave some
# problems so ill-conditioned that the oracle's own pose moves by more than the 1e-8 it is asked to judge by when nothing but the
# order of its features -- the order of its sums -- changes.  Such a scene gets another seed (+100000).  The criterion involves the
# oracle alone, and the child holds every problem it runs to it ("oracle_self" in its output).
UNJUDGED_SCENE_SEEDS = frozenset((
    700005, 700045, 700049, 700056, 700061, 700066, 700120, 700131, 700145, 700167, 700169, 700174, 700189, 700191, 700199, 700226,
    700267, 700325, 700344, 700358, 700363, 700451, 700460, 700575, 700602, 700627, 700633, 700640, 700645, 700655, 700679, 700732,
    700768, 700805, 700813, 700824, 700846, 700885, 700910, 700947, 700948, 700999, 701026, 701034, 701046, 701055, 701060, 701072,
    701141, 701165, 701196, 701207, 701239, 701261, 701262, 701282, 701286, 701343, 701347, 701357, 701370, 701373, 701393, 701406,
    701424, 701449, 701483, 701501, 800061, 800131, 800167, 800575, 800627, 800640, 800645, 800679, 900131, 900627,
))


def compose_sets(num_cus, seed=20250307):
    """name -> specs.  A: num_cus + 17 problems of 12..64 features.  B, C: a third more problems, near 64 features each, so that their
    workspace (50 bytes per feature) no longer fits the megabyte a workspace starts with; D: twice A, past what B's grew to."""
    rng = np.random.RandomState(seed)
    n_a = num_cus + 17
    n_b = max(n_a + 24, 21500 // 61 + 1)
    n_d = max(2 * n_a, 36000 // 61 + 1)
    sets, next_seed = {}, [700000]

    def spec(n):
        next_seed[0] += 1
        sd = next_seed[0]
        while sd in UNJUDGED_SCENE_SEEDS:
            sd += 100000
        return bs.ProblemSpec("mono", [bs.CamSpec("small320", sd, n, gain=1.0 + 0.04 * rng.uniform(), offset=3.0 * rng.uniform())],
                              mem="host" if rng.uniform() < 0.2 else "device")

    sets["A"] = [spec(n) for n in [12, 33, 63, 64] + [int(x) for x in rng.randint(12, 65, n_a - 4)]]
    for name, n in (("B", n_b), ("C", n_b), ("D", n_d)):
        sets[name] = [spec(k) for k in [12, 64] + [int(x) for x in rng.randint(58, 65, n - 2)]]
    big = bs.ProblemSpec("mono", [bs.CamSpec("pinhole640", 799999, 720)], mem="device")   # the cluster launch of scenario 4
    return sets, big


def compare_with_oracle(specs, res, oracle):
    """compare_with_oracle of tests/test_sparse_align_batch_build_gpu.py: the indices that miss its bars, and the largest pose difference"""
    bad, worst = [], 0.0
    for i, (s, rg, (n, ro)) in enumerate(zip(specs, res, oracle)):
        d_pose = helpers.se3_max_abs_diff(rg.T_icur_iref, ro.T_icur_iref)
        ok = (rg.n_fts_to_track == n and rg.status == ro.status and list(rg.iters) == list(ro.iters) and list(rg.n_meas) == list(ro.n_meas)
              and rg.n_patch_iters == ro.n_patch_iters and d_pose < helpers.TOL_POSE and abs(rg.alpha - ro.alpha) < helpers.TOL_POSE
              and abs(rg.beta - ro.beta) < 1e-6)
        worst = max(worst, float(d_pose))
        if not ok:
            bad.append(i)
    return bad[:20], worst


def main(out_path):
    step("set-up")
    orc.build()
    lib = capi.load()
    ctx = fe.Context(0, lib=lib)
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    sets, big = compose_sets(num_cus)
    names = "ABCD"
    S = bs.BatchSet(ctx, orc, bs.Composition(num_cus, 0, [], sum((sets[k] for k in names), []) + [big]))
    L = S.launch("mid", 4)
    opt = capi.default_align_options(patch_size=4, max_level=2, min_level=0)
    bounds = np.cumsum([0] + [len(sets[k]) for k in names])
    idx = {k: np.arange(bounds[i], bounds[i + 1]) for i, k in enumerate(names)}
    pb = {k: (capi.svoh_align_problem * len(idx[k]))(*[L.problems[int(i)] for i in idx[k]]) for k in names}
    n_of = {k: len(idx[k]) for k in names}
    big_pb = (capi.svoh_align_problem * 1)(L.problems[int(bounds[-1])])
    small_pb = (capi.svoh_align_problem * 8)(*[L.problems[int(i)] for i in idx["C"][10:18]])
    out = {"num_cus": num_cus, "n": n_of, "features": {k: int(sum(s.n_features for s in sets[k])) for k in names},
           "overlap": os.environ.get("SVOH_ALIGN_OVERLAP"), "side": os.environ.get("SVOH_ALIGN_SIDE_COPIES")}

    def lane1():
        return ctx.last_align_lane()["lane1_launches"]

    def enqueue(k, lanes=None):
        ctx.sparse_align_enqueue(opt, pb[k])
        if lanes is not None:
            lanes.append(ctx.last_align_lane()["lane"])

    # 2. (first, while the context's workspaces are what a new context has) fetch after every second or third enqueue, a launch pending
    #    on each lane; the later launches of a queue are larger than the first.
    #      A B C   B, the context's first launch into the second descriptor block, waits for A as it always has; C takes lane 1
    #      A C D   D, on lane 0 again, outgrows the first workspace (B's size) while C runs on lane 1: it waits for both lanes
    #      B D     D outgrows what C made of the second workspace while B runs on lane 0: again
    #      A B, C D, A D   nothing left to grow: the second launch of each pair runs on lane 1
    step("growth")
    got, lanes = {}, []
    for q in GROWTH_QUEUES:
        for k in q:
            enqueue(k, lanes)
        got[q] = result_bytes(ctx.sparse_align_fetch_all(sum(n_of[k] for k in q)))
    out["growth"] = {"lanes": lanes, "lane1": lane1()}

    # 1. four launches back to back with four different sets, one fetch_all
    step("four launches")
    before, lanes = lane1(), []
    for k in names:
        enqueue(k, lanes)
    got["ABCD"] = result_bytes(ctx.sparse_align_fetch_all(sum(n_of.values())))
    out["four"] = {"lanes": lanes, "lane1": lane1() - before}

    # the sets run alone, and the oracle on them
    step("alone")
    alone, alone_res, builds = {}, {}, {}
    for k in names:
        alone_res[k] = ctx.sparse_align(opt, pb[k])
        alone[k] = result_bytes(alone_res[k])
        builds[k] = dict(ctx.last_align_launch(), **ctx.last_align_lane())
    out["alone_sha"] = {k: sha(alone[k]) for k in names}
    out["alone_builds"] = builds
    step("oracle")
    out["oracle"] = {}
    with ThreadPoolExecutor(max_workers=16) as ex:   # a ctypes call: releases the GIL
        for k in names:
            ref = list(ex.map(lambda p: orc.sparse_align_run(opt, p)[:2], [L.oracle_problems[int(i)] for i in idx[k]]))
            bad, worst = compare_with_oracle(sets[k], alone_res[k], ref)
            # the oracle against itself with every problem's features in another order: what it cannot tell from itself it cannot judge
            again = list(ex.map(lambda p: orc.sparse_align_run(opt, p)[:2], [L.oracle_problems_permuted[int(i)] for i in idx[k]]))
            unjudged, _ = compare_with_oracle(sets[k], [ro for _, ro in ref], [(n, ro) for (n, _), (_, ro) in zip(ref, again)])
            unjudged += [i for i, ((n, _), (n2, _)) in enumerate(zip(ref, again)) if n != n2]
            out["oracle"][k] = {"bad": bad, "worst_pose": worst, "tracked": int(sum(r.n_fts_to_track for r in alone_res[k])),
                                "oracle_self": [sets[k][i].cams[0].seed for i in unjudged]}

    def differing(g, order):
        want = np.concatenate([alone[k] for k in order])
        return [int(i) for i in np.flatnonzero((g != want).any(1))[:20]]

    out["growth"]["differ"] = {q: differing(got[q], q) for q in GROWTH_QUEUES}
    out["growth"]["sha"] = sha(*[got[q] for q in GROWTH_QUEUES])
    out["four"]["differ"] = differing(got["ABCD"], names)
    out["four"]["sha"] = sha(got["ABCD"])

    # 3. a blocking entry that uses the context's stream behind a launch on each lane: a pyramid build whose levels come back
    step("join")
    img = (np.random.RandomState(3).randint(0, 256, (240, 320))).astype(np.uint8)
    f0, want_levels = ctx.build_pyramid(img, 4, return_levels=True)
    ctx.release_frame(f0)
    before, lanes = lane1(), []
    enqueue("A", lanes); enqueue("B", lanes)
    f1, levels = ctx.build_pyramid(img, 4, return_levels=True)
    g = result_bytes(ctx.sparse_align_fetch_all(n_of["A"] + n_of["B"]))
    ctx.release_frame(f1)
    out["join"] = {"lanes": lanes, "lane1": lane1() - before, "differ": differing(g, "AB"), "sha": sha(g, *levels),
                   "pyramid_equal": bool(all(np.array_equal(a, b) for a, b in zip(levels, want_levels))),
                   "error": lib.svoh_last_error_string(ctx.h).decode()}

    # 4. what must stay on lane 0, between two pairs of overlapped launches: a cluster launch (one problem of 720 features), a small
    #    launch (8 problems), an evaluation
    step("lane 0 paths")
    want_big = result_bytes(ctx.sparse_align(opt, big_pb))
    big_build = ctx.last_align_launch()
    want_small = result_bytes(ctx.sparse_align(opt, small_pb))
    small_build = ctx.last_align_launch()
    want_eval = ctx.sparse_align_evaluate(opt, pb["A"][1], 1)
    before, lanes = lane1(), []
    enqueue("A", lanes); enqueue("B", lanes)
    ctx.sparse_align_enqueue(opt, big_pb); lanes.append(ctx.last_align_lane()["lane"])
    ctx.sparse_align_enqueue(opt, small_pb); lanes.append(ctx.last_align_lane()["lane"])
    enqueue("C", lanes); enqueue("D", lanes)
    got_eval = ctx.sparse_align_evaluate(opt, pb["A"][1], 1)
    lanes.append(ctx.last_align_lane()["lane"])
    enqueue("A", lanes); enqueue("B", lanes)
    g = result_bytes(ctx.sparse_align_fetch_all(2 * n_of["A"] + 2 * n_of["B"] + 1 + 8 + n_of["C"] + n_of["D"]))
    want = np.concatenate([alone["A"], alone["B"], want_big, want_small, alone["C"], alone["D"], alone["A"], alone["B"]])

    def flat(ev):
        return [np.asarray(x, dtype=np.float64).ravel() for x in ev]

    out["lane0"] = {"lanes": lanes, "lane1": lane1() - before, "differ": [int(i) for i in np.flatnonzero((g != want).any(1))[:20]],
                    "sha": sha(g, *flat(got_eval)), "big_build": big_build, "small_build": small_build,
                    "eval_equal": bool(all(np.array_equal(a, b) for a, b in zip(flat(got_eval), flat(want_eval))))}
    out["lanes"] = ctx.last_align_lane()["lanes"]

    # 5. the context destroyed with a launch pending on each lane; then set A on a second context
    step("destroy")
    before, lanes = lane1(), []
    enqueue("A", lanes); enqueue("B", lanes)
    out["destroy"] = {"lanes": lanes, "lane1": lane1() - before}
    ctx.close()
    step("second context")
    ctx2 = fe.Context(0, lib=lib)
    S2 = bs.BatchSet(ctx2, orc, bs.Composition(num_cus, 0, [], sets["A"]))
    L2 = S2.launch("mid", 4)
    again = result_bytes(ctx2.sparse_align(opt, L2.problems))
    out["second_context"] = {"differ": differing(again, "A"), "sha": sha(again)}
    with open(out_path, "w") as f:
        json.dump(out, f)
    S2.close()
    ctx2.close()
    signal.alarm(0)
    print("align_overlap_child: done", flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
