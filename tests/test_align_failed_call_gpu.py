"""Calls that do not launch, between launches that do: a call that fails in its fill pass, a blocking wide call that is refused
because results are pending, and an evaluation between two queued launches leave the launches queued around them with the bits
they have when run alone.  (The rule behind the first -- a descriptor slot is taken only once the upload has been queued -- is
pinned without a device by tests/test_align_queue_cpu.py; here a wrongly advanced slot would be a race between the host's writes
and an upload in flight, which blocks this small need not lose.  This test holds the results, the error codes and the texts.)

160x120 images, levels 2..0, 4x4 patches; two sets A and B of three problems with 12 - 20 features each, on a context of its own
(the queue's slots and lanes start from nothing)."""
import ctypes as C

import numpy as np
import pytest

from svo_pro_universal_amd import _capi as capi, frontend as fe, synth

pytestmark = pytest.mark.gpu

N_FEATURES = {"A": (12, 16, 20), "B": (20, 13, 17)}
SVOH_ERR_BAD_HANDLE = -4   # include/svo_hip.h, svoh_status


def result_bytes(res):
    return np.frombuffer(bytes(res), dtype=np.uint8).reshape(len(res), C.sizeof(capi.svoh_align_result)).copy()


def flat(ev):
    return [np.asarray(x, dtype=np.float64).ravel() for x in ev]


@pytest.fixture(scope="module")
def bench():
    ctx = fe.Context(0)
    cam = synth.Camera(160, 120, 80.0, 80.0, 80.0, 60.0)
    opt = capi.default_align_options(max_level=2, min_level=0, patch_size=4)
    sets, keep = {}, []
    seed = 4100
    for name, counts in N_FEATURES.items():
        items = []
        for n in counts:
            sc = synth.make_align_scene(seed, n_features=n, patch_size=4, cam=cam, max_level=2)
            seed += 1
            items.append([(sc, ctx.build_pyramid(sc.img_ref, 3), ctx.build_pyramid(sc.img_cur, 3))])
        pb, k = fe.make_align_problems(items)
        sets[name] = pb
        keep.append(k)
    alone = {name: result_bytes(ctx.sparse_align(opt, pb)) for name, pb in sets.items()}   # svoh_sparse_align_batch, each set alone
    # the premise: every problem ran (status 0) and tracked its features
    for name, pb in sets.items():
        for r in ctx.sparse_align(opt, pb):
            print("[failed-call sets] %s: status %d, %d features tracked, iterations %s" % (name, r.status, r.n_fts_to_track, list(r.iters)[:3]))
            assert r.status == 0 and r.n_fts_to_track >= 1, (name, r.status, r.n_fts_to_track)
    bad = (capi.svoh_align_problem * 3)(*[sets["B"][i] for i in range(3)])
    bad[2].cams[0].ref_frame = 0x7fffffffffff   # a handle no frame has: problems 0 and 1 are staged before the call fails
    yield dict(ctx=ctx, opt=opt, sets=sets, alone=alone, bad=bad, keep=keep)
    ctx.close()


def queued(bench, between):
    """A queued, `between`, B queued, one fetch_all"""
    ctx, opt, sets = bench["ctx"], bench["opt"], bench["sets"]
    ctx.sparse_align_enqueue(opt, sets["A"])
    between()
    ctx.sparse_align_enqueue(opt, sets["B"])
    got = result_bytes(ctx.sparse_align_fetch_all(6))
    want = np.concatenate([bench["alone"]["A"], bench["alone"]["B"]])
    return got, want


def test_a_call_that_fails_in_its_fill_pass_leaves_the_queue_alone(bench):
    ctx, opt = bench["ctx"], bench["opt"]

    def fails():
        with pytest.raises(fe.SvohError) as e:
            ctx.sparse_align_enqueue(opt, bench["bad"])
        assert e.value.code == SVOH_ERR_BAD_HANDLE and "problem 2 camera 0: unknown frame handle" in str(e.value)

    for _ in range(2):   # the second round starts on the other descriptor slot
        got, want = queued(bench, fails)
        assert np.array_equal(got, want), np.flatnonzero((got != want).any(1))
    # two failing calls in a row, and one in front of the first launch
    fails()
    got, want = queued(bench, lambda: (fails(), fails()))
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(1))


def test_a_refused_wide_call_leaves_the_queue_alone(bench):
    ctx, opt = bench["ctx"], bench["opt"]

    def refused():
        with pytest.raises(fe.SvohError) as e:
            ctx.sparse_align_wide(opt, bench["sets"]["B"])
        assert e.value.code == capi.SVOH_ERR_INVALID_ARGUMENT
        assert "the wide alignment entries are blocking: fetch the results of earlier svoh_sparse_align_enqueue calls first" in str(e.value)

    got, want = queued(bench, refused)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(1))


def test_an_evaluation_between_two_queued_launches(bench):
    ctx, opt, sets = bench["ctx"], bench["opt"], bench["sets"]
    want_eval = flat(ctx.sparse_align_evaluate(opt, sets["A"][1], 1))
    got_eval = []
    got, want = queued(bench, lambda: got_eval.extend(flat(ctx.sparse_align_evaluate(opt, sets["A"][1], 1))))
    assert len(got_eval) == len(want_eval) and all(np.array_equal(a, b) for a, b in zip(got_eval, want_eval))
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(1))
