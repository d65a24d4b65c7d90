"""Side copies of the alignment batch (csrc/svoh_internal.h): a launch of the batch build queued behind an alignment launch that is
still in flight uploads its descriptor block on the alignment's copy stream, into the device block the running kernel does not read,
and its results come down on that stream beside the next kernel.  Nothing a caller sees may change: every scenario of
tests/align_side_copies_child.py compares bits with the same problems run alone through svoh_sparse_align_batch.

The child runs once with SVOH_ALIGN_SIDE_COPIES=1 and once with =0, each time in a fresh process (the knob is read when a context
is made; the copy stream and both device blocks start from nothing), on the ragged mid set of tests/align_batch_set.py: num_cus + 17
problems, the smallest launch that takes the batch build.  (=1 and not the default: left alone, the library keeps a launch whose
block is no larger than 1 MB -- this set's is -- on the context's stream, where copy kernels move it; =1 sends every queued batch
launch over the copy stream.)"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SETTINGS = ("1", "0")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    out = {}
    for setting in SETTINGS:
        path = str(tmp_path_factory.mktemp("side_copies") / ("out_%s.json" % setting))
        env = dict(os.environ)
        env["SVOH_ALIGN_SIDE_COPIES"] = setting
        p = subprocess.run([sys.executable, "-s", os.path.join(HERE, "align_side_copies_child.py"), path], env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        text = p.stdout.decode(errors="replace")
        # (6: the child's last act is to destroy its context with three launches queued and not fetched)
        assert p.returncode == 0 and "align_side_copies_child: done" in text, "child (%s) ended with %r:\n%s" % (setting, p.returncode, text[-4000:])
        out[setting] = json.load(open(path))
    return out


@pytest.mark.parametrize("setting", SETTINGS)
def test_premises(runs, setting):
    """the sets run alone take the batch build, agree with each other problem by problem, and blocking calls never take the side path"""
    r = runs[setting]
    assert r["n"] == r["num_cus"] + 17
    for k in "ABC":
        b = r["alone_builds"][k]
        assert b["nt"] == 256 and b["latency"] is False and b["cluster_g"] == 0 and b["rows"] == 1 and b["n_desc"] == r["n"], b
    assert r["alone_consistent"] and r["side_after_blocking_calls"] == 0
    assert r["host_arrays"] >= 4 * 10          # the garbage scenario has something to overwrite
    assert r["setting"] == setting


@pytest.mark.parametrize("setting", SETTINGS)
def test_five_queued_launches_one_fetch_all(runs, setting):
    """A B C A B back to back: each device block and each pinned block is reused at least twice with other contents"""
    assert runs[setting]["five"]["differ"] == []


@pytest.mark.parametrize("setting", SETTINGS)
def test_queue_that_outgrows_the_result_blocks(runs, setting):
    """60 launches, one fetch_all: the 49th drains and replaces the device and the pinned result block while copies of earlier
    results are held back or under way on the copy stream (the drain shows in the counter: the launch behind it is the first of a
    queue again)"""
    r = runs[setting]["grow"]
    assert r["launches"] == 60 and r["differ"] == []
    if setting == "1":
        assert 56 <= r["side"] <= 58, r["side"]


@pytest.mark.parametrize("setting", SETTINGS)
def test_host_arrays_overwritten_after_enqueue(runs, setting):
    assert runs[setting]["garbage"]["differ"] == []


@pytest.mark.parametrize("setting", SETTINGS)
def test_refused_enqueue_between_two_queued_batch_launches(runs, setting):
    r = runs[setting]["refused"]
    assert all(rc != 0 for rc in r["rc"]) and len(r["rc"]) == 3
    assert r["differ"] == []


@pytest.mark.parametrize("setting", SETTINGS)
def test_mixed_queue_with_candidate_projection(runs, setting):
    """batch, small (8 problems, on the context's stream), batch, then a candidate projection that reads a result of the last
    launch on the device: results and projections equal the blocking sequence"""
    r = runs[setting]["mixed"]
    assert r["small_build"]["n_desc"] < runs[setting]["num_cus"] or r["small_build"]["cluster_g"] >= 2, r["small_build"]
    assert r["blocking_c_is_alone_c"] and r["differ"] == [] and r["projection_equal"]
    assert 50 < r["visible"] < r["points"] - 50


@pytest.mark.parametrize("setting", SETTINGS)
def test_fetch_of_the_last_launch_then_a_new_queue(runs, setting):
    r = runs[setting]["fetch_last"]
    assert r["last_differ"] == [] and r["differ"] == [] and r["nothing_left"]


def test_both_settings_deliver_the_same_bits(runs):
    a, b = runs["1"], runs["0"]
    assert a["alone_sha"] == b["alone_sha"]
    for name in ("five", "grow", "garbage", "refused", "mixed", "fetch_last"):
        assert a[name]["sha"] == b[name]["sha"], name


def test_the_side_path_ran_and_the_switch_turns_it_off(runs):
    """the counter of libsvo_hip_testhooks.so: every batch launch queued behind an alignment launch that nobody has waited for takes
    the side path -- not the first of a queue, not the small launch; a refused call in between queues nothing and changes nothing --
    and none does with SVOH_ALIGN_SIDE_COPIES=0"""
    on, off = runs["1"], runs["0"]
    assert on["five"]["side"] == 4 and on["garbage"]["side"] == 3 and on["refused"]["side"] == [1, 1, 1]
    assert on["mixed"]["side"] == 1            # A first of its queue, the small launch in-stream, C behind it
    assert on["fetch_last"]["side"] == [2, 1] and on["destroy"]["side"] == 2
    for name in ("five", "grow", "garbage", "mixed", "destroy"):
        assert off[name]["side"] == 0, name
    assert off["refused"]["side"] == [0, 0, 0] and off["fetch_last"]["side"] == [0, 0]
