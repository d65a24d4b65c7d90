"""Launch lanes of the alignment batch (csrc/svoh_internal.h): a launch of the batch build queued right behind another one that
nobody has waited for runs on a second stream, with a feature workspace of its own, beside the tail of the launch before it.
Nothing a caller sees may change: every scenario of tests/align_overlap_child.py compares bits with the same problems run alone
through svoh_sparse_align_batch, and the sets run alone are held against the oracle.

The child runs in a fresh process per setting (the knobs are read when a context is made; the second lane and both workspaces
start from nothing): SVOH_ALIGN_OVERLAP=1 with SVOH_ALIGN_SIDE_COPIES=1 and =0, and SVOH_ALIGN_OVERLAP=0, the single lane, whose
results are the reference of the other two.  320x240 images, levels 2..0, 4x4 patches, 12..64 features per problem,
num_cus + 17 problems in the smallest set: the smallest launch that takes the batch build and gives workgroups a second problem.

The fixture stops at the first child that does not end with status 0; every step inside a child has a time limit of its own."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SETTINGS = (("1", "1"), ("1", "0"), ("0", "1"))          # (SVOH_ALIGN_OVERLAP, SVOH_ALIGN_SIDE_COPIES)
OVERLAPPED = [s for s in SETTINGS if s[0] == "1"]
IDS = ["overlap%s_side%s" % s for s in SETTINGS]
QUEUES = ("ABC", "ACD", "BD", "AB", "CD", "AD")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    out = {}
    for setting in SETTINGS:
        path = str(tmp_path_factory.mktemp("overlap") / ("out_%s_%s.json" % setting))
        env = dict(os.environ)
        env["SVOH_ALIGN_OVERLAP"], env["SVOH_ALIGN_SIDE_COPIES"] = setting
        p = subprocess.run([sys.executable, "-s", os.path.join(HERE, "align_overlap_child.py"), path], env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        text = p.stdout.decode(errors="replace")
        assert p.returncode == 0 and "align_overlap_child: done" in text, "child %r ended with %r:\n%s" % (setting, p.returncode, text[-4000:])
        out[setting] = json.load(open(path))
    return out


@pytest.mark.parametrize("setting", SETTINGS, ids=IDS)
def test_premises(runs, setting):
    """the sets run alone take the batch build on lane 0, agree with the oracle, and have the shapes of the module's docstring"""
    r = runs[setting]
    assert (r["overlap"], r["side"]) == setting
    assert r["n"]["A"] == r["num_cus"] + 17 and r["n"]["A"] < r["n"]["B"] == r["n"]["C"] < r["n"]["D"]
    assert r["features"]["A"] < r["features"]["B"] < r["features"]["D"] and r["features"]["A"] < r["features"]["C"]
    for k in "ABCD":
        b = r["alone_builds"][k]
        assert b["nt"] == 256 and b["latency"] is False and b["cluster_g"] == 0 and b["rows"] == 1 and b["n_desc"] == r["n"][k], b
        assert b["lane"] == 0
        o = r["oracle"][k]
        assert o["oracle_self"] == [], (k, o)          # scenes the oracle cannot judge: UNJUDGED_SCENE_SEEDS of the child
        assert o["bad"] == [] and o["worst_pose"] < 1e-8 and o["tracked"] > 10 * r["n"][k], (k, o)
    assert r["lanes"] == (2 if setting[0] == "1" else 1)


@pytest.mark.parametrize("setting", SETTINGS, ids=IDS)
def test_four_queued_launches_equal_launches_run_alone(runs, setting):
    """A B C D back to back, one fetch_all: every result equals, byte for byte, the set run alone"""
    r = runs[setting]["four"]
    assert r["differ"] == []
    assert r["lanes"] == ([0, 1, 0, 1] if setting[0] == "1" else [0, 0, 0, 0]) and r["lane1"] == (2 if setting[0] == "1" else 0)


@pytest.mark.parametrize("setting", SETTINGS, ids=IDS)
def test_fetch_after_every_second_enqueue_while_the_workspaces_grow(runs, setting):
    """on a new context: A B C (B waits for A, as the first launch into the second descriptor block always has; C takes lane 1),
    A C D (D, on lane 0, outgrows the first workspace while C runs on lane 1), B D (D outgrows the second workspace while B runs on
    lane 0), then three pairs with a launch pending on each lane.  A launch that finds its workspace too small while the other lane
    is busy waits for both lanes and is the first of a new queue."""
    r = runs[setting]["growth"]
    assert all(r["differ"][q] == [] for q in QUEUES), r["differ"]
    if setting[0] == "1":
        assert r["lanes"][:8] == [0, 0, 1, 0, 1, 0, 0, 0] and r["lanes"][8:] == [0, 1] * 3 and r["lane1"] == 5, r
    else:
        assert not any(r["lanes"]) and r["lane1"] == 0


@pytest.mark.parametrize("setting", SETTINGS, ids=IDS)
def test_blocking_entry_on_the_context_stream_joins_both_lanes(runs, setting):
    r = runs[setting]["join"]
    assert r["differ"] == [] and r["pyramid_equal"] and r["error"] == "no error", r
    assert r["lanes"] == ([0, 1] if setting[0] == "1" else [0, 0])


@pytest.mark.parametrize("setting", SETTINGS, ids=IDS)
def test_cluster_small_and_evaluation_launches_stay_on_lane_0(runs, setting):
    """A B cluster small C D evaluation A B: results unchanged; the cluster launch, the 8-problem launch, the batch launch behind them
    (the first of a new queue) and the evaluation report lane 0"""
    r = runs[setting]["lane0"]
    assert r["big_build"]["cluster_g"] >= 2 and r["small_build"]["n_desc"] == 8, r
    assert r["differ"] == [] and r["eval_equal"]
    if setting[0] == "1":
        assert r["lanes"] == [0, 1, 0, 0, 0, 1, 0, 0, 1] and r["lane1"] == 3, r
    else:
        assert not any(r["lanes"]) and r["lane1"] == 0


@pytest.mark.parametrize("setting", SETTINGS, ids=IDS)
def test_context_destroyed_with_a_launch_pending_on_each_lane(runs, setting):
    """(the child ended with status 0: the fixture) and a second context in the same process computes set A as the first one did"""
    r = runs[setting]
    assert r["destroy"]["lanes"] == ([0, 1] if setting[0] == "1" else [0, 0])
    assert r["second_context"]["differ"] == []


def test_the_switch_off_is_one_lane_with_the_same_bits(runs):
    off = runs[("0", "1")]
    assert off["lanes"] == 1
    for setting in OVERLAPPED:
        on = runs[setting]
        assert on["alone_sha"] == off["alone_sha"]
        for name in ("four", "growth", "join", "lane0", "second_context"):
            assert on[name]["sha"] == off[name]["sha"], (setting, name)
