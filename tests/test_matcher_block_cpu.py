"""The matcher's staging blocks as csrc/svoh_matcher_block.h lays them out (printed by tests/cpp/matcher_block_cpu, which is
built from the header alone) against tests/matcher_block_layout.py, the plain restatement of the layouts the entries used to
build by hand: every column offset and the three marks, for the direct, seed, epipolar, chain and staged forms at the unit
counts where 4-byte and 1-byte columns cross a 64-byte boundary."""
import os
import subprocess

import pytest

import matcher_block_layout as mbl

TOOL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "matcher_block_cpu")


def _cases():
    # built here, as the other tools of tests/cpp are by their tests: a tree whose tests/ holds sources only still runs this
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(TOOL), os.path.basename(TOOL)])
    out = subprocess.check_output([TOOL], text=True)
    cases, cur = [], None
    for line in out.splitlines():
        w = line.split()
        if w[0] == "case":
            cur = dict(layout=w[1], args={k: int(v) for k, v in (kv.split("=") for kv in w[2:])}, cols=[], handed={})
            cases.append(cur)
        elif w[0] == "col":
            cur["cols"].append((w[1], int(w[2])))
        elif w[0] == "handed":
            cur["handed"][w[1]] = int(w[2])
        elif w[0] == "marks":
            cur["marks"] = dict(zip(("in_total", "back_from", "end", "total"), map(int, w[1:])))
        else:
            raise AssertionError(line)
    return cases


def _restated(layout, a):
    if layout == "direct":
        return mbl.direct_batch(a["n"], a["views"], a["view_bytes"], bool(a["cur_idx"]), bool(a["landmark_xyz"]))
    if layout == "seeds":
        return mbl.seed_batch(a["n"], a["views"], a["view_bytes"], bool(a["cur_idx"]), bool(a["px_cur"]))
    if layout == "epipolar":
        return mbl.epipolar_batch(a["n"], a["views"], a["view_bytes"], a["t_bytes"], bool(a["d_inv"]), bool(a["cur_idx"]))
    if layout == "chain":
        return mbl.seed_chain(a["n"], a["views"], a["view_bytes"], a["n_ref"], a["links"], a["max_steps"], bool(a["step_result"]), bool(a["step_success"]))
    if layout == "staged":
        return mbl.matcher_stage(bool(a["seeds"]), a["n"], a["views"], bool(a["outputs"]), bool(a["resident"]), a["view_bytes"])
    raise AssertionError(layout)


@pytest.fixture(scope="module")
def cases():
    return _cases()


def test_every_layout_is_the_restated_one(cases):
    for c in cases:
        want = _restated(c["layout"], c["args"])
        assert c["cols"] == want["cols"], (c["layout"], c["args"])
        assert c["marks"] == {k: want[k] for k in ("in_total", "back_from", "end", "total")}, (c["layout"], c["args"])


def test_the_cases_are_the_ones_asked_for(cases):
    by = {}
    for c in cases:
        by.setdefault(c["layout"], []).append(c["args"])
    assert set(by) == {"direct", "seeds", "epipolar", "chain", "staged"}
    for layout, args in by.items():
        assert {a["n"] for a in args} == {1, 15, 16, 17, 63, 64, 65}, layout
        assert {a["view_bytes"] for a in args} == {mbl.DEV_FRAME_VIEW_BYTES, mbl.DEV_FRAME_VIEW_WIDE_BYTES}, layout
        assert len({tuple(sorted(a.items())) for a in args}) == len(args), layout   # no case twice
    assert {a["views"] for a in by["staged"]} == {2, 5}
    assert {(a["seeds"], a["outputs"], a["resident"]) for a in by["staged"]} == {(s, o, r) for s in (0, 1) for o in (0, 1) for r in (0, 1)}
    assert {(a["cur_idx"], a["landmark_xyz"]) for a in by["direct"]} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {(a["cur_idx"], a["px_cur"]) for a in by["seeds"]} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {(a["cur_idx"], a["d_inv"], a["t_bytes"] > 0) for a in by["epipolar"]} == {(c, d, t) for c in (0, 1) for d in (0, 1) for t in (False, True)}
    assert {(a["links"], a["max_steps"], a["step_result"], a["step_success"]) for a in by["chain"]} == \
        {(l, m, r, s) for l in (0, 4) for m in (0, 2) for r in (0, 1) for s in (0, 1)}


def test_a_staged_block_hands_out_its_pinned_columns_only(cases):
    for c in cases:
        if c["layout"] != "staged":
            continue
        a = c["args"]
        if a["view_bytes"] != mbl.DEV_FRAME_VIEW_BYTES:
            continue
        want = mbl.matcher_stage_handed_out(bool(a["seeds"]), a["n"], a["views"], bool(a["outputs"]), bool(a["resident"]))
        got = {k: v for k, v in c["handed"].items() if k not in ("views", "n_success")}
        assert got == want, a
