"""The alignment's staged block and feature workspace as csrc/svoh_align_block.h lays them out (printed by
tests/cpp/align_block_cpu, which is built from the header alone) against tests/align_block_layout.py, the plain restatement of
what the launch code used to compute by hand: the descriptor area, the control words, every camera's columns, the units and the
job table of pos_seed_unit cameras, the pointers of every share, and the workspace -- at the feature counts where 65n and 4n
cross 64-byte boundaries and the descriptor counts where the control words move across a 256-byte boundary."""
import os
import subprocess

import pytest

import align_block_layout as abl

TOOL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "align_block_cpu")


def build_tool():
    # built here, as the other tools of tests/cpp are by their tests: a tree whose tests/ holds sources only still runs this
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(TOOL), os.path.basename(TOOL)])
    return TOOL


@pytest.fixture(scope="module")
def cases():
    out = subprocess.check_output([build_tool()], text=True)
    cases, cur = [], None
    for line in out.splitlines():
        w = line.split()
        if w[0] == "case":
            cur = dict(kind=w[1], args={k: int(v) for k, v in (kv.split("=") for kv in w[2:])}, cam=[], units=[], share=[], jobs=None)
            cases.append(cur)
        elif w[0] == "desc":
            cur.update(zip(("cams_off", "ctl_off", "bar_off", "up_base"), map(int, w[1:])))
        elif w[0] in ("cam", "units", "share"):
            cur[w[0]].append(tuple(map(int, w[1:])))
        elif w[0] == "jobs":
            cur["jobs"] = int(w[1])
        elif w[0] == "total":
            cur["reserve"], cur["used"] = int(w[1]), int(w[2])
        elif w[0] == "ws":
            cur.update(zip(("slots", "wpk", "wsel", "wvis", "bytes"), map(int, w[1:])))
        else:
            raise AssertionError(line)
    return cases


def test_every_block_is_the_restated_one(cases):
    n = 0
    for c in cases:
        if c["kind"] != "block":
            continue
        a = c["args"]
        want = abl.block(a["problems"], a["cams"], a["n"], a["shares"], bool(a["units"]))
        got = {k: c[k] for k in want}
        assert got == want, a
        n += 1
    assert n == 8 * 2 * 3 * 2 * 2


def test_the_workspace_is_the_restated_one(cases):
    seen = set()
    for c in cases:
        if c["kind"] != "workspace":
            continue
        want = abl.workspace(c["args"]["feat"])
        assert {k: c[k] for k in want} == want, c["args"]
        seen.add(c["args"]["feat"])
    assert seen >= {1, 340, 341}


def test_the_cases_are_the_ones_asked_for(cases):
    args = [c["args"] for c in cases if c["kind"] == "block"]
    assert {a["n"] for a in args} == {0, 1, 15, 16, 17, 63, 64, 65}
    assert {a["cams"] for a in args} == {1, 2}
    assert {a["shares"] for a in args} == {1, 3}
    assert {a["units"] for a in args} == {0, 1}
    assert {a["problems"] * a["shares"] for a in args} >= {1, 3, 7}            # descriptors
    assert len({tuple(sorted(a.items())) for a in args}) == len(args)         # no case twice
    # the control words do move across a 256-byte boundary with the descriptor count, and the rounding of 65n and 4n is exercised
    one_cam = {a["problems"]: c["ctl_off"] for c in cases if c["kind"] == "block" for a in [c["args"]] if a["cams"] == 1 and a["shares"] == 1}
    assert len(set(one_cam.values())) == 3 and all(v % 256 == 0 for v in one_cam.values())
    strides = {c["args"]["n"]: c["cam"][0][5] for c in cases if c["kind"] == "block" and c["cam"]}
    assert strides[63] == 4096 and strides[64] == 4160 and strides[1] == 128 and strides[15] == 1024 and strides[16] == 1088


def test_shares_tile_a_camera(cases):
    for c in cases:
        if c["kind"] != "block" or not c["share"]:
            continue
        a = c["args"]
        by_cam = {}
        for (k, s, n, px, f, pos, flags) in c["share"]:
            by_cam.setdefault(k, []).append((s, n, px, flags))
        for k, shares in by_cam.items():
            assert [s for s, *_ in shares] == list(range(a["shares"]))
            assert sum(n for _, n, *_ in shares) == a["n"]
            for (s0, n0, px0, fl0), (s1, n1, px1, fl1) in zip(shares, shares[1:]):
                assert px1 == px0 + 16 * n0 and fl1 == fl0 + n0
