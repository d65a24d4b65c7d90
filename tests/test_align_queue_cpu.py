"""The alignment's launch queue without a device: sequences of calls replayed through place_block / place_launch / commit_launch
(csrc/svoh_align_block.h) by tests/cpp/align_block_cpu, in the order enqueue_align carries them out.  The lane sequences are the
ones tests/test_align_overlap_gpu.py pins on the device; the rest is what the comments of the launch code promise.

What is held here is the header: lanes, slots, the side path, overlap, the wait for an event before a pinned block is written again
and the slot a failed call leaves behind all come out of place_block / place_launch / commit_launch.  WHEN a block, a result queue
or a new stream makes the launch code drain first (the "!" of an operation, the first launch of the batch kind) is decided in
sparse_align.hip (take_blocks, side_setup, lane_setup) with the header's align_busy; the tool restates that glue, so the cases that
turn on it ("the first launch into the second descriptor block", "makes the copy stream behind everything queued") show what the
header does with such a drain and rest on tests/test_align_overlap_gpu.py for the drain itself."""
import subprocess

import pytest

from test_align_block_cpu import build_tool

MB = 1 << 20


@pytest.fixture(scope="module")
def tool():
    return build_tool()


def replay(tool, overlap, side, ops):
    out = subprocess.check_output([tool, "queue", overlap, side] + ops.split(), text=True)
    rows = []
    for line in out.splitlines():
        w = line.split()
        row = {"what": w[0]}
        for kv in w[1:]:
            k, v = kv.split("=")
            row[k] = int(v) if v.lstrip("-").isdigit() else v
        rows.append(row)
    return rows[:-1], rows[-1]


def lanes(rows):
    return [r["lane"] for r in rows if r["what"] == "launch"]


def test_four_batch_launches_back_to_back(tool):
    rows, end = replay(tool, "u", "u", "b100 b100 b100 b100")
    assert lanes(rows) == [0, 1, 0, 1] and end["lane1_launches"] == 2
    assert [r["overlapped"] for r in rows] == [0, 1, 1, 1]
    rows, end = replay(tool, "1", "u", "b100 b100 b100 b100")
    assert lanes(rows) == [0, 1, 0, 1]
    rows, end = replay(tool, "0", "u", "b100 b100 b100 b100")
    assert lanes(rows) == [0, 0, 0, 0] and end["lane1_launches"] == 0
    assert not any(r["overlapped"] for r in rows)


def test_cluster_small_and_evaluation_launches_stay_on_lane_0(tool):
    # batch batch cluster small batch batch evaluation batch batch
    rows, end = replay(tool, "u", "u", "b100 b100 s s b100 b100 e b100 b100")
    assert lanes(rows) == [0, 1, 0, 0, 0, 1, 0, 0, 1] and end["lane1_launches"] == 3
    rows, end = replay(tool, "0", "u", "b100 b100 s s b100 b100 e b100 b100")
    assert not any(lanes(rows)) and end["lane1_launches"] == 0


def test_other_work_on_the_stream_ends_the_queue(tool):
    rows, _ = replay(tool, "u", "u", "b100 b100 j b100 b100")
    assert lanes(rows) == [0, 1, 0, 1]
    assert [r["overlapped"] for r in rows] == [0, 1, 0, 1]


def test_the_first_launch_into_the_second_descriptor_block_waits_for_the_first(tool):
    # a new context: the second launch's device block does not exist yet and must be made while the first is in flight
    rows, _ = replay(tool, "u", "u", "b100 b100! b100")
    assert [r["drained"] for r in rows] == [0, 1, 0]
    assert lanes(rows) == [0, 0, 1]
    assert [r["slot"] for r in rows] == [1, 0, 1]


def test_a_workspace_that_must_grow_while_the_other_lane_is_busy_starts_a_new_queue(tool):
    # tests/test_align_overlap_gpu.py's growth scenario: A B C | A C D | B D | A B | C D | A D with A <= B < C < D
    a, b, c, d = "b100", "b200", "b300", "b400"
    ops = f"{a} {b}! {c} f {a} {c} {d} f {b} {d} f {a} {b} f {c} {d} f {a} {d} f"
    rows, end = replay(tool, "u", "u", ops)
    assert lanes(rows) == [0, 0, 1, 0, 1, 0, 0, 0] + [0, 1] * 3 and end["lane1_launches"] == 5
    # D of the second queue (headed for lane 0) and D of the third (headed for lane 1) drain first
    assert [r["drained"] for r in rows] == [0, 1, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0]
    # before lane 1 has run anything a workspace grows without a wait
    rows, _ = replay(tool, "0", "u", f"{a} {d}")
    assert [r["drained"] for r in rows] == [0, 0]


def test_side_path_from_the_second_queued_launch_on_and_above_a_megabyte(tool):
    big, small = f"b100:{MB + 1}", f"b100:{MB}"
    rows, end = replay(tool, "u", "u", f"{big} {big} {big} f {big} {big}")
    assert [r["side"] for r in rows] == [0, 1, 1, 0, 1] and end["side_launches"] == 3
    rows, end = replay(tool, "u", "u", f"{small} {small} {small}")
    assert [r["side"] for r in rows] == [0, 0, 0] and end["side_launches"] == 0
    rows, _ = replay(tool, "u", "1", f"{small} {small} {small}")        # the knob says every one
    assert [r["side"] for r in rows] == [0, 1, 1]
    rows, _ = replay(tool, "u", "0", f"{big} {big} {big}")              # ... or none
    assert [r["side"] for r in rows] == [0, 0, 0]
    # launches of another kind never; the context's first launch of the batch kind makes the copy stream behind everything queued
    rows, _ = replay(tool, "u", "1", "s s b100:5 b100:5 s")
    assert [r["side"] for r in rows] == [0, 0, 0, 1, 0] and [r["drained"] for r in rows] == [0, 0, 1, 0, 0]
    # the lanes are the same with and without side copies
    assert lanes(replay(tool, "u", "1", "b1 b1 b1 b1")[0]) == [0, 1, 0, 1]


def test_the_pinned_blocks_alternate_and_the_third_launch_waits_for_an_event(tool):
    for side in "01":
        rows, end = replay(tool, "u", side, "b100 b100 b100 b100 b100")
        assert [r["slot"] for r in rows] == [1, 0, 1, 0, 1] and end["slot"] == 1
        assert [r["wait"] for r in rows] == ["free", "free", "event", "event", "event"]
        assert not any(r["drained"] for r in rows)
    # the host has waited in between: nothing to wait for
    rows, _ = replay(tool, "u", "u", "s f s f s f")
    assert [r["wait"] for r in rows] == ["free"] * 3 and [r["slot"] for r in rows] == [1, 0, 1]


def test_a_call_that_fails_before_its_upload_does_not_take_a_slot(tool):
    rows, end = replay(tool, "u", "u", "b100 x b100 x x b100")
    assert [(r["what"], r["slot"]) for r in rows] == [("launch", 1), ("failed", 0), ("launch", 0), ("failed", 1), ("failed", 1), ("launch", 1)]
    assert lanes(rows) == [0, 1, 0] and end["slot"] == 1
    # ... and waits for what the launch that does take it would have waited for
    assert [r["wait"] for r in rows] == ["free", "free", "free", "event", "event", "event"]
