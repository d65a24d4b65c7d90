"""The landmark bookkeeping of the host mirrors against an independent reading of the reference (tests/landmark_cases.py):
which observations a landmark holds decides what the structure kernel is given, and nothing else in the suite looks at it
from outside.  tests/cpp/landmarks_tool replays each scenario's script through the real mirrors without a device call; its
dump -- points with their live observations, frames, liveness, every gathered structure batch -- equals the reading's
exactly (integers and copied doubles, no tolerance).  The same under the address and undefined-behaviour sanitizers.

On the host code before Point::addObservation existed (bare push_back at all seven sites, the seed reference cleared in
one arm only) scenarios b, c, e and f fail, a, d and g pass: b and c by duplicated observations, e by a seed reference
that keeps the old keyframe alive, f by the missing refusal.

Discrimination (test_duplicates_move_the_landmarks; oracle only, 5 iterations): the structure steps of scenarios b and
c with the duplicates put back -- as `Reading(dedupe=False)` makes them, which is what the mirrors did -- against the same
steps without.  Measured, over the landmarks that received a duplicate and have at least two observations:

    scenario                  landmarks   moved > 1e-4   minimum     median      maximum
    b_stereo_keyframe_step    82          100 %          1.35e-4 m   1.02e-3 m   6.50e-2 m
    c_bootstrap               28          100 %          7.98e-4 m   3.68e-2 m   3.70e-1 m

1e-4 is a hundred times the tolerance of tests/test_landmarks_gpu.py, so that test fails on a duplicate.  (A landmark whose
observations are ALL doubled does not move at all -- the normal equations are the same ones times two -- which is why
scenario c takes its structure steps after a third view.)
"""
import os
import subprocess

import numpy as np
import pytest

import landmark_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:allocator_may_return_null=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


@pytest.fixture(scope="module")
def cases():
    """name -> (script, the reading's dump, the Reading): made once, read by every test."""
    out = {}
    for name, make in lc.SCENARIOS.items():
        text = make()
        dump, reading = lc.read_script(text)
        out[name] = (text, dump, reading)
    return out


@pytest.fixture(scope="module")
def tool():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "svo_pro_universal_amd", "host"), "libsvo_hip_host.so"])
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "landmarks_tool"])
    return os.path.join(ROOT, "tests", "cpp", "landmarks_tool")


@pytest.fixture(scope="module")
def tool_asan():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "svo_pro_universal_amd", "host"), "libsvo_hip_host.so"])
    subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(ROOT, "tests", "san"), "landmarks_tool_asan"])
    return os.path.join(ROOT, "tests", "san", "landmarks_tool_asan")


def replay(exe, text, tmp_path, env=None):
    script, dump = tmp_path / "script.txt", tmp_path / "dump.txt"
    script.write_text(text)
    r = subprocess.run([exe, str(script), str(dump)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    return dump.read_text(), r.stderr


@pytest.mark.parametrize("name", sorted(lc.SCENARIOS))
def test_the_mirrors_keep_the_readings_books(cases, tool, tmp_path, name):
    text, want, reading = cases[name]
    got, _ = replay(tool, text, tmp_path)
    lc.assert_same_dump(got, want, reading.batches)


@pytest.mark.parametrize("name", sorted(lc.SCENARIOS))
def test_the_same_under_address_and_ub_sanitizer(cases, tool_asan, tmp_path, name):
    text, want, reading = cases[name]
    got, err = replay(tool_asan, text, tmp_path, env=SAN_ENV)
    assert "ERROR: AddressSanitizer" not in err and "ERROR: LeakSanitizer" not in err and "runtime error:" not in err, err[-6000:]
    lc.assert_same_dump(got, want, reading.batches)


def test_the_scenarios_hold_what_they_are_for(cases):
    """The scripts are made from random numbers: that each still contains the situation it is named after."""
    def lines(name, word):
        return [l.split() for l in cases[name][1].splitlines() if l.split()[0] == word]

    def final_points(name):
        dump = cases[name][1]
        rows = [l.split() for l in dump[dump.rindex("state\n"):].splitlines() if l.startswith("point ")]
        return [(int(p[1]), [int(f) for f in p[7::2]]) for p in rows]      # (id, the frames of its live observations)

    # a: every seed type upgraded, edgelets among them; a landmark that loses its second observation with the first keyframe
    assert {int(t) for l in lines("a_mono_keyframes", "types") for t in l[1:]} >= {lc.capi.FT_CORNER, lc.capi.FT_EDGELET, lc.capi.FT_MAPPOINT}
    assert any(int(l[3]) > 0 for l in lines("a_mono_keyframes", "upgraded"))
    assert {len(fr) for _, fr in final_points("a_mono_keyframes")} >= {1, 2} and "alive 10 0" in cases["a_mono_keyframes"][1]
    # b: successes, failures, the cut-off (the second frame got fewer features than there were successes to be had), and every
    # triangulated point with exactly one observation per frame of the pair after both keyframe steps
    (ok1, failed1, _), (ok2, failed2, _) = [[int(x) for x in l[1:]] for l in lines("b_stereo_keyframe_step", "stereo")]
    assert ok1 == 20 and failed1 > 0 and ok1 + failed1 < 30 and ok2 + failed2 == 6
    tri = [fr for pid, fr in final_points("b_stereo_keyframe_step") if pid < lc.FIRST_UPGRADE_ID]
    assert len(tri) == ok1 + ok2 and all(fr == [22, 23] for fr in tri)
    assert [20, 23, 22] in [fr for _, fr in final_points("b_stereo_keyframe_step")]      # a seed of the old keyframe seen from both frames
    # c: two, then three observations, one per frame
    assert {tuple(fr) for _, fr in final_points("c_bootstrap")} == {(30, 31), (30, 31, 32)}
    # d: one point, three observations
    assert [fr for _, fr in final_points("d_multi_camera_bundle")].count([40, 41, 42]) == 4
    # e: the old keyframe is alive while the scene holds it and gone afterwards
    alive = lines("e_stale_seed_reference", "alive")
    assert alive[0][1:5] == ["50", "1", "51", "1"] and alive[-1][1:5] == ["50", "0", "51", "1"]
    # f: refused
    assert lines("f_index_conflict", "throw") == [["throw", "upgrade", "71"]]
    # g: 0 does nothing; 4 is below the candidates of both frames; 10 is above those of the first frame, which hands its count on
    steps = [[int(x) for x in l[1:]] for l in lines("g_selection", "step")]
    assert cases["g_selection"][1].splitlines()[0] == "structure 0"
    assert [s[:4] for s in steps] == [[61, 4, 4, 8], [62, 4, 4, 7], [61, 10, 8, 8], [62, 8, 7, 7], [62, -1, -1, 7], [61, -1, -1, 8]]


def test_the_refusal_names_the_frame_and_both_features(cases, tool, tmp_path):
    _, err = replay(tool, cases["f_index_conflict"][0], tmp_path)
    assert "frame 71" in err and "feature 1 " in err and "at 3" in err, err


def _arrays(b):
    return ([np.array(v) for v in b["views"]], np.array(b["obs_begin"], np.int32), np.array(b["obs_view"], np.int32),
            np.array(b["obs_f"]).reshape(-1, 3), np.array(b["pos"]).reshape(-1, 3))


@pytest.mark.parametrize("name", ["b_stereo_keyframe_step", "c_bootstrap"])
def test_duplicates_move_the_landmarks(cases, oracle_lib, name):
    """What makes tests/test_landmarks_gpu.py able to fail: see the module's docstring for the measured figures."""
    text, _, clean = cases[name]
    _, dup = lc.read_script(text, dedupe=False)
    moved = []
    for bc, bd in zip(clean.batches, dup.batches):
        assert bc["pts"] == bd["pts"] and bc["pos"] == bd["pos"] and bc["pts"]
        pc, _ = oracle_lib.optimize_points(*_arrays(bc), n_iter=5)
        pd, _ = oracle_lib.optimize_points(*_arrays(bd), n_iter=5)
        nc, nd = np.diff(bc["obs_begin"]), np.diff(bd["obs_begin"])
        assert (nd >= nc).all()
        sel = (nd > nc) & (nc >= 2)
        moved += list(np.linalg.norm(pc - pd, axis=1)[sel])
    moved = np.array(moved)
    print("%s: %d landmarks with a duplicate, %.1f %% moved by more than 1e-4, minimum %.3g, median %.3g, maximum %.3g"
          % (name, len(moved), 100.0 * np.mean(moved > 1e-4), moved.min(), np.median(moved), moved.max()))
    assert len(moved) >= 20 and np.mean(moved > 1e-4) >= 0.9
