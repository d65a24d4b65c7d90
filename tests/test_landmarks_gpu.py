"""Landmark positions after structure steps on scripted keyframe sequences (tests/landmark_cases.py: scenarios a, b, c and g):
tests/cpp/landmarks_tool --device replays a script through the real mirrors and runs optimizeStructure(ctx, bundle, max_n_pts, 5)
on the device; the reading replays the same script with the oracle's Point::optimize on ITS batches, frame by frame of the
bundle, positions carried from step to step.  Which observations a landmark is optimised over is therefore part of what is
compared: one duplicated observation moves a landmark by a hundred times the tolerance (tests/test_landmarks_cpu.py).
Tolerance as in tests/test_point_optimize_gpu.py: 1e-6 absolute, median below 1e-12 (fp64 on both sides).  Landmarks that no
structure step touches -- edgelets, fewer than two observations -- are bit-equal to where they were made; stamps, observations
and everything else in the dump are equal.  The scenes contain no constructed degenerate landmark."""
import os
import subprocess

import numpy as np
import pytest

import landmark_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tool():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "svo_pro_universal_amd", "host"), "libsvo_hip_host.so"])
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "landmarks_tool"])
    return os.path.join(ROOT, "tests", "cpp", "landmarks_tool")


def _oracle_step(orc):
    def solve(b):
        pos, _ = orc.optimize_points([np.array(v) for v in b["views"]], np.array(b["obs_begin"], np.int32), np.array(b["obs_view"], np.int32),
                                     np.array(b["obs_f"]).reshape(-1, 3), np.array(b["pos"]).reshape(-1, 3), n_iter=5)
        return pos
    return solve


@pytest.mark.parametrize("name", ["a_mono_keyframes", "b_stereo_keyframe_step", "c_bootstrap", "g_selection"])
def test_structure_steps_match_the_oracle_on_the_readings_batches(tool, oracle_lib, tmp_path, name):
    text = lc.SCENARIOS[name]()
    want, reading = lc.read_script(text, solver=_oracle_step(oracle_lib))
    script, dump = tmp_path / "script.txt", tmp_path / "dump.txt"
    script.write_text(text)
    r = subprocess.run([tool, str(script), str(dump), "--device"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    got = dump.read_text().splitlines()
    want = want.splitlines()
    assert len(got) == len(want)
    n_states, moved, d_all = 0, 0, []
    for g, w in zip(got, want):
        tg, tw = g.split(), w.split()
        if tw[0] == "state":
            n_states += 1
        if tw[0] != "point" or int(tw[1]) not in reading.touched:
            assert g == w                                   # untouched landmarks included: bit-equal positions
            continue
        assert tg[:2] == tw[:2] and tg[5:] == tw[5:], (g, w)      # id; stamp and observations
        d = np.abs(np.array(tg[2:5], float) - np.array(tw[2:5], float)).max()
        d_all.append(d)
        moved += 1
    d_all = np.array(d_all)
    print("%s: %d states, %d compared positions of %d optimised landmarks, worst %.3g, median %.3g"
          % (name, n_states, moved, len(reading.touched), d_all.max(), np.median(d_all)))
    assert len(reading.touched) >= 10 and d_all.max() < 1e-6 and np.median(d_all) < 1e-12
    # every kind of untouched landmark is there to be compared where the scenario has it
    if name != "c_bootstrap":
        assert any(w.startswith("point ") and int(w.split()[1]) not in reading.touched for w in want)
