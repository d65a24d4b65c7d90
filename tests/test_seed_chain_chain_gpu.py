"""The frame handler's step at a new keyframe with update_seeds_with_old_keyframes (frame_handler_mono.cpp:218-225: the fresh seeds are
updated with the last frame and the overlap keyframes) in the per-frame chains: tools/svoh_mini_frontend.cpp with
SVOH_MINI_SEEDS_OLD_KEYFRAMES, alone and in lock step.  The one-call form (DepthFilterHip::updateSeedsWithFrames /
svoh_update_seeds_chain) against one updateSeeds call per frame, the pipelined flow against the blocking one, every lock-step stream
against its own single-stream run: byte for byte."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_mini_frontend_gpu import COUNTER_COLS, ROOT, make_dataset

pytestmark = pytest.mark.gpu
N_FRAMES, KF_EVERY = 17, 4
SWITCH = "SVOH_MINI_SEEDS_OLD_KEYFRAMES"


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """The rendered sequence: made once for the tests of this file (they read it, and write into its out directory in turn)."""
    return make_dataset(tmp_path_factory.mktemp("seed_chain"))


def run_tool(cmd, out_dir, args, env, n_streams=1):
    dirs = [out_dir] + [out_dir / ("stream%d" % k) for k in range(1, n_streams)]
    for d in [out_dir] + [out_dir / ("stream%d" % k) for k in range(1, 8)]:
        for name in ("trajectory.txt", "frontend.csv", "seed_chain.csv"):
            if (d / name).exists():
                (d / name).unlink()
    r = subprocess.run(cmd + args, capture_output=True, text=True, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stdout + r.stderr
    out = []
    for d in dirs:
        chain = open(str(d / "seed_chain.csv")).read() if (d / "seed_chain.csv").exists() else None
        out.append((open(str(d / "trajectory.txt")).read(), np.loadtxt(str(d / "frontend.csv"), delimiter=",", skiprows=1)[:, COUNTER_COLS].copy(), chain))
    return out


def same_run(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] is not None and a[2] == b[2]


def test_single_stream_one_call_equals_one_call_per_frame(dataset):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import ate
    cmd, out_dir, poses, stamps, _ = dataset
    args = [str(N_FRAMES), str(KF_EVERY), "1"]
    off = run_tool(cmd, out_dir, args, {})[0]
    assert off[2] is None                                    # unset: no file (the tool as it was)
    one = run_tool(cmd, out_dir, args, {SWITCH: "1"})[0]
    seq = run_tool(cmd, out_dir, args, {SWITCH: "seq"})[0]
    blocking = run_tool(cmd, out_dir, args, {SWITCH: "1", "SVOH_MINI_SYNC": "1"})[0]
    assert same_run(one, seq), "the chain call differs from one updateSeeds call per frame"
    assert same_run(one, blocking), "the pipelined flow differs from the blocking flow"
    assert one[0] != off[0], "the switch changed nothing: the case tests nothing"
    rows = np.loadtxt(one[2].splitlines(), delimiter=",", skiprows=1, ndmin=2)
    kf_frames = one[1][one[1][:, 1] == 1, 0]
    assert list(rows[:, 0]) == list(kf_frames[1:]) and len(rows) >= 3          # every keyframe after the first
    assert np.all(rows[:, 1] >= 1) and np.all(rows[:, 3] > 0)
    assert rows[:, 1].max() >= 3                                               # last frame and several keyframes
    # a parameter file that switches the key off: the tool as without the switch
    params = cmd[3]
    text = open(params).read()
    try:
        open(params, "w").write(text + "update_seeds_with_old_keyframes: False\n")
        no = run_tool(cmd, out_dir, args, {SWITCH: "1"})[0]
    finally:
        open(params, "w").write(text)
    assert no[2] is None and no[0] == off[0] and np.array_equal(no[1], off[1])
    (out_dir / "trajectory_one.txt").write_text(one[0])
    est = ate.load_tum(str(out_dir / "trajectory_one.txt"))
    gt = np.array([[stamps[k] * 1e-9] + list(T.t) + [T.q[1], T.q[2], T.q[3], T.q[0]] for k, T in enumerate(poses[:N_FRAMES])])
    res = ate.ate(est, gt, with_scale=True, max_dt=1e-3)
    path_len = float(np.linalg.norm(np.diff(gt[:, 1:4], axis=0), axis=1).sum())
    print("ATE rmse %.4f m over a %.3f m path with the switch on" % (res["rmse"], path_len))
    assert res["n"] == N_FRAMES
    assert res["rmse"] < 0.03 * path_len + 0.003


def test_lockstep_streams_reproduce_their_single_stream_runs(dataset, tmp_path):
    cmd, out_dir, poses, stamps, _ = dataset
    # three streams; one makes a keyframe every third frame, so the chains of a round differ in length and not every round's
    # keyframes are everybody's
    spec = tmp_path / "streams.spec"
    spec.write_text("kf_every=4\nkf_every=3\nkf_every=4 start=2 frames=15 T0=%s\n" % ",".join("%.17g" % v for v in poses[2].inverse().as7()))
    args = [str(N_FRAMES), str(KF_EVERY)]
    env = {SWITCH: "1", "SVOH_MINI_SPEC": str(spec)}
    singles = [run_tool(cmd, out_dir, args + ["1"], dict(env, SVOH_MINI_SPEC_LINE=str(i)))[0] for i in range(3)]
    assert all(s[2] is not None and len(s[2].splitlines()) >= 4 for s in singles)
    assert singles[0][2] != singles[1][2] and singles[0][0] != singles[2][0]
    for n_workers in ("1", "2"):
        streams = run_tool(cmd, out_dir, args + ["3", "lockstep", n_workers, "1"], env, n_streams=3)
        for k in range(3):
            assert streams[k][0] == singles[k][0], "trajectory of stream %d (workers %s)" % (k, n_workers)
            assert np.array_equal(streams[k][1], singles[k][1]), "counters of stream %d (workers %s)" % (k, n_workers)
            assert streams[k][2] == singles[k][2], "seed_chain.csv of stream %d (workers %s)" % (k, n_workers)
