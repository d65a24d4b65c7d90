"""A calibration's camera mask through the whole chain: the single-stream harness (tools/svoh_mini_frontend.cpp; the mask
goes with every frame into depth_filter_utils::initializeSeeds' detector, depth_filter.cpp:294, 320) and a lock-step run of
four streams, two with a masked calibration and two without (FrontendLockstep: one uploaded mask per distinct camera, the
round's keyframes through svoh_detect_cells_batch_masked_enqueue).

* no feature a keyframe's detector adds lies on a zero mask pixel -- in the single-stream run and in the masked lock-step streams;
* every lock-step stream writes the trajectory, the counters and the keyframe features of ITS OWN single-stream run, byte for byte
  (the engine's standing contract, tests/test_mini_frontend_gpu.py);
* the unmasked streams are byte-identical to what they give in a lock-step run without any masked neighbour."""
import os
import subprocess

import numpy as np
import pytest

from test_io_cpu import write_png
from test_mini_frontend_gpu import COUNTER_COLS, make_dataset

pytestmark = pytest.mark.gpu

N_FRAMES = 17         # keyframes at frames 0, 8 and 16
BAND = (170, 290)     # rows of the image the mask zeroes (a band across the whole width)
# (start, masked): every stream its own stretch of the sequence, so that a stream handed another's mask or cells shows
STREAMS = ((0, True), (3, False), (6, True), (9, False))
FILES = ("trajectory.txt", "frontend.csv", "keyframes.csv")


def read_run(d):
    traj = open(str(d / "trajectory.txt")).read()
    counters = np.loadtxt(str(d / "frontend.csv"), delimiter=",", skiprows=1)[:, COUNTER_COLS].copy()
    kf_text = open(str(d / "keyframes.csv")).read()
    kf = np.loadtxt(str(d / "keyframes.csv"), delimiter=",", ndmin=2)
    return traj, counters, kf_text, kf


def in_band(kf):
    y = kf[:, 2].astype(int)
    return (y >= BAND[0]) & (y < BAND[1])


def clean(out_dir):
    for d in [out_dir] + [out_dir / ("stream%d" % k) for k in range(1, 8)]:
        for name in FILES:
            if (d / name).exists():
                (d / name).unlink()


def write_spec(tmp_path, poses, name, masked_calib):
    lines = []
    for start, masked in STREAMS:
        line = "start=%d step=1 frames=%d every=1 phase=0 kf_every=8 min_tracked=60 T0=%s" % (
            start, N_FRAMES, ",".join("%.17g" % v for v in poses[start].inverse().as7()))
        if masked and masked_calib:
            line += " calib=%s" % masked_calib
        lines.append(line)
    spec = tmp_path / name
    spec.write_text("\n".join(lines) + "\n")
    return spec


def test_masks_from_the_calibration_through_the_harness_and_the_lockstep_engine(tmp_path):
    cmd, out_dir, poses, stamps, n_frames = make_dataset(tmp_path)
    mask = np.full((480, 752), 255, np.uint8)
    mask[BAND[0]:BAND[1], :] = 0
    write_png(str(tmp_path / "band.png"), mask, chunk=65536)
    plain = (tmp_path / "calib.yaml").read_text()
    assert "    label: cam0\n" in plain
    masked_calib = tmp_path / "calib_masked.yaml"
    masked_calib.write_text(plain.replace("    label: cam0\n", "    label: cam0\n    mask: band.png\n"))
    env = dict(os.environ, SVOH_MINI_DUMP_KEYFRAMES="1")

    # ---- the single-stream harness: the mask comes with the calibration, no new argument
    clean(out_dir)
    c = list(cmd)
    c[2] = str(masked_calib)
    r = subprocess.run(c + [str(N_FRAMES), "8", "1"], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    alone = read_run(out_dir)
    print("single stream with the mask: %d new keyframe features" % len(alone[3]))
    assert len(set(alone[3][:, 0])) >= 3, "fewer than three keyframes"
    assert len(alone[3]) > 100 and not in_band(alone[3]).any()
    assert mask[alone[3][:, 2].astype(int), alone[3][:, 1].astype(int)].all()

    # ---- four streams, two masked: each alone through the single-stream chain ...
    spec = write_spec(tmp_path, poses, "mixed.spec", masked_calib)
    singles = []
    for i in range(len(STREAMS)):
        clean(out_dir)
        r = subprocess.run(cmd + [str(N_FRAMES), "8", "1"], capture_output=True, text=True, env=dict(env, SVOH_MINI_SPEC=str(spec), SVOH_MINI_SPEC_LINE=str(i)))
        assert r.returncode == 0, r.stdout + r.stderr
        singles.append(read_run(out_dir))
        # (an unmasked stream does put features into the band: without that the case would test nothing)
        assert (int(in_band(singles[i][3]).sum()) >= 20) != STREAMS[i][1] and in_band(singles[i][3]).any() != STREAMS[i][1], "stream %d alone" % i
    assert len({s[0] for s in singles}) == len(STREAMS)

    # ---- ... and together in lock step; then all four without a mask
    def lockstep(spec_file, n_workers):
        clean(out_dir)
        r = subprocess.run(cmd + [str(N_FRAMES), "8", str(len(STREAMS)), "lockstep", str(n_workers), "1"], capture_output=True, text=True, env=dict(env, SVOH_MINI_SPEC=str(spec_file)))
        assert r.returncode == 0, r.stdout + r.stderr
        return [read_run(out_dir if k == 0 else out_dir / ("stream%d" % k)) for k in range(len(STREAMS))]

    for n_workers in (2,):
        together = lockstep(spec, n_workers)
        for k, (start, masked) in enumerate(STREAMS):
            traj, counters, kf_text, kf = together[k]
            if masked:
                assert len(kf) > 100 and not in_band(kf).any(), "stream %d: a feature on the mask" % k
            assert traj == singles[k][0], "trajectory of stream %d (%d workers)" % (k, n_workers)
            assert np.array_equal(counters, singles[k][1]), "counters of stream %d (%d workers)" % (k, n_workers)
            assert kf_text == singles[k][2], "keyframe features of stream %d (%d workers)" % (k, n_workers)
    unmasked = lockstep(write_spec(tmp_path, poses, "unmasked.spec", None), 1)
    for k, (start, masked) in enumerate(STREAMS):
        same = unmasked[k][0] == together[k][0] and np.array_equal(unmasked[k][1], together[k][1]) and unmasked[k][2] == together[k][2]
        assert same != masked, "stream %d against the run without masks" % k
