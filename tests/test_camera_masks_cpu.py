"""The calibration loader's camera masks (svo_hip::io::loadCameraRig through tests/cpp_masks/mask_tool): the `mask:` key at
both places where the reference accepts it -- a camera node of a rig (ncamera.cpp:44-48) and the top level of a
single-camera document (camera_geometry_base.cpp:33-37) --, the path relative to the calibration file's directory, a
missing file and a mask of the wrong size as errors (camera_geometry_base.cpp:62-76), the committed calibrations as before,
and the omni file refused for its camera type, not for its mask."""
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALIB = os.path.join(ROOT, "tests", "golden", "param", "calib")
TOOL = os.path.join(ROOT, "tests", "cpp_masks", "mask_tool")
TEST_IO = os.path.join(ROOT, "tests", "cpp", "test_io")
W, H = 48, 32

CAMERA = ("{i}distortion:\n{i}  parameters:\n{i}    data: [-0.28, 0.07, 0.0002, 0.00002]\n{i}  type: radial-tangential\n"
          "{i}image_height: %d\n{i}image_width: %d\n{i}intrinsics:\n{i}  data: [30.0, 30.0, 24.0, 16.0]\n{i}label: {label}\n{i}type: pinhole\n" % (H, W))


@pytest.fixture(scope="module")
def tools():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp_masks")])
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "test_io"])


def write_png(path, img):
    """An 8-bit grey PNG, non-interlaced, filter 0 on every row."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    raw = b"".join(b"\x00" + img[y].tobytes() for y in range(h))
    with open(str(path), "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


def band_mask(w=W, h=H):
    m = np.full((h, w), 255, np.uint8)
    m[h // 4:h // 2, :] = 0
    m[0, 0] = 7          # a grey value that is neither 0 nor 255 stays what it is
    return m


def rig_yaml(masks):
    """A rig of len(masks) cameras; masks[i]: the camera's `mask:` value or None."""
    s = "cameras:\n"
    for i, m in enumerate(masks):
        s += "- camera:\n" + CAMERA.format(i="    ", label="cam%d" % i)
        if m is not None:
            s += "    mask: %s\n" % m
        s += "  T_B_C:\n    data: [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]\n"
    return s + "label: rig\n"


def single_yaml(mask):
    return CAMERA.format(i="", label="solo") + ("" if mask is None else "mask: %s\n" % mask)


def run(mode, path):
    out = subprocess.run([TOOL, mode, str(path)], capture_output=True, text=True)
    lines = out.stdout.splitlines()
    if out.returncode != 0:
        assert lines and lines[0].startswith("error "), out.stdout + out.stderr
        return out.returncode, lines[0][6:]
    cams = []
    for line in lines:
        key, _, rest = line.partition(" ")
        if key == "camera":
            label, w, h = rest.split()
            cams.append(dict(label=label, size=(int(w), int(h))))
        elif key == "mask_file":
            cams[-1]["mask_file"] = None if rest == "-" else rest
        elif key == "mask":
            cams[-1]["mask"] = tuple(int(v) for v in rest.split())
    return 0, cams


def stats(m):
    return (m.shape[1], m.shape[0], int((m == 0).sum()), int(m.astype(np.int64).sum()))


def test_rig_camera_node_mask(tools, tmp_path):
    m = band_mask()
    write_png(tmp_path / "guard.png", m)
    (tmp_path / "rig.yaml").write_text(rig_yaml([None, "guard.png"]))
    rc, cams = run("rig", tmp_path / "rig.yaml")
    assert rc == 0, cams
    assert [c["label"] for c in cams] == ["cam0", "cam1"] and all(c["size"] == (W, H) for c in cams)
    assert cams[0]["mask_file"] is None and cams[0]["mask"] == (0, 0, 0, 0)      # empty image = no mask
    assert cams[1]["mask_file"] == "guard.png" and cams[1]["mask"] == stats(m)


def test_single_camera_document_mask(tools, tmp_path):
    m = band_mask()
    write_png(tmp_path / "rim.png", m)
    (tmp_path / "solo.yaml").write_text(single_yaml("rim.png"))
    rc, cams = run("rig", tmp_path / "solo.yaml")
    assert rc == 0, cams
    assert len(cams) == 1 and cams[0]["label"] == "solo" and cams[0]["size"] == (W, H) and cams[0]["mask"] == stats(m)
    (tmp_path / "plain.yaml").write_text(single_yaml(None))
    rc, cams = run("rig", tmp_path / "plain.yaml")
    assert rc == 0 and cams[0]["mask_file"] is None and cams[0]["mask"] == (0, 0, 0, 0)


@pytest.mark.parametrize("form", ["rig", "single"])
def test_relative_path_is_resolved_against_the_yaml_directory(tools, tmp_path, form):
    m = band_mask()
    (tmp_path / "calib" / "masks").mkdir(parents=True)
    write_png(tmp_path / "calib" / "masks" / "m.png", m)
    y = tmp_path / "calib" / "c.yaml"
    y.write_text(rig_yaml(["masks/m.png"]) if form == "rig" else single_yaml("masks/m.png"))
    elsewhere = tmp_path / "elsewhere"
    elsewhere.mkdir()
    out = subprocess.run([TOOL, "rig", os.path.relpath(str(y), str(elsewhere))], capture_output=True, text=True, cwd=str(elsewhere))
    assert out.returncode == 0, out.stdout
    assert ("mask %d %d %d %d" % stats(m)) in out.stdout
    out = subprocess.run([TOOL, "rig", "c.yaml"], capture_output=True, text=True, cwd=str(tmp_path / "calib"))   # a path without a directory
    assert out.returncode == 0 and ("mask %d %d %d %d" % stats(m)) in out.stdout, out.stdout


@pytest.mark.parametrize("form", ["rig", "single"])
def test_missing_mask_file_is_an_error(tools, tmp_path, form):
    (tmp_path / "c.yaml").write_text(rig_yaml(["nowhere.png"]) if form == "rig" else single_yaml("nowhere.png"))
    rc, err = run("rig", tmp_path / "c.yaml")
    assert rc != 0 and "unable to load mask file" in err and "nowhere.png" in err, err
    (tmp_path / "junk.png").write_bytes(b"not a png")
    (tmp_path / "d.yaml").write_text(rig_yaml(["junk.png"]) if form == "rig" else single_yaml("junk.png"))
    rc, err = run("rig", tmp_path / "d.yaml")
    assert rc != 0 and "unable to load mask file" in err, err


@pytest.mark.parametrize("form", ["rig", "single"])
@pytest.mark.parametrize("size", [(W, H - 1), (W + 1, H), (H, W)])
def test_mask_of_the_wrong_size_is_an_error(tools, tmp_path, form, size):
    write_png(tmp_path / "m.png", band_mask(*size))
    (tmp_path / "c.yaml").write_text(rig_yaml(["m.png"]) if form == "rig" else single_yaml("m.png"))
    rc, err = run("rig", tmp_path / "c.yaml")
    assert rc != 0 and "%d x %d" % size in err and "%d x %d" % (W, H) in err, err


def test_committed_calibrations_load_as_before(tools, tmp_path):
    for name in sorted(os.listdir(CALIB)):
        if name == "bluefox_25000826_fisheye.yaml":
            continue
        copy = tmp_path / name
        shutil.copy(os.path.join(CALIB, name), str(copy))
        rc, cams = run("rig", copy)
        assert rc == 0 and cams and all(c["mask_file"] is None and c["mask"] == (0, 0, 0, 0) for c in cams), (name, cams)
        a = subprocess.run([TEST_IO, "rig", str(copy)], capture_output=True, text=True)
        b = subprocess.run([TEST_IO, "rig", os.path.join(CALIB, name)], capture_output=True, text=True)
        assert a.returncode == 0 and a.stdout == b.stdout and a.stdout.count("label ") == len(cams)


def test_omni_is_still_refused_for_its_type(tools, tmp_path):
    copy = tmp_path / "bluefox_25000826_fisheye.yaml"
    shutil.copy(os.path.join(CALIB, "bluefox_25000826_fisheye.yaml"), str(copy))     # names a mask file that is not there
    for path in (copy, os.path.join(CALIB, "bluefox_25000826_fisheye.yaml")):
        rc, err = run("rig", path)
        assert rc != 0 and err == "calibration: only pinhole cameras are supported", err
    write_png(tmp_path / "25000826_fisheye_mask.png", np.full((480, 752), 255, np.uint8))   # ... and with the file in place
    rc, err = run("rig", copy)
    assert rc != 0 and err == "calibration: only pinhole cameras are supported", err
