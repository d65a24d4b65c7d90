#!/usr/bin/env python3
"""Generates tests/golden/homography_held_case.npz: the 70 bearing pairs and the focal length that the reference's own
homography test holds (src/vikit/vikit_common/test/test_homography.cpp, loadData) -- test DATA of the reference, parsed
out of that file's text; nothing of its program goes into the fixture.  The test there asserts 69 inliers of
vk::computeInliers at 2 px for the motion of vk::estimateHomography (with OpenCV's estimator); that number is stored
beside the data as `reference_inliers`.
Usage: python tests/golden/make_homography_held_case.py <path to test_homography.cpp> [--check]"""
import os
import re
import sys

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "homography_held_case.npz")


def parse(text):
    num = r"([-+0-9.eE]+)"
    out = {}
    for name in ("f_ref", "f_cur"):
        rows = re.findall(name + r"\.col\(i\+\+\)\s*=\s*Vector3d\(\s*" + num + r"\s*,\s*" + num + r"\s*,\s*" + num + r"\s*\)", text)
        out[name] = np.array(rows, np.float64)
    out["focal_length"] = np.float64(re.search(r"focal_length\s*=\s*" + num + r"\s*;", text).group(1))
    out["reproj_error_thresh"] = np.float64(re.search(r"reproj_error_thresh\s*=\s*" + num + r"\s*;", text).group(1))
    out["reference_inliers"] = np.int64(re.search(r"EXPECT_EQ\(inliers\.size\(\)\s*,\s*(\d+)\)", text).group(1))
    assert out["f_ref"].shape == out["f_cur"].shape == (70, 3), (out["f_ref"].shape, out["f_cur"].shape)
    return out


def main(argv):
    data = parse(open(argv[1]).read())
    if "--check" in argv:
        old = np.load(PATH)
        for k, v in data.items():
            assert np.array_equal(old[k], v), k
        print("fixture matches")
        return
    np.savez(PATH, **data)
    print("wrote %s: %d pairs, focal_length %.3f" % (PATH, data["f_ref"].shape[0], data["focal_length"]))


if __name__ == "__main__":
    main(sys.argv)
