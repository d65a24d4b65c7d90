"""The parameter loader's keys of the initialiser (svo_factory.cpp:123, 178-195) through tests/cpp_init/init_params_tool."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tests", "cpp_init", "init_params_tool")


@pytest.fixture(scope="module", autouse=True)
def tool():
    """The tool, made here when build() has not left it (it links the host library); nothing to do otherwise."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "svo_pro_universal_amd", "host"), "libsvo_hip_host.so"])
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(TOOL), "init_params_tool"])

DEFAULTS = dict(init_min_features="100", init_min_tracked="80", init_min_inliers="70", init_min_disparity="40",
                init_min_features_factor="2", init_disparity_pivot_ratio="0.5", reproj_err_thresh="2", map_scale="1",
                init_method="FivePoint", init_type="2")


def read(arg):
    out = subprocess.check_output([TOOL, arg], timeout=60).decode()
    return dict(line.split("=", 1) for line in out.splitlines())


def test_defaults_are_the_factorys():
    assert read("-") == DEFAULTS


def test_every_key_is_read(tmp_path):
    p = tmp_path / "params.yaml"
    p.write_text("init_min_features: 60\ninit_min_tracked: 41\ninit_min_inliers: 33\ninit_min_disparity: 12.5\n"
                 "init_min_features_factor: 2.5\ninit_disparity_pivot_ratio: 0.25\nreproj_err_thresh: 1.5\nmap_scale: 3.75\n"
                 "init_method: Homography\n")
    assert read(str(p)) == dict(init_min_features="60", init_min_tracked="41", init_min_inliers="33", init_min_disparity="12.5",
                                init_min_features_factor="2.5", init_disparity_pivot_ratio="0.25", reproj_err_thresh="1.5",
                                map_scale="3.75", init_method="Homography", init_type="0")


def test_methods(tmp_path):
    p = tmp_path / "params.yaml"
    for method, kind in (("TwoPoint", "1"), ("FivePoint", "2"), ("OneShot", "3"), ("Homography", "0")):
        p.write_text("init_method: %s\n" % method)
        got = read(str(p))
        assert (got["init_method"], got["init_type"]) == (method, kind)
    # a method the factory does not know keeps its name (whoever needs an initialiser refuses it by that name) and the default type
    p.write_text("init_method: Sideways\n")
    got = read(str(p))
    assert (got["init_method"], got["init_type"]) == ("Sideways", "2")
    # the other keys of a file are untouched by these
    p.write_text("max_fts: 180\ninit_method: Homography\n")
    assert read(str(p))["init_method"] == "Homography"
