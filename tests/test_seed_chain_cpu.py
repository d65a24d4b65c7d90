"""The seed chain's CPU side: the data the GPU tests compare on (tests/seed_chain.py) sits on no threshold -- the C oracle and the
NumPy second reading of the reference (tests/np_restatement_direct.py) agree over the chain of three, discrete outputs exactly --
and the parameter loader reads update_seeds_with_old_keyframes as the reference's factory does (svo_factory.cpp:147-148)."""
import os
import subprocess

import numpy as np
import pytest

from svo_pro_universal_amd import _capi as capi

import np_restatement_direct as nd
import seed_chain as scn
from test_np_second_opinion_cpu import _nd_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tests", "cpp_seed_chain", "params_tool")


def test_oracle_and_numpy_reading_agree_over_the_chain_of_three(oracle_lib):
    orc = oracle_lib
    d = scn.make_data("pinhole")
    ref = orc.create_img_pyramid(d.sc.img_ref, 5)
    pyr = [orc.create_img_pyramid(im, 5) for im in d.imgs[:5]]
    orefs, olst = scn.make_views(d, orc.make_frame_view, ref, pyr)
    mopt = capi.default_matcher_options()
    dopt = capi.default_depth_filter_options(d.cam, check_visibility=1, check_convergence=0)
    ns_o, st_o, types_o, res_o, suc_o = scn.run_sequence(orc.update_seeds_batch, orc.make_feature_batch, orefs, olst, scn.CHAINS_3, d.sd, mopt, dopt)

    ncam = nd.Cam.of(d.cam)
    frames = pyr + [pyr[0], pyr[1]]
    nrefs = [nd.FrameView(ref, ncam, nd.Tf.from7(d.sc.T_ref_f_w.as7()), i, d.sd["mu_range"]) for i in scn.REF_IDS]
    nlst = [nd.FrameView(frames[k], ncam, nd.Tf.from7(d.T_f_w[k].as7()), d.ids[k], 0.0) for k in range(len(frames))]

    def nd_update(mopt_, dopt_, refs, cur, fb, state):
        fb, types = fb
        got = nd.update_seeds(cur, refs, fb["ref_frame_idx"], fb["px"], fb["f"], fb["grad"], fb["level"], types["type"], state, _nd_options(mopt_),
                              dopt_.seed_convergence_sigma2_thresh, dopt_.mappoint_convergence_sigma2_thresh, dopt_.px_error_angle,
                              bool(dopt_.check_visibility), bool(dopt_.check_convergence), bool(dopt_.use_vogiatzis_update))
        types["type"] = got["type"]
        return int(got["success"].sum()), got["state"], got["success"], got["match_result"]

    def nd_batch(ref_frame_idx, px, f, grad, level, ftype):
        keep = dict(type=np.array(ftype, np.uint8))
        return (dict(ref_frame_idx=ref_frame_idx, px=px, f=f, grad=grad, level=level), keep), keep

    ns_n, st_n, types_n, res_n, suc_n = scn.run_sequence(nd_update, nd_batch, nrefs, nlst, scn.CHAINS_3, d.sd, mopt, dopt)
    assert np.array_equal(res_o, res_n), np.argwhere(res_o != res_n)[:10]
    assert np.array_equal(suc_o, suc_n) and np.array_equal(types_o, types_n) and ns_o == ns_n
    # (np.allclose' rtol against the larger of the two would be the same bar; NaN states, if any, must agree)
    assert np.allclose(st_o, st_n, rtol=1e-9, atol=0, equal_nan=True), np.abs(st_o - st_n).max()
    assert ns_o > scn.N_SEEDS[0]   # the chain does work: more successes than seeds


@pytest.mark.parametrize("text,want", [("update_seeds_with_old_keyframes: True\n", 1), ("update_seeds_with_old_keyframes: False\n", 0),
                                       ("max_fts: 180\n", 1), (None, 1)])
def test_parameter_loader_reads_the_key(tmp_path, text, want):
    if not os.path.exists(TOOL):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(TOOL)])
    arg = "-"
    if text is not None:
        (tmp_path / "params.yaml").write_text(text)
        arg = str(tmp_path / "params.yaml")
    r = subprocess.run([TOOL, arg], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "update_seeds_with_old_keyframes=%d" % want
