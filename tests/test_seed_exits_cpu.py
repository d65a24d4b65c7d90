"""The crafted seed set of tests/seed_exits.py does what it was made for, shown with the CPU oracle alone: the oracle's
run over it leaves depth_filter_utils::updateSeed through every exit at least once (no GPU)."""
import numpy as np
import pytest

import seed_exits as sx


@pytest.fixture(scope="module")
def oracle_runs(oracle_lib):
    orc = oracle_lib
    d = sx.make_data()
    pyr_ref, pyr_cur = orc.create_img_pyramid(d.sc.img_ref, 5), orc.create_img_pyramid(d.sc.img_cur, 5)   # (the views point into them)
    refs, cur = sx.make_views(d, orc.make_frame_view, pyr_ref, pyr_cur)
    runs = {}
    for run in sx.RUNS:
        mopt, dopt = sx.options(d, run)
        fb, keep = orc.make_feature_batch(d.sd["ref_frame_idx"], d.sd["px"], d.sd["f"], d.sd["grad"], d.sd["level"], d.sd["type"])
        ns, st, suc, res = orc.update_seeds_batch(mopt, dopt, refs, cur, fb, d.sd["state"])
        runs[run] = (ns, st, keep["type"], suc, res)
    return d, runs


def test_the_set_is_small_and_on_a_320x240_pinhole_pair(oracle_runs):
    d, runs = oracle_runs
    assert d.sd["level"].size == sx.N <= 64
    assert (d.cam.width, d.cam.height) == (320, 240) and d.sc.img_ref.shape == (240, 320) and d.sc.img_cur.shape == (240, 320)


@pytest.mark.parametrize("run", sorted(sx.RUNS))
def test_oracle_run_reaches_every_exit(oracle_runs, run):
    d, runs = oracle_runs
    ns, st, types, suc, res = runs[run]
    classes = sx.classify(d, run, st, types, suc, res)
    print({k: v.tolist() for k, v in classes.items()})
    empty = [name for name in sx.EXITS[run] if classes[name].size == 0]
    assert not empty, empty
    assert ns == int(suc.sum())
    # no unit outside the classification: every unit took exactly one of the exits
    count = np.zeros(sx.N, int)
    for idx in classes.values():
        count[idx] += 1
    assert np.all(count == 1), np.nonzero(count != 1)[0]
