"""Kernel time of the matcher's wide twins against the narrow kernels in the same geometry, taken in turns on one device
(svoh_last_kernel_ms, median of five after two warm-up rounds): the 400-seed update (eight lanes per unit), the direct
matcher on the same units (one lane per unit) and the 120-feature stereo seam with 500-step searches (one wave per unit),
cases of tests/wide_matcher.py.  The narrow side is the radtan pair with SVOH_MATCHER_G8 set to the twin's geometry.
Prints one line per case and one JSON line at the end (profiles/wide_matcher.json)."""
import json, sys, os
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from svo_pro_universal_amd import _capi as capi, frontend as fe
import bench, wide_matcher as wm
ctx = fe.Context(0)
names = ("radtan", "equidistant", "atan")


def views(name, mu_range, seam=False):
    sc, ref, cur, cam_r, cam_c = wm.pair(name, seam)
    fr, fc = ctx.build_pyramid(ref[0], 5), ctx.build_pyramid(cur[0], 5)
    return fe.make_frame_view(fr, cam_r, sc.T_ref_f_w, mu_range, 1), fe.make_frame_view(fc, cam_c, sc.T_cur_f_w_gt, 0.0, 2)


def seeds(name):
    sd = wm.seed_set(name)
    rv, cv = views(name, sd["mu_range"])
    mopt, dopt = wm.seed_options(name, 0, 0)
    fb, keep = fe.make_feature_batch(sd["ref_frame_idx"], sd["px"], sd["f"], sd["grad"], sd["level"], sd["type"])
    return lambda: (keep, ctx.update_seeds_batch(mopt, dopt, [rv], cv, fb, sd["state"]))


def direct(name):
    sd, di = wm.seed_set(name), wm.direct_inputs(name)
    rv, cv = views(name, sd["mu_range"])
    fb, keep = fe.make_feature_batch(sd["ref_frame_idx"], sd["px"], sd["f"], sd["grad"], sd["level"], di["type"])
    return lambda: (keep, ctx.match_direct_batch(capi.default_matcher_options(), [rv], cv, fb, sd["true_depth"], di["px_init"]))


def seam(name):
    si = wm.seam_inputs(name)
    sd = si["sd"]
    rv, cv = views(name, 0.0, seam=True)
    fb, keep = fe.make_feature_batch(sd["ref_frame_idx"], sd["px"], sd["f"], sd["grad"], sd["level"], si["type"])
    return lambda: (keep, ctx.epipolar_match_batch(wm.seam_options(), [rv], cv, fb, d_inv_common=list(si["d_inv_common"]), T_cur_ref=[si["T_f1f0"]]))


out = {}
for case, make, g8 in (("seeds_400_eight_lanes", seeds, "1"), ("direct_400_one_lane", direct, "0"), ("seam_120x500_one_wave", seam, "3")):
    os.environ["SVOH_MATCHER_G8"] = g8       # the narrow launch's geometry; a wide launch ignores it
    ctx.reload_knobs()
    calls = {name: make(name) for name in names}
    ks = {name: [] for name in names}
    for i in range(7):
        for name in names:   # in turns
            calls[name]()
            if i >= 2: ks[name].append(bench.misc_kernel_ms(ctx))
    for name in names:
        key = "%s_%s_kernel_ms" % (case, name)
        out[key] = float(np.median(ks[name]))
        print("%-56s %.4f" % (key, out[key]), flush=True)
os.environ.pop("SVOH_MATCHER_G8")
print(json.dumps(out))
