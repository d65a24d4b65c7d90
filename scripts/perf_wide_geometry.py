"""Kernel time of the pose optimiser on a radtan camera (narrow kernel) and on an equidistant one (wide twin), taken in
turns on one device: 2048 bundles x 180 features and one bundle, image-plane and bearing-difference errors.  Prints
one line per case and one JSON line at the end (profiles/).  The candidate projection's launch is not bracketed by
the timing events (svoh_last_kernel_ms does not see it) and is not measured here."""
import json, sys, os
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from svo_pro_universal_amd import _capi as capi, frontend as fe, synth
import bench, pose_helpers as ph
ctx = fe.Context(0)
cams = {"radtan": synth.Camera.euroc_like(752, 480), "equidistant": synth.Camera.visensor_like()}
out = {}
for n_bundles in (2048, 1):
    for et, et_name in ((capi.POSE_ERR_IMAGE_PLANE, "image_plane"), (capi.POSE_ERR_BEARING_DIFF, "bearing_diff")):
        built = {}
        for name, cam in cams.items():
            scs = [ph.make_pose_scene(900 + k, n=180, cam=cam) for k in range(8)]
            pbs = [fe.make_pose_problem(scs[k % 8]["cams"], scs[k % 8]["T_imu_world_init"]) for k in range(n_bundles)]
            built[name] = (capi.default_pose_options(cam, error_type=et), pbs)
        ks = {name: [] for name in cams}
        for i in range(7):
            for name in cams:   # in turns
                opt, pbs = built[name]
                ctx.optimize_pose(opt, [p[0] for p in pbs])
                if i >= 2: ks[name].append(bench.misc_kernel_ms(ctx))
        for name in cams:
            key = "pose_%s_%dx180_%s_kernel_ms" % (et_name, n_bundles, name)
            out[key] = float(np.median(ks[name]))
            print("%-56s %.4f" % (key, out[key]), flush=True)
print(json.dumps(out))
