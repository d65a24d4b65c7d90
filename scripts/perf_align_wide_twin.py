"""Kernel time of ONE 2000-feature 4x4 problem through the wide twin (an equidistant camera, sparse_align_wide_kernel<4, false, false>)
and of the radtan scene of the same seed through the twin's narrow counterpart, sparse_align_kernel<4, 512, false, false, false, 1,
false, false> (SVOH_ALIGN_THREADS=512, cluster mode off).  Device events of the library (svoh_sparse_align_last_kernel_ms), the two
alternating in one process, five warm-up launches each, then the median / min / max of REPS launches.

  python scripts/perf_align_wide_twin.py [out.txt]"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from svo_pro_universal_amd import _capi as capi, frontend as fe, synth   # noqa: E402
import wide_geometry as wg                                               # noqa: E402

SEED, N, REPS, WARM = 313, 2000, 41, 5
os.environ["SVOH_ALIGN_THREADS"] = "512"
os.environ["SVOH_ALIGN_CLUSTER"] = "0"     # one workgroup for the problem, as the twin has
ctx = fe.Context(0)
ms = ctypes.c_float()
opt = capi.default_align_options(patch_size=4, max_level=4, min_level=0)
cases = {}
for kind in ("equidistant", "radtan"):
    sc = synth.make_align_scene(SEED, n_features=N, patch_size=4, cam=wg.camera(kind), border_features=100)
    pb, keep = fe.make_align_problems([[(sc, ctx.build_pyramid(sc.img_ref, 5), ctx.build_pyramid(sc.img_cur, 5))]])
    cases[kind] = (pb, keep, ctx.sparse_align_wide if kind == "equidistant" else ctx.sparse_align)
times = {k: [] for k in cases}
res = {}
for i in range(WARM + REPS):
    for kind, (pb, _keep, call) in cases.items():
        res[kind] = call(opt, pb)[0]
        ctx._check(ctx.lib.svoh_sparse_align_last_kernel_ms(ctx.h, ctypes.byref(ms)))
        if i >= WARM:
            times[kind].append(ms.value)
info = ctx.last_align_launch()
assert info["nt"] == 512 and info["rows"] == 1 and info["cluster_g"] == 0 and not info["rig"], info
lines = ["one problem, %d features (+100 at the border), 4x4 patches, levels 4..0, kernel ms over %d launches after %d warm-up launches, alternating" % (N, REPS, WARM)]
for kind, name in (("equidistant", "sparse_align_wide_kernel<4, false, false> (equidistant)"),
                   ("radtan", "sparse_align_kernel<4, 512, false, false, false, 1, false, false> (radtan)")):
    t, r = np.array(times[kind]), res[kind]
    lines.append("%-82s median %.4f  min %.4f  max %.4f   patch-iterations %d, iterations per level %s, status %d" % (
        name, np.median(t), t.min(), t.max(), r.n_patch_iters, list(r.iters)[:5], r.status))
text = "\n".join(lines)
print(text)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(text + "\n")
