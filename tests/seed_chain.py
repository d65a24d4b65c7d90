"""Shared data of the seed-chain tests (svoh_update_seeds_chain: a new keyframe's seeds against a list of frames in one
launch): one scene, five further views, three reference views on the same image with chains of different length, and
the comparison arm -- one update_seeds_batch call per chain position, on the GPU or in the oracle.

Sizes: 301 seeds leave a ragged tail in every geometry (301 mod 64 = 45, mod 8 = 5); 77 and 40 seeds belong to the
reference views with a chain of one and with none."""
import math

import numpy as np

from svo_pro_universal_amd import _capi as capi, synth

N_SEEDS = (301, 77, 40)
REF_IDS = (1, 2, 3)
# where the views stand in the frame list: five views, then view 0 once more under the FIRST reference view's id (every
# unit of that reference view skips the step), then view 1 at a pose that looks away (no seed is visible: NOT_RUN)
VIEW_SAME_ID, VIEW_AWAY = 5, 6
CHAINS_4 = ([0, VIEW_SAME_ID, VIEW_AWAY, 1], [2], [])
CHAINS_6 = ([0, 1, 2, 3, 4, 1], [2], [])
CHAINS_3 = ([0, 1, 2], [2], [])
SCENE_SEED = 61   # chosen on the CPU: the oracle's run over CHAINS_3 meets the conditions of the oracle test


class ChainData(object):
    pass


def make_data(cam_kind="pinhole", seed=SCENE_SEED):
    """Scene, images and poses of all views, the seeds.  No GPU, no oracle."""
    cam = synth.Camera.test_camera() if cam_kind == "pinhole" else synth.Camera.euroc_like()
    sc = synth.make_align_scene(seed, n_features=10, cam=cam, rot_deg=(0.5, 1.5), trans_m=(0.05, 0.15))
    rng = np.random.RandomState(seed + 31)
    d = ChainData()
    d.sc, d.cam = sc, cam
    d.imgs, d.T_f_w, d.ids = [], [], []
    for k in range(5):   # the motions of the matcher tests' scene_and_frames: 0.5-1.5 degrees, 0.05-0.15 m from the reference
        q = synth.quat_from_axis_angle(rng.normal(size=3), np.deg2rad(rng.uniform(0.5, 1.5)))
        t = rng.normal(size=3)
        T_w_c = sc.T_w_ref * synth.SE3(q, t / np.linalg.norm(t) * rng.uniform(0.05, 0.15))
        d.imgs.append(synth.render(cam, T_w_c, sc.plane, sc.tex))
        d.T_f_w.append(T_w_c.inverse())
        d.ids.append(10 + k)
    d.imgs.append(d.imgs[0]); d.T_f_w.append(d.T_f_w[0]); d.ids.append(REF_IDS[0])
    away = sc.T_w_ref * synth.SE3(synth.quat_from_axis_angle([1.0, 0.0, 0.0], np.deg2rad(85.0)), [0.0, 0.0, 0.0])
    d.imgs.append(d.imgs[1]); d.T_f_w.append(away.inverse()); d.ids.append(20)
    n = sum(N_SEEDS)
    sd = synth.make_seed_set(sc, n, margin=12)
    sd["type"][::17] = capi.FT_MAPPOINT_SEED       # the input types of test_update_seeds_parity
    sd["type"][5::41] = capi.FT_CORNER             # not a seed: skipped
    sd["type"][7::53] = capi.FT_OUTLIER
    sd["type"][9::59] = capi.FT_EDGELET_SEED_CONVERGED
    # Seeds late in their life, one observation short of convergence (sigma just above mu_range / 200, mu within half a
    # per cent of the truth): two motions of this size take a fresh seed's sigma from mu_range / 6 to about mu_range / 20,
    # never to convergence, and the chain has to carry a seed that converges on the way as a converged seed
    st = sd["state"].reshape(-1, 4)
    late = np.arange(3, n, 23)
    # (corner and edgelet seeds only: the data dates from when the single-call per-unit kernels marked a map-point seed
    # converged at the seed threshold.  Map-point seeds between the two thresholds are tests/seed_exits.py's now.)
    late = late[late % 17 != 0]
    st[late, 0] = 1.0 / (sd["true_depth"][late] * np.random.RandomState(seed + 77).uniform(0.995, 1.005, late.size))
    st[late, 1] = (sd["mu_range"] / 199.9) ** 2
    sd["ref_frame_idx"] = np.repeat(np.arange(3, dtype=np.int32), N_SEEDS)
    d.sd = sd
    return d


def make_views(d, make_frame_view, ref_frame, view_frames):
    """(reference views, frame list) through fe.make_frame_view or orc.make_frame_view; view_frames: the five views'
    frames (handles or oracle pyramids)."""
    frames = list(view_frames) + [view_frames[0], view_frames[1]]
    refs = [make_frame_view(ref_frame, d.cam, d.sc.T_ref_f_w, d.sd["mu_range"], i) for i in REF_IDS]
    lst = [make_frame_view(frames[k], d.cam, d.T_f_w[k], 0.0, d.ids[k]) for k in range(len(frames))]
    return refs, lst


def subset(sd, sel):
    px, f, grad = sd["px"].reshape(-1, 2), sd["f"].reshape(-1, 3), sd["grad"].reshape(-1, 2)
    return px[sel].ravel(), f[sel].ravel(), grad[sel].ravel(), sd["level"][sel]


def run_sequence(update, make_feature_batch, ref_views, frame_list, chains, sd, mopt, dopt, state=None, types=None):
    """The comparison arm: update(mopt, dopt, [ref view], cur view, fb, state) once per chain position, states and types
    fed back; the units of a reference view are left out of the calls beyond its chain.
    Returns (n_success, state, types, step_result, step_success) laid out like the chain call's outputs."""
    n = len(sd["level"])
    state = np.array(sd["state"] if state is None else state, np.float64).reshape(n, 4).copy()
    types = np.array(sd["type"] if types is None else types, np.uint8).copy()
    max_steps = max(len(c) for c in chains)
    res = np.full((n, max_steps), capi.MATCH_NOT_RUN, np.int32)
    suc = np.zeros((n, max_steps), np.uint8)
    total = 0
    for r, chain in enumerate(chains):
        sel = np.nonzero(sd["ref_frame_idx"] == r)[0]
        px, f, grad, level = subset(sd, sel)
        for j, k in enumerate(chain):
            fb, keep = make_feature_batch(np.zeros(sel.size, np.int32), px, f, grad, level, types[sel])
            ns, st, s, mr = update(mopt, dopt, [ref_views[r]], frame_list[k], fb, state[sel].ravel())
            state[sel] = st.reshape(-1, 4); types[sel] = keep["type"]
            res[sel, j] = mr; suc[sel, j] = s
            total += ns
    return total, state.ravel(), types, res, suc
