"""Camera masks on the device: svoh_mask_upload / svoh_mask_release and the batched detector with a mask per frame
(svoh_detect_cells_batch_masked, _masked_enqueue + svoh_detect_cells_batch_collect) against the CPU oracle and against
svoh_detect_features with the same mask on the host.

A mask acts BETWEEN the detector's two phases (fd_utils::fillFeatures, then edgeletDetector_V2 on the cells still free,
feature_detection.cpp:157-194): a cell whose corner winner lies on a zero mask pixel is free for an edgelet, and an
edgelet winner on a zero pixel leaves its cell empty.  The third frame's mask is built so that both happen; the test
asserts that on the oracle's own output before it looks at the device.

Bars (those of tests/test_detector_gpu.py): positions, levels, types, counts and scores exact; gradient directions exact
unless the device's atan2 puts a pixel of the 9x9 histogram window into the other of two adjacent 10-degree bins
(<= 2 % of the features, which then differ by one bin).  Device against device: every field bitwise."""
import ctypes as C

import numpy as np
import pytest

from svo_pro_universal_amd import _capi as capi, frontend as fe, synth

pytestmark = pytest.mark.gpu

W, H, CELL = 160, 120, 20
N_COLS, N_ROWS = W // CELL, H // CELL
N_CELLS = N_COLS * N_ROWS          # 48
N_LEVELS = 3
SCENE_SEEDS = (301, 302, 303)
# the seed of the third frame's mask: chosen on the CPU (oracle only) so that cases (a) and (b) below both occur
MASK_SEED = 0
N_BLOCKS = 16                      # corner winners that get a 3 x 3 block of zeros around them
FT_CORNER, FT_EDGELET = 7, 6     # svoh_feature_type
ERR_INVALID_ARGUMENT, ERR_BAD_HANDLE = -1, -4   # svoh_status
SCATTER = 0.25                     # share of single pixels zeroed on top


def options():
    return capi.default_detector_options(cell_size=CELL, min_level=0, max_level=2, detect_edgelets=1)


def cell_of(px):
    return (np.floor(px[:, 1] / CELL) * N_COLS + np.floor(px[:, 0] / CELL)).astype(int)


def seeded_mask(unmasked, seed):
    """Zeroes a 3 x 3 block around N_BLOCKS of the corner winners of the unmasked detection, plus scattered pixels.
    Returns the mask, and the mask with the blocks alone."""
    rng = np.random.RandomState(seed)
    blocks = np.full((H, W), 255, np.uint8)
    corners = unmasked["px"][unmasked["type"] == FT_CORNER].astype(int)
    for x, y in corners[rng.permutation(len(corners))[:N_BLOCKS]]:
        blocks[max(0, y - 1):y + 2, max(0, x - 1):x + 2] = 0
    mask = blocks.copy()
    mask[rng.uniform(size=(H, W)) < SCATTER] = 0
    return mask, blocks


def on_zero(mask, d):
    return mask[d["px"][:, 1].astype(int), d["px"][:, 0].astype(int)] == 0


def cases_a_b(unmasked, with_blocks, masked, mask):
    """(a) cells whose unmasked corner winner is masked and which then hold an edgelet; (b) cells whose edgelet winner is
    masked and which stay empty.  A cell's edgelet winner does not depend on the mask (the mask only decides whether the
    cell is free and whether the winner is kept), so the winners are read off the oracle's output for the blocks alone,
    where nothing but the chosen corners is masked: its edgelets in cells without a corner under the full mask."""
    cu, cb, cm = cell_of(unmasked["px"]), cell_of(with_blocks["px"]), cell_of(masked["px"])
    is_corner = unmasked["type"] == FT_CORNER
    edge_cells_masked = set(cm[masked["type"] == FT_EDGELET])
    a = [c for c in cu[is_corner & on_zero(mask, unmasked)] if c in edge_cells_masked]
    b = [c for c in cb[(with_blocks["type"] == FT_EDGELET) & on_zero(mask, with_blocks)] if c not in set(cm)]
    return a, b


def compare(dg, do):
    assert len(dg["score"]) == len(do["score"])
    assert np.array_equal(dg["type"], do["type"]) and np.array_equal(dg["px"], do["px"])
    assert np.array_equal(dg["level"], do["level"]) and np.array_equal(dg["score"], do["score"])
    same = np.all(dg["grad"] == do["grad"], axis=1)
    if not same.all():
        ang = np.arccos(np.clip(np.sum(dg["grad"] * do["grad"], axis=1), -1, 1))
        assert (~same).mean() <= 0.02 and ang.max() < np.deg2rad(10.5), ((~same).sum(), ang.max())


def same_features(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("px", "score", "level", "grad", "type"))


def make_inputs(oracle_lib):
    cam = synth.Camera.euroc_like(W, H)
    imgs = [synth.make_align_scene(s, n_features=8, cam=cam).img_ref for s in SCENE_SEEDS]
    pyramids = [oracle_lib.create_img_pyramid(im, N_LEVELS) for im in imgs]
    opt = options()
    left = np.full((H, W), 255, np.uint8); left[:, :W // 2] = 0
    unmasked3 = oracle_lib.detect_features(opt, pyramids[2], None, None)
    mask3, blocks3 = seeded_mask(unmasked3, MASK_SEED)
    masks = [None, left, mask3]
    occ = (np.random.RandomState(11).uniform(size=(3, N_CELLS)) < 0.25).astype(np.uint8)
    return imgs, pyramids, masks, occ, unmasked3, oracle_lib.detect_features(opt, pyramids[2], None, blocks3)


@pytest.fixture(scope="module")
def setup(gpu_ctx, oracle_lib):
    imgs, pyramids, masks, occ, unmasked3, with_blocks3 = make_inputs(oracle_lib)
    opt = options()
    want = {None: [oracle_lib.detect_features(opt, pyramids[i], None, masks[i]) for i in range(3)],
            "occ": [oracle_lib.detect_features(opt, pyramids[i], occ[i], masks[i]) for i in range(3)]}
    frames = [gpu_ctx.build_pyramid(im, N_LEVELS) for im in imgs]
    handles = [0 if m is None else gpu_ctx.upload_mask(m) for m in masks]
    yield dict(imgs=imgs, pyramids=pyramids, masks=masks, occ=occ, unmasked3=unmasked3, with_blocks3=with_blocks3, want=want, frames=frames, handles=handles)
    for hd in handles:
        if hd:
            gpu_ctx.release_mask(hd)
    for f in frames:
        gpu_ctx.release_frame(f)


def fill(opt, arrays, i):
    ck, ek, ang = arrays
    return fe.detect_fill_features(opt, W, H, ck[i], ek[i], ang[i])


def test_the_third_mask_meets_both_cases(oracle_lib):
    """On the oracle's own output (no device call): (a) a masked corner winner's cell receives an edgelet, (b) a masked edgelet
    winner's cell stays empty -- each at least once in the third frame.  Without them the parity below would prove nothing."""
    imgs, pyramids, masks, occ, unmasked3, with_blocks3 = make_inputs(oracle_lib)
    a, b = cases_a_b(unmasked3, with_blocks3, oracle_lib.detect_features(options(), pyramids[2], None, masks[2]), masks[2])
    print("case (a) cells", a, "case (b) cells", b)
    assert len(a) >= 1 and len(b) >= 1


@pytest.mark.parametrize("with_occupancy", [False, True])
def test_masked_batch_equals_oracle_and_single_frame_detector(gpu_ctx, setup, with_occupancy):
    opt = options()
    occ = setup["occ"] if with_occupancy else None
    want = setup["want"]["occ" if with_occupancy else None]
    arrays = gpu_ctx.detect_cells_batch(opt, setup["frames"], W, H, occupancy=occ, masks=setup["handles"])
    for i in range(3):
        got = fill(opt, arrays, i)
        print("frame", i, "features", len(got["score"]), "oracle", len(want[i]["score"]))
        assert len(want[i]["score"]) > 0
        compare(got, want[i])
        m = setup["masks"][i]
        if m is not None:
            assert (m[got["px"][:, 1].astype(int), got["px"][:, 0].astype(int)] != 0).all()
        single = gpu_ctx.detect_features(opt, setup["frames"][i], W, H, None if occ is None else occ[i], m)
        assert same_features(got, single)


def raw_masked(ctx, opt, frames, occ, masks):
    n = len(frames)
    fr = (capi.svoh_frame_t * n)(*frames)
    mk = None if masks is None else (capi.svoh_mask_t * n)(*masks)
    ck = np.zeros((n, N_CELLS), np.uint64); ek = np.zeros((n, N_CELLS), np.uint64); ang = np.zeros((n, N_CELLS), np.float32)
    rc = ctx.lib.svoh_detect_cells_batch_masked(ctx.h, n, fr, C.byref(opt), None if occ is None else occ.ctypes.data, mk,
                                                ck.ctypes.data, ek.ctypes.data, ang.ctypes.data)
    return rc, (ck, ek, ang)


def test_no_mask_is_the_unmasked_entry(gpu_ctx, setup):
    opt = options()
    plain = gpu_ctx.detect_cells_batch(opt, setup["frames"], W, H, occupancy=setup["occ"])
    assert plain[0].any()   # (every free cell of these scenes holds a corner: without a mask no edgelet is looked for)
    for masks in (None, [0, 0, 0]):
        rc, got = raw_masked(gpu_ctx, opt, setup["frames"], setup["occ"], masks)
        assert rc == 0
        for a, b in zip(got, plain):
            assert a.tobytes() == b.tobytes()


def test_all_zero_mask_gives_no_feature(gpu_ctx, setup):
    opt = options()
    hd = gpu_ctx.upload_mask(np.zeros((H, W), np.uint8))
    try:
        arrays = gpu_ctx.detect_cells_batch(opt, setup["frames"], W, H, masks=[hd, hd, hd])
        assert not arrays[0].any() and not arrays[1].any()
        for i in range(3):
            assert len(fill(opt, arrays, i)["score"]) == 0
    finally:
        gpu_ctx.release_mask(hd)


def test_bad_masks_are_refused_and_the_context_stays_usable(gpu_ctx, setup):
    opt = options()
    good = gpu_ctx.detect_cells_batch(opt, setup["frames"], W, H, masks=setup["handles"])
    small = gpu_ctx.upload_mask(np.full((H // 2, W // 2), 255, np.uint8))
    released = gpu_ctx.upload_mask(np.full((H, W), 255, np.uint8))
    gpu_ctx.release_mask(released)
    for masks, code in (([0, small, 0], ERR_INVALID_ARGUMENT), ([released, 0, 0], ERR_BAD_HANDLE),
                        ([0, 0, 1 << 40], ERR_BAD_HANDLE)):
        with pytest.raises(fe.SvohError) as e:
            gpu_ctx.detect_cells_batch(opt, setup["frames"], W, H, masks=masks)
        assert e.value.code == code, (masks, e.value.code)
        with pytest.raises(fe.SvohError) as e:
            gpu_ctx.detect_cells_batch_enqueue(opt, setup["frames"], masks=masks)
        assert e.value.code == code
    for hd in (released, 1 << 40, 0):
        with pytest.raises(fe.SvohError) as e:
            gpu_ctx.release_mask(hd)
        assert e.value.code == ERR_BAD_HANDLE
    gpu_ctx.release_mask(small)
    again = gpu_ctx.detect_cells_batch(opt, setup["frames"], W, H, masks=setup["handles"])
    for a, b in zip(again, good):
        assert a.tobytes() == b.tobytes()


def test_enqueue_and_collect_equal_the_blocking_call(gpu_ctx, setup):
    opt = options()
    blocking = gpu_ctx.detect_cells_batch(opt, setup["frames"], W, H, occupancy=setup["occ"], masks=setup["handles"])
    gpu_ctx.detect_cells_batch_enqueue(opt, setup["frames"], occupancy=setup["occ"], masks=setup["handles"])
    between = gpu_ctx.detect_features(opt, setup["frames"][1], W, H, None, setup["masks"][1])   # another blocking call of the context
    assert len(between["score"]) > 0
    queued = gpu_ctx.detect_cells_batch_collect(opt, 3, W, H)
    for a, b in zip(queued, blocking):
        assert a.tobytes() == b.tobytes()
