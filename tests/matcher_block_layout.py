"""The staging blocks of the matcher entries (csrc/matcher.hip), restated in plain Python from the host code as it stood BEFORE the
layouts moved to csrc/svoh_matcher_block.h: per entry the list of columns in the order that code appended them, each offset the
running total, the total rounded up to 64 after every column.  Not generated from the header: tests/test_matcher_block_cpu.py holds
the header against this file, tests/test_matcher_stage_layout_gpu.py holds the library (through the pointers svoh_matcher_stage
hands out) against it.

A layout is a dict: "cols" = [(name, offset), ...] in block order, and the marks "in_total" (end of what is uploaded), "back_from"
(first byte that comes back), "end" (end of what comes back) and "total" (bytes of the block)."""

DEV_FRAME_VIEW_BYTES = 432        # sizeof(svoh::DevFrameView)
DEV_FRAME_VIEW_WIDE_BYTES = 472   # sizeof(svoh::DevFrameViewWide)
RIGID_BYTES = 56                  # sizeof(svoh::Rigid)


class _Block:
    def __init__(self):
        self.cols, self.total = [], 0

    def add(self, name, nbytes):
        off = self.total
        self.cols.append((name, off))
        self.total = (self.total + nbytes + 63) & ~63
        return off

    def off(self, name):
        return dict(self.cols)[name]

    def done(self, in_total, back_from, end):
        return {"cols": self.cols, "in_total": in_total, "back_from": back_from, "end": end, "total": self.total}


def _feature_columns(b, n, cur_idx):
    b.add("ref_frame_idx", 4 * n)
    if cur_idx:
        b.add("cur_frame_idx", 4 * n)
    b.add("px", 16 * n)
    b.add("f", 24 * n)
    b.add("grad", 16 * n)
    b.add("level", 4 * n)
    b.add("type", n)


def direct_batch(n, n_views, view_bytes, cur_idx=False, landmark_xyz=False):
    """run_matcher, direct matches over host arrays (svoh_match_direct_batch, ..._pixelwise with landmark_xyz)"""
    b = _Block()
    b.add("views", view_bytes * n_views)
    _feature_columns(b, n, cur_idx)
    b.add("depth", 8 * n)
    b.add("px_cur", 16 * n)
    if landmark_xyz:
        b.add("landmark_xyz", 24 * n)
    in_total = b.total
    b.add("result", 4 * n)
    b.add("f_cur", 24 * n)
    b.add("search_level", 4 * n)
    b.add("h_inv", 8 * n)
    b.add("A_cur_ref", 32 * n)
    b.add("success", n)
    end = b.add("n_success", 4)
    return b.done(in_total, b.off("type"), end)


def seed_batch(n, n_views, view_bytes, cur_idx=False, px_cur=False):
    """run_matcher, seed updates over host arrays (svoh_update_seeds_batch, ..._ex with outputs->px_cur)"""
    b = _Block()
    b.add("views", view_bytes * n_views)
    _feature_columns(b, n, cur_idx)
    b.add("state", 32 * n)
    in_total = b.total
    b.add("result", 4 * n)
    b.add("f_cur", 24 * n)
    b.add("search_level", 4 * n)
    b.add("h_inv", 8 * n)
    b.add("A_cur_ref", 32 * n)
    b.add("success", n)
    if px_cur:
        b.add("px_cur", 16 * n)
    end = b.add("n_success", 4)
    return b.done(in_total, b.off("type"), end)


def epipolar_batch(n, n_views, view_bytes, t_bytes=0, d_inv=False, cur_idx=False):
    """run_epipolar over host arrays; t_bytes = sizeof(Rigid) * n_ref_frames * n_cur_frames where T_cur_ref is given, else 0"""
    b = _Block()
    b.add("views", view_bytes * n_views)
    if t_bytes:
        b.add("T_cur_ref", t_bytes)
    _feature_columns(b, n, cur_idx)
    if d_inv:
        b.add("d_inv", 24 * n)
    in_total = b.total
    b.add("result", 4 * n)
    b.add("depth_out", 8 * n)
    b.add("px_cur", 16 * n)
    b.add("f_cur", 24 * n)
    b.add("search_level", 4 * n)
    b.add("h_inv", 8 * n)
    b.add("A_cur_ref", 32 * n)
    return b.done(in_total, b.off("result"), b.total)


def seed_chain(n, n_views, view_bytes, n_ref_frames, n_links, max_steps, step_result=False, step_success=False):
    """run_seed_chain; max_steps counts only where one of the step outputs is asked for"""
    n_steps_out = n * max_steps if (step_result or step_success) else 0
    b = _Block()
    b.add("views", view_bytes * n_views)
    b.add("chain_begin", 4 * (n_ref_frames + 1))
    b.add("chain_idx", 4 * n_links)
    _feature_columns(b, n, False)
    b.add("state", 32 * n)
    in_total = b.total
    b.add("steps_succeeded", 4 * n)
    if step_result:
        b.add("step_result", 4 * n_steps_out)
    if step_success:
        b.add("step_success", n_steps_out)
    return b.done(in_total, b.off("type"), b.total)


def matcher_stage(seeds, n, max_views, want_outputs, resident, view_bytes=DEV_FRAME_VIEW_BYTES):
    """layout_matcher_stage (svoh_matcher_stage); the resident form's px / f / grad / level lie behind n_success, on the device only"""
    want_outputs = want_outputs or not seeds
    b = _Block()
    b.add("views", view_bytes * max_views)
    b.add("ref_frame_idx", 4 * n)
    b.add("cur_frame_idx", 4 * n)
    if resident:
        b.add("feature_index", 4 * n)
    else:
        b.add("px", 16 * n)
        b.add("f", 24 * n)
        b.add("grad", 16 * n)
        b.add("level", 4 * n)
    if not seeds:
        b.add("depth", 8 * n)
    back_from = b.add("type", n)
    if seeds:
        b.add("state", 32 * n)
    else:
        b.add("px_cur", 16 * n)
    in_total = b.total
    b.add("result", 4 * n)
    b.add("success", n)
    if want_outputs:
        if seeds:
            b.add("px_cur", 16 * n)
        b.add("f_cur", 24 * n)
        b.add("search_level", 4 * n)
        b.add("h_inv", 8 * n)
        b.add("A_cur_ref", 32 * n)
    end = b.add("n_success", 4)
    if resident:
        b.add("px", 16 * n)
        b.add("f", 24 * n)
        b.add("grad", 16 * n)
        b.add("level", 4 * n)
    return b.done(in_total, back_from, end)


# the members of svoh_matcher_stage_t a staged block hands out: its columns but the view table, the count and, in the resident form,
# the four device-only columns
def matcher_stage_handed_out(seeds, n, max_views, want_outputs, resident):
    lay = matcher_stage(seeds, n, max_views, want_outputs, resident)
    hidden = {"views", "n_success"} | ({"px", "f", "grad", "level"} if resident else set())
    return {name: off for name, off in lay["cols"] if name not in hidden}
