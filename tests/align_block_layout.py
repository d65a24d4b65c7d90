"""The alignment's staged block and feature workspace, restated in plain Python from the launch code as it stood before
csrc/svoh_align_block.h described them once (enqueue_align / run_align_wide / fetch_evaluation of csrc/sparse_align.hip wrote the
offsets out by hand).  Not generated from the header: tests/test_align_block_cpu.py holds the header's output against this.

    [P*S problem descriptors | P*C*S camera descriptors | 256-aligned: 512 control bytes (queue head; arrival counters at +256) |
     per camera with features: px 16n, f 24n, pos_world 24n, flags n, together rounded up to 64; behind it, if the camera has
     pos_seed_unit, its units, 4n rounded up to 64 | the job table, 24 bytes per such camera, rounded up to 64]
"""

PROBLEM_DESC_BYTES = 192   # sizeof(DevProblemDesc)
CAM_DESC_BYTES = 696       # sizeof(DevCamDesc)
POS_JOB_BYTES = 24         # sizeof(PosFromSeedsJob)
WS_PAIRS = 3               # kWsPairs


def _up64(b):
    return (b + 63) & ~63


def block(problems, cams, n, shares, units):
    """problems x cams cameras of n features each, every problem spread over `shares` descriptors; units: every camera has
    pos_seed_unit.  Offsets are relative to the block."""
    n_desc = problems * shares
    n_cams_total = problems * cams * shares
    # pass 1 (sizes): what both buffers are asked to hold
    host_bytes = 0
    for _ in range(problems * cams):
        host_bytes += (n * (8 * 8 + 1) + 63) & ~63
        if units:
            host_bytes += ((n * 4 + 63) & ~63) + 64
    desc_only = PROBLEM_DESC_BYTES * n_desc + CAM_DESC_BYTES * n_cams_total
    ctl_off = (desc_only + 255) & ~255
    up_base = ctl_off + 512
    out = dict(cams_off=PROBLEM_DESC_BYTES * n_desc, ctl_off=ctl_off, bar_off=ctl_off + 256, up_base=up_base, reserve=up_base + host_bytes,
               cam=[], units=[], share=[], jobs=None)
    # pass 2 (fill): a camera's arrays go up once, every share points into them
    up_off = 0
    n_jobs = 0
    for k in range(problems * cams):
        if n == 0:
            continue
        base = up_base + up_off
        out["cam"].append((k, base, base + n * 16, base + n * 40, base + n * 64, (n * 65 + 63) & ~63))
        up_off += (n * 65 + 63) & ~63
        if units:
            out["units"].append((k, up_base + up_off))
            up_off += (n * 4 + 63) & ~63
            n_jobs += 1
        for s in range(shares):
            lo, hi = n * s // shares, n * (s + 1) // shares
            out["share"].append((k, s, hi - lo, base + 16 * lo, base + n * 16 + 24 * lo, base + n * 40 + 24 * lo, base + n * 64 + lo))
    if n_jobs:
        out["jobs"] = up_base + up_off
        up_off += _up64(POS_JOB_BYTES * n_jobs)
    out["used"] = up_base + up_off
    return out


def workspace(n_features):
    """the per-feature workspace of a launch: rows, the two byte masks an evaluation reads back, and 256 bytes"""
    slots = n_features if n_features else 1
    wsel = 2 * WS_PAIRS * slots * 8      # behind the rows: 2 * kWsPairs * slots doubles
    return dict(slots=slots, wpk=0, wsel=wsel, wvis=wsel + slots, bytes=slots * (WS_PAIRS * 16 + 2) + 256)
