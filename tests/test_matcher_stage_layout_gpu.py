"""svoh_matcher_stage's block as the public ABI shows it: the distances between the pointers it hands out are those of
tests/matcher_block_layout.py (the restated layout: column order, round-up to 64), and the members a form does not have are NULL --
for both kinds, all four flag combinations, at unit counts where the 1-byte and 4-byte columns end inside, on and behind a
64-byte boundary, with a small and a larger view table."""
import ctypes as C

import pytest

from svo_pro_universal_amd import _capi as capi

import matcher_block_layout as mbl

pytestmark = pytest.mark.gpu

MEMBERS = [k for k, _ in capi.svoh_matcher_stage_t._fields_]


@pytest.mark.parametrize("seeds", [0, 1])
@pytest.mark.parametrize("flags", [0, capi.SVOH_STAGE_MATCH_OUTPUTS, capi.SVOH_STAGE_RESIDENT_COLUMNS,
                                   capi.SVOH_STAGE_MATCH_OUTPUTS | capi.SVOH_STAGE_RESIDENT_COLUMNS])
def test_the_pointers_handed_out_lie_as_restated(gpu_ctx, seeds, flags):
    ctx = gpu_ctx
    outputs, resident = bool(flags & capi.SVOH_STAGE_MATCH_OUTPUTS), bool(flags & capi.SVOH_STAGE_RESIDENT_COLUMNS)
    for n in (1, 17, 65):
        for max_views in (2, 5):
            want = mbl.matcher_stage_handed_out(bool(seeds), n, max_views, outputs, resident)
            ctx._check(ctx.lib.svoh_matcher_begin_deferred(ctx.h))
            try:
                g = capi.svoh_matcher_stage_t()
                ctx._check(ctx.lib.svoh_matcher_stage(ctx.h, seeds, n, max_views, flags, C.byref(g)))
                got = {k: getattr(g, k) for k in MEMBERS}
            finally:
                ctx._check(ctx.lib.svoh_matcher_collect(ctx.h))
            case = dict(seeds=seeds, flags=flags, n=n, max_views=max_views)
            assert {k for k in MEMBERS if got[k]} == set(want), case
            base = got["ref_frame_idx"] - want["ref_frame_idx"]   # where the block begins: its view table
            assert base % 64 == 0, case
            assert {k: got[k] - base for k in want} == want, case
