"""Register budgets of the matcher's wide twins (matcher.hip, *_wide_kernel), read from the built matcher.o as
tests/test_kernel_resources_wide_cpu.py reads context.o.  The device functions became templates on the view's camera type;
the narrow kernels must be the code they were, and a twin is instantiated only in a geometry where it spills no more
VGPRs than its narrow counterpart and uses the same LDS."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svo_pro_universal_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "scripts"))

# name -> (vgpr, vgpr_spill, lds) of every kernel of matcher.o at commit e0f1f66 (the parent of the change that added the
# twins), from scripts/kernel_resources_built.py on that commit's build
NARROW_AT_E0F1F66 = {
    "seed_bin_count_kernel": (10, 0, 0),
    "seed_bin_scan_kernel": (14, 0, 4096),
    "seed_unsort_kernel": (26, 0, 0),
    "count_success_kernel": (6, 0, 0),
    "project_candidates_kernel": (52, 0, 0),
    "project_candidates_wide_kernel": (64, 0, 0),
    "project_candidates_multi_kernel": (74, 0, 0),
    "project_candidates_multi_wide_kernel": (86, 0, 0),
    "select_matches_kernel": (16, 0, 1036),
    "project_candidates_ranges_kernel": (80, 0, 0),
    "project_candidates_ranges_wide_kernel": (86, 0, 0),
    "matcher_prologue_kernel": (48, 0, 0),
    "pos_from_seed_batch_kernel": (46, 0, 0),
    "seed_bin_scatter_kernel<true>": (44, 0, 33792),
    "seed_bin_scatter_kernel<false>": (36, 0, 0),
    "update_seeds_kernel<3>": (178, 0, 6400),
    "update_seeds_kernel<1>": (238, 0, 6400),
    "update_seeds_kernel<0>": (238, 0, 6400),
    "match_direct_kernel<true>": (146, 0, 6400),
    "match_direct_kernel<false>": (216, 0, 6400),
    "epipolar_match_kernel<3>": (158, 0, 6400),
    "epipolar_match_kernel<1>": (206, 0, 6400),
    "epipolar_match_kernel<0>": (225, 0, 6400),
    "update_seeds_chain_kernel<3>": (256, 0, 6400),
    "update_seeds_chain_kernel<0>": (293, 0, 6400),
    "update_seeds_chain_kernel<1>": (326, 12, 6400),
    "match_mixed_kernel<true>": (240, 0, 6400),
    "match_mixed_kernel<false>": (239, 0, 6400),
    "update_seeds_packed_kernel<false>": (168, 1, 51232),
    "update_seeds_packed_kernel<true>": (168, 5, 51232),
    "match_packed_kernel<true>": (168, 16, 51232),
    "match_packed_kernel<false>": (168, 25, 51232),
}

# twin -> its narrow counterpart in the same geometry: eight lanes per unit (seed update), one lane per unit (direct
# matcher, both warps), one wave per unit (stereo seam)
TWINS = {
    "update_seeds_wide_kernel<1>": "update_seeds_kernel<1>",
    "match_direct_wide_kernel<false>": "match_direct_kernel<false>",
    "epipolar_match_wide_kernel<3>": "epipolar_match_kernel<3>",
}


@pytest.fixture(scope="module")
def matcher_kernels():
    import kernel_resources_built as krb
    if not os.path.exists(os.path.join(CSRC, "matcher.o")):
        subprocess.check_call(["make", "-s", "-C", CSRC])
    return krb.kernels(os.path.join(CSRC, "matcher.o"))


def test_narrow_kernels_keep_their_names_and_figures(matcher_kernels):
    for name, want in NARROW_AT_E0F1F66.items():
        assert name in matcher_kernels, name
        k = matcher_kernels[name]
        assert (k["vgpr"], k["vgpr_spill"], k["lds"]) == want, (name, k)


def test_every_other_kernel_of_the_object_is_a_twin(matcher_kernels):
    assert set(matcher_kernels) - set(NARROW_AT_E0F1F66) == set(TWINS)      # one geometry per entry, nothing else new


@pytest.mark.parametrize("twin", sorted(TWINS))
def test_twin_budget(matcher_kernels, twin):
    wide, narrow = matcher_kernels[twin], matcher_kernels[TWINS[twin]]
    assert wide["vgpr_spill"] <= narrow["vgpr_spill"]
    assert wide["lds"] == narrow["lds"]
