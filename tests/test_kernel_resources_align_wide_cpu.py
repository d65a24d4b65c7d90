"""Register budgets of the alignment's wide twins (sparse_align.hip, sparse_align_wide_kernel<P, ILLUM, ROBUST>), read from the
built sparse_align.o as tests/test_kernel_resources_matcher_wide_cpu.py reads matcher.o.  The camera-dependent device functions
became templates on the camera type and the kernel's body is shared with the twin; the narrow kernels must be the code they
were.  A twin runs ONE geometry -- 512 threads, a lane per patch -- and has the LDS of its narrow counterpart there,
sparse_align_kernel<P, 512, ILLUM, false, ROBUST, 1, false, false>; what it spills beside the counterpart is printed here and
stated in DESIGN.md 4.1."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svo_pro_universal_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "scripts"))

# name -> (vgpr, vgpr_spill, lds) of every kernel of sparse_align.o at commit 9623a06 (the parent of the change that added the
# twins), from scripts/kernel_resources_built.py on that commit's build
NARROW_AT_9623A06 = {
    "align_gn_update_kernel<4, false>": (196, 0, 2008),
    "align_gn_update_kernel<4, true>": (248, 0, 2008),
    "align_gn_update_kernel<8, false>": (196, 0, 2008),
    "align_gn_update_kernel<8, true>": (248, 0, 2008),
    "sparse_align_kernel<4, 128, false, false, false, 1, false, false>": (256, 52, 16208),
    "sparse_align_kernel<4, 128, false, false, true, 1, false, false>": (256, 29, 15952),
    "sparse_align_kernel<4, 128, true, false, false, 1, false, false>": (256, 83, 16480),
    "sparse_align_kernel<4, 128, true, false, true, 1, false, false>": (256, 107, 16224),
    "sparse_align_kernel<4, 256, false, false, false, 1, false, false>": (256, 49, 28944),
    "sparse_align_kernel<4, 256, false, false, false, 1, true, false>": (272, 0, 28560),
    "sparse_align_kernel<4, 256, false, false, false, 1, true, true>": (274, 0, 28560),
    "sparse_align_kernel<4, 256, false, false, true, 1, false, false>": (256, 27, 28688),
    "sparse_align_kernel<4, 256, false, false, true, 1, true, false>": (262, 0, 28304),
    "sparse_align_kernel<4, 256, false, false, true, 1, true, true>": (265, 0, 28304),
    "sparse_align_kernel<4, 256, false, true, false, 1, false, false>": (256, 27, 29072),
    "sparse_align_kernel<4, 256, false, true, true, 1, false, false>": (256, 17, 28816),
    "sparse_align_kernel<4, 256, true, false, false, 1, false, false>": (256, 80, 29488),
    "sparse_align_kernel<4, 256, true, false, false, 1, true, false>": (300, 0, 29104),
    "sparse_align_kernel<4, 256, true, false, false, 1, true, true>": (302, 0, 29104),
    "sparse_align_kernel<4, 256, true, false, true, 1, false, false>": (256, 95, 29232),
    "sparse_align_kernel<4, 256, true, false, true, 1, true, false>": (308, 0, 28848),
    "sparse_align_kernel<4, 256, true, false, true, 1, true, true>": (308, 0, 28848),
    "sparse_align_kernel<4, 256, true, true, false, 1, false, false>": (256, 66, 29616),
    "sparse_align_kernel<4, 256, true, true, true, 1, false, false>": (256, 73, 29360),
    "sparse_align_kernel<4, 512, false, false, false, 1, false, false>": (256, 33, 4880),
    "sparse_align_kernel<4, 512, false, false, false, 1, false, true>": (256, 33, 4880),
    "sparse_align_kernel<4, 512, false, false, false, 2, false, false>": (256, 22, 4880),
    "sparse_align_kernel<4, 512, false, false, false, 4, false, false>": (256, 19, 4880),
    "sparse_align_kernel<4, 512, false, false, true, 1, false, false>": (256, 14, 4624),
    "sparse_align_kernel<4, 512, false, false, true, 1, false, true>": (256, 14, 4624),
    "sparse_align_kernel<4, 512, false, false, true, 2, false, false>": (256, 15, 4624),
    "sparse_align_kernel<4, 512, false, false, true, 4, false, false>": (256, 21, 4624),
    "sparse_align_kernel<4, 512, true, false, false, 1, false, false>": (256, 57, 5968),
    "sparse_align_kernel<4, 512, true, false, false, 1, false, true>": (256, 67, 5968),
    "sparse_align_kernel<4, 512, true, false, false, 2, false, false>": (256, 61, 5968),
    "sparse_align_kernel<4, 512, true, false, false, 4, false, false>": (256, 31, 5968),
    "sparse_align_kernel<4, 512, true, false, true, 1, false, false>": (256, 68, 5712),
    "sparse_align_kernel<4, 512, true, false, true, 1, false, true>": (256, 75, 5712),
    "sparse_align_kernel<4, 512, true, false, true, 2, false, false>": (256, 75, 5712),
    "sparse_align_kernel<4, 512, true, false, true, 4, false, false>": (256, 29, 5712),
    "sparse_align_kernel<8, 128, false, false, false, 1, false, false>": (256, 77, 16208),
    "sparse_align_kernel<8, 128, false, false, true, 1, false, false>": (256, 55, 15952),
    "sparse_align_kernel<8, 128, true, false, false, 1, false, false>": (256, 205, 16480),
    "sparse_align_kernel<8, 128, true, false, true, 1, false, false>": (256, 156, 16224),
    "sparse_align_kernel<8, 256, false, false, false, 1, false, false>": (256, 75, 28944),
    "sparse_align_kernel<8, 256, false, false, false, 1, true, false>": (288, 0, 28560),
    "sparse_align_kernel<8, 256, false, false, false, 1, true, true>": (294, 0, 28560),
    "sparse_align_kernel<8, 256, false, false, true, 1, false, false>": (256, 49, 28688),
    "sparse_align_kernel<8, 256, false, false, true, 1, true, false>": (272, 0, 28304),
    "sparse_align_kernel<8, 256, false, false, true, 1, true, true>": (274, 0, 28304),
    "sparse_align_kernel<8, 256, false, true, false, 1, false, false>": (256, 60, 29072),
    "sparse_align_kernel<8, 256, false, true, true, 1, false, false>": (256, 28, 28816),
    "sparse_align_kernel<8, 256, true, false, false, 1, false, false>": (256, 156, 29488),
    "sparse_align_kernel<8, 256, true, false, false, 1, true, false>": (340, 0, 29104),
    "sparse_align_kernel<8, 256, true, false, false, 1, true, true>": (344, 0, 29104),
    "sparse_align_kernel<8, 256, true, false, true, 1, false, false>": (256, 133, 29232),
    "sparse_align_kernel<8, 256, true, false, true, 1, true, false>": (318, 0, 28848),
    "sparse_align_kernel<8, 256, true, false, true, 1, true, true>": (322, 0, 28848),
    "sparse_align_kernel<8, 256, true, true, false, 1, false, false>": (256, 153, 29616),
    "sparse_align_kernel<8, 256, true, true, true, 1, false, false>": (256, 111, 29360),
    "sparse_align_kernel<8, 512, false, false, false, 1, false, false>": (256, 47, 4880),
    "sparse_align_kernel<8, 512, false, false, false, 1, false, true>": (256, 49, 4880),
    "sparse_align_kernel<8, 512, false, false, false, 2, false, false>": (256, 52, 4880),
    "sparse_align_kernel<8, 512, false, false, false, 4, false, false>": (256, 35, 4880),
    "sparse_align_kernel<8, 512, false, false, false, 8, false, false>": (256, 22, 4880),
    "sparse_align_kernel<8, 512, false, false, true, 1, false, false>": (256, 24, 4624),
    "sparse_align_kernel<8, 512, false, false, true, 1, false, true>": (256, 29, 4624),
    "sparse_align_kernel<8, 512, false, false, true, 2, false, false>": (256, 31, 4624),
    "sparse_align_kernel<8, 512, false, false, true, 4, false, false>": (256, 23, 4624),
    "sparse_align_kernel<8, 512, false, false, true, 8, false, false>": (256, 60, 4624),
    "sparse_align_kernel<8, 512, true, false, false, 1, false, false>": (256, 133, 5968),
    "sparse_align_kernel<8, 512, true, false, false, 1, false, true>": (256, 145, 5968),
    "sparse_align_kernel<8, 512, true, false, false, 2, false, false>": (256, 80, 5968),
    "sparse_align_kernel<8, 512, true, false, false, 4, false, false>": (256, 80, 5968),
    "sparse_align_kernel<8, 512, true, false, false, 8, false, false>": (256, 55, 5968),
    "sparse_align_kernel<8, 512, true, false, true, 1, false, false>": (256, 101, 5712),
    "sparse_align_kernel<8, 512, true, false, true, 1, false, true>": (256, 114, 5712),
    "sparse_align_kernel<8, 512, true, false, true, 2, false, false>": (256, 101, 5712),
    "sparse_align_kernel<8, 512, true, false, true, 4, false, false>": (256, 95, 5712),
    "sparse_align_kernel<8, 512, true, false, true, 8, false, false>": (256, 136, 5712),
    "sum_shares_kernel": (8, 0, 0),
}


def twins():
    """twin -> its narrow counterpart"""
    out = {}
    for P in (4, 8):
        for illum in ("false", "true"):
            for robust in ("false", "true"):
                out["sparse_align_wide_kernel<%d, %s, %s>" % (P, illum, robust)] = \
                    "sparse_align_kernel<%d, 512, %s, false, %s, 1, false, false>" % (P, illum, robust)
    return out


@pytest.fixture(scope="module")
def align_kernels():
    import kernel_resources_built as krb
    if not os.path.exists(os.path.join(CSRC, "sparse_align.o")):
        subprocess.check_call(["make", "-s", "-C", CSRC])
    return krb.kernels(os.path.join(CSRC, "sparse_align.o"))


def test_narrow_kernels_keep_their_names_and_figures(align_kernels):
    for name, want in NARROW_AT_9623A06.items():
        assert name in align_kernels, name
        k = align_kernels[name]
        assert (k["vgpr"], k["vgpr_spill"], k["lds"]) == want, (name, k, want)


def test_the_object_holds_exactly_the_eight_twins_beside_the_parents_set(align_kernels):
    assert len(twins()) == 8
    assert set(align_kernels) == set(NARROW_AT_9623A06) | set(twins())
    # no twin carries the narrow kernel's name prefix (the existing resource tests select by it)
    assert sum(1 for n in align_kernels if n.startswith("sparse_align_kernel<")) == sum(1 for n in NARROW_AT_9623A06 if n.startswith("sparse_align_kernel<"))
    assert len([n for n in align_kernels if re.match(r"sparse_align_kernel<\d, 128,", n)]) == 8


def test_twins_fit_the_register_file_and_have_their_counterparts_lds(align_kernels):
    for twin, narrow in sorted(twins().items()):
        t, n = align_kernels[twin], align_kernels[narrow]
        print("%-44s vgpr %3d spill %3d scratch %4d lds %5d   |   counterpart: vgpr %3d spill %3d scratch %4d lds %5d" % (
            twin, t["vgpr"], t["vgpr_spill"], t["scratch"], t["lds"], n["vgpr"], n["vgpr_spill"], n["scratch"], n["lds"]))
        assert t["vgpr"] <= 256, (twin, t)          # two waves per SIMD (512 threads on four SIMDs)
        assert t["lds"] == n["lds"], (twin, t, n)
