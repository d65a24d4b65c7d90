"""Budget of the 128-thread batch build of the alignment kernel (csrc/sparse_align.hip), read from the built object as
tests/test_kernel_resources_fivepoint_cpu.py reads the essential-matrix kernel's.  The build rests on FOUR workgroups per
compute unit: two waves per SIMD at 256 vector registers, and 40 KB of LDS per workgroup -- the static part plus the image area
launch_one grants (what a quarter of the compute unit's 160 KB leaves, at most the 24 576 bytes enqueue_align asks for).  A
fourth workgroup that does not fit would halve nothing visibly: every parity test stays green."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svo_pro_universal_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "scripts"))

LDS_PER_CU = 163840
LDS_IMG_REQUEST_128 = 24576      # enqueue_align, nt == 128
LEVEL2_IMAGE_640x480 = 19200     # what the half-level residency keeps of level 2
LEVELS_43_PAIR_640x480 = 12000


@pytest.fixture(scope="module")
def align128_kernels():
    import kernel_resources_built as krb
    obj = os.path.join(CSRC, "sparse_align.o")
    if not os.path.exists(obj):
        subprocess.check_call(["make", "-s", "-C", CSRC])
    ks = {n: k for n, k in krb.kernels(obj).items() if re.match(r"sparse_align_kernel<\d, 128,", n)}
    assert len(ks) == 8, sorted(ks)   # P 4 / 8 x illumination x robust weights
    return ks


def granted_image_area(static_lds):
    """launch_one for four workgroups per compute unit"""
    share = LDS_PER_CU // 4
    room = (share - static_lds) & ~15 if share > static_lds else 0
    return min(LDS_IMG_REQUEST_128 & ~15, room)


def test_four_workgroups_fit_a_compute_unit(align128_kernels):
    for name, k in sorted(align128_kernels.items()):
        area = granted_image_area(k["lds"])
        print("%-66s vgpr %3d (spilled %3d)  static lds %5d  image area %5d" % (name[:66], k["vgpr"], k["vgpr_spill"], k["lds"], area))
        assert k["vgpr"] <= 256, name                       # two waves per SIMD (512 registers a lane)
        # The grant is what the share leaves by construction, so the sum cannot exceed the share; what can go wrong is the STATIC part
        # growing until the grant no longer holds the residency the build is chosen for -- levels 4 and 3 of a 640x480 pair side by side,
        # one image of level 2 over them.  Stated on the static part directly: at most 40 960 - 19 200 = 21 760 bytes.
        assert k["lds"] <= LDS_PER_CU // 4 - max(LEVEL2_IMAGE_640x480, LEVELS_43_PAIR_640x480), name
        assert area >= LEVEL2_IMAGE_640x480 and area >= LEVELS_43_PAIR_640x480, name
