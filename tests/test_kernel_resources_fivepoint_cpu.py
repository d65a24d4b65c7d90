"""Register budget of the essential-matrix estimator's kernel (csrc/essential.hip), read from the built object as
tests/test_kernel_resources_twopoint_cpu.py reads the translation's: a candidate's motion lives in registers while it is
scored, so a VGPR spill is a defect, and the static LDS in front of the dynamic match columns must keep them
16-byte aligned.  The solver's working set is private memory by design; its size is printed."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svo_pro_universal_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "scripts"))


@pytest.fixture(scope="module")
def essential_kernels():
    import kernel_resources_built as krb
    if not os.path.exists(os.path.join(CSRC, "essential.o")):
        subprocess.check_call(["make", "-s", "-C", CSRC])
    return krb.kernels(os.path.join(CSRC, "essential.o"))


def test_essential_ransac_kernel_budget(essential_kernels):
    k = essential_kernels["essential_ransac_kernel"]
    print(k)
    print("private segment of essential_ransac_kernel: %d bytes a lane" % k["scratch"])
    assert k["vgpr_spill"] == 0
    assert k["vgpr"] <= 256                 # 256 threads = one wave per SIMD; accumulation registers count (they would be spills)
    assert k["lds"] % 16 == 0 and k["lds"] <= 1024   # static words only; the match columns are dynamic (48 bytes a match)
