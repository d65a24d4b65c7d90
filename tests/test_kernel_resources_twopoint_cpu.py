"""Register budget of the translation estimator's kernel (csrc/init.hip), read from the built object as
tests/test_kernel_resources_init_cpu.py reads the homography's: every hypothesis lives in registers, so a VGPR spill is a
defect, and the static LDS in front of the dynamic match columns must keep them 16-byte aligned."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svo_pro_universal_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "scripts"))


@pytest.fixture(scope="module")
def init_kernels():
    import kernel_resources_built as krb
    if not os.path.exists(os.path.join(CSRC, "init.o")):
        subprocess.check_call(["make", "-s", "-C", CSRC])
    return krb.kernels(os.path.join(CSRC, "init.o"))


def test_translation_ransac_kernel_budget(init_kernels):
    k = init_kernels["translation_ransac_kernel"]
    print(k)
    assert k["vgpr_spill"] == 0
    assert k["vgpr"] <= 256                 # 256 threads = one wave per SIMD: the whole register file of a lane is there
    assert k["lds"] % 16 == 0 and k["lds"] <= 1024   # static words only; the match columns are dynamic (72 bytes a match)
