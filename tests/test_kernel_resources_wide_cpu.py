"""Register budgets of the wide camera family's kernels (svoh_math.h, CamModelWide), read from the built objects as
tests/test_kernel_resources_cpu.py reads the narrow ones.  The wide models bring atan / tan / sqrt into the projection;
they are compiled into kernels of their own, so the narrow kernels keep their names and figures."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svo_pro_universal_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "scripts"))


@pytest.fixture(scope="module")
def context_kernels():
    import kernel_resources_built as krb
    if not os.path.exists(os.path.join(CSRC, "context.o")):
        subprocess.check_call(["make", "-s", "-C", CSRC])
    return krb.kernels(os.path.join(CSRC, "context.o"))


def test_camera_maths_wide_kernel_has_its_own_name(context_kernels):
    assert "camera_maths_kernel" in context_kernels           # the narrow entry, unchanged
    assert "camera_maths_wide_kernel" in context_kernels


def test_camera_maths_wide_kernel_budget(context_kernels):
    narrow, wide = context_kernels["camera_maths_kernel"], context_kernels["camera_maths_wide_kernel"]
    assert wide["vgpr_spill"] <= narrow["vgpr_spill"] == 0
    assert wide["lds"] == 0 and wide["vgpr"] <= 64      # a 64-thread diagnostic entry: no reason to grow past that
