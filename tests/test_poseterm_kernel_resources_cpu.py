"""Register / spill / scratch budget of the pose-termination instances of the step kernel (rr_poseterm_kernel), read from the code
object of the built library (tools/kernel_meta.py).  No GPU needed.  The reference-observation instances' caps are
tests/test_refobs_kernel_resources_cpu.py's, the pose instances' tests/test_pose_kernel_resources_cpu.py's."""
import os
import re
import sys

import pytest

from rodent_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def poseterm_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    return [k for k in kernel_meta.kernels(hip.LIB_PATH) if "rr_poseterm_kernel" in k["name"]]


def _flags(name):
    """(fixed dims or None, UNROLL, ACTOR) from the mangled instance name."""
    m = re.match(r"_Z18rr_poseterm_kernelI(6RRDims|11RRDimsFixedILi(\d+)ELi(\d+)ELi(\d+)EE)Lb(\d)ELb(\d)EE", name)
    assert m, name
    g = m.groups()
    return (None if g[0] == "6RRDims" else (int(g[1]), int(g[2]), int(g[3])), g[4] == "1", g[5] == "1")


def test_nine_instances_three_dims_types_by_three_launch_forms(poseterm_kernels):
    seen = {_flags(k["name"]) for k in poseterm_kernels}
    assert len(poseterm_kernels) == 9 and len(seen) == 9, [k["name"] for k in poseterm_kernels]
    assert {f[0] for f in seen} == {None, (67, 57, 1279), (66, 59, 1263)}, seen        # generic, rodent_optimized, rodent_new
    assert {(u, a) for _, u, a in seen} == {(False, False), (True, False), (True, True)}


def test_no_poseterm_instance_uses_scratch_or_spills_vgprs(poseterm_kernels):
    assert poseterm_kernels
    for k in poseterm_kernels:
        print(k["name"], "vgpr", k["vgpr"], "sgpr_spill", k["sgpr_spill"])
        assert k["scratch"] == 0, (k["name"], k["scratch"])
        assert k["vgpr_spill"] == 0, (k["name"], k["vgpr_spill"])
        assert k["vgpr"] <= 256, (k["name"], k["vgpr"])        # two waves per SIMD (VGPRs + AGPRs are one file of 512)
