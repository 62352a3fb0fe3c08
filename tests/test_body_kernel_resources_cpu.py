"""Register / spill / scratch budget of the body-tracking instances of the step kernel (rr_body_kernel), read from the code object of
the built library (tools/kernel_meta.py).  No GPU needed.  The pose-termination instances' caps are
tests/test_poseterm_kernel_resources_cpu.py's."""
import os
import re
import sys

import pytest

from rodent_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def body_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    return [k for k in kernel_meta.kernels(hip.LIB_PATH) if "rr_body_kernel" in k["name"]]


def _flags(name):
    """(fixed dims or None, UNROLL, ACTOR) from the mangled instance name."""
    m = re.match(r"_Z14rr_body_kernelI(6RRDims|11RRDimsFixedILi(\d+)ELi(\d+)ELi(\d+)EE)Lb(\d)ELb(\d)EE", name)
    assert m, name
    g = m.groups()
    return (None if g[0] == "6RRDims" else (int(g[1]), int(g[2]), int(g[3])), g[4] == "1", g[5] == "1")


def test_nine_instances_three_dims_types_by_three_launch_forms(body_kernels):
    seen = {_flags(k["name"]) for k in body_kernels}
    assert len(body_kernels) == 9 and len(seen) == 9, [k["name"] for k in body_kernels]
    assert {f[0] for f in seen} == {None, (67, 57, 1279), (66, 59, 1263)}, seen        # generic and the two fixed-dimension types
    assert {(u, a) for _, u, a in seen} == {(False, False), (True, False), (True, True)}


def test_no_body_instance_uses_scratch_or_spills_vgprs(body_kernels):
    assert body_kernels
    for k in body_kernels:
        print(k["name"], "vgpr", k["vgpr"], "sgpr_spill", k["sgpr_spill"])
        assert k["scratch"] == 0, (k["name"], k["scratch"])
        assert k["vgpr_spill"] == 0, (k["name"], k["vgpr_spill"])
        assert k["vgpr"] <= 256, (k["name"], k["vgpr"])        # two waves per SIMD (VGPRs + AGPRs are one file of 512)
