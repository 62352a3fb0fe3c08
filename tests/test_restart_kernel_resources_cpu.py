"""Register / spill / scratch budget of the clip-restart instances of the step kernel (rr_restart_kernel), read from the code object of
the built library (tools/kernel_meta.py).  No GPU needed.  The body-tracking instances' caps are tests/test_body_kernel_resources_cpu.py's."""
import os
import re
import sys

import pytest

from rodent_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def restart_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    return [k for k in kernel_meta.kernels(hip.LIB_PATH) if "rr_restart_kernel" in k["name"]]


def _flags(name):
    """(fixed dims or None, ACTOR) from the mangled instance name."""
    m = re.match(r"_Z17rr_restart_kernelI(6RRDims|11RRDimsFixedILi(\d+)ELi(\d+)ELi(\d+)EE)Lb(\d)EE", name)
    assert m, name
    g = m.groups()
    return (None if g[0] == "6RRDims" else (int(g[1]), int(g[2]), int(g[3])), g[4] == "1")


def test_six_instances_three_dims_types_by_two_multi_step_forms(restart_kernels):
    seen = {_flags(k["name"]) for k in restart_kernels}
    assert len(restart_kernels) == 6 and len(seen) == 6, [k["name"] for k in restart_kernels]
    assert {f[0] for f in seen} == {None, (67, 57, 1279), (66, 59, 1263)}, seen        # generic and the two fixed-dimension types
    assert {a for _, a in seen} == {False, True}                                        # without and with the actor; no single-step form


def test_no_restart_instance_uses_scratch_or_spills_vgprs(restart_kernels):
    assert restart_kernels
    for k in restart_kernels:
        print(k["name"], "vgpr", k["vgpr"], "sgpr_spill", k["sgpr_spill"])
        assert k["scratch"] == 0, (k["name"], k["scratch"])
        assert k["vgpr_spill"] == 0, (k["name"], k["vgpr_spill"])
        assert k["lds"] == 0, (k["name"], k["lds"])             # no static LDS: the level schedules address the dynamic segment from 0
        assert k["vgpr"] <= 256, (k["name"], k["vgpr"])        # two waves per SIMD (VGPRs + AGPRs are one file of 512)
