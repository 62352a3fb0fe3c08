"""Register / spill / scratch budget of the pose family of the step kernel -- rr_pose_kernel (the pose block alone), rr_body_kernel
(with any of reference frames, pose termination and body tracking), rr_poseterm_kernel (pose termination without body tracking) and
rr_restart_kernel (with clip restarts) -- read from the code object of the built library (tools/kernel_meta.py).  No GPU needed.  The
caps of the rr_step_kernel instances are tests/test_kernel_resources_cpu.py's."""
import os
import re
import sys

import pytest

from rodent_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# entry -> the launch forms (UNROLL, ACTOR) it is compiled in; rr_restart_kernel has no single-step form and no UNROLL argument
FORMS = {"rr_pose_kernel": {(False, False), (True, False), (True, True)},
         "rr_poseterm_kernel": {(False, False), (True, False), (True, True)},
         "rr_body_kernel": {(False, False), (True, False), (True, True)},
         "rr_restart_kernel": {(True, False), (True, True)}}
RETIRED = ("rr_refobs_kernel",)      # rr_body_kernel serves its launches


@pytest.fixture(scope="module")
def all_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    return kernel_meta.kernels(hip.LIB_PATH)


def _flags(entry, name):
    """(fixed dims or None, UNROLL, ACTOR) from the mangled instance name."""
    m = re.match(r"_Z%d%sI(6RRDims|11RRDimsFixedILi(\d+)ELi(\d+)ELi(\d+)EE)((?:Lb\dE)+)E" % (len(entry), entry), name)
    assert m, name
    g = m.groups()
    bools = [b == "1" for b in re.findall(r"Lb(\d)E", g[4])]
    assert len(bools) == (1 if entry == "rr_restart_kernel" else 2), name
    unroll, actor = (True, bools[0]) if entry == "rr_restart_kernel" else bools
    return (None if g[0] == "6RRDims" else (int(g[1]), int(g[2]), int(g[3])), unroll, actor)


@pytest.mark.parametrize("entry", sorted(FORMS))
def test_instances_three_dims_types_by_the_launch_forms(all_kernels, entry):
    ks = [k for k in all_kernels if entry in k["name"]]
    seen = {_flags(entry, k["name"]) for k in ks}
    n = {"rr_pose_kernel": 9, "rr_poseterm_kernel": 9, "rr_body_kernel": 9, "rr_restart_kernel": 6}[entry]
    assert len(ks) == n and len(seen) == n, [k["name"] for k in ks]
    assert {f[0] for f in seen} == {None, (67, 57, 1279), (66, 59, 1263)}, seen        # generic and the two fixed-dimension types
    assert {(u, a) for _, u, a in seen} == FORMS[entry]


@pytest.mark.parametrize("entry", sorted(FORMS))
def test_no_instance_uses_scratch_or_spills_vgprs(all_kernels, entry):
    ks = [k for k in all_kernels if entry in k["name"]]
    assert ks
    for k in ks:
        print(k["name"], "vgpr", k["vgpr"], "sgpr_spill", k["sgpr_spill"])
        assert k["scratch"] == 0, (k["name"], k["scratch"])
        assert k["vgpr_spill"] == 0, (k["name"], k["vgpr_spill"])
        if entry == "rr_restart_kernel":
            assert k["lds"] == 0, (k["name"], k["lds"])             # no static LDS: the level schedules address the dynamic segment from 0
        assert k["vgpr"] <= 256, (k["name"], k["vgpr"])        # two waves per SIMD (VGPRs + AGPRs are one file of 512)


def test_the_family_is_four_entries_and_the_retired_one_is_gone(all_kernels):
    names = [k["name"] for k in all_kernels]
    assert not [n for n in names if any(r in n for r in RETIRED)]
    assert len([n for n in names if any(e in n for e in FORMS)]) == 33
