"""Register / spill / scratch budget of the step kernel's instances, read from the code object of the built library
(tools/kernel_meta.py).  No GPU needed: the metadata is what the device compiler recorded.

The kernel is bound by vector issue with exactly two waves per SIMD, so what these numbers guard is instructions in the wave's own
stream: a spilled SGPR costs a v_readlane_b32 (plus its hazard slots) at every reload, scratch costs memory traffic, and a VGPR count
above the cap costs the second wave.  tools/isa_report.py shows where the reloads sit."""
import os
import re
import sys

import pytest

from rodent_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def step_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = [k for k in kernel_meta.kernels(hip.LIB_PATH) if "rr_step_kernel" in k["name"]]
    assert len(ks) >= 20, [k["name"] for k in ks]
    return ks


def _flags(name):
    """(NBS, NVS, NCS, PROF, DBG, fixed dims or None, NEWTON, UNROLL, ACTOR, PAIR, DYN) from the mangled instance name."""
    m = re.match(r"_Z14rr_step_kernelILi(\d)ELi(\d)ELi(\d)ELb(\d)ELb(\d)E(6RRDims|11RRDimsFixedILi(\d+)ELi(\d+)ELi(\d+)EE)"
                 r"Lb(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)EE", name)
    assert m, name
    g = m.groups()
    dims = None if g[5] == "6RRDims" else (int(g[6]), int(g[7]), int(g[8]))
    return (int(g[0]), int(g[1]), int(g[2]), g[3] == "1", g[4] == "1", dims) + tuple(x == "1" for x in g[9:14])


def test_no_instance_uses_scratch_or_spills_vgprs(step_kernels):
    for k in step_kernels:
        nbs = _flags(k["name"])[0]
        assert k["scratch"] == 0, (k["name"], k["scratch"])
        assert k["vgpr_spill"] == 0, (k["name"], k["vgpr_spill"])
        # two waves per SIMD need <= 256 registers (VGPRs + AGPRs, one unified file); the three-slot instances run one wave per SIMD
        cap = 512 if nbs == 3 else 256
        assert k["vgpr"] <= cap, (k["name"], k["vgpr"], cap)


# (UNROLL, ACTOR) -> SGPR spills of the fixed-dimension rodent instances (both RRDimsRodent and RRDimsRodentNew)
SGPR_SPILL_CAP = {
    (False, False): 67,      # single-step;                   parent: 110
    (True, False): 83,       # multi-step (the timed one);    parent: 163
    (True, True): 158,       # multi-step with the actor;     parent: 221
}


def test_sgpr_spills_of_the_fixed_dimension_instances(step_kernels):
    seen = set()
    for k in step_kernels:
        nbs, nvs, ncs, prof, dbg, dims, newton, unroll, actor, pair, dyn = _flags(k["name"])
        if dims is None or prof or dbg or pair:
            continue
        assert (nbs, nvs, ncs) == (2, 2, 1) and not newton and not dyn, k["name"]
        cap = SGPR_SPILL_CAP[(unroll, actor)]
        print(k["name"], "sgpr_spill", k["sgpr_spill"], "cap", cap)
        assert k["sgpr_spill"] <= cap, (k["name"], k["sgpr_spill"], cap)
        seen.add((dims, unroll, actor))
    assert len(seen) == 6, seen      # two models x three launch forms


def test_dims_and_tables_lie_where_the_kernel_rereads_them(step_kernels):
    """The kernel re-reads RRDims and RRTables through the kernarg segment pointer at offsetof(RRKArgs, D) = 0 and
    offsetof(RRKArgs, T) = sizeof(RRDims) rounded up to 8 (static_asserts in rr_kernel.h): the device compiler must have put
    the first two explicit arguments there, RRTables ending where the RRIO block begins (tests/test_abi_and_oracle.py checks that one)."""
    for k in step_kernels:
        explicit = [a for a in k["args"] if a[2] == "by_value"]
        assert len(explicit) == 5, k["name"]
        (d_off, d_size, _), (t_off, t_size, _), (io_off, _, _) = explicit[:3]
        assert d_off == 0, (k["name"], explicit)
        assert t_off == (d_size + 7) // 8 * 8, (k["name"], explicit)
        assert t_size == 22 * 8 and t_off + t_size == io_off, (k["name"], explicit)
