"""The root body in a body slot of its own (rr_kernel.h RR_ROOT_SLOT), as far as it can be seen without a GPU: the comparison arm
rr_twoslot_kernel is in the built library's code object within the step kernel's register budget, the C ABI switch is exported and
mirrored, the switch is refused in words for a model that has no such instance, and the rule by which the host decides that a model may
run the root-slot tree phases holds for rodent_optimized and fails for rodent_new, read from the blobs themselves."""
import ctypes
import os
import sys

import numpy as np
import pytest

from rodent_amd import assets, hip, mjcf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES = 64
REFUSAL = "rr_batch_set_root_slot: only the fixed-dimension CG instance of the rodent_optimized model"


def test_the_plain_map_arm_is_in_the_code_object_within_budget():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = [k for k in kernel_meta.kernels(hip.LIB_PATH) if "rr_twoslot_kernel" in k["name"]]
    assert len(ks) == 1, [k["name"] for k in ks]
    k = ks[0]
    print(k["name"], "vgpr", k["vgpr"], "sgpr spills", k["sgpr_spill"])
    assert "rr_step_kernel" not in k["name"]      # tests/test_kernel_resources_cpu.py parses the names that hold it
    assert "RRDimsFixedILi66ELi59ELi1263EE" in k["name"]      # RRDimsRodent
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0
    assert k["vgpr"] <= 256      # VGPRs + AGPRs, one unified file: two waves per SIMD
    assert k["lds"] == 0         # the level schedules need the dynamic segment at LDS address 0


def test_switch_is_exported_and_mirrored():
    lib = ctypes.CDLL(hip.LIB_PATH)
    for sym in ("rr_batch_set_root_slot", "rr_model_root_slot_switch"):
        assert sym in hip.EXPORTS
        getattr(lib, sym)
    assert callable(hip.Batch.set_root_slot)
    with open(os.path.join(ROOT, "include", "rodent_rr.h")) as f:
        header = f.read()
    assert "int rr_batch_set_root_slot(rr_batch* b, int32_t enable);" in header
    assert "int rr_model_root_slot_switch(const rr_model* m);" in header
    # a null batch is an error with words, not a crash
    assert hip.lib().rr_batch_set_root_slot(None, 0) < 0
    assert b"rr_batch_set_root_slot: null batch" in hip.lib().rr_last_error()


@pytest.mark.parametrize("blob, solver", [("rodent_new", "cg"), ("rodent_cpu", "cg"), ("rodent_optimized", "newton")])
def test_switch_is_refused_in_words_for_other_models(blob, solver):
    m = hip.Model(assets.asset_path(blob), 8, 8, solver=solver)
    with pytest.raises(RuntimeError, match=REFUSAL):
        m.check_root_slot_switch()


def test_switch_is_accepted_for_the_benchmark_model():
    hip.Model(assets.asset_path("rodent_optimized"), 8, 8, solver="cg").check_root_slot_switch()


def _qualifies(m):
    """The rule of rr_api.hip root_slot_ok on the model's own arrays: one tree; body 1 is the child of the world and holds the only free
    joint; at most two bodies beyond the 64 lanes."""
    nbody = int(m["nbody"])
    free = np.flatnonzero(m["jnt_type"] == 0)
    one_tree = len(m["k_root_mass"]) == 1 and bool((m["body_parentid"][2:] >= 1).all())
    return bool(one_tree and m["body_parentid"][1] == 0 and len(free) == 1 and m["jnt_bodyid"][free[0]] == 1 and 2 <= nbody and nbody - LANES <= 2)


def test_qualification_rule_from_the_blobs():
    opt = mjcf.load_blob(assets.asset_path("rodent_optimized"))
    new = mjcf.load_blob(assets.asset_path("rodent_new"))
    assert _qualifies(opt)
    assert not _qualifies(new)
    # rodent_optimized: 66 bodies, one free joint, on body 1, whose parent is the world
    free = np.flatnonzero(opt["jnt_type"] == 0)
    assert int(opt["nbody"]) == 66
    assert len(free) == 1 and int(opt["jnt_bodyid"][free[0]]) == 1 and int(opt["body_parentid"][1]) == 0
    # what the root's slot takes for granted instead of reading tables: the joint is qpos[0 .. 6], the dofs 0 .. 5, the subtree every body
    assert int(opt["jnt_qposadr"][free[0]]) == 0 and int(opt["jnt_dofadr"][free[0]]) == 0
    assert int(opt["body_dofadr"][1]) == 0 and int(opt["body_dofnum"][1]) == 6 and int(opt["k_body_i"][1][10]) == 65
    # the bodies that move to lanes 0 and 1 of the first slot are the last two links of a chain, one hinge each
    assert [int(opt["body_parentid"][b]) for b in (64, 65)] == [63, 64] and [int(opt["body_jntnum"][b]) for b in (64, 65)] == [1, 1]
    # rodent_new fails on the body count alone: 67 bodies are three beyond the lanes
    assert int(new["nbody"]) == 67
