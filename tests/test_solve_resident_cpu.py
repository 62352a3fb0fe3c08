"""The A/B arm of the resident inverse-factor entries (rr_kernel.h RR_SOLVE_MAT_RESIDENT), as far as it can be seen without a GPU: the
extra entry point rr_matlds_kernel is in the built library's code object within the step kernel's register budget, the C ABI switch is
exported and mirrored, and the switch is refused in words for a model the entry point is not built for."""
import ctypes
import os
import sys

import pytest

from rodent_amd import assets, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_lds_arm_is_in_the_code_object_within_budget():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = [k for k in kernel_meta.kernels(hip.LIB_PATH) if "rr_matlds_kernel" in k["name"]]
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
    for sym in ("rr_batch_set_solve_resident", "rr_model_solve_resident_switch"):
        assert sym in hip.EXPORTS
        getattr(lib, sym)
    assert callable(hip.Batch.set_solve_resident)
    with open(os.path.join(ROOT, "include", "rodent_rr.h")) as f:
        header = f.read()
    assert "int rr_batch_set_solve_resident(rr_batch* b, int32_t enable);" in header
    # a null batch is an error with words, not a crash
    assert hip.lib().rr_batch_set_solve_resident(None, 0) < 0
    assert b"rr_batch_set_solve_resident: null batch" in hip.lib().rr_last_error()


@pytest.mark.parametrize("blob, solver", [("rodent_new", "cg"), ("rodent_cpu", "cg"), ("rodent_optimized", "newton")])
def test_switch_is_refused_in_words_for_other_models(blob, solver):
    m = hip.Model(assets.asset_path(blob), 8, 8, solver=solver)
    with pytest.raises(RuntimeError, match="rr_batch_set_solve_resident: only the fixed-dimension CG instance of the rodent_optimized dimensions"):
        m.check_solve_resident_switch()


def test_switch_is_accepted_for_the_benchmark_model():
    hip.Model(assets.asset_path("rodent_optimized"), 8, 8, solver="cg").check_solve_resident_switch()
