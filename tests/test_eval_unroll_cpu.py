"""The evaluation entry of the step kernel (rr_eval_kernel, C ABI rr_env_unroll_eval) as the device compiler recorded it in the code
object of the built library (tools/kernel_meta.py).  No GPU needed."""
import ctypes
import os
import sys

import pytest

from rodent_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eval_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    return [k for k in kernel_meta.kernels(hip.LIB_PATH) if "rr_eval_kernel" in k["name"]]


def test_exactly_the_four_instances(eval_kernels):
    """Fixed-dimension rodent_optimized and rodent_new, generic, generic with candidate-pair contacts (DYN) -- and under a name the
    metadata tests of the other two entries do not pick up."""
    names = sorted(k["name"] for k in eval_kernels)
    assert len(names) == 4, names
    assert not any("rr_step_kernel" in n or "rr_rand_kernel" in n for n in names)
    assert sum("RRDimsFixedILi66ELi59ELi1263EELb0E" in n for n in names) == 1
    assert sum("RRDimsFixedILi67ELi57ELi1279EELb0E" in n for n in names) == 1
    assert sum("I6RRDimsLb0E" in n for n in names) == 1 and sum("I6RRDimsLb1E" in n for n in names) == 1


def test_budget_of_the_production_instances(eval_kernels):
    """No scratch, no VGPR spill, two waves per SIMD (<= 256 registers of the unified file), no static LDS (the level schedules address
    LDS by absolute byte address: the dynamic segment must begin at 0)."""
    assert eval_kernels
    for k in eval_kernels:
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, k
        assert k["vgpr"] <= 256 and k["vgpr"] + k["agpr"] <= 256, k
        assert k["lds"] == 0, k


def test_kernarg_block_lies_where_the_host_says(eval_kernels):
    """The argument list of rr_step_kernel: RRDims at 0, RRTables (22 pointers) behind it, the I/O block where rr_kernarg_layout() and the
    kernel's re-reads through the kernarg segment pointer assume it, the two scalars closing the block."""
    off, size, total = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    hip.lib().rr_kernarg_layout(ctypes.byref(off), ctypes.byref(size), ctypes.byref(total))
    assert eval_kernels
    for k in eval_kernels:
        explicit = [a for a in k["args"] if a[2] == "by_value"]
        assert len(explicit) == 5, k["name"]
        assert explicit[0][0] == 0 and explicit[1][0] == (explicit[0][1] + 7) // 8 * 8
        assert explicit[1][1] == 22 * 8 and explicit[1][0] + explicit[1][1] == explicit[2][0]
        assert explicit[2][:2] == (off.value, size.value), (k["name"], explicit)
        assert explicit[3] == (off.value + size.value, 4, "by_value") and explicit[4][0] + explicit[4][1] == total.value


def test_symbols_resolve():
    lib = ctypes.CDLL(hip.LIB_PATH)
    for sym in ("rr_env_unroll_eval", "rr_batch_eval_supported"):
        assert sym in hip.EXPORTS
        getattr(lib, sym)
    assert hasattr(hip.Batch, "env_unroll_eval") and hasattr(hip.Batch, "eval_supported")
    from rodent_amd.envs import rodent, wrappers
    from rodent_amd.training import acting
    assert hasattr(rodent.Rodent, "unroll_eval") and hasattr(wrappers.EvalWrapper, "unroll_policy")
    assert "actor_fn" in acting.Evaluator.__init__.__code__.co_varnames
