"""The learner / actor kernels that carry policy heads of up to 128 logits, read from the code object of the built library
(tools/kernel_meta.py; no GPU needed), and the switch that sends such a head to them."""
import os
import sys

import pytest

from rodent_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORWARD = ("_Z21rr_mlp_forward_kernelILb1ELb1EEv9RRMlpArgs", "_Z21rr_mlp_forward_kernelILb1ELb0EEv9RRMlpArgs",
           "_Z21rr_mlp_forward_kernelILb0ELb1EEv9RRMlpArgs")
OTHERS = ("_Z25rr_policy_backward_kernel12RRPolBwdArgs", "_Z21rr_policy_tail_kernelILi64EEv13RRPolTailArgs", "_Z21rr_policy_tail_kernelILi128EEv13RRPolTailArgs")


@pytest.fixture(scope="module")
def meta():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    return {k["name"]: k for k in kernel_meta.kernels(hip.LIB_PATH)}


def test_wide_head_kernels_use_no_scratch_and_spill_no_vgpr(meta):
    for name in FORWARD + OTHERS:
        assert name in meta, name
        k = meta[name]
        print(name, {f: k[f] for f in ("vgpr", "agpr", "sgpr", "sgpr_spill", "lds")})
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, (name, k["scratch"], k["vgpr_spill"])


def test_forward_instances_keep_three_workgroups_per_cu(meta):
    """__launch_bounds__(256, 3): at most 168 registers per lane; and no static LDS next to the 51.5 KB dynamic segment (three segments of
    52 736 B are 158 208 of a CU's 163 840 B).  The build before the head became a loop over column halves had 0 B of static LDS in all
    three instances; the two passes re-stage into the same region B, so it stays 0."""
    for name in FORWARD:
        k = meta[name]
        assert k["vgpr"] + k["agpr"] <= 168, (name, k["vgpr"], k["agpr"])
        assert k["lds"] == 0, (name, k["lds"])


def test_max_policy_head_follows_the_switch(monkeypatch):
    from rodent_amd.training import fused_mlp
    monkeypatch.delenv("RR_FUSED_WIDE_HEAD", raising=False)
    assert fused_mlp.max_policy_head() == 64
    monkeypatch.setenv("RR_FUSED_WIDE_HEAD", "0")
    assert fused_mlp.max_policy_head() == 64
    monkeypatch.setenv("RR_FUSED_WIDE_HEAD", "1")
    assert fused_mlp.max_policy_head() == 128
