"""A policy network with 256-wide hidden layers: which shapes go to the hand-written kernels (`fused_mlp.policy_width` / `fusable_policy`, on
CPU tensors and stubs), what stays with the 32-wide shape (the in-kernel actor), and the resources of the two new kernels read from the
code object of the built library (tools/kernel_meta.py; no GPU needed)."""
import os
import sys
import types

import pytest
import torch

from rodent_amd import hip
from rodent_amd.envs import wrappers
from rodent_amd.training import acting, fused_mlp, networks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORWARD = "_Z31rr_mlp_policy256_forward_kernel9RRMlpArgs"
BACKWARD = "_Z32rr_mlp_policy256_backward_kernel15RRPol256BwdArgs"


def _stub(outputs, hidden, cuda=True, dtype=torch.float32):
    w = types.SimpleNamespace(is_cuda=cuda, dtype=dtype)
    return types.SimpleNamespace(layers=[types.SimpleNamespace(out_features=h, weight=w) for h in tuple(hidden) + (outputs,)])


@pytest.mark.parametrize("hidden,want", [((32,) * 4, 32), ((32,), 32), ((32,) * 7, 32), ((256,), 256), ((256,) * 4, 256), ((256,) * 7, 256),
                                         ((256,) * 8, None), ((), None), ((64, 64), None), ((256, 32), None), ((32, 256), None),
                                         ((256, 256, 128), None), ((128,), None)])
def test_policy_width(hidden, want):
    assert fused_mlp.policy_width(_stub(60, hidden)) == want
    assert fused_mlp.policy_width(networks.MLP(20, list(hidden) + [60])) == want          # a real module, on the CPU


def test_fusable_policy_follows_width_head_device_and_switches(monkeypatch):
    for k in ("RR_FUSED_POLICY256", "RR_FUSED_WIDE_HEAD"):
        monkeypatch.delenv(k, raising=False)
    wide_default = fused_mlp.wide_policy_enabled()
    assert fused_mlp.fusable_policy(_stub(60, (32,) * 4))
    assert fused_mlp.fusable_policy(_stub(60, (256,) * 4)) is wide_default
    monkeypatch.setenv("RR_FUSED_POLICY256", "1")
    assert fused_mlp.fusable_policy(_stub(60, (256,) * 4)) and fused_mlp.fusable_policy(_stub(64, (256,)))
    assert not fused_mlp.fusable_policy(_stub(76, (256, 256)))                      # heads of 65 .. 128 logits: gated as for the 32-wide policy
    assert not fused_mlp.fusable_policy(_stub(60, (256, 64)))
    assert not fused_mlp.fusable_policy(_stub(60, (256, 256), cuda=False))
    assert not fused_mlp.fusable_policy(_stub(60, (256, 256), dtype=torch.float64))
    assert not fused_mlp.fusable_policy(networks.MLP(20, [256, 256, 60]))           # CPU parameters
    monkeypatch.setenv("RR_FUSED_WIDE_HEAD", "1")
    assert fused_mlp.fusable_policy(_stub(76, (256, 256))) and fused_mlp.fusable_policy(_stub(128, (256, 256)))
    assert not fused_mlp.fusable_policy(_stub(130, (256, 256)))
    monkeypatch.setenv("RR_FUSED_POLICY256", "0")
    assert not fused_mlp.fusable_policy(_stub(60, (256,) * 4)) and fused_mlp.fusable_policy(_stub(60, (32,) * 4))


class _Batch:
    def unroll_supported(self, with_actor=False):
        return True


class _Base:
    """What `fused_unroll_supported` reads of a HIP rodent env."""

    def __init__(self, action_size):
        self.device = types.SimpleNamespace(type="cuda")
        self._pipeline_outputs = self._contact_outputs = False
        self.sys = types.SimpleNamespace(solver="cg")
        self.action_size, self.observation_size = action_size, 1263
        self._batch = _Batch()

    def unroll_policy_wrapped(self, *a, **k):
        raise NotImplementedError


def test_the_in_kernel_actor_does_not_serve_the_wide_shape():
    wenv = wrappers.FusedEpisodeAutoResetWrapper(_Base(30), 150)
    dist = networks.NormalTanhDistribution(30)
    assert acting.fused_unroll_supported(wenv, _stub(60, (32,) * 4), dist)
    for hidden in ((256,), (256, 256), (256,) * 4):
        assert not acting.fused_unroll_supported(wenv, _stub(60, hidden), dist)
        assert not acting.actor_shape_supported(_stub(60, hidden), 30)
    with pytest.raises(ValueError, match="32"):
        acting.actor_params(networks.MLP(20, [256, 256, 60]), None, 0.001)


@pytest.fixture(scope="module")
def meta():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    return {k["name"]: k for k in kernel_meta.kernels(hip.LIB_PATH)}


def test_the_two_kernels_exist_and_use_no_scratch(meta):
    for name in (FORWARD, BACKWARD):
        assert name in meta, name
        k = meta[name]
        print(name, {f: k[f] for f in ("vgpr", "agpr", "sgpr", "sgpr_spill", "vgpr_spill", "scratch", "lds")})
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["lds"] == 0, (name, k["scratch"], k["vgpr_spill"], k["lds"])


def test_the_forward_keeps_three_workgroups_per_cu(meta):
    """__launch_bounds__(256, 3): at most 168 registers per lane next to 51.5 KB of dynamic LDS, as the value network's forward."""
    k = meta[FORWARD]
    assert k["vgpr"] + k["agpr"] <= 168, (k["vgpr"], k["agpr"])
    assert meta[BACKWARD]["vgpr"] + meta[BACKWARD]["agpr"] <= 256            # two workgroups per CU
