"""CPU: the parameter layout `acting.actor_params` hands to the in-kernel actor (head padded to 64 columns up to 64 logits, to 128
columns for 65 .. 128) and the width rule of `acting.fused_unroll_supported` (at most 64 actions)."""
import types

import pytest
import torch

from rodent_amd.envs import wrappers
from rodent_amd.training import acting, networks, running_statistics


def _net(obs, outputs, seed):
    torch.manual_seed(seed)
    net = networks.MLP(obs, [32] * 4 + [outputs])
    for l in net.layers:
        l.bias.data.uniform_(-0.3, 0.3)
    return net


def test_a_76_output_head_is_padded_to_128_columns():
    net = _net(50, 76, 0)
    norm = running_statistics.init_state(50, "cpu")
    p = acting.actor_params(net, norm, 0.001)
    head = net.layers[-1]
    assert p["head_wt"].shape == (32, 128) and p["head_b"].shape == (128,)
    assert torch.equal(p["head_wt"][:, :76], head.weight.detach().t()) and torch.equal(p["head_b"][:76], head.bias.detach())
    assert not p["head_wt"][:, 76:].any() and not p["head_b"][76:].any()
    assert p["head_wt"].is_contiguous() and p["w0"].shape == (32, 50) and len(p["hidden_wt"]) == 3
    assert torch.equal(p["mean"], norm.mean) and torch.equal(p["std"], norm.std)


def test_a_60_output_head_keeps_the_64_column_layout():
    net = _net(50, 60, 1)
    p = acting.actor_params(net, None, 0.001)
    head = net.layers[-1]
    want = torch.zeros(32, 64)
    want[:, :60] = head.weight.detach().t()
    wb = torch.zeros(64)
    wb[:60] = head.bias.detach()
    assert p["head_wt"].shape == (32, 64) and torch.equal(p["head_wt"], want) and torch.equal(p["head_b"], wb)
    assert torch.equal(p["w0"], net.layers[0].weight.detach()) and torch.equal(p["hidden_wt"][0], net.layers[1].weight.detach().t())
    assert p["mean"] is None and p["std"] is None and p["min_std"] == 0.001
    assert acting.actor_params(_net(50, 64, 2), None, 0.001)["head_wt"].shape == (32, 64)      # 64 logits: still one pass


def test_heads_wider_than_128_are_refused():
    with pytest.raises(ValueError, match="130"):
        acting.actor_params(_net(50, 130, 3), None, 0.001)


class _Batch:
    def unroll_supported(self, with_actor=False):
        return True


class _Base:
    """What `fused_unroll_supported` reads of a HIP rodent env."""

    def __init__(self, action_size):
        self.device = types.SimpleNamespace(type="cuda")
        self._pipeline_outputs = self._contact_outputs = False
        self.sys = types.SimpleNamespace(solver="cg")
        self.action_size, self.observation_size = action_size, 1244
        self._batch = _Batch()

    def unroll_policy_wrapped(self, *a, **k):
        raise NotImplementedError


def _stub_policy(outputs, hidden=(32, 32, 32, 32)):
    w = types.SimpleNamespace(is_cuda=True, dtype=torch.float32)
    return types.SimpleNamespace(layers=[types.SimpleNamespace(out_features=h, weight=w) for h in hidden + (outputs,)])


@pytest.mark.parametrize("actions,ok", [(30, True), (32, True), (33, True), (38, True), (64, True), (65, False), (100, False)])
def test_fused_unroll_width_rule(actions, ok):
    wenv = wrappers.FusedEpisodeAutoResetWrapper(_Base(actions), 150)
    dist = networks.NormalTanhDistribution(actions)
    assert acting.fused_unroll_supported(wenv, _stub_policy(2 * actions), dist) is ok
    assert acting.actor_shape_supported(_stub_policy(2 * actions), actions) is ok


def test_fused_unroll_other_refusals():
    wenv = wrappers.FusedEpisodeAutoResetWrapper(_Base(38), 150)
    dist = networks.NormalTanhDistribution(38)
    assert not acting.fused_unroll_supported(wenv, _stub_policy(76, hidden=(64, 64)), dist)          # hidden width
    assert not acting.fused_unroll_supported(wenv, _stub_policy(76, hidden=(32,) * 5), dist)         # depth
    assert not acting.fused_unroll_supported(wenv, _stub_policy(60), dist)                            # head != 2 x actions
    assert not acting.fused_unroll_supported(_Base(38), _stub_policy(76), dist)                       # not the fused wrapper
