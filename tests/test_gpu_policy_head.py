"""GPU: what the one tanh-normal head (csrc/rr_tanh_normal.h) and the one head body of `rr_policy_tail_kernel<W>` promise -- the two-launch
actor, the sampling kernel and the learner's loss kernel form the same numbers from the same logits -- and that the scratch cache of
`rodent_amd.hip` keeps one buffer per (call, device, stream, shape)."""
import functools

import pytest
import torch

from tests import ppo_batches
from tests.test_gpu_ppo_loss import _hip_sampler

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M, K = 9, 70                                   # one full 8-row group + a partial one; four full 16-wide k-chunks + a partial one
ACTIONS = (1, 31, 32, 33, 38, 64)              # both head widths (64 / 128 columns), both sides of the 32-action and the 32-lane boundary


@functools.lru_cache(maxsize=None)
def _case(A):
    """(policy parameters, min_std, obs, mean, std, noise, policy_act's outputs with that noise) for a head of 2A logits."""
    from rodent_amd import hip
    from rodent_amd.training import fused_mlp, networks
    torch.manual_seed(100 + A)
    nets = networks.make_ppo_networks(K, A, device=DEV)
    net, dist = nets.policy_network, nets.parametric_action_distribution
    for l in net.layers:
        l.bias.data.uniform_(-0.2, 0.2)
    obs = torch.randn(M, K, device=DEV) * 2 + 0.3
    mean, std = torch.randn(K, device=DEV) * 0.3, torch.rand(K, device=DEV) + 0.5
    eps = torch.randn(M, A, device=DEV)
    params = fused_mlp.net_params(net)
    out = hip.policy_act(obs, mean, std, params, eps, dist.min_std, want_logits=True)
    torch.cuda.synchronize()
    return params, dist.min_std, obs, mean, std, eps, out


@pytest.mark.parametrize("A", ACTIONS)
def test_two_launch_actor_equals_the_sampling_kernel(A):
    """rr_policy_tail_kernel and rr_policy_sample_kernel on the same logits and noise: raw action, action and log-prob bit for bit (the
    same head term, a lane adds dimension `lane` then `lane + 32`, the same 32-lane butterfly)."""
    from rodent_amd import hip
    _, min_std, _, _, _, eps, (act, raw, lp, logits) = _case(A)
    assert logits.shape == (M, 2 * A) and torch.isfinite(logits).all()
    act_s, raw_s, lp_s = hip.policy_sample(logits, eps, min_std)
    torch.cuda.synchronize()
    print(f"A={A}: max |log_prob difference| {float((lp - lp_s).abs().max()):.2e}")
    assert torch.equal(raw, raw_s)
    assert torch.equal(act, act_s)
    assert torch.equal(lp, lp_s)


@pytest.mark.parametrize("A", ACTIONS)
def test_deterministic_policy_equals_zero_noise(A):
    from rodent_amd import hip
    params, min_std, obs, mean, std, eps, _ = _case(A)
    act_d, raw_d, lp_d, _ = hip.policy_act(obs, mean, std, params, None, min_std)
    act_0 = hip.policy_act(obs, mean, std, params, torch.zeros_like(eps), min_std)[0]
    torch.cuda.synchronize()
    assert raw_d is None and lp_d is None
    assert torch.equal(act_d, act_0)


def test_learner_agrees_with_the_actor_at_the_actors_own_point():
    """The t == 0 rows of an on-policy batch carry the action and log-prob `rr_policy_sample` formed at the current logits; rr_ppo_loss
    must find rho = 1 there, by the bound of test_loss_kernel_on_on_policy_batches (`assert_t0_rows_on_policy`).  The kernel's own rho
    is read off its gradient: with no entropy term d loss / d loc_a = -(1 / n) adv w rho z_a / scale_a, w = 1 inside the clip range (and
    0 or 1 outside, which fails the bound); values 0, discount 0 and no truncation make adv the reward itself, exactly."""
    from rodent_amd import hip
    T, B, R, A = 3, 8, 8, 38                   # the smallest on-policy batch of tests/test_gpu_ppo_loss.py
    cfg = dict(ppo_batches.CFG, entropy_cost=0.0)
    data, logits, values, noise, idx = ppo_batches.onpolicy_batch(T, B, R, A, seed=T * 1000 + B + A, use_idx=False, sampler=_hip_sampler)
    assert idx is None and (data["reward"] > 0).all()
    data["discount"], data["truncation"], values = torch.zeros_like(data["discount"]), torch.zeros_like(data["truncation"]), torch.zeros_like(values)
    dd = {k: v.to(DEV).contiguous() for k, v in data.items()}
    gl, _, _ = hip.ppo_loss(logits.to(DEV), values.to(DEV), dd, None, noise.to(DEV), T, normalize_advantage=False, **cfg)
    torch.cuda.synchronize()
    n = T * B
    loc, s = logits[:B, :A].double(), logits[:B, A:].double()
    scale = torch.nn.functional.softplus(s) + 0.001
    z = (data["raw_action"][:B, 0].double() - loc) / scale
    a = z.abs().argmax(1, keepdim=True)        # the best-conditioned dimension of each row
    adv = data["reward"][:B, 0].double() * cfg["reward_scaling"]
    dloc = gl[:B, :A].double().cpu().gather(1, a).squeeze(1)
    rho = -n * dloc * scale.gather(1, a).squeeze(1) / (z.gather(1, a).squeeze(1) * adv)
    ppo_batches.assert_t0_rows_on_policy(rho, cfg["clipping_epsilon"], B)


def test_scratch_cache_is_address_stable_per_key():
    """`policy_act` on two streams: each stream keeps ONE workspace (the same address at the second call) that is not the other
    stream's, and both results are the single-stream result."""
    from rodent_amd import hip
    A = 38
    params, min_std, obs, mean, std, eps, ref = _case(A)
    streams = [torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)]
    spans, outs = [], []
    for st in streams:
        st.wait_stream(torch.cuda.current_stream(obs.device))
        with torch.cuda.stream(st):
            key = ("policy_act", obs.device, st.cuda_stream, M)
            first = hip.policy_act(obs, mean, std, params, eps, min_std, want_logits=True)
            ws = hip._scratch[key]
            outs.append(hip.policy_act(obs, mean, std, params, eps, min_std, want_logits=True))
            assert hip._scratch[key] is ws and ws.numel() * 4 >= hip.lib().rr_policy_act_workspace_bytes(M)
            outs.append(first)
            spans.append((ws.data_ptr(), ws.data_ptr() + ws.numel() * 4))
    torch.cuda.synchronize()
    assert spans[0][1] <= spans[1][0] or spans[1][1] <= spans[0][0]          # two buffers, not one
    for out in outs:
        for got, want in zip(out, ref):
            assert torch.equal(got, want)
