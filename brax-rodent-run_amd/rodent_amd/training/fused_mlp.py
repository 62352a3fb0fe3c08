"""Actor / critic forward on the hand-written f32-MFMA kernel (C ABI `rr_mlp_forward`, csrc/rr_mlp.h) with an explicit
backward pass, as one `torch.autograd.Function`.

Replaces, for the `make_ppo_networks` default shapes (policy obs -> 32 x4 -> 2*action_size, value obs -> 256 x5 -> 1, SiLU),
the ~40 library launches of `normalize -> policy_net -> value_net` in `ppo.losses.compute_ppo_loss`'s forward
[UP brax.training.agents.ppo.losses; SURVEY.md a22 / a25] by ONE launch that reads the observation tile once for both
networks.  The kernel also writes the hidden pre-activations.  Two backward passes read them:

* the learner's default on a GPU, `agents/ppo/fused_update.FusedUpdate`, takes no autograd graph at all: `hip.mlp_forward` with the
  minibatch addressed in place, `rr_ppo_loss`, then the delta chains (`rr_mlp_value_backward` on the matrix cores, `rr_policy_backward`)
  and every dW = delta' h as a split-row matrix-core product (`rr_mlp_weight_grad_batch`), all hand-written kernels;
* `_ActorCritic.backward` below, the path under `compute_ppo_loss` + `loss.backward()` (`RR_FUSED_LOSS=0`, and what the tests hold
  `FusedUpdate` against), forms the same gradients with library matrix products (rocBLAS / hipBLASLt) and `silu_backward`:
  dW_l = delta_l' h_{l-1}, delta_{l-1} = silu_backward(delta_l W_l, z_{l-1}).

In both, the first layer's dW uses the raw observations and folds the normaliser in afterwards, so the normalised copy of the
minibatch is never written.

A policy whose hidden layers are all 256 wide (`policy_width`) is served as well: `rr_mlp_forward` runs it as a launch of its own
(rr_mlp_policy256_forward_kernel, the value path's pieces with a [256 x P] product as the head) and `FusedUpdate` takes its delta chain
from `rr_mlp_policy_backward`; `_ActorCritic.backward` is width-agnostic.
"""
from __future__ import annotations

import os
from typing import Optional, Sequence

import torch

from .. import hip

POLICY_HIDDEN, VALUE_HIDDEN = 32, 256
WIDE_POLICY_HIDDEN = 256      # the second policy width the kernels serve: the value network's (rr_mlp_policy256_* in csrc/rr_mlp.h)


def max_policy_head() -> int:
    """Widest policy head (in logits) that `ppo.train` and `make_inference_fn` hand to the hand-written learner / actor kernels: 64, or
    128 with RR_FUSED_WIDE_HEAD=1.  The kernels themselves take up to 128 (two passes over column halves of 64); the switch is
    opt-in until the wide path has been measured against the autograd path it replaces."""
    return 128 if os.environ.get("RR_FUSED_WIDE_HEAD", "0") == "1" else 64


def wide_policy_enabled() -> bool:
    """`ppo.train` and `make_inference_fn` hand a 256-wide policy to the hand-written kernels (RR_FUSED_POLICY256, default 1: the fused
    learner's median time was below the autograd path's minimum); 0 keeps that shape on the nn.Linear path."""
    return os.environ.get("RR_FUSED_POLICY256", "1") == "1"


def net_params(mlp):
    """(weights, biases) of an `MLP` in the order / layout the kernel takes (nn.Linear: [out, in])."""
    return [l.weight for l in mlp.layers], [l.bias for l in mlp.layers]


def fusable(mlp, hidden: int, max_out: int) -> bool:
    ls = list(mlp.layers)
    return (2 <= len(ls) <= 8 and all(l.out_features == hidden for l in ls[:-1]) and ls[-1].out_features <= max_out
            and ls[0].weight.is_cuda and ls[0].weight.dtype == torch.float32)


def policy_width(mlp):
    """Hidden width of a policy `MLP` the hand-written kernels serve -- 32 (`POLICY_HIDDEN`) or 256 (`WIDE_POLICY_HIDDEN`), the same in
    every hidden layer, 1 .. 7 of them -- or None for any other shape.  Says nothing about the head or the device: `fusable_policy`."""
    ls = list(mlp.layers)
    if not 2 <= len(ls) <= 8:
        return None
    widths = {l.out_features for l in ls[:-1]}
    if len(widths) == 1 and next(iter(widths)) in (POLICY_HIDDEN, WIDE_POLICY_HIDDEN):
        return next(iter(widths))
    return None


def fusable_policy(mlp) -> bool:
    """The policy network goes to the hand-written forward / learner kernels: a served width (`policy_width`), a head of at most
    `max_policy_head()` logits, float32 parameters on a GPU, and for the 256-wide shape the switch of `wide_policy_enabled`."""
    w = policy_width(mlp)
    if w is None or (w == WIDE_POLICY_HIDDEN and not wide_policy_enabled()):
        return False
    return fusable(mlp, w, max_policy_head())


class _ActorCritic(torch.autograd.Function):
    @staticmethod
    def forward(ctx, obs, mean, std, n_pol, *params):
        pw, pb = list(params[0:2 * n_pol:2]), list(params[1:2 * n_pol:2])
        vw, vb = list(params[2 * n_pol::2]), list(params[2 * n_pol + 1::2])
        need = any(p.requires_grad for p in params)
        with torch.no_grad():
            pol, val, ppre, vpre = hip.mlp_forward(obs, mean, std, ([w.detach() for w in pw], [b.detach() for b in pb]),
                                                   ([w.detach() for w in vw], [b.detach() for b in vb]), want_pre=need)
        ctx.n_pol = n_pol
        ctx.has_norm = mean is not None
        if need:
            ctx.save_for_backward(obs, *([mean, std] if mean is not None else []), ppre, vpre, *params)
        return pol, val

    @staticmethod
    def backward(ctx, g_pol, g_val):
        saved = list(ctx.saved_tensors)
        obs = saved.pop(0)
        mean, std = (saved.pop(0), saved.pop(0)) if ctx.has_norm else (None, None)
        ppre, vpre = saved[0], saved[1]
        params, n_pol = saved[2:], ctx.n_pol
        grads = [None] * len(params)

        def net_backward(ws, pre, delta, base):
            for l in range(len(ws) - 1, -1, -1):
                dsum = delta.sum(0)
                if l == 0 and mean is not None:
                    # dW_1 = delta' ((obs - mean) / std) = (delta' obs - (sum delta) mean') / std: the normalised observations
                    # (114 MB at the learner's shape) are never materialised
                    grads[base] = (delta.t() @ obs).addr_(dsum, mean, alpha=-1.0).div_(std)
                else:
                    grads[base + 2 * l] = delta.t() @ (obs if l == 0 else torch.nn.functional.silu(pre[l - 1]))
                grads[base + 2 * l + 1] = dsum
                if l > 0:
                    delta = torch.ops.aten.silu_backward(delta @ ws[l], pre[l - 1])      # (delta W_l) * silu'(z_{l-1}), one kernel

        if g_pol is not None:
            net_backward(params[0:2 * n_pol:2], ppre, g_pol.contiguous(), 0)
        if g_val is not None:
            net_backward(params[2 * n_pol::2], vpre, g_val.reshape(-1, 1).contiguous(), 2 * n_pol)
        return (None, None, None, None, *grads)


def actor_critic(obs: torch.Tensor, mean: Optional[torch.Tensor], std: Optional[torch.Tensor], policy_net, value_net):
    """(policy logits [M, P], values [M]) of the RAW observations `obs` [M, K] (normalised inside the kernel)."""
    pw, pb = net_params(policy_net)
    vw, vb = net_params(value_net)
    params = [t for wb in zip(pw, pb) for t in wb] + [t for wb in zip(vw, vb) for t in wb]
    return _ActorCritic.apply(obs.contiguous(), mean, std, len(pw), *params)


@torch.no_grad()
def policy_logits(obs: torch.Tensor, mean: Optional[torch.Tensor], std: Optional[torch.Tensor], policy_net) -> torch.Tensor:
    """Inference: normalise + policy MLP in one launch (the rollout's actor step)."""
    pw, pb = net_params(policy_net)
    return hip.mlp_forward(obs.contiguous(), mean, std, policy=(pw, pb))[0]
