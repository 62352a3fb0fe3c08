"""Rollouts: `actor_step` / `generate_unroll` / `Evaluator` with the data flow of `brax.training.acting`
(SURVEY.md Appendix E), storing each observation ONCE per unroll ([T+1] instead of obs + next_obs:
the upstream Transition keeps both, 13.6 GB per training step at 2048 envs)."""
from __future__ import annotations

import os
import time
from typing import Callable, Dict, Optional

import torch

from .. import hip
from ..envs import wrappers


class UnrollBuffer:
    """Trajectory storage of one training step: [U unrolls, N envs, T(+1) steps, ...], a trajectory
    (u, n) is contiguous so minibatch gathers copy whole rows."""

    def __init__(self, U, N, T, obs_dim, act_dim, device):
        self.U, self.N, self.T = U, N, T
        self.obs = torch.empty(U, N, T + 1, obs_dim, device=device)
        self.raw_action = torch.empty(U, N, T, act_dim, device=device)
        self.log_prob = torch.empty(U, N, T, device=device)
        self.reward = torch.empty(U, N, T, device=device)
        self.discount = torch.empty(U, N, T, device=device)
        self.truncation = torch.empty(U, N, T, device=device)

    def flat(self):
        f = lambda x: x.reshape((self.U * self.N,) + x.shape[2:])
        return dict(obs=f(self.obs), raw_action=f(self.raw_action), log_prob=f(self.log_prob), reward=f(self.reward),
                    discount=f(self.discount), truncation=f(self.truncation))


@torch.no_grad()
def generate_unroll(env, state, policy: Callable, buf: UnrollBuffer, u: int, generator=None):
    """Collect `buf.T` steps with `policy`; transition t holds (obs_t, action_t, reward_{t+1}, 1-done_{t+1},
    truncation_{t+1}) and obs[T] is the bootstrap observation [UP acting.generate_unroll]."""
    for t in range(buf.T):
        buf.obs[u, :, t] = state.obs
        action, extras = policy(state.obs, generator)
        nstate = env.step(state, action)
        buf.raw_action[u, :, t] = extras["raw_action"]
        buf.log_prob[u, :, t] = extras["log_prob"]
        buf.reward[u, :, t] = nstate.reward
        buf.discount[u, :, t] = 1 - nstate.done
        buf.truncation[u, :, t] = nstate.info["truncation"]
        state = nstate
    buf.obs[u, :, buf.T] = state.obs
    return state


ACTOR_MAX_ACTIONS = 64      # the in-kernel actor: lane = action, so at most one wave of actions (head <= 128 logits, two passes)


def actor_params(policy_net, normalizer_params, min_std: float) -> dict:
    """The policy's parameters in the layout of the in-kernel actor (`rr_env_unroll_policy`): first layer as torch holds it, hidden
    weights transposed, head transposed and zero-padded to 64 outputs (heads of up to 64 logits: one pass of the wave) or to 128
    outputs (65 .. 128 logits, i.e. 33 .. 64 actions: two passes).  Copies: call again after the parameters change."""
    layers = list(policy_net.layers)
    dev = layers[0].weight.device
    P = layers[-1].out_features
    if P > 2 * ACTOR_MAX_ACTIONS:
        raise ValueError(f"actor_params: a head of {P} outputs exceeds the in-kernel actor's {2 * ACTOR_MAX_ACTIONS}")
    widths = sorted({l.out_features for l in layers[:-1]})
    if widths != [32]:      # a 256-wide policy (served by rr_mlp_forward / rr_mlp_policy_backward) has no in-kernel actor
        raise ValueError(f"actor_params: the in-kernel actor takes hidden layers of 32 units, got {widths}")
    W = hip.head_columns(P)
    head_wt = torch.zeros(32, W, device=dev)
    head_wt[:, :P] = layers[-1].weight.detach().t()
    head_b = torch.zeros(W, device=dev)
    head_b[:P] = layers[-1].bias.detach()
    out = dict(w0=layers[0].weight.detach().contiguous(), b0=layers[0].bias.detach().contiguous(),
               hidden_wt=[l.weight.detach().t().contiguous() for l in layers[1:-1]], hidden_b=[l.bias.detach().contiguous() for l in layers[1:-1]],
               head_wt=head_wt, head_b=head_b, min_std=min_std, mean=None, std=None)
    if normalizer_params is not None:
        out.update(mean=normalizer_params.mean.contiguous(), std=normalizer_params.std.contiguous())
    return out


def actor_shape_supported(policy_net, action_size: int) -> bool:
    """The policy shapes the in-kernel actor evaluates: 1 .. 4 hidden layers of 32 units, float32, a head of 2 x action_size
    logits with action_size <= 64.  (The LEARNER's kernels take the same widths, but `ppo.train` hands them a head of more than 64
    logits only with RR_FUSED_WIDE_HEAD=1 -- `fused_mlp.max_policy_head()` -- which decides the learner's path only.)"""
    from . import fused_mlp
    ls = list(policy_net.layers)
    return (2 <= len(ls) <= 5 and all(l.out_features == fused_mlp.POLICY_HIDDEN for l in ls[:-1]) and ls[0].weight.dtype == torch.float32
            and ls[-1].out_features == 2 * action_size and 1 <= action_size <= ACTOR_MAX_ACTIONS)


def fused_unroll_supported(wenv, policy_net, dist) -> bool:
    """The one-launch unroll needs the fused wrapper of a HIP rodent env (rollout configuration) whose model has a multi-step kernel
    instance, and a policy the in-kernel actor evaluates (`actor_shape_supported`) on a row as wide as the env's -- the env says
    whether the actor of the instance it would launch reads that width (`Rodent.fused_actor_refusal`: 1280 entries without reference
    frames, 1664 with them or with a higher pose option); a wider row falls back to per-step collection."""
    base = wenv.unwrapped if hasattr(wenv, "unwrapped") else wenv
    refusal = getattr(base, "fused_actor_refusal", None)
    if refusal is not None:
        width_ok = refusal() is None
    else:       # an env that cannot say (not a `Rodent`): the 64 x 20 entries of the instances without reference frames
        width_ok = getattr(base, "observation_size", 0) <= 1280
    return (isinstance(wenv, wrappers.FusedEpisodeAutoResetWrapper) and hasattr(base, "unroll_policy_wrapped") and base.device.type == "cuda"
            and not base._pipeline_outputs and not base._contact_outputs and getattr(getattr(base, "sys", None), "solver", "cg") == "cg"
            and policy_net.layers[0].weight.is_cuda and dist.event_size == base.action_size and actor_shape_supported(policy_net, base.action_size)
            and width_ok
            and base._batch.unroll_supported(with_actor=True))


@torch.no_grad()
def generate_unroll_fused(wenv, state, actor: dict, buf: UnrollBuffer, u: int, generator=None):
    """`generate_unroll` as ONE launch (policy, sampling, env steps, wrappers and the recording of the transitions all inside the
    multi-step kernel): the envs of the batch never wait for each other between the T steps."""
    N, T = buf.N, buf.T
    noise = torch.randn(T, N, buf.raw_action.shape[-1], device=buf.obs.device, generator=generator)
    traj = dict(obs=buf.obs[u], raw_action=buf.raw_action[u], log_prob=buf.log_prob[u], reward=buf.reward[u], discount=buf.discount[u],
                truncation=buf.truncation[u])
    state, _ = wenv.unroll_policy(state, actor, noise, traj)
    return state


@torch.no_grad()
def generate_unrolls_fused(wenv, state, actor: dict, buf: UnrollBuffer, generator=None):
    """ALL `buf.U` unrolls of a training step as one launch: the policy does not change during the rollout phase, so its U x T env
    steps are one multi-step rollout recorded as U trajectories (`segment` = T).  Over U x T = 640 unsynchronised steps the envs'
    costs average out (a synchronised step lasts as long as its slowest env)."""
    U, N, T = buf.U, buf.N, buf.T
    noise = torch.randn(U * T, N, buf.raw_action.shape[-1], device=buf.obs.device, generator=generator)
    traj = dict(obs=buf.obs, raw_action=buf.raw_action, log_prob=buf.log_prob, reward=buf.reward, discount=buf.discount, truncation=buf.truncation)
    state, _ = wenv.unroll_policy(state, actor, noise, traj, segment=T)
    return state


class SubBatchRollout:
    """The rank's N envs collected as S sub-batches of N / S envs, each with its own env batch, HIP stream, wrapper state and
    sampling generator; one unroll of a sub-batch (T x [policy forward, sampling, fused env step, wrapper kernel, buffer
    writes]) is captured once as a HIP graph and replayed (`envs.graphed.GraphedSteps`).

    Why: a 2048-env step kernel lasts as long as its slowest env, and between two step kernels the GPU runs the policy's small
    launches; with two sub-batches in flight one's tail and policy launches overlap the other's step kernel (config 2 measured
    1.49 -> 1.43 ms per 2048-env step), and replay removes the ~0.7 ms of host work per env step that would otherwise serialise
    the two streams.  Every env still steps exactly once per rollout step: only the order of work on the GPU changes
    (`tests/test_gpu_env.py` holds sub-batches and replay to the one-launch, host-issued trajectories bit for bit).
    """

    def __init__(self, environment, num_sub: int, device, episode_length: int, action_repeat: int, T: int, seed: int, use_graph: bool = True):
        from ..envs import graphed
        self._graphed = graphed
        self.N = environment.num_envs
        self.S, self.n, self.T, self.device, self.use_graph = num_sub, environment.num_envs // num_sub, T, device, use_graph
        self.subs = []
        for si in range(num_sub):
            st = torch.cuda.Stream(device)
            with torch.cuda.stream(st):                                  # the batch binds the stream it is created on
                env = environment.with_num_envs(self.n, device)
                params = environment.env_params() if hasattr(environment, "env_params") else None
                if params is not None:                                   # domain randomisation: this sub-batch's slice of the draws
                    env.set_env_params(**{k: (v[si * self.n:(si + 1) * self.n].contiguous() if v is not None else None) for k, v in params.items()})
                wenv = wrappers.wrap(env, episode_length=episode_length, action_repeat=action_repeat)
                gen = torch.Generator(device=device)
                gen.manual_seed(seed * 1009 + si)
                stage = UnrollBuffer(1, self.n, T, env.observation_size, env.action_size, device)
            self.subs.append(dict(stream=st, env=env, wenv=wenv, gen=gen, stage=stage, state=None, graph=None))

    def reset(self, keys):
        for si, sub in enumerate(self.subs):
            with torch.cuda.stream(sub["stream"]):
                sub["state"] = sub["wenv"].reset(keys[si * self.n:(si + 1) * self.n])
            sub["graph"] = None                                          # recaptured after the next host-issued unroll

    def unroll(self, policy: Callable, buf: UnrollBuffer, u: int):
        """One unroll of every sub-batch into buf[u] (asynchronous: `join()` before reading `buf`).  `policy` must be the SAME
        callable at every call (it is part of the captured graph): parameters and normaliser are read from fixed buffers."""
        main = torch.cuda.current_stream(self.device)
        for si, sub in enumerate(self.subs):
            sub["stream"].wait_stream(main)                              # parameter / normaliser updates issued on the caller's stream
            with torch.cuda.stream(sub["stream"]):
                if sub["graph"] is not None:
                    sub["graph"].replay()
                else:
                    step_fn = lambda st_, sub=sub: generate_unroll(sub["wenv"], st_, policy, sub["stage"], 0, sub["gen"])
                    sub["state"] = step_fn(sub["state"])
                    if self.use_graph and sub.get("warm"):               # second host-issued unroll done: capture from a step OUTPUT
                        sub["graph"] = self._graphed.GraphedSteps(step_fn, sub["state"], 1, sub["stream"], [sub["gen"]])
                        sub["state"] = sub["graph"].state
                    sub["warm"] = True
                lo, hi = si * self.n, (si + 1) * self.n
                for name in ("obs", "raw_action", "log_prob", "reward", "discount", "truncation"):
                    getattr(buf, name)[u, lo:hi].copy_(getattr(sub["stage"], name)[0])

    def join(self):
        main = torch.cuda.current_stream(self.device)
        for sub in self.subs:
            main.wait_stream(sub["stream"])


class Evaluator:
    """`brax.training.acting.Evaluator`: episode_length steps of a freshly reset eval env, episode metric sums."""

    def __init__(self, eval_env, eval_policy_fn: Callable, num_eval_envs: int, episode_length: int, action_repeat: int, key,
                 actor_fn: Optional[Callable] = None, deterministic: bool = False):
        """`actor_fn(policy_params)` -> the policy in the layout of the in-kernel actor (`actor_params`), `deterministic`: whether
        `eval_policy_fn` builds the deterministic policy.  With them and RR_FUSED_EVAL=1 the evaluation is ONE launch
        (`EvalWrapper.unroll_policy`) where the env has an evaluation instance (the fused wrapper of a HIP env, action_repeat 1);
        everything else runs the per-step loop.  The loop is the default: at 128 envs x 150 steps both paths wait for the same chain of
        dependent env steps and the one launch measured no faster (tools/bench_eval.py)."""
        self._key = key
        self._actor_fn = actor_fn
        self._deterministic = deterministic
        self._action_repeat = action_repeat
        self._eval_walltime = 0.0
        self._env = wrappers.EvalWrapper(eval_env)
        self._policy_fn = eval_policy_fn
        self._steps_per_unroll = episode_length * num_eval_envs
        self._unroll_length = episode_length // action_repeat

    def one_launch(self) -> bool:
        """Whether `run_evaluation` takes the one-launch path now (per-env parameters set on the env later turn it off).  Never for a
        pose env (`Rodent(track_quat=..., track_joints=...)`: no evaluation instance rewards the pose): the per-step loop below runs, and
        its `EvalWrapper` sums `quat_reward` and `joint_reward` like every other metric (eval/episode_quat_reward, eval/episode_joint_reward)."""
        return (self._actor_fn is not None and self._action_repeat == 1 and os.environ.get("RR_FUSED_EVAL", "0") == "1"
                and self._env.unroll_supported())

    @torch.no_grad()
    def run_evaluation(self, policy_params, training_metrics: Dict, aggregate_episodes: bool = True) -> Dict:
        from .. import jax_random
        self._key, unroll_key = jax_random.split(self._key)
        t = time.time()
        policy = self._policy_fn(policy_params)
        state = self._env.reset(jax_random.split(unroll_key, self._env.num_envs))
        # the clips the episodes START on: `EvalWrapper` scores an env's first episode only, and an env with `restart_across_clips` may be
        # on another clip by the end of the unroll (the tensor is the same one after the unroll where clips do not move)
        clip = state.info.get("clip")
        if self.one_launch():
            T, N = self._unroll_length, self._env.num_envs
            noise = None if self._deterministic else torch.randn(T, N, self._env.action_size, device=state.obs.device)
            state = self._env.unroll_policy(state, self._actor_fn(policy_params), noise, T)
        else:
            for _ in range(self._unroll_length):
                action, _ = policy(state.obs, None)
                state = self._env.step(state, action)
        if state.obs.is_cuda:
            torch.cuda.synchronize(state.obs.device)
        em = state.info["eval_metrics"]
        epoch_eval_time = time.time() - t
        metrics = {}
        for name, value in em["episode_metrics"].items():
            metrics[f"eval/episode_{name}"] = float(value.mean()) if aggregate_episodes else value.cpu().numpy()
        # multi-clip eval env: the episode reward per clip, over the eval envs that follow it (a clip no eval env drew has no key)
        if clip is not None and getattr(self._env, "num_clips", 1) > 1 and aggregate_episodes:
            reward, ids = em["episode_metrics"]["reward"].cpu(), clip.cpu()
            for c in torch.unique(ids).tolist():
                metrics[f"eval/episode_reward_clip{c}"] = float(reward[ids == c].mean())
        metrics["eval/avg_episode_length"] = float(em["episode_steps"].mean())
        metrics["eval/epoch_eval_time"] = epoch_eval_time
        metrics["eval/sps"] = self._steps_per_unroll / epoch_eval_time
        self._eval_walltime += epoch_eval_time
        metrics = {"eval/walltime": self._eval_walltime, **training_metrics, **metrics}
        return metrics
