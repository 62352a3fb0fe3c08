"""Proximal policy optimization training: the `brax.training.agents.ppo.train.train` entry point the
reference launcher calls [REF brax_rodent_run_ppo.py:97-114,200-202], with the same keyword
arguments, schedule arithmetic, callbacks and return value -- on PyTorch-ROCm.

Data parallelism: one process per GPU (launch with torch.distributed.run); `num_envs` / `batch_size`
are GLOBAL as upstream, each rank steps `num_envs // world_size` environments; the only collectives
are the per-minibatch gradient all-reduce(mean) on one flat buffer and the normaliser all-reduce(sum)
once per training step (RCCL over xGMI; gloo in the CPU tests).
"""
from __future__ import annotations

import copy
import math
import logging
import os
import time
import warnings
from typing import Callable, Optional, Tuple

import numpy as np
import torch

from .... import hip, jax_random
from ....envs import wrappers
from ... import acting, distributed as D, fused_mlp, networks as ppo_networks_mod, optim, running_statistics
from ...types import PPONetworkParams, TrainingState
from . import losses as ppo_losses


def _local_env(environment, local_num_envs: int, device):
    if getattr(environment, "num_envs", None) == local_num_envs:
        return environment
    if hasattr(environment, "with_num_envs"):
        return environment.with_num_envs(local_num_envs, device)
    raise ValueError(f"environment has {getattr(environment, 'num_envs', '?')} envs, need {local_num_envs} per rank")


def randomization_keys(seed: int, process_id: int, local_num_envs: int, num_eval_envs: int):
    """The keys `train` binds to `randomization_fn` on rank `process_id` [UP ppo.train]: `local_num_envs` keys split from the rank's
    env key for the training env, `num_eval_envs` keys split from its eval key for the eval env (uint32 [n, 2] each).  The rank's key
    is folded from its process id, so two ranks draw different parameters."""
    _, local_key = jax_random.split(jax_random.PRNGKey(seed))
    local_key = jax_random.fold_in(local_key, process_id)
    _, key_env, eval_key = jax_random.split(local_key, 3)
    return jax_random.split(key_env, local_num_envs), jax_random.split(eval_key, num_eval_envs)


def train(
    environment,
    num_timesteps: int,
    episode_length: int,
    action_repeat: int = 1,
    num_envs: int = 1,
    max_devices_per_host: Optional[int] = None,
    num_eval_envs: int = 128,
    learning_rate: float = 1e-4,
    entropy_cost: float = 1e-4,
    discounting: float = 0.9,
    seed: int = 0,
    unroll_length: int = 10,
    batch_size: int = 32,
    num_minibatches: int = 16,
    num_updates_per_batch: int = 2,
    num_evals: int = 1,
    num_resets_per_eval: int = 0,
    normalize_observations: bool = False,
    reward_scaling: float = 1.0,
    clipping_epsilon: float = 0.3,
    gae_lambda: float = 0.95,
    deterministic_eval: bool = False,
    network_factory: Callable = ppo_networks_mod.make_ppo_networks,
    progress_fn: Callable = lambda *args: None,
    normalize_advantage: bool = True,
    global_advantage_normalization: bool = False,
    eval_env=None,
    policy_params_fn: Callable = lambda *args: None,
    randomization_fn=None,
    max_training_steps: Optional[int] = None,
    timing_fn: Optional[Callable] = None,
    return_training_state: bool = False,
    clip_weight_fn: Optional[Callable] = None,
    max_grad_norm: Optional[float] = None,
    learner_diagnostics: bool = False,
    target_kl: Optional[float] = None,
    learning_rate_schedule: Optional[str] = None,
    desired_kl: float = optim.DESIRED_KL_DEFAULT,
    learning_rate_bounds: Tuple[float, float] = optim.LR_BOUNDS_DEFAULT,
):
    """PPO training.  Returns (make_policy, params=(normalizer_params, policy_params), metrics).

    `max_training_steps` (extension) stops after that many training steps (benchmarks / tests).
    `return_training_state` (extension): also return the final `TrainingState` (optimizer, params, normaliser, env_steps).
    `global_advantage_normalization` (extension, default off = the reference's behaviour: advantages are normalised over
    the rank-local minibatch): normalise with the mean / variance of the GLOBAL minibatch instead, one
    3-float all-reduce {n, sum a, sum a^2} per minibatch (the north star's "advantage-normalisation all-reduce").
    `clip_weight_fn` (extension; an env built with `clip_outcomes=True`): after every training step the training envs' per-clip outcome
    counters are read and cleared, summed over the sub-batches and over the ranks (one int64 all-reduce), and reported as
    `training/clip_fail_rate` ((pose failures + env dones) / ended episodes), `training/clip_truncated_share` and, with at most 16
    clips, `training/clip_fail_rate_clip{c}`.  The function is called with that step's int64 [C, 5] table on every rank; a result
    other than None goes to `set_clip_weights` of every training batch (`envs.rodent.FailureWeights` is one such function).  The eval
    env keeps its uniform weights.
    `max_grad_norm` (upstream's argument of that name; default None = no clipping, the optimiser and the captured graphs of a build
    without the option): a number > 0 (`inf` allowed, anything else raises ValueError) puts `optax.clip_by_global_norm` in front of Adam
    (`training.optim.ClippedAdam`, three HIP launches per minibatch update): the all-reduced gradient of BOTH networks is scaled by
    max_grad_norm / norm where its global norm (squares summed in float64, rounded to float32 once) exceeds max_grad_norm, and used as
    it is otherwise.  EXTENSION over optax: an update whose norm is not finite (some gradient element is NaN or +-inf) is skipped --
    parameters, both moments and Adam's step count keep their bits -- instead of turning every parameter into NaN for the rest of the
    run; the learner's counterpart of the env's `bad_state_max`.  Reported per training step, read and cleared after its closing
    synchronisation: `training/grad_norm` (mean pre-clip norm over the applied updates), `training/grad_norm_max`,
    `training/grad_clip_share` (applied updates that were scaled), `training/skipped_updates` (one warning the first time it is not 0).
    `learner_diagnostics` (extension, default off; also on with either option below): every evaluated minibatch contributes approx_kl
    (mean of expm1(d) - d, d = new - behaviour log-prob: the k3 estimator, >= 0), the clip fraction of the surrogate, the explained
    variance 1 - Var(vs - v) / Var(vs) and the sampled entropy.  Reported per training step as `training/approx_kl`,
    `training/clip_fraction`, `training/explained_variance`, `training/entropy` (means over ALL minibatches evaluated in the step) and
    `training/approx_kl_max`; the four loss keys keep their last-minibatch meaning.  The sums live in device memory (the loss kernels'
    DIAG instances on the fused path, persistent tensors elsewhere) and are read and cleared after the closing synchronisation.
    `target_kl` (default None; a finite number > 0, anything else raises ValueError): the early stop of Spinning Up and Stable-Baselines3.
    Once a minibatch's approx_kl, measured before its own update, is not <= 1.5 * target_kl (that convention's factor; a NaN KL too), that
    update and every later one of the training step is not applied; the host reads the flag once per pass over the batch and leaves
    the loops.  `training/stopped_updates` counts the evaluated updates that were not applied.
    `learning_rate_schedule="adaptive_kl"` (default None = constant) with `desired_kl` and `learning_rate_bounds`: rsl_rl's rule, before
    the update of the minibatch whose KL was measured: kl > 2 desired_kl: lr = max(lo, lr / 1.5); 0 < kl < desired_kl / 2: lr = min(hi,
    lr * 1.5).  `learning_rate` must lie inside the bounds.  The three defaults (0.01, (1e-5, 1e-2)) are rsl_rl's and untuned here.
    `training/learning_rate` is the value after the step's last update.  Both controls decide on the device, inside the clipped Adam
    step, from a KL that travels behind the gradients through their all-reduce, so every rank takes the same decision; with
    `max_grad_norm=None` they therefore REPLACE torch.optim.Adam by `training.optim.ClippedAdam(max_grad_norm=inf)` on that path (the
    `training/grad_*` keys are reported too).  Whether either control trains the rodent better has not been measured.
    """
    if max_grad_norm is not None:
        max_grad_norm = optim.check_max_grad_norm(max_grad_norm)
    if learning_rate_schedule not in (None, "adaptive_kl"):
        raise ValueError(f"learning_rate_schedule must be None or 'adaptive_kl', got {learning_rate_schedule!r}")
    if target_kl is not None:
        target_kl = optim.check_target_kl(target_kl)
    adaptive_lr = learning_rate_schedule == "adaptive_kl"
    if adaptive_lr:
        desired_kl, *learning_rate_bounds = optim.check_adaptive_kl(learning_rate, desired_kl, learning_rate_bounds)
    kl_control = target_kl is not None or adaptive_lr
    diagnostics = bool(learner_diagnostics) or kl_control
    assert batch_size * num_minibatches % num_envs == 0
    xt = time.time()
    process_count, process_id = D.world_size(), D.rank()
    device_count = process_count                         # one device per process
    if num_envs % device_count:
        raise ValueError("num_envs must be divisible by the number of ranks")
    local_num_envs = num_envs // device_count
    env_step_per_training_step = batch_size * unroll_length * num_minibatches * action_repeat
    num_evals_after_init = max(num_evals - 1, 1)
    num_training_steps_per_epoch = int(np.ceil(
        num_timesteps / (num_evals_after_init * env_step_per_training_step * max(num_resets_per_eval, 1))))

    env = _local_env(environment, local_num_envs, getattr(environment, "device", None))
    device = env.device
    # domain randomisation: `randomization_fn(sys, rng)` with the rank's keys bound, one key per env; the parameters stay with the env
    rand_fn = eval_rand_fn = None
    if randomization_fn is not None:
        import functools
        rand_keys, eval_rand_keys = randomization_keys(seed, process_id, local_num_envs, num_eval_envs)
        rand_fn = functools.partial(randomization_fn, rng=rand_keys)
        eval_rand_fn = functools.partial(randomization_fn, rng=eval_rand_keys)
    wenv = wrappers.wrap(env, episode_length=episode_length, action_repeat=action_repeat, randomization_fn=rand_fn)

    # ---- keys [UP ppo.train]: reset keys follow the jax key tree so initial states match the reference
    key = jax_random.PRNGKey(seed)
    global_key, local_key = jax_random.split(key)
    local_key = jax_random.fold_in(local_key, process_id)
    local_key, key_env, eval_key = jax_random.split(local_key, 3)
    key_envs = jax_random.split(key_env, local_num_envs)
    gen = torch.Generator(device=device)
    gen.manual_seed(int(local_key[0]) * 2 ** 32 + int(local_key[1]))
    torch.manual_seed(int(global_key[0]) * 2 ** 32 + int(global_key[1]))     # identical parameter init on every rank
    perm_gen = torch.Generator(device="cpu")
    perm_gen.manual_seed(int(local_key[1]))

    # Optional (RR_ROLLOUT_SUBSTREAMS=2): the rollouts as S sub-batches on S streams, each unroll replayed from a HIP graph
    # (acting.SubBatchRollout).  Off by default: it pays for the bare env step (bench config 2: 1.49 -> 1.43 ms) but not here --
    # measured 1.22 s against 1.05 s of rollout per training step, because the 256-VGPR policy forward of one sub-batch cannot
    # be placed while the other sub-batch's step kernel fills the register files, so the two streams end up taking turns.
    n_sub_streams = int(os.environ.get("RR_ROLLOUT_SUBSTREAMS", "1"))
    sub_rollout = None
    if (device.type == "cuda" and n_sub_streams > 1 and hasattr(env, "with_num_envs") and local_num_envs % n_sub_streams == 0
            and local_num_envs // n_sub_streams >= int(os.environ.get("RR_ROLLOUT_SUBSTREAMS_MIN_ENVS", "512"))):
        sub_rollout = acting.SubBatchRollout(env, n_sub_streams, device, episode_length, action_repeat, unroll_length,
                                             seed=int(local_key[1]) % (2 ** 31), use_graph=os.environ.get("RR_ROLLOUT_GRAPH", "1") == "1")
        sub_rollout.reset(key_envs)
        env_state = None
    else:
        env_state = wenv.reset(key_envs)

    ppo_network = network_factory(env.observation_size, env.action_size, device=device)
    dist = ppo_network.parametric_action_distribution
    policy_net, value_net = ppo_network.policy_network, ppo_network.value_network
    params = list(policy_net.parameters()) + list(value_net.parameters())
    if process_count > 1:                                # replicate (rank 0's init), like device_put_replicated
        for p in params:
            torch.distributed.broadcast(p.data, src=0)
    # the KL controls read the minibatch's approx_kl from the first of four slots behind the gradients (four: what follows stays float4-aligned)
    flat = D.FlatGrads(params, extra=4) if kl_control else D.FlatGrads(params)
    # optax.adam(lr): b1=.9, b2=.999, eps=1e-8, eps outside the sqrt -- torch.optim.Adam's update; one fused
    # multi-tensor launch per step on the GPU
    # One process on a GPU: the minibatch update (gather, normalise, both MLPs forward + backward, GAE kernel, fused Adam) is
    # captured once in a HIP graph and replayed -- ~70 small launches per update otherwise leave the GPU idle between them
    # (half of the learner's wall time at the launcher's sizes).  RR_PPO_GRAPH=0 keeps the eager path.
    # Several ranks: the same capture split in two around the gradient all-reduce -- graph A (gather .. backward), the RCCL
    # all-reduce of the flat gradient buffer issued eagerly, graph B (fused Adam) -- so a multi-GPU run keeps the replayed
    # learner instead of falling back to ~70 eager launches per minibatch.  (The optional global advantage normalisation
    # puts a collective inside the loss: that mode runs eagerly.)
    use_graph = (device.type == "cuda" and os.environ.get("RR_PPO_GRAPH", "1") == "1"
                 and not (global_advantage_normalization and process_count > 1))
    if max_grad_norm is None and not kl_control:
        optimizer = torch.optim.Adam(params, lr=learning_rate, betas=(0.9, 0.999), eps=1e-8, fused=(device.type == "cuda"),
                                     capturable=use_graph)
    else:                                                # clip_by_global_norm -> adam, non-finite updates skipped: rr_clipped_adam_step
        optimizer = optim.ClippedAdam(params, flat, lr=learning_rate, max_grad_norm=float("inf") if max_grad_norm is None else max_grad_norm,
                                      betas=(0.9, 0.999), eps=1e-8, target_kl=target_kl, desired_kl=desired_kl if adaptive_lr else None,
                                      learning_rate_bounds=tuple(learning_rate_bounds) if adaptive_lr else None)
    clipped_adam = isinstance(optimizer, optim.ClippedAdam)
    clip_stats = {"warned": False}
    normalizer_params = running_statistics.init_state(env.observation_size, device)
    normalize = running_statistics.normalize if normalize_observations else (lambda x, y: x)
    make_policy = ppo_networks_mod.make_inference_fn(ppo_network)
    training_state = TrainingState(optimizer_state=optimizer, params=PPONetworkParams(policy=policy_net, value=value_net),
                                   normalizer_params=normalizer_params, env_steps=torch.zeros((), dtype=torch.int64))

    def current_params():
        return (normalizer_params if normalize_observations else None, policy_net)

    if eval_env is None and num_evals > 0 and num_eval_envs > 0:
        eval_env = _local_env(environment, num_eval_envs, device) if hasattr(environment, "with_num_envs") or \
            getattr(environment, "num_envs", None) == num_eval_envs else None
    if eval_rand_fn is not None and eval_env is env and hasattr(environment, "with_num_envs"):
        eval_env = environment.with_num_envs(num_eval_envs, device)     # its own batch: the eval env carries its own draws
    evaluator = None
    if eval_env is not None:
        weval = wrappers.wrap(eval_env, episode_length=episode_length, action_repeat=action_repeat, randomization_fn=eval_rand_fn)
        # evaluation as one launch (rr_env_unroll_eval, RR_FUSED_EVAL=1) under the conditions of the one-launch rollout; the Evaluator
        # itself checks the env.  Off by default: it measured no faster than the per-step loop
        actor_fn = None
        if action_repeat == 1 and acting.fused_unroll_supported(weval, policy_net, dist):
            actor_fn = lambda p: acting.actor_params(p[1], p[0], dist.min_std)
        evaluator = acting.Evaluator(weval, lambda p: make_policy(p, deterministic=deterministic_eval), num_eval_envs,
                                     episode_length, action_repeat, eval_key, actor_fn=actor_fn, deterministic=deterministic_eval)

    U = batch_size * num_minibatches // num_envs
    N, T = local_num_envs, unroll_length
    buf = acting.UnrollBuffer(U, N, T, env.observation_size, env.action_size, device)
    local_batch = U * N // num_minibatches               # trajectories per rank per minibatch

    def sync():
        if device.type == "cuda":
            torch.cuda.synchronize(device)

    rollout_policy = {"fn": None, "norm": None}
    # rollouts as one launch per unroll (rr_env_unroll_policy) where the env / policy shapes allow; RR_FUSED_ROLLOUT=0 keeps per-step launches
    fused_rollout = (sub_rollout is None and action_repeat == 1 and os.environ.get("RR_FUSED_ROLLOUT", "1") == "1"
                     and acting.fused_unroll_supported(wenv, policy_net, dist))
    gstate = {"graph": None, "graph_b": None, "calls": 0, "idx": None, "norm": None, "metrics": None, "failed": False}

    def adv_stats(adv):
        """mean / std of the advantages over the GLOBAL minibatch (all ranks): one all-reduce of {n, sum, sum of squares}."""
        st = torch.stack([torch.tensor(float(adv.numel()), device=adv.device), adv.sum(), (adv * adv).sum()])
        D.all_reduce_sum_(st)
        mean = st[1] / st[0]
        return mean, torch.sqrt(torch.clamp(st[2] / st[0] - mean * mean, min=0.0))

    # forward of both networks on the hand-written f32-MFMA kernel (one launch, observation tile read once for both nets,
    # normalisation fused) with an explicit backward; nn.Linear path for other shapes / CPU (RR_FUSED_MLP=0 forces it).  Policy heads of
    # 65 .. 128 logits (rodent_cpu.xml: 76) take this path only with RR_FUSED_WIDE_HEAD=1 (`fused_mlp.max_policy_head`)
    # A policy with 256-wide hidden layers (`fused_mlp.policy_width`) takes it too (RR_FUSED_POLICY256=0 keeps it off); its rollouts stay
    # per-step launches (`generate_unroll`: one forward launch + one sampling launch for all envs), the in-kernel actor is 32-wide only
    use_fused = (device.type == "cuda" and os.environ.get("RR_FUSED_MLP", "1") == "1"
                 and fused_mlp.fusable_policy(policy_net) and fused_mlp.fusable(value_net, fused_mlp.VALUE_HIDDEN, 1))

    # ... and the loss half + backward without an autograd graph (`fused_update`: rr_ppo_loss, gradients written straight into the
    # flat buffer).  RR_FUSED_LOSS=0 keeps compute_ppo_loss + loss.backward() on the fused forward.
    fused_update_fn = None
    if use_fused and os.environ.get("RR_FUSED_LOSS", "1") == "1" and not (global_advantage_normalization and process_count > 1):
        from . import fused_update
        fused_update_fn = fused_update.FusedUpdate(policy_net, value_net, dist, T, entropy_cost=entropy_cost, discounting=discounting,
                                                   reward_scaling=reward_scaling, gae_lambda=gae_lambda, clipping_epsilon=clipping_epsilon,
                                                   normalize_advantage=normalize_advantage, diagnostics=diagnostics,
                                                   kl_out=flat.tail[:1] if kl_control else None)
    # diagnostics of the autograd and CPU paths: a persistent float64 tensor laid out as the fused path's block and updated in place, so a
    # captured graph replays the additions
    diag_acc = None
    if diagnostics and fused_update_fn is None:
        diag_acc = torch.zeros(hip.DIAG_DOUBLES, dtype=torch.float64, device=device)

    def fwd_bwd(data, idx, nparams):
        if fused_update_fn is not None:
            mean, std = (nparams.mean, nparams.std) if normalize_observations else (None, None)
            return fused_update_fn(data, idx, mean, std, gen)
        mbd = {k: data[k][idx].transpose(0, 1) for k in ("raw_action", "log_prob", "reward", "discount", "truncation")}
        if use_fused:
            raw = data["obs"][idx].transpose(0, 1)                         # [T+1, B, obs], time-major gather
            B_ = raw.shape[1]
            mean, std = (nparams.mean, nparams.std) if normalize_observations else (None, None)
            logits_all, values_all = fused_mlp.actor_critic(raw.reshape((T + 1) * B_, -1), mean, std, policy_net, value_net)
            policy_logits = logits_all[:T * B_].reshape(T, B_, -1)        # the bootstrap row's logits carry no gradient
            values = values_all.reshape(T + 1, B_)
        else:
            obs = normalize(data["obs"][idx].transpose(0, 1), nparams)     # [T+1, B, obs]
            policy_logits = policy_net(obs[:T])
            values = value_net(obs).squeeze(-1)
        loss, m = ppo_losses.compute_ppo_loss(
            policy_logits, values[:T], values[T], mbd, dist, entropy_cost=entropy_cost, discounting=discounting,
            reward_scaling=reward_scaling, gae_lambda=gae_lambda, clipping_epsilon=clipping_epsilon,
            normalize_advantage=normalize_advantage, generator=gen,
            advantage_stats_fn=adv_stats if (global_advantage_normalization and process_count > 1) else None, diagnostics=diagnostics)
        flat.zero_()
        loss.backward()
        if diagnostics:
            kl, cf, ev, ent = (m.pop(k) for k in ("approx_kl", "clip_fraction", "explained_variance", "entropy"))
            diag_acc[hip.DIAG_COUNT] += 1.0
            diag_acc[hip.DIAG_KL_SUM] += kl
            diag_acc[hip.DIAG_KL_MAX] = torch.fmax(diag_acc[hip.DIAG_KL_MAX], kl)       # fmax: a NaN KL does not erase the maximum (the kernel's fmax)
            diag_acc[hip.DIAG_CLIP_SUM] += cf
            diag_acc[hip.DIAG_EV_SUM] += ev
            diag_acc[hip.DIAG_ENT_SUM] += ent
            if kl_control:
                flat.tail[0] = kl.float()                    # rounded to float32 once; averaged over the ranks with the gradients
        return m

    def eager_update(data, idx, nparams):
        m = fwd_bwd(data, idx, nparams)
        flat.pmean_()                            # jax.lax.pmean(grads, 'i')
        optimizer.step()
        return m

    def minibatch_update(data, idx):
        if not use_graph or gstate["failed"]:
            return eager_update(data, idx, normalizer_params)
        gstate["calls"] += 1
        if gstate["graph"] is None:
            if gstate["calls"] <= 3:             # first updates run eagerly: they create the Adam state and the GEMM workspaces
                return eager_update(data, idx, normalizer_params)
            try:                                 # 4th update: capture it, then run it by replaying the capture
                gstate["idx"] = idx.clone()
                gstate["norm"] = normalizer_params.clone() if normalize_observations else None
                g = torch.cuda.CUDAGraph()
                if hasattr(g, "register_generator_state"):
                    g.register_generator_state(gen)
                torch.cuda.synchronize(device)
                npar = gstate["norm"] if normalize_observations else normalizer_params
                if process_count == 1:
                    with torch.cuda.graph(g, capture_error_mode="thread_local"):
                        gstate["metrics"] = eager_update(data, gstate["idx"], npar)
                else:                            # capture records, it does not run: both halves are replayed below
                    with torch.cuda.graph(g, capture_error_mode="thread_local"):
                        gstate["metrics"] = fwd_bwd(data, gstate["idx"], npar)
                    gb = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(gb, capture_error_mode="thread_local"):
                        optimizer.step()
                    gstate["graph_b"] = gb
                gstate["graph"] = g
            except Exception as e:               # keep training on the eager path
                gstate["failed"] = True
                gstate["graph"] = gstate["graph_b"] = None
                logging.warning("PPO update graph capture failed (%s); continuing eagerly", e)
                return eager_update(data, idx, normalizer_params)
        gstate["idx"].copy_(idx)
        gstate["graph"].replay()
        if gstate["graph_b"] is not None:
            flat.pmean_()
            gstate["graph_b"].replay()
        return gstate["metrics"]

    D.time_collectives(timing_fn is not None)

    # Models with candidate-pair contacts (rodent_cpu.xml) drop the pairs in penetration beyond the kernel's contact slots and count the
    # (env, env step) events: reported as training/contact_overflow (events since the previous report), with one warning.  The counter is
    # read after the training step's closing synchronisation, never inside the rollout.
    overflow_envs = []
    if getattr(getattr(env, "sys", None), "candidate_contacts", False) and hasattr(env, "contact_overflow"):
        overflow_envs = [sub["env"] for sub in sub_rollout.subs] if sub_rollout is not None else [env]
    overflow = {"total": 0, "reported": 0, "warned": False}
    # Envs built with the bad-state check (Rodent(bad_state_max=...)) end and restore an episode whose qpos / qvel is non-finite or beyond the
    # threshold, and count the (env, env step) events: reported as training/bad_state_resets (events since the previous report), with one
    # warning.  Read next to the counter above, after the closing synchronisation.  The env carries the setting; off: no metric.
    bad_envs = []
    if getattr(env, "bad_state_max", None) and hasattr(env, "bad_states"):
        bad_envs = [sub["env"] for sub in sub_rollout.subs] if sub_rollout is not None else [env]
    bad = {"total": 0, "reported": 0, "warned": False}
    # Envs built with the outcome counters (Rodent(clip_outcomes=True)): read and cleared after the closing synchronisation, like the two
    # counters above.  The env carries the setting; off: no metric, and `clip_weight_fn` has nothing to be called with.
    outcome_envs = []
    if (getattr(env, "clip_sampling", None) or {}).get("outcomes") is not None:
        outcome_envs = [sub["env"] for sub in sub_rollout.subs] if sub_rollout is not None else [env]
    elif clip_weight_fn is not None:
        raise ValueError("ppo.train: clip_weight_fn needs an environment built with clip_outcomes=True (it is called with the outcome table)")

    def clip_outcome_metrics(out):
        table = sum(e.clip_outcomes(clear=True) for e in outcome_envs)      # int64 [C, 5]
        if process_count > 1:
            t = torch.from_numpy(np.ascontiguousarray(table)).to(device)
            table = D.all_reduce_sum_(t).cpu().numpy()
        ended = table[:, 0]
        rate = lambda num, den: float(num) / float(den) if den else 0.0
        out["training/clip_fail_rate"] = rate(table[:, 1].sum() + table[:, 2].sum(), ended.sum())
        out["training/clip_truncated_share"] = rate(table[:, 3].sum(), ended.sum())
        if table.shape[0] <= 16:
            for c in range(table.shape[0]):
                out[f"training/clip_fail_rate_clip{c}"] = rate(table[c, 1] + table[c, 2], ended[c])
        if clip_weight_fn is not None:
            w = clip_weight_fn(table)
            if w is not None:
                for e in outcome_envs:
                    e.set_clip_weights(w)

    def training_step():
        nonlocal env_state, normalizer_params
        t0 = time.time()
        if sub_rollout is not None:
            if rollout_policy["fn"] is None:             # ONE policy object for all training steps: the captured graphs hold it;
                rollout_policy["norm"] = normalizer_params.clone() if normalize_observations else None     # it reads these buffers
                rollout_policy["fn"] = make_policy((rollout_policy["norm"], policy_net))
            elif normalize_observations:
                for f in ("count", "mean", "summed_variance", "std"):
                    getattr(rollout_policy["norm"], f).copy_(getattr(normalizer_params, f))
            for u in range(U):
                sub_rollout.unroll(rollout_policy["fn"], buf, u)
            sub_rollout.join()
        elif fused_rollout:                              # generate_unroll as ONE launch per unroll: the actor runs inside the kernel
            actor = acting.actor_params(policy_net, normalizer_params if normalize_observations else None, dist.min_std)
            if os.environ.get("RR_FUSED_ROLLOUT_PHASE", "1") == "1":     # the whole rollout phase (U unrolls, same policy) as ONE launch
                env_state = acting.generate_unrolls_fused(wenv, env_state, actor, buf, gen)
            else:
                for u in range(U):
                    env_state = acting.generate_unroll_fused(wenv, env_state, actor, buf, u, gen)
        else:
            policy = make_policy(current_params())
            for u in range(U):
                env_state = acting.generate_unroll(wenv, env_state, policy, buf, u, gen)
        sync()
        t1 = time.time()
        data = buf.flat()
        if normalize_observations:                       # update on `observation` (not next_observation), all ranks
            normalizer_params = running_statistics.update_from_unroll_buffer(normalizer_params, buf.obs, T)
        metrics = {}
        if normalize_observations and gstate["norm"] is not None:     # the graph reads the normaliser from fixed buffers
            for f in ("count", "mean", "summed_variance", "std"):
                getattr(gstate["norm"], f).copy_(getattr(normalizer_params, f))
        if kl_control:
            optimizer.begin_training_step()              # clears the sticky stop flag of target_kl
        for _ in range(num_updates_per_batch):
            perm = torch.randperm(U * N, generator=perm_gen).to(device)
            for mb in range(num_minibatches):
                idx = perm[mb * local_batch:(mb + 1) * local_batch]
                metrics = minibatch_update(data, idx)
            # target_kl: one 8-byte read per pass, so that no pass is spent on updates that can change nothing.  The flag derives from the
            # all-reduced KL: every rank reads the same value and leaves together
            if target_kl is not None and optimizer.stopped:
                break
        sync()
        t2 = time.time()
        training_state.normalizer_params = normalizer_params
        training_state.env_steps += env_step_per_training_step          # int64 (upstream: int32, which wraps past 2.1e9 steps)
        if timing_fn is not None:
            # allreduce_s: the part of learner_s spent in the gradient / normaliser all-reduces as the learner's stream sees them
            # (0 on one rank); SURVEY.md 8(d): rollout / learner / all-reduce
            timing_fn({"rollout_s": t1 - t0, "learner_s": t2 - t1, "allreduce_s": D.pop_collective_seconds(),
                       "env_steps": env_step_per_training_step})
        out = {f"training/{k}": float(v) for k, v in metrics.items()}
        if overflow_envs:
            overflow["total"] = sum(e.contact_overflow() for e in overflow_envs)
            out["training/contact_overflow"] = float(overflow["total"] - overflow["reported"])
            if overflow["total"] and not overflow["warned"]:
                overflow["warned"] = True
                warnings.warn(f"ppo.train: {overflow['total']} (env, step) events so far with more than 64 contact pairs in penetration; the "
                              "surplus pairs were dropped for those substeps (training/contact_overflow counts them)", RuntimeWarning, stacklevel=2)
        if bad_envs:
            bad["total"] = sum(e.bad_states() for e in bad_envs)
            out["training/bad_state_resets"] = float(bad["total"] - bad["reported"])
            if bad["total"] and not bad["warned"]:
                bad["warned"] = True
                warnings.warn(f"ppo.train: {bad['total']} (env, step) events so far in which an env's qpos / qvel was non-finite or beyond "
                              f"bad_state_max = {env.bad_state_max:g}; those episodes were ended and restored "
                              "(training/bad_state_resets counts them)", RuntimeWarning, stacklevel=2)
        if outcome_envs:
            clip_outcome_metrics(out)
        if diagnostics:                                  # read and cleared next to the optimiser's block below
            blk = fused_update_fn.diag if fused_update_fn is not None else diag_acc
            dg = blk.tolist()                            # a copy: the block is cleared next
            blk[hip.DIAG_COUNT:hip.DIAG_ENT_SUM + 1].zero_()
            cnt = max(float(dg[hip.DIAG_COUNT]), 1.0)
            out.update({"training/approx_kl": float(dg[hip.DIAG_KL_SUM]) / cnt, "training/approx_kl_max": float(dg[hip.DIAG_KL_MAX]),
                        "training/clip_fraction": float(dg[hip.DIAG_CLIP_SUM]) / cnt, "training/explained_variance": float(dg[hip.DIAG_EV_SUM]) / cnt,
                        "training/entropy": float(dg[hip.DIAG_ENT_SUM]) / cnt})
        if clipped_adam:                                 # the optimiser's device block: read and cleared here, after the closing synchronisation
            st = optimizer.stats(clear=True)
            if target_kl is not None:
                out["training/stopped_updates"] = float(st["stopped_updates"])
            if adaptive_lr:
                out["training/learning_rate"] = float(st["learning_rate"])
            for k in ("grad_norm", "grad_norm_max", "grad_clip_share", "skipped_updates"):
                out[f"training/{k}"] = float(st[k])
            if st["skipped_updates"] and not clip_stats["warned"]:
                clip_stats["warned"] = True
                warnings.warn(f"ppo.train: {st['skipped_updates']} of {st['skipped_updates'] + st['applied_updates']} minibatch updates of this "
                              "training step had a gradient with a non-finite element and were skipped: parameters and optimiser state kept "
                              "(training/skipped_updates counts them)", RuntimeWarning, stacklevel=2)
        return out

    metrics = {}
    if process_id == 0 and evaluator is not None and num_evals > 1:
        metrics = evaluator.run_evaluation(current_params(), training_metrics={})
        progress_fn(0, metrics)

    training_metrics = {}
    training_walltime = 0.0
    current_step = 0
    steps_done = 0
    stop = False
    for it in range(num_evals_after_init):
        for _ in range(max(num_resets_per_eval, 1)):
            t = time.time()
            for _ in range(num_training_steps_per_epoch):
                training_metrics = training_step()
                steps_done += 1
                if max_training_steps is not None and steps_done >= max_training_steps:
                    stop = True
                    break
            epoch_training_time = time.time() - t
            training_walltime += epoch_training_time
            done_steps = steps_done if stop else num_training_steps_per_epoch
            sps = (min(done_steps, num_training_steps_per_epoch) * env_step_per_training_step) / epoch_training_time
            training_metrics = {"training/sps": sps, "training/walltime": training_walltime, **training_metrics}
            current_step = steps_done * env_step_per_training_step
            if num_resets_per_eval > 0 and not stop:
                local_key, key_env = jax_random.split(local_key)
                if sub_rollout is not None:
                    sub_rollout.reset(jax_random.split(key_env, local_num_envs))
                else:
                    env_state = wenv.reset(jax_random.split(key_env, local_num_envs))
            if stop:
                break
        if process_id == 0:
            if evaluator is not None:
                metrics = evaluator.run_evaluation(current_params(), training_metrics)
            else:
                metrics = dict(training_metrics)
            progress_fn(current_step, metrics)
            overflow["reported"] = overflow["total"]
            bad["reported"] = bad["total"]
            # callbacks get a SNAPSHOT (the live network keeps training)
            policy_params_fn(current_step, make_policy, params_tuple(normalizer_params.clone(), copy.deepcopy(policy_net).requires_grad_(False),
                                                                     normalize_observations))
        if stop:
            break

    total_steps = current_step
    if max_training_steps is None:
        assert total_steps >= num_timesteps
    if process_count > 1:                                # pmap.assert_is_replicated / synchronize_hosts
        chk = torch.stack([p.detach().float().sum() for p in params]).sum().reshape(1)
        lo, hi = chk.clone(), chk.clone()
        torch.distributed.all_reduce(lo, op=torch.distributed.ReduceOp.MIN)
        torch.distributed.all_reduce(hi, op=torch.distributed.ReduceOp.MAX)
        assert torch.allclose(lo, hi, rtol=1e-5, atol=1e-6), "parameters diverged across ranks"
    out = (make_policy, params_tuple(normalizer_params, policy_net, normalize_observations), metrics)
    return out + (training_state,) if return_training_state else out


def params_tuple(normalizer_params, policy_net, normalize_observations: bool):
    """(normalizer_params, policy_params) as the reference's callbacks receive them."""
    return (normalizer_params if normalize_observations else None, policy_net)
