"""Training wrappers with the semantics of `brax.envs.wrappers.training`, batched.

The env is batched by construction, so `VmapWrapper` only validates shapes.  `EpisodeWrapper`
maintains `info['steps']` / `info['truncation']`; `AutoResetWrapper` selects the stored first
state back on `done` -- no re-randomisation and `info` (hence `cur_frame`) is NOT restored, exactly
as upstream.  The same holds for `info['clip']` of a multi-clip env: an env keeps
its clip across restores.  `reset(rng, **kw)` hands keyword arguments (`clip=`) down to the env.

An env with clip restarts (`Rodent(clip_restarts=K)`, K >= 1) is wrapped by `ClipEpisodeWrapper` and `ClipAutoResetWrapper` instead: the
clip's end may truncate the episode, and a restore takes the next entry of the env's start bank -- state, observation AND frame.
With the clip library (`Rodent(clip_lengths=..., restart_across_clips=True)`) the clip's end is that of the env's own clip, and the restore
also takes the entry's clip: `info['clip']` then changes at a restore.  With clip sampling (`Rodent(restart_sampling="weighted",
clip_outcomes=True)`) the restore draws its entry by the clips' weights and every wrapped step is counted per clip, in integers.
"""
from __future__ import annotations

import dataclasses

import torch

from .base import PipelineState, State


def _tree_map2(fn, a, b):
    """Apply fn leaf-wise over two identically structured pytrees (dataclass / dict / tensor / None)."""
    if a is None:
        return None
    if torch.is_tensor(a):
        return fn(a, b)
    if dataclasses.is_dataclass(a):
        return type(a)(**{f.name: _tree_map2(fn, getattr(a, f.name), getattr(b, f.name)) for f in dataclasses.fields(a)})
    if isinstance(a, dict):
        return {k: _tree_map2(fn, a[k], b[k]) for k in a}
    raise TypeError(type(a))


class Wrapper:
    def __init__(self, env):
        self.env = env

    def __getattr__(self, name):
        if name == "__setstate__":
            raise AttributeError(name)
        return getattr(self.env, name)

    def reset(self, rng, **kw):
        return self.env.reset(rng, **kw)

    def step(self, state, action):
        return self.env.step(state, action)

    @property
    def unwrapped(self):
        return self.env.unwrapped if hasattr(self.env, "unwrapped") else self.env


class VmapWrapper(Wrapper):
    """No-op: the HIP env already carries the leading env axis."""

    def __init__(self, env, batch_size=None):
        super().__init__(env)
        if batch_size is not None and batch_size != env.num_envs:
            raise ValueError(f"batch_size {batch_size} != env.num_envs {env.num_envs}")


class EpisodeWrapper(Wrapper):
    """Maintains episode step count and sets done at episode end."""

    def __init__(self, env, episode_length: int, action_repeat: int):
        super().__init__(env)
        self.episode_length = episode_length
        self.action_repeat = action_repeat

    def reset(self, rng, **kw):
        state = self.env.reset(rng, **kw)
        state.info["steps"] = torch.zeros_like(state.reward)
        state.info["truncation"] = torch.zeros_like(state.reward)
        return state

    def step(self, state, action):
        total = None
        nstate = state
        for _ in range(self.action_repeat):
            nstate = self.env.step(nstate, action)
            total = nstate.reward if total is None else total + nstate.reward
        state = nstate.replace(reward=total)
        steps = state.info["steps"] + self.action_repeat
        one, zero = torch.ones_like(state.done), torch.zeros_like(state.done)
        over = steps >= self.episode_length
        done = torch.where(over, one, state.done)
        state.info["truncation"] = torch.where(over, 1 - state.done, zero)
        state.info["steps"] = steps
        return state.replace(done=done)


class AutoResetWrapper(Wrapper):
    """Automatically resets Brax envs that are done (to the FIRST state of the batch member)."""

    def reset(self, rng, **kw):
        state = self.env.reset(rng, **kw)
        state.info["first_pipeline_state"] = state.pipeline_state
        state.info["first_obs"] = state.obs
        return state

    def step(self, state, action):
        if "steps" in state.info:
            steps = state.info["steps"]
            steps = torch.where(state.done.bool(), torch.zeros_like(steps), steps)
            state.info.update(steps=steps)
        state = state.replace(done=torch.zeros_like(state.done))
        state = self.env.step(state, action)
        done = state.done.bool()

        def where_done(x, y):
            d = done.reshape((-1,) + (1,) * (x.dim() - 1))
            return torch.where(d, x, y)

        new_ps = _tree_map2(where_done, state.info["first_pipeline_state"], state.pipeline_state)
        obs = where_done(state.info["first_obs"], state.obs)
        return state.replace(pipeline_state=new_ps, obs=obs)


def _base(env):
    return env.unwrapped if hasattr(env, "unwrapped") else env


class ClipEpisodeWrapper(EpisodeWrapper):
    """`EpisodeWrapper` of an env with clip restarts: with `end_at_clip_end` the episode also ends -- a truncation, like
    `episode_length` -- when the stepped frame reaches the clip's last one, new_frame >= T - 1: the new state's observation has no next
    frame left to read without clamping.  An env with `clip_lengths` (int [C], on the env's device) ends at its own clip's length:
    new_frame >= L_c - 1, c = `info['clip']` after the step (clip 0 without ids)."""

    def step(self, state, action):
        total = None
        nstate = state
        for _ in range(self.action_repeat):
            nstate = self.env.step(nstate, action)
            total = nstate.reward if total is None else total + nstate.reward
        state = nstate.replace(reward=total)
        steps = state.info["steps"] + self.action_repeat
        one, zero = torch.ones_like(state.done), torch.zeros_like(state.done)
        over = steps >= self.episode_length
        base = _base(self.env)
        if base.end_at_clip_end:
            lengths = getattr(base, "clip_lengths", None)
            if lengths is None:
                over = over | (state.info["cur_frame"] >= base.track_len - 1)
            else:
                own = lengths[state.info["clip"].long()] if "clip" in state.info else lengths[0]
                over = over | (state.info["cur_frame"] >= own - 1)
        done = torch.where(over, one, state.done)
        state.info["truncation"] = torch.where(over, 1 - state.done, zero)
        state.info["steps"] = steps
        return state.replace(done=done)


_M32 = 0xFFFFFFFF


def _fmix32(h):
    """MurmurHash3's 32-bit finaliser on int64 tensors holding 32-bit values (a product's low 32 bits survive the int64 wrap-around)."""
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & _M32
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & _M32
    return h ^ (h >> 16)


def weighted_slots(weights, bank_clips, seed: int, draws):
    """`rodent.weighted_slot` for every env at once, in torch integers: `weights` int32 [C], `bank_clips` int32 [K, N], `draws` int32 [N]
    -> int64 [N], the drawn slot, -1 where every entry of the env's bank has weight 0."""
    q = (weights.long() & 0xFFFF)[bank_clips.long().clamp(0, weights.shape[0] - 1)]      # [K, N]
    prefix = q.cumsum(0)
    S = prefix[-1]
    env = torch.arange(bank_clips.shape[1], device=bank_clips.device)
    h = _fmix32((_fmix32((int(seed) & _M32) ^ ((env * 0x9E3779B1) & _M32)) + (draws.long() & _M32)) & _M32)
    r = (h * S) >> 32
    k = (prefix <= r).sum(0)            # prefixes never decrease: the count of those <= r is the first index with prefix > r
    return torch.where(S > 0, k, torch.full_like(k, -1))


def count_outcomes(outcomes, clip, failed, done_env, done):
    """`rodent.clip_outcome_update` in torch integers, added to the int64 [C, 5] device table `outcomes` in place: `clip` int64 [N],
    `failed` / `done_env` / `done` bool [N]."""
    flat, d = outcomes.view(-1), done.long()
    col = torch.where(failed, 1, torch.where(done_env, 2, 3))
    flat.index_add_(0, clip * 5 + 4, torch.ones_like(d))
    flat.index_add_(0, clip * 5, d)
    flat.index_add_(0, clip * 5 + col, d)


def _reference_restore(base, state, done, nslot):
    """The restore of an env with `restart_from_reference`: where `done`, state, observation, `cur_frame` and `info['clip']` come from
    `base.reference_restart` at the env's restore count (no bank entry is read), and `info['restart_draws']` grows by one; the slot
    advances cyclically (`nslot`) and selects nothing.  Cost: the per-step forms pay ONE forward-only launch (a reset of all N envs)
    per wrapped step, whether or not an env is done -- no host synchronisation, and a captured graph replays it -- and that launch
    clears the restart, library and sampling blocks of the batch, which the next step launch sets again.  The one-launch rollouts
    (`unroll`, `unroll_policy`) pay a forward pass per ended episode only."""
    draws = state.info["restart_draws"]
    ps, obs, frame, clip = base.reference_restart(state.info.get("clip"), draws)

    def where_done(x, y):
        return torch.where(done.reshape((-1,) + (1,) * (y.dim() - 1)), x, y)

    state.info["cur_frame"] = where_done(frame, state.info["cur_frame"])
    if clip is not None:
        state.info["clip"] = where_done(clip, state.info["clip"])
    state.info["restart_draws"] = draws + done.to(draws.dtype)
    state.info["restart_slot"] = nslot
    return state.replace(pipeline_state=_tree_map2(where_done, ps, state.pipeline_state), obs=where_done(obs, state.obs))


class ClipAutoResetWrapper(Wrapper):
    """`AutoResetWrapper` of an env with clip restarts: where done, the env takes the NEXT entry of its start bank
    (`info['restart_bank']`, built by the env's `reset`) -- slot' = (slot + 1) mod K; pipeline state, observation and `cur_frame` come
    from entry slot' -- so the restarted episode rejoins its clip at the frame its state was formed at.  Bank and slot are info: never
    re-drawn, never restored.  A bank with a `clip` leaf (`restart_across_clips`) also hands its entry's clip to `info['clip']`.  An env
    with `clip_sampling` tables (`Rodent(restart_sampling=..., clip_outcomes=...)`) has its steps counted on the clip they were made on,
    and its restores drawn by the clips' weights (`weighted_slots`; `info['restart_draws']` grows by one at every restore).  An env with
    `restart_from_reference` takes no bank entry: `_reference_restore`."""

    def step(self, state, action):
        if "steps" in state.info:
            steps = state.info["steps"]
            steps = torch.where(state.done.bool(), torch.zeros_like(steps), steps)
            state.info.update(steps=steps)
        state = state.replace(done=torch.zeros_like(state.done))
        state = self.env.step(state, action)
        done = state.done.bool()
        bank, slot = state.info["restart_bank"], state.info["restart_slot"]
        K = bank["frame"].shape[0]
        nslot = torch.where(done, (slot + 1) % K, slot)
        sampling = getattr(_base(self.env), "clip_sampling", None)
        if sampling is not None:
            if sampling["outcomes"] is not None:
                # the env's own done back out of the wrapped one: truncation = over ? 1 - done_env : 0, so done_env = done and no truncation
                own = done & (state.info["truncation"] == 0)
                failed = state.metrics["pose_fail"] != 0 if "pose_fail" in state.metrics else torch.zeros_like(done)
                on = state.info["clip"].long() if "clip" in state.info else torch.zeros_like(slot, dtype=torch.long)
                count_outcomes(sampling["outcomes"], on.clamp(0, sampling["outcomes"].shape[0] - 1), failed, own, done)
            if sampling["weights"] is not None and not getattr(_base(self.env), "restart_from_reference", False):
                draws = state.info["restart_draws"]
                drawn = weighted_slots(sampling["weights"], bank["clip"], sampling["seed"], draws)
                nslot = torch.where(done & (drawn >= 0), drawn.to(slot.dtype), nslot)
                state.info["restart_draws"] = draws + done.to(draws.dtype)
        if getattr(_base(self.env), "restart_from_reference", False):
            return _reference_restore(_base(self.env), state, done, nslot)
        row, env = nslot.long(), torch.arange(done.shape[0], device=done.device)

        def where_done(x, y):      # x: the bank's leaf [K, N, ...]
            d = done.reshape((-1,) + (1,) * (y.dim() - 1))
            return torch.where(d, x[row, env], y)

        new_ps = _tree_map2(where_done, bank["pipeline_state"], state.pipeline_state)
        obs = where_done(bank["obs"], state.obs)
        state.info["cur_frame"] = where_done(bank["frame"], state.info["cur_frame"])
        if "clip" in bank:
            state.info["clip"] = where_done(bank["clip"], state.info["clip"])
        state.info["restart_slot"] = nslot
        return state.replace(pipeline_state=new_ps, obs=obs)


class EvalWrapper(Wrapper):
    """Accumulates episode metrics for evaluation (brax EvalWrapper)."""

    def reset(self, rng, **kw):
        rs = self.env.reset(rng, **kw)
        rs.metrics["reward"] = rs.reward
        z = torch.zeros_like(rs.reward)
        rs.info["eval_metrics"] = dict(episode_metrics={k: torch.zeros_like(v) for k, v in rs.metrics.items()},
                                       active_episodes=torch.ones_like(rs.reward), episode_steps=z.clone())
        return rs

    def step(self, state, action):
        em = state.info["eval_metrics"]
        nstate = self.env.step(state, action)
        nstate.metrics["reward"] = nstate.reward
        steps = em["episode_steps"] + em["active_episodes"]
        ep = {k: em["episode_metrics"][k] + nstate.metrics[k] * em["active_episodes"] for k in em["episode_metrics"]}
        active = em["active_episodes"] * (1 - nstate.done)
        nstate.info["eval_metrics"] = dict(episode_metrics=ep, active_episodes=active, episode_steps=steps)
        return nstate


    EVAL_KEYS = ("pos_reward", "reward_quadctrl", "reward_alive", "reward")      # the order of the kernel's sums (rr_env_unroll_eval)

    def unroll_supported(self) -> bool:
        """`unroll_policy` needs this wrapper directly on the fused Episode + AutoReset wrapper of a HIP env with an evaluation instance."""
        base = self.env.unwrapped if hasattr(self.env, "unwrapped") else self.env
        return isinstance(self.env, FusedEpisodeAutoResetWrapper) and hasattr(base, "eval_supported") and base.eval_supported()

    def unroll_policy(self, state, actor, noise, T: int, actions_out=None, qpos_out=None):
        """T x [policy -> action -> `step`] in one launch (`Rodent.unroll_eval` / C ABI `rr_env_unroll_eval`): the state T calls of `step`
        on the same actions give, `info["eval_metrics"]` included.  `actor`: `acting.actor_params`; `noise` [T, N, A] or None (the
        deterministic policy); `actions_out` [T, N, A] / `qpos_out` [T + 1, N, nq] (optional) receive the actions taken / the qpos of every step."""
        if not self.unroll_supported():
            raise ValueError("EvalWrapper.unroll_policy: not directly on the fused wrapper of a HIP env with an evaluation instance")
        em = state.info["eval_metrics"]
        if set(em["episode_metrics"]) != set(self.EVAL_KEYS):
            raise ValueError(f"EvalWrapper.unroll_policy: the kernel sums exactly {self.EVAL_KEYS}")
        packed = torch.stack([em["episode_steps"], em["active_episodes"]] + [em["episode_metrics"][k] for k in self.EVAL_KEYS], dim=1).contiguous()
        base = self.env.unwrapped
        nstate = base.unroll_eval(state, T, actor, noise, episode_length=self.env.episode_length, eval_metrics=packed, actions_out=actions_out,
                                  qpos_out=qpos_out)
        nstate.metrics["reward"] = nstate.reward
        nstate.info["eval_metrics"] = dict(episode_metrics={k: packed[:, 2 + self.EVAL_KEYS.index(k)] for k in em["episode_metrics"]},
                                           active_episodes=packed[:, 1], episode_steps=packed[:, 0])
        return nstate


class FusedEpisodeAutoResetWrapper(Wrapper):
    """EpisodeWrapper + AutoResetWrapper of a HIP env with action_repeat 1: the same values, but the ~15 elementwise
    launches of the composed wrappers (step count, truncation, done, ten `where(done, first, current)` selects) are one
    launch of `rr_wrap_episode_autoreset` on the freshly produced state.  `tests/test_gpu_env.py` holds it to bitwise
    equality with the composition."""

    def __init__(self, env, episode_length: int):
        super().__init__(env)
        self.episode_length = episode_length
        self.action_repeat = 1

    def reset(self, rng, **kw):
        state = self.env.reset(rng, **kw)
        state.info["steps"] = torch.zeros_like(state.reward)
        state.info["truncation"] = torch.zeros_like(state.reward)
        if getattr(_base(self.env), "clip_restarts", 0) >= 1:      # the restores draw from info['restart_bank'], whose entry 0 is this state
            return state
        state.info["first_pipeline_state"] = state.pipeline_state
        state.info["first_obs"] = state.obs
        return state

    def step(self, state, action):
        from .. import hip
        nstate = self.env.step(state, action)              # fresh tensors: safe to finish in place
        base = _base(self.env)
        restarts = getattr(base, "clip_restarts", 0) >= 1  # clip restarts: the rule of the two Clip wrappers, the stored states a bank
        if restarts:
            bank = nstate.info["restart_bank"]
            fps, fobs = bank["pipeline_state"], bank["obs"]
        else:
            fps, fobs = nstate.info["first_pipeline_state"], nstate.info["first_obs"]
        ps = nstate.pipeline_state
        names = [f.name for f in dataclasses.fields(ps) if torch.is_tensor(getattr(ps, f.name))]
        first = [getattr(fps, n) for n in names] + [fobs]
        cur = [getattr(ps, n) for n in names] + [nstate.obs]
        steps, trunc = torch.empty_like(nstate.done), torch.empty_like(nstate.done)
        common = (first, cur, state.done, state.info["steps"], nstate.done, steps, trunc, self.episode_length, 1)
        nstate.info.update(steps=steps, truncation=trunc)
        if not restarts:
            hip.wrap_episode_autoreset(*common)
            return nstate
        slot = torch.empty_like(state.info["restart_slot"])
        lengths = getattr(base, "clip_lengths", None)
        sampling = getattr(base, "clip_sampling", None)
        ref = getattr(base, "restart_from_reference", False)
        if ref:      # reference restarts: the rule below with the cyclic slot (its restore is replaced after it), the counters as they are
            sampling = None if sampling is None or sampling["outcomes"] is None else dict(sampling, weights=None)
        # the clip library (the env's own clip's end, the entry's clip with its frame) and clip sampling (the counters and the weighted draw on
        # top of it) finish the clip ids, in a copy: the bare step leaves them alone
        library = lengths is not None or "clip" in bank or sampling is not None
        clip = state.info["clip"].clone() if library and "clip" in state.info else None
        draws = state.info.get("restart_draws") if sampling is not None else None
        ndraws = None if draws is None else torch.empty_like(draws)
        weights, outcomes, seed = (sampling["weights"], sampling["outcomes"], sampling["seed"]) if sampling is not None else (None, None, 0)
        hip.wrap_clip(*common, nstate.info["cur_frame"], bank["frame"], state.info["restart_slot"], slot, base.track_len, base.end_at_clip_end,
                      clip, bank.get("clip"), lengths, base.num_clips, nstate.metrics.get("pose_fail"), weights, draws, ndraws, outcomes, seed)
        nstate.info["restart_slot"] = slot
        if clip is not None:
            nstate.info["clip"] = clip
        if ndraws is not None:
            nstate.info["restart_draws"] = ndraws
        if ref:      # where done, the bank entry the launch above restored gives way to the freshly drawn start state
            for k in ("clip", "restart_draws"):
                if k in state.info:
                    nstate.info[k] = state.info[k]
            return _reference_restore(base, nstate, nstate.done.bool(), slot)
        return nstate


    def unroll(self, state, actions):
        """`actions` [T, N, nu]: T wrapped steps in one launch (`Rodent.unroll_wrapped` / C ABI `rr_env_unroll`); the state after the
        last step, equal to T calls of `step` bit for bit."""
        base = self.env.unwrapped if hasattr(self.env, "unwrapped") else self.env
        return base.unroll_wrapped(state, actions, self.episode_length)


    def unroll_policy(self, state, actor, noise, traj, segment: int = 0):
        """`acting.generate_unroll` in one launch: see `Rodent.unroll_policy_wrapped` (C ABI `rr_env_unroll_policy`).
        Returns (state after the last step, actions taken [T, N, nu])."""
        base = self.env.unwrapped if hasattr(self.env, "unwrapped") else self.env
        return base.unroll_policy_wrapped(state, self.episode_length, actor, noise, traj, segment)


def wrap(env, episode_length: int = 1000, action_repeat: int = 1, randomization_fn=None):
    """brax.envs.wrappers.training.wrap: Vmap -> Episode -> AutoReset (one fused wrapper for a HIP env with
    action_repeat 1; RR_FUSED_WRAPPERS=0 selects the composition; an env with `clip_restarts >= 1` gets the fused wrapper too, or
    `ClipEpisodeWrapper` -> `ClipAutoResetWrapper` as the composition).  `randomization_fn(sys) -> (sys_v, in_axes)` (keys already bound):
    brax puts a DomainRandomizationVmapWrapper in place of the VmapWrapper; here the env's batch takes the per-env parameters
    (`PipelineEnv.randomize`) and every later step of it, wrapped or not, runs on them."""
    import os
    base = env.unwrapped if hasattr(env, "unwrapped") else env
    if randomization_fn is not None:
        if not hasattr(base, "randomize"):
            raise ValueError("wrap: this environment does not take a randomization_fn")
        base.randomize(randomization_fn)
    if action_repeat == 1 and hasattr(base, "_batch") and os.environ.get("RR_FUSED_WRAPPERS", "1") == "1":
        return FusedEpisodeAutoResetWrapper(VmapWrapper(env), episode_length)
    env = VmapWrapper(env)
    if getattr(base, "clip_restarts", 0) >= 1:      # an env with a start bank: the clip's end and the restored frame
        return ClipAutoResetWrapper(ClipEpisodeWrapper(env, episode_length, action_repeat))
    env = EpisodeWrapper(env, episode_length, action_repeat)
    return AutoResetWrapper(env)
