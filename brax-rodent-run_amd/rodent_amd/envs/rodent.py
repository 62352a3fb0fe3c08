"""`Rodent`: the reference task env [REF Rodent_Env_Brax.py:19-162] on the HIP backend.

Same constructor arguments, `reset(rng)` / `step(state, action)` surface, reward / done / obs
arithmetic and `info['cur_frame']` bookkeeping as the reference; tensors are torch (leading env
axis N) instead of vmapped jax arrays.  `step` runs ONE fused kernel launch: n_frames physics
substeps + reward / done / observation epilogue (C ABI `rr_env_step`).
"""
from __future__ import annotations

import os
import warnings
from typing import Optional

import numpy as np
import torch

from .. import assets, jax_random
from .base import PipelineEnv, PipelineState, State, System

_XML_PATH = "./models/rodent_new.xml"   # [REF Rodent_Env_Brax.py:16]


def bad_state_mask(qpos: torch.Tensor, qvel: torch.Tensor, bad_state_max: float) -> torch.Tensor:
    """The bad-state rule of the step kernel's epilogue in plain torch: env e is bad iff some element x of qpos[e] or qvel[e] fails
    |x| <= bad_state_max (float32) -- written that way round, so NaN and +-inf are bad.  bool [N].  For tests and for users who compose the
    env step by step themselves (MuJoCo's mj_checkPos / mj_checkVel with mjMAXVAL = 1e10)."""
    lim = torch.tensor(float(bad_state_max), dtype=torch.float32, device=qpos.device)
    ok = lambda x: (x.to(torch.float32).abs() <= lim).flatten(1).all(dim=1)
    return ~(ok(qpos) & ok(qvel))


class Rodent(PipelineEnv):

    def __init__(
        self,
        track_pos,
        forward_reward_weight=10,
        ctrl_cost_weight=0.1,
        healthy_reward=1.0,
        terminate_when_unhealthy=True,
        healthy_z_range=(0.03, 0.5),
        reset_noise_scale=1e-2,
        solver="cg",
        iterations: int = 6,
        ls_iterations: int = 6,
        vision=False,
        num_envs: int = 1,
        xml_path: str = _XML_PATH,
        device=None,
        bad_state_max: Optional[float] = None,
        **kwargs,
    ):
        """`bad_state_max` (None = off, the default): the bad-state check of MuJoCo (`mj_checkPos` / `mj_checkVel`, there with
        mjMAXVAL = 1e10).  After an env step an env is bad when some element x of its qpos or qvel fails |x| <= bad_state_max (NaN and
        +-inf included); that step then has done = 1 (whatever `terminate_when_unhealthy` is), reward 0 and metrics 0, and is counted
        (`bad_states()`).  Under `AutoResetWrapper` -- composed or in the one-launch rollouts -- the first state comes back as for any
        finished episode, with no bootstrap from the bad step.  The bare `step` does NOT sanitise: it returns the bad state and its
        observation as they are, flagged by `done`; so does the raw evaluation form (`unroll_eval` without `episode_length`)."""
        if bad_state_max is not None:
            with np.errstate(over="ignore", under="ignore"):
                thr32 = np.float32(bad_state_max)        # what the kernel gets: 1e-50 would arrive as 0 (= off), 1e39 as inf
            if not (np.isfinite(thr32) and thr32 > 0):
                raise ValueError(f"bad_state_max must be finite and > 0 as a float32 (or None: no check), got {bad_state_max!r}")
        if solver.lower() not in ("cg", "newton"):       # [REF Rodent_Env_Brax.py:42-45]
            raise ValueError(f"solver must be 'cg' or 'newton', got {solver!r}")
        if vision:
            raise NotImplementedError("vision observations are not part of the reference obs either")
        if iterations < 2:
            # measured on the float64 oracle as on the GPU: with ONE solver iteration per substep the rollout under
            # random actions reaches |qvel| > 1e4 and non-finite states within two env steps (Newton 1/4), within a few (CG 1/4)
            warnings.warn(f"Rodent(solver={solver!r}, iterations={iterations}): a single solver iteration per substep diverges "
                          "under random actions (non-finite states within a few env steps, on the CPU oracle too); use iterations >= 2",
                          RuntimeWarning, stacklevel=2)
        sys = System(assets.resolve_model(xml_path), iterations, ls_iterations, solver)
        physics_steps_per_control_step = 10   # [REF Rodent_Env_Brax.py:53-57]
        kwargs["n_frames"] = kwargs.get("n_frames", physics_steps_per_control_step)
        kwargs["backend"] = "hip"
        super().__init__(sys, num_envs=num_envs, device=device, **kwargs)
        self._track_pos = torch.as_tensor(np.asarray(track_pos), dtype=torch.float32).to(self.device).contiguous()
        self._forward_reward_weight = forward_reward_weight
        self._ctrl_cost_weight = ctrl_cost_weight
        self._healthy_reward = healthy_reward
        self._terminate_when_unhealthy = terminate_when_unhealthy
        self._healthy_z_range = healthy_z_range
        self._reset_noise_scale = reset_noise_scale
        self._vision = vision
        self._bad_state_max = None if bad_state_max is None else float(bad_state_max)
        self._ctor = dict(track_pos=track_pos, forward_reward_weight=forward_reward_weight, ctrl_cost_weight=ctrl_cost_weight,
                          healthy_reward=healthy_reward, terminate_when_unhealthy=terminate_when_unhealthy,
                          healthy_z_range=healthy_z_range, reset_noise_scale=reset_noise_scale, solver=solver,
                          iterations=iterations, ls_iterations=ls_iterations, vision=vision, xml_path=xml_path,
                          n_frames=kwargs["n_frames"], pipeline_outputs=kwargs.get("pipeline_outputs", False),
                          contact_outputs=kwargs.get("contact_outputs", False), balance=kwargs.get("balance"),
                          rebalance_every=kwargs.get("rebalance_every", 4), bad_state_max=bad_state_max)

    def with_num_envs(self, num_envs: int, device=None):
        """A sibling env with another batch size (ppo.train builds its per-rank and eval envs this way)."""
        return Rodent(num_envs=num_envs, device=device or self.device, **self._ctor)

    def contact_overflow(self) -> int:
        """(env, env step) events so far in which more sphere / capsule pairs were in penetration than the kernel's 64 contact slots;
        the surplus pairs were DROPPED for that substep (models with candidate-pair contacts, e.g. rodent_cpu.xml; always 0 for the
        floor-contact models).  Reads a device counter: synchronises the env's stream."""
        return self._batch.contact_overflow()

    @property
    def bad_state_max(self) -> Optional[float]:
        """The threshold of the bad-state check, None when it is off."""
        return self._bad_state_max

    def bad_states(self) -> int:
        """(env, env step) events so far in which the bad-state check ended an episode (`bad_state_max`; always 0 while it is off).  A
        multi-step launch counts each of its steps.  Reads a device counter: synchronises the env's stream."""
        return self._batch.bad_states()

    def _env_io(self, cur_frame, obs, reward=None, done=None, metrics=None):
        return dict(track_pos=self._track_pos, cur_frame=cur_frame, obs=obs, reward=reward, done=done, metrics=metrics,
                    healthy_reward=self._healthy_reward, ctrl_cost_weight=self._ctrl_cost_weight,
                    healthy_z_range=self._healthy_z_range, terminate_when_unhealthy=self._terminate_when_unhealthy,
                    bad_state_max=self._bad_state_max)

    def reset(self, rng) -> State:
        """Resets the environment to an initial state.  `rng`: uint32 keys [N, 2] (one jax-style
        PRNG key per env, as `jax.vmap(env.reset)(split(key, N))` passes) or an int seed."""
        N, dev, s = self.num_envs, self.device, self.sys
        if isinstance(rng, (int, np.integer)):
            rng = jax_random.split(jax_random.PRNGKey(int(rng)), N)
        keys = np.asarray(rng, dtype=np.uint32).reshape(N, 2)
        ks = jax_random.split(keys, 4)                       # rng, rng1, rng2, rng_pos
        start_frame = jax_random.randint(ks[:, 0], 0, 100)   # [N] int32
        low, hi = -self._reset_noise_scale, self._reset_noise_scale
        track = self._track_pos.cpu().numpy()
        qpos = np.tile(np.asarray(s.qpos0, dtype=np.float32), (N, 1))
        qpos[:, :3] = track[np.clip(start_frame, 0, len(track) - 1)]
        qpos = qpos + jax_random.uniform(ks[:, 1], s.nq, low, hi)
        qvel = jax_random.uniform(ks[:, 2], s.nv, low, hi)

        st = dict(qpos=torch.from_numpy(qpos).to(dev), qvel=torch.from_numpy(qvel).to(dev),
                  act=torch.zeros(N, s.na, device=dev), qacc_warmstart=torch.zeros(N, s.nv, device=dev))
        out = self._alloc_outputs(full=False)
        cur_frame = torch.from_numpy(start_frame.astype(np.int32)).to(dev)
        obs = torch.empty(N, s.obs_dim, device=dev)
        self._batch.env_reset(st, self._env_io(cur_frame, obs), out)
        zero = torch.zeros(N, device=dev)
        metrics = {"pos_reward": zero, "reward_quadctrl": zero.clone(), "reward_alive": zero.clone()}
        return State(PipelineState(**st, **out), obs, zero.clone(), zero.clone(), metrics, {"cur_frame": cur_frame})

    def _launch_buffers(self, state: State, episode_length: Optional[float] = None):
        """What a step launch reads and writes: (st_in, st_out, env-io outputs dict(cur_frame, reward, done, metrics), wrap) -- `wrap` the
        Episode + AutoReset wrappers' state of a multi-step launch (`hip.Batch._unroll_io`), None without `episode_length`.  The previous
        state is left untouched (no copies)."""
        N, dev = self.num_envs, self.device
        ps, info = state.pipeline_state, state.info
        fields = lambda p: dict(qpos=p.qpos, qvel=p.qvel, act=p.act, qacc_warmstart=p.qacc_warmstart)
        st_in = fields(ps)
        st = {k: torch.empty_like(v) for k, v in st_in.items()}
        io = dict(cur_frame=torch.empty_like(info["cur_frame"]), reward=torch.empty(N, device=dev), done=torch.empty(N, device=dev),
                  metrics=torch.empty(N, 3, device=dev))
        wrap = None
        if episode_length is not None:
            wrap = dict(first=fields(info["first_pipeline_state"]), first_obs=info["first_obs"], prev_done=state.done, steps_in=info["steps"],
                        steps_out=torch.empty(N, device=dev), truncation_out=torch.empty(N, device=dev), episode_length=episode_length)
        return st_in, st, io, wrap

    def _next_state(self, state: State, st, io, obs, wrap=None, out=None) -> State:
        """The State a launch on `_launch_buffers` left."""
        info = dict(state.info)
        info["cur_frame"] = io["cur_frame"]
        if wrap is not None:
            info.update(steps=wrap["steps_out"], truncation=wrap["truncation_out"])
        m = dict(state.metrics)
        m.update(pos_reward=io["metrics"][:, 0], reward_quadctrl=io["metrics"][:, 1], reward_alive=io["metrics"][:, 2])
        return state.replace(pipeline_state=PipelineState(**st, **(out or {})), obs=obs, reward=io["reward"], done=io["done"], metrics=m, info=info)

    def unroll_wrapped(self, state: State, actions: torch.Tensor, episode_length: float) -> State:
        """`actions.shape[0]` steps with `EpisodeWrapper(episode_length)` + `AutoResetWrapper` (action_repeat 1) in ONE launch
        (`rr_env_unroll`): what `lax.scan` over the wrapped `step` is to the reference.  `state` is a state of the wrapped env
        (info carries steps, truncation, first_pipeline_state, first_obs); returns the state after the last step, bit for bit what
        the per-step calls give.  Intermediate observations / rewards are not returned (a random-action rollout needs none)."""
        if self._pipeline_outputs or self._contact_outputs:
            raise ValueError("a multi-step rollout returns no pipeline / contact outputs: build the env without them")
        st_in, st, io, wrap = self._launch_buffers(state, episode_length)
        obs = torch.empty(self.num_envs, self.sys.obs_dim, device=self.device)
        actions = actions.to(self.device, torch.float32).contiguous()
        self._rebalance()
        self._batch.env_unroll(st_in, st, actions, self._n_frames, self._env_io(obs=obs, **io), state.info["cur_frame"], wrap)
        return self._next_state(state, st, io, obs, wrap)

    def unroll_policy_wrapped(self, state: State, episode_length: float, actor: dict, noise: torch.Tensor, traj: dict, segment: int = 0) -> State:
        """`generate_unroll` in one launch (`rr_env_unroll_policy`): T = noise.shape[0] x [policy(obs) -> tanh-normal sample -> step ->
        EpisodeWrapper + AutoResetWrapper], the transitions written into `traj` (views of the learner's buffers, batch-major).
        `actor`: the policy's parameters as the kernel takes them (`acting.actor_params`).  `segment` = L: the T steps are recorded as
        T / L trajectories ([U, N, L(+1), ...] buffers) -- a whole rollout phase in one launch.  Returns the state after the last step."""
        if self._pipeline_outputs or self._contact_outputs:
            raise ValueError("a multi-step rollout returns no pipeline / contact outputs: build the env without them")
        N, T = self.num_envs, noise.shape[0]
        st_in, st, io, wrap = self._launch_buffers(state, episode_length)
        actions = torch.empty(T, N, self.action_size, device=self.device)
        obs_in = state.obs.contiguous()            # (also fills the env io's obs slot, which this entry point does not write)
        self._batch.env_unroll_policy(st_in, st, T, self._n_frames, self._env_io(obs=obs_in, **io), state.info["cur_frame"], wrap, actor, noise,
                                      actions, traj, obs_in, segment)
        L_ = segment or T
        obs = traj["obs"].reshape(T // L_, N, L_ + 1, -1)[-1, :, L_].contiguous()
        return self._next_state(state, st, io, obs, wrap), actions

    def eval_supported(self) -> bool:
        """Whether `unroll_eval` serves this env: a batch with an evaluation instance (CG solver, a model with a multi-step instance, no
        per-env parameters) and no pipeline / contact outputs."""
        return (self.device.type == "cuda" and not self._pipeline_outputs and not self._contact_outputs and self._batch.eval_supported())

    def unroll_eval(self, state: State, T: int, actor: dict, noise: Optional[torch.Tensor] = None, episode_length: Optional[float] = None,
                    eval_metrics: Optional[torch.Tensor] = None, actions_out: Optional[torch.Tensor] = None, qpos_out: Optional[torch.Tensor] = None) -> State:
        """T x [policy(obs) -> action -> step] in ONE launch without a trajectory (`rr_env_unroll_eval`): what an evaluation needs.
        `episode_length` given: `state` is a state of the wrapped env and `EpisodeWrapper(episode_length)` + `AutoResetWrapper` act between
        the steps, with brax's EvalWrapper bookkeeping on `eval_metrics` [N, 6] = (episode_steps, active_episodes, sums of pos_reward,
        reward_quadctrl, reward_alive, reward), updated in place.  `episode_length` None: the unwrapped env, stepping on past `done`.
        `actor`: `acting.actor_params`; `noise` [T, N, A] standard normal draws, None = the deterministic policy.  Optional records:
        `actions_out` [T, N, A], `qpos_out` [T + 1, N, nq] (row 0 the incoming qpos; wrapped: taken before a restore).  Returns the state
        after the last step, as T calls of `step` on the same actions leave it.  A batch without an evaluation instance (`eval_supported`)
        refuses with the reason (RuntimeError)."""
        if self._pipeline_outputs or self._contact_outputs:
            raise ValueError("an evaluation launch returns no pipeline / contact outputs: build the env without them")
        st_in, st, io, wrap = self._launch_buffers(state, episode_length)
        ring = torch.empty(self.num_envs, 2, self.sys.obs_dim, device=self.device)
        obs_in = state.obs.contiguous()
        self._batch.env_unroll_eval(st_in, st, int(T), self._n_frames, self._env_io(obs=obs_in, **io), state.info["cur_frame"], actor,
                                    obs_in, ring, noise, actions_out, eval_metrics, qpos_out, wrap)
        return self._next_state(state, st, io, ring[:, int(T) & 1].contiguous(), wrap)

    def step(self, state: State, action: torch.Tensor) -> State:
        """Runs one timestep of the environment's dynamics.  With `bad_state_max` set, a bad env comes back with done = 1, reward 0 and
        metrics 0, but its state and observation are returned as they are (possibly non-finite): restoring is AutoReset's part."""
        st_in, st, io, _ = self._launch_buffers(state)
        out = self._alloc_outputs(full=False)
        obs = torch.empty(self.num_envs, self.sys.obs_dim, device=self.device)
        action = action.to(self.device, torch.float32).contiguous()
        self._rebalance()
        self._batch.env_step_to(st_in, st, action, self._n_frames, self._env_io(obs=obs, **io), state.info["cur_frame"], out)
        return self._next_state(state, st, io, obs, out=out)
