"""Reference restarts on the GPU (`Rodent(restart_from_reference=True)`; rr_batch_set_reference_restart, the RESTART instances of the
step kernel): a restore draws a clip and a start frame, builds its start state from the clip's rows and runs the
reset's forward pass inside the rollout.

Fixture: N = 8 envs, 24 steps, episodes of 5 (every env restores four or more times), three clips of 104 rows with the lengths
(104, 14, 9) of tests/clip_library_fixture.py, K = 1, n_frames 2, CG 4/4, reset clips arange(N) % 3.  The rule is integer hashing and
single float32 roundings, so every comparison is exact."""
import functools
import math

import numpy as np
import pytest
import torch

from rodent_amd import jax_random
from rodent_amd.envs import graphed, rodent, wrappers
from tests import clip_library_fixture as X
from tests import pose_fixture as F
from tests.pose_fixture import DEV
from tests.test_gpu_clip_library import _velocities
from tests.test_gpu_clip_restart import _assert_same

pytestmark = pytest.mark.gpu
N, C, T, L, STEPS, K = 8, 3, 104, 5, 24, 1
LENGTHS, IDS, SEED, RANGE = X.LENGTHS, (np.arange(N) % C).astype(np.int32), 11, (0, 100)
MODELS = ["rodent_optimized", "rodent_0"]          # a fixed-dimension instance and the generic one


def _keys():
    return jax_random.split(jax_random.PRNGKey(94), N)


def _make(model, H=0, vel=False, ref=True, lengths=True, across=True, **kw):
    kw.update(clip_restarts=K, end_at_clip_end=True, reset_to_reference=True)
    if ref:
        kw.update(restart_from_reference=True, restart_noise_seed=SEED)
    if H:
        kw.update(reference_obs_frames=H)
    if vel:
        kw.update(_velocities(model))
    if lengths:
        kw.update(clip_lengths=LENGTHS)
    if across:
        kw.update(restart_across_clips=True)
    return F.make(model, T, n=N, **kw)


def _draws(env, steps, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    A = env.action_size
    return torch.rand(steps, N, A, device=DEV, generator=gen) * 2 - 1, torch.randn(steps, N, A, device=DEV, generator=gen)


def _composed(env):
    return wrappers.ClipAutoResetWrapper(wrappers.ClipEpisodeWrapper(wrappers.VmapWrapper(env), L, 1))


def _fused(env):
    return wrappers.FusedEpisodeAutoResetWrapper(wrappers.VmapWrapper(env), L)


def _run(wenv, acts, s=None):
    snap = lambda s: s.replace(info=dict(s.info), metrics=dict(s.metrics))
    s = wenv.reset(_keys(), clip=IDS) if s is None else s
    out = [snap(s)]
    for t in range(acts.shape[0]):
        s = wenv.step(s, acts[t])
        out.append(snap(s))
    torch.cuda.synchronize()
    return out


def _same(got, want, what, **kw):
    """Every state leaf and info entry a wrapped step produces, the restore count included, bit for bit."""
    _assert_same(got, want, what, **kw)
    assert torch.equal(got.info["restart_draws"], want.info["restart_draws"]) and got.info["restart_draws"].dtype == torch.int32, (what, "restart_draws")


def _ints(s):
    return torch.stack([s.info[k] for k in ("cur_frame", "clip", "restart_draws")], dim=-1).cpu().numpy().astype(np.int64)


# ---------------------------------------------------------------------------------------------- 1 + 2. the restored state and its observation
CASES = [(m, H, vel) for m in MODELS for H, vel in ((0, False), (2, True), (0, True), (2, False))]


@functools.lru_cache(maxsize=None)
def _single_launches(model, H, vel):
    """Computed once per case and shared: the run as 24 one-step launches of `unroll` (the kernel's restore), a state per step."""
    env = _make(model, H, vel)
    acts, _ = _draws(env, STEPS, 1)
    wenv = _fused(env)
    s = wenv.reset(_keys(), clip=IDS)
    out = [s]
    for t in range(STEPS):
        out.append(wenv.unroll(out[-1], acts[t:t + 1]))
    torch.cuda.synchronize()
    return env, out


@pytest.mark.parametrize("model,H,vel", CASES)
def test_the_restored_state_is_the_host_restatement_bit_for_bit(model, H, vel):
    env, states = _single_launches(model, H, vel)
    restores = 0
    for t in range(1, STEPS + 1):
        before, s = states[t - 1], states[t]
        done = s.done.cpu().numpy() != 0
        if not done.any():
            continue
        e = np.nonzero(done)[0]
        n = before.info["restart_draws"].cpu().numpy()[e]
        clip, draw, frame = rodent.reference_restart_draws(SEED, e, n, RANGE, clip=before.info["clip"].cpu().numpy()[e], num_clips=C, across_clips=True,
                                                           lengths=LENGTHS)
        assert ((draw >= RANGE[0]) & (draw < RANGE[1])).all() and (frame <= LENGTHS[clip] - 2).all()
        qpos, qvel = rodent.reference_restart_state(SEED, e, n, clip, frame, env._track_host, env._pose_host, env._vel_host if vel else env.sys.nv,
                                                    env._reset_noise_scale, LENGTHS)
        assert np.array_equal(s.info["cur_frame"].cpu().numpy()[e], frame) and np.array_equal(s.info["clip"].cpu().numpy()[e], clip), t
        assert np.array_equal(s.info["restart_draws"].cpu().numpy()[e], n + 1), t
        assert np.array_equal(s.pipeline_state.qpos.cpu().numpy()[e], qpos), t
        assert np.array_equal(s.pipeline_state.qvel.cpu().numpy()[e], qvel), t
        assert not s.pipeline_state.act[torch.from_numpy(e).to(DEV)].any(), t
        restores += len(e)
    print(f"{model} H={H} vel={vel}: {restores} restores checked")
    assert restores >= 4 * N          # episodes of 5 in 24 steps


@pytest.mark.parametrize("model,H,vel", CASES)
def test_the_restored_observation_is_the_reset_launchs_bit_for_bit(model, H, vel):
    """The in-loop forward pass is the reset's: the existing reset launch on the restored qpos / qvel / frame / clip writes the same
    observation row and leaves the same warm start."""
    env, states = _single_launches(model, H, vel)
    checked = 0
    for t in range(1, STEPS + 1):
        s = states[t]
        done = s.done != 0
        if not bool(done.any()):
            continue
        ps = s.pipeline_state
        st = dict(qpos=ps.qpos.clone(), qvel=ps.qvel.clone(), act=torch.zeros_like(ps.act), qacc_warmstart=torch.zeros_like(ps.qacc_warmstart))
        obs = torch.empty(N, env.observation_size, device=DEV)
        env._batch.env_reset(st, env._env_io(s.info["cur_frame"], obs, clip=s.info["clip"], clip_library=dict(lengths=env.clip_lengths)), env._alloc_outputs(full=False))
        torch.cuda.synchronize()
        assert obs.shape[1] == env.sys.obs_dim + H * env.sys.nq
        assert torch.equal(obs[done], s.obs[done]), (t, int((obs[done] != s.obs[done]).sum()))
        assert torch.equal(st["qacc_warmstart"][done], ps.qacc_warmstart[done]), t
        assert bool(torch.isfinite(s.obs).all())
        checked += int(done.sum())
    assert checked >= 4 * N


# ---------------------------------------------------------------------------------------------- 3 + 4. the forms agree
@functools.lru_cache(maxsize=None)
def _forms(model):
    env = _make(model, 2, True, clip_outcomes=True)
    acts, noise = _draws(env, STEPS, 1)
    out, tables = dict(env=env, acts=acts), {}

    def table(name):
        torch.cuda.synchronize()
        tables[name] = env.clip_outcomes(clear=True)
    out["composed"] = _run(_composed(env), acts); table("composed")
    out["fused"] = _run(_fused(env), acts); table("fused")
    wenv = _fused(env)
    s0 = wenv.reset(_keys(), clip=IDS)
    out["s0"] = s0
    out["unroll"] = wenv.unroll(s0, acts); table("unroll")
    out["programmed"] = env._batch._refrestart is not None
    out["unroll10"] = wenv.unroll(s0, acts[:10])
    out["unroll10+14"] = wenv.unroll(out["unroll10"], acts[10:]); table("unroll10+14")
    from rodent_amd.training import acting
    buf = acting.UnrollBuffer(2, N, 12, env.observation_size, env.action_size, torch.device(DEV))
    traj = dict(obs=buf.obs, raw_action=buf.raw_action, log_prob=buf.log_prob, reward=buf.reward, discount=buf.discount, truncation=buf.truncation)
    out["policy"], out["policy_actions"] = wenv.unroll_policy(s0, F.actor(env, 7), noise, traj, segment=12)
    out["buf"] = buf; table("policy")
    out["replay"] = _run(wenv, out["policy_actions"], s0); table("replay")
    out["tables"] = tables
    return out


@pytest.mark.parametrize("model", MODELS)
def test_unroll_equals_the_composed_wrappers_step_by_step_and_across_two_launches(model):
    f = _forms(model)
    s0 = f["s0"]
    assert s0.info["restart_draws"].dtype == torch.int32 and not s0.info["restart_draws"].any() and f["programmed"]
    for t, (g, w) in enumerate(zip(f["fused"], f["composed"])):
        _same(g, w, ("fused / composed", t))
    env, acts, wenv = f["env"], f["acts"], _fused(f["env"])
    s = s0
    for t in range(STEPS):          # step by step: one launch per step against the composed wrappers
        s = wenv.unroll(s, acts[t:t + 1])
        _same(s, f["composed"][t + 1], ("unroll(1) / composed", t + 1))
    torch.cuda.synchronize()
    env.clip_outcomes(clear=True)
    for name, at in (("unroll", STEPS), ("unroll10", 10), ("unroll10+14", STEPS)):
        _same(f[name], f["composed"][at], name)
    final = _ints(f["unroll"])
    print(f"{model}: restores per env {final[:, 2].tolist()}, clips {final[:, 1].tolist()}")
    assert (final[:, 2] >= 4).all()
    assert not s0.info["restart_draws"].any() and f["unroll"].info["restart_draws"].data_ptr() != s0.info["restart_draws"].data_ptr()


@pytest.mark.parametrize("model", MODELS)
def test_unroll_policy_replays_per_step(model):
    """The criterion of tests/test_gpu_clip_sampling.py for the bank restore: observations, discounts and truncations of the trajectory
    equal the per-step replay of the recorded actions bit for bit, the reward within the actor instance's one ulp."""
    f = _forms(model)
    why = f["env"]._batch.reference_restart_supported(with_actor=True)
    assert why is None, why
    buf, replay, worst = f["buf"], f["replay"], 0.0
    for t in range(STEPS):
        u, i = divmod(t, 12)
        assert torch.equal(buf.obs[u, :, i], replay[t].obs), t
        assert torch.equal(buf.discount[u, :, i], 1 - replay[t + 1].done) and torch.equal(buf.truncation[u, :, i], replay[t + 1].info["truncation"]), t
        worst = max(worst, float((buf.reward[u, :, i] - replay[t + 1].reward).abs().max()))
    assert torch.equal(buf.obs[0, :, 12], replay[12].obs) and torch.equal(buf.obs[1, :, 12], replay[STEPS].obs)
    print(f"{model}: max |traj.reward - per-step reward| = {worst:.3g} (allowed {F.ACTOR_REWARD_TOL})")
    assert worst <= F.ACTOR_REWARD_TOL
    _same(f["policy"], replay[STEPS], "policy final", reward_tol=F.ACTOR_REWARD_TOL)
    assert np.array_equal(f["tables"]["policy"], f["tables"]["replay"])


# ---------------------------------------------------------------------------------------------- 6. the outcome counters
@pytest.mark.parametrize("model", MODELS)
def test_the_outcome_counters_equal_the_host_update_over_the_composed_trajectory(model):
    f = _forms(model)
    want = np.zeros((C, 5), dtype=np.int64)
    states = f["composed"]
    for t in range(1, STEPS + 1):
        s, before = states[t], states[t - 1].info["clip"].cpu().numpy()
        done, trunc = s.done.cpu().numpy(), s.info["truncation"].cpu().numpy()
        rodent.clip_outcome_update(want, before, np.zeros(N), (done != 0) & (trunc == 0), done)
    print(f"{model}: outcome table {want.tolist()}")
    assert want[:, 4].sum() == N * STEPS and want[:, 0].sum() >= 4 * N
    for name in ("composed", "fused", "unroll", "unroll10+14"):
        assert np.array_equal(f["tables"][name], want), name


# ---------------------------------------------------------------------------------------------- 5. the weighted draw
def test_a_clip_of_weight_zero_is_never_drawn():
    env = _make(MODELS[0], restart_sampling="weighted")
    env.set_clip_weights([1, 0, 1])
    acts, _ = _draws(env, STEPS, 1)
    wenv = _fused(env)
    s = wenv.reset(_keys(), clip=IDS)
    landed = 0
    for t in range(STEPS):
        s = wenv.unroll(s, acts[t:t + 1])
        ints = _ints(s)
        restored = ints[:, 2] >= 1
        assert (ints[restored, 1] != 1).all(), t
        landed += int(restored.sum())
    assert landed >= N * (STEPS - L) and (ints[:, 2] >= 4).all()
    # in one launch, and against the host restatement with the table
    u = wenv.unroll(wenv.reset(_keys(), clip=IDS), acts)
    assert np.array_equal(_ints(u), ints)
    full = _run(_composed(env), acts)[-1]
    assert np.array_equal(_ints(full), ints)


def test_a_replayed_graph_reads_the_weights_written_after_its_capture():
    """One wrapped step as a one-step launch of `unroll`, captured with weights (1, 1, 1) and replayed after the table was rewritten in
    place to (0, 0, 1): the states are those of host-issued launches with the same rewrite, and not those without it."""
    dev = torch.device(DEV)
    stream = torch.cuda.Stream(dev)

    def make():
        with torch.cuda.stream(stream):
            env = _make(MODELS[0], restart_sampling="weighted")
            wenv = _fused(env)
            return env, wenv, wenv.reset(_keys(), clip=IDS)
    env_h, wenv_h, s = make()
    acts = _draws(env_h, STEPS, 1)[0]
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for t in range(STEPS):
            if t == 6:
                env_h.set_clip_weights([0, 0, 1])
            s = wenv_h.unroll(s, acts[t:t + 1])
    torch.cuda.synchronize()
    want = s
    env_g, wenv_g, sg = make()
    cursor = torch.zeros((), dtype=torch.long, device=dev)

    def step_fn(state):
        a = acts.index_select(0, cursor.reshape(1))
        cursor.add_(1)
        return wenv_g.unroll(state, a)
    with torch.cuda.stream(stream):
        st1 = step_fn(sg)
    torch.cuda.synchronize()
    g = graphed.GraphedSteps(step_fn, st1, 1, stream)
    for t in range(1, STEPS):
        if t == 6:
            with torch.cuda.stream(stream):
                env_g.set_clip_weights([0, 0, 1])
        got = g.replay()
    torch.cuda.synchronize()
    assert int(cursor) == STEPS
    _same(got, want, "graph")
    assert (_ints(got)[:, 1] == 2).all()          # every env restored after the rewrite, and only clip 2 was left to draw
    env_n, wenv_n, sn = make()
    with torch.cuda.stream(stream):
        sn = wenv_n.unroll(sn, acts)
    torch.cuda.synchronize()
    assert not np.array_equal(_ints(sn), _ints(want))


# ---------------------------------------------------------------------------------------------- 7. off is off
def test_with_the_option_off_the_run_is_the_env_without_the_argument():
    every = dict(H=2, vel=True, restart_sampling="weighted", clip_outcomes=True, bad_state_max=1e10)
    plain = _make(MODELS[0], ref=False, **every)
    off = _make(MODELS[0], ref=False, restart_from_reference=False, restart_noise_seed=0, **every)
    acts, _ = _draws(plain, STEPS, 1)
    runs = {}
    for name, env in (("plain", plain), ("off", off)):
        w = _fused(env)
        s0 = w.reset(_keys(), clip=IDS)
        runs[name] = (_run(w, acts), _run(_composed(env), acts), w.unroll(s0, acts))
        torch.cuda.synchronize()
        assert env._batch._refrestart is None and not env.restart_from_reference
    for t in range(STEPS + 1):
        _same(runs["off"][0][t], runs["plain"][0][t], ("fused", t))
        _same(runs["off"][1][t], runs["plain"][1][t], ("composed", t))
    _same(runs["off"][2], runs["plain"][2], "unroll")
    assert set(runs["off"][2].info) == set(runs["plain"][2].info)
    assert np.array_equal(off.clip_outcomes(), plain.clip_outcomes())


# ---------------------------------------------------------------------------------------------- 8. refusals
def test_refusals():
    with pytest.raises(RuntimeError, match="Newton"):
        _make(MODELS[0], solver="newton")
    from rodent_amd import envs
    cpu = envs.get_environment("rodent", track_pos=F.tracks(T)[0], num_envs=N, xml_path="rodent_cpu.xml", iterations=4, ls_iterations=4, n_frames=2, device=DEV)
    assert "candidate-pair" in cpu._batch.reference_restart_supported() and "candidate-pair" in cpu._batch.reference_restart_supported(with_actor=True)
    din, dout = torch.zeros(N, dtype=torch.int32, device=DEV), torch.zeros(N, dtype=torch.int32, device=DEV)
    plain = F.make(MODELS[0], T, n=N, pose=False)
    with pytest.raises(RuntimeError, match="needs a pose block"):
        plain._batch.set_reference_restart(din, dout)
    pose = F.make(MODELS[0], T, n=N)                  # a batch with the pose block and no restart block
    pose.step(pose.reset(_keys(), clip=IDS), _draws(pose, 1, 1)[0][0])
    with pytest.raises(RuntimeError, match="needs a clip-restart block"):
        pose._batch.set_reference_restart(din, dout)
    env = _make(MODELS[0])
    wenv = _fused(env)
    acts = _draws(env, 2, 1)[0]
    s = wenv.unroll(wenv.reset(_keys(), clip=IDS), acts)
    assert env._batch._refrestart is not None
    with pytest.raises(RuntimeError, match="may not alias"):
        env._batch.set_reference_restart(din, din)
    with pytest.raises(RuntimeError, match="frame_lo < frame_hi"):
        env._batch.set_reference_restart(din, dout, frame_range=(5, 5))
    with pytest.raises(RuntimeError, match="reference-restart block"):
        env._batch.set_clip_restarts(None)
    env.step(s, acts[0])                               # a bare step clears the blocks in order, and a launch sets them again
    assert env._batch._refrestart is None
    wenv.unroll(s, acts)
    assert env._batch._refrestart is not None


# ---------------------------------------------------------------------------------------------- 9. training
def test_one_ppo_train_step_with_reference_restarts(monkeypatch):
    from rodent_amd.training import acting
    from rodent_amd.training.agents.ppo import train as ppo
    env = F.make(MODELS[0], T, n=64, clip_restarts=1, end_at_clip_end=True, reset_to_reference=True, reference_obs_frames=2, clip_lengths=LENGTHS,
                 restart_across_clips=True, restart_sampling="weighted", clip_outcomes=True, restart_from_reference=True, restart_noise_seed=SEED)
    calls, log, tables = {"fused": 0}, [], []
    real_fused = acting.generate_unrolls_fused
    fw = rodent.FailureWeights()

    def spy(*a, **k):
        calls["fused"] += 1
        return real_fused(*a, **k)

    def weight_fn(table):
        tables.append(table.copy())
        return fw(table)
    monkeypatch.setattr(acting, "generate_unrolls_fused", spy)
    ppo.train(environment=env, num_timesteps=10 ** 9, episode_length=10, num_envs=64, batch_size=64, num_minibatches=2, unroll_length=5,
              num_updates_per_batch=2, num_evals=1, num_eval_envs=6, learning_rate=5e-5, entropy_cost=1e-3, discounting=0.97,
              normalize_observations=True, seed=3, max_training_steps=1, progress_fn=lambda n, m: log.append(m), clip_weight_fn=weight_fn)
    assert calls["fused"] == 1 and len(tables) == 1
    t = tables[0]
    assert t[:, 4].sum() == 64 * 10 and (t[:, 1:4].sum(1) == t[:, 0]).all() and t[:, 0].sum() > 0
    m = [x for x in log if "training/clip_fail_rate" in x][-1]
    assert math.isfinite(float(m["training/clip_fail_rate"])) and 0.0 <= float(m["training/clip_fail_rate"]) <= 1.0
