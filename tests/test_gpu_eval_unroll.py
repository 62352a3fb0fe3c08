"""One-launch evaluation (rr_env_unroll_eval, the rr_eval_kernel instances): `EvalWrapper.unroll_policy`, `Rodent.unroll_eval`,
`acting.Evaluator(actor_fn=...)` and `rollout.eval_rollout(actor=...)` against the per-step path of the same build.

The yardstick throughout is REPLAY: the launch records the actions it took, and the per-step path (`EvalWrapper.step` over the fused
Episode + AutoReset wrapper, or the unwrapped `env.step`) is driven by exactly those actions from the same start.  Physics, wrappers and
bookkeeping must then agree bit for bit; the two sums that contain `pos_reward = exp(..)` get the bound derived at `_tol`."""
import math

import pytest
import torch

from tests import randomisation_sets as rs, util

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, EP, T = 16, 7, 12
LAUNCHED = 6                  # envs started just below healthy_z_range's upper edge, moving up: they leave the range in flight
STATE = ("qpos", "qvel", "act", "qacc_warmstart")
EXACT_SUMS, ULP_SUMS = ("reward_quadctrl", "reward_alive"), ("pos_reward", "reward")


def _tol(steps, largest_partial_sum):
    """The actor instances expand `expf` of the reward inline and may round its last bit differently from the per-step instance (the
    existing one-launch tests allow exactly that: one ulp of a value <= 1).  A sum over `steps` steps then differs by at most `steps`
    one-ulp terms plus `steps` differently rounded additions: 2 * steps * 2^-24 * max(1, largest partial sum)."""
    return 2 * steps * 2.0 ** -24 * max(1.0, largest_partial_sum)


def _policy(env, seed):
    from rodent_amd.training import acting, networks, running_statistics
    torch.manual_seed(seed)
    nets = networks.make_ppo_networks(env.observation_size, env.action_size, device=DEV)
    net, dist = nets.policy_network, nets.parametric_action_distribution
    for l in net.layers:
        l.bias.data.uniform_(-0.3, 0.3)
    norm = running_statistics.init_state(env.observation_size, torch.device(DEV))
    norm.mean.copy_(torch.randn(env.observation_size, device=DEV) * 0.05)
    norm.std.copy_(torch.rand(env.observation_size, device=DEV) + 0.7)
    return nets, norm, acting.actor_params(net, norm, dist.min_std)


def _start(model, n, episode_length, z_range, iters, key, launched=0):
    """(env, EvalWrapper over the fused training wrappers, freshly reset state).  `launched` > 0 (models with a free joint): that many
    envs start 25 mm below the upper edge of healthy_z_range with 1 .. 1.5 m/s upwards -- in free flight z gains t - 4.9 t^2 (32 mm
    after two 20 ms env steps at 1 m/s), so they turn unhealthy within a few steps whatever the policy does.  The reset state is also
    the stored first state of the AutoReset wrapper (the same tensors), so a restored env is launched again."""
    from rodent_amd import envs, jax_random
    from rodent_amd.envs import wrappers
    env = envs.get_environment("rodent", track_pos=util.synthetic_track(), num_envs=n, xml_path=model, iterations=iters, ls_iterations=iters,
                               device=DEV, healthy_z_range=z_range)
    ew = wrappers.EvalWrapper(wrappers.wrap(env, episode_length=episode_length, action_repeat=1))
    st = ew.reset(jax_random.split(jax_random.PRNGKey(key), n))
    if launched:
        st.pipeline_state.qpos[:launched, 2] = z_range[1] - 0.025
        st.pipeline_state.qvel[:launched, 2] = torch.linspace(1.0, 1.5, launched, device=DEV)
    return env, ew, st


def _replay(ew, st, actions, policy=None):
    """The per-step path on the recorded actions.  Returns (final state, largest partial sum of the two inexact sums, per-step done /
    truncation, largest |policy(obs) - action| when a policy is given)."""
    partial, dones, truncs, act_err = 0.0, [], [], 0.0
    for t in range(actions.shape[0]):
        if policy is not None:
            a, _ = policy(st.obs, None)
            act_err = max(act_err, float((a - actions[t]).abs().max()))
        st = ew.step(st, actions[t])
        em = st.info["eval_metrics"]["episode_metrics"]
        partial = max(partial, *(float(em[k].abs().max()) for k in ULP_SUMS))
        dones.append(st.done.clone()); truncs.append(st.info["truncation"].clone())
    return st, partial, torch.stack(dones), torch.stack(truncs), act_err


def _assert_matches_replay(got, want, steps, partial):
    ga, wa = got.info["eval_metrics"], want.info["eval_metrics"]
    assert torch.equal(ga["episode_steps"], wa["episode_steps"]) and torch.equal(ga["active_episodes"], wa["active_episodes"])
    assert list(ga["episode_metrics"]) == list(wa["episode_metrics"])
    for k in EXACT_SUMS:
        assert torch.equal(ga["episode_metrics"][k], wa["episode_metrics"][k]), k
    bound = _tol(steps, partial)
    for k in ULP_SUMS:
        err = float((ga["episode_metrics"][k] - wa["episode_metrics"][k]).abs().max())
        print(f"{k}: |one launch - replay| = {err:.3e}, bound {bound:.3e} (largest partial sum {partial:.3f})")
        assert err <= bound, (k, err, bound)
    for k in STATE:
        assert torch.equal(getattr(got.pipeline_state, k), getattr(want.pipeline_state, k)), k
    assert torch.equal(got.obs, want.obs) and torch.equal(got.done, want.done)
    for k in ("cur_frame", "steps", "truncation"):
        assert torch.equal(got.info[k], want.info[k]), k
    for k in EXACT_SUMS:
        assert torch.equal(got.metrics[k], want.metrics[k]), k
    assert float((got.reward - want.reward).abs().max()) <= 2.5e-7 and float((got.metrics["pos_reward"] - want.metrics["pos_reward"]).abs().max()) <= 2.5e-7


def _assert_identical(a, b):
    """Two states of the one-launch path, every field bit for bit."""
    for k in STATE:
        assert torch.equal(getattr(a.pipeline_state, k), getattr(b.pipeline_state, k)), k
    assert torch.equal(a.obs, b.obs) and torch.equal(a.done, b.done) and torch.equal(a.reward, b.reward)
    for k in ("cur_frame", "steps", "truncation"):
        assert torch.equal(a.info[k], b.info[k]), k
    ea, eb = a.info["eval_metrics"], b.info["eval_metrics"]
    assert torch.equal(ea["episode_steps"], eb["episode_steps"]) and torch.equal(ea["active_episodes"], eb["active_episodes"])
    for k in ea["episode_metrics"]:
        assert torch.equal(ea["episode_metrics"][k], eb["episode_metrics"][k]), k
    for k in a.metrics:
        assert torch.equal(a.metrics[k], b.metrics[k]), k


@pytest.fixture(scope="module")
def sampled():
    """The 12-step sampling launch on rodent_optimized that the replay, chaining and determinism tests share."""
    env, ew, st0 = _start("rodent_optimized.xml", N, EP, (0.03, 0.5), 8, 2, LAUNCHED)
    nets, norm, actor = _policy(env, 3)
    noise = torch.randn(T, N, env.action_size, device=DEV)
    actions = torch.empty(T, N, env.action_size, device=DEV)
    assert ew.unroll_supported() and env.eval_supported()
    got = ew.unroll_policy(st0, actor, noise, T, actions_out=actions)
    torch.cuda.synchronize()
    return dict(nets=nets, norm=norm, actor=actor, noise=noise, actions=actions, got=got)


def test_evaluator_unroll_by_replay(sampled):
    """16 envs, episodes of 7 steps, 12 steps in the launch (past the episode end: finished envs keep stepping, inactive), sampling noise.
    Both kinds of episode end are in the batch, and the launch leaves what EvalWrapper.step leaves on the same actions."""
    _, ew, st0 = _start("rodent_optimized.xml", N, EP, (0.03, 0.5), 8, 2, LAUNCHED)
    want, partial, dones, truncs, _ = _replay(ew, st0, sampled["actions"])
    first = dones[:EP].argmax(0)                                   # every env is done by step EP - 1 at the latest
    assert bool(dones[:EP].any(0).all())
    terminated_early = (first < EP - 1) & (truncs[first, torch.arange(N, device=DEV)] == 0)
    truncated = (first == EP - 1) & (truncs[EP - 1] == 1)
    assert int(terminated_early.sum()) >= 3 and int(truncated.sum()) >= 3, (first.tolist(), truncs[EP - 1].tolist())
    em = want.info["eval_metrics"]
    assert float(em["active_episodes"].sum()) == 0 and float(em["episode_steps"].max()) == EP and float(em["episode_steps"].min()) < EP
    assert torch.isfinite(sampled["actions"]).all() and float(sampled["actions"].abs().max()) <= 1
    _assert_matches_replay(sampled["got"], want, T, partial)


def test_chained_launches_equal_one(sampled):
    """5 + 7 steps, the second launch fed the first one's state and eval_metrics: the 12-step launch bit for bit."""
    env, ew, st = _start("rodent_optimized.xml", N, EP, (0.03, 0.5), 8, 2, LAUNCHED)
    acts = torch.empty(T, N, env.action_size, device=DEV)
    st = ew.unroll_policy(st, sampled["actor"], sampled["noise"][:5].contiguous(), 5, actions_out=acts[:5])
    st = ew.unroll_policy(st, sampled["actor"], sampled["noise"][5:].contiguous(), 7, actions_out=acts[5:])
    torch.cuda.synchronize()
    assert torch.equal(acts, sampled["actions"])
    _assert_identical(st, sampled["got"])


def test_deterministic_policy(sampled):
    """No noise pointer = an all-zero noise array, bit for bit; and the actions are those of make_policy(deterministic=True) on the
    observations of the replay, to the bound test_one_launch_unroll_with_the_actor_inside holds the in-kernel actor's actions to (2e-5)."""
    from rodent_amd.training import networks
    out = []
    for noise in (None, torch.zeros(T, N, 30, device=DEV)):
        env, ew, st0 = _start("rodent_optimized.xml", N, EP, (0.03, 0.5), 8, 2, LAUNCHED)
        acts = torch.empty(T, N, env.action_size, device=DEV)
        out.append((ew.unroll_policy(st0, sampled["actor"], noise, T, actions_out=acts), acts))
    torch.cuda.synchronize()
    assert torch.equal(out[0][1], out[1][1])
    _assert_identical(out[0][0], out[1][0])
    assert not torch.equal(out[0][1], sampled["actions"])
    # without actions_out the launch keeps the current action in the batch's own rows: same result
    _, ew, st0 = _start("rodent_optimized.xml", N, EP, (0.03, 0.5), 8, 2, LAUNCHED)
    _assert_identical(ew.unroll_policy(st0, sampled["actor"], None, T), out[0][0])
    policy = networks.make_inference_fn(sampled["nets"])((sampled["norm"], sampled["nets"].policy_network), deterministic=True)
    _, ew, st0 = _start("rodent_optimized.xml", N, EP, (0.03, 0.5), 8, 2, LAUNCHED)
    want, partial, _, _, act_err = _replay(ew, st0, out[0][1], policy)
    print("deterministic actions: largest |policy(obs) - action| =", act_err)
    assert act_err <= 2e-5
    _assert_matches_replay(out[0][0], want, T, partial)


def test_raw_mode_single_env_and_eval_rollout(monkeypatch):
    """The launcher's evaluation rollout: one unwrapped env, deterministic policy, 40 steps in one launch.  qpos_out equals the replay
    through the unwrapped env.step row for row, `done` fires mid-way and the env steps on from where it is (no restore), and
    eval_rollout(actor=...) returns those rows.  healthy_z_range does not enter the physics of an unwrapped env, so it is chosen from
    the per-step rollout of the same env under the default range: the edge goes half-way into the largest new extreme of z after step 5."""
    from rodent_amd import envs, jax_random, rollout
    from rodent_amd.training import networks
    S, SEED = 40, 5

    def make(z_range):
        return envs.get_environment("rodent", track_pos=util.synthetic_track(), num_envs=1, xml_path="rodent_optimized.xml", iterations=8,
                                    ls_iterations=8, device=DEV, healthy_z_range=z_range)
    env = make((0.03, 0.5))
    nets, norm, actor = _policy(env, 7)
    make_policy = networks.make_inference_fn(nets)
    params = (norm, nets.policy_network)
    monkeypatch.setenv("RR_FUSED_EVAL", "0")
    z = torch.from_numpy(rollout.eval_rollout(env, make_policy, params, steps=S, seed=SEED, actor=actor))[:, 2]          # per-step loop
    lows = [(float(z[:k].min() - z[k]), k) for k in range(6, S - 4)]
    highs = [(float(z[k] - z[:k].max()), k) for k in range(6, S - 4)]
    (gl, kl), (gh, kh) = max(lows), max(highs)
    assert max(gl, gh) > 1e-3, "z stays inside the envelope of its first steps: pick another seed"
    z_range = (float(z[:kl].min()) - gl / 2, 0.5) if gl >= gh else (0.0, float(z[:kh].max()) + gh / 2)
    env = make(z_range)
    # (1) one launch, actions and qpos recorded
    key = jax_random.split(jax_random.split(jax_random.PRNGKey(SEED))[1])[0]
    st0 = env.reset(key[None])
    acts, qpos = torch.empty(S, 1, env.action_size, device=DEV), torch.empty(S + 1, 1, 74, device=DEV)
    got = env.unroll_eval(st0, S, actor, None, actions_out=acts, qpos_out=qpos)
    torch.cuda.synchronize()
    # (2) replay through the unwrapped step
    st, dones = env.reset(key[None]), []
    assert torch.equal(qpos[0], st.pipeline_state.qpos)
    for t in range(S):
        st = env.step(st, acts[t])
        assert torch.equal(qpos[t + 1], st.pipeline_state.qpos), t
        dones.append(float(st.done[0]))
    fired = [t for t, d in enumerate(dones) if d]
    assert fired and 0 < fired[0] < S - 1, dones                     # mid-way; every later row still equals the plain step's: no restore
    for k in STATE:
        assert torch.equal(getattr(got.pipeline_state, k), getattr(st.pipeline_state, k)), k
    assert torch.equal(got.obs, st.obs) and torch.equal(got.done, st.done) and torch.equal(got.info["cur_frame"], st.info["cur_frame"])
    assert float((got.reward - st.reward).abs().max()) <= 2.5e-7
    # (3) eval_rollout with the actor takes the launch where RR_FUSED_EVAL=1 asks for it (the loop is the default) and returns its rows
    calls = []
    real = type(env).unroll_eval
    monkeypatch.setattr(type(env), "unroll_eval", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    monkeypatch.delenv("RR_FUSED_EVAL")
    loop_rows = rollout.eval_rollout(env, make_policy, params, steps=S, seed=SEED, actor=actor)
    assert calls == [] and loop_rows.shape == (S + 1, 74)
    monkeypatch.setenv("RR_FUSED_EVAL", "1")
    rows = rollout.eval_rollout(env, make_policy, params, steps=S, seed=SEED, actor=actor)
    assert calls == [1] and rows.shape == (S + 1, 74) and rows.dtype.name == "float32"
    assert (torch.from_numpy(rows) == qpos[:, 0].cpu()).all()


def test_evaluator_unroll_on_the_self_collision_model():
    """rodent_cpu.xml (the DYN instance; 38 actuators: the two-pass head), 8 envs, 10 steps, the replay check.  qpos[2] is a hinge angle
    there; the band is the one tests/test_gpu_unroll_self_collision.py ends episodes with."""
    n, steps = 8, 10
    env, ew, st0 = _start("rodent_cpu.xml", n, EP, (-0.3, 0.3), 6, 4)
    _, _, actor = _policy(env, 5)
    assert env.action_size == 38 and ew.unroll_supported()
    noise = torch.randn(steps, n, 38, device=DEV)
    acts = torch.empty(steps, n, 38, device=DEV)
    got = ew.unroll_policy(st0, actor, noise, steps, actions_out=acts)
    torch.cuda.synchronize()
    _, ew, st0 = _start("rodent_cpu.xml", n, EP, (-0.3, 0.3), 6, 4)
    want, partial, dones, _, _ = _replay(ew, st0, acts)
    assert bool(dones[:EP].any(0).all())
    _assert_matches_replay(got, want, steps, partial)


def _train(env, log):
    from rodent_amd.training.agents.ppo import train as ppo
    return ppo.train(environment=env, num_timesteps=10 ** 9, episode_length=10, num_envs=64, batch_size=64, num_minibatches=4, unroll_length=5,
                     num_updates_per_batch=2, num_evals=2, num_eval_envs=16, learning_rate=5e-5, entropy_cost=1e-3, discounting=0.97,
                     normalize_observations=True, seed=1, max_training_steps=2, progress_fn=lambda n, m: log.append(m))


def test_ppo_train_evaluates_in_one_launch(monkeypatch):
    """ppo.train hands the Evaluator the actor's layout: with RR_FUSED_EVAL=1 no per-step env.step runs inside run_evaluation (it raises
    here), the evaluations complete and report.  RR_FUSED_EVAL=0, and the default, keep the per-step loop."""
    from rodent_amd import envs
    from rodent_amd.training import acting
    flag = {"in_eval": False, "steps_in_eval": 0, "raise": True}
    real_step, real_eval = envs.Rodent.step, acting.Evaluator.run_evaluation

    def step(self, state, action):
        if flag["in_eval"]:
            flag["steps_in_eval"] += 1
            if flag["raise"]:
                raise AssertionError("per-step env.step inside run_evaluation")
        return real_step(self, state, action)

    def run_evaluation(self, *a, **k):
        flag["in_eval"] = True
        try:
            return real_eval(self, *a, **k)
        finally:
            flag["in_eval"] = False
    monkeypatch.setattr(envs.Rodent, "step", step)
    monkeypatch.setattr(acting.Evaluator, "run_evaluation", run_evaluation)
    make = lambda: envs.get_environment("rodent", track_pos=util.synthetic_track(), num_envs=64, xml_path="rodent_optimized.xml", iterations=8,
                                        ls_iterations=8, device=DEV)
    log = []
    monkeypatch.setenv("RR_FUSED_EVAL", "1")
    _train(make(), log)
    assert len(log) >= 2 and flag["steps_in_eval"] == 0
    for m in log:
        assert math.isfinite(float(m["eval/episode_reward"])) and 0 < float(m["eval/avg_episode_length"]) <= 10
    monkeypatch.setenv("RR_FUSED_EVAL", "0")
    flag["raise"] = False
    log2 = []
    _train(make(), log2)
    assert flag["steps_in_eval"] == len(log2) * 10 and math.isfinite(float(log2[-1]["eval/episode_reward"]))
    monkeypatch.delenv("RR_FUSED_EVAL")
    flag["steps_in_eval"] = 0
    log3 = []
    _train(make(), log3)
    assert flag["steps_in_eval"] == len(log3) * 10


def test_refusals(monkeypatch):
    """Newton, a batch with per-env parameters and the two-tree model have no evaluation instance: eval_supported() says so, the
    Evaluator evaluates them step by step without a word, and the ABI call names the reason."""
    from rodent_amd import envs, jax_random
    from rodent_amd.envs import wrappers
    from rodent_amd.training import acting, networks
    n = 8

    def make(model, **kw):
        return envs.get_environment("rodent", track_pos=util.synthetic_track(), num_envs=n, xml_path=model, iterations=4, ls_iterations=8, device=DEV, **kw)
    mixed = make("rodent_optimized.xml")
    assert mixed.eval_supported()
    fn = rs.system_fn(rs.mixed_fields)
    mixed.randomize(lambda sys: fn(sys, n))
    for env, why in ((make("rodent_optimized.xml", solver="newton"), "Newton"), (mixed, "per-env parameters"), (make("rodent_pair.xml"), "two-wave pair")):
        assert not env.eval_supported()
        nets, norm, actor = _policy(env, 1)
        ew = wrappers.EvalWrapper(wrappers.wrap(env, episode_length=2, action_repeat=1))
        assert not ew.unroll_supported()
        make_policy = networks.make_inference_fn(nets)
        ev = acting.Evaluator(ew.env, lambda p: make_policy(p, deterministic=False), n, 2, 1, jax_random.PRNGKey(0),
                              actor_fn=lambda p: acting.actor_params(p[1], p[0], 0.001))
        monkeypatch.setenv("RR_FUSED_EVAL", "1")
        assert not ev.one_launch()
        m = ev.run_evaluation((norm, nets.policy_network), {})
        assert math.isfinite(m["eval/episode_reward"]) and m["eval/avg_episode_length"] > 0
        with pytest.raises(RuntimeError, match="rr_env_unroll_eval.*" + why):
            env.unroll_eval(env.reset(jax_random.split(jax_random.PRNGKey(1), n)), 2, actor)
        with pytest.raises(ValueError, match="evaluation instance"):
            ew.unroll_policy(ew.reset(jax_random.split(jax_random.PRNGKey(1), n)), actor, None, 2)
    torch.cuda.synchronize()
