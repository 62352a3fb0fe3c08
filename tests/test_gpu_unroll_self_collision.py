"""One-launch rollouts on the self-collision model (rodent_cpu.xml [REF models/rodent_cpu.xml]: candidate-pair contacts, tendon
transmissions, 38 actuators): the `UNROLL x DYN` and `UNROLL x ACTOR x DYN` instances of the step kernel against the per-step path of
the same build, bit for bit; the in-kernel actor's two-pass head (76 logits) against the policy evaluated by torch in float64; and
`ppo.train` collecting its rollouts through them."""
import math
import warnings

import numpy as np
import pytest
import torch

from rodent_amd import assets, mjcf
from tests import parity, util

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODEL = "rodent_cpu.xml"


def _colliding_inputs(ref, n_envs, steps, seed):
    """(state, ctrl) pairs on rodent_cpu: random poses inside the joint limits, about half of them with sphere / capsule pairs in
    penetration (the recipe of tests/test_gpu_self_collision.py)."""
    path = assets.asset_path("rodent_cpu")
    tab = mjcf.load_blob(path)
    M = ref.RefModel(path, "f64")
    rng = np.random.default_rng(seed)
    lo, hi = tab["jnt_range"][:, 0], tab["jnt_range"][:, 1]
    pen, free = [], []
    d = ref.RefData(M)
    while len(pen) < n_envs * steps // 2 or len(free) < n_envs * steps // 2:
        q = (tab["qpos0"] + rng.uniform(0.2, 1.0) * rng.uniform(lo, hi)).astype(np.float64)
        d.init(q, np.zeros(M.nv))
        (pen if (d.get("con_dist") < 0).any() else free).append(q)
    seq, npen = [], 0
    for t in range(steps):
        qs = []
        for e in range(n_envs):
            src = pen if (e + t) % 2 == 0 and pen else free
            qs.append(src.pop())
        st = dict(qpos=np.asarray(qs), qvel=rng.uniform(-0.5, 0.5, (n_envs, M.nv)), act=rng.uniform(-0.5, 0.5, (n_envs, M.nu)),
                  qacc_warmstart=np.zeros((n_envs, M.nv)))
        seq.append(({k: parity.f32r(v) for k, v in st.items()}, parity.f32r(rng.uniform(-1, 1, (n_envs, M.nu)))))
    return seq, tab


def _folded_pose(ref):
    """Every joint at the same end of its range (alternating): the animal folded into itself.  Returns (pose, number of pairs in
    penetration by the float64 oracle) -- the pose of test_contact_slot_overflow_is_counted."""
    tab = mjcf.load_blob(assets.asset_path("rodent_cpu"))
    M = ref.RefModel(assets.asset_path("rodent_cpu"), "f64")
    d = ref.RefData(M)
    worst, q_worst = -1, None
    for sgn in (0, 1):
        q = np.where(np.arange(67) % 2 == sgn, tab["jnt_range"][:, 0], tab["jnt_range"][:, 1]).astype(np.float64) * 0.98
        d.init(q, np.zeros(67))
        n = int((d.get("con_dist") < 0).sum())
        if n > worst:
            worst, q_worst = n, q
    return q_worst, worst


def _make(N, episode_length, z_range, keys):
    from rodent_amd import envs
    from rodent_amd.envs import wrappers
    env = envs.get_environment("rodent", track_pos=util.synthetic_track(), num_envs=N, xml_path=MODEL, iterations=6, ls_iterations=6,
                               device=DEV, healthy_z_range=z_range)
    wenv = wrappers.wrap(env, episode_length=episode_length, action_repeat=1)
    return env, wenv, wenv.reset(keys)


def _assert_same_state(got, want):
    """Every leaf equal bit for bit (an entry that is NaN on both sides counts as equal: `torch.equal` alone would call a state that
    blew up identically on both paths different)."""
    from rodent_amd.envs import graphed
    la, lb = graphed.tree_leaves(got), graphed.tree_leaves(want)
    assert len(la) == len(lb)
    for i, (x, y) in enumerate(zip(la, lb)):
        assert x.shape == y.shape, i
        same = (x == y) | (torch.isnan(x) & torch.isnan(y)) if x.is_floating_point() else x == y
        assert bool(same.all()), (i, int((~same).sum()))


# qpos[2] of rodent_cpu.xml is a hinge angle (the model has no free joint); the epilogue applies the reference's "healthy z" rule to it
# literally.  Under uniform random actions the float64 oracle shows it swinging within about +-0.45 rad (10 % / 90 % quantiles of a
# step: -0.23 / +0.22; over 7 steps about a quarter of 80 envs leave +-0.3), so this band ends some episodes early and lets the
# others run into episode_length.
Z_BAND = (-0.3, 0.3)


def test_multi_step_rollout_equals_single_steps_on_the_self_collision_model():
    """rr_env_unroll on rodent_cpu.xml leaves every leaf of the state exactly as T calls of the wrapped step do -- through episode
    ends (episode_length 7) and unhealthy terminations -- and so do chained launches (8 + the rest)."""
    from rodent_amd import jax_random
    dev = torch.device(DEV)
    N, T = 80, 21
    g = torch.Generator(device=dev).manual_seed(21)
    acts = torch.rand(T, N, 38, device=dev, generator=g) * 2 - 1
    keys = jax_random.split(jax_random.PRNGKey(5), N)
    env, wenv, s0 = _make(N, 7, Z_BAND, keys)
    assert env._batch.unroll_supported(with_actor=False) and env._batch.unroll_supported(with_actor=True)
    want = wenv.step(s0, acts[0])
    n_term = n_trunc = 0
    ended_early = torch.zeros(N, dtype=torch.bool, device=dev)
    for t in range(1, T):
        want = wenv.step(want, acts[t])
        n_trunc += int((want.info["truncation"] > 0).sum())
        term = (want.done > 0) & (want.info["truncation"] == 0)
        n_term += int(term.sum())
        ended_early |= term
    env2, wenv2, s2 = _make(N, 7, Z_BAND, keys)
    st2 = wenv2.step(s2, acts[0])
    c1 = env2.contact_overflow()
    got = wenv2.unroll(st2, acts[1:])
    torch.cuda.synchronize()
    print(f"terminations {n_term} (envs {int(ended_early.sum())} of {N}), truncations {n_trunc}")
    assert n_trunc > 0 and n_term > 0 and 0 < int(ended_early.sum()) < N          # both kinds of reset happened; not every env terminates
    assert all(torch.isfinite(x).all() for x in (got.obs, got.pipeline_state.qpos, got.pipeline_state.qvel))
    _assert_same_state(got, want)
    c2 = env2.contact_overflow()
    assert c2 == env.contact_overflow()                           # the same (env, env step) events counted by both paths
    got2 = wenv2.unroll(wenv2.unroll(st2, acts[1:9]), acts[9:])
    torch.cuda.synchronize()
    _assert_same_state(got2, want)
    assert env2.contact_overflow() - c2 == c2 - c1                # ... and by the chained launches over the same steps


def test_contacts_and_slot_overflow_are_counted_alike(oracle_built):
    """Envs started from self-colliding poses and from the folded pose: the T-step launch and the T single launches (a second batch)
    agree bit for bit, and `contact_overflow()` counts the same (env, env step) events on both.
    Measured on the MI355X: the float64 oracle finds 20 pairs in penetration at the folded pose itself (fewer than the 64 slots), but
    released from it the folded envs blow up within their first env step -- more than 64 pairs in penetration on the way (14 overflow
    events in step 1, 46 over the 12 steps, the same on both paths) and 14 of the 16 end non-finite, on the per-step path exactly as
    in the one launch.  Hence the NaN-aware comparison; the blow-up itself is what the counter and `ppo.train`'s warning are for."""
    from rodent_amd import jax_random
    dev = torch.device(DEV)
    N, T = 64, 12
    seq, _ = _colliding_inputs(oracle_built, N, 1, seed=31)
    poses = seq[0][0]["qpos"].astype(np.float32).copy()
    folded, worst = _folded_pose(oracle_built)
    poses[N - 16:] = folded.astype(np.float32)                 # 24 envs with pairs in penetration, 24 without, 16 folded
    g = torch.Generator(device=dev).manual_seed(22)
    acts = torch.rand(T, N, 38, device=dev, generator=g) * 2 - 1
    acts[:, N - 8:] = 0                                          # half of the folded envs are left alone, half are driven
    keys = jax_random.split(jax_random.PRNGKey(6), N)

    def start():
        # the poses go in as the CURRENT and as the stored FIRST state (the observation leaves stay those of the reset: neither path reads
        # them), so the folded envs come back folded when their episode ends, in the middle of the launch
        env, wenv, s0 = _make(N, 9, (-10.0, 10.0), keys)
        ps = s0.pipeline_state.replace(qpos=torch.tensor(poses, device=dev), qvel=torch.zeros_like(s0.pipeline_state.qvel))
        info = dict(s0.info)
        info["first_pipeline_state"] = ps
        return env, wenv, s0.replace(pipeline_state=ps, info=info)
    env_a, wenv_a, want = start()
    per_step = []
    for t in range(T):
        want = wenv_a.step(want, acts[t])
        per_step.append(env_a.contact_overflow())
    env_b, wenv_b, st_b = start()
    assert env_b.contact_overflow() == 0
    got = wenv_b.unroll(st_b, acts)
    torch.cuda.synchronize()
    _assert_same_state(got, want)
    a, b = env_a.contact_overflow(), env_b.contact_overflow()
    bad = ~torch.isfinite(want.pipeline_state.qpos).all(1)
    print(f"envs with a non-finite state after {T} steps (both paths alike): {bad.nonzero().flatten().tolist()}")
    print(f"folded pose: {worst} pairs in penetration by the float64 oracle (slots: 64); overflow events of {T} single launches {a} "
          f"(running total per step {per_step}), of one {T}-step launch {b}")
    assert a == b and isinstance(b, int) and b <= N * T
    if b == 0:
        print("no env ever had more than 64 pairs in penetration: the counters were compared as 0 == 0 -- NO overflow coverage in this run")
    if worst > 64:
        assert b > 0 and per_step[0] > 0                          # the folded envs overflow in their first step at the least


@torch.no_grad()
def _policy64(net, norm, obs, noise, min_std):
    """The policy in float64 on `obs` [M, K] with the given noise [M, A]: (raw, action, log_prob)."""
    x = (obs.double() - norm.mean.double()) / norm.std.double()
    layers = list(net.layers)
    for i, l in enumerate(layers):
        x = x @ l.weight.double().t() + l.bias.double()
        if i != len(layers) - 1:
            x = torch.nn.functional.silu(x)
    loc, s = torch.chunk(x, 2, dim=-1)
    scale = torch.nn.functional.softplus(s) + min_std
    raw = loc + scale * noise.double()
    lp = -0.5 * ((raw - loc) / scale) ** 2 - torch.log(scale) - 0.5 * math.log(2 * math.pi)
    lp = (lp - 2.0 * (math.log(2.0) - raw - torch.nn.functional.softplus(-2.0 * raw))).sum(-1)
    return raw, torch.tanh(raw), lp


def test_one_launch_unroll_with_the_actor_inside_38_actuators():
    """rr_env_unroll_policy on rodent_cpu.xml (A = 38: the two-pass head).  (a) replaying the recorded actions through the per-step path
    reproduces every recorded observation, discount, truncation and the final state bit for bit, the reward to one ulp (2.5e-7, as
    test_one_launch_unroll_with_the_actor_inside allows and explains); (b) the same steps recorded as three segments give identical
    buffers; (c) raw actions / actions / log-probs are those of the policy evaluated by torch in float64 on the recorded
    observations with the same noise: 2e-5 relative on raw, 2e-5 on actions, 2e-3 on log-prob (the bounds of the 60-logit test)."""
    from rodent_amd import jax_random
    from rodent_amd.envs import graphed
    from rodent_amd.training import acting, networks, running_statistics
    dev = torch.device(DEV)
    N, T = 64, 9
    torch.manual_seed(4)
    keys = jax_random.split(jax_random.PRNGKey(3), N)
    env, wenv, st0 = _make(N, 5, Z_BAND, keys)
    assert env.action_size == 38
    nets = networks.make_ppo_networks(env.observation_size, env.action_size, device=dev)
    net, dist = nets.policy_network, nets.parametric_action_distribution
    for l in net.layers:
        l.bias.data.uniform_(-0.3, 0.3)
    norm = running_statistics.init_state(env.observation_size, dev)
    norm.mean.copy_(torch.randn(env.observation_size, device=dev) * 0.05)
    norm.std.copy_(torch.rand(env.observation_size, device=dev) + 0.7)
    assert acting.fused_unroll_supported(wenv, net, dist)
    buf = acting.UnrollBuffer(2, N, T, env.observation_size, env.action_size, dev)
    actor = acting.actor_params(net, norm, dist.min_std)
    assert actor["head_wt"].shape == (32, 128)
    noise = torch.randn(T, N, env.action_size, device=dev)
    traj = dict(obs=buf.obs[1], raw_action=buf.raw_action[1], log_prob=buf.log_prob[1], reward=buf.reward[1], discount=buf.discount[1],
                truncation=buf.truncation[1])
    got, actions = wenv.unroll_policy(st0, actor, noise, traj)
    torch.cuda.synchronize()
    assert torch.isfinite(buf.obs[1]).all() and torch.isfinite(buf.log_prob[1]).all()
    # (b) three trajectories of three steps in one launch: same transitions
    env3, wenv3, st3 = _make(N, 5, Z_BAND, keys)
    buf3 = acting.UnrollBuffer(3, N, 3, env.observation_size, env.action_size, dev)
    traj3 = dict(obs=buf3.obs, raw_action=buf3.raw_action, log_prob=buf3.log_prob, reward=buf3.reward, discount=buf3.discount, truncation=buf3.truncation)
    got3, actions3 = wenv3.unroll_policy(st3, actor, noise, traj3, segment=3)
    torch.cuda.synchronize()
    assert torch.equal(actions3, actions) and torch.equal(got3.obs, got.obs) and torch.equal(got3.pipeline_state.qpos, got.pipeline_state.qpos)
    for u in range(3):
        assert torch.equal(buf3.obs[u], buf.obs[1, :, 3 * u:3 * u + 4]) and torch.equal(buf3.raw_action[u], buf.raw_action[1, :, 3 * u:3 * u + 3])
        for name in ("log_prob", "reward", "discount", "truncation"):
            assert torch.equal(getattr(buf3, name)[u], getattr(buf, name)[1, :, 3 * u:3 * u + 3]), name
    # (a) physics + wrappers: replay the recorded actions step by step
    env2, wenv2, st = _make(N, 5, Z_BAND, keys)
    rew_gap = 0.0
    for t in range(T):
        assert torch.equal(buf.obs[1, :, t], st.obs), t
        st = wenv2.step(st, actions[t])
        rew_gap = max(rew_gap, float((buf.reward[1, :, t] - st.reward).abs().max()))
        assert (buf.reward[1, :, t] - st.reward).abs().max() <= 2.5e-7 and torch.equal(buf.discount[1, :, t], 1 - st.done), t
        assert torch.equal(buf.truncation[1, :, t], st.info["truncation"]), t
    assert torch.equal(buf.obs[1, :, T], st.obs)
    assert float(buf.truncation[1].sum()) > 0                          # episodes of 5 steps: the reset path ran
    la, lb = graphed.tree_leaves(got), graphed.tree_leaves(st)
    assert len(la) == len(lb)
    ninexact = 0
    for x, y in zip(la, lb):
        assert x.shape == y.shape
        if not torch.equal(x, y):                # reward and its pos_reward metric: one ulp; everything else exact
            assert x.dim() == 1 and (x - y).abs().max() <= 2.5e-7
            ninexact += 1
    assert ninexact <= 2
    assert torch.equal(got.pipeline_state.qpos, st.pipeline_state.qpos) and torch.equal(got.obs, st.obs) and torch.equal(got.done, st.done)
    assert env.contact_overflow() == env2.contact_overflow()
    # (c) the actor against float64
    obs_t = buf.obs[1, :, :T].transpose(0, 1).reshape(T * N, -1)
    raw, act, lp = _policy64(net, norm, obs_t, noise.reshape(T * N, -1), dist.min_std)
    raw_k = buf.raw_action[1].transpose(0, 1).reshape(T * N, -1).double()
    lp_k = buf.log_prob[1].transpose(0, 1).reshape(-1).double()
    e_raw = float((raw_k - raw).abs().max()) / max(1.0, float(raw.abs().max()))
    e_act = float((actions.reshape(T * N, -1).double() - act).abs().max())
    e_lp = float((lp_k - lp).abs().max())
    print(f"reward gap {rew_gap:.3g}; actor vs float64: raw {e_raw:.3g} (rel), action {e_act:.3g}, log-prob {e_lp:.3g}")
    assert e_raw <= 2e-5
    assert e_act <= 2e-5
    assert e_lp <= 2e-3


def test_ppo_train_collects_its_rollouts_in_one_launch_on_the_self_collision_model(monkeypatch):
    """ppo.train on a 38-actuator env: the rollout phase goes through generate_unrolls_fused; the 76-wide head keeps the learner on the
    autograd path (none of the learner's / actor's <= 64-wide kernels is called); training/contact_overflow is reported."""
    from rodent_amd import envs, hip
    from rodent_amd.envs import wrappers
    from rodent_amd.training import acting, networks
    from rodent_amd.training.agents.ppo import train as ppo
    env = envs.get_environment("rodent", track_pos=util.synthetic_track(), num_envs=64, xml_path=MODEL, iterations=6, ls_iterations=6,
                               device=DEV)
    nets = networks.make_ppo_networks(env.observation_size, env.action_size, device=DEV)
    assert acting.fused_unroll_supported(wrappers.wrap(env, episode_length=150, action_repeat=1), nets.policy_network,
                                         nets.parametric_action_distribution)
    calls = {"fused": 0, "per_step": 0, "narrow": []}
    real_fused, real_unroll = acting.generate_unrolls_fused, acting.generate_unroll
    monkeypatch.setattr(acting, "generate_unrolls_fused", lambda *a, **k: (calls.__setitem__("fused", calls["fused"] + 1), real_fused(*a, **k))[1])
    monkeypatch.setattr(acting, "generate_unroll", lambda *a, **k: (calls.__setitem__("per_step", calls["per_step"] + 1), real_unroll(*a, **k))[1])
    for name in ("mlp_forward", "policy_act", "policy_sample", "ppo_loss"):        # kernels limited to heads of <= 64 logits

        def refuse(*a, _n=name, **k):
            calls["narrow"].append(_n)
            raise AssertionError(f"hip.{_n} called for a 76-wide head")
        monkeypatch.setattr(hip, name, refuse)
    log = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)           # the overflow warning is allowed, not required
        _, params, _ = ppo.train(environment=env, num_timesteps=10 ** 9, episode_length=150, num_envs=64, batch_size=64, num_minibatches=4,
                                 unroll_length=5, num_updates_per_batch=2, num_evals=2, num_eval_envs=0, learning_rate=5e-5, entropy_cost=1e-3,
                                 discounting=0.97, normalize_observations=True, seed=1, max_training_steps=2, progress_fn=lambda n, m: log.append(m))
    assert calls["fused"] == 2 and calls["per_step"] == 0 and not calls["narrow"]
    assert math.isfinite(float(log[-1]["training/total_loss"])) and float(params[0].count) == 64 * 4 * 5 * 2
    assert "training/contact_overflow" in log[-1] and log[-1]["training/contact_overflow"] >= 0
    assert log[-1]["training/contact_overflow"] <= env.contact_overflow()
