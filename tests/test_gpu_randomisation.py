"""Domain randomisation on the GPU: batches whose environments carry their own friction / damping / armature / actuator-gain rows
(`rr_batch_set_env_params`, the rr_rand_kernel instances) against plain batches of the same build -- bit for bit -- and against the
CPU oracle.  Fixture: tests/randomisation_sets.py, three parameter sets, env e of a mixed batch on set e % 3; each set is also a model
blob of its own (`with_parameters` + `save_blob`), which a plain batch and the oracle load like any other model."""
import math

import numpy as np
import pytest
import torch

from rodent_amd import assets, hip, jax_random, mjcf
from rodent_amd.ktables import env_param_tables
from tests import parity, randomisation_sets as rs, util

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = rs.G


def _env(model, n, **kw):
    """`model`: a shipped model's name, or the path of a blob (.rrm)."""
    from rodent_amd import envs
    path = model if model.endswith(".rrm") else f"{model}.xml"
    return envs.get_environment("rodent", track_pos=util.synthetic_track(), num_envs=n, xml_path=path, iterations=8, ls_iterations=8,
                                device=DEV, **kw)


def _mixed_env(model, n, **kw):
    env = _env(model, n, **kw)
    fn = rs.system_fn(rs.mixed_fields)
    env.randomize(lambda sys: fn(sys, n))
    return env


def _leaves(state):
    from rodent_amd.envs import graphed
    return graphed.tree_leaves(state)


def _assert_same(got, want, rows=None, what=""):
    """Every leaf of the two states equal bit for bit (`rows`: the envs of `got` that `want` holds)."""
    la, lb = _leaves(got), _leaves(want)
    assert len(la) == len(lb) > 10
    for i, (x, y) in enumerate(zip(la, lb)):
        x = x if rows is None else x[rows]
        assert x.shape == y.shape and torch.equal(x, y), (what, i, int((x != y).sum()))


def _actor(env, seed):
    from rodent_amd.training import acting, networks, running_statistics
    torch.manual_seed(seed)
    nets = networks.make_ppo_networks(env.observation_size, env.action_size, device=DEV)
    net, dist = nets.policy_network, nets.parametric_action_distribution
    for l in net.layers:
        l.bias.data.uniform_(-0.3, 0.3)
    norm = running_statistics.init_state(env.observation_size, torch.device(DEV))
    norm.mean.copy_(torch.randn(env.observation_size, device=DEV) * 0.05)
    norm.std.copy_(torch.rand(env.observation_size, device=DEV) + 0.7)
    return net, dist, acting.actor_params(net, norm, dist.min_std)


def _traj(buf):
    return dict(obs=buf.obs[0], raw_action=buf.raw_action[0], log_prob=buf.log_prob[0], reward=buf.reward[0], discount=buf.discount[0],
                truncation=buf.truncation[0])


def _run_three_paths(env, keys, acts, actor, noise, episode_length):
    """The three launch forms on one env: T wrapped single steps; one wrapped step + a (T-1)-step unroll; an actor-inside unroll.
    Returns (state after the steps, state after the unroll, state after the policy unroll, its actions, its buffer)."""
    from rodent_amd.envs import wrappers
    from rodent_amd.training import acting
    wenv = wrappers.wrap(env, episode_length=episode_length, action_repeat=1)
    s0 = wenv.reset(keys)
    s = s0
    for t in range(acts.shape[0]):
        s = wenv.step(s, acts[t])
    u = wenv.unroll(wenv.step(wenv.reset(keys), acts[0]), acts[1:])
    buf = acting.UnrollBuffer(1, env.num_envs, noise.shape[0], env.observation_size, env.action_size, torch.device(DEV))
    p, actions = wenv.unroll_policy(wenv.reset(keys), actor, noise, _traj(buf))
    torch.cuda.synchronize()
    return s, u, p, actions, buf


@pytest.mark.parametrize("model", ["rodent_optimized", "rodent_new"])
def test_identity_parameters_equal_a_plain_batch(model):
    """Every env carrying the model's own values: the rr_rand_kernel instances give what rr_step_kernel gives, bit for bit, over 23
    wrapped steps with episodes of 7 (single steps, the multi-step launch, the launch with the actor inside)."""
    N, T = 64, 23
    keys = jax_random.split(jax_random.PRNGKey(11), N)
    gen = torch.Generator(device=DEV).manual_seed(2)
    acts = torch.rand(T, N, 30, device=DEV, generator=gen) * 2 - 1
    noise = torch.randn(T, N, 30, device=DEV, generator=gen)
    plain, rand = _env(model, N), _env(model, N)
    m = rand.sys.tables
    ident = {k: np.repeat(v[None], N, axis=0) for k, v in rs.base_fields(m).items()}
    dof_f, act_f, con_f = (torch.from_numpy(a).to(DEV) for a in env_param_tables(m, ident))
    assert rand._batch.env_params_supported() and rand.env_params() is None
    rand.set_env_params(dof_f=dof_f, act_f=act_f, con_f=con_f)
    assert rand.env_params() is not None and rand._batch.unroll_supported(False) and rand._batch.unroll_supported(True)
    _, _, actor = _actor(plain, 7)
    a, b = _run_three_paths(plain, keys, acts, actor, noise, 7), _run_three_paths(rand, keys, acts, actor, noise, 7)
    for i, what in enumerate(("wenv.step", "wenv.unroll", "unroll_policy")):
        _assert_same(b[i], a[i], what=what)
    assert torch.equal(b[3], a[3])
    for name in ("obs", "raw_action", "log_prob", "reward", "discount", "truncation"):
        assert torch.equal(getattr(b[4], name), getattr(a[4], name)), name
    assert bool((a[4].discount == 0).any())                   # episodes ended (7 steps, or unhealthy before): the reset path ran
    # clearing the parameters gives the plain batch back; a partial set (friction only) is a legal state too
    rand.set_env_params()
    assert rand.env_params() is None
    _assert_same(_run_three_paths(rand, keys, acts[:3], actor, noise[:3], 7)[0], _run_three_paths(plain, keys, acts[:3], actor, noise[:3], 7)[0])
    rand.set_env_params(con_f=con_f)
    _assert_same(_run_three_paths(rand, keys, acts[:3], actor, noise[:3], 7)[0], _run_three_paths(plain, keys, acts[:3], actor, noise[:3], 7)[0])


@pytest.mark.parametrize("model,balance", [("rodent_optimized", False), ("rodent_new", False), ("rodent_0", False), ("rodent_optimized", True)])
def test_mixed_batch_equals_homogeneous_batches(model, balance, tmp_path):
    """96 envs, env e on set e % 3, against three plain batches of 32 envs built from the three sets' blobs with the same keys
    and actions: every state leaf and every trajectory buffer identical, on the single-step, multi-step and actor-inside paths.
    rodent_optimized / rodent_new run the fixed-dimension instances, rodent_0 (34 contacts) the generic one.  `balance`: with the
    workgroup -> env map set (envs re-paired every second launch), still bit for bit."""
    N, T = 96, 12
    n = N // G
    assert hip.Model(assets.asset_path(model)).dims.fixed_instance == (0 if model == "rodent_0" else 1)
    stems = rs.write_blobs(model, tmp_path)
    keys = jax_random.split(jax_random.PRNGKey(13), N)
    gen = torch.Generator(device=DEV).manual_seed(4)
    acts = torch.rand(T, N, 30, device=DEV, generator=gen) * 2 - 1
    noise = torch.randn(T, N, 30, device=DEV, generator=gen)
    kw = dict(balance=True, rebalance_every=2) if balance else {}
    mixed = _mixed_env(model, N, **kw)
    _, _, actor = _actor(mixed, 9)
    got = _run_three_paths(mixed, keys, acts, actor, noise, 5)
    if balance:
        assert not torch.equal(mixed._env_map, torch.arange(N, dtype=torch.int32, device=DEV))      # the map was in use, and not the identity
    differ = 0
    for g in range(G):
        rows = torch.arange(g, N, G, device=DEV)
        homog = _env(stems[g] + ".rrm", n)
        assert homog.env_params() is None
        want = _run_three_paths(homog, keys[g::G], acts[:, rows].contiguous(), actor, noise[:, rows].contiguous(), 5)
        for i, what in enumerate(("wenv.step", "wenv.unroll", "unroll_policy")):
            _assert_same(got[i], want[i], rows=rows, what=(what, g))
        assert torch.equal(got[3][:, rows], want[3])
        for name in ("obs", "raw_action", "log_prob", "reward", "discount", "truncation"):
            assert torch.equal(getattr(got[4], name)[:, rows], getattr(want[4], name)), (name, g)
        if g != 1:          # a set with other parameters is another trajectory: the plain batch of the shipped model does not reproduce it
            base = _run_three_paths(_env(model, n), keys[g::G], acts[:, rows].contiguous(), actor, noise[:, rows].contiguous(), 5)
            differ += int(not torch.equal(base[0].pipeline_state.qpos, want[0].pipeline_state.qpos))
    assert differ == 2


def test_parameter_sets_give_different_trajectories():
    """From identical states under identical actions, sets 0 and 2 part: after 20 steps qpos, obs and reward differ (where the identity
    test measures exactly zero)."""
    N = 48
    mixed = _mixed_env("rodent_optimized", N)
    keys = np.repeat(jax_random.split(jax_random.PRNGKey(17), N // G), G, axis=0)          # envs 3k, 3k+1, 3k+2 start alike
    gen = torch.Generator(device=DEV).manual_seed(6)
    acts = (torch.rand(20, N // G, 30, device=DEV, generator=gen) * 2 - 1).repeat_interleave(G, dim=1)
    s = mixed.reset(keys)
    assert torch.equal(s.pipeline_state.qpos[0::G], s.pipeline_state.qpos[2::G])
    for t in range(20):
        s = mixed.step(s, acts[t])
    torch.cuda.synchronize()
    d_qpos = float((s.pipeline_state.qpos[0::G] - s.pipeline_state.qpos[2::G]).abs().max())
    d_obs = float((s.obs[0::G] - s.obs[2::G]).abs().max())
    d_rew = float((s.reward[0::G] - s.reward[2::G]).abs().max())
    print(f"sets 0 and 2 after 20 steps: max |dqpos| {d_qpos:.3g}, max |dobs| {d_obs:.3g}, max |dreward| {d_rew:.3g}")
    assert torch.isfinite(s.obs).all()
    assert d_qpos > 0 and d_obs > 0 and d_rew > 0


class _Grouped:
    """An env-step impl of the parity harness over a mixed batch: rows e % 3 == g go to the impl of set g."""

    def __init__(self, impls):
        self.impls = impls

    def env_step(self, st, ctrl, cur_frame):
        n = len(cur_frame)
        outs = [imp.env_step({k: v[g::G] for k, v in st.items()}, ctrl[g::G], cur_frame[g::G]) for g, imp in enumerate(self.impls)]
        res = {}
        for k in outs[0]:
            if k == "metrics":
                continue
            a = np.zeros((n,) + np.shape(outs[0][k])[1:], np.asarray(outs[0][k]).dtype)
            for g in range(G):
                a[g::G] = outs[g][k]
            res[k] = a
        return res


class _HipMixed:
    def __init__(self, env):
        self.env = env
        self.state0 = env.reset(0)

    def env_step(self, st, ctrl, cur_frame):
        ps = self.state0.pipeline_state.replace(**{k: torch.tensor(st[k], dtype=torch.float32, device=DEV).contiguous() for k in parity.STATE})
        s = self.state0.replace(pipeline_state=ps, info=dict(cur_frame=torch.tensor(cur_frame, dtype=torch.int32, device=DEV)))
        ns = self.env.step(s, torch.tensor(ctrl, dtype=torch.float32, device=DEV))
        out = {k: getattr(ns.pipeline_state, k).cpu().numpy().astype(np.float64) for k in parity.STATE}
        out.update(obs=ns.obs.cpu().numpy().astype(np.float64), reward=ns.reward.cpu().numpy().astype(np.float64),
                   done=ns.done.cpu().numpy().astype(np.float64), cur_frame=ns.info["cur_frame"].cpu().numpy())
        return out


def test_mixed_batch_against_the_oracle(oracle_built, tmp_path):
    """One mixed batch (48 envs, 120 teacher-forced env steps: 5760 samples) through `parity.envstep_ladder` unchanged: each env's group
    is held to the float64 oracle of ITS blob, with the float32 oracle of the same blob as the gap; the existing criteria
    (`check_quantiles` with `ENV_FLOORS`) decide.  The input states of group g come from the float64 oracle's own rollout on blob g."""
    n, T = 16, 120
    N = n * G
    track = util.synthetic_track()
    stems = rs.write_blobs("rodent_optimized", tmp_path)
    seqs, tab = [], None
    for g in range(G):
        seq, _, tab = parity.rollout_inputs(stems[g], n, T, (8, 8), seed=35 + g, n_frames=10, reset_every=150)
        seqs.append(seq)
    rng = np.random.default_rng(36)
    seq = []
    for t in range(T):
        st = {k: np.zeros((N,) + seqs[0][t][0][k].shape[1:]) for k in parity.STATE}
        ctrl = np.zeros((N, 30))
        for g in range(G):
            for k in parity.STATE:
                st[k][g::G] = seqs[g][t][0][k]
            ctrl[g::G] = seqs[g][t][1]
        seq.append((st, ctrl, rng.integers(0, 260, N).astype(np.int32)))
    A = _Grouped([parity.OracleEnvImpl(stems[g], n, "f64", (8, 8), track) for g in range(G)])
    gap = _Grouped([parity.OracleEnvImpl(stems[g], n, "f32", (8, 8), track) for g in range(G)])
    out = parity.envstep_ladder(_HipMixed(_mixed_env("rodent_optimized", N)), seq, A, gap, tab)
    for row in out["quantiles"]:
        print("envsteps_mixed", row)
    assert out["samples"] == N * T
    parity.check_quantiles(out["quantiles"], parity.ENV_FLOORS)
    # the check has teeth: the plain batch of the shipped model, held to the same per-set oracles, is far outside them
    plain = parity.envstep_ladder(_HipMixed(_env("rodent_optimized", N)), seq[:10], A, gap, tab)
    with pytest.raises(AssertionError):
        parity.check_quantiles(plain["quantiles"], parity.ENV_FLOORS)


def test_refusals():
    """Models / solvers / outputs without an instance that reads per-env rows say so."""
    fn = rs.system_fn(rs.mixed_fields)
    for model, why in (("rodent_cpu", "candidate-pair"), ("rodent_pair", "two-wave pair")):
        env = _env(model, 8) if model != "rodent_cpu" else _env(model, 8, healthy_z_range=(-0.3, 0.3))
        assert not env._batch.env_params_supported()
        with pytest.raises(RuntimeError, match="per-env parameters.*" + why):
            env.randomize(lambda sys: fn(sys, 8))
        assert env.env_params() is None
    from rodent_amd import envs
    newton = envs.get_environment("rodent", track_pos=util.synthetic_track(), num_envs=8, xml_path="rodent_optimized.xml", solver="newton",
                                  iterations=4, ls_iterations=8, device=DEV)
    with pytest.raises(RuntimeError, match="per-env parameters.*Newton"):
        newton.randomize(lambda sys: fn(sys, 8))
    # a debug dump, the contact-geometry outputs and the profile build on a randomised batch
    env = _mixed_env("rodent_optimized", 8)
    b = env._batch
    st = b.zeros_state()
    st["qpos"][:] = torch.from_numpy(env.sys.qpos0).to(DEV)
    ctrl = torch.zeros(8, 30, device=DEV)
    b.pipeline_step(st, ctrl, 1)                                                   # the plain outputs are served
    b.pipeline_step(st, ctrl, 1, out=dict(xpos=torch.empty(8, env.sys.nbody, 3, device=DEV)))
    with pytest.raises(RuntimeError, match="debug dump.*per-env parameters"):
        b.pipeline_step(st, ctrl, 1, out=dict(debug=torch.zeros(8, b.dims.dbg_floats, device=DEV)))
    with pytest.raises(RuntimeError, match="contact-geometry.*per-env parameters"):
        b.pipeline_step(st, ctrl, 1, out=dict(contact_dist=torch.zeros(8, env.sys.ncon, device=DEV)))
    with pytest.raises(RuntimeError, match="profile.*per-env parameters"):
        b.set_profile(torch.zeros(8, 16, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="dof_f has shape"):
        b.set_env_params(dof_f=torch.zeros(7, env.sys.nv, 16, device=DEV))
    # fields outside the supported five, through the env's surface
    with pytest.raises(ValueError, match="body_mass"):
        env.randomize(lambda sys: (sys.replace(body_mass=np.repeat(sys.body_mass[None], 8, axis=0)), {"body_mass": 0}))
    with pytest.raises(ValueError, match="leading axis of 8 envs"):
        env.randomize(lambda sys: (sys.replace(dof_damping=np.repeat(sys.dof_damping[None], 7, axis=0)), {"dof_damping": 0}))
    torch.cuda.synchronize()
    assert torch.isfinite(st["qpos"]).all()


def _draw(sys, rng):
    """A randomization_fn in brax's shape: per env (key) a friction scale and a gain scale."""
    n = len(rng)
    ks = jax_random.split(rng, 2)
    friction = np.repeat(sys.geom_friction[None], n, axis=0)
    friction[:, :, 0] *= jax_random.uniform(ks[:, 0], 1, 0.6, 1.4)
    scale = jax_random.uniform(ks[:, 1], 1, 0.8, 1.2)[:, :, None]
    gain = np.repeat(sys.actuator_gainprm[None], n, axis=0)
    bias = np.repeat(sys.actuator_biasprm[None], n, axis=0)
    gain[:, :, 0:1] *= scale
    bias[:, :, 1:2] *= scale
    return sys.tree_replace({"geom_friction": friction, "actuator_gainprm": gain, "actuator_biasprm": bias}), \
        {"geom_friction": 0, "actuator_gainprm": 0, "actuator_biasprm": 0}


def test_ppo_train_with_a_randomization_fn(monkeypatch):
    """Two training steps at 64 envs with a randomization_fn: the rollouts still go through the one-launch path, the loss is finite,
    and the training / eval envs carry the rows the function returned for the keys `train` binds on this rank."""
    from rodent_amd.training import acting
    from rodent_amd.training.agents.ppo import train as ppo
    env = _env("rodent_optimized", 64)
    calls = {"fused": 0, "per_step": 0}
    real_fused, real_unroll = acting.generate_unrolls_fused, acting.generate_unroll
    monkeypatch.setattr(acting, "generate_unrolls_fused", lambda *a, **k: (calls.__setitem__("fused", calls["fused"] + 1), real_fused(*a, **k))[1])
    monkeypatch.setattr(acting, "generate_unroll", lambda *a, **k: (calls.__setitem__("per_step", calls["per_step"] + 1), real_unroll(*a, **k))[1])
    seen, log = [], []

    def fn(sys, rng):
        seen.append(np.asarray(rng).copy())
        return _draw(sys, rng)
    eval_env = env.with_num_envs(32)
    assert eval_env.env_params() is None                    # a sibling env starts without parameters: another size needs other draws
    ppo.train(environment=env, num_timesteps=10 ** 9, episode_length=150, num_envs=64, batch_size=64, num_minibatches=4, unroll_length=5,
              num_updates_per_batch=2, num_evals=2, num_eval_envs=32, eval_env=eval_env, learning_rate=5e-5, entropy_cost=1e-3, discounting=0.97,
              normalize_observations=True, seed=3, max_training_steps=2, randomization_fn=fn, progress_fn=lambda n, m: log.append(m))
    assert calls["fused"] == 2 and calls["per_step"] == 0
    assert math.isfinite(float(log[-1]["training/total_loss"]))
    k_train, k_eval = ppo.randomization_keys(3, 0, 64, 32)
    assert len(seen) == 2 and np.array_equal(seen[0], k_train) and np.array_equal(seen[1], k_eval)
    for e, keys in ((env, k_train), (eval_env, k_eval)):
        sys_v, _ = _draw(e.sys, keys)
        want = env_param_tables(e.sys.tables, dict(geom_friction=sys_v.geom_friction, actuator_gainprm=sys_v.actuator_gainprm,
                                                   actuator_biasprm=sys_v.actuator_biasprm))
        got = e.env_params()
        assert got["dof_f"] is None                          # nothing of the dof table was randomised: it stays the shared one
        assert np.array_equal(got["act_f"].cpu().numpy(), want[1]) and np.array_equal(got["con_f"].cpu().numpy(), want[2])
        assert len(np.unique(want[2][:, 0, 16])) > len(keys) // 2          # the envs do differ
    # two ranks: other keys, hence other rows (the key split alone; no second process needed)
    k_other, _ = ppo.randomization_keys(3, 1, 64, 32)
    assert not np.array_equal(k_other, k_train)
    other = env_param_tables(env.sys.tables, dict(geom_friction=_draw(env.sys, k_other)[0].geom_friction))[2]
    assert not np.array_equal(other, env.env_params()["con_f"].cpu().numpy())


def test_graph_replay_of_a_randomised_batch():
    """A HIP graph of R wrapped steps of a mixed batch replays to the host-issued result."""
    from rodent_amd.envs import graphed, wrappers
    dev = torch.device(DEV)
    N, R = 48, 3
    keys = jax_random.split(jax_random.PRNGKey(5), N)
    acts = torch.rand(1 + R, N, 30, device=dev, generator=torch.Generator(device=dev).manual_seed(3)) * 2 - 1
    s0 = torch.cuda.Stream(dev)

    def make():
        with torch.cuda.stream(s0):
            wenv = wrappers.wrap(_mixed_env("rodent_new", N), episode_length=3, action_repeat=1)
            return wenv, wenv.reset(keys)
    wenv, st = make()
    with torch.cuda.stream(s0):
        want = st
        for t in range(1 + R):
            want = wenv.step(want, acts[t])
    torch.cuda.synchronize()
    wenv_g, st_g = make()
    cursor = torch.zeros((), dtype=torch.long, device=dev)

    def step_fn(state):
        a = acts.index_select(0, cursor.reshape(1))[0]
        cursor.add_(1)
        return wenv_g.step(state, a)
    with torch.cuda.stream(s0):
        st1 = step_fn(st_g)
    torch.cuda.synchronize()
    g = graphed.GraphedSteps(step_fn, st1, R, s0)
    got = g.replay()
    torch.cuda.synchronize()
    assert int(cursor) == 1 + R
    _assert_same(got, want)
