"""The bad-state check of the step kernel's epilogue (`Rodent(bad_state_max=...)`, rr_env_io::bad_state_max, rr_batch_bad_states) on the GPU.

The yardstick is EMULATION: an env built with the check off, a test-local wrapper that applies the rule in Python to every step it makes
(`bad_state_mask`, then done = 1, reward = 0, metrics = 0) and the Python composition EpisodeWrapper + AutoResetWrapper on top.  The kernel
paths -- bare step, fused single-step wrapper, multi-step launch, actor inside, evaluation -- must leave what it leaves, bit for bit, and
count the events it counts.  Bad states come from values written into the incoming state (a NaN in qpos, +inf in qvel, a finite 1e12 in
a hinge qvel), from a threshold tightened into the range the rollout's own |qvel| reaches, and from the folded pose of rodent_cpu.xml."""
import math
import warnings

import numpy as np
import pytest
import torch

from tests import randomisation_sets as rs, util

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = ((1, "qpos", 5, float("nan")), (4, "qvel", 0, float("inf")), (6, "qvel", 10, 1e12))      # (env, leaf, column, value); column 10 of qvel is a hinge
POISONED = [p[0] for p in POISON]


def _env(model, n, bad=None, iters=2, **kw):
    from rodent_amd import envs
    kw.setdefault("n_frames", 2)
    return envs.get_environment("rodent", track_pos=util.synthetic_track(), num_envs=n, xml_path=f"{model}.xml", iterations=iters,
                                ls_iterations=iters, device=DEV, bad_state_max=bad, **kw)


def _keys(n, seed):
    from rodent_amd import jax_random
    return jax_random.split(jax_random.PRNGKey(seed), n)


def _poison(state, poison=POISON):
    """`state` with the values written into a COPY of its qpos / qvel (the stored first state of the wrappers shares the reset's tensors
    and must stay clean)."""
    ps = state.pipeline_state
    new = dict(qpos=ps.qpos.clone(), qvel=ps.qvel.clone())
    for e, leaf, col, val in poison:
        new[leaf][e, col] = val
    return state.replace(pipeline_state=ps.replace(**new))


def _leaves(state):
    from rodent_amd.envs import graphed
    return graphed.tree_leaves(state)


def _assert_same(got, want, what="", rows=None):
    la, lb = _leaves(got), _leaves(want)
    assert len(la) == len(lb) > 10, (what, len(la), len(lb))
    for i, (x, y) in enumerate(zip(la, lb)):
        if rows is not None:
            x, y = x[rows], y[rows]
        assert x.shape == y.shape and torch.equal(x, y), (what, i, int((x != y).sum()))


def _assert_finite(state, what=""):
    for i, x in enumerate(_leaves(state)):
        assert not x.is_floating_point() or bool(torch.isfinite(x).all()), (what, i)


class RuleEnv:
    """An env built with the check OFF, the rule applied in Python to each step it makes.  Records per step the bad mask and max |qvel|."""

    def __init__(self, env, bad_state_max):
        self.env, self.thr = env, bad_state_max
        self.masks, self.peaks = [], []

    def __getattr__(self, name):
        return getattr(self.env, name)

    @property
    def unwrapped(self):
        return self.env

    def reset(self, rng):
        return self.env.reset(rng)

    def step(self, state, action):
        from rodent_amd.envs.rodent import bad_state_mask
        ns = self.env.step(state, action)
        ps = ns.pipeline_state
        bad = bad_state_mask(ps.qpos, ps.qvel, self.thr)
        self.masks.append(bad)
        self.peaks.append(ps.qvel.abs().amax(1))
        zero, one = torch.zeros_like(ns.reward), torch.ones_like(ns.done)
        return ns.replace(done=torch.where(bad, one, ns.done), reward=torch.where(bad, zero, ns.reward),
                          metrics={k: torch.where(bad, zero, v) for k, v in ns.metrics.items()})

    def count(self):
        return int(torch.stack(self.masks).sum()) if self.masks else 0


def _composed(rule_env, episode_length):
    from rodent_amd.envs import wrappers
    return wrappers.AutoResetWrapper(wrappers.EpisodeWrapper(wrappers.VmapWrapper(rule_env), episode_length, 1))


def _fused(env, episode_length):
    from rodent_amd.envs import wrappers
    w = wrappers.wrap(env, episode_length=episode_length, action_repeat=1)
    assert isinstance(w, wrappers.FusedEpisodeAutoResetWrapper)
    return w


def _actions(T, n, nu, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.rand(T, n, nu, device=DEV, generator=g) * 2 - 1


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


def _threshold_between(peaks, exclude=()):
    """A threshold half-way between the two middle values of the sorted per-env peaks (`exclude`: envs left out): the envs above it trip."""
    keep = [e for e in range(peaks.shape[0]) if e not in exclude]
    v, _ = torch.sort(peaks[keep])
    k = len(keep) // 2
    lo, hi = float(v[k - 1]), float(v[k])
    assert math.isfinite(lo) and math.isfinite(hi) and lo < hi, (lo, hi)
    thr = 0.5 * (lo + hi)
    return thr, [e for e in keep if float(peaks[e]) > thr]


# ---------------------------------------------------------------------------------------------- 1. bare step
def _bare_step_case(model, n, seed, **kw):
    """One bare step of `n` envs, three of them poisoned, with the check on and off."""
    from rodent_amd.envs.rodent import bad_state_mask
    acts = _actions(1, n, 30, seed)[0]
    keys = _keys(n, seed)
    on, off = _env(model, n, bad=1e10, **kw), _env(model, n, **kw)
    clean = off.reset(keys)
    base = off.step(clean, acts)                                   # the same batch without poison
    want = off.step(_poison(clean), acts)
    got = on.step(_poison(on.reset(keys)), acts)
    torch.cuda.synchronize()
    mask = bad_state_mask(want.pipeline_state.qpos, want.pipeline_state.qvel, 1e10)
    print("bad after the step by the rule:", mask.nonzero().flatten().tolist(), "max |qvel| of the poisoned envs",
          want.pipeline_state.qvel[POISONED].abs().amax(1).tolist())
    assert mask.nonzero().flatten().tolist() == POISONED           # the poison survives the step in all three envs, and nowhere else
    assert got.done.nonzero().flatten().tolist() == POISONED and bool((got.done[POISONED] == 1).all())
    assert bool((got.reward[POISONED] == 0).all())
    for k in ("pos_reward", "reward_quadctrl", "reward_alive"):
        assert bool((got.metrics[k][POISONED] == 0).all()), k
    others = [e for e in range(n) if e not in POISONED]
    _assert_same(got, base, "untouched envs", rows=others)
    assert bool((base.done[others] == 0).all())
    # documented limit: the bare step does not sanitise -- the state of the bad envs is the one the check-off step returns
    for k in ("qpos", "qvel"):
        x, y = getattr(got.pipeline_state, k)[POISONED], getattr(want.pipeline_state, k)[POISONED]
        assert bool(((x == y) | (torch.isnan(x) & torch.isnan(y))).all()), k
    assert on.bad_states() == 3 and off.bad_states() == 0
    assert on.with_num_envs(4).bad_state_max == 1e10               # siblings inherit the setting


def test_bare_step_flags_and_counts_the_poisoned_envs():
    _bare_step_case("rodent_optimized", 12, 11)


# ---------------------------------------------------------------------------------------------- 7. Newton
def test_newton_single_step_shares_the_epilogue():
    _bare_step_case("rodent_optimized", 8, 12, solver="newton", iters=4)


# ---------------------------------------------------------------------------------------------- 2. emulation
@pytest.mark.parametrize("model", ["rodent_optimized", "rodent_new", "rodent_0"])
def test_wrapped_paths_equal_the_python_emulation(model):
    N, T, EP = 12, 8, 6
    keys = _keys(N, 21)
    probe_env = _env(model, N)
    acts = _actions(T, N, probe_env.action_size, 22)
    # the check-off run's own max |qvel| per env (no poison, the same wrappers): the threshold goes between two of the sorted values
    probe = RuleEnv(probe_env, 1e10)
    w = _composed(probe, EP)
    st = w.reset(keys)
    for t in range(T):
        st = w.step(st, acts[t])
    assert probe.count() == 0
    thr, trippers = _threshold_between(torch.stack(probe.peaks).amax(0), exclude=POISONED)
    assert 0 < len(trippers) < N - len(POISONED)
    # the emulation
    rule = RuleEnv(_env(model, N), thr)
    w = _composed(rule, EP)
    want = _poison(w.reset(keys))
    for t in range(T):
        want = w.step(want, acts[t])
    tripped = torch.stack(rule.masks).any(0).nonzero().flatten().tolist()
    first = torch.stack(rule.masks).float().argmax(0)
    print(f"{model}: threshold {thr:.4g}; tripped {tripped} (first at steps {first[tripped].tolist()}); events {rule.count()}")
    assert tripped == sorted(set(POISONED) | set(trippers))
    assert bool(torch.stack(rule.masks)[0][POISONED].all()) and int(first[trippers].max()) > 0      # poison at once, the threshold mid-rollout
    _assert_finite(want, "emulation")

    def start():
        env = _env(model, N, bad=thr)
        wenv = _fused(env, EP)
        return env, wenv, _poison(wenv.reset(keys))
    env, wenv, got = start()
    for t in range(T):
        got = wenv.step(got, acts[t])
    _assert_same(got, want, "fused single-step wrapper")
    assert env.bad_states() == rule.count()
    env, wenv, st0 = start()
    got = wenv.unroll(st0, acts)
    _assert_same(got, want, "one launch")
    _assert_finite(got, "one launch")
    assert env.bad_states() == rule.count()
    env, wenv, st0 = start()
    got = wenv.unroll(wenv.unroll(st0, acts[:3].contiguous()), acts[3:].contiguous())
    _assert_same(got, want, "3 + 5")
    assert env.bad_states() == rule.count()


# ---------------------------------------------------------------------------------------------- 3. actor inside
def test_actor_inside_records_the_bad_transition():
    from rodent_amd.training import acting
    model, N, T, EP = "rodent_optimized", 8, 8, 5
    poison = POISON[:2]
    poisoned = [p[0] for p in poison]
    keys = _keys(N, 31)
    env0 = _env(model, N)
    nets, norm, actor = _policy(env0, 5)
    noise = torch.randn(T, N, env0.action_size, device=DEV)

    def launch(bad, with_poison):
        env = _env(model, N, bad=bad)
        wenv = _fused(env, EP)
        assert acting.fused_unroll_supported(wenv, nets.policy_network, nets.parametric_action_distribution)
        buf = acting.UnrollBuffer(1, N, T, env.observation_size, env.action_size, torch.device(DEV))
        traj = dict(obs=buf.obs[0], raw_action=buf.raw_action[0], log_prob=buf.log_prob[0], reward=buf.reward[0], discount=buf.discount[0],
                    truncation=buf.truncation[0])
        st0 = wenv.reset(keys)
        got, actions = wenv.unroll_policy(_poison(st0, poison) if with_poison else st0, actor, noise, traj)
        torch.cuda.synchronize()
        return env, buf, got, actions, st0
    # check off, no poison: the rollout's own max |qvel| per env, from the recorded observations (rows 1 .. T)
    env, buf, _, _, _ = launch(None, False)
    nq, nv = env.sys.nq, env.sys.nv
    thr, trippers = _threshold_between(buf.obs[0][:, 1:, nq:nq + nv].abs().amax((1, 2)), exclude=poisoned)
    env, buf, got, actions, st0 = launch(thr, True)
    # replay of the recorded actions through the emulation
    rule = RuleEnv(_env(model, N), thr)
    w = _composed(rule, EP)
    st = _poison(w.reset(keys), poison)
    for t in range(T):
        assert torch.equal(buf.obs[0][:, t], st.obs), t
        st = w.step(st, actions[t])
        bad = rule.masks[-1]
        assert float((buf.reward[0][:, t] - st.reward).abs().max()) <= 2.5e-7, t       # one ulp (test_one_launch_unroll_with_the_actor_inside)
        assert torch.equal(buf.discount[0][:, t], 1 - st.done) and torch.equal(buf.truncation[0][:, t], st.info["truncation"]), t
        # at the bad transition: reward 0, discount 0, truncation 0, the next observation row the first observation
        assert bool((buf.reward[0][bad, t] == 0).all()) and bool((buf.discount[0][bad, t] == 0).all()) and bool((buf.truncation[0][bad, t] == 0).all())
        assert torch.equal(buf.obs[0][bad, t + 1], st0.obs[bad])
    assert torch.equal(buf.obs[0][:, T], st.obs)
    masks = torch.stack(rule.masks)
    print(f"threshold {thr:.4g}; bad transitions (t, env): {masks.nonzero().tolist()}")
    tripped = masks.any(0).nonzero().flatten().tolist()
    # (the recorded rows hide the stepped state of a step that ended an episode, so the emulation may find more trippers than the rows show)
    assert bool(masks[0][poisoned].all()) and bool(masks[1:].any()) and set(poisoned) | set(trippers) <= set(tripped) and len(tripped) < N
    for name in ("obs", "raw_action", "log_prob", "reward", "discount", "truncation"):
        assert bool(torch.isfinite(getattr(buf, name)).all()), name
    assert bool(torch.isfinite(actions).all())
    for k in ("qpos", "qvel", "act", "qacc_warmstart"):
        assert torch.equal(getattr(got.pipeline_state, k), getattr(st.pipeline_state, k)), k
    assert torch.equal(got.obs, st.obs) and torch.equal(got.done, st.done)
    for k in ("cur_frame", "steps", "truncation"):
        assert torch.equal(got.info[k], st.info[k]), k
    assert env.bad_states() == rule.count()


# ---------------------------------------------------------------------------------------------- 4. evaluation
def test_evaluation_launch_wrapped_and_raw():
    from rodent_amd.envs import wrappers
    model, N, T, EP = "rodent_optimized", 8, 8, 5
    poison = POISON[:2]
    poisoned = [p[0] for p in poison]
    keys = _keys(N, 41)
    env = _env(model, N, bad=1e10)
    nets, norm, actor = _policy(env, 6)
    noise = torch.randn(T, N, env.action_size, device=DEV)
    # wrapped
    ew = wrappers.EvalWrapper(_fused(env, EP))
    assert ew.unroll_supported()
    actions = torch.empty(T, N, env.action_size, device=DEV)
    got = ew.unroll_policy(_poison(ew.reset(keys), poison), actor, noise, T, actions_out=actions)
    torch.cuda.synchronize()
    rule = RuleEnv(_env(model, N), 1e10)
    ew2 = wrappers.EvalWrapper(_composed(rule, EP))
    want = _poison(ew2.reset(keys), poison)
    partial = 0.0
    for t in range(T):
        want = ew2.step(want, actions[t])
        partial = max(partial, *(float(want.info["eval_metrics"]["episode_metrics"][k].abs().max()) for k in ("pos_reward", "reward")))
    assert torch.stack(rule.masks).any(0).nonzero().flatten().tolist() == poisoned and rule.count() == len(poisoned)
    ga, wa = got.info["eval_metrics"], want.info["eval_metrics"]
    assert torch.equal(ga["episode_steps"], wa["episode_steps"]) and torch.equal(ga["active_episodes"], wa["active_episodes"])
    assert bool((ga["episode_steps"][poisoned] == 1).all())                   # the bad step ends the episode: one active step
    bound = 2 * T * 2.0 ** -24 * max(1.0, partial)                            # the bound of tests/test_gpu_eval_unroll.py::_tol
    for k in ("reward_quadctrl", "reward_alive"):
        assert torch.equal(ga["episode_metrics"][k], wa["episode_metrics"][k]), k
    for k in ("pos_reward", "reward"):
        assert float((ga["episode_metrics"][k] - wa["episode_metrics"][k]).abs().max()) <= bound, k
        assert bool((ga["episode_metrics"][k][poisoned] == 0).all()), k      # the bad step added zeros
    for k in ("qpos", "qvel", "act", "qacc_warmstart"):
        assert torch.equal(getattr(got.pipeline_state, k), getattr(want.pipeline_state, k)), k
    assert torch.equal(got.obs, want.obs) and torch.equal(got.done, want.done)
    _assert_finite(got, "wrapped evaluation")
    assert bool(torch.isfinite(actions).all())
    assert env.bad_states() == rule.count()
    # raw: no restore -- flagged, counted, and left as it is
    env = _env(model, N, bad=1e10)
    st0 = _poison(env.reset(keys), POISON[:1])
    got = env.unroll_eval(st0, 4, actor, None)
    torch.cuda.synchronize()
    e = POISON[0][0]
    others = [i for i in range(N) if i != e]
    assert float(got.done[e]) == 1 and float(got.reward[e]) == 0
    assert bool(torch.isnan(got.pipeline_state.qpos[e]).any())               # the documented limit of the raw form
    assert bool(torch.isfinite(got.pipeline_state.qpos[others]).all())
    assert env.bad_states() == 4                                              # one event per env step of the bad env


# ---------------------------------------------------------------------------------------------- 5. check on, nothing bad
def _three_forms(make, N, T, EP, seed):
    """Final states of (T fused wrapped steps, one T-step launch, one T-step launch with the actor inside) on a fresh env each, and the
    envs (for their counters)."""
    from rodent_amd.training import acting
    keys = _keys(N, seed)
    out, envs_ = [], []
    env = make()
    acts = _actions(T, N, env.action_size, seed + 1)
    nets, norm, actor = _policy(env, seed + 2)
    noise = torch.randn(T, N, env.action_size, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed + 3))
    wenv = _fused(env, EP)
    st = wenv.reset(keys)
    for t in range(T):
        st = wenv.step(st, acts[t])
    out.append(st); envs_.append(env)
    env = make(); wenv = _fused(env, EP)
    out.append(wenv.unroll(wenv.reset(keys), acts)); envs_.append(env)
    env = make(); wenv = _fused(env, EP)
    buf = acting.UnrollBuffer(1, N, T, env.observation_size, env.action_size, torch.device(DEV))
    traj = dict(obs=buf.obs[0], raw_action=buf.raw_action[0], log_prob=buf.log_prob[0], reward=buf.reward[0], discount=buf.discount[0],
                truncation=buf.truncation[0])
    st, actions = wenv.unroll_policy(wenv.reset(keys), actor, noise, traj)
    out.append((st, buf, actions)); envs_.append(env)
    torch.cuda.synchronize()
    return out, envs_


def _mixed(model, n, bad):
    env = _env(model, n, bad=bad)
    fn = rs.system_fn(rs.mixed_fields)
    env.randomize(lambda sys: fn(sys, n))
    return env


@pytest.mark.parametrize("randomised", [False, True])
def test_check_on_and_nothing_bad_changes_nothing(randomised):
    N, T, EP = 16, 12, 7
    make = (lambda bad: _mixed("rodent_new", N, bad)) if randomised else (lambda bad: _env("rodent_optimized", N, bad=bad))
    on, envs_on = _three_forms(lambda: make(1e10), N, T, EP, 51)
    off, _ = _three_forms(lambda: make(None), N, T, EP, 51)
    _assert_same(on[0], off[0], "fused single steps")
    _assert_same(on[1], off[1], "one launch")
    _assert_same(on[2][0], off[2][0], "actor inside: state")
    assert torch.equal(on[2][2], off[2][2])
    for name in ("obs", "raw_action", "log_prob", "reward", "discount", "truncation"):
        assert torch.equal(getattr(on[2][1], name), getattr(off[2][1], name)), name
    assert float(on[1].info["truncation"].sum()) + float(on[2][1].truncation.sum()) > 0          # episodes did end in between
    assert [e.bad_states() for e in envs_on] == [0, 0, 0]


def test_graph_replay_carries_the_threshold():
    """The threshold is a by-value kernel argument: a captured graph of wrapped steps replays with it.  Once with nothing bad (equal to
    the check-off steps), once with a tightened threshold (equal to the host-issued steps of the same env, events counted)."""
    from rodent_amd.envs import graphed
    N, R, EP = 16, 3, 7
    keys = _keys(N, 61)
    acts = _actions(1 + R, N, 30, 62)
    s0 = torch.cuda.Stream(torch.device(DEV))

    def host(bad):
        with torch.cuda.stream(s0):
            env = _env("rodent_optimized", N, bad=bad)
            wenv = _fused(env, EP)
            st = wenv.reset(keys)
            peaks = []
            for t in range(1 + R):
                st = wenv.step(st, acts[t])
                peaks.append(st.pipeline_state.qvel.abs().amax(1))
        torch.cuda.synchronize()
        return env, st, torch.stack(peaks)

    def replayed(bad):
        with torch.cuda.stream(s0):
            env = _env("rodent_optimized", N, bad=bad)
            wenv = _fused(env, EP)
            st = wenv.reset(keys)
        cursor = torch.zeros((), dtype=torch.long, device=DEV)

        def step_fn(state):
            a = acts.index_select(0, cursor.reshape(1))[0]
            cursor.add_(1)
            return wenv.step(state, a)
        with torch.cuda.stream(s0):
            st1 = step_fn(st)
        torch.cuda.synchronize()
        g = graphed.GraphedSteps(step_fn, st1, R, s0)
        got = g.replay()
        torch.cuda.synchronize()
        assert int(cursor) == 1 + R
        return env, got
    _, want_off, peaks = host(None)
    env, got = replayed(1e10)
    _assert_same(got, want_off, "graph replay, nothing bad")
    assert env.bad_states() == 0
    thr, trippers = _threshold_between(peaks[1:].amax(0))                       # trips inside the replayed steps
    env_h, want, _ = host(thr)
    env, got = replayed(thr)
    _assert_same(got, want, "graph replay, tightened threshold")
    assert env.bad_states() == env_h.bad_states() > 0


# ---------------------------------------------------------------------------------------------- 6. rodent_cpu from the folded pose
def _folded_start(N, bad, oracle):
    from tests.test_gpu_unroll_self_collision import _folded_pose
    from rodent_amd import envs
    from rodent_amd.envs import wrappers
    folded, _ = _folded_pose(oracle)
    env = envs.get_environment("rodent", track_pos=util.synthetic_track(), num_envs=N, xml_path="rodent_cpu.xml", iterations=6, ls_iterations=6,
                               device=DEV, healthy_z_range=(-10.0, 10.0), bad_state_max=bad)
    pose = torch.tensor(np.tile(folded.astype(np.float32), (N, 1)), device=DEV)
    real_reset = env.reset

    def folded_reset(rng):
        # the folded pose as the current AND (through the wrappers' reset) the stored first state: the envs fold again after each restore
        st = real_reset(rng)
        return st.replace(pipeline_state=st.pipeline_state.replace(qpos=pose.clone(), qvel=torch.zeros_like(st.pipeline_state.qvel)))
    env.reset = folded_reset
    return env, wrappers.wrap(env, episode_length=9, action_repeat=1)


def test_folded_rodent_cpu_is_ended_and_restored(oracle_built):
    N, T = 16, 12
    keys = _keys(N, 71)
    acts = _actions(T, N, 38, 72)
    acts[:, N // 2:] = 0                                                       # half of the envs are left alone, half are driven
    env_off, wenv = _folded_start(N, None, oracle_built)
    off = wenv.unroll(wenv.reset(keys), acts)
    env_on, wenv = _folded_start(N, 1e10, oracle_built)
    on = wenv.unroll(wenv.reset(keys), acts)
    torch.cuda.synchronize()
    nonfinite = (~torch.isfinite(off.pipeline_state.qpos).all(1)) | (~torch.isfinite(off.pipeline_state.qvel).all(1))
    print(f"check off: {int(nonfinite.sum())} of {N} envs non-finite after {T} steps; check on: {env_on.bad_states()} events, "
          f"contact overflow {env_on.contact_overflow()} (off: {env_off.contact_overflow()})")
    assert int(nonfinite.sum()) > 0                                            # the input bites
    _assert_finite(on, "check on")
    assert env_on.bad_states() > 0 and env_off.bad_states() == 0
    assert env_on.contact_overflow() > 0


def test_ppo_train_survives_the_folded_start(oracle_built):
    from rodent_amd.training.agents.ppo import train as ppo
    N = 64
    env, _ = _folded_start(N, 1e10, oracle_built)
    log = []
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        _, params, _ = ppo.train(environment=env, num_timesteps=10 ** 9, episode_length=9, num_envs=N, batch_size=N, num_minibatches=4, unroll_length=5,
                                 num_updates_per_batch=2, num_evals=2, num_eval_envs=0, learning_rate=5e-5, entropy_cost=1e-3, discounting=0.97,
                                 normalize_observations=True, seed=1, max_training_steps=2, progress_fn=lambda n, m: log.append(m))
    norm, policy = params[0], params[1]
    assert all(bool(torch.isfinite(p).all()) for p in policy.parameters())
    assert bool(torch.isfinite(norm.mean).all()) and bool(torch.isfinite(norm.std).all())
    assert math.isfinite(float(log[-1]["training/total_loss"]))
    assert log[-1]["training/bad_state_resets"] > 0 and env.bad_states() >= log[-1]["training/bad_state_resets"]
    assert sum("bad_state_max" in str(w.message) for w in caught) == 1
