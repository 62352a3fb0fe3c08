"""Pose termination on the GPU (`Rodent(max_pos_error=, max_quat_error=, max_joint_error=)`; rr_batch_set_pose_termination, the
rr_poseterm_kernel instances): the code against the float64 restatements `rodent.pose_errors` / `rodent.pose_fail_code`, and everything
else of the step against a pose env of the same build, bit for bit.

Fixture: that of tests/test_gpu_pose.py (12 envs on 3 clips, n_frames 2, CG 4/4, five steps; rodent_optimized and rodent_0; T = 104 and
T = 3), from tests/pose_fixture.py.

THRESHOLDS come from the data, not from the code under test: the existing pose env (no termination) makes five bare steps, `pose_errors`
gives the 60 (env, step) errors per criterion from the returned qpos, and each threshold stands in the middle of the widest gap between
sorted ranks 15 and 45 -- so each criterion fires in 25 % .. 75 % of the pairs.  The comparison `error > threshold` is decided in
float32 on the device and in float64 here; the two agree wherever the error is further from the threshold than its float32 error, and the
tests ASSERT, for every pair they check, that none lies within 100 x that bound (`_margin_ok`).

Float32 bounds (eps = 2^-24, factor 2 for the slack of a first-order count, as tests/test_gpu_pose.py):
  e_pos   = sqrt(dx^2 + dy^2 + dz^2): a difference (eps), its square (2 eps + eps), two additions of positive terms (2 eps): 5 eps on the
            sum, which the root halves, and sqrtf within 1 ulp = 2 eps: 4.5 eps -> 2 x 5 eps x e_pos.
  e_quat  = theta: (22 + 4 theta) eps absolute, derived in tests/test_gpu_pose.py::test_against_the_formula -> 2 x (22 + 4 theta) eps.
  e_joint = sqrt(S), S a sum of nq - 7 squares: a difference (eps), its square (3 eps), at most one addition inside a lane and the six of
            the wave sum (7 eps): 10 eps on S, halved by the root, plus sqrtf's 2 eps: 7 eps -> 2 x 7 eps x e_joint."""
import math

import numpy as np
import pytest
import torch

from rodent_amd import jax_random
from rodent_amd.envs import rodent
from tests import pose_fixture as F
from tests.pose_fixture import C, DEV, EPS, FAIL_METRICS, IDS, N, STEPS

pytestmark = pytest.mark.gpu
CASES = [(m, T) for m in F.MODELS for T in (104, 3)]
POSE_METRICS = F.OLD_METRICS + ("quat_reward", "joint_reward")           # the five metrics a pose env has
INF = math.inf


# ---------------------------------------------------------------------------------------------- the reference side
def _margin_ok(e, thr, which=(0, 1, 2)):
    """No error of the criteria `which` lies within 100 float32 bounds of its threshold."""
    b = F.term_bound(e)
    return all(bool((np.abs(e[k] - thr[k]) > 100 * b[k]).all()) for k in which if math.isfinite(thr[k]))


def _term_env(model, T, thr, **kw):
    env = F.make(model, T, max_pos_error=None if math.isinf(thr[0]) else thr[0], max_quat_error=None if math.isinf(thr[1]) else thr[1],
                  max_joint_error=None if math.isinf(thr[2]) else thr[2], **kw)
    got = env.pose_termination
    assert got is not None and all(a == float(np.float32(b)) for a, b in zip(got, thr))       # what the kernel compares with
    return env


def _assert_equal_trees(a, b, what):
    la, lb = F.leaves(a), F.leaves(b)
    assert len(la) == len(lb) >= 1, what
    for i, (x, y) in enumerate(zip(la, lb)):
        assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), (what, i, int((x != y).sum()))


def _assert_same_but_done(got, want, what):
    """Everything of the two states except `done` and the four new metrics, which only `got` has: bit for bit."""
    assert set(got.metrics) - set(want.metrics) == set(FAIL_METRICS), what
    for name, a, b in (("pipeline_state", got.pipeline_state, want.pipeline_state), ("obs", got.obs, want.obs), ("reward", got.reward, want.reward),
                       ("info", got.info, want.info), ("metrics", {k: got.metrics[k] for k in POSE_METRICS}, {k: want.metrics[k] for k in POSE_METRICS})):
        _assert_equal_trees(a, b, (what, name))


# ---------------------------------------------------------------------------------------------- 0. the fixture's own condition
@pytest.mark.parametrize("model,T", CASES)
def test_the_thresholds_stand_clear_of_every_error(model, T):
    _, _, errs, thr = F.term_reference(model, T)
    e = errs.transpose(1, 0, 2).reshape(3, -1)
    for k, name in enumerate(("e_pos", "e_quat", "e_joint")):
        fires = int((e[k] > thr[k]).sum())
        nearest = float(np.abs(e[k] - thr[k]).min())
        print(f"{model} T={T}: {name} in [{e[k].min():.4g}, {e[k].max():.4g}], threshold {thr[k]:.6g}, fires in {fires} of 60, nearest error "
              f"{nearest:.3g} away = {nearest / float(F.term_bound(e)[k].max()):.0f} float32 bounds")
        assert 15 <= fires <= 45
    assert _margin_ok(e, thr)


# ---------------------------------------------------------------------------------------------- 1. bare steps
@pytest.mark.parametrize("which", ["all", "pos", "quat", "joint"])
@pytest.mark.parametrize("model,T", CASES)
def test_bare_steps_raise_done_and_nothing_else(model, T, which):
    """Five bare steps with all three thresholds, and with each alone (the other two off: only its bit appears): the code is
    `pose_fail_code` of the float64 errors for all 60 pairs, done = max(the pose env's done, code != 0), and the rest of the state is
    the pose env's in every bit."""
    _, want, errs, thr = F.term_reference(model, T)
    assert _margin_ok(errs.transpose(1, 0, 2).reshape(3, -1), thr)
    on = {"all": (0, 1, 2), "pos": (0,), "quat": (1,), "joint": (2,)}[which]
    use = tuple(thr[k] if k in on else INF for k in range(3))
    env = _term_env(model, T, use)
    assert env.pose_tracking and not env.eval_supported()
    acts, _ = F.draws(env, STEPS, 1)
    got = F.steps(env, acts)
    assert all(float(got[0].metrics[k].abs().max()) == 0.0 for k in FAIL_METRICS)       # zeros at reset
    _assert_same_but_done(got[0], want[0], (model, T, which, 0))
    assert torch.equal(got[0].done, want[0].done)
    seen = set()
    for t in range(1, STEPS + 1):
        _assert_same_but_done(got[t], want[t], (model, T, which, t))
        code = rodent.pose_fail_code(errs[t - 1], env.pose_termination)
        assert np.array_equal(F.code_of(got[t]), code), (model, T, which, t, F.code_of(got[t]), code)
        assert np.array_equal(got[t].done.cpu().numpy(), np.maximum(want[t].done.cpu().numpy(), (code != 0).astype(np.float32))), (model, T, which, t)
        seen |= set(code.tolist())
    allowed = set(range(8)) if which == "all" else {0, 1 << on[0]}
    assert seen <= allowed and 0 in seen and len(seen) >= 2, (which, seen)           # fired and stayed quiet; only the criteria that are on
    if which == "all":
        assert {c & 1 for c in seen} == {0, 1} and {c & 2 for c in seen} == {0, 2} and {c & 4 for c in seen} == {0, 4}, seen


# ---------------------------------------------------------------------------------------------- 2. off / next to the reference observation
@pytest.mark.parametrize("model,T", CASES)
def test_all_thresholds_none_is_the_pose_env(model, T):
    _, want, _, _ = F.term_reference(model, T)
    env = F.make(model, T, max_pos_error=None, max_quat_error=None, max_joint_error=INF)
    assert env.pose_termination is None
    acts, _ = F.draws(env, STEPS, 1)
    got = F.steps(env, acts)
    assert env._batch._pterm is None and env._batch._pose is not None           # no termination block on the batch: its launches pick the pose instances
    for t, (g, w) in enumerate(zip(got, want)):
        assert set(g.metrics) == set(w.metrics)
        _assert_equal_trees(g, w, (model, T, t))


@pytest.mark.parametrize("model,T", CASES)
def test_one_threshold_next_to_five_reference_frames(model, T):
    """H = 5 with one finite threshold: the whole row, reference blocks included, is the reference-observation env's in every bit -- at
    reset (served by the instance a reset runs without the block) and after every step -- and the code is the restatement's."""
    _, _, errs, thr = F.term_reference(model, T)
    ref_env = F.make(model, T, reference_obs_frames=5)
    env = _term_env(model, T, (INF, INF, thr[2]), reference_obs_frames=5)
    assert env.observation_size == env.sys.obs_dim + 5 * env.sys.nq
    acts, _ = F.draws(env, STEPS, 1)
    got, want = F.steps(env, acts), F.steps(ref_env, acts)
    for t in range(STEPS + 1):
        _assert_same_but_done(got[t], want[t], (model, T, t))
        assert got[t].obs.shape == (N, env.observation_size)
        if t:
            assert np.array_equal(F.code_of(got[t]), rodent.pose_fail_code(errs[t - 1], env.pose_termination)), (model, T, t)


# ---------------------------------------------------------------------------------------------- 3. wrapped forms
class _Recorder:
    """Sits between EpisodeWrapper and AutoResetWrapper and keeps what the episode step returned: the stepped state before the restore."""

    def __init__(self, env):
        self.env, self.seen = env, []

    def __getattr__(self, name):
        return getattr(self.env, name)

    def reset(self, rng, **kw):
        return self.env.reset(rng, **kw)

    def step(self, state, action):
        before = state.info["cur_frame"]
        out = self.env.step(state, action)
        self.seen.append((before, out.pipeline_state.qpos, out.done.clone(), out.info["truncation"].clone(), out.info["steps"].clone()))
        return out


@pytest.mark.parametrize("model,T", CASES)
def test_wrapped_forms_terminate_and_restore(model, T):
    """Episode(4) + AutoReset, six steps, `max_quat_error` alone (its gaps come from the clips' 0.1 rad spacing and survive the restores;
    the margin condition is asserted on this walk too).  The composed wrappers, driven step by step with the stepped qpos recorded before
    the restore, against the float64 code; the fused per-step wrapper and `unroll_wrapped` against the composition, bit for bit."""
    from rodent_amd.envs import wrappers
    _, _, _, thr = F.term_reference(model, T)
    env = _term_env(model, T, (INF, thr[1], INF))
    use = env.pose_termination
    acts, _ = F.draws(env, 6, 2)
    rec = _Recorder(wrappers.EpisodeWrapper(wrappers.VmapWrapper(env), 4, 1))
    comp = wrappers.AutoResetWrapper(rec)
    s = comp.reset(F.keys(), clip=IDS)
    first = s
    walk = [s]
    steps = np.zeros(N, np.float32)
    prev_done = np.zeros(N, np.float32)
    failed = ran_out = 0
    z_min, z_max = np.float32(0.03), np.float32(0.5)
    for t in range(6):
        s = comp.step(s, acts[t])
        walk.append(s.replace(info=dict(s.info)))           # (AutoReset's next step edits the incoming info dict in place)
        torch.cuda.synchronize()
        before, qpos, done, trunc, nsteps = rec.seen[-1]
        e = F.term_errors(env, T, qpos, before)
        assert _margin_ok(e, use), (model, T, t, e[1], use[1])
        code = rodent.pose_fail_code(e, use)
        assert set(code.tolist()) <= {0, 2}
        assert np.array_equal(F.code_of(s), code), (model, T, t)
        z = qpos[:, 2].cpu().numpy()
        own = ((z < z_min) | (z > z_max)).astype(np.float32)                          # the env's own done (terminate_when_unhealthy)
        done_env = np.maximum(own, (code != 0).astype(np.float32))
        steps = np.where(prev_done != 0, 0.0, steps).astype(np.float32) + 1
        over = steps >= 4
        want_done, want_trunc = np.where(over, 1.0, done_env).astype(np.float32), np.where(over, 1.0 - done_env, 0.0).astype(np.float32)
        assert np.array_equal(done.cpu().numpy(), want_done) and np.array_equal(trunc.cpu().numpy(), want_trunc) and np.array_equal(nsteps.cpu().numpy(), steps)
        assert np.array_equal(s.done.cpu().numpy(), want_done) and np.array_equal(s.info["truncation"].cpu().numpy(), want_trunc)
        prev_done = want_done
        clip_ended = torch.from_numpy((code != 0) & (own == 0)).to(DEV)              # ended by the clip alone
        only_over = torch.from_numpy(over & (done_env == 0)).to(DEV)
        if bool(clip_ended.any()):
            assert float(s.info["truncation"][clip_ended].max()) == 0.0 and float(s.done[clip_ended].min()) == 1.0
            for a, b in ((s.pipeline_state.qpos, first.pipeline_state.qpos), (s.pipeline_state.qvel, first.pipeline_state.qvel), (s.obs, first.obs)):
                assert torch.equal(a[clip_ended], b[clip_ended])
            assert s.obs.shape[1] == env.observation_size
            assert not torch.equal(qpos[clip_ended], first.pipeline_state.qpos[clip_ended])      # ... and the stepped state was another one
        if bool(only_over.any()):
            assert float(s.info["truncation"][only_over].min()) == 1.0 and float(s.metrics["pose_fail"][only_over].max()) == 0.0
        failed += int(clip_ended.sum())
        ran_out += int(only_over.sum())
    print(f"{model} T={T}: threshold {use[1]:.6g}: {failed} (env, step) pairs ended by the clip, {ran_out} by the episode length")
    assert failed >= 1 and ran_out >= 1
    fused = wrappers.wrap(env, episode_length=4, action_repeat=1)
    assert isinstance(fused, wrappers.FusedEpisodeAutoResetWrapper)
    f = fused.reset(F.keys(), clip=IDS)
    for t in range(6):
        f = fused.step(f, acts[t])
        for name in ("pipeline_state", "obs", "reward", "done", "metrics"):
            _assert_equal_trees(getattr(f, name), getattr(walk[t + 1], name), (model, T, "fused step", t, name))
        for k in ("cur_frame", "steps", "truncation"):
            assert torch.equal(f.info[k], walk[t + 1].info[k]), (model, T, "fused step", t, k)
    u = fused.unroll(fused.reset(F.keys(), clip=IDS), acts)
    torch.cuda.synchronize()
    for name in ("pipeline_state", "obs", "reward", "done", "metrics"):
        _assert_equal_trees(getattr(u, name), getattr(walk[-1], name), (model, T, "unroll", name))
    for k in ("cur_frame", "steps", "truncation"):
        assert torch.equal(u.info[k], walk[-1].info[k]), (model, T, "unroll", k)


# ---------------------------------------------------------------------------------------------- 4. the actor inside
@pytest.mark.parametrize("model,T", CASES)
def test_the_actor_inside_terminates_like_the_replay(model, T):
    """rr_env_unroll_policy on the pose-termination instance, six steps recorded as two segments of three, episodes of four steps,
    `terminate_when_unhealthy=False` -- so a done that is no truncation can only stem from the clip.  Replaying the returned actions
    through wrapped single steps reproduces traj.obs, traj.discount and traj.truncation bit for bit and traj.reward within the one ulp
    tests/test_gpu_ppo.py allows the actor instance."""
    from rodent_amd.envs import wrappers
    from rodent_amd.training import acting
    _, _, _, thr = F.term_reference(model, T)
    env = _term_env(model, T, (INF, thr[1], INF), terminate_when_unhealthy=False)
    Wd, A = env.observation_size, env.action_size
    actor = F.actor(env, 7)
    wenv = wrappers.wrap(env, episode_length=4, action_repeat=1)
    assert env._batch.pose_termination_supported(with_actor=True) is None
    _, noise = F.draws(env, 6, 3)
    buf = acting.UnrollBuffer(2, N, 3, Wd, A, torch.device(DEV))
    traj = dict(obs=buf.obs, raw_action=buf.raw_action, log_prob=buf.log_prob, reward=buf.reward, discount=buf.discount, truncation=buf.truncation)
    got, actions = wenv.unroll_policy(wenv.reset(F.keys(), clip=IDS), actor, noise, traj, segment=3)
    torch.cuda.synchronize()
    assert torch.isfinite(buf.obs).all() and torch.isfinite(buf.reward).all()
    st = wenv.reset(F.keys(), clip=IDS)
    by_clip = 0
    worst = 0.0
    for s in range(6):
        u, t = s // 3, s % 3
        assert torch.equal(buf.obs[u, :, t], st.obs), (model, T, s)
        st = wenv.step(st, actions[s])
        assert torch.equal(buf.obs[u, :, t + 1], st.obs), (model, T, s)
        assert torch.equal(buf.discount[u, :, t], 1.0 - st.done), (model, T, s)
        assert torch.equal(buf.truncation[u, :, t], st.info["truncation"]), (model, T, s)
        worst = max(worst, float((buf.reward[u, :, t] - st.reward).abs().max()))
        ended = (buf.discount[u, :, t] == 0) & (buf.truncation[u, :, t] == 0)
        assert torch.equal(ended, (st.metrics["pose_fail"] != 0) & (st.info["truncation"] == 0)), (model, T, s)
        assert torch.equal(st.metrics["pose_fail"], st.metrics["pose_fail_quat"])
        by_clip += int(ended.sum())
    print(f"{model} T={T}: {by_clip} (env, step) pairs ended by the clip inside the launch; max |traj.reward - replay| = {worst:.3g}")
    assert worst <= F.ACTOR_REWARD_TOL
    assert by_clip >= 1
    _assert_equal_trees(got.pipeline_state, st.pipeline_state, (model, T, "final state"))
    assert torch.equal(got.obs, st.obs) and torch.equal(got.done, st.done) and torch.equal(got.info["steps"], st.info["steps"])
    for k in FAIL_METRICS:
        assert torch.equal(got.metrics[k], st.metrics[k]), k


# ---------------------------------------------------------------------------------------------- 5. bad state
@pytest.mark.parametrize("model", F.MODELS)
def test_a_bad_step_is_done_with_code_zero(model):
    from rodent_amd.envs import wrappers
    from rodent_amd.training import acting
    _, _, _, thr = F.term_reference(model, 104)
    env = _term_env(model, 104, thr, bad_state_max=1e10)
    bad = 4

    def poison(state):       # NaN into a COPY of the incoming qvel (the stored first state shares the reset's tensors)
        qvel = state.pipeline_state.qvel.clone()
        qvel[bad, 3] = float("nan")
        return state.replace(pipeline_state=state.pipeline_state.replace(qvel=qvel))
    acts, noise = F.draws(env, 1, 3)
    wenv = wrappers.wrap(env, episode_length=100, action_repeat=1)
    buf = acting.UnrollBuffer(1, N, 1, env.observation_size, env.action_size, torch.device(DEV))
    res = dict(step=env.step(poison(env.reset(F.keys(), clip=IDS)), acts[0]), unroll=wenv.unroll(poison(wenv.reset(F.keys(), clip=IDS)), acts),
               policy=wenv.unroll_policy(poison(wenv.reset(F.keys(), clip=IDS)), F.actor(env, 5), noise, F.traj(buf))[0])
    torch.cuda.synchronize()
    for k, s in res.items():
        assert float(s.done[bad]) == 1.0 and float(s.reward[bad]) == 0.0, (model, k)
        for name in FAIL_METRICS:
            assert float(s.metrics[name][bad]) == 0.0, (model, k, name)
        code = F.code_of(s)
        assert code[bad] == 0 and bool((s.done.cpu().numpy()[code != 0] == 1.0).all()), (model, k)          # the others: ended where their code says so
    assert float(buf.discount[0, bad, 0]) == 0.0 and float(buf.truncation[0, bad, 0]) == 0.0
    assert env.bad_states() == 3


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_refusals():
    from rodent_amd import envs
    track = F.tracks(104)[0]

    def build(model, pose=True, **kw):
        q0 = F.qpos0(model)
        if pose:
            kw.update(track_quat=np.tile([1.0, 0.0, 0.0, 0.0], (104, 1)), track_joints=np.tile(q0[7:], (104, 1)))
        return envs.get_environment("rodent", track_pos=track, num_envs=4, xml_path=f"{model}.xml", iterations=4, ls_iterations=4, n_frames=2,
                                    device=DEV, **kw)
    with pytest.raises(RuntimeError, match="candidate-pair contacts"):
        build("rodent_cpu", healthy_z_range=(-0.3, 0.3), max_quat_error=0.5)
    with pytest.raises(RuntimeError, match="Newton solver"):
        build("rodent_optimized", solver="newton", max_pos_error=0.1)
    with pytest.raises(ValueError, match="track_quat and track_joints"):
        build("rodent_optimized", pose=False, max_joint_error=1.0)
    with pytest.raises(ValueError, match="max_quat_error must be > 0"):
        build("rodent_optimized", max_quat_error=0.0)
    with pytest.raises(ValueError, match="max_pos_error must be > 0"):
        build("rodent_optimized", max_pos_error=float("nan"))
    env = build("rodent_optimized", max_pos_error=0.5, max_quat_error=1.0)
    assert env.pose_termination == (0.5, 1.0, INF) and env.with_num_envs(2).pose_termination == (0.5, 1.0, INF)
    with pytest.raises(RuntimeError, match="per-env parameters"):
        env.set_env_params(dof_f=torch.zeros(4, env.sys.nv, 16, device=DEV))
    with pytest.raises(RuntimeError, match="per-env parameters"):
        env.randomize(lambda sys: (sys.replace(dof_damping=np.repeat(sys.dof_damping[None], 4, axis=0)), {"dof_damping": 0}))
    keys = jax_random.split(jax_random.PRNGKey(1), 4)
    st = env.step(env.reset(keys), torch.zeros(4, env.action_size, device=DEV))            # still a working env
    assert float(st.metrics["quat_reward"].min()) > 0 and float(st.metrics["pose_fail"].max()) == 0.0
    b = env._batch
    with pytest.raises(RuntimeError, match="clear it first"):             # the pose block cannot go while the termination block stands
        b.set_pose(None)
    fail = torch.zeros(4, device=DEV)
    for bad in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, float("nan"))):
        with pytest.raises(RuntimeError, match="thresholds must be > 0"):
            b.set_pose_termination(fail, bad)
    b.set_pose_termination(None)
    b.set_pose(None)
    with pytest.raises(RuntimeError, match="needs a pose block"):
        b.set_pose_termination(fail, (1.0, 1.0, 1.0))
    st = env.step(env.reset(keys), torch.zeros(4, env.action_size, device=DEV))            # the env-io dict sets both blocks again
    assert float(st.metrics["pose_fail"].max()) == 0.0 and b._pterm is not None
    with pytest.raises(RuntimeError, match="no evaluation instance"):
        env.unroll_eval(env.reset(keys), 2, F.actor(env, 1))


# ---------------------------------------------------------------------------------------------- 7. training
def test_ppo_train_with_pose_termination(monkeypatch):
    """One training step at 64 envs through the one-launch rollout (rr_env_unroll_policy on the pose-termination instance with the
    actor), evaluations by the per-step loop: finite losses, and eval/episode_pose_fail -- the share of evaluation episodes the clip
    ended -- finite and in [0, 1]."""
    from rodent_amd.training import acting
    from rodent_amd.training.agents.ppo import train as ppo
    _, _, _, thr = F.term_reference("rodent_optimized", 104)
    env = _term_env("rodent_optimized", 104, (INF, thr[1], INF), n=64)
    calls, log = {"fused": 0}, []
    real_fused = acting.generate_unrolls_fused
    monkeypatch.setattr(acting, "generate_unrolls_fused", lambda *a, **k: (calls.__setitem__("fused", calls["fused"] + 1), real_fused(*a, **k))[1])
    ppo.train(environment=env, num_timesteps=10 ** 9, episode_length=10, num_envs=64, batch_size=64, num_minibatches=2, unroll_length=5,
              num_updates_per_batch=2, num_evals=2, num_eval_envs=6, learning_rate=5e-5, entropy_cost=1e-3, discounting=0.97,
              normalize_observations=True, seed=3, max_training_steps=1, progress_fn=lambda n, m: log.append(m))
    assert calls["fused"] == 1
    assert math.isfinite(float(log[-1]["training/total_loss"]))
    evals = [m for m in log if "eval/episode_reward" in m]
    assert len(evals) >= 2
    for m in evals:
        for k in ("eval/episode_reward", "eval/episode_quat_reward", "eval/episode_pose_fail", "eval/episode_pose_fail_quat"):
            assert k in m and math.isfinite(float(m[k])), k
        assert 0.0 <= float(m["eval/episode_pose_fail"]) <= 1.0
        assert float(m["eval/episode_pose_fail_pos"]) == 0.0 and float(m["eval/episode_pose_fail_joint"]) == 0.0
