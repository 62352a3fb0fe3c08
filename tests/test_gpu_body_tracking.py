"""Body tracking on the GPU (`Rodent(track_bodies=, body_ids=, end_effector_ids=)`; rr_batch_set_body_tracking / rr_body_io, the
rr_body_kernel instances): the reward's body-position and end-effector terms against a pose env of the same build -- bit for bit where
nothing but the reward may move -- and against the float64 restatement `rodent.body_rewards` of the step's own returned xpos.

Fixture: that of tests/test_gpu_pose.py, from tests/pose_fixture.py (12 envs on 3 clips, n_frames 2, CG 4/4, five steps; T = 104 and
T = 3), on rodent_optimized, rodent_new (nbody 67: three bodies on the lanes' second pass, under the root-slot map) and rodent_0 (the
generic dims).  Reference bodies: `preprocessing.extract_features` of the pose (track position, qpos0[3:]) at every frame of every clip,
plus AMP sin(0.9 b + 1.7 k + 0.05 t + c) per body b, axis k, frame t and clip c, so every entry differs.  B = all bodies, E = foot_L,
foot_R, hand_L, hand_R, skull (ids 11, 15, 59, 64, 54; one higher on rodent_new), which puts body 64 / 65 -- a lane's second body -- in
E.  Weights 0.6 / 0.4 (not the defaults).

AMP and the two scales were chosen from the POSE env's own `pipeline_state.xpos` on this fixture (the build without the body block,
`pipeline_outputs=True`), not from the code under test, so that both exponents k S lie in [0.051, 3.0] = [-log 0.95, -log 0.05] for all
60 (env, step) pairs of every case; `test_against_the_formula` asserts that on the float64 restatement.  Measured on that env, over the
three models: without the sine term S_B lies in [0.00096, 0.0386] and S_E in [0.00004, 0.0024] -- a spread of 40 and 60, and exponents
below 0.051 at any scale that keeps the largest below 3 with a margin -- so the term carries the sums: with AMP = 0.03, S_B in
[0.0888, 0.1253] (T = 104) and [0.0905, 0.1094] (T = 3), S_E in [0.00544, 0.01023] and [0.00562, 0.01057]; with body_reward_scale 8 and
endeff_reward_scale 100 (the defaults) the exponents lie in [0.71, 1.00] / [0.72, 0.88] and [0.54, 1.02] / [0.56, 1.06].  (AMP 0.02
gives [0.32, 0.62] and [0.24, 0.63], AMP 0.04 [1.25, 1.55] and [0.96, 1.64]: the choice is not tight.)  The body env's own xpos is
bit-equal to the pose env's (`test_state_is_untouched_by_plain_steps`), so the test sees these ranges.

Float32 bound of a term w exp(-k S), eps = 2^-24, factor 2 for the slack of a first-order count (as tests/test_gpu_pose.py).  Per body:
three differences (eps each on its d), three squares (2 eps + eps), two sums of positive terms (2 eps), the product with the 0 / 1 mask
(counted, eps): 6 eps on the body's term.  A lane accumulates at most A = ceil(nbody / 64) terms (A eps), the wave sum has six levels
(6 eps; all terms positive, so relative errors do not grow): (12 + A) eps on S; the product with the scale one more: (13 + A) eps x
on the exponent x = k S, which exp turns into a relative error of the result; expf within 2 ulp = 4 eps, the product with the weight
eps: 2 ((13 + A) x + 5) eps, relative."""
import functools
import math

import numpy as np
import pytest
import torch

from rodent_amd import jax_random
from rodent_amd.envs import rodent
from tests import pose_fixture as F
from tests.pose_fixture import BW, C, DEV, EFF, EPS, IDS, N, SCALES, STEPS

pytestmark = pytest.mark.gpu
MODELS = ["rodent_optimized", "rodent_new", "rodent_0"]
CASES = [(m, T) for m in MODELS for T in (104, 3)]
POSE_METRICS = F.OLD_METRICS + ("quat_reward", "joint_reward")
BODY_METRICS = ("body_reward", "endeff_reward")


# ---------------------------------------------------------------------------------------------- the fixture
@functools.lru_cache(maxsize=None)
def _body_steps(model, T):
    """Computed once per (model, T) and shared: (the body env, pipeline outputs on; its states of five bare steps on the same keys, clips
    and actions as `F.pose_ref`)."""
    env = F.make_body(model, T, pipeline_outputs=True)
    return env, F.steps(env, F.draws(env, STEPS, 1)[0])


@functools.lru_cache(maxsize=None)
def _forms(model, T):
    """Computed once per (model, T) and shared: the wrapped forms (tests/test_gpu_pose.py: seven steps, episodes of three) of the body env
    and of the pose env, same keys, clips, actions, noise and actor."""
    env = F.make_body(model, T)
    assert env._batch.unroll_supported(False) and env._batch.unroll_supported(True)
    acts, noise = F.draws(env, 7, 2)
    return F.wrapped_forms(env, acts, noise, F.actor(env, 7)), F.forms(model, T)[0]


def _assert_same(got, want, what, metrics=POSE_METRICS, reward=False):
    """Everything of the two states except `reward` (unless asked) and the metrics only `got` has: pipeline state, obs, done, info and
    `metrics`, bit for bit."""
    assert set(got.metrics) - set(want.metrics) == set(BODY_METRICS) and set(metrics) <= set(want.metrics), what
    pairs = [("pipeline_state", got.pipeline_state, want.pipeline_state), ("obs", got.obs, want.obs), ("done", got.done, want.done),
             ("info", got.info, want.info), ("metrics", {k: got.metrics[k] for k in metrics}, {k: want.metrics[k] for k in metrics})]
    if reward:
        pairs.append(("reward", got.reward, want.reward))
    for name, a, b in pairs:
        la, lb = F.leaves(a), F.leaves(b)
        assert len(la) == len(lb) >= 1, (what, name)
        for i, (x, y) in enumerate(zip(la, lb)):
            assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), (what, name, i, int((x != y).sum()))


def _composed(pose_reward, state):
    """f32(f32(pose env's reward + body_reward) + endeff_reward) in numpy float32 arithmetic."""
    return (F.f32(pose_reward) + F.f32(state.metrics["body_reward"])) + F.f32(state.metrics["endeff_reward"])


# ---------------------------------------------------------------------------------------------- 1. nothing else moves
@pytest.mark.parametrize("model,T", CASES)
def test_state_is_untouched_by_plain_steps(model, T):
    env, got = _body_steps(model, T)
    _, want = F.pose_ref(model, T)
    bt = env.body_tracking
    assert bt is not None and bt["body_ids"] == tuple(range(1, env.sys.nbody)) and bt["end_effector_ids"] == EFF[model] and not env.eval_supported()
    assert bt["body_reward"] == (BW[0], SCALES[0]) and bt["endeff_reward"] == (BW[1], SCALES[1])
    assert all(float(got[0].metrics[k].abs().max()) == 0.0 for k in BODY_METRICS)       # zeros at reset
    _assert_same(got[0], want[0], (model, T, "reset"), reward=True)
    for t in range(1, STEPS + 1):
        _assert_same(got[t], want[t], (model, T, t))
        assert not torch.equal(got[t].reward, want[t].reward)
    sib = env.with_num_envs(4)
    assert sib.body_tracking == bt and sib.num_envs == 4


@pytest.mark.parametrize("model,T", CASES)
def test_state_is_untouched_by_the_multi_step_forms(model, T):
    got, want = _forms(model, T)
    for k in ("steps", "unroll", "policy"):
        _assert_same(got[k], want[k], (model, T, k))
    assert torch.equal(got["policy_actions"], want["policy_actions"])
    for name in ("obs", "raw_action", "log_prob", "discount", "truncation"):            # everything but traj.reward
        assert torch.equal(getattr(got["buf"], name), getattr(want["buf"], name)), (model, T, name)
    assert float(got["unroll"].info["steps"].max()) <= 3 and bool((got["buf"].discount == 0).any())       # episodes ended: restores ran
    assert not torch.equal(got["buf"].reward, want["buf"].reward)


# ---------------------------------------------------------------------------------------------- 2. composition
@pytest.mark.parametrize("model,T", CASES)
def test_reward_is_the_pose_reward_plus_body_plus_endeff(model, T):
    """reward == f32(f32(pose env's reward + body_reward) + endeff_reward), from the env's own metrics: bit for bit in `step` and
    `unroll`; in the actor form (last step of the launch, whose metrics the state carries) within the one ulp tests/test_gpu_ppo.py
    allows that instance's reward."""
    _, got = _body_steps(model, T)
    _, want = F.pose_ref(model, T)
    for t in range(1, STEPS + 1):
        assert np.array_equal(F.f32(got[t].reward), _composed(want[t].reward, got[t])), (model, T, t)
        assert float(got[t].metrics["body_reward"].min()) > 0 and float(got[t].metrics["endeff_reward"].min()) > 0
    fg, fw = _forms(model, T)
    for k in ("steps", "unroll"):
        assert np.array_equal(F.f32(fg[k].reward), _composed(fw[k].reward, fg[k])), (model, T, k)
    last = np.abs(F.f32(fg["buf"].reward[0, :, -1]).astype(np.float64) - _composed(fw["buf"].reward[0, :, -1], fg["policy"]).astype(np.float64))
    print(f"{model} T={T}: actor form, last step: max |traj.reward - composed| = {last.max():.3g}")
    assert last.max() <= F.ACTOR_REWARD_TOL
    assert np.array_equal(F.f32(fg["policy"].reward), F.f32(fg["buf"].reward[0, :, -1]))       # t_reward receives the total the state carries


# ---------------------------------------------------------------------------------------------- 3. formula
def _bound(want, weight, nbody):
    """Float32 error bound of a term around its float64 value `want` (module docstring)."""
    x = -np.log(want / weight)
    return 2 * ((13 + math.ceil(nbody / 64)) * x + 5) * EPS * want


@pytest.mark.parametrize("model,T", CASES)
def test_against_the_formula(model, T):
    """The two metrics against `body_rewards` in float64 on the step's own returned float32 xpos (whose parity the parity tests hold)
    and the float32 rows the device holds, within the bound of the module docstring.  Both exponents must lie in [0.051, 3.0] -- every
    term within [0.05, 0.95] x its weight -- for all 60 pairs.  The wrong row must fail: evaluated for the neighbouring clip, the
    neighbouring frame and the bodies shifted by one index, the largest error-to-bound ratio over the samples is at least 100.

    Measured over the six cases: largest |error| / bound 0.069 (body_reward) and 0.075 (endeff_reward); the wrong rows miss by at least
    5.2e5 (clip), 2.4e4 (frame) and 3.1e5 (body shift) bounds."""
    env, states = _body_steps(model, T)
    nbody = env.sys.nbody
    rows = env._body["track_bodies"].cpu().numpy().astype(np.float64)
    assert rows.shape == (C, T, nbody, 3) and np.array_equal(rows, F.ref_bodies(model, T).astype(np.float32).astype(np.float64))
    B, E = tuple(range(1, nbody)), EFF[model]
    assert nbody - 1 in E or nbody - 2 in E                 # an end effector on a lane's second body
    worst, alt = np.zeros(2), {k: np.zeros(2) for k in ("clip", "frame", "shift")}
    lo, hi = np.full(2, np.inf), np.zeros(2)

    def terms(xpos, row):
        return rodent.body_rewards(xpos, row, B, E, BW, SCALES)
    for t in range(1, STEPS + 1):
        s = states[t]
        xpos = s.pipeline_state.xpos.cpu().numpy().astype(np.float64).reshape(N, nbody, 3)
        fi = np.clip(states[t - 1].info["cur_frame"].cpu().numpy(), 0, T - 1)
        want = terms(xpos, rows[IDS, fi])
        got = [s.metrics[k].cpu().numpy().astype(np.float64) for k in BODY_METRICS]
        for i in range(2):
            x = -np.log(want[i] / BW[i])
            lo[i], hi[i] = min(lo[i], x.min()), max(hi[i], x.max())
            assert (x >= 0.051).all() and (x <= 3.0).all(), (model, T, t, i, x.min(), x.max())
            bound = _bound(want[i], BW[i], nbody)
            worst[i] = max(worst[i], float((np.abs(got[i] - want[i]) / bound).max()))
        fj = np.where(fi + 1 <= T - 1, fi + 1, fi - 1)       # a neighbouring frame inside the clip
        for name, row in (("clip", rows[(IDS + 1) % C, fi]), ("frame", rows[IDS, fj]), ("shift", np.roll(rows[IDS, fi], 1, axis=1))):
            other = terms(xpos, row)
            for i in range(2):
                alt[name][i] = max(alt[name][i], float((np.abs(got[i] - other[i]) / _bound(want[i], BW[i], nbody)).max()))
    print(f"{model} T={T}: exponents body [{lo[0]:.4f}, {hi[0]:.4f}] endeff [{lo[1]:.4f}, {hi[1]:.4f}]; largest |error| / bound: body_reward "
          f"{worst[0]:.3f}, endeff_reward {worst[1]:.3f}; wrong rows, largest ratio (body, endeff): clip {alt['clip'][0]:.3g} {alt['clip'][1]:.3g}, "
          f"frame {alt['frame'][0]:.3g} {alt['frame'][1]:.3g}, body shift {alt['shift'][0]:.3g} {alt['shift'][1]:.3g}")
    assert worst[0] <= 1.0 and worst[1] <= 1.0, worst
    assert alt["clip"].min() >= 100 and alt["frame"].min() >= 100 and alt["shift"].min() >= 100, alt


# ---------------------------------------------------------------------------------------------- 4. launch forms
@pytest.mark.parametrize("model,T", CASES)
def test_single_step_and_multi_step_agree(model, T):
    got, _ = _forms(model, T)
    a, b = got["steps"], got["unroll"]
    for k in BODY_METRICS:
        assert torch.equal(a.metrics[k], b.metrics[k]), (model, T, k)
    assert torch.equal(a.reward, b.reward)
    la, lb = F.leaves(a), F.leaves(b)
    assert len(la) == len(lb) > 10
    for i, (x, y) in enumerate(zip(la, lb)):
        assert torch.equal(x, y), (model, T, i)


# ---------------------------------------------------------------------------------------------- 5. combinations
@pytest.mark.parametrize("model", MODELS)
def test_with_reference_frames_and_a_termination_threshold(model):
    """H = 5 and `max_quat_error` (the data-derived threshold of tests/test_gpu_pose_termination.py, which fires in 25 % .. 75 % of the
    pairs): the whole state but the reward is that env's without bodies -- the observation's blocks, done and the failure code included --
    in bare steps and in the wrapped forms; the reward composes as everywhere."""
    T = 104
    thr = F.term_reference(model, T)[3][1]
    with_b, without = F.make_body(model, T, reference_obs_frames=5, max_quat_error=thr), F.make(model, T, reference_obs_frames=5, max_quat_error=thr)
    acts, _ = F.draws(with_b, STEPS, 1)
    got, want = F.steps(with_b, acts), F.steps(without, acts)
    fails = 0
    for t in range(1, STEPS + 1):
        _assert_same(got[t], want[t], (model, t), metrics=POSE_METRICS + F.FAIL_METRICS)
        assert np.array_equal(F.f32(got[t].reward), _composed(want[t].reward, got[t])), (model, t)
        fails += int(got[t].metrics["pose_fail"].sum())
    assert 15 <= fails <= 45 and got[1].obs.shape[1] == with_b.sys.obs_dim + 5 * with_b.sys.nq
    acts, noise = F.draws(with_b, 7, 2)
    fg, fw = F.wrapped_forms(with_b, acts, noise, F.actor(with_b, 7)), F.wrapped_forms(without, acts, noise, F.actor(without, 7))
    for k in ("steps", "unroll", "policy"):
        _assert_same(fg[k], fw[k], (model, k), metrics=POSE_METRICS + F.FAIL_METRICS)
    for name in ("obs", "raw_action", "log_prob", "discount", "truncation"):
        assert torch.equal(getattr(fg["buf"], name), getattr(fw["buf"], name)), (model, name)


# ---------------------------------------------------------------------------------------------- 6. zero weights, no end effectors
@pytest.mark.parametrize("model", MODELS)
def test_zero_weights_give_the_pose_env(model):
    _, want = F.pose_ref(model, 104)
    env = F.make_body(model, 104, weights=(0.0, 0.0), pipeline_outputs=True)
    got = F.steps(env, F.draws(env, STEPS, 1)[0])
    for t, (g, w) in enumerate(zip(got, want)):
        _assert_same(g, w, (model, t), reward=True)
        assert all(float(g.metrics[k].abs().max()) == 0.0 for k in BODY_METRICS)


@pytest.mark.parametrize("model", MODELS)
def test_without_end_effectors_the_reward_has_the_body_term_alone(model):
    _, want = F.pose_ref(model, 104)
    _, full = _body_steps(model, 104)
    env = F.make_body(model, 104, eff=None, pipeline_outputs=True)
    assert env.body_tracking["end_effector_ids"] == () and env.body_tracking["endeff_reward"][0] == 0.0
    got = F.steps(env, F.draws(env, STEPS, 1)[0])
    for t in range(1, STEPS + 1):
        _assert_same(got[t], want[t], (model, t))
        assert float(got[t].metrics["endeff_reward"].abs().max()) == 0.0
        assert torch.equal(got[t].metrics["body_reward"], full[t].metrics["body_reward"])
        assert np.array_equal(F.f32(got[t].reward), F.f32(want[t].reward) + F.f32(got[t].metrics["body_reward"])), (model, t)


# ---------------------------------------------------------------------------------------------- 7. bad state
@pytest.mark.parametrize("model", MODELS)
def test_a_bad_step_zeroes_the_body_terms(model):
    from rodent_amd.envs import wrappers
    from rodent_amd.training import acting
    env = F.make_body(model, 104, bad_state_max=1e10)
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
    ok = [e for e in range(N) if e != bad]
    for k, s in res.items():
        for name in BODY_METRICS + POSE_METRICS:
            assert float(s.metrics[name][bad]) == 0.0, (model, k, name)
        assert float(s.reward[bad]) == 0.0 and float(s.done[bad]) == 1.0, (model, k)
        assert float(s.metrics["body_reward"][ok].min()) > 0 and float(s.metrics["endeff_reward"][ok].min()) > 0 and float(s.done[ok].max()) == 0.0
    assert float(buf.reward[0, bad, 0]) == 0.0 and float(buf.reward[0, ok, 0].min()) > 0
    assert env.bad_states() == 3


# ---------------------------------------------------------------------------------------------- 8. refusals
def test_refusals():
    from rodent_amd import envs
    T = 104
    track = F.tracks(T)[0]

    def build(model, pose=True, **kw):
        q0 = F.qpos0(model)
        if pose:
            kw.update(track_quat=np.tile([1.0, 0.0, 0.0, 0.0], (T, 1)), track_joints=np.tile(q0[7:], (T, 1)))
        return envs.get_environment("rodent", track_pos=track, num_envs=4, xml_path=f"{model}.xml", iterations=4, ls_iterations=4, n_frames=2,
                                    device=DEV, **kw)
    bodies = F.ref_bodies("rodent_optimized", T)[0]
    with pytest.raises(ValueError, match="track_quat and track_joints"):
        build("rodent_optimized", pose=False, track_bodies=bodies)
    with pytest.raises(RuntimeError, match="Newton solver"):
        build("rodent_optimized", solver="newton", track_bodies=bodies)
    cpu = build("rodent_cpu", pose=False, healthy_z_range=(-0.3, 0.3))
    with pytest.raises(RuntimeError, match="candidate-pair contacts"):
        build("rodent_cpu", healthy_z_range=(-0.3, 0.3), track_bodies=np.zeros((T, cpu.sys.nbody, 3)))
    # the library's own answers, on batches without a pose block
    assert "candidate-pair contacts" in cpu._batch.body_tracking_supported() and "candidate-pair contacts" in cpu._batch.body_tracking_supported(with_actor=True)
    assert "Newton solver" in build("rodent_optimized", pose=False, solver="newton")._batch.body_tracking_supported()
    plain = build("rodent_optimized", pose=False)
    assert plain._batch.body_tracking_supported() is None and plain._batch.body_tracking_supported(with_actor=True) is None
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)
    block = (dev(bodies), torch.zeros(2, plain.sys.nbody, device=DEV), torch.zeros(4, 2, device=DEV))
    with pytest.raises(RuntimeError, match="needs a pose block"):
        plain._batch.set_body_tracking(*block)
    env = build("rodent_optimized", track_bodies=bodies, end_effector_ids=EFF["rodent_optimized"])
    with pytest.raises(RuntimeError, match="per-env parameters"):
        env.randomize(lambda sys: (sys.replace(dof_damping=np.repeat(sys.dof_damping[None], 4, axis=0)), {"dof_damping": 0}))
    with pytest.raises(RuntimeError, match="per-env parameters"):
        env.set_env_params(dof_f=torch.zeros(4, env.sys.nv, 16, device=DEV))
    st = env.step(env.reset(jax_random.split(jax_random.PRNGKey(1), 4)), torch.zeros(4, env.action_size, device=DEV))      # still a working env
    assert float(st.metrics["body_reward"].min()) > 0
    b = env._batch      # the block stands on the batch after the step
    with pytest.raises(RuntimeError, match="clear it first"):
        b.set_pose(None)
    for bad in ((-1.0, 8.0), (1.0, float("nan")), (float("inf"), 1.0)):
        with pytest.raises(RuntimeError, match="finite and >= 0"):
            b.set_body_tracking(*block, body_reward=bad)
        with pytest.raises(RuntimeError, match="finite and >= 0"):
            b.set_body_tracking(*block, endeff_reward=bad)
    with pytest.raises(RuntimeError, match="null track_bodies, body_weights or body_metrics"):
        b.set_body_tracking(block[0], None, block[2])
    with pytest.raises(RuntimeError, match="no evaluation instance rewards the body positions"):
        env.unroll_eval(env.reset(jax_random.split(jax_random.PRNGKey(1), 4)), 2, F.actor(env, 1))


# ---------------------------------------------------------------------------------------------- 9. training
def test_ppo_train_on_a_body_env(monkeypatch):
    """One training step at 64 envs through the one-launch rollout (rr_env_unroll_policy on the body instance with the actor), evaluations
    by the per-step loop: finite losses and finite eval/episode_body_reward and eval/episode_endeff_reward next to the existing keys."""
    from rodent_amd.training import acting
    from rodent_amd.training.agents.ppo import train as ppo
    env = F.make_body("rodent_optimized", 104, n=64)
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
        for k in ("eval/episode_reward", "eval/episode_quat_reward", "eval/episode_body_reward", "eval/episode_endeff_reward"):
            assert k in m and math.isfinite(float(m[k])), k
        assert 0 < float(m["eval/episode_body_reward"]) <= 10 * BW[0] and 0 < float(m["eval/episode_endeff_reward"]) <= 10 * BW[1]
