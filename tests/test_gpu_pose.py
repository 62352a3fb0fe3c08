"""Pose tracking on the GPU (`Rodent(track_quat=..., track_joints=...)`; rr_batch_set_pose / rr_pose_io, the rr_pose_kernel instances): the reward's
two pose terms against a plain env of the same build -- bit for bit where nothing but the reward may move -- and against the float64
restatement `rodent.pose_rewards`.

Fixture (as tests/test_gpu_multiclip.py): N = 12 envs, C = 3 clips, env e on clip e % 3 (explicit ids); n_frames = 2, solver iterations
4 / 4, five steps.  T = 104 (start frames 0 .. 99: the two envs that start at frame 99 run past the clip's end) and T = 3 (every read
clamps).  Reference pose: the quaternion of clip c at frame t is a rotation about z by 0.1 (c + 1) + 0.003 t, the joints are
qpos0[7:] + 0.02 sin(0.7 j + 0.05 t + c): every (clip, frame, joint) differs.  Scales: the rotation angle between the rodent and its clip
lies in [0.10, 0.34] for T = 3 and in [0.12, 0.62] for T = 104, the summed squared joint error in [0.2, 2.5] (float64 CPU oracle on this
fixture under uniform random actions), so quat_reward_scale 12 / 5 and joint_reward_scale 0.6 keep both exponents inside
[-log 0.95, -log 0.05] = [0.051, 3.0]; the formula test asserts that.  Weights 0.75 / 0.5 (not the defaults)."""
import math

import numpy as np
import pytest
import torch

from rodent_amd import jax_random
from rodent_amd.envs import rodent
from tests.pose_fixture import (ACTOR_REWARD_TOL, C, DEV, EPS, IDS, JOINT_SCALE, MODELS, N, OLD_METRICS, QUAT_SCALE, STEPS, W, actor, draws, f32, forms,
                                keys, leaves, make, plain_steps, qpos0, steps, tracks, traj)

pytestmark = pytest.mark.gpu


def _assert_same_but_reward(got, want, what):
    """Everything of the two states except `reward` (and the two pose metrics, which only `got` has): the pipeline state, obs, done, info
    and the three old metrics, bit for bit."""
    assert set(got.metrics) - set(want.metrics) == {"quat_reward", "joint_reward"}
    pairs = [("pipeline_state", got.pipeline_state, want.pipeline_state), ("obs", got.obs, want.obs), ("done", got.done, want.done),
             ("info", got.info, want.info), ("metrics", {k: got.metrics[k] for k in OLD_METRICS}, {k: want.metrics[k] for k in OLD_METRICS})]
    for name, a, b in pairs:
        la, lb = leaves(a), leaves(b)
        assert len(la) == len(lb) >= 1, (what, name)
        for i, (x, y) in enumerate(zip(la, lb)):
            assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), (what, name, i, int((x != y).sum()))


def _composed(plain_reward, state):
    """f32(f32(plain + quat_reward) + joint_reward) in numpy float32 arithmetic (each `+` of two float32 arrays rounds once)."""
    return (f32(plain_reward) + f32(state.metrics["quat_reward"])) + f32(state.metrics["joint_reward"])


CASES = [(m, T) for m in MODELS for T in (104, 3)]


# ---------------------------------------------------------------------------------------------- 1. nothing else moves
@pytest.mark.parametrize("model,T", CASES)
def test_physics_and_old_outputs_are_untouched_by_plain_steps(model, T):
    env, got, want = plain_steps(model, T)
    assert env.pose_tracking and not env.eval_supported()
    assert all(float(got[0].metrics[k].abs().max()) == 0.0 for k in ("quat_reward", "joint_reward"))       # zeros at reset
    assert torch.equal(got[0].reward, want[0].reward)
    for t, (g, w) in enumerate(zip(got, want)):
        _assert_same_but_reward(g, w, (model, T, t))
    frames = got[-1].info["cur_frame"].cpu().numpy()
    if T == 104:
        assert (frames > T - 1).sum() >= 2 and (frames < T - 1).sum() >= 6         # reads past the clip's end / inside the clip


@pytest.mark.parametrize("model,T", CASES)
def test_physics_and_old_outputs_are_untouched_by_the_multi_step_forms(model, T):
    got, want = forms(model, T)
    for k in ("steps", "unroll", "policy"):
        _assert_same_but_reward(got[k], want[k], (model, T, k))
    assert torch.equal(got["policy_actions"], want["policy_actions"])
    for name in ("obs", "raw_action", "log_prob", "discount", "truncation"):            # everything but traj.reward
        assert torch.equal(getattr(got["buf"], name), getattr(want["buf"], name)), (model, T, name)
    assert float(got["unroll"].info["steps"].max()) <= 3 and bool((got["buf"].discount == 0).any())       # episodes ended: restores ran
    assert not torch.equal(got["buf"].reward, want["buf"].reward)


# ---------------------------------------------------------------------------------------------- 2. composition
@pytest.mark.parametrize("model,T", CASES)
def test_reward_is_plain_plus_quat_plus_joint(model, T):
    """reward == f32(f32(plain.reward + quat_reward) + joint_reward), the plain env's reward and the pose env's own metrics: bit for
    bit in `step` and `unroll`; in the actor form (last step of the launch, whose metrics the state carries) within the one ulp
    tests/test_gpu_ppo.py allows that instance's plain reward."""
    _, got, want = plain_steps(model, T)
    for t in range(1, STEPS + 1):
        assert np.array_equal(f32(got[t].reward), _composed(want[t].reward, got[t])), (model, T, t)
        assert float(got[t].metrics["quat_reward"].min()) > 0 and float(got[t].metrics["joint_reward"].min()) > 0
    fg, fw = forms(model, T)
    for k in ("steps", "unroll"):
        assert np.array_equal(f32(fg[k].reward), _composed(fw[k].reward, fg[k])), (model, T, k)
    last = np.abs(f32(fg["buf"].reward[0, :, -1]).astype(np.float64) - _composed(fw["buf"].reward[0, :, -1], fg["policy"]).astype(np.float64))
    print(f"{model} T={T}: actor form, last step: max |traj.reward - composed| = {last.max():.3g}")
    assert last.max() <= ACTOR_REWARD_TOL
    assert np.array_equal(f32(fg["policy"].reward), f32(fg["buf"].reward[0, :, -1]))       # t_reward receives the total the state carries


# ---------------------------------------------------------------------------------------------- 3. formula
def _bounds(qr, jr, kq, kj):
    """Error bounds of the two terms around the float64 values `qr`, `jr` (see test_against_the_formula)."""
    xq, xj = -np.log(qr / W[0]), -np.log(jr / W[1])
    return 2 * (32 * xq + 22 * kq + 5) * EPS * qr, 2 * (11 * xj + 5) * EPS * jr


@pytest.mark.parametrize("model,T", CASES)
def test_against_the_formula(model, T):
    """The two metrics against `pose_rewards` in float64 on the returned float32 qpos and the float32 rows the device holds.

    Bounds c (a x + b) eps want, eps = 2^-24, x the exponent's magnitude, c = 2 for the slack of a first-order count (as
    tests/test_gpu_multiclip.py).

    joint_reward, x = k S, S = sum of 67 squares: a difference (eps), its square (2 eps + eps), at most one addition inside a lane and
    the six additions of the wave sum's butterfly (7 eps; all terms positive, so relative errors do not grow), the product with k (eps):
    11 eps x on the exponent, which exp turns into a relative error of the result; expf within 2 ulp = 4 eps, the product with the
    weight eps: (11 x + 5) eps.

    quat_reward, x = k theta^2: each component of d is a sum of four products of magnitude <= s = |r||q| whose absolute values sum to
    <= s: 4 eps s absolute (four products, three sums).  |d.xyz|: sqrt(3) * 4 eps s from the components plus 3 eps s of its own (squares,
    sums, sqrtf within 1 ulp), <= 10 eps s; |d.w|: 4 eps s.  atan2's gradient has length 1 / s, so theta / 2 carries <= 11 eps absolute
    plus atan2f's 2 ulp = 4 eps relative: theta carries (22 + 4 theta) eps; theta^2 then (44 theta + 9 theta^2) eps, the product with k
    one more eps: k (44 theta + 10 theta^2) eps = (10 x + 44 sqrt(k x)) eps <= (32 x + 22 k) eps by sqrt(k x) <= (k + x) / 2.  With expf
    and the weight: (32 x + 22 k + 5) eps.

    Neither exp may be saturated: every checked term lies within [0.05, 0.95] x its weight.  The wrong row must fail: evaluated for
    the neighbouring clip, for the neighbouring frame and (joints) with the joint row shifted by one index, the largest error-to-bound
    ratio over the samples -- the number this test holds below 1 for the right row -- is at least 100.  (Over the samples, not per
    sample: the joint term moves by -2 sum e_i dr_i + sum dr_i^2, which for a single env and step can cancel to nothing.)"""
    env, states, _ = plain_steps(model, T)
    kq, kj = QUAT_SCALE[T], JOINT_SCALE
    rows = env._pose_host.astype(np.float64)                 # float32 [C, T, nq - 3], what the device holds
    assert rows.shape == (C, T, env.sys.nq - 3) and torch.equal(env._track_pose.cpu(), torch.from_numpy(env._pose_host))
    worst = np.zeros(2)
    alt = {k: np.zeros(2) for k in ("clip", "frame", "shift")}

    def terms(qpos, row):
        return rodent.pose_rewards(qpos, row[:, :4], row[:, 4:], W, (kq, kj))
    for t in range(1, STEPS + 1):
        s = states[t]
        qpos = s.pipeline_state.qpos.cpu().numpy().astype(np.float64)
        old = states[t - 1].info["cur_frame"].cpu().numpy()
        fi = np.clip(old, 0, T - 1)
        want = terms(qpos, rows[IDS, fi])
        got = [s.metrics[k].cpu().numpy().astype(np.float64) for k in ("quat_reward", "joint_reward")]
        bound = _bounds(want[0], want[1], kq, kj)
        for i in range(2):
            assert (want[i] >= 0.05 * W[i]).all() and (want[i] <= 0.95 * W[i]).all(), (model, T, t, i, want[i].min() / W[i], want[i].max() / W[i])
            ratio = np.abs(got[i] - want[i]) / bound[i]
            worst[i] = max(worst[i], float(ratio.max()))
        fj = np.where(fi + 1 <= T - 1, fi + 1, fi - 1)       # a neighbouring frame inside the clip
        shifted = rows[IDS, fi].copy()
        shifted[:, 4:] = np.roll(shifted[:, 4:], 1, axis=1)
        for name, row in (("clip", rows[(IDS + 1) % C, fi]), ("frame", rows[IDS, fj]), ("shift", shifted)):
            other = terms(qpos, row)
            for i in range(2):
                alt[name][i] = max(alt[name][i], float((np.abs(got[i] - other[i]) / bound[i]).max()))
    print(f"{model} T={T}: largest |error| / bound: quat_reward {worst[0]:.3f}, joint_reward {worst[1]:.3f}; wrong rows, largest ratio "
          f"(quat, joint): clip {alt['clip'][0]:.0f} {alt['clip'][1]:.0f}, frame {alt['frame'][0]:.0f} {alt['frame'][1]:.0f}, "
          f"joint shift {alt['shift'][1]:.0f}")
    assert worst[0] <= 1.0 and worst[1] <= 1.0, worst
    assert alt["clip"].min() >= 100 and alt["frame"].min() >= 100 and alt["shift"][1] >= 100, alt
    assert alt["shift"][0] <= 1.0                            # (the quaternion part of the shifted row is the right one)


# ---------------------------------------------------------------------------------------------- 4. launch forms
@pytest.mark.parametrize("model,T", CASES)
def test_single_step_and_multi_step_agree(model, T):
    got, _ = forms(model, T)
    a, b = got["steps"], got["unroll"]
    for k in ("quat_reward", "joint_reward"):
        assert torch.equal(a.metrics[k], b.metrics[k]), (model, T, k)
    assert torch.equal(a.reward, b.reward)
    la, lb = leaves(a), leaves(b)
    assert len(la) == len(lb) > 10
    for i, (x, y) in enumerate(zip(la, lb)):
        assert torch.equal(x, y), (model, T, i)


# ---------------------------------------------------------------------------------------------- 5. bad state
@pytest.mark.parametrize("model", MODELS)
def test_a_bad_step_zeroes_the_pose_terms(model):
    from rodent_amd.envs import wrappers
    from rodent_amd.training import acting
    env = make(model, 104, bad_state_max=1e10)
    bad = 4

    def poison(state):       # NaN into a COPY of the incoming qvel (the stored first state shares the reset's tensors)
        qvel = state.pipeline_state.qvel.clone()
        qvel[bad, 3] = float("nan")
        return state.replace(pipeline_state=state.pipeline_state.replace(qvel=qvel))
    acts, noise = draws(env, 1, 3)
    wenv = wrappers.wrap(env, episode_length=100, action_repeat=1)
    buf = acting.UnrollBuffer(1, N, 1, env.observation_size, env.action_size, torch.device(DEV))
    res = dict(step=env.step(poison(env.reset(keys(), clip=IDS)), acts[0]), unroll=wenv.unroll(poison(wenv.reset(keys(), clip=IDS)), acts),
               policy=wenv.unroll_policy(poison(wenv.reset(keys(), clip=IDS)), actor(env, 5), noise, traj(buf))[0])
    torch.cuda.synchronize()
    ok = [e for e in range(N) if e != bad]
    for k, s in res.items():
        for name in ("quat_reward", "joint_reward") + OLD_METRICS:
            assert float(s.metrics[name][bad]) == 0.0, (model, k, name)
        assert float(s.reward[bad]) == 0.0 and float(s.done[bad]) == 1.0, (model, k)
        assert float(s.metrics["quat_reward"][ok].min()) > 0 and float(s.metrics["joint_reward"][ok].min()) > 0 and float(s.done[ok].max()) == 0.0
    assert float(buf.reward[0, bad, 0]) == 0.0 and float(buf.reward[0, ok, 0].min()) > 0
    assert env.bad_states() == 3


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_refusals():
    from rodent_amd import envs
    track = tracks(104)[0]

    def build(model, **kw):
        q0 = qpos0(model)
        quat = np.tile([1.0, 0.0, 0.0, 0.0], (104, 1))
        return envs.get_environment("rodent", track_pos=track, num_envs=4, xml_path=f"{model}.xml", iterations=4, ls_iterations=4, n_frames=2,
                                    device=DEV, track_quat=quat, track_joints=np.tile(q0[7:], (104, 1)), **kw)
    with pytest.raises(RuntimeError, match="candidate-pair contacts"):
        build("rodent_cpu", healthy_z_range=(-0.3, 0.3))
    with pytest.raises(RuntimeError, match="Newton solver"):
        build("rodent_optimized", solver="newton")
    env = build("rodent_optimized")
    with pytest.raises(RuntimeError, match="per-env parameters"):
        env.randomize(lambda sys: (sys.replace(dof_damping=np.repeat(sys.dof_damping[None], 4, axis=0)), {"dof_damping": 0}))
    with pytest.raises(RuntimeError, match="per-env parameters"):
        env.set_env_params(dof_f=torch.zeros(4, env.sys.nv, 16, device=DEV))
    assert env.env_params() is None
    st = env.step(env.reset(jax_random.split(jax_random.PRNGKey(1), 4)), torch.zeros(4, env.action_size, device=DEV))      # still a working pose env
    assert float(st.metrics["quat_reward"].min()) > 0
    with pytest.raises(RuntimeError, match="no evaluation instance rewards the pose"):
        env.unroll_eval(env.reset(jax_random.split(jax_random.PRNGKey(1), 4)), 2, actor(env, 1))


# ---------------------------------------------------------------------------------------------- 7. training
def test_ppo_train_on_a_pose_env(monkeypatch):
    """One training step at 64 envs through the one-launch rollout (rr_env_unroll_policy on the pose instance with the actor), evaluations
    by the per-step loop: finite losses and finite eval/episode_quat_reward and eval/episode_joint_reward next to the existing keys."""
    from rodent_amd.training import acting
    from rodent_amd.training.agents.ppo import train as ppo
    env = make("rodent_optimized", 104, n=64)
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
        for k in ("eval/episode_reward", "eval/episode_pos_reward", "eval/episode_quat_reward", "eval/episode_joint_reward"):
            assert k in m and math.isfinite(float(m[k])), k
        assert 0 < float(m["eval/episode_quat_reward"]) <= 10 * W[0] and 0 < float(m["eval/episode_joint_reward"]) <= 10 * W[1]


# ---------------------------------------------------------------------------------------------- 8. zero weights
@pytest.mark.parametrize("model", MODELS)
def test_zero_weights_give_the_plain_env(model):
    """Both weights 0: the pose instances run, the reward gains + 0 + 0, and the whole state -- reward included -- is the plain env's, apart
    from the two metrics, which are 0."""
    _, _, want = plain_steps(model, 104)
    env = make(model, 104, weights=(0.0, 0.0))
    acts, _ = draws(env, STEPS, 1)
    got = steps(env, acts)
    for t, (g, w) in enumerate(zip(got, want)):
        _assert_same_but_reward(g, w, (model, t))
        assert torch.equal(g.reward, w.reward), (model, t)
        assert float(g.metrics["quat_reward"].abs().max()) == 0.0 and float(g.metrics["joint_reward"].abs().max()) == 0.0
