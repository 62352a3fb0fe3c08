"""Velocity tracking on the GPU (`Rodent(track_velocity=, track_angular_velocity=, track_joint_velocity=)`; rr_batch_set_velocity_tracking /
rr_vel_io, the `if (BODY)` code of the rr_body_kernel and rr_restart_kernel instances): the reward's three velocity terms against a pose
env -- and a body env -- of the same build, bit for bit where nothing but the reward may move, and against the float64 restatement
`rodent.velocity_rewards` of the step's own returned qvel.

Fixture: that of tests/pose_fixture.py (12 envs on 3 clips, n_frames 2, CG 4/4, five bare steps and the seven-step wrapped forms with
episodes of three; T = 104 and T = 3, the short clip making every frame clamp), on rodent_optimized (fixed dimensions, root-slot map),
rodent_new (the other fixed type) and rodent_0 (generic dims).  nv = 73 puts dofs 64 .. 72 on the lanes' second pass: the smallest shape
that exercises the two-pass accumulation and the wave sum.  Weights 0.7 / 0.5 / 0.3 (not the defaults).

Reference velocities: ref[c, t, d] = A(d) sin(0.7 d + 0.05 t + c) per dof d, frame t and clip c, so every entry differs; A = A_LIN on
dofs 0 .. 2, A_ANG on 3 .. 5, A_JOINT on 6 .. 72.  The amplitudes and the three scales were chosen from the POSE env's own returned
qvel on this fixture (`pose_fixture.plain_steps`: the build path without the block), not from the code under test, so that all three
exponents k S lie in [0.051, 3.0] = [-log 0.95, -log 0.05] for all 60 (env, step) pairs of every case; `test_against_the_formula`
asserts that on the float64 restatement.  Measured on that env, over the six cases, against a zero reference (the raw sums of the
env's own qvel squared): S_lin in [0.00756, 0.242], S_ang in [0.381, 53.6], S_joint in [1417, 17728] -- spreads of 32, 141 and 12.5
against the window's 3.0 / 0.051 = 59: the angular sum does not fit at any scale, the linear one only without a margin -- so the
reference's amplitude carries the sums, as the sine term of the body fixture does.  With A_LIN = 1, A_ANG = 10, A_JOINT = 20 the same
qvel gives S_lin in [0.565, 2.85], S_ang in [61.6, 401.2], S_joint in [11421, 33125]; with the scales 0.3, 0.0025 and 2e-5 the
exponents lie in [0.170, 0.855], [0.154, 1.003] and [0.228, 0.663].  (A = (1.5, 12, 0) gives spreads of 4.0, 5.5 and 12.5, A = (2, 15,
40) of 3.6, 4.6 and 1.6: the choice is not tight.)  The velocity env's own qvel is bit-equal to the pose env's
(`test_state_is_untouched_by_plain_steps`), so the test sees these ranges.

Float32 bound of a term w exp(-k S), eps = 2^-24, factor 2 for the slack of a first-order count (as tests/test_gpu_body_tracking.py).
Per dof: one difference of two float32 values (eps on d, 2 eps on d^2), the square (eps): 3 eps on the dof's term.  A lane accumulates
at most A = ceil(nv / 64) = 2 terms of a sum (A eps; the +0 a dof adds to the other two sums is exact), the wave sum has six levels
(6 eps; all terms positive, so relative errors do not grow): (9 + A) eps on S; the product with the scale one more: (10 + A) eps x on
the exponent x = k S, which exp turns into a relative error of the result; expf within 2 ulp = 4 eps, the product with the weight eps:
2 ((10 + A) x + 5) eps, relative -- c = 10."""
import functools
import math

import numpy as np
import pytest
import torch

from rodent_amd import jax_random
from rodent_amd.envs import rodent, wrappers
from tests import pose_fixture as F
from tests.pose_fixture import C, DEV, EPS, IDS, N, STEPS

pytestmark = pytest.mark.gpu
MODELS = ["rodent_optimized", "rodent_new", "rodent_0"]
CASES = [(m, T) for m in MODELS for T in (104, 3)]
POSE_METRICS = F.OLD_METRICS + ("quat_reward", "joint_reward")
BODY_METRICS = ("body_reward", "endeff_reward")
VEL_METRICS = ("lin_vel_reward", "ang_vel_reward", "joint_vel_reward")
VW = (0.7, 0.5, 0.3)                              # lin / ang / joint _vel_reward_weight
A_LIN, A_ANG, A_JOINT = 1.0, 10.0, 20.0           # amplitudes of the reference (module docstring)
VS = (0.3, 0.0025, 2e-5)                          # lin / ang / joint _vel_reward_scale (module docstring)
RANGE = (90, 102)                                 # restart_frame_range of the clip-restart envs (T = 104)


# ---------------------------------------------------------------------------------------------- the fixture
@functools.lru_cache(maxsize=None)
def ref_vel(model, T):
    """Reference velocities [C, T, nv] in qvel layout, float64."""
    nv = len(F.qpos0(model)) - 1
    d, t, c = np.arange(nv, dtype=np.float64)[None, None], np.arange(T, dtype=np.float64)[None, :, None], np.arange(C, dtype=np.float64)[:, None, None]
    amp = np.where(d < 3, A_LIN, np.where(d < 6, A_ANG, A_JOINT))
    return amp * np.sin(0.7 * d + 0.05 * t + c)


def vel_kw(model, T, weights=VW):
    v = ref_vel(model, T)
    return dict(track_velocity=v[..., :3], track_angular_velocity=v[..., 3:6], track_joint_velocity=v[..., 6:], lin_vel_reward_weight=weights[0],
                lin_vel_reward_scale=VS[0], ang_vel_reward_weight=weights[1], ang_vel_reward_scale=VS[1], joint_vel_reward_weight=weights[2],
                joint_vel_reward_scale=VS[2])


def make_vel(model, T, weights=VW, bodies=False, **kw):
    return (F.make_body if bodies else F.make)(model, T, **vel_kw(model, T, weights), **kw)


@functools.lru_cache(maxsize=None)
def _steps(model, T, bodies=False):
    """Computed once and shared: (the velocity env, its states of five bare steps on the keys, clips and actions of `F.plain_steps`)."""
    env = make_vel(model, T, bodies=bodies)
    return env, F.steps(env, F.draws(env, STEPS, 1)[0])


@functools.lru_cache(maxsize=None)
def _body_steps(model, T):
    """Computed once and shared: the states of five bare steps of the body env WITHOUT the velocity block."""
    env = F.make_body(model, T)
    return F.steps(env, F.draws(env, STEPS, 1)[0])


@functools.lru_cache(maxsize=None)
def _forms(model, T):
    """Computed once and shared: the wrapped forms (seven steps, episodes of three) of the velocity env and of the pose env."""
    env = make_vel(model, T)
    assert env._batch.unroll_supported(False) and env._batch.unroll_supported(True)
    acts, noise = F.draws(env, 7, 2)
    return F.wrapped_forms(env, acts, noise, F.actor(env, 7)), F.forms(model, T)[0]


def _assert_same(got, want, what, metrics=POSE_METRICS, reward=False, new=VEL_METRICS):
    """Everything of the two states except `reward` (unless asked) and the metrics only `got` has: pipeline state, obs, done, info and
    `metrics`, bit for bit."""
    assert set(got.metrics) - set(want.metrics) == set(new) and set(metrics) <= set(want.metrics), what
    pairs = [("pipeline_state", got.pipeline_state, want.pipeline_state), ("obs", got.obs, want.obs), ("done", got.done, want.done),
             ("info", got.info, want.info), ("metrics", {k: got.metrics[k] for k in metrics}, {k: want.metrics[k] for k in metrics})]
    if reward:
        pairs.append(("reward", got.reward, want.reward))
    for name, a, b in pairs:
        la, lb = F.leaves(a), F.leaves(b)
        assert len(la) == len(lb) >= 1, (what, name)
        for i, (x, y) in enumerate(zip(la, lb)):
            assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), (what, name, i, int((x != y).sum()))


def _composed(reward, state, zero=None):
    """f32(f32(f32(reward + lin) + ang) + joint) in numpy float32 arithmetic, the three terms from `state`'s own metrics (`zero`: that
    term left out)."""
    out = F.f32(reward)
    for j, k in enumerate(VEL_METRICS):
        if j != zero:
            out = out + F.f32(state.metrics[k])
    assert out.dtype == np.float32
    return out


# ---------------------------------------------------------------------------------------------- 1. nothing else moves
@pytest.mark.parametrize("model,T", CASES)
def test_state_is_untouched_by_plain_steps(model, T):
    env, got = _steps(model, T)
    _, want, _ = F.plain_steps(model, T)
    vt = env.velocity_tracking
    assert vt == dict(lin_vel_reward=(VW[0], VS[0]), ang_vel_reward=(VW[1], VS[1]), joint_vel_reward=(VW[2], VS[2])) and not env.eval_supported()
    assert list(got[1].metrics) == list(POSE_METRICS + VEL_METRICS)
    assert all(float(got[0].metrics[k].abs().max()) == 0.0 for k in VEL_METRICS)        # zeros at reset
    _assert_same(got[0], want[0], (model, T, "reset"), reward=True)
    for t in range(1, STEPS + 1):
        _assert_same(got[t], want[t], (model, T, t))
        assert not torch.equal(got[t].reward, want[t].reward)
    sib = env.with_num_envs(4)
    assert sib.velocity_tracking == vt and sib.num_envs == 4


@pytest.mark.parametrize("model,T", CASES)
def test_with_bodies_the_state_is_the_body_envs(model, T):
    """(pose, bodies, velocity) against (pose, bodies): everything but the reward, the body metrics included; the reward composes on
    the body env's; the velocity metrics are those of the env without bodies (the same qvel, the same rows)."""
    env, got = _steps(model, T, True)
    want, alone = _body_steps(model, T), _steps(model, T)[1]
    assert list(got[1].metrics) == list(POSE_METRICS + BODY_METRICS + VEL_METRICS)
    _assert_same(got[0], want[0], (model, T, "reset"), metrics=POSE_METRICS + BODY_METRICS, reward=True)
    for t in range(1, STEPS + 1):
        _assert_same(got[t], want[t], (model, T, t), metrics=POSE_METRICS + BODY_METRICS)
        assert np.array_equal(F.f32(got[t].reward), _composed(want[t].reward, got[t])) and not torch.equal(got[t].reward, want[t].reward)
        for k in VEL_METRICS:
            assert torch.equal(got[t].metrics[k], alone[t].metrics[k]), (model, T, t, k)


@pytest.mark.parametrize("model,T", CASES)
def test_state_is_untouched_by_the_multi_step_forms(model, T):
    got, want = _forms(model, T)
    for k in ("steps", "unroll", "policy"):
        _assert_same(got[k], want[k], (model, T, k))
    assert torch.equal(got["policy_actions"], want["policy_actions"])
    for name in ("obs", "raw_action", "log_prob", "discount", "truncation"):            # everything but traj.reward
        assert torch.equal(getattr(got["buf"], name), getattr(want["buf"], name)), (model, T, name)
    assert float(got["unroll"].info["steps"].max()) <= 3 and bool((got["buf"].discount == 0).any())       # episodes ended: restores ran
    assert not torch.equal(got["buf"].reward, want["buf"].reward) and not torch.equal(got["unroll"].reward, want["unroll"].reward)


# ---------------------------------------------------------------------------------------------- 2. composition
@pytest.mark.parametrize("model,T", CASES)
def test_reward_is_the_pose_reward_plus_the_three_terms(model, T):
    """reward == f32(f32(f32(r + lin) + ang) + joint) with r the pose env's reward and the terms the env's own metrics: bit for bit in
    `step` and `unroll`; in the actor form (last step of the launch, whose metrics the state carries) within the one ulp
    tests/test_gpu_ppo.py allows that instance's reward.  `step` and `unroll` agree bit for bit on all three metrics."""
    _, got = _steps(model, T)
    _, want, _ = F.plain_steps(model, T)
    for t in range(1, STEPS + 1):
        assert np.array_equal(F.f32(got[t].reward), _composed(want[t].reward, got[t])), (model, T, t)
        assert all(float(got[t].metrics[k].min()) > 0 for k in VEL_METRICS)
    fg, fw = _forms(model, T)
    for k in ("steps", "unroll"):
        assert np.array_equal(F.f32(fg[k].reward), _composed(fw[k].reward, fg[k])), (model, T, k)
    for k in VEL_METRICS:
        assert torch.equal(fg["steps"].metrics[k], fg["unroll"].metrics[k]), (model, T, k)
    assert torch.equal(fg["steps"].reward, fg["unroll"].reward)
    last = np.abs(F.f32(fg["buf"].reward[0, :, -1]).astype(np.float64) - _composed(fw["buf"].reward[0, :, -1], fg["policy"]).astype(np.float64))
    print(f"{model} T={T}: actor form, last step: max |traj.reward - composed| = {last.max():.3g}")
    assert last.max() <= F.ACTOR_REWARD_TOL
    assert np.array_equal(F.f32(fg["policy"].reward), F.f32(fg["buf"].reward[0, :, -1]))       # t_reward receives the total the state carries


# ---------------------------------------------------------------------------------------------- 3. formula
def _bound(want, weight, nv):
    """Float32 error bound of a term around its float64 value `want` (module docstring)."""
    x = -np.log(want / weight)
    return 2 * ((10 + math.ceil(nv / 64)) * x + 5) * EPS * want


@pytest.mark.parametrize("model,T", CASES)
def test_against_the_formula(model, T):
    """The three metrics against `velocity_rewards` in float64 on the step's own returned float32 qvel and the float32 rows the device
    holds, at the clip and the clamped frame, within the bound of the module docstring.  All three exponents must lie in [0.051, 3.0]
    -- every term within [0.05, 0.95] x its weight -- for all 60 pairs.  The wrong row must fail: evaluated for the neighbouring clip,
    the neighbouring frame and the dofs shifted by one index, the largest error-to-bound ratio over the samples is at least 100.

    Measured over the six cases: exponents lin [0.170, 0.855], ang [0.154, 1.003], joint [0.228, 0.663]; largest |error| / bound 0.141
    (lin), 0.099 (ang) and 0.129 (joint); the wrong rows miss by at least 8.2e4 (clip), 2.9e3 (frame) and 3.1e4 (dof shift) bounds."""
    env, states = _steps(model, T)
    nv = env.sys.nv
    rows = env._track_vel.cpu().numpy().astype(np.float64)
    assert nv == 73 and rows.shape == (C, T, nv) and np.array_equal(rows, ref_vel(model, T).astype(np.float32).astype(np.float64))
    assert np.array_equal(env._vel_host.astype(np.float64), rows)
    worst, alt = np.zeros(3), {k: np.zeros(3) for k in ("clip", "frame", "shift")}
    lo, hi = np.full(3, np.inf), np.zeros(3)
    for t in range(1, STEPS + 1):
        s = states[t]
        qvel = s.pipeline_state.qvel.cpu().numpy().astype(np.float64)
        fi = np.clip(states[t - 1].info["cur_frame"].cpu().numpy(), 0, T - 1)
        want = rodent.velocity_rewards(qvel, rows[IDS, fi], VW, VS)
        got = [s.metrics[k].cpu().numpy().astype(np.float64) for k in VEL_METRICS]
        for i in range(3):
            x = -np.log(want[i] / VW[i])
            lo[i], hi[i] = min(lo[i], x.min()), max(hi[i], x.max())
            assert (x >= 0.051).all() and (x <= 3.0).all(), (model, T, t, i, x.min(), x.max())
            worst[i] = max(worst[i], float((np.abs(got[i] - want[i]) / _bound(want[i], VW[i], nv)).max()))
        fj = np.where(fi + 1 <= T - 1, fi + 1, fi - 1)       # a neighbouring frame inside the clip
        for name, row in (("clip", rows[(IDS + 1) % C, fi]), ("frame", rows[IDS, fj]), ("shift", np.roll(rows[IDS, fi], 1, axis=1))):
            other = rodent.velocity_rewards(qvel, row, VW, VS)
            for i in range(3):
                alt[name][i] = max(alt[name][i], float((np.abs(got[i] - other[i]) / _bound(want[i], VW[i], nv)).max()))
    print(f"{model} T={T}: exponents lin [{lo[0]:.4f}, {hi[0]:.4f}] ang [{lo[1]:.4f}, {hi[1]:.4f}] joint [{lo[2]:.4f}, {hi[2]:.4f}]; largest "
          f"|error| / bound (lin, ang, joint): {worst[0]:.3f} {worst[1]:.3f} {worst[2]:.3f}; wrong rows, largest ratio: clip {alt['clip']}, "
          f"frame {alt['frame']}, dof shift {alt['shift']}")
    assert (worst <= 1.0).all(), worst
    assert alt["clip"].min() >= 100 and alt["frame"].min() >= 100 and alt["shift"].min() >= 100, alt


# ---------------------------------------------------------------------------------------------- 4. weight 0
@pytest.mark.parametrize("term", [0, 1, 2], ids=VEL_METRICS)
@pytest.mark.parametrize("model", MODELS)
def test_a_zero_weight_switches_its_term_off(model, term):
    """That metric is exactly 0, the other two are the full env's bits, and the reward is the reward without that term in every bit:
    f32(f32(r + a) + b) of the two terms left, in their order (x + 0 is x)."""
    T = 104
    _, full = _steps(model, T)
    _, pose, _ = F.plain_steps(model, T)
    env = make_vel(model, T, weights=tuple(0.0 if j == term else w for j, w in enumerate(VW)))
    got = F.steps(env, F.draws(env, STEPS, 1)[0])
    for t in range(1, STEPS + 1):
        _assert_same(got[t], pose[t], (model, term, t))
        for j, k in enumerate(VEL_METRICS):
            if j == term:
                assert float(got[t].metrics[k].abs().max()) == 0.0, (model, term, t)
            else:
                assert torch.equal(got[t].metrics[k], full[t].metrics[k]), (model, term, t, k)
        assert np.array_equal(F.f32(got[t].reward), _composed(pose[t].reward, full[t], zero=term)), (model, term, t)
        assert not torch.equal(got[t].reward, full[t].reward)


# ---------------------------------------------------------------------------------------------- 5. with the other options
@pytest.mark.parametrize("model", MODELS)
def test_with_a_termination_threshold_and_no_bodies(model):
    """Pose termination without bodies runs rr_poseterm_kernel; with the velocity block the launch runs the body instance -- the only
    one with the velocity code, so the three metrics are there -- and `done` and the failure code are the termination-only env's."""
    T = 104
    thr = F.term_reference(model, T)[3][1]
    with_v, without = make_vel(model, T, max_quat_error=thr), F.make(model, T, max_quat_error=thr)
    acts, _ = F.draws(with_v, STEPS, 1)
    got, want = F.steps(with_v, acts), F.steps(without, acts)
    fails = 0
    for t in range(1, STEPS + 1):
        _assert_same(got[t], want[t], (model, t), metrics=POSE_METRICS + F.FAIL_METRICS)
        assert np.array_equal(F.f32(got[t].reward), _composed(want[t].reward, got[t])), (model, t)
        assert all(float(got[t].metrics[k].min()) > 0 for k in VEL_METRICS)
        fails += int(got[t].metrics["pose_fail"].sum())
    assert 15 <= fails <= 45
    acts, noise = F.draws(with_v, 7, 2)
    fg, fw = F.wrapped_forms(with_v, acts, noise, F.actor(with_v, 7)), F.wrapped_forms(without, acts, noise, F.actor(without, 7))
    for k in ("steps", "unroll", "policy"):
        _assert_same(fg[k], fw[k], (model, k), metrics=POSE_METRICS + F.FAIL_METRICS)
    for name in ("obs", "raw_action", "log_prob", "discount", "truncation"):
        assert torch.equal(getattr(fg["buf"], name), getattr(fw["buf"], name)), (model, name)


def _flat(s):
    d = {"ps." + k: v for k, v in s.pipeline_state.tree().items()}
    d.update(obs=s.obs, reward=s.reward, done=s.done)
    d.update({"metrics." + k: v for k, v in s.metrics.items()})
    d.update({"info." + k: s.info[k] for k in ("cur_frame", "restart_slot", "steps", "truncation", "clip") if k in s.info})
    return d


@pytest.mark.parametrize("model", MODELS)
def test_clip_restarts_in_one_launch_equal_the_composed_wrappers(model):
    """K = 3 with `end_at_clip_end`: the one-launch rollout (rr_restart_kernel) against `ClipEpisodeWrapper` + `ClipAutoResetWrapper`
    over the bare `step`, seven steps with episodes of three, every leaf of the final state bit for bit -- the three metrics included."""
    T = 104
    env = make_vel(model, T, clip_restarts=3, restart_frame_range=RANGE, end_at_clip_end=True, reset_to_reference=True)
    acts, _ = F.draws(env, 7, 2)
    comp = wrappers.ClipAutoResetWrapper(wrappers.ClipEpisodeWrapper(wrappers.VmapWrapper(env), 3, 1))
    s = comp.reset(F.keys(), clip=IDS)
    for t in range(7):
        s = comp.step(s, acts[t])
    fused = wrappers.wrap(env, episode_length=3, action_repeat=1)
    u = fused.unroll(fused.reset(F.keys(), clip=IDS), acts)
    torch.cuda.synchronize()
    a, b = _flat(u), _flat(s)
    assert set(a) == set(b) and {"metrics." + k for k in VEL_METRICS} <= set(a) and "info.restart_slot" in a
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (model, k)
    assert int(u.info["restart_slot"].max()) > 0 and float(u.metrics["joint_vel_reward"].min()) > 0


@pytest.mark.parametrize("model", MODELS)
def test_with_reference_frames_the_observation_is_the_envs_without_velocity(model):
    T = 104
    with_v, without = make_vel(model, T, reference_obs_frames=2), F.make(model, T, reference_obs_frames=2)
    acts, _ = F.draws(with_v, STEPS, 1)
    got, want = F.steps(with_v, acts), F.steps(without, acts)
    assert got[1].obs.shape[1] == with_v.sys.obs_dim + 2 * with_v.sys.nq
    for t in range(STEPS + 1):
        _assert_same(got[t], want[t], (model, t), reward=(t == 0))
        assert torch.equal(got[t].obs, want[t].obs)


# ---------------------------------------------------------------------------------------------- 6. bad state
@pytest.mark.parametrize("model", MODELS)
def test_a_bad_step_zeroes_the_velocity_terms(model):
    from rodent_amd.training import acting
    env = make_vel(model, 104, bad_state_max=1e10)
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
        for name in VEL_METRICS + POSE_METRICS:
            assert float(s.metrics[name][bad]) == 0.0, (model, k, name)
        assert float(s.reward[bad]) == 0.0 and float(s.done[bad]) == 1.0, (model, k)
        assert all(float(s.metrics[name][ok].min()) > 0 for name in VEL_METRICS) and float(s.done[ok].max()) == 0.0
    clean = env.step(env.reset(F.keys(), clip=IDS), acts[0])       # the other envs are untouched: what the step gives without the NaN
    for name in VEL_METRICS:
        assert torch.equal(res["step"].metrics[name][ok], clean.metrics[name][ok]), (model, name)
    assert torch.equal(res["step"].reward[ok], clean.reward[ok])
    assert float(buf.reward[0, bad, 0]) == 0.0 and float(buf.reward[0, ok, 0].min()) > 0
    assert env.bad_states() == 3


# ---------------------------------------------------------------------------------------------- 7. start state
@pytest.mark.parametrize("model", MODELS)
def test_reset_to_reference_starts_at_the_clips_velocity(model):
    T, K = 104, 3
    env = make_vel(model, T, clip_restarts=K, restart_frame_range=RANGE, reset_to_reference=True)
    nq, nv = env.sys.nq, env.sys.nv
    frames, _, noise, _ = rodent.restart_bank_draws(F.keys(), K, nq, nv, env._reset_noise_scale, RANGE, C)
    s = env.reset(F.keys(), clip=IDS)
    want = [rodent.reset_qvel(env._vel_host, frames[k], noise[k], IDS) for k in range(K)]
    assert np.array_equal(F.f32(s.pipeline_state.qvel), want[0]) and not np.array_equal(want[0], noise[0])
    bank = s.info["restart_bank"]
    for k in range(K):
        assert np.array_equal(F.f32(bank["pipeline_state"].qvel[k]), want[k]), (model, k)
        assert np.array_equal(bank["frame"][k].cpu().numpy(), frames[k])
    # three steps with episodes of three: an env whose third step ends its first episode comes out of the launch restored to bank entry 1
    wenv = wrappers.wrap(env, episode_length=3, action_repeat=1)
    u = wenv.unroll(wenv.reset(F.keys(), clip=IDS), F.draws(env, 3, 4)[0])
    torch.cuda.synchronize()
    hit = ((u.info["steps"] == 3) & (u.done == 1) & (u.info["restart_slot"] == 1)).cpu().numpy()
    assert hit.any(), (model, u.info["steps"], u.done)
    assert np.array_equal(F.f32(u.pipeline_state.qvel)[hit], want[1][hit]) and np.array_equal(u.info["cur_frame"].cpu().numpy()[hit], frames[1][hit])
    # without reset_to_reference: the bare noise
    rest = make_vel(model, T).reset(F.keys(), clip=IDS)
    assert np.array_equal(F.f32(rest.pipeline_state.qvel), noise[0])


# ---------------------------------------------------------------------------------------------- 8. refusals
def test_refusals():
    from rodent_amd import envs
    T = 104
    track = F.tracks(T)[0]
    v = ref_vel("rodent_optimized", T)[0]
    vel = dict(vel_kw("rodent_optimized", T), track_velocity=v[:, :3], track_angular_velocity=v[:, 3:6], track_joint_velocity=v[:, 6:])      # clip 0, the fixture's scales

    def build(model, pose=True, **kw):
        q0 = F.qpos0(model)
        if pose:
            kw.update(track_quat=np.tile([1.0, 0.0, 0.0, 0.0], (T, 1)), track_joints=np.tile(q0[7:], (T, 1)))
        return envs.get_environment("rodent", track_pos=track, num_envs=4, xml_path=f"{model}.xml", iterations=4, ls_iterations=4, n_frames=2,
                                    device=DEV, **kw)
    with pytest.raises(ValueError, match="track_quat and track_joints"):
        build("rodent_optimized", pose=False, **vel)
    with pytest.raises(RuntimeError, match=r"Rodent\(track_quat=..., track_joints=...\): .*Newton solver"):
        build("rodent_optimized", solver="newton", **vel)
    cpu = build("rodent_cpu", pose=False, healthy_z_range=(-0.3, 0.3))
    with pytest.raises(RuntimeError, match="candidate-pair contacts"):
        build("rodent_cpu", healthy_z_range=(-0.3, 0.3), track_velocity=np.zeros((T, 3)), track_angular_velocity=np.zeros((T, 3)),
              track_joint_velocity=np.zeros((T, cpu.sys.nv - 6)))
    # the library's own answers, on batches without a pose block
    assert "candidate-pair contacts" in cpu._batch.velocity_tracking_supported() and "candidate-pair contacts" in cpu._batch.velocity_tracking_supported(with_actor=True)
    assert "Newton solver" in build("rodent_optimized", pose=False, solver="newton")._batch.velocity_tracking_supported()
    plain = build("rodent_optimized", pose=False)
    assert plain._batch.velocity_tracking_supported() is None and plain._batch.velocity_tracking_supported(with_actor=True) is None
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)
    block = (dev(v), torch.zeros(4, 3, device=DEV))
    with pytest.raises(RuntimeError, match="needs a pose block"):
        plain._batch.set_velocity_tracking(*block)
    plain.set_env_params(dof_f=torch.zeros(4, plain.sys.nv, 16, device=DEV))      # a batch with per-env parameters
    assert "per-env parameters" in plain._batch.velocity_tracking_supported()
    with pytest.raises(RuntimeError, match="rr_batch_set_velocity_tracking: .*per-env parameters"):
        plain._batch.set_velocity_tracking(*block)
    env = build("rodent_optimized", **vel)
    assert not env.eval_supported()
    with pytest.raises(RuntimeError, match="per-env parameters"):
        env.randomize(lambda sys: (sys.replace(dof_damping=np.repeat(sys.dof_damping[None], 4, axis=0)), {"dof_damping": 0}))
    with pytest.raises(RuntimeError, match="per-env parameters"):
        env.set_env_params(dof_f=torch.zeros(4, env.sys.nv, 16, device=DEV))
    st = env.step(env.reset(jax_random.split(jax_random.PRNGKey(1), 4)), torch.zeros(4, env.action_size, device=DEV))      # still a working env
    assert float(st.metrics["joint_vel_reward"].min()) > 0
    b = env._batch      # the block stands on the batch after the step
    with pytest.raises(RuntimeError, match=r"velocity-tracking block.*clear it first"):
        b.set_pose(None)
    for bad in ((-1.0, 8.0), (1.0, float("nan")), (float("inf"), 1.0)):
        for key in ("lin_vel_reward", "ang_vel_reward", "joint_vel_reward"):
            with pytest.raises(RuntimeError, match="finite and >= 0"):
                b.set_velocity_tracking(*block, **{key: bad})
    with pytest.raises(RuntimeError, match="null track_vel or vel_metrics"):
        b.set_velocity_tracking(block[0], None)
    with pytest.raises(RuntimeError, match="no evaluation instance rewards the velocities"):
        env.unroll_eval(env.reset(jax_random.split(jax_random.PRNGKey(1), 4)), 2, F.actor(env, 1))


# ---------------------------------------------------------------------------------------------- 9. training
def test_ppo_train_on_a_velocity_env(monkeypatch):
    """One training step at 64 envs through the one-launch rollout (rr_env_unroll_policy on the body instance with the actor), evaluations
    by the per-step loop: finite losses and finite eval/episode_*_vel_reward next to the existing keys."""
    from rodent_amd.training import acting
    from rodent_amd.training.agents.ppo import train as ppo
    env = make_vel("rodent_optimized", 104, n=64, reset_to_reference=True)
    nets_ok = acting.fused_unroll_supported
    calls, log, asked = {"fused": 0}, [], []
    real_fused = acting.generate_unrolls_fused
    monkeypatch.setattr(acting, "generate_unrolls_fused", lambda *a, **k: (calls.__setitem__("fused", calls["fused"] + 1), real_fused(*a, **k))[1])
    monkeypatch.setattr(acting, "fused_unroll_supported", lambda *a, **k: (asked.append(nets_ok(*a, **k)), asked[-1])[1])
    ppo.train(environment=env, num_timesteps=10 ** 9, episode_length=10, num_envs=64, batch_size=64, num_minibatches=2, unroll_length=5,
              num_updates_per_batch=2, num_evals=2, num_eval_envs=6, learning_rate=5e-5, entropy_cost=1e-3, discounting=0.97,
              normalize_observations=True, seed=3, max_training_steps=1, progress_fn=lambda n, m: log.append(m))
    assert calls["fused"] == 1 and (not asked or all(asked))
    assert math.isfinite(float(log[-1]["training/total_loss"]))
    evals = [m for m in log if "eval/episode_reward" in m]
    assert len(evals) >= 2
    for m in evals:
        for k in ("eval/episode_reward", "eval/episode_quat_reward") + tuple("eval/episode_" + v for v in VEL_METRICS):
            assert k in m and math.isfinite(float(m[k])), k
        assert 0 < float(m["eval/episode_joint_vel_reward"]) <= 10 * VW[2]
