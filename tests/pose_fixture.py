"""The fixture the GPU tests of the pose family share: constants, clips, env builders, draws, actor, launch forms and the references
computed once per process.  No tests here.  N = 12 envs on C = 3 clips (env e on clip e % 3, explicit ids), n_frames 2, CG 4 / 4, five
steps; T = 104 and T = 3.  tests/test_gpu_pose.py describes the clips and says where the reward scales come from,
test_gpu_pose_termination.py the bounds of the three errors, test_gpu_body_tracking.py the reference bodies."""
import functools

import numpy as np
import torch

from rodent_amd import assets, jax_random, mjcf, preprocessing
from rodent_amd.envs import rodent
from rodent_amd.envs.graphed import tree_leaves as leaves      # the tensors of a state, in field order

DEV = "cuda:0"
N, C, STEPS = 12, 3, 5
SEED = 78            # start frames [42, 99, 35, 32, 33, 99, 10, 46, 47, 47, 19, 51]
IDS = np.arange(N) % C
MODELS = ["rodent_optimized", "rodent_0"]
EPS = 2.0 ** -24
W = (0.75, 0.5)                                  # quat_reward_weight, joint_reward_weight
QUAT_SCALE, JOINT_SCALE = {104: 5.0, 3: 12.0}, 0.6
ACTOR_REWARD_TOL = 2.5e-7                        # tests/test_gpu_ppo.py::test_one_launch_unroll_with_the_actor_inside: the actor instance's reward, one ulp
OLD_METRICS = ("pos_reward", "reward_quadctrl", "reward_alive")
FAIL_METRICS = ("pose_fail", "pose_fail_pos", "pose_fail_quat", "pose_fail_joint")
EFF = {"rodent_optimized": (11, 15, 59, 64, 54), "rodent_0": (11, 15, 59, 64, 54), "rodent_new": (12, 16, 60, 65, 55)}
AMP = 0.03
BW = (0.6, 0.4)                                   # body_reward_weight, endeff_reward_weight
SCALES = (8.0, 100.0)                             # body_reward_scale, endeff_reward_scale


def tracks(T):
    t = np.arange(T, dtype=np.float64)
    return np.stack([np.stack([0.004 * t, np.full(T, 0.1 * c), np.full(T, 0.0681 + 0.002 * c)], axis=1) for c in range(C)])


@functools.lru_cache(maxsize=None)
def qpos0(model):
    return mjcf.load_blob(assets.asset_path(model))["qpos0"].astype(np.float64)


def reference(model, T):
    """(quat [C, T, 4], joints [C, T, nq - 7]) of the fixture, float64."""
    q0 = qpos0(model)
    t, c, j = np.arange(T, dtype=np.float64), np.arange(C, dtype=np.float64), np.arange(len(q0) - 7, dtype=np.float64)
    ang = 0.1 * (c[:, None] + 1) + 0.003 * t[None]
    quat = np.stack([np.cos(ang / 2), np.zeros_like(ang), np.zeros_like(ang), np.sin(ang / 2)], axis=-1)
    joints = q0[7:][None, None] + 0.02 * np.sin(0.7 * j[None, None] + 0.05 * t[None, :, None] + c[:, None, None])
    return quat, joints


def make(model, T, n=N, pose=True, weights=W, **kw):
    from rodent_amd import envs
    if pose:
        quat, joints = reference(model, T)
        kw.update(track_quat=quat, track_joints=joints, quat_reward_weight=weights[0], quat_reward_scale=QUAT_SCALE[T],
                  joint_reward_weight=weights[1], joint_reward_scale=JOINT_SCALE)
    kw.setdefault("iterations", 4)
    return envs.get_environment("rodent", track_pos=tracks(T), num_envs=n, xml_path=f"{model}.xml", ls_iterations=4, n_frames=2, device=DEV, **kw)


def keys():
    return jax_random.split(jax_random.PRNGKey(SEED), N)


def draws(env, T, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    A = env.action_size
    return torch.rand(T, N, A, device=DEV, generator=gen) * 2 - 1, torch.randn(T, N, A, device=DEV, generator=gen)


def actor(env, seed):
    from rodent_amd.training import acting, networks, running_statistics
    torch.manual_seed(seed)
    nets = networks.make_ppo_networks(env.observation_size, env.action_size, device=DEV)
    net, dist = nets.policy_network, nets.parametric_action_distribution
    for l in net.layers:
        l.bias.data.uniform_(-0.3, 0.3)
    norm = running_statistics.init_state(env.observation_size, torch.device(DEV))
    norm.mean.copy_(torch.randn(env.observation_size, device=DEV) * 0.05)
    norm.std.copy_(torch.rand(env.observation_size, device=DEV) + 0.7)
    return acting.actor_params(net, norm, dist.min_std)


def steps(env, acts):
    """The reset state and the state after each plain `step`."""
    out = [env.reset(keys(), clip=IDS)]
    for t in range(acts.shape[0]):
        out.append(env.step(out[-1], acts[t]))
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def plain_steps(model, T):
    """Computed once per (model, T) and shared: (pose env, its states, the plain env's states) of five plain steps on the same keys,
    clips and actions."""
    pose_env, plain_env = make(model, T), make(model, T, pose=False)
    acts, _ = draws(pose_env, STEPS, 1)
    return pose_env, steps(pose_env, acts), steps(plain_env, acts)


def f32(x):
    return x.detach().cpu().numpy().astype(np.float32)


def traj(buf):
    return dict(obs=buf.obs[0], raw_action=buf.raw_action[0], log_prob=buf.log_prob[0], reward=buf.reward[0], discount=buf.discount[0],
                truncation=buf.truncation[0])


def wrapped_forms(env, acts, noise, actor):
    """Under Episode(3) + AutoReset: wrapped single steps, `unroll`, `unroll_policy` into trajectory buffers."""
    from rodent_amd.envs import wrappers
    from rodent_amd.training import acting
    wenv = wrappers.wrap(env, episode_length=3, action_repeat=1)
    s = wenv.reset(keys(), clip=IDS)
    for t in range(acts.shape[0]):
        s = wenv.step(s, acts[t])
    out = dict(steps=s, unroll=wenv.unroll(wenv.reset(keys(), clip=IDS), acts))
    buf = acting.UnrollBuffer(1, env.num_envs, acts.shape[0], env.observation_size, env.action_size, torch.device(DEV))
    out["policy"], out["policy_actions"] = wenv.unroll_policy(wenv.reset(keys(), clip=IDS), actor, noise, traj(buf))
    out["buf"] = buf
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def forms(model, T):
    """Computed once per (model, T) and shared: the wrapped forms of the pose env and of the plain env, seven steps with episodes of
    three (restores happen inside every launch)."""
    pose_env, plain_env = make(model, T), make(model, T, pose=False)
    assert pose_env._batch.unroll_supported(False) and pose_env._batch.unroll_supported(True)
    act = actor(pose_env, 7)
    acts, noise = draws(pose_env, 7, 2)
    return wrapped_forms(pose_env, acts, noise, act), wrapped_forms(plain_env, acts, noise, act)


def term_errors(env, T, qpos, old_frame):
    """`pose_errors` (float64) of the returned float32 `qpos` [N, nq] against the float32 rows the device holds, at the clip and the
    clamped frame the step's rewards read."""
    fi = np.clip(old_frame.cpu().numpy(), 0, T - 1)
    rows, tp = env._pose_host.astype(np.float64)[IDS, fi], env._track_host.astype(np.float64)[IDS, fi]
    return np.stack(rodent.pose_errors(qpos.cpu().numpy().astype(np.float64), tp, rows[:, :4], rows[:, 4:]))       # [3, N]


def term_bound(e):
    """Float32 error bounds of the three errors `e` [3, ...] (docstring of tests/test_gpu_pose_termination.py)."""
    return np.stack([2 * 5 * EPS * e[0], 2 * (22 + 4 * e[1]) * EPS, 2 * 7 * EPS * e[2]])


def mid_gap(e):
    """The middle of the widest gap between sorted ranks 15 and 45 of the 60 errors `e`: 15 .. 45 of them lie above it."""
    s = np.sort(np.asarray(e).ravel())
    assert s.size == 60
    i = 14 + int(np.argmax(np.diff(s)[14:45]))                # the gap s[i] .. s[i + 1], i = 14 .. 44: 59 - i = 15 .. 45 values above
    return 0.5 * (s[i] + s[i + 1])


@functools.lru_cache(maxsize=None)
def term_reference(model, T):
    """Computed once per (model, T) and shared: (pose env, its states of five bare steps, the errors [STEPS, 3, N] of those steps, the
    three thresholds)."""
    env, states, _ = plain_steps(model, T)
    errs = np.stack([term_errors(env, T, states[t].pipeline_state.qpos, states[t - 1].info["cur_frame"]) for t in range(1, STEPS + 1)])
    thr = tuple(float(mid_gap(errs[:, k])) for k in range(3))
    return env, states, errs, thr


def code_of(state):
    m = {k: state.metrics[k].cpu().numpy() for k in FAIL_METRICS}
    code = (m["pose_fail_pos"] + 2 * m["pose_fail_quat"] + 4 * m["pose_fail_joint"]).astype(np.int64)
    assert np.array_equal(m["pose_fail"], (code != 0).astype(np.float32))
    assert all(set(np.unique(v)) <= {0.0, 1.0} for v in m.values())
    return code


@functools.lru_cache(maxsize=None)
def pose_ref(model, T):
    """Computed once per (model, T) and shared: (the pose env WITHOUT bodies, pipeline outputs on; its states of five bare steps)."""
    env = make(model, T, pipeline_outputs=True)
    return env, steps(env, draws(env, STEPS, 1)[0])


@functools.lru_cache(maxsize=None)
def ref_bodies(model, T):
    """Reference body positions [C, T, nbody, 3], float64: forward kinematics of (track position, qpos0[3:]) plus the sine term."""
    q0, tr = qpos0(model), tracks(T)
    qpos = np.concatenate([tr, np.broadcast_to(q0[3:], tr.shape[:-1] + (len(q0) - 3,))], axis=-1).reshape(C * T, len(q0))
    base = preprocessing.extract_features(pose_ref(model, T)[0], qpos).body_positions.astype(np.float64)
    nbody = base.shape[1]
    b, k, t, c = np.arange(nbody)[None, None, :, None], np.arange(3)[None, None, None, :], np.arange(T)[None, :, None, None], np.arange(C)[:, None, None, None]
    return base.reshape(C, T, nbody, 3) + AMP * np.sin(0.9 * b + 1.7 * k + 0.05 * t + c)


def make_body(model, T, weights=BW, eff="fixture", **kw):
    return make(model, T, track_bodies=ref_bodies(model, T), end_effector_ids=EFF[model] if eff == "fixture" else eff,
                body_reward_weight=weights[0], body_reward_scale=SCALES[0], endeff_reward_weight=weights[1], endeff_reward_scale=SCALES[1], **kw)
