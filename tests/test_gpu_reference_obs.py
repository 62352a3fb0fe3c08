"""The reference observation on the GPU (`Rodent(reference_obs_frames=H)`; rr_batch_set_reference_obs, the rr_body_kernel instances):
every observation row carries the clip's next H frames behind the model's obs_dim entries.  Held against a pose env with H = 0 of the same
build -- bit for bit in everything but the new columns -- and against the float64 restatement `rodent.reference_obs`.

Fixture (tests/pose_fixture.py's; the reference, env builder, actor and step loop are its own): N = 12 envs, C = 3 clips, env e on clip e % 3 (explicit ids); n_frames = 2, solver
iterations 4 / 4, five steps.  T = 104 (start frames 0 .. 99: the two envs that start at frame 99 read past the clip's end) and T = 3
(every read clamps); H = 1 and H = 5.  Reference pose: the quaternion of clip c at frame t is a rotation about z by 0.1 (c + 1) + 0.003 t,
the joints are qpos0[7:] + 0.02 sin(0.7 j + 0.05 t + c); the quaternions of clip 1 are NEGATED, so the sign rule of q_h runs in both
branches."""
import functools
import math

import numpy as np
import pytest
import torch

from rodent_amd import jax_random
from rodent_amd.envs import rodent
from tests.pose_fixture import C, DEV, EPS, IDS, MODELS, N, STEPS, draws, keys, leaves, qpos0, tracks

pytestmark = pytest.mark.gpu
CASES = [(m, T, H) for m in MODELS for T in (104, 3) for H in (1, 5)]


def _reference(model, T):
    """(quat [C, T, 4], joints [C, T, nq - 7]) of the fixture, float64; clip 1's quaternions negated."""
    q0 = qpos0(model)
    t, c, j = np.arange(T, dtype=np.float64), np.arange(C, dtype=np.float64), np.arange(len(q0) - 7, dtype=np.float64)
    ang = 0.1 * (c[:, None] + 1) + 0.003 * t[None]
    quat = np.stack([np.cos(ang / 2), np.zeros_like(ang), np.zeros_like(ang), np.sin(ang / 2)], axis=-1)
    quat[1] = -quat[1]
    joints = q0[7:][None, None] + 0.02 * np.sin(0.7 * j[None, None] + 0.05 * t[None, :, None] + c[:, None, None])
    return quat, joints


def _make(model, T, H=0, n=N, pose=True, n_frames=2, **kw):
    from rodent_amd import envs
    if pose:
        quat, joints = _reference(model, T)
        kw.update(track_quat=quat, track_joints=joints, quat_reward_weight=0.75, quat_reward_scale=5.0, joint_reward_weight=0.5, joint_reward_scale=0.6)
    if H:
        kw["reference_obs_frames"] = H
    return envs.get_environment("rodent", track_pos=tracks(T), num_envs=n, xml_path=f"{model}.xml", iterations=4, ls_iterations=4, n_frames=n_frames,
                                device=DEV, **kw)


def _actor(env, seed):
    from rodent_amd.training import acting, networks, running_statistics
    torch.manual_seed(seed)
    nets = networks.make_ppo_networks(env.observation_size, env.action_size, device=DEV)
    net, dist = nets.policy_network, nets.parametric_action_distribution
    for l in net.layers:
        l.bias.data.uniform_(-0.3, 0.3)
    # the reference columns at eight times the default initialisation (uniform within 1 / sqrt(W) = 0.027): H = 1 adds 74 columns to
    # 1263, and the raw action has to respond to them well above the rounding bounds of test_the_actor_inside_reads_the_whole_row
    net.layers[0].weight.data[:, env.sys.obs_dim:] *= 8.0
    norm = running_statistics.init_state(env.observation_size, torch.device(DEV))
    norm.mean.copy_(torch.randn(env.observation_size, device=DEV) * 0.05)
    norm.std.copy_(torch.rand(env.observation_size, device=DEV) + 0.7)
    return acting.actor_params(net, norm, dist.min_std), net, norm, dist


def _steps(env, acts, pre=None):
    """The reset state and the state after each plain `step`.  `pre` (an env of n_frames = 1): also the qpos after the FIRST substep of
    every step, which is what the last forward pass of the two-substep step sees (list aligned with the states; entry 0 is None)."""
    out, first = [env.reset(keys(), clip=IDS)], [None]
    for t in range(acts.shape[0]):
        if pre is not None:
            first.append(pre.step(out[-1], acts[t]).pipeline_state.qpos)
        out.append(env.step(out[-1], acts[t]))
    torch.cuda.synchronize()
    return out, first


@functools.lru_cache(maxsize=None)
def _base_steps(model, T):
    """Shared by the H cases of (model, T): the H = 0 pose env's states of five plain steps, and the qpos after the first substep of each."""
    env = _make(model, T)
    acts, _ = draws(env, STEPS, 1)
    return _steps(env, acts, _make(model, T, pose=False, n_frames=1))


@functools.lru_cache(maxsize=None)
def _ref_steps(model, T, H):
    env = _make(model, T, H)
    acts, _ = draws(env, STEPS, 1)
    return env, _steps(env, acts)[0]


def _wrapped(env, acts):
    """Under Episode(3) + AutoReset: the states of wrapped single steps, and the state `unroll` leaves."""
    from rodent_amd.envs import wrappers
    wenv = wrappers.wrap(env, episode_length=3, action_repeat=1)
    steps = [wenv.reset(keys(), clip=IDS)]
    for t in range(acts.shape[0]):
        steps.append(wenv.step(steps[-1], acts[t]))
    unroll = wenv.unroll(wenv.reset(keys(), clip=IDS), acts)
    unroll3 = wenv.unroll(wenv.reset(keys(), clip=IDS), acts[:3].contiguous())
    torch.cuda.synchronize()
    return dict(steps=steps, unroll=unroll, unroll3=unroll3)


@functools.lru_cache(maxsize=None)
def _base_wrapped(model, T):
    env = _make(model, T)
    return _wrapped(env, draws(env, STEPS, 2)[0])


@functools.lru_cache(maxsize=None)
def _ref_wrapped(model, T, H):
    env = _make(model, T, H)
    return env, _wrapped(env, draws(env, STEPS, 2)[0])


def _assert_same_but_the_blocks(got, want, K, Wd, what):
    """Every leaf of the two states bit for bit; a leaf that is an observation (last axis Wd wide in `got`, K in `want`: obs, first_obs)
    in its first K columns."""
    la, lb = leaves(got), leaves(want)
    assert len(la) == len(lb) > 10, (what, len(la), len(lb))
    wide = 0
    for i, (x, y) in enumerate(zip(la, lb)):
        if x.dim() == 2 and x.shape[1] == Wd and y.shape[1] == K:
            x, wide = x[:, :K], wide + 1
        assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), (what, i, tuple(x.shape), int((x != y).sum()))
    return wide


def _f64(x):
    return x.detach().cpu().numpy().astype(np.float64)


# ---------------------------------------------------------------------------------------------- 1. nothing else moves
@pytest.mark.parametrize("model,T,H", CASES)
def test_everything_but_the_new_columns_is_the_pose_env(model, T, H):
    env, got = _ref_steps(model, T, H)
    want, _ = _base_steps(model, T)
    K, nq = env.sys.obs_dim, env.sys.nq
    assert env.observation_size == K + H * nq == env._batch.obs_width() and env.reference_obs_frames == H
    for t, (g, w) in enumerate(zip(got, want)):
        assert g.obs.shape == (N, K + H * nq) and w.obs.shape == (N, K)
        assert _assert_same_but_the_blocks(g, w, K, K + H * nq, (model, T, H, "step", t)) == 1
    fg, fw = _ref_wrapped(model, T, H)[1], _base_wrapped(model, T)
    for t, (g, w) in enumerate(zip(fg["steps"], fw["steps"])):
        assert _assert_same_but_the_blocks(g, w, K, K + H * nq, (model, T, H, "wrapped step", t)) == 2       # obs and info.first_obs
    for k in ("unroll", "unroll3"):
        assert _assert_same_but_the_blocks(fg[k], fw[k], K, K + H * nq, (model, T, H, k)) == 2
    frames = got[-1].info["cur_frame"].cpu().numpy()
    if T == 104:
        assert (frames + H > T - 1).sum() >= 2 and (frames + H < T - 1).sum() >= 6         # reads past the clip's end / inside the clip


# ---------------------------------------------------------------------------------------------- 2. the blocks
@pytest.mark.parametrize("model,T,H", CASES)
def test_blocks_against_the_float64_restatement(model, T, H):
    """Each block of every row -- at reset and after each of the five steps -- against `reference_obs` in float64 on the state's own
    float32 qpos, the float32 tables the device holds and the state's cur_frame.

    x, the world quaternion of body 1 the epilogue holds, is the free joint's quaternion as the LAST FORWARD PASS normalised it: at reset
    that of the state's qpos, after a step that of the qpos after the step's first substep (n_frames = 2), which an env of one substep
    per step returns.  The test normalises that float32 quaternion in float64; the kernel in float32: sum of four squares (4 eps
    relative), square root (half of that and its own: 3 eps), reciprocal and product (2 eps) -- each component within 5 eps of the
    test's, rounded up to 6.  eps = 2^-24; factor 2 on every bound for the slack of a first-order count, as tests/test_gpu_pose.py.

    j_h: one subtraction of two float32 numbers -- bit for bit.  p_1: the three entries before the blocks -- bit for bit.  q_h.w >= 0.
    q_h: each component is a sum of four products whose magnitudes sum to at most s = |x||r|: four products and three additions, 4 eps s,
    and x's 6 eps s; bound 2 * 10 eps s.
    p_h = R(x) v, v = track_pos[f_h] - qpos[:3]: the subtraction (eps |v_i| per component) and the row's three products and two
    additions (3 eps |v|) give 4 eps |v|; an entry of R is a sum of at most four products of magnitudes summing to <= |x|^2 = 1 (4 eps)
    and moves by 2 * 6 eps with x: 16 eps |v|_1; bound 2 eps (4 |v|_2 + 16 |v|_1).
    The wrong row must miss: with the neighbouring frame, the neighbouring clip and the joint row shifted by one index, the largest
    error-to-bound ratio over the samples (for j: the error in units of eps max|j|) is at least 100."""
    env, states = _ref_steps(model, T, H)
    _, first = _base_steps(model, T)
    K, nq = env.sys.obs_dim, env.sys.nq
    tp = env._track_host.astype(np.float64)
    rows = env._pose_host.astype(np.float64)
    assert rows.shape == (C, T, nq - 3) and (rows[1, :, 0] < 0).all() and (rows[0, :, 0] > 0).all()
    worst = dict(p=0.0, q=0.0)
    alt = {k: dict(p=0.0, q=0.0, j=0.0) for k in ("frame", "clip", "shift")}
    flipped = 0
    for t, s in enumerate(states):
        obs = s.obs.cpu().numpy()
        qpos32 = s.pipeline_state.qpos.cpu().numpy()
        qpos = qpos32.astype(np.float64)
        frame = s.info["cur_frame"].cpu().numpy()
        xq = qpos[:, 3:7] if t == 0 else _f64(first[t])[:, 3:7]
        x = xq / np.linalg.norm(xq, axis=1, keepdims=True)
        blocks = obs[:, K:].reshape(N, H, nq)
        assert np.array_equal(blocks[:, 0, :3], obs[:, K - 3:K]), (model, T, H, t)                   # p_1 IS the track entry
        assert (blocks[:, :, 3] >= 0).all(), (model, T, H, t)

        def restated(tq, tj, fr, ids):
            return rodent.reference_obs(qpos, tp, tq, tj, fr, H, clip=ids, xquat=x).reshape(N, H, nq)
        want = restated(rows[..., :4], rows[..., 4:], frame, IDS)
        fh = np.clip(frame[:, None] + np.arange(1, H + 1)[None], 0, T - 1)
        r32 = env._pose_host[IDS[:, None], fh]                                                         # float32 [N, H, nq - 3]
        assert np.array_equal(blocks[:, :, 7:], r32[:, :, 4:] - qpos32[:, None, 7:]), (model, T, H, t)   # j_h: one float32 subtraction
        v = tp[IDS[:, None], fh] - qpos[:, None, :3]
        bound_p = 2 * EPS * (4 * np.linalg.norm(v, axis=-1) + 16 * np.abs(v).sum(-1))
        bound_q = 2 * EPS * 10 * np.linalg.norm(x, axis=1)[:, None] * np.linalg.norm(rows[IDS[:, None], fh][..., :4], axis=-1)
        err_p = np.abs(blocks[:, :, :3] - want[:, :, :3]).max(-1)
        err_q = np.abs(blocks[:, :, 3:7] - want[:, :, 3:7]).max(-1)
        worst["p"] = max(worst["p"], float((err_p / bound_p).max()))
        worst["q"] = max(worst["q"], float((err_q / bound_q).max()))
        flipped += int(((x[:, None] * rows[IDS[:, None], fh][..., :4]).sum(-1) < 0).sum())
        # wrong rows.  A neighbouring frame INSIDE the clip: frame - 1 where the reads clamp at the end
        other_frame = np.where(frame + H + 1 <= T - 1, frame + 1, np.minimum(frame, T - 1 - H) - 1)
        shifted = np.roll(rows[..., 4:], 1, axis=-1)
        unit_j = EPS * np.abs(want[:, :, 7:]).max()
        for name, o in (("frame", restated(rows[..., :4], rows[..., 4:], other_frame, IDS)), ("clip", restated(rows[..., :4], rows[..., 4:], frame, (IDS + 1) % C)),
                        ("shift", restated(rows[..., :4], shifted, frame, IDS))):
            alt[name]["p"] = max(alt[name]["p"], float((np.abs(blocks[:, :, :3] - o[:, :, :3]).max(-1) / bound_p).max()))
            alt[name]["q"] = max(alt[name]["q"], float((np.abs(blocks[:, :, 3:7] - o[:, :, 3:7]).max(-1) / bound_q).max()))
            alt[name]["j"] = max(alt[name]["j"], float(np.abs(blocks[:, :, 7:] - o[:, :, 7:]).max() / unit_j))
    print(f"{model} T={T} H={H}: largest |error| / bound: p_h {worst['p']:.3f}, q_h {worst['q']:.3f}; wrong rows miss by (p, q, j): "
          f"frame {alt['frame']['p']:.0f} {alt['frame']['q']:.0f} {alt['frame']['j']:.0f}, clip {alt['clip']['p']:.0f} {alt['clip']['q']:.0f} "
          f"{alt['clip']['j']:.0f}, joint shift {alt['shift']['j']:.0f}; sign flips {flipped}")
    assert worst["p"] <= 1.0 and worst["q"] <= 1.0, worst
    assert flipped >= 4 * H * (STEPS + 1)                     # clip 1's four envs, every block of every row
    for name in ("frame", "clip"):
        assert min(alt[name].values()) >= 100, (name, alt[name])
    assert alt["shift"]["j"] >= 100 and alt["shift"]["p"] <= 1.0 and alt["shift"]["q"] <= 1.0, alt["shift"]


# ---------------------------------------------------------------------------------------------- 3. launch forms
@pytest.mark.parametrize("model,T,H", CASES)
def test_single_step_and_multi_step_agree_and_restores_are_verbatim(model, T, H):
    env, f = _ref_wrapped(model, T, H)
    a, b = f["steps"][-1], f["unroll"]
    la, lb = leaves(a), leaves(b)
    assert len(la) == len(lb) > 10
    for i, (x, y) in enumerate(zip(la, lb)):
        assert x.shape == y.shape and torch.equal(x, y), (model, T, H, i)
    Wd = env.observation_size
    s3 = f["steps"][3]                                        # episodes of three steps: every env is restored after the third
    assert float(s3.done.min()) == 1.0 and s3.obs.shape == (N, Wd) and torch.equal(s3.obs, s3.info["first_obs"])
    u3 = f["unroll3"]                                         # ... and by the multi-step instance itself
    assert float(u3.done.min()) == 1.0 and u3.obs.shape == (N, Wd) and torch.equal(u3.obs, u3.info["first_obs"])
    assert torch.equal(u3.obs, f["steps"][0].obs) and not torch.equal(f["steps"][2].obs[:, -H * env.sys.nq:], s3.obs[:, -H * env.sys.nq:])
    assert torch.equal(u3.info["cur_frame"], f["steps"][0].info["cur_frame"] + 3)      # info is not restored


# ---------------------------------------------------------------------------------------------- 4. the actor inside
PPO_RAW_TOL, PPO_ACTION_TOL, PPO_LOGP_TOL = 2e-5, 2e-5, 2e-3        # tests/test_gpu_ppo.py::test_one_launch_unroll_with_the_actor_inside, at K = 1279


@pytest.mark.parametrize("model,T,H", CASES)
def test_the_actor_inside_reads_the_whole_row(model, T, H):
    """rr_env_unroll_policy on the reference-observation instance, six steps recorded as two segments of three, episodes of three steps:
    (1) replaying the recorded actions through the wrapped per-step path reproduces every traj_obs row bit for bit; (2) raw actions and
    log-probs are those of the two-launch actor (`hip.policy_act`) on the recorded rows within the bounds of tests/test_gpu_ppo.py scaled
    by W / 1279, the length of the first layer's sum; (3) with w0's reference columns zeroed the raw action of the first step moves by
    at least 100 of those bounds: the in-kernel actor reads the columns behind obs_dim (with H = 5 up to entry 1633, past the 1280 the other
    instances' actor reads)."""
    from rodent_amd import hip
    from rodent_amd.envs import wrappers
    from rodent_amd.training import acting, fused_mlp
    env = _make(model, T, H)
    K, Wd, A = env.sys.obs_dim, env.observation_size, env.action_size
    actor, net, norm, dist = _actor(env, 7)
    wenv = wrappers.wrap(env, episode_length=3, action_repeat=1)
    assert acting.fused_unroll_supported(wenv, net, dist) and env._batch.reference_obs_supported(H, with_actor=True) is None
    _, noise = draws(env, 6, 3)

    def launch(act):
        buf = acting.UnrollBuffer(2, N, 3, Wd, A, torch.device(DEV))
        traj = dict(obs=buf.obs, raw_action=buf.raw_action, log_prob=buf.log_prob, reward=buf.reward, discount=buf.discount, truncation=buf.truncation)
        st, actions = wenv.unroll_policy(wenv.reset(keys(), clip=IDS), act, noise, traj, segment=3)
        torch.cuda.synchronize()
        return buf, st, actions
    buf, got, actions = launch(actor)
    assert torch.isfinite(buf.obs).all() and torch.isfinite(buf.log_prob).all() and buf.obs.shape == (2, N, 4, Wd)
    # (1)
    st = wenv.reset(keys(), clip=IDS)
    for s in range(6):
        assert torch.equal(buf.obs[s // 3, :, s % 3], st.obs), (model, T, H, s)
        st = wenv.step(st, actions[s])
        if s % 3 == 2:
            assert torch.equal(buf.obs[s // 3, :, 3], st.obs), (model, T, H, s)
    assert torch.equal(got.obs, st.obs) and torch.equal(got.pipeline_state.qpos, st.pipeline_state.qpos)
    assert bool((buf.discount == 0).any())                   # episodes ended inside the launch: restored rows were recorded
    # (2)
    scale = Wd / 1279.0
    obs_t = buf.obs[:, :, :3].permute(0, 2, 1, 3).reshape(6 * N, Wd).contiguous()            # [u][t][n] = step-major, as the noise
    act, raw, lp, _ = hip.policy_act(obs_t, norm.mean, norm.std, fused_mlp.net_params(net), noise.reshape(6 * N, -1).contiguous(), dist.min_std)
    raw_k = buf.raw_action.permute(0, 2, 1, 3).reshape(6 * N, A)
    lp_k = buf.log_prob.permute(0, 2, 1).reshape(-1)
    raw_bound = PPO_RAW_TOL * scale * max(1.0, float(raw.abs().max()))
    e_raw, e_act, e_lp = float((raw_k - raw).abs().max()), float((actions.reshape(6 * N, A) - act).abs().max()), float((lp_k - lp).abs().max())
    print(f"{model} T={T} H={H}: W = {Wd}; |raw - policy_act| {e_raw:.3g} (bound {raw_bound:.3g}), actions {e_act:.3g} (bound {PPO_ACTION_TOL * scale:.3g}), "
          f"log-prob {e_lp:.3g} (bound {PPO_LOGP_TOL * scale:.3g})")
    assert e_raw <= raw_bound and e_act <= PPO_ACTION_TOL * scale and e_lp <= PPO_LOGP_TOL * scale
    # (3)
    blind = dict(actor)
    blind["w0"] = actor["w0"].clone()
    blind["w0"][:, K:] = 0.0
    buf0, _, _ = launch(blind)
    moved = float((buf0.raw_action[0, :, 0] - buf.raw_action[0, :, 0]).abs().max())
    print(f"{model} T={T} H={H}: zeroed reference columns move the first raw action by {moved:.3g} = {moved / raw_bound:.0f} bounds")
    assert torch.equal(buf0.obs[0, :, 0], buf.obs[0, :, 0]) and moved >= 100 * raw_bound


# ---------------------------------------------------------------------------------------------- 5. refusals
def test_refusals():
    from rodent_amd import hip
    from rodent_amd.envs import wrappers
    from rodent_amd.training import acting
    with pytest.raises(ValueError, match="track_quat and track_joints"):
        _make("rodent_optimized", 104, pose=False, reference_obs_frames=1)
    with pytest.raises(ValueError, match=r"\[0, 16\]"):
        _make("rodent_optimized", 104, H=17)
    plain = _make("rodent_optimized", 104, pose=False)
    with pytest.raises(RuntimeError, match="need a pose block"):                  # frames without a pose block
        plain._batch.set_reference_obs(1)
    assert plain._batch.obs_width() == plain.sys.obs_dim
    env = _make("rodent_optimized", 104, H=2)
    with pytest.raises(RuntimeError, match=r"0 \.\. 16"):                          # frames = 17
        env._batch.set_reference_obs(17)
    with pytest.raises(RuntimeError, match="carries reference frames"):           # clearing pose while frames are set
        env._batch.set_pose(None)
    assert env._batch.obs_width() == env.sys.obs_dim + 2 * env.sys.nq             # ... and both refusals left the batch as it was
    keys4 = jax_random.split(jax_random.PRNGKey(1), N)
    with pytest.raises(RuntimeError, match="no evaluation instance writes the reference observation"):
        env.unroll_eval(env.reset(keys4, clip=IDS), 2, _actor(env, 1)[0])
    assert not env.eval_supported()
    with pytest.raises(RuntimeError, match="Newton solver"):
        _make("rodent_optimized", 104, H=1, solver="newton")
    # H = 6: 1263 + 6 * 74 = 1707 entries -- wider than the 1664 the in-kernel actor reads; the forms without the actor serve it
    env6 = _make("rodent_optimized", 104, H=6)
    W6 = env6.sys.obs_dim + 6 * env6.sys.nq
    assert env6.observation_size == W6 == 1707
    why = env6._batch.reference_obs_supported(6, with_actor=True)
    assert why is not None and "1664" in why and env6._batch.reference_obs_supported(6) is None
    assert env6._batch.reference_obs_supported(5, with_actor=True) is None and env6._batch.reference_obs_supported(16) is None
    actor, net, _, dist = _actor(env6, 2)
    wenv6 = wrappers.wrap(env6, episode_length=3, action_repeat=1)
    assert not acting.fused_unroll_supported(wenv6, net, dist)
    acts, noise = draws(env6, 2, 4)
    s = wenv6.step(wenv6.reset(keys(), clip=IDS), acts[0])                        # `step` works
    assert s.obs.shape == (N, W6) and torch.isfinite(s.obs).all()
    u = wenv6.unroll(wenv6.reset(keys(), clip=IDS), acts[:1].contiguous())
    assert torch.equal(u.obs, s.obs)
    buf = acting.UnrollBuffer(1, N, 2, W6, env6.action_size, torch.device(DEV))
    traj = dict(obs=buf.obs[0], raw_action=buf.raw_action[0], log_prob=buf.log_prob[0], reward=buf.reward[0], discount=buf.discount[0], truncation=buf.truncation[0])
    with pytest.raises(RuntimeError, match="wider than 1664"):
        wenv6.unroll_policy(wenv6.reset(keys(), clip=IDS), actor, noise, traj)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 6. the learner's forward at the new widths
@pytest.mark.parametrize("K", [1353, 1649])
def test_mlp_forward_at_the_new_widths(K):
    """rr_mlp_forward at 1279 + 74 and 1279 + 5 * 74 columns, 200 rows, by the criterion tests/test_gpu_mlp.py applies at 1279
    (test_single_network_calls_and_no_normaliser)."""
    from rodent_amd import hip
    from rodent_amd.training import networks
    M = 200
    torch.manual_seed(K)
    obs = torch.randn(M, K, device=DEV)
    n = networks.make_ppo_networks(K, 30, policy_hidden_layer_sizes=(32,) * 2, value_hidden_layer_sizes=(256,) * 3, device=DEV)
    for net in (n.policy_network, n.value_network):
        for lin in net.layers:
            torch.nn.init.uniform_(lin.bias, -0.1, 0.1)
    wb = lambda net: ([l.weight.detach() for l in net.layers], [l.bias.detach() for l in net.layers])

    def ref(x, net):
        ws, bs = wb(net)
        for i, (w, b) in enumerate(zip(ws, bs)):
            x = x @ w.t() + b
            if i < len(ws) - 1:
                x = torch.nn.functional.silu(x)
        return x
    both = hip.mlp_forward(obs, None, None, wb(n.policy_network), wb(n.value_network))
    only_p = hip.mlp_forward(obs, None, None, policy=wb(n.policy_network))
    only_v = hip.mlp_forward(obs, None, None, value=wb(n.value_network))
    assert torch.equal(both[0], only_p[0]) and torch.equal(both[1], only_v[1]) and only_p[1] is None and only_v[0] is None
    err = float((both[0] - ref(obs, n.policy_network)).abs().max())
    print(f"K={K}: |rr_mlp_forward - torch float32| policy {err:.3g}")
    assert err < 1e-4


# ---------------------------------------------------------------------------------------------- 7. bad state
@pytest.mark.parametrize("model", MODELS)
def test_a_bad_step_ends_the_episode_and_the_restored_row_is_finite(model):
    from rodent_amd.envs import wrappers
    env = _make(model, 104, H=5, bad_state_max=1e10)
    bad = 4

    def poison(state):       # NaN into a COPY of the incoming qvel (the stored first state shares the reset's tensors)
        qvel = state.pipeline_state.qvel.clone()
        qvel[bad, 3] = float("nan")
        return state.replace(pipeline_state=state.pipeline_state.replace(qvel=qvel))
    acts, _ = draws(env, 1, 3)
    wenv = wrappers.wrap(env, episode_length=100, action_repeat=1)
    s = env.step(poison(env.reset(keys(), clip=IDS)), acts[0])
    w0 = wenv.reset(keys(), clip=IDS)
    u = wenv.unroll(poison(w0), acts)
    torch.cuda.synchronize()
    ok = [e for e in range(N) if e != bad]
    for k, st in (("step", s), ("unroll", u)):
        assert float(st.done[bad]) == 1.0 and float(st.reward[bad]) == 0.0 and float(st.done[ok].max()) == 0.0, (model, k)
        assert torch.isfinite(st.obs[ok]).all(), (model, k)
    assert not torch.isfinite(s.obs[bad]).all()                        # the bare step does not sanitise
    assert torch.isfinite(u.obs[bad]).all() and torch.equal(u.obs[bad], w0.obs[bad]) and u.obs.shape[1] == env.observation_size
    assert env.bad_states() == 2


# ---------------------------------------------------------------------------------------------- 8. training
def test_ppo_train_with_five_reference_frames(monkeypatch):
    """One training step at 64 envs with H = 5 (1263 + 370 = 1633 columns) through the one-launch rollout: `fused_unroll_supported` says yes, the
    rollout runs as one launch, and the losses are finite."""
    from rodent_amd.training import acting
    from rodent_amd.training.agents.ppo import train as ppo
    env = _make("rodent_optimized", 104, H=5, n=64)
    assert env.observation_size == env.sys.obs_dim + 5 * env.sys.nq == 1633
    calls, log, said = {"fused": 0}, [], []
    real_fused, real_supported = acting.generate_unrolls_fused, acting.fused_unroll_supported
    monkeypatch.setattr(acting, "generate_unrolls_fused", lambda *a, **k: (calls.__setitem__("fused", calls["fused"] + 1), real_fused(*a, **k))[1])
    monkeypatch.setattr(acting, "fused_unroll_supported", lambda *a, **k: (said.append(real_supported(*a, **k)), said[-1])[1])
    ppo.train(environment=env, num_timesteps=10 ** 9, episode_length=10, num_envs=64, batch_size=64, num_minibatches=2, unroll_length=5,
              num_updates_per_batch=2, num_evals=1, num_eval_envs=6, learning_rate=5e-5, entropy_cost=1e-3, discounting=0.97,
              normalize_observations=True, seed=3, max_training_steps=1, progress_fn=lambda n, m: log.append(m))
    assert said and all(said) and calls["fused"] == 1
    losses = [m for m in log if "training/total_loss" in m]
    assert losses
    for k in ("training/total_loss", "training/policy_loss", "training/v_loss"):
        if k in losses[-1]:
            assert math.isfinite(float(losses[-1][k])), k
    assert math.isfinite(float(losses[-1]["training/total_loss"]))
