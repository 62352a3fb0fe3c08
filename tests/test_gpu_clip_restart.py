"""Clip restarts on the GPU (`Rodent(clip_restarts=K, restart_frame_range=, end_at_clip_end=)`; rr_batch_set_clip_restarts, the
rr_restart_kernel instances, rr_wrap_clip_restart): the three wrapped forms against the two composed wrappers in plain torch
(`ClipEpisodeWrapper`, `ClipAutoResetWrapper`), bit for bit.

Fixture: that of tests/test_gpu_pose.py (3 clips, env e on clip e % 3, n_frames 2, CG 4/4, its reference pose and reset noise) enlarged to
32 envs, T = 104, episodes of 5 steps, 14 steps: the smallest shapes at which slot arithmetic, bank strides and the two observation widths
can go wrong.  Bank entries 1 .. K - 1 start in frames [90, 102), so they meet the clip's end (new_frame >= 103) within an episode.

SEED 94 was chosen on the host, from the draws alone (`_schedule_counts`, integer bookkeeping of the rule on an env that never ends by
itself): with K = 1 the 448 (env, step) pairs hold 60 restores by `episode_length` and 8 by the clip's end, with K = 3 63 and 20 -- each
between 8 and three quarters of the pairs.  Start frames of entry 0: 99 twice, 98 once, 91 twice, 0 once.

THRESHOLDS of the cases with pose termination come from the data, not from the code under test, as in
tests/test_gpu_pose_termination.py: the K = 3 env WITHOUT termination makes the 14 composed wrapped steps, `pose_errors` gives the 448
errors per criterion from the stepped qpos (taken before the restore), and each threshold stands in the widest gap between the sorted
ranks 70 % .. 80 % (each criterion alone fires in 20 % .. 30 % of those pairs: low enough for episodes to reach `episode_length` and
the clip's end as well).  The failures of the run WITH the thresholds are then counted on the float64 restatement (`pose_fail_code` of
the recorded stepped states) and must lie in 25 % .. 75 % of the pairs.  The device decides `error > threshold` in float32; its code is
compared with the restatement wherever the error is further from the threshold than 100 float32 bounds (`pose_fixture.term_bound`)."""
import functools
import math

import numpy as np
import pytest
import torch

from rodent_amd import jax_random
from rodent_amd.envs import rodent, wrappers
from tests import pose_fixture as F
from tests.pose_fixture import DEV

pytestmark = pytest.mark.gpu
N, C, T, L, STEPS = 32, 3, 104, 5, 14
SEED, RANGE = 94, (90, 102)
IDS = np.arange(N) % C
# (model, K, H, body tracking, pose termination): K in {1, 3}, H in {0, 5}, with and without bodies and thresholds on the fixed-dimension
# root-slot model and on the generic dims; rodent_new (nbody 67) for one case
CASES = [("rodent_optimized", 1, 0, False, False), ("rodent_optimized", 3, 5, True, True), ("rodent_optimized", 3, 0, False, True),
         ("rodent_0", 1, 5, True, False), ("rodent_0", 3, 0, True, True), ("rodent_0", 3, 5, False, False), ("rodent_new", 3, 5, True, True)]


# ---------------------------------------------------------------------------------------------- the fixture
def _keys():
    return jax_random.split(jax_random.PRNGKey(SEED), N)


def _schedule_counts(K, steps=STEPS, end=True):
    """(restores caused by `episode_length`, restores caused by the clip's end) among the N x steps pairs of an env that never ends by
    itself, from the host draws alone; a pair where both hold counts in both."""
    frames = rodent.restart_bank_draws(_keys(), K, 74, 73, 0.01, RANGE if K > 1 else (0, 100), C)[0]
    by_len = by_end = 0
    for e in range(N):
        f, slot, n = int(frames[0, e]), 0, 0
        for _ in range(steps):
            n, nf = n + 1, f + 1
            a, b = n >= L, end and nf >= T - 1
            by_len, by_end = by_len + a, by_end + b
            if a or b:
                slot = (slot + 1) % K
                f, n = int(frames[slot, e]), 0
            else:
                f = nf
    return by_len, by_end


def _make(model, K, H=0, bodies=False, thr=None, end=None, **kw):
    if K:
        kw.update(clip_restarts=K, end_at_clip_end=(True if end is None else end))
    if K > 1:
        kw.update(restart_frame_range=RANGE)
    if H:
        kw.update(reference_obs_frames=H)
    if bodies:
        kw.update(track_bodies=F.ref_bodies(model, T), end_effector_ids=F.EFF[model], body_reward_weight=F.BW[0], body_reward_scale=F.SCALES[0],
                  endeff_reward_weight=F.BW[1], endeff_reward_scale=F.SCALES[1])
    if thr is not None:
        kw.update(max_pos_error=thr[0], max_quat_error=thr[1], max_joint_error=thr[2])
    frames = kw.pop("frames", T)
    if frames == T:
        return F.make(model, T, n=N, **kw)
    from rodent_amd import envs          # the same fixture on a clip of another length (tests/test_gpu_pose.py has scales for T = 104 and 3 only)
    quat, joints = F.reference(model, frames)
    return envs.get_environment("rodent", track_pos=F.tracks(frames), num_envs=N, xml_path=f"{model}.xml", iterations=4, ls_iterations=4, n_frames=2,
                                device=DEV, track_quat=quat, track_joints=joints, quat_reward_weight=F.W[0], quat_reward_scale=F.QUAT_SCALE[T],
                                joint_reward_weight=F.W[1], joint_reward_scale=F.JOINT_SCALE, **kw)


def _draws(env, steps, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    A = env.action_size
    return torch.rand(steps, N, A, device=DEV, generator=gen) * 2 - 1, torch.randn(steps, N, A, device=DEV, generator=gen)


def _composed(env):
    v = wrappers.VmapWrapper(env)
    if env.clip_restarts:
        return wrappers.ClipAutoResetWrapper(_Tap(wrappers.ClipEpisodeWrapper(v, L, 1)))
    return wrappers.AutoResetWrapper(_Tap(wrappers.EpisodeWrapper(v, L, 1)))


def _fused(env):
    return wrappers.FusedEpisodeAutoResetWrapper(wrappers.VmapWrapper(env), L)


class _Tap(wrappers.Wrapper):
    """Between the episode wrapper and the auto-reset wrapper: keeps (cur_frame before the step, stepped qpos) -- the state before the restore."""

    def __init__(self, env):
        super().__init__(env)
        self.seen = []

    def step(self, state, action):
        before = state.info["cur_frame"]
        out = self.env.step(state, action)
        self.seen.append((before, out.pipeline_state.qpos))
        return out


def _run(wenv, acts):
    """The reset state and the state after every wrapped step, each with a copy of its info and metrics dicts as the step returned them
    (the composed AutoReset wrapper writes `steps` into the info of the state it is handed)."""
    snap = lambda s: s.replace(info=dict(s.info), metrics=dict(s.metrics))
    s = wenv.reset(_keys(), clip=IDS)
    out = [snap(s)]
    for t in range(acts.shape[0]):
        s = wenv.step(s, acts[t])
        out.append(snap(s))
    torch.cuda.synchronize()
    return out


def _flat(s):
    """Every leaf a wrapped step produces, by name (the bank is constant and the dicts' orders differ between the forms)."""
    d = {"ps." + k: v for k, v in s.pipeline_state.tree().items()}
    d.update(obs=s.obs, reward=s.reward, done=s.done)
    d.update({"metrics." + k: v for k, v in s.metrics.items()})
    d.update({"info." + k: s.info[k] for k in ("cur_frame", "restart_slot", "steps", "truncation", "clip") if k in s.info})
    return d


def _assert_same(got, want, what, skip=(), reward_tol=None):
    a, b = _flat(got), _flat(want)
    assert set(a) == set(b), (what, set(a) ^ set(b))
    for k in a:
        if k in skip:
            continue
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (what, k)
        if reward_tol is not None and k in ("reward", "metrics.pos_reward") and not torch.equal(a[k], b[k]):
            assert float((a[k] - b[k]).abs().max()) <= reward_tol, (what, k)
            continue
        assert torch.equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))


def _errors(env, qpos, old_frame):
    fi = np.clip(old_frame.cpu().numpy(), 0, env.track_len - 1)
    rows, tp = env._pose_host.astype(np.float64)[IDS, fi], env._track_host.astype(np.float64)[IDS, fi]
    return np.stack(rodent.pose_errors(qpos.cpu().numpy().astype(np.float64), tp, rows[:, :4], rows[:, 4:]))       # [3, N]


def _quartile_gap(e):
    """The middle of the widest gap between the sorted ranks 70 % .. 80 % of the errors `e`: 20 % .. 30 % of them lie above it."""
    s = np.sort(np.asarray(e).ravel())
    lo, hi = int(0.70 * s.size), int(0.80 * s.size)
    i = lo + int(np.argmax(np.diff(s)[lo:hi]))
    return 0.5 * (s[i] + s[i + 1])


@functools.lru_cache(maxsize=None)
def _thresholds(model):
    """Computed once per model and shared: the three thresholds, from the 14 composed wrapped steps of the K = 3 env without termination."""
    env = _make(model, 3)
    w = _composed(env)
    _run(w, _draws(env, STEPS, 1)[0])
    errs = np.stack([_errors(env, q, f) for f, q in w.env.seen])          # [STEPS, 3, N]
    return tuple(float(_quartile_gap(errs[:, k])) for k in range(3))


@functools.lru_cache(maxsize=None)
def _forms(case):
    """Computed once per case and shared: the env, its actions, noise and actor, and the states of the per-step composed and fused
    runs, of `unroll` as one launch and as 7 + 7, and of `unroll_policy` as two segments of 7."""
    from rodent_amd.training import acting
    model, K, H, bodies, term = case
    env = _make(model, K, H, bodies, _thresholds(model) if term else None)
    assert env.clip_restarts == K and env.end_at_clip_end and env.observation_size == env.sys.obs_dim + H * env.sys.nq
    acts, noise = _draws(env, STEPS, 1)
    comp = _composed(env)
    out = dict(env=env, acts=acts, noise=noise, composed=_run(comp, acts), seen=comp.env.seen, fused=_run(_fused(env), acts))
    wenv = _fused(env)
    out["unroll"] = wenv.unroll(wenv.reset(_keys(), clip=IDS), acts)
    out["unroll7"] = wenv.unroll(wenv.reset(_keys(), clip=IDS), acts[:7])
    out["unroll77"] = wenv.unroll(out["unroll7"], acts[7:])
    buf = acting.UnrollBuffer(2, N, 7, env.observation_size, env.action_size, torch.device(DEV))
    traj = dict(obs=buf.obs, raw_action=buf.raw_action, log_prob=buf.log_prob, reward=buf.reward, discount=buf.discount, truncation=buf.truncation)
    out["policy"], out["policy_actions"] = wenv.unroll_policy(wenv.reset(_keys(), clip=IDS), F.actor(env, 7), noise, traj, segment=7)
    out["buf"] = buf
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------------------- 6a. the fixture's own conditions
@pytest.mark.parametrize("K", [1, 3])
def test_the_draws_give_restores_of_both_causes(K):
    by_len, by_end = _schedule_counts(K)
    print(f"K={K}: {by_len} restores by episode_length, {by_end} by the clip's end, of {N * STEPS} pairs")
    for n in (by_len, by_end):
        assert 8 <= n <= 3 * N * STEPS // 4


@pytest.mark.parametrize("case", [c for c in CASES if c[4]])
def test_pose_failures_fall_in_a_quarter_to_three_quarters_of_the_pairs(case):
    """Counted on the float64 restatement of the recorded stepped states; the device's code agrees wherever the error stands clear of
    its threshold.  The three causes of a restore all occur."""
    f = _forms(case)
    env, thr = f["env"], f["env"].pose_termination
    fails = close = 0
    causes = np.zeros(3, dtype=np.int64)
    for t in range(1, STEPS + 1):
        old, qpos = f["seen"][t - 1]
        e = _errors(env, qpos, old)
        code = rodent.pose_fail_code(e, thr)
        clear = np.all(np.abs(e - np.asarray(thr)[:, None]) > 100 * F.term_bound(e), axis=0)
        got = F.code_of(f["composed"][t])
        assert np.array_equal(got[clear], code[clear]), (case, t)
        fails, close = fails + int((code != 0).sum()), close + int((~clear).sum())
        s = f["composed"][t]
        trunc, done = s.info["truncation"].cpu().numpy(), s.done.cpu().numpy()
        new_frame = old.cpu().numpy() + 1
        over = (s.info["steps"].cpu().numpy() >= L) | (new_frame >= T - 1)
        causes += [int((got != 0).sum()), int((s.info["steps"].cpu().numpy() >= L).sum()), int((new_frame >= T - 1).sum())]
        assert (done[(got != 0) | over] == 1).all() and (trunc[got != 0] == 0).all() and (trunc[~over] == 0).all(), (case, t)
    print(f"{case}: thresholds {thr}; pose failures in {fails} of {N * STEPS} pairs (float64), {close} pairs within 100 bounds of a threshold; "
          f"restores by pose failure / episode_length / clip end: {causes.tolist()}")
    assert N * STEPS // 4 <= fails <= 3 * N * STEPS // 4
    assert (causes >= 1).all()


# ---------------------------------------------------------------------------------------------- 1. per-step path
@pytest.mark.parametrize("case", CASES)
def test_fused_wrapped_step_equals_the_composed_wrappers(case):
    f = _forms(case)
    K = case[1]
    assert len(f["fused"]) == STEPS + 1
    restores = 0
    for t, (g, w) in enumerate(zip(f["fused"], f["composed"])):
        _assert_same(g, w, (case, t))
        assert g.info["restart_slot"].dtype == torch.int32 and g.info["cur_frame"].dtype == torch.int32
        assert int(g.info["restart_slot"].min()) >= 0 and int(g.info["restart_slot"].max()) <= K - 1
        restores += int(g.done.sum())
    bank = f["fused"][-1].info["restart_bank"]
    assert bank["frame"].shape == (K, N) and bank["obs"].shape == (K, N, f["env"].observation_size)
    assert restores >= 60                                                    # 32 envs x 14 steps in episodes of at most 5


# ---------------------------------------------------------------------------------------------- 2. multi-step path
@pytest.mark.parametrize("case", CASES)
def test_unroll_equals_the_wrapped_steps_in_one_launch_and_in_two(case):
    f = _forms(case)
    assert f["env"]._batch._restart is not None
    _assert_same(f["unroll"], f["fused"][STEPS], (case, "14"))
    _assert_same(f["unroll7"], f["fused"][7], (case, "7"))
    _assert_same(f["unroll77"], f["fused"][STEPS], (case, "7 + 7"))           # slot and frame carry across the launches


# ---------------------------------------------------------------------------------------------- 3. actor path
@pytest.mark.parametrize("case", CASES)
def test_unroll_policy_in_two_segments_replays_per_step(case):
    from rodent_amd.training import acting
    f = _forms(case)
    env, buf, acts = f["env"], f["buf"], f["policy_actions"]
    nets_ok = env._batch.clip_restarts_supported(with_actor=True)
    assert nets_ok is None, nets_ok
    replay = _run(_fused(env), acts)
    worst = 0.0
    for t in range(STEPS):
        u, i = divmod(t, 7)
        assert torch.equal(buf.obs[u, :, i], replay[t].obs), (case, t)
        assert torch.equal(buf.discount[u, :, i], 1 - replay[t + 1].done) and torch.equal(buf.truncation[u, :, i], replay[t + 1].info["truncation"]), (case, t)
        worst = max(worst, float((buf.reward[u, :, i] - replay[t + 1].reward).abs().max()))
    assert torch.equal(buf.obs[0, :, 7], replay[7].obs) and torch.equal(buf.obs[1, :, 7], replay[STEPS].obs)
    print(f"{case}: max |traj.reward - per-step reward| = {worst:.3g} (allowed {F.ACTOR_REWARD_TOL})")
    assert worst <= F.ACTOR_REWARD_TOL
    _assert_same(f["policy"], replay[STEPS], (case, "final"), reward_tol=F.ACTOR_REWARD_TOL)


# ---------------------------------------------------------------------------------------------- 4. no-restart equality
@pytest.mark.parametrize("model", ["rodent_optimized", "rodent_0"])
def test_k1_is_the_plain_env_until_an_envs_first_restore(model):
    env0, env1 = _make(model, 0), _make(model, 1, end=False)
    acts, _ = _draws(env0, STEPS, 1)
    a, b = _run(_fused(env0), acts), _run(_fused(env1), acts)
    restored = np.zeros(N, dtype=bool)
    frame_leaves = {"reward", "metrics.pos_reward", "metrics.quat_reward", "metrics.joint_reward", "info.cur_frame", "obs"}
    od = env0.sys.obs_dim
    differs = 0
    for t in range(STEPS + 1):
        fa, fb = _flat(a[t]), _flat(b[t])
        assert set(fb) - set(fa) == {"info.restart_slot"} and int(fb["info.restart_slot"].abs().max()) == 0
        before = torch.from_numpy(~restored).to(DEV)
        for k in fa:
            if k in frame_leaves:      # equal until the env's first restore; the restoring step itself reads the old frame
                assert torch.equal(fa[k][before], fb[k][before]) or k == "info.cur_frame", (model, t, k)
            else:                      # the physics does not read the frame: state, done, steps, truncation agree throughout
                assert torch.equal(fa[k], fb[k]), (model, t, k)
        assert torch.equal(fa["obs"][:, :od - 3], fb["obs"][:, :od - 3]), (model, t)       # all but the track entry
        now = a[t].done.cpu().numpy() == 1
        first = now & ~restored
        if t:
            ca, cb = fa["info.cur_frame"].cpu().numpy(), fb["info.cur_frame"].cpu().numpy()
            keep = ~restored & ~now
            assert np.array_equal(ca[keep], cb[keep]), (model, t)
            assert np.array_equal(cb[now], b[0].info["cur_frame"].cpu().numpy()[now]), (model, t)       # K = 1: the start frame comes back
            assert (ca[first] > cb[first]).all()                                                          # K = 0: it does not
            assert torch.equal(fa["obs"][torch.from_numpy(now).to(DEV)], fb["obs"][torch.from_numpy(now).to(DEV)])      # the stored first row
            differs += int((ca != cb).sum())
        restored |= now
    assert restored.all() and differs > N


# ---------------------------------------------------------------------------------------------- 5. purpose
@pytest.mark.parametrize("model", ["rodent_optimized", "rodent_0"])
def test_a_restored_env_stands_on_its_clip(model):
    """reset_to_reference, no noise, K = 3: after every restore the restored qpos meets the clip's row at the restored frame exactly as
    the bank entry did at reset (position error 0), and the row is the bank's.  The same env with K = 0 stands further from the row it
    is compared with than the fixture's max_pos_error: the defect this feature removes.

    On a clip of 120 frames, so that no read of the 14 steps clamps: at T = 104 the three envs that start at frames 98 and 99 reach the
    clip's last row, where the K = 0 env's error stops growing at 0.004 (103 - start) = 0.016 .. 0.02 -- measured 0.016 against thresholds
    of 0.0166 (rodent_optimized) and 0.0182 (rodent_0).  Unclamped it is 0.004 per step since the reset, 0.02 at the first restore."""
    max_pos = _thresholds(model)[0]
    env = _make(model, 3, H=5, reset_to_reference=True, reset_noise_scale=0.0, frames=120)
    acts, _ = _draws(env, STEPS, 1)
    s = _run(_fused(env), acts)
    bank = s[0].info["restart_bank"]
    bq, bf, bo = bank["pipeline_state"].qpos, bank["frame"], bank["obs"]
    pairs = 0
    for t in range(1, STEPS + 1):
        for e in np.nonzero(s[t].done.cpu().numpy() == 1)[0]:
            k = int(s[t].info["restart_slot"][e])
            assert k == (int(s[t - 1].info["restart_slot"][e]) + 1) % 3
            assert int(s[t].info["cur_frame"][e]) == int(bf[k, e])
            assert torch.equal(s[t].pipeline_state.qpos[e], bq[k, e]) and torch.equal(s[t].obs[e], bo[k, e])
            pairs += 1
        got = _errors(env, s[t].pipeline_state.qpos, s[t].info["cur_frame"])
        rst = s[t].done.cpu().numpy() == 1
        slot = s[t].info["restart_slot"].cpu().numpy()
        at_reset = _errors(env, bq[torch.from_numpy(slot).long().to(DEV), torch.arange(N, device=DEV)], s[t].info["cur_frame"])
        assert np.array_equal(got[:, rst], at_reset[:, rst]) and (got[0, rst] == 0).all(), (model, t)
    assert pairs >= 60
    env0 = _make(model, 0, H=5, reset_to_reference=True, reset_noise_scale=0.0, frames=120)
    s0 = _run(_fused(env0), acts)
    worst, n0 = math.inf, 0
    for t in range(1, STEPS + 1):
        rst = s0[t].done.cpu().numpy() == 1
        e_pos = _errors(env0, s0[t].pipeline_state.qpos, s0[t].info["cur_frame"])[0]
        if rst.any():
            worst, n0 = min(worst, float(e_pos[rst].min())), n0 + int(rst.sum())
    print(f"{model}: K = 0 stands at least {worst:.4g} from the row it is compared with after its {n0} restores; max_pos_error {max_pos:.4g}")
    assert n0 >= 60 and worst > max_pos


# ---------------------------------------------------------------------------------------------- 6b. a bad state in the three forms
def test_a_nan_in_qvel_takes_the_next_bank_entry_in_all_three_forms():
    from rodent_amd.training import acting
    env = _make("rodent_optimized", 3, H=5, bad_state_max=1e10)
    acts, noise = _draws(env, 2, 3)
    wenv = _fused(env)
    s0 = wenv.reset(_keys(), clip=IDS)
    qvel = s0.pipeline_state.qvel.clone()
    bad = [3, 17]
    qvel[bad, 5] = float("nan")
    poisoned = s0.replace(pipeline_state=s0.pipeline_state.replace(qvel=qvel))
    buf = acting.UnrollBuffer(1, N, 1, env.observation_size, env.action_size, torch.device(DEV))
    outs = dict(step=wenv.step(poisoned, acts[0]), unroll=wenv.unroll(poisoned, acts[:1]),
                policy=wenv.unroll_policy(poisoned, F.actor(env, 7), noise[:1], F.traj(buf))[0])
    torch.cuda.synchronize()
    bank = s0.info["restart_bank"]
    for name, s in outs.items():
        for e in bad:
            assert float(s.done[e]) == 1 and int(s.info["restart_slot"][e]) == 1 and float(s.info["truncation"][e]) == 0, (name, e)
            assert int(s.info["cur_frame"][e]) == int(bank["frame"][1, e]), (name, e)
            assert torch.equal(s.pipeline_state.qpos[e], bank["pipeline_state"].qpos[1, e]) and torch.equal(s.obs[e], bank["obs"][1, e]), (name, e)
        assert bool(torch.isfinite(s.pipeline_state.qvel).all()) and float(s.reward[bad].abs().max()) == 0, name
    assert float(buf.discount[0, 3, 0]) == 0 and float(buf.reward[0, 17, 0]) == 0
    assert env.bad_states() == 3 * len(bad)


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_refusals():
    with pytest.raises(ValueError, match="need the reference pose"):
        F.make("rodent_optimized", T, n=N, pose=False, clip_restarts=2)
    with pytest.raises(ValueError, match="needs clip_restarts >= 1"):
        _make("rodent_optimized", 0, end_at_clip_end=True)
    with pytest.raises(RuntimeError, match="Newton"):
        _make("rodent_optimized", 2, solver="newton")
    plain = F.make("rodent_optimized", T, n=N, pose=False)
    newton = F.make("rodent_optimized", T, n=N, pose=False, solver="newton")
    assert "Newton" in newton._batch.clip_restarts_supported() and plain._batch.clip_restarts_supported() is None
    from rodent_amd import envs
    cpu = envs.get_environment("rodent", track_pos=F.tracks(T)[0], num_envs=N, xml_path="rodent_cpu.xml", iterations=4, ls_iterations=4, n_frames=2, device=DEV)
    assert "candidate-pair" in cpu._batch.clip_restarts_supported() and "candidate-pair" in cpu._batch.clip_restarts_supported(with_actor=True)
    # the setter's own: no pose block, a slot count outside 1 .. 64, null pointers
    frames, slot = torch.zeros(2, N, dtype=torch.int32, device=DEV), torch.zeros(N, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="needs a pose block"):
        plain._batch.set_clip_restarts(frames, slot, slot.clone())
    env = _make("rodent_optimized", 2)
    wenv = _fused(env)
    s = wenv.step(wenv.reset(_keys(), clip=IDS), _draws(env, 1, 1)[0][0])       # a step: the pose block stands on the batch
    with pytest.raises(RuntimeError, match="1 .. 64"):
        env._batch.set_clip_restarts(torch.zeros(65, N, dtype=torch.int32, device=DEV), slot, slot.clone())
    with pytest.raises(RuntimeError, match="null frames, slot_in or slot_out"):
        env._batch.set_clip_restarts(frames, None, slot)
    env._batch.set_clip_restarts(frames, slot, slot.clone())
    with pytest.raises(RuntimeError, match="clip-restart block"):
        env._batch.set_pose(None)
    env._batch.set_clip_restarts(None)
    assert env._batch._restart is None
    # per-env parameters, as for any pose env
    with pytest.raises(RuntimeError, match="per-env parameters"):
        env.set_env_params(dof_f=torch.zeros(N, env.sys.nv, 16, device=DEV))
    # the evaluation form
    assert not env.eval_supported() and not wrappers.EvalWrapper(wenv).unroll_supported()
    ring_actor = F.actor(env, 7)
    with pytest.raises(RuntimeError, match="rr_env_unroll_eval"):
        env.unroll_eval(s, 2, ring_actor, None, episode_length=L, eval_metrics=torch.zeros(N, 6, device=DEV))
    # the per-step evaluator runs the fused wrapper and so gets the rule
    ev = wrappers.EvalWrapper(wenv)
    es = ev.reset(_keys(), clip=IDS)
    for t in range(6):
        es = ev.step(es, torch.zeros(N, env.action_size, device=DEV))
    assert int(es.info["restart_slot"].max()) == 1 and "first_obs" not in es.info


# ---------------------------------------------------------------------------------------------- 8. training
def test_ppo_train_with_clip_restarts(monkeypatch):
    """One training step at 64 envs with clip_restarts 3 and end_at_clip_end through the one-launch rollout: `fused_unroll_supported` says
    yes, the rollout runs as one launch, and the losses are finite."""
    from rodent_amd.training import acting
    from rodent_amd.training.agents.ppo import train as ppo
    env = F.make("rodent_optimized", T, n=64, clip_restarts=3, restart_frame_range=RANGE, end_at_clip_end=True, reference_obs_frames=5,
                  max_pos_error=0.05)
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
    evals = [m for m in log if "eval/episode_reward" in m]
    assert evals and all(math.isfinite(float(m["eval/episode_reward"])) for m in evals)
