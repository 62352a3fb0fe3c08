"""Clip sampling on the GPU (`Rodent(restart_sampling="weighted", clip_outcomes=True)`; rr_batch_set_clip_sampling, the RESTART instances
of the step kernel, rr_wrap_clip_sampling).

Fixture: that of tests/test_gpu_clip_library.py -- rodent_optimized, 32 envs, three clips, T = 104, lengths (104, 14, 9), n_frames 2,
CG 4/4, episodes of 5, 14 steps, bank frames drawn in [90, 102), reset clips arange(N) % 3 -- with K = 4 bank entries.  The rule is in
integers, so every comparison of slots, clips, frames, restore counts and outcome tables is exact; the host schedule is the loop of
tests/test_clip_sampling_cpu.py (`_loop`), played on the bank the reset state carries."""
import functools
import math

import numpy as np
import pytest
import torch

from rodent_amd.envs import graphed, rodent
from tests import clip_library_fixture as X
from tests import pose_fixture as F
from tests import test_gpu_clip_restart as R
from tests.pose_fixture import DEV
from tests.test_clip_sampling_cpu import _loop
from tests.test_gpu_clip_library import _assert_replay, _policy, _run_from

pytestmark = pytest.mark.gpu
N, C, T, L, STEPS, K = X.N, X.C, X.T, X.EPISODE, X.STEPS, 4
IDS, LENGTHS, SEED = X.IDS, X.LENGTHS, 17
MODEL = "rodent_optimized"


def _make(sampling="weighted", outcomes=True, lengths=True, across=True, **kw):
    if sampling is not None:
        kw.update(restart_sampling=sampling, restart_sampling_seed=SEED)
    if outcomes:
        kw.update(clip_outcomes=True)
    if lengths:
        kw.update(clip_lengths=LENGTHS)
    if across:
        kw.update(restart_across_clips=True)
    return R._make(MODEL, kw.pop("K", K), **kw)


def _bank(s):
    return s.info["restart_bank"]["frame"].cpu().numpy(), s.info["restart_bank"]["clip"].cpu().numpy()


def _ints(s):
    """(frame, clip, slot, draws) of a state, int64 [N, 4]."""
    return torch.stack([s.info[k] for k in ("cur_frame", "clip", "restart_slot", "restart_draws")], dim=-1).cpu().numpy().astype(np.int64)


# ---------------------------------------------------------------------------------------------- 1. the three forms agree
@functools.lru_cache(maxsize=None)
def _forms():
    """Computed once and shared: weights (1, 2, 5), an env that never ends by itself; every form starts from a cleared table and leaves
    its own."""
    env = _make(terminate_when_unhealthy=False)
    env.set_clip_weights([1, 2, 5])
    acts, noise = R._draws(env, STEPS, 1)
    out = dict(env=env, acts=acts)
    tables = {}

    def table(name):
        torch.cuda.synchronize()
        tables[name] = env.clip_outcomes(clear=True)
    out["composed"] = R._run(R._composed(env), acts); table("composed")
    out["fused"] = R._run(R._fused(env), acts); table("fused")
    wenv = R._fused(env)
    s0 = wenv.reset(R._keys(), clip=IDS)
    out["s0"] = s0
    out["unroll"] = wenv.unroll(s0, acts); table("unroll")
    out["programmed"] = env._batch._sampling is not None          # (a later bare step clears the block again)
    out["unroll7"] = wenv.unroll(s0, acts[:7])
    out["unroll77"] = wenv.unroll(out["unroll7"], acts[7:]); table("unroll77")
    out["policy"], out["policy_actions"], out["buf"] = _policy(wenv, env, s0, noise); table("policy")
    out["replay"] = _run_from(wenv, s0, out["policy_actions"]); table("replay")
    out["tables"] = tables
    frames, clips = _bank(s0)
    out["want"], out["want_table"] = _loop(frames, clips, LENGTHS, rodent.quantise_clip_weights([1, 2, 5]), SEED, L, STEPS)
    out["cyclic"] = _loop(frames, clips, LENGTHS, None, SEED, L, STEPS)[0]
    return out


def test_the_per_step_forms_agree_and_follow_the_host_schedule():
    f = _forms()
    assert f["env"].clip_weights().tolist() == [13107, 26214, 65535]
    assert f["s0"].info["restart_draws"].dtype == torch.int32 and not f["s0"].info["restart_draws"].any()
    for t, (g, w) in enumerate(zip(f["fused"], f["composed"])):
        R._assert_same(g, w, ("fused / composed", t))
        assert torch.equal(g.info["restart_draws"], w.info["restart_draws"]) and g.info["restart_draws"].dtype == torch.int32, t
        if t:
            assert np.array_equal(_ints(g), f["want"][t - 1]), ("host schedule", t)
    want, cyc = f["want"], f["cyclic"]
    restores, differ = int(want[-1, :, 3].sum()), int((want[:, :, 2] != cyc[:, :, 2]).sum())
    print(f"{restores} restores, {differ} (step, env) pairs whose slot differs from the cyclic walk; table {f['want_table'].tolist()}")
    assert restores >= 60 and differ >= 30
    assert np.array_equal(f["tables"]["composed"], f["want_table"]) and np.array_equal(f["tables"]["fused"], f["want_table"])


def test_unroll_equals_the_wrapped_steps_in_one_launch_and_in_two():
    f = _forms()
    assert f["programmed"]
    for name, at in (("unroll", STEPS), ("unroll7", 7), ("unroll77", STEPS)):
        R._assert_same(f[name], f["fused"][at], name)
        assert np.array_equal(_ints(f[name]), f["want"][at - 1]), name          # slot, frame, clip and restore count carry across launches
    assert np.array_equal(f["tables"]["unroll"], f["want_table"])
    assert np.array_equal(f["tables"]["unroll77"], f["want_table"])                   # segments flushed at a launch's end add up
    # the input state's count is left alone, the result is a fresh tensor
    assert not f["s0"].info["restart_draws"].any() and f["unroll"].info["restart_draws"].data_ptr() != f["s0"].info["restart_draws"].data_ptr()


def test_unroll_policy_replays_per_step_with_the_same_draws_and_table():
    f = _forms()
    why = f["env"]._batch.clip_sampling_supported(with_actor=True)
    assert why is None, why
    _assert_replay(f["buf"], f["replay"], f["policy"], "policy")
    assert np.array_equal(_ints(f["policy"]), _ints(f["replay"][STEPS])) and np.array_equal(_ints(f["policy"]), f["want"][STEPS - 1])
    assert np.array_equal(f["tables"]["policy"], f["tables"]["replay"]) and np.array_equal(f["tables"]["policy"], f["want_table"])


# ---------------------------------------------------------------------------------------------- 2. weight 0 is exact
def test_a_clip_of_weight_zero_is_never_drawn():
    """Weights (1, 0, 1): after its first restore no env is on clip 1 -- except env 1, whose whole bank is built on clip 1 (S == 0), which
    walks its bank cyclically."""
    env = _make(terminate_when_unhealthy=False)
    env.set_clip_weights([1, 0, 1])
    ids = X.bank(K)[1].copy()
    ids[:, 1] = 1
    assert all(len(set(ids[:, e].tolist()) - {1}) >= 1 for e in range(N) if e != 1)       # every other bank holds another clip
    acts, _ = R._draws(env, STEPS, 1)
    wenv = R._fused(env)
    s0 = wenv.reset(R._keys(), clip=ids)
    frames, clips = _bank(s0)
    assert np.array_equal(clips, ids)
    want, _ = _loop(frames, clips, LENGTHS, [65535, 0, 65535], SEED, L, STEPS)
    states = _run_from(wenv, s0, acts)
    landed = 0
    for t in range(1, STEPS + 1):
        got = _ints(states[t])
        assert np.array_equal(got, want[t - 1]), t
        restored = got[:, 3] >= 1
        others = restored & (np.arange(N) != 1)
        assert (got[others, 1] != 1).all(), t
        landed += int(others.sum())
        assert got[1, 1] == 1 and got[1, 2] == got[1, 3] % K                              # the cyclic walk of the all-zero bank
    assert landed >= 200 and want[-1, 1, 3] >= 2
    u = wenv.unroll(s0, acts)
    assert np.array_equal(_ints(u), want[STEPS - 1])
    # some env started on clip 1 and did leave it
    assert any(ids[0, e] == 1 and want[-1, e, 1] != 1 for e in range(N) if e != 1)


# ---------------------------------------------------------------------------------------------- 3. the counter columns
def test_the_columns_split_the_episode_ends_by_cause():
    thr = R._thresholds(MODEL)
    env = _make(thr=thr)
    acts, noise = R._draws(env, STEPS, 1)
    wenv = R._fused(env)
    s0 = wenv.reset(R._keys(), clip=IDS)
    states = _run_from(wenv, s0, acts)
    torch.cuda.synchronize()
    got = env.clip_outcomes(clear=True)
    want = np.zeros((C, 5), dtype=np.int64)
    fails = 0
    for t in range(1, STEPS + 1):
        s, before = states[t], states[t - 1].info["clip"].cpu().numpy()
        done, trunc, code = (x.cpu().numpy() for x in (s.done, s.info["truncation"], s.metrics["pose_fail"]))
        rodent.clip_outcome_update(want, before, code, (done != 0) & (trunc == 0), done)
        fails += int(((code != 0) & (done != 0)).sum())
    print(f"outcome table {got.tolist()}; {fails} steps with pose_fail and done")
    assert np.array_equal(got, want)
    assert (got[:, 1:4].sum(1) == got[:, 0]).all() and got[:, 1].sum() == fails and got[:, 4].sum() == N * STEPS
    assert fails >= 10 and got[:, 3].sum() >= 10          # both a failing and a truncating cause occur at these thresholds
    u = wenv.unroll(s0, acts)
    R._assert_same(u, states[STEPS], "unroll")
    torch.cuda.synchronize()
    assert np.array_equal(env.clip_outcomes(clear=True), want)
    comp = R._composed(env)
    s = comp.reset(R._keys(), clip=IDS)
    for t in range(STEPS):
        s = comp.step(s, acts[t])
    torch.cuda.synchronize()
    assert np.array_equal(env.clip_outcomes(clear=True), want)
    _policy(wenv, env, s0, noise)
    p = env.clip_outcomes(clear=True)
    assert (p[:, 1:4].sum(1) == p[:, 0]).all() and p[:, 4].sum() == N * STEPS


def test_a_nan_in_qvel_lands_in_the_env_done_column_of_its_clip():
    from rodent_amd.training import acting
    env = _make(bad_state_max=1e10, terminate_when_unhealthy=False)
    acts, noise = R._draws(env, 2, 3)
    wenv = R._fused(env)
    s0 = wenv.reset(R._keys(), clip=IDS)
    frames, _ = _bank(s0)
    bad = next(e for e in range(N) if frames[0, e] + 1 < LENGTHS[IDS[e]] - 1)          # an env the clip's end does not truncate at step 1
    qvel = s0.pipeline_state.qvel.clone()
    qvel[bad, 5] = float("nan")
    poisoned = s0.replace(pipeline_state=s0.pipeline_state.replace(qvel=qvel))
    buf = acting.UnrollBuffer(1, N, 1, env.observation_size, env.action_size, torch.device(DEV))
    forms = dict(step=lambda: wenv.step(poisoned, acts[0]), unroll=lambda: wenv.unroll(poisoned, acts[:1]),
                 policy=lambda: wenv.unroll_policy(poisoned, F.actor(env, 7), noise[:1], F.traj(buf))[0],
                 composed=lambda: R._composed(env).step(poisoned.replace(info=dict(poisoned.info)), acts[0]))
    for name, run in forms.items():
        s = run()
        torch.cuda.synchronize()
        t = env.clip_outcomes(clear=True)
        assert float(s.done[bad]) == 1 and float(s.info["truncation"][bad]) == 0 and int(s.info["restart_draws"][bad]) == 1, name
        assert t[:, 2].sum() == 1 and t[IDS[bad], 2] == 1 and t[:, 1].sum() == 0 and t[:, 4].tolist() == np.bincount(IDS, minlength=C).tolist(), (name, t.tolist())
        assert (t[:, 1:4].sum(1) == t[:, 0]).all(), name


# ---------------------------------------------------------------------------------------------- 4. off is off
def test_with_the_options_off_nothing_is_programmed_and_counting_alone_changes_only_the_table():
    plain = R._make(MODEL, K, clip_lengths=LENGTHS, restart_across_clips=True)
    off = R._make(MODEL, K, clip_lengths=LENGTHS, restart_across_clips=True, restart_sampling=None, clip_outcomes=False, restart_sampling_seed=0)
    counting = _make(sampling=None)
    acts, _ = R._draws(plain, STEPS, 1)
    runs = {}
    for name, env in (("plain", plain), ("off", off), ("counting", counting)):
        w = R._fused(env)
        s0 = w.reset(R._keys(), clip=IDS)
        fused, composed = R._run(w, acts), R._run(R._composed(env), acts)
        runs[name] = (fused, w.unroll(s0, acts), composed)          # the multi-step launch last: its blocks stand on the batch below
        assert "restart_draws" not in s0.info and set(s0.info) == {"cur_frame", "clip", "restart_bank", "restart_slot", "steps", "truncation"}
    torch.cuda.synchronize()
    assert plain._batch._sampling is None and off._batch._sampling is None and off.clip_sampling is None
    assert counting._batch._sampling is not None and counting.clip_weights() is None
    for name in ("off", "counting"):
        for t in range(STEPS + 1):
            R._assert_same(runs[name][0][t], runs["plain"][0][t], (name, "fused", t))
            R._assert_same(runs[name][2][t], runs["plain"][2][t], (name, "composed", t))
        R._assert_same(runs[name][1], runs["plain"][1], (name, "unroll"))
        assert set(runs[name][1].info) == set(runs["plain"][1].info)
    table = counting.clip_outcomes()
    assert table[:, 4].sum() == 3 * N * STEPS and (table[:, 1:4].sum(1) == table[:, 0]).all() and table[:, 0].sum() > 0
    # uniform weights draw, so the slots differ from the walk -- but an env with the block set and cleared again is the plain env
    counting._batch.set_clip_sampling(None)
    assert counting._batch._sampling is None


# ---------------------------------------------------------------------------------------------- 5. weights updated in place
def test_weights_written_between_two_launches_take_effect_in_the_second():
    env = _make(outcomes=False, terminate_when_unhealthy=False)
    acts, _ = R._draws(env, STEPS, 1)
    wenv = R._fused(env)
    s0 = wenv.reset(R._keys(), clip=IDS)
    frames, clips = _bank(s0)
    ptr = env.clip_sampling["weights"].data_ptr()
    env.set_clip_weights([1, 2, 5])
    half = wenv.unroll(s0, acts[:7])
    env.set_clip_weights([0, 0, 1])
    assert env.clip_sampling["weights"].data_ptr() == ptr
    full = wenv.unroll(half, acts[7:])
    first, _ = _loop(frames, clips, LENGTHS, rodent.quantise_clip_weights([1, 2, 5]), SEED, L, 7)
    assert np.array_equal(_ints(half), first[-1])
    # the second launch by hand: the loop continued from the first launch's end with the new table
    q = [0, 0, 65535]
    steps = torch.where(half.done != 0, torch.zeros_like(half.done), half.info["steps"]).cpu().numpy()      # a finished episode starts over
    want = _continue(frames, clips, _ints(half), steps, q, 7)
    assert np.array_equal(_ints(full), want)
    restored = want[:, 3] > first[-1][:, 3]
    has2 = (clips == 2).any(0)
    assert (want[restored & has2, 1] == 2).all() and int((restored & has2).sum()) >= 20
    # the same two halves per step
    env.set_clip_weights([1, 2, 5])
    s = s0
    for t in range(STEPS):
        if t == 7:
            env.set_clip_weights([0, 0, 1])
        s = wenv.step(s, acts[t])
    R._assert_same(s, full, "per step")
    assert np.array_equal(_ints(s), want)


def _continue(frames, clips, ints, steps, q, nsteps):
    """`_loop` continued for an env that never ends by itself: from (frame, clip, slot, draws) and the episode's step count."""
    out = ints.copy()
    for e in range(N):
        f, c, slot, draws = (int(x) for x in ints[e])
        n = int(steps[e])
        for _ in range(nsteps):
            n, nf = n + 1, f + 1
            if n >= L or nf >= LENGTHS[c] - 1:
                slot = rodent.weighted_slot(int(rodent.restart_hash(SEED, e, draws)), [q[clips[k, e]] for k in range(K)], slot)
                draws += 1
                f, c, n = int(frames[slot, e]), int(clips[slot, e]), 0
            else:
                f = nf
        out[e] = (f, c, slot, draws)
    return out


def test_a_replayed_graph_reads_the_weights_written_after_its_capture():
    """The graph `SubBatchRollout` replays: one wrapped step, captured with weights (1, 2, 5), replayed after the table was rewritten in
    place -- the states are those of host-issued steps with the same rewrite."""
    dev = torch.device(DEV)
    stream = torch.cuda.Stream(dev)

    def make():
        with torch.cuda.stream(stream):
            env = _make(terminate_when_unhealthy=False)
            env.set_clip_weights([1, 2, 5])
            wenv = R._fused(env)
            return env, wenv, wenv.reset(R._keys(), clip=IDS)
    env_h, wenv_h, s = make()
    acts = R._draws(env_h, STEPS, 1)[0]
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for t in range(STEPS):
            if t == 6:
                env_h.set_clip_weights([0, 0, 1])
            s = wenv_h.step(s, acts[t])
    torch.cuda.synchronize()
    want, want_table = s, env_h.clip_outcomes()
    env_g, wenv_g, sg = make()
    cursor = torch.zeros((), dtype=torch.long, device=dev)

    def step_fn(state):
        a = acts.index_select(0, cursor.reshape(1))[0]
        cursor.add_(1)
        return wenv_g.step(state, a)
    with torch.cuda.stream(stream):
        st1 = step_fn(sg)
    torch.cuda.synchronize()
    g = graphed.GraphedSteps(step_fn, st1, 1, stream)
    for t in range(1, STEPS):
        if t == 6:
            with torch.cuda.stream(stream):
                env_g.set_clip_weights([0, 0, 1])
        got = g.replay()
    torch.cuda.synchronize()
    assert int(cursor) == STEPS
    R._assert_same(got, want, "graph")
    assert np.array_equal(_ints(got), _ints(want)) and np.array_equal(env_g.clip_outcomes(), want_table)
    # the rewrite mattered: without it the run ends elsewhere
    env_n, wenv_n, sn = make()
    with torch.cuda.stream(stream):
        for t in range(STEPS):
            sn = wenv_n.step(sn, acts[t])
    torch.cuda.synchronize()
    assert not np.array_equal(_ints(sn), _ints(want))


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_refusals():
    with pytest.raises(RuntimeError, match="Newton"):
        _make(solver="newton")
    plain = F.make(MODEL, T, n=N, pose=False)
    newton = F.make(MODEL, T, n=N, pose=False, solver="newton")
    assert "Newton" in newton._batch.clip_sampling_supported() and plain._batch.clip_sampling_supported() is None
    from rodent_amd import envs
    cpu = envs.get_environment("rodent", track_pos=F.tracks(T)[0], num_envs=N, xml_path="rodent_cpu.xml", iterations=4, ls_iterations=4, n_frames=2, device=DEV)
    assert "candidate-pair" in cpu._batch.clip_sampling_supported() and "candidate-pair" in cpu._batch.clip_sampling_supported(with_actor=True)
    weights = torch.full((C,), 65535, dtype=torch.int32, device=DEV)
    table = torch.zeros(C, 5, dtype=torch.int64, device=DEV)
    din, dout = torch.zeros(N, dtype=torch.int32, device=DEV), torch.zeros(N, dtype=torch.int32, device=DEV)
    # no restart block
    pose = R._make(MODEL, 0)
    pose.step(pose.reset(R._keys(), clip=IDS), R._draws(pose, 1, 1)[0][0])
    with pytest.raises(RuntimeError, match="needs a clip-restart block"):
        pose._batch.set_clip_sampling(None, None, None, table)
    # weights without the bank's clips, without the restore counts
    same = R._make(MODEL, 2)
    w = R._fused(same)
    acts = R._draws(same, 2, 1)[0]
    w.unroll(w.reset(R._keys(), clip=IDS), acts)                      # the restart block stands, no library
    assert same._batch._restart is not None and same._batch._library is None
    with pytest.raises(RuntimeError, match="clip_weights needs a clip-library block with bank_clips"):
        same._batch.set_clip_sampling(weights, din, dout)
    same._batch.set_clip_sampling(None, None, None, table)           # counting alone needs no library
    with pytest.raises(RuntimeError, match="clip-sampling block"):
        same._batch.set_clip_restarts(None)
    same._batch.set_clip_sampling(None)
    same._batch.set_clip_restarts(None)
    env = _make()
    wenv = R._fused(env)
    s = wenv.unroll(wenv.reset(R._keys(), clip=IDS), acts)
    assert env._batch._sampling is not None and env._batch._library is not None
    with pytest.raises(RuntimeError, match="clip_weights needs draws_in and draws_out"):
        env._batch.set_clip_sampling(weights, None, None)
    with pytest.raises(RuntimeError, match="may not alias"):
        env._batch.set_clip_sampling(weights, din, din)
    with pytest.raises(ValueError, match="shape"):
        env._batch.set_clip_sampling(weights, din, dout, table[:, :4].contiguous())
    with pytest.raises(RuntimeError, match="clip-sampling block"):
        env._batch.set_clip_restarts(None)
    with pytest.raises(RuntimeError, match="clip-sampling block with clip_weights"):
        env._batch.set_clip_library(None)
    # a bare step after a multi-step launch: the env io clears and sets the blocks in the right order, and a launch follows again
    env.step(s, acts[0])
    assert env._batch._sampling is None
    wenv.unroll(s, acts)
    assert env._batch._sampling is not None


# ---------------------------------------------------------------------------------------------- 7. training
def test_one_ppo_train_step_reweights_the_clips(monkeypatch):
    from rodent_amd.training import acting
    from rodent_amd.training.agents.ppo import train as ppo
    thr = R._thresholds(MODEL)
    env = F.make(MODEL, T, n=64, clip_restarts=K, restart_frame_range=X.RANGE, end_at_clip_end=True, reference_obs_frames=5,
                 clip_lengths=LENGTHS, restart_across_clips=True, restart_sampling="weighted", clip_outcomes=True,
                 max_pos_error=thr[0], max_quat_error=thr[1], max_joint_error=thr[2])
    assert env.clip_weights().tolist() == [65535] * C
    calls, log, tables = {"fused": 0}, [], []
    real_fused = acting.generate_unrolls_fused
    fw = rodent.FailureWeights()

    def spy(*a, **k):
        calls["fused"] += 1
        return real_fused(*a, **k)

    def weight_fn(table):
        tables.append(table.copy())
        return fw(table)
    monkeypatch.setattr(acting, "generate_unrolls_fused", spy)
    ppo.train(environment=env, num_timesteps=10 ** 9, episode_length=10, num_envs=64, batch_size=64, num_minibatches=2, unroll_length=5,
              num_updates_per_batch=2, num_evals=1, num_eval_envs=6, learning_rate=5e-5, entropy_cost=1e-3, discounting=0.97,
              normalize_observations=True, seed=3, max_training_steps=1, progress_fn=lambda n, m: log.append(m), clip_weight_fn=weight_fn)
    assert calls["fused"] == 1 and len(tables) == 1
    t = tables[0]
    print(f"outcome table of the training step {t.tolist()}, weights {env.clip_weights().tolist()}")
    assert t[:, 4].sum() == 64 * 10 and (t[:, 1:4].sum(1) == t[:, 0]).all() and t[:, 0].sum() > 0
    m = [x for x in log if "training/clip_fail_rate" in x][-1]
    for k in ["training/clip_fail_rate", "training/clip_truncated_share"] + [f"training/clip_fail_rate_clip{c}" for c in range(C)]:
        assert math.isfinite(float(m[k])) and 0.0 <= float(m[k]) <= 1.0, k
    assert m["training/clip_fail_rate"] == (t[:, 1].sum() + t[:, 2].sum()) / t[:, 0].sum()
    assert env.clip_weights().tolist() != [65535] * C and max(env.clip_weights().tolist()) == 65535
    assert np.array_equal(env.clip_weights(), rodent.quantise_clip_weights(rodent.FailureWeights()(t)))
    assert not env.clip_outcomes().any()                  # read and cleared
