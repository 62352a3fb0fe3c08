"""One set of step-kernel instances behind the options of pose tracking: rr_body_kernel serves reference frames, pose termination and
body tracking in any combination, and an option a batch does not carry reaches it switched off at run time (zero frames, +inf
thresholds with a null pose_fail, a null track_bodies).  That rests on one property, pinned here: an option that is off, or on without
effect, moves no bit of anything else.

Fixture and helpers of tests/pose_fixture.py (12 envs on 3 clips, T = 104, n_frames 2, CG 4/4; rodent_optimized -- fixed dims -- and
rodent_0 -- generic dims).  Per model the eight envs of the lattice H in {0, 5} x thresholds in {none, (1e30, 1e30, 1e30): every compare
made, none fires} x bodies in {none, the fixture of tests/test_gpu_body_tracking.py}, all on the same keys, clips, actions and noise.
Each runs (a) five bare steps, (b) the wrapped multi-step launch of seven steps with episodes of three and (c) the same with the actor
inside (and, with them, seven wrapped single steps).

Within a form any two envs agree bit for bit in every leaf they share -- state arrays, the first obs_dim columns of every observation
row, the reference columns where both have H = 5, done, cur_frame, steps, truncation, every common metric -- and no pose_fail flag is
raised; the reward (and the trajectory's) agrees between envs with the same bodies flag.  Form (c) compares envs of equal H only: the
actor's first layer has the row's width.  The env with H = 0, no thresholds and no bodies runs rr_pose_kernel, whose actor reads 20
entries per lane against the 26 of rr_body_kernel: the six further entries are zeros that the first layer adds to its sums, so it joins
(c) like the others (this held bit for bit before the retirement too).

Of the eight envs the two with thresholds and no bodies run rr_poseterm_kernel, which is rr_body_kernel without the body code; the
five others with an option run rr_body_kernel.  The file passes against the library of the commit before rr_refobs_kernel was retired
as well (RR_LIB): there the env with frames only and the resets of every env with frames ran that entry, and the code of the entries
that remain did not change."""
import functools
import itertools

import pytest
import torch

from tests import pose_fixture as F
from tests.pose_fixture import FAIL_METRICS, MODELS

pytestmark = pytest.mark.gpu
T = 104
LATTICE = list(itertools.product((0, 5), (False, True), (False, True)))      # (H, thresholds, bodies)
POSE_ENV = (0, False, False)
FORMS = ("bare", "steps", "unroll", "policy")


@functools.lru_cache(maxsize=None)
def _runs(model):
    """Computed once per model and shared: {(H, thresholds, bodies): the env and its final states of every form, the states of the bare
    steps, the trajectory and the actions of the launch with the actor inside}."""
    out = {}
    for H, thr, bod in LATTICE:
        kw = dict(reference_obs_frames=H) if H else {}
        if thr:
            kw.update(max_pos_error=1e30, max_quat_error=1e30, max_joint_error=1e30)
        env = (F.make_body if bod else F.make)(model, T, **kw)
        assert env.observation_size == env.sys.obs_dim + H * env.sys.nq
        acts, noise = F.draws(env, 7, 2)
        r = F.wrapped_forms(env, acts, noise, F.actor(env, 7))
        r.update(env=env, bare_all=F.steps(env, F.draws(env, F.STEPS, 1)[0]))
        r["bare"] = r["bare_all"][-1]
        out[(H, thr, bod)] = r
    return out


def _same(x, y, D, what):
    """Bit equality of two leaves; two observation-wide leaves of different width agree in the model's own D columns."""
    if x.shape != y.shape:
        assert x.shape[:-1] == y.shape[:-1] and min(x.shape[-1], y.shape[-1]) == D, (what, x.shape, y.shape)
        x, y = x[..., :D], y[..., :D]
    assert x.dtype == y.dtype and torch.equal(x, y), (what, int((x != y).sum()))


def _assert_states_agree(a, b, D, what, reward):
    pairs = [("pipeline_state", a.pipeline_state, b.pipeline_state), ("obs", a.obs, b.obs), ("done", a.done, b.done)]
    pairs += [("info." + k, a.info[k], b.info[k]) for k in sorted(set(a.info) & set(b.info))]
    pairs += [("metrics." + k, a.metrics[k], b.metrics[k]) for k in sorted(set(a.metrics) & set(b.metrics))]
    if reward:
        pairs.append(("reward", a.reward, b.reward))
    for name, u, v in pairs:
        lu, lv = F.leaves(u), F.leaves(v)
        assert len(lu) == len(lv) >= 1, (what, name)
        for i, (x, y) in enumerate(zip(lu, lv)):
            _same(x, y, D, (what, name, i))
    assert "cur_frame" in set(a.info) & set(b.info) and {"pos_reward", "quat_reward", "joint_reward"} <= set(a.metrics) & set(b.metrics)


def _pairs(form):
    """The pairs of lattice points compared in `form`."""
    for ka, kb in itertools.combinations(LATTICE, 2):
        if form == "policy" and ka[0] != kb[0]:
            continue
        yield ka, kb


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("model", MODELS)
def test_an_option_that_is_off_or_never_fires_moves_no_other_bit(model, form):
    runs = _runs(model)
    D = runs[POSE_ENV]["env"].sys.obs_dim
    n = 0
    for ka, kb in _pairs(form):
        a, b = runs[ka], runs[kb]
        same_bodies = ka[2] == kb[2]
        if form == "bare":
            for t, (sa, sb) in enumerate(zip(a["bare_all"], b["bare_all"])):
                _assert_states_agree(sa, sb, D, (model, form, ka, kb, t), same_bodies)
        else:
            _assert_states_agree(a[form], b[form], D, (model, form, ka, kb), same_bodies)
        if form == "steps":
            assert {"steps", "truncation", "first_obs"} <= set(a[form].info) & set(b[form].info)
        if form == "policy":
            _same(a["policy_actions"], b["policy_actions"], D, (model, form, ka, kb, "actions"))
            for f in ("obs", "raw_action", "log_prob", "discount", "truncation") + (("reward",) if same_bodies else ()):
                _same(getattr(a["buf"], f), getattr(b["buf"], f), D, (model, form, ka, kb, "traj." + f))
        n += 1
    assert n == (12 if form == "policy" else 28)      # pairs of equal H | all pairs of eight


@pytest.mark.parametrize("model", MODELS)
def test_the_fixture_exercises_what_it_compares(model):
    """Thresholds of 1e30 raise no flag in any form; episodes end inside the launches; the rewards of envs with and
    without bodies differ (the body terms are not zero); the reference columns are written."""
    runs = _runs(model)
    D = runs[POSE_ENV]["env"].sys.obs_dim
    for key, r in runs.items():
        states = r["bare_all"] + [r[f] for f in FORMS[1:]]
        if key[1]:
            assert all(float(s.metrics[k].abs().max()) == 0.0 for s in states for k in FAIL_METRICS), key
        else:
            assert not set(FAIL_METRICS) & set(r["bare"].metrics), key
        if key[0]:
            assert all(float(s.obs[:, D:].abs().max()) > 0.0 for s in states), key
            assert float(r["buf"].obs[..., D:].abs().max()) > 0.0, key
        assert float(r["buf"].truncation.max()) == 1.0 and float(r["unroll"].info["steps"].max()) <= 3.0, key      # episodes of three end inside the launch
    a, b = runs[(5, True, False)], runs[(5, True, True)]
    for f in FORMS:
        assert not torch.equal(a[f].reward, b[f].reward), f


def _launch_sequence():
    """reset, step, reset, wrapped unroll of three (episodes of three: a restore from the bank inside), step -- on one fresh env with every
    option: (which of the pose, termination, body and restart blocks stand on its batch after each launch, the final state)."""
    from rodent_amd.envs import wrappers
    env = F.make_body("rodent_optimized", T, reference_obs_frames=5, max_pos_error=1e30, max_quat_error=1e30, max_joint_error=1e30, clip_restarts=2)
    wenv, b, acts, stand = wrappers.wrap(env, episode_length=3, action_repeat=1), env._batch, F.draws(env, 5, 4)[0], []

    def seen(state):
        stand.append(tuple(x is not None for x in (b._pose, b._pterm, b._body, b._restart)))
        return state
    s = seen(env.step(seen(env.reset(F.keys(), clip=F.IDS)), acts[0]))
    s = seen(wenv.unroll(seen(wenv.reset(F.keys(), clip=F.IDS)), acts[1:4].contiguous()))
    s = seen(env.step(s, acts[4]))
    torch.cuda.synchronize()
    return stand, s


def test_each_launch_leaves_the_blocks_it_carries_and_the_sequence_replays():
    """A reset of an env with reference frames hands the pose block alone, a step the pose, termination and body blocks, the multi-step
    launch all four: every clear and set of `hip.Batch._program_blocks`, both ways; a second fresh env ends in the same state, bit for bit."""
    (stand, got), (_, want) = _launch_sequence(), _launch_sequence()
    reset, step, unroll = (True, False, False, False), (True, True, True, False), (True, True, True, True)
    assert stand == [reset, step, reset, unroll, step]
    lg, lw = F.leaves(got), F.leaves(want)
    assert len(lg) == len(lw) > 10 and all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(lg, lw))
    assert int(got.info["restart_slot"].max()) == 1 and torch.isfinite(got.obs).all()       # the restore ran
