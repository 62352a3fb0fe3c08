"""What `Rodent` hands its batch, launch by launch and option by option, held without a GPU: `hip.Batch` is replaced by a fake that records
every call, so the env-io dict of `reset`, `step` and the wrapped multi-step launch -- its keys, the identity of the option tensors, the
scalar tuples, the buffers' shapes and dtypes -- and the metric and info keys of the returned states are pinned for every set of pose
options.  Also: the constructor arguments `with_num_envs` rebuilds a sibling from, and the query `fused_unroll_supported` asks about the
in-kernel actor.  The model blob loads on the host (`hip.Model` needs no device); the values the kernels compute are the GPU tests' part."""
import inspect

import numpy as np
import pytest
import torch

from rodent_amd import jax_random
from rodent_amd.envs import base, rodent, wrappers
from rodent_amd.training import acting

N, T, H, K = 3, 120, 2, 2
TRUE_QUERIES = ("unroll_supported", "eval_supported", "env_params_supported")


class FakeBatch:
    """Records (method, args, kwargs) of every call.  The refusal-style `*_supported` queries answer None (served) or the text planted in
    `refuse`; the three boolean queries answer True; everything else returns None."""

    def __init__(self, model, num_envs, device=None):
        self.model, self.N, self.dims, self.calls, self.refuse = model, int(num_envs), model.dims, [], {}
        self._pose = self._pterm = self._body = self._restart = None

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def call(*args, **kw):
            self.calls.append((name, args, kw))
            return True if name in TRUE_QUERIES else self.refuse.get(name)
        return call

    def last_env_io(self, method):
        """The env-io dict of the last `method` call, without its None entries."""
        args = [a for n, a, _ in self.calls if n == method][-1]
        io = [a for a in args if isinstance(a, dict) and "track_pos" in a]
        assert len(io) == 1
        return {k: v for k, v in io[0].items() if v is not None}


@pytest.fixture(autouse=True)
def fake_batch(monkeypatch):
    monkeypatch.setattr(base.hip, "Batch", FakeBatch)


POSE, FRAMES, TERM, BODIES, RESTART = "pose", "frames", "term", "bodies", "restart"
OPTION_SETS = [(), (POSE,), (POSE, FRAMES), (POSE, TERM), (POSE, BODIES), (POSE, RESTART), (POSE, FRAMES, TERM, BODIES, RESTART)]
IDS = ["none", "pose", "pose+H2", "pose+max_pos_error", "pose+bodies", "pose+restarts", "all"]


def _kwargs(options, nq=74, nbody=None):
    kw = dict(track_pos=np.zeros((T, 3)), xml_path="rodent_optimized.xml", device="cpu")
    if POSE in options:
        kw.update(track_quat=np.tile([1.0, 0.0, 0.0, 0.0], (T, 1)), track_joints=np.zeros((T, nq - 7)))
    if FRAMES in options:
        kw.update(reference_obs_frames=H)
    if TERM in options:
        kw.update(max_pos_error=1.0)
    if BODIES in options:
        kw.update(track_bodies=np.zeros((T, nbody, 3)), end_effector_ids=[3])
    if RESTART in options:
        kw.update(clip_restarts=K)
    return kw


def _make(options):
    nbody = rodent.Rodent(num_envs=1, **_kwargs(())).sys.nbody if BODIES in options else None
    kw = _kwargs(options, nbody=nbody)
    return rodent.Rodent(num_envs=N, **kw), kw


BASE_RESET = {"track_pos", "cur_frame", "obs", "healthy_reward", "ctrl_cost_weight", "healthy_z_range", "terminate_when_unhealthy"}
BASE_STEP = BASE_RESET | {"reward", "done", "metrics"}
POSE_KEYS = {"track_pose", "pose_metrics", "quat_reward", "joint_reward"}
TERM_KEYS = {"pose_fail", "pose_termination"}
BODY_KEYS = {"track_bodies", "body_weights", "body_metrics", "body_reward", "endeff_reward"}
METRICS = {None: ["pos_reward", "reward_quadctrl", "reward_alive"], POSE: ["quat_reward", "joint_reward"],
           TERM: ["pose_fail", "pose_fail_pos", "pose_fail_quat", "pose_fail_joint"], BODIES: ["body_reward", "endeff_reward"]}


def _want_keys(options, launch):
    if launch == "reset":        # a reset has no reward: it hands the pose block only where it writes the reference blocks
        return BASE_RESET | (POSE_KEYS if FRAMES in options else set())
    want = BASE_STEP | (POSE_KEYS if POSE in options else set()) | (TERM_KEYS if TERM in options else set()) | (BODY_KEYS if BODIES in options else set())
    return want | ({"restart"} if launch == "unroll" and RESTART in options else set())


def _want_metrics(options):
    return [k for o in (None, POSE, TERM, BODIES) if o is None or o in options for k in METRICS[o]]


def _buf(io, key, shape, dtype=torch.float32):
    t = io[key]
    assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous(), (key, tuple(t.shape), t.dtype)
    return t


def _check_io(env, options, io, launch, state_in=None):
    assert set(io) == _want_keys(options, launch), (launch, sorted(set(io) ^ _want_keys(options, launch)))
    assert io["track_pos"] is env._track_pos
    _buf(io, "cur_frame", (N,), torch.int32)
    _buf(io, "obs", (N, env.observation_size))
    assert (io["healthy_reward"], io["ctrl_cost_weight"], io["healthy_z_range"], io["terminate_when_unhealthy"]) == (1.0, 0.1, (0.03, 0.5), True)
    if launch != "reset":
        _buf(io, "reward", (N,)), _buf(io, "done", (N,)), _buf(io, "metrics", (N, 3))
    if "track_pose" in io:
        assert io["track_pose"] is env._track_pose and tuple(env._track_pose.shape) == (T, env.sys.nq - 3)
        assert io["quat_reward"] == (1.0, 2.0) == env._quat_reward and io["joint_reward"] == (1.0, 0.5) == env._joint_reward
        assert _buf(io, "pose_metrics", (N, 2)) is not None
        assert (io["pose_metrics"] is getattr(env, "_reset_pose_metrics", None)) == (launch == "reset")
    if "pose_fail" in io:
        _buf(io, "pose_fail", (N,))
        assert io["pose_termination"] == env.pose_termination == (1.0, np.inf, np.inf)
    if "track_bodies" in io:
        assert io["track_bodies"] is env._body["track_bodies"] and io["body_weights"] is env._body["body_weights"]
        assert tuple(io["track_bodies"].shape) == (T, env.sys.nbody, 3) and tuple(io["body_weights"].shape) == (2, env.sys.nbody)
        _buf(io, "body_metrics", (N, 2))
        assert io["body_reward"] == env.body_tracking["body_reward"] == (1.0, 8.0)
        assert io["endeff_reward"] == env.body_tracking["endeff_reward"] == (1.0, 100.0) and env.body_tracking["end_effector_ids"] == (3,)
    if "restart" in io:
        r, info = io["restart"], state_in.info
        assert set(r) == {"frames", "slot_in", "slot_out", "end_at_clip_end"} and r["end_at_clip_end"] is False
        assert r["frames"] is info["restart_bank"]["frame"] and r["slot_in"] is info["restart_slot"]
        assert tuple(r["frames"].shape) == (K, N) and r["frames"].dtype == torch.int32
        assert tuple(r["slot_out"].shape) == (N,) and r["slot_out"].dtype == torch.int32 and r["slot_out"] is not r["slot_in"]


def _check_state(env, options, state, info_keys, io=None):
    assert list(state.metrics) == _want_metrics(options)
    assert set(state.info) == info_keys, sorted(set(state.info) ^ info_keys)
    for k, v in state.metrics.items():
        assert tuple(v.shape) == (N,) and v.dtype == torch.float32, k
    assert tuple(state.obs.shape) == (N, env.observation_size) and tuple(state.reward.shape) == (N,) and tuple(state.done.shape) == (N,)
    if io is None:               # a reset: every metric its own zero tensor, no two of them (nor reward, done) share memory
        own = list(state.metrics.values()) + [state.reward, state.done]
        assert all(float(v.abs().max()) == 0.0 and v._base is None for v in own) and len({v.data_ptr() for v in own}) == len(own)
        return
    assert state.reward is io["reward"] and state.done is io["done"] and state.obs is io["obs"] and state.info["cur_frame"] is io["cur_frame"]
    columns = [("metrics", METRICS[None])] + [(b, METRICS[o]) for o, b in ((POSE, "pose_metrics"), (BODIES, "body_metrics")) if o in options]
    for key, names in columns:   # column j of the launch's buffer, as a view
        for j, name in enumerate(names):
            m = state.metrics[name]
            assert m._base is io[key] and m.data_ptr() == io[key][:, j].data_ptr() and m.stride() == (io[key].shape[1],), name
    if TERM in options:          # the bits of the code: fresh tensors
        assert all(state.metrics[k]._base is None and state.metrics[k].is_contiguous() for k in METRICS[TERM])


@pytest.mark.parametrize("options", OPTION_SETS, ids=IDS)
def test_what_reaches_the_batch_and_what_comes_back(options):
    env, _ = _make(options)
    assert env.observation_size == env.sys.obs_dim + (H * env.sys.nq if FRAMES in options else 0)
    keys = jax_random.split(jax_random.PRNGKey(3), N)
    bank = {"restart_bank", "restart_slot"} if RESTART in options else set()
    # reset: one launch per bank entry, each with the same keys
    env._batch.calls.clear()
    s0 = env.reset(keys)
    assert [n for n, _, _ in env._batch.calls] == ["env_reset"] * (K if RESTART in options else 1)
    _check_io(env, options, env._batch.last_env_io("env_reset"), "reset")
    _check_state(env, options, s0, {"cur_frame"} | bank)
    # step
    s1 = env.step(s0, torch.zeros(N, env.action_size))
    io = env._batch.last_env_io("env_step_to")
    _check_io(env, options, io, "step")
    _check_state(env, options, s1, {"cur_frame"} | bank, io)
    assert list(s0.metrics) == _want_metrics(options) and all(float(v.abs().max()) == 0.0 for v in s0.metrics.values())      # the argument is left alone
    # the wrapped multi-step launch
    wenv = wrappers.wrap(env, episode_length=5)
    assert isinstance(wenv, wrappers.FusedEpisodeAutoResetWrapper)
    w0 = wenv.reset(keys)
    wrapped = {"cur_frame", "steps", "truncation"} | (bank or {"first_pipeline_state", "first_obs"})
    _check_state(env, options, w0, wrapped)
    w1 = wenv.unroll(w0, torch.zeros(2, N, env.action_size))
    io = env._batch.last_env_io("env_unroll")
    _check_io(env, options, io, "unroll", w0)
    _check_state(env, options, w1, wrapped, io)
    wrap = [a for n, a, _ in env._batch.calls if n == "env_unroll"][-1][-1]
    assert wrap["episode_length"] == 5 and (wrap.get("slots") == K if RESTART in options else "slots" not in wrap)
    if RESTART in options:
        assert w1.info["restart_slot"] is io["restart"]["slot_out"] and wrap["first_obs"] is w0.info["restart_bank"]["obs"]
    else:
        assert wrap["first_obs"] is w0.info["first_obs"]


def test_the_probes_of_the_constructor_and_the_reference_frames():
    """Which `*_supported` query each option asks at construction, in order, and where the pose block and the frame count are set."""
    env, _ = _make(OPTION_SETS[-1])
    calls = [(n, a) for n, a, _ in env._batch.calls if n.endswith("_supported") or n.startswith("set_")]
    assert [n for n, _ in calls] == ["pose_supported", "reference_obs_supported", "set_pose", "set_reference_obs", "pose_termination_supported",
                                     "body_tracking_supported", "clip_restarts_supported"]
    assert calls[1][1] == (H,) and calls[3][1] == (H,)
    assert calls[2][1][0] is env._track_pose and calls[2][1][1] is env._reset_pose_metrics and calls[2][1][2:] == ((1.0, 2.0), (1.0, 0.5))
    assert tuple(env._reset_pose_metrics.shape) == (N, 2) and float(env._reset_pose_metrics.abs().max()) == 0.0
    plain, _ = _make(())
    assert [n for n, _, _ in plain._batch.calls if n.endswith("_supported") or n.startswith("set_")] == []


REFUSALS = [((POSE,), "pose_supported", "Rodent(track_quat=..., track_joints=...): no"), ((POSE, FRAMES), "reference_obs_supported", f"Rodent(reference_obs_frames={H}): no"),
            ((POSE, TERM), "pose_termination_supported", "Rodent(max_pos_error / max_quat_error / max_joint_error): no"),
            ((POSE, BODIES), "body_tracking_supported", "Rodent(track_bodies=...): no"), ((POSE, RESTART), "clip_restarts_supported", f"Rodent(clip_restarts={K}): no")]


@pytest.mark.parametrize("options,query,text", REFUSALS, ids=[q for _, q, _ in REFUSALS])
def test_a_refused_option_raises_with_the_librarys_text(monkeypatch, options, query, text):
    class Refusing(FakeBatch):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.refuse = {query: "no"}
    nbody = rodent.Rodent(num_envs=1, **_kwargs(())).sys.nbody
    monkeypatch.setattr(base.hip, "Batch", Refusing)
    with pytest.raises(RuntimeError) as e:
        rodent.Rodent(num_envs=N, **_kwargs(options, nbody=nbody))
    assert str(e.value) == text


FORWARDED = dict(n_frames=10, pipeline_outputs=False, contact_outputs=False, balance=None, rebalance_every=4)


@pytest.mark.parametrize("options", [OPTION_SETS[0], OPTION_SETS[-1]], ids=["none", "all"])
def test_the_constructor_arguments_a_sibling_is_built_from(options):
    env, kw = _make(options)
    params = inspect.signature(rodent.Rodent.__init__).parameters
    own = set(params) - {"self", "num_envs", "device", "kwargs"}
    assert set(env._ctor) == own | set(FORWARDED)
    for k in own:                # what was passed, the very object; else the default
        assert env._ctor[k] is kw[k] if k in kw else env._ctor[k] == params[k].default, k
    assert {k: env._ctor[k] for k in FORWARDED} == FORWARDED
    other = rodent.Rodent(num_envs=N, n_frames=3, rebalance_every=7, **kw)
    assert (other._ctor["n_frames"], other._ctor["rebalance_every"], other._n_frames) == (3, 7, 3)


def test_a_sibling_keeps_every_option():
    env, _ = _make(OPTION_SETS[-1])
    env = rodent.Rodent(num_envs=N, bad_state_max=1e9, restart_frame_range=(5, 60), end_at_clip_end=True,
                        **{**_kwargs(OPTION_SETS[-1], nbody=env.sys.nbody), "track_pos": np.zeros((T + 40, 3)),
                           "track_quat": np.tile([1.0, 0.0, 0.0, 0.0], (T + 40, 1)), "track_joints": np.zeros((T + 40, env.sys.nq - 7)),
                           "track_bodies": np.zeros((T + 40, env.sys.nbody, 3))})
    sib = env.with_num_envs(2)
    assert sib.num_envs == 2 and sib is not env and sib._batch is not env._batch and sib._batch.N == 2
    names = ("pose_tracking", "reference_obs_frames", "pose_termination", "body_tracking", "clip_restarts", "restart_frame_range",
             "end_at_clip_end", "bad_state_max", "observation_size")
    assert {k: getattr(sib, k) for k in names} == {k: getattr(env, k) for k in names}
    assert sib.pose_tracking and sib.reference_obs_frames == H and sib.pose_termination == (1.0, np.inf, np.inf) and sib.clip_restarts == K
    assert sib.body_tracking["end_effector_ids"] == (3,) and sib.restart_frame_range == (5, 60) and sib.end_at_clip_end and sib.bad_state_max == 1e9
    assert sib.observation_size == sib.sys.obs_dim + H * sib.sys.nq


ARMS = [((POSE, FRAMES, TERM, BODIES, RESTART), "clip_restarts_supported", ()), ((POSE, FRAMES, TERM, BODIES), "body_tracking_supported", ()),
        ((POSE, FRAMES, TERM), "pose_termination_supported", ()), ((POSE, FRAMES), "reference_obs_supported", (H,)),
        ((POSE,), "reference_obs_supported", (0,)), ((), "reference_obs_supported", (0,))]


def _actor_queries(batch):
    """(name, positional arguments before `with_actor`, with_actor) of the with-actor queries recorded."""
    out = []
    for n, a, kw in batch.calls:
        if n.endswith("_supported") and n not in TRUE_QUERIES:
            lead = 1 if n == "reference_obs_supported" else 0
            out.append((n, tuple(a[:lead]), bool(kw["with_actor"] if "with_actor" in kw else a[lead])))
    return out


@pytest.mark.parametrize("options,query,lead", ARMS, ids=["restarts", "bodies", "termination", "frames", "pose", "plain"])
def test_the_query_about_the_in_kernel_actor(options, query, lead):
    """`fused_unroll_supported` asks the batch ONE question about the actor's row width, the one of the instance the env's multi-step
    launches run: clip restarts outrank body tracking, which outranks pose termination, which outranks the reference frames."""
    env, _ = _make(options)
    wenv = wrappers.wrap(env, episode_length=5)
    env._batch.calls.clear()
    assert acting.fused_unroll_supported(wenv, None, None) is False          # (a CPU env: refused after the query)
    assert _actor_queries(env._batch) == [(query, lead, True)]


@pytest.mark.parametrize("options,query,lead", ARMS, ids=["restarts", "bodies", "termination", "frames", "pose", "plain"])
def test_the_env_asks_that_query_itself(options, query, lead):
    """`Rodent.fused_actor_refusal` holds the order: the same one query, and the library's text where it refuses."""
    env, _ = _make(options)
    env._batch.calls.clear()
    assert env.fused_actor_refusal() is None
    assert _actor_queries(env._batch) == [(query, lead, True)]
    env._batch.refuse = {query: "too wide"}
    assert env.fused_actor_refusal() == "too wide"
