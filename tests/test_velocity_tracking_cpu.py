"""Velocity tracking (`Rodent(track_velocity=, track_angular_velocity=, track_joint_velocity=)`; rr_batch_set_velocity_tracking) as far as
it can be held without a GPU: the float64 restatement `velocity_rewards`, the argument check, the start state (`reset_qvel` and the
`qvel` every `env_reset` call is handed), what reaches the batch and what comes back (the `FakeBatch` pattern of
tests/test_env_io_options_cpu.py), the ctypes mirror of `rr_vel_io` against the header, and the example's refusal.  The GPU half is
tests/test_gpu_velocity_tracking.py."""
import ctypes
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

from rodent_amd import hip, jax_random
from rodent_amd.envs import base, rodent, wrappers
from rodent_amd.training import acting
from tests.test_env_io_options_cpu import FakeBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL_BATCH = hip.Batch      # (the fixture below replaces the attribute)
N, T, C, K, NV, NQ = 3, 120, 2, 3, 73, 74
WS = (0.7, 10.0, 0.5, 0.1, 0.3, 0.01)
VEL_KEYS = {"track_vel", "vel_metrics", "lin_vel_reward", "ang_vel_reward", "joint_vel_reward"}
VEL_METRICS = ["lin_vel_reward", "ang_vel_reward", "joint_vel_reward"]


@pytest.fixture(autouse=True)
def fake_batch(monkeypatch):
    monkeypatch.setattr(base.hip, "Batch", FakeBatch)


# ---------------------------------------------------------------------------------------------- the restatement
def test_the_restatement_against_a_hand_written_evaluation():
    rng = np.random.default_rng(5)
    qvel, ref = rng.normal(size=(4, 6, NV)), rng.normal(size=(4, 6, NV))
    w, k = (0.7, 0.5, 0.3), (0.4, 0.2, 0.01)
    got = rodent.velocity_rewards(qvel, ref, w, k)
    assert len(got) == 3 and all(g.shape == (4, 6) and g.dtype == np.float64 for g in got)
    for a in range(4):
        for b in range(6):
            s = [0.0, 0.0, 0.0]
            for i in range(NV):
                s[0 if i < 3 else (1 if i < 6 else 2)] += (qvel[a, b, i] - ref[a, b, i]) ** 2
            for j in range(3):
                assert got[j][a, b] == pytest.approx(w[j] * math.exp(-k[j] * s[j]), rel=1e-13)
    # the sums stay apart: moving one dof of a range moves that term alone
    for i, j in ((1, 0), (4, 1), (6, 2), (NV - 1, 2)):
        moved = qvel.copy()
        moved[..., i] += 0.5
        other = rodent.velocity_rewards(moved, ref, w, k)
        assert [np.array_equal(other[m], got[m]) for m in range(3)] == [m != j for m in range(3)]
    same = rodent.velocity_rewards(qvel.astype(np.float32), qvel.astype(np.float32), w, k)       # a row equal to qvel: the weights themselves
    assert all(np.array_equal(same[j], np.full((4, 6), w[j])) for j in range(3))
    assert all(np.array_equal(a, b) for a, b in zip(rodent.velocity_rewards(qvel, ref), rodent.velocity_rewards(qvel, ref, (1.0, 1.0, 1.0), (10.0, 0.1, 0.01))))


# ---------------------------------------------------------------------------------------------- the argument check
def _chk(track=None, lin="d", ang="d", joint="d", ws=WS, have_pose=True, nv=NV):
    track = np.zeros((5, 3), dtype=np.float32) if track is None else track
    lead = track.shape[:-1]
    dflt = lambda a, w: np.zeros(lead + (w,)) if isinstance(a, str) else a
    return rodent._check_velocity_tracking(track, dflt(lin, 3), dflt(ang, 3), dflt(joint, nv - 6), nv, ws, have_pose)


def test_what_the_argument_check_returns():
    assert _chk(lin=None, ang=None, joint=None) is None and _chk(lin=None, ang=None, joint=None, have_pose=False) is None
    rng = np.random.default_rng(1)
    lin, ang, joint = rng.normal(size=(5, 3)), rng.normal(size=(5, 3)), rng.normal(size=(5, NV - 6))
    rows = _chk(lin=lin, ang=torch.from_numpy(ang), joint=joint)
    assert rows.dtype == np.float32 and rows.shape == (5, NV) and rows.flags["C_CONTIGUOUS"]
    assert np.array_equal(rows, np.concatenate([lin, ang, joint], axis=-1).astype(np.float32))       # qvel layout
    rows = _chk(track=np.zeros((C, 5, 3), dtype=np.float32))
    assert rows.shape == (C, 5, NV)
    assert _chk(ws=(0, 0.0, np.float32(0), 0, 0, 0.0)) is not None                                    # 0 is allowed: that term is off


def test_every_refusal_of_the_argument_check():
    for missing in ("lin", "ang", "joint"):
        with pytest.raises(ValueError, match="go together"):
            _chk(**{missing: None})
        with pytest.raises(ValueError, match="go together"):
            _chk(**{k: None for k in ("lin", "ang", "joint") if k != missing})
    with pytest.raises(ValueError, match="track_quat and track_joints"):
        _chk(have_pose=False)
    for key, shapes in (("lin", ((5, 4), (4, 3), (5,), (1, 5, 3))), ("ang", ((5, 2), (6, 3), (C, 5, 3))), ("joint", ((5, NV), (5, NV - 7), (4, NV - 6), (1, 5, NV - 6)))):
        for shape in shapes:
            with pytest.raises(ValueError, match="must have shapes"):
                _chk(**{key: np.zeros(shape)})
    clips = np.zeros((C, 5, 3), dtype=np.float32)
    for key, shape in (("lin", (5, 3)), ("ang", (C + 1, 5, 3)), ("joint", (5, NV - 6)), ("joint", (C, 4, NV - 6)), ("joint", (C, 5, NV - 5))):
        with pytest.raises(ValueError, match="must have shapes"):
            _chk(track=clips, **{key: np.zeros(shape)})
    for key, w in (("lin", 3), ("ang", 3), ("joint", NV - 6)):
        for bad in (np.nan, np.inf, -np.inf):
            a = np.zeros((5, w))
            a[3, w - 1] = bad
            with pytest.raises(ValueError, match="non-finite"):
                _chk(**{key: a})
    for k in range(6):
        for bad in (-1.0, -1e-30, math.inf, -math.inf, math.nan, 1e39):       # 1e39 is inf as a float32
            ws = list(WS)
            ws[k] = bad
            with pytest.raises(ValueError, match="finite and >= 0"):
                _chk(ws=ws)
            with pytest.raises(ValueError, match="finite and >= 0"):
                _chk(lin=None, ang=None, joint=None, ws=ws)                    # checked whether or not the arrays are given
        for bad in ("1", True, None, [1.0]):
            ws = list(WS)
            ws[k] = bad
            with pytest.raises(ValueError, match="must be numbers"):
                _chk(ws=ws)


# ---------------------------------------------------------------------------------------------- the envs of this file
POSE, FRAMES, TERM, BODIES, RESTART, VEL = "pose", "frames", "term", "bodies", "restart", "velocity"
ALL = (POSE, FRAMES, TERM, BODIES, RESTART)


def _vel(lead, seed=2):
    rng = np.random.default_rng(seed)
    return rng.normal(size=lead + (3,)), rng.normal(size=lead + (3,)), rng.normal(size=lead + (NV - 6,))


def _kwargs(options, lead=(T,), nbody=None, **more):
    kw = dict(track_pos=np.zeros(lead + (3,)), xml_path="rodent_optimized.xml", device="cpu")
    if POSE in options:
        kw.update(track_quat=np.broadcast_to([1.0, 0.0, 0.0, 0.0], lead + (4,)), track_joints=np.zeros(lead + (NQ - 7,)))
    if FRAMES in options:
        kw.update(reference_obs_frames=2)
    if TERM in options:
        kw.update(max_pos_error=1.0)
    if BODIES in options:
        kw.update(track_bodies=np.zeros(lead + (nbody, 3)), end_effector_ids=[3])
    if RESTART in options:
        kw.update(clip_restarts=K)
    if VEL in options:
        lin, ang, joint = _vel(lead)
        kw.update(track_velocity=lin, track_angular_velocity=ang, track_joint_velocity=joint, lin_vel_reward_weight=WS[0], lin_vel_reward_scale=WS[1],
                  ang_vel_reward_weight=WS[2], ang_vel_reward_scale=WS[3], joint_vel_reward_weight=WS[4], joint_vel_reward_scale=WS[5])
    kw.update(more)
    return kw


def _make(options, lead=(T,), **more):
    nbody = rodent.Rodent(num_envs=1, **_kwargs(())).sys.nbody if BODIES in options else None
    kw = _kwargs(options, lead, nbody, **more)
    return rodent.Rodent(num_envs=N, **kw), kw


# ---------------------------------------------------------------------------------------------- the start state
def test_reset_qvel_is_the_row_plus_the_noise():
    rng = np.random.default_rng(3)
    rows = rng.normal(size=(C, 7, NV)).astype(np.float32)
    noise = rng.uniform(-0.01, 0.01, size=(5, NV)).astype(np.float32)
    frame, clip = np.array([0, 6, 3, 99, -2], dtype=np.int32), np.array([1, 0, 1, 1, 0], dtype=np.int32)
    got = rodent.reset_qvel(rows, frame, noise, clip)
    assert got.dtype == np.float32 and got.shape == (5, NV)
    for e in range(5):
        f = min(max(int(frame[e]), 0), 6)             # the frame clamped within the clip
        for i in range(NV):
            assert got[e, i] == np.float32(rows[clip[e], f, i]) + noise[e, i]
    single = rodent.reset_qvel(rows[1], frame, noise)
    assert np.array_equal(single, rodent.reset_qvel(rows, frame, noise, np.ones(5, dtype=np.int32)))
    assert np.array_equal(rodent.reset_qvel(rows.astype(np.float64), frame, noise, clip), got)       # float32(row) first, then a float32 sum


def _reset_qvels(env):
    return [a[0]["qvel"] for n, a, _ in env._batch.calls if n == "env_reset"]


@pytest.mark.parametrize("lead", [(T,), (C, T)], ids=["one clip", "clip axis"])
@pytest.mark.parametrize("options", [(POSE, VEL), (POSE, VEL, RESTART)], ids=["K=0", "K=3"])
def test_the_qvel_every_reset_launch_is_handed(options, lead):
    keys = jax_random.split(jax_random.PRNGKey(11), N)
    entries = K if RESTART in options else 1
    num_clips = C if len(lead) == 2 else None
    env, _ = _make(options, lead, reset_to_reference=True)
    frames, _, noise, clip = rodent.restart_bank_draws(keys, entries, NQ, NV, env._reset_noise_scale, env.restart_frame_range, num_clips)
    env._batch.calls.clear()
    s = env.reset(keys)
    got = _reset_qvels(env)
    assert len(got) == entries
    assert env._vel_host.dtype == np.float32 and env._vel_host.shape == lead + (NV,) and np.array_equal(env._track_vel.numpy(), env._vel_host)
    for k in range(entries):
        want = rodent.reset_qvel(env._vel_host, frames[k], noise[k], clip)
        assert got[k].dtype == torch.float32 and np.array_equal(got[k].numpy(), want), k
        assert not np.array_equal(want, noise[k])
    assert s.pipeline_state.qvel is got[0]
    if RESTART in options:
        assert np.array_equal(s.info["restart_bank"]["pipeline_state"].qvel.numpy(), np.stack([g.numpy() for g in got]))
    # without reset_to_reference, and without the arrays: the bare noise, what `reset_draws` gives
    for other in (_make(options, lead)[0], _make(tuple(o for o in options if o != VEL), lead, reset_to_reference=True)[0]):
        other._batch.calls.clear()
        other.reset(keys)
        bare = _reset_qvels(other)
        assert len(bare) == entries
        for k in range(entries):
            assert np.array_equal(bare[k].numpy(), noise[k]), k
        assert np.array_equal(bare[0].numpy(), rodent.reset_draws(keys, NQ, NV, other._reset_noise_scale, num_clips)[2])


# ---------------------------------------------------------------------------------------------- what reaches the batch
OLD = ["pos_reward", "reward_quadctrl", "reward_alive"]
BY_OPTION = {POSE: ["quat_reward", "joint_reward"], TERM: ["pose_fail", "pose_fail_pos", "pose_fail_quat", "pose_fail_joint"],
             BODIES: ["body_reward", "endeff_reward"], VEL: VEL_METRICS}


@pytest.mark.parametrize("options", [(POSE, VEL), (POSE, BODIES, VEL), ALL + (VEL,)], ids=["pose+velocity", "pose+bodies+velocity", "all+velocity"])
def test_what_reaches_the_batch_and_what_comes_back(options):
    env, _ = _make(options)
    assert env.velocity_tracking == dict(lin_vel_reward=(WS[0], WS[1]), ang_vel_reward=(WS[2], WS[3]), joint_vel_reward=(WS[4], WS[5]))
    want_metrics = OLD + [m for o in (POSE, TERM, BODIES, VEL) if o in options for m in BY_OPTION[o]]
    keys = jax_random.split(jax_random.PRNGKey(3), N)
    s0 = env.reset(keys)
    io = env._batch.last_env_io("env_reset")
    assert not (VEL_KEYS & set(io))                                   # a reset has no reward: it hands no velocity block
    assert list(s0.metrics) == want_metrics and all(float(s0.metrics[k].abs().max()) == 0.0 for k in VEL_METRICS)
    assert len({s0.metrics[k].data_ptr() for k in want_metrics}) == len(want_metrics)

    def check(io, state):
        assert VEL_KEYS <= set(io)
        assert io["track_vel"] is env._track_vel and tuple(io["track_vel"].shape) == (T, NV) and io["track_vel"].dtype == torch.float32
        assert (io["lin_vel_reward"], io["ang_vel_reward"], io["joint_vel_reward"]) == ((WS[0], WS[1]), (WS[2], WS[3]), (WS[4], WS[5]))
        buf = io["vel_metrics"]
        assert tuple(buf.shape) == (N, 3) and buf.dtype == torch.float32 and buf.is_contiguous()
        assert list(state.metrics) == want_metrics
        for j, name in enumerate(VEL_METRICS):                        # column j of the launch's buffer, as a view
            m = state.metrics[name]
            assert m._base is buf and m.data_ptr() == buf[:, j].data_ptr() and m.stride() == (3,) and tuple(m.shape) == (N,), name
        assert ("track_bodies" in io) == (BODIES in options) and ("pose_fail" in io) == (TERM in options) and "track_pose" in io
    s1 = env.step(s0, torch.zeros(N, env.action_size))
    check(env._batch.last_env_io("env_step_to"), s1)
    wenv = wrappers.wrap(env, episode_length=5)
    w1 = wenv.unroll(wenv.reset(keys), torch.zeros(2, N, env.action_size))
    io = env._batch.last_env_io("env_unroll")
    check(io, w1)
    assert ("restart" in io) == (RESTART in options)


@pytest.mark.parametrize("options", [(), (POSE,), (POSE, BODIES), ALL], ids=["none", "pose", "pose+bodies", "all"])
def test_without_the_arrays_nothing_of_the_option_appears(options):
    env, _ = _make(options)
    assert env.velocity_tracking is None and env._track_vel is None
    keys = jax_random.split(jax_random.PRNGKey(3), N)
    s1 = env.step(env.reset(keys), torch.zeros(N, env.action_size))
    assert not (VEL_KEYS & set(env._batch.last_env_io("env_step_to"))) and not (set(VEL_METRICS) & set(s1.metrics))
    assert "velocity_tracking_supported" not in [n for n, _, _ in env._batch.calls]


def test_the_probe_and_its_place_in_the_constructor():
    env, _ = _make(ALL + (VEL,))
    calls = [n for n, _, _ in env._batch.calls if n.endswith("_supported") or n.startswith("set_")]
    assert calls == ["pose_supported", "reference_obs_supported", "set_pose", "set_reference_obs", "pose_termination_supported",
                     "body_tracking_supported", "velocity_tracking_supported", "clip_restarts_supported"]
    env, _ = _make((POSE, VEL))
    assert [n for n, _, _ in env._batch.calls if n.endswith("_supported")] == ["pose_supported", "velocity_tracking_supported"]


def test_a_refused_option_raises_with_the_librarys_text(monkeypatch):
    class Refusing(FakeBatch):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.refuse = {"velocity_tracking_supported": "no"}
    monkeypatch.setattr(base.hip, "Batch", Refusing)
    with pytest.raises(RuntimeError) as e:
        rodent.Rodent(num_envs=N, **_kwargs((POSE, VEL)))
    assert str(e.value) == "Rodent(track_velocity=...): no"


def test_a_sibling_keeps_the_option():
    env, kw = _make(ALL + (VEL,), reset_to_reference=True)
    for k in ("track_velocity", "track_angular_velocity", "track_joint_velocity"):
        assert env._ctor[k] is kw[k]
    sib = env.with_num_envs(2)
    assert sib.num_envs == 2 and sib._batch is not env._batch and sib.velocity_tracking == env.velocity_tracking is not None
    assert np.array_equal(sib._vel_host, env._vel_host) and sib._reset_to_reference


ARMS = [(ALL + (VEL,), "clip_restarts_supported"), ((POSE, FRAMES, TERM, BODIES, VEL), "body_tracking_supported"),
        ((POSE, FRAMES, TERM, VEL), "velocity_tracking_supported"), ((POSE, VEL), "velocity_tracking_supported")]


@pytest.mark.parametrize("options,query", ARMS, ids=["restarts", "bodies", "velocity over termination", "velocity"])
def test_the_query_about_the_in_kernel_actor(options, query):
    """Velocity tracking ranks below body tracking and above pose termination."""
    env, _ = _make(options)
    wenv = wrappers.wrap(env, episode_length=5)
    for ask in (lambda: acting.fused_unroll_supported(wenv, None, None) is False, lambda: env.fused_actor_refusal() is None):
        env._batch.calls.clear()
        assert ask()
        asked = [(n, a, kw) for n, a, kw in env._batch.calls if n.endswith("_supported") and n not in ("unroll_supported", "eval_supported", "env_params_supported")]
        assert [(n, a, kw) for n, a, kw in asked] == [(query, (), {"with_actor": True})]
    env._batch.refuse = {query: "too wide"}
    assert env.fused_actor_refusal() == "too wide"


def test_a_velocity_env_is_a_pose_env_to_the_parameter_setters_and_the_evaluation():
    env, _ = _make((POSE, VEL))
    assert env.pose_tracking and not env.eval_supported()
    with pytest.raises(RuntimeError, match="per-env parameters"):
        env.set_env_params(dof_f=torch.zeros(N, NV, 16))
    with pytest.raises(RuntimeError, match="per-env parameters"):
        env.randomize(lambda sys: (sys, {}))


# ---------------------------------------------------------------------------------------------- ABI
def test_the_ctypes_mirror_matches_the_header():
    header = open(os.path.join(ROOT, "include", "rodent_rr.h")).read()
    m = re.search(r"typedef struct rr_vel_io \{(.*?)\} rr_vel_io;", header, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    members = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.rsplit("*", 1) if "*" in decl else decl.split(None, 1)
        for n in names.split(","):
            members.append((n.strip(), "ptr" if "*" in decl else ctype.strip()))
    want = [("track_vel", "ptr"), ("vel_metrics", "ptr"), ("lin_weight", "float"), ("lin_scale", "float"), ("ang_weight", "float"),
            ("ang_scale", "float"), ("joint_weight", "float"), ("joint_scale", "float")]
    assert members == want, members
    kinds = {"ptr": ctypes.c_void_p, "float": ctypes.c_float}
    assert [(n, t) for n, t in hip.RRVelIO._fields_] == [(n, kinds[k]) for n, k in members]
    offsets = [getattr(hip.RRVelIO, n).offset for n, _ in members]
    assert offsets == [0, 8, 16, 20, 24, 28, 32, 36] and ctypes.sizeof(hip.RRVelIO) == 40
    for decl in ("int rr_batch_set_velocity_tracking(rr_batch* b, const rr_vel_io* vel);",
                 "int rr_batch_velocity_tracking_supported(const rr_batch* b, int32_t with_actor);"):
        assert decl in header


def test_the_two_exports_and_their_signatures():
    for name in ("rr_batch_set_velocity_tracking", "rr_batch_velocity_tracking_supported"):
        assert name in hip.EXPORTS
    lib = hip.lib()
    assert lib.rr_batch_set_velocity_tracking.argtypes == [ctypes.c_void_p, ctypes.POINTER(hip.RRVelIO)]
    assert lib.rr_batch_velocity_tracking_supported.argtypes == [ctypes.c_void_p, ctypes.c_int32]
    assert lib.rr_batch_set_velocity_tracking(None, None) == -1 and b"null batch" in lib.rr_last_error()          # RR_EINVAL, no device needed
    assert lib.rr_batch_velocity_tracking_supported(None, 0) == -1 and b"null batch" in lib.rr_last_error()
    assert hasattr(REAL_BATCH, "set_velocity_tracking") and hasattr(REAL_BATCH, "velocity_tracking_supported")


# ---------------------------------------------------------------------------------------------- the example
def test_the_example_refuses_velocity_without_pose(monkeypatch, capsys):
    spec = importlib.util.spec_from_file_location("rodent_run_ppo_example", os.path.join(ROOT, "examples", "rodent_run_ppo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr("sys.argv", ["rodent_run_ppo.py", "--track-velocity"])
    with pytest.raises(SystemExit) as e:
        mod.main()
    assert e.value.code == 2
    last = capsys.readouterr().err.strip().splitlines()[-1]
    assert last == "rodent_run_ppo.py: error: --track-velocity: the velocities are indexed like the reference pose; add --track-pose"
