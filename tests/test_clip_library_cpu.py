"""The clip library without a GPU (`Rodent(clip_lengths=..., restart_across_clips=True)`): the draws of the bank's
clips, the fold of the start frames, padding that nothing reads, the two composed wrappers on a frame-counting fake env, every
ValueError, the ABI, what `Rodent` hands its batch (the recording fake batch of tests/test_env_io_options_cpu.py), the loader of unequal
clips, and the host bookkeeping of the GPU fixture (tests/clip_library_fixture.py).  The GPU half is tests/test_gpu_clip_library.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from rodent_amd import hip, jax_random, preprocessing
from rodent_amd.envs import base, rodent, wrappers
from rodent_amd.envs.base import State
from tests import clip_library_fixture as X
from tests.test_env_io_options_cpu import FakeBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NQ, NV = 74, 73
KEYS = jax_random.split(jax_random.PRNGKey(5), 6)


# ---------------------------------------------------------------------------------------------- draws
def test_the_banks_clips_are_the_draws_today_discards_and_nothing_else_moves():
    K, C = 4, 5
    old = rodent.restart_bank_draws(KEYS, K, NQ, NV, 0.01, (3, 40), C)
    new = rodent.restart_bank_draws(KEYS, K, NQ, NV, 0.01, (3, 40), C, across_clips=True)
    for a, b in zip(old[:3], new[:3]):                  # start frames, noise, qvel: unchanged
        assert np.array_equal(a, b)
    assert old[3].shape == (6,) and new[3].shape == (K, 6) and new[3].dtype == np.int32
    assert np.array_equal(new[3][0], old[3])            # entry 0: the reset's clip
    for k in range(1, K):
        assert np.array_equal(new[3][k], rodent.reset_draws(jax_random.fold_in(KEYS, k), NQ, NV, 0.01, num_clips=C)[3])
    again = rodent.restart_bank_draws(KEYS.copy(), K, NQ, NV, 0.01, (3, 40), C, across_clips=True)
    assert all(np.array_equal(a, b) for a, b in zip(new, again))
    assert len({tuple(r) for r in new[3].tolist()}) > 1          # the entries do differ
    assert rodent.restart_bank_draws(KEYS, K, NQ, NV, 0.01, (3, 40), None, across_clips=True)[3] is None


def test_the_fold_is_draw_mod_length_minus_one_and_the_identity_below_it():
    L = np.array([104, 14, 9])
    draws = np.array([[0, 12, 13, 7, 8, 103], [102, 99, 5, 90, 101, 8]], dtype=np.int32)
    clips = np.array([[0, 1, 1, 2, 2, 0], [0, 1, 2, 2, 1, 2]])
    got = rodent.fold_start_frames(draws, L, clips)
    assert got.dtype == np.int32 and np.array_equal(got, draws % (L[clips] - 1))
    assert np.array_equal(got, [[0, 12, 0, 7, 0, 0], [102, 8, 5, 2, 10, 0]])
    same = draws < L[clips] - 1
    assert np.array_equal(got[same], draws[same]) and (got <= L[clips] - 2).all()
    assert rodent.fold_start_frames(draws, None, clips) is not None and np.array_equal(rodent.fold_start_frames(draws, None), draws)
    assert np.array_equal(rodent.fold_start_frames(np.array([5, 9, 20]), np.array([10])), [5, 0, 2])      # no clip axis: clip 0


# ---------------------------------------------------------------------------------------------- env construction on the fake batch
@pytest.fixture
def fake_batch(monkeypatch):
    monkeypatch.setattr(base.hip, "Batch", FakeBatch)


N, T, C, K = 4, 30, 3, 3
LENGTHS = [30, 12, 7]


def _clips(nan_padding=False):
    """Three clips whose rows say which (clip, frame) they are; rows at or behind L_c are NaN on request."""
    c, t = np.arange(C, dtype=np.float64)[:, None, None], np.arange(T, dtype=np.float64)[None, :, None]
    pos = np.concatenate([0.01 * t + 0 * c, 0.1 * c + 0 * t, 0.07 + 0 * t + 0 * c], axis=-1)
    ang = 0.1 * (c + 1) + 0.003 * t
    quat = np.concatenate([np.cos(ang / 2), 0 * ang, 0 * ang, np.sin(ang / 2)], axis=-1)
    joints = 0.01 * c + 0.001 * t + 0.0001 * np.arange(NQ - 7)[None, None]
    vel = 0.5 * c + 0.01 * t + 0.001 * np.arange(NV)[None, None]
    out = dict(track_pos=pos, track_quat=quat, track_joints=joints, track_velocity=vel[..., :3], track_angular_velocity=vel[..., 3:6],
               track_joint_velocity=vel[..., 6:])
    return out


def _nan_padding(arrs, lengths=LENGTHS):
    out = {k: np.array(v, dtype=np.float64) for k, v in arrs.items()}
    for v in out.values():
        for c, L in enumerate(lengths):
            v[c, L:] = np.nan
    return out


def _env(**kw):
    arrs = _clips()
    return rodent.Rodent(num_envs=N, xml_path="rodent_optimized.xml", device="cpu", **arrs, **kw)


def test_reset_draws_folds_and_forms_each_entry_on_its_own_clip(fake_batch):
    env = _env(clip_restarts=K, restart_frame_range=(0, 30), clip_lengths=LENGTHS, restart_across_clips=True, reset_to_reference=True)
    keys = jax_random.split(jax_random.PRNGKey(11), N)
    s = env.reset(keys)
    frames, noise, qvel, clip = rodent.restart_bank_draws(keys, K, NQ, NV, 0.01, (0, 30), C, across_clips=True)
    bank = s.info["restart_bank"]
    assert bank["clip"].dtype == torch.int32 and np.array_equal(bank["clip"].numpy(), clip)
    assert np.array_equal(s.info["clip"].numpy(), clip[0])
    want = frames % (np.asarray(LENGTHS)[clip] - 1)
    assert np.array_equal(bank["frame"].numpy(), want) and (want != frames).any()
    arrs = _clips()
    for k in range(K):
        f, c = want[k], clip[k]
        row = np.concatenate([arrs["track_pos"][c, f], arrs["track_quat"][c, f], arrs["track_joints"][c, f]], axis=-1).astype(np.float32)
        assert np.array_equal(bank["pipeline_state"].qpos[k].numpy(), row + noise[k])
        vrow = np.concatenate([arrs[n][c, f] for n in ("track_velocity", "track_angular_velocity", "track_joint_velocity")], axis=-1).astype(np.float32)
        assert np.array_equal(bank["pipeline_state"].qvel[k].numpy(), vrow + qvel[k])
    # the reset launches: one per entry, each with its own clip ids
    resets = [a for n, a, _ in env._batch.calls if n == "env_reset"]
    assert len(resets) == K
    for k, args in enumerate(resets):
        assert np.array_equal(args[1]["clip"].numpy(), clip[k])
    # explicit ids: [N] sets entry 0 and the others are drawn, [K, N] sets every entry
    ids = np.array([2, 2, 1, 0])
    b1 = env.reset(keys, clip=ids).info
    assert np.array_equal(b1["clip"].numpy(), ids) and np.array_equal(b1["restart_bank"]["clip"].numpy()[0], ids)
    assert np.array_equal(b1["restart_bank"]["clip"].numpy()[1:], clip[1:])
    full = np.array([[0, 1, 2, 0], [1, 1, 1, 1], [2, 0, 2, 0]])
    b2 = env.reset(keys, clip=full).info
    assert np.array_equal(b2["restart_bank"]["clip"].numpy(), full) and np.array_equal(b2["clip"].numpy(), full[0])
    assert np.array_equal(b2["restart_bank"]["frame"].numpy(), frames % (np.asarray(LENGTHS)[full] - 1))
    with pytest.raises(ValueError, match="shape"):
        env.reset(keys, clip=full[:2])
    with pytest.raises(ValueError, match=r"clip ids must lie in \[0, 3\)"):
        env.reset(keys, clip=full + 1)
    plain = _env(clip_restarts=K)
    with pytest.raises(ValueError, match="shape"):       # [K, N] ids need restart_across_clips
        plain.reset(keys, clip=full)
    # a sibling keeps both arguments
    sib = env.with_num_envs(2)
    assert sib.restart_across_clips and sib.clip_lengths.tolist() == LENGTHS


def test_padding_is_never_read_on_the_host(fake_batch):
    arrs = _nan_padding(_clips())
    L = np.asarray(LENGTHS)
    clip = np.array([0, 1, 2, 2, 1, 0])
    frame = np.array([29, 11, 6, 40, 12, 3])            # at and past the clips' ends
    pose = np.concatenate([arrs["track_quat"], arrs["track_joints"]], axis=-1)
    vel = np.concatenate([arrs["track_velocity"], arrs["track_angular_velocity"], arrs["track_joint_velocity"]], axis=-1)
    q0 = np.zeros(NQ)
    zero_q, zero_v = np.zeros((6, NQ), np.float32), np.zeros((6, NV), np.float32)
    qpos = rodent.reset_qpos(q0, arrs["track_pos"], frame, zero_q, clip, pose, L)
    qvel = rodent.reset_qvel(vel, frame, zero_v, clip, L)
    assert np.isfinite(qpos).all() and np.isfinite(qvel).all()
    assert not np.isfinite(rodent.reset_qpos(q0, arrs["track_pos"], frame, zero_q, clip, pose)).all()       # without lengths the padding is met
    fi = np.minimum(frame, L[clip] - 1)
    assert np.array_equal(qpos[:, :3], arrs["track_pos"][clip, fi].astype(np.float32))
    rows = lambda a: rodent.reference_rows(a, frame, clip, L)
    assert np.array_equal(rows(pose), pose[clip, fi])
    state = np.tile(np.concatenate([[0, 0, 0.07, 1, 0, 0, 0], np.zeros(NQ - 7)]), (6, 1))
    for out in (rodent.pose_rewards(state, rows(pose)[:, :4], rows(pose)[:, 4:]),
                rodent.pose_errors(state, rows(arrs["track_pos"]), rows(pose)[:, :4], rows(pose)[:, 4:]),
                rodent.velocity_rewards(np.zeros((6, NV)), rows(vel)),
                rodent.body_rewards(np.zeros((6, 5, 3)), rows(np.repeat(arrs["track_pos"][:, :, None], 5, axis=2)), (1, 2), (3,))):
        assert all(np.isfinite(o).all() for o in out)
    ro = rodent.reference_obs(state, arrs["track_pos"], arrs["track_quat"], arrs["track_joints"], frame, 5, clip=clip, lengths=L)
    assert np.isfinite(ro).all()
    want = rodent.reference_obs(state, *(_clips()[k] for k in ("track_pos", "track_quat", "track_joints")), np.minimum(frame + 5, L[clip] - 1) - 5, 5, clip=clip)
    assert np.array_equal(ro[:, 4 * NQ:], want[:, 4 * NQ:])          # block 5 reads clamp(frame + 5, L_c - 1)
    with np.errstate(invalid="ignore"):
        assert not np.isfinite(rodent.reference_obs(state, arrs["track_pos"], arrs["track_quat"], arrs["track_joints"], frame, 5, clip=clip)).all()
    # single clip, an int length
    one = rodent.reference_rows(arrs["track_pos"][1], np.array([3, 11, 12, 29]), None, np.array([12]))
    assert np.isfinite(one).all() and np.array_equal(one[1:], arrs["track_pos"][1][[11, 11, 11]])


def test_the_env_with_nan_padding_builds_states_without_nan(fake_batch):
    """The constructor refuses non-finite rows, so the padding is poisoned after construction, in the host copies `reset` reads."""
    env = _env(clip_restarts=K, restart_frame_range=(0, 30), clip_lengths=LENGTHS, restart_across_clips=True, reset_to_reference=True)
    for a in (env._track_host, env._pose_host, env._vel_host):
        for c, L in enumerate(LENGTHS):
            a[c, L:] = np.nan
    s = env.reset(jax_random.split(jax_random.PRNGKey(3), N))
    ps = s.info["restart_bank"]["pipeline_state"]
    assert bool(torch.isfinite(ps.qpos).all()) and bool(torch.isfinite(ps.qvel).all())


def test_every_value_error(fake_batch):
    arrs = _clips()
    pos_only = dict(track_pos=arrs["track_pos"], num_envs=N, xml_path="rodent_optimized.xml", device="cpu")
    with pytest.raises(ValueError, match="need the reference pose"):
        rodent.Rodent(clip_lengths=LENGTHS, **pos_only)
    with pytest.raises(ValueError, match="need the reference pose"):
        rodent.Rodent(restart_across_clips=True, **pos_only)
    with pytest.raises(ValueError, match="clip_restarts >= 1"):
        _env(restart_across_clips=True)
    single = {k: v[0] for k, v in arrs.items()}
    with pytest.raises(ValueError, match="no other clip"):
        rodent.Rodent(num_envs=N, xml_path="rodent_optimized.xml", device="cpu", clip_restarts=2, restart_across_clips=True, **single)
    for bad, why in (([30, 12], "shape"), ([30, 12, 7, 7], "shape"), (12, "shape"), ([30.0, 12.0, 7.0], "integers"), ([30, 12, 1], "2 .. T"),
                     ([31, 12, 7], "2 .. T"), ([[30, 12, 7]], "shape")):
        with pytest.raises(ValueError, match=why):
            _env(clip_lengths=bad)
    for ok in (12, [12], np.array([30], dtype=np.int64)):        # a [T, 3] track: an int or [1]
        e = rodent.Rodent(num_envs=N, xml_path="rodent_optimized.xml", device="cpu", clip_lengths=ok, **single)
        assert e.clip_lengths.dtype == torch.int32 and tuple(e.clip_lengths.shape) == (1,)
    # the clip-length refusal of end_at_clip_end stands without lengths and does not apply with them
    with pytest.raises(ValueError, match="truncate on every step"):
        _env(clip_restarts=2, end_at_clip_end=True)
    assert _env(clip_restarts=2, end_at_clip_end=True, clip_lengths=LENGTHS).end_at_clip_end


def test_the_constructor_asks_one_probe_only_when_an_option_is_on(fake_batch):
    asked = lambda env: [n for n, _, _ in env._batch.calls if n == "clip_library_supported"]
    assert asked(_env()) == [] and asked(_env(clip_restarts=2)) == []
    assert len(asked(_env(clip_lengths=LENGTHS))) == 1 and len(asked(_env(clip_restarts=2, restart_across_clips=True))) == 1


def test_a_refusal_of_the_library_is_a_runtime_error(fake_batch, monkeypatch):
    class Refusing(FakeBatch):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.refuse["clip_library_supported"] = "pose tracking: no pose instance here"
    monkeypatch.setattr(base.hip, "Batch", Refusing)
    with pytest.raises(RuntimeError, match=r"clip_lengths=\.\.\. / restart_across_clips=True\): pose tracking: no pose instance here"):
        _env(clip_lengths=LENGTHS)
    _env()          # an env without the options does not ask


# ---------------------------------------------------------------------------------------------- env io
def test_the_io_key_and_the_info_keys_appear_exactly_when_an_option_is_on(fake_batch):
    keys = jax_random.split(jax_random.PRNGKey(2), N)
    acts = torch.zeros(2, N, 38)
    for lengths, across, H in ((None, False, 0), (LENGTHS, False, 0), (None, True, 0), (LENGTHS, True, 0), (LENGTHS, True, 2), (None, False, 2)):
        kw = dict(clip_restarts=K, reference_obs_frames=H)
        if lengths is not None:
            kw.update(clip_lengths=lengths)
        if across:
            kw.update(restart_across_clips=True)
        env = _env(**kw)
        on = lengths is not None or across
        wenv = wrappers.FusedEpisodeAutoResetWrapper(wrappers.VmapWrapper(env), 5)
        s = wenv.reset(keys)
        assert ("clip" in s.info["restart_bank"]) == across
        assert set(s.info["restart_bank"]) == {"pipeline_state", "obs", "frame"} | ({"clip"} if across else set())
        assert set(s.info) == {"cur_frame", "clip", "restart_bank", "restart_slot", "steps", "truncation"}
        rio = env._batch.last_env_io("env_reset")
        # a reset hands the lengths where it runs the instance that reads them (reference frames), never the bank's clips
        assert ("clip_library" in rio) == (lengths is not None and H > 0)
        if "clip_library" in rio:
            assert set(rio["clip_library"]) == {"lengths"} and rio["clip_library"]["lengths"] is env.clip_lengths
        env.step(s, acts[0])
        sio = env._batch.last_env_io("env_step_to")
        assert ("clip_library" in sio) == (lengths is not None)           # the bare step reads the lengths and moves no clip
        if "clip_library" in sio:
            assert set(sio["clip_library"]) == {"lengths"}
        out = env.unroll_wrapped(s, acts, 5)
        uio = env._batch.last_env_io("env_unroll")
        assert ("clip_library" in uio) == on
        assert set(out.info) == set(s.info)
        if on:
            lib = uio["clip_library"]
            assert lib["lengths"] is (env.clip_lengths if lengths is not None else None)
            if across:
                assert lib["bank_clips"] is s.info["restart_bank"]["clip"]
                co = lib["clip_out"]
                assert co.dtype == torch.int32 and tuple(co.shape) == (N,) and co is not s.info["clip"] and co.data_ptr() != s.info["clip"].data_ptr()
                assert out.info["clip"] is co and uio["clip"] is s.info["clip"]
            else:
                assert set(lib) == {"lengths"} and out.info["clip"] is s.info["clip"]
            assert "clip" not in uio["restart"] and set(uio["restart"]) == {"frames", "slot_in", "slot_out", "end_at_clip_end"}
        else:
            assert out.info["clip"] is s.info["clip"]


# ---------------------------------------------------------------------------------------------- composed wrappers on a fake env
class FrameEnv:
    """A frame-counting env with the surface the two Clip wrappers read: never done by itself, obs = (frame, clip)."""

    def __init__(self, frames, clips, lengths=None, end=True, across=True, track_len=20):
        self.frames, self.clips = torch.as_tensor(frames, dtype=torch.int32), torch.as_tensor(clips, dtype=torch.int32)
        self.num_envs = self.frames.shape[1]
        self.clip_restarts, self.end_at_clip_end, self.track_len = self.frames.shape[0], end, track_len
        self.clip_lengths = None if lengths is None else torch.as_tensor(lengths, dtype=torch.int32)
        self.across = across

    def _obs(self, f, c):
        return torch.stack([f.float(), c.float()], dim=-1)

    def reset(self, rng):
        z = torch.zeros(self.num_envs)
        clips = self.clips if self.across else self.clips[:1].expand_as(self.clips)
        bank = dict(pipeline_state={"x": self.frames.float().unsqueeze(-1)}, obs=torch.stack([self._obs(f, c) for f, c in zip(self.frames, clips)]),
                    frame=self.frames.clone())
        if self.across:
            bank["clip"] = self.clips.clone()
        info = {"cur_frame": self.frames[0].clone(), "clip": self.clips[0].clone(), "restart_bank": bank,
                "restart_slot": torch.zeros(self.num_envs, dtype=torch.int32)}
        return State({"x": self.frames[0].float().unsqueeze(-1)}, self._obs(self.frames[0], self.clips[0]), z, z.clone(), {}, info)

    def step(self, state, action):
        info = dict(state.info)
        info["cur_frame"] = info["cur_frame"] + 1
        return state.replace(pipeline_state={"x": state.pipeline_state["x"] + 1}, obs=self._obs(info["cur_frame"], info["clip"]), info=info)


FRAMES = [[0, 3, 1, 0], [2, 0, 4, 5], [1, 1, 0, 2]]
CLIPS = [[0, 1, 2, 0], [1, 1, 0, 2], [2, 0, 1, 2]]
WL = [20, 6, 4]


def _play(env, episode_length, steps):
    w = wrappers.ClipAutoResetWrapper(wrappers.ClipEpisodeWrapper(wrappers.VmapWrapper(env), episode_length, 1))
    s = w.reset(None)
    out = []
    for _ in range(steps):
        s = w.step(s, None)
        out.append({k: s.info[k].clone() for k in ("cur_frame", "clip", "restart_slot", "truncation")} | {"done": s.done.clone(), "obs": s.obs.clone()})
    return out


def _rule(frames, clips, lengths, episode_length, steps, end=True, track_len=20):
    """The rule of section 4s, env by env, in integers."""
    frames, clips = np.asarray(frames), np.asarray(clips)
    Kk, Nn = frames.shape
    out = np.zeros((steps, Nn, 4), dtype=np.int64)           # frame, clip, slot, truncation
    for e in range(Nn):
        f, c, slot, n = frames[0, e], clips[0, e], 0, 0
        for t in range(steps):
            n, nf = n + 1, f + 1
            L = track_len if lengths is None else lengths[c]
            over = n >= episode_length or (end and nf >= L - 1)
            if over:
                slot = (slot + 1) % Kk
                f, c, n = frames[slot, e], clips[slot, e], 0
            else:
                f = nf
            out[t, e] = (f, c, slot, over)
    return out


def test_the_composed_wrappers_follow_the_bank_and_the_envs_own_length():
    got = _play(FrameEnv(FRAMES, CLIPS, WL), 5, 12)
    want = _rule(FRAMES, CLIPS, WL, 5, 12)
    for t, g in enumerate(got):
        assert np.array_equal(g["cur_frame"].numpy(), want[t, :, 0]) and np.array_equal(g["clip"].numpy(), want[t, :, 1]), t
        assert np.array_equal(g["restart_slot"].numpy(), want[t, :, 2]) and np.array_equal(g["truncation"].numpy(), want[t, :, 3]), t
        assert np.array_equal(g["obs"][:, 0].numpy(), want[t, :, 0]) and np.array_equal(g["obs"][:, 1].numpy(), want[t, :, 1]), t
    assert (want[:, :, 1] != np.asarray(CLIPS)[0]).any()            # clips did move
    # an env that never restores keeps its clip: episodes longer than the run, clip 0 has 20 frames
    quiet = _play(FrameEnv(FRAMES, CLIPS, WL), 100, 3)
    assert all(np.array_equal(g["clip"].numpy()[[0, 3]], [0, 0]) and not g["done"][[0, 3]].any() for g in quiet)
    # the clip's end: env 1 starts on clip 1 (6 frames) at frame 3 and ends when new_frame reaches 5, not 19
    assert [int(g["truncation"][1]) for g in quiet] == [0, 1, 0]


def test_with_both_options_off_the_two_wrappers_behave_as_today():
    got = _play(FrameEnv(FRAMES, CLIPS, None, across=False, track_len=6), 5, 12)
    want = _rule(FRAMES, np.broadcast_to(np.asarray(CLIPS)[0], (3, 4)), None, 5, 12, track_len=6)
    for t, g in enumerate(got):
        assert np.array_equal(g["cur_frame"].numpy(), want[t, :, 0]) and np.array_equal(g["clip"].numpy(), np.asarray(CLIPS)[0]), t
        assert np.array_equal(g["restart_slot"].numpy(), want[t, :, 2]) and np.array_equal(g["truncation"].numpy(), want[t, :, 3]), t
    # lengths alone: the clip's end moves, the clip stays
    got = _play(FrameEnv(FRAMES, CLIPS, WL, across=False), 5, 12)
    want = _rule(FRAMES, np.broadcast_to(np.asarray(CLIPS)[0], (3, 4)), WL, 5, 12)
    for t, g in enumerate(got):
        assert np.array_equal(g["cur_frame"].numpy(), want[t, :, 0]) and np.array_equal(g["clip"].numpy(), np.asarray(CLIPS)[0]), t


# ---------------------------------------------------------------------------------------------- ABI
def test_the_ctypes_mirror_matches_the_header():
    header = open(os.path.join(ROOT, "include", "rodent_rr.h")).read()
    m = re.search(r"typedef struct rr_clip_library_io \{(.*?)\} rr_clip_library_io;", header, re.S)
    assert m
    members = []
    for decl in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(";"):
        decl = decl.strip()
        if decl:
            assert "*" in decl and "int32_t" in decl, decl
            members.append(decl.split("*")[-1].strip())
    assert members == ["clip_lengths", "bank_clips", "clip_out"]
    assert [(n, t) for n, t in hip.RRClipLibraryIO._fields_] == [(n, ctypes.c_void_p) for n in members]
    assert [getattr(hip.RRClipLibraryIO, n).offset for n in members] == [0, 8, 16] and ctypes.sizeof(hip.RRClipLibraryIO) == 24
    for decl in ("int rr_batch_set_clip_library(rr_batch* b, const rr_clip_library_io* lib);",
                 "int rr_batch_clip_library_supported(const rr_batch* b, int32_t with_actor);", "int rr_wrap_clip_library(int32_t num_envs,",
                 "int32_t* clip, const int32_t* bank_clips, const int32_t* clip_lengths, void* stream);"):
        assert decl in header, decl


def test_the_closed_structs_keep_their_sizes():
    assert ctypes.sizeof(hip.RRPoseIO) == 32 and ctypes.sizeof(hip.RRPoseTermIO) == 24 and ctypes.sizeof(hip.RRBodyIO) == 40
    assert ctypes.sizeof(hip.RRClipRestartIO) == 32 and ctypes.sizeof(hip.RRVelIO) == 40 and ctypes.sizeof(hip.RRUnrollIO) == 80
    assert [n for n, _ in hip.RRClipRestartIO._fields_] == ["frames", "slot_in", "slot_out", "num_slots", "end_at_clip_end"]
    assert len(hip.lib().rr_wrap_clip_restart.argtypes) == 20


def test_the_three_exports_and_their_signatures():
    for name in ("rr_batch_set_clip_library", "rr_batch_clip_library_supported", "rr_wrap_clip_library"):
        assert name in hip.EXPORTS
    lib = hip.lib()
    assert lib.rr_batch_set_clip_library.argtypes == [ctypes.c_void_p, ctypes.POINTER(hip.RRClipLibraryIO)]
    assert lib.rr_batch_clip_library_supported.argtypes == [ctypes.c_void_p, ctypes.c_int32]
    restart = lib.rr_wrap_clip_restart.argtypes
    assert lib.rr_wrap_clip_library.argtypes == restart[:-1] + [ctypes.c_void_p] * 3 + [restart[-1]] and len(lib.rr_wrap_clip_library.argtypes) == 23
    assert lib.rr_batch_set_clip_library(None, None) == -1 and b"null batch" in lib.rr_last_error()
    assert lib.rr_batch_clip_library_supported(None, 0) == -1 and b"null batch" in lib.rr_last_error()
    args = [1, 0, None, None, None] + [None] * 5 + [5.0, 1.0] + [None] * 4 + [1, 10, 0] + [None] * 4
    assert lib.rr_wrap_clip_library(*args) == -1 and b"rr_wrap_clip_library: bad argument" in lib.rr_last_error()


# ---------------------------------------------------------------------------------------------- the loader
def test_load_reference_clips_pads_by_the_last_row_and_returns_the_lengths(tmp_path):
    rng = np.random.default_rng(0)
    path = str(tmp_path / "clips.npz")
    lens = {"a": 7, "b": 4, "c": 5}
    clips = {n: preprocessing.ReferenceClip(position=rng.normal(size=(L, 3)), quaternion=rng.normal(size=(L, 4)), joints=rng.normal(size=(L, 67)),
                                            velocity=rng.normal(size=(L, 3))) for n, L in lens.items()}
    items = {f"{n}/{a}": getattr(c, a) for n, c in clips.items() for a in ("position", "quaternion", "joints", "velocity")}
    np.savez(path, **items)
    got, lengths = preprocessing.load_reference_clips(path, ["b", "a", "c"])
    assert lengths.dtype == np.int32 and lengths.tolist() == [4, 7, 5]
    assert got.position.shape == (3, 7, 3) and got.joints.shape == (3, 7, 67) and got.body_positions is None
    for i, n in enumerate(["b", "a", "c"]):
        L = lens[n]
        for a in ("position", "quaternion", "joints", "velocity"):
            arr, src = getattr(got, a)[i], getattr(clips[n], a)
            assert np.array_equal(arr[:L], src) and np.array_equal(arr[L:], np.repeat(src[-1:], 7 - L, axis=0)), (n, a)
    with pytest.raises(ValueError):
        preprocessing.load_reference_clip(path, ["a", "b"])            # the old loader stacks: unequal clips fail as before
    same = preprocessing.load_reference_clip(path, ["a"])
    assert np.array_equal(same.position[0], clips["a"].position)


# ---------------------------------------------------------------------------------------------- the GPU fixture's bookkeeping
def test_the_gpu_fixtures_draws_hold_its_conditions():
    by_end, by_len, changed = X.counts(3)
    print(f"restores by the clip's end per clip {by_end}, by episode_length {by_len}, clip changes {changed}, of {X.N * X.STEPS} pairs")
    assert all(n >= 5 for n in by_end) and by_len >= 30 and changed >= 30
    frames, clips = X.bank(3)
    assert (frames <= X.LENGTHS[clips] - 2).all() and np.array_equal(clips[0], X.IDS)
    raw = rodent.restart_bank_draws(X.keys(), 3, X.NQ, X.NV, X.NOISE, X.RANGE, X.C, True)
    assert np.array_equal(frames, raw[0] % (X.LENGTHS[clips] - 1)) and np.array_equal(clips[1:], raw[3][1:])
    # without restart_across_clips no env ever changes its clip; with lengths off the short clips never end
    assert X.schedule(3, across=False)["changed"].sum() == 0
    s = X.schedule(3, lengths=False)
    assert (s["by_end"] * (s["clip_before"] > 0)).sum() < X.schedule(3)["by_end"].sum()
