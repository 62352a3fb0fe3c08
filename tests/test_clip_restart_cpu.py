"""Clip restarts (`Rodent(clip_restarts=K, restart_frame_range=, end_at_clip_end=)`; rr_batch_set_clip_restarts) as far as they can be held
without a GPU: the host draws of the start bank, the two composed wrappers (`ClipEpisodeWrapper`, `ClipAutoResetWrapper`) on a small env
that counts frames, every refusal of the constructor's argument check through the helper it calls, and the ctypes mirror of
`rr_clip_restart_io` against the header.  The GPU half is tests/test_gpu_clip_restart.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from rodent_amd import hip, jax_random
from rodent_amd.envs import rodent, wrappers
from rodent_amd.envs.base import PipelineState, State

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NQ, NV = 74, 73
KEYS = jax_random.split(jax_random.PRNGKey(7), 12)


# ---------------------------------------------------------------------------------------------- bank draws
@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_entry_zero_is_the_reset_draw_whatever_k_is(K):
    f0, n0, v0, c0 = rodent.reset_draws(KEYS, NQ, NV, 0.01, 3)
    f, n, v, c = rodent.restart_bank_draws(KEYS, K, NQ, NV, 0.01, (10, 20), 3)
    assert f.shape == (K, 12) and f.dtype == np.int32 and n.shape == (K, 12, NQ) and v.shape == (K, 12, NV) and n.dtype == np.float32
    assert np.array_equal(f[0], f0) and np.array_equal(n[0], n0) and np.array_equal(v[0], v0) and np.array_equal(c, c0)
    assert rodent.restart_bank_draws(KEYS, K, NQ, NV, 0.01, (10, 20))[3] is None          # no clip axis: no ids, the other draws as they are
    assert np.array_equal(rodent.restart_bank_draws(KEYS, K, NQ, NV, 0.01, (10, 20))[1], n)


def test_entry_k_is_the_reset_draw_of_the_folded_key_except_the_frame():
    lo, hi = 37, 45
    f, n, v, _ = rodent.restart_bank_draws(KEYS, 5, NQ, NV, 0.02, (lo, hi), 3)
    for k in range(1, 5):
        kk = jax_random.fold_in(KEYS, k)
        fk, nk, vk, _ = rodent.reset_draws(kk, NQ, NV, 0.02, 3)
        assert np.array_equal(n[k], nk) and np.array_equal(v[k], vk)
        want = jax_random.randint(jax_random.split(kk, 4)[:, 0], lo, hi)      # the key's first subkey, the one reset_draws takes its frame from
        assert np.array_equal(f[k], want) and (f[k] >= lo).all() and (f[k] < hi).all()
        assert not np.array_equal(n[k], n[0])
    assert len(np.unique(f[1:])) > 1                                                # the range is used, not one frame
    assert ((f[0] >= 0) & (f[0] < 100)).all()                                       # entry 0 keeps the reference's own range
    full = rodent.restart_bank_draws(KEYS, 5, NQ, NV, 0.02, (0, 100), 3)[0]
    for k in range(1, 5):                                                           # (0, 100): the frame reset_draws itself gives for that key
        assert np.array_equal(full[k], rodent.reset_draws(jax_random.fold_in(KEYS, k), NQ, NV, 0.02, 3)[0])


def test_equal_keys_give_equal_banks():
    a = rodent.restart_bank_draws(KEYS, 4, NQ, NV, 0.01, (0, 60), 2)
    b = rodent.restart_bank_draws(KEYS.copy(), 4, NQ, NV, 0.01, (0, 60), 2)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    other = rodent.restart_bank_draws(jax_random.split(jax_random.PRNGKey(8), 12), 4, NQ, NV, 0.01, (0, 60), 2)
    assert not np.array_equal(a[1], other[1])


def test_reset_to_reference_starts_entry_k_from_the_clips_row_at_its_frame():
    rng = np.random.default_rng(0)
    C_, T = 3, 104
    track = rng.normal(size=(C_, T, 3)).astype(np.float32)
    pose = rng.normal(size=(C_, T, NQ - 3)).astype(np.float32)
    qpos0 = rng.normal(size=NQ).astype(np.float32)
    f, n, _, clip = rodent.restart_bank_draws(KEYS, 3, NQ, NV, 0.01, (50, 100), C_)
    for k in range(3):
        qpos = rodent.reset_qpos(qpos0, track, f[k], n[k], clip, pose)
        assert np.array_equal(qpos[:, 3:], pose[clip, f[k]] + n[k][:, 3:])
        assert np.array_equal(qpos[:, :3], track[clip, f[k]] + n[k][:, :3])
        plain = rodent.reset_qpos(qpos0, track, f[k], n[k], clip, None)
        assert np.array_equal(plain[:, 3:], qpos0[3:] + n[k][:, 3:])


def test_the_gpu_fixtures_draws_give_restores_of_both_causes():
    """tests/test_gpu_clip_restart.py's seed, checked where no GPU is needed: integer bookkeeping of the rule on the host draws alone."""
    from tests import test_gpu_clip_restart as G
    assert (G._schedule_counts(1), G._schedule_counts(3)) == ((60, 8), (63, 20))
    for K in (1, 3):
        for n in G._schedule_counts(K):
            assert 8 <= n <= 3 * G.N * G.STEPS // 4


# ---------------------------------------------------------------------------------------------- the composed wrappers
class CountingEnv:
    """N envs whose state is the frame they are at: qpos = [frame, env id], obs = [frame]; `step` moves one frame on and is done where
    the script says so (`done_at`: set of (env, frame reached))."""

    def __init__(self, N, K, T, starts, end_at_clip_end=False, done_at=()):
        self.num_envs, self.clip_restarts, self.track_len, self.end_at_clip_end = N, K, T, end_at_clip_end
        self.starts = np.asarray(starts, dtype=np.int32).reshape(max(K, 1), N)
        self.done_at = set(done_at)

    @property
    def unwrapped(self):
        return self

    def _ps(self, frames):
        f = torch.as_tensor(frames, dtype=torch.float32)
        ids = torch.arange(self.num_envs, dtype=torch.float32).expand_as(f)
        z = torch.zeros(f.shape + (1,))
        return PipelineState(qpos=torch.stack([f, ids], -1), qvel=z.clone(), act=z.clone(), qacc_warmstart=z.clone())

    def reset(self, rng):
        N = self.num_envs
        info = {"cur_frame": torch.as_tensor(self.starts[0].copy())}
        if self.clip_restarts:
            info["restart_bank"] = dict(pipeline_state=self._ps(self.starts), obs=torch.as_tensor(self.starts, dtype=torch.float32)[..., None],
                                        frame=torch.as_tensor(self.starts.copy()))
            info["restart_slot"] = torch.zeros(N, dtype=torch.int32)
        return State(self._ps(self.starts[0]), torch.as_tensor(self.starts[0], dtype=torch.float32)[:, None], torch.zeros(N), torch.zeros(N), {}, info)

    def step(self, state, action):
        frame = state.info["cur_frame"] + 1
        # the state moves on from where it IS (qpos), which after a restore must be the frame the info says
        assert torch.equal(state.pipeline_state.qpos[:, 0], state.info["cur_frame"].float())
        done = torch.tensor([1.0 if (e, int(frame[e])) in self.done_at else 0.0 for e in range(self.num_envs)])
        info = dict(state.info)
        info["cur_frame"] = frame
        return State(self._ps(frame.numpy()), frame.float()[:, None], torch.ones(self.num_envs), done, {}, info)


def _wrap(env, episode_length):
    w = wrappers.ClipAutoResetWrapper(wrappers.ClipEpisodeWrapper(wrappers.VmapWrapper(env), episode_length, 1))
    return w, w.reset(None)


def _row(s):
    return (s.info["cur_frame"].tolist(), s.info["restart_slot"].tolist(), s.done.tolist(), s.info["truncation"].tolist(), s.info["steps"].tolist())


def test_wrap_chooses_the_clip_wrappers_for_an_env_with_a_bank():
    w = wrappers.wrap(CountingEnv(2, 1, 50, [[3, 4]]), episode_length=5)
    assert isinstance(w, wrappers.ClipAutoResetWrapper) and isinstance(w.env, wrappers.ClipEpisodeWrapper)
    w0 = wrappers.wrap(CountingEnv(2, 0, 50, [[3, 4]]), episode_length=5)
    assert type(w0) is wrappers.AutoResetWrapper and type(w0.env) is wrappers.EpisodeWrapper


def test_k1_restores_the_frame_with_the_state():
    w, s = _wrap(CountingEnv(2, 1, 1000, [[40, 7]]), 3)
    assert s.info["restart_slot"].dtype == torch.int32 and _row(s)[:2] == ([40, 7], [0, 0])
    rows = []
    for _ in range(7):
        s = w.step(s, None)
        rows.append(_row(s))
        assert torch.equal(s.pipeline_state.qpos[:, 0], s.info["cur_frame"].float()) and torch.equal(s.obs[:, 0], s.info["cur_frame"].float())
        assert s.info["cur_frame"].dtype == torch.int32 and s.info["restart_slot"].dtype == torch.int32
    assert [r[0] for r in rows] == [[41, 8], [42, 9], [40, 7], [41, 8], [42, 9], [40, 7], [41, 8]]
    assert [r[2] for r in rows] == [[0, 0], [0, 0], [1, 1], [0, 0], [0, 0], [1, 1], [0, 0]]
    assert [r[3] for r in rows] == [r[2] for r in rows]                     # the env itself is never done: every end is a truncation
    assert [r[4] for r in rows] == [[1, 1], [2, 2], [3, 3], [1, 1], [2, 2], [3, 3], [1, 1]]      # steps restarts from 0
    assert all(r[1] == [0, 0] for r in rows)


def test_k3_cycles_through_the_bank():
    w, s = _wrap(CountingEnv(2, 3, 1000, [[40, 7], [60, 0], [11, 99]]), 2)
    frames, slots = [], []
    for _ in range(8):
        s = w.step(s, None)
        frames.append(s.info["cur_frame"].tolist()); slots.append(s.info["restart_slot"].tolist())
        assert torch.equal(s.pipeline_state.qpos[:, 0], s.info["cur_frame"].float()) and torch.equal(s.obs[:, 0], s.info["cur_frame"].float())
        assert torch.equal(s.pipeline_state.qpos[:, 1], torch.tensor([0.0, 1.0]))          # every env restores its OWN column of the bank
    assert slots == [[0, 0], [1, 1], [1, 1], [2, 2], [2, 2], [0, 0], [0, 0], [1, 1]]
    assert frames == [[41, 8], [60, 0], [61, 1], [11, 99], [12, 100], [40, 7], [41, 8], [60, 0]]


def test_the_envs_own_done_restores_too_and_each_env_keeps_its_own_slot():
    w, s = _wrap(CountingEnv(2, 3, 1000, [[40, 7], [60, 0], [11, 99]], done_at={(1, 8), (1, 1)}), 100)
    out = []
    for _ in range(3):
        s = w.step(s, None)
        out.append(_row(s))
    assert out[0] == ([41, 0], [0, 1], [0, 1], [0, 0], [1, 1])               # env 1 fails at once: a termination (truncation 0), next entry
    assert out[1] == ([42, 99], [0, 2], [0, 1], [0, 0], [2, 1])              # ... and again from frame 0 -> 1
    assert out[2] == ([43, 100], [0, 2], [0, 0], [0, 0], [3, 1])


def test_the_clip_end_truncates_unless_the_env_is_done_on_the_same_step():
    T = 50
    env = CountingEnv(3, 2, T, [[46, 46, 10], [20, 20, 20]], end_at_clip_end=True, done_at={(1, 49)})
    w, s = _wrap(env, 1000)
    for want_frame in ([47, 47, 11], [48, 48, 12]):
        s = w.step(s, None)
        assert _row(s)[0] == want_frame and _row(s)[2] == [0, 0, 0]
    s = w.step(s, None)                                                      # new_frame = 49 = T - 1: no next frame left
    assert _row(s) == ([20, 20, 13], [1, 1, 0], [1, 1, 0], [1, 0, 0], [3, 3, 3])      # env 0 truncated; env 1 its own done: truncation 0
    s = w.step(s, None)
    assert _row(s) == ([21, 21, 14], [1, 1, 0], [0, 0, 0], [0, 0, 0], [1, 1, 4])
    off, s0 = _wrap(CountingEnv(1, 1, T, [[46]], end_at_clip_end=False), 1000)    # without the flag the frame runs past the clip as today
    for _ in range(6):
        s0 = off.step(s0, None)
    assert _row(s0) == ([52], [0], [0], [0], [6])


def test_an_env_that_is_never_done_keeps_slot_zero_and_counts_frames_as_today():
    w, s = _wrap(CountingEnv(2, 3, 1000, [[5, 6], [50, 60], [70, 80]]), 1000)
    old = wrappers.AutoResetWrapper(wrappers.EpisodeWrapper(wrappers.VmapWrapper(CountingEnv(2, 0, 1000, [[5, 6]])), 1000, 1))
    so = old.reset(None)
    for t in range(1, 9):
        s, so = w.step(s, None), old.step(so, None)
        assert _row(s) == ([5 + t, 6 + t], [0, 0], [0, 0], [0, 0], [t, t])
        assert torch.equal(s.info["cur_frame"], so.info["cur_frame"]) and torch.equal(s.obs, so.obs) and torch.equal(s.info["steps"], so.info["steps"])


# ---------------------------------------------------------------------------------------------- argument check
def _chk(K=0, rng=None, end=False, have_pose=True, T=250):
    return rodent._check_clip_restarts(K, rng, end, have_pose, T)


def test_what_the_argument_check_returns():
    assert _chk() == (0, (0, 100), False) and _chk(have_pose=False) == (0, (0, 100), False)
    assert _chk(3, (5, 40), True) == (3, (5, 40), True) and _chk(64) == (64, (0, 100), False) and _chk(np.int64(2), (np.int32(1), 2)) == (2, (1, 2), False)
    assert _chk(1, None, True, T=101) == (1, (0, 100), True)                 # entry 0 draws at most 99 = T - 2
    assert _chk(1, (0, 500), True, T=101) == (1, (0, 500), True)             # K = 1: no entry draws from the range
    assert _chk(2, (0, 150), True, T=151) == (2, (0, 150), True)


def test_every_refusal_of_the_argument_check():
    for bad in (-1, 65, 1000, 1.0, "2", None, True):
        with pytest.raises(ValueError, match="clip_restarts must be an int in 0 .. 64"):
            _chk(bad)
    for kw in (dict(K=1), dict(rng=(0, 10)), dict(K=2, rng=(0, 10), end=True)):
        with pytest.raises(ValueError, match="need the reference pose"):
            _chk(have_pose=False, **kw)
    with pytest.raises(ValueError, match="needs clip_restarts >= 1"):
        _chk(0, None, True)
    for bad in ((-1, 5), (5, 5), (7, 3), (0, 0)):
        with pytest.raises(ValueError, match="needs 0 <= lo < hi"):
            _chk(2, bad)
    for bad in ((0.0, 5), (0, "5"), (True, 5)):
        with pytest.raises(ValueError, match="must be two ints"):
            _chk(2, bad)
    for K, rng, T in ((1, None, 100), (1, None, 50), (3, None, 100), (2, (0, 150), 150), (2, (0, 10), 100), (2, (140, 150), 150)):
        with pytest.raises(ValueError, match="would truncate on every step"):
            _chk(K, rng, True, T=T)
    assert _chk(2, (0, 150), False, T=20) == (2, (0, 150), False)            # without the flag a short clip clamps, as today


# ---------------------------------------------------------------------------------------------- ABI
def test_the_ctypes_mirror_matches_the_header():
    header = open(os.path.join(ROOT, "include", "rodent_rr.h")).read()
    m = re.search(r"typedef struct rr_clip_restart_io \{(.*?)\} rr_clip_restart_io;", header, re.S)
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
    want = [("frames", "ptr"), ("slot_in", "ptr"), ("slot_out", "ptr"), ("num_slots", "int32_t"), ("end_at_clip_end", "int32_t")]
    assert members == want, members
    kinds = {"ptr": ctypes.c_void_p, "int32_t": ctypes.c_int32}
    assert [(n, t) for n, t in hip.RRClipRestartIO._fields_] == [(n, kinds[k]) for n, k in members]
    offsets = {n: getattr(hip.RRClipRestartIO, n).offset for n, _ in members}
    assert offsets == dict(frames=0, slot_in=8, slot_out=16, num_slots=24, end_at_clip_end=28) and ctypes.sizeof(hip.RRClipRestartIO) == 32
    for decl in ("int rr_batch_set_clip_restarts(rr_batch* b, const rr_clip_restart_io* restart);",
                 "int rr_batch_clip_restarts_supported(const rr_batch* b, int32_t with_actor);", "int rr_wrap_clip_restart(int32_t num_envs,"):
        assert decl in header


def test_the_three_exports_and_their_signatures():
    for name in ("rr_batch_set_clip_restarts", "rr_batch_clip_restarts_supported", "rr_wrap_clip_restart"):
        assert name in hip.EXPORTS
    lib = hip.lib()
    assert lib.rr_batch_set_clip_restarts.argtypes == [ctypes.c_void_p, ctypes.POINTER(hip.RRClipRestartIO)]
    assert lib.rr_batch_clip_restarts_supported.argtypes == [ctypes.c_void_p, ctypes.c_int32]
    assert len(lib.rr_wrap_clip_restart.argtypes) == 20
    assert lib.rr_batch_set_clip_restarts(None, None) == -1 and b"null batch" in lib.rr_last_error()          # RR_EINVAL, no device needed
    assert lib.rr_batch_clip_restarts_supported(None, 0) == -1 and b"null batch" in lib.rr_last_error()
    args = [1, 0, None, None, None] + [None] * 5 + [5.0, 1.0] + [None] * 4 + [1, 10, 0, None]
    assert lib.rr_wrap_clip_restart(*args) == -1 and b"bad argument" in lib.rr_last_error()


def test_the_closed_structs_stay_closed():
    """rr_env_io, rr_pose_io, rr_pose_term_io, rr_body_io and rr_unroll_io keep their members and sizes: the clip-restart block is a struct
    of its own."""
    assert [n for n, _ in hip.RREnvIOClips._fields_][-2:] == ["clip", "num_clips"]
    assert ctypes.sizeof(hip.RRPoseIO) == 32 and ctypes.sizeof(hip.RRPoseTermIO) == 24 and ctypes.sizeof(hip.RRBodyIO) == 40
    assert [n for n, _ in hip.RRUnrollIO._fields_] == ["first", "first_obs", "prev_done", "steps_in", "steps_out", "truncation_out", "episode_length"]
    assert ctypes.sizeof(hip.RRUnrollIO) == 80
    header = open(os.path.join(ROOT, "include", "rodent_rr.h")).read()
    for name in ("rr_env_io", "rr_pose_io", "rr_pose_term_io", "rr_body_io", "rr_unroll_io"):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S)
        assert m and "slot" not in m.group(1) and "restart" not in m.group(1), name
