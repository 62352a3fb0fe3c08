"""Clip sampling without a GPU (`Rodent(restart_sampling="weighted", clip_outcomes=True)`): the hash and the draw
against a Python-int restatement written here, the distribution of the draws, the quantiser and `FailureWeights`, every ValueError, what
`Rodent` hands its batch (the recording fake batch of tests/test_env_io_options_cpu.py), the two composed wrappers on a frame-counting
fake env against a loop written here, `ppo.train`'s metrics and `clip_weight_fn` (one rank and two over gloo), the ABI, and the register
budget of the built library.  The GPU half is tests/test_gpu_clip_sampling.py."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from rodent_amd import hip, jax_random
from rodent_amd.envs import base, rodent, wrappers
from rodent_amd.training.agents.ppo import train as ppo
from tests import clip_library_fixture as X
from tests.fake_env import PointEnv
from tests.test_clip_library_cpu import CLIPS, FRAMES, WL, FrameEnv, _clips
from tests.test_env_io_options_cpu import FakeBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------- the rule, in Python ints
def fmix32(h):
    h &= M
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M
    return h ^ (h >> 16)


def the_hash(seed, env, n):
    return fmix32((fmix32((seed ^ ((env * 0x9E3779B1) & M)) & M) + n) & M)


def the_slot(h, q, slot):
    S = sum(q)
    if S == 0:
        return (slot + 1) % len(q)
    r = (h * S) >> 32
    return int(np.searchsorted(np.cumsum(q), r, "right"))


def test_fmix32_and_the_restart_hash_known_answers():
    # written down from the Python-int implementation above
    assert [fmix32(x) for x in (0, 1, 0xFFFFFFFF, 0x12345678)] == [0x0, 0x514E28B7, 0x81F16F39, 0xE37CD1BC]
    known = {(0, 0, 0): 0x0, (0, 1, 0): 0xBB73D643, (94, 31, 7): 0x8E539480, (1, 2047, 3): 0x68F9D41E,
             (0xFFFFFFFF, 5, 0xFFFFFFFF): 0x480DB3BE, (7, 0, 1): 0x9641E981}
    for (seed, env, n), want in known.items():
        assert the_hash(seed, env, n) == want
        assert int(rodent.restart_hash(seed, env, n)) == want, (seed, env, n)
    # broadcast over envs and draws
    got = rodent.restart_hash(94, np.arange(40)[:, None], np.arange(5)[None])
    assert got.shape == (40, 5) and all(int(got[e, n]) == the_hash(94, e, n) for e in range(40) for n in range(5))
    # the torch restatement of the composed wrapper is the same function
    t = wrappers._fmix32(torch.tensor([0, 1, 0xFFFFFFFF, 0x12345678], dtype=torch.int64))
    assert t.tolist() == [0x0, 0x514E28B7, 0x81F16F39, 0xE37CD1BC]


@pytest.mark.parametrize("q", [(7,), (0,), (1, 2, 5, 0), (0, 0, 3), (0, 0, 0, 0), (65535,) * 64, tuple(range(64)), (0,) * 63 + (1,)], ids=str)
def test_weighted_slot_is_searchsorted_of_the_prefix_sums(q):
    rng = np.random.default_rng(len(q))
    hs = [0, 1, M, M - 1, 1 << 31] + [int(x) for x in rng.integers(0, 1 << 32, 200)]
    S, prefix = sum(q), np.cumsum(q)
    for i, h in enumerate(hs):
        got = rodent.weighted_slot(h, q, slot=i % len(q))
        if S == 0:
            assert got == (i % len(q) + 1) % len(q)          # every weight 0: the cyclic rule
            continue
        r = (h * S) >> 32
        assert got == int(np.searchsorted(prefix, r, "right")) and q[got] > 0 and 0 <= got < len(q)
    if S:
        assert rodent.weighted_slot(0, q) == int(np.flatnonzero(np.asarray(q) > 0)[0])
        assert rodent.weighted_slot(M, q) == int(np.flatnonzero(np.asarray(q) > 0)[-1])         # the top of the 32-bit range: r = S - 1
    if q == (65535,) * 64:
        assert (M * S) >> 32 == S - 1 and S == 64 * 65535 < 1 << 32


@pytest.mark.parametrize("seed", [0, 1, 94])
def test_the_draws_follow_the_weights(seed):
    """2048 envs x draws 0 .. 7, q = (1, 2, 5, 0): every cell within 4 binomial standard deviations, the weight-0 cell exactly 0."""
    q = (1, 2, 5, 0)
    h = rodent.restart_hash(seed, np.arange(2048)[:, None], np.arange(8)[None]).reshape(-1)
    cells = np.bincount([rodent.weighted_slot(int(x), q) for x in h], minlength=4)
    n, p = h.size, np.asarray(q) / sum(q)
    z = (cells[:3] - n * p[:3]) / np.sqrt(n * p[:3] * (1 - p[:3]))
    print(f"seed {seed}: cells {cells.tolist()}, z {np.round(z, 2).tolist()}")
    assert cells[3] == 0 and (np.abs(z) <= 4).all()


def test_the_torch_draw_of_the_composed_wrapper_is_the_host_rule():
    rng = np.random.default_rng(3)
    K, N, C = 5, 37, 4
    bank = rng.integers(0, C, (K, N)).astype(np.int32)
    bank[:, 7] = 2                                           # an env whose whole bank is the weight-0 clip
    w = np.array([3, 65535, 0, 9], dtype=np.int32)
    draws = rng.integers(0, 50, N).astype(np.int32)
    got = wrappers.weighted_slots(torch.from_numpy(w), torch.from_numpy(bank), 94, torch.from_numpy(draws)).numpy()
    for e in range(N):
        q = w[bank[:, e]].tolist()
        assert got[e] == (-1 if sum(q) == 0 else the_slot(the_hash(94, e, int(draws[e])), q, 0)), e
    assert got[7] == -1 and (got >= 0).sum() == N - 1


# ---------------------------------------------------------------------------------------------- quantiser, FailureWeights, counters
def test_quantise_clip_weights():
    q = rodent.quantise_clip_weights([0.0, 1.0, 0.5, 1e-9, 0.25])
    assert q.dtype == np.int32 and q.tolist() == [0, 65535, 32768, 1, 16384]          # 0 stays 0, a tiny weight is not lost; 32767.5 -> even
    assert rodent.quantise_clip_weights([3.0, 3.0]).tolist() == [65535, 65535]
    assert rodent.quantise_clip_weights(np.array([2.0, 1.0, 0.0])).tolist() == [65535, 32768, 0]
    for bad in ([0.0, 0.0], [1.0, -0.1], [1.0, np.nan], [np.inf, 1.0], [[1.0, 2.0]], []):
        with pytest.raises(ValueError, match="finite, >= 0 and not all zero"):
            rodent.quantise_clip_weights(bad)


def test_failure_weights_arithmetic():
    fw = rodent.FailureWeights(floor=0.1, decay=0.5)
    assert fw.rates() is None
    t1 = np.array([[4, 1, 1, 2, 40], [2, 0, 0, 2, 20], [0, 0, 0, 0, 5]])
    w = fw(t1)
    np.testing.assert_allclose(w, [0.1 + 0.9 * 0.5, 0.1, 1.0], rtol=1e-15)             # no finished episode yet: weight 1
    t2 = np.array([[2, 0, 0, 2, 10], [0, 0, 0, 0, 10], [1, 1, 0, 0, 10]])
    w = fw(t2)
    fails, eps = 0.5 * np.array([2.0, 0, 0]) + [0, 0, 1], 0.5 * np.array([4.0, 2, 0]) + [2, 0, 1]
    np.testing.assert_allclose(w, 0.1 + 0.9 * fails / eps, rtol=1e-15)
    np.testing.assert_allclose(fw.rates(), fails / eps, rtol=1e-15)
    assert rodent.FailureWeights(floor=0.0)(np.array([[3, 0, 0, 3, 9]])) is None         # every weight 0: keep the table
    d = rodent.FailureWeights()
    assert (d.floor, d.decay) == (0.1, 0.9)
    for kw in (dict(floor=-0.1), dict(floor=1.5), dict(decay=1.0), dict(decay=-0.5)):
        with pytest.raises(ValueError, match="FailureWeights needs"):
            rodent.FailureWeights(**kw)


def test_clip_outcome_update_columns():
    t = np.zeros((3, 5), dtype=np.int64)
    clip = np.array([0, 1, 1, 2, 2, 2])
    code = np.array([0, 3, 0, 0, 4, 0])
    done_env = np.array([0, 1, 1, 0, 1, 0])
    done = np.array([0, 1, 1, 1, 0, 0])                      # (env 4: a code without done does not count as an episode)
    assert rodent.clip_outcome_update(t, clip, code, done_env, done) is t
    assert t.tolist() == [[0, 0, 0, 0, 1], [2, 1, 1, 0, 2], [1, 0, 0, 1, 3]]
    rodent.clip_outcome_update(t, clip, code, done_env, done)
    assert (t[:, 1:4].sum(1) == t[:, 0]).all() and t[:, 4].tolist() == [2, 4, 6]
    tt = torch.zeros(3, 5, dtype=torch.int64)
    for _ in range(2):
        wrappers.count_outcomes(tt, torch.from_numpy(clip), torch.from_numpy(code) != 0, torch.from_numpy(done_env) != 0, torch.from_numpy(done) != 0)
    assert np.array_equal(tt.numpy(), t)
    assert rodent.OUTCOME_COLUMNS == ("episodes", "pose_fail", "env_done", "truncated", "steps")


# ---------------------------------------------------------------------------------------------- env construction on the fake batch
@pytest.fixture
def fake_batch(monkeypatch):
    monkeypatch.setattr(base.hip, "Batch", FakeBatch)


N, K, C = 4, 3, 3


def _env(**kw):
    return rodent.Rodent(num_envs=kw.pop("num_envs", N), xml_path="rodent_optimized.xml", device="cpu", **_clips(), **kw)


def test_constructor_validation_messages(fake_batch):
    with pytest.raises(ValueError, match="restart_sampling='weighted' needs restart_across_clips=True"):
        _env(clip_restarts=K, restart_sampling="weighted")
    with pytest.raises(ValueError, match="restart_sampling='weighted' needs restart_across_clips=True"):
        _env(restart_sampling="weighted")
    with pytest.raises(ValueError, match="clip_outcomes=True needs clip_restarts >= 1"):
        _env(clip_outcomes=True)
    single = {k: v[0] for k, v in _clips().items()}
    with pytest.raises(ValueError, match="clip_outcomes=True needs a \\[C, T, 3\\] track_pos"):
        rodent.Rodent(num_envs=N, xml_path="rodent_optimized.xml", device="cpu", clip_restarts=2, clip_outcomes=True, **single)
    with pytest.raises(ValueError, match="restart_sampling must be None"):
        _env(clip_restarts=K, restart_across_clips=True, restart_sampling="uniform")
    for bad in (-1, 2 ** 32, 1.5, True):
        with pytest.raises(ValueError, match="restart_sampling_seed must be an int in 0"):
            _env(clip_restarts=K, restart_across_clips=True, restart_sampling="weighted", restart_sampling_seed=bad)
    env = _env(clip_restarts=K, restart_across_clips=True, restart_sampling="weighted", clip_outcomes=True, restart_sampling_seed=2 ** 32 - 1)
    assert env.clip_sampling["seed"] == 2 ** 32 - 1
    # the accessors of an env without the options refuse or answer None
    plain = _env(clip_restarts=K, restart_across_clips=True)
    assert plain.clip_sampling is None and plain.clip_weights() is None
    with pytest.raises(ValueError, match="restart_sampling='weighted'"):
        plain.set_clip_weights([1, 1, 1])
    with pytest.raises(ValueError, match="clip_outcomes=True"):
        plain.clip_outcomes()


def test_weights_start_uniform_and_are_written_in_place(fake_batch):
    env = _env(clip_restarts=K, restart_across_clips=True, restart_sampling="weighted", clip_outcomes=True)
    table = env.clip_sampling["weights"]
    assert table.dtype == torch.int32 and env.clip_weights().tolist() == [65535] * C
    ptr = table.data_ptr()
    env.set_clip_weights([1.0, 0.0, 0.5])
    assert env.clip_sampling["weights"] is table and table.data_ptr() == ptr and table.tolist() == [65535, 0, 32768]
    env.set_clip_weights(torch.tensor([0.0, 2.0, 2.0]))
    assert env.clip_weights().tolist() == [0, 65535, 65535]
    for bad, why in (([1.0, 1.0], "shape"), ([0.0, 0.0, 0.0], "not all zero"), ([1.0, -1.0, 1.0], "not all zero"), ([1.0, np.nan, 1.0], "finite")):
        with pytest.raises(ValueError, match=why):
            env.set_clip_weights(bad)
    assert env.clip_weights().tolist() == [0, 65535, 65535]           # a refused table leaves the old one
    out = env.clip_outcomes()
    assert out.dtype == np.int64 and out.shape == (C, 5) and not out.any()
    env.clip_sampling["outcomes"][1, 4] = 7
    optr = env.clip_sampling["outcomes"].data_ptr()
    assert env.clip_outcomes(clear=True)[1, 4] == 7 and not env.clip_outcomes().any() and env.clip_sampling["outcomes"].data_ptr() == optr


def test_with_num_envs_keeps_the_options(fake_batch):
    env = _env(clip_restarts=K, restart_across_clips=True, restart_sampling="weighted", clip_outcomes=True, restart_sampling_seed=11)
    sib = env.with_num_envs(2)
    assert sib.num_envs == 2 and sib.clip_sampling["seed"] == 11
    assert sib.clip_sampling["weights"] is not None and sib.clip_sampling["outcomes"] is not None
    assert sib.clip_sampling["weights"] is not env.clip_sampling["weights"]               # its own tables (the eval env keeps uniform weights)
    only = _env(clip_restarts=K, clip_outcomes=True).with_num_envs(2)
    assert only.clip_sampling["weights"] is None and only.clip_sampling["outcomes"] is not None
    assert _env(clip_restarts=K, restart_across_clips=True).with_num_envs(2).clip_sampling is None


def test_the_constructor_asks_the_probe_only_when_an_option_is_on(fake_batch, monkeypatch):
    asked = lambda env: [n for n, _, _ in env._batch.calls if n == "clip_sampling_supported"]
    assert asked(_env()) == [] and asked(_env(clip_restarts=2, restart_across_clips=True)) == []
    assert len(asked(_env(clip_restarts=2, clip_outcomes=True))) == 1
    assert len(asked(_env(clip_restarts=2, restart_across_clips=True, restart_sampling="weighted"))) == 1

    class Refusing(FakeBatch):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.refuse["clip_sampling_supported"] = "pose tracking: no pose instance here"
    monkeypatch.setattr(base.hip, "Batch", Refusing)
    with pytest.raises(RuntimeError, match=r"restart_sampling=\.\.\. / clip_outcomes=True\): pose tracking: no pose instance here"):
        _env(clip_restarts=2, clip_outcomes=True)
    _env(clip_restarts=2)


def test_the_io_key_and_the_info_key_appear_exactly_when_an_option_is_on(fake_batch):
    keys = jax_random.split(jax_random.PRNGKey(2), N)
    acts = torch.zeros(2, N, 38)
    for weighted, counting in ((False, False), (True, False), (False, True), (True, True)):
        kw = dict(clip_restarts=K, restart_across_clips=True)
        if weighted:
            kw.update(restart_sampling="weighted", restart_sampling_seed=5)
        if counting:
            kw.update(clip_outcomes=True)
        env = _env(**kw)
        s = wrappers.FusedEpisodeAutoResetWrapper(wrappers.VmapWrapper(env), 5).reset(keys)
        base_keys = {"cur_frame", "clip", "restart_bank", "restart_slot", "steps", "truncation"}
        assert set(s.info) == base_keys | ({"restart_draws"} if weighted else set())
        if weighted:
            d = s.info["restart_draws"]
            assert d.dtype == torch.int32 and tuple(d.shape) == (N,) and not d.any()
        assert "clip_sampling" not in env._batch.last_env_io("env_reset")
        env.step(s, acts[0])
        assert "clip_sampling" not in env._batch.last_env_io("env_step_to")        # single steps have no restore in the kernel
        out = env.unroll_wrapped(s, acts, 5)
        uio = env._batch.last_env_io("env_unroll")
        assert ("clip_sampling" in uio) == (weighted or counting)
        assert set(out.info) == set(s.info)
        if weighted or counting:
            blk = uio["clip_sampling"]
            assert blk["weights"] is (env.clip_sampling["weights"] if weighted else None)
            assert blk["outcomes"] is (env.clip_sampling["outcomes"] if counting else None)
            assert blk["seed"] == (5 if weighted else 0)
            if weighted:
                assert blk["draws_in"] is s.info["restart_draws"] and out.info["restart_draws"] is blk["draws_out"]
                assert blk["draws_out"].data_ptr() != blk["draws_in"].data_ptr() and blk["draws_out"].dtype == torch.int32
            else:
                assert "draws_in" not in blk and "draws_out" not in blk


# ---------------------------------------------------------------------------------------------- composed wrappers on a fake env
class SamplingEnv(FrameEnv):
    """`FrameEnv` with the clip-sampling surface: the two tables, the restore count, and a script of the env's own dones and pose
    failures, [steps, N] each."""

    def __init__(self, frames, clips, lengths, weights, seed, own=None, fail=None, counting=True):
        super().__init__(frames, clips, lengths)
        self.num_clips = len(lengths)
        self.clip_sampling = dict(weights=None if weights is None else torch.as_tensor(weights, dtype=torch.int32),
                                  outcomes=torch.zeros(self.num_clips, 5, dtype=torch.int64) if counting else None, seed=seed)
        self.own, self.fail, self.t = own, fail, 0

    def reset(self, rng):
        s = super().reset(rng)
        if self.clip_sampling["weights"] is not None:
            s.info["restart_draws"] = torch.zeros(self.num_envs, dtype=torch.int32)
        self.t = 0
        return s

    def step(self, state, action):
        s = super().step(state, action)
        if self.own is not None:
            fail = torch.as_tensor(self.fail[self.t], dtype=torch.float32)
            s = s.replace(done=torch.maximum(torch.as_tensor(self.own[self.t], dtype=torch.float32), (fail != 0).float()), metrics={"pose_fail": fail})
        self.t += 1
        return s


def _loop(frames, clips, lengths, weights, seed, episode_length, steps, own=None, fail=None):
    """The rule of section 4t, env by env, in Python ints: `clip_library_fixture.schedule`'s loop with the drawn slot, the env's own
    dones and the counters.  -> ([steps, N, 4] = (frame, clip, slot, draws), table [C, 5])."""
    frames, clips = np.asarray(frames), np.asarray(clips)
    Kk, Nn = frames.shape
    out = np.zeros((steps, Nn, 4), dtype=np.int64)
    table = np.zeros((len(lengths), 5), dtype=np.int64)
    for e in range(Nn):
        f, c, slot, n, draws = int(frames[0, e]), int(clips[0, e]), 0, 0, 0
        for t in range(steps):
            n, nf = n + 1, f + 1
            failed = bool(fail[t][e]) if fail is not None else False
            done_env = failed or (bool(own[t][e]) if own is not None else False)
            over = n >= episode_length or nf >= lengths[c] - 1
            table[c, 4] += 1
            if over or done_env:
                table[c, 0] += 1
                table[c, 1 if failed else (2 if done_env else 3)] += 1
                if weights is None:
                    slot = (slot + 1) % Kk
                else:
                    slot = the_slot(the_hash(seed, e, draws), [int(weights[clips[k, e]]) for k in range(Kk)], slot)
                draws += 1
                f, c, n = int(frames[slot, e]), int(clips[slot, e]), 0
            else:
                f = nf
            out[t, e] = (f, c, slot, draws)
    return out, table


def _play(env, episode_length, steps):
    w = wrappers.ClipAutoResetWrapper(wrappers.ClipEpisodeWrapper(wrappers.VmapWrapper(env), episode_length, 1))
    s = w.reset(None)
    rows = []
    for _ in range(steps):
        s = w.step(s, None)
        draws = s.info["restart_draws"] if "restart_draws" in s.info else torch.zeros(env.num_envs, dtype=torch.int32)
        rows.append(torch.stack([s.info["cur_frame"], s.info["clip"], s.info["restart_slot"], draws], dim=-1).numpy().astype(np.int64))
    return np.stack(rows)


@pytest.mark.parametrize("weights", [(1, 2, 5), (65535, 65535, 65535), (1, 0, 1), (0, 0, 0), None], ids=str)
def test_the_composed_wrappers_follow_the_loop(weights):
    steps, ep = 16, 5
    rng = np.random.default_rng(8)
    own = (rng.random((steps, 4)) < 0.12).astype(np.int64)
    fail = (rng.random((steps, 4)) < 0.1).astype(np.int64) * 3
    env = SamplingEnv(FRAMES, CLIPS, WL, weights, 94, own, fail)
    got = _play(env, ep, steps)
    want, table = _loop(FRAMES, CLIPS, WL, weights, 94, ep, steps, own, fail)
    cols = 4 if weights is not None else 3               # (without a weight table the state carries no restore count)
    for t in range(steps):
        assert np.array_equal(got[t][:, :cols], want[t][:, :cols]), (t, got[t].tolist(), want[t].tolist())
    assert np.array_equal(env.clip_sampling["outcomes"].numpy(), table)
    assert (table[:, 1:4].sum(1) == table[:, 0]).all() and table[:, 4].sum() == 4 * steps
    assert table[:, 1].sum() > 0 and table[:, 2].sum() > 0 and table[:, 3].sum() > 0          # each cause occurs in this script
    if weights == (1, 0, 1):          # no env lands on the weight-0 clip at a restore (every bank of CLIPS has another clip)
        assert all(want[t, e, 1] != 1 for e in range(4) for t in range(steps) if want[t, e, 3] > (want[t - 1, e, 3] if t else 0))
    if weights in ((0, 0, 0), None):  # S == 0 and no table: the cyclic rule, and the restore count still grows
        cyc, _ = _loop(FRAMES, CLIPS, WL, None, 94, ep, steps, own, fail)
        assert np.array_equal(want[:, :, :3], cyc[:, :, :3]) and want[-1, :, 3].min() >= 2
    else:
        assert not np.array_equal(want[:, :, 2], _loop(FRAMES, CLIPS, WL, None, 94, ep, steps, own, fail)[0][:, :, 2])     # the draws differ from the walk


def test_counting_alone_leaves_the_schedule_alone():
    env = SamplingEnv(FRAMES, CLIPS, WL, None, 0)
    a = _play(env, 5, 12)
    want, table = _loop(FRAMES, CLIPS, WL, None, 0, 5, 12)
    assert np.array_equal(a[:, :, :3], want[:, :, :3]) and (want[:, :, 3] > 0).any() and not a[:, :, 3].any()
    assert np.array_equal(env.clip_sampling["outcomes"].numpy(), table)
    assert table[:, 1].sum() == 0 and table[:, 2].sum() == 0 and table[:, 3].sum() == table[:, 0].sum() > 0


def test_the_gpu_fixtures_weighted_schedule_holds_its_conditions():
    """The GPU cases compare slots with this host schedule (K = 4, weights (1, 2, 5), seed 94): it must contain restores, clip changes
    and draws that differ from the cyclic walk."""
    frames, clips = X.bank(4)
    q = rodent.quantise_clip_weights([1, 2, 5])
    want, table = _loop(frames, clips, X.LENGTHS, q, X.SEED, X.EPISODE, X.STEPS)
    cyc, _ = _loop(frames, clips, X.LENGTHS, None, X.SEED, X.EPISODE, X.STEPS)
    restores = int(want[-1, :, 3].sum())
    print(f"restores {restores}, slots that differ from the walk {(want[:, :, 2] != cyc[:, :, 2]).sum()}, table {table.tolist()}")
    assert restores >= 60 and (want[:, :, 2] != cyc[:, :, 2]).sum() >= 30 and table[:, 4].sum() == X.N * X.STEPS
    assert np.array_equal(cyc[:, :, 2], X.schedule(4)["slot"]) and np.array_equal(cyc[:, :, 1], X.schedule(4)["clip"])


# ---------------------------------------------------------------------------------------------- ppo.train
class CountingPointEnv(PointEnv):
    """`PointEnv` with an outcome table: every step adds (1, 0, 1, 0, num_envs) to clip 0 and (2, 1, 0, 1, 0) to clip 1."""
    seen = []

    def __init__(self, num_envs=8, device="cpu"):
        super().__init__(num_envs, device)
        self.clip_sampling = dict(weights=torch.full((2,), 65535, dtype=torch.int32), outcomes=torch.zeros(2, 5, dtype=torch.int64), seed=0)
        self.set = []

    def with_num_envs(self, n, device=None):
        return CountingPointEnv(n, device or self.device)

    def step(self, state, action):
        self.clip_sampling["outcomes"] += torch.tensor([[1, 0, 1, 0, self.num_envs], [2, 1, 0, 1, 0]])
        return super().step(state, action)

    def clip_outcomes(self, clear=False):
        out = self.clip_sampling["outcomes"].numpy().copy()
        if clear:
            self.clip_sampling["outcomes"].zero_()
        return out

    def set_clip_weights(self, w):
        self.set.append(np.asarray(w).copy())


def _train(env, fn, **kw):
    args = dict(environment=env, num_timesteps=10 ** 6, episode_length=20, num_envs=16, batch_size=16, num_minibatches=2, unroll_length=5,
                num_updates_per_batch=1, num_evals=2, num_eval_envs=4, seed=1, max_training_steps=3, clip_weight_fn=fn)
    args.update(kw)
    return ppo.train(**args)


def test_train_reports_the_metrics_and_calls_the_weight_fn_once_per_step():
    env = CountingPointEnv(16)
    tables = []

    def fn(table):
        tables.append(table.copy())
        return None if len(tables) == 2 else np.array([1.0, len(tables)])

    _, _, metrics = _train(env, fn)
    steps = 5 * 2                                            # unroll_length x unrolls per training step
    want = np.array([[1, 0, 1, 0, 16], [2, 1, 0, 1, 0]]) * steps
    assert len(tables) == 3 and all(t.dtype == np.int64 and np.array_equal(t, want) for t in tables)       # cleared each time
    assert [w.tolist() for w in env.set] == [[1.0, 1.0], [1.0, 3.0]]                     # None keeps the table
    assert metrics["training/clip_fail_rate"] == pytest.approx(2 / 3) and metrics["training/clip_truncated_share"] == pytest.approx(1 / 3)
    assert metrics["training/clip_fail_rate_clip0"] == 1.0 and metrics["training/clip_fail_rate_clip1"] == 0.5
    # without a function: the metrics alone; a function without the counters is refused
    env2 = CountingPointEnv(16)
    _, _, m2 = _train(env2, None)
    assert "training/clip_fail_rate" in m2 and env2.set == []
    with pytest.raises(ValueError, match="clip_weight_fn needs an environment built with clip_outcomes=True"):
        _train(PointEnv(16), lambda t: None)
    _, _, m3 = _train(PointEnv(16), None)
    assert not [k for k in m3 if "clip_" in k]


def _dp_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    try:
        tables = []
        _train(CountingPointEnv(8), lambda t: tables.append(t.copy()), max_training_steps=2)
        out[rank] = [t.tolist() for t in tables]
    finally:
        torch.distributed.destroy_process_group()


def test_two_ranks_receive_the_same_summed_table():
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    out = mgr.dict()
    port = 31500 + os.getpid() % 2000
    mp.spawn(_dp_worker, args=(2, port, out), nprocs=2, join=True)
    assert out[0] == out[1] and len(out[0]) == 2
    # 8 envs per rank, 10 steps per training step, both ranks added
    assert out[0][0] == (np.array([[1, 0, 1, 0, 8], [2, 1, 0, 1, 0]]) * 10 * 2).tolist()


# ---------------------------------------------------------------------------------------------- ABI
def test_the_ctypes_mirror_matches_the_header():
    header = open(os.path.join(ROOT, "include", "rodent_rr.h")).read()
    m = re.search(r"typedef struct rr_clip_sampling_io \{(.*?)\} rr_clip_sampling_io;", header, re.S)
    assert m
    members = [d.strip().split("*")[-1].split()[-1] for d in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(";") if d.strip()]
    assert members == ["clip_weights", "draws_in", "draws_out", "outcomes", "seed"]
    assert [n for n, _ in hip.RRClipSamplingIO._fields_] == members
    assert [getattr(hip.RRClipSamplingIO, n).offset for n in members] == [0, 8, 16, 24, 32] and ctypes.sizeof(hip.RRClipSamplingIO) == 40
    for decl in ("int rr_batch_set_clip_sampling(rr_batch* b, const rr_clip_sampling_io* sampling);",
                 "int rr_batch_clip_sampling_supported(const rr_batch* b, int32_t with_actor);", "int rr_wrap_clip_sampling(int32_t num_envs,",
                 "const float* pose_fail, const rr_clip_sampling_io* sampling, void* stream);"):
        assert decl in header, decl


def test_the_three_exports_and_their_signatures():
    for name in ("rr_batch_set_clip_sampling", "rr_batch_clip_sampling_supported", "rr_wrap_clip_sampling"):
        assert name in hip.EXPORTS
    lib = hip.lib()
    assert lib.rr_batch_set_clip_sampling.argtypes == [ctypes.c_void_p, ctypes.POINTER(hip.RRClipSamplingIO)]
    assert lib.rr_batch_clip_sampling_supported.argtypes == [ctypes.c_void_p, ctypes.c_int32]
    assert len(lib.rr_wrap_clip_sampling.argtypes) == 26 and len(lib.rr_wrap_clip_library.argtypes) == 23       # the older entry is unchanged
    assert lib.rr_batch_set_clip_sampling(None, None) == -1 and b"null batch" in lib.rr_last_error()
    assert lib.rr_batch_clip_sampling_supported(None, 0) == -1 and b"null batch" in lib.rr_last_error()
    args = [1, 0, None, None, None] + [None] * 5 + [5.0, 1.0] + [None] * 4 + [1, 10, 0] + [None] * 3 + [1, None, None, None]
    assert lib.rr_wrap_clip_sampling(*args) == -1 and b"rr_wrap_clip_sampling: bad argument" in lib.rr_last_error()


# ---------------------------------------------------------------------------------------------- the built library
@pytest.fixture(scope="module")
def all_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    return kernel_meta.kernels(hip.LIB_PATH)


def test_no_new_instance_and_the_restart_kernel_keeps_its_budget(all_kernels):
    names = [k["name"] for k in all_kernels]
    family = ("rr_pose_kernel", "rr_poseterm_kernel", "rr_body_kernel", "rr_restart_kernel")
    assert len([n for n in names if any(e in n for e in family)]) == 33
    restart = [k for k in all_kernels if "rr_restart_kernel" in k["name"]]
    assert len(restart) == 6
    for k in restart:
        print(k["name"], "vgpr", k["vgpr"], "sgpr_spill", k["sgpr_spill"])
        assert k["vgpr"] <= 256 and k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["lds"] == 0, k
    wrap = [k for k in all_kernels if "rr_wrap_kernelILi3EE" in k["name"]]      # the sampling level of the per-step wrapper's template
    assert len(wrap) == 1 and wrap[0]["scratch"] == 0 and wrap[0]["lds"] == 0
