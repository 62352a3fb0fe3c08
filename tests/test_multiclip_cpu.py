"""Multi-clip tracking without a GPU: the host draws of `Rodent.reset` (`rodent.reset_draws`), the validation of `track_pos` and of the
explicit clip ids, and the ctypes mirror of `rr_env_io`.  The GPU half is tests/test_gpu_multiclip.py."""
import ctypes
import os

import numpy as np
import pytest

from rodent_amd import hip, jax_random
from rodent_amd.envs import rodent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = jax_random.split(jax_random.PRNGKey(21), 64)
NQ, NV, SCALE = 74, 73, 1e-2


def test_the_clip_draw_moves_no_other_draw():
    """Same keys: start_frame, qpos noise and qvel are identical with num_clips None, 1 and 5 -- and equal the reference's chain
    `rng, rng1, rng2, rng_pos = split(rng, 4)` written out here."""
    ks = jax_random.split(KEYS, 4)
    want = (jax_random.randint(ks[:, 0], 0, 100), jax_random.uniform(ks[:, 1], NQ, -SCALE, SCALE), jax_random.uniform(ks[:, 2], NV, -SCALE, SCALE))
    for c in (None, 1, 5):
        got = rodent.reset_draws(KEYS, NQ, NV, SCALE, c)
        for g, w in zip(got[:3], want):
            assert g.dtype == w.dtype and np.array_equal(g, w), c
        assert (got[3] is None) == (c is None)
    assert want[1].shape == (64, NQ) and want[2].shape == (64, NV) and want[0].min() >= 0 and want[0].max() < 100


@pytest.mark.parametrize("C", [1, 2, 5, 8])
def test_clip_ids_come_from_the_fourth_key(C):
    clip = rodent.reset_draws(KEYS, NQ, NV, SCALE, C)[3]
    assert clip.dtype == np.int32 and clip.shape == (64,)
    for e in range(64):                        # key by key, as `jax.vmap(env.reset)` would draw them
        assert clip[e] == jax_random.randint(jax_random.split(KEYS[e], 4)[3], 0, C)
    assert clip.min() >= 0 and clip.max() < C
    if C > 1:
        assert len(np.unique(clip)) == C         # 64 draws over at most 8 clips: every clip appears


def test_track_rank_is_checked_before_any_device_work():
    """[T, 3] and [C, T, 3] pass; anything else raises ValueError from the constructor's first lines (no model is loaded, no GPU is
    touched: this test runs without one)."""
    from rodent_amd import envs
    for shape in ((3,), (2, 2, 5, 3), (5, 2), (2, 5, 4), (0, 5, 3), (2, 0, 3)):
        with pytest.raises(ValueError, match="track_pos must be"):
            envs.Rodent(track_pos=np.zeros(shape), num_envs=2, xml_path="rodent_optimized.xml", device="cuda:0")
    assert rodent._check_track(np.zeros((5, 3))).shape == (5, 3) and rodent._check_track(np.zeros((1, 5, 3), np.float64)).dtype == np.float32


def _skeleton(num_clips, n=4):
    """A Rodent without a batch: `reset` validates `clip` before it touches anything else."""
    env = object.__new__(rodent.Rodent)
    env.num_envs, env.device, env.sys, env._num_clips = n, "cpu", None, num_clips
    return env


def test_explicit_clip_ids_are_validated_first():
    keys = KEYS[:4]
    for bad in (3, -1, [0, 1, 2, 3], np.array([0, 0, -1, 0])):
        with pytest.raises(ValueError, match=r"clip ids must lie in \[0, 3\)"):
            _skeleton(3).reset(keys, clip=bad)
    with pytest.raises(ValueError, match="shape"):
        _skeleton(3).reset(keys, clip=[0, 1])
    with pytest.raises(ValueError, match="integers"):
        _skeleton(3).reset(keys, clip=[0.0, 1.0, 2.0, 0.0])
    for c in (0, [0, 0, 0, 0]):
        with pytest.raises(ValueError, match="single"):
            _skeleton(None).reset(keys, clip=c)
    assert _skeleton(3).num_clips == 3 and _skeleton(1).num_clips == 1 and _skeleton(None).num_clips == 1
    ids = rodent._check_clip(2, 3, 4)
    assert ids.dtype == np.int32 and ids.tolist() == [2, 2, 2, 2]
    assert rodent._check_clip(np.array([2, 0, 1, 1], np.int64), 3, 4).tolist() == [2, 0, 1, 1]


def test_env_io_mirror_ends_with_the_clip_fields():
    """The two new members close `rr_env_io` in the header and in the ctypes mirror the env calls pass (`RREnvIOClips`: the single-clip
    `RREnvIO`, unchanged, then the two), so a zero-initialised struct is the single-clip path."""
    names = [n for n, _ in hip.RREnvIOClips._fields_]
    assert names[:-2] == [n for n, _ in hip.RREnvIO._fields_] and names[-2:] == ["clip", "num_clips"]
    e = hip.RREnvIOClips()
    assert e.clip is None and e.num_clips == 0
    assert hip.RREnvIOClips.clip.offset == ctypes.sizeof(hip.RREnvIO) and hip.RREnvIOClips.num_clips.offset == hip.RREnvIOClips.clip.offset + 8
    assert ctypes.sizeof(hip.RREnvIOClips) == ctypes.sizeof(hip.RREnvIO) + 16
    header = open(os.path.join(ROOT, "include", "rodent_rr.h")).read()
    body = header[header.index("typedef struct rr_env_io {"):header.index("} rr_env_io;")]
    assert 0 < body.index("float bad_state_max;") < body.index("const int32_t* clip;") < body.index("int32_t num_clips;")
    assert body.rstrip().endswith("/* C */")                  # nothing after the two
    lib = hip.lib()                                           # every entry point that takes the env io takes the whole struct
    for fn in ("rr_env_step", "rr_env_step_to", "rr_env_unroll", "rr_env_unroll_policy", "rr_env_unroll_eval", "rr_env_reset"):
        assert ctypes.POINTER(hip.RREnvIOClips) in getattr(lib, fn).argtypes, fn


def test_eval_rollout_refuses_a_clip_on_a_single_clip_env():
    from rodent_amd import rollout

    class Env:
        num_envs, num_clips = 1, 1
    with pytest.raises(ValueError, match="single clip"):
        rollout.eval_rollout(Env(), None, None, clip=1)
