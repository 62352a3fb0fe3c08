"""Reference restarts without a GPU (`Rodent(restart_from_reference=True)`): the host restatements of the draw
(`rodent.reference_restart_hash`, `reference_restart_draws`, `reference_restart_noise`, `reference_restart_state`), the argument checks
and refusal texts, and the resources of the step-kernel instances that carry the restore (the six of rr_restart_kernel)."""
import os
import sys

import numpy as np
import pytest

from rodent_amd import hip
from rodent_amd.envs import rodent
from tests import clip_library_fixture as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, T, LENGTHS, NQ, NV, NOISE = X.C, X.T, X.LENGTHS, X.NQ, X.NV, X.NOISE
SEED, N, RESTORES, RANGE = 11, 8, 6, (0, 100)
ENV, CNT = (a.reshape(-1) for a in np.meshgrid(np.arange(N), np.arange(RESTORES), indexing="ij"))          # every (env, restore count) pair


def _rows(rng, width, pad=np.nan):
    """Clip rows [C, T, width], the rows at and behind each clip's length set to `pad`."""
    a = rng.standard_normal((C, T, width)).astype(np.float32)
    for c, n in enumerate(LENGTHS.tolist()):
        a[c, n:] = pad
    return a


def test_the_hash_is_fmix32_of_the_weighted_draws_hash_and_a_tag():
    def fmix(h):
        h ^= h >> 16; h = (h * 0x85EBCA6B) & 0xFFFFFFFF; h ^= h >> 13; h = (h * 0xC2B2AE35) & 0xFFFFFFFF
        return h ^ (h >> 16)
    for seed, env, n, p, i in ((0, 0, 0, 1, 0), (11, 5, 3, 3, 73), (2 ** 32 - 1, 2047, 2 ** 31, 4, 72)):
        base = int(rodent.restart_hash(seed, env, n))
        assert int(rodent.reference_restart_hash(seed, env, n, p, i)) == fmix(base ^ ((((p << 16) | i) * 0x9E3779B1) & 0xFFFFFFFF))


def test_frames_lie_in_the_range_before_folding_and_within_the_clip_after():
    for lo, hi in ((0, 100), (90, 102), (3, 4)):
        clip, draw, frame = rodent.reference_restart_draws(SEED, ENV, CNT, (lo, hi), num_clips=C, across_clips=True, lengths=LENGTHS)
        assert draw.dtype == np.int32 and ((draw >= lo) & (draw < hi)).all()
        assert (frame >= 0).all() and (frame <= LENGTHS[clip] - 2).all()
        assert np.array_equal(frame, draw % (LENGTHS[clip] - 1))
        _, draw2, frame2 = rodent.reference_restart_draws(SEED, ENV, CNT, (lo, hi), num_clips=C, across_clips=True)
        assert np.array_equal(draw2, draw) and np.array_equal(frame2, draw)          # without lengths the draw itself (the rows clamp)
    wide = rodent.reference_restart_draws(SEED, np.arange(4096), 0, (0, 100))[1]
    assert wide.min() == 0 and wide.max() == 99


def test_the_env_stays_on_its_clip_without_restart_across_clips():
    ids = (ENV % C).astype(np.int32)
    clip, _, frame = rodent.reference_restart_draws(SEED, ENV, CNT, RANGE, clip=ids, num_clips=C, across_clips=False, lengths=LENGTHS)
    assert np.array_equal(clip, ids) and (frame <= LENGTHS[ids] - 2).all()
    assert rodent.reference_restart_draws(SEED, ENV, CNT, RANGE)[0] is None          # no clip axis


def test_the_noise_is_bounded_exact_and_reproducible():
    a = rodent.reference_restart_noise(SEED, ENV, CNT, 3, NQ, NOISE)
    assert a.dtype == np.float32 and a.shape == (N * RESTORES, NQ)
    assert (np.abs(a) <= np.float32(NOISE)).all() and np.abs(a).max() > 0.9 * NOISE
    assert np.array_equal(a, rodent.reference_restart_noise(SEED, ENV, CNT, 3, NQ, NOISE))
    # s = (h >> 8) * 2**-23 - 1 is exact in float32: the float64 value rounds to itself
    h = rodent.reference_restart_hash(SEED, ENV[:, None], CNT[:, None], 3, np.arange(NQ)[None])
    s64 = (h >> np.uint64(8)).astype(np.float64) * 2.0 ** -23 - 1.0
    assert np.array_equal(s64.astype(np.float32).astype(np.float64), s64) and (s64 >= -1).all() and (s64 < 1).all()
    assert np.array_equal(a, np.float32(NOISE) * s64.astype(np.float32))
    # qpos and qvel elements are kept apart, and so are seeds
    assert not np.array_equal(a[:, :NV], rodent.reference_restart_noise(SEED, ENV, CNT, 4, NV, NOISE))
    assert not np.array_equal(a, rodent.reference_restart_noise(SEED + 1, ENV, CNT, 3, NQ, NOISE))
    assert abs(float(a.mean())) < 0.05 * NOISE


def test_different_envs_and_restore_counts_draw_differently():
    _, draw, _ = rodent.reference_restart_draws(SEED, ENV, CNT, (0, 10 ** 6))
    assert len(set(draw.tolist())) == N * RESTORES
    noise = rodent.reference_restart_noise(SEED, ENV, CNT, 3, NQ, NOISE)
    assert len({row.tobytes() for row in noise}) == N * RESTORES


def test_a_clip_of_weight_zero_is_never_drawn_and_every_other_clip_is():
    """Coverage as a condition on the inputs: with this seed, N = 8 envs and 6 restores each, the restatement alone lands on every clip
    of positive weight, for the weighted and for the uniform draw."""
    for w in ([1, 0, 1], [0, 3, 1], [5, 1, 0], [0, 0, 7]):
        q = rodent.quantise_clip_weights(w)
        clip = rodent.reference_restart_draws(SEED, ENV, CNT, RANGE, num_clips=C, across_clips=True, weights=q)[0]
        assert set(clip.tolist()) == {c for c in range(C) if w[c] > 0}, w
    uniform = rodent.reference_restart_draws(SEED, ENV, CNT, RANGE, num_clips=C, across_clips=True)[0]
    assert set(uniform.tolist()) == set(range(C))
    zero = rodent.reference_restart_draws(SEED, ENV, CNT, RANGE, num_clips=C, across_clips=True, weights=[0, 0, 0])[0]
    assert np.array_equal(zero, uniform)                                               # S == 0: the uniform draw
    # the prefix rule of `weighted_slot` on the clip weights
    q = rodent.quantise_clip_weights([1, 2, 5])
    got = rodent.reference_restart_draws(SEED, ENV, CNT, RANGE, num_clips=C, across_clips=True, weights=q)[0]
    want = [rodent.weighted_slot(int(rodent.reference_restart_hash(SEED, e, n, 1)), q) for e, n in zip(ENV, CNT)]
    assert got.tolist() == want
    # more clips than one chunk of the wave scan
    many = np.zeros(200, dtype=np.int32)
    many[[3, 64, 130, 199]] = 65535
    far = rodent.reference_restart_draws(SEED, np.arange(256), 0, RANGE, num_clips=200, across_clips=True, weights=many)[0]
    assert set(far.tolist()) == {3, 64, 130, 199}


def test_no_drawn_state_reads_a_padding_row():
    """The three unequal clips with NaN behind their lengths: every drawn state is finite, with and without the velocity rows."""
    rng = np.random.default_rng(0)
    track, pose, vel = _rows(rng, 3), _rows(rng, NQ - 3), _rows(rng, NV)
    clip, _, frame = rodent.reference_restart_draws(SEED, ENV, CNT, RANGE, num_clips=C, across_clips=True, lengths=LENGTHS)
    assert set(clip.tolist()) == set(range(C))
    for v in (vel, NV):
        qpos, qvel = rodent.reference_restart_state(SEED, ENV, CNT, clip, frame, track, pose, v, NOISE, LENGTHS)
        assert qpos.dtype == np.float32 and qvel.dtype == np.float32 and qpos.shape == (N * RESTORES, NQ) and qvel.shape == (N * RESTORES, NV)
        assert np.isfinite(qpos).all() and np.isfinite(qvel).all()
    assert np.array_equal(qpos[:, :3], track[clip, frame] + rodent.reference_restart_noise(SEED, ENV, CNT, 3, NQ, NOISE)[:, :3])
    assert np.array_equal(qpos[:, 3:], pose[clip, frame] + rodent.reference_restart_noise(SEED, ENV, CNT, 3, NQ, NOISE)[:, 3:])
    assert np.array_equal(qvel, rodent.reference_restart_noise(SEED, ENV, CNT, 4, NV, NOISE))          # no velocity block: the bare noise
    # the unfolded draw would have read padding: the fold is what keeps the rows inside
    unfolded = rodent.reference_restart_draws(SEED, ENV, CNT, RANGE, num_clips=C, across_clips=True)[2]
    assert (unfolded >= LENGTHS[clip]).any()


def _args(**kw):
    from tests import pose_fixture as F
    quat, joints = F.reference("rodent_optimized", T)
    base = dict(track_pos=F.tracks(T), track_quat=quat, track_joints=joints, xml_path="rodent_optimized.xml", num_envs=4, device="cpu",
                reset_to_reference=True, clip_restarts=1, restart_from_reference=True)
    base.update(kw)
    return base


@pytest.mark.parametrize("kw,text", [
    (dict(track_quat=None, track_joints=None, reset_to_reference=False, clip_restarts=0), "position-only env"),
    (dict(reset_to_reference=False), "needs reset_to_reference=True"),
    (dict(clip_restarts=0), "needs clip_restarts >= 1"),
    (dict(restart_noise_seed=-1), "restart_noise_seed must be an int"),
    (dict(restart_noise_seed=2 ** 32), "restart_noise_seed must be an int"),
    (dict(restart_noise_seed=True), "restart_noise_seed must be an int"),
    (dict(restart_from_reference=False, restart_noise_seed=1.5), "restart_noise_seed must be an int"),
])
def test_argument_validation(kw, text):
    with pytest.raises(ValueError, match=text):
        rodent.Rodent(**_args(**kw))


def test_the_check_itself_and_its_clip_limit():
    assert rodent._check_reference_restart(True, 7, True, 1, True, 3) == (True, 7)
    assert rodent._check_reference_restart(False, 0, False, 0, False, None) == (False, 0)
    with pytest.raises(ValueError, match="at most 32768 clips"):
        rodent._check_reference_restart(True, 0, True, 1, True, rodent.MAX_REFERENCE_CLIPS + 1)
    assert "restart_from_reference" in rodent._CTOR_PARAMS and "restart_noise_seed" in rodent._CTOR_PARAMS      # siblings keep the option


def test_the_library_exports_the_block_and_refuses_a_null_batch():
    L = hip.lib()
    assert L.rr_batch_set_reference_restart(None, None) != 0 and b"null batch" in L.rr_last_error()
    assert L.rr_batch_reference_restart_supported(None, 0) < 0 and b"rr_batch_reference_restart_supported: null batch" in L.rr_last_error()
    import ctypes
    assert ctypes.sizeof(hip.RRReferenceRestartIO) == 48


def test_the_instances_that_carry_the_restore_keep_their_budget():
    """The six rr_restart_kernel instances grew (no further entry): 0 scratch, 0 VGPR spills, <= 256 VGPRs, no static LDS."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = [k for k in kernel_meta.kernels(hip.LIB_PATH) if "rr_restart_kernel" in k["name"]]
    assert len(ks) == 6
    # what only the grown instances have: the I/O block with the seven reference-restart words at its end (888 -> 912 bytes), as the
    # host lays it out and as every instance's code object declares its third argument
    import ctypes
    off, size, total = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    hip.lib().rr_kernarg_layout(ctypes.byref(off), ctypes.byref(size), ctypes.byref(total))
    assert size.value == 912, size.value
    for k in ks:
        assert (off.value, 912) in [tuple(a[:2]) for a in k["args"]], (k["name"], k["args"])
    for k in ks:
        print(k["name"], "vgpr", k["vgpr"], "sgpr_spill", k["sgpr_spill"])
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["vgpr"] <= 256 and k["lds"] == 0, k
