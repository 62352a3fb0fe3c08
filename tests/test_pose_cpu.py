"""Pose tracking (`Rodent(track_quat=..., track_joints=...)`; rr_batch_set_pose / rr_pose_io) as far as it can be held without a GPU: known answers
of the float64 restatement `pose_rewards`, the constructor's validation through the helper it calls, the ctypes mirror of `rr_pose_io`
against the header, and `reset_to_reference` on the host draws.  The GPU half is tests/test_gpu_pose.py."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from rodent_amd import hip, jax_random
from rodent_amd.envs import rodent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NQ = 74
W, K = (1.5, 0.75), (2.0, 0.5)       # (quat, joint) weights and scales


def _pose(seed=0):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    qpos = np.concatenate([rng.normal(size=3), q, rng.uniform(-1, 1, NQ - 7)])
    return qpos, q.copy(), qpos[7:].copy()


def _qmul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def test_equal_pose_gives_the_weights():
    qpos, rq, rj = _pose()
    qr, jr = rodent.pose_rewards(qpos, rq, rj, W, K)
    assert qr == pytest.approx(W[0], rel=1e-14) and jr == W[1]


def test_sign_and_scale_of_the_quaternion_do_not_matter():
    qpos, _, rj = _pose(1)
    _, rq, _ = _pose(2)                     # another orientation: a large angle
    want = rodent.pose_rewards(qpos, rq, rj, W, K)
    assert 0.0 < want[0] < W[0]
    for f in (-1.0, 3.0):
        other = qpos.copy()
        other[3:7] *= f
        got = rodent.pose_rewards(other, rq, rj, W, K)
        assert got[0] == pytest.approx(want[0], rel=1e-13) and got[1] == want[1]
        got = rodent.pose_rewards(qpos, f * rq, rj, W, K)
        assert got[0] == pytest.approx(want[0], rel=1e-13)


def test_half_turn_about_z():
    qpos, rq, rj = _pose(3)
    qpos[3:7] = _qmul(rq, np.array([0.0, 0.0, 0.0, 1.0]))       # the reference turned by pi about its z axis
    qr, jr = rodent.pose_rewards(qpos, rq, rj, W, K)
    assert qr == pytest.approx(W[0] * math.exp(-K[0] * math.pi ** 2), rel=1e-12) and jr == W[1]


def test_small_angles_are_resolved():
    """theta comes from |d.xyz|, so an angle of 1e-9 rad is seen (acos of d.w would return 0 below 1.5e-8)."""
    qpos, rq, rj = _pose(4)
    a = 1e-6
    qpos[3:7] = _qmul(rq, np.array([math.cos(a / 2), math.sin(a / 2), 0.0, 0.0]))
    qr, _ = rodent.pose_rewards(qpos, rq, rj, (1.0, 1.0), (1e10, 0.5))
    assert qr == pytest.approx(math.exp(-1e10 * a * a), rel=1e-6)


def test_one_joint_off_by_a_tenth():
    qpos, rq, rj = _pose(5)
    qpos[7 + 11] += 0.1
    qr, jr = rodent.pose_rewards(qpos, rq, rj, W, K)
    assert jr == pytest.approx(W[1] * math.exp(-K[1] * 0.01), rel=1e-12) and qr == pytest.approx(W[0], rel=1e-14)


def test_batched_shapes():
    qs = np.stack([_pose(s)[0] for s in range(6)]).reshape(2, 3, NQ)
    qr, jr = rodent.pose_rewards(qs, qs[..., 3:7], qs[..., 7:] + 0.05, W, K)
    assert qr.shape == jr.shape == (2, 3) and qr.dtype == np.float64
    np.testing.assert_allclose(jr, W[1] * math.exp(-K[1] * (NQ - 7) * 0.0025), rtol=1e-12)


# ---------------------------------------------------------------------------------------------- validation
def _clip(lead):
    rng = np.random.default_rng(7)
    return (rng.normal(size=lead + (3,)).astype(np.float32), rng.normal(size=lead + (4,)), rng.uniform(-1, 1, lead + (NQ - 7,)))


def test_check_pose_returns_unit_quaternions_then_joints():
    for lead in ((5,), (2, 5)):
        track, quat, joints = _clip(lead)
        rows = rodent._check_pose(track, 3.0 * quat, joints, NQ)
        assert rows.dtype == np.float32 and rows.shape == lead + (NQ - 3,) and rows.flags["C_CONTIGUOUS"]
        np.testing.assert_allclose(np.linalg.norm(rows[..., :4].astype(np.float64), axis=-1), 1.0, atol=2e-7)
        np.testing.assert_array_equal(rows[..., :4], (quat / np.linalg.norm(quat, axis=-1, keepdims=True)).astype(np.float32))
        np.testing.assert_array_equal(rows[..., 4:], joints.astype(np.float32))
    assert rodent._check_pose(track, None, None, NQ) is None


def test_check_pose_refuses():
    track, quat, joints = _clip((5,))
    with pytest.raises(ValueError, match="go together"):
        rodent._check_pose(track, quat, None, NQ)
    with pytest.raises(ValueError, match="go together"):
        rodent._check_pose(track, None, joints, NQ)
    with pytest.raises(ValueError, match="shapes"):
        rodent._check_pose(track, quat[:, :3], joints, NQ)                # not a quaternion
    with pytest.raises(ValueError, match="shapes"):
        rodent._check_pose(track, quat, joints[:, :-1], NQ)               # not nq - 7 joints
    with pytest.raises(ValueError, match="shapes"):
        rodent._check_pose(track, quat[:4], joints[:4], NQ)               # another T
    with pytest.raises(ValueError, match="shapes"):
        rodent._check_pose(track, quat[None], joints[None], NQ)           # a clip axis the track lacks
    t3, q3, j3 = _clip((2, 5))
    with pytest.raises(ValueError, match="shapes"):
        rodent._check_pose(t3, q3[0], j3[0], NQ)                          # the track's clip axis missing
    with pytest.raises(ValueError, match="shapes"):
        rodent._check_pose(t3, q3[:1], j3[:1], NQ)                        # another C
    for bad in (0.0, np.nan, np.inf):
        q = quat.copy()
        q[2] = bad if bad == 0.0 else [1.0, bad, 0.0, 0.0]
        with pytest.raises(ValueError, match="zero or non-finite quaternion"):
            rodent._check_pose(track, q, joints, NQ)
    j = joints.copy()
    j[1, 3] = np.nan
    with pytest.raises(ValueError, match="non-finite joint"):
        rodent._check_pose(track, quat, j, NQ)
    for bad in (-1.0, np.nan, np.inf, 1e39):
        for at in range(4):
            ws = [1.0, 2.0, 1.0, 0.5]
            ws[at] = bad
            with pytest.raises(ValueError, match="weights and scales"):
                rodent._check_pose(track, quat, joints, NQ, ws)
    assert rodent._check_pose(track, quat, joints, NQ, (0.0, 0.0, 0.0, 0.0)) is not None       # zero is a value: the term is off


# ---------------------------------------------------------------------------------------------- ABI
def _header_members(struct):
    header = open(os.path.join(ROOT, "include", "rodent_rr.h")).read()
    body = header[header.index("typedef struct %s {" % struct) + len("typedef struct %s {" % struct):header.index("} %s;" % struct)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.search(r"(\w+)\s*$", piece).group(1) for piece in decl.split(",")]
    return names


def test_ctypes_mirrors_follow_the_header():
    """`rr_pose_io` and its mirror member by member; `rr_env_io` is closed (its mirror is what it was: the pose block rides on the batch)."""
    P = hip.RRPoseIO
    names = [n for n, _ in P._fields_]
    assert names == _header_members("rr_pose_io")
    assert names == ["track_pose", "pose_metrics", "quat_reward_weight", "quat_reward_scale", "joint_reward_weight", "joint_reward_scale"]
    assert [getattr(P, n).offset for n in names] == [0, 8, 16, 20, 24, 28] and ctypes.sizeof(P) == 32
    e = P()
    assert e.track_pose is None and e.pose_metrics is None and e.quat_reward_weight == 0.0 and e.joint_reward_scale == 0.0
    assert [n for n, _ in hip.RREnvIOClips._fields_] == _header_members("rr_env_io") and ctypes.sizeof(hip.RREnvIOClips) == 96
    assert "rr_batch_pose_supported" in hip.EXPORTS and "rr_batch_set_pose" in hip.EXPORTS
    lib = hip.lib()
    assert lib.rr_batch_set_pose.argtypes == [ctypes.c_void_p, ctypes.POINTER(P)]
    assert lib.rr_batch_set_pose(None, None) == -1 and b"null batch" in lib.rr_last_error()        # RR_EINVAL, no device needed


# ---------------------------------------------------------------------------------------------- reset_to_reference
def test_reset_to_reference_moves_no_draw():
    N, C, T = 16, 3, 40
    rng = np.random.default_rng(11)
    track = rng.normal(size=(C, T, 3)).astype(np.float32)
    pose = rodent._check_pose(track, rng.normal(size=(C, T, 4)), rng.uniform(-1, 1, (C, T, NQ - 7)), NQ)
    qpos0 = rng.uniform(-1, 1, NQ).astype(np.float32)
    keys = jax_random.split(jax_random.PRNGKey(5), N)
    start, noise, qvel, clip = rodent.reset_draws(keys, NQ, NQ - 1, 1e-2, C)
    assert (start > T - 1).any() and (start <= T - 1).any()        # both the in-clip and the clamped frame
    plain = rodent.reset_qpos(qpos0, track, start, noise, clip)
    ref = rodent.reset_qpos(qpos0, track, start, noise, clip, pose)
    fi = np.minimum(start, T - 1)
    np.testing.assert_array_equal(ref[:, :3], plain[:, :3])
    np.testing.assert_array_equal(plain[:, 3:], qpos0[None, 3:] + noise[:, 3:])
    np.testing.assert_array_equal(ref[:, 3:], pose[clip, fi] + noise[:, 3:])
    assert ref.dtype == np.float32 and not np.array_equal(ref[:, 3:], plain[:, 3:])
    again = rodent.reset_draws(keys, NQ, NQ - 1, 1e-2, C)            # the draws are a function of the keys alone
    for a, b in zip(again, (start, noise, qvel, clip)):
        np.testing.assert_array_equal(a, b)
    one = rodent.reset_qpos(qpos0, track[1], start, noise, None, pose[1])      # a single clip: no ids
    np.testing.assert_array_equal(one[:, 3:], pose[1][fi] + noise[:, 3:])
