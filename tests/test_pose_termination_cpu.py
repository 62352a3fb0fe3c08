"""Pose termination (`Rodent(max_pos_error=, max_quat_error=, max_joint_error=)`; rr_batch_set_pose_termination) as far as it can be
held without a GPU: known answers of the float64 restatements `pose_errors` and `pose_fail_code`, every refusal of the constructor's
argument check through the helper it calls, and the ctypes mirror of `rr_pose_term_io` against the header.  The GPU half is
tests/test_gpu_pose_termination.py."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from rodent_amd import hip
from rodent_amd.envs import rodent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NQ = 74
INF = math.inf


def _qmul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def _state(seed, N=4):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(N, 4))
    return np.concatenate([rng.normal(size=(N, 3)), q / np.linalg.norm(q, axis=-1, keepdims=True), rng.uniform(-1, 1, (N, NQ - 7))], axis=1)


def _errors(qpos, ref):
    return rodent.pose_errors(qpos, ref[..., :3], ref[..., 3:7], ref[..., 7:])


# ---------------------------------------------------------------------------------------------- pose_errors
def test_equal_pose_has_no_error():
    qpos = _state(0)
    e = _errors(qpos, qpos)
    assert all(x.shape == (4,) and x.dtype == np.float64 for x in e)
    assert np.array_equal(e[0], np.zeros(4)) and np.array_equal(e[2], np.zeros(4))
    np.testing.assert_allclose(e[1], 0.0, atol=1e-7)           # |d.xyz| is a rounding residue of order 1e-16; atan2 keeps it that small


def test_negated_quaternion_is_the_same_orientation():
    qpos = _state(1)
    ref = qpos.copy()
    ref[:, 3:7] *= -1.0
    np.testing.assert_allclose(_errors(qpos, ref)[1], 0.0, atol=1e-7)
    other = _state(2)
    neg = other.copy()
    neg[:, 3:7] *= -1.0
    np.testing.assert_array_equal(_errors(qpos, other)[1], _errors(qpos, neg)[1])


def test_a_half_turn_is_pi():
    qpos = _state(3, N=3)
    for n, axis in enumerate(([0, 1.0, 0, 0], [0, 0, 1.0, 0], [0, 0, 0, 1.0])):       # pi about x, y, z of the reference's own frame
        ref = qpos[n].copy()
        qpos[n, 3:7] = _qmul(ref[3:7], np.array(axis))
        e = _errors(qpos[n], ref)
        assert e[1].shape == () and abs(float(e[1]) - math.pi) < 1e-12
        assert float(e[0]) == 0.0 and float(e[2]) == 0.0


def test_a_quarter_turn_and_a_scaled_quaternion():
    qpos = _state(4, N=1)[0]
    ref = qpos.copy()
    qpos[3:7] = 3.0 * _qmul(ref[3:7], np.array([math.cos(math.pi / 8), 0.0, 0.0, math.sin(math.pi / 8)]))      # pi / 4 about z, not unit length
    assert abs(float(_errors(qpos, ref)[1]) - math.pi / 4) < 1e-12


def test_one_joint_off_by_a_tenth():
    qpos = _state(5)
    for i in (0, 33, NQ - 8):
        ref = qpos.copy()
        ref[:, 7 + i] -= 0.1
        e = _errors(qpos, ref)
        np.testing.assert_allclose(e[2], 0.1, rtol=0, atol=1e-15)
        assert np.array_equal(e[0], np.zeros(4))
        np.testing.assert_allclose(e[1], 0.0, atol=1e-7)
    ref = qpos.copy()
    ref[:, 7:9] += [[0.3, -0.4]]                              # two joints: the 2-norm, not the sum
    np.testing.assert_allclose(_errors(qpos, ref)[2], 0.5, rtol=0, atol=1e-15)


def test_root_off_by_three_and_four_centimetres():
    qpos = _state(6)
    ref = qpos.copy()
    ref[:, :3] += [0.03, 0.04, 0.0]
    e = _errors(qpos, ref)
    np.testing.assert_allclose(e[0], 0.05, rtol=0, atol=1e-15)
    assert np.array_equal(e[2], np.zeros(4))


def test_leading_axes_broadcast():
    qpos, ref = _state(7, N=6).reshape(2, 3, NQ), _state(8, N=6).reshape(2, 3, NQ)
    e = _errors(qpos, ref)
    flat = _errors(qpos.reshape(6, NQ), ref.reshape(6, NQ))
    for a, b in zip(e, flat):
        assert a.shape == (2, 3) and np.array_equal(a.reshape(6), b)


# ---------------------------------------------------------------------------------------------- pose_fail_code
def test_every_single_bit_and_their_or():
    thr = (0.05, 0.5, 1.0)
    over, under = (0.06, 0.6, 1.1), (0.04, 0.4, 0.9)
    for code in range(8):
        errs = tuple(over[i] if code >> i & 1 else under[i] for i in range(3))
        got = rodent.pose_fail_code(errs, thr)
        assert got.dtype == np.int64 and int(got) == code, (code, got)
    errs = tuple(np.array([under[i], over[i]]) for i in range(3))
    assert rodent.pose_fail_code(errs, thr).tolist() == [0, 7]
    assert int(rodent.pose_fail_code(thr, thr)) == 0                      # equal is not above


def test_an_infinite_threshold_never_fires():
    huge = (1e300, 1e300, 1e300)
    assert int(rodent.pose_fail_code(huge, (INF, INF, INF))) == 0
    assert int(rodent.pose_fail_code(huge, (None, None, None))) == 0
    assert int(rodent.pose_fail_code((INF, INF, INF), (INF, INF, INF))) == 0          # inf > inf is false
    assert int(rodent.pose_fail_code(huge, (INF, 1.0, INF))) == 2
    assert int(rodent.pose_fail_code(huge, (1.0, None, 1.0))) == 5


def test_a_nan_error_sets_no_bit():
    nan = float("nan")
    assert int(rodent.pose_fail_code((nan, nan, nan), (0.1, 0.1, 0.1))) == 0
    assert int(rodent.pose_fail_code((nan, 1.0, nan), (0.1, 0.1, 0.1))) == 2
    qpos = _state(9, N=2)
    ref = qpos.copy()
    qpos[0, 0] = qpos[0, 4] = qpos[0, 20] = nan
    e = _errors(qpos, ref)
    assert all(np.isnan(x[0]) for x in e)
    assert rodent.pose_fail_code(e, (1e-3, 1e-3, 1e-3)).tolist() == [0, 0]


# ---------------------------------------------------------------------------------------------- argument check
def test_every_refusal_of_the_argument_check():
    chk = rodent._check_pose_termination
    assert chk(None, None, None, False) is None and chk(None, None, None, True) is None
    assert chk(INF, None, INF, False) is None                 # inf is "off", with or without pose
    assert chk(0.5, None, None, True) == (0.5, INF, INF)
    assert chk(None, 0.25, None, True) == (INF, 0.25, INF)
    assert chk(None, None, 2, True) == (INF, INF, 2.0)
    got = chk(0.1, np.float32(0.2), np.float64(0.3), True)
    assert got == (float(np.float32(0.1)), float(np.float32(0.2)), float(np.float32(0.3))) and all(type(x) is float for x in got)
    for k in range(3):
        for bad in (0, 0.0, -0.0, -1.0, -INF, float("nan"), 1e-50):      # 1e-50 is 0 as a float32
            args = [None, None, None]
            args[k] = bad
            with pytest.raises(ValueError, match="must be > 0 as a float32 and not NaN"):
                chk(*args, True)
            with pytest.raises(ValueError, match="must be > 0 as a float32 and not NaN"):
                chk(*args, False)
        for bad in ("1", True, [1.0], (1.0,)):
            args = [None, None, None]
            args[k] = bad
            with pytest.raises(ValueError, match="must be a number"):
                chk(*args, True)
        args = [None, None, None]
        args[k] = 0.5
        with pytest.raises(ValueError, match="track_quat and track_joints"):
            chk(*args, False)
    for name, k in (("max_pos_error", 0), ("max_quat_error", 1), ("max_joint_error", 2)):       # the message names the argument
        args = [None, None, None]
        args[k] = -1
        with pytest.raises(ValueError, match=name):
            chk(*args, True)


# ---------------------------------------------------------------------------------------------- ABI
def test_the_ctypes_mirror_matches_the_header():
    header = open(os.path.join(ROOT, "include", "rodent_rr.h")).read()
    m = re.search(r"typedef struct rr_pose_term_io \{(.*?)\} rr_pose_term_io;", header, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    members = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)                  # "float* fail" | "float max_pos, max_quat, max_joint" | "int32_t pad"
        for n in names.split(","):
            members.append((n.strip(), "ptr" if ctype.endswith("*") else ctype))
    assert members == [("fail", "ptr"), ("max_pos", "float"), ("max_quat", "float"), ("max_joint", "float"), ("pad", "int32_t")], members
    kinds = {"ptr": ctypes.c_void_p, "float": ctypes.c_float, "int32_t": ctypes.c_int32}
    assert [(n, t) for n, t in hip.RRPoseTermIO._fields_] == [(n, kinds[k]) for n, k in members]
    offsets = {n: getattr(hip.RRPoseTermIO, n).offset for n, _ in members}
    assert offsets == dict(fail=0, max_pos=8, max_quat=12, max_joint=16, pad=20) and ctypes.sizeof(hip.RRPoseTermIO) == 24
    for decl in ("int rr_batch_set_pose_termination(rr_batch* b, const rr_pose_term_io* term);",
                 "int rr_batch_pose_termination_supported(const rr_batch* b, int32_t with_actor);"):
        assert decl in header


def test_the_two_exports_and_their_signatures():
    for name in ("rr_batch_set_pose_termination", "rr_batch_pose_termination_supported"):
        assert name in hip.EXPORTS
    lib = hip.lib()
    assert lib.rr_batch_set_pose_termination.argtypes == [ctypes.c_void_p, ctypes.POINTER(hip.RRPoseTermIO)]
    assert lib.rr_batch_pose_termination_supported.argtypes == [ctypes.c_void_p, ctypes.c_int32]
    assert lib.rr_batch_set_pose_termination(None, None) == -1 and b"null batch" in lib.rr_last_error()          # RR_EINVAL, no device needed
    assert lib.rr_batch_pose_termination_supported(None, 0) == -1 and b"null batch" in lib.rr_last_error()


def test_the_closed_structs_stay_closed():
    """rr_env_io ends with the clip members and rr_pose_io with its four floats: the termination block is a struct of its own."""
    assert [n for n, _ in hip.RREnvIOClips._fields_][-2:] == ["clip", "num_clips"]
    assert [n for n, _ in hip.RRPoseIO._fields_] == ["track_pose", "pose_metrics", "quat_reward_weight", "quat_reward_scale", "joint_reward_weight", "joint_reward_scale"]
