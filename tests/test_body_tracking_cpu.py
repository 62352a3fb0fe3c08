"""Body tracking (`Rodent(track_bodies=, body_ids=, end_effector_ids=)`; rr_batch_set_body_tracking) as far as it can be held without
a GPU: known answers of the float64 restatement `body_rewards`, every refusal of the constructor's argument check through the helper
it calls, and the ctypes mirror of `rr_body_io` against the header.  The GPU half is tests/test_gpu_body_tracking.py."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from rodent_amd import hip
from rodent_amd.envs import rodent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NBODY = 66
ALL = tuple(range(1, NBODY))
EFF = (11, 15, 59, 64, 54)
W, K = (0.7, 1.3), (8.0, 100.0)


def _xpos(seed, N=4):
    return np.random.default_rng(seed).normal(size=(N, NBODY, 3))


# ---------------------------------------------------------------------------------------------- body_rewards
def test_equal_positions_give_the_weights():
    x = _xpos(0)
    b, e = rodent.body_rewards(x, x, ALL, EFF, W, K)
    assert b.shape == (4,) and e.shape == (4,) and b.dtype == np.float64 and e.dtype == np.float64
    assert np.array_equal(b, np.full(4, W[0])) and np.array_equal(e, np.full(4, W[1]))


def test_one_body_off_by_three_and_four_centimetres():
    x = _xpos(1)
    for body in (1, 30, NBODY - 1):           # none of them an end effector
        ref = x.copy()
        ref[:, body] += [0.03, 0.04, 0.0]
        b, e = rodent.body_rewards(x, ref, ALL, EFF, W, K)
        np.testing.assert_allclose(b, W[0] * math.exp(-K[0] * 0.0025), rtol=1e-12)
        assert np.array_equal(e, np.full(4, W[1]))
    ref = x.copy()
    ref[:, 64] -= [0.0, 0.03, 0.04]           # an end effector: both terms see it, the sharper one more
    b, e = rodent.body_rewards(x, ref, ALL, EFF, W, K)
    np.testing.assert_allclose(b, W[0] * math.exp(-K[0] * 0.0025), rtol=1e-12)
    np.testing.assert_allclose(e, W[1] * math.exp(-K[1] * 0.0025), rtol=1e-12)
    ref[:, 11] += [0.1, 0.0, 0.0]             # two bodies: the squared distances add
    b, e = rodent.body_rewards(x, ref, ALL, EFF, W, K)
    np.testing.assert_allclose(b, W[0] * math.exp(-K[0] * 0.0125), rtol=1e-12)
    np.testing.assert_allclose(e, W[1] * math.exp(-K[1] * 0.0125), rtol=1e-12)


def test_a_body_outside_the_set_does_not_count():
    x = _xpos(2)
    ref = x.copy()
    ref[:, 7] += 5.0
    ref[:, 0] += 3.0                          # the world body is in no set
    b, e = rodent.body_rewards(x, ref, (1, 2, 3, 8), EFF, W, K)
    assert np.array_equal(b, np.full(4, W[0])) and np.array_equal(e, np.full(4, W[1]))
    b, _ = rodent.body_rewards(x, ref, (1, 7), EFF, W, K)
    np.testing.assert_allclose(b, W[0] * math.exp(-K[0] * 75.0), rtol=1e-12)


def test_an_empty_set_sums_to_zero():
    x, ref = _xpos(3), _xpos(4)
    for none in (None, (), []):
        b, e = rodent.body_rewards(x, ref, ALL, none, W, K)
        assert np.array_equal(e, np.full(4, W[1]))          # exp(-k * 0): the env gives such a term weight 0 (below)
        assert (b < W[0]).all()
    b, e = rodent.body_rewards(x, ref, ALL, None, (1.0, 0.0), K)
    assert np.array_equal(e, np.zeros(4))


def test_overlapping_sets_score_a_body_in_both():
    x = _xpos(5)
    ref = x.copy()
    ref[:, 2] += [0.0, 0.0, 0.1]
    ref[:, 3] += [0.2, 0.0, 0.0]
    ref[:, 4] += [0.0, 0.3, 0.0]
    b, e = rodent.body_rewards(x, ref, (2, 3), (3, 4), (1.0, 1.0), (1.0, 1.0))
    np.testing.assert_allclose(b, math.exp(-(0.01 + 0.04)), rtol=1e-12)
    np.testing.assert_allclose(e, math.exp(-(0.04 + 0.09)), rtol=1e-12)


def test_leading_axes_broadcast():
    x, ref = _xpos(6, N=6).reshape(2, 3, NBODY, 3), _xpos(7, N=6).reshape(2, 3, NBODY, 3)
    got = rodent.body_rewards(x, ref, ALL, EFF, W, (0.01, 0.02))
    flat = rodent.body_rewards(x.reshape(6, NBODY, 3), ref.reshape(6, NBODY, 3), ALL, EFF, W, (0.01, 0.02))
    for a, b in zip(got, flat):
        assert a.shape == (2, 3) and np.array_equal(a.reshape(6), b)


# ---------------------------------------------------------------------------------------------- argument check
def _chk(track=None, bodies="ok", body_ids=None, eff=None, ws=(1.0, 8.0, 1.0, 100.0), have_pose=True, nbody=NBODY):
    track = np.zeros((5, 3)) if track is None else track
    if isinstance(bodies, str):
        bodies = np.zeros(track.shape[:-1] + (nbody, 3))
    return rodent._check_body_tracking(track, bodies, body_ids, eff, nbody, ws, have_pose)


def test_what_the_argument_check_returns():
    assert _chk(bodies=None) is None and _chk(bodies=None, have_pose=False) is None
    rows, masks, B, E = _chk()
    assert rows.dtype == np.float32 and rows.shape == (5, NBODY, 3) and rows.flags["C_CONTIGUOUS"]
    assert B == ALL and E == ()
    assert masks.dtype == np.float32 and masks.shape == (2, NBODY)
    assert masks[0, 0] == 0 and (masks[0, 1:] == 1).all() and (masks[1] == 0).all()
    rows, masks, B, E = _chk(track=np.zeros((3, 5, 3)), body_ids=[4, 2], eff=np.array(EFF))
    assert rows.shape == (3, 5, NBODY, 3) and B == (4, 2) and E == EFF
    assert sorted(np.nonzero(masks[0])[0].tolist()) == [2, 4] and sorted(np.nonzero(masks[1])[0].tolist()) == sorted(EFF)
    assert _chk(body_ids=[], eff=[NBODY - 1])[2:] == ((), (NBODY - 1,))


def test_every_refusal_of_the_argument_check():
    with pytest.raises(ValueError, match="need track_bodies"):
        _chk(bodies=None, body_ids=[1])
    with pytest.raises(ValueError, match="need track_bodies"):
        _chk(bodies=None, eff=[1])
    with pytest.raises(ValueError, match="track_quat and track_joints"):
        _chk(have_pose=False)
    for shape in ((5, NBODY), (5, NBODY - 1, 3), (4, NBODY, 3), (1, 5, NBODY, 3), (5, NBODY, 4)):
        with pytest.raises(ValueError, match="must have shape"):
            _chk(bodies=np.zeros(shape))
    with pytest.raises(ValueError, match="must have shape"):
        _chk(track=np.zeros((2, 5, 3)), bodies=np.zeros((5, NBODY, 3)))
    for bad in (np.nan, np.inf, -np.inf):
        b = np.zeros((5, NBODY, 3))
        b[3, 17, 1] = bad
        with pytest.raises(ValueError, match="non-finite"):
            _chk(bodies=b)
    for name, key in (("body_ids", "body_ids"), ("end_effector_ids", "eff")):
        for bad in ([0], [NBODY], [-1], [1, NBODY + 5], [1.0], [True], ["3"], [None]):
            with pytest.raises(ValueError, match=name + " must be ints in 1 .. %d" % (NBODY - 1)):
                _chk(**{key: bad})
        with pytest.raises(ValueError, match=name + " must be unique"):
            _chk(**{key: [3, 5, 3]})
    for k in range(4):
        for bad in (-1.0, -1e-30, math.inf, -math.inf, math.nan, 1e39):       # 1e39 is inf as a float32
            ws = [1.0, 8.0, 1.0, 100.0]
            ws[k] = bad
            with pytest.raises(ValueError, match="finite and >= 0"):
                _chk(ws=ws)
            with pytest.raises(ValueError, match="finite and >= 0"):
                _chk(bodies=None, ws=ws)                                       # checked whether or not the bodies are given
        for bad in ("1", True, None, [1.0]):
            ws = [1.0, 8.0, 1.0, 100.0]
            ws[k] = bad
            with pytest.raises(ValueError, match="must be numbers"):
                _chk(ws=ws)
    assert _chk(ws=(0, 0.0, np.float32(0), 0)) is not None                    # 0 is allowed: that term is off


# ---------------------------------------------------------------------------------------------- ABI
def test_the_ctypes_mirror_matches_the_header():
    header = open(os.path.join(ROOT, "include", "rodent_rr.h")).read()
    m = re.search(r"typedef struct rr_body_io \{(.*?)\} rr_body_io;", header, re.S)
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
    want = [("track_bodies", "ptr"), ("body_weights", "ptr"), ("body_metrics", "ptr"), ("body_reward_weight", "float"),
            ("body_reward_scale", "float"), ("endeff_reward_weight", "float"), ("endeff_reward_scale", "float")]
    assert members == want, members
    kinds = {"ptr": ctypes.c_void_p, "float": ctypes.c_float}
    assert [(n, t) for n, t in hip.RRBodyIO._fields_] == [(n, kinds[k]) for n, k in members]
    offsets = {n: getattr(hip.RRBodyIO, n).offset for n, _ in members}
    assert offsets == dict(track_bodies=0, body_weights=8, body_metrics=16, body_reward_weight=24, body_reward_scale=28,
                           endeff_reward_weight=32, endeff_reward_scale=36) and ctypes.sizeof(hip.RRBodyIO) == 40
    for decl in ("int rr_batch_set_body_tracking(rr_batch* b, const rr_body_io* body);",
                 "int rr_batch_body_tracking_supported(const rr_batch* b, int32_t with_actor);"):
        assert decl in header


def test_the_two_exports_and_their_signatures():
    for name in ("rr_batch_set_body_tracking", "rr_batch_body_tracking_supported"):
        assert name in hip.EXPORTS
    lib = hip.lib()
    assert lib.rr_batch_set_body_tracking.argtypes == [ctypes.c_void_p, ctypes.POINTER(hip.RRBodyIO)]
    assert lib.rr_batch_body_tracking_supported.argtypes == [ctypes.c_void_p, ctypes.c_int32]
    assert lib.rr_batch_set_body_tracking(None, None) == -1 and b"null batch" in lib.rr_last_error()          # RR_EINVAL, no device needed
    assert lib.rr_batch_body_tracking_supported(None, 0) == -1 and b"null batch" in lib.rr_last_error()


def test_the_closed_structs_stay_closed():
    """rr_env_io ends with the clip members, rr_pose_io with its four floats, rr_pose_term_io with its pad: the body block is a struct
    of its own."""
    assert [n for n, _ in hip.RREnvIOClips._fields_][-2:] == ["clip", "num_clips"]
    assert [n for n, _ in hip.RRPoseIO._fields_] == ["track_pose", "pose_metrics", "quat_reward_weight", "quat_reward_scale", "joint_reward_weight", "joint_reward_scale"]
    assert [n for n, _ in hip.RRPoseTermIO._fields_] == ["fail", "max_pos", "max_quat", "max_joint", "pad"]
    assert ctypes.sizeof(hip.RRPoseIO) == 32 and ctypes.sizeof(hip.RRPoseTermIO) == 24
    header = open(os.path.join(ROOT, "include", "rodent_rr.h")).read()
    for name in ("rr_env_io", "rr_pose_io", "rr_pose_term_io"):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S)
        assert m and "track_bodies" not in m.group(1) and "body_metrics" not in m.group(1), name
