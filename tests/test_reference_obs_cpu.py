"""Reference observation (`Rodent(reference_obs_frames=H)`; rr_batch_set_reference_obs) as far as it can be held without a GPU: known
answers of the float64 restatement `reference_obs`, every refusal of the constructor's argument check through the helper it calls, and
the three new exports with their ctypes signatures.  The GPU half is tests/test_gpu_reference_obs.py."""
import ctypes
import os

import numpy as np
import pytest

from rodent_amd import hip
from rodent_amd.envs import rodent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NQ = 74


def _qmul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def _unit(rng, shape):
    q = rng.normal(size=shape + (4,))
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def _state(seed, N=5):
    rng = np.random.default_rng(seed)
    return rng, np.concatenate([rng.normal(size=(N, 3)), _unit(rng, (N,)), rng.uniform(-1, 1, (N, NQ - 7))], axis=1)


def _blocks(out, H):
    b = out.reshape(out.shape[0], H, NQ)
    return b[..., :3], b[..., 3:7], b[..., 7:]


def test_reference_equal_to_the_state_gives_the_identity_and_zero():
    """The clip IS the state at every frame: p = 0, q = (1, 0, 0, 0), j = 0 in every block."""
    _, qpos = _state(0, N=1)
    T, H = 6, 3
    tp, tq, tj = (np.repeat(qpos[:, s], T, axis=0) for s in (slice(0, 3), slice(3, 7), slice(7, None)))
    out = rodent.reference_obs(qpos, tp, tq, tj, frame=[2], frames=H)
    assert out.shape == (1, H * NQ)
    p, q, j = _blocks(out, H)
    np.testing.assert_allclose(p, 0.0, atol=1e-15)
    np.testing.assert_allclose(q, np.broadcast_to([1.0, 0.0, 0.0, 0.0], q.shape), atol=1e-15)
    assert np.array_equal(j, np.zeros_like(j))


def test_negated_reference_quaternion_gives_the_same_block():
    rng, qpos = _state(1)
    T, H = 7, 2
    tp, tq, tj = rng.normal(size=(T, 3)), _unit(rng, (T,)), rng.uniform(-1, 1, (T, NQ - 7))
    frame = np.array([0, 1, 2, 3, 4])
    want = rodent.reference_obs(qpos, tp, tq, tj, frame, H)
    got = rodent.reference_obs(qpos, tp, -tq, tj, frame, H)
    np.testing.assert_array_equal(got, want)
    _, q, _ = _blocks(want, H)
    assert (q[..., 0] >= 0).all() and np.allclose(np.linalg.norm(q, axis=-1), 1.0, atol=1e-14)
    signs = np.sign(np.einsum("ni,nhi->nh", qpos[:, 3:7], tq[np.clip(frame[:, None] + np.arange(1, H + 1), 0, T - 1)]))
    assert (signs > 0).any() and (signs < 0).any()                # both branches of the sign rule ran


def test_half_turn_about_z():
    """The reference is the root turned by pi about its own z axis: q = conj(x) (x) (x (x) (0,0,0,1)) = (0, 0, 0, 1) (w = 0: no flip), and the
    track point one unit ahead along the root's x axis has p = (1, 0, 0)."""
    _, qpos = _state(2, N=1)
    x = qpos[0, 3:7]
    R = rodent._quat_to_mat(x)
    tq = _qmul(x, np.array([0.0, 0.0, 0.0, 1.0]))[None]
    tp = (qpos[0, :3] + R.T @ np.array([1.0, 0.0, 0.0]))[None]           # xmat[1] @ (tp - pos) = R R' e_x
    out = rodent.reference_obs(qpos, tp, tq, qpos[:, 7:] + 0.25, frame=[0], frames=1)
    p, q, j = _blocks(out, 1)
    np.testing.assert_allclose(p[0, 0], [1.0, 0.0, 0.0], atol=1e-14)
    np.testing.assert_allclose(np.abs(q[0, 0]), [0.0, 0.0, 0.0, 1.0], atol=1e-14)
    np.testing.assert_allclose(j, 0.25, rtol=0, atol=1e-15)


def test_frames_past_the_clip_end_repeat_the_last_row():
    rng, qpos = _state(3, N=3)
    T, H = 4, 5
    tp, tq, tj = rng.normal(size=(T, 3)), _unit(rng, (T,)), rng.uniform(-1, 1, (T, NQ - 7))
    out = rodent.reference_obs(qpos, tp, tq, tj, frame=[0, 2, 50], frames=H).reshape(3, H, NQ)
    last = rodent.reference_obs(qpos, tp[-1:], tq[-1:], tj[-1:], frame=[0, 0, 0], frames=1).reshape(3, NQ)
    for n, first_clamped in enumerate((2, 0, 0)):       # frame + h >= T - 1 from block index first_clamped on
        for h in range(first_clamped, H):
            np.testing.assert_array_equal(out[n, h], last[n])
    assert not np.array_equal(out[0, 0], out[0, 1]) and not np.array_equal(out[0, 1], out[0, 2])       # frames 1, 2, 3 differ
    neg = rodent.reference_obs(qpos, tp, tq, tj, frame=[-9, -9, -9], frames=1).reshape(3, NQ)          # ... and the clamp at 0
    first = rodent.reference_obs(qpos, tp[:1], tq[:1], tj[:1], frame=[0, 0, 0], frames=1).reshape(3, NQ)
    np.testing.assert_array_equal(neg, first)


def test_the_clip_id_selects_its_clip():
    rng, qpos = _state(4, N=4)
    C, T, H = 3, 6, 2
    tp, tq, tj = rng.normal(size=(C, T, 3)), _unit(rng, (C, T)), rng.uniform(-1, 1, (C, T, NQ - 7))
    frame, clip = np.array([0, 1, 2, 3]), np.array([2, 0, 1, 7])        # 7: clamped to the last clip
    out = rodent.reference_obs(qpos, tp, tq, tj, frame, H, clip=clip)
    for n, c in enumerate((2, 0, 1, 2)):
        one = rodent.reference_obs(qpos[n:n + 1], tp[c], tq[c], tj[c], frame[n:n + 1], H)
        np.testing.assert_array_equal(out[n], one[0])
        other = rodent.reference_obs(qpos[n:n + 1], tp[(c + 1) % C], tq[(c + 1) % C], tj[(c + 1) % C], frame[n:n + 1], H)
        assert not np.array_equal(out[n], other[0])


def test_xquat_and_xmat_override_the_root_pose():
    rng, qpos = _state(5, N=2)
    T = 3
    tp, tq, tj = rng.normal(size=(T, 3)), _unit(rng, (T,)), rng.uniform(-1, 1, (T, NQ - 7))
    x = _unit(rng, (2,))
    moved = qpos.copy()
    moved[:, 3:7] = x
    np.testing.assert_array_equal(rodent.reference_obs(qpos, tp, tq, tj, [0, 1], 2, xquat=x, xmat=rodent._quat_to_mat(x)),
                                  rodent.reference_obs(moved, tp, tq, tj, [0, 1], 2))


def test_every_refusal_of_the_argument_check():
    for bad in (-1, 17, 100):
        with pytest.raises(ValueError, match=r"\[0, 16\]"):
            rodent._check_reference_frames(bad, True)
    for bad in (1.0, 2.5, "3", None, True, np.float32(2)):
        with pytest.raises(ValueError, match="must be an int"):
            rodent._check_reference_frames(bad, True)
    for h in (1, 16):
        with pytest.raises(ValueError, match="track_quat and track_joints"):
            rodent._check_reference_frames(h, False)
    assert rodent._check_reference_frames(0, False) == 0 and rodent._check_reference_frames(0, True) == 0
    assert rodent._check_reference_frames(16, True) == 16 and rodent._check_reference_frames(np.int64(5), True) == 5
    assert type(rodent._check_reference_frames(np.int32(3), True)) is int


def test_the_three_exports_and_their_signatures():
    for name in ("rr_batch_set_reference_obs", "rr_batch_obs_width", "rr_batch_reference_obs_supported"):
        assert name in hip.EXPORTS
    lib = hip.lib()
    assert lib.rr_batch_set_reference_obs.argtypes == [ctypes.c_void_p, ctypes.c_int32]
    assert lib.rr_batch_obs_width.argtypes == [ctypes.c_void_p] and lib.rr_batch_obs_width.restype is ctypes.c_int32
    assert lib.rr_batch_reference_obs_supported.argtypes == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32]
    for call, args in ((lib.rr_batch_set_reference_obs, (None, 1)), (lib.rr_batch_obs_width, (None,)), (lib.rr_batch_reference_obs_supported, (None, 1, 0))):
        assert call(*args) == -1 and b"null batch" in lib.rr_last_error()        # RR_EINVAL, no device needed
    header = open(os.path.join(ROOT, "include", "rodent_rr.h")).read()
    for decl in ("int rr_batch_set_reference_obs(rr_batch* b, int32_t frames);", "int32_t rr_batch_obs_width(const rr_batch* b);",
                 "int rr_batch_reference_obs_supported(const rr_batch* b, int32_t frames, int32_t with_actor);"):
        assert decl in header
