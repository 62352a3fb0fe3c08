"""`Rodent`: the reference task env [REF Rodent_Env_Brax.py:19-162] on the HIP backend.

Same constructor arguments, `reset(rng)` / `step(state, action)` surface, reward / done / obs
arithmetic and `info['cur_frame']` bookkeeping as the reference; tensors are torch (leading env
axis N) instead of vmapped jax arrays.  `step` runs ONE fused kernel launch: n_frames physics
substeps + reward / done / observation epilogue (C ABI `rr_env_step`).
"""
from __future__ import annotations

import inspect
import math
import os
import warnings
from typing import Callable, NamedTuple, Optional

import numpy as np
import torch

from .. import assets, jax_random
from .base import PipelineEnv, PipelineState, State, System

_XML_PATH = "./models/rodent_new.xml"   # [REF Rodent_Env_Brax.py:16]


def bad_state_mask(qpos: torch.Tensor, qvel: torch.Tensor, bad_state_max: float) -> torch.Tensor:
    """The bad-state rule of the step kernel's epilogue in plain torch: env e is bad iff some element x of qpos[e] or qvel[e] fails
    |x| <= bad_state_max (float32) -- written that way round, so NaN and +-inf are bad.  bool [N].  For tests and for users who compose the
    env step by step themselves (MuJoCo's mj_checkPos / mj_checkVel with mjMAXVAL = 1e10)."""
    lim = torch.tensor(float(bad_state_max), dtype=torch.float32, device=qpos.device)
    ok = lambda x: (x.to(torch.float32).abs() <= lim).flatten(1).all(dim=1)
    return ~(ok(qpos) & ok(qvel))


def reset_draws(keys, nq: int, nv: int, reset_noise_scale: float, num_clips: Optional[int] = None):
    """The host draws of `Rodent.reset`, without a device: `keys` uint32 [N, 2] -> (start_frame int32 [N], qpos noise float32 [N, nq],
    qvel float32 [N, nv], clip int32 [N] or None).  The key chain is the reference's, `rng, rng1, rng2, rng_pos = split(rng, 4)`
    [REF Rodent_Env_Brax.py:98-113]: start_frame from rng, the qpos noise from rng1, qvel from rng2.  The reference splits off rng_pos and
    never uses it; with `num_clips` given (an env with a [C, T, 3] track) the clip id is `randint(rng_pos, 0, num_clips)`, so no other draw
    moves whether there are clips or not."""
    keys = np.asarray(keys, dtype=np.uint32).reshape(-1, 2)
    ks = jax_random.split(keys, 4)                       # rng, rng1, rng2, rng_pos
    start_frame = jax_random.randint(ks[:, 0], 0, 100)   # [N] int32
    low, hi = -reset_noise_scale, reset_noise_scale
    qpos_noise = jax_random.uniform(ks[:, 1], nq, low, hi)
    qvel = jax_random.uniform(ks[:, 2], nv, low, hi)
    clip = None if num_clips is None else jax_random.randint(ks[:, 3], 0, int(num_clips)).astype(np.int32)
    return start_frame, qpos_noise, qvel, clip


def restart_bank_draws(keys, num_entries: int, nq: int, nv: int, reset_noise_scale: float, frame_range=(0, 100), num_clips: Optional[int] = None,
                       across_clips: bool = False):
    """The host draws of the start bank of `Rodent(clip_restarts=K)`, without a device: `keys` uint32 [N, 2] -> (start_frame int32
    [K, N], qpos noise float32 [K, N, nq], qvel float32 [K, N, nv], clip int32 [N] or None).  Entry 0 is `reset_draws(keys)` itself,
    whatever K is.  Entry k = 1 .. K - 1 is `reset_draws(fold_in(keys, k))` -- qpos noise and qvel -- except its start frame, which is
    `randint(lo, hi)` of that key's first subkey, `frame_range` = (lo, hi).  The clip is the one of `keys`: every entry follows it.
    `across_clips` (`Rodent(restart_across_clips=True)`, needs `num_clips`): the clip is int32 [K, N] instead, entry k the clip that
    `reset_draws(fold_in(keys, k), num_clips=C)` returns and the default discards -- no new key is consumed, no other draw moves."""
    keys = np.asarray(keys, dtype=np.uint32).reshape(-1, 2)
    lo, hi = frame_range
    frames, noises, qvels, clips = [], [], [], []
    for k in range(int(num_entries)):
        kk = keys if k == 0 else jax_random.fold_in(keys, k)
        f, noise, qvel, drawn = reset_draws(kk, nq, nv, reset_noise_scale, num_clips)
        if k > 0:
            f = jax_random.randint(jax_random.split(kk, 4)[:, 0], int(lo), int(hi))
        frames.append(np.asarray(f, dtype=np.int32)); noises.append(noise); qvels.append(qvel); clips.append(drawn)
    clip = clips[0] if not across_clips or clips[0] is None else np.stack(clips)
    return np.stack(frames), np.stack(noises), np.stack(qvels), clip


def fold_start_frames(start_frame, lengths: Optional[np.ndarray], clip=None) -> np.ndarray:
    """The start frames of an env with per-clip lengths (`Rodent(clip_lengths=...)`), int32 like `start_frame` ([N] or [K, N]): the
    draws folded into their clip, start = draw mod (L_c - 1) with c the entry's clip (`clip` broadcast against `start_frame`; None:
    clip 0).  The identity wherever draw < L_c - 1, and every start is <= L_c - 2, so the track entry of the reset observation (frame
    + 1) lies within the clip.  `lengths` None: the draws as they are."""
    start_frame = np.asarray(start_frame, dtype=np.int32)
    if lengths is None:
        return start_frame
    L = np.asarray(lengths, dtype=np.int64)[0 if clip is None else np.asarray(clip, dtype=np.int64)]
    return (start_frame.astype(np.int64) % (L - 1)).astype(np.int32)


def reference_rows(rows: np.ndarray, frame, clip=None, lengths: Optional[np.ndarray] = None) -> np.ndarray:
    """The rows of a clip array `rows` [(C,) T, ...] (track_pos, the pose rows, track_bodies, track_vel) that an env on clip `clip` at
    frame `frame` reads: rows[(clip,) clamp(frame, 0, L_c - 1)], L_c = `lengths`[clip] (None: T for every clip; `clip` None: clip 0 of
    a [T, ...] array).  The one place the host restatements clamp a frame: `pose_rewards`, `pose_errors`, `body_rewards` and
    `velocity_rewards` take the rows it returns, `reference_obs`, `reset_qpos` and `reset_qvel` call it with their `lengths` argument.
    No row at or behind L_c is touched."""
    frame = np.asarray(frame, dtype=np.int64)
    T = rows.shape[0] if clip is None else rows.shape[1]
    if clip is None:
        last = T - 1 if lengths is None else int(np.asarray(lengths).reshape(-1)[0]) - 1
        return rows[np.clip(frame, 0, last)]
    c = np.clip(np.asarray(clip, dtype=np.int64), 0, rows.shape[0] - 1)
    last = T - 1 if lengths is None else np.asarray(lengths, dtype=np.int64)[c] - 1
    return rows[c, np.clip(frame, 0, last)]


def _check_clip_library(clip_lengths, restart_across_clips, track: np.ndarray, have_pose: bool, clip_restarts: int):
    """`clip_lengths` and `restart_across_clips` of `Rodent` against its (checked) `track` [(C,) T, 3] as (lengths int32 [C] or None,
    flag).  ValueError for either without the pose arguments, lengths that are not integers of shape [C] (an int or [1] next to a
    [T, 3] track) with 2 <= L_c <= T, and `restart_across_clips` without `clip_restarts >= 1` or without a clip axis."""
    across = bool(restart_across_clips)
    if (clip_lengths is not None or across) and not have_pose:
        raise ValueError("clip_lengths / restart_across_clips need the reference pose: pass track_quat and track_joints")
    if across and clip_restarts < 1:
        raise ValueError("restart_across_clips=True needs clip_restarts >= 1: the clips belong to the entries of the start bank")
    if across and track.ndim != 3:
        raise ValueError("restart_across_clips=True needs a [C, T, 3] track_pos: a single [T, 3] track has no other clip to move to")
    if clip_lengths is None:
        return None, across
    C_, T = (track.shape[0] if track.ndim == 3 else 1), track.shape[-2]
    L = clip_lengths.detach().cpu().numpy() if torch.is_tensor(clip_lengths) else np.asarray(clip_lengths)
    if L.dtype.kind not in "iu":
        raise ValueError(f"clip_lengths must be integers, got dtype {L.dtype}")
    if L.ndim == 0 and track.ndim == 2:
        L = L.reshape(1)
    if L.shape != (C_,):
        raise ValueError(f"clip_lengths must have shape ({C_},) next to a track_pos of shape {track.shape}"
                         f"{' (or be an int)' if track.ndim == 2 else ''}, got {tuple(L.shape)}")
    if L.min() < 2 or L.max() > T:
        raise ValueError(f"clip_lengths must lie in 2 .. T = {T} (a clip needs a frame to start at and a next one), got {int(L.min())} .. {int(L.max())}")
    return np.ascontiguousarray(L, dtype=np.int32), across


_M32 = np.uint64(0xFFFFFFFF)
MAX_CLIP_WEIGHT = 65535      # the largest entry of the device's weight table; K <= 64 entries then sum within 32 bits
OUTCOME_COLUMNS = ("episodes", "pose_fail", "env_done", "truncated", "steps")      # the columns of the [C, 5] outcome table


def _fmix32(h):
    """MurmurHash3's 32-bit finaliser on uint64 arrays holding 32-bit values."""
    h = np.asarray(h, dtype=np.uint64) & _M32
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & _M32
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & _M32
    return h ^ (h >> np.uint64(16))


def restart_hash(seed, env, n) -> np.ndarray:
    """The 32-bit hash a weighted restore draws with (`Rodent(restart_sampling="weighted")`; C ABI `rr_clip_sampling_io`), uint64 holding
    32-bit values, broadcast over `env` and `n`: fmix32((fmix32(seed ^ (env * 0x9E3779B1)) + n)), every operation mod 2**32, fmix32
    MurmurHash3's finaliser.  `env` the env's index, `n` its restore count (`info['restart_draws']`) before the restore."""
    env = np.asarray(env).astype(np.uint64) & _M32
    n = np.asarray(n).astype(np.uint64) & _M32
    first = _fmix32((np.uint64(int(seed) & 0xFFFFFFFF) ^ ((env * np.uint64(0x9E3779B1)) & _M32)))
    return _fmix32((first + n) & _M32)


def weighted_slot(h, slot_weights, slot: int = 0) -> int:
    """The bank entry a weighted restore takes: `h` the 32-bit hash (`restart_hash`), `slot_weights` the K integer weights q_k of the
    env's bank entries (`clip_weights()[bank clip[k]]`, 0 .. 65535), S their sum.  r = (h * S) >> 32 and the result is the smallest k
    with q_0 + .. + q_k > r: an entry of weight 0 is never drawn.  S == 0: the cyclic rule's (`slot` + 1) mod K."""
    q = [int(x) for x in np.asarray(slot_weights).reshape(-1)]
    S = sum(q)
    if S == 0:
        return (int(slot) + 1) % len(q)
    r = (int(h) * S) >> 32
    acc = 0
    for k, qk in enumerate(q):
        acc += qk
        if acc > r:
            return k
    raise AssertionError("unreachable: r < S")


MAX_REFERENCE_CLIPS = 32768      # clips a reference restart draws over: the weights' sum times a 32-bit hash stays within 63 bits


def reference_restart_hash(seed, env, n, purpose: int, element=0) -> np.ndarray:
    """The 32-bit hashes a reference restart draws with (`Rodent(restart_from_reference=True)`; C ABI `rr_reference_restart_io`), uint64
    holding 32-bit values: fmix32(restart_hash(seed, env, n) ^ (((purpose << 16) | element) * 0x9E3779B1)), mod 2**32.  `purpose`: 1 the
    clip, 2 the frame, 3 the qpos noise, 4 the qvel noise; `element` the index within qpos / qvel (broadcast against `env` and `n`)."""
    tag = (np.uint64(int(purpose) << 16) | (np.asarray(element).astype(np.uint64) & np.uint64(0xFFFF))) * np.uint64(0x9E3779B1)
    return _fmix32(restart_hash(seed, env, n) ^ (tag & _M32))


def reference_restart_draws(seed, env, n, frame_range, clip=None, num_clips: Optional[int] = None, across_clips: bool = False, weights=None,
                            lengths=None):
    """The clip and start frame a reference restart of env `env` at restore count `n` (`info['restart_draws']` before the restore) takes,
    in integers: (clip int32 [N] or None, draw int32 [N], frame int32 [N]).

    clip:  with `across_clips` and `num_clips` = C, over all C clips with h = reference_restart_hash(seed, env, n, 1): by `weights` (the
           int table of `clip_weights()`, sum S > 0) the smallest c with q_0 + .. + q_c > (h * S) >> 32 -- `weighted_slot`'s prefix rule
           on the C clip weights, a clip of weight 0 is never drawn --, without a table or with S == 0 uniformly, (h * C) >> 32.
           Otherwise `clip` itself (None without a clip axis).
    draw:  lo + ((h' * (hi - lo)) >> 32), h' = reference_restart_hash(seed, env, n, 2), `frame_range` = (lo, hi): in [lo, hi).
    frame: the draw folded into the drawn clip as every start frame is (`fold_start_frames`: draw mod (L_c - 1) with `lengths`, else the
           draw itself; the rows are then read at the clamped frame, `reference_rows`)."""
    env, n = np.broadcast_arrays(np.asarray(env, dtype=np.int64), np.asarray(n, dtype=np.int64))
    lo, hi = (int(x) for x in frame_range)
    if across_clips and num_clips is not None:
        h = reference_restart_hash(seed, env, n, 1)
        q = None if weights is None else (np.asarray(weights).astype(np.uint64) & np.uint64(0xFFFF))
        if q is not None and int(q.sum()) > 0:
            prefix = np.cumsum(q)
            r = (h * prefix[-1]) >> np.uint64(32)
            clip = np.searchsorted(prefix, r, side="right").astype(np.int32)       # the first index whose prefix exceeds r
        else:
            clip = ((h * np.uint64(int(num_clips))) >> np.uint64(32)).astype(np.int32)
    elif clip is not None:
        clip = np.broadcast_to(np.asarray(clip, dtype=np.int32), env.shape).copy()
    draw = (lo + ((reference_restart_hash(seed, env, n, 2) * np.uint64(hi - lo)) >> np.uint64(32)).astype(np.int64)).astype(np.int32)
    return clip, draw, fold_start_frames(draw, lengths, clip)


def reference_restart_noise(seed, env, n, purpose: int, width: int, noise_scale: float) -> np.ndarray:
    """The noise of a reference restart, float32 [N, width]: noise_scale * s with s = (h_i >> 8) * 2**-23 - 1 in [-1, 1) -- exact in
    float32 -- and h_i = reference_restart_hash(seed, env, n, purpose, i); one rounded float32 product.  Uniform like the noise of
    `reset_draws`, from another generator."""
    env, n = np.broadcast_arrays(np.asarray(env, dtype=np.int64), np.asarray(n, dtype=np.int64))
    h = reference_restart_hash(seed, env[:, None], n[:, None], purpose, np.arange(int(width))[None, :])
    s = (h >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1.0)
    return np.float32(noise_scale) * s


def reference_restart_state(seed, env, n, clip, frame, track: np.ndarray, pose: np.ndarray, track_vel: Optional[np.ndarray], noise_scale: float,
                            lengths=None):
    """The state a reference restart starts from, (qpos float32 [N, nq], qvel float32 [N, nv]), for the clip and frame of
    `reference_restart_draws`: qpos = [track[(clip,) frame], pose[(clip,) frame]] and qvel = track_vel[(clip,) frame] (zeros for
    `track_vel` an int: that many dofs, an env without a velocity block), the frame clamped within the clip (`reference_rows`: no row at
    or behind L_c is read), each plus `reference_restart_noise` (purpose 3 / 4) in one rounded float32 sum."""
    rows = lambda a: np.asarray(reference_rows(a, frame, clip, lengths), dtype=np.float32)
    qpos = np.concatenate([rows(track), rows(pose)], axis=-1)
    qvel = np.zeros((qpos.shape[0], int(track_vel)), dtype=np.float32) if isinstance(track_vel, (int, np.integer)) else rows(track_vel)
    return (qpos + reference_restart_noise(seed, env, n, 3, qpos.shape[1], noise_scale),
            qvel + reference_restart_noise(seed, env, n, 4, qvel.shape[1], noise_scale))


def _fmix32_t(h: torch.Tensor) -> torch.Tensor:
    """`_fmix32` on int64 tensors holding 32-bit values (a product's low 32 bits survive the int64 wrap-around)."""
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    return h ^ (h >> 16)


def _reference_restart_hash_t(seed: int, env: torch.Tensor, n: torch.Tensor, purpose: int, element=0) -> torch.Tensor:
    """`reference_restart_hash` in torch integers (the device form the per-step wrappers draw with)."""
    base = _fmix32_t((_fmix32_t((int(seed) & 0xFFFFFFFF) ^ ((env * 0x9E3779B1) & 0xFFFFFFFF)) + (n & 0xFFFFFFFF)) & 0xFFFFFFFF)
    return _fmix32_t(base ^ ((((int(purpose) << 16) | element) * 0x9E3779B1) & 0xFFFFFFFF))


def _check_reference_restart(restart_from_reference, restart_noise_seed, reset_to_reference: bool, clip_restarts: int, have_pose: bool,
                             num_clips: Optional[int]):
    """`restart_from_reference` and `restart_noise_seed` of `Rodent` as (flag, seed); ValueError for the flag on a position-only env,
    without `reset_to_reference=True` or without `clip_restarts >= 1`, for more than `MAX_REFERENCE_CLIPS` clips, and for a seed outside
    0 .. 2**32 - 1."""
    on = bool(restart_from_reference)
    if isinstance(restart_noise_seed, (bool, np.bool_)) or not isinstance(restart_noise_seed, (int, np.integer)) or not 0 <= int(restart_noise_seed) < 2 ** 32:
        raise ValueError(f"restart_noise_seed must be an int in 0 .. 2**32 - 1, got {restart_noise_seed!r}")
    if on and not have_pose:
        raise ValueError("restart_from_reference=True needs the reference pose: pass track_quat and track_joints (a position-only env has no pose rows to start from)")
    if on and not reset_to_reference:
        raise ValueError("restart_from_reference=True needs reset_to_reference=True: a restore starts from the clip's pose as the reset does")
    if on and clip_restarts < 1:
        raise ValueError("restart_from_reference=True needs clip_restarts >= 1: it replaces the restore of the clip-restart rule")
    if on and num_clips is not None and num_clips > MAX_REFERENCE_CLIPS:
        raise ValueError(f"restart_from_reference=True serves at most {MAX_REFERENCE_CLIPS} clips, got {num_clips}")
    return on, int(restart_noise_seed)


def quantise_clip_weights(w) -> np.ndarray:
    """Float weights [C], finite, >= 0 and not all zero, as the int32 table the device reads: 0 -> 0, otherwise
    max(1, round(65535 * w / max w)) (round half to even), so the largest weight is 65535 and no positive weight is lost."""
    w = np.asarray(w, dtype=np.float64)
    if w.ndim != 1 or not np.isfinite(w).all() or (w < 0).any() or not (w > 0).any():
        raise ValueError(f"clip weights must be a float [C] array, finite, >= 0 and not all zero, got {w!r}")
    q = np.maximum(1, np.rint(MAX_CLIP_WEIGHT * (w / w.max()))).astype(np.int32)
    return np.where(w > 0, q, 0).astype(np.int32)


def clip_outcome_update(outcomes: np.ndarray, clip, code, done_env, done) -> np.ndarray:
    """One wrapped env step of the outcome counters (`Rodent(clip_outcomes=True)`; C ABI `rr_clip_sampling_io`), added to `outcomes`
    int64 [C, 5] in place (and returned): `clip` int [N] the clip each step was made on (before any restore), `code` [N] the step's
    pose-termination code (0 without pose termination), `done_env` [N] the env's own done, `done` [N] the wrapped done.  Col 4 counts
    the steps, col 0 the ended episodes, and each of those falls into exactly one of col 1 (code != 0), col 2 (else done_env), col 3
    (else: a truncation)."""
    clip = np.asarray(clip, dtype=np.int64).reshape(-1)
    N = clip.shape[0]
    as_flag = lambda a: np.broadcast_to(np.asarray(a).reshape(-1) != 0, (N,))
    failed, own, ended = as_flag(code), as_flag(done_env), as_flag(done)
    col = np.where(failed, 1, np.where(own, 2, 3))
    np.add.at(outcomes, (clip, 4), 1)
    np.add.at(outcomes, (clip[ended], 0), 1)
    np.add.at(outcomes, (clip[ended], col[ended]), 1)
    return outcomes


class FailureWeights:
    """A `clip_weight_fn` for `ppo.train`: restart weights from an exponentially decayed failure rate per clip.  Called with a training
    step's outcome table [C, 5] it updates fails_c <- decay * fails_c + (col 1 + col 2) and episodes_c <- decay * episodes_c + col 0,
    and returns w_c = floor + (1 - floor) * fails_c / episodes_c, with weight 1 for a clip that has not finished an episode yet (so an
    unseen clip is tried).  None -- keep the weights -- while every weight would be 0 (`floor` 0 and no failure so far).  `floor` and
    `decay` are untuned defaults."""

    def __init__(self, floor: float = 0.1, decay: float = 0.9):
        if not 0.0 <= floor <= 1.0 or not 0.0 <= decay < 1.0:
            raise ValueError(f"FailureWeights needs 0 <= floor <= 1 and 0 <= decay < 1, got floor={floor!r}, decay={decay!r}")
        self.floor, self.decay = float(floor), float(decay)
        self.fails = self.episodes = None

    def rates(self) -> Optional[np.ndarray]:
        """The decayed failure rate per clip, NaN for a clip without a finished episode; None before the first call."""
        if self.fails is None:
            return None
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.episodes > 0, self.fails / self.episodes, np.nan)

    def __call__(self, outcomes) -> Optional[np.ndarray]:
        o = np.asarray(outcomes, dtype=np.float64)
        if self.fails is None:
            self.fails, self.episodes = np.zeros(o.shape[0]), np.zeros(o.shape[0])
        self.fails = self.decay * self.fails + (o[:, 1] + o[:, 2])
        self.episodes = self.decay * self.episodes + o[:, 0]
        rate = self.rates()
        w = np.where(np.isnan(rate), 1.0, self.floor + (1.0 - self.floor) * np.nan_to_num(rate))
        return w if (w > 0).any() else None


def _check_clip_sampling(restart_sampling, clip_outcomes, restart_sampling_seed, across: bool, clip_restarts: int, num_clips: Optional[int]):
    """`restart_sampling`, `clip_outcomes` and `restart_sampling_seed` of `Rodent` as (weighted, counting, seed); ValueError for a
    sampling other than None / "weighted", "weighted" without `restart_across_clips=True`, `clip_outcomes=True` without
    `clip_restarts >= 1` or without a clip axis, and a seed outside 0 .. 2**32 - 1."""
    if restart_sampling not in (None, "weighted"):
        raise ValueError(f"restart_sampling must be None (the next entry of the bank) or 'weighted', got {restart_sampling!r}")
    weighted, counting = restart_sampling == "weighted", bool(clip_outcomes)
    if weighted and not across:
        raise ValueError("restart_sampling='weighted' needs restart_across_clips=True: the weights are those of the bank entries' clips")
    if counting and clip_restarts < 1:
        raise ValueError("clip_outcomes=True needs clip_restarts >= 1: the counters sit in the clip-restart rule")
    if counting and num_clips is None:
        raise ValueError("clip_outcomes=True needs a [C, T, 3] track_pos: a single [T, 3] track has no clip axis to count by")
    if isinstance(restart_sampling_seed, (bool, np.bool_)) or not isinstance(restart_sampling_seed, (int, np.integer)) or not 0 <= int(restart_sampling_seed) < 2 ** 32:
        raise ValueError(f"restart_sampling_seed must be an int in 0 .. 2**32 - 1, got {restart_sampling_seed!r}")
    return weighted, counting, int(restart_sampling_seed)


def _check_clip_restarts(clip_restarts, restart_frame_range, end_at_clip_end, have_pose: bool, track_len: int, have_lengths: bool = False):
    """`clip_restarts`, `restart_frame_range` and `end_at_clip_end` of `Rodent` as (K, (lo, hi), flag); ValueError for K outside 0 .. 64,
    any of the three without the pose arguments, `end_at_clip_end` with K = 0, lo < 0 or hi <= lo, and -- with `end_at_clip_end` -- a
    clip so short that some entry can start at its end (T - 1 <= the largest frame an entry can draw; 99 for entry 0): such an env would
    truncate on every step.  With `have_lengths` (`clip_lengths` given) that last refusal does not apply: every start is folded into
    its clip (`fold_start_frames`), which guarantees what it checked."""
    if isinstance(clip_restarts, (bool, np.bool_)) or not isinstance(clip_restarts, (int, np.integer)) or not 0 <= int(clip_restarts) <= 64:
        raise ValueError(f"clip_restarts must be an int in 0 .. 64 (0: the first state comes back, the frame does not), got {clip_restarts!r}")
    K, end = int(clip_restarts), bool(end_at_clip_end)
    if (K > 0 or restart_frame_range is not None or end) and not have_pose:
        raise ValueError("clip_restarts / restart_frame_range / end_at_clip_end need the reference pose: pass track_quat and track_joints")
    if end and K == 0:
        raise ValueError("end_at_clip_end=True needs clip_restarts >= 1: without the bank the restored state does not rejoin the clip")
    lo, hi = (0, 100) if restart_frame_range is None else restart_frame_range
    for x in (lo, hi):
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)):
            raise ValueError(f"restart_frame_range must be two ints (lo, hi), got {restart_frame_range!r}")
    lo, hi = int(lo), int(hi)
    if lo < 0 or hi <= lo:
        raise ValueError(f"restart_frame_range = (lo, hi) needs 0 <= lo < hi (frames are drawn in [lo, hi)), got {(lo, hi)!r}")
    if end and not have_lengths:
        largest = max(99, hi - 1) if K > 1 else 99
        if track_len - 1 <= largest:
            raise ValueError(f"end_at_clip_end=True: the clip has {track_len} frames, but an entry of the start bank can start at frame {largest}; "
                             f"with T - 1 <= {largest} such an env would truncate on every step (use a longer clip or a smaller restart_frame_range)")
    return K, (lo, hi), end


def reset_qpos(qpos0, track: np.ndarray, start_frame, qpos_noise, clip=None, pose: Optional[np.ndarray] = None, lengths=None) -> np.ndarray:
    """The qpos `Rodent.reset` starts from, float32 [N, nq], out of the draws of `reset_draws`: qpos0 with the root position replaced by
    track[(clip,) start_frame] (the frame clamped within the clip), plus the noise.  `pose` (the env's [(C,) T, nq - 3] rows, given with
    `reset_to_reference=True`): qpos[3:] starts from pose[(clip,) start_frame] instead of qpos0[3:].  `lengths` (int [C], the env's
    `clip_lengths`): the clamp is the clip's own, and no row at or behind L_c is read.  The draws are not touched."""
    N = len(start_frame)
    qpos = np.tile(np.asarray(qpos0, dtype=np.float32), (N, 1))
    if lengths is None:
        fi = np.clip(start_frame, 0, track.shape[-2] - 1)
        qpos[:, :3] = track[fi] if clip is None else track[clip, fi]
        if pose is not None:
            qpos[:, 3:] = pose[fi] if clip is None else pose[clip, fi]
    else:
        qpos[:, :3] = reference_rows(track, start_frame, clip, lengths)
        if pose is not None:
            qpos[:, 3:] = reference_rows(pose, start_frame, clip, lengths)
    return qpos + qpos_noise


def reset_qvel(track_vel: np.ndarray, start_frame, qvel_noise, clip=None, lengths=None) -> np.ndarray:
    """The qvel `Rodent.reset` starts from with the clip's velocities given and `reset_to_reference=True`, float32 [N, nv], out of the
    draws of `reset_draws`: track_vel[(clip,) start_frame] (the env's [(C,) T, nv] rows, the frame clamped within the clip) plus the
    noise, a float32 sum.  `lengths`: as in `reset_qpos`.  The draws are not touched."""
    if lengths is None:
        fi = np.clip(start_frame, 0, track_vel.shape[-2] - 1)
        row = track_vel[fi] if clip is None else track_vel[clip, fi]
    else:
        row = reference_rows(track_vel, start_frame, clip, lengths)
    return np.asarray(row, dtype=np.float32) + np.asarray(qvel_noise, dtype=np.float32)


def _check_track(track_pos) -> np.ndarray:
    """track_pos as float32 [T, 3] or [C, T, 3] (C >= 1, T >= 1), ValueError otherwise."""
    t = track_pos.detach().cpu().numpy() if torch.is_tensor(track_pos) else np.asarray(track_pos)
    if t.ndim not in (2, 3) or t.shape[-1] != 3 or 0 in t.shape:
        raise ValueError(f"track_pos must be [T, 3] (one clip) or [C, T, 3] (C >= 1 clips of equal length), got shape {tuple(t.shape)}")
    return np.ascontiguousarray(t, dtype=np.float32)


def _check_clip(clip, num_clips: Optional[int], num_envs: int, entries: Optional[int] = None) -> np.ndarray:
    """Explicit clip ids of `Rodent.reset` as int32 [N]; ValueError for an env without a clip axis, a wrong shape or an id outside [0, C).
    `entries` = K (an env with `restart_across_clips`): ids of shape [K, N], one row per bank entry, pass too and come back as they are."""
    if num_clips is None:
        raise ValueError("reset(clip=...) needs an env built with a [C, T, 3] track_pos; this one has a single [T, 3] track")
    c = clip.detach().cpu().numpy() if torch.is_tensor(clip) else np.asarray(clip)
    if c.dtype.kind not in "iu":
        raise ValueError(f"clip ids must be integers, got dtype {c.dtype}")
    if c.ndim == 0:
        c = np.full(num_envs, c)
    if c.shape != (num_envs,) and (entries is None or c.shape != (entries, num_envs)):
        raise ValueError(f"clip must be an int or have shape ({num_envs},){'' if entries is None else f' or ({entries}, {num_envs})'}, got {tuple(c.shape)}")
    if c.size and (c.min() < 0 or c.max() >= num_clips):
        raise ValueError(f"clip ids must lie in [0, {num_clips}), got {int(c.min())} .. {int(c.max())}")
    return c.astype(np.int32)


def pose_rewards(qpos, ref_quat, ref_joints, weights=(1.0, 1.0), scales=(2.0, 0.5)):
    """The two pose terms of the step kernel's epilogue (`Rodent(track_quat=..., track_joints=...)`; rr_pose_io) restated in
    numpy float64.  `qpos` [..., nq] the stepped state, `ref_quat` [..., 4] (w, x, y, z) and `ref_joints` [..., nq - 7] the clip's row at
    the clip and frame the position reward reads, `weights` = (quat_reward_weight, joint_reward_weight), `scales` likewise.  With
    q = qpos[3:7], j = qpos[7:]:

        d = conj(ref_quat) (x) q,   theta = 2 atan2(|d.xyz|, |d.w|)
        quat_reward  = weights[0] * exp(-scales[0] * theta**2)
        joint_reward = weights[1] * exp(-scales[1] * sum((j - ref_joints)**2))

    theta is the rotation angle between the two orientations in [0, pi]: q and -q are the same rotation (|d.w|), the scale of either
    quaternion cancels in the atan2, and near theta = 0 the angle comes from |d.xyz|, not from 1 - d.w**2.  Returns (quat_reward,
    joint_reward), float64 [...]."""
    qpos, r, rj = (np.asarray(a, dtype=np.float64) for a in (qpos, ref_quat, ref_joints))
    q = qpos[..., 3:7]
    rw, rx, ry, rz = (r[..., i] for i in range(4))
    qw, qx, qy, qz = (q[..., i] for i in range(4))
    dw = rw * qw + rx * qx + ry * qy + rz * qz
    dx = rw * qx - rx * qw - ry * qz + rz * qy
    dy = rw * qy + rx * qz - ry * qw - rz * qx
    dz = rw * qz - rx * qy + ry * qx - rz * qw
    theta = 2.0 * np.arctan2(np.sqrt(dx * dx + dy * dy + dz * dz), np.abs(dw))
    e2 = ((qpos[..., 7:] - rj) ** 2).sum(-1)
    return weights[0] * np.exp(-scales[0] * theta ** 2), weights[1] * np.exp(-scales[1] * e2)


def _check_pose(track: np.ndarray, track_quat, track_joints, nq: int, weights_and_scales=()) -> Optional[np.ndarray]:
    """The pose arguments of `Rodent` against its (checked) `track` [(C,) T, 3]: None when neither is given, else the rows the device
    holds, float32 [(C,) T, nq - 3] = unit quaternion (normalised here, in float64) then joints.  ValueError for one without the other,
    a shape other than track.shape[:-1] + (4,) / + (nq - 7,), a zero or non-finite quaternion, a non-finite joint angle, and a negative
    or non-finite reward weight or scale."""
    for x in weights_and_scales:
        with np.errstate(over="ignore"):
            x32 = np.float32(x)
        if not (np.isfinite(x32) and x32 >= 0):
            raise ValueError(f"pose reward weights and scales must be finite and >= 0 (as float32), got {x!r}")
    if track_quat is None and track_joints is None:
        return None
    if track_quat is None or track_joints is None:
        raise ValueError("track_quat and track_joints go together: pass both (pose tracking) or neither")
    arr = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    quat, joints = arr(track_quat).astype(np.float64), arr(track_joints).astype(np.float64)
    lead = track.shape[:-1]
    if quat.shape != lead + (4,) or joints.shape != lead + (nq - 7,):
        raise ValueError(f"track_quat / track_joints must have shapes {lead + (4,)} / {lead + (nq - 7,)} next to a track_pos of shape "
                         f"{track.shape} (the same clips and frames), got {quat.shape} / {joints.shape}")
    norm = np.sqrt((quat * quat).sum(-1, keepdims=True))
    if not np.isfinite(norm).all() or (norm == 0).any():
        raise ValueError("track_quat holds a zero or non-finite quaternion")
    if not np.isfinite(joints).all():
        raise ValueError("track_joints holds a non-finite joint angle")
    return np.ascontiguousarray(np.concatenate([quat / norm, joints], axis=-1), dtype=np.float32)


def _quat_to_mat(q: np.ndarray) -> np.ndarray:
    """Rotation matrix [..., 3, 3] of a quaternion (w, x, y, z) [..., 4], MuJoCo's mju_quat2Mat, float64."""
    w, x, y, z = (q[..., i] for i in range(4))
    return np.stack([np.stack([w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z], -1)], -2)


def reference_obs(qpos, track_pos, track_quat, track_joints, frame, frames: int, clip=None, xquat=None, xmat=None, lengths=None) -> np.ndarray:
    """The reference blocks the step kernel appends to the observation (`Rodent(reference_obs_frames=H)`; C ABI
    `rr_batch_set_reference_obs`) restated in numpy float64: [..., frames * nq], block h = 1 .. frames = (p_h[3], q_h[4], j_h[nq - 7]).

    `qpos` [N, nq] the state the observation is formed from; `track_pos` [T, 3], `track_quat` [T, 4] (w, x, y, z), `track_joints`
    [T, nq - 7] -- with `clip` (int ids [N], clamped into [0, C)) [C, T, ...]; `frame` int [N]: the frame the observation's track entry
    counts from (the stepped `cur_frame` after a step, the start frame at reset).  With f_h = clamp(frame + h, 0, T - 1), x the world
    quaternion of body 1 and r_q, r_j the clip's row at f_h:

        p_h = xmat[1] @ (track_pos[f_h] - qpos[:3])
        q_h = s * (conj(x) (x) r_q),   s = -1 where that product's w is negative, else +1
        j_h = r_j - qpos[7:]

    Body 1 is the root body of the free joint, so x = qpos[3:7] and xmat[1] is its matrix; `xquat` [N, 4] / `xmat` [N, 3, 3] override
    them (e.g. with the values of a forward pass).  r_q and -r_q give the same block; frames past the clip's end repeat its last row.
    `lengths` (int [C], the env's `clip_lengths`): the clip's end is its own, f_h = clamp(frame + h, 0, L_c - 1), and no row at or behind
    L_c is read (`reference_rows`)."""
    qpos = np.asarray(qpos, dtype=np.float64)
    tp, tq, tj = (np.asarray(a, dtype=np.float64) for a in (track_pos, track_quat, track_joints))
    N, nq = qpos.shape
    frame = np.broadcast_to(np.asarray(frame, dtype=np.int64), (N,))
    if clip is not None:
        c = np.clip(np.broadcast_to(np.asarray(clip, dtype=np.int64), (N,)), 0, tp.shape[0] - 1)
    T = tp.shape[-2]
    x = qpos[:, 3:7] if xquat is None else np.asarray(xquat, dtype=np.float64)
    R = _quat_to_mat(x) if xmat is None else np.asarray(xmat, dtype=np.float64)
    xw, xx, xy, xz = (x[:, i] for i in range(4))
    out = np.empty((N, int(frames), nq))
    for h in range(1, int(frames) + 1):
        if lengths is None:
            f = np.clip(frame + h, 0, T - 1)
            row = (lambda a: a[f]) if clip is None else (lambda a: a[c, f])
        else:
            row = lambda a, fh=frame + h: reference_rows(a, fh, None if clip is None else c, lengths)
        out[:, h - 1, :3] = np.einsum("nij,nj->ni", R, row(tp) - qpos[:, :3])
        rw, rx, ry, rz = (row(tq)[:, i] for i in range(4))
        d = np.stack([xw * rw + xx * rx + xy * ry + xz * rz, xw * rx - xx * rw - xy * rz + xz * ry,
                      xw * ry + xx * rz - xy * rw - xz * rx, xw * rz - xx * ry + xy * rx - xz * rw], -1)
        out[:, h - 1, 3:7] = np.where(d[:, :1] < 0, -d, d)
        out[:, h - 1, 7:] = row(tj) - qpos[:, 7:]
    return out.reshape(N, int(frames) * nq)


def _check_reference_frames(frames, have_pose: bool) -> int:
    """`reference_obs_frames` of `Rodent` as an int in [0, 16]; ValueError for anything else, and for frames without the pose arguments."""
    if isinstance(frames, (bool, np.bool_)) or not isinstance(frames, (int, np.integer)):
        raise ValueError(f"reference_obs_frames must be an int in [0, 16], got {frames!r}")
    if not 0 <= int(frames) <= 16:
        raise ValueError(f"reference_obs_frames must lie in [0, 16], got {frames!r}")
    if int(frames) > 0 and not have_pose:
        raise ValueError("reference_obs_frames > 0 needs the reference pose: pass track_quat and track_joints")
    return int(frames)


def pose_errors(qpos, ref_pos, ref_quat, ref_joints):
    """The three errors pose termination compares (`Rodent(max_pos_error=..., max_quat_error=..., max_joint_error=...)`; C ABI
    `rr_batch_set_pose_termination`) restated in numpy float64.  `qpos` [..., nq] the stepped state; `ref_pos` [..., 3], `ref_quat`
    [..., 4] (w, x, y, z) and `ref_joints` [..., nq - 7] the clip's row at the clip and frame the step's rewards read (`cur_frame` before
    the step, clamped).  Returns (e_pos, e_quat, e_joint), float64 [...]:

        e_pos   = |qpos[:3] - ref_pos|_2
        e_quat  = theta of `pose_rewards` = 2 atan2(|d.xyz|, |d.w|), d = conj(ref_quat) (x) qpos[3:7]     (in [0, pi]; q and -q agree)
        e_joint = sqrt(sum((qpos[7:] - ref_joints)**2))"""
    qpos, rp, r, rj = (np.asarray(a, dtype=np.float64) for a in (qpos, ref_pos, ref_quat, ref_joints))
    q = qpos[..., 3:7]
    rw, rx, ry, rz = (r[..., i] for i in range(4))
    qw, qx, qy, qz = (q[..., i] for i in range(4))
    dw = rw * qw + rx * qx + ry * qy + rz * qz
    dx = rw * qx - rx * qw - ry * qz + rz * qy
    dy = rw * qy + rx * qz - ry * qw - rz * qx
    dz = rw * qz - rx * qy + ry * qx - rz * qw
    e_quat = 2.0 * np.arctan2(np.sqrt(dx * dx + dy * dy + dz * dz), np.abs(dw))
    return np.sqrt(((qpos[..., :3] - rp) ** 2).sum(-1)), e_quat, np.sqrt(((qpos[..., 7:] - rj) ** 2).sum(-1))


def pose_fail_code(errors, thresholds) -> np.ndarray:
    """The pose-termination code of `errors` = (e_pos, e_quat, e_joint) (`pose_errors`) against `thresholds` = (max_pos_error,
    max_quat_error, max_joint_error): int64 [...] = 1 (e_pos > max_pos) | 2 (e_quat > max_quat) | 4 (e_joint > max_joint).  A threshold
    of inf (or None) never fires; a NaN error sets no bit (`x > t` is false)."""
    code = 0
    with np.errstate(invalid="ignore"):
        for bit, e, t in zip((1, 2, 4), errors, thresholds):
            code = code + bit * (np.asarray(e, dtype=np.float64) > (np.inf if t is None else float(t))).astype(np.int64)
    return np.asarray(code, dtype=np.int64)


def _check_pose_termination(max_pos_error, max_quat_error, max_joint_error, have_pose: bool) -> Optional[tuple]:
    """The three thresholds of `Rodent` as floats (None -> inf), or None when all three are None or inf (no termination block).  ValueError
    for a value that is NaN or not > 0 as a float32 (what the kernel compares with), and for any finite value without the pose
    arguments."""
    out = []
    for name, x in (("max_pos_error", max_pos_error), ("max_quat_error", max_quat_error), ("max_joint_error", max_joint_error)):
        if x is None:
            out.append(math.inf)
            continue
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)):
            raise ValueError(f"{name} must be a number > 0 (or None: that criterion off), got {x!r}")
        with np.errstate(over="ignore", under="ignore"):
            x32 = np.float32(x)
        if not x32 > 0:       # NaN included
            raise ValueError(f"{name} must be > 0 as a float32 and not NaN (or None: that criterion off), got {x!r}")
        out.append(float(x32))
    if all(math.isinf(x) for x in out):
        return None
    if not have_pose:
        raise ValueError("max_pos_error / max_quat_error / max_joint_error need the reference pose: pass track_quat and track_joints")
    return tuple(out)


def body_rewards(xpos, ref_bodies, body_ids, end_effector_ids, weights=(1.0, 1.0), scales=(8.0, 100.0)):
    """The two body-position terms the step kernel adds to the reward of an env with body tracking (`Rodent(track_bodies=...)`; C ABI
    `rr_batch_set_body_tracking`) restated in numpy float64.  `xpos` [..., nbody, 3] the body positions of the step's last forward pass
    (`State.pipeline_state.xpos`), `ref_bodies` [..., nbody, 3] the clip's row at the clip and frame the step's rewards read (`cur_frame`
    before the step, clamped); `body_ids` / `end_effector_ids` the sets B and E of body ids (None or empty: that sum is 0).  Returns
    (body_reward, endeff_reward), float64 [...]:

        S_B = sum_{b in B} |xpos[b] - ref_bodies[b]|^2,   S_E the same over E
        body_reward = weights[0] * exp(-scales[0] * S_B),   endeff_reward = weights[1] * exp(-scales[1] * S_E)"""
    xpos, ref = np.asarray(xpos, dtype=np.float64), np.asarray(ref_bodies, dtype=np.float64)
    d2 = ((xpos - ref) ** 2).sum(-1)
    sums = [d2[..., np.asarray([] if ids is None else list(ids), dtype=np.int64)].sum(-1) for ids in (body_ids, end_effector_ids)]
    return weights[0] * np.exp(-scales[0] * sums[0]), weights[1] * np.exp(-scales[1] * sums[1])


def _check_body_tracking(track: np.ndarray, track_bodies, body_ids, end_effector_ids, nbody: int, weights_and_scales, have_pose: bool):
    """The body-tracking arguments of `Rodent` against its (checked) `track` [(C,) T, 3]: None when `track_bodies` is None, else
    (rows float32 [(C,) T, nbody, 3], masks float32 [2, nbody] -- row 0 the tracked bodies, row 1 the end effectors --, B, E as tuples).
    ValueError for ids without `track_bodies`, `track_bodies` without the pose arguments, a shape other than track.shape[:-1] +
    (nbody, 3), a non-finite entry, ids that are not unique ints in 1 .. nbody - 1, and a negative or non-finite weight or scale."""
    for x in weights_and_scales:
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)):
            raise ValueError(f"body reward weights and scales must be numbers, finite and >= 0, got {x!r}")
        with np.errstate(over="ignore"):
            x32 = np.float32(x)
        if not (np.isfinite(x32) and x32 >= 0):
            raise ValueError(f"body reward weights and scales must be finite and >= 0 (as float32), got {x!r}")
    if track_bodies is None:
        if body_ids is not None or end_effector_ids is not None:
            raise ValueError("body_ids / end_effector_ids need track_bodies (the clip's body positions)")
        return None
    if not have_pose:
        raise ValueError("track_bodies needs the reference pose: pass track_quat and track_joints")
    bodies = (track_bodies.detach().cpu().numpy() if torch.is_tensor(track_bodies) else np.asarray(track_bodies)).astype(np.float64)
    want = track.shape[:-1] + (nbody, 3)
    if bodies.shape != want:
        raise ValueError(f"track_bodies must have shape {want} next to a track_pos of shape {track.shape} (the same clips and frames, "
                         f"one global position per body), got {bodies.shape}")
    if not np.isfinite(bodies).all():
        raise ValueError("track_bodies holds a non-finite position")
    sets = []
    for name, ids in (("body_ids", body_ids), ("end_effector_ids", end_effector_ids)):
        if ids is None:
            sets.append(tuple(range(1, nbody)) if name == "body_ids" else ())
            continue
        ids = list(ids.tolist() if isinstance(ids, np.ndarray) else ids)
        for b in ids:
            if isinstance(b, (bool, np.bool_)) or not isinstance(b, (int, np.integer)) or not 1 <= int(b) <= nbody - 1:
                raise ValueError(f"{name} must be ints in 1 .. {nbody - 1} (body 0 is the world), got {b!r}")
        if len(set(int(b) for b in ids)) != len(ids):
            raise ValueError(f"{name} must be unique, got {ids!r}")
        sets.append(tuple(int(b) for b in ids))
    masks = np.zeros((2, nbody), dtype=np.float32)
    for row, ids in enumerate(sets):
        masks[row, list(ids)] = 1.0
    return np.ascontiguousarray(bodies, dtype=np.float32), masks, sets[0], sets[1]


def velocity_rewards(qvel, ref_vel, weights=(1.0, 1.0, 1.0), scales=(10.0, 0.1, 0.01)):
    """The three velocity terms the step kernel adds to the reward of an env with velocity tracking (`Rodent(track_velocity=...)`; C ABI
    `rr_batch_set_velocity_tracking`) restated in numpy float64.  `qvel` [..., nv] the stepped state, `ref_vel` [..., nv] the clip's row
    in qvel layout at the clip and frame the step's rewards read (`cur_frame` before the step, clamped); `weights` = (lin, ang, joint)
    reward weights, `scales` likewise.  With d = qvel - ref_vel:

        S_lin = sum d[0:3]**2,   S_ang = sum d[3:6]**2,   S_joint = sum d[6:]**2
        lin_vel_reward = weights[0] * exp(-scales[0] * S_lin),  ang_vel_reward and joint_vel_reward likewise

    Returns (lin_vel_reward, ang_vel_reward, joint_vel_reward), float64 [...]."""
    d2 = (np.asarray(qvel, dtype=np.float64) - np.asarray(ref_vel, dtype=np.float64)) ** 2
    sums = (d2[..., :3].sum(-1), d2[..., 3:6].sum(-1), d2[..., 6:].sum(-1))
    return tuple(w * np.exp(-k * s) for w, k, s in zip(weights, scales, sums))


def _check_velocity_tracking(track: np.ndarray, track_velocity, track_angular_velocity, track_joint_velocity, nv: int, weights_and_scales,
                             have_pose: bool) -> Optional[np.ndarray]:
    """The velocity-tracking arguments of `Rodent` against its (checked) `track` [(C,) T, 3]: None when none of the three arrays is given,
    else the rows the device holds, float32 [(C,) T, nv] in qvel layout = [velocity | angular_velocity | joints_velocity].  ValueError for
    some of the three without the others, the arrays without the pose arguments, a shape other than track.shape[:-1] + (3,) / + (3,) /
    + (nv - 6,), a non-finite entry, and a negative or non-finite weight or scale."""
    for x in weights_and_scales:
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)):
            raise ValueError(f"velocity reward weights and scales must be numbers, finite and >= 0, got {x!r}")
        with np.errstate(over="ignore"):
            x32 = np.float32(x)
        if not (np.isfinite(x32) and x32 >= 0):
            raise ValueError(f"velocity reward weights and scales must be finite and >= 0 (as float32), got {x!r}")
    given = [a is not None for a in (track_velocity, track_angular_velocity, track_joint_velocity)]
    if not any(given):
        return None
    if not all(given):
        raise ValueError("track_velocity, track_angular_velocity and track_joint_velocity go together: pass all three (velocity tracking) or none")
    if not have_pose:
        raise ValueError("track_velocity / track_angular_velocity / track_joint_velocity need the reference pose: pass track_quat and track_joints")
    arr = lambda a: (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).astype(np.float64)
    lin, ang, joint = arr(track_velocity), arr(track_angular_velocity), arr(track_joint_velocity)
    lead = track.shape[:-1]
    if lin.shape != lead + (3,) or ang.shape != lead + (3,) or joint.shape != lead + (nv - 6,):
        raise ValueError(f"track_velocity / track_angular_velocity / track_joint_velocity must have shapes {lead + (3,)} / {lead + (3,)} / "
                         f"{lead + (nv - 6,)} next to a track_pos of shape {track.shape} (the same clips and frames), got {lin.shape} / "
                         f"{ang.shape} / {joint.shape}")
    rows = np.concatenate([lin, ang, joint], axis=-1)
    if not np.isfinite(rows).all():
        raise ValueError("track_velocity / track_angular_velocity / track_joint_velocity hold a non-finite entry")
    with np.errstate(over="ignore"):
        rows32 = np.ascontiguousarray(rows, dtype=np.float32)
    if not np.isfinite(rows32).all():
        raise ValueError("track_velocity / track_angular_velocity / track_joint_velocity hold an entry that is not finite as a float32")
    return rows32


class _StepOption(NamedTuple):
    """One option of the env step as `Rodent` hands it to its batch and reads it back: the output buffer a step launch gets under the
    env-io key `key` (float32 [N] + `shape`), the `static` env-io entries that go with it (the option's tensors and scalar tuples), the
    `metrics` it adds to `State.metrics`, and `read`: buffer -> those metrics, in that order."""
    key: str
    shape: tuple
    static: dict
    metrics: tuple
    read: Callable


_columns = lambda buf: tuple(buf[:, j] for j in range(buf.shape[1]))      # the columns of an [N, 2] or [N, 3] metrics buffer, as views


def _code_bits(buf):
    """The pose-termination code of the (last) step, 0 .. 7 as a float [N], split: (any, bit 0, bit 1, bit 2) as floats 0 / 1."""
    code = buf.to(torch.int32)
    return (code != 0).float(), (code & 1).float(), ((code >> 1) & 1).float(), ((code >> 2) & 1).float()


class Rodent(PipelineEnv):

    def __init__(
        self,
        track_pos,
        forward_reward_weight=10,
        ctrl_cost_weight=0.1,
        healthy_reward=1.0,
        terminate_when_unhealthy=True,
        healthy_z_range=(0.03, 0.5),
        reset_noise_scale=1e-2,
        solver="cg",
        iterations: int = 6,
        ls_iterations: int = 6,
        vision=False,
        num_envs: int = 1,
        xml_path: str = _XML_PATH,
        device=None,
        bad_state_max: Optional[float] = None,
        track_quat=None,
        track_joints=None,
        quat_reward_weight: float = 1.0,
        quat_reward_scale: float = 2.0,
        joint_reward_weight: float = 1.0,
        joint_reward_scale: float = 0.5,
        reset_to_reference: bool = False,
        reference_obs_frames: int = 0,
        max_pos_error: Optional[float] = None,
        max_quat_error: Optional[float] = None,
        max_joint_error: Optional[float] = None,
        track_bodies=None,
        body_ids=None,
        end_effector_ids=None,
        body_reward_weight: float = 1.0,
        body_reward_scale: float = 8.0,
        endeff_reward_weight: float = 1.0,
        endeff_reward_scale: float = 100.0,
        clip_restarts: int = 0,
        restart_frame_range=None,
        end_at_clip_end: bool = False,
        track_velocity=None,
        track_angular_velocity=None,
        track_joint_velocity=None,
        lin_vel_reward_weight: float = 1.0,
        lin_vel_reward_scale: float = 10.0,
        ang_vel_reward_weight: float = 1.0,
        ang_vel_reward_scale: float = 0.1,
        joint_vel_reward_weight: float = 1.0,
        joint_vel_reward_scale: float = 0.01,
        clip_lengths=None,
        restart_across_clips: bool = False,
        restart_sampling: Optional[str] = None,
        clip_outcomes: bool = False,
        restart_sampling_seed: int = 0,
        restart_from_reference: bool = False,
        restart_noise_seed: int = 0,
        **kwargs,
    ):
        """`track_pos`: the reference positions to track, float [T, 3] -- one clip, followed by every env -- or [C, T, 3], C >= 1 clips of
        equal length (what `preprocessing.load_reference_clip` returns for a list of clip names).  With the clip axis each env follows ONE
        clip, drawn at `reset` (or given there) and kept in `info['clip']`: its reward reads `track_pos[clip, cur_frame]`, its observation
        `track_pos[clip, cur_frame + 1]`, frames clamped within the clip.  Any other rank raises ValueError.  `num_clips` is C, or 1.

        `bad_state_max` (None = off, the default): the bad-state check of MuJoCo (`mj_checkPos` / `mj_checkVel`, there with
        mjMAXVAL = 1e10).  After an env step an env is bad when some element x of its qpos or qvel fails |x| <= bad_state_max (NaN and
        +-inf included); that step then has done = 1 (whatever `terminate_when_unhealthy` is), reward 0 and metrics 0, and is counted
        (`bad_states()`).  Under `AutoResetWrapper` -- composed or in the one-launch rollouts -- the first state comes back as for any
        finished episode, with no bootstrap from the bad step.  The bare `step` does NOT sanitise: it returns the bad state and its
        observation as they are, flagged by `done`; so does the raw evaluation form (`unroll_eval` without `episode_length`).

        Pose tracking: `track_quat` [T, 4] (w, x, y, z) and `track_joints` [T, nq - 7] -- with a [C, T, 3] track_pos [C, T, 4] and
        [C, T, nq - 7] -- are the clip's root orientation and joint angles (`preprocessing.ReferenceClip.quaternion` / `.joints`); both or
        neither.  Quaternions are normalised here; a zero or non-finite one raises ValueError.  With them every env step (never a reset)
        adds two terms to the reward, formed in the step kernel at the clip and frame the position reward reads (`pose_rewards` is their
        float64 restatement):

            quat_reward  = quat_reward_weight  * exp(-quat_reward_scale  * theta**2),  theta the angle between qpos[3:7] and the clip's
            joint_reward = joint_reward_weight * exp(-joint_reward_scale * sum((qpos[7:] - joints)**2))
            reward       = (reward without pose + quat_reward) + joint_reward

        and `State.metrics` gains `quat_reward` and `joint_reward` (zeros at reset and after a bad step).  done, cur_frame, the
        observation and the other metrics are what they are without pose (`reference_obs_frames` below adds the reference pose to the
        observation).  The four
        defaults (1, 2, 1, 0.5) are UNTUNED choices, not values from a reference.  Served by the CG solver on the floor-contact models
        in `step`, `unroll_wrapped` and `unroll_policy_wrapped`; a model or solver without a pose instance raises RuntimeError here with
        the library's reason, `randomize` / `set_env_params` raise on a pose env, and `eval_supported()` is False (evaluation runs the
        per-step loop).  `reset_to_reference=True` (pose envs only): reset starts from the clip's pose, qpos[3:] = reference[clip,
        start_frame] + noise instead of qpos0[3:] + noise; the random draws are the same.

        `reference_obs_frames` = H (pose envs only, an int in [0, 16]; 0, the default, is the observation above in every bit): the
        observation carries what the pose reward scores.  Every row -- at reset and after every step, in `step`, `unroll_wrapped` and
        `unroll_policy_wrapped` -- becomes [the observation above | block_1 | ... | block_H], `observation_size` = obs_dim + H * nq, with
        block_h = (p_h[3], q_h[4], j_h[nq - 7]) read at frame clamp(cur_frame + h) of the env's clip: the next track positions in the root
        frame (p_1 is the observation's own last three entries), the reference orientations relative to the root's with w >= 0, and the
        reference joint angles minus the current ones (`reference_obs` restates them in float64).  AutoReset restores the stored first
        observation at the full width.  The one-launch rollout with the actor inside serves rows up to 1664 wide (H <= 5 on the shipped
        floor-contact models); above that `ppo.train` collects per step.

        Pose termination: `max_pos_error` (metres), `max_quat_error` (radians), `max_joint_error` (radians, the 2-norm over the joints)
        -- pose envs only; None, the default, or inf: that criterion off; each > 0 and not NaN.  With any of them finite an env step
        (never a reset) whose stepped pose has strayed from the clip's row -- the row its rewards read -- ends the episode:
        `pose_errors` gives (e_pos, e_quat, e_joint), `pose_fail_code` the code 1 (e_pos > max_pos_error) | 2 (e_quat > max_quat_error)
        | 4 (e_joint > max_joint_error), and done = max(done, code != 0), whatever `terminate_when_unhealthy` is.  Nothing else of the
        step changes.  It is a termination, not a truncation: under AutoReset -- composed or in the one-launch rollouts -- the first
        state comes back, discount 0.  `State.metrics` gains `pose_fail`, `pose_fail_pos`, `pose_fail_quat`, `pose_fail_joint` (0 / 1;
        zeros at reset and after a bad step), so an evaluation reports `eval/episode_pose_fail`, the share of episodes ended by the
        clip.  The thresholds have no defaults: they depend on the clips and on how far training has come.

        Body tracking: `track_bodies` [T, nbody, 3] -- with a [C, T, 3] track_pos [C, T, nbody, 3] -- are the clip's global body positions
        (`preprocessing.ReferenceClip.body_positions`); pose envs only, every entry finite.  `body_ids` is the set B of tracked bodies
        (None: bodies 1 .. nbody - 1), `end_effector_ids` the set E of end effectors (None: no such term); unique ints in 1 .. nbody - 1.
        A joint-angle reward lets errors add up along a limb; these two terms score where the bodies ARE.  Every env step (never a
        reset) adds, at the clip and frame the other rewards read (`body_rewards` is the float64 restatement):

            body_reward   = body_reward_weight   * exp(-body_reward_scale   * sum_{b in B} |xpos[b] - track_bodies[b]|**2)
            endeff_reward = endeff_reward_weight * exp(-endeff_reward_scale * sum_{b in E} |xpos[b] - track_bodies[b]|**2)
            reward        = (reward with the pose terms + body_reward) + endeff_reward

        with xpos the body positions of the step's last forward pass -- `State.pipeline_state.xpos` with `pipeline_outputs=True`, MJX's
        `data.xpos` after `step`: the pose before the last substep's integration, one substep behind qpos.  `State.metrics` gains
        `body_reward` and `endeff_reward` (zeros at reset and after a bad step); everything else of the step is what it is without the
        terms.  An empty set gives its term weight 0.  The four defaults (1, 8, 1, 100) are UNTUNED choices, not values from a reference.
        Served where pose tracking is, in `step`, `unroll_wrapped` and `unroll_policy_wrapped`, with or without reference frames and
        pose termination.

        Clip restarts: `clip_restarts` = K (pose envs only, an int in 0 .. 64; 0, the default, is today's behaviour in every bit).  Upstream's
        AutoReset brings back the first state and leaves `cur_frame` alone, so a restarted tracking env is compared with frames it never
        started at.  With K >= 1 `reset` builds a bank of K start states per env -- entry 0 the reset state itself, entry k = 1 .. K - 1
        what `reset_draws` gives for `fold_in(key, k)` with its start frame drawn in `restart_frame_range` = (lo, hi) (None: (0, 100), the
        reference's range); all on the env's one clip (`restart_bank_draws`) -- and keeps it in `info['restart_bank']` (dict:
        `pipeline_state` [K, N, ...], `obs` [K, N, observation_size], `frame` int32 [K, N]) next to `info['restart_slot']` (int32 [N],
        zeros at reset).  Bank and slot are info: never re-drawn, never restored.  Per wrapped env step (`wrappers.wrap`,
        `unroll_wrapped`, `unroll_policy_wrapped`), with new_frame = old_frame + 1 and T the clip length:

            over = steps' >= episode_length  or  (end_at_clip_end and new_frame >= T - 1);   done, truncation as ever
            done:  slot' = (slot + 1) mod K;  state, obs <- bank[slot'];  cur_frame <- bank frame[slot'];    else slot, new_frame

        The clip's end (`end_at_clip_end=True`, needs K >= 1) is a truncation like `episode_length`, so the value bootstraps; the step
        that ends the episode is untouched.  K = 1 restores the frame with the state.  The bare `step` and the raw evaluation rollout have
        no wrappers and do not change.

        Velocity tracking: `track_velocity` [T, 3], `track_angular_velocity` [T, 3] and `track_joint_velocity` [T, nv - 6] -- with a
        [C, T, 3] track_pos each gains the clip axis -- are the clip's velocities (`preprocessing.ReferenceClip.velocity`,
        `.angular_velocity`, `.joints_velocity`); all three or none, pose envs only, every entry finite.  They are kept as one device
        array `track_vel` [(C,) T, nv] whose rows are in `qvel` layout, [velocity | angular_velocity | joints_velocity].  The frames
        agree: qvel[0:3] is the world-frame linear velocity of the free joint and qvel[3:6] its angular velocity in the root's OWN frame,
        and `preprocessing.compute_velocity_from_kinematics` forms the clip's angular velocity as the axis-angle of conj(q_t) q_{t+1}
        over dt, which is that same frame -- so the rows are compared with qvel as they are.  A pose reward alone pays a policy that holds
        the right pose at the wrong speed, or jitters around it, in full; these three terms score the speed.  Every env step (never a
        reset) adds, at the clip and frame the other rewards read and with d = qvel - row on the stepped qvel (`velocity_rewards` is the
        float64 restatement):

            lin_vel_reward   = lin_vel_reward_weight   * exp(-lin_vel_reward_scale   * sum(d[0:3]**2))
            ang_vel_reward   = ang_vel_reward_weight   * exp(-ang_vel_reward_scale   * sum(d[3:6]**2))
            joint_vel_reward = joint_vel_reward_weight * exp(-joint_vel_reward_scale * sum(d[6:]**2))
            reward           = ((reward with the pose and body terms + lin_vel_reward) + ang_vel_reward) + joint_vel_reward

        `State.metrics` gains `lin_vel_reward`, `ang_vel_reward` and `joint_vel_reward`, after the body metrics (zeros at reset and after
        a bad step); physics, done, the observation, cur_frame and the other metrics are what they are without the terms.  A weight of 0
        switches its term off.  The six defaults (1, 10, 1, 0.1, 1, 0.01) are UNTUNED choices, not values from a reference.  Served where
        body tracking is, in `step`, `unroll_wrapped` and `unroll_policy_wrapped`, with or without the other options.  With the arrays
        given, `reset_to_reference=True` also starts the episode MOVING: qvel = track_vel[clip, start_frame] + noise instead of the bare
        noise (`reset_qvel`), in the reset state and in every entry of the clip-restart bank; the random draws are the same.  Without the
        arrays, or with `reset_to_reference=False`, `reset` is what it is without them in every bit.

        Clip library (pose envs only; both off by default, and off is today's path in every bit and every key).  `clip_lengths`: int
        [C] next to a [C, T, 3] track (an int or [1] next to a [T, 3] one), 2 <= L_c <= T: clip c consists of rows 0 .. L_c - 1 of every
        clip array, and the rows behind them are padding that nothing reads -- no launch, not `reset_qpos` / `reset_qvel`
        (`preprocessing.load_reference_clips` pads unequal clips and returns the lengths).  Wherever an env on clip c clamps a frame into
        [0, T - 1] it clamps into [0, L_c - 1] instead -- the position reward's row, the observation's track entry, the reference blocks,
        the pose reward and pose-termination row, the body rows, the velocity rows -- and `end_at_clip_end` becomes new_frame >=
        L_c - 1.  Start frames fold into the clip: start = draw mod (L_c - 1) for the reset state and for every bank entry
        (`fold_start_frames`; the identity where draw < L_c - 1), so the clip-length refusal of `end_at_clip_end` does not apply.  The
        float64 restatements take their rows from `reference_rows(..., lengths=)`; `reference_obs` has a `lengths` argument.
        `restart_across_clips=True` (needs `clip_restarts` >= 1 and a clip axis): bank entry k >= 1 takes the clip that
        `reset_draws(fold_in(key, k), num_clips=C)` returns (`restart_bank_draws(across_clips=True)`; no other draw moves), entry 0 the
        reset's clip; `reset(rng, clip=ids)` takes [N] (entry 0, the others drawn) or [K, N].  Each entry's start state is formed on its
        own clip, `info['restart_bank']` gains `clip` (int32 [K, N]), and the rule above gains one line,

            done:  clip <- bank clip[slot']

        so `info['clip']` changes at a restore in the wrapped forms (a fresh tensor; the input state's is left alone).  The bare `step`
        does not change the clip.

        Clip sampling (both off by default, and off is today's path in every bit and every key; integers only, so the composed
        wrappers, the fused per-step wrapper and both one-launch rollouts agree bit for bit).  `clip_outcomes=True` (needs
        `clip_restarts` >= 1 and a clip axis): the wrapped forms count, per clip the step was made on, the wrapped steps (col 4), the
        ended episodes (col 0) and why each ended -- pose failure (col 1), else the env's own done: unhealthy or a bad state (col 2),
        else a truncation by `episode_length` or the clip's end (col 3) -- in an int64 [C, 5] device table that `clip_outcomes()` reads
        (`clip_outcome_update` restates a step).  `restart_sampling="weighted"` (needs `restart_across_clips=True`): a restore draws its
        bank entry instead of taking the next one, with probability proportional to the weight of the entry's clip,

            q_k = clip_weights()[bank clip[k]];  S = sum q_k;  h = restart_hash(restart_sampling_seed, env, n);  r = (h * S) >> 32
            done:  slot' = the smallest k with q_0 + .. + q_k > r        (`weighted_slot`; S == 0: the cyclic rule)

        n = `info['restart_draws']` (int32 [N], zeros at `reset`), the env's restore count, which grows by one at every restore.  The
        weights start uniform (all 65535) and are set with `set_clip_weights` -- in place, so later launches and replayed graphs see
        them; a clip of weight 0 is never drawn while another entry of the env's bank has a positive one.

        Reference restarts (`restart_from_reference=True`; off by default, and off is today's path in every bit and every key; needs
        `reset_to_reference=True` and `clip_restarts` >= 1, K = 1 suffices).  A restore of the wrapped forms takes NO bank entry: it
        draws a clip and a start frame, builds the start state from the clip's rows plus noise and forms the observation the reset
        launch gives for that state -- inside the one-launch rollouts, by a forward-only pass of the step kernel that is not counted as
        a step; in the per-step wrappers by a reset launch and a select.  So the start states of a run are not the K per env that
        `reset` drew, but any frame of any clip.  With n = `info['restart_draws']` (now present whatever the sampling; it grows by one
        per restore) every draw is an integer hash of (`restart_noise_seed`, env, n, purpose, element) (`reference_restart_hash`):

            clip:   with `restart_across_clips`, over all C clips -- by `clip_weights()` when `restart_sampling="weighted"` (a clip of
                    weight 0 is never drawn), else uniformly; otherwise the env stays on its clip       (`reference_restart_draws`)
            frame:  lo + ((h * (hi - lo)) >> 32) in `restart_frame_range`, folded into the clip like every start frame
            state:  qpos = [track_pos, pose][clip, frame], qvel = track_vel[clip, frame] (0 without the velocity arrays), each element
                    plus reset_noise_scale * ((h_i >> 8) * 2**-23 - 1); act and warm start 0                (`reference_restart_state`)

        `info['cur_frame']` and `info['clip']` move to the draw; `reset`, the bank it builds (entry 0 still is the reset state) and
        `info['restart_slot']` (which advances cyclically and selects nothing) stay, as do the outcome counters, `end_at_clip_end`, pose
        termination, the bad-state check and truncation.  `restart_sampling_seed` is not used by these restores."""
        given = locals()                  # the arguments as they came (first statement: nothing else is a local yet): `_ctor` below
        if bad_state_max is not None:
            with np.errstate(over="ignore", under="ignore"):
                thr32 = np.float32(bad_state_max)        # what the kernel gets: 1e-50 would arrive as 0 (= off), 1e39 as inf
            if not (np.isfinite(thr32) and thr32 > 0):
                raise ValueError(f"bad_state_max must be finite and > 0 as a float32 (or None: no check), got {bad_state_max!r}")
        track_np = _check_track(track_pos)
        if solver.lower() not in ("cg", "newton"):       # [REF Rodent_Env_Brax.py:42-45]
            raise ValueError(f"solver must be 'cg' or 'newton', got {solver!r}")
        if vision:
            raise NotImplementedError("vision observations are not part of the reference obs either")
        if iterations < 2:
            # measured on the float64 oracle as on the GPU: with ONE solver iteration per substep the rollout under
            # random actions reaches |qvel| > 1e4 and non-finite states within two env steps (Newton 1/4), within a few (CG 1/4)
            warnings.warn(f"Rodent(solver={solver!r}, iterations={iterations}): a single solver iteration per substep diverges "
                          "under random actions (non-finite states within a few env steps, on the CPU oracle too); use iterations >= 2",
                          RuntimeWarning, stacklevel=2)
        sys = System(assets.resolve_model(xml_path), iterations, ls_iterations, solver)
        pose_np = _check_pose(track_np, track_quat, track_joints, sys.nq, (quat_reward_weight, quat_reward_scale, joint_reward_weight, joint_reward_scale))
        ref_frames = _check_reference_frames(reference_obs_frames, pose_np is not None)
        pose_term = _check_pose_termination(max_pos_error, max_quat_error, max_joint_error, pose_np is not None)
        body_np = _check_body_tracking(track_np, track_bodies, body_ids, end_effector_ids, sys.nbody,
                                       (body_reward_weight, body_reward_scale, endeff_reward_weight, endeff_reward_scale), pose_np is not None)
        restarts = _check_clip_restarts(clip_restarts, restart_frame_range, end_at_clip_end, pose_np is not None, track_np.shape[-2], clip_lengths is not None)
        lengths_np, across = _check_clip_library(clip_lengths, restart_across_clips, track_np, pose_np is not None, restarts[0])
        weighted, counting, sample_seed = _check_clip_sampling(restart_sampling, clip_outcomes, restart_sampling_seed, across, restarts[0],
                                                               track_np.shape[0] if track_np.ndim == 3 else None)
        ref_restart, noise_seed = _check_reference_restart(restart_from_reference, restart_noise_seed, bool(reset_to_reference), restarts[0], pose_np is not None,
                                                           track_np.shape[0] if track_np.ndim == 3 else None)
        vel_np = _check_velocity_tracking(track_np, track_velocity, track_angular_velocity, track_joint_velocity, sys.nv,
                                          (lin_vel_reward_weight, lin_vel_reward_scale, ang_vel_reward_weight, ang_vel_reward_scale,
                                           joint_vel_reward_weight, joint_vel_reward_scale), pose_np is not None)
        if reset_to_reference and pose_np is None:
            raise ValueError("reset_to_reference=True needs the reference pose: pass track_quat and track_joints")
        physics_steps_per_control_step = 10   # [REF Rodent_Env_Brax.py:53-57]
        kwargs["n_frames"] = kwargs.get("n_frames", physics_steps_per_control_step)
        kwargs["backend"] = "hip"
        super().__init__(sys, num_envs=num_envs, device=device, **kwargs)
        self._track_pos = torch.from_numpy(track_np).to(self.device).contiguous()
        self._track_host = track_np
        self._num_clips = track_np.shape[0] if track_np.ndim == 3 else None      # None: no clip axis (the single-clip path, no ids anywhere)
        self._pose_host = pose_np                            # None: no pose tracking (the position-only reward, no pose members anywhere)
        self._track_pose = None if pose_np is None else torch.from_numpy(pose_np).to(self.device).contiguous()
        self._quat_reward = (float(quat_reward_weight), float(quat_reward_scale))
        self._joint_reward = (float(joint_reward_weight), float(joint_reward_scale))
        self._reset_to_reference = bool(reset_to_reference)
        self._ref_frames = ref_frames
        self._pose_term = pose_term       # None: no pose termination (no such members anywhere, the launches run the instances they ran)
        self._clip_restarts, self._restart_frame_range, self._end_at_clip_end = restarts
        self._lengths_host = lengths_np       # None: every clip has T frames (no such members anywhere)
        self._clip_lengths = None if lengths_np is None else torch.from_numpy(lengths_np).to(self.device).contiguous()
        self._across_clips = across
        self._ref_restart, self._noise_seed = ref_restart, noise_seed
        # clip sampling: None without either option (no such members anywhere); the two tables live for the env's life and are rewritten
        # in place, so a captured launch keeps reading them
        self._sampling = None
        if weighted or counting:
            C_ = track_np.shape[0]
            self._sampling = dict(weights=torch.full((C_,), MAX_CLIP_WEIGHT, dtype=torch.int32, device=self.device) if weighted else None,
                                  outcomes=torch.zeros(C_, 5, dtype=torch.int64, device=self.device) if counting else None, seed=sample_seed)
        batch = self._batch

        def reference_frames_supported():
            # the batch carries the count; its rows come from the pose block, which therefore stands from here on (every launch of this
            # env, resets included, hands the block: a reset writes no pose metrics and gets a buffer nobody reads)
            why = batch.reference_obs_supported(ref_frames)
            if why is None:
                self._reset_pose_metrics = torch.zeros(num_envs, 2, device=self.device)
                batch.set_pose(self._track_pose, self._reset_pose_metrics, self._quat_reward, self._joint_reward)
                batch.set_reference_obs(ref_frames)
            return why
        probes = ((pose_np is not None, "track_quat=..., track_joints=...", batch.pose_supported),
                  (ref_frames > 0, f"reference_obs_frames={ref_frames}", reference_frames_supported),
                  (pose_term is not None, "max_pos_error / max_quat_error / max_joint_error", batch.pose_termination_supported),
                  (body_np is not None, "track_bodies=...", batch.body_tracking_supported),
                  (vel_np is not None, "track_velocity=...", batch.velocity_tracking_supported),
                  (self._clip_restarts > 0, f"clip_restarts={self._clip_restarts}", batch.clip_restarts_supported),
                  (lengths_np is not None or across, "clip_lengths=... / restart_across_clips=True", batch.clip_library_supported),
                  (weighted or counting, "restart_sampling=... / clip_outcomes=True", batch.clip_sampling_supported),
                  (ref_restart, "restart_from_reference=True", batch.reference_restart_supported))
        for wanted, label, query in probes:       # a model, solver or frame count without the option's instance: the library's reason
            why = query() if wanted else None
            if why is not None:
                raise RuntimeError(f"Rodent({label}): {why}")
        self._body = None                 # None: no body tracking (no such members anywhere, the launches run the instances they ran)
        if body_np is not None:
            rows, masks, B, E = body_np
            # an empty set gives its term weight 0 here, so the term is 0 whatever its (empty) sum
            self._body = dict(track_bodies=torch.from_numpy(rows).to(self.device).contiguous(), body_weights=torch.from_numpy(masks).to(self.device).contiguous(),
                              body_reward=(float(body_reward_weight) if B else 0.0, float(body_reward_scale)),
                              endeff_reward=(float(endeff_reward_weight) if E else 0.0, float(endeff_reward_scale)), body_ids=B, end_effector_ids=E)
        self._vel_host = vel_np           # None: no velocity tracking (no such members anywhere; reset starts at rest)
        self._track_vel = None if vel_np is None else torch.from_numpy(vel_np).to(self.device).contiguous()
        self._vel = None if vel_np is None else dict(lin_vel_reward=(float(lin_vel_reward_weight), float(lin_vel_reward_scale)),
                                                     ang_vel_reward=(float(ang_vel_reward_weight), float(ang_vel_reward_scale)),
                                                     joint_vel_reward=(float(joint_vel_reward_weight), float(joint_vel_reward_scale)))
        # the step options in force, in the order their metrics follow the three old ones; a reset hands none of them (it has no reward
        # and no done to raise) -- but see `_env_io` for an env with reference frames
        self._options = tuple(o for o in (
            pose_np is not None and _StepOption("pose_metrics", (2,), dict(track_pose=self._track_pose, quat_reward=self._quat_reward, joint_reward=self._joint_reward),
                                                ("quat_reward", "joint_reward"), _columns),
            pose_term is not None and _StepOption("pose_fail", (), dict(pose_termination=pose_term),
                                                  ("pose_fail", "pose_fail_pos", "pose_fail_quat", "pose_fail_joint"), _code_bits),
            body_np is not None and _StepOption("body_metrics", (2,), {k: self._body[k] for k in ("track_bodies", "body_weights", "body_reward", "endeff_reward")},
                                                ("body_reward", "endeff_reward"), _columns),
            vel_np is not None and _StepOption("vel_metrics", (3,), dict(track_vel=self._track_vel, lin_vel_reward=self._vel["lin_vel_reward"],
                                                                       ang_vel_reward=self._vel["ang_vel_reward"], joint_vel_reward=self._vel["joint_vel_reward"]),
                                               ("lin_vel_reward", "ang_vel_reward", "joint_vel_reward"), _columns)) if o)
        self._forward_reward_weight = forward_reward_weight
        self._ctrl_cost_weight = ctrl_cost_weight
        self._healthy_reward = healthy_reward
        self._terminate_when_unhealthy = terminate_when_unhealthy
        self._healthy_z_range = healthy_z_range
        self._reset_noise_scale = reset_noise_scale
        self._vision = vision
        self._bad_state_max = None if bad_state_max is None else float(bad_state_max)
        # what `with_num_envs` rebuilds a sibling from: every parameter of this constructor as it was given, and the keywords PipelineEnv takes
        self._ctor = {name: given[name] for name in _CTOR_PARAMS}
        self._ctor.update(n_frames=kwargs["n_frames"], pipeline_outputs=kwargs.get("pipeline_outputs", False),
                          contact_outputs=kwargs.get("contact_outputs", False), balance=kwargs.get("balance"),
                          rebalance_every=kwargs.get("rebalance_every", 4))

    def with_num_envs(self, num_envs: int, device=None):
        """A sibling env with another batch size (ppo.train builds its per-rank and eval envs this way)."""
        return Rodent(num_envs=num_envs, device=device or self.device, **self._ctor)

    @property
    def num_clips(self) -> int:
        """Clips in `track_pos`: C of a [C, T, 3] track, 1 for a [T, 3] one."""
        return 1 if self._num_clips is None else self._num_clips

    def contact_overflow(self) -> int:
        """(env, env step) events so far in which more sphere / capsule pairs were in penetration than the kernel's 64 contact slots;
        the surplus pairs were DROPPED for that substep (models with candidate-pair contacts, e.g. rodent_cpu.xml; always 0 for the
        floor-contact models).  Reads a device counter: synchronises the env's stream."""
        return self._batch.contact_overflow()

    @property
    def bad_state_max(self) -> Optional[float]:
        """The threshold of the bad-state check, None when it is off."""
        return self._bad_state_max

    def bad_states(self) -> int:
        """(env, env step) events so far in which the bad-state check ended an episode (`bad_state_max`; always 0 while it is off).  A
        multi-step launch counts each of its steps.  Reads a device counter: synchronises the env's stream."""
        return self._batch.bad_states()

    @property
    def pose_tracking(self) -> bool:
        """Whether the reward has the two pose terms (`track_quat` / `track_joints` were given)."""
        return self._pose_host is not None

    @property
    def pose_termination(self) -> Optional[tuple]:
        """(max_pos_error, max_quat_error, max_joint_error) as the kernel compares them, inf = off; None without pose termination."""
        return self._pose_term

    @property
    def body_tracking(self) -> Optional[dict]:
        """None without body tracking, else dict(body_ids, end_effector_ids, body_reward=(weight, scale), endeff_reward=(weight, scale))
        as the kernel uses them (an empty set has weight 0)."""
        if self._body is None:
            return None
        return {k: self._body[k] for k in ("body_ids", "end_effector_ids", "body_reward", "endeff_reward")}

    @property
    def velocity_tracking(self) -> Optional[dict]:
        """None without velocity tracking, else dict(lin_vel_reward=(weight, scale), ang_vel_reward=(weight, scale),
        joint_vel_reward=(weight, scale)) as the kernel uses them."""
        return None if self._vel is None else dict(self._vel)

    @property
    def clip_restarts(self) -> int:
        """Entries K of the start bank a restarted episode draws from (0: no bank, the first state comes back and the frame does not)."""
        return self._clip_restarts

    @property
    def end_at_clip_end(self) -> bool:
        """Whether the wrapped env truncates an episode whose next observation would read past the clip's last frame."""
        return self._end_at_clip_end

    @property
    def restart_frame_range(self) -> tuple:
        """(lo, hi): bank entries 1 .. K - 1 start at frames drawn in [lo, hi)."""
        return self._restart_frame_range

    @property
    def clip_lengths(self) -> Optional[torch.Tensor]:
        """Frames of each clip, int32 [C] on the env's device (None: every clip has `track_len` frames)."""
        return self._clip_lengths

    @property
    def restart_across_clips(self) -> bool:
        """Whether the entries of the start bank have clips of their own, so that a restore may move the env to another clip."""
        return self._across_clips

    @property
    def restart_from_reference(self) -> bool:
        """Whether a restore of the wrapped forms starts from a freshly drawn clip frame instead of a bank entry."""
        return self._ref_restart

    def reference_restart(self, clip: Optional[torch.Tensor], draws: torch.Tensor):
        """The reference restart of EVERY env at restore counts `draws` (int32 [N]), from the clips `clip` (int32 [N]; None without a clip
        axis), as the per-step wrappers apply it where an episode ended: the draws of `reference_restart_draws` and the state of
        `reference_restart_state` in torch on the device, then the reset launch on that state.  Returns (pipeline state, obs, cur_frame
        int32 [N], clip int32 [N] or None)."""
        N, dev, s, seed = self.num_envs, self.device, self.sys, self._noise_seed
        env, n = torch.arange(N, device=dev), draws.long()
        lo, hi = self._restart_frame_range
        c = None if clip is None else clip.long()
        if self._across_clips:
            h = _reference_restart_hash_t(seed, env, n, 1)
            uniform = (h * self.num_clips) >> 32
            w = None if self._sampling is None else self._sampling["weights"]
            if w is not None:
                prefix = (w.long() & 0xFFFF).cumsum(0)
                c = torch.where(prefix[-1] > 0, torch.searchsorted(prefix, (h * prefix[-1]) >> 32, right=True).clamp(max=self.num_clips - 1), uniform)
            else:
                c = uniform
        f = lo + ((_reference_restart_hash_t(seed, env, n, 2) * (hi - lo)) >> 32)
        if self._clip_lengths is not None:
            L = self._clip_lengths.long()[c if c is not None else torch.zeros_like(env)]
            f = f % (L - 1)
            fr = torch.minimum(f.clamp(min=0), L - 1)
        else:
            fr = f.clamp(0, self.track_len - 1)
        rows = lambda a: a[fr] if c is None else a[c, fr]
        scale = torch.tensor(self._reset_noise_scale, dtype=torch.float32, device=dev)

        def noise(purpose, width):
            h = _reference_restart_hash_t(seed, env[:, None], n[:, None], purpose, torch.arange(width, device=dev)[None, :])
            return scale * ((h >> 8).to(torch.float32) * (2.0 ** -23) - 1.0)
        qpos = torch.cat([rows(self._track_pos), rows(self._track_pose)], dim=-1) + noise(3, s.nq)
        qvel = (rows(self._track_vel) if self._track_vel is not None else torch.zeros(N, s.nv, device=dev)) + noise(4, s.nv)
        st = dict(qpos=qpos.contiguous(), qvel=qvel.contiguous(), act=torch.zeros(N, s.na, device=dev), qacc_warmstart=torch.zeros(N, s.nv, device=dev))
        out = self._alloc_outputs(full=False)
        cur_frame = f.to(torch.int32)
        clip_dev = None if c is None else c.to(torch.int32)
        obs = torch.empty(N, self.observation_size, device=dev)
        library = None if self._clip_lengths is None else dict(lengths=self._clip_lengths)
        self._batch.env_reset(st, self._env_io(cur_frame, obs, clip=clip_dev, clip_library=library), out)
        return PipelineState(**st, **out), obs, cur_frame, clip_dev

    @property
    def clip_sampling(self) -> Optional[dict]:
        """None without `restart_sampling` / `clip_outcomes`, else dict(weights=int32 [C] device table or None, outcomes=int64 [C, 5]
        device table or None, seed): the tables themselves, which the wrapped forms read and add to."""
        return self._sampling

    def set_clip_weights(self, w):
        """The weights a weighted restore draws by (`restart_sampling="weighted"`): float [C], finite, >= 0, not all zero, quantised by
        `quantise_clip_weights`.  Written into the device table IN PLACE: every later launch sees them, a replayed graph included."""
        if self._sampling is None or self._sampling["weights"] is None:
            raise ValueError("set_clip_weights needs an env built with restart_sampling='weighted'")
        w = w.detach().cpu().numpy() if torch.is_tensor(w) else np.asarray(w)
        if w.shape != (self.num_clips,):
            raise ValueError(f"clip weights must have shape ({self.num_clips},), got {tuple(w.shape)}")
        self._sampling["weights"].copy_(torch.from_numpy(quantise_clip_weights(w)))

    def clip_weights(self) -> Optional[np.ndarray]:
        """The weight table as the device holds it, int32 numpy [C] (None without `restart_sampling="weighted"`)."""
        if self._sampling is None or self._sampling["weights"] is None:
            return None
        return self._sampling["weights"].cpu().numpy().copy()

    def clip_outcomes(self, clear: bool = False) -> np.ndarray:
        """The outcome counters so far, int64 numpy [C, 5] with the columns `OUTCOME_COLUMNS` (`clip_outcomes=True`, else ValueError);
        `clear` zeroes the device table after the read (in place).  Synchronises the env's stream."""
        if self._sampling is None or self._sampling["outcomes"] is None:
            raise ValueError("clip_outcomes() needs an env built with clip_outcomes=True")
        out = self._sampling["outcomes"].cpu().numpy().copy()      # (a copy: a CPU tensor shares its memory with the array)
        if clear:
            self._sampling["outcomes"].zero_()
        return out

    @property
    def track_len(self) -> int:
        """Frames T of a clip."""
        return int(self._track_host.shape[-2])

    @property
    def reference_obs_frames(self) -> int:
        """Reference frames H behind every observation row (0: none)."""
        return self._ref_frames

    @property
    def observation_size(self) -> int:
        """Entries of an observation row: the model's obs_dim plus `reference_obs_frames` blocks of nq."""
        return self.sys.obs_dim + self._ref_frames * self.sys.nq

    def set_env_params(self, dof_f=None, act_f=None, con_f=None):
        if self.pose_tracking and not (dof_f is None and act_f is None and con_f is None):
            raise RuntimeError("pose tracking: no pose instance reads per-env parameters (randomize / set_env_params on a pose env)")
        super().set_env_params(dof_f, act_f, con_f)

    def randomize(self, randomization_fn):
        if self.pose_tracking:
            raise RuntimeError("pose tracking: no pose instance reads per-env parameters (randomize / set_env_params on a pose env)")
        return super().randomize(randomization_fn)

    def _env_io(self, cur_frame, obs, reward=None, done=None, metrics=None, clip=None, restart=None, clip_library=None, clip_sampling=None,
                reference_restart=None, **buffers):
        """The env-io dict of a launch.  `buffers`: the step options' output buffers by env-io key (`_launch_buffers`); each brings its
        option's static entries along.  `restart`: the clip-restart block of a multi-step launch (single steps and resets pass none).
        `clip_library`: the clip-library block (an env with `clip_lengths` or `restart_across_clips` only); it rides on the pose block,
        so a reset that hands none (no reference frames: it reads no clamped frame) hands no library either.  `clip_sampling`: the
        clip-sampling block, which rides on the clip-restart block."""
        io = dict(track_pos=self._track_pos, cur_frame=cur_frame, obs=obs, reward=reward, done=done, metrics=metrics, clip=clip,
                  healthy_reward=self._healthy_reward, ctrl_cost_weight=self._ctrl_cost_weight,
                  healthy_z_range=self._healthy_z_range, terminate_when_unhealthy=self._terminate_when_unhealthy,
                  bad_state_max=self._bad_state_max)
        if "pose_metrics" not in buffers and self._ref_frames:      # a reset that writes the reference blocks: it reads the pose rows too,
            buffers["pose_metrics"] = self._reset_pose_metrics     # so it hands the pose block -- and nothing else of the options
        for o in self._options:
            if o.key in buffers:
                io[o.key] = buffers[o.key]
                io.update(o.static)
        if restart is not None:
            io["restart"] = restart
        if clip_library is not None and "pose_metrics" in buffers:
            io["clip_library"] = clip_library
        if clip_sampling is not None and restart is not None:
            io["clip_sampling"] = clip_sampling
        if reference_restart is not None and restart is not None:      # reference restarts ride on the clip-restart block too
            io["reference_restart"] = reference_restart
        return io

    def reset(self, rng, clip=None) -> State:
        """Resets the environment to an initial state.  `rng`: uint32 keys [N, 2] (one jax-style
        PRNG key per env, as `jax.vmap(env.reset)(split(key, N))` passes) or an int seed.

        An env with a [C, T, 3] track gives each env a clip: `randint(rng_pos, 0, C)` from the fourth key of the reference's split (which
        the reference never uses, so start frame, qpos noise and qvel are what a single-clip env draws from the same key), or `clip`, an
        int or integer ids [N] in [0, C) (ValueError outside, and for an env without a clip axis).  The ids live in `info['clip']` (int32
        [N], device) and stay for the life of the state: like `cur_frame` they are not restored by AutoReset, and never re-drawn.  With
        `restart_across_clips` every entry of the start bank has a clip of its own -- `clip` [N] sets entry 0 and the others are drawn,
        [K, N] sets every entry -- kept in `info['restart_bank']['clip']`, and the wrapped forms move `info['clip']` at a restore."""
        N, dev, s = self.num_envs, self.device, self.sys
        if clip is not None:      # (validated before anything else of the env is touched)
            clip = _check_clip(clip, self._num_clips, N, self._clip_restarts if getattr(self, "_across_clips", False) else None)
        K = max(self._clip_restarts, 1)      # entry 0 of the bank is the reset state itself: the same draws, whatever K is
        if isinstance(rng, (int, np.integer)):
            rng = jax_random.split(jax_random.PRNGKey(int(rng)), N)
        keys = np.asarray(rng, dtype=np.uint32).reshape(N, 2)
        frames, noises, qvels, drawn = restart_bank_draws(keys, K, s.nq, s.nv, self._reset_noise_scale, self._restart_frame_range, self._num_clips,
                                                          self._across_clips)
        if clip is None:
            clip = drawn
        elif self._across_clips and clip.ndim == 1:      # entry 0 given, the others as drawn
            clip = np.concatenate([clip[None], drawn[1:]], axis=0)
        # the clip of entry k: its row with `restart_across_clips`, else the env's one clip (None without a clip axis)
        clips = [clip[k] if self._across_clips else clip for k in range(K)]
        to_dev = lambda c: None if c is None else torch.from_numpy(np.ascontiguousarray(c, dtype=np.int32)).to(dev)
        clip_dev = to_dev(clips[0])
        L = self._lengths_host
        library = None if L is None else dict(lengths=self._clip_lengths)
        entries = []
        for k in range(K):
            clip = clips[k]
            if L is not None:       # the draw folded into the entry's clip
                frames[k] = fold_start_frames(frames[k], L, clip)
            # float32 [T, 3] or [C, T, 3] (and the pose rows), what the device holds
            qpos = reset_qpos(s.qpos0, self._track_host, frames[k], noises[k], clip, self._pose_host if self._reset_to_reference else None, L)
            # with the clip's velocities the episode starts moving: the row of the start frame plus the (same) noise
            qvel = reset_qvel(self._vel_host, frames[k], qvels[k], clip, L) if self._vel_host is not None and self._reset_to_reference else qvels[k]
            st = dict(qpos=torch.from_numpy(qpos).to(dev), qvel=torch.from_numpy(qvel).to(dev),
                      act=torch.zeros(N, s.na, device=dev), qacc_warmstart=torch.zeros(N, s.nv, device=dev))
            out = self._alloc_outputs(full=False)
            cur_frame = torch.from_numpy(frames[k].astype(np.int32)).to(dev)
            obs = torch.empty(N, self.observation_size, device=dev)
            self._batch.env_reset(st, self._env_io(cur_frame, obs, clip=clip_dev if k == 0 else to_dev(clip), clip_library=library), out)
            entries.append((st, out, cur_frame, obs))
        st, out, cur_frame, obs = entries[0]
        info = {"cur_frame": cur_frame}
        if clip_dev is not None:
            info["clip"] = clip_dev
        if self._clip_restarts:
            stack = lambda name, src: torch.stack([e[src][name] for e in entries]).contiguous()
            bank_ps = PipelineState(**{n: stack(n, 0) for n in st}, **{n: (stack(n, 1) if out[n] is not None else None) for n in out})
            info["restart_bank"] = dict(pipeline_state=bank_ps, obs=torch.stack([e[3] for e in entries]).contiguous(),
                                        frame=torch.stack([e[2] for e in entries]).contiguous())
            if self._across_clips:
                info["restart_bank"]["clip"] = to_dev(np.stack(clips))
            info["restart_slot"] = torch.zeros(N, dtype=torch.int32, device=dev)
            if (self._sampling is not None and self._sampling["weights"] is not None) or self._ref_restart:      # the restore count the draws hash
                info["restart_draws"] = torch.zeros(N, dtype=torch.int32, device=dev)
        zero = torch.zeros(N, device=dev)
        metrics = {"pos_reward": zero, "reward_quadctrl": zero.clone(), "reward_alive": zero.clone()}
        for o in self._options:
            metrics.update({k: zero.clone() for k in o.metrics})
        return State(PipelineState(**st, **out), obs, zero.clone(), zero.clone(), metrics, info)

    def _launch_buffers(self, state: State, episode_length: Optional[float] = None):
        """What a step launch reads and writes: (st_in, st_out, env-io outputs dict(cur_frame, reward, done, metrics), wrap) -- `wrap` the
        Episode + AutoReset wrappers' state of a multi-step launch (`hip.Batch._unroll_io`), None without `episode_length`.  The previous
        state is left untouched (no copies)."""
        N, dev = self.num_envs, self.device
        ps, info = state.pipeline_state, state.info
        fields = lambda p: dict(qpos=p.qpos, qvel=p.qvel, act=p.act, qacc_warmstart=p.qacc_warmstart)
        st_in = fields(ps)
        st = {k: torch.empty_like(v) for k, v in st_in.items()}
        io = dict(cur_frame=torch.empty_like(info["cur_frame"]), reward=torch.empty(N, device=dev), done=torch.empty(N, device=dev),
                  metrics=torch.empty(N, 3, device=dev), clip=info.get("clip"))      # clip: read only (None without a clip axis)
        for o in self._options:
            io[o.key] = torch.empty((N,) + o.shape, device=dev)
        wrap = None
        if episode_length is not None:
            bank = info["restart_bank"] if self._clip_restarts else dict(pipeline_state=info["first_pipeline_state"], obs=info["first_obs"])
            wrap = dict(first=fields(bank["pipeline_state"]), first_obs=bank["obs"], prev_done=state.done, steps_in=info["steps"],
                        steps_out=torch.empty(N, device=dev), truncation_out=torch.empty(N, device=dev), episode_length=episode_length)
            if self._clip_restarts:      # the restores draw from the bank, and frame and slot travel with the state
                wrap["slots"] = self._clip_restarts
                io["restart"] = dict(frames=bank["frame"], slot_in=info["restart_slot"], slot_out=torch.empty_like(info["restart_slot"]),
                                     end_at_clip_end=self._end_at_clip_end)
        if self._clip_lengths is not None or (self._across_clips and wrap is not None):
            # the clip library: the lengths in every step launch; the entries' clips in the multi-step forms, which return the clip each
            # env is on in a fresh tensor (the incoming state's ids are read only)
            io["clip_library"] = dict(lengths=self._clip_lengths)
            if self._across_clips and wrap is not None:
                io["clip_library"].update(bank_clips=info["restart_bank"]["clip"], clip_out=torch.empty_like(info["clip"]))
        if self._sampling is not None and wrap is not None:      # clip sampling: the multi-step forms count and draw in the kernel
            if not self._ref_restart:
                io["clip_sampling"] = dict(self._sampling)
                if self._sampling["weights"] is not None:
                    io["clip_sampling"].update(draws_in=info["restart_draws"], draws_out=torch.empty_like(info["restart_draws"]))
            elif self._sampling["outcomes"] is not None:
                # reference restarts draw a clip, not a slot: weights and restore counts travel in that block (below), the counters stay here
                io["clip_sampling"] = dict(weights=None, outcomes=self._sampling["outcomes"], seed=self._sampling["seed"])
        if self._ref_restart and wrap is not None:      # reference restarts: the multi-step forms draw and build the start state in the kernel
            io["reference_restart"] = dict(draws_in=info["restart_draws"], draws_out=torch.empty_like(info["restart_draws"]),
                                           weights=None if self._sampling is None else self._sampling["weights"], seed=self._noise_seed,
                                           frame_range=self._restart_frame_range, across_clips=self._across_clips, noise_scale=self._reset_noise_scale)
        return st_in, st, io, wrap

    def _next_state(self, state: State, st, io, obs, wrap=None, out=None) -> State:
        """The State a launch on `_launch_buffers` left."""
        info = dict(state.info)
        info["cur_frame"] = io["cur_frame"]
        if wrap is not None:
            info.update(steps=wrap["steps_out"], truncation=wrap["truncation_out"])
            if "restart" in io:
                info["restart_slot"] = io["restart"]["slot_out"]
            if io.get("clip_library", {}).get("clip_out") is not None:
                info["clip"] = io["clip_library"]["clip_out"]
            if io.get("clip_sampling", {}).get("draws_out") is not None:
                info["restart_draws"] = io["clip_sampling"]["draws_out"]
            if "reference_restart" in io:
                info["restart_draws"] = io["reference_restart"]["draws_out"]
        m = dict(state.metrics)
        m.update(pos_reward=io["metrics"][:, 0], reward_quadctrl=io["metrics"][:, 1], reward_alive=io["metrics"][:, 2])
        for o in self._options:
            m.update(zip(o.metrics, o.read(io[o.key])))
        return state.replace(pipeline_state=PipelineState(**st, **(out or {})), obs=obs, reward=io["reward"], done=io["done"], metrics=m, info=info)

    def unroll_wrapped(self, state: State, actions: torch.Tensor, episode_length: float) -> State:
        """`actions.shape[0]` steps with `EpisodeWrapper(episode_length)` + `AutoResetWrapper` (action_repeat 1) in ONE launch
        (`rr_env_unroll`): what `lax.scan` over the wrapped `step` is to the reference.  `state` is a state of the wrapped env
        (info carries steps, truncation, first_pipeline_state, first_obs -- with `clip_restarts >= 1` restart_bank and restart_slot instead,
        and the launch applies the clip-restart rule); returns the state after the last step, bit for bit what the per-step calls give.  Intermediate observations / rewards are not returned (a random-action rollout needs none)."""
        if self._pipeline_outputs or self._contact_outputs:
            raise ValueError("a multi-step rollout returns no pipeline / contact outputs: build the env without them")
        st_in, st, io, wrap = self._launch_buffers(state, episode_length)
        obs = torch.empty(self.num_envs, self.observation_size, device=self.device)
        actions = actions.to(self.device, torch.float32).contiguous()
        self._rebalance()
        self._batch.env_unroll(st_in, st, actions, self._n_frames, self._env_io(obs=obs, **io), state.info["cur_frame"], wrap)
        return self._next_state(state, st, io, obs, wrap)

    def unroll_policy_wrapped(self, state: State, episode_length: float, actor: dict, noise: torch.Tensor, traj: dict, segment: int = 0) -> State:
        """`generate_unroll` in one launch (`rr_env_unroll_policy`): T = noise.shape[0] x [policy(obs) -> tanh-normal sample -> step ->
        EpisodeWrapper + AutoResetWrapper], the transitions written into `traj` (views of the learner's buffers, batch-major).
        `actor`: the policy's parameters as the kernel takes them (`acting.actor_params`).  `segment` = L: the T steps are recorded as
        T / L trajectories ([U, N, L(+1), ...] buffers) -- a whole rollout phase in one launch.  Returns the state after the last step."""
        if self._pipeline_outputs or self._contact_outputs:
            raise ValueError("a multi-step rollout returns no pipeline / contact outputs: build the env without them")
        N, T = self.num_envs, noise.shape[0]
        st_in, st, io, wrap = self._launch_buffers(state, episode_length)
        actions = torch.empty(T, N, self.action_size, device=self.device)
        obs_in = state.obs.contiguous()            # (also fills the env io's obs slot, which this entry point does not write)
        self._batch.env_unroll_policy(st_in, st, T, self._n_frames, self._env_io(obs=obs_in, **io), state.info["cur_frame"], wrap, actor, noise,
                                      actions, traj, obs_in, segment)
        L_ = segment or T
        obs = traj["obs"].reshape(T // L_, N, L_ + 1, -1)[-1, :, L_].contiguous()
        return self._next_state(state, st, io, obs, wrap), actions

    def eval_supported(self) -> bool:
        """Whether `unroll_eval` serves this env: a batch with an evaluation instance (CG solver, a model with a multi-step instance, no
        per-env parameters) and no pipeline / contact outputs.  False for a pose env: no evaluation instance rewards the pose, so
        evaluation runs the per-step loop, whose `EvalWrapper` sums the two pose metrics like the others."""
        return (not self.pose_tracking and self.device.type == "cuda" and not self._pipeline_outputs and not self._contact_outputs and self._batch.eval_supported())

    def fused_actor_refusal(self) -> Optional[str]:
        """None when the in-kernel actor of the instance this env's multi-step launches run reads the env's row width, else the
        library's text.  The launches run the instance of the highest option in force -- clip restarts, then body tracking, then velocity tracking, then pose
        termination, then the pose instance at the env's reference frames (0 without) -- so that one is asked."""
        if self._clip_restarts:
            return self._batch.clip_restarts_supported(with_actor=True)
        if self._body is not None:
            return self._batch.body_tracking_supported(with_actor=True)
        if self._vel is not None:
            return self._batch.velocity_tracking_supported(with_actor=True)
        if self._clip_lengths is not None:      # per-clip lengths alone: the env steps run the body-tracking instance too
            return self._batch.clip_library_supported(with_actor=True)
        if self._pose_term is not None:
            return self._batch.pose_termination_supported(with_actor=True)
        return self._batch.reference_obs_supported(self._ref_frames, with_actor=True)

    def unroll_eval(self, state: State, T: int, actor: dict, noise: Optional[torch.Tensor] = None, episode_length: Optional[float] = None,
                    eval_metrics: Optional[torch.Tensor] = None, actions_out: Optional[torch.Tensor] = None, qpos_out: Optional[torch.Tensor] = None) -> State:
        """T x [policy(obs) -> action -> step] in ONE launch without a trajectory (`rr_env_unroll_eval`): what an evaluation needs.
        `episode_length` given: `state` is a state of the wrapped env and `EpisodeWrapper(episode_length)` + `AutoResetWrapper` act between
        the steps, with brax's EvalWrapper bookkeeping on `eval_metrics` [N, 6] = (episode_steps, active_episodes, sums of pos_reward,
        reward_quadctrl, reward_alive, reward), updated in place.  `episode_length` None: the unwrapped env, stepping on past `done`.
        `actor`: `acting.actor_params`; `noise` [T, N, A] standard normal draws, None = the deterministic policy.  Optional records:
        `actions_out` [T, N, A], `qpos_out` [T + 1, N, nq] (row 0 the incoming qpos; wrapped: taken before a restore).  Returns the state
        after the last step, as T calls of `step` on the same actions leave it.  A batch without an evaluation instance (`eval_supported`)
        refuses with the reason (RuntimeError)."""
        if self._pipeline_outputs or self._contact_outputs:
            raise ValueError("an evaluation launch returns no pipeline / contact outputs: build the env without them")
        st_in, st, io, wrap = self._launch_buffers(state, episode_length)
        ring = torch.empty(self.num_envs, 2, self.observation_size, device=self.device)
        obs_in = state.obs.contiguous()
        self._batch.env_unroll_eval(st_in, st, int(T), self._n_frames, self._env_io(obs=obs_in, **io), state.info["cur_frame"], actor,
                                    obs_in, ring, noise, actions_out, eval_metrics, qpos_out, wrap)
        return self._next_state(state, st, io, ring[:, int(T) & 1].contiguous(), wrap)

    def step(self, state: State, action: torch.Tensor) -> State:
        """Runs one timestep of the environment's dynamics.  With `bad_state_max` set, a bad env comes back with done = 1, reward 0 and
        metrics 0, but its state and observation are returned as they are (possibly non-finite): restoring is AutoReset's part."""
        st_in, st, io, _ = self._launch_buffers(state)
        out = self._alloc_outputs(full=False)
        obs = torch.empty(self.num_envs, self.observation_size, device=self.device)
        action = action.to(self.device, torch.float32).contiguous()
        self._rebalance()
        self._batch.env_step_to(st_in, st, action, self._n_frames, self._env_io(obs=obs, **io), state.info["cur_frame"], out)
        return self._next_state(state, st, io, obs, out=out)


_CTOR_PARAMS = tuple(p for p in inspect.signature(Rodent.__init__).parameters if p not in ("self", "num_envs", "device", "kwargs"))
