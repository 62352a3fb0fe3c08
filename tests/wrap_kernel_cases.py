"""Shared by tests/test_wrap_kernels_cpu.py and tests/test_gpu_wrap_kernels.py: synthetic inputs of the fused per-step wrapper entries
(rr_wrap_episode_autoreset, rr_wrap_clip_restart, rr_wrap_clip_library, rr_wrap_clip_sampling) and their rule restated in plain torch
from include/rodent_rr.h (rr_clip_restart_io, rr_clip_library_io, rr_clip_sampling_io and the four entries' own comments), with the draw
and the counters taken from the composed wrappers (`wrappers.weighted_slots`, `wrappers.count_outcomes`).  No env, no model.

One thing the header leaves to the entries: a slot_in outside 0 .. K - 1 is clamped into the bank before anything else is done with it,
so slot_out holds the clamped slot where the env is not done.

Shapes: 64 envs from one seeded generator, K = 1 or 3 bank entries, 4 clips, restored arrays of widths 1, 5 and 300 (300 > 256 threads:
the strided copy makes a second trip), twelve arrays (RR_WRAP_MAX) of which a case uses the first `narr`."""
import torch

from rodent_amd.envs import wrappers

N, C, SLOTS = 64, 4, (1, 3)
WIDTHS = (1, 5, 300) * 4
EPISODE, TRACK_LEN = 5.0, 20
LENGTHS = (9, 12, 7, 25)              # clip 0 differs from TRACK_LEN (it applies without clip ids); 25 > TRACK_LEN is clamped to it
WEIGHTS = (3, 0, 65535, 9)            # clip 1 is never drawn
SEED = 94
NAN_BITS = 0x7FC01234                 # a quiet NaN with a payload: copies and survivals are checked bit for bit
DONE_ENV, LIVE_ENV = 10, 11           # a done env and one that no case ends: each holds NaNs in its `cur` rows
ZERO_BANK_ENVS = (5, 6)               # their whole bank lies on the weight-0 clip
LEVELS = ("plain", "restart", "library", "sampling")


def _nan():
    return torch.tensor([NAN_BITS], dtype=torch.int32).view(torch.float32)[0]


def inputs(K, seed=20):
    """CPU tensors of one case family.  `first` are the plain entry's stored states [N, w], `bank` the clip entries' [K, N, w]."""
    g = torch.Generator().manual_seed(seed + K)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi, shape, generator=g, dtype=torch.int32)
    rf = lambda *shape: torch.randn(*shape, generator=g)
    coin = lambda p: (torch.rand(N, generator=g) < p).float()
    x = dict(K=K, prev_done=coin(0.25), prev_steps=ri(0, 5, N).float(), done=coin(0.25), cur_frame=ri(0, TRACK_LEN, N), slot_in=ri(0, K, N),
             clip=ri(0, C, N), bank_frames=ri(0, TRACK_LEN, K, N), bank_clips=ri(0, C, K, N), draws=ri(0, 50, N), pose_fail=coin(0.2) * 3.0,
             outcomes=torch.randint(0, 100, (C, 5), generator=g), lengths=torch.tensor(LENGTHS, dtype=torch.int32),
             weights=torch.tensor(WEIGHTS, dtype=torch.int32), first=[rf(N, w) for w in WIDTHS], bank=[rf(K, N, w) for w in WIDTHS],
             cur=[rf(N, w) for w in WIDTHS])
    x["slot_in"][:4] = torch.tensor([-2, K + 3, -1, K], dtype=torch.int32)
    x["done"][0], x["done"][1] = 1.0, 0.0                     # the clamp is seen on an env that restores and on one that may not
    for e in ZERO_BANK_ENVS:
        x["bank_clips"][:, e] = 1
    x["done"][ZERO_BANK_ENVS[0]] = 1.0
    x["done"][DONE_ENV] = 1.0
    x["done"][LIVE_ENV], x["prev_done"][LIVE_ENV], x["cur_frame"][LIVE_ENV], x["pose_fail"][LIVE_ENV] = 0.0, 1.0, 0, 0.0
    nan = _nan()
    for e in (DONE_ENV, LIVE_ENV):
        x["cur"][0][e, 0] = x["cur"][1][e, 2] = x["cur"][2][e, 257] = x["cur"][2][e, 299] = nan
    x["first"][1][DONE_ENV, 0] = nan                           # a stored NaN comes back with its payload
    x["bank"][1][:, DONE_ENV, 0] = nan
    return x


def restate(x, level, *, narr=3, action_repeat=1.0, end_at_clip_end=True, clip=True, bank_clips=True, lengths=True, pose_fail=True,
            weights=True, outcomes=True):
    """What the entry of `level` leaves behind on the inputs `x`; the flags say which optional pointers are given (a level ignores those
    it does not have).  -> (outputs by name, intermediate values for the input-class checks)."""
    i = LEVELS.index(level)
    clip, bank_clips, lengths = clip and i >= 2, bank_clips and i >= 2, lengths and i >= 2
    pose_fail, weights, outcomes = pose_fail and i >= 3, weights and i >= 3, outcomes and i >= 3
    K, env = x["K"], torch.arange(N)
    s1 = torch.where(x["prev_done"] != 0, torch.zeros(N), x["prev_steps"]) + torch.tensor(action_repeat, dtype=torch.float32)
    over_len = s1 >= EPISODE
    over_end = torch.zeros(N, dtype=torch.bool)
    on = x["clip"].long().clamp(0, C - 1) if clip else torch.zeros(N, dtype=torch.long)      # the clip the step was made on
    if i >= 1 and end_at_clip_end:
        own = x["lengths"][on].clamp(1, TRACK_LEN) if lengths else TRACK_LEN
        over_end = x["cur_frame"] >= own - 1
    over = over_len | over_end
    d_env = x["done"]
    done = torch.where(over, torch.ones(N), d_env)
    d = done != 0
    out = dict(steps=s1, truncation=torch.where(over, 1.0 - d_env, torch.zeros(N)), done=done)
    aux = dict(over_len=over_len, over_end=over_end, over=over, d=d)
    if i == 0:
        src = [f for f in x["first"][:narr]]
    else:
        slot = x["slot_in"].long().clamp(0, K - 1)
        cyclic = (slot + 1) % K
        nslot = torch.where(d, cyclic, slot)
        if weights:
            drawn = wrappers.weighted_slots(x["weights"], x["bank_clips"], SEED, x["draws"])
            nslot = torch.where(d & (drawn >= 0), drawn, nslot)
            out["draws"] = x["draws"] + d.to(torch.int32)
            aux.update(drawn=drawn)
        out["slot"] = nslot.to(torch.int32)
        out["cur_frame"] = torch.where(d, x["bank_frames"][nslot, env], x["cur_frame"])
        if clip:
            out["clip"] = torch.where(d, x["bank_clips"][nslot, env], x["clip"]) if bank_clips else x["clip"].clone()
        if outcomes:
            table = x["outcomes"].clone()
            wrappers.count_outcomes(table, on, x["pose_fail"] != 0 if pose_fail else torch.zeros(N, dtype=torch.bool), d_env != 0, d)
            out["outcomes"] = table
        aux.update(slot=slot, cyclic=cyclic, nslot=nslot)
        src = [b[nslot, env] for b in x["bank"][:narr]]
    out["cur"] = [torch.where(d[:, None], s, c) for s, c in zip(src, x["cur"][:narr])]
    return out, aux


def same_bits(a, b):
    """Bitwise equality; float arrays through their int32 view, so NaN payloads count."""
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)
