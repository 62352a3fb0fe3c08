"""Host bookkeeping of the clip-library tests, shared by tests/test_clip_library_cpu.py and tests/test_gpu_clip_library.py.  No tests
here and no device: everything comes from the draws alone.

Fixture: that of tests/test_gpu_clip_restart.py -- 32 envs, three clips, T = 104, episodes of 5 steps, 14 steps, bank frames drawn in
[90, 102), reset clips arange(N) % 3 -- with the lengths (104, 14, 9): clip 0 keeps every row, clips 1 and 2 are so short that the
clamps, the H = 5 reference blocks and the clip's end bite within an episode.  Every start is folded into its entry's clip,
start = draw mod (L_c - 1).  `schedule` plays the rule of DESIGN.md section 4s on an env that never ends by itself (the GPU cases that
compare with it run `terminate_when_unhealthy=False`)."""
import functools

import numpy as np

from rodent_amd import jax_random
from rodent_amd.envs import rodent

N, C, T, EPISODE, STEPS = 32, 3, 104, 5, 14
SEED, RANGE = 94, (90, 102)
LENGTHS = np.array([104, 14, 9], dtype=np.int32)
IDS = (np.arange(N) % C).astype(np.int32)
NQ, NV, NOISE = 74, 73, 0.01       # rodent_optimized / rodent_0 (the draws' widths; frames and clips do not depend on them)


def keys(seed=SEED):
    return jax_random.split(jax_random.PRNGKey(seed), N)


@functools.lru_cache(maxsize=None)
def bank(K, across=True, lengths=True, seed=SEED):
    """(start frames int32 [K, N], folded where `lengths`; clips int32 [K, N]) of the fixture's bank: entry 0 on the reset clips IDS,
    the others as drawn (`across`) or on the env's clip."""
    frames, _, _, clip = rodent.restart_bank_draws(keys(seed), K, NQ, NV, NOISE, RANGE if K > 1 else (0, 100), C, across)
    clips = np.concatenate([IDS[None], clip[1:]], axis=0) if across else np.broadcast_to(IDS, (K, N)).copy()
    if lengths:
        frames = rodent.fold_start_frames(frames, LENGTHS, clips)
    return frames, clips.astype(np.int32)


def schedule(K, across=True, lengths=True, end=True, steps=STEPS, seed=SEED):
    """The rule on an env that never ends by itself.  dict of arrays [steps, N]: `by_len` / `by_end` (which cause holds at that step;
    both may), `over` (either), `clip_before` (the clip the step was made on), `clip` / `frame` / `slot` after the step's restore,
    `changed` (a restore that changed the env's clip)."""
    frames, clips = bank(K, across, lengths, seed)
    Ls = LENGTHS if lengths else np.full(C, T)
    out = {k: np.zeros((steps, N), dtype=np.int64) for k in ("by_len", "by_end", "over", "clip_before", "clip", "frame", "slot", "changed")}
    for e in range(N):
        f, c, slot, n = int(frames[0, e]), int(clips[0, e]), 0, 0
        for t in range(steps):
            n, nf = n + 1, f + 1
            a, b = n >= EPISODE, bool(end) and nf >= Ls[c] - 1
            out["by_len"][t, e], out["by_end"][t, e], out["over"][t, e], out["clip_before"][t, e] = a, b, a or b, c
            if a or b:
                slot = (slot + 1) % K
                out["changed"][t, e] = int(clips[slot, e]) != c
                f, c, n = int(frames[slot, e]), int(clips[slot, e]), 0
            else:
                f = nf
            out["clip"][t, e], out["frame"][t, e], out["slot"][t, e] = c, f, slot
    return out


def counts(K=3, seed=SEED):
    """(restores by the clip's end on each of the three clips, restores by `episode_length`, restores that change the env's clip) of
    the run with both options on."""
    s = schedule(K, seed=seed)
    by_end = [int((s["by_end"] * (s["clip_before"] == c)).sum()) for c in range(C)]
    return by_end, int(s["by_len"].sum()), int(s["changed"].sum())
