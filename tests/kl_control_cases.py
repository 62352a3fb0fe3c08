"""Shared by tests/test_kl_control_cpu.py and tests/test_gpu_kl_control.py: the case table of the KL controls' rule (`optim.kl_control_rule`)
with the outcome of every case written down by hand, the diagnostics of a minibatch formed by hand in numpy float64, and the shapes of
the diagnostic kernel's tests.

Every KL of the table is a float32 number (the rule's input is the float32-rounded KL), and the settings are chosen so that the edges are
exact: target_kl = 0.5 stops above 0.75; desired_kl = 2^-7 has its edges at 2^-6 and 2^-8."""
import math

import numpy as np

TARGET = 0.5
THR = 0.75                       # 1.5 x TARGET, exact
DES = 2.0 ** -7
LO, HI, LR = 1e-3, 4e-3, 2e-3
OFF = (0.0, 0.0, 0.0, 0.0)
STOP_ONLY = (THR, 0.0, 0.0, 0.0)
LR_ONLY = (0.0, DES, LO, HI)
BOTH = (THR, DES, LO, HI)


def up32(x):
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


def down32(x):
    return float(np.nextafter(np.float32(x), np.float32(-np.inf)))


# (name, kl, lr, stop flag before, gradient norm finite, (threshold, desired_kl, lo, hi), (lr, stop flag, applied) after)
RULE_TABLE = [
    ("kl_at_the_threshold_does_not_stop", THR, LR, False, True, STOP_ONLY, (LR, False, True)),
    ("next_float_above_the_threshold_stops", up32(THR), LR, False, True, STOP_ONLY, (LR, True, False)),
    ("nan_stops", math.nan, LR, False, True, STOP_ONLY, (LR, True, False)),
    ("inf_stops", math.inf, LR, False, True, STOP_ONLY, (LR, True, False)),
    ("flag_is_sticky_at_zero_kl", 0.0, LR, True, True, STOP_ONLY, (LR, True, False)),
    ("flag_is_sticky_with_the_schedule_and_leaves_lr", 2.0 ** -20, LR, True, True, BOTH, (LR, True, False)),
    ("controls_off_apply", 5.0, LR, False, True, OFF, (LR, False, True)),
    ("nan_without_a_target_is_applied_at_the_old_lr", math.nan, LR, False, True, LR_ONLY, (LR, False, True)),
    ("kl_at_twice_desired_leaves_lr", 2.0 * DES, LR, False, True, LR_ONLY, (LR, False, True)),
    ("next_float_above_twice_desired_lowers_lr", up32(2.0 * DES), LR, False, True, LR_ONLY, (LR / 1.5, False, True)),
    ("kl_at_half_desired_leaves_lr", 0.5 * DES, LR, False, True, LR_ONLY, (LR, False, True)),
    ("next_float_below_half_desired_raises_lr", down32(0.5 * DES), LR, False, True, LR_ONLY, (LR * 1.5, False, True)),
    ("zero_kl_leaves_lr", 0.0, LR, False, True, LR_ONLY, (LR, False, True)),
    ("clamped_at_the_lower_bound", 0.25, 1.2e-3, False, True, LR_ONLY, (LO, False, True)),
    ("clamped_at_the_upper_bound", 2.0 ** -20, 3e-3, False, True, LR_ONLY, (HI, False, True)),
    ("already_at_the_lower_bound", 0.25, LO, False, True, LR_ONLY, (LO, False, True)),
    ("stopping_update_leaves_lr", 1.0, LR, False, True, BOTH, (LR, True, False)),
    ("below_the_threshold_the_schedule_acts", 0.5, LR, False, True, BOTH, (LR / 1.5, False, True)),
    ("skipped_update_leaves_lr", 0.25, LR, False, False, LR_ONLY, (LR, False, False)),
    ("stop_comes_before_the_skip", 1.0, LR, False, False, BOTH, (LR, True, False)),
]

# (T, B, A) of the diagnostic kernel's tests: 32 lanes per sample and 8 samples per block in the loss kernel, 256 trajectories per GAE block
DIAG_SHAPES = [(1, 1, 1), (3, 5, 30), (2, 257, 33), (4, 9, 64), (7, 130, 38)]


def numpy_diagnostics(data, logits, values, noise, idx, T, B, A, cfg, min_std=0.001):
    """approx_kl, clip_fraction, explained_variance, entropy and the float64 rho of a minibatch, formed by hand in numpy float64 from the
    float32 inputs of `ppo_batches` (torch only hands the arrays over): tanh-normal log-prob, GAE by its recursion, population variances."""
    f = lambda x: np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x, dtype=np.float64)
    rows = np.arange(B) if idx is None else np.asarray(idx.cpu().numpy())
    tm = lambda k: np.swapaxes(f(data[k])[rows], 0, 1)                     # time-major [T, B(, A)]
    raw, lp_b, rew, disc, trunc = (tm(k) for k in ("raw_action", "log_prob", "reward", "discount", "truncation"))
    lg = f(logits)[:T * B].reshape(T, B, 2 * A)
    loc, scale = lg[..., :A], np.logaddexp(0.0, lg[..., A:]) + min_std
    softplus = lambda x: np.logaddexp(0.0, x)
    logdet = lambda x: 2.0 * (math.log(2.0) - x - softplus(-2.0 * x))      # log |d tanh / dx|
    z = (raw - loc) / scale
    lp = (-0.5 * z * z - np.log(scale) - 0.5 * math.log(2.0 * math.pi) - logdet(raw)).sum(-1)
    d = lp - lp_b
    kl = float(np.mean(np.expm1(d) - d))
    rho = np.exp(d)
    eps = cfg["clipping_epsilon"]
    clip = float(np.mean(~((rho >= 1.0 - eps) & (rho <= 1.0 + eps))))
    # GAE, truncation-aware
    v = f(values).reshape(T + 1, B)
    r = rew * cfg["reward_scaling"]
    term = (1.0 - disc) * (1.0 - trunc)
    mask = 1.0 - trunc
    acc = np.zeros(B)
    vs = np.zeros((T, B))
    for t in range(T - 1, -1, -1):
        delta = (r[t] + cfg["discounting"] * (1.0 - term[t]) * v[t + 1] - v[t]) * mask[t]
        acc = delta + cfg["discounting"] * (1.0 - term[t]) * mask[t] * cfg["gae_lambda"] * acc
        vs[t] = acc + v[t]
    ve = vs - v[:T]
    var_vs = float(np.var(vs))
    ev = 1.0 - float(np.var(ve)) / var_vs if var_vs > 0.0 else 0.0
    raw_s = loc + scale * f(noise).reshape(T, B, A)
    ent = float(np.mean((0.5 + 0.5 * math.log(2.0 * math.pi) + np.log(scale) + logdet(raw_s)).sum(-1)))
    return dict(approx_kl=kl, clip_fraction=clip, explained_variance=ev, entropy=ent, rho=rho.reshape(-1))


def diag_batch(T, B, A, use_idx, sampler=None):
    """The on-policy batch of the diagnostic kernel's tests at one shape: a fixed seed per shape, R = B + 3 rows to index into."""
    from tests import ppo_batches
    return ppo_batches.onpolicy_batch(T, B, B + 3 if use_idx else B, A, seed=T * 1000 + B + A, use_idx=use_idx, sampler=sampler)


def edge_rows(rho, eps_clip):
    """Rows whose float64 rho lies within `ppo_batches.EDGE` of a clip edge: a float32 evaluation may count them on the other side."""
    from tests import ppo_batches
    rho = np.asarray(rho, dtype=np.float64)
    return int(((np.abs(rho - (1.0 - eps_clip)) < ppo_batches.EDGE) | (np.abs(rho - (1.0 + eps_clip)) < ppo_batches.EDGE)).sum())
