"""CPU validation of the criterion the GPU tests hold `rr_ppo_loss` to (tests/ppo_batches.py), after the pattern of
tests/test_parity_criteria.py: a float32 torch transcription of the formulas of `rr_ppo_gae_kernel` and `rr_ppo_loss_kernel`
(csrc/rr_ppo.h) stands in for the kernel.  Unmutated it must PASS on every batch of the GPU tests; with each of five seeded errors --
the mistakes a kernel of this shape invites -- it must FAIL.  The same batches must reach every branch of the clipped surrogate
(coverage conditions, from the float64 reference alone), and one test documents why the `_batch` tests are not enough on their own."""
import functools

import pytest
import torch

from tests import ppo_batches as pb

ERRORS = ("tie_weight_half", "inr_ignores_upper_bound", "no_clipping", "dscale_without_minus_one", "second_trip_reads_first_z")
# the classes (indices into ppo_batches.CLASS_NAMES) whose rows an error changes: the tie is the in-range rows; the upper bound matters where
# s1 > s2 and rho > hi (adv > 0); an unclipped gradient differs where the true weight is 0 (adv > 0 and rho > hi, adv < 0 and rho < lo); the two
# errors in z show wherever the weight is not 0
SHOWS_ON = dict(tie_weight_half=(1, 4), inr_ignores_upper_bound=(2,), no_clipping=(2, 3), dscale_without_minus_one=(0, 1, 4, 5),
                second_trip_reads_first_z=(0, 1, 4, 5))
SHAPES = [(7, 130, 200, True), (5, 77, 77, False), (3, 8, 8, False)]             # T, B, R, use_idx: the GPU tests' batches
ACTIONS = [2, 30, 32, 33, 38, 64]
CASES = [(T, B, R, A, u, True, 0.3) for (T, B, R, u) in SHAPES for A in ACTIONS] + [(7, 130, 200, 30, True, False, 0.3), (7, 130, 200, 38, True, True, 0.05)]
MIN_STD = 0.001


def transcription(data, logits, values, noise, idx, T, B, A, cfg, normalize_advantage=True, dtype=torch.float32, error=None):
    """(metrics [4], grad_logits [(T+1) B, 2A], grad_values [(T+1) B]) by the kernels' formulas in `dtype`, one tensor op per kernel
    statement; `error` seeds one of ERRORS.  Sums over the action dimension and the block sums are plain sums (the kernels' summation
    ORDER is not transcribed; the block sums are double in the kernels and here)."""
    c = lambda x: x.to(dtype)
    n = T * B
    rows = idx if idx is not None else torch.arange(B)
    tm = lambda k: c(data[k][rows]).transpose(0, 1)                                 # [T, B(, A)]
    reward, discount, truncation = tm("reward") * cfg["reward_scaling"], tm("discount"), tm("truncation")
    gamma, lam = cfg["discounting"], cfg["gae_lambda"]
    v = c(values).reshape(T + 1, B)
    # K1: reverse scan, then the advantages from vs_{t+1}
    mask = 1 - truncation
    nt = 1 - (1 - discount) * mask
    acc, vs = torch.zeros(B, dtype=dtype), [None] * T
    for t in range(T - 1, -1, -1):
        delta = (reward[t] + gamma * nt[t] * v[t + 1] - v[t]) * mask[t]
        acc = delta + gamma * nt[t] * mask[t] * lam * acc
        vs[t] = acc + v[t]
    vs = torch.stack(vs + [v[T]])
    adv = ((reward + gamma * nt * vs[1:] - v[:T]) * mask).reshape(n)
    if normalize_advantage:
        a64 = adv.double()
        mean = a64.sum() / n
        var = (((a64 * a64).sum() / n) - mean * mean).clamp_min(0.0)
        adv = (adv - mean.to(dtype)) * (1.0 / (var.sqrt().to(dtype) + 1e-8))
    # K2, pass 1
    HALF_LOG_2PI, LOG2 = 0.91893853320467274178, 0.69314718055994530942
    sp = torch.nn.functional.softplus
    lg = c(logits)[:n]
    loc, sr = lg[:, :A], lg[:, A:]
    scale = sp(sr) + MIN_STD
    raw, eps = tm("raw_action").reshape(n, A), c(noise)
    z, ls = (raw - loc) / scale, torch.log(scale)
    lp = (-0.5 * z * z - ls - HALF_LOG_2PI - 2.0 * (LOG2 - raw - sp(-2.0 * raw))).sum(1)
    x = loc + scale * eps
    ent = (0.5 + HALF_LOG_2PI + ls + 2.0 * (LOG2 - x - sp(-2.0 * x))).sum(1)
    rho = torch.exp(lp - tm("log_prob").reshape(n))
    lo, hi = 1.0 - cfg["clipping_epsilon"], 1.0 + cfg["clipping_epsilon"]
    s1 = rho * adv
    s2 = rho.clamp(lo, hi) * adv
    inr = ((rho >= lo) if error == "inr_ignores_upper_bound" else (rho >= lo) & (rho <= hi)).to(dtype)
    tie = torch.full_like(inr, 0.5) if error == "tie_weight_half" else 0.5 + 0.5 * inr
    w = torch.where(s1 < s2, torch.ones_like(inr), torch.where(s1 > s2, inr, tie))
    if error == "no_clipping":                # the gradient of the unclipped surrogate (the loss value still clips)
        w = torch.ones_like(inr)
    invn = 1.0 / n
    g_lp = -invn * adv * w * rho
    g_h = -cfg["entropy_cost"] * invn
    ve = vs[:T].reshape(n) - v[:T].reshape(n)
    # K2, pass 2
    i_s = 1.0 / scale
    z2 = (raw - loc) * i_s
    if error == "second_trip_reads_first_z" and A > 32:
        z2 = torch.cat([z2[:, :32], z2[:, :A - 32]], 1)
    th = torch.tanh(loc + scale * eps)
    g_lp, zz1 = g_lp[:, None], z2 * z2 - (0.0 if error == "dscale_without_minus_one" else 1.0)
    dloc = g_lp * z2 * i_s + g_h * (-2.0 * th)
    dscale = g_lp * zz1 * i_s + g_h * (i_s - 2.0 * th * eps)
    sig = 1.0 / (1.0 + torch.exp(-sr))
    gl = torch.zeros((T + 1) * B, 2 * A, dtype=dtype)
    gl[:n] = torch.cat([dloc, dscale * sig], 1)
    gv = torch.zeros((T + 1) * B, dtype=dtype)
    gv[:n] = -0.5 * invn * ve
    # K3
    pl = (-torch.minimum(s1, s2).double().sum() / n).to(dtype)
    vl = (0.25 * (ve.double() * ve.double()).sum() / n).to(dtype)
    el = (-cfg["entropy_cost"] * ent.double().sum() / n).to(dtype)
    return torch.stack([pl + vl + el, pl, vl, el]).double(), gl.double(), gv.double()


@functools.lru_cache(maxsize=None)
def _case(T, B, R, A, use_idx, norm, eps_clip):
    """The batch, its float64 and float32 autograd references and the kept rows: computed once, shared, read only."""
    cfg = dict(pb.CFG, clipping_epsilon=eps_clip)
    batch = pb.onpolicy_batch(T, B, R, A, seed=T * 1000 + B + A, use_idx=use_idx)
    ref64 = pb._reference(*batch, T, B, A, torch.float64, "cpu", norm, cfg)
    ref32 = pb._reference(*batch, T, B, A, torch.float32, "cpu", norm, cfg)
    data, logits, values, noise, idx = batch
    rho, adv = pb.rho_and_advantage64(data, logits, values, idx, T, B, A, norm, cfg)
    return cfg, batch, ref64, ref32, rho, adv


def _label(T, B, R, A, use_idx, norm, eps_clip):
    return f"T={T} B={B} A={A} norm={norm} eps={eps_clip}"


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_batches_reach_every_branch_of_the_clipped_surrogate(case):
    T, B, R, A = case[:4]
    cfg, batch, ref64, ref32, rho, adv = _case(*case)
    pb.assert_coverage(rho, adv, cfg["clipping_epsilon"], T, B, A, _label(*case))
    pb.assert_t0_rows_on_policy(rho, cfg["clipping_epsilon"], B)
    assert float(ref64[0][1].abs()) > 1e-3                                         # policy_loss is O(1), not the ~0 of rho ~ 0


def test_the_overwrite_touches_only_the_minibatch_rows():
    T, B, R, A = 7, 130, 200, 30
    old = pb._batch(T, B, R, A, 5)
    for use_idx in (True, False):
        new = pb.onpolicy_batch(T, B, R, A, 5, use_idx=use_idx)
        rows = old[4] if use_idx else torch.arange(B)
        rest = torch.ones(R, dtype=torch.bool)
        rest[rows] = False
        for k in old[0]:
            assert torch.equal(new[0][k][rest], old[0][k][rest])
            assert torch.equal(new[0][k][rows], old[0][k][rows]) == (k not in ("raw_action", "log_prob"))
        for a, b in zip(new[1:4], old[1:4]):
            assert torch.equal(a, b)
        assert (new[4] is None) if not use_idx else torch.equal(new[4], old[4])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_the_transcription_passes_and_every_seeded_error_fails(case):
    T, B, R, A, use_idx, norm, eps_clip = case
    cfg, batch, (m64, gl64, gv64), (m32, gl32, gv32), rho, adv = _case(*case)
    kept = pb.classes(rho, adv, eps_clip)[1]
    label = _label(*case)
    # the formulas are right: in float64 they are autograd's float64 result
    m, gl, gv = transcription(*batch, T, B, A, cfg, norm, torch.float64)
    assert float((gl - gl64).abs().max()) <= 1e-12 * float(gl64.abs().max()) and float((gv - gv64).abs().max()) <= 1e-12 * float(gv64.abs().max())
    assert float((m - m64).abs().max()) <= 1e-12 * float(m64.abs().max())
    m, gl, gv = transcription(*batch, T, B, A, cfg, norm)
    pb.assert_rowrel_criterion(gl, gl32, gl64, kept, label)
    pb.assert_global_criterion("values", gv, gv32, gv64, label)
    pb.assert_global_criterion("metrics", m, m32, m64, label)
    shares = pb.classes(rho, adv, eps_clip)[0]
    for error in ERRORS:
        if error == "second_trip_reads_first_z" and A <= 32:
            continue
        if sum(shares[k] for k in SHOWS_ON[error]) == 0:       # only the 24-sample batch at 2 actions: no row with adv > 0 and rho > hi
            assert T * B < 900
            continue
        m, gl, gv = transcription(*batch, T, B, A, cfg, norm, error=error)
        with pytest.raises(AssertionError):
            pb.assert_rowrel_criterion(gl, gl32, gl64, kept, f"{label} [{error}]")


def test_the_independent_batches_do_not_see_the_seeded_errors():
    """Why the `_batch` tests are not enough on their own: at 64 actions its rho is 0 to float32, d loss / d logits is the entropy term
    alone, and all five errors pass the global-maximum criterion those tests apply (gradients and metrics alike)."""
    T, B, R, A = 7, 130, 200, 64
    batch = pb._batch(T, B, R, A, seed=T * 1000 + B + A)
    m64, gl64, gv64 = pb._reference(*batch, T, B, A, torch.float64, "cpu")
    m32, gl32, gv32 = pb._reference(*batch, T, B, A, torch.float32, "cpu")
    rho, adv = pb.rho_and_advantage64(batch[0], *batch[1:3], batch[4], T, B, A)
    assert float(rho.median()) < 1e-6 and float(((rho > 0.7) & (rho < 1.3)).double().mean()) == 0
    for error in ERRORS:
        m, gl, gv = transcription(*batch, T, B, A, pb.CFG, error=error)
        for name, got, f32, f64 in (("logits", gl, gl32, gl64), ("values", gv, gv32, gv64), ("metrics", m, m32, m64)):
            pb.assert_global_criterion(name, got, f32, f64, f"_batch A=64 [{error}]")
