"""The learner's KL diagnostics and the two controls they drive, on the CPU: `compute_ppo_loss(diagnostics=True)` against figures formed by
hand in numpy float64, the rule `optim.kl_control_rule` against a table of outcomes written down by hand, the plain-torch `ClippedAdam`
with a KL fed in, and `ppo.train` with `learner_diagnostics`, `target_kl` and the KL-adaptive learning rate -- two gloo ranks included."""
import math
import os

import numpy as np
import pytest
import torch

from rodent_amd.training import optim
from rodent_amd.training.agents.ppo import losses, train as ppo
from rodent_amd.training.distributed import FlatGrads
from tests import kl_control_cases as cases
from tests import ppo_batches as pb
from tests.fake_env import PointEnv

DIAG_KEYS = ("training/approx_kl", "training/approx_kl_max", "training/clip_fraction", "training/explained_variance", "training/entropy")


# ---------------------------------------------------------------------------------------------- diagnostics against numpy float64
def _torch_diag(data, logits, values, noise, idx, T, B, A, dtype=torch.float64):
    c = lambda x: x.to(dtype)
    rows = idx if idx is not None else torch.arange(B)
    mbd = {k: c(data[k][rows]).transpose(0, 1) for k in ("raw_action", "log_prob", "reward", "discount", "truncation")}
    v = c(values).reshape(T + 1, B)
    _, m = losses.compute_ppo_loss(c(logits)[:T * B].reshape(T, B, 2 * A), v[:T], v[T], mbd, pb._fixed_noise_dist(A, noise), diagnostics=True, **pb.CFG)
    return m


@pytest.mark.parametrize("use_idx", [True, False])
def test_diagnostics_match_numpy_float64(use_idx):
    T, B, A = 3, 5, 30
    batch = pb.onpolicy_batch(T, B, 2 * B, A, seed=11, use_idx=use_idx)
    want = cases.numpy_diagnostics(*batch, T, B, A, pb.CFG)
    m = _torch_diag(*batch, T, B, A)
    for k in ("approx_kl", "clip_fraction", "explained_variance", "entropy"):
        assert m[k].dtype == torch.float64
        assert abs(float(m[k]) - want[k]) <= 1e-12 * max(1.0, abs(want[k])), (k, float(m[k]), want[k])
    assert float(m["approx_kl"]) >= 0.0 and want["approx_kl"] > 1e-4            # off-policy rows: a KL to speak of
    assert 0.0 <= want["clip_fraction"] <= 1.0 and want["explained_variance"] < 1.0
    assert set(m) == {"total_loss", "policy_loss", "v_loss", "entropy_loss", "approx_kl", "clip_fraction", "explained_variance", "entropy"}
    # without the option: the four keys of before
    rows = batch[4] if batch[4] is not None else torch.arange(B)
    mbd = {k: batch[0][k][rows].double().transpose(0, 1) for k in ("raw_action", "log_prob", "reward", "discount", "truncation")}
    v = batch[2].double().reshape(T + 1, B)
    _, m0 = losses.compute_ppo_loss(batch[1].double()[:T * B].reshape(T, B, 2 * A), v[:T], v[T], mbd, pb._fixed_noise_dist(A, batch[3]), **pb.CFG)
    assert set(m0) == {"total_loss", "policy_loss", "v_loss", "entropy_loss"}
    assert all(float(m0[k]) == float(m[k]) for k in m0)


def test_on_policy_rows_have_a_tiny_nonnegative_kl():
    """T = 1: every row is a t == 0 row, drawn from the current policy; d is the float32 rounding of the stored log-prob (~1e-6 relative
    to |log_prob| ~ 40), so the k3 term d^2 / 2 is far below 1e-8 -- and not negative, which (rho - 1) - d in float32 could not promise."""
    T, B, A = 1, 5, 30
    batch = pb.onpolicy_batch(T, B, 2 * B, A, seed=12)
    want = cases.numpy_diagnostics(*batch, T, B, A, pb.CFG)
    m = _torch_diag(*batch, T, B, A)
    m32 = _torch_diag(*batch, T, B, A, dtype=torch.float32)
    for kl in (want["approx_kl"], float(m["approx_kl"]), float(m32["approx_kl"])):
        assert 0.0 <= kl < 1e-8, kl
    assert want["clip_fraction"] == 0.0 and float(m["clip_fraction"]) == 0.0
    # the t == 0 rows of the longer batch alone
    T, B = 3, 5
    batch = pb.onpolicy_batch(T, B, 2 * B, A, seed=11)
    rho = cases.numpy_diagnostics(*batch, T, B, A, pb.CFG)["rho"]
    d0 = np.log(rho[:B])
    assert 0.0 <= float(np.mean(np.expm1(d0) - d0)) < 1e-8


@pytest.mark.parametrize("use_idx", [True, False])
def test_the_gpu_tests_reference_batch_covers_the_surrogate(use_idx):
    """The (7, 130, 38) batch of tests/test_gpu_kl_control.py reaches every class of the clipped surrogate with <= 1 % of its rows left
    out near a clip edge (`assert_coverage`), and those rows bound how far a float32 clip count may lie from the float64 one.  The GPU
    test draws the t == 0 rows' action and log-prob with `hip.policy_sample` where this one uses the float64 sampler, so the two batches
    differ at float32 rounding in those B rows; the GPU test therefore asserts the coverage of its own batch again."""
    T, B, A = cases.DIAG_SHAPES[-1]
    data, logits, values, noise, idx = batch = cases.diag_batch(T, B, A, use_idx)
    rho, adv = pb.rho_and_advantage64(data, logits, values, idx, T, B, A, True, pb.CFG)
    kept = pb.assert_coverage(rho, adv, pb.CFG["clipping_epsilon"], T, B, A, f"T={T} B={B} A={A}")
    want = cases.numpy_diagnostics(*batch, T, B, A, pb.CFG)
    np.testing.assert_allclose(want["rho"], rho.numpy(), rtol=1e-10)
    assert cases.edge_rows(rho, pb.CFG["clipping_epsilon"]) == int((~kept).sum()) <= 0.01 * T * B
    m32 = _torch_diag(*batch, T, B, A, dtype=torch.float32)
    assert abs(round(float(m32["clip_fraction"]) * T * B) - round(want["clip_fraction"] * T * B)) <= int((~kept).sum())


def test_explained_variance_is_zero_where_the_returns_do_not_vary():
    T, B, A = 2, 3, 4
    data, logits, values, noise, idx = pb.onpolicy_batch(T, B, B, A, seed=5, use_idx=False)
    data = dict(data, reward=torch.zeros_like(data["reward"]), truncation=torch.zeros_like(data["truncation"]), discount=torch.ones_like(data["discount"]))
    m = _torch_diag(data, logits, torch.zeros_like(values), noise, idx, T, B, A)
    assert float(m["explained_variance"]) == 0.0
    assert cases.numpy_diagnostics(data, logits, torch.zeros_like(values), noise, idx, T, B, A, pb.CFG)["explained_variance"] == 0.0


# ---------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("case", cases.RULE_TABLE, ids=[c[0] for c in cases.RULE_TABLE])
def test_rule_table(case):
    _, kl, lr, stopped, finite, (thr, des, lo, hi), want = case
    got = optim.kl_control_rule(kl, lr, stopped, stop_threshold=thr, desired_kl=des, lr_lo=lo, lr_hi=hi, norm_finite=finite)
    assert got == want and isinstance(got[0], float)
    assert cases.THR == optim.KL_STOP_FACTOR * cases.TARGET


def _make(sizes, p0, lr, **kw):
    params = [torch.tensor(x.copy()) for x in p0]
    flat = FlatGrads(params, extra=4)
    return params, flat, optim.ClippedAdam(params, flat, lr=lr, max_grad_norm=float("inf"), **kw)


def _bits(opt, params):
    return [p.detach().numpy().copy().view(np.uint32) for p in params] + [opt.exp_avg.numpy().copy().view(np.uint32),
                                                                         opt.exp_avg_sq.numpy().copy().view(np.uint32)]


def test_flat_grads_extra_slots():
    p = [torch.zeros(3), torch.zeros(2, 2)]
    f = FlatGrads(p, extra=4)
    assert f.n == 7 and f.flat.numel() == 11 and f.tail.numel() == 4 and f.tail.data_ptr() == f.flat[7:].data_ptr()
    assert p[1].grad.data_ptr() == f.flat[3:].data_ptr()
    g = FlatGrads([torch.zeros(3)])
    assert g.flat.numel() == 3 and g.extra == 0 and g.tail.numel() == 0


def test_flag_is_sticky_until_begin_training_step():
    rng = np.random.default_rng(0)
    sizes = [3, 6]
    p0 = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    params, flat, opt = _make(sizes, p0, 1e-2, target_kl=cases.TARGET)
    g = rng.standard_normal(9).astype(np.float32)
    flat.flat[:9] = torch.tensor(g)
    flat.tail[0] = 0.1
    opt.step()
    assert opt.t == 1 and not opt.stopped
    before = _bits(opt, params)
    flat.tail[0] = 1.0                                       # above 0.75: stops
    opt.step()
    flat.tail[0] = 0.0                                       # harmless KL, but the flag is sticky
    opt.step()
    assert opt.stopped and opt.t == 1 and all(np.array_equal(a, b) for a, b in zip(before, _bits(opt, params)))
    st = opt.stats(clear=False)
    assert st["stopped_updates"] == 2 and st["applied_updates"] == 1 and st["skipped_updates"] == 0 and st["last_kl"] == 1.0
    opt.begin_training_step()
    assert not opt.stopped
    opt.step()
    assert opt.t == 2 and opt.stats()["applied_updates"] == 2
    assert opt.stats()["stopped_updates"] == 0              # cleared with the other counters


@pytest.mark.parametrize("case", cases.RULE_TABLE, ids=[c[0] for c in cases.RULE_TABLE])
def test_cpu_step_follows_the_table(case):
    """One step from t = 4 with the case's KL fed in: a step that is not applied keeps p, m, v and t bitwise; an applied one equals
    `clipped_adam_reference` at the adapted learning rate within the counted bound of tests/grad_clip_cases.py."""
    from tests import grad_clip_cases
    _, kl, lr, stopped, finite, (thr, des, lo, hi), (want_lr, want_stop, want_applied) = case
    rng = np.random.default_rng(3)
    sizes = [5, 1, 6]
    n = sum(sizes)
    p0 = [rng.standard_normal(k).astype(np.float32) for k in sizes]
    kw = {}
    if thr:
        kw["target_kl"] = cases.TARGET
    if des:
        kw.update(desired_kl=des, learning_rate_bounds=(lo, hi))
    if not kw:
        params = [torch.tensor(x.copy()) for x in p0]
        flat = FlatGrads(params, extra=4)
        opt = optim.ClippedAdam(params, flat, lr=lr, max_grad_norm=float("inf"))
        assert opt.kl is None
    else:
        params, flat, opt = _make(sizes, p0, lr, **kw)
    m0, v0 = (0.1 * rng.standard_normal(n)).astype(np.float32), (0.01 * rng.random(n)).astype(np.float32)
    opt.load_state_dict({"t": 4, "exp_avg": torch.tensor(m0), "exp_avg_sq": torch.tensor(v0), "kl_stop": stopped, "lr": lr})
    g = rng.standard_normal(n).astype(np.float32)
    if not finite:
        g[7] = np.nan
    flat.flat[:n] = torch.tensor(g)
    flat.tail[0] = kl
    before = _bits(opt, params)
    opt.step()
    assert opt.learning_rate == want_lr and opt.stopped == want_stop
    if not want_applied:
        assert opt.t == 4 and all(np.array_equal(a, b) for a, b in zip(before, _bits(opt, params)))
        st = opt.stats()
        assert st["applied_updates"] == 0 and st.get("stopped_updates", 0) == (1 if want_stop else 0) and st["skipped_updates"] == (0 if want_stop else 1)
        return
    ref = grad_clip_cases.reference_step(np.concatenate(p0), g, m0, v0, 4, want_lr, float("inf"))
    assert opt.t == 5 == ref["t"]
    sh = grad_clip_cases.shares(np.concatenate([p.detach().numpy() for p in params]), opt.exp_avg.numpy(), opt.exp_avg_sq.numpy(), ref)
    assert max(sh) <= 1.0, sh
    if want_lr != lr:                                        # the test is sharp: the old rate would miss the bound
        old = grad_clip_cases.reference_step(np.concatenate(p0), g, m0, v0, 4, lr, float("inf"))
        assert grad_clip_cases.shares(np.concatenate([p.detach().numpy() for p in params]), opt.exp_avg.numpy(), opt.exp_avg_sq.numpy(), old)[0] > 1.0


def test_state_dict_carries_lr_and_flag():
    rng = np.random.default_rng(4)
    sizes = [4, 3]
    p0 = [rng.standard_normal(k).astype(np.float32) for k in sizes]
    kw = dict(target_kl=cases.TARGET, desired_kl=cases.DES, learning_rate_bounds=(cases.LO, cases.HI))
    params, flat, opt = _make(sizes, p0, cases.LR, **kw)
    flat.flat[:7] = torch.tensor(rng.standard_normal(7).astype(np.float32))
    flat.tail[0] = 0.5
    opt.step()                                               # lr / 1.5
    flat.tail[0] = 2.0
    opt.step()                                               # stop
    sd = opt.state_dict()
    assert sd["lr"] == cases.LR / 1.5 and sd["kl_stop"] is True and sd["t"] == 1 and len(sd["stats"]) == 5 and sd["hyper"]["lr"] == cases.LR
    params_b, flat_b, opt_b = _make(sizes, [p.detach().numpy() for p in params], cases.LR, **kw)
    opt_b.load_state_dict(sd)
    assert opt_b.stopped and opt_b.learning_rate == cases.LR / 1.5 and opt_b.t == 1
    drop = lambda st: {k: v for k, v in st.items() if k != "last_kl"}          # the last KL is a readout, not state
    assert drop(opt_b.stats(clear=False)) == drop(opt.stats(clear=False))


@pytest.mark.parametrize("kw", [dict(target_kl=0.0), dict(target_kl=-1.0), dict(target_kl=float("nan")), dict(target_kl=float("inf")), dict(target_kl="0.1"),
                                dict(target_kl=True), dict(learning_rate_schedule="cosine"), dict(learning_rate_schedule="adaptive_kl", desired_kl=0.0),
                                dict(learning_rate_schedule="adaptive_kl", learning_rate_bounds=(1e-3, 1e-2)),        # learning_rate 1e-4 outside
                                dict(learning_rate_schedule="adaptive_kl", learning_rate_bounds=(1e-2, 1e-5)),
                                dict(learning_rate_schedule="adaptive_kl", learning_rate_bounds=1e-3),
                                dict(learning_rate_schedule="adaptive_kl", desired_kl=float("nan"))])
def test_bad_arguments_raise(kw):
    with pytest.raises(ValueError):
        ppo.train(environment=PointEnv(8), num_timesteps=100, episode_length=10, num_envs=8, batch_size=8, num_minibatches=1, **kw)


def test_constructor_needs_a_kl_slot():
    p = [torch.zeros(3)]
    with pytest.raises(ValueError):
        optim.ClippedAdam(p, FlatGrads(p), lr=1e-3, max_grad_norm=1.0, target_kl=0.1)
    with pytest.raises(ValueError):
        optim.ClippedAdam(p, torch.zeros(3), lr=1e-3, max_grad_norm=1.0, desired_kl=0.01, learning_rate_bounds=(1e-5, 1e-2))
    opt = optim.ClippedAdam(p, FlatGrads(p, extra=4), lr=1e-3, max_grad_norm=1.0, target_kl=0.1)
    assert opt.kl is not None and opt.flat.numel() == 3


# ---------------------------------------------------------------------------------------------- ppo.train
_TRAIN = dict(num_timesteps=16 * 5 * 4 * 3, episode_length=20, num_envs=16, batch_size=16, num_minibatches=4, unroll_length=5,
              num_updates_per_batch=3, num_evals=4, num_eval_envs=8, learning_rate=3e-3, normalize_observations=True, seed=0)


def _run(**kw):
    log = []
    out = ppo.train(environment=PointEnv(16), return_training_state=True, progress_fn=lambda n, m: log.append(dict(m)), **dict(_TRAIN, **kw))
    vec = torch.cat([p.detach().reshape(-1) for p in out[1][1].parameters()] + [p.detach().reshape(-1) for p in out[3].params.value.parameters()])
    return log, vec.numpy().view(np.uint32), out[3].optimizer_state


def test_new_metric_keys_appear_only_with_an_option():
    log, _, _ = _run()
    assert not any(k in log[-1] for k in DIAG_KEYS + ("training/stopped_updates", "training/learning_rate"))
    log, _, opt = _run(learner_diagnostics=True)
    assert isinstance(opt, torch.optim.Adam)                 # diagnostics alone keep the optimiser
    for m in log[1:]:
        assert all(k in m and math.isfinite(m[k]) for k in DIAG_KEYS), m
        assert 0.0 <= m["training/approx_kl"] <= m["training/approx_kl_max"] and 0.0 <= m["training/clip_fraction"] <= 1.0
        assert m["training/explained_variance"] <= 1.0
        assert "training/stopped_updates" not in m and "training/learning_rate" not in m and "training/grad_norm" not in m
    log, _, opt = _run(target_kl=1e9)
    assert isinstance(opt, optim.ClippedAdam) and all(k in log[-1] for k in DIAG_KEYS + ("training/stopped_updates",))
    assert "training/learning_rate" not in log[-1]
    log, _, opt = _run(learning_rate_schedule="adaptive_kl", learning_rate_bounds=(1e-5, 1e-2))
    assert all(k in log[-1] for k in DIAG_KEYS + ("training/learning_rate",)) and "training/stopped_updates" not in log[-1]
    assert 1e-5 <= log[-1]["training/learning_rate"] <= 1e-2 and log[-1]["training/learning_rate"] == opt.learning_rate


def test_diagnostics_leave_the_default_run_unchanged():
    _, a, _ = _run()
    _, b, _ = _run(learner_diagnostics=True)
    assert np.array_equal(a, b)


def test_a_target_never_reached_gives_the_bits_of_max_grad_norm_inf():
    log_a, a, opt_a = _run(max_grad_norm=float("inf"))
    log_b, b, opt_b = _run(target_kl=1e9)
    assert np.array_equal(a, b) and opt_a.t == opt_b.t == 3 * 3 * 4
    assert all(m["training/stopped_updates"] == 0 for m in log_b[1:])
    assert [m["training/grad_norm"] for m in log_a[1:]] == [m["training/grad_norm"] for m in log_b[1:]]


def test_a_tiny_target_stops_every_training_step_after_its_first_pass():
    counts = {"evaluated": 0}
    real = losses.compute_ppo_loss

    def counting(*a, **k):
        counts["evaluated"] += 1
        return real(*a, **k)

    _, _, opt_full = _run(max_grad_norm=float("inf"))
    tot = {"applied": 0, "stopped": 0, "skipped": 0}
    stats = optim.ClippedAdam.stats

    def recording(self, clear=True):
        st = stats(self, clear)
        if clear:
            tot["applied"] += st["applied_updates"]; tot["stopped"] += st["stopped_updates"]; tot["skipped"] += st["skipped_updates"]
        return st

    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(ppo.ppo_losses, "compute_ppo_loss", counting)
        mp.setattr(optim.ClippedAdam, "stats", recording)
        log, _, opt = _run(target_kl=1e-12)
    finally:
        mp.undo()
    nmb = _TRAIN["num_minibatches"]
    assert tot["applied"] + tot["stopped"] + tot["skipped"] == counts["evaluated"]
    assert counts["evaluated"] % nmb == 0 and counts["evaluated"] < 3 * 3 * nmb
    assert tot["stopped"] >= 1 and sum(m["training/stopped_updates"] for m in log[1:]) == tot["stopped"]
    assert opt.t == tot["applied"] < opt_full.t == 3 * 3 * nmb
    assert all(m["training/approx_kl_max"] > 1.5e-12 for m in log[1:])


# ---------------------------------------------------------------------------------------------- two ranks
class RankEnv(PointEnv):
    """PointEnv whose rewards differ between the ranks, so that each rank measures another KL."""

    def step(self, state, action):
        s = super().step(state, action)
        return s.replace(reward=s.reward * (1.0 + 2.0 * int(os.environ.get("RANK", "0"))))

    def with_num_envs(self, n, device=None):
        return RankEnv(n, device or self.device)


def _dp_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    try:
        log = []
        _, params, _, ts = ppo.train(environment=RankEnv(16), num_timesteps=32 * 5 * 2 * 2, episode_length=20, num_envs=32, batch_size=32,
                                     num_minibatches=2, unroll_length=5, num_updates_per_batch=3, num_evals=3, num_eval_envs=8, learning_rate=3e-3,
                                     normalize_observations=True, seed=3, target_kl=2e-3, learning_rate_schedule="adaptive_kl",
                                     desired_kl=1e-4, learning_rate_bounds=(1e-4, 1e-2), return_training_state=True,
                                     progress_fn=lambda n, m: log.append(dict(m)))
        vec = torch.cat([p.detach().reshape(-1) for p in params[1].parameters()])
        opt = ts.optimizer_state
        out[rank] = (vec.numpy().copy().view(np.uint32), opt.t, opt.learning_rate, sum(m.get("training/stopped_updates", 0) for m in log),
                     float(ts.params.value.layers[0].weight.detach().double().sum()))
    finally:
        torch.distributed.destroy_process_group()


def test_two_gloo_ranks_take_the_same_decisions():
    """Different data on each rank (their own envs and a rank-dependent reward scale) and a target small enough to stop: the KL travels
    through the gradient all-reduce, so both ranks stop at the same update and adapt the same learning rate -- identical bits."""
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    out = mgr.dict()
    port = 35500 + os.getpid() % 2000
    mp.spawn(_dp_worker, args=(2, port, out), nprocs=2, join=True)
    (p0, t0, lr0, s0, v0), (p1, t1, lr1, s1, v1) = out[0], out[1]
    assert np.array_equal(p0, p1) and t0 == t1 and lr0 == lr1 and v0 == v1
    print("two ranks: t %d, lr %g, stopped updates %d" % (t0, lr0, s0))
    assert s0 >= 1 and 0 < t0 < 2 * 3 * 2 and lr0 != 3e-3         # some updates applied at an adapted rate, then a stop
