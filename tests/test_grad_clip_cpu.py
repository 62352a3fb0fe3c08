"""`ppo.train(max_grad_norm=...)` on the CPU: the rule restated in float64 (`optim.clipped_adam_reference`) against torch's own
clip_grad_norm_ + Adam, the plain-torch `ClippedAdam` against that reference, the skip of non-finite updates, and `ppo.train` with the
option -- metrics, a NaN reward that ruins a run without it, and two gloo ranks."""
import math
import os
import warnings

import numpy as np
import pytest
import torch

from rodent_amd.training import optim
from rodent_amd.training.agents.ppo import train as ppo
from rodent_amd.training.distributed import FlatGrads
from tests import grad_clip_cases
from tests.fake_env import PointEnv

EPS32 = float(np.finfo(np.float32).eps)
NEW_KEYS = ("training/grad_norm", "training/grad_norm_max", "training/grad_clip_share", "training/skipped_updates")


def _tensors(rng, sizes, scale=1.0):
    return [(scale * rng.standard_normal(n)).astype(np.float32) for n in sizes]


def _make(sizes, p0, lr=1e-2, max_grad_norm=1.0):
    params = [torch.tensor(x.copy()) for x in p0]
    flat = FlatGrads(params)
    return params, flat, optim.ClippedAdam(params, flat, lr=lr, max_grad_norm=max_grad_norm)


def _bits(opt, params):
    return [p.detach().numpy().copy().view(np.uint32) for p in params] + [opt.exp_avg.numpy().copy().view(np.uint32),
                                                                         opt.exp_avg_sq.numpy().copy().view(np.uint32)]


# ---------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("max_norm", [0.05, 1e6])
def test_reference_matches_torch_clip_and_adam_in_float64(max_norm):
    """Three steps of clip_grad_norm_ + torch.optim.Adam in float64 against the restated rule.  torch scales by max / (norm + 1e-6) and
    forms its norm in float64 where the rule rounds it to float32 and divides in float32: a relative difference of the scale of at most
    1e-6 / norm + 2 eps32 (norm ~ 5 here), which the update carries at most once per step into values of size <= 1."""
    rng = np.random.default_rng(0)
    sizes = [7, 12, 1, 5]
    p0 = [x.astype(np.float64) for x in _tensors(rng, sizes)]
    tp = [torch.tensor(x.copy(), dtype=torch.float64, requires_grad=True) for x in p0]
    topt = torch.optim.Adam(tp, lr=1e-2, betas=(0.9, 0.999), eps=1e-8)
    p, m, v, t = p0, [np.zeros(n) for n in sizes], [np.zeros(n) for n in sizes], 0
    for step in range(3):
        g = [x.astype(np.float64) for x in _tensors(rng, sizes)]
        for q, gg in zip(tp, g):
            q.grad = torch.tensor(gg.copy())
        torch.nn.utils.clip_grad_norm_(tp, max_norm)
        topt.step()
        p, m, v, t, info = optim.clipped_adam_reference(p, g, m, v, t, lr=1e-2, max_grad_norm=max_norm)
        assert info["skipped"] is False and (info["scale"] < 1.0) == (max_norm < 1.0)
        tol = (step + 1) * 1e-2 * (1e-6 + 4 * EPS32) if max_norm < 1.0 else 1e-13
        for k in range(len(sizes)):
            np.testing.assert_allclose(p[k], tp[k].detach().numpy(), rtol=0, atol=tol)
            st = topt.state[tp[k]]
            np.testing.assert_allclose(m[k], st["exp_avg"].numpy(), rtol=0, atol=max(tol * 100, 1e-13))
    assert t == 3


# ---------------------------------------------------------------------------------------------- the CPU ClippedAdam against the reference
def _run_against_reference(sizes, g, max_norm, t0, lr=1e-2, seed=1):
    rng = np.random.default_rng(seed)
    p0 = _tensors(rng, sizes)
    params, flat, opt = _make(sizes, p0, lr=lr, max_grad_norm=max_norm)
    n = sum(sizes)
    m0 = (0.1 * rng.standard_normal(n)).astype(np.float32) if t0 else np.zeros(n, np.float32)
    v0 = (0.01 * rng.random(n)).astype(np.float32) if t0 else np.zeros(n, np.float32)
    opt.load_state_dict({"t": t0, "exp_avg": torch.tensor(m0), "exp_avg_sq": torch.tensor(v0)})
    flat.flat.copy_(torch.tensor(np.concatenate(g)))
    opt.step()
    ref = grad_clip_cases.reference_step(np.concatenate(p0), np.concatenate(g), m0, v0, t0, lr, max_norm)
    assert opt.t == ref["t"] and not ref["skipped"]
    # per element, within the bound counted from the rule's roundings (tests/grad_clip_cases.py)
    got_p = np.concatenate([p.detach().numpy() for p in params])
    sh = grad_clip_cases.shares(got_p, opt.exp_avg.numpy(), opt.exp_avg_sq.numpy(), ref)
    print("t0 %d max_norm %g: largest share of the bound p %.3f m %.3f v %.3f" % (t0, max_norm, *sh))
    assert max(sh) <= 1.0, sh
    info = dict(norm=ref["norm"], scale=ref["scale"])
    return opt, info


@pytest.mark.parametrize("t0", [0, 1, 999])                 # the step taken is t = 1, 2, 1000
@pytest.mark.parametrize("max_norm", [0.5, 1e3, float("inf")])
def test_cpu_step_matches_reference(t0, max_norm):
    rng = np.random.default_rng(5)
    sizes = [3, 4, 5, 1, 17]
    g = _tensors(rng, sizes)
    opt, info = _run_against_reference(sizes, g, max_norm, t0)
    st = opt.stats(clear=False)
    assert st["applied_updates"] == 1 and st["skipped_updates"] == 0
    assert st["grad_clip_share"] == (1.0 if max_norm == 0.5 else 0.0)
    assert st["grad_norm"] == st["grad_norm_max"] == info["norm"]


def test_threshold_equal_to_the_norm_does_not_clip():
    """g = [3, 4], max_grad_norm = 5: norm <= max, the gradient is used as it is -- the same bits as max_grad_norm = inf."""
    g = [np.array([3.0, 4.0], np.float32)]
    a, info = _run_against_reference([2], g, 5.0, 0)
    b, _ = _run_against_reference([2], g, float("inf"), 0)
    assert info["norm"] == 5.0 and info["scale"] == 1.0
    assert a.stats()["grad_clip_share"] == 0.0
    assert np.array_equal(a.exp_avg.numpy().view(np.uint32), b.exp_avg.numpy().view(np.uint32))
    assert np.array_equal(a.params[0].detach().numpy().view(np.uint32), b.params[0].detach().numpy().view(np.uint32))
    c, info = _run_against_reference([2], g, 4.999, 0)
    assert info["scale"] < 1.0 and c.stats()["grad_clip_share"] == 1.0


# ---------------------------------------------------------------------------------------------- skip
@pytest.mark.parametrize("where", ["nan_first", "inf_last", "both"])
def test_non_finite_gradient_skips_the_update(where):
    rng = np.random.default_rng(9)
    sizes = [5, 1, 6]
    p0 = _tensors(rng, sizes)
    params, flat, opt = _make(sizes, p0, max_grad_norm=float("inf"))
    g1 = np.concatenate(_tensors(rng, sizes))
    flat.flat.copy_(torch.tensor(g1)); opt.step()
    before, t_before = _bits(opt, params), opt.t
    bad = g1.copy()
    if where in ("nan_first", "both"):
        bad[0] = np.nan
    if where in ("inf_last", "both"):
        bad[-1] = -np.inf
    flat.flat.copy_(torch.tensor(bad)); opt.step()
    after = _bits(opt, params)
    assert all(np.array_equal(x, y) for x, y in zip(before, after)) and opt.t == t_before == 1
    st = opt.stats(clear=False)
    assert st["skipped_updates"] == 1 and st["applied_updates"] == 1 and math.isfinite(st["grad_norm"]) and math.isfinite(st["grad_norm_max"])
    # the next finite step continues with the old t: it equals the second step of a run that never saw the bad gradient
    g2 = np.concatenate(_tensors(rng, sizes))
    flat.flat.copy_(torch.tensor(g2)); opt.step()
    params_b, flat_b, opt_b = _make(sizes, p0, max_grad_norm=float("inf"))
    for g in (g1, g2):
        flat_b.flat.copy_(torch.tensor(g)); opt_b.step()
    assert opt.t == opt_b.t == 2
    assert all(np.array_equal(x, y) for x, y in zip(_bits(opt, params), _bits(opt_b, params_b)))
    st = opt.stats(clear=True)
    assert st["skipped_updates"] == 1 and st["applied_updates"] == 2
    assert opt.stats()["skipped_updates"] == 0 and opt.stats()["applied_updates"] == 0


# ---------------------------------------------------------------------------------------------- arguments, state_dict
@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), "1.0", True, float("-inf")])
def test_max_grad_norm_argument_is_checked(bad):
    with pytest.raises(ValueError):
        optim.check_max_grad_norm(bad)
    with pytest.raises(ValueError):
        ppo.train(environment=PointEnv(8), num_timesteps=100, episode_length=10, num_envs=8, batch_size=8, num_minibatches=1, max_grad_norm=bad)


def test_constructor_checks():
    p = [torch.zeros(3), torch.zeros(4)]
    flat = FlatGrads(p)
    assert optim.check_max_grad_norm(float("inf")) == float("inf") and optim.check_max_grad_norm(2) == 2.0
    with pytest.raises(ValueError):
        optim.ClippedAdam(p, torch.zeros(8), lr=1e-3, max_grad_norm=1.0)            # flat of another size
    with pytest.raises(ValueError):
        optim.ClippedAdam([torch.zeros(1) for _ in range(65)], torch.zeros(65), lr=1e-3, max_grad_norm=1.0)
    with pytest.raises(ValueError):
        optim.ClippedAdam(p, flat, lr=1e-3, max_grad_norm=1.0, betas=(1.0, 0.999))
    opt = optim.ClippedAdam(p, flat, lr=1e-3, max_grad_norm=1.0)
    assert len(opt.state) == 0
    opt.step()
    assert len(opt.state) > 0
    with pytest.raises(ValueError):
        opt.load_state_dict({"t": 1, "exp_avg": torch.zeros(3), "exp_avg_sq": torch.zeros(3)})


def test_state_dict_round_trip():
    rng = np.random.default_rng(2)
    sizes = [4, 9]
    p0 = _tensors(rng, sizes)
    gs = [np.concatenate(_tensors(rng, sizes, scale=3.0)) for _ in range(4)]
    params, flat, opt = _make(sizes, p0, max_grad_norm=1.0)
    for g in gs[:2]:
        flat.flat.copy_(torch.tensor(g)); opt.step()
    sd = opt.state_dict()
    mid = [p.detach().clone() for p in params]
    for g in gs[2:]:
        flat.flat.copy_(torch.tensor(g)); opt.step()
    params_b = [x.clone() for x in mid]
    flat_b = FlatGrads(params_b)
    opt_b = optim.ClippedAdam(params_b, flat_b, lr=1e-2, max_grad_norm=1.0)
    opt_b.load_state_dict(sd)
    assert opt_b.t == 2 and len(opt_b.state) > 0 and sd["hyper"]["max_grad_norm"] == 1.0
    for g in gs[2:]:
        flat_b.flat.copy_(torch.tensor(g)); opt_b.step()
    assert all(np.array_equal(x, y) for x, y in zip(_bits(opt, params), _bits(opt_b, params_b)))
    assert opt.stats() == opt_b.stats()                   # the counters travel with the state


# ---------------------------------------------------------------------------------------------- ppo.train
_TRAIN = dict(num_timesteps=16 * 5 * 2 * 3, episode_length=20, num_envs=16, batch_size=16, num_minibatches=2, unroll_length=5,
              num_updates_per_batch=2, num_evals=2, num_eval_envs=8, learning_rate=3e-3, normalize_observations=True, seed=0)


def test_train_reports_the_new_metrics_only_with_the_option():
    seen = {}
    out = ppo.train(environment=PointEnv(16), max_grad_norm=0.5, return_training_state=True, progress_fn=lambda n, m: seen.update(m), **_TRAIN)
    for k in NEW_KEYS:
        assert k in seen and math.isfinite(seen[k]), (k, seen)
    assert seen["training/grad_norm"] > 0 and seen["training/grad_norm_max"] >= seen["training/grad_norm"]
    assert 0.0 <= seen["training/grad_clip_share"] <= 1.0 and seen["training/skipped_updates"] == 0
    ts = out[3]
    assert isinstance(ts.optimizer_state, optim.ClippedAdam) and len(ts.optimizer_state.state) > 0
    assert ts.optimizer_state.t == 3 * 2 * 2                                  # training steps x epochs x minibatches
    assert all(torch.isfinite(p).all() for p in out[1][1].parameters())
    seen = {}
    ppo.train(environment=PointEnv(16), progress_fn=lambda n, m: seen.update(m), **_TRAIN)
    assert not any(k in seen for k in NEW_KEYS) and "training/total_loss" in seen


class NaNRewardEnv(PointEnv):
    """PointEnv whose reward is NaN on env 3 at its 7th step (of the instance): one bad minibatch in the second unroll."""

    def __init__(self, num_envs=8, device="cpu"):
        super().__init__(num_envs, device)
        self.calls = 0

    def with_num_envs(self, n, device=None):
        return NaNRewardEnv(n, device or self.device) if n == self.num_envs else PointEnv(n, device or self.device)

    def step(self, state, action):
        s = super().step(state, action)
        self.calls += 1
        if self.calls == 7:
            r = s.reward.clone()
            r[3] = float("nan")
            s = s.replace(reward=r)
        return s


def test_nan_reward_ruins_the_default_run_and_is_skipped_with_the_option():
    cfg = dict(_TRAIN, num_evals=4)                       # one training step per report: progress_fn sees every step's counters
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, params, _ = ppo.train(environment=NaNRewardEnv(16), **cfg)
    assert not all(torch.isfinite(p).all() for p in params[1].parameters())    # the test is sharp: without the option the NaN spreads
    seen = {"skipped": 0.0}

    def progress(n, m):
        seen["skipped"] += m.get("training/skipped_updates", 0.0)
        seen.update({k: v for k, v in m.items() if k != "training/skipped_updates"})

    with pytest.warns(RuntimeWarning, match="skipped"):
        _, params, _ = ppo.train(environment=NaNRewardEnv(16), max_grad_norm=float("inf"), progress_fn=progress, **cfg)
    assert all(torch.isfinite(p).all() for p in params[1].parameters())
    assert seen["skipped"] > 0 and seen["training/grad_clip_share"] == 0.0


def _dp_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    try:
        seen = {}
        _, params, _ = ppo.train(environment=PointEnv(16), num_timesteps=32 * 5 * 2 * 2, episode_length=20, num_envs=32,
                                 batch_size=32, num_minibatches=2, unroll_length=5, num_updates_per_batch=2, num_evals=2,
                                 num_eval_envs=8, normalize_observations=True, seed=3, max_grad_norm=0.3,
                                 progress_fn=lambda n, m: seen.update(m))
        vec = torch.cat([p.detach().reshape(-1) for p in params[1].parameters()])
        out[rank] = (vec.numpy().copy(), params[0].mean.numpy().copy(), {k: seen.get(k) for k in NEW_KEYS})
    finally:
        torch.distributed.destroy_process_group()


def test_two_gloo_ranks_end_with_identical_parameters():
    """The clip acts on the all-reduced gradient, so both ranks compute the same norm, the same scale and the same update."""
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    out = mgr.dict()
    port = 31500 + os.getpid() % 2000
    mp.spawn(_dp_worker, args=(2, port, out), nprocs=2, join=True)
    (p0, m0, k0), (p1, m1, _) = out[0], out[1]
    np.testing.assert_allclose(p0, p1, rtol=0, atol=1e-7)
    np.testing.assert_allclose(m0, m1, rtol=0, atol=1e-7)
    assert np.isfinite(p0).all() and all(k0[k] is not None and math.isfinite(k0[k]) for k in NEW_KEYS)    # progress_fn runs on rank 0
