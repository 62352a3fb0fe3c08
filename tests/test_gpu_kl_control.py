"""GPU: the DIAG instances of the PPO loss kernels (`rr_ppo_loss_diag`), the KL instance of the clipped Adam step's finalisation
(`rr_clipped_adam_step_kl`), a captured graph of both, and `ppo.train` with `learner_diagnostics`, `target_kl` and the KL-adaptive learning
rate at 64 envs.  tests/kl_control_cases.py holds the rule's case table and the shapes; tests/test_kl_control_cpu.py the CPU side."""
import logging
import math

import numpy as np
import pytest
import torch

from tests import grad_clip_cases
from tests import kl_control_cases as cases
from tests import ppo_batches as pb
from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIGS = ("approx_kl", "clip_fraction", "explained_variance", "entropy")


def _hip_sampler(logits, eps):
    from rodent_amd import hip
    _, raw, lp = hip.policy_sample(logits.to(DEV), eps.to(DEV), 0.001)
    return raw, lp


def _torch_figures(batch, T, B, A, dtype, device):
    from rodent_amd.training.agents.ppo import losses
    data, logits, values, noise, idx = batch
    c = lambda x: x.to(dtype).to(device)
    rows = idx if idx is not None else torch.arange(B)
    mbd = {k: c(data[k][rows]).transpose(0, 1) for k in ("raw_action", "log_prob", "reward", "discount", "truncation")}
    v = c(values).reshape(T + 1, B)
    _, m = losses.compute_ppo_loss(c(logits)[:T * B].reshape(T, B, 2 * A), v[:T], v[T], mbd, pb._fixed_noise_dist(A, noise), diagnostics=True, **pb.CFG)
    return {k: m[k].double().cpu().reshape(1) for k in FIGS}


def _device_batch(batch):
    data, logits, values, noise, idx = batch
    return ({k: v.to(DEV).contiguous() for k, v in data.items()}, logits.to(DEV), values.to(DEV), noise.to(DEV),
            idx.to(DEV) if idx is not None else None)


# ---------------------------------------------------------------------------------------------- the diagnostic kernels
@pytest.mark.parametrize("use_idx", [True, False], ids=["idx", "rows"])
@pytest.mark.parametrize("T,B,A", cases.DIAG_SHAPES)
def test_diag_instances_against_the_plain_ones_and_float64(T, B, A, use_idx):
    """Gradients and the four metrics bitwise those of rr_ppo_loss; KL, explained variance and entropy within the suite's criterion of
    float64 (torch float32 as the yardstick); the clip count within the rows near a clip edge of the float64 count; the accumulators."""
    from rodent_amd import hip
    label = f"T={T} B={B} A={A} idx={use_idx}"
    batch = cases.diag_batch(T, B, A, use_idx, sampler=_hip_sampler)
    dd, lg, vl, nz, ix = _device_batch(batch)
    gl0, gv0, m0 = hip.ppo_loss(lg, vl, dd, ix, nz, T, normalize_advantage=True, out={}, **pb.CFG)
    diag = torch.zeros(hip.DIAG_DOUBLES, dtype=torch.float64, device=DEV)
    slots = torch.full((4,), -1.0, device=DEV)
    out = {}
    gl1, gv1, m1 = hip.ppo_loss(lg, vl, dd, ix, nz, T, normalize_advantage=True, out=out, diag=diag, kl_out=slots[:1], **pb.CFG)
    torch.cuda.synchronize()
    for a, b in ((gl0, gl1), (gv0, gv1), (m0, m1)):
        assert a.data_ptr() != b.data_ptr() and torch.equal(a.view(torch.int32), b.view(torch.int32)), label
    d = diag.cpu().numpy().copy()
    got = {k: torch.tensor([d[i]], dtype=torch.float64) for i, k in enumerate(FIGS)}
    f64, f32 = _torch_figures(batch, T, B, A, torch.float64, "cpu"), _torch_figures(batch, T, B, A, torch.float32, DEV)
    want = cases.numpy_diagnostics(*batch, T, B, A, pb.CFG)
    n = T * B
    print(f"{label}: kernel kl {d[0]:.6e} clip {d[1]:.6f} ev {d[2]:.6f} entropy {d[3]:.6f} | float64 kl {want['approx_kl']:.6e} "
          f"clip {want['clip_fraction']:.6f} ev {want['explained_variance']:.6f} entropy {want['entropy']:.6f}")
    assert d[0] >= 0.0 and 0.0 <= d[1] <= 1.0 and all(math.isfinite(x) for x in d[:4])
    # the slot the optimiser reads: the KL rounded to float32 once; the other slots untouched
    assert slots.cpu().tolist() == [float(np.float32(d[0])), -1.0, -1.0, -1.0]
    # accumulators after one call, and after a second one (x + x is exact)
    assert d[hip.DIAG_COUNT] == 1 and [d[hip.DIAG_KL_SUM], d[hip.DIAG_KL_MAX], d[hip.DIAG_CLIP_SUM], d[hip.DIAG_EV_SUM], d[hip.DIAG_ENT_SUM]] == \
        [d[0], d[0], d[1], d[2], d[3]]
    hip.ppo_loss(lg, vl, dd, ix, nz, T, normalize_advantage=True, out=out, diag=diag, kl_out=slots[:1], **pb.CFG)
    d2 = diag.cpu().numpy()
    assert d2[hip.DIAG_COUNT] == 2 and d2[hip.DIAG_KL_MAX] == d[0] and np.array_equal(d2[:4], d[:4])
    assert [d2[hip.DIAG_KL_SUM], d2[hip.DIAG_CLIP_SUM], d2[hip.DIAG_EV_SUM], d2[hip.DIAG_ENT_SUM]] == [2 * d[0], 2 * d[1], 2 * d[2], 2 * d[3]]
    # clip count: exact up to the rows whose float64 rho lies within EDGE of a clip edge
    near = cases.edge_rows(want["rho"], pb.CFG["clipping_epsilon"])
    print(f"{label}: clipped samples kernel {round(d[1] * n)} float64 {round(want['clip_fraction'] * n)} of {n}, {near} rows near an edge")
    assert abs(d[1] * n - round(d[1] * n)) < 1e-6 and abs(round(d[1] * n) - round(want["clip_fraction"] * n)) <= near
    if (T, B, A) == cases.DIAG_SHAPES[-1]:
        data, logits, values, _, idx = batch
        rho, adv = pb.rho_and_advantage64(data, logits, values, idx, T, B, A, True, pb.CFG)
        kept = pb.assert_coverage(rho, adv, pb.CFG["clipping_epsilon"], T, B, A, label)
        assert int((~kept).sum()) == near <= 0.01 * n
    for k in ("approx_kl", "explained_variance", "entropy"):
        assert abs(float(f64[k]) - want[k]) <= 1e-12 * max(1.0, abs(want[k]))
    for k in ("approx_kl", "explained_variance", "entropy"):
        if float(f64[k].abs().max()) == 0.0:                 # one sample: no variance, explained variance is 0 by definition -- exactly
            assert float(got[k]) == 0.0 and float(f32[k]) == 0.0, (label, k)
            continue
        pb.assert_global_criterion(k, got[k], f32[k], f64[k], label)


def test_refusals_of_the_new_entries():
    from rodent_amd import hip
    T, B, A = 3, 5, 30
    dd, lg, vl, nz, ix = _device_batch(cases.diag_batch(T, B, A, True))
    with pytest.raises(ValueError):
        hip.ppo_loss(lg, vl, dd, ix, nz, T, out={}, kl_out=torch.zeros(1, device=DEV), **pb.CFG)                       # kl_out without diag
    with pytest.raises(ValueError):
        hip.ppo_loss(lg, vl, dd, ix, nz, T, out={}, diag=torch.zeros(8, dtype=torch.float64, device=DEV), **pb.CFG)    # a short block
    buf = torch.zeros(8, device=DEV)
    g, m, v = (torch.zeros(8, device=DEV) for _ in range(3))
    kw = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, max_grad_norm=1.0)
    with pytest.raises(ValueError):
        hip.ClippedAdamBuffers([buf], g, m, v, kl=torch.zeros(2, device=DEV), kl_cfg=cases.BOTH, **kw)
    with pytest.raises(ValueError):
        hip.ClippedAdamBuffers([buf], g, m, v, kl=torch.zeros(1, device=DEV), kl_cfg=(1.0, 2.0), **kw)
    # the shared checks report under the name of the entry that was called
    b65 = torch.zeros(65, device=DEV)
    g65, m65, v65 = (torch.zeros(65, device=DEV) for _ in range(3))
    many = hip.ClippedAdamBuffers([b65[i:i + 1] for i in range(65)], g65, m65, v65, kl=torch.zeros(1, device=DEV), kl_cfg=cases.BOTH, **kw)
    with pytest.raises(RuntimeError, match="rr_clipped_adam_step_kl: more than 64 tensors"):
        many.step()
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0 and float(b65.abs().sum()) == 0.0


# ---------------------------------------------------------------------------------------------- the decision kernel
SIZES = [5, 1031, 3]                # a segment off the float4 grid with two blocks of the update between two short odd ones


class Case:
    """One optimiser's buffers on SIZES (layouts as in tests/test_gpu_grad_clip.py: 'packed' = parameters laid out like the gradient,
    'shifted' = one element further, so no parameter address is congruent with its gradient segment), with the KL slot and settings."""

    def __init__(self, layout, lr, kl_cfg, p0, m0, v0, t0, stopped=False, sizes=SIZES, g=None):
        from rodent_amd import hip
        from rodent_amd.training import optim
        self.n = sum(sizes)
        shift = {"packed": 0, "shifted": 1}[layout]
        self.pbuf = torch.zeros(self.n + 4, device=DEV)
        off = np.concatenate([[0], np.cumsum(sizes)])
        self.params = [self.pbuf[shift + off[k]:shift + off[k + 1]] for k in range(len(sizes))]
        self.pview = self.pbuf[shift:shift + self.n]
        self.g = torch.zeros(self.n, device=DEV) if g is None else g
        self.m, self.v = torch.zeros(self.n, device=DEV), torch.zeros(self.n, device=DEV)
        self.pview.copy_(torch.from_numpy(p0)); self.m.copy_(torch.from_numpy(m0)); self.v.copy_(torch.from_numpy(v0))
        self.kl = torch.zeros(4, device=DEV)
        kw = dict(kl=self.kl[:1], kl_cfg=kl_cfg) if kl_cfg is not None else {}
        self.b = hip.ClippedAdamBuffers(self.params, self.g, self.m, self.v, lr=lr, b1=grad_clip_cases.B1, b2=grad_clip_cases.B2,
                                        eps=grad_clip_cases.EPS, max_grad_norm=float("inf"), **kw)
        self.b.state[optim.ST_T] = float(t0)
        if stopped:
            self.b.state[optim.ST_STOP] = 1.0
            self.b.state[optim.ST_SKIP] = 1.0

    def step(self, g=None, kl=None):
        if g is not None:
            self.g.copy_(torch.from_numpy(np.ascontiguousarray(g, dtype=np.float32)))
        if kl is not None:
            self.kl[0] = kl
        self.b.step()

    def bits(self):
        torch.cuda.synchronize()
        return [self.pbuf.cpu().numpy().view(np.uint32), self.m.cpu().numpy().view(np.uint32), self.v.cpu().numpy().view(np.uint32)]

    def blocks(self):
        torch.cuda.synchronize()
        return self.b.state.cpu().numpy().copy(), self.b.cfg.cpu().numpy().copy()


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def adam_inputs():
    rng = np.random.default_rng(0)
    n = sum(SIZES)
    return dict(p0=rng.standard_normal(n).astype(np.float32), g=rng.standard_normal(n).astype(np.float32),
                m0=(0.1 * rng.standard_normal(n)).astype(np.float32), v0=(0.01 * rng.random(n)).astype(np.float32))


@pytest.mark.parametrize("layout", ["packed", "shifted"])
@pytest.mark.parametrize("case", cases.RULE_TABLE, ids=[c[0] for c in cases.RULE_TABLE])
def test_decision_kernel_follows_the_rule_table(case, layout, adam_inputs):
    """Every case of the CPU rule table through rr_clipped_adam_step_kl: lr, the flags and the counters bit-equal to the host function;
    a step that is not applied keeps every bit of p, m, v and t; an applied one has the bits of rr_clipped_adam_step at the adapted lr."""
    from rodent_amd.training import optim
    _, kl, lr, stopped, finite, cfg, table_want = case
    x = adam_inputs
    want_lr, want_stop, want_applied = optim.kl_control_rule(kl, lr, stopped, stop_threshold=cfg[0], desired_kl=cfg[1], lr_lo=cfg[2], lr_hi=cfg[3],
                                                             norm_finite=finite)
    assert (want_lr, want_stop, want_applied) == table_want
    g = x["g"].copy()
    if not finite:
        g[6] = np.nan
    c = Case(layout, lr, cfg, x["p0"], x["m0"], x["v0"], 4, stopped)
    before = c.bits()
    c.step(g, kl)
    st, cf = c.blocks()
    assert cf[0] == want_lr and np.float64(cf[0]).view(np.uint64) == np.float64(want_lr).view(np.uint64)
    assert list(cf[1:5]) == [grad_clip_cases.B1, grad_clip_cases.B2, grad_clip_cases.EPS, float("inf")]
    assert st[optim.ST_STOP] == (1.0 if want_stop else 0.0)
    assert st[optim.ST_STOPPED] == (1.0 if want_stop else 0.0)
    assert st[optim.ST_APPLIED] == (1.0 if want_applied else 0.0)
    assert st[optim.ST_SKIPPED] == (1.0 if not want_applied and not want_stop else 0.0)
    assert st[optim.ST_SKIP] == (0.0 if want_applied else 1.0)
    if not stopped:                                          # the KL the decision saw (a sticky stop reads nothing)
        assert st[optim.ST_KL] == kl or (math.isnan(kl) and math.isnan(st[optim.ST_KL]))
    if not want_applied:
        assert st[optim.ST_T] == 4 and _same(before, c.bits())
        if want_stop:                                        # a stop touches nothing else, the norm statistics included
            assert st[optim.ST_NORM] == 0.0 and st[optim.ST_NORM_SUM] == 0.0 and st[optim.ST_NORM_MAX] == 0.0
        return
    plain = Case(layout, want_lr, None, x["p0"], x["m0"], x["v0"], 4)
    plain.step(g)
    assert st[optim.ST_T] == 5 and _same(plain.bits(), c.bits())
    pst, _ = plain.blocks()
    assert np.array_equal(pst[[optim.ST_NORM, optim.ST_SCALE, optim.ST_BC1, optim.ST_BC2, optim.ST_NORM_SUM, optim.ST_NORM_MAX]],
                          st[[optim.ST_NORM, optim.ST_SCALE, optim.ST_BC1, optim.ST_BC2, optim.ST_NORM_SUM, optim.ST_NORM_MAX]])


def test_clipped_adam_on_the_gpu_reads_the_tail_of_flat_grads(adam_inputs):
    """`ClippedAdam` on a `FlatGrads(params, extra=4)`: the norm never sees the tail, begin_training_step clears the flag."""
    from rodent_amd.training import optim
    from rodent_amd.training.distributed import FlatGrads
    params = [torch.ones(5, device=DEV), torch.ones(3, 4, device=DEV)]
    flat = FlatGrads(params, extra=4)
    opt = optim.ClippedAdam(params, flat, lr=cases.LR, max_grad_norm=float("inf"), target_kl=cases.TARGET, desired_kl=cases.DES,
                            learning_rate_bounds=(cases.LO, cases.HI))
    flat.flat[:17] = 2.0
    flat.tail.copy_(torch.tensor([0.5, 1e30, 1e30, 1e30], device=DEV))     # kl 0.5: lr / 1.5; the other slots would blow the norm up
    opt.step()
    st = opt.stats(clear=False)
    assert st["grad_norm"] == float(np.float32(np.sqrt(17 * 4.0))) and opt.learning_rate == cases.LR / 1.5 and opt.t == 1 and not opt.stopped
    flat.tail[0] = 2.0
    opt.step()
    assert opt.stopped and opt.t == 1 and opt.stats(clear=False)["stopped_updates"] == 1
    sd = opt.state_dict()
    assert sd["kl_stop"] is True and sd["lr"] == cases.LR / 1.5
    opt.begin_training_step()
    assert not opt.stopped
    flat.tail[0] = 0.5
    opt.step()
    assert opt.t == 2 and opt.stats()["stopped_updates"] == 1 and opt.stats()["stopped_updates"] == 0


# ---------------------------------------------------------------------------------------------- graph replay
def test_captured_loss_and_step_replayed_equal_eager_calls(adam_inputs):
    """Loss-with-diagnostics plus the KL step, captured once and replayed seven times on logits that move away from the behaviour policy,
    against seven eager calls: the gradient the step consumes is the loss kernel's d loss / d logits, the KL it decides on is the slot the
    metrics kernel wrote.  The learning rate goes up twice, holds, comes down twice; the sixth update stops, the seventh meets the flag.
    Parameters, moments, both device blocks of the optimiser, the diagnostics block and the metrics are equal bit for bit."""
    from rodent_amd import hip
    from rodent_amd.training import optim
    T, B, A = 3, 5, 30
    data, logits, values, noise, idx = pb.onpolicy_batch(T, B, B + 3, A, seed=77, step=0.0, sampler=_hip_sampler)
    pert = torch.randn(logits.shape, generator=torch.Generator().manual_seed(5))
    seq = [logits + s * pert for s in (0.002, 0.004, 0.012, 0.04, 0.1, 0.3, 0.0)]
    kls = [cases.numpy_diagnostics(data, lg, values, noise, idx, T, B, A, pb.CFG)["approx_kl"] for lg in seq]
    print("float64 KL of the sequence:", " ".join(f"{k:.3e}" for k in kls))
    assert all(kls[i + 1] > 4 * kls[i] for i in range(1, 5)) and kls[0] < 0.4 * kls[2]
    desired = kls[2]                                         # below half of it twice, inside once, above twice it twice
    assert kls[1] < 0.45 * desired and kls[3] > 2.2 * desired
    target = math.sqrt(kls[4] * kls[5]) / optim.KL_STOP_FACTOR
    lr0 = 1e-3
    cfg = (optim.KL_STOP_FACTOR * target, desired, 1e-5, 1e-2)
    n = logits.numel()
    rng = np.random.default_rng(8)
    p0, z = rng.standard_normal(n).astype(np.float32), np.zeros(n, np.float32)
    dd, _, vl, nz, ix = _device_batch((data, logits, values, noise, idx))

    def make():
        lg = torch.zeros_like(logits, device=DEV)
        out, diag = {}, torch.zeros(hip.DIAG_DOUBLES, dtype=torch.float64, device=DEV)
        hip.ppo_loss(lg, vl, dd, ix, nz, T, out=out, diag=diag, **pb.CFG)        # allocates the persistent buffers
        diag.zero_()
        c = Case("packed", lr0, cfg, p0, z, z, 0, sizes=[n - 7, 7], g=out["grad_logits"].view(-1))

        def run():
            hip.ppo_loss(lg, vl, dd, ix, nz, T, out=out, diag=diag, kl_out=c.kl[:1], **pb.CFG)
            c.b.step()
        return lg, out, diag, c, run

    lg_e, out_e, diag_e, ce, run_e = make()
    seen = []
    for x in seq:
        lg_e.copy_(x)
        run_e()
        seen.append((float(ce.kl[0]), float(ce.b.cfg[0]), float(ce.b.state[optim.ST_STOP])))
    lg_r, out_r, diag_r, cr, run_r = make()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        run_r()
    for x in seq:
        lg_r.copy_(x)
        graph.replay()
    assert _same(ce.bits(), cr.bits())
    (st_e, cf_e), (st_r, cf_r) = ce.blocks(), cr.blocks()
    assert np.array_equal(st_e.view(np.uint64), st_r.view(np.uint64)) and np.array_equal(cf_e.view(np.uint64), cf_r.view(np.uint64))
    assert np.array_equal(diag_e.cpu().numpy().view(np.uint64), diag_r.cpu().numpy().view(np.uint64))
    assert torch.equal(out_e["metrics"].view(torch.int32), out_r["metrics"].view(torch.int32))
    assert torch.equal(out_e["grad_logits"].view(torch.int32), out_r["grad_logits"].view(torch.int32))
    # the trajectory is the host rule's on the KLs the kernel wrote
    lr, stop = lr0, False
    for i, (kl, lr_seen, stop_seen) in enumerate(seen):
        lr, stop, _ = optim.kl_control_rule(kl, lr, stop, stop_threshold=cfg[0], desired_kl=cfg[1], lr_lo=cfg[2], lr_hi=cfg[3])
        assert lr == lr_seen and stop == bool(stop_seen), (i, kl, lr, lr_seen)
    assert [s[1] for s in seen[:5]] == [lr0 * 1.5, lr0 * 1.5 * 1.5, lr0 * 1.5 * 1.5, lr0 * 1.5 * 1.5 / 1.5, lr0 * 1.5 * 1.5 / 1.5 / 1.5]
    assert [s[2] for s in seen] == [0, 0, 0, 0, 0, 1, 1]
    assert st_r[optim.ST_T] == 5 and st_r[optim.ST_APPLIED] == 5 and st_r[optim.ST_STOPPED] == 2 and st_r[optim.ST_SKIPPED] == 0
    d = diag_r.cpu().numpy()
    assert d[hip.DIAG_COUNT] == 7 and float(np.float32(d[hip.DIAG_KL_MAX])) == max(s[0] for s in seen) == seen[5][0]


# ---------------------------------------------------------------------------------------------- ppo.train
_DIAG_KEYS = ("training/approx_kl", "training/approx_kl_max", "training/clip_fraction", "training/explained_variance", "training/entropy")


# A target the learner reaches by construction, whatever the data: without observation normalisation the first minibatch of a training step
# is on-policy (its KL is the float32 rounding of two log-probs, rho - 1 <= 1e-4 by tests/test_gpu_ppo_loss.py, so KL <= ~1e-8), and one Adam
# update at lr = 1e-3 moves every parameter by 1e-3, which shifts the logits by >= 1e-3 and the KL of the next minibatch far above 1.5e-6.
# So each training step applies its first update(s) and stops later in the same pass.
_REACHED = dict(target_kl=1e-6, learning_rate=1e-3, normalize_observations=False)


@pytest.mark.parametrize("option", ["diagnostics", "target_never", "target_reached", "adaptive"])
def test_ppo_train_with_each_option_at_64_envs(option, monkeypatch, caplog):
    """Two training steps (4 minibatches x 2 passes each) on the fused update with its captured graph, as test_gpu_grad_clip.py's train test.
    The first three updates run eagerly, the fourth is captured, every later one replays: the second training step is replays only."""
    from rodent_amd import envs
    from rodent_amd.training import optim
    from rodent_amd.training.agents.ppo import fused_update, train as ppo
    calls = {"update": 0, "applied": [], "stopped": [], "skipped": []}
    real_call, real_stats = fused_update.FusedUpdate.__call__, optim.ClippedAdam.stats

    def stats(self, clear=True):
        st = real_stats(self, clear)
        if clear:                                            # once per training step
            for k in ("applied", "stopped", "skipped"):
                calls[k].append(st.get(k + "_updates", 0))
        return st

    def update(self, *a, **k):
        calls["update"] += 1
        assert self.diag is not None
        return real_call(self, *a, **k)

    monkeypatch.setattr(fused_update.FusedUpdate, "__call__", update)
    monkeypatch.setattr(optim.ClippedAdam, "stats", stats)
    kw = {"diagnostics": dict(learner_diagnostics=True), "target_never": dict(target_kl=1e9), "target_reached": _REACHED,
          "adaptive": dict(learning_rate_schedule="adaptive_kl", desired_kl=0.01, learning_rate_bounds=(1e-5, 1e-2))}[option]
    kw = dict(dict(learning_rate=5e-5, normalize_observations=True), **kw)
    env = envs.get_environment("rodent", track_pos=util.synthetic_track(), num_envs=64, xml_path="rodent_optimized.xml", iterations=8,
                               ls_iterations=8, device=DEV)
    log = []
    with caplog.at_level(logging.WARNING):
        _, params, _, ts = ppo.train(environment=env, num_timesteps=10 ** 9, episode_length=150, num_envs=64, batch_size=64, num_minibatches=4,
                                     unroll_length=5, num_updates_per_batch=2, num_evals=3, num_eval_envs=0,
                                     entropy_cost=1e-3, discounting=0.97, seed=1, max_training_steps=2,
                                     return_training_state=True, progress_fn=lambda n, m: log.append(m), **kw)
    assert not [r for r in caplog.records if "graph capture failed" in r.getMessage()]
    m = log[-1]
    print(option, {k: m[k] for k in m if k.startswith("training/") and k not in ("training/sps", "training/walltime")},
          {k: v for k, v in calls.items()})
    for k in _DIAG_KEYS + ("training/total_loss",):
        assert k in m and math.isfinite(float(m[k])), (k, m)
    assert 0.0 <= m["training/approx_kl"] <= m["training/approx_kl_max"] and 0.0 <= m["training/clip_fraction"] <= 1.0
    assert m["training/explained_variance"] <= 1.0
    assert all(torch.isfinite(p).all() for p in params[1].parameters())
    assert calls["update"] == 4                              # three eager updates and the capture; everything after is a replay
    opt = ts.optimizer_state
    if option == "diagnostics":
        assert isinstance(opt, torch.optim.Adam) and "training/stopped_updates" not in m and "training/learning_rate" not in m
        return
    assert isinstance(opt, optim.ClippedAdam) and m["training/skipped_updates"] == 0
    if option == "target_never":
        assert opt.t == 16 and m["training/stopped_updates"] == 0 and not opt.stopped
    elif option == "target_reached":
        # each training step applies at least its first update, stops later in its first pass and leaves after that pass: 4 evaluated
        # updates per step.  The second step is replays only: applied updates followed by a stop under the captured graph
        assert opt.stopped and m["training/stopped_updates"] == calls["stopped"][1]
        for step in (0, 1):
            assert calls["applied"][step] >= 1 and calls["stopped"][step] >= 1 and calls["skipped"][step] == 0
            assert calls["applied"][step] + calls["stopped"][step] == 4
        assert 0 < opt.t == sum(calls["applied"]) < 16
        assert m["training/approx_kl_max"] > 1.5e-6
    else:
        assert opt.t == 16 and 1e-5 <= m["training/learning_rate"] <= 1e-2 and m["training/learning_rate"] == opt.learning_rate
        assert m["training/learning_rate"] != 5e-5            # the KL of these steps (~0.04, the normaliser's shift) is above 2 x 0.01: it moved


def _two_rank_worker(rank, world, port, out):
    import os
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), RR_PPO_GRAPH="1")
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from rodent_amd import envs
        from rodent_amd.training import distributed as D
        from rodent_amd.training.agents.ppo import train as ppo
        torch.cuda.set_device(0)
        # the all-reduce runs eagerly between the two graphs: read the KL slot on either side of it
        kls, real_pmean = [], D.FlatGrads.pmean_

        def pmean(self):
            local = float(self.tail[0])
            real_pmean(self)
            kls.append((local, float(self.tail[0])))

        D.FlatGrads.pmean_ = pmean
        env = envs.get_environment("rodent", track_pos=util.synthetic_track(), num_envs=64, xml_path="rodent_optimized.xml",
                                   iterations=8, ls_iterations=8, device=DEV)
        log = []
        _, params, _, ts = ppo.train(environment=env, num_timesteps=128 * 4 * 4 * 2, episode_length=150, num_envs=128, batch_size=128,
                                     num_minibatches=4, unroll_length=4, num_updates_per_batch=3, num_evals=1, num_eval_envs=0,
                                     entropy_cost=1e-3, discounting=0.97, seed=3, learning_rate_schedule="adaptive_kl", desired_kl=1e-6,
                                     learning_rate_bounds=(1e-5, 1e-2), return_training_state=True,
                                     progress_fn=lambda n, m: log.append(dict(m)), **_REACHED)
        vec = torch.cat([p.detach().reshape(-1) for p in list(params[1].parameters()) + list(ts.params.value.parameters())]).cpu()
        opt = ts.optimizer_state
        out[rank] = (vec.numpy().copy(), opt.t, opt.learning_rate, sum(m.get("training/stopped_updates", 0) for m in log), kls,
                     opt.stats(clear=False)["last_kl"])
    finally:
        torch.distributed.destroy_process_group()


def test_two_ranks_take_the_same_decisions_from_an_all_reduced_kl():
    """Two processes sharing the GPU, each with its own envs: graph A ends with the rank's KL in the tail of the flat buffer, the eager
    all-reduce averages it with the gradients, graph B decides -- on every rank from the same bits.  `_REACHED` makes every training step
    apply its first update(s), at a learning rate the schedule has raised (the on-policy KL lies below desired_kl / 2), and then stop; the
    second step is replays only.  The ranks measure different KLs, so a decision taken on a rank's own KL would not be the same decision."""
    import os
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    out = mgr.dict()
    port = 36500 + os.getpid() % 2000
    mp.spawn(_two_rank_worker, args=(2, port, out), nprocs=2, join=True)
    (p0, t0, lr0, s0, kl0, last0), (p1, t1, lr1, s1, kl1, last1) = out[0], out[1]
    print("two ranks: t %d, lr %g, stopped updates in the last step %d; KL per update, rank 0 | rank 1 -> all-reduced: %s"
          % (t0, lr0, s0, "  ".join("%.3e | %.3e -> %.3e" % (a[0], b[0], a[1]) for a, b in zip(kl0, kl1))))
    assert len(kl0) == len(kl1) == 2 * 4                     # each step leaves after its first pass
    for (a, avg_a), (b, avg_b) in zip(kl0, kl1):
        assert avg_a == avg_b == float((np.float32(a) + np.float32(b)) / np.float32(2))
    stopping = next(i for i, a in enumerate(kl0) if a[1] > 1.5e-6)
    assert kl0[stopping][0] != kl1[stopping][0]              # the ranks measured different KLs where the stop was decided
    assert last0 == last1
    assert 0 < t0 == t1 < 2 * 3 * 4 and lr0 == lr1 != _REACHED["learning_rate"] and s0 >= 1 and s1 == 0   # progress_fn runs on rank 0
    assert np.isfinite(p0).all()
    np.testing.assert_array_equal(p0, p1)
