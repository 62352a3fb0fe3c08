"""GPU: `rr_clipped_adam_step` (three launches, csrc/rr_ppo.h) through `hip.ClippedAdamBuffers` on synthetic tensor lists chosen for
their edges -- single elements, segments that start off the float4 grid, totals on both sides of every change of the partial count, 64
tensors -- and `ppo.train(max_grad_norm=...)` at 64 envs.  The non-finite values are ordinary data of elementwise kernels."""
import logging
import math

import numpy as np
import pytest
import torch

from tests import grad_clip_cases as cases
from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR = 1e-2


def _edge_totals():
    """Totals one element on either side of every change of the partial count, up to three partials (the query decides where)."""
    from rodent_amd import hip
    out, n, k = [], 1, hip.clipped_adam_partials(1)
    assert k == 1
    while k < 3:
        lo, hi = n, n
        while hip.clipped_adam_partials(hi) == k:          # gallop, then bisect: the count is monotone in n
            lo, hi = hi, hi * 2
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if hip.clipped_adam_partials(mid) == k else (lo, mid)
        assert hip.clipped_adam_partials(lo) == k and hip.clipped_adam_partials(hi) == k + 1
        out += [lo, hi]
        n, k = hi, k + 1
    return out


def _lists():
    ls = {"1": [1], "3_4_5": [3, 4, 5], "255_256_257_1": [255, 256, 257, 1], "1023_1025_7": [1023, 1025, 7],
          "64_tensors": [i % 7 + 1 for i in range(64)]}
    for tot in _edge_totals():                               # a long tensor (several blocks of the update) between two short odd ones
        ls["total_%d" % tot] = [5, tot - 5 - 3, 3]
    return ls


class Case:
    """Buffers of one optimiser on a tensor list.  layout 'packed': the parameters are views of one buffer laid out like the gradient, so a
    segment off the float4 grid has scalar head and tail elements around an aligned body; 'shifted': the same buffer one element further,
    so no parameter address is congruent with its gradient segment (scalar parameter accesses around float4 gradient / moment accesses)."""

    def __init__(self, sizes, layout, max_grad_norm, p0=None, m0=None, v0=None, t0=0):
        from rodent_amd import hip
        from rodent_amd.training import optim
        self.sizes, self.n = sizes, sum(sizes)
        shift = {"packed": 0, "shifted": 1}[layout]
        self.pbuf = torch.zeros(self.n + 4, device=DEV)
        off = np.concatenate([[0], np.cumsum(sizes)])
        self.params = [self.pbuf[shift + off[k]:shift + off[k + 1]] for k in range(len(sizes))]
        self.pview = self.pbuf[shift:shift + self.n]
        self.g, self.m, self.v = (torch.zeros(self.n, device=DEV) for _ in range(3))
        if p0 is not None:
            self.pview.copy_(torch.from_numpy(p0)); self.m.copy_(torch.from_numpy(m0)); self.v.copy_(torch.from_numpy(v0))
        self.b = hip.ClippedAdamBuffers(self.params, self.g, self.m, self.v, lr=LR, b1=cases.B1, b2=cases.B2, eps=cases.EPS, max_grad_norm=max_grad_norm)
        self.b.state[optim.ST_T] = float(t0)

    def step(self, g=None):
        if g is not None:
            self.g.copy_(torch.from_numpy(np.ascontiguousarray(g, dtype=np.float32)))
        self.b.step()

    def host(self):
        torch.cuda.synchronize()
        return self.pview.cpu().numpy(), self.m.cpu().numpy(), self.v.cpu().numpy(), self.b.state.cpu().numpy()

    def bits(self):
        p, m, v, st = self.host()
        return [p.view(np.uint32), m.view(np.uint32), v.view(np.uint32), st.view(np.uint64), self.pbuf.cpu().numpy().view(np.uint32)]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def lists():
    return _lists()


@pytest.fixture(scope="module")
def inputs(lists):
    """Per list: float32 p0, g, m0 (signed), v0 (>= 0); one draw, shared and left unchanged."""
    rng = np.random.default_rng(0)
    out = {}
    for name, sizes in lists.items():
        n = sum(sizes)
        out[name] = dict(p0=rng.standard_normal(n).astype(np.float32), g=rng.standard_normal(n).astype(np.float32),
                         m0=(0.1 * rng.standard_normal(n)).astype(np.float32), v0=(0.01 * rng.random(n)).astype(np.float32))
    return out


def test_partial_count_query_and_edges(lists):
    from rodent_amd import hip
    edges = _edge_totals()
    assert len(edges) == 4 and [hip.clipped_adam_partials(n) for n in edges] == [1, 2, 2, 3]
    assert hip.clipped_adam_partials(0) == 0 and hip.clipped_adam_partials(10 ** 9) == hip.clipped_adam_partials(10 ** 10)     # capped
    assert sum(lists["64_tensors"]) > 64 and all(sum(s) > 0 for s in lists.values())


# ---------------------------------------------------------------------------------------------- exact norm
@pytest.mark.parametrize("layout", ["packed", "shifted"])
def test_norm_of_integer_gradients_is_exact(lists, layout):
    """Entries in {-3 .. 3}: every square and every partial sum is an integer below 2^53, so the double sum is exact in any order and the
    reported norm must be float32(sqrt(exact)) bit for bit."""
    from rodent_amd.training import optim
    rng = np.random.default_rng(1)
    for name, sizes in lists.items():
        g = rng.integers(-3, 4, sum(sizes)).astype(np.float32)
        c = Case(sizes, layout, float("inf"))
        c.step(g)
        st = c.host()[3]
        want = np.float32(np.sqrt(np.float64((g.astype(np.int64) ** 2).sum())))
        assert np.float32(st[optim.ST_NORM]) == want and st[optim.ST_NORM] == float(want), (name, st[optim.ST_NORM], want)
        assert st[optim.ST_T] == 1 and st[optim.ST_SKIP] == 0 and st[optim.ST_SCALE] == 1.0


def test_norm_of_all_ones_at_powers_of_four():
    from rodent_amd import hip
    from rodent_amd.training import optim
    for k in range(0, 8):                                   # n = 1 .. 16384: norm = 2^k; the last is four partials
        n = 4 ** k
        c = Case([n], "packed", float("inf"))
        c.step(np.ones(n, np.float32))
        assert c.host()[3][optim.ST_NORM] == float(2 ** k), (n, hip.clipped_adam_partials(n))
    assert hip.clipped_adam_partials(4 ** 7) == 4


# ---------------------------------------------------------------------------------------------- against the float64 reference, and torch against it
@pytest.mark.parametrize("layout", ["packed", "shifted"])
def test_step_within_the_counted_bound_of_the_float64_reference(lists, inputs, layout):
    """One step from t = 0, 1 and 999, clipped (max = norm / 2) and unclipped, every element of p, m, v against `clipped_adam_reference` from
    identical float32 inputs, within the bound counted from the rule's roundings (tests/grad_clip_cases.py; nothing fitted).  Measured on
    an MI355X: the largest share of the bound over all lists, layouts and steps is recorded in DESIGN.md section 4v."""
    from rodent_amd.training import optim
    worst = [0.0, 0.0, 0.0]
    for name, sizes in lists.items():
        x = inputs[name]
        norm = float(np.sqrt((x["g"].astype(np.float64) ** 2).sum()))
        for t0 in (0, 1, 999):
            m0, v0 = (x["m0"], x["v0"]) if t0 else (np.zeros_like(x["m0"]), np.zeros_like(x["v0"]))
            for mx in (0.5 * norm, 2.0 * norm):
                ref = cases.reference_step(x["p0"], x["g"], m0, v0, t0, LR, mx)
                c = Case(sizes, layout, mx, x["p0"], m0, v0, t0)
                c.step(x["g"])
                p, m, v, st = c.host()
                assert st[optim.ST_T] == ref["t"] == t0 + 1 and st[optim.ST_NORM] == ref["norm"] and st[optim.ST_SCALE] == ref["scale"]
                assert (ref["scale"] < 1.0) == (mx < norm) and st[optim.ST_CLIPPED] == (1.0 if mx < norm else 0.0)
                sh = cases.shares(p, m, v, ref)
                worst = [max(a, b) for a, b in zip(worst, sh)]
                assert max(sh) <= 1.0, (name, t0, mx, sh)
                assert c.pbuf.cpu().numpy()[[0, -1, -2, -3] if layout == "shifted" else [-1, -2, -3, -4]].tolist() == [0.0] * 4     # nothing written beside the tensors
    print("rr_clipped_adam_step, layout %s: largest share of the counted bound p %.3f m %.3f v %.3f" % (layout, *worst))


def test_torch_adam_after_clip_grad_norm_against_the_same_reference(lists, inputs):
    """The stock pair on the same inputs (t = 0, so that torch's own step count applies): within the SAME bound where nothing is clipped; where
    it clips, torch scales by max / (norm + 1e-6), which the bound it needs adds (`torch_extra_*`).  Both shares are printed: the criterion
    is no looser for the hand-written kernels than for the stock ones."""
    same, need = [0.0] * 3, [0.0] * 3
    for name, sizes in lists.items():
        x = inputs[name]
        norm = float(np.sqrt((x["g"].astype(np.float64) ** 2).sum()))
        zeros = np.zeros_like(x["m0"])
        for mx in (0.5 * norm, 2.0 * norm):
            ref = cases.reference_step(x["p0"], x["g"], zeros, zeros, 0, LR, mx)
            p = torch.tensor(x["p0"], device=DEV, requires_grad=True)
            p.grad = torch.tensor(x["g"], device=DEV)
            opt = torch.optim.Adam([p], lr=LR, betas=(cases.B1, cases.B2), eps=cases.EPS, fused=True)
            torch.nn.utils.clip_grad_norm_([p], mx)
            opt.step()
            got = (p.detach().cpu().numpy(), opt.state[p]["exp_avg"].cpu().numpy(), opt.state[p]["exp_avg_sq"].cpu().numpy())
            s0, s1 = cases.shares(*got, ref), cases.shares(*got, ref, extra=True)
            if mx > norm:
                same = [max(a, b) for a, b in zip(same, s0)]
                assert max(s0) <= 1.0, (name, mx, s0)
            need = [max(a, b) for a, b in zip(need, s1)]
            assert max(s1) <= 1.0, (name, mx, s1)
    print("torch clip_grad_norm_ + Adam(fused): largest share of the same bound, unclipped: p %.3f m %.3f v %.3f; "
          "of the bound it needs (with its 1e-6), all cases: p %.3f m %.3f v %.3f" % (*same, *need))


# ---------------------------------------------------------------------------------------------- unscaled at or below the threshold
@pytest.mark.parametrize("layout", ["packed", "shifted"])
def test_threshold_at_or_above_the_norm_gives_the_bits_of_inf(lists, inputs, layout):
    for name in ("3_4_5", "1023_1025_7", "64_tensors"):
        sizes, x = lists[name], inputs[name]
        g = np.random.default_rng(3).integers(-3, 4, sum(sizes)).astype(np.float32)
        g[:2] = (3.0, 4.0)
        norm = float(np.float32(np.sqrt(np.float64((g.astype(np.int64) ** 2).sum()))))
        runs = {}
        for mx in (float("inf"), 2.0 * norm, norm, float(np.nextafter(np.float32(norm), np.float32(0)))):
            c = Case(sizes, layout, mx, x["p0"], x["m0"], x["v0"], 7)
            c.step(g)
            runs[mx] = c.bits()
        a = runs[float("inf")]
        assert _same([a[0], a[1], a[2]], runs[2.0 * norm][:3]) and _same([a[0], a[1], a[2]], runs[norm][:3])        # equal to the norm: not clipped
        assert not np.array_equal(a[1], list(runs.values())[3][1])                                                  # one float32 below it: clipped


def test_g_3_4_with_threshold_5_is_not_clipped():
    from rodent_amd.training import optim
    a, b = Case([2], "packed", 5.0), Case([2], "packed", float("inf"))
    for c in (a, b):
        c.step(np.array([3.0, 4.0], np.float32))
    assert _same(a.bits()[:3], b.bits()[:3])
    st = a.host()[3]
    assert st[optim.ST_NORM] == 5.0 and st[optim.ST_SCALE] == 1.0 and st[optim.ST_CLIPPED] == 0 and st[optim.ST_APPLIED] == 1


# ---------------------------------------------------------------------------------------------- skip
@pytest.mark.parametrize("layout", ["packed", "shifted"])
def test_non_finite_element_skips_the_update(lists, inputs, layout):
    """The bad element in the first block's range, in the last tail element, and in a scalar head element of a segment off the float4 grid."""
    from rodent_amd.training import optim
    name = "total_%d" % _edge_totals()[-1]                  # three partials; segments [5, long, 3]: the long one starts at offset 5 (head 3)
    sizes, x = lists[name], inputs[name]
    n = sum(sizes)
    for where, val in ((0, np.nan), (n - 1, np.inf), (5, -np.inf), (6, np.nan)):
        c = Case(sizes, layout, 1.0, x["p0"], x["m0"], x["v0"], 3)
        c.step(x["g"])
        before = c.bits()
        bad = x["g"].copy()
        bad[where] = val
        c.step(bad)
        after = c.bits()
        assert _same(before[:3], after[:3]) and np.array_equal(before[4], after[4]), (where, val)
        st = c.host()[3]
        assert st[optim.ST_T] == 4 and st[optim.ST_SKIP] == 1 and st[optim.ST_SKIPPED] == 1 and st[optim.ST_APPLIED] == 1
        assert not math.isfinite(st[optim.ST_NORM]) and math.isfinite(st[optim.ST_NORM_SUM]) and math.isfinite(st[optim.ST_NORM_MAX])
        c.step(x["g"])                                       # the next finite step continues with the old t
        d = Case(sizes, layout, 1.0, x["p0"], x["m0"], x["v0"], 3)
        d.step(x["g"]); d.step(x["g"])
        assert _same(c.bits()[:3], d.bits()[:3]) and c.host()[3][optim.ST_T] == 5 and c.host()[3][optim.ST_SKIP] == 0


# ---------------------------------------------------------------------------------------------- graph
def test_captured_step_replayed_equals_eager_steps(lists, inputs):
    """One captured step replayed five times against five eager calls, the gradient buffer refilled between them (one of the five with a
    NaN: the skip replays too): parameters, moments, t and the statistics bit for bit."""
    name = "total_%d" % _edge_totals()[-1]
    sizes, x = lists[name], inputs[name]
    rng = np.random.default_rng(4)
    gs = [(3.0 * rng.standard_normal(sum(sizes))).astype(np.float32) * (1e-4 if i == 3 else 1.0) for i in range(5)]
    gs[2][17] = np.nan
    warm = Case(sizes, "packed", 1.0, x["p0"], x["m0"], x["v0"], 0)
    warm.step(gs[0])                                         # the kernels are loaded before anything is captured
    eager = Case(sizes, "packed", 1.0, x["p0"], x["m0"], x["v0"], 0)
    for g in gs:
        eager.step(g)
    rep = Case(sizes, "packed", 1.0, x["p0"], x["m0"], x["v0"], 0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        rep.step()
    for g in gs:
        rep.g.copy_(torch.from_numpy(g))
        graph.replay()
    a, b = eager.bits(), rep.bits()
    assert _same(a, b)
    from rodent_amd.training import optim
    st = rep.host()[3]
    assert st[optim.ST_T] == 4 and st[optim.ST_SKIPPED] == 1 and st[optim.ST_APPLIED] == 4 and st[optim.ST_CLIPPED] == 3


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals():
    from rodent_amd import hip
    from rodent_amd.training import optim
    kw = dict(lr=LR, b1=cases.B1, b2=cases.B2, eps=cases.EPS, max_grad_norm=1.0)
    buf = torch.zeros(65, device=DEV)
    g, m, v = (torch.zeros(65, device=DEV) for _ in range(3))
    b = hip.ClippedAdamBuffers([buf[i:i + 1] for i in range(65)], g, m, v, **kw)
    with pytest.raises(RuntimeError, match="more than 64 tensors"):
        b.step()
    b = hip.ClippedAdamBuffers([buf[0:3], buf[3:7]], g, m, v, n=8, **kw)            # the table sums to 7
    with pytest.raises(RuntimeError, match="n differs from the sum"):
        b.step()
    b = hip.ClippedAdamBuffers([buf[0:3], buf[3:7]], g, m, v, n=6, **kw)
    with pytest.raises(RuntimeError, match="sum to n"):
        b.step()
    b = hip.ClippedAdamBuffers([buf[0:3], buf[3:7]], g[1:], m, v, n=7, **kw)         # a flat buffer off the 16-byte grid
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        b.step()
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0 and float(m.abs().sum()) == 0.0              # a refused call launches nothing
    with pytest.raises(ValueError):
        optim.ClippedAdam([buf[i:i + 1] for i in range(65)], g, lr=LR, max_grad_norm=1.0)


# ---------------------------------------------------------------------------------------------- ppo.train
def test_ppo_train_with_max_grad_norm_at_64_envs(monkeypatch, caplog):
    """Two training steps with max_grad_norm = 1: the fused update and the one-launch rollout are still the path taken, the update graph is
    captured (no fallback warning), metrics and parameters are finite, and the optimiser's counters are cleared after the run."""
    from rodent_amd import envs
    from rodent_amd.training import acting, optim
    from rodent_amd.training.agents.ppo import fused_update, train as ppo
    calls = {"rollout": 0, "update": 0, "replay": 0}
    real_rollout, real_call, real_replay = acting.generate_unrolls_fused, fused_update.FusedUpdate.__call__, torch.cuda.CUDAGraph.replay

    def rollout(*a, **k):
        calls["rollout"] += 1
        return real_rollout(*a, **k)

    def update(self, *a, **k):
        calls["update"] += 1
        return real_call(self, *a, **k)

    def replay(self):
        calls["replay"] += 1
        return real_replay(self)

    monkeypatch.setattr(acting, "generate_unrolls_fused", rollout)
    monkeypatch.setattr(fused_update.FusedUpdate, "__call__", update)
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", replay)
    env = envs.get_environment("rodent", track_pos=util.synthetic_track(), num_envs=64, xml_path="rodent_optimized.xml", iterations=8,
                               ls_iterations=8, device=DEV)
    log = []
    with caplog.at_level(logging.WARNING):
        _, params, _, ts = ppo.train(environment=env, num_timesteps=10 ** 9, episode_length=150, num_envs=64, batch_size=64, num_minibatches=4,
                                     unroll_length=5, num_updates_per_batch=2, num_evals=3, num_eval_envs=0, learning_rate=5e-5,
                                     entropy_cost=1e-3, discounting=0.97, normalize_observations=True, seed=1, max_training_steps=2,
                                     max_grad_norm=1.0, return_training_state=True, progress_fn=lambda n, m: log.append(m))
    assert not [r for r in caplog.records if "graph capture failed" in r.getMessage()]
    assert calls["rollout"] == 2 and calls["update"] == 4 and calls["replay"] == 16 - 3      # 3 eager updates, one capture, every update replayed from the 4th
    m = log[-1]
    for k in ("training/grad_norm", "training/grad_norm_max", "training/grad_clip_share", "training/skipped_updates", "training/total_loss"):
        assert k in m and math.isfinite(float(m[k])), (k, m)
    assert m["training/grad_norm"] > 0 and m["training/grad_norm_max"] >= m["training/grad_norm"] and m["training/skipped_updates"] == 0
    assert all(torch.isfinite(p).all() for p in params[1].parameters())
    opt = ts.optimizer_state
    assert isinstance(opt, optim.ClippedAdam) and len(opt.state) > 0 and opt.t == 16
    st = opt.stats(clear=False)
    assert st["applied_updates"] == 0 and st["skipped_updates"] == 0 and st["grad_norm_max"] == 0.0


def _two_rank_worker(rank, world, port, out):
    import os
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), RR_PPO_GRAPH="1")
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from rodent_amd import envs
        from rodent_amd.training.agents.ppo import train as ppo
        torch.cuda.set_device(0)
        env = envs.get_environment("rodent", track_pos=util.synthetic_track(), num_envs=64, xml_path="rodent_optimized.xml",
                                   iterations=8, ls_iterations=8, device=DEV)
        seen = {}
        _, params, _, ts = ppo.train(environment=env, num_timesteps=128 * 4 * 4 * 2, episode_length=150, num_envs=128, batch_size=128,
                                     num_minibatches=4, unroll_length=4, num_updates_per_batch=3, num_evals=1, num_eval_envs=0,
                                     learning_rate=5e-5, entropy_cost=1e-3, discounting=0.97, normalize_observations=True, seed=3,
                                     max_grad_norm=1e-3, return_training_state=True, progress_fn=lambda n, m: seen.update(m))
        vec = torch.cat([p.detach().reshape(-1) for p in params[1].parameters()]).cpu()
        out[rank] = (vec.numpy().copy(), ts.optimizer_state.t, {k: v for k, v in seen.items() if "grad_" in k or "skipped" in k})
    finally:
        torch.distributed.destroy_process_group()


def test_two_ranks_with_the_option_end_with_identical_parameters():
    """The two-graph learner of multi-rank runs (capture A | all-reduce | capture B: here the clipped step) on two ranks sharing the GPU:
    the clip acts on the all-reduced gradient, so both ranks hold the same bits; the small threshold makes updates clip."""
    import os
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    out = mgr.dict()
    port = 33500 + os.getpid() % 2000
    mp.spawn(_two_rank_worker, args=(2, port, out), nprocs=2, join=True)
    (p0, t0, k0), (p1, t1, _) = out[0], out[1]
    assert np.isfinite(p0).all() and t0 == t1 == 2 * 3 * 4
    np.testing.assert_array_equal(p0, p1)
    assert k0["training/skipped_updates"] == 0 and k0["training/grad_clip_share"] > 0 and math.isfinite(k0["training/grad_norm"])
