"""GPU: the learner's and the two-launch actor's MLP kernels (csrc/rr_mlp.h, csrc/rr_ppo.h) at the shapes where their code branches --
observation widths around the 16-wide k-chunk, row counts around the 32-row tile, 1 and 7 hidden layers, weight-gradient tiles that
overhang the matrix by 1 .. 3 columns, slice counts around the reduction's unroll of 8 -- against the float64 reference of
tests/mlp_shapes.py, with the float32 library path as the yardstick and the suite's existing floors (tests/mlp_shapes.py lists them).
tests/test_mlp_edges_cpu.py holds the reference to autograd and asserts that the tables below populate every class of shape."""
import functools

import pytest
import torch

from tests import mlp_shapes as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
_id = lambda c: "-".join(str(int(x)) if not isinstance(x, str) and x is not None else str(x) for x in c)


# ----------------------------------------------------------------------------------------------------------------- a. forward
@pytest.mark.parametrize("case", S.FORWARD_CASES, ids=_id)
def test_forward_at_the_edges(case):
    """rr_mlp_forward_kernel<..> / rr_mlp_policy256_forward_kernel: outputs and every layer's pre-activations against float64; the
    `rows` form equals the gathered form and the single-network calls equal the joint call, bit for bit."""
    from rodent_amd import hip
    K, M, norm, rows, vl, pl, pw, P = case
    nets = S.make_networks(K, P, pl, vl, pw, seed=K + M, device=DEV)
    obs, mean, std, idx = S.make_inputs(K, M, norm, rows, seed=K * 7 + M, device=DEV)
    pp, vp = S.params(nets.policy_network), S.params(nets.value_network)
    pol, val, ppre, vpre = hip.mlp_forward(obs, mean, std, pp, vp, want_pre=True, rows=idx)
    torch.cuda.synchronize()
    assert pol.shape == (M, P) and val.shape == (M,) and ppre.shape == (pl, M, pw) and vpre.shape == (vl, M, 256)
    label = _id(case)
    for name, prm, out, pre in (("policy", pp, pol, ppre), ("value", vp, val, vpre)):
        o64, z64 = S.forward(obs, mean, std, idx, *prm, F64)
        o32, _ = S.forward(obs, mean, std, idx, *prm, F32)
        S.check_output(label, name, out.reshape(o64.shape), o32, o64)
        for l in range(len(z64)):
            S.check_pre(label, f"{name} z{l}", pre[l], z64[l])
    if rows:
        gathered = hip.mlp_forward(obs[idx].contiguous(), mean, std, pp, vp, want_pre=True)
        for a, b in zip((pol, val, ppre, vpre), gathered):
            assert torch.equal(a, b)
    only_p = hip.mlp_forward(obs, mean, std, policy=pp, want_pre=True, rows=idx)
    only_v = hip.mlp_forward(obs, mean, std, value=vp, want_pre=True, rows=idx)
    assert only_p[1] is None and only_p[3] is None and only_v[0] is None and only_v[2] is None
    assert torch.equal(only_p[0], pol) and torch.equal(only_p[2], ppre) and torch.equal(only_v[1], val) and torch.equal(only_v[3], vpre)


@pytest.mark.parametrize("K", S.INTEGER_K)
@pytest.mark.parametrize("pw", [32, 256])
def test_integer_data_is_exact_at_the_chunk_edges(K, pw):
    """As test_gpu_mlp.test_integer_data_is_exact, at K = 16 (one full chunk, no partial one), 1264 (79 full chunks) and 3 (one partial
    chunk): small-integer observations and first-layer weights give integer pre-activations, so a column masked or kept wrongly at the
    chunk tail is a wrong integer, not a rounding-sized error."""
    from rodent_amd import hip
    M = 33
    g = torch.Generator(device=DEV).manual_seed(K)
    obs = torch.randint(-3, 4, (M, K), device=DEV, generator=g).float()
    n = S.make_networks(K, 60, 1, 1, pw, seed=1, device=DEV)
    with torch.no_grad():
        for net in (n.policy_network, n.value_network):
            w = net.layers[0].weight
            w.copy_(torch.randint(-2, 3, w.shape, device=DEV, generator=g).float())
            net.layers[0].bias.copy_(torch.arange(w.shape[0], device=DEV).float() % 7 - 3)
    _, _, ppre, vpre = hip.mlp_forward(obs, None, None, S.params(n.policy_network), S.params(n.value_network), want_pre=True)
    for pre, net in ((ppre, n.policy_network), (vpre, n.value_network)):
        want = obs.double() @ net.layers[0].weight.double().t() + net.layers[0].bias.double()
        assert torch.equal(pre[0].double(), want)


@pytest.mark.parametrize("K", S.ALONE_K)
def test_a_row_alone_equals_the_row_in_a_batch(K):
    """A row's outputs and pre-activations are the same bits computed alone (M = 1) and as row 37 of M = 77: csrc/rr_mlp.h promises a
    k-ordered chain per row, and a tile's other rows -- real ones, or copies of the last row where the tile overhangs -- do not enter
    it.  Holds bitwise for all of rr_mlp_forward_kernel, rr_mlp_policy256_forward_kernel and rr_policy_l1_kernel + rr_policy_tail_kernel
    (their k-slices are cut by K alone), so none of them falls back to the float32 criterion."""
    from rodent_amd import hip
    obs, mean, std, _ = S.make_inputs(K, 77, True, False, seed=K, device=DEV)
    one = obs[37:38].contiguous()
    for pw in (32, 256):
        n = S.make_networks(K, 60, 7, 7, pw, seed=K + pw, device=DEV)
        pp, vp = S.params(n.policy_network), S.params(n.value_network)
        full = hip.mlp_forward(obs, mean, std, pp, vp, want_pre=True)
        alone = hip.mlp_forward(one, mean, std, pp, vp, want_pre=True)
        assert torch.equal(full[0][37:38], alone[0]) and torch.equal(full[1][37:38], alone[1])
        assert torch.equal(full[2][:, 37:38], alone[2]) and torch.equal(full[3][:, 37:38], alone[3])
        if pw == 32:
            eps = torch.randn(77, 30, device=DEV)
            a = hip.policy_act(obs, mean, std, pp, eps, 0.001, want_logits=True)
            b = hip.policy_act(one, mean, std, pp, eps[37:38].contiguous(), 0.001, want_logits=True)
            for x, y in zip(a, b):
                assert torch.equal(x[37:38], y)


# ----------------------------------------------------------------------------------------------------------------- b. row isolation
@pytest.mark.parametrize("K,nan_at,inf_at", S.ISOLATION_CASES)
def test_a_non_finite_row_leaves_the_other_rows_alone(K, nan_at, inf_at):
    """One row of NaN and one of +Inf / -Inf / 3e38 (first row, row 31, or the last row of a ragged tile -- the row the rows past M are
    clamped onto): every other row's outputs and pre-activations are bit for bit those of the clean call, in rr_mlp_forward (both
    policy widths) and rr_policy_act.  Forward kernels only: a gradient sums over the rows by definition."""
    from rodent_amd import hip
    M = S.ISOLATION_M
    obs, mean, std, _ = S.make_inputs(K, M, True, False, seed=K + 1, device=DEV)
    bad = obs.clone()
    bad[nan_at] = float("nan")
    bad[inf_at] = torch.tensor([float("inf"), float("-inf"), 3e38], device=DEV).repeat(K // 3 + 1)[:K]
    keep = torch.ones(M, dtype=torch.bool, device=DEV)
    keep[nan_at] = keep[inf_at] = False
    eps = torch.randn(M, 30, device=DEV)
    for pw in (32, 256):
        n = S.make_networks(K, 60, 2, 2, pw, seed=K, device=DEV)
        pp, vp = S.params(n.policy_network), S.params(n.value_network)
        clean = hip.mlp_forward(obs, mean, std, pp, vp, want_pre=True)
        dirty = hip.mlp_forward(bad, mean, std, pp, vp, want_pre=True)
        torch.cuda.synchronize()
        assert torch.isfinite(clean[0]).all() and not torch.isfinite(dirty[0][nan_at]).any() and not torch.isfinite(dirty[1][nan_at])
        assert torch.equal(clean[0][keep], dirty[0][keep]) and torch.equal(clean[1][keep], dirty[1][keep])
        assert torch.equal(clean[2][:, keep], dirty[2][:, keep]) and torch.equal(clean[3][:, keep], dirty[3][:, keep])
        if pw == 32:
            for noise in (eps, None):
                a = hip.policy_act(obs, mean, std, pp, noise, 0.001, want_logits=True)
                b = hip.policy_act(bad, mean, std, pp, noise, 0.001, want_logits=True)
                for x, y in zip(a, b):
                    assert (x is None and y is None) or torch.equal(x[keep], y[keep])


# ----------------------------------------------------------------------------------------------------------------- c. the two-launch actor
@pytest.mark.parametrize("case", S.ACT_CASES, ids=_id)
def test_policy_act_at_the_edges(case):
    """rr_policy_l1_kernel + rr_policy_tail_kernel: the checks and tolerances of test_gpu_ppo_loss.test_policy_act_two_launches, at one
    partial chunk, one full chunk, fewer than 8 one-chunk slices, exactly 8, 8 slices of several chunks; 1 and 7 hidden layers; heads of
    2, 60, 66 and 128 logits.  Both the actor's logits and rr_mlp_forward's meet the float32 criterion against float64.  Bitwise: the
    sampling kernel on the actor's logits gives the actor's raw action / action / log-prob (the relation
    test_gpu_policy_head.test_two_launch_actor_equals_the_sampling_kernel establishes, and through `rr_policy_sample` the one
    test_learner_agrees_with_the_actor_at_the_actors_own_point stands on).  Between the actor's and the learner's LOGITS no test
    establishes a bitwise relation and the code rules it out (the actor adds k-slices and runs fmaf chains from the bias,
    rr_ppo.h rr_policy_tail_kernel; the learner runs one MFMA chain from zero and adds the bias last, rr_mlp.h rr_mlp_store_pol), so
    that pair is held to the criterion only."""
    from rodent_amd import hip
    from rodent_amd.training import networks
    K, M, nh, A, rows = case
    label = "act " + _id(case)
    n = S.make_networks(K, 2 * A, nh, 1, 32, seed=K + M + A, device=DEV)
    dist = networks.NormalTanhDistribution(A)
    pp = S.params(n.policy_network)
    obs, mean, std, idx = S.make_inputs(K, M, True, rows, seed=K + A, device=DEV)
    eps = torch.randn(M, A, device=DEV)
    lg64, _ = S.forward(obs, mean, std, idx, *pp, F64)
    lg32, _ = S.forward(obs, mean, std, idx, *pp, F32)
    loc, scale = dist._params(lg64)
    raw64 = loc + scale * eps.double()
    lp64 = dist.log_prob(lg64, raw64)
    act, raw, lp, lg = hip.policy_act(obs, mean, std, pp, eps, dist.min_std, want_logits=True, rows=idx)
    fwd = hip.mlp_forward(obs, mean, std, policy=pp, rows=idx)[0]
    torch.cuda.synchronize()
    S.check(label, "actor logits", lg, lg32, lg64)
    S.check(label, "learner logits", fwd, lg32, lg64)
    scale_l = float(lg64.abs().max())
    err = float((lg.double() - lg64).abs().max()) / scale_l
    tol = 20 * max(err, 1e-7) * scale_l                        # what the logits' error can do to the head's outputs
    assert float((raw.double() - raw64).abs().max()) <= tol + 1e-5
    assert float((act.double() - torch.tanh(raw64)).abs().max()) <= tol + 1e-5
    assert float((lp.double() - lp64).abs().max()) <= 50 * tol + 1e-4
    act_s, raw_s, lp_s = hip.policy_sample(lg, eps, dist.min_std)
    assert torch.equal(act, act_s) and torch.equal(raw, raw_s) and torch.equal(lp, lp_s)
    act_d, raw_d, lp_d, lg_d = hip.policy_act(obs, mean, std, pp, None, dist.min_std, rows=idx)
    assert raw_d is None and lp_d is None and lg_d is None
    assert float((act_d.double() - torch.tanh(loc)).abs().max()) <= tol + 1e-5
    if rows:
        gathered = hip.policy_act(obs[idx].contiguous(), mean, std, pp, eps, dist.min_std, want_logits=True)
        for x, y in zip((act, raw, lp, lg), gathered):
            assert torch.equal(x, y)


# ----------------------------------------------------------------------------------------------------------------- d. delta chains
def _check_chain(label, nh, n, z, delta, h, bgs, ref, extra):
    (d64, h64), (d32, _) = ref
    for j in range(nh):
        S.check(label, f"delta{j}", delta[j], d32[j], d64[j])
        assert float((h[j, :n].double() - h64[j]).abs().max()) <= 2e-6 * float(h64[j].abs().max()), (label, j)
        S.check_bias(label, f"db{j}", bgs[j], d64[j])
        if extra:
            assert torch.equal(h[j, n:], z[j][n:]), (label, j)                      # the rows behind the used ones: untouched


@pytest.mark.parametrize("nh,M", S.VALUE_BWD_CASES)
def test_value_backward_chain_at_the_edges(nh, M):
    """rr_mlp_value_backward at 1 hidden layer (the head epilogue alone: the `for (j = nh-1; j >= 1; --j)` loop never runs), 2 and 7,
    at one row, ragged tiles on both sides of 32, and three tiles."""
    from rodent_amd import hip
    G, wh, Ws, z = S.value_chain_inputs(nh, M)
    dev = lambda t: None if t is None else t.to(DEV)
    G, wh, Ws, z = dev(G), dev(wh), [dev(w) for w in Ws], [dev(t) for t in z]
    ref = S.delta_chain(G, wh, Ws, z, F64), S.delta_chain(G, wh, Ws, z, F32)
    pre = torch.stack(z).contiguous()
    bgs = [torch.full((256,), 7.0, device=DEV) for _ in range(nh)]
    delta, h = hip.mlp_value_backward(G[:, 0].contiguous(), wh, [None] + [Ws[j].t().contiguous() for j in range(1, nh)], pre, bgs)
    torch.cuda.synchronize()
    assert h.data_ptr() == pre.data_ptr() and delta.shape == (nh, M, 256)
    _check_chain(f"value chain nh={nh} M={M}", nh, M, z, delta, h, bgs, ref, 0)


@pytest.mark.parametrize("nh,P,extra,M", S.POLICY_BWD_CASES)
def test_policy_backward_chain_at_the_edges(nh, P, extra, M):
    """rr_policy_backward at 1 and 7 hidden layers, heads of 2 / 60 / 65 / 128 logits, with and without bootstrap rows behind M."""
    from rodent_amd import hip
    G, wh, Ws, z = S.policy_chain_inputs(nh, P, extra, M)
    dev = lambda t: None if t is None else t.to(DEV)
    G, wh, Ws, z = dev(G), dev(wh), [dev(w) for w in Ws], [dev(t) for t in z]
    zM = [t[:M] for t in z]
    ref = S.delta_chain(G, wh, Ws, zM, F64), S.delta_chain(G, wh, Ws, zM, F32)
    pre = torch.stack(z).contiguous()
    bgs = [torch.full((32,), 7.0, device=DEV) for _ in range(nh)]
    delta, h = hip.policy_backward(G, wh, Ws, pre, bgs)
    torch.cuda.synchronize()
    assert delta.shape == (nh, M, 32)
    _check_chain(f"policy chain nh={nh} P={P} M={M}+{extra}", nh, M, z, delta, h, bgs, ref, extra)


@pytest.mark.parametrize("nh,n,P,extra", S.POLICY256_BWD_CASES)
def test_policy256_backward_chain_at_the_edges(nh, n, P, extra):
    """rr_mlp_policy_backward (256-wide policy) at 1 and 7 hidden layers; P = 2 and 65 end in a partial k-chunk of the head product, 60
    in an odd chunk count, 128 in neither."""
    from rodent_amd import hip
    G, wh, Ws, z = S.policy256_chain_inputs(nh, n, P, extra)
    dev = lambda t: None if t is None else t.to(DEV)
    G, wh, Ws, z = dev(G), dev(wh), [dev(w) for w in Ws], [dev(t) for t in z]
    zn = [t[:n] for t in z]
    ref = S.delta_chain(G, wh, Ws, zn, F64), S.delta_chain(G, wh, Ws, zn, F32)
    pre = torch.stack(z).contiguous()
    bgs = [torch.full((256,), 7.0, device=DEV) for _ in range(nh)]
    delta, h = hip.mlp_policy_backward(G, wh.t().contiguous(), [None] + [Ws[j].t().contiguous() for j in range(1, nh)], pre, bgs)
    torch.cuda.synchronize()
    assert delta.shape == (nh, n, 256)
    _check_chain(f"policy256 chain nh={nh} P={P} n={n}+{extra}", nh, n, z, delta, h, bgs, ref, extra)


# ----------------------------------------------------------------------------------------------------------------- e. weight gradients
@functools.lru_cache(maxsize=None)
def _dw_single(i):
    """(inputs, keyword arguments, the single call's result, float64, float32) of DW_CASES[i]; computed once, left unchanged."""
    from rodent_amd import hip
    M, O, I, rows, norm = S.DW_CASES[i]
    delta, act, idx, mean, std = S.dw_inputs(M, O, I, rows, norm, DEV)
    kw = dict(rows=idx)
    if norm:
        kw.update(mean=mean, std=std, delta_colsum=delta.sum(0))
    out = torch.full((O, I), 7.0, device=DEV)
    hip.mlp_weight_grad(delta, act, out, **kw)
    torch.cuda.synchronize()
    return (delta, act), kw, out, S.weight_grad(delta, act, idx, mean, std, F64), S.weight_grad(delta, act, idx, mean, std, F32)


@pytest.mark.parametrize("i", range(len(S.DW_CASES)), ids=[_id(c) for c in S.DW_CASES])
def test_weight_grad_at_the_edges(i):
    """rr_mlp_dw_kernel (all three instances) + rr_mlp_dw_reduce_kernel: last tile columns 1, 2, 3 wide next to vector-path tiles, I < 4,
    O in {2, 3, 5, 33, 65}; the reduction's aligned branch at 1, 3, 8 and 9 slices (remainder loop alone, one unrolled pass of 8 with an empty
    remainder, both) and its unaligned branch at 1, 2, 5 and 8 (tests/test_mlp_edges_cpu.py reads the counts from the library)."""
    M, O, I, _, _ = S.DW_CASES[i]
    _, _, out, w64, w32 = _dw_single(i)
    S.check(f"dW M={M} O={O} I={I}", "single", out, w32, w64)


@pytest.mark.parametrize("b", range(len(S.DW_BATCHES)))
def test_weight_grad_batch_at_the_edges(b):
    """`rr_mlp_weight_grad_batch` over the whole table in two calls; the first holds all three tile groups, with overhang-1 products and
    a whole-tile product in one group.  Every product against float64 by the criterion, and the relations
    test_gpu_ppo_loss.test_weight_grad_batch_against_single_calls establishes: a repeated batch bit for bit, a batch of one against the
    single call bit for bit, a batched product against the single call by that test's two-sided round-off bound.  At these row counts
    (M <= 400) the row limit M / (2 kc) of the slice plan binds alone and in a batch, so the batched plans are not expected to differ
    from the single ones here; plans that differ are what that test runs at M = 4096, and the bound asserted holds either way."""
    from rodent_amd import hip
    items, again = [], []
    for i in S.DW_BATCHES[b]:
        (delta, act), kw, single, _, _ = _dw_single(i)
        items.append(dict(delta=delta, act=act, out=torch.full_like(single, 7.0), **kw))
        again.append(dict(delta=delta, act=act, out=torch.full_like(single, -7.0), **kw))
    hip.mlp_weight_grad_batch(items)
    hip.mlp_weight_grad_batch(again)
    torch.cuda.synchronize()
    for i, it, ag in zip(S.DW_BATCHES[b], items, again):
        M, O, I, _, _ = S.DW_CASES[i]
        (delta, act), kw, single, w64, w32 = _dw_single(i)
        assert torch.equal(it["out"], ag["out"])
        S.check(f"dW M={M} O={O} I={I}", "batched", it["out"], w32, w64)
        scale = float(w64.abs().max())
        e_single, e_batch = float((single.double() - w64).abs().max()), float((it["out"].double() - w64).abs().max())
        assert e_batch <= 2 * e_single + 2e-6 * scale and e_single <= 2 * e_batch + 2e-6 * scale, (i, e_single, e_batch, scale)
        one = torch.full_like(single, 3.0)
        hip.mlp_weight_grad_batch([dict(delta=delta, act=act, out=one, **kw)])
        assert torch.equal(one, single)


# ----------------------------------------------------------------------------------------------------------------- f. FusedUpdate
@pytest.mark.parametrize("vl,pl,streams", S.FUSED_UPDATE_CASES, ids=[_id(c) for c in S.FUSED_UPDATE_CASES])
def test_fused_update_on_other_depths(vl, pl, streams, monkeypatch):
    """FusedUpdate on 1 + 1 and 7 + 7 hidden layers (32-wide policy) against compute_ppo_loss + backward on the same fused forward, by
    the bounds of test_gpu_ppo_loss.test_fused_update_equals_the_autograd_path.  7 + 7 is 16 weight-gradient products: on one stream
    (RR_LEARNER_STREAMS=0) the split branch of FusedUpdate.__call__, with the default streams one batched call per network."""
    from rodent_amd.training import distributed as D, fused_mlp
    from rodent_amd.training.agents.ppo import fused_update, losses
    from tests.ppo_batches import CFG, _batch
    if streams is None:
        monkeypatch.delenv("RR_LEARNER_STREAMS", raising=False)
    else:
        monkeypatch.setenv("RR_LEARNER_STREAMS", streams)
    T, B, R, K, A = (S.FUSED_UPDATE_SHAPE[k] for k in "TBRKA")
    nets = S.make_networks(K, 2 * A, pl, vl, 32, seed=0, device=DEV)
    pnet, vnet, dist = nets.policy_network, nets.value_network, nets.parametric_action_distribution
    params = list(pnet.parameters()) + list(vnet.parameters())
    flat = D.FlatGrads(params)
    g = torch.Generator(device=DEV).manual_seed(1)
    data, _, _, _, idx = _batch(T, B, R, A, seed=9)
    data = {k: v.to(DEV).contiguous() for k, v in data.items()}
    data["obs"] = torch.randn(R, T + 1, K, device=DEV, generator=g) * 2 + 0.5
    idx = idx.to(DEV)
    mean, std = torch.randn(K, device=DEV, generator=g) * 0.3, torch.rand(K, device=DEV, generator=g) + 0.5
    fu = fused_update.FusedUpdate(pnet, vnet, dist, T, normalize_advantage=True, **CFG)
    assert (fu.side is None) == (streams == "0")
    m_f = fu(data, idx, mean, std, torch.Generator(device=DEV).manual_seed(77))
    torch.cuda.synchronize()
    got = flat.flat.clone()
    m_f = {k: float(v) for k, v in m_f.items()}
    gen = torch.Generator(device=DEV).manual_seed(77)                       # the path it replaces, same noise stream
    mbd = {k: data[k][idx].transpose(0, 1) for k in ("raw_action", "log_prob", "reward", "discount", "truncation")}
    raw = data["obs"][idx].transpose(0, 1)
    logits_all, values_all = fused_mlp.actor_critic(raw.reshape((T + 1) * B, -1), mean, std, pnet, vnet)
    values = values_all.reshape(T + 1, B)
    loss, m = losses.compute_ppo_loss(logits_all[:T * B].reshape(T, B, -1), values[:T], values[T], mbd, dist, normalize_advantage=True, generator=gen, **CFG)
    flat.zero_()
    loss.backward()
    want = flat.flat.clone()
    o, figures = 0, []
    for p in params:                                                        # per tensor: the scales differ by orders of magnitude
        a, b = got[o:o + p.numel()], want[o:o + p.numel()]
        o += p.numel()
        figures.append((tuple(p.shape), bool(torch.isfinite(a).all()), float((a - b).abs().max()), float(b.abs().max())))
    label = f"FusedUpdate value {vl} policy {pl} streams {streams}"
    S.record(label, "largest gradient error against the autograd path over the parameters, relative to each one's largest entry (bound 2e-4)", max(e / m for _, _, e, m in figures if m > 0))
    S.record(label, "largest metric error against the autograd path, relative to max(1, metric) (bound 1e-5)", max(abs(m_f[k] - float(m[k])) / max(1.0, abs(float(m[k]))) for k in m_f))
    for shape, finite, err, scale in figures:
        assert finite and scale > 0 and err <= 2e-4 * scale + 1e-9, (shape, err, scale)
    for k in m_f:
        assert abs(m_f[k] - float(m[k])) <= 1e-5 * max(1.0, abs(float(m[k]))), (k, m_f[k], float(m[k]))


@pytest.mark.parametrize("depth", [1, 7])
def test_actor_critic_gradients_on_other_depths(depth):
    """`fused_mlp.actor_critic` (kernel forward + explicit backward) at 1 + 1 and 7 + 7 hidden layers: every parameter's gradient against
    the float64 reference, the float32 library path as the yardstick (bias gradients by the bias-sum bound)."""
    from rodent_amd.training import fused_mlp
    T, B, R, K, A = (S.FUSED_UPDATE_SHAPE[k] for k in "TBRKA")
    M = (T + 1) * B
    nets = S.make_networks(K, 2 * A, depth, depth, 32, seed=depth, device=DEV)
    obs, mean, std, _ = S.make_inputs(K, M, True, False, seed=depth, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(5)
    gp, gv = torch.randn(M, 2 * A, device=DEV, generator=g), torch.randn(M, device=DEV, generator=g)
    pol, val = fused_mlp.actor_critic(obs, mean, std, nets.policy_network, nets.value_network)
    ((pol * gp).sum() + (val * gv).sum()).backward()
    torch.cuda.synchronize()
    for name, net, G in (("policy", nets.policy_network, gp), ("value", nets.value_network, gv)):
        r64 = S.gradients(obs, mean, std, None, *S.params(net), G, F64)
        r32 = S.gradients(obs, mean, std, None, *S.params(net), G, F32)
        for l, lin in enumerate(net.layers):
            label = f"actor_critic depth={depth} {name}"
            S.check(label, f"dW{l}", lin.weight.grad, r32["dW"][l], r64["dW"][l])
            S.check_bias(label, f"db{l}", lin.bias.grad, r64["delta"][l])
