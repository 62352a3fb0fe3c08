"""GPU: policy heads of 65 .. 128 logits through the learner's and the actor's hand-written kernels (rodent_cpu.xml has 38 actuators =
76 logits): `rr_mlp_forward` (the head as two passes over column halves of 64), `rr_policy_backward` (P <= 128), `rr_policy_act`
(action_size <= 64), the already general `rr_ppo_loss` / `rr_policy_sample`, `FusedUpdate` and `ppo.train` behind RR_FUSED_WIDE_HEAD=1.
Shapes: one column into the second pass (65), the real model (76), full (128); row counts that are no multiple of 32 or of 8."""
import copy
import math
import warnings

import pytest
import torch

from tests import util
from tests.test_gpu_ppo_loss import CFG, _batch, _reference, fused_update_on_an_on_policy_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _policy(K, P, seed, nh=4):
    """Policy MLP obs -> 32 x nh -> P (P may be odd: the forward and the backward do not care), non-zero biases."""
    from rodent_amd.training import networks
    torch.manual_seed(seed)
    net = networks.MLP(K, [32] * nh + [P]).to(DEV)
    for lin in net.layers:
        torch.nn.init.uniform_(lin.bias, -0.2, 0.2)
    return net


def _value(K, seed):
    from rodent_amd.training import networks
    torch.manual_seed(seed + 1)
    net = networks.MLP(K, [256] * 5 + [1]).to(DEV)
    for lin in net.layers:
        torch.nn.init.uniform_(lin.bias, -0.1, 0.1)
    return net


def _wb(net):
    return [l.weight.detach() for l in net.layers], [l.bias.detach() for l in net.layers]


def _ref(x, net, dtype):
    """(output, [pre-activations of the hidden layers]) of `net` on x in `dtype`."""
    x = x.to(dtype)
    pre = []
    for i, lin in enumerate(net.layers):
        x = x @ lin.weight.detach().to(dtype).t() + lin.bias.detach().to(dtype)
        if i < len(net.layers) - 1:
            pre.append(x)
            x = torch.nn.functional.silu(x)
    return x, pre


def _within(name, got, f32, f64):
    """|got - f64| <= 3 |f32 - f64| + 2e-6, relative to max |f64|."""
    scale = float(f64.abs().max())
    err, err32 = float((got.double() - f64).abs().max()) / scale, float((f32.double() - f64).abs().max()) / scale
    print(f"  {name}: kernel {err:.2e}  torch-f32 {err32:.2e}  (relative to max |.| = {scale:.3g})")
    assert err <= 3 * err32 + 2e-6, (name, err, err32)


@pytest.mark.parametrize("K", [211, 1263])
@pytest.mark.parametrize("M", [1, 33, 100])
@pytest.mark.parametrize("P", [65, 76, 128])
def test_forward_matches_torch(P, M, K):
    """rr_mlp_forward with a head of P > 64 logits against float64; nn.Linear arithmetic in float32 is the yardstick.  With and without the
    normaliser, policy alone and policy + value, every output and every pre-activation dump."""
    from rodent_amd import hip
    g = torch.Generator(device=DEV).manual_seed(1000 * P + 10 * M + K)
    obs = torch.randn(M, K, device=DEV, generator=g) * 3 + 0.5
    mean = torch.randn(K, device=DEV, generator=g) * 0.5
    std = torch.rand(K, device=DEV, generator=g) * 2 + 0.1
    pnet, vnet = _policy(K, P, seed=P + M + K), _value(K, seed=P + M + K)
    for norm in (True, False):
        x64 = (obs.double() - mean.double()) / std.double() if norm else obs.double()
        x32 = (obs - mean) / std if norm else obs
        p64, pp64 = _ref(x64, pnet, torch.float64)
        p32, pp32 = _ref(x32, pnet, torch.float32)
        v64, vp64 = _ref(x64, vnet, torch.float64)
        v32, vp32 = _ref(x32, vnet, torch.float32)
        for with_value in (False, True):
            print(f"P={P} M={M} K={K} normaliser={norm} value={with_value}")
            pol, val, ppre, vpre = hip.mlp_forward(obs, mean if norm else None, std if norm else None, _wb(pnet),
                                                   _wb(vnet) if with_value else None, want_pre=True)
            assert pol.shape == (M, P) and ppre.shape == (4, M, 32) and torch.isfinite(pol).all()
            _within("logits", pol, p32, p64)
            for l in range(4):
                _within(f"policy z{l}", ppre[l], pp32[l], pp64[l])
            if with_value:
                _within("values", val, v32.squeeze(-1), v64.squeeze(-1))
                for l in range(5):
                    _within(f"value z{l}", vpre[l], vp32[l], vp64[l])
            else:
                assert val is None and vpre is None


@pytest.mark.parametrize("P,cuts", [(128, [(0, 64), (64, 128)]), (76, [(0, 60)]), (65, [(0, 64), (64, 65)])])
def test_columns_of_a_wide_head_equal_the_narrow_network_bitwise(P, cuts):
    """The two passes are independent per column: logits[:, a:b] of the wide head equal, bit for bit, the output of the network whose
    head has rows a .. b-1 only (<= 64 of them: the one-pass path).  Catches a mis-staged second half at its edges."""
    from rodent_amd import hip
    M, K = 100, 211
    g = torch.Generator(device=DEV).manual_seed(P)
    obs = torch.randn(M, K, device=DEV, generator=g) * 2 + 0.3
    mean, std = torch.randn(K, device=DEV, generator=g) * 0.3, torch.rand(K, device=DEV, generator=g) + 0.5
    pnet, vnet = _policy(K, P, seed=P), _value(K, seed=P)
    for value in (None, _wb(vnet)):
        wide = hip.mlp_forward(obs, mean, std, _wb(pnet), value, want_pre=True)
        for a, b in cuts:
            ws, bs = _wb(pnet)
            narrow = hip.mlp_forward(obs, mean, std, (ws[:-1] + [ws[-1][a:b].contiguous()], bs[:-1] + [bs[-1][a:b].contiguous()]), value,
                                     want_pre=True)
            assert narrow[0].shape == (M, b - a)
            assert torch.equal(wide[0][:, a:b], narrow[0]), (P, a, b)
            assert torch.equal(wide[2], narrow[2])
            if value is not None:
                assert torch.equal(wide[1], narrow[1]) and torch.equal(wide[3], narrow[3])


@pytest.mark.parametrize("M,extra", [(333, 0), (50, 7)])
@pytest.mark.parametrize("P", [65, 76, 128])
def test_policy_backward_chain_kernel(P, M, extra):
    """rr_policy_backward at P > 64 against float64: delta_j, h_j = silu(z_j), db_j; the rows behind the first M are left alone."""
    from rodent_amd import hip
    nh, H = 4, 32
    g = torch.Generator().manual_seed(M + P)
    z = torch.randn(nh, M + extra, H, generator=g) * 1.5
    Ws = [None] + [torch.randn(H, H, generator=g) / 5 for _ in range(1, nh)]
    wh = torch.randn(P, H, generator=g) / 5
    gl = torch.randn(M, P, generator=g)

    def chain(dt, dev):
        c = lambda x: x.to(dt).to(dev)
        zz = c(z[:, :M])
        s = torch.sigmoid(zz)
        sp, hh = s * (1 + zz * (1 - s)), zz * s
        d = [None] * nh
        d[nh - 1] = (c(gl) @ c(wh)) * sp[nh - 1]
        for j in range(nh - 1, 0, -1):
            d[j - 1] = (d[j] @ c(Ws[j])) * sp[j - 1]
        return torch.stack(d).double().cpu(), hh.double().cpu()
    d64, h64 = chain(torch.float64, "cpu")
    d32, _ = chain(torch.float32, DEV)
    pre = z.to(DEV).contiguous()
    bgs = [torch.empty(H, device=DEV) for _ in range(nh)]
    delta, h = hip.policy_backward(gl.to(DEV), wh.to(DEV), [None] + [Ws[j].to(DEV) for j in range(1, nh)], pre, bgs)
    torch.cuda.synchronize()
    assert (h[:, :M].double().cpu() - h64).abs().max() <= 2e-6 * h64.abs().max()
    assert torch.equal(h[:, M:].cpu(), z[:, M:])                                   # untouched
    for j in range(nh):
        scale = d64[j].abs().max()
        err, err32 = (delta[j].double().cpu() - d64[j]).abs().max() / scale, (d32[j] - d64[j]).abs().max() / scale
        print(f"P={P} M={M} layer {j}: policy chain {err:.2e}  torch-f32 {err32:.2e}")
        assert err <= 3 * err32 + 2e-6, (j, float(err), float(err32))
        assert (bgs[j].double().cpu() - d64[j].sum(0)).abs().max() <= 3e-5 * d64[j].abs().sum(0).max(), j


@pytest.mark.parametrize("T,B,R", [(3, 8, 8), (7, 130, 200)])
@pytest.mark.parametrize("A", [38, 64])
def test_loss_kernel_at_more_than_32_actions(A, T, B, R):
    """rr_ppo_loss loops `a += 32` over any A: pinned at the self-collision model's 38 actions and at 64."""
    from rodent_amd import hip
    data, logits, values, noise, idx = _batch(T, B, R, A, seed=T * 1000 + B + A)
    if R == B:
        idx = None
    m64, gl64, gv64 = _reference(data, logits, values, noise, idx, T, B, A, torch.float64, "cpu", True)
    m32, gl32, gv32 = _reference(data, logits, values, noise, idx, T, B, A, torch.float32, DEV, True)
    dd = {k: v.to(DEV).contiguous() for k, v in data.items()}
    gl, gv, m = hip.ppo_loss(logits.to(DEV), values.to(DEV), dd, idx.to(DEV) if idx is not None else None, noise.to(DEV), T,
                             normalize_advantage=True, **CFG)
    torch.cuda.synchronize()
    gl, gv, m = gl.double().cpu(), gv.double().cpu(), m.double().cpu()
    assert torch.isfinite(gl).all() and torch.isfinite(gv).all()
    assert (gl[T * B:] == 0).all() and (gv[T * B:] == 0).all()                 # bootstrap rows
    for name, got, t32, want in (("logits", gl, gl32, gl64), ("values", gv, gv32, gv64), ("metrics", m, m32, m64)):
        scale = want.abs().max()
        err, err32 = (got - want).abs().max() / scale, (t32 - want).abs().max() / scale
        print(f"T={T} B={B} A={A} {name}: fused {err:.2e}  torch-f32 {err32:.2e}  (relative to max |.|)")
        assert err <= 3 * err32 + 2e-6, (name, float(err), float(err32))
    assert (gl64[:T * B].abs().sum(1) > 0).all()


@pytest.mark.parametrize("N", [3 * 8, 7 * 130])
@pytest.mark.parametrize("A", [38, 64])
def test_sample_kernel_at_more_than_32_actions(A, N):
    from rodent_amd import hip
    from rodent_amd.training.networks import NormalTanhDistribution
    g = torch.Generator().manual_seed(A + N)
    logits, eps = torch.randn(N, 2 * A, generator=g) * 0.8, torch.randn(N, A, generator=g)
    dist = NormalTanhDistribution(A)
    loc, scale = dist._params(logits.double())
    raw64 = loc + scale * eps.double()
    act64, lp64 = torch.tanh(raw64), dist.log_prob(logits.double(), raw64)
    loc32, scale32 = dist._params(logits)
    lp32 = dist.log_prob(logits, loc32 + scale32 * eps).double()
    act, raw, lp = hip.policy_sample(logits.to(DEV), eps.to(DEV), dist.min_std)
    torch.cuda.synchronize()
    assert (raw.double().cpu() - raw64).abs().max() <= 2e-6 * raw64.abs().max()
    assert (act.double().cpu() - act64).abs().max() <= 2e-6
    err, err32 = (lp.double().cpu() - lp64).abs().max(), (lp32 - lp64).abs().max()
    print(f"A={A} N={N} log_prob: kernel {err:.2e}  composed float32 {err32:.2e}  (|log_prob| up to {lp64.abs().max():.1f})")
    assert err <= 3 * err32 + 1e-5


@pytest.mark.parametrize("use_rows", [False, True])
@pytest.mark.parametrize("M,K", [(100, 333), (1, 1263)])
@pytest.mark.parametrize("A", [33, 38, 64])
def test_policy_act_two_launches(A, M, K, use_rows):
    """rr_policy_act with 33 .. 64 actions (head [32][128] in LDS, two action dimensions per lane) against the float64 policy; stochastic and
    deterministic, optional row indirection; its logits against rr_mlp_forward's on the same rows."""
    from rodent_amd import hip
    from rodent_amd.training import fused_mlp, networks
    torch.manual_seed(M + K + A)
    nets = networks.make_ppo_networks(K, A, device=DEV)
    net, dist = nets.policy_network, nets.parametric_action_distribution
    for l in net.layers:
        l.bias.data.uniform_(-0.2, 0.2)
    R = M + 50 if use_rows else M
    obs = torch.randn(R, K, device=DEV) * 2 + 0.3
    rows = torch.randperm(R, device=DEV)[:M] if use_rows else None
    mean, std = torch.randn(K, device=DEV) * 0.3, torch.rand(K, device=DEV) + 0.5
    eps = torch.randn(M, A, device=DEV)
    x = obs[rows] if use_rows else obs
    net64 = copy.deepcopy(net).double()
    with torch.no_grad():
        lg64 = net64((x.double() - mean.double()) / std.double())
        lg32 = net((x - mean) / std).double()
    loc, scale = dist._params(lg64)
    raw64 = loc + scale * eps.double()
    lp64 = dist.log_prob(lg64, raw64)
    act, raw, lp, lg = hip.policy_act(obs, mean, std, fused_mlp.net_params(net), eps, dist.min_std, want_logits=True, rows=rows)
    torch.cuda.synchronize()
    assert lg.shape == (M, 2 * A) and act.shape == (M, A)
    scale_l = lg64.abs().max()
    err, err32 = (lg.double() - lg64).abs().max() / scale_l, (lg32 - lg64).abs().max() / scale_l
    print(f"A={A} M={M} K={K}: logits two-launch {float(err):.2e}  nn.Linear f32 {float(err32):.2e}")
    assert err <= 3 * err32 + 2e-6
    tol = 20 * float(err.clamp_min(1e-7)) * float(scale_l)                      # what the logits' error can do to the head's outputs
    assert (raw.double() - raw64).abs().max() <= tol + 1e-5
    assert (act.double() - torch.tanh(raw64)).abs().max() <= tol + 1e-5
    assert (lp.double() - lp64).abs().max() <= 50 * tol + 1e-4
    act_d, raw_d, lp_d, lg_d = hip.policy_act(obs, mean, std, fused_mlp.net_params(net), None, dist.min_std, want_logits=True, rows=rows)
    assert raw_d is None and lp_d is None and torch.equal(lg_d, lg)
    assert (act_d.double() - torch.tanh(loc)).abs().max() <= tol + 1e-5
    fwd = hip.mlp_forward(obs, mean, std, policy=fused_mlp.net_params(net), rows=rows)[0]
    gap = (lg.double() - fwd.double()).abs().max() / scale_l
    print(f"  logits two-launch vs rr_mlp_forward: {float(gap):.2e}")
    assert gap <= 3 * err32 + 2e-6


def test_fused_update_equals_the_autograd_path_at_38_actions():
    """FusedUpdate on a 76-logit policy fills the flat gradient buffer with what compute_ppo_loss + backward produce."""
    from rodent_amd.training import distributed as D, fused_mlp, networks
    from rodent_amd.training.agents.ppo import fused_update, losses
    torch.manual_seed(0)
    T, B, R, K, A = 6, 96, 300, 211, 38
    nets = networks.make_ppo_networks(K, A, device=DEV)
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
    gen = torch.Generator(device=DEV).manual_seed(77)
    m_f = fu(data, idx, mean, std, gen)
    got = flat.flat.clone()
    m_f = {k: float(v) for k, v in m_f.items()}
    # the path it replaces (compute_ppo_loss + autograd on the same forward), same noise stream
    gen = torch.Generator(device=DEV).manual_seed(77)
    mbd = {k: data[k][idx].transpose(0, 1) for k in ("raw_action", "log_prob", "reward", "discount", "truncation")}
    raw = data["obs"][idx].transpose(0, 1)
    logits_all, values_all = fused_mlp.actor_critic(raw.reshape((T + 1) * B, -1), mean, std, pnet, vnet)
    values = values_all.reshape(T + 1, B)
    loss, m = losses.compute_ppo_loss(logits_all[:T * B].reshape(T, B, -1), values[:T], values[T], mbd, dist, normalize_advantage=True,
                                      generator=gen, **CFG)
    flat.zero_()
    loss.backward()
    want = flat.flat.clone()
    o = 0
    for p in params:                                           # per tensor: the scales differ by orders of magnitude
        a, b = got[o:o + p.numel()], want[o:o + p.numel()]
        o += p.numel()
        assert torch.isfinite(a).all()
        assert (a - b).abs().max() <= 2e-4 * b.abs().max() + 1e-9, (tuple(p.shape), float((a - b).abs().max()), float(b.abs().max()))
    for k in m_f:
        assert abs(m_f[k] - float(m[k])) <= 1e-5 * max(1.0, abs(float(m[k]))), (k, m_f[k], float(m[k]))


def test_fused_update_equals_the_autograd_path_at_38_actions_on_policy(monkeypatch):
    """The same on a 76-logit policy with the switch that sends `ppo.train`'s learner this way, on a batch with rho ~ 1: the policy term,
    not the entropy term alone, goes through the two-pass head forward and the four-segment `rr_policy_backward`."""
    monkeypatch.setenv("RR_FUSED_WIDE_HEAD", "1")
    fused_update_on_an_on_policy_batch(38)


MODEL = "rodent_cpu.xml"
TRAIN = dict(num_timesteps=10 ** 9, episode_length=150, num_envs=64, batch_size=64, num_minibatches=4, unroll_length=5, num_updates_per_batch=2,
             num_evals=2, num_eval_envs=0, entropy_cost=1e-3, discounting=0.97, normalize_observations=True)


def _train(monkeypatch, wide, steps, lr, seed, count=None):
    from rodent_amd import envs, hip
    from rodent_amd.training import acting
    from rodent_amd.training.agents.ppo import train as ppo
    if wide:
        monkeypatch.setenv("RR_FUSED_WIDE_HEAD", "1")
    else:
        monkeypatch.delenv("RR_FUSED_WIDE_HEAD", raising=False)
    if count is not None:                      # wrappers that count and pass through
        for mod, name in ((hip, "mlp_forward"), (hip, "ppo_loss"), (hip, "policy_backward"), (hip, "policy_act"), (hip, "policy_sample"),
                          (acting, "generate_unrolls_fused"), (acting, "generate_unroll")):
            def counted(*a, _f=getattr(mod, name), _n=name, **k):
                count[_n] = count.get(_n, 0) + 1
                return _f(*a, **k)
            monkeypatch.setattr(mod, name, counted)
    env = envs.get_environment("rodent", track_pos=util.synthetic_track(), num_envs=64, xml_path=MODEL, iterations=6, ls_iterations=6, device=DEV)
    log = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)           # the contact-overflow warning is allowed, not required
        _, params, _ = ppo.train(environment=env, learning_rate=lr, seed=seed, max_training_steps=steps, progress_fn=lambda n, m: log.append(m),
                                 **TRAIN)
    return params, log


@pytest.mark.parametrize("wide", [True, False])
def test_ppo_train_on_the_self_collision_model_with_and_without_the_switch(monkeypatch, wide):
    """RR_FUSED_WIDE_HEAD=1 sends the 76-logit learner through rr_mlp_forward / rr_ppo_loss / rr_policy_backward; unset, none of the
    learner kernels is called (the behaviour before the switch existed).  Either way the rollouts are one launch per training step."""
    count = {}
    params, log = _train(monkeypatch, wide, steps=2, lr=5e-5, seed=1, count=count)
    print(count)
    assert count.get("generate_unrolls_fused") == 2 and "generate_unroll" not in count
    for name in ("mlp_forward", "ppo_loss", "policy_backward"):
        assert (count.get(name, 0) >= 1) == wide, (name, count)
    assert "policy_act" not in count and "policy_sample" not in count          # no per-step actor: the rollout's actor is inside the step kernel
    assert math.isfinite(float(log[-1]["training/total_loss"])) and float(params[0].count) == 64 * 4 * 5 * 2


def test_wide_head_learner_trains_like_the_autograd_path(monkeypatch):
    """ONE training step of ppo.train on rodent_cpu.xml with the switch on and off, same seed, same rollout (the in-kernel actor either way),
    compared as tests/test_gpu_ppo.py compares the hand-written update with autograd: parameter DISPLACEMENTS from the common initial point
    (a third run with lr = 0) point the same way, differ by a bounded number of Adam steps, and the last minibatch's losses agree."""
    lr, out, loss = 5e-5, {}, {}
    for mode, wide, rate in (("init", True, 0.0), ("on", True, lr), ("off", False, lr)):
        params, log = _train(monkeypatch, wide, steps=1, lr=rate, seed=1)
        out[mode] = torch.cat([p.detach().reshape(-1) for p in params[1].parameters()]).double()
        loss[mode] = {k: float(v) for k, v in log[-1].items() if k.startswith("training/") and k.endswith("loss")}
    k = TRAIN["num_minibatches"] * TRAIN["num_updates_per_batch"]
    d1, d0 = out["on"] - out["init"], out["off"] - out["init"]
    cos = float((d1 * d0).sum() / (d1.norm() * d0.norm()))
    diff = (out["on"] - out["off"]).abs()
    print(f"displacement cosine {cos:.4f}; |displacement| {float(d1.norm()):.3e} / {float(d0.norm()):.3e}; max |param diff| "
          f"{float(diff.max()) / lr:.2f} lr; losses {loss['on']} vs {loss['off']}")
    assert float(d0.norm()) > 0 and cos > 0.9
    assert float(diff.max()) <= 2 * k * lr
    for name in loss["off"]:
        assert abs(loss["on"][name] - loss["off"][name]) <= 5e-3 * max(abs(loss["off"][name]), 1e-2), name


def test_heads_wider_than_128_are_refused():
    from rodent_amd import hip
    M, K, P = 8, 64, 130
    net = _policy(K, P, seed=0)
    obs = torch.randn(M, K, device=DEV)
    with pytest.raises(RuntimeError, match="rr_mlp_forward.*130"):
        hip.mlp_forward(obs, None, None, policy=_wb(net))
    with pytest.raises(RuntimeError, match="rr_policy_act.*130"):
        hip.policy_act(obs, None, None, _wb(net), None, 1e-3)
    pre = torch.zeros(4, M, 32, device=DEV)
    with pytest.raises(RuntimeError, match="rr_policy_backward.*130"):
        hip.policy_backward(torch.zeros(M, P, device=DEV), net.layers[-1].weight.detach(), [None] + [l.weight.detach() for l in net.layers[1:4]], pre,
                            [torch.empty(32, device=DEV) for _ in range(4)])
    odd = _policy(K, 77, seed=0)                         # an odd head has no (loc | scale) halves
    with pytest.raises(RuntimeError, match="rr_policy_act.*77"):
        hip.policy_act(obs, None, None, _wb(odd), None, 1e-3)
