"""GPU: a policy network whose hidden layers are all 256 wide on the hand-written kernels -- `rr_mlp_forward`'s second policy width
(rr_mlp_policy256_forward_kernel), the delta chain `rr_mlp_policy_backward`, `FusedUpdate`'s dispatch on the width, `make_inference_fn`'s
two-launch actor step and `ppo.train` through a real HIP env.

Criterion unless stated: `ppo_batches.assert_global_criterion`, max |got - f64| <= 3 max |torch-f32 - f64| + 2e-6 relative to max |f64|, with
f64 = torch float64 on the float32-rounded parameters and inputs and the yardstick torch's own float32 path."""
import math
import warnings

import pytest
import torch

from tests import ppo_batches, util
from tests.ppo_batches import CFG, _batch, _reference, assert_global_criterion

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _policy(K, P, depth, seed=0):
    from rodent_amd.training import networks
    torch.manual_seed(seed)
    net = networks.MLP(K, [256] * depth + [P]).to(DEV)
    for lin in net.layers:                                   # non-zero biases so the bias path is exercised
        torch.nn.init.uniform_(lin.bias, -0.1, 0.1)
    return net


def _value(K, seed=1, depth=2):
    from rodent_amd.training import networks
    torch.manual_seed(seed)
    net = networks.MLP(K, [256] * depth + [1]).to(DEV)
    for lin in net.layers:
        torch.nn.init.uniform_(lin.bias, -0.1, 0.1)
    return net


def _wb(net):
    return [l.weight.detach() for l in net.layers], [l.bias.detach() for l in net.layers]


def _ref(x, net, dtype):
    """(logits, [pre-activations]) of `net` on x in `dtype` (torch, on the GPU)."""
    x = x.to(dtype)
    pre = []
    for i, l in enumerate(net.layers):
        x = x @ l.weight.detach().to(dtype).t() + l.bias.detach().to(dtype)
        if i < len(net.layers) - 1:
            pre.append(x)
            x = torch.nn.functional.silu(x)
    return x, pre


_OBS = {}


def _obs(K):
    """One observation block per width, shared by the tests and never written: [333, K], with a normaliser."""
    if K not in _OBS:
        g = torch.Generator(device=DEV).manual_seed(K)
        _OBS[K] = (torch.randn(333, K, device=DEV, generator=g) * 2 + 0.5, torch.randn(K, device=DEV, generator=g) * 0.3,
                   torch.rand(K, device=DEV, generator=g) + 0.5)
    return _OBS[K]


@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("P", [2, 60, 65, 128])
@pytest.mark.parametrize("depth", [1, 4])
@pytest.mark.parametrize("K", [211, 1263])
@pytest.mark.parametrize("M", [1, 33, 100])
def test_forward_against_torch(M, K, depth, P, norm):
    """M = 1: every staged row is a clamped duplicate; 33: a second tile of one row; K = 211: partial last chunk; depth 1: the head
    directly after layer 1; P = 65: one column in the third wave's tile, 2: one tile nearly empty, 128: all four full."""
    from rodent_amd import hip
    obs, mean, std = _obs(K)
    obs = obs[:M].contiguous()
    if not norm:
        mean = std = None
    net = _policy(K, P, depth, seed=depth * 1000 + P)
    pol, val, pre, vpre = hip.mlp_forward(obs, mean, std, policy=_wb(net), want_pre=True)
    torch.cuda.synchronize()
    assert val is None and vpre is None and pol.shape == (M, P) and pre.shape == (depth, M, 256)
    x64 = (obs.double() - mean.double()) / std.double() if norm else obs.double()
    x32 = (obs - mean) / std if norm else obs
    l64, z64 = _ref(x64, net, torch.float64)
    l32, z32 = _ref(x32, net, torch.float32)
    label = f"M={M} K={K} depth={depth} P={P} norm={norm}"
    assert torch.isfinite(pol).all() and torch.isfinite(pre).all()
    assert_global_criterion("logits", pol.double(), l32.double(), l64, label)
    for j in range(depth):
        assert_global_criterion(f"z{j}", pre[j].double(), z32[j].double(), z64[j], label)


def test_same_instance_everywhere():
    """Bitwise: the policy's launch does not depend on the value network being in the call, on `rows`, or on the row count of the call (the
    rollout evaluates M = 100 rows, the learner the same rows inside a larger minibatch); the value outputs are a value-only call's."""
    from rodent_amd import hip
    K, P = 211, 60
    obs, mean, std = _obs(K)
    pnet, vnet = _policy(K, P, 2), _value(K)
    only_p = hip.mlp_forward(obs, mean, std, policy=_wb(pnet), want_pre=True)
    only_v = hip.mlp_forward(obs, mean, std, value=_wb(vnet), want_pre=True)
    both = hip.mlp_forward(obs, mean, std, _wb(pnet), _wb(vnet), want_pre=True)
    assert torch.equal(both[0], only_p[0]) and torch.equal(both[2], only_p[2])
    assert torch.equal(both[1], only_v[1]) and torch.equal(both[3], only_v[3])
    g = torch.Generator(device=DEV).manual_seed(3)
    rows = torch.randperm(333, device=DEV, generator=g)[:77]
    by_rows = hip.mlp_forward(obs, mean, std, policy=_wb(pnet), want_pre=True, rows=rows)
    gathered = hip.mlp_forward(obs[rows].contiguous(), mean, std, policy=_wb(pnet), want_pre=True)
    assert torch.equal(by_rows[0], gathered[0]) and torch.equal(by_rows[2], gathered[2])
    sel = torch.arange(100, device=DEV) * 3 + 7                      # 100 rows scattered over the 333, other tile positions
    small = hip.mlp_forward(obs[sel].contiguous(), mean, std, policy=_wb(pnet))[0]
    assert torch.equal(small, only_p[0][sel])


@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("P", [60, 65, 128])
@pytest.mark.parametrize("n,extra", [(333, 0), (50, 7)])
def test_backward_chain(n, extra, P, depth):
    """Every delta_j, h_j = silu(z_j) written over the dump and every bias gradient against float64 autograd (yardstick: float32 autograd);
    the rows beyond n of the dump are bitwise untouched.  P = 65: five k-chunks, the last holding one column; 60: a partial fourth."""
    from rodent_amd import hip
    K = 211
    M = n + extra
    obs = _obs(K)[0][:M].contiguous()
    net = _policy(K, P, depth, seed=P + depth)
    g = torch.Generator(device=DEV).manual_seed(n + P)
    G = torch.randn(n, P, device=DEV, generator=g)
    _, _, pre, _ = hip.mlp_forward(obs, None, None, policy=_wb(net), want_pre=True)
    before = pre.clone()
    layers = net.layers
    bg = [torch.empty(256, device=DEV) for _ in range(depth)]
    delta, h = hip.mlp_policy_backward(G, layers[depth].weight.detach().t().contiguous(),
                                       [None] + [layers[j].weight.detach().t().contiguous() for j in range(1, depth)], pre, bg)
    torch.cuda.synchronize()
    assert h.data_ptr() == pre.data_ptr() and delta.shape == (depth, n, 256)
    assert torch.equal(h[:, n:], before[:, n:])

    def autograd(dtype):
        """(d loss / d z_j, silu(z_j)) of the stack above the dump's first layer, loss = sum(logits * G)."""
        z = before[0, :n].to(dtype).clone().requires_grad_(True)
        zs = []
        for j in range(depth):
            zs.append(z)
            lin = layers[j + 1]
            z = torch.nn.functional.silu(z) @ lin.weight.detach().to(dtype).t() + lin.bias.detach().to(dtype)
            if j + 1 < depth:
                z.retain_grad()
        (z * G.to(dtype)).sum().backward()
        return [k.grad for k in zs], [torch.nn.functional.silu(k.detach()) for k in zs]

    d64, h64 = autograd(torch.float64)
    d32, h32 = autograd(torch.float32)
    label = f"n={n}+{extra} P={P} depth={depth}"
    # both references run from the dump's first layer z_0 (float32-rounded input); the kernel's deeper z_j are its own forward's
    for j in range(depth):
        assert_global_criterion(f"delta{j}", delta[j].double(), d32[j].double(), d64[j], label)
        assert_global_criterion(f"h{j}", h[j, :n].double(), h32[j].double(), h64[j], label)
        assert_global_criterion(f"db{j}", bg[j].double(), d32[j].double().sum(0), d64[j].sum(0), label)


def test_fused_update_equals_the_autograd_path():
    """One minibatch, A = 30, T = 7, B = 130, R = 200, policy (256, 256), default value network: coverage of the clipped surrogate's classes
    by float64 networks on the CPU, d loss / d logits per row, every parameter gradient and the metrics against compute_ppo_loss + backward."""
    from rodent_amd import hip
    from rodent_amd.training import distributed as D, fused_mlp, networks
    from rodent_amd.training.agents.ppo import fused_update, losses
    import copy
    torch.manual_seed(0)
    T, B, R, K, A = 7, 130, 200, 211, 30
    nets = networks.make_ppo_networks(K, A, policy_hidden_layer_sizes=(256, 256), device=DEV)
    pnet, vnet, dist = nets.policy_network, nets.value_network, nets.parametric_action_distribution
    assert fused_mlp.policy_width(pnet) == 256
    params = list(pnet.parameters()) + list(vnet.parameters())
    flat = D.FlatGrads(params)
    g = torch.Generator(device=DEV).manual_seed(1)
    idx = _batch(T, B, R, A, seed=9)[4].to(DEV)
    obs = torch.randn(R, T + 1, K, device=DEV, generator=g) * 2 + 0.5
    mean, std = torch.randn(K, device=DEV, generator=g) * 0.3, torch.rand(K, device=DEV, generator=g) + 0.5
    rows = (idx.unsqueeze(0) * (T + 1) + torch.arange(T + 1, device=DEV).unsqueeze(1)).reshape(-1)
    with torch.no_grad():
        cur, val = hip.mlp_forward(obs.reshape(-1, K), mean, std, fused_mlp.net_params(pnet), fused_mlp.net_params(vnet), rows=rows)[:2]

    def sampler(logits, eps):
        _, raw, lp = hip.policy_sample(logits.to(DEV).contiguous(), eps.to(DEV).contiguous(), 0.001)
        return raw, lp
    data, cur, _, _, _ = ppo_batches.onpolicy_batch(T, B, R, A, seed=9, sampler=sampler, logits=cur)
    # coverage by the reference alone: float64 copies of the networks on the CPU
    with torch.no_grad():
        x64 = (obs.reshape(-1, K)[rows].double().cpu() - mean.double().cpu()) / std.double().cpu()
        lg64, v64 = copy.deepcopy(pnet).cpu().double()(x64), copy.deepcopy(vnet).cpu().double()(x64).squeeze(-1)
    rho, adv = ppo_batches.rho_and_advantage64(data, lg64, v64, idx.cpu(), T, B, A, True, CFG)
    kept = ppo_batches.assert_coverage(rho, adv, CFG["clipping_epsilon"], T, B, A, "FusedUpdate policy 256 x 2")
    data = {k: v.to(DEV).contiguous() for k, v in data.items()}
    data["obs"] = obs
    fu = fused_update.FusedUpdate(pnet, vnet, dist, T, normalize_advantage=True, **CFG)
    gen = torch.Generator(device=DEV).manual_seed(77)
    m_f = fu(data, idx, mean, std, gen)
    torch.cuda.synchronize()
    got = flat.flat.clone()
    m_f = {k: float(v) for k, v in m_f.items()}
    # d loss / d logits per row, at the logits and values FusedUpdate's own forward produced, with its noise draw
    noise = torch.randn(T * B, A, device=DEV, generator=torch.Generator(device=DEV).manual_seed(77)).cpu()
    cpu_data = {k: v.cpu() for k, v in data.items() if k != "obs"}
    _, gl64, _ = _reference(cpu_data, cur, val.cpu(), noise, idx.cpu(), T, B, A, torch.float64, "cpu", True, CFG)
    _, gl32, _ = _reference(cpu_data, cur, val.cpu(), noise, idx.cpu(), T, B, A, torch.float32, DEV, True, CFG)
    ppo_batches.assert_rowrel_criterion(fu.bufs["grad_logits"].double().cpu(), gl32, gl64, kept, "FusedUpdate policy 256 x 2")
    # the path it replaces, same noise stream
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
        print(tuple(p.shape), f"max |diff| {float((a - b).abs().max()):.3e}  max |grad| {float(b.abs().max()):.3e}")
        assert (a - b).abs().max() <= 2e-4 * b.abs().max() + 1e-9, (tuple(p.shape), float((a - b).abs().max()), float(b.abs().max()))
    for k in m_f:
        assert abs(m_f[k] - float(m[k])) <= 1e-5 * max(1.0, abs(float(m[k]))), (k, m_f[k], float(m[k]))


def test_seven_hidden_layers_on_one_stream(monkeypatch):
    """The deepest policy served (7 hidden layers, 8 weight-gradient products) next to the default value network (6): on one stream
    (RR_LEARNER_STREAMS=0) the 14 products exceed one `rr_mlp_weight_grad_batch` call's 12 and go as one call per network -- the calls
    the two-stream path makes, so the gradients are the same bit for bit -- and they agree with the autograd path as in the test above."""
    from rodent_amd.training import distributed as D, fused_mlp, networks
    from rodent_amd.training.agents.ppo import fused_update, losses
    torch.manual_seed(2)
    T, B, R, K, A = 3, 40, 60, 211, 30
    nets = networks.make_ppo_networks(K, A, policy_hidden_layer_sizes=(256,) * 7, device=DEV)
    pnet, vnet, dist = nets.policy_network, nets.value_network, nets.parametric_action_distribution
    params = list(pnet.parameters()) + list(vnet.parameters())
    flat = D.FlatGrads(params)
    g = torch.Generator(device=DEV).manual_seed(1)
    data, _, _, _, idx = _batch(T, B, R, A, seed=5)
    data = {k: v.to(DEV).contiguous() for k, v in data.items()}
    data["obs"] = torch.randn(R, T + 1, K, device=DEV, generator=g) * 2 + 0.5
    idx = idx.to(DEV)
    mean, std = torch.randn(K, device=DEV, generator=g) * 0.3, torch.rand(K, device=DEV, generator=g) + 0.5
    got = {}
    for streams in ("1", "0"):
        monkeypatch.setenv("RR_LEARNER_STREAMS", streams)
        fu = fused_update.FusedUpdate(pnet, vnet, dist, T, normalize_advantage=True, **CFG)
        assert (fu.side is None) == (streams == "0")
        flat.zero_()
        fu(data, idx, mean, std, torch.Generator(device=DEV).manual_seed(77))
        torch.cuda.synchronize()
        got[streams] = flat.flat.clone()
    assert torch.isfinite(got["0"]).all() and torch.equal(got["0"], got["1"])
    gen = torch.Generator(device=DEV).manual_seed(77)
    mbd = {k: data[k][idx].transpose(0, 1) for k in ("raw_action", "log_prob", "reward", "discount", "truncation")}
    logits_all, values_all = fused_mlp.actor_critic(data["obs"][idx].transpose(0, 1).reshape((T + 1) * B, -1), mean, std, pnet, vnet)
    values = values_all.reshape(T + 1, B)
    loss, _ = losses.compute_ppo_loss(logits_all[:T * B].reshape(T, B, -1), values[:T], values[T], mbd, dist, normalize_advantage=True, generator=gen, **CFG)
    flat.zero_()
    loss.backward()
    want, o = flat.flat.clone(), 0
    for p in params:
        a, b = got["0"][o:o + p.numel()], want[o:o + p.numel()]
        o += p.numel()
        assert (a - b).abs().max() <= 2e-4 * b.abs().max() + 1e-9, (tuple(p.shape), float((a - b).abs().max()), float(b.abs().max()))


TRAIN = dict(num_timesteps=10 ** 9, episode_length=10, num_envs=64, batch_size=32, num_minibatches=2, unroll_length=5, num_updates_per_batch=1,
             num_evals=2, num_eval_envs=0, entropy_cost=1e-3, discounting=0.97, normalize_observations=True)


def _train(monkeypatch, steps, env=(), count=None, updates=1, seed=1, lr=5e-5):
    from rodent_amd import envs, hip
    from rodent_amd.training import acting, networks
    from rodent_amd.training.agents.ppo import train as ppo
    monkeypatch.setenv("RR_FUSED_POLICY256", "1")
    for k in ("RR_FUSED_LOSS", "RR_PPO_GRAPH"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)
    if count is not None:                      # wrappers that count and pass through
        for mod, name in ((hip, "mlp_forward"), (hip, "mlp_policy_backward"), (hip, "policy_backward"), (hip, "policy_act"), (hip, "policy_sample"),
                          (acting, "generate_unrolls_fused"), (acting, "generate_unroll")):
            def counted(*a, _f=getattr(mod, name), _n=name, **k):
                count[_n] = count.get(_n, 0) + 1
                return _f(*a, **k)
            monkeypatch.setattr(mod, name, counted)
    e = envs.get_environment("rodent", track_pos=util.synthetic_track(), num_envs=64, xml_path="rodent_optimized.xml", iterations=4, ls_iterations=4,
                             device=DEV)
    factory = lambda obs_size, act_size, **kw: networks.make_ppo_networks(obs_size, act_size, policy_hidden_layer_sizes=(256, 256), **kw)
    log = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        make_policy, params, _ = ppo.train(environment=e, learning_rate=lr, seed=seed, max_training_steps=steps, network_factory=factory,
                                           progress_fn=lambda n, m: log.append(m), **dict(TRAIN, num_updates_per_batch=updates))
    return make_policy, params, log, e


def test_training_uses_the_fused_update_and_follows_the_autograd_path(monkeypatch):
    """64 envs, episode length 10, unroll 5, 2 minibatches, policy (256, 256): the learner calls `hip.mlp_policy_backward` (never the 32-wide
    chain), the rollouts are per-step (`generate_unroll`; the in-kernel actor does not serve the shape), and the losses after the first and
    after the second training step are within 5e-3 relative of the run whose learner is compute_ppo_loss + backward (RR_FUSED_LOSS=0), same
    seed.  (`progress_fn` reports the last step of a run: the first step's losses come from a run of one step.)

    The first step is compared at lr = 5e-5, the second at lr = 0, for a reason that lies in the setup and not in the kernels: the two
    learners can only be compared on the same data.  Adam divides by the gradient's magnitude, so a parameter whose gradient is rounding
    noise around zero moves by +-lr per update with the sign of the noise: after the two updates of the first step the parameters of the two
    runs differ by up to 4 lr whatever computed the gradients (measured: 3.96 lr with the 32-wide policy on the kernels the project already
    had, 3.98 lr here).  The normaliser then holds the statistics of 320 observations, with columns whose deviation is at its floor, and the
    second rollout is very sensitive to the parameters: at lr = 1e-7 the sum of the second rollout's raw actions is -69.3 (this learner),
    -75.0 (autograd) and -82.3 at lr = 0, and the last minibatch's total loss of the two runs differs by 2.4 % (2.6 % at lr = 5e-5; 12 % at
    5e-5 with the 32-wide policy).  At lr = 0 both runs make the same second rollout (measured: equal checksums), and what is compared at the
    second step is the learner on new data with an updated normaliser, its update captured and replayed -- 1e-7 relative on the MI355X."""
    from rodent_amd.envs import wrappers
    from rodent_amd.training import acting, networks
    losses = {}
    for steps, lr in ((1, 5e-5), (2, 0.0)):
        for mode, env in (("fused", ()), ("autograd", (("RR_FUSED_LOSS", "0"),))):
            count = {} if (mode, steps) == ("fused", 2) else None
            _, params, log, e = _train(monkeypatch, steps, env, count, lr=lr)
            losses[mode, steps] = {k: float(v) for k, v in log[-1].items() if k.startswith("training/") and k.endswith("loss")}
            if count is not None:
                print(count)
                assert count.get("mlp_policy_backward", 0) == 2 * 2 and "policy_backward" not in count and "policy_act" not in count
                assert count.get("generate_unroll", 0) == 2 and "generate_unrolls_fused" not in count
                assert count.get("policy_sample", 0) == 2 * 5
                wenv = wrappers.wrap(e, episode_length=10, action_repeat=1)
                assert not acting.fused_unroll_supported(wenv, params[1], networks.NormalTanhDistribution(e.action_size))
    print(losses)
    for steps in (1, 2):
        a, b = losses["fused", steps], losses["autograd", steps]
        assert len(b) == 4
        for name in b:
            assert math.isfinite(a[name]) and abs(a[name] - b[name]) <= 5e-3 * max(abs(b[name]), 1e-2), (steps, name, a[name], b[name])
    assert losses["fused", 1] != losses["fused", 2]                     # the second step saw other data


def test_graph_replay_equals_eager_bitwise(monkeypatch, caplog):
    """Three training steps of two minibatches (six updates: the fourth is captured, the fifth and sixth replayed) leave bit for bit the
    parameters of the same run with RR_PPO_GRAPH=0."""
    out = {}
    for mode, env in (("graph", ()), ("eager", (("RR_PPO_GRAPH", "0"),))):
        _, params, _, _ = _train(monkeypatch, 3, env)
        out[mode] = torch.cat([p.detach().reshape(-1) for p in list(params[1].parameters())])
    assert "graph capture failed" not in caplog.text                     # the capture was made, not abandoned for the eager path
    assert torch.isfinite(out["graph"]).all() and torch.equal(out["graph"], out["eager"])


def test_actor_step_is_two_launches_and_on_policy(monkeypatch):
    """`make_policy(params)(obs)` on a (256, 256) policy: one `hip.mlp_forward` and one `hip.policy_sample`, nothing else of the actor
    kernels; its log_prob is the log-prob the learner's forward + float64 head give for the same raw action at unchanged parameters
    (<= 1e-4 absolute, the bound of `assert_t0_rows_on_policy`); the deterministic policy is the mode at the same logits."""
    from rodent_amd import hip
    from rodent_amd.training import fused_mlp, networks, running_statistics
    monkeypatch.setenv("RR_FUSED_POLICY256", "1")
    K, A, N = 211, 30, 100
    torch.manual_seed(4)
    nets = networks.make_ppo_networks(K, A, policy_hidden_layer_sizes=(256, 256), device=DEV)
    obs, mean, std = _obs(K)
    norm = running_statistics.init_state(K, torch.device(DEV))
    norm.mean.copy_(mean); norm.std.copy_(std)
    count = {}
    for name in ("mlp_forward", "policy_sample", "policy_act"):
        def counted(*a, _f=getattr(hip, name), _n=name, **k):
            count[_n] = count.get(_n, 0) + 1
            return _f(*a, **k)
        monkeypatch.setattr(hip, name, counted)
    make_policy = networks.make_inference_fn(nets)
    policy = make_policy((norm, nets.policy_network))
    gen = torch.Generator(device=DEV).manual_seed(5)
    action, extras = policy(obs[:N].contiguous(), gen)
    assert count == {"mlp_forward": 1, "policy_sample": 1}
    assert action.shape == (N, A) and torch.equal(action, torch.tanh(extras["raw_action"]))
    # the learner's view: the same rows inside a larger call, the log-prob of the stored action recomputed in float64
    logits = hip.mlp_forward(obs, mean, std, policy=fused_mlp.net_params(nets.policy_network))[0][:N]
    lp64 = nets.parametric_action_distribution.log_prob(logits.double(), extras["raw_action"].double())
    gap = float((extras["log_prob"].double() - lp64).abs().max())
    print(f"max |actor log_prob - learner log_prob| = {gap:.2e}")
    assert gap <= 1e-4
    det, ex = make_policy((norm, nets.policy_network), deterministic=True)(obs[:N].contiguous())
    assert ex == {} and torch.equal(det, nets.parametric_action_distribution.mode(logits))


def test_refusals():
    from rodent_amd import hip
    from rodent_amd.training import networks
    K = 64
    obs = torch.randn(8, K, device=DEV)
    for hidden in ((64, 64), (256, 32), (32, 256)):
        net = networks.MLP(K, list(hidden) + [60]).to(DEV)
        with pytest.raises(RuntimeError, match="hidden width.*32 or 256"):
            hip.mlp_forward(obs, None, None, policy=_wb(net))
    with pytest.raises(RuntimeError, match="130.*1 .. 128"):
        hip.mlp_forward(obs, None, None, policy=_wb(_policy(K, 130, 2)))
    pre = torch.zeros(2, 8, 256, device=DEV)
    wt = [None, torch.zeros(256, 256, device=DEV)]
    with pytest.raises(RuntimeError, match="rr_mlp_policy_backward.*130.*1 .. 128"):
        hip.mlp_policy_backward(torch.zeros(8, 130, device=DEV), torch.zeros(256, 130, device=DEV), wt, pre, [torch.empty(256, device=DEV) for _ in range(2)])
    pre8 = torch.zeros(8, 8, 256, device=DEV)
    with pytest.raises(RuntimeError, match="rr_mlp_policy_backward.*8 hidden layers"):
        hip.mlp_policy_backward(torch.zeros(8, 60, device=DEV), torch.zeros(256, 60, device=DEV), [None] + [wt[1]] * 7, pre8,
                                [torch.empty(256, device=DEV) for _ in range(8)])
    with pytest.raises(RuntimeError, match="rr_policy_act.*hidden width must be 32"):
        hip.policy_act(obs, None, None, _wb(_policy(K, 60, 2)), None, 1e-3)
