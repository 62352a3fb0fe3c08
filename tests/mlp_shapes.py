"""Helper of tests/test_mlp_edges_cpu.py, tests/test_gpu_mlp_edges.py and tests/test_gpu_actor_depth.py (no tests in it): networks of
any served depth, a float64 reference of the learner's and actor's MLP operations in plain torch, the suite's float32 yardstick, and the
tables of edge shapes the three files walk.

The reference is written from the formulas in the docstring of `rodent_amd/training/fused_mlp.py`, not from the kernels:

    x = (obs[rows] - mean) / std;   z_0 = x W_0' + b_0,  h_l = silu(z_l),  z_l = h_{l-1} W_l' + b_l,  out = z_L
    delta_L = G;   delta_{l-1} = (delta_l W_l) * silu'(z_{l-1});   db_l = column sums of delta_l;   dW_l = delta_l' h_{l-1}
    dW_0 = (delta_0' obs[rows] - db_0 mean') / std        (the normalised observations are never formed)

The yardstick is the same operation in float32 through library products on the same inputs.  The criterion and its floors are the
ones the suite already holds these kernels to (tests/test_gpu_mlp.py, tests/test_gpu_ppo_loss.py, tests/ppo_batches.py), unchanged:

    delta chains, dW    max |got - f64| <= 3 max |f32 - f64| + 2e-6, both relative to max |f64|
    forward outputs     max |got - f64| <= 2 max |f32 - f64| + 2e-5 (absolute)
    pre-activations     max |got - f64| <  1e-4 max(1, max |z|)
    bias sums           max |got - f64| <= 3e-5 max_n sum_m |delta[m, n]|
"""
import torch

FLOOR = 2e-6                        # delta chains and dW
FORWARD_FLOOR = 2e-5                # forward outputs, absolute, next to 2 x err32
PRE_ACT_TOL = 1e-4                  # x max(1, |z|)
BIAS_TOL = 3e-5                     # x max sum |delta|


# ----------------------------------------------------------------------------------------------------------------- case tables
# forward: (K, M, normaliser, rows, value depth, policy depth, policy width, P).  Edges meet each other: K walks
# {1, 3, 4, 15, 16, 17, 30, 32, 112, 1262, 1264} four times while M, P, the depths, the width, `rows` and the normaliser turn at other
# periods, and the listed tail adds meetings by name (the smallest K with M = 1, K % 16 == 0 with `rows`, the widest case of both policy widths, ..).
FORWARD_K = (1, 3, 4, 15, 16, 17, 30, 32, 112, 1262, 1264)
FORWARD_M = (1, 31, 32, 33, 77)
FORWARD_P = (2, 60, 65, 128)


def _forward_cases():
    out, n = [], 0
    for rep in range(4):
        for K in FORWARD_K:
            M = FORWARD_M[(n + rep) % 5]
            P = FORWARD_P[(n + n // 4) % 4]
            vl, pl = (1, 7)[n % 2], (1, 7)[(n // 2 + rep) % 2]
            pw = 256 if rep == 3 else 32
            out.append((K, M, n % 3 != 0, (n // 2) % 2 == 1, vl, pl, pw, P))
            n += 1
    out += [(1, 1, True, True, 1, 1, 32, 2), (3, 1, False, False, 7, 7, 32, 65), (16, 33, True, True, 7, 1, 32, 128), (16, 1, False, True, 1, 7, 256, 60),
            (1264, 77, True, True, 7, 7, 256, 128), (1264, 31, False, True, 1, 1, 32, 65), (32, 32, True, False, 7, 7, 32, 60), (15, 33, True, True, 1, 7, 256, 2)]
    return tuple(out)


FORWARD_CASES = _forward_cases()
INTEGER_K = (16, 1264, 3)           # integer-data exactness of the first layer
ALONE_K = (3, 16, 17, 112, 1264)    # a row alone (M = 1) against the same row as row 37 of M = 77
ISOLATION_CASES = tuple((K, nan_at, inf_at) for K in (17, 112) for nan_at, inf_at in ((0, 31), (31, -1), (-1, 0)))     # M = 45: -1 = row 44 of a ragged tile
ISOLATION_M = 45

# the two-launch actor: (K, M, hidden layers, A, rows)
ACT_CASES = ((3, 1, 1, 1, False), (3, 9, 7, 64, True), (16, 33, 1, 30, True), (16, 77, 7, 33, False), (17, 9, 7, 1, False), (17, 1, 1, 64, True),
             (112, 77, 1, 33, False), (112, 33, 7, 30, True), (113, 9, 7, 64, False), (113, 33, 1, 1, True), (128, 1, 7, 33, True), (128, 77, 1, 30, False),
             (1264, 33, 1, 64, True), (1264, 9, 7, 30, False), (30, 33, 7, 30, True), (30, 1, 1, 33, False))

# delta chains
VALUE_BWD_CASES = tuple((nh, M) for nh in (1, 2, 7) for M in (1, 31, 33, 77))
POLICY_BWD_CASES = tuple((nh, P, extra, (1, 31, 33, 77)[(i + j + (extra > 0)) % 4]) for i, nh in enumerate((1, 7)) for j, P in enumerate((2, 60, 65, 128))
                         for extra in (0, 5))                                   # (hidden layers, P, rows behind M, M)
POLICY256_BWD_CASES = tuple((nh, M, (2, 60, 65, 128)[(i + j) % 4], 7 * (j % 2)) for i, nh in enumerate((1, 7)) for j, M in enumerate((1, 31, 33, 77)))    # (nh, n, P, rows behind n)

# weight gradients: (M, O, I, rows, normaliser)
DW_CASES = ((77, 32, 129, False, False), (256, 3, 129, True, True), (400, 32, 130, True, False), (131, 5, 131, False, True), (45, 60, 77, True, False),
            (400, 33, 65, True, True), (77, 64, 64, False, False), (256, 65, 129, False, True), (400, 128, 131, True, False), (100, 256, 256, False, False),
            (33, 2, 1, False, False), (77, 65, 2, True, True), (31, 33, 3, False, True), (400, 256, 1281, True, True), (1, 32, 32, False, False),
            (64, 1, 256, False, False), (256, 128, 129, False, False))
# `rr_mlp_weight_grad_batch` over the whole table in two calls (indices into DW_CASES).  The first mixes all three tile groups, and in the
# 128-wide one (256, 65, 129) / (256, 128, 129) (last tile column 1 wide) sit next to (100, 256, 256) (whole tiles).
DW_BATCHES = ((0, 5, 6, 7, 9, 2, 11, 4, 16), (1, 3, 8, 10, 12, 13, 14, 15))


def dw_tile(O):
    """(TO, TI) of the weight-gradient kernel's three instances (csrc/rr_api.hip `dw_plan`): chosen by O alone."""
    return (32, 128) if O <= 32 else ((64, 64) if O <= 64 else (128, 128))


def dw_overhang(O, I):
    """Width of the last tile column, 0 when I is a whole number of tiles."""
    return I % dw_tile(O)[1]


def dw_slices(lib, M, O, I):
    """The slice count of a single product, from the library: rr_mlp_weight_grad_workspace_bytes = align256(nslice O I 4), which pins
    nslice whenever one slice is at least the 256 bytes of the alignment (O I >= 64)."""
    assert O * I >= 64
    return int(lib.rr_mlp_weight_grad_workspace_bytes(M, O, I)) // (O * I * 4)


# FusedUpdate on non-default networks: (value depth, policy depth, RR_LEARNER_STREAMS or None)
FUSED_UPDATE_SHAPE = dict(T=3, B=24, R=40, K=112, A=30)
FUSED_UPDATE_CASES = ((1, 1, None), (7, 7, "0"), (7, 7, None))
ACTOR_DEPTHS = (1, 2, 3, 5)          # the in-kernel actor (tests/test_gpu_actor_depth.py); 4 is every other test's default
ACTOR_REFUSED_DEPTH = 6


# ----------------------------------------------------------------------------------------------------------------- networks, inputs
def make_networks(K, P, pl=4, vl=5, pw=32, seed=0, device="cpu"):
    """`networks.make_ppo_networks` at any depth / width, biases non-zero (the bias path is exercised).  An odd P (the kernels take any
    1 .. 128 logits; the tanh-normal head needs an even count) swaps the head for a fresh layer of that width, same initialisation."""
    from rodent_amd.training import networks
    torch.manual_seed(seed)
    n = networks.make_ppo_networks(K, (P + 1) // 2, policy_hidden_layer_sizes=(pw,) * pl, value_hidden_layer_sizes=(256,) * vl, device=device)
    if P % 2:
        n.policy_network.layers[-1] = networks.MLP(pw, [P]).layers[0].to(device)
    for net in (n.policy_network, n.value_network):
        for lin in net.layers:
            torch.nn.init.uniform_(lin.bias, -0.1, 0.1)
    return n


def params(net, dtype=None):
    """(weights, biases) of an MLP, detached, optionally cast."""
    return [l.weight.detach().to(dtype) if dtype else l.weight.detach() for l in net.layers], \
           [l.bias.detach().to(dtype) if dtype else l.bias.detach() for l in net.layers]


def make_inputs(K, M, norm, rows, seed, device="cpu"):
    """(obs [R, K], mean, std, rows): with `rows` the buffer holds more rows than M and the index list includes its last row."""
    g = torch.Generator().manual_seed(seed)
    R = M + 11 if rows else M
    obs = torch.randn(R, K, generator=g) * 2 + 0.5
    mean = std = idx = None
    if norm:
        mean, std = torch.randn(K, generator=g) * 0.3, torch.rand(K, generator=g) + 0.5
    if rows:
        idx = torch.randperm(R, generator=g)[:M]
        idx[M // 2] = R - 1
    mv = lambda t: None if t is None else t.to(device)
    return mv(obs), mv(mean), mv(std), mv(idx)


def chain_inputs(nh, M, P, H, seed):
    """(G [M, P], head weight [P, H], [None, W_1 .. W_{nh-1}], [z_0 .. z_{nh-1}]) of a delta-chain case, scaled as the chain tests of
    tests/test_gpu_ppo_loss.py scale theirs."""
    g = torch.Generator().manual_seed(seed)
    z = [torch.randn(M, H, generator=g) * 1.5 for _ in range(nh)]
    s = 16.0 if H == 256 else 5.0
    Ws = [None] + [torch.randn(H, H, generator=g) / s for _ in range(1, nh)]
    wh = torch.randn(P, H, generator=g) / s
    G = torch.randn(M, P, generator=g)
    return G, wh, Ws, z


def value_chain_inputs(nh, M):
    """Inputs of VALUE_BWD_CASES entry (nh, M): G [M, 1], head weight [1, 256], hidden weights, z [M, 256] per layer."""
    return chain_inputs(nh, M, 1, 256, seed=nh * 1000 + M + 1)


def policy_chain_inputs(nh, P, extra, M):
    """Inputs of a POLICY_BWD_CASES entry: G [M, P] (the first M rows), head weight [P, 32], hidden weights, z [M + extra, 32] per layer."""
    G, wh, Ws, z = chain_inputs(nh, M + extra, P, 32, seed=nh * 1000 + M + P)
    return G[:M].contiguous(), wh, Ws, z


def policy256_chain_inputs(nh, n, P, extra):
    """Inputs of a POLICY256_BWD_CASES entry: G [n, P], head weight [P, 256], hidden weights, z [n + extra, 256] per layer."""
    G, wh, Ws, z = chain_inputs(nh, n + extra, P, 256, seed=nh * 1000 + n + P + 7)
    return G[:n].contiguous(), wh, Ws, z


def dw_inputs(M, O, I, rows, norm, device="cpu"):
    """(delta [M, O], act [R, I], rows, mean, std) of a weight-gradient case, as tests/test_gpu_ppo_loss.test_weight_grad_kernel draws them."""
    g = torch.Generator().manual_seed(M + O + I)
    R = M + 37 if rows else M
    delta, act = torch.randn(M, O, generator=g), torch.randn(R, I, generator=g) * 2 + 0.3
    idx = torch.randperm(R, generator=g)[:M] if rows else None
    mean, std = (torch.randn(I, generator=g) * 0.3, torch.rand(I, generator=g) + 0.5) if norm else (None, None)
    mv = lambda t: None if t is None else t.to(device)
    return mv(delta), mv(act), mv(idx), mv(mean), mv(std)


# ----------------------------------------------------------------------------------------------------------------- the reference
def _mm(a, b, order):
    """a [m, k] @ b [k, n].  order 1: the same product with k walked backwards (a second float32 evaluation order)."""
    return a @ b if order == 0 else a.flip(1) @ b.flip(0)


def normalise(obs, mean, std, rows, dtype):
    x = (obs if rows is None else obs[rows]).to(dtype)
    return x if mean is None else (x - mean.to(dtype)) / std.to(dtype)


def silu_prime(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def forward(obs, mean, std, rows, ws, bs, dtype=torch.float64, order=0):
    """(out [M, P], [z_0 .. z_{L-1}]) of one network on the raw observations."""
    h, zs = normalise(obs, mean, std, rows, dtype), []
    for l, (w, b) in enumerate(zip(ws, bs)):
        z = _mm(h, w.to(dtype).t(), order) + b.to(dtype)
        if l == len(ws) - 1:
            return z, zs
        zs.append(z)
        h = torch.nn.functional.silu(z)


def delta_chain(G, w_head, Ws, zs, dtype=torch.float64, order=0):
    """([delta_0 .. delta_{nh-1}], [h_0 .. h_{nh-1}]) of a hidden stack: G [M, P] = d loss / d outputs, w_head [P, H], Ws[j] = W_j [H, H]
    for j >= 1 (entry 0 unused), zs the pre-activations."""
    nh = len(zs)
    zs = [z.to(dtype) for z in zs]
    d = [None] * nh
    d[nh - 1] = _mm(G.to(dtype), w_head.to(dtype), order) * silu_prime(zs[nh - 1])
    for j in range(nh - 1, 0, -1):
        d[j - 1] = _mm(d[j], Ws[j].to(dtype), order) * silu_prime(zs[j - 1])
    return d, [torch.nn.functional.silu(z) for z in zs]


def weight_grad(delta, act, rows=None, mean=None, std=None, dtype=torch.float64, order=0):
    """dW [O, I] = delta' x, x = act[rows]; with mean / std in the form (delta' act[rows] - colsum(delta) mean') / std."""
    a = (act if rows is None else act[rows]).to(dtype)
    dw = _mm(delta.to(dtype).t(), a, order)
    if mean is not None:
        dw = (dw - delta.to(dtype).sum(0)[:, None] * mean.to(dtype)[None, :]) / std.to(dtype)[None, :]
    return dw


def gradients(obs, mean, std, rows, ws, bs, G, dtype=torch.float64, order=0):
    """Everything of one network for the output gradient G [M, P]: dict(out, z, h, delta, dW, db), lists indexed by layer 0 .. L-1."""
    L = len(ws)
    out, zs = forward(obs, mean, std, rows, ws, bs, dtype, order)
    G = G.to(dtype).reshape(out.shape[0], -1)
    delta, h = delta_chain(G, ws[L - 1], [None] + list(ws[1:L - 1]), zs, dtype, order)
    delta = delta + [G]
    dW = [weight_grad(delta[0], obs, rows, mean, std, dtype, order)] + [weight_grad(delta[l], h[l - 1], dtype=dtype, order=order) for l in range(1, L)]
    return dict(out=out, z=zs, h=h, delta=delta, dW=dW, db=[d.sum(0) for d in delta])


# ----------------------------------------------------------------------------------------------------------------- the criterion
def _d(t):
    return t.detach().double().cpu()


def record(label, name, err, err32=None):
    """One line per measured figure (pytest -s shows them): every check prints before it asserts."""
    print(f"[edge] {label} | {name} | err {err:.3e} | f32 {'-' if err32 is None else format(err32, '.3e')}")


def check(label, name, got, f32, f64, floor=FLOOR):
    """max |got - f64| <= 3 max |f32 - f64| + floor, relative to max |f64|."""
    got, f32, f64 = _d(got), _d(f32), _d(f64)
    assert got.shape == f64.shape and torch.isfinite(got).all(), (label, name, tuple(got.shape), tuple(f64.shape))
    scale = float(f64.abs().max())
    assert scale > 0, (label, name)
    err, err32 = float((got - f64).abs().max()) / scale, float((f32 - f64).abs().max()) / scale
    record(label, name, err, err32)
    assert err <= 3 * err32 + floor, (label, name, err, err32)


def check_output(label, name, got, f32, f64):
    """Forward outputs: max |got - f64| <= 2 max |f32 - f64| + 2e-5, absolute."""
    got, f32, f64 = _d(got), _d(f32), _d(f64)
    assert got.shape == f64.shape and torch.isfinite(got).all(), (label, name, tuple(got.shape), tuple(f64.shape))
    err, err32 = float((got - f64).abs().max()), float((f32 - f64).abs().max())
    record(label, name, err, err32)
    assert err <= 2 * err32 + FORWARD_FLOOR, (label, name, err, err32)


def check_pre(label, name, got, f64):
    """Pre-activations: max |got - z| < 1e-4 max(1, max |z|)."""
    got, f64 = _d(got), _d(f64)
    assert got.shape == f64.shape and torch.isfinite(got).all(), (label, name, tuple(got.shape), tuple(f64.shape))
    err = float((got - f64).abs().max())
    record(label, name, err, None)
    assert err < PRE_ACT_TOL * max(1.0, float(f64.abs().max())), (label, name, err)


def check_bias(label, name, got, delta64):
    """Bias sums: max |got - sum_m delta| <= 3e-5 max_n sum_m |delta[m, n]|."""
    got, delta64 = _d(got).reshape(-1), _d(delta64)
    err = float((got - delta64.sum(0)).abs().max())
    record(label, name, err, None)
    assert torch.isfinite(got).all() and err <= BIAS_TOL * float(delta64.abs().sum(0).max()), (label, name, err)
