"""CPU: what tests/test_gpu_mlp_edges.py and tests/test_gpu_actor_depth.py stand on (tests/mlp_shapes.py) -- the float64 reference
equals torch.autograd, the float32 library path itself meets the criterion at every shape of the tables, and the tables hold every
class of shape the kernels treat differently."""
import copy

import pytest
import torch

from tests import mlp_shapes as S


def _stack64(net):
    return copy.deepcopy(net).double()


@pytest.mark.parametrize("depth", [7, 1])
@pytest.mark.parametrize("norm", [True, False])
def test_reference_gradients_equal_autograd(depth, norm):
    """`mlp_shapes.gradients` (delta chain, dW, db, the first layer in its normaliser form, `rows`) against torch.autograd in float64 on
    the nn.Linear / SiLU stack: 1e-12 relative, deepest and shallowest network of the tables, both networks."""
    K, M, P = 30, 33, 65
    nets = S.make_networks(K, P, pl=depth, vl=depth, seed=depth)
    obs, mean, std, rows = S.make_inputs(K, M, norm, True, seed=3)
    g = torch.Generator().manual_seed(5)
    for net, G in ((nets.policy_network, torch.randn(M, P, generator=g).double()), (nets.value_network, torch.randn(M, generator=g).double())):
        ws, bs = S.params(net)
        ref = S.gradients(obs, mean, std, rows, ws, bs, G)
        net64 = _stack64(net)
        x = obs[rows].double()
        if norm:
            x = (x - mean.double()) / std.double()
        out = net64(x)
        (out * G.reshape(out.shape)).sum().backward()
        assert (ref["out"] - out.detach()).abs().max() <= 1e-12 * out.detach().abs().max()
        for l, lin in enumerate(net64.layers):
            for got, want in ((ref["dW"][l], lin.weight.grad), (ref["db"][l], lin.bias.grad)):
                assert got.shape == want.shape
                assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), (depth, norm, l)


def _both(fn):
    """(float64, float32 library path, float32 in a second evaluation order) of one reference call."""
    return fn(torch.float64, 0), fn(torch.float32, 0), fn(torch.float32, 1)


@pytest.mark.parametrize("case", S.FORWARD_CASES, ids=lambda c: "-".join(str(int(x)) for x in c))
def test_float32_forward_meets_the_criterion(case):
    K, M, norm, rows, vl, pl, pw, P = case
    nets = S.make_networks(K, P, pl, vl, pw, seed=K + M)
    obs, mean, std, idx = S.make_inputs(K, M, norm, rows, seed=K * 7 + M)
    for name, net in (("policy", nets.policy_network), ("value", nets.value_network)):
        ws, bs = S.params(net)
        (o64, z64), (o32, z32), (o32b, _) = _both(lambda dt, order: S.forward(obs, mean, std, idx, ws, bs, dt, order))
        S.check_output(str(case), name, o32, o32b, o64)
        for l in range(len(z64)):
            S.check_pre(str(case), f"{name} z{l}", z32[l], z64[l])


def test_float32_delta_chains_meet_the_criterion():
    """On the inputs the GPU tests draw (the same helper calls), the rows the kernels use."""
    cases = [(f"value nh={nh} M={M}", M, S.value_chain_inputs(nh, M)) for nh, M in S.VALUE_BWD_CASES] + \
            [(f"policy nh={c[0]} P={c[1]} M={c[3]}+{c[2]}", c[3], S.policy_chain_inputs(*c)) for c in S.POLICY_BWD_CASES] + \
            [(f"policy256 nh={c[0]} P={c[2]} n={c[1]}+{c[3]}", c[1], S.policy256_chain_inputs(*c)) for c in S.POLICY256_BWD_CASES]
    for label, M, (G, wh, Ws, z) in cases:
        nh, z = len(z), [t[:M] for t in z]
        (d64, h64), (d32, h32), (d32b, _) = _both(lambda dt, order: S.delta_chain(G, wh, Ws, z, dt, order))
        label = "chain " + label
        for j in range(nh):
            S.check(label, f"delta{j}", d32[j], d32b[j], d64[j])
            S.check_bias(label, f"db{j}", d32[j].sum(0), d64[j])
            assert float((h32[j].double() - h64[j]).abs().max()) <= 2e-6 * float(h64[j].abs().max())


def test_float32_weight_gradients_meet_the_criterion():
    for M, O, I, rows, norm in S.DW_CASES:
        delta, act, idx, mean, std = S.dw_inputs(M, O, I, rows, norm)
        w64, w32, w32b = _both(lambda dt, order: S.weight_grad(delta, act, idx, mean, std, dt, order))
        S.check(f"dW M={M} O={O} I={I}", "dW", w32, w32b, w64)


def test_float32_actor_logits_and_network_gradients_meet_the_criterion():
    """The remaining tables: the two-launch actor's cases (logits) and the learner's two networks at the FusedUpdate shape (every dW, db)."""
    for K, M, nh, A, rows in S.ACT_CASES:
        nets = S.make_networks(K, 2 * A, nh, 1, 32, seed=K + M + A)
        obs, mean, std, idx = S.make_inputs(K, M, True, rows, seed=K + A)
        ws, bs = S.params(nets.policy_network)
        (o64, _), (o32, _), (o32b, _) = _both(lambda dt, order: S.forward(obs, mean, std, idx, ws, bs, dt, order))
        S.check(f"act {K}-{M}-{nh}-{A}", "logits", o32, o32b, o64)
    T, B, K, A = (S.FUSED_UPDATE_SHAPE[k] for k in "TBKA")
    M = (T + 1) * B
    for depth in (1, 7):
        nets = S.make_networks(K, 2 * A, depth, depth, 32, seed=depth)
        obs, mean, std, _ = S.make_inputs(K, M, True, False, seed=depth)
        g = torch.Generator().manual_seed(5)
        for name, net, G in (("policy", nets.policy_network, torch.randn(M, 2 * A, generator=g)), ("value", nets.value_network, torch.randn(M, generator=g))):
            ws, bs = S.params(net)
            r64, r32, r32b = _both(lambda dt, order: S.gradients(obs, mean, std, None, ws, bs, G, dt, order))
            for l in range(len(ws)):
                S.check(f"gradients depth={depth} {name}", f"dW{l}", r32["dW"][l], r32b["dW"][l], r64["dW"][l])
                S.check_bias(f"gradients depth={depth} {name}", f"db{l}", r32["db"][l], r64["delta"][l])


def test_tables_cover_the_observation_widths():
    for name, Ks in (("forward", [c[0] for c in S.FORWARD_CASES]), ("actor", [c[0] for c in S.ACT_CASES])):
        assert {K % 4 for K in Ks} == {0, 1, 2, 3}, name
        assert any(K % 16 == 0 and K > 16 for K in Ks) and any(K < 16 for K in Ks) and 16 in Ks and any(17 <= K <= 31 for K in Ks), name
        assert any((K + 15) // 16 < 8 for K in Ks) and any((K + 15) // 16 > 8 for K in Ks), name
    # the actor cuts the chunks into at most 8 k-slices: one chunk, fewer than 8 one-chunk slices, exactly 8, and slices of several chunks
    assert {1, 7, 8} <= {(c[0] + 15) // 16 for c in S.ACT_CASES} and any((c[0] + 15) // 16 > 8 for c in S.ACT_CASES)
    assert set(S.FORWARD_K) <= {c[0] for c in S.FORWARD_CASES} and {3, 16, 17, 112, 113, 128, 1264} <= {c[0] for c in S.ACT_CASES}
    assert all(c[0] <= 1300 and c[1] <= 400 for c in S.FORWARD_CASES + S.ACT_CASES) and 40 <= len(S.FORWARD_CASES) <= 60
    # edges meet: the smallest K with M = 1, no partial chunk with `rows`, every M with and without rows / normaliser
    fc = S.FORWARD_CASES
    assert any(K == 1 and M == 1 for K, M, *_ in fc) and any(K % 16 == 0 and rows for K, _, _, rows, *_ in fc)
    for M in S.FORWARD_M:
        assert {(c[2], c[3]) for c in fc if c[1] == M} >= {(True, True), (False, False)}, M
    for K in S.FORWARD_K:                                            # no K sits at one M, one depth or one width only
        mine = [c for c in fc if c[0] == K]
        assert len({c[1] for c in mine}) >= 3 and {c[6] for c in mine} == {32, 256} and {c[4] for c in mine} == {1, 7} and {c[5] for c in mine} == {1, 7}, K
    assert {c[7] for c in fc} == set(S.FORWARD_P) and {c[7] for c in fc if c[6] == 256} == set(S.FORWARD_P)
    assert {A for _, _, _, A, _ in S.ACT_CASES} == {1, 30, 33, 64} and {nh for _, _, nh, _, _ in S.ACT_CASES} == {1, 7}
    assert {r for *_, r in S.ACT_CASES} == {True, False}


def test_tables_cover_the_row_counts():
    for name, Ms in (("forward", [c[1] for c in S.FORWARD_CASES]), ("value chain", [M for _, M in S.VALUE_BWD_CASES]),
                     ("policy chain", [c[3] for c in S.POLICY_BWD_CASES]), ("policy256 chain", [c[1] for c in S.POLICY256_BWD_CASES])):
        assert {1, 31, 33} <= set(Ms) and (32 in Ms or "chain" in name), name      # the chains: on both sides of the 32-row tile
        assert any(M >= 65 and M % 8 for M in Ms), name
    assert {e for _, _, e, _ in S.POLICY_BWD_CASES} == {0, 5} and {e > 0 for *_, e in S.POLICY256_BWD_CASES} == {True, False}


def test_tables_cover_the_depths():
    assert {c[4] for c in S.FORWARD_CASES} == {1, 7} and {c[5] for c in S.FORWARD_CASES if c[6] == 32} == {1, 7}
    assert {c[5] for c in S.FORWARD_CASES if c[6] == 256} == {1, 7}
    assert {nh for nh, _ in S.VALUE_BWD_CASES} == {1, 2, 7} and {c[0] for c in S.POLICY_BWD_CASES} == {1, 7} and {c[0] for c in S.POLICY256_BWD_CASES} == {1, 7}
    assert {c[1] for c in S.POLICY_BWD_CASES} == {2, 60, 65, 128}
    assert {(v, p) for v, p, _ in S.FUSED_UPDATE_CASES} == {(1, 1), (7, 7)} and {s for v, p, s in S.FUSED_UPDATE_CASES if v == 7} == {"0", None}
    assert set(S.ACTOR_DEPTHS) == {1, 2, 3, 5} and S.ACTOR_REFUSED_DEPTH == 6
    # 7 + 7 hidden layers: 16 weight-gradient products, more than one batched call takes
    from rodent_amd import hip
    assert 2 * (7 + 1) > hip.DW_MAX_ITEMS


def test_tables_cover_the_weight_gradient_paths():
    from rodent_amd import hip
    lib = hip.lib()
    over = {S.dw_overhang(O, I) for _, O, I, _, _ in S.DW_CASES if I >= 4}
    assert {1, 2, 3} <= over and any(w >= 4 for w in over)
    for tile in ((32, 128), (64, 64), (128, 128)):                   # an overhang of 1 in each of the three instances
        assert any(S.dw_tile(O) == tile and I > tile[1] and S.dw_overhang(O, I) == 1 for _, O, I, _, _ in S.DW_CASES), tile
    assert any(O % S.dw_tile(O)[0] == 0 and I % S.dw_tile(O)[1] == 0 and O % 4 == 0 for _, O, I, _, _ in S.DW_CASES)     # whole tiles only
    assert {I for _, _, I, _, _ in S.DW_CASES if I < 4} == {1, 2, 3}
    assert {2, 3, 5, 33, 65} <= {O for _, O, _, _, _ in S.DW_CASES}
    assert any((O * I) & 3 for _, O, I, _, _ in S.DW_CASES) and any((O * I) & 3 == 0 for _, O, I, _, _ in S.DW_CASES)
    assert {(r, n) for *_, r, n in S.DW_CASES} == {(False, False), (True, True), (True, False), (False, True)}
    assert all(M <= 400 and I <= 1300 for M, _, I, _, _ in S.DW_CASES)
    # rr_mlp_dw_reduce_kernel has two branches.  The aligned one ((O I) & 3 == 0) splits the slices into an 8-unrolled loop plus a remainder:
    # 1 and 2 .. 7 slices (remainder alone), exactly 8 (one unrolled pass, empty remainder), 9 or more (both) must all be aligned cases.
    # The unaligned one is a plain loop: one slice and more than one.
    aligned = {S.dw_slices(lib, M, O, I) for M, O, I, _, _ in S.DW_CASES if O * I >= 64 and (O * I) & 3 == 0}
    unaligned = {S.dw_slices(lib, M, O, I) for M, O, I, _, _ in S.DW_CASES if O * I >= 64 and (O * I) & 3}
    print("slice counts of the table: aligned", sorted(aligned), "unaligned", sorted(unaligned))
    assert 1 in aligned and any(2 <= s <= 7 for s in aligned) and 8 in aligned and any(s >= 9 for s in aligned)
    assert 1 in unaligned and any(s > 1 for s in unaligned)
    # the batches: the whole table in calls of at most DW_MAX_ITEMS products; the first holds all three tile groups, and an overhang of 1
    # next to a whole-tile product in one group
    assert sorted(i for b in S.DW_BATCHES for i in b) == list(range(len(S.DW_CASES))) and all(len(b) <= hip.DW_MAX_ITEMS for b in S.DW_BATCHES)
    batch = [S.DW_CASES[i] for i in S.DW_BATCHES[0]]
    assert {S.dw_tile(O) for _, O, _, _, _ in batch} == {(32, 128), (64, 64), (128, 128)}
    assert any(S.dw_tile(O) == S.dw_tile(O2) and S.dw_overhang(O, I) == 1 and I > S.dw_tile(O)[1] and O2 % S.dw_tile(O2)[0] == 0 and I2 % S.dw_tile(O2)[1] == 0
               for _, O, I, _, _ in batch for _, O2, I2, _, _ in batch)
