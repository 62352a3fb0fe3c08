"""Time the kernels that carry the tanh-normal head outside the step kernel, at the launcher's shapes: `rr_ppo_loss` on a minibatch
(unroll 10 x 2048 sequences) and the two-launch actor `rr_policy_act` on 2048 observation rows, each at 30 actions (64 head columns,
`rr_policy_tail_kernel<64>`) and 38 actions (128 columns, `<128>`).  RR_LIB selects the library build.  Prints one JSON line (ms per call,
HIP-event time over 50 calls after 5)."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "brax-rodent-run_amd"))
import torch
from rodent_amd import hip
from rodent_amd.training import fused_mlp, networks
from tests.ppo_batches import CFG, _batch

dev = "cuda:0"
K, T, B, N = 1263, 10, 2048, 2048


def timeit(fn, reps=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


out = {"lib": os.path.basename(hip.LIB_PATH)}
torch.manual_seed(0)
obs = torch.randn(N, K, device=dev)
mean, std = torch.randn(K, device=dev) * 0.1, torch.rand(K, device=dev) + 0.5
with torch.no_grad():
    for A in (30, 38):
        data, logits, values, noise, idx = _batch(T, B, B, A, seed=A)
        data = {k: v.to(dev).contiguous() for k, v in data.items()}
        logits, values, noise, idx, bufs = logits.to(dev), values.to(dev), noise.to(dev), idx.to(dev), {}
        out[f"ppo_loss_A{A}_ms"] = timeit(lambda: hip.ppo_loss(logits, values, data, idx, noise, T, out=bufs, **CFG))
        pp = fused_mlp.net_params(networks.make_ppo_networks(K, A, device=dev).policy_network)
        eps = torch.randn(N, A, device=dev)
        out[f"policy_act_A{A}_ms"] = timeit(lambda: hip.policy_act(obs, mean, std, pp, eps, 0.001))
print(json.dumps(out))
