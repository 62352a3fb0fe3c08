"""What the learner costs for a policy head of more than 64 logits: rodent_cpu.xml (38 actuators, 76 logits) at its observation width,
default networks (policy 32 x 4 -> 76, value 256 x 5 -> 1), the launcher's minibatch (unroll 10, 2048 sequences = 22528 rows), ONE
process, two update paths alternating on the same data and the same parameters:

    fused      `FusedUpdate` (rr_mlp_forward, rr_ppo_loss, rr_policy_backward, rr_mlp_value_backward, rr_mlp_weight_grad_batch): what
               RR_FUSED_WIDE_HEAD=1 selects for this head in ppo.train
    autograd   normalise, nn.Linear forward of both networks, `compute_ppo_loss`, `loss.backward()`: what it runs otherwise

Both leave d total_loss / d parameter in the flat gradient buffer; the optimiser step (the same for both) is not timed.  HIP-event time per
minibatch update, `--updates` updates per window.

With --train it also runs `ppo.train` on rodent_cpu.xml at --envs environments with the launcher's hyper-parameters, switch on and
off, and reports `rollout_s` / `learner_s` of the last of --train-steps training steps (the earlier ones warm up and capture the
update's graph).

usage: python tools/bench_wide_head_learner.py [--train] [--out FILE.json]
One JSON line.  Needs a GPU (no fallback); profiler off."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "brax-rodent-run_amd"))

MODEL = "rodent_cpu.xml"
CFG = dict(entropy_cost=1e-3, discounting=0.97, reward_scaling=1.0, gae_lambda=0.95, clipping_epsilon=0.3)


def track():
    import numpy as np
    t = np.arange(250, dtype=np.float64)
    return np.stack([0.004 * t, np.zeros(250), np.full(250, 0.0681)], axis=1)


def train_line(envs_n, steps, dev):
    """rollout_s / learner_s of the last training step of a fresh ppo.train, switch on and off."""
    import torch
    from rodent_amd import envs
    from rodent_amd.training.agents.ppo import train as ppo
    out = {}
    for name, flag in (("wide_head_on", "1"), ("wide_head_off", "0")):
        os.environ["RR_FUSED_WIDE_HEAD"] = flag
        env = envs.get_environment("rodent", track_pos=track(), num_envs=envs_n, xml_path=MODEL, terminate_when_unhealthy=True, solver="cg",
                                   iterations=8, ls_iterations=8, device=dev)
        times = []
        ppo.train(environment=env, num_timesteps=500_000_000, num_evals=100, reward_scaling=1, episode_length=150, normalize_observations=True,
                  action_repeat=1, unroll_length=10, num_minibatches=64, num_updates_per_batch=8, discounting=0.97, learning_rate=5e-5,
                  entropy_cost=1e-3, num_envs=envs_n, batch_size=envs_n, seed=0, num_eval_envs=0, max_training_steps=steps, timing_fn=times.append)
        torch.cuda.synchronize(dev)
        out[name] = dict(rollout_s=times[-1]["rollout_s"], learner_s=times[-1]["learner_s"], env_steps=times[-1]["env_steps"],
                         all_steps=[dict(rollout_s=t["rollout_s"], learner_s=t["learner_s"]) for t in times])
        del env
    os.environ.pop("RR_FUSED_WIDE_HEAD", None)
    out["learner_ratio_off_over_on"] = out["wide_head_off"]["learner_s"] / out["wide_head_on"]["learner_s"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--unroll", type=int, default=10)
    ap.add_argument("--sequences", type=int, default=2048, help="trajectories per minibatch")
    ap.add_argument("--pool", type=int, default=4096, help="trajectories in the buffer the minibatch is drawn from")
    ap.add_argument("--updates", type=int, default=20, help="minibatch updates per path and window")
    ap.add_argument("--warmup", type=int, default=2, help="untimed windows")
    ap.add_argument("--repeats", type=int, default=5, help="timed windows")
    ap.add_argument("--train", action="store_true", help="also one ppo.train line, switch on and off")
    ap.add_argument("--envs", type=int, default=2048, help="--train: environments")
    ap.add_argument("--train-steps", type=int, default=2, help="--train: training steps per run (the last one is reported)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from rodent_amd import envs
    from rodent_amd.training import distributed as D, networks
    from rodent_amd.training.agents.ppo import fused_update, losses
    if not torch.cuda.is_available():
        raise SystemExit("bench_wide_head_learner: needs a GPU")
    dev = torch.device("cuda:0")
    env = envs.get_environment("rodent", track_pos=track(), num_envs=8, xml_path=MODEL, iterations=8, ls_iterations=8, device=dev)
    K, A = env.observation_size, env.action_size
    del env
    T, B, R = a.unroll, a.sequences, a.pool
    torch.manual_seed(0)
    nets = networks.make_ppo_networks(K, A, device=dev)
    pnet, vnet, dist = nets.policy_network, nets.value_network, nets.parametric_action_distribution
    params = list(pnet.parameters()) + list(vnet.parameters())
    flat = D.FlatGrads(params)
    g = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    data = dict(obs=rnd(R, T + 1, K) * 2 + 0.5, raw_action=rnd(R, T, A) * 0.8, log_prob=rnd(R, T) * 2 - 30, reward=torch.rand(R, T, device=dev, generator=g),
                truncation=(torch.rand(R, T, device=dev, generator=g) < 0.05).float(), discount=1 - (torch.rand(R, T, device=dev, generator=g) < 0.1).float())
    mean, std = rnd(K) * 0.3, torch.rand(K, device=dev, generator=g) + 0.5
    fu = fused_update.FusedUpdate(pnet, vnet, dist, T, normalize_advantage=True, **CFG)
    gen = torch.Generator(device=dev).manual_seed(2)

    def fused(idx):
        return fu(data, idx, mean, std, gen)

    def autograd(idx):
        mbd = {k: data[k][idx].transpose(0, 1) for k in ("raw_action", "log_prob", "reward", "discount", "truncation")}
        x = (data["obs"][idx].transpose(0, 1) - mean) / std
        values = vnet(x).squeeze(-1)
        loss, m = losses.compute_ppo_loss(pnet(x[:T]), values[:T], values[T], mbd, dist, normalize_advantage=True, generator=gen, **CFG)
        flat.zero_()
        loss.backward()
        return m

    paths = {"fused": fused, "autograd": autograd}
    ms = {k: [] for k in paths}
    perm_gen = torch.Generator(device=dev).manual_seed(3)

    def window(record):
        idxs = [torch.randperm(R, device=dev, generator=perm_gen)[:B] for _ in range(a.updates)]
        for name, fn in paths.items():                 # alternating: both paths see the same minibatches in every window
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            e0.record()
            for idx in idxs:
                fn(idx)
            e1.record()
            torch.cuda.synchronize(dev)
            if record:
                ms[name].append(e0.elapsed_time(e1) / a.updates)

    for _ in range(a.warmup):
        window(False)
    for _ in range(a.repeats):
        window(True)
    # one more update each on the same minibatch and noise: the two gradients, compared per tensor
    idx = torch.randperm(R, device=dev, generator=perm_gen)[:B]
    grads = {}
    for name, fn in paths.items():
        gen.manual_seed(4)
        fn(idx)
        grads[name] = flat.flat.clone()
    worst, o = 0.0, 0
    for p in params:
        x, y = grads["fused"][o:o + p.numel()], grads["autograd"][o:o + p.numel()]
        o += p.numel()
        worst = max(worst, float((x - y).abs().max() / y.abs().max().clamp_min(1e-30)))
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = dict(model=MODEL, observation_size=K, action_size=A, policy_logits=2 * A, unroll=T, sequences=B, rows=(T + 1) * B, updates_per_window=a.updates,
               warmup_windows=a.warmup, timed_windows=a.repeats, ms_per_minibatch_update=ms, median_ms=med,
               range_frac_of_median={k: (max(v) - min(v)) / med[k] for k, v in ms.items()}, ratio_autograd_over_fused=med["autograd"] / med["fused"],
               per_window_ratio=[y / x for x, y in zip(ms["fused"], ms["autograd"])], max_gradient_gap_rel_to_tensor_max=worst,
               device=torch.cuda.get_device_name(0))
    if a.train:
        out["ppo_train"] = dict(envs=a.envs, training_steps=a.train_steps, **train_line(a.envs, a.train_steps, dev))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
