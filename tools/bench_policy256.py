"""What a policy with 256-wide hidden layers costs in `ppo.train`: bench.py --config 3's hyper-parameters (rodent_optimized.xml, 2048 envs,
unroll 10, 64 minibatches x 8 epochs, CG 8/8) with policy_hidden_layer_sizes = (256,) * 4, `timing_fn` splitting rollout_s / learner_s.

Two arms, alternating, each run in a fresh child process (one warm-up training step, then --steps timed ones):

    A   what the shape got before the kernels took it: autograd learner (nn.Linear forward, compute_ppo_loss, loss.backward()) and the
        nn.Linear actor -- RR_FUSED_MLP=0
    B   this build's path: rr_mlp_forward (policy: rr_mlp_policy256_forward_kernel), rr_ppo_loss, rr_mlp_policy_backward,
        rr_mlp_value_backward, rr_mlp_weight_grad_batch in the learner; rr_mlp_forward + rr_policy_sample per actor step -- RR_FUSED_POLICY256=1

Reports per arm the median and range over the pairs of the per-child median rollout_s / learner_s, and the learner time per minibatch
update (512 per training step).  The rule the default follows: arm B is the default for this shape only if its MEDIAN
learner_s is below arm A's MINIMUM.

usage: python tools/bench_policy256.py [--pairs 5] [--steps 2] [--out FILE.json]
One JSON line.  Needs a GPU (no fallback); profiler off.  A child that fails or overruns its time limit ends the run: nothing more is started."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = {"A": {"RR_FUSED_MLP": "0"}, "B": {"RR_FUSED_MLP": "1", "RR_FUSED_POLICY256": "1"}}
UPDATES_PER_STEP = 64 * 8


def child(steps, depth, envs_n):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "brax-rodent-run_amd"))
    import numpy as np
    import torch
    from rodent_amd import envs
    from rodent_amd.training import networks
    from rodent_amd.training.agents.ppo import train as ppo
    t = np.arange(250, dtype=np.float64)
    track = np.stack([0.004 * t, np.zeros(250), np.full(250, 0.0681)], axis=1)
    env = envs.get_environment("rodent", track_pos=track, num_envs=envs_n, xml_path="rodent_optimized.xml", terminate_when_unhealthy=True,
                               solver="cg", iterations=8, ls_iterations=8, device="cuda:0")
    times = []
    factory = lambda o, a, **kw: networks.make_ppo_networks(o, a, policy_hidden_layer_sizes=(256,) * depth, **kw)
    ppo.train(environment=env, num_timesteps=500_000_000, num_evals=100, reward_scaling=1, episode_length=150, normalize_observations=True,
              action_repeat=1, unroll_length=10, num_minibatches=64, num_updates_per_batch=8, discounting=0.97, learning_rate=5e-5,
              entropy_cost=1e-3, num_envs=envs_n, batch_size=envs_n, seed=0, num_eval_envs=0, max_training_steps=1 + steps,
              network_factory=factory, timing_fn=times.append)
    torch.cuda.synchronize()
    timed = times[1:]
    print(json.dumps(dict(rollout_s=statistics.median(x["rollout_s"] for x in timed), learner_s=statistics.median(x["learner_s"] for x in timed),
                          all_steps=[dict(rollout_s=x["rollout_s"], learner_s=x["learner_s"]) for x in times])), flush=True)


def summary(runs):
    out = {}
    for key in ("rollout_s", "learner_s"):
        v = [r[key] for r in runs]
        out[key] = dict(median=statistics.median(v), min=min(v), max=max(v))
    out["learner_ms_per_minibatch"] = 1e3 * out["learner_s"]["median"] / UPDATES_PER_STEP
    out["runs"] = runs
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2, help="timed training steps per child, after one warm-up step")
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--child-timeout", type=int, default=150)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=tuple(ARMS))
    args = ap.parse_args()
    if args.child:
        return child(args.steps, args.depth, args.envs)
    runs = {a: [] for a in ARMS}
    for pair in range(args.pairs):
        for arm in (("A", "B") if pair % 2 == 0 else ("B", "A")):
            env = dict(os.environ, **ARMS[arm])
            cmd = [sys.executable, os.path.abspath(__file__), "--child", arm, "--steps", str(args.steps), "--depth", str(args.depth), "--envs", str(args.envs)]
            r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=args.child_timeout)
            if r.returncode:
                sys.exit(f"arm {arm}, pair {pair}: child exited with status {r.returncode}; stopping")
            runs[arm].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(f"pair {pair} arm {arm}: rollout_s {runs[arm][-1]['rollout_s']:.3f} learner_s {runs[arm][-1]['learner_s']:.3f}", file=sys.stderr, flush=True)
    out = dict(workload=f"ppo.train, bench.py --config 3 hyper-parameters, policy 256 x {args.depth}, {args.envs} envs, {args.pairs} alternating pairs of "
                        f"fresh processes, 1 warm-up + {args.steps} timed training steps each",
               arm_A="RR_FUSED_MLP=0: autograd learner, nn.Linear actor", arm_B="RR_FUSED_POLICY256=1: hand-written learner and two-launch actor step",
               A=summary(runs["A"]), B=summary(runs["B"]))
    out["B_median_learner_below_A_min"] = out["B"]["learner_s"]["median"] < out["A"]["learner_s"]["min"]
    out["learner_ratio_A_over_B"] = out["A"]["learner_s"]["median"] / out["B"]["learner_s"]["median"]
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
