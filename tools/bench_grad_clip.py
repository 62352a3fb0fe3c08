"""What `ppo.train(max_grad_norm=...)` costs in the learner: bench.py --config 3's hyper-parameters (rodent_optimized.xml, 2048 envs, unroll 10,
64 minibatches x 8 epochs, CG 8/8), `timing_fn` splitting rollout_s / learner_s.

Two arms, alternating, each run in a fresh child process (one warm-up training step, then --steps timed ones):

    off   max_grad_norm=None: torch.optim.Adam(fused, capturable) inside the captured update
    on    max_grad_norm=--max-grad-norm (default inf: norm, statistics and the non-finite check, never a scaled gradient; the three launches
          of rr_clipped_adam_step do the same work whether or not they scale) inside the captured update

Reports per arm the median and range over the pairs of the per-child median learner_s / rollout_s, the learner time per minibatch update
(512 per training step), the difference of the medians, and whether that difference lies inside the off arm's own repeat-to-repeat range
(max - min over its children).  No gate: the option is off by default.

usage: python tools/bench_grad_clip.py [--pairs 5] [--steps 2] [--max-grad-norm inf] [--out FILE.json]
One JSON line.  Needs a GPU (no fallback); profiler off.  A child that fails or overruns its time limit ends the run: nothing more is started."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UPDATES_PER_STEP = 64 * 8


def child(steps, envs_n, max_grad_norm):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "brax-rodent-run_amd"))
    import numpy as np
    import torch
    from rodent_amd import envs
    from rodent_amd.training.agents.ppo import train as ppo
    t = np.arange(250, dtype=np.float64)
    track = np.stack([0.004 * t, np.zeros(250), np.full(250, 0.0681)], axis=1)
    env = envs.get_environment("rodent", track_pos=track, num_envs=envs_n, xml_path="rodent_optimized.xml", terminate_when_unhealthy=True,
                               solver="cg", iterations=8, ls_iterations=8, device="cuda:0")
    times, seen = [], {}
    ppo.train(environment=env, num_timesteps=500_000_000, num_evals=100, reward_scaling=1, episode_length=150, normalize_observations=True,
              action_repeat=1, unroll_length=10, num_minibatches=64, num_updates_per_batch=8, discounting=0.97, learning_rate=5e-5,
              entropy_cost=1e-3, num_envs=envs_n, batch_size=envs_n, seed=0, num_eval_envs=0, max_training_steps=1 + steps,
              max_grad_norm=max_grad_norm, timing_fn=times.append, progress_fn=lambda n, m: seen.update(m))
    torch.cuda.synchronize()
    timed = times[1:]
    print(json.dumps(dict(rollout_s=statistics.median(x["rollout_s"] for x in timed), learner_s=statistics.median(x["learner_s"] for x in timed),
                          all_steps=[dict(rollout_s=x["rollout_s"], learner_s=x["learner_s"]) for x in times],
                          last_step_metrics={k: v for k, v in seen.items() if k.startswith("training/grad_") or k == "training/skipped_updates"})),
          flush=True)


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
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--max-grad-norm", type=float, default=float("inf"))
    ap.add_argument("--child-timeout", type=int, default=150)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=("off", "on"))
    args = ap.parse_args()
    if args.child:
        return child(args.steps, args.envs, args.max_grad_norm if args.child == "on" else None)
    runs = {"off": [], "on": []}
    for pair in range(args.pairs):
        for arm in (("off", "on") if pair % 2 == 0 else ("on", "off")):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", arm, "--steps", str(args.steps), "--envs", str(args.envs),
                   "--max-grad-norm", repr(args.max_grad_norm)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.child_timeout)
            if r.returncode:
                sys.exit(f"arm {arm}, pair {pair}: child exited with status {r.returncode}; stopping")
            runs[arm].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(f"pair {pair} arm {arm}: rollout_s {runs[arm][-1]['rollout_s']:.3f} learner_s {runs[arm][-1]['learner_s']:.3f}", file=sys.stderr, flush=True)
    out = dict(workload=f"ppo.train, bench.py --config 3 hyper-parameters, {args.envs} envs, {args.pairs} alternating pairs of fresh processes, "
                        f"1 warm-up + {args.steps} timed training steps each",
               arm_off="max_grad_norm=None: torch.optim.Adam(fused, capturable)", arm_on=f"max_grad_norm={args.max_grad_norm}: rr_clipped_adam_step",
               off=summary(runs["off"]), on=summary(runs["on"]))
    d = out["on"]["learner_s"]["median"] - out["off"]["learner_s"]["median"]
    out["learner_s_on_minus_off"] = d
    out["learner_us_per_minibatch_on_minus_off"] = 1e6 * d / UPDATES_PER_STEP
    out["off_arm_range_s"] = out["off"]["learner_s"]["max"] - out["off"]["learner_s"]["min"]
    out["difference_inside_off_arm_range"] = abs(d) <= out["off_arm_range_s"]
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
