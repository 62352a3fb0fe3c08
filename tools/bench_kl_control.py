"""What the learner's KL options cost: bench.py --config 3's hyper-parameters (rodent_optimized.xml, 2048 envs, unroll 10, 64 minibatches x 8
epochs, CG 8/8), `timing_fn` splitting rollout_s / learner_s.

Four arms, every one on `training.optim.ClippedAdam(max_grad_norm=inf)` so that the optimiser is the same and only the option differs; the
arms rotate within each round, each run in a fresh child process (one warm-up training step, then --steps timed ones):

    base       max_grad_norm=inf alone
    diag       + learner_diagnostics=True: the DIAG instances of the loss and metrics kernels
    target     + target_kl=1e9, which never fires: DIAG, the KL instance of the step's finalisation, and the 8-byte flag read after each pass
    adaptive   + learning_rate_schedule="adaptive_kl" with its defaults: DIAG, the KL instance, the learning rate moving

Reports per arm the median and range over the rounds of the per-child median learner_s / rollout_s, the ratio of each option's median
learner_s to the base arm's, the difference per minibatch update (512 per training step), and whether the difference lies inside the base
arm's own repeat-to-repeat range (max - min over its children).  No gate: the options are off by default.

usage: python tools/bench_kl_control.py [--rounds 3] [--steps 2] [--out FILE.json]
One JSON line.  Needs a GPU (no fallback); profiler off.  A child that fails or overruns its time limit ends the run: nothing more is started."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UPDATES_PER_STEP = 64 * 8
ARMS = {"base": {}, "diag": dict(learner_diagnostics=True), "target": dict(target_kl=1e9),
        "adaptive": dict(learning_rate_schedule="adaptive_kl")}


def child(steps, envs_n, arm):
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
              max_grad_norm=float("inf"), timing_fn=times.append, progress_fn=lambda n, m: seen.update(m), **ARMS[arm])
    torch.cuda.synchronize()
    timed = times[1:]
    keep = ("training/approx_kl", "training/approx_kl_max", "training/clip_fraction", "training/explained_variance", "training/entropy",
            "training/stopped_updates", "training/learning_rate", "training/grad_norm", "training/skipped_updates")
    print(json.dumps(dict(rollout_s=statistics.median(x["rollout_s"] for x in timed), learner_s=statistics.median(x["learner_s"] for x in timed),
                          all_steps=[dict(rollout_s=x["rollout_s"], learner_s=x["learner_s"]) for x in times],
                          last_step_metrics={k: seen[k] for k in keep if k in seen})), flush=True)


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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=2, help="timed training steps per child, after one warm-up step")
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--child-timeout", type=int, default=150)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=tuple(ARMS))
    args = ap.parse_args()
    if args.child:
        return child(args.steps, args.envs, args.child)
    names = list(ARMS)
    runs = {a: [] for a in names}
    for rnd in range(args.rounds):
        for arm in names[rnd % len(names):] + names[:rnd % len(names)]:      # rotate: no arm always runs first or last
            cmd = [sys.executable, os.path.abspath(__file__), "--child", arm, "--steps", str(args.steps), "--envs", str(args.envs)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.child_timeout)
            if r.returncode:
                sys.exit(f"arm {arm}, round {rnd}: child exited with status {r.returncode}; stopping")
            runs[arm].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(f"round {rnd} arm {arm}: rollout_s {runs[arm][-1]['rollout_s']:.3f} learner_s {runs[arm][-1]['learner_s']:.3f}", file=sys.stderr, flush=True)
    out = dict(workload=f"ppo.train, bench.py --config 3 hyper-parameters, {args.envs} envs, {args.rounds} rounds of rotating fresh processes, "
                        f"1 warm-up + {args.steps} timed training steps each; every arm with max_grad_norm=inf",
               arms={a: repr(ARMS[a]) for a in names}, **{a: summary(runs[a]) for a in names})
    base = out["base"]["learner_s"]
    out["base_arm_range_s"] = base["max"] - base["min"]
    for a in names[1:]:
        d = out[a]["learner_s"]["median"] - base["median"]
        out[a + "_vs_base"] = dict(learner_s_ratio=out[a]["learner_s"]["median"] / base["median"], learner_s_difference=d,
                                   learner_us_per_minibatch=1e6 * d / UPDATES_PER_STEP, inside_base_arm_range=abs(d) <= out["base_arm_range_s"])
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
