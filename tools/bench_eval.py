"""What a training run's evaluations cost, per-step against one launch (`rr_env_unroll_eval`), in ONE process, alternating, at the
launcher's shapes [REF brax_rodent_run_ppo.py:97-151]:

  * `acting.Evaluator.run_evaluation`: 128 envs, episode_length 150, rodent_new, CG 8/8 -> eval/epoch_eval_time;
  * `rollout.eval_rollout`: 1 env, 500 steps, deterministic policy -> host clock around a device synchronise.

The path is selected by RR_FUSED_EVAL (1 = one launch; 0, the default = the per-step loop).  On a build without the one-launch path (no `actor_fn` / `actor`
arguments) the script times the per-step path alone: that is the baseline.

usage: python tools/bench_eval.py [--evals 5] [--warmup 2] [--envs 128] [--episode 150] [--steps 500] [--out FILE.json]
One JSON line: per form and path the samples, median, min and max in seconds.  Needs a GPU (no fallback); profiler off."""
import argparse
import inspect
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "brax-rodent-run_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--evals", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--envs", type=int, default=128)
    ap.add_argument("--episode", type=int, default=150)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--model", default="rodent_new.xml")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    from rodent_amd import envs, jax_random, rollout
    from rodent_amd.envs import wrappers
    from rodent_amd.training import acting, networks, running_statistics
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval: needs a GPU")
    dev = torch.device("cuda:0")
    t = np.arange(250, dtype=np.float64)
    track = np.stack([0.004 * t, np.zeros(250), np.full(250, 0.0681)], axis=1)
    env = envs.get_environment("rodent", track_pos=track, num_envs=a.envs, xml_path=a.model, iterations=8, ls_iterations=8, device=dev)
    env1 = env.with_num_envs(1)
    torch.manual_seed(0)
    nets = networks.make_ppo_networks(env.observation_size, env.action_size, device=dev)
    make_policy = networks.make_inference_fn(nets)
    norm = running_statistics.init_state(env.observation_size, dev)
    params = (norm, nets.policy_network)
    actor = acting.actor_params(nets.policy_network, norm, nets.parametric_action_distribution.min_std)
    one_launch = "actor_fn" in inspect.signature(acting.Evaluator.__init__).parameters and "actor" in inspect.signature(rollout.eval_rollout).parameters
    weval = wrappers.wrap(env, episode_length=a.episode, action_repeat=1)
    kw = dict(actor_fn=lambda p: actor) if one_launch else {}
    ev = acting.Evaluator(weval, lambda p: make_policy(p, deterministic=False), a.envs, a.episode, 1, jax_random.PRNGKey(0), **kw)
    rkw = dict(actor=actor) if one_launch else {}

    def evaluator():
        return ev.run_evaluation(params, {})["eval/epoch_eval_time"]

    def rollout_500():
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        rollout.eval_rollout(env1, make_policy, params, steps=a.steps, seed=0, **rkw)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0

    paths = [("per_step", "0")] + ([("one_launch", "1")] if one_launch else [])
    res = {}
    for form, fn in (("evaluator", evaluator), ("eval_rollout", rollout_500)):
        samples = {name: [] for name, _ in paths}
        for i in range(a.warmup + a.evals):
            for name, switch in paths:              # alternating: both paths see the same clocks and the same neighbours
                os.environ["RR_FUSED_EVAL"] = switch
                s = fn()
                if i >= a.warmup:
                    samples[name].append(s)
        res[form] = {name: dict(samples_s=[round(x, 5) for x in v], median_s=round(statistics.median(v), 5), min_s=round(min(v), 5),
                                max_s=round(max(v), 5)) for name, v in samples.items()}
    os.environ.pop("RR_FUSED_EVAL", None)
    out = dict(bench="eval", model=a.model, evaluator=dict(envs=a.envs, episode_length=a.episode), eval_rollout=dict(envs=1, steps=a.steps),
               evals=a.evals, warmup=a.warmup, one_launch_available=one_launch, device=torch.cuda.get_device_name(0), results=res)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
