"""Cost of multi-clip tracking: rodent_optimized under random actions through Episode(150) + AutoReset, T wrapped steps per launch
(`rr_env_unroll`), in ONE process, two batches alternating that start from the same keys and get the same actions:

    single      track_pos [250, 3]      (null `clip`: every env reads the one track)
    clips       track_pos [8, 250, 3]   (env e on the clip drawn at its reset: one scalar load of clip[e] per env step, then the same two reads)

Clip 0 of the second arm is the first arm's line, the others are the line turned to other headings, so the envs on clip 0 compute what
their twins in the first arm compute (reported as a check).

usage: python tools/bench_multiclip.py [--envs 2048] [--clips 8] [--unroll 20] [--launches 40] [--repeats 5] [--out FILE.json]
One JSON line: ms per env step (HIP-event time of the step-kernel launches) per arm and repeat, medians, ranges, the ratio to single.
Needs a GPU (no fallback); profiler off."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "brax-rodent-run_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--unroll", type=int, default=20, help="env steps per launch")
    ap.add_argument("--launches", type=int, default=40, help="launches per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2, help="untimed launches per arm")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    from rodent_amd import envs, jax_random
    from rodent_amd.envs import wrappers
    if not torch.cuda.is_available():
        raise SystemExit("bench_multiclip: needs a GPU")
    dev = torch.device("cuda:0")
    N, T = a.envs, a.unroll
    t = np.arange(250, dtype=np.float64)
    heading = np.linspace(0.0, np.pi / 2, a.clips)
    tracks = np.stack([np.stack([0.004 * t * np.cos(h), 0.004 * t * np.sin(h), np.full(250, 0.0681)], axis=1) for h in heading])
    keys = jax_random.split(jax_random.PRNGKey(0), N)
    arms = {}
    for name, track in (("single", tracks[0]), ("clips", tracks)):
        env = envs.get_environment("rodent", track_pos=track, num_envs=N, xml_path="rodent_optimized.xml", iterations=8, ls_iterations=8, device=dev)
        wenv = wrappers.wrap(env, episode_length=150, action_repeat=1)
        arms[name] = dict(env=env, wenv=wenv, state=wenv.reset(keys), ms=[])
    g = torch.Generator(device=dev).manual_seed(0)

    def window(launches, record):
        acts = torch.rand(launches * T, N, 30, device=dev, generator=g) * 2 - 1
        for name, arm in arms.items():              # alternating: both arms run the same actions in every window
            arm["env"]._batch.set_timing(True)      # (re)starts the event ring's totals
            for l in range(launches):
                arm["state"] = arm["wenv"].unroll(arm["state"], acts[l * T:(l + 1) * T])
            torch.cuda.synchronize()
            ms, n = arm["env"]._batch.kernel_time()
            if record:
                arm["ms"].append(ms / (n * T))

    window(a.warmup, False)
    for _ in range(a.repeats):
        window(a.launches, True)
    s, c = arms["single"]["state"], arms["clips"]["state"]
    ids = c.info["clip"]
    on0 = ids == 0
    same = bool(torch.equal(s.pipeline_state.qpos[on0], c.pipeline_state.qpos[on0]) and torch.equal(s.obs[on0], c.obs[on0])
                and torch.equal(s.reward[on0], c.reward[on0]))
    med = {k: statistics.median(v["ms"]) for k, v in arms.items()}
    out = dict(model="rodent_optimized.xml", envs=N, clips=a.clips, track_len=250, iterations=[8, 8], n_frames=10, episode_length=150,
               steps_per_launch=T, launches_per_window=a.launches, repeats=a.repeats, ms_per_env_step={k: v["ms"] for k, v in arms.items()},
               median_ms_per_env_step=med, range_frac_of_median={k: (max(v["ms"]) - min(v["ms"])) / med[k] for k, v in arms.items()},
               ratio_to_single=med["clips"] / med["single"], per_window_ratio_to_single=[x / y for x, y in zip(arms["clips"]["ms"], arms["single"]["ms"])],
               envs_per_clip=torch.bincount(ids.long(), minlength=a.clips).tolist(), envs_on_clip0_equal_single_bitwise=same,
               final_state_finite=bool(torch.isfinite(c.obs).all()), device=torch.cuda.get_device_name(0))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
