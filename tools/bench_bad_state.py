"""Cost of the bad-state check when it is ON: rodent_optimized under random actions through Episode(150) + AutoReset, T wrapped steps per
launch (`rr_env_unroll`), in ONE process, two batches alternating that start from the same reset and get the same actions:

    off     Rodent(...)                         (bad_state_max = 0: the epilogue's check is one scalar compare)
    on      Rodent(..., bad_state_max=1e10)     (one pass over qpos / qvel in LDS and a ballot per env step)

usage: python tools/bench_bad_state.py [--envs 2048] [--unroll 20] [--launches 40] [--repeats 5] [--out FILE.json]
One JSON line: ms per env step (HIP-event time of the step-kernel launches) per arm and window, medians, ranges, the ratio on / off per
window, the events counted and whether the two final states are identical (they are when nothing trips).
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
    ap.add_argument("--unroll", type=int, default=20, help="env steps per launch")
    ap.add_argument("--launches", type=int, default=40, help="launches per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2, help="untimed launches per arm")
    ap.add_argument("--bad-state-max", type=float, default=1e10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    from rodent_amd import envs, jax_random
    from rodent_amd.envs import wrappers
    if not torch.cuda.is_available():
        raise SystemExit("bench_bad_state: needs a GPU")
    dev = torch.device("cuda:0")
    N, T = a.envs, a.unroll
    t = np.arange(250, dtype=np.float64)
    track = np.stack([0.004 * t, np.zeros(250), np.full(250, 0.0681)], axis=1)
    keys = jax_random.split(jax_random.PRNGKey(0), N)
    arms = {}
    for name, thr in (("off", None), ("on", a.bad_state_max)):
        env = envs.get_environment("rodent", track_pos=track, num_envs=N, xml_path="rodent_optimized.xml", iterations=8, ls_iterations=8, device=dev,
                                   bad_state_max=thr)
        wenv = wrappers.wrap(env, episode_length=150, action_repeat=1)
        arms[name] = dict(env=env, wenv=wenv, state=wenv.reset(keys), ms=[])
    g = torch.Generator(device=dev).manual_seed(0)

    def window(launches, record, order):
        acts = torch.rand(launches * T, N, 30, device=dev, generator=g) * 2 - 1
        for name in order:                              # alternating: both arms run the same actions in every window
            arm = arms[name]
            arm["env"]._batch.set_timing(True)          # (re)starts the event ring's totals
            for l in range(launches):
                arm["state"] = arm["wenv"].unroll(arm["state"], acts[l * T:(l + 1) * T])
            torch.cuda.synchronize()
            ms, n = arm["env"]._batch.kernel_time()
            if record:
                arm["ms"].append(ms / (n * T))

    window(a.warmup, False, ("off", "on"))
    for r in range(a.repeats):
        window(a.launches, True, ("off", "on") if r % 2 == 0 else ("on", "off"))      # the first place changes hands
    off, on = arms["off"]["state"], arms["on"]["state"]
    same = all(bool(torch.equal(x, y)) for x, y in ((off.pipeline_state.qpos, on.pipeline_state.qpos), (off.pipeline_state.qvel, on.pipeline_state.qvel),
                                                    (off.obs, on.obs), (off.reward, on.reward), (off.done, on.done), (off.info["steps"], on.info["steps"])))
    med = {k: statistics.median(v["ms"]) for k, v in arms.items()}
    ratios = [x / y for x, y in zip(arms["on"]["ms"], arms["off"]["ms"])]
    out = dict(model="rodent_optimized.xml", envs=N, iterations=[8, 8], n_frames=10, episode_length=150, steps_per_launch=T, launches_per_window=a.launches,
               repeats=a.repeats, bad_state_max=a.bad_state_max, ms_per_env_step={k: v["ms"] for k, v in arms.items()}, median_ms_per_env_step=med,
               range_frac_of_median={k: (max(v["ms"]) - min(v["ms"])) / med[k] for k, v in arms.items()}, ratio_on_to_off=med["on"] / med["off"],
               per_window_ratio_on_to_off=ratios, per_window_ratio_range=[min(ratios), max(ratios)], bad_state_events=arms["on"]["env"].bad_states(),
               final_state_identical=same, final_state_finite=bool(torch.isfinite(on.obs).all()), device=torch.cuda.get_device_name(0))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
