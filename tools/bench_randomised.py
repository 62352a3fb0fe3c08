"""Cost of domain randomisation: rodent_optimized under random actions through Episode(150) + AutoReset, T wrapped steps per launch
(`rr_env_unroll`), in ONE process, three batches alternating that start from the same reset and get the same actions:

    plain       no per-env parameters                  (rr_step_kernel: every env reads the model's shared rows)
    identity    every env carries the model's own rows (rr_rand_kernel: private rows, the same physics bit for bit)
    spread      env e on parameter set e % 3           (friction x {0.5, 1, 2}, damping x {0.5, 1, 1.5}, armature x {1, 2, 1}, gain x {0.8, 1, 1.2})

usage: python tools/bench_randomised.py [--envs 2048] [--unroll 20] [--launches 40] [--repeats 5] [--out FILE.json]
One JSON line: ms per env step (HIP-event time of the step-kernel launches) per arm and repeat, medians, ranges, ratios to plain.
Needs a GPU (no fallback); profiler off."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "brax-rodent-run_amd"))

FACTORS = dict(geom_friction=(0.5, 1.0, 2.0), dof_damping=(0.5, 1.0, 1.5), dof_armature=(1.0, 2.0, 1.0), gain=(0.8, 1.0, 1.2))


def fields(m, n, spread):
    """[n, ...] fields: the model's own values, or env e on set e % 3."""
    import numpy as np
    f32 = lambda k: np.asarray(m[k], np.float32)
    g = np.arange(n) % 3
    s = lambda k, shape: (np.asarray(FACTORS[k], np.float32)[g] if spread else np.ones(n, np.float32)).reshape((n,) + (1,) * shape)
    gain, bias = f32("actuator_gainprm0")[:, None], f32("actuator_biasprm")
    position = (bias[:, 1] == -gain[:, 0]) & (gain[:, 0] != 0)
    bias_n = np.repeat(bias[None], n, axis=0)
    bias_n[:, position, 1] = bias[None, position, 1] * s("gain", 1)
    return dict(geom_friction=f32("geom_friction")[None] * s("geom_friction", 2), dof_damping=f32("dof_damping")[None] * s("dof_damping", 1),
                dof_armature=f32("dof_armature")[None] * s("dof_armature", 1), actuator_gainprm=gain[None] * s("gain", 2), actuator_biasprm=bias_n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--unroll", type=int, default=20, help="env steps per launch")
    ap.add_argument("--launches", type=int, default=40, help="launches per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2, help="untimed launches per arm")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    from rodent_amd import envs, jax_random, ktables
    from rodent_amd.envs import wrappers
    if not torch.cuda.is_available():
        raise SystemExit("bench_randomised: needs a GPU")
    dev = torch.device("cuda:0")
    N, T = a.envs, a.unroll
    t = np.arange(250, dtype=np.float64)
    track = np.stack([0.004 * t, np.zeros(250), np.full(250, 0.0681)], axis=1)
    keys = jax_random.split(jax_random.PRNGKey(0), N)
    arms = {}
    for name in ("plain", "identity", "spread"):
        env = envs.get_environment("rodent", track_pos=track, num_envs=N, xml_path="rodent_optimized.xml", iterations=8, ls_iterations=8, device=dev)
        if name != "plain":
            tabs = ktables.env_param_tables(env.sys.tables, fields(env.sys.tables, N, name == "spread"))
            env.set_env_params(*(torch.from_numpy(x).to(dev) for x in tabs))
        wenv = wrappers.wrap(env, episode_length=150, action_repeat=1)
        arms[name] = dict(env=env, wenv=wenv, state=wenv.reset(keys), ms=[])
    g = torch.Generator(device=dev).manual_seed(0)

    def window(launches, record):
        acts = torch.rand(launches * T, N, 30, device=dev, generator=g) * 2 - 1
        for name, arm in arms.items():              # alternating: every arm runs the same actions in every window
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
    p, i = arms["plain"]["state"], arms["identity"]["state"]
    same = bool(torch.equal(p.pipeline_state.qpos, i.pipeline_state.qpos) and torch.equal(p.obs, i.obs))
    med = {k: statistics.median(v["ms"]) for k, v in arms.items()}
    out = dict(model="rodent_optimized.xml", envs=N, iterations=[8, 8], n_frames=10, episode_length=150, steps_per_launch=T,
               launches_per_window=a.launches, repeats=a.repeats, ms_per_env_step={k: v["ms"] for k, v in arms.items()}, median_ms_per_env_step=med,
               range_frac_of_median={k: (max(v["ms"]) - min(v["ms"])) / med[k] for k, v in arms.items()},
               ratio_to_plain={k: med[k] / med["plain"] for k in ("identity", "spread")},
               per_window_ratio_to_plain={k: [x / y for x, y in zip(arms[k]["ms"], arms["plain"]["ms"])] for k in ("identity", "spread")},
               identity_equals_plain_bitwise=same, spread_final_state_finite=bool(torch.isfinite(arms["spread"]["state"].obs).all()),
               private_row_bytes_per_env=4 * (int(arms["plain"]["env"].sys.nv) * 16 + 30 * 8 + int(arms["plain"]["env"].sys.ncon) * 26),
               device=torch.cuda.get_device_name(0))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
