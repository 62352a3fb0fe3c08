"""Cost of the reference observation: env-steps/s of a pose env whose observation carries --frames reference frames
(`Rodent(reference_obs_frames=H)`) against a pose env without them, the SAME build, alternating in one process on one GPU.

Both envs: rodent_optimized.xml, CG 8/8, n_frames 10, 2048 envs, random actions through Episode(150) + AutoReset in multi-step launches
(`rr_env_unroll`, --unroll env steps each) -- the workload of bench.py config 2 -- tracking a synthetic reference pose (identity
quaternion, qpos0's joints) with the default weights and scales.  Each repeat times --launches launches per env with a host clock
around a device synchronise, pose then pose + frames; the medians, the per-repeat values and the range are printed as one JSON line.

usage: python tools/bench_refobs.py [--num-envs 2048] [--frames 5] [--unroll 50] [--launches 4] [--repeats 7] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "brax-rodent-run_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--unroll", type=int, default=50)
    ap.add_argument("--launches", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from rodent_amd import envs, jax_random
    from rodent_amd.envs import wrappers
    from tests.util import synthetic_track
    dev = torch.device("cuda:0")
    N, U = args.num_envs, args.unroll
    track = synthetic_track()
    T = len(track)
    keys = jax_random.split(jax_random.PRNGKey(0), N)
    from rodent_amd import assets, mjcf
    rest = np.asarray(mjcf.load_blob(assets.asset_path("rodent_optimized"))["qpos0"], np.float64)[7:]
    sides = {}
    for name in ("pose", "refobs"):
        kw = dict(track_quat=np.tile([1.0, 0.0, 0.0, 0.0], (T, 1)), track_joints=np.tile(rest, (T, 1)))
        if name == "refobs":
            kw["reference_obs_frames"] = args.frames
        env = envs.get_environment("rodent", track_pos=track, num_envs=N, xml_path="rodent_optimized.xml", iterations=8, ls_iterations=8, device=dev, **kw)
        wenv = wrappers.wrap(env, episode_length=150, action_repeat=1)
        gen = torch.Generator(device=dev)
        gen.manual_seed(1234)
        sides[name] = dict(env=env, wenv=wenv, gen=gen, state=wenv.reset(keys), ms=[])

    def run(side, launches):
        for _ in range(launches):
            a = torch.empty(U, N, side["env"].action_size, device=dev).uniform_(-1.0, 1.0, generator=side["gen"])
            side["state"] = side["wenv"].unroll(side["state"], a)
    for side in sides.values():
        run(side, 2)
    torch.cuda.synchronize(dev)
    for _ in range(args.repeats):
        for side in sides.values():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            run(side, args.launches)
            torch.cuda.synchronize(dev)
            side["ms"].append((time.perf_counter() - t0) * 1e3 / (args.launches * U))
    res = {"num_envs": N, "frames": args.frames, "obs_width": {k: v["env"].observation_size for k, v in sides.items()}, "unroll": U, "launches_per_repeat": args.launches, "device": torch.cuda.get_device_name(dev)}
    for name, side in sides.items():
        ms = np.array(side["ms"])
        res[name] = {"ms_per_step": [round(float(x), 5) for x in ms], "median_ms_per_step": round(float(np.median(ms)), 5),
                     "range_percent": round(float((ms.max() - ms.min()) / np.median(ms) * 100), 3),
                     "env_steps_per_s": round(N / (float(np.median(ms)) * 1e-3))}
    res["refobs_over_pose_median_time"] = round(res["refobs"]["median_ms_per_step"] / res["pose"]["median_ms_per_step"], 5)
    res["per_repeat_time_ratio"] = [round(float(a / b), 5) for a, b in zip(sides["refobs"]["ms"], sides["pose"]["ms"])]
    assert float(sides["refobs"]["state"].metrics["quat_reward"].max()) > 0 and torch.isfinite(sides["refobs"]["state"].obs).all()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
