"""Cost of clip restarts: env-steps/s of a pose env whose restarted episodes rejoin the clip (`Rodent(clip_restarts=K)`: the
rr_restart_kernel instances -- the slot next to the step count, the clip-end term, the restore read from a bank of K start states)
against the same env without them, on the family its multi-step launches would otherwise run (pose termination with a threshold that
never fires: the rr_poseterm_kernel instances), the SAME build, alternating in one process on one GPU.  No gate: it reports.

All three envs (base, K = 1, K = 8): rodent_optimized.xml, CG 8/8, n_frames 10, 2048 envs through Episode(150) + AutoReset in multi-step
launches, tracking a synthetic reference pose (identity quaternion, qpos0's joints) with the default weights and scales and
max_pos_error 1e9.  Default: random actions through `rr_env_unroll`, --unroll env steps per launch -- the workload of bench.py config 2.
--actor: the one-launch rollout with the actor inside (`rr_env_unroll_policy`, a 4 x 32 policy, one segment of --unroll steps per
launch); all three sides run the actor that reads 26 observation entries per lane.  Each repeat times --launches launches per env with a
host clock around a device synchronise, base then K = 1 then K = 8; the medians, the per-repeat values and the range are printed as one
JSON line.

usage: python tools/bench_restart.py [--actor] [--num-envs 2048] [--unroll 50] [--launches 4] [--repeats 7] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "brax-rodent-run_amd")]
SIDES = (("base", 0), ("k1", 1), ("k8", 8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--actor", action="store_true")
    ap.add_argument("--num-envs", type=int, default=2048)
    ap.add_argument("--unroll", type=int, default=50)
    ap.add_argument("--launches", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from rodent_amd import assets, envs, jax_random, mjcf
    from rodent_amd.envs import wrappers
    from rodent_amd.training import acting, networks, running_statistics
    from tests.util import synthetic_track
    dev = torch.device("cuda:0")
    N, U = args.num_envs, args.unroll
    track = synthetic_track()
    T = len(track)
    keys = jax_random.split(jax_random.PRNGKey(0), N)
    q0 = np.asarray(mjcf.load_blob(assets.asset_path("rodent_optimized"))["qpos0"], np.float64)
    quat, joints = np.tile([1.0, 0.0, 0.0, 0.0], (T, 1)), np.tile(q0[7:], (T, 1))
    sides = {}
    for name, K in SIDES:
        kw = dict(track_quat=quat, track_joints=joints, max_pos_error=1e9, clip_restarts=K)
        env = envs.get_environment("rodent", track_pos=track, num_envs=N, xml_path="rodent_optimized.xml", iterations=8, ls_iterations=8, device=dev, **kw)
        wenv = wrappers.wrap(env, episode_length=150, action_repeat=1)
        gen = torch.Generator(device=dev)
        gen.manual_seed(1234)
        side = dict(env=env, wenv=wenv, gen=gen, state=wenv.reset(keys), ms=[])
        if args.actor:
            torch.manual_seed(5)
            nets = networks.make_ppo_networks(env.observation_size, env.action_size, device=dev)
            norm = running_statistics.init_state(env.observation_size, dev)
            assert acting.fused_unroll_supported(wenv, nets.policy_network, nets.parametric_action_distribution)
            side["actor"] = acting.actor_params(nets.policy_network, norm, nets.parametric_action_distribution.min_std)
            side["buf"] = acting.UnrollBuffer(1, N, U, env.observation_size, env.action_size, dev)
        sides[name] = side

    def run(side, launches):
        A = side["env"].action_size
        for _ in range(launches):
            if args.actor:
                b = side["buf"]
                traj = dict(obs=b.obs[0], raw_action=b.raw_action[0], log_prob=b.log_prob[0], reward=b.reward[0], discount=b.discount[0], truncation=b.truncation[0])
                noise = torch.empty(U, N, A, device=dev).normal_(generator=side["gen"])
                side["state"], _ = side["wenv"].unroll_policy(side["state"], side["actor"], noise, traj)
            else:
                a = torch.empty(U, N, A, device=dev).uniform_(-1.0, 1.0, generator=side["gen"])
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
    res = {"form": "rr_env_unroll_policy (actor inside)" if args.actor else "rr_env_unroll (random actions)", "num_envs": N, "unroll": U,
           "launches_per_repeat": args.launches, "device": torch.cuda.get_device_name(dev)}
    for name, side in sides.items():
        ms = np.array(side["ms"])
        res[name] = {"ms_per_step": [round(float(x), 5) for x in ms], "median_ms_per_step": round(float(np.median(ms)), 5),
                     "range_percent": round(float((ms.max() - ms.min()) / np.median(ms) * 100), 3),
                     "env_steps_per_s": round(N / (float(np.median(ms)) * 1e-3))}
    for name in ("k1", "k8"):
        res[name + "_over_base_median_time"] = round(res[name]["median_ms_per_step"] / res["base"]["median_ms_per_step"], 5)
        res[name + "_per_repeat_time_ratio"] = [round(float(a / b), 5) for a, b in zip(sides[name]["ms"], sides["base"]["ms"])]
        st = sides[name]["state"]
        assert float(st.metrics["quat_reward"].max()) > 0 and torch.isfinite(st.obs).all() and int(st.info["restart_slot"].max()) <= 7
    if not args.actor:          # same actions, and K = 1 restores the state the base restores: the two sides walked the same states
        res["k1_final_states_identical"] = bool(torch.equal(sides["k1"]["state"].pipeline_state.qpos, sides["base"]["state"].pipeline_state.qpos))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
