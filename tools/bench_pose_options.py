"""Cost of one option of the pose family: env-steps/s of an env with the option against the env one rung below it, the SAME build,
alternating in one process on one GPU.  No gate: it reports.

  --option pose      a plain env | a pose env (`track_quat`, `track_joints`)
  --option refobs    a pose env | the same with `reference_obs_frames=--frames` (1633 against 1263 columns at 5)
  --option poseterm  a pose env | the same with three thresholds of 1e30: every comparison made, no episode ended by it
  --option body      a pose env | the same with `track_bodies` (the forward kinematics of the reference pose at every frame,
                     `preprocessing.extract_features`), B = all bodies, E = foot_L, foot_R, hand_L, hand_R, skull
  --option velocity  that body env | the same with the clip's velocities (`track_velocity`, `track_angular_velocity`,
                     `track_joint_velocity`: `preprocessing.compute_velocity_from_kinematics` of the reference poses); both sides run
                     the body instances, and the final states must be identical, with and without --actor
  --option restart   a pose env with max_pos_error 1e9 (the family its multi-step launches would otherwise run) | the same with
                     `clip_restarts` 1 | with 8
  --option library   that `clip_restarts` 8 env on three copies of the clip ([3, T, ...] arrays) | the same with `clip_lengths`
                     (T, 2T/3, T/3) and `restart_across_clips`
  --option sampling  that `clip_restarts` 8 env on three copies of the clip with `restart_across_clips` | the same with
                     `restart_sampling="weighted"` (weights 1, 2, 5) and `clip_outcomes`
  --option reference_restart  that `clip_restarts` 8, `restart_across_clips` env with `reset_to_reference` on three copies of the clip |
                     the same with `clip_restarts` 1 and `restart_from_reference`: every restore draws a clip and a frame, builds its
                     state and runs the reset's forward pass in the launch; the episode-end rate of the timed side is reported

All envs: rodent_optimized.xml, CG 8/8, n_frames 10, --num-envs envs through Episode(150) + AutoReset in multi-step launches, tracking a
synthetic reference pose (identity quaternion, qpos0's joints) with the default weights and scales.  Default: random actions through
`rr_env_unroll`, --unroll env steps per launch -- the workload of bench.py config 2.  --actor (poseterm, body, velocity, restart, library, sampling, reference_restart): the one-launch
rollout with the actor inside (`rr_env_unroll_policy`, a 4 x 32 policy, one segment of --unroll steps per launch).  After two warm-up
launches per side, each repeat times --launches launches per side, in the order above, with a host clock around a device synchronise;
the medians, the per-repeat values, the ranges and the ratios against the first side are printed as one JSON line.

usage: python tools/bench_pose_options.py --option {pose,refobs,poseterm,body,velocity,restart,library,sampling,reference_restart} [--actor] [--frames 5] [--num-envs 2048]
                                          [--unroll 50] [--launches 4] [--repeats 7] [--out FILE]"""
import argparse
import json
import os
import sys
import time
from typing import Callable, NamedTuple, Optional

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "brax-rodent-run_amd")]
END_EFFECTORS = (11, 15, 59, 64, 54)      # foot_L, foot_R, hand_L, hand_R, skull of rodent_optimized
NEVER = dict(max_pos_error=1e30, max_quat_error=1e30, max_joint_error=1e30)


class Option(NamedTuple):
    """`sides`: (name, constructor keywords on top of the side's base keywords) in timing order, the first the one every ratio is taken
    against; `pose_base`: whether the first side is a pose env too; `actor`: whether --actor is a mode of it; `check`: the closing
    assertion on the final state of every side but the first; `identical`: the JSON key under which the final qpos of that side is
    compared with the first side's (same actions, and the option moves no state), None: no such claim."""
    sides: tuple
    pose_base: bool
    actor: bool
    check: Callable
    identical: Optional[tuple] = None
    identical_with_actor: bool = False      # whether that claim is also checked under --actor
    clips: int = 0                          # > 0: every side tracks that many copies of the clip, [clips, T, ...] arrays


def _alive(st):
    return float(st.metrics["quat_reward"].max()) > 0 and bool(torch.isfinite(st.obs).all())


def options(frames: int, bodies: Callable, velocity: dict, T: int = 250) -> dict:
    """The table.  `bodies`: an env of the model -> track_bodies (a callable keyword is called with the first side's env, or a one-env
    probe while that side is being built); `velocity`: the three velocity keywords; `T`: the clip's frames."""
    body = dict(track_bodies=bodies, end_effector_ids=END_EFFECTORS)
    k8 = dict(max_pos_error=1e9, clip_restarts=8)
    across = dict(k8, restart_across_clips=True)
    ref8 = dict(across, reset_to_reference=True)
    return {
        "reference_restart": Option((("across", ref8), ("reference", dict(ref8, clip_restarts=1, restart_from_reference=True))), True, True,
                                    lambda st: _alive(st) and int(st.info["restart_draws"].max()) >= 1 and 0 <= int(st.info["clip"].min())
                                    and int(st.info["clip"].max()) <= 2, clips=3),
        "sampling": Option((("across", across), ("sampling", dict(across, restart_sampling="weighted", clip_outcomes=True))), True, True,
                           lambda st: _alive(st) and int(st.info["restart_slot"].max()) <= 7 and int(st.info["restart_draws"].max()) >= 1,
                           clips=3),
        "library": Option((("k8", k8), ("library", dict(k8, clip_lengths=(T, 2 * T // 3, T // 3), restart_across_clips=True))), True, True,
                          lambda st: _alive(st) and int(st.info["restart_slot"].max()) <= 7 and 0 <= int(st.info["clip"].min()) and int(st.info["clip"].max()) <= 2,
                          clips=3),
        "velocity": Option((("body", body), ("velocity", dict(body, **velocity))), True, True,
                           lambda st: _alive(st) and all(bool(torch.isfinite(st.metrics[k]).all()) and float(st.metrics[k].max()) > 0
                                                         for k in ("lin_vel_reward", "ang_vel_reward", "joint_vel_reward")),
                           ("final_states_identical", "velocity"), True),
        "pose": Option((("plain", {}), ("pose", {})), False, False, lambda st: float(st.metrics["quat_reward"].max()) > 0),
        "refobs": Option((("pose", {}), ("refobs", dict(reference_obs_frames=frames))), True, False, _alive),
        "poseterm": Option((("pose", {}), ("poseterm", NEVER)), True, True, lambda st: float(st.metrics["pose_fail"].max()) == 0.0 and _alive(st),
                           ("final_states_identical", "poseterm")),
        "body": Option((("pose", {}), ("body", dict(track_bodies=bodies, end_effector_ids=END_EFFECTORS))), True, True,
                       lambda st: _alive(st) and bool(torch.isfinite(st.metrics["body_reward"]).all()), ("final_states_identical", "body")),
        "restart": Option(tuple((name, dict(max_pos_error=1e9, clip_restarts=K)) for name, K in (("base", 0), ("k1", 1), ("k8", 8))), True, True,
                          lambda st: _alive(st) and int(st.info["restart_slot"].max()) <= 7, ("k1_final_states_identical", "k1")),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--option", required=True, choices=("pose", "refobs", "poseterm", "body", "velocity", "restart", "library", "sampling", "reference_restart"))
    ap.add_argument("--actor", action="store_true")
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--num-envs", type=int, default=2048)
    ap.add_argument("--unroll", type=int, default=50)
    ap.add_argument("--launches", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from rodent_amd import assets, envs, jax_random, mjcf, preprocessing
    from rodent_amd.envs import wrappers
    from rodent_amd.training import acting, networks, running_statistics
    from tests.util import synthetic_track
    N, U = args.num_envs, args.unroll
    track = synthetic_track()
    T = len(track)
    q0 = np.asarray(mjcf.load_blob(assets.asset_path("rodent_optimized"))["qpos0"], np.float64)
    quat, joints = np.tile([1.0, 0.0, 0.0, 0.0], (T, 1)), np.tile(q0[7:], (T, 1))
    qpos = np.concatenate([np.asarray(track, np.float64), quat, joints], axis=1)
    qvel = preprocessing.compute_velocity_from_kinematics(np.concatenate([qpos, qpos[-1:]], axis=0), 0.02)      # [T, nv], the last row zero
    velocity = dict(track_velocity=qvel[:, :3], track_angular_velocity=qvel[:, 3:6], track_joint_velocity=qvel[:, 6:])
    opt = options(args.frames, lambda env: preprocessing.extract_features(env, qpos).body_positions, velocity, T)[args.option]
    if args.actor and not opt.actor:
        ap.error(f"--actor: --option {args.option} has no such mode (poseterm, body, velocity, restart, library, sampling and reference_restart have)")
    if opt.clips:      # the same clip `clips` times over
        track, quat, joints = (np.stack([np.asarray(a)] * opt.clips) for a in (track, quat, joints))
    dev = torch.device("cuda:0")
    keys = jax_random.split(jax_random.PRNGKey(0), N)
    first, sides = opt.sides[0][0], {}

    def model_env():      # an env to run forward kinematics on: the first side's, or a probe while that side is being built
        if first in sides:
            return sides[first]["env"]
        return envs.get_environment("rodent", track_pos=track, num_envs=1, xml_path="rodent_optimized.xml", device=dev)
    for name, kw in opt.sides:
        kw = {k: (v(model_env()) if callable(v) else v) for k, v in kw.items()}
        if opt.pose_base or name != first:
            kw.update(track_quat=quat, track_joints=joints)
        env = envs.get_environment("rodent", track_pos=track, num_envs=N, xml_path="rodent_optimized.xml", iterations=8, ls_iterations=8, device=dev, **kw)
        if env.clip_weights() is not None:      # unequal weights, so the draw's scan and search do work
            env.set_clip_weights([1, 2, 5])
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
    res = {"form": "rr_env_unroll_policy (actor inside)" if args.actor else "rr_env_unroll (random actions)"} if opt.actor else {}
    res["num_envs"] = N
    if args.option == "refobs":
        res.update(frames=args.frames, obs_width={k: v["env"].observation_size for k, v in sides.items()})
    res.update(unroll=U, launches_per_repeat=args.launches, device=torch.cuda.get_device_name(dev))
    for name, side in sides.items():
        ms = np.array(side["ms"])
        res[name] = {"ms_per_step": [round(float(x), 5) for x in ms], "median_ms_per_step": round(float(np.median(ms)), 5),
                     "range_percent": round(float((ms.max() - ms.min()) / np.median(ms) * 100), 3),
                     "env_steps_per_s": round(N / (float(np.median(ms)) * 1e-3))}
    others = [name for name, _ in opt.sides[1:]]
    for name in others:
        res[f"{name}_over_{first}_median_time"] = round(res[name]["median_ms_per_step"] / res[first]["median_ms_per_step"], 5)
        res["per_repeat_time_ratio" if len(others) == 1 else name + "_per_repeat_time_ratio"] = [
            round(float(a / b), 5) for a, b in zip(sides[name]["ms"], sides[first]["ms"])]
        assert opt.check(sides[name]["state"]), (args.option, name)
    if args.option == "sampling":      # the counters of the timed side: every wrapped step of every launch, and each end by exactly one cause
        table = sides["sampling"]["env"].clip_outcomes()
        assert table[:, 4].sum() == N * U * (2 + args.repeats * args.launches) and (table[:, 1:4].sum(1) == table[:, 0]).all(), table
        res["outcomes"] = table.tolist()
    if args.option == "reference_restart":      # restores of the timed side per wrapped env step, warm-up launches included
        steps = N * U * (2 + args.repeats * args.launches)
        res["episode_ends_per_env_step"] = round(float(sides["reference"]["state"].info["restart_draws"].sum()) / steps, 6)
    if opt.identical and (not args.actor or opt.identical_with_actor):
        key, name = opt.identical
        res[key] = bool(torch.equal(sides[name]["state"].pipeline_state.qpos, sides[first]["state"].pipeline_state.qpos))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
