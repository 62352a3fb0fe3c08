"""Launcher with the configuration of the reference's `brax_rodent_run_ppo.py` [REF :39-55,97-114],
against this package instead of brax (only the imports change):

    from rodent_amd import envs
    from rodent_amd.training.agents.ppo import train as ppo
    from rodent_amd.io import model

Single GPU:  python examples/rodent_run_ppo.py
N GPUs:      python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 examples/rodent_run_ppo.py
wandb / video rendering of the reference are observability only and are replaced by a JSON-lines log.
"""
import argparse
import functools
import json
import os
import sys
import uuid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "brax-rodent-run_amd"))

import numpy as np
import torch

from rodent_amd import assets, envs, jax_random, mjcf, preprocessing, rollout
from rodent_amd.io import model
from rodent_amd.training import acting, networks, optim
from rodent_amd.training.agents.ppo import train as ppo


def domain_randomize(sys, rng):
    """Example `randomization_fn` (--randomize), shaped like brax's: one key per env in `rng` [N, 2]; per env a friction scale in
    [0.6, 1.4] and an actuator gain scale in [0.8, 1.2] (a position actuator's bias term -kp scales with its gain)."""
    n = len(rng)
    friction = np.repeat(sys.geom_friction[None], n, axis=0)
    friction[:, :, 0] *= jax_random.uniform(jax_random.split(rng, 2)[:, 0], 1, 0.6, 1.4)
    scale = jax_random.uniform(jax_random.split(rng, 2)[:, 1], 1, 0.8, 1.2)[:, :, None]
    gain = np.repeat(sys.actuator_gainprm[None], n, axis=0)
    bias = np.repeat(sys.actuator_biasprm[None], n, axis=0)
    gain[:, :, 0:1] *= scale
    bias[:, :, 1:2] *= scale
    in_axes = {"geom_friction": 0, "actuator_gainprm": 0, "actuator_biasprm": 0}
    return sys.tree_replace({"geom_friction": friction, "actuator_gainprm": gain, "actuator_biasprm": bias}), in_axes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-timesteps", type=int, default=500_000_000)
    ap.add_argument("--eval-every", type=int, default=5_000_000)
    ap.add_argument("--envs-per-gpu", type=int, default=1024)          # [REF :43] 1024 * n_gpus
    ap.add_argument("--xml", default="./models/rodent_new.xml")        # [REF Rodent_Env_Brax.py:16]
    ap.add_argument("--clip", default=None, help="reference clip: .npz / .h5 written by preprocessing.save_reference_clip (clip name "
                    "--clip-name) or .npy with the root positions [T,3]; a synthetic line if absent")
    ap.add_argument("--clip-name", nargs="+", default=["84"], help="one or more clip names of --clip; with several, each env follows one of "
                    "them (drawn at reset) and the evaluation reports eval/episode_reward_clip{c} per clip")
    ap.add_argument("--synthetic-clips", type=int, default=1, help="without a clip file: K synthetic lines of different heading (1: one line along x)")
    ap.add_argument("--max-training-steps", type=int, default=None)
    ap.add_argument("--randomize", action="store_true", help="domain randomisation: per-env friction and actuator gain (domain_randomize)")
    ap.add_argument("--bad-state-max", type=float, default=None, help="end and restore episodes whose qpos / qvel is non-finite or exceeds this "
                    "magnitude (MuJoCo's mjMAXVAL is 1e10); off by default")
    ap.add_argument("--track-pose", action="store_true", help="reward the clip's root orientation and joint angles too (Rodent(track_quat=..., "
                    "track_joints=...), untuned default weights); the synthetic line carries the identity quaternion and qpos0's joints.  Not with --randomize")
    ap.add_argument("--reference-frames", type=int, default=0, metavar="H", help="with --track-pose: the observation also carries the clip's next "
                    "H frames (Rodent(reference_obs_frames=H), 0 .. 16): next positions in the root frame, relative orientations, joint-angle "
                    "differences.  Up to 5 the rollout stays one launch; above that it is collected per step")
    ap.add_argument("--max-pos-error", type=float, default=None, metavar="M", help="with --track-pose: end an episode whose root is more than M metres "
                    "from the clip's (Rodent(max_pos_error=M)); a termination, not a truncation.  Off by default")
    ap.add_argument("--max-quat-error", type=float, default=None, metavar="RAD", help="with --track-pose: ... whose root orientation is more than RAD "
                    "radians from the clip's (Rodent(max_quat_error=RAD))")
    ap.add_argument("--max-joint-error", type=float, default=None, metavar="RAD", help="with --track-pose: ... whose joint angles are more than RAD "
                    "radians (2-norm over the joints) from the clip's (Rodent(max_joint_error=RAD))")
    ap.add_argument("--track-bodies", action="store_true", help="with --track-pose: reward the clip's body positions too (Rodent(track_bodies=..., "
                    "untuned default weights): every body of the model, from the clip's body_positions; the synthetic line gets the forward "
                    "kinematics of its own poses")
    ap.add_argument("--end-effector-ids", type=int, nargs="+", default=None, metavar="ID", help="with --track-bodies: body ids of the end effectors, "
                    "which get a sharper term of their own (Rodent(end_effector_ids=...)).  The model blobs hold no body names: on "
                    "rodent_optimized / rodent_0 foot_L, foot_R, hand_L, hand_R, skull are 11 15 59 64 54, on rodent_new each is one higher")
    ap.add_argument("--clip-restarts", type=int, default=0, metavar="K", help="with --track-pose: a restarted episode rejoins its clip "
                    "(Rodent(clip_restarts=K), 1 .. 64): each env keeps K start states drawn at reset and takes the next one -- state, "
                    "observation AND frame -- at every restart.  0, the default: the first state comes back and the frame runs on, as upstream")
    ap.add_argument("--restart-frames", type=int, nargs=2, default=None, metavar=("LO", "HI"), help="with --clip-restarts K > 1: start frames of "
                    "the K - 1 further start states are drawn in [LO, HI) (default 0 100, the reference's range)")
    ap.add_argument("--end-at-clip-end", action="store_true", help="with --clip-restarts: truncate an episode at the clip's last frame instead "
                    "of comparing it with the clamped last row (the clip must be longer than every start frame: the synthetic line has 250 frames)")
    ap.add_argument("--restart-across-clips", action="store_true", help="with --clip-restarts and several clips: every start state of the bank has a "
                    "clip of its own, so a restarted episode may move to another clip (Rodent(restart_across_clips=True))")
    ap.add_argument("--restart-from-reference", action="store_true", help="with --clip-restarts K >= 1 (1 suffices): a restarted episode starts from a "
                    "freshly drawn clip and frame -- the clip's pose (and velocities) plus noise -- instead of one of its K stored start states, "
                    "so a run starts episodes all over the library (Rodent(reset_to_reference=True, restart_from_reference=True))")
    ap.add_argument("--restart-noise-seed", type=int, default=0, metavar="S", help="with --restart-from-reference: the seed of its draws")
    ap.add_argument("--clip-outcomes", action="store_true", help="with --clip-restarts and several clips: count per clip the wrapped steps, the ended "
                    "episodes and why they ended (Rodent(clip_outcomes=True)); reported as training/clip_fail_rate, training/clip_truncated_share "
                    "and, up to 16 clips, training/clip_fail_rate_clip{c}")
    ap.add_argument("--weighted-restarts", action="store_true", help="with --restart-across-clips: a restarted episode draws its start state with "
                    "probability proportional to its clip's weight, and the weights follow the clips' failure rates "
                    "(Rodent(restart_sampling='weighted'), ppo.train(clip_weight_fn=FailureWeights(...)); implies --clip-outcomes)")
    ap.add_argument("--weight-floor", type=float, default=0.1, metavar="F", help="with --weighted-restarts: the weight of a clip that never fails, "
                    "relative to one that always does (FailureWeights(floor=F); untuned default)")
    ap.add_argument("--weight-decay", type=float, default=0.9, metavar="D", help="with --weighted-restarts: the decay per training step of the "
                    "failure and episode counts the rates are formed from (FailureWeights(decay=D); untuned default)")
    ap.add_argument("--clip-lengths", type=int, nargs="+", default=None, metavar="L", help="with --track-pose and --synthetic-clips K: the frames of each "
                    "synthetic line, K ints in 2 .. 250 (Rodent(clip_lengths=...)): rewards, observation and --end-at-clip-end stop at the clip's own "
                    "last frame.  Clips of unequal length in a --clip file get theirs from the file (preprocessing.load_reference_clips)")
    ap.add_argument("--track-velocity", action="store_true", help="with --track-pose: reward the clip's velocities too (Rodent(track_velocity=..., "
                    "track_angular_velocity=..., track_joint_velocity=...), untuned default weights), and with them a reset to the reference starts "
                    "moving: the clip file's velocity, angular_velocity and joints_velocity; the synthetic lines get "
                    "preprocessing.compute_velocity_from_kinematics of their own poses")
    ap.add_argument("--lin-vel-scale", type=float, default=10.0, metavar="K", help="with --track-velocity: Rodent(lin_vel_reward_scale=K)")
    ap.add_argument("--ang-vel-scale", type=float, default=0.1, metavar="K", help="with --track-velocity: Rodent(ang_vel_reward_scale=K)")
    ap.add_argument("--joint-vel-scale", type=float, default=0.01, metavar="K", help="with --track-velocity: Rodent(joint_vel_reward_scale=K)")
    ap.add_argument("--policy-width", type=int, choices=(32, 256), default=32, help="units per hidden layer of the policy network; both "
                    "widths run on the hand-written learner kernels (256: per-step rollouts, the in-kernel actor is 32-wide)")
    ap.add_argument("--policy-depth", type=int, default=4, help="hidden layers of the policy network (1 .. 7 for the hand-written kernels; "
                    "the one-launch rollout of the 32-wide policy takes 1 .. 4)")
    ap.add_argument("--max-grad-norm", type=float, default=None, metavar="X", help="clip every minibatch gradient to global norm X before Adam and "
                    "skip updates whose gradient is not finite (ppo.train(max_grad_norm=X); inf: only the skip); default: no clipping")
    ap.add_argument("--learner-diagnostics", action="store_true", help="report training/approx_kl, approx_kl_max, clip_fraction, "
                    "explained_variance and entropy, means over all minibatches of a training step (ppo.train(learner_diagnostics=True))")
    ap.add_argument("--target-kl", type=float, default=None, metavar="X", help="stop a training step's updates once a minibatch's approx_kl "
                    "exceeds 1.5 X, the rule of Spinning Up / Stable-Baselines3 (ppo.train(target_kl=X)); default: no stop")
    ap.add_argument("--lr-schedule", choices=("adaptive_kl",), default=None, help="adaptive_kl: rsl_rl's KL-adaptive learning rate "
                    "(ppo.train(learning_rate_schedule='adaptive_kl')); default: constant")
    ap.add_argument("--desired-kl", type=float, default=None, metavar="X", help="with --lr-schedule adaptive_kl: the KL the schedule steers "
                    f"to (default {optim.DESIRED_KL_DEFAULT:g}: rsl_rl's, untuned here)")
    ap.add_argument("--lr-bounds", type=float, nargs=2, default=None, metavar=("LO", "HI"), help="with --lr-schedule adaptive_kl: the learning "
                    "rate stays inside [LO, HI] (default %g %g: rsl_rl's, untuned here)" % optim.LR_BOUNDS_DEFAULT)
    args = ap.parse_args()
    if args.max_grad_norm is not None and not args.max_grad_norm > 0:
        ap.error("--max-grad-norm: a number > 0 (inf allowed)")
    if args.target_kl is not None and not 0 < args.target_kl < float("inf"):
        ap.error("--target-kl: a finite number > 0")
    if args.lr_schedule is None and (args.desired_kl is not None or args.lr_bounds is not None):
        ap.error("--desired-kl / --lr-bounds: only with --lr-schedule adaptive_kl")
    if args.track_velocity and not args.track_pose:      # (before any device is touched)
        ap.error("--track-velocity: the velocities are indexed like the reference pose; add --track-pose")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    if world > 1:
        torch.distributed.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    n_gpus = world
    config = {
        "env_name": "rodent", "algo_name": "ppo", "task_name": "run", "num_envs": args.envs_per_gpu * n_gpus,
        "num_timesteps": args.num_timesteps, "eval_every": args.eval_every, "episode_length": 150,
        "batch_size": args.envs_per_gpu * n_gpus, "learning_rate": 5e-5, "terminate_when_unhealthy": True,
        "solver": "cg", "iterations": 8, "ls_iterations": 8, "vision": False,
    }
    if args.track_pose and args.randomize:
        ap.error("--track-pose: the step kernel's pose instances read no per-env parameters; drop --randomize")
    if args.reference_frames and not args.track_pose:
        ap.error("--reference-frames: the frames are rows of the reference pose; add --track-pose")
    for flag in ("max_pos_error", "max_quat_error", "max_joint_error"):
        if getattr(args, flag) is not None and not args.track_pose:
            ap.error(f"--{flag.replace('_', '-')}: the errors are taken against the reference pose; add --track-pose")
        if getattr(args, flag) is not None and not getattr(args, flag) > 0:
            ap.error(f"--{flag.replace('_', '-')}: must be > 0")
    if args.track_bodies and not args.track_pose:
        ap.error("--track-bodies: the body positions are indexed like the reference pose; add --track-pose")
    if args.end_effector_ids is not None and not args.track_bodies:
        ap.error("--end-effector-ids: the end effectors are bodies of the clip; add --track-bodies")
    if (args.clip_restarts or args.restart_frames is not None or args.end_at_clip_end) and not args.track_pose:
        ap.error("--clip-restarts / --restart-frames / --end-at-clip-end: the restarted env rejoins the reference pose; add --track-pose")
    if not 0 <= args.clip_restarts <= 64:
        ap.error("--clip-restarts: 0 .. 64")
    if args.end_at_clip_end and args.clip_restarts < 1:
        ap.error("--end-at-clip-end: needs --clip-restarts K >= 1")
    if not 0 <= args.reference_frames <= 16:
        ap.error("--reference-frames: 0 .. 16")
    if (args.restart_across_clips or args.clip_lengths is not None) and not args.track_pose:
        ap.error("--restart-across-clips / --clip-lengths: they serve envs that track the reference pose; add --track-pose")
    if args.restart_across_clips and args.clip_restarts < 1:
        ap.error("--restart-across-clips: needs --clip-restarts K >= 1")
    if args.weighted_restarts and not args.restart_across_clips:
        ap.error("--weighted-restarts: needs --restart-across-clips (the weights are those of the bank entries' clips)")
    if args.clip_outcomes and args.clip_restarts < 1:
        ap.error("--clip-outcomes: needs --clip-restarts K >= 1")
    if args.restart_from_reference and args.clip_restarts < 1:
        ap.error("--restart-from-reference: needs --clip-restarts K >= 1 (and with it --track-pose)")
    clip_lengths = args.clip_lengths
    clips = None                                     # the loaded ReferenceClip(s), [C, T, ...] fields; None for a .npy track or the synthetic line
    if args.clip and os.path.exists(args.clip) and not args.clip.endswith(".npy"):
        try:
            clips = preprocessing.load_reference_clip(args.clip, args.clip_name)
        except ValueError:                            # clips of unequal length: padded to the longest, each keeps its own length
            if not args.track_pose:
                raise
            clips, clip_lengths = preprocessing.load_reference_clips(args.clip, args.clip_name)
        position = np.asarray(clips.position)         # reference_clip.position [REF :84], [C, T, 3]
        track_pos = position[0] if len(args.clip_name) == 1 else position
    elif args.clip and os.path.exists(args.clip):
        track_pos = np.load(args.clip)
    else:   # the reference clip (clips/84.p) is not distributed: straight line at 0.2 m/s, torso rest height
        t = np.arange(250)
        track_pos = np.stack([0.004 * t, np.zeros(250), np.full(250, 0.0681)], axis=1)
        if args.synthetic_clips > 1:    # K lines from the same start, headings spread over +-45 degrees
            heading = np.linspace(-np.pi / 4, np.pi / 4, args.synthetic_clips)
            track_pos = np.stack([np.stack([0.004 * t * np.cos(h), 0.004 * t * np.sin(h), np.full(250, 0.0681)], axis=1) for h in heading])

    pose = {}
    if args.track_pose:
        if clips is not None:                        # the clip's own orientation and joint angles, the clip axis as track_pos has it
            quat, joints = np.asarray(clips.quaternion), np.asarray(clips.joints)
            pose = dict(track_quat=quat[0] if track_pos.ndim == 2 else quat, track_joints=joints[0] if track_pos.ndim == 2 else joints)
        else:                                        # no pose in the file: upright, the model's rest joint angles
            rest = np.asarray(mjcf.load_blob(assets.resolve_model(args.xml))["qpos0"], np.float64)[7:]
            lead = track_pos.shape[:-1]
            pose = dict(track_quat=np.broadcast_to([1.0, 0.0, 0.0, 0.0], lead + (4,)), track_joints=np.broadcast_to(rest, lead + rest.shape))

    if args.track_bodies:
        if clips is not None:
            bodies = np.asarray(clips.body_positions)
            bodies = bodies[0] if track_pos.ndim == 2 else bodies
        else:                                        # the synthetic line: forward kinematics of (track position, upright, rest joints) per frame
            probe = envs.Rodent(track_pos=track_pos, num_envs=1, xml_path=args.xml, device=f"cuda:{local_rank}")
            lead = track_pos.shape[:-1]
            qpos = np.concatenate([track_pos, pose["track_quat"], pose["track_joints"]], axis=-1).reshape(-1, probe.sys.nq)
            bodies = preprocessing.extract_features(probe, qpos).body_positions
            bodies = bodies.reshape(lead + bodies.shape[1:])
        pose.update(track_bodies=bodies, end_effector_ids=args.end_effector_ids)

    if args.track_velocity:
        single = track_pos.ndim == 2
        if clips is not None and clips.velocity is not None:      # the clip's own velocities, the clip axis as track_pos has it
            vel = [np.asarray(a) for a in (clips.velocity, clips.angular_velocity, clips.joints_velocity)]
            vel = [a[0] if single else a for a in vel]
        else:                                        # finite differences of the poses the env tracks, as preprocessing.process_clip forms them
            lead = track_pos.shape[:-1]              # (the last frame is repeated, so the last row is zero); dt 0.02: the env's control step
            qpos = np.concatenate([track_pos, np.broadcast_to(pose["track_quat"], lead + (4,)), pose["track_joints"]], axis=-1)
            qpos = qpos[None] if single else qpos
            qvel = np.stack([preprocessing.compute_velocity_from_kinematics(np.concatenate([q, q[-1:]], axis=0), 0.02) for q in qpos])
            qvel = qvel[0] if single else qvel
            vel = [qvel[..., :3], qvel[..., 3:6], qvel[..., 6:]]
        pose.update(track_velocity=vel[0], track_angular_velocity=vel[1], track_joint_velocity=vel[2], lin_vel_reward_scale=args.lin_vel_scale,
                    ang_vel_reward_scale=args.ang_vel_scale, joint_vel_reward_scale=args.joint_vel_scale)

    envs.register_environment("rodent", envs.Rodent)
    env = envs.get_environment(
        config["env_name"], track_pos=track_pos, terminate_when_unhealthy=config["terminate_when_unhealthy"],
        solver=config["solver"], iterations=config["iterations"], ls_iterations=config["ls_iterations"],
        vision=config["vision"], num_envs=args.envs_per_gpu, xml_path=args.xml, device=f"cuda:{local_rank}",
        bad_state_max=args.bad_state_max, reference_obs_frames=args.reference_frames, max_pos_error=args.max_pos_error,
        max_quat_error=args.max_quat_error, max_joint_error=args.max_joint_error, clip_restarts=args.clip_restarts,
        restart_frame_range=None if args.restart_frames is None else tuple(args.restart_frames), end_at_clip_end=args.end_at_clip_end,
        clip_lengths=None if clip_lengths is None else np.asarray(clip_lengths, dtype=np.int32), restart_across_clips=args.restart_across_clips,
        restart_sampling="weighted" if args.weighted_restarts else None, clip_outcomes=args.clip_outcomes or args.weighted_restarts,
        reset_to_reference=args.restart_from_reference, restart_from_reference=args.restart_from_reference, restart_noise_seed=args.restart_noise_seed,
        **pose)     # a clip too short for --end-at-clip-end is refused here with the reason (ValueError)

    train_fn = functools.partial(
        ppo.train, num_timesteps=config["num_timesteps"], num_evals=int(config["num_timesteps"] / config["eval_every"]),
        reward_scaling=1, episode_length=config["episode_length"], normalize_observations=True, action_repeat=1,
        unroll_length=10, num_minibatches=64, num_updates_per_batch=8, discounting=0.97,
        learning_rate=config["learning_rate"], entropy_cost=1e-3, num_envs=config["num_envs"],
        batch_size=config["batch_size"], seed=0, max_training_steps=args.max_training_steps,
        randomization_fn=domain_randomize if args.randomize else None,
        max_grad_norm=args.max_grad_norm,
        learner_diagnostics=args.learner_diagnostics, target_kl=args.target_kl, learning_rate_schedule=args.lr_schedule,
        desired_kl=optim.DESIRED_KL_DEFAULT if args.desired_kl is None else args.desired_kl,
        learning_rate_bounds=optim.LR_BOUNDS_DEFAULT if args.lr_bounds is None else tuple(args.lr_bounds),
        clip_weight_fn=envs.rodent.FailureWeights(floor=args.weight_floor, decay=args.weight_decay) if args.weighted_restarts else None,
        network_factory=functools.partial(networks.make_ppo_networks, policy_hidden_layer_sizes=(args.policy_width,) * args.policy_depth))

    run_id = uuid.uuid4()
    model_path = f"./model_checkpoints/{run_id}"

    def progress(num_steps, metrics):
        metrics["num_steps"] = num_steps
        print(json.dumps({k: (float(v) if np.isscalar(v) else v) for k, v in metrics.items()}), flush=True)

    eval_env = env.with_num_envs(1)                  # the launcher's un-vmapped jit_reset / jit_step pair [REF :93-94]
    track0 = track_pos if track_pos.ndim == 2 else track_pos[0]       # the evaluation rollout follows clip 0
    if clips is not None:                            # the real clip: its own orientation and joints next to the rollout's
        ref_clip = preprocessing.ReferenceClip(position=track0, quaternion=np.asarray(clips.quaternion)[0], joints=np.asarray(clips.joints)[0])
    else:                                            # a bare track: dummies, only to pair the rollout with the positions
        ref_clip = preprocessing.ReferenceClip(position=track0, quaternion=np.tile([1.0, 0, 0, 0], (len(track0), 1)),
                                               joints=np.zeros((len(track0), env.sys.nq - 7)))

    def policy_params_fn(num_steps, make_policy, params, model_path=model_path):
        """Checkpoint + the 500-step evaluation rollout paired with the reference clip [REF brax_rodent_run_ppo.py:135-191];
        the qpos pairs are saved instead of rendered (mujoco.Renderer / wandb are out of scope)."""
        os.makedirs(model_path, exist_ok=True)
        model.save_params(f"{model_path}/{num_steps}", params)
        net = params[1]                                  # the snapshot network in the in-kernel actor's layout: RR_FUSED_EVAL=1 makes the rollout one launch
        actor = acting.actor_params(net, params[0], 0.001) if isinstance(net, torch.nn.Module) and acting.actor_shape_supported(net, eval_env.action_size) else None
        qposes = rollout.eval_rollout(eval_env, make_policy, params, steps=500, seed=0, actor=actor, clip=0)
        rollout.save_rollout(f"{model_path}/{num_steps}_rollout.npz", rollout.qpos_pairs(ref_clip, qposes), eval_env.dt, qposes)

    make_inference_fn, params, _ = train_fn(environment=env, progress_fn=progress, policy_params_fn=policy_params_fn)
    if int(os.environ.get("RANK", "0")) == 0:
        os.makedirs(model_path, exist_ok=True)
        model.save_params(f"{model_path}/brax_ppo_rodent_run_finished", params)
        print(f"Run finished. Model saved to {model_path}/brax_ppo_rodent_run_finished")
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
