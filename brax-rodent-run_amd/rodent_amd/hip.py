"""ctypes binding of librodent_hip.so (C ABI: include/rodent_rr.h).

PyTorch is used only for device memory and streams: every tensor handed to the library is a
contiguous float32 / int32 CUDA(HIP) tensor whose `data_ptr()` crosses the ABI.  There is no CPU
fallback: if the shared library is missing or no GPU is present the calls raise.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Dict, Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RR_LIB") or os.path.join(os.path.dirname(_HERE), "csrc", "librodent_hip.so")


class RRDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("nq", "nv", "nu", "na", "nbody", "njnt", "ngeom", "nM", "ncon", "nlimit",
                                         "nefc", "obs_dim", "iterations", "ls_iterations", "lds_bytes", "dbg_floats")] \
        + [("timestep", C.c_float), ("solver", C.c_int32), ("fixed_instance", C.c_int32)]


class RRState(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("qpos", "qvel", "act", "qacc_warmstart")]


class RROutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("cinert", "cvel", "qfrc_actuator", "xpos", "xmat", "subtree_com", "debug",
                                                "contact_dist", "contact_pos", "contact_frame")]


class RRMlpNet(C.Structure):
    _fields_ = [("weights", C.POINTER(C.c_void_p)), ("biases", C.POINTER(C.c_void_p)), ("sizes", C.POINTER(C.c_int32)), ("nlayers", C.c_int32)]


class RREnvIO(C.Structure):
    _fields_ = [("track_pos", C.c_void_p), ("track_len", C.c_int32), ("cur_frame", C.c_void_p), ("obs", C.c_void_p),
                ("reward", C.c_void_p), ("done", C.c_void_p), ("metrics", C.c_void_p), ("healthy_reward", C.c_float),
                ("ctrl_cost_weight", C.c_float), ("healthy_z_min", C.c_float), ("healthy_z_max", C.c_float),
                ("terminate_when_unhealthy", C.c_int32), ("bad_state_max", C.c_float)]


class RREnvIOClips(C.Structure):
    """The whole `rr_env_io`, and what every env call passes: the 80 bytes of `RREnvIO` (the single-clip members, kept as they were) followed
    by the two multi-clip members.  All zero behind `bad_state_max` is the single-clip path."""
    _fields_ = RREnvIO._fields_ + [("clip", C.c_void_p), ("num_clips", C.c_int32)]


class RRPoseIO(C.Structure):
    """`rr_pose_io`, the pose-tracking block a batch carries (`rr_batch_set_pose`); all zero is the position-only reward."""
    _fields_ = [("track_pose", C.c_void_p), ("pose_metrics", C.c_void_p), ("quat_reward_weight", C.c_float), ("quat_reward_scale", C.c_float),
                ("joint_reward_weight", C.c_float), ("joint_reward_scale", C.c_float)]


class RRPoseTermIO(C.Structure):
    """`rr_pose_term_io`, the pose-termination block a batch carries next to its pose block (`rr_batch_set_pose_termination`)."""
    _fields_ = [("fail", C.c_void_p), ("max_pos", C.c_float), ("max_quat", C.c_float), ("max_joint", C.c_float), ("pad", C.c_int32)]


class RRBodyIO(C.Structure):
    """`rr_body_io`, the body-tracking block a batch carries next to its pose block (`rr_batch_set_body_tracking`)."""
    _fields_ = [("track_bodies", C.c_void_p), ("body_weights", C.c_void_p), ("body_metrics", C.c_void_p),
                ("body_reward_weight", C.c_float), ("body_reward_scale", C.c_float),
                ("endeff_reward_weight", C.c_float), ("endeff_reward_scale", C.c_float)]


class RRClipRestartIO(C.Structure):
    """`rr_clip_restart_io`, the clip-restart block a batch carries next to its pose block (`rr_batch_set_clip_restarts`)."""
    _fields_ = [("frames", C.c_void_p), ("slot_in", C.c_void_p), ("slot_out", C.c_void_p), ("num_slots", C.c_int32), ("end_at_clip_end", C.c_int32)]


class RRVelIO(C.Structure):
    """`rr_vel_io`, the velocity-tracking block a batch carries next to its pose block (`rr_batch_set_velocity_tracking`)."""
    _fields_ = [("track_vel", C.c_void_p), ("vel_metrics", C.c_void_p), ("lin_weight", C.c_float), ("lin_scale", C.c_float),
                ("ang_weight", C.c_float), ("ang_scale", C.c_float), ("joint_weight", C.c_float), ("joint_scale", C.c_float)]


class RRClipLibraryIO(C.Structure):
    """`rr_clip_library_io`, the clip-library block a batch carries next to its pose block (`rr_batch_set_clip_library`)."""
    _fields_ = [("clip_lengths", C.c_void_p), ("bank_clips", C.c_void_p), ("clip_out", C.c_void_p)]


class RRClipSamplingIO(C.Structure):
    """`rr_clip_sampling_io`, the clip-sampling block a batch carries next to its clip-restart block (`rr_batch_set_clip_sampling`)."""
    _fields_ = [("clip_weights", C.c_void_p), ("draws_in", C.c_void_p), ("draws_out", C.c_void_p), ("outcomes", C.c_void_p), ("seed", C.c_uint32)]


class RRReferenceRestartIO(C.Structure):
    """`rr_reference_restart_io`, the reference-restart block a batch carries next to its clip-restart block (`rr_batch_set_reference_restart`)."""
    _fields_ = [("clip_weights", C.c_void_p), ("draws_in", C.c_void_p), ("draws_out", C.c_void_p), ("seed", C.c_uint32), ("frame_lo", C.c_int32),
                ("frame_hi", C.c_int32), ("across_clips", C.c_int32), ("noise_scale", C.c_float), ("pad", C.c_int32)]


class RRUnrollIO(C.Structure):
    _fields_ = [("first", RRState), ("first_obs", C.c_void_p), ("prev_done", C.c_void_p), ("steps_in", C.c_void_p), ("steps_out", C.c_void_p),
                ("truncation_out", C.c_void_p), ("episode_length", C.c_float)]


class RRActorIO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("obs_in", "mean", "std", "w0", "b0")] + [("hidden_wt", C.c_void_p * 4), ("hidden_b", C.c_void_p * 4)] + \
        [(n, C.c_void_p) for n in ("head_wt", "head_b", "noise", "actions_out", "traj_obs", "traj_raw_action", "traj_log_prob", "traj_reward",
                                   "traj_discount", "traj_truncation")] + [("min_std", C.c_float), ("nhidden", C.c_int32), ("segment_length", C.c_int32)]


class RREvalIO(C.Structure):
    _fields_ = [("eval_metrics", C.c_void_p), ("obs_ring", C.c_void_p), ("qpos_out", C.c_void_p), ("raw_env", C.c_int32)]


class RREnvParams(C.Structure):
    _fields_ = [("dof_f", C.c_void_p), ("act_f", C.c_void_p), ("con_f", C.c_void_p), ("dof_rows", C.c_int32), ("act_rows", C.c_int32),
                ("con_rows", C.c_int32), ("num_envs", C.c_int32)]


class RRDwItem(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("delta", "act", "act_rows", "mean", "std", "delta_colsum")] + \
        [("M", C.c_int32), ("O", C.c_int32), ("I", C.c_int32), ("grad", C.c_void_p)]


class RRAdamTensor(C.Structure):
    _fields_ = [("param", C.c_void_p), ("offset", C.c_int64), ("numel", C.c_int64)]


class RRPpoCfg(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("entropy_cost", "discounting", "reward_scaling", "gae_lambda", "clipping_epsilon", "min_std")] + \
        [("normalize_advantage", C.c_int32)]


EXPORTS = ["rr_model_load", "rr_model_dims", "rr_model_set_solver", "rr_model_set_solver_type", "rr_model_destroy", "rr_model_table", "rr_kernarg_layout", "rr_batch_create",
           "rr_batch_destroy", "rr_pipeline_init", "rr_pipeline_step", "rr_env_step", "rr_env_reset", "rr_pipeline_step_to", "rr_env_step_to", "rr_batch_contact_overflow", "rr_batch_bad_states", "rr_batch_unroll_supported", "rr_env_unroll", "rr_env_unroll_policy", "rr_batch_eval_supported", "rr_env_unroll_eval", "rr_batch_pose_supported", "rr_batch_set_pose", "rr_batch_set_reference_obs", "rr_batch_obs_width", "rr_batch_reference_obs_supported", "rr_batch_set_pose_termination", "rr_batch_pose_termination_supported", "rr_batch_set_body_tracking", "rr_batch_body_tracking_supported", "rr_batch_set_clip_restarts", "rr_batch_clip_restarts_supported", "rr_batch_set_velocity_tracking", "rr_batch_velocity_tracking_supported", "rr_batch_set_clip_library", "rr_batch_clip_library_supported", "rr_batch_set_clip_sampling", "rr_batch_clip_sampling_supported", "rr_batch_set_reference_restart", "rr_batch_reference_restart_supported", "rr_wrap_clip_restart", "rr_wrap_clip_library", "rr_wrap_clip_sampling",
           "rr_compute_gae", "rr_mlp_forward", "rr_ppo_loss_workspace_bytes", "rr_ppo_loss", "rr_ppo_loss_diag_workspace_bytes", "rr_ppo_loss_diag", "rr_policy_act_workspace_bytes", "rr_policy_act", "rr_policy_sample", "rr_policy_backward_workspace_bytes", "rr_policy_backward", "rr_mlp_silu_backward_workspace_bytes", "rr_mlp_silu_backward", "rr_mlp_value_backward_workspace_bytes", "rr_mlp_policy_backward", "rr_mlp_policy_backward_workspace_bytes", "rr_mlp_value_backward", "rr_mlp_weight_grad_workspace_bytes", "rr_mlp_weight_grad", "rr_mlp_weight_grad_batch_workspace_bytes", "rr_mlp_weight_grad_batch", "rr_obs_moments_workspace_bytes", "rr_obs_moments", "rr_clipped_adam_workspace_bytes", "rr_clipped_adam_partials", "rr_clipped_adam_step", "rr_clipped_adam_step_kl", "rr_wrap_episode_autoreset", "rr_debug_layout", "rr_batch_set_schedule", "rr_batch_set_env_params", "rr_batch_env_params_supported", "rr_batch_set_profile", "rr_batch_set_ls_repeat_exit", "rr_batch_set_solver_trim", "rr_batch_set_solver_batch", "rr_batch_set_solve_resident", "rr_model_solve_resident_switch", "rr_batch_set_root_slot", "rr_model_root_slot_switch", "rr_batch_set_timing", "rr_batch_kernel_time", "rr_last_error"]

_lib = None


def lib():
    """Load librodent_hip.so (fails loudly when it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(LIB_PATH)
        L.rr_last_error.restype = C.c_char_p
        L.rr_model_load.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        L.rr_model_dims.argtypes = [C.c_void_p, C.POINTER(RRDims)]
        L.rr_model_set_solver.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        L.rr_model_set_solver_type.argtypes = [C.c_void_p, C.c_int32]
        L.rr_model_destroy.argtypes = [C.c_void_p]
        L.rr_model_destroy.restype = None
        L.rr_model_table.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]
        L.rr_kernarg_layout.argtypes = [C.POINTER(C.c_int32)] * 3
        L.rr_batch_create.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]
        L.rr_batch_destroy.argtypes = [C.c_void_p]
        L.rr_batch_destroy.restype = None
        L.rr_pipeline_init.argtypes = [C.c_void_p, C.POINTER(RRState), C.POINTER(RROutputs)]
        L.rr_pipeline_step.argtypes = [C.c_void_p, C.POINTER(RRState), C.c_void_p, C.c_int32, C.POINTER(RROutputs)]
        L.rr_env_step.argtypes = [C.c_void_p, C.POINTER(RRState), C.c_void_p, C.c_int32, C.POINTER(RREnvIOClips),
                                  C.POINTER(RROutputs)]
        L.rr_pipeline_step_to.argtypes = [C.c_void_p, C.POINTER(RRState), C.POINTER(RRState), C.c_void_p, C.c_int32, C.POINTER(RROutputs)]
        L.rr_env_step_to.argtypes = [C.c_void_p, C.POINTER(RRState), C.POINTER(RRState), C.c_void_p, C.c_int32, C.POINTER(RREnvIOClips),
                                     C.c_void_p, C.POINTER(RROutputs)]
        L.rr_batch_unroll_supported.argtypes = [C.c_void_p, C.c_int32]
        L.rr_batch_contact_overflow.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.rr_batch_bad_states.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.rr_env_unroll.argtypes = [C.c_void_p, C.POINTER(RRState), C.POINTER(RRState), C.c_void_p, C.c_int32, C.c_int32, C.POINTER(RREnvIOClips),
                                    C.c_void_p, C.POINTER(RRUnrollIO)]
        L.rr_env_unroll_policy.argtypes = [C.c_void_p, C.POINTER(RRState), C.POINTER(RRState), C.c_int32, C.c_int32, C.POINTER(RREnvIOClips), C.c_void_p,
                                           C.POINTER(RRUnrollIO), C.POINTER(RRActorIO)]
        L.rr_batch_eval_supported.argtypes = [C.c_void_p]
        L.rr_env_unroll_eval.argtypes = [C.c_void_p, C.POINTER(RRState), C.POINTER(RRState), C.c_int32, C.c_int32, C.POINTER(RREnvIOClips), C.c_void_p,
                                         C.POINTER(RRUnrollIO), C.POINTER(RRActorIO), C.POINTER(RREvalIO)]
        L.rr_env_reset.argtypes = [C.c_void_p, C.POINTER(RRState), C.POINTER(RREnvIOClips), C.POINTER(RROutputs)]
        L.rr_debug_layout.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_char_p)), C.POINTER(C.POINTER(C.c_int32)),
                                      C.POINTER(C.POINTER(C.c_int32))]
        L.rr_compute_gae.argtypes = [C.c_void_p] * 5 + [C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rr_mlp_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(RRMlpNet), C.POINTER(RRMlpNet),
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rr_ppo_loss_workspace_bytes.argtypes = [C.c_int32, C.c_int32]
        L.rr_ppo_loss_workspace_bytes.restype = C.c_size_t
        L.rr_ppo_loss.argtypes = [C.c_void_p] * 9 + [C.c_int32] * 3 + [C.POINTER(RRPpoCfg)] + [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]
        L.rr_ppo_loss_diag_workspace_bytes.argtypes = [C.c_int32, C.c_int32]
        L.rr_ppo_loss_diag_workspace_bytes.restype = C.c_size_t
        L.rr_ppo_loss_diag.argtypes = [C.c_void_p] * 9 + [C.c_int32] * 3 + [C.POINTER(RRPpoCfg)] + [C.c_void_p] * 6 + [C.c_size_t, C.c_void_p]
        L.rr_policy_act_workspace_bytes.argtypes = [C.c_int32]
        L.rr_policy_act_workspace_bytes.restype = C.c_size_t
        L.rr_policy_act.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(RRMlpNet), C.c_void_p, C.c_float,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.rr_policy_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rr_policy_backward_workspace_bytes.argtypes = [C.c_int32, C.c_int32]
        L.rr_policy_backward_workspace_bytes.restype = C.c_size_t
        L.rr_policy_backward.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                         C.POINTER(C.c_void_p), C.c_void_p, C.c_size_t, C.c_void_p]
        L.rr_mlp_silu_backward_workspace_bytes.argtypes = [C.c_int32, C.c_int32]
        L.rr_mlp_silu_backward_workspace_bytes.restype = C.c_size_t
        L.rr_mlp_silu_backward.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.rr_mlp_value_backward_workspace_bytes.argtypes = [C.c_int32, C.c_int32]
        L.rr_mlp_value_backward_workspace_bytes.restype = C.c_size_t
        L.rr_mlp_value_backward.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                            C.POINTER(C.c_void_p), C.c_void_p, C.c_size_t, C.c_void_p]
        L.rr_mlp_policy_backward_workspace_bytes.argtypes = [C.c_int32, C.c_int32]
        L.rr_mlp_policy_backward_workspace_bytes.restype = C.c_size_t
        L.rr_mlp_policy_backward.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                             C.POINTER(C.c_void_p), C.c_void_p, C.c_size_t, C.c_void_p]
        L.rr_mlp_weight_grad_workspace_bytes.argtypes = [C.c_int32] * 3
        L.rr_mlp_weight_grad_workspace_bytes.restype = C.c_size_t
        L.rr_mlp_weight_grad.argtypes = [C.c_void_p] * 6 + [C.c_int32] * 3 + [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.rr_mlp_weight_grad_batch_workspace_bytes.argtypes = [C.POINTER(RRDwItem), C.c_int32]
        L.rr_mlp_weight_grad_batch_workspace_bytes.restype = C.c_size_t
        L.rr_mlp_weight_grad_batch.argtypes = [C.POINTER(RRDwItem), C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]
        L.rr_wrap_episode_autoreset.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int32)] + \
            [C.c_void_p] * 5 + [C.c_float, C.c_float, C.c_void_p]
        L.rr_obs_moments_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int32]
        L.rr_obs_moments_workspace_bytes.restype = C.c_size_t
        L.rr_obs_moments.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.rr_clipped_adam_workspace_bytes.argtypes = [C.c_int64]
        L.rr_clipped_adam_workspace_bytes.restype = C.c_size_t
        L.rr_clipped_adam_partials.argtypes = [C.c_int64]
        L.rr_clipped_adam_step.argtypes = [C.POINTER(RRAdamTensor), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p]
        L.rr_clipped_adam_step_kl.argtypes = [C.POINTER(RRAdamTensor), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 6
        L.rr_batch_set_profile.argtypes = [C.c_void_p, C.c_void_p]
        L.rr_batch_set_schedule.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rr_batch_set_env_params.argtypes = [C.c_void_p, C.POINTER(RREnvParams)]
        L.rr_batch_env_params_supported.argtypes = [C.c_void_p]
        L.rr_batch_pose_supported.argtypes = [C.c_void_p]
        L.rr_batch_set_pose.argtypes = [C.c_void_p, C.POINTER(RRPoseIO)]
        L.rr_batch_set_reference_obs.argtypes = [C.c_void_p, C.c_int32]
        L.rr_batch_obs_width.argtypes = [C.c_void_p]
        L.rr_batch_obs_width.restype = C.c_int32
        L.rr_batch_reference_obs_supported.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        L.rr_batch_set_pose_termination.argtypes = [C.c_void_p, C.POINTER(RRPoseTermIO)]
        L.rr_batch_pose_termination_supported.argtypes = [C.c_void_p, C.c_int32]
        L.rr_batch_set_body_tracking.argtypes = [C.c_void_p, C.POINTER(RRBodyIO)]
        L.rr_batch_body_tracking_supported.argtypes = [C.c_void_p, C.c_int32]
        L.rr_batch_set_clip_restarts.argtypes = [C.c_void_p, C.POINTER(RRClipRestartIO)]
        L.rr_batch_clip_restarts_supported.argtypes = [C.c_void_p, C.c_int32]
        L.rr_batch_set_velocity_tracking.argtypes = [C.c_void_p, C.POINTER(RRVelIO)]
        L.rr_batch_velocity_tracking_supported.argtypes = [C.c_void_p, C.c_int32]
        L.rr_batch_set_clip_library.argtypes = [C.c_void_p, C.POINTER(RRClipLibraryIO)]
        L.rr_batch_clip_library_supported.argtypes = [C.c_void_p, C.c_int32]
        L.rr_wrap_clip_restart.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int32)] + \
            [C.c_void_p] * 5 + [C.c_float, C.c_float] + [C.c_void_p] * 4 + [C.c_int32] * 3 + [C.c_void_p]
        L.rr_wrap_clip_library.argtypes = L.rr_wrap_clip_restart.argtypes[:-1] + [C.c_void_p] * 4      # ... clip, bank_clips, clip_lengths, stream
        L.rr_batch_set_clip_sampling.argtypes = [C.c_void_p, C.POINTER(RRClipSamplingIO)]
        L.rr_batch_clip_sampling_supported.argtypes = [C.c_void_p, C.c_int32]
        L.rr_batch_set_reference_restart.argtypes = [C.c_void_p, C.POINTER(RRReferenceRestartIO)]
        L.rr_batch_reference_restart_supported.argtypes = [C.c_void_p, C.c_int32]
        # ... clip, bank_clips, clip_lengths, num_clips, pose_fail, sampling, stream
        L.rr_wrap_clip_sampling.argtypes = L.rr_wrap_clip_restart.argtypes[:-1] + [C.c_void_p] * 3 + [C.c_int32, C.c_void_p, C.POINTER(RRClipSamplingIO), C.c_void_p]
        L.rr_batch_set_ls_repeat_exit.argtypes = [C.c_void_p, C.c_int32]
        L.rr_batch_set_solver_trim.argtypes = [C.c_void_p, C.c_int32]
        L.rr_batch_set_solver_batch.argtypes = [C.c_void_p, C.c_int32]
        L.rr_batch_set_solve_resident.argtypes = [C.c_void_p, C.c_int32]
        L.rr_model_solve_resident_switch.argtypes = [C.c_void_p]
        L.rr_batch_set_root_slot.argtypes = [C.c_void_p, C.c_int32]
        L.rr_model_root_slot_switch.argtypes = [C.c_void_p]
        L.rr_batch_set_timing.argtypes = [C.c_void_p, C.c_int32]
        L.rr_batch_kernel_time.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
        _lib = L
    return _lib


def _check(rc):
    if rc < 0:
        raise RuntimeError(f"librodent_hip: {lib().rr_last_error().decode()} (status {rc})")
    return rc


def _ptr(t: Optional[torch.Tensor], dtype=torch.float32, numel: Optional[int] = None):
    if t is None:
        return None
    if not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"expected a contiguous {dtype} device tensor, got {t.dtype} on {t.device}")
    if numel is not None and t.numel() != numel:
        raise ValueError(f"tensor has {t.numel()} elements, expected {numel}")
    return t.data_ptr()


def _dp(t: Optional[torch.Tensor]):
    """data_ptr() of a tensor that has been checked already, None for None."""
    return t.data_ptr() if t is not None else None


def head_columns(P: int) -> int:
    """Columns the in-kernel actor's head of P logits is padded to (`head_cols` in csrc/rr_api.hip): 64 up to 64 logits, 128 above."""
    return 64 if P <= 64 else 128


_scratch: dict = {}


def _ws(bufs: Optional[dict], call: str, dev, shape_key, nbytes: int, dtype=torch.float32, shape=None) -> torch.Tensor:
    """Device buffer of at least `nbytes` (or of `shape`) for `call`, one per (call, device, stream, shape key): scratch of a launch
    must not be shared between streams or devices.  It lives in `bufs` when the caller keeps one (so a captured HIP graph sees the same
    addresses for the life of that object), else in the module's dict, and is never replaced: the address is stable per key."""
    store = _scratch if bufs is None else bufs
    key = (call, dev, torch.cuda.current_stream(dev).cuda_stream, shape_key)
    if key not in store:
        item = dtype.itemsize
        store[key] = torch.empty(shape if shape is not None else ((nbytes + item - 1) // item,), dtype=dtype, device=dev)
    return store[key]


class Model:
    """A compiled model loaded from an RRM1 blob (host side)."""

    def __init__(self, blob_path: str, iterations: Optional[int] = None, ls_iterations: Optional[int] = None, solver: Optional[str] = None):
        self.h = C.c_void_p()
        _check(lib().rr_model_load(blob_path.encode(), C.byref(self.h)))
        if solver is not None:
            _check(lib().rr_model_set_solver_type(self.h, {"cg": 1, "newton": 2}[solver.lower()]))
        if iterations is not None:
            d = self.dims
            _check(lib().rr_model_set_solver(self.h, iterations, ls_iterations if ls_iterations is not None else d.ls_iterations))

    def table(self, name: str):
        """A static table of the LOADED model by its MuJoCo field name (C ABI `rr_model_table`) as a numpy copy."""
        import numpy as np
        ptr, cnt, dt = C.c_void_p(), C.c_size_t(), C.c_int32()
        _check(lib().rr_model_table(self.h, name.encode(), C.byref(ptr), C.byref(cnt), C.byref(dt)))
        ctype = C.c_float if dt.value == 0 else C.c_int32
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(cnt.value,)).copy()

    @property
    def dims(self) -> RRDims:
        d = RRDims()
        _check(lib().rr_model_dims(self.h, C.byref(d)))
        return d

    def check_solve_resident_switch(self):
        """Raise, with the words `Batch.set_solve_resident(False)` would be refused with, unless this model has the instance that
        switch selects (C ABI `rr_model_solve_resident_switch`; needs no device)."""
        _check(lib().rr_model_solve_resident_switch(self.h))

    def check_root_slot_switch(self):
        """Raise, with the words `Batch.set_root_slot(False)` would be refused with, unless this model has the instance that switch
        selects (C ABI `rr_model_root_slot_switch`; needs no device)."""
        _check(lib().rr_model_root_slot_switch(self.h))

    def __del__(self):
        try:
            if self.h:
                lib().rr_model_destroy(self.h)
        except Exception:
            pass


class Batch:
    """`num_envs` environments of one model on one GPU.  All launches go to the stream that was torch's current stream on
    `device` WHEN THE BATCH WAS CREATED (the C ABI binds the stream at rr_batch_create); create the batch inside the
    `torch.cuda.stream(...)` context it should run on."""

    def __init__(self, model: Model, num_envs: int, device: Optional[torch.device] = None):
        if not torch.cuda.is_available():
            raise RuntimeError("rodent_amd.hip.Batch needs a GPU (no CPU fallback)")
        self.model = model
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.N = int(num_envs)
        self.dims = model.dims
        self.h = C.c_void_p()
        self._pose = None           # the tensors of the pose block in force (set_pose)
        self._pterm = None          # the tensor of the pose-termination block in force (set_pose_termination)
        self._body = None           # the tensors of the body-tracking block in force (set_body_tracking)
        self._restart = None        # the tensors of the clip-restart block in force (set_clip_restarts)
        self._vel = None            # the tensors of the velocity-tracking block in force (set_velocity_tracking)
        self._library = None        # the tensors of the clip-library block in force (set_clip_library)
        self._sampling = None       # the tensors of the clip-sampling block in force (set_clip_sampling)
        self._refrestart = None     # the tensors of the reference-restart block in force (set_reference_restart)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream().cuda_stream
        _check(lib().rr_batch_create(model.h, self.N, self.device.index or 0, C.c_void_p(stream), C.byref(self.h)))

    def __del__(self):
        try:
            if self.h:
                lib().rr_batch_destroy(self.h)
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    def zeros_state(self) -> Dict[str, torch.Tensor]:
        d, N, dev = self.dims, self.N, self.device
        return dict(qpos=torch.zeros(N, d.nq, device=dev), qvel=torch.zeros(N, d.nv, device=dev),
                    act=torch.zeros(N, d.na, device=dev), qacc_warmstart=torch.zeros(N, d.nv, device=dev))

    def _state(self, st) -> RRState:
        d, N = self.dims, self.N
        return RRState(_ptr(st["qpos"], numel=N * d.nq), _ptr(st["qvel"], numel=N * d.nv),
                       _ptr(st["act"], numel=N * d.na), _ptr(st["qacc_warmstart"], numel=N * d.nv))

    def _outputs(self, out) -> Optional[RROutputs]:
        if not out:
            return None
        d, N = self.dims, self.N
        sizes = dict(cinert=10 * d.nbody, cvel=6 * d.nbody, qfrc_actuator=d.nv, xpos=3 * d.nbody, xmat=9 * d.nbody,
                     subtree_com=3, debug=d.dbg_floats, contact_dist=d.ncon, contact_pos=3 * d.ncon, contact_frame=9 * d.ncon)
        unknown = set(out) - set(sizes)
        if unknown:
            raise ValueError(f"unknown rr_outputs field(s): {sorted(unknown)}")
        o = RROutputs()
        for k, w in sizes.items():
            setattr(o, k, _ptr(out.get(k), numel=N * w))
        return o

    def _env(self, env) -> RREnvIOClips:
        N = self.N
        tp = env["track_pos"]
        clip = env.get("clip")
        if (clip is not None) != (tp.dim() == 3):
            raise ValueError("env io: `clip` goes with a [C, T, 3] track_pos, and only with one")
        e = RREnvIOClips()
        e.track_pos = _ptr(tp)
        e.track_len = tp.shape[-2]
        if clip is not None:        # multi-clip tracking: env e follows track_pos[clip[e]]
            e.clip = _ptr(clip, torch.int32, N)
            e.num_clips = tp.shape[0]
        e.cur_frame = _ptr(env["cur_frame"], torch.int32, N)
        e.obs = _ptr(env["obs"], numel=N * self.obs_width())
        e.reward = _ptr(env.get("reward"), numel=N)
        e.done = _ptr(env.get("done"), numel=N)
        e.metrics = _ptr(env.get("metrics"), numel=3 * N)
        e.healthy_reward = env.get("healthy_reward", 1.0)
        e.ctrl_cost_weight = env.get("ctrl_cost_weight", 0.1)
        e.healthy_z_min, e.healthy_z_max = env.get("healthy_z_range", (0.03, 0.5))
        e.terminate_when_unhealthy = int(env.get("terminate_when_unhealthy", True))
        e.bad_state_max = float(env.get("bad_state_max") or 0.0)      # 0 = no bad-state check
        self._program_blocks(env)
        return e

    def _program_blocks(self, env):
        """The pose options ride on the batch, not in rr_env_io: the env-io dict decides what the launch about to be issued sees.  One row
        per block -- the env-io key that decides its presence, the attribute that says whether it stands, its setter, the setter's
        arguments out of the dict (the setters say what each entry is) -- in dependency order: termination, body tracking, velocity tracking
        and clip restarts each need the pose block, the clip library (`clip_library` key) the pose block and, for its bank clips, the
        clip-restart block, clip sampling (`clip_sampling` key) the clip-restart block and, for its weights, the library's bank clips,
        reference restarts (`reference_restart` key) the pose and clip-restart blocks,
        and the library keeps a block while one that needs it stands.  So the blocks absent from the
        dict are cleared last to first, then the present ones are set first to last.  (Clearing the pose block is refused while the
        batch carries reference frames: their launches all carry `track_pose`.)"""
        lead, d, inf = tuple(env["track_pos"].shape[:-1]), self.dims, math.inf

        def rows(key, tail):        # the clip's rows of a block: the same clips and frames as track_pos
            if tuple(env[key].shape) != lead + tail:
                raise ValueError(f"env io: {key} has shape {tuple(env[key].shape)}, expected {lead + tail}")
            return env[key]
        blocks = (("track_pose", "_pose", self.set_pose, lambda: (rows("track_pose", (d.nq - 3,)), env.get("pose_metrics"),
                                                                 env.get("quat_reward", (1.0, 2.0)), env.get("joint_reward", (1.0, 0.5)))),
                  ("pose_fail", "_pterm", self.set_pose_termination, lambda: (env["pose_fail"], env.get("pose_termination", (inf, inf, inf)))),
                  ("track_bodies", "_body", self.set_body_tracking, lambda: (rows("track_bodies", (d.nbody, 3)), env.get("body_weights"), env.get("body_metrics"),
                                                                             env.get("body_reward", (1.0, 8.0)), env.get("endeff_reward", (1.0, 100.0)))),
                  ("track_vel", "_vel", self.set_velocity_tracking, lambda: (rows("track_vel", (d.nv,)), env.get("vel_metrics"), env.get("lin_vel_reward", (1.0, 10.0)),
                                                                           env.get("ang_vel_reward", (1.0, 0.1)), env.get("joint_vel_reward", (1.0, 0.01)))),
                  ("restart", "_restart", self.set_clip_restarts, lambda: (env["restart"]["frames"], env["restart"]["slot_in"], env["restart"]["slot_out"],
                                                                           env["restart"].get("end_at_clip_end", False))),
                  ("clip_library", "_library", self.set_clip_library, lambda: (env["clip_library"].get("lengths"), env["clip_library"].get("bank_clips"),
                                                                               env["clip_library"].get("clip_out"), 1 if len(lead) == 1 else lead[0])),
                  ("clip_sampling", "_sampling", self.set_clip_sampling, lambda: (env["clip_sampling"].get("weights"), env["clip_sampling"].get("draws_in"),
                                                                                 env["clip_sampling"].get("draws_out"), env["clip_sampling"].get("outcomes"),
                                                                                 env["clip_sampling"].get("seed", 0), 1 if len(lead) == 1 else lead[0])),
                  ("reference_restart", "_refrestart", self.set_reference_restart, lambda: (env["reference_restart"]["draws_in"], env["reference_restart"]["draws_out"],
                                                                                           env["reference_restart"].get("weights"), env["reference_restart"].get("seed", 0),
                                                                                           env["reference_restart"].get("frame_range", (0, 100)),
                                                                                           env["reference_restart"].get("across_clips", False),
                                                                                           env["reference_restart"].get("noise_scale", 0.0), 1 if len(lead) == 1 else lead[0])))
        for key, attr, setter, _ in reversed(blocks):
            # (the clip library and clip sampling are always set afresh: the bank clips of an earlier launch would keep the restart block
            # from being cleared, the weights the bank clips)
            if (env.get(key) is None or key in ("clip_library", "clip_sampling", "reference_restart")) and getattr(self, attr) is not None:
                setter(None)
        for key, _, setter, args in blocks:
            if env.get(key) is not None:
                setter(*args())

    # ------------------------------------------------------------------ C-ABI calls
    def pipeline_init(self, st, out=None):
        o = self._outputs(out)
        _check(lib().rr_pipeline_init(self.h, C.byref(self._state(st)), C.byref(o) if o else None))

    def pipeline_step(self, st, ctrl, n_frames: int, out=None):
        o = self._outputs(out)
        _check(lib().rr_pipeline_step(self.h, C.byref(self._state(st)), _ptr(ctrl, numel=self.N * self.dims.nu),
                                      int(n_frames), C.byref(o) if o else None))

    def env_step(self, st, action, n_frames: int, env, out=None):
        o = self._outputs(out)
        _check(lib().rr_env_step(self.h, C.byref(self._state(st)), _ptr(action, numel=self.N * self.dims.nu),
                                 int(n_frames), C.byref(self._env(env)), C.byref(o) if o else None))

    def pipeline_step_to(self, st_in, st_out, ctrl, n_frames: int, out=None):
        """Out-of-place pipeline_step: reads st_in, writes st_out (no copies of the previous state needed)."""
        o = self._outputs(out)
        _check(lib().rr_pipeline_step_to(self.h, C.byref(self._state(st_in)), C.byref(self._state(st_out)),
                                         _ptr(ctrl, numel=self.N * self.dims.nu), int(n_frames), C.byref(o) if o else None))

    def env_step_to(self, st_in, st_out, action, n_frames: int, env, cur_frame_in, out=None):
        o = self._outputs(out)
        _check(lib().rr_env_step_to(self.h, C.byref(self._state(st_in)), C.byref(self._state(st_out)),
                                    _ptr(action, numel=self.N * self.dims.nu), int(n_frames), C.byref(self._env(env)),
                                    _ptr(cur_frame_in, torch.int32, self.N), C.byref(o) if o else None))

    def contact_overflow(self) -> int:
        """(env, env step) events with more pairs in penetration than contact slots -- a multi-step launch counts each of its steps
        (candidate-pair models; 0 for the others; synchronises the stream)."""
        n = C.c_int64()
        _check(lib().rr_batch_contact_overflow(self.h, C.byref(n)))
        return int(n.value)

    def bad_states(self) -> int:
        """(env, env step) events in which the bad-state check (env io `bad_state_max` > 0) found a non-finite or out-of-range qpos /
        qvel -- a multi-step launch counts each of its steps (0 while the check is off; synchronises the stream)."""
        n = C.c_int64()
        _check(lib().rr_batch_bad_states(self.h, C.byref(n)))
        return int(n.value)

    def unroll_supported(self, with_actor: bool = False) -> bool:
        return _check(lib().rr_batch_unroll_supported(self.h, int(with_actor))) == 1

    def _unroll_io(self, wrap) -> RRUnrollIO:
        """`wrap` = dict(first, first_obs, prev_done, steps_in, steps_out, truncation_out, episode_length): the state of the Episode +
        AutoReset wrappers that a multi-step launch reads and writes.  With `slots` = K (an env with clip restarts) `first` and
        `first_obs` are the bank, [K, N, width] each."""
        N, K = self.N, self.obs_width()
        S = int(wrap.get("slots", 1))
        d = self.dims
        f = wrap["first"]
        first = RRState(_ptr(f["qpos"], numel=S * N * d.nq), _ptr(f["qvel"], numel=S * N * d.nv), _ptr(f["act"], numel=S * N * d.na),
                        _ptr(f["qacc_warmstart"], numel=S * N * d.nv))
        return RRUnrollIO(first, _ptr(wrap["first_obs"], numel=S * N * K), *(_ptr(wrap[k], numel=N) for k in
                          ("prev_done", "steps_in", "steps_out", "truncation_out")), float(wrap["episode_length"]))

    def _actor_io(self, who: str, actor: dict, obs_in, T: int, noise=None, actions_out=None, traj: Optional[dict] = None, segment: int = 0) -> RRActorIO:
        """The in-kernel actor's block.  actor (`acting.actor_params`): mean, std (or None), w0, b0, hidden_wt / hidden_b (lists, transposed
        32 x 32 weights), head_wt, head_b (padded to 64 columns for up to 32 actions, to 128 for 33 .. 64), min_std;  traj (the recording
        form): obs [N, T+1, K], raw_action [N, T, A], log_prob / reward / discount / truncation [N, T] (contiguous views); with `segment`
        = L < T: U = T / L such blocks ([U, N, L+1, K], ...), a whole rollout phase of U unrolls."""
        N, A_, K = self.N, self.dims.nu, self.obs_width()
        HW = head_columns(2 * A_)
        bad = f"{who}: inconsistent shapes" if traj is not None else f"{who}: inconsistent actor shapes"
        if actor["w0"].shape != (32, K) or actor["head_wt"].shape != (32, HW) or actor["head_b"].numel() != HW or actor["b0"].numel() != 32:
            raise ValueError(bad)
        if any(w.numel() != 1024 or b.numel() != 32 for w, b in zip(actor["hidden_wt"], actor["hidden_b"])):
            raise ValueError(f"{who}: hidden layers are 32 x 32")
        L_ = segment or T
        if traj is not None and (noise.numel() != T * N * A_ or actions_out.numel() != T * N * A_ or traj["obs"].numel() != (T // L_) * N * (L_ + 1) * K
                                 or traj["raw_action"].numel() != N * T * A_ or any(traj[k].numel() != N * T for k in ("log_prob", "reward", "discount", "truncation"))):
            raise ValueError(bad)
        hidden = lambda ts: (C.c_void_p * 4)(*([_ptr(t) for t in ts] + [None] * (4 - len(ts))))
        names = ("obs", "raw_action", "log_prob", "reward", "discount", "truncation")
        return RRActorIO(_ptr(obs_in, numel=N * K), _ptr(actor.get("mean"), numel=K), _ptr(actor.get("std"), numel=K), _ptr(actor["w0"]), _ptr(actor["b0"]),
                         hidden(actor["hidden_wt"]), hidden(actor["hidden_b"]), _ptr(actor["head_wt"]), _ptr(actor["head_b"]), _ptr(noise, numel=T * N * A_),
                         _ptr(actions_out, numel=T * N * A_), *(_ptr(traj[k]) if traj is not None else None for k in names), float(actor["min_std"]),
                         len(actor["hidden_wt"]) + 1, int(segment))

    def env_unroll(self, st_in, st_out, actions, n_frames: int, env, cur_frame_in, wrap: dict):
        """`actions.shape[0]` env steps with the Episode + AutoReset wrappers (`wrap`: see `_unroll_io`) in one launch (C ABI `rr_env_unroll`)."""
        T = actions.shape[0]
        _check(lib().rr_env_unroll(self.h, C.byref(self._state(st_in)), C.byref(self._state(st_out)),
                                   _ptr(actions, numel=T * self.N * self.dims.nu), T, int(n_frames), C.byref(self._env(env)),
                                   _ptr(cur_frame_in, torch.int32, self.N), C.byref(self._unroll_io(wrap))))

    def env_unroll_policy(self, st_in, st_out, T: int, n_frames: int, env, cur_frame_in, wrap: dict, actor: dict, noise, actions_out, traj: dict,
                          obs_in, segment: int = 0):
        """T x [policy -> sample -> wrapped env step] with the transitions recorded in `traj`, one launch (C ABI `rr_env_unroll_policy`);
        `wrap`, `actor`, `traj`, `segment`: see `_unroll_io` / `_actor_io`."""
        if T % (segment or T):
            raise ValueError("rr_env_unroll_policy: the number of steps must be a multiple of the segment length")
        a = self._actor_io("rr_env_unroll_policy", actor, obs_in, T, noise, actions_out, traj, segment or T)
        _check(lib().rr_env_unroll_policy(self.h, C.byref(self._state(st_in)), C.byref(self._state(st_out)), int(T), int(n_frames),
                                          C.byref(self._env(env)), _ptr(cur_frame_in, torch.int32, self.N), C.byref(self._unroll_io(wrap)), C.byref(a)))

    def eval_supported(self) -> bool:
        """Whether this batch evaluates in one launch (C ABI `rr_batch_eval_supported`): CG solver, a model with a multi-step instance,
        no per-env parameters."""
        return _check(lib().rr_batch_eval_supported(self.h)) == 1

    def env_unroll_eval(self, st_in, st_out, T: int, n_frames: int, env, cur_frame_in, actor: dict, obs_in, obs_ring, noise=None, actions_out=None,
                        eval_metrics=None, qpos_out=None, wrap: Optional[dict] = None):
        """T x [policy -> action -> env step] without a trajectory, one launch (C ABI `rr_env_unroll_eval`).  `wrap` (see `_unroll_io`): the
        Episode + AutoReset wrappers between the steps and brax's EvalWrapper on `eval_metrics` [N, 6] (in place); None: the unwrapped env.
        noise [T, N, A] or None (deterministic policy); actions_out [T, N, A] and qpos_out [T + 1, N, nq] optional; obs_ring [N, 2, K]
        (final observation: obs_ring[:, T & 1])."""
        d, N = self.dims, self.N
        a = self._actor_io("rr_env_unroll_eval", actor, obs_in, T, noise, actions_out)
        e = RREvalIO(_ptr(eval_metrics, numel=N * 6), _ptr(obs_ring, numel=N * 2 * self.obs_width()), _ptr(qpos_out, numel=(T + 1) * N * d.nq),
                     0 if wrap is not None else 1)
        w = self._unroll_io(wrap) if wrap is not None else None
        _check(lib().rr_env_unroll_eval(self.h, C.byref(self._state(st_in)), C.byref(self._state(st_out)), int(T), int(n_frames), C.byref(self._env(env)),
                                        _ptr(cur_frame_in, torch.int32, N), C.byref(w) if w is not None else None, C.byref(a), C.byref(e)))

    def env_reset(self, st, env, out=None):
        o = self._outputs(out)
        _check(lib().rr_env_reset(self.h, C.byref(self._state(st)), C.byref(self._env(env)), C.byref(o) if o else None))

    def debug_layout(self):
        names, offs, sizes = C.POINTER(C.c_char_p)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)()
        n = _check(lib().rr_debug_layout(self.h, C.byref(names), C.byref(offs), C.byref(sizes)))
        return {names[i].decode(): (offs[i], sizes[i]) for i in range(n)}

    def set_profile(self, buf: Optional[torch.Tensor]):
        """Diagnostic: int64 device tensor [N,24] receiving per-phase cycle sums (None = off); slots 20 / 21 count the line searches'
        bracketing iterations executed / left out by the repeat exit."""
        _check(lib().rr_batch_set_profile(self.h, _dp(buf)))

    def set_schedule(self, env_map: Optional[torch.Tensor], cost: Optional[torch.Tensor]):
        """workgroup -> environment map (int32 [N] device, a permutation) and per-env cycle output (int32 [N] device); None = off.
        The tensors must stay alive while the batch launches (C ABI `rr_batch_set_schedule`)."""
        self._sched = (env_map, cost)
        _check(lib().rr_batch_set_schedule(self.h, _ptr(env_map, torch.int32, self.N), _ptr(cost, torch.int32, self.N)))

    def _set_block(self, attr: str, setter, block, tensors):
        """The tail of the block setters below: hand `block` (the block's struct; None clears it) to the library's `setter`, then
        keep `tensors` alive in `attr` while the block stands, or drop them."""
        _check(setter(self.h, None if block is None else C.byref(block)))
        setattr(self, attr, None if block is None else tensors)

    def set_pose(self, track_pose: Optional[torch.Tensor], pose_metrics: Optional[torch.Tensor] = None, quat_reward=(1.0, 2.0), joint_reward=(1.0, 0.5)):
        """The pose-tracking block of this batch's later env steps (C ABI `rr_batch_set_pose`): `track_pose` [(C,) T, nq - 3] rows of
        quaternion then joints, `pose_metrics` [N, 2] out, `quat_reward` / `joint_reward` = (weight, scale); None clears it.  The env-io
        dict of a launch (`track_pose`, `pose_metrics`, `quat_reward`, `joint_reward` keys) sets or clears it by itself.  The batch keeps
        the tensors alive."""
        p = None if track_pose is None else RRPoseIO(_ptr(track_pose), _ptr(pose_metrics, numel=2 * self.N), *quat_reward, *joint_reward)
        self._set_block("_pose", lib().rr_batch_set_pose, p, (track_pose, pose_metrics))

    def set_pose_termination(self, fail: Optional[torch.Tensor], thresholds=(math.inf, math.inf, math.inf)):
        """The pose-termination block of this batch's later env steps (C ABI `rr_batch_set_pose_termination`): `fail` [N] out, the code
        of each env's step as a float 0 .. 7; `thresholds` = (max_pos, max_quat, max_joint), each > 0, inf = that criterion off; None
        clears it.  Needs the pose block (`set_pose`).  The env-io dict of a launch (`pose_fail`, `pose_termination` keys) sets or clears
        it by itself.  The batch keeps the tensor alive."""
        t = None if fail is None else RRPoseTermIO(_ptr(fail, numel=self.N), *(float(x) for x in thresholds), 0)
        self._set_block("_pterm", lib().rr_batch_set_pose_termination, t, fail)

    def set_body_tracking(self, track_bodies: Optional[torch.Tensor], body_weights: Optional[torch.Tensor] = None,
                          body_metrics: Optional[torch.Tensor] = None, body_reward=(1.0, 8.0), endeff_reward=(1.0, 100.0)):
        """The body-tracking block of this batch's later env steps (C ABI `rr_batch_set_body_tracking`): `track_bodies` [(C), T, nbody, 3]
        the clip's global body positions, `body_weights` [2, nbody] the 0 / 1 masks of the tracked bodies and of the end effectors,
        `body_metrics` [N, 2] out (body_reward, endeff_reward); `body_reward` / `endeff_reward` = (weight, scale); None clears it.
        Needs the pose block (`set_pose`).  The env-io dict of a launch (`track_bodies`, `body_weights`, `body_metrics`, `body_reward`,
        `endeff_reward` keys) sets or clears it by itself.  The batch keeps the tensors alive."""
        t, nb = None, self.dims.nbody
        if track_bodies is not None:
            if track_bodies.dim() < 3 or tuple(track_bodies.shape[-2:]) != (nb, 3):
                raise ValueError(f"track_bodies has shape {tuple(track_bodies.shape)}, expected [(C), T, {nb}, 3]")
            t = RRBodyIO(_ptr(track_bodies), _ptr(body_weights, numel=2 * nb), _ptr(body_metrics, numel=2 * self.N),
                         float(body_reward[0]), float(body_reward[1]), float(endeff_reward[0]), float(endeff_reward[1]))
        self._set_block("_body", lib().rr_batch_set_body_tracking, t, (track_bodies, body_weights, body_metrics))

    def set_velocity_tracking(self, track_vel: Optional[torch.Tensor], vel_metrics: Optional[torch.Tensor] = None, lin_vel_reward=(1.0, 10.0),
                              ang_vel_reward=(1.0, 0.1), joint_vel_reward=(1.0, 0.01)):
        """The velocity-tracking block of this batch's later env steps (C ABI `rr_batch_set_velocity_tracking`): `track_vel` [(C), T, nv]
        the clip's velocities, rows in qvel layout, `vel_metrics` [N, 3] out (lin_vel_reward, ang_vel_reward, joint_vel_reward); the three
        pairs = (weight, scale); None clears it.  Needs the pose block (`set_pose`).  The env-io dict of a launch (`track_vel`,
        `vel_metrics`, `lin_vel_reward`, `ang_vel_reward`, `joint_vel_reward` keys) sets or clears it by itself.  The batch keeps the
        tensors alive."""
        t, nv = None, self.dims.nv
        if track_vel is not None:
            if track_vel.dim() < 2 or track_vel.shape[-1] != nv:
                raise ValueError(f"track_vel has shape {tuple(track_vel.shape)}, expected [(C), T, {nv}]")
            t = RRVelIO(_ptr(track_vel), _ptr(vel_metrics, numel=3 * self.N), *(float(x) for pair in (lin_vel_reward, ang_vel_reward, joint_vel_reward) for x in pair))
        self._set_block("_vel", lib().rr_batch_set_velocity_tracking, t, (track_vel, vel_metrics))

    def velocity_tracking_supported(self, with_actor: bool = False) -> Optional[str]:
        """None when this batch serves velocity tracking at its frame count (C ABI `rr_batch_velocity_tracking_supported`) -- with
        `with_actor` also in the one-launch rollout with the actor inside -- else the refusal's text."""
        return self._refusal(lib().rr_batch_velocity_tracking_supported, int(with_actor))

    def set_clip_restarts(self, frames: Optional[torch.Tensor], slot_in: Optional[torch.Tensor] = None, slot_out: Optional[torch.Tensor] = None,
                          end_at_clip_end: bool = False):
        """The clip-restart block of this batch's later multi-step launches (C ABI `rr_batch_set_clip_restarts`): `frames` int32 [K, N]
        the start frame of each bank entry, `slot_in` / `slot_out` int32 [N]; None clears it.  Needs the pose block (`set_pose`).  The
        env-io dict of a launch (`restart` key) sets or clears it by itself.  The batch keeps the tensors alive."""
        t = None
        if frames is not None:
            if frames.dim() != 2 or frames.shape[1] != self.N:
                raise ValueError(f"clip restarts: frames has shape {tuple(frames.shape)}, expected [K, {self.N}]")
            t = RRClipRestartIO(_ptr(frames, torch.int32), _ptr(slot_in, torch.int32, self.N), _ptr(slot_out, torch.int32, self.N),
                                int(frames.shape[0]), int(bool(end_at_clip_end)))
        self._set_block("_restart", lib().rr_batch_set_clip_restarts, t, (frames, slot_in, slot_out))

    def set_clip_library(self, lengths: Optional[torch.Tensor], bank_clips: Optional[torch.Tensor] = None, clip_out: Optional[torch.Tensor] = None,
                         num_clips: Optional[int] = None):
        """The clip-library block of this batch's later env launches (C ABI `rr_batch_set_clip_library`): `lengths` int32 [C] the frames
        of each clip (None: every clip has T), `bank_clips` int32 [K, N] the clip of each clip-restart bank entry (None: every entry on
        the env's clip) with `clip_out` int32 [N], which a multi-step launch fills with the clip each env is on after it; all None clears
        the block.  `num_clips` (given by the env-io path): the length `lengths` must have.  Needs the pose block, and for `bank_clips`
        the clip-restart block.  The env-io dict of a launch (`clip_library` key) sets or clears it by itself.  The batch keeps the
        tensors alive."""
        t = None
        if lengths is not None or bank_clips is not None:
            if lengths is not None and (lengths.dim() != 1 or (num_clips is not None and lengths.shape[0] != num_clips)):
                raise ValueError(f"clip library: lengths has shape {tuple(lengths.shape)}, expected [{'C' if num_clips is None else num_clips}]")
            if bank_clips is not None and (bank_clips.dim() != 2 or bank_clips.shape[1] != self.N):
                raise ValueError(f"clip library: bank_clips has shape {tuple(bank_clips.shape)}, expected [K, {self.N}]")
            t = RRClipLibraryIO(_ptr(lengths, torch.int32), _ptr(bank_clips, torch.int32), _ptr(clip_out, torch.int32, self.N))
        self._set_block("_library", lib().rr_batch_set_clip_library, t, (lengths, bank_clips, clip_out))

    def clip_library_supported(self, with_actor: bool = False) -> Optional[str]:
        """None when this batch serves the clip library at its frame count (C ABI `rr_batch_clip_library_supported`) -- with
        `with_actor` also in the one-launch rollout with the actor inside -- else the refusal's text."""
        return self._refusal(lib().rr_batch_clip_library_supported, int(with_actor))

    def set_clip_sampling(self, weights: Optional[torch.Tensor], draws_in: Optional[torch.Tensor] = None, draws_out: Optional[torch.Tensor] = None,
                          outcomes: Optional[torch.Tensor] = None, seed: int = 0, num_clips: Optional[int] = None):
        """The clip-sampling block of this batch's later multi-step launches (C ABI `rr_batch_set_clip_sampling`): `weights` int32 [C],
        entries 0 .. 65535, the weights a restore draws its bank entry by (None: the next entry), with `draws_in` / `draws_out` int32 [N],
        each env's restore count before and after the launch; `outcomes` int64 [C, 5], the per-clip outcome counters the launches add to
        (None: no counting); `seed` the draw's seed; `weights` and `outcomes` both None clears the block.  `num_clips` (given by the
        env-io path): the length both tables must have.  Needs the clip-restart block, and for `weights` the clip library's bank clips.
        The launches read the tables' content when they run: rewrite them in place.  The env-io dict of a launch (`clip_sampling` key)
        sets or clears it by itself.  The batch keeps the tensors alive."""
        t = None
        if weights is not None or outcomes is not None:
            for name, a, tail in (("weights", weights, ()), ("outcomes", outcomes, (5,))):
                if a is not None and (a.dim() != 1 + len(tail) or tuple(a.shape[1:]) != tail or (num_clips is not None and a.shape[0] != num_clips)):
                    raise ValueError(f"clip sampling: {name} has shape {tuple(a.shape)}, expected {(('C' if num_clips is None else num_clips),) + tail}")
            t = RRClipSamplingIO(_ptr(weights, torch.int32), _ptr(draws_in, torch.int32, self.N), _ptr(draws_out, torch.int32, self.N),
                                 _ptr(outcomes, torch.int64), int(seed) & 0xFFFFFFFF)
        self._set_block("_sampling", lib().rr_batch_set_clip_sampling, t, (weights, draws_in, draws_out, outcomes))

    def set_reference_restart(self, draws_in: Optional[torch.Tensor], draws_out: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None,
                              seed: int = 0, frame_range=(0, 100), across_clips: bool = False, noise_scale: float = 0.0, num_clips: Optional[int] = None):
        """The reference-restart block of this batch's later multi-step launches (C ABI `rr_batch_set_reference_restart`): a restore reads
        no bank entry but draws a clip (`across_clips`; by `weights` int32 [C] or, None, uniformly) and a start frame in `frame_range`,
        builds the start state from the clip's rows plus `noise_scale` noise and forms its observation in the launch (`seed` the draws'
        seed).  `draws_in` / `draws_out` int32 [N]: each env's restore count before and after the launch; `draws_in` None clears the
        block.  Needs the pose and clip-restart blocks.  The env-io dict of a launch (`reference_restart` key) sets or clears it by
        itself.  The batch keeps the tensors alive."""
        t = None
        if draws_in is not None:
            if weights is not None and (weights.dim() != 1 or (num_clips is not None and weights.shape[0] != num_clips)):
                raise ValueError(f"reference restarts: weights has shape {tuple(weights.shape)}, expected [{'C' if num_clips is None else num_clips}]")
            t = RRReferenceRestartIO(_ptr(weights, torch.int32), _ptr(draws_in, torch.int32, self.N), _ptr(draws_out, torch.int32, self.N),
                                     int(seed) & 0xFFFFFFFF, int(frame_range[0]), int(frame_range[1]), int(bool(across_clips)), float(noise_scale), 0)
        self._set_block("_refrestart", lib().rr_batch_set_reference_restart, t, (weights, draws_in, draws_out))

    def reference_restart_supported(self, with_actor: bool = False) -> Optional[str]:
        """None when this batch's multi-step launches serve reference restarts at its frame count (C ABI
        `rr_batch_reference_restart_supported`) -- with `with_actor` the one-launch rollout with the actor inside -- else the refusal's text."""
        return self._refusal(lib().rr_batch_reference_restart_supported, int(with_actor))

    def clip_sampling_supported(self, with_actor: bool = False) -> Optional[str]:
        """None when this batch serves clip sampling at its frame count (C ABI `rr_batch_clip_sampling_supported`) -- with `with_actor`
        also in the one-launch rollout with the actor inside -- else the refusal's text."""
        return self._refusal(lib().rr_batch_clip_sampling_supported, int(with_actor))

    def _refusal(self, query, *args) -> Optional[str]:
        """None when the `rr_batch_*_supported` function `query` answers 1 for this batch, else the text it left in `rr_last_error`."""
        if _check(query(self.h, *args)) == 1:
            return None
        return lib().rr_last_error().decode()

    def clip_restarts_supported(self, with_actor: bool = False) -> Optional[str]:
        """None when this batch's multi-step launches serve clip restarts at its frame count (C ABI `rr_batch_clip_restarts_supported`)
        -- with `with_actor` the one-launch rollout with the actor inside -- else the refusal's text."""
        return self._refusal(lib().rr_batch_clip_restarts_supported, int(with_actor))

    def body_tracking_supported(self, with_actor: bool = False) -> Optional[str]:
        """None when this batch serves body tracking at its frame count (C ABI `rr_batch_body_tracking_supported`) -- with
        `with_actor` also in the one-launch rollout with the actor inside -- else the refusal's text."""
        return self._refusal(lib().rr_batch_body_tracking_supported, int(with_actor))

    def pose_termination_supported(self, with_actor: bool = False) -> Optional[str]:
        """None when this batch serves pose termination at its frame count (C ABI `rr_batch_pose_termination_supported`) -- with
        `with_actor` also in the one-launch rollout with the actor inside -- else the refusal's text."""
        return self._refusal(lib().rr_batch_pose_termination_supported, int(with_actor))

    def pose_supported(self) -> Optional[str]:
        """None when this batch serves pose tracking (`set_pose`; C ABI `rr_batch_pose_supported`), else the refusal's text."""
        return self._refusal(lib().rr_batch_pose_supported)

    def set_reference_obs(self, frames: int):
        """`frames` = H reference frames behind every observation row of this batch (C ABI `rr_batch_set_reference_obs`): 0 .. 16, more
        than 0 only with the pose block set (`set_pose`).  Every buffer documented as obs wide is then `obs_width()` wide."""
        _check(lib().rr_batch_set_reference_obs(self.h, int(frames)))

    def obs_width(self) -> int:
        """Entries of an observation row of this batch (C ABI `rr_batch_obs_width`): obs_dim + frames * nq."""
        return _check(lib().rr_batch_obs_width(self.h))

    def reference_obs_supported(self, frames: int, with_actor: bool = False) -> Optional[str]:
        """None when this batch serves `frames` reference frames (C ABI `rr_batch_reference_obs_supported`) -- with `with_actor` also in
        the one-launch rollout with the actor inside, whose actor reads a bounded row width -- else the refusal's text."""
        return self._refusal(lib().rr_batch_reference_obs_supported, int(frames), int(with_actor))

    def env_params_supported(self) -> bool:
        """Whether this batch's model / solver has kernel instances with per-env parameters (C ABI `rr_batch_env_params_supported`)."""
        return _check(lib().rr_batch_env_params_supported(self.h)) == 1

    def set_env_params(self, dof_f: Optional[torch.Tensor] = None, act_f: Optional[torch.Tensor] = None, con_f: Optional[torch.Tensor] = None):
        """Per-environment parameter rows (C ABI `rr_batch_set_env_params`): float32 device tensors dof_f [N, nv, 16], act_f [N, nu, 8],
        con_f [N, ncon, 26] as `ktables.env_param_tables` builds them; None leaves that table the model's shared one, all None clears
        the parameters.  The batch keeps its own copy."""
        d, N = self.dims, self.N
        for name, t, shape in (("dof_f", dof_f, (N, d.nv, 16)), ("act_f", act_f, (N, d.nu, 8)), ("con_f", con_f, (N, d.ncon, 26))):
            if t is not None and tuple(t.shape) != shape:
                raise ValueError(f"set_env_params: {name} has shape {tuple(t.shape)}, expected {shape}")
        p = RREnvParams(_ptr(dof_f), _ptr(act_f), _ptr(con_f), d.nv, d.nu, d.ncon, N)
        _check(lib().rr_batch_set_env_params(self.h, C.byref(p)))

    def set_ls_repeat_exit(self, enable: bool):
        """Debug-dump launches only: False makes the line search run the bracketing iterations that repeat the one before instead of
        leaving the loop (C ABI `rr_batch_set_ls_repeat_exit`); the dump field `ls_iters` counts both kinds.  Default True."""
        _check(lib().rr_batch_set_ls_repeat_exit(self.h, int(enable)))

    def set_solver_trim(self, enable: bool):
        """Debug-dump launches only: False makes the solver do the work the production code leaves out because nothing reads it -- the
        solve and the new search direction before the exit test, the contact walk of the cost-only context at qacc_smooth, the rebuild
        of that context's rows where it is chosen (C ABI `rr_batch_set_solver_trim`).  The dump field `solver_end` tells which start was
        chosen and how the loop ended.  Default True."""
        _check(lib().rr_batch_set_solver_trim(self.h, int(enable)))

    def set_solver_batch(self, enable: bool):
        """Debug-dump launches only: False makes the line search form and stage its compacted row positions and D values in every call
        instead of once per substep (C ABI `rr_batch_set_solver_batch`).  Default True."""
        _check(lib().rr_batch_set_solver_batch(self.h, int(enable)))

    def set_solve_resident(self, enable: bool):
        """A/B switch for tests: False makes the batch's production single-step launches run the instance that gathers the inverse
        factor's entries from LDS in every solve instead of holding them in registers for the substep (C ABI
        `rr_batch_set_solve_resident`).  Same results bit for bit; rodent_optimized dimensions with the CG solver only.  Default True."""
        _check(lib().rr_batch_set_solve_resident(self.h, int(enable)))

    def set_root_slot(self, enable: bool):
        """A/B switch for tests: False makes the batch's production single-step launches run the instance whose tree phases use the plain
        map body = lane + 64 * slot instead of the root body in a slot of its own (C ABI `rr_batch_set_root_slot`).  Same results bit
        for bit; the rodent_optimized model with the CG solver only.  Default True."""
        _check(lib().rr_batch_set_root_slot(self.h, int(enable)))

    def set_timing(self, enable: bool):
        _check(lib().rr_batch_set_timing(self.h, int(enable)))

    def kernel_time(self):
        ms, n = C.c_double(), C.c_int64()
        _check(lib().rr_batch_kernel_time(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value


def compute_gae(truncation, termination, rewards, values, bootstrap_value, lambda_: float, discount: float):
    """GAE on the GPU in one launch (C ABI `rr_compute_gae`): inputs time-major [T, B] float32 device tensors."""
    T, B = values.shape
    args = [t.contiguous() for t in (truncation, termination, rewards, values, bootstrap_value)]
    for t in args:
        _ptr(t)
    vs = torch.empty_like(args[3])
    adv = torch.empty_like(args[3])
    stream = torch.cuda.current_stream(values.device).cuda_stream
    _check(lib().rr_compute_gae(*[t.data_ptr() for t in args], T, B, float(lambda_), float(discount), vs.data_ptr(),
                                adv.data_ptr(), C.c_void_p(stream)))
    return vs, adv


def _wrap_common(first, cur, prev_done, prev_steps, done, steps, truncation, K=None):
    """The head every per-step wrapper entry takes: (N, narr, first[], cur[], widths[]) and the current stream.  `first` holds states
    [N, ...] like `cur` (K None) or banks [K, N, ...]."""
    n = len(cur)
    N = done.numel()
    for t in list(first) + list(cur) + [prev_done, prev_steps, done, steps, truncation]:
        _ptr(t)
    for f, c in zip(first, cur):
        if K is None and f.shape != c.shape:
            raise ValueError("first / current state shapes differ")
        if K is not None and tuple(f.shape) != (K,) + tuple(c.shape):
            raise ValueError("bank / current state shapes differ")
    F = (C.c_void_p * n)(*[t.data_ptr() for t in first])
    Cu = (C.c_void_p * n)(*[t.data_ptr() for t in cur])
    W = (C.c_int32 * n)(*[t.numel() // N for t in cur])
    return (N, n, F, Cu, W), C.c_void_p(torch.cuda.current_stream(done.device).cuda_stream)


def wrap_episode_autoreset(first, cur, prev_done, prev_steps, done, steps, truncation, episode_length: float, action_repeat: float):
    """Fused EpisodeWrapper + AutoResetWrapper bookkeeping (C ABI `rr_wrap_episode_autoreset`): `first` / `cur` are equally
    long lists of contiguous float32 device tensors with a leading env axis; `cur`, `done`, `steps`, `truncation` are written."""
    head, stream = _wrap_common(first, cur, prev_done, prev_steps, done, steps, truncation)
    _check(lib().rr_wrap_episode_autoreset(*head, prev_done.data_ptr(), prev_steps.data_ptr(), done.data_ptr(), steps.data_ptr(),
                                           truncation.data_ptr(), float(episode_length), float(action_repeat), stream))


def wrap_clip(first, cur, prev_done, prev_steps, done, steps, truncation, episode_length: float, action_repeat: float,
              cur_frame, bank_frames, slot_in, slot_out, track_len: int, end_at_clip_end: bool, clip=None, bank_clips=None, lengths=None,
              num_clips=None, pose_fail=None, weights=None, draws_in=None, draws_out=None, outcomes=None, seed: int = 0):
    """`wrap_episode_autoreset` for an env with clip restarts: `first` are banks [K, N, ...], `cur_frame` int32 [N] holds the stepped
    frame and is finished in place, `bank_frames` int32 [K, N], `slot_in` / `slot_out` int32 [N].
    The clip library: `clip` int32 [N], the clip each env made the step on, finished in place (the bank entry's clip where done);
    `bank_clips` int32 [K, N] or None; `lengths` int32 [C] or None -- the clip's end is taken at the env's own clip's length.
    Clip sampling (needs `num_clips` C): `weights` int32 [C] or None with `draws_in` / `draws_out` int32 [N]; `outcomes` int64 [C, 5] or
    None, added to in place; `pose_fail` float [N] or None, the step's pose-termination codes; `seed` the draw's seed.
    The call goes to the narrowest C entry that serves what was passed -- `rr_wrap_clip_restart`, with `bank_clips` or `lengths`
    `rr_wrap_clip_library`, with `weights` or `outcomes` `rr_wrap_clip_sampling` -- and arguments of a wider entry are not read."""
    K = bank_frames.shape[0]
    head, stream = _wrap_common(first, cur, prev_done, prev_steps, done, steps, truncation, K)
    N = head[0]
    args = head + (prev_done.data_ptr(), prev_steps.data_ptr(), done.data_ptr(), steps.data_ptr(), truncation.data_ptr(), float(episode_length),
                   float(action_repeat), _ptr(cur_frame, torch.int32, N), _ptr(bank_frames, torch.int32, K * N), _ptr(slot_in, torch.int32, N),
                   _ptr(slot_out, torch.int32, N), int(K), int(track_len), int(bool(end_at_clip_end)))
    sampling, library = weights is not None or outcomes is not None, bank_clips is not None or lengths is not None
    if not sampling and not library:
        _check(lib().rr_wrap_clip_restart(*args, stream))
        return
    args += (_ptr(clip, torch.int32, N), _ptr(bank_clips, torch.int32, K * N), _ptr(lengths, torch.int32))
    if not sampling:
        _check(lib().rr_wrap_clip_library(*args, stream))
        return
    block = RRClipSamplingIO(_ptr(weights, torch.int32, int(num_clips)), _ptr(draws_in, torch.int32, N), _ptr(draws_out, torch.int32, N),
                             _ptr(outcomes, torch.int64, 5 * int(num_clips)), int(seed) & 0xFFFFFFFF)
    _check(lib().rr_wrap_clip_sampling(*args, int(num_clips), _ptr(pose_fail, numel=N), C.byref(block), stream))


def _mlp_net(weights, biases, in_dim=None):
    """(RRMlpNet, keep-alive) for a list of nn.Linear-layout weights [out, in] and biases [out] (float32 device tensors); in_dim: the input
    width when the first matrix is stored with padded rows."""
    n = len(weights)
    for w, b in zip(weights, biases):
        _ptr(w); _ptr(b)
        if w.dim() != 2 or b.numel() != w.shape[0]:
            raise ValueError("weights must be [out, in] with biases [out]")
    W = (C.c_void_p * n)(*[w.data_ptr() for w in weights])
    B = (C.c_void_p * n)(*[b.data_ptr() for b in biases])
    S = (C.c_int32 * (n + 1))(in_dim or weights[0].shape[1], *[w.shape[0] for w in weights])
    return RRMlpNet(C.cast(W, C.POINTER(C.c_void_p)), C.cast(B, C.POINTER(C.c_void_p)), C.cast(S, C.POINTER(C.c_int32)), n), (W, B, S)


def mlp_forward(obs, mean=None, std=None, policy=None, value=None, want_pre=False, rows=None):
    """Fused normalise + policy MLP + value MLP forward on the f32 matrix cores (C ABI `rr_mlp_forward`).

    obs [M, K] float32 device; policy / value: (weights, biases) lists in nn.Linear layout or None.  Returns
    (policy_out [M, P] | None, value_out [M] | None, policy_pre [L-1, M, 32] | None, value_pre [L-1, M, 256] | None); P <= 128.
    A policy whose hidden layers are all 256 wide runs as a launch of its own (policy_pre [L-1, M, 256]); widths other than 32 / 256: refused.
    rows (int64 [M], optional): sample m is row rows[m] of obs (the minibatch addressed in place)."""
    M, K = obs.shape
    _ptr(obs)
    if rows is not None:
        M = rows.numel()
        _ptr(rows, torch.int64)
    dev = obs.device
    pn = vn = None
    keep = []
    pol_out = val_out = pol_pre = val_pre = None
    if policy is not None:
        pn, k = _mlp_net(*policy, in_dim=K); keep.append((k, policy))
        pol_out = torch.empty(M, policy[0][-1].shape[0], device=dev)
        if want_pre:
            pol_pre = torch.empty(len(policy[0]) - 1, M, policy[0][0].shape[0], device=dev)      # the policy's hidden width: 32 or 256
    if value is not None:
        vn, k = _mlp_net(*value, in_dim=K); keep.append((k, value))
        val_out = torch.empty(M, device=dev)
        if want_pre:
            val_pre = torch.empty(len(value[0]) - 1, M, 256, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    _check(lib().rr_mlp_forward(obs.data_ptr(), _dp(rows), M, K, _ptr(mean, numel=K), _ptr(std, numel=K), C.byref(pn) if pn is not None else None,
                                C.byref(vn) if vn is not None else None, _dp(pol_out), _dp(val_out), _dp(pol_pre), _dp(val_pre), C.c_void_p(stream)))
    return pol_out, val_out, pol_pre, val_pre


def ppo_loss(policy_logits, values, data, idx, noise, T: int, *, entropy_cost, discounting, reward_scaling, gae_lambda, clipping_epsilon,
             normalize_advantage=True, min_std=0.001, out=None, diag=None, kl_out=None):
    """Loss half of a PPO minibatch update and its gradient w.r.t. the network outputs (C ABI `rr_ppo_loss`, 3 launches).
    `diag` (device float64 [16]): the same through `rr_ppo_loss_diag`, which also writes the minibatch's approx_kl, clip_fraction,
    explained_variance and entropy to diag[0:4], adds them to the accumulators diag[8:14] (`DIAG_*`) and, with `kl_out` (one float32
    element), stores the KL there; gradients and metrics are bitwise those of the plain call.

    policy_logits [(T+1)*B, 2A] / values [(T+1)*B]: the networks' outputs on the gathered minibatch, time-major; `data`: the
    collected batch, batch-major (`raw_action` [R, T, A]; `log_prob`, `reward`, `discount`, `truncation` [R, T]); idx [B] int64
    minibatch rows (None = the first B rows); noise [T*B, A].  Returns (grad_logits, grad_values, metrics[4]); `out` = a dict
    of persistent buffers {grad_logits, grad_values, metrics, workspace} reused across calls (HIP-graph capture needs that)."""
    M, P2 = policy_logits.shape
    B = M // (T + 1)
    A = P2 // 2
    dev = policy_logits.device
    for t in (policy_logits, values, noise, data["raw_action"], data["log_prob"], data["reward"], data["discount"], data["truncation"]):
        _ptr(t)
    if values.numel() != M or noise.numel() != T * B * A or data["raw_action"].shape[1:] != (T, A) or data["log_prob"].shape[1] != T:
        raise ValueError("rr_ppo_loss: inconsistent shapes")
    if idx is not None:
        _ptr(idx, torch.int64, B)
    elif data["log_prob"].shape[0] < B:
        raise ValueError("rr_ppo_loss: fewer batch rows than the minibatch")
    out = out if out is not None else {}
    wb = lib().rr_ppo_loss_workspace_bytes(T, B) if diag is None else lib().rr_ppo_loss_diag_workspace_bytes(T, B)
    if "workspace" not in out or out["workspace"].numel() * 8 < wb or out["grad_logits"].shape != policy_logits.shape:
        out["workspace"] = torch.empty((wb + 7) // 8, dtype=torch.float64, device=dev)
        out["grad_logits"] = torch.empty_like(policy_logits)
        out["grad_values"] = torch.empty(M, device=dev)
        out["metrics"] = torch.empty(4, device=dev)
    cfg = RRPpoCfg(entropy_cost, discounting, reward_scaling, gae_lambda, clipping_epsilon, min_std, 1 if normalize_advantage else 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    head = (policy_logits.data_ptr(), values.data_ptr(), data["raw_action"].data_ptr(), data["log_prob"].data_ptr(),
            data["reward"].data_ptr(), data["discount"].data_ptr(), data["truncation"].data_ptr(),
            _dp(idx), noise.data_ptr(), T, B, A, C.byref(cfg),
            out["grad_logits"].data_ptr(), out["grad_values"].data_ptr(), out["metrics"].data_ptr())
    tail = (out["workspace"].data_ptr(), out["workspace"].numel() * 8, C.c_void_p(stream))
    if diag is None:
        if kl_out is not None:
            raise ValueError("rr_ppo_loss: kl_out needs diag (rr_ppo_loss_diag)")
        _check(lib().rr_ppo_loss(*head, *tail))
    else:
        _ptr(diag, torch.float64, DIAG_DOUBLES)
        _check(lib().rr_ppo_loss_diag(*head, diag.data_ptr(), None if kl_out is None else _ptr(kl_out, numel=1), *tail))
    return out["grad_logits"], out["grad_values"], out["metrics"]


# the diagnostics block of `rr_ppo_loss_diag` (device float64; include/rodent_rr.h)
DIAG_DOUBLES = 16
DIAG_KL, DIAG_CLIP, DIAG_EV, DIAG_ENT = 0, 1, 2, 3
DIAG_COUNT, DIAG_KL_SUM, DIAG_KL_MAX, DIAG_CLIP_SUM, DIAG_EV_SUM, DIAG_ENT_SUM = 8, 9, 10, 11, 12, 13


def mlp_silu_backward(g, z, bias_grad):
    """delta = g * silu'(z) written over `g`, h = silu(z) written over `z`, bias_grad[n] = column sums of delta (C ABI
    `rr_mlp_silu_backward`).  g, z: [M, H] contiguous float32 device tensors.  Returns (delta, h) = (g, z)."""
    M, H = g.shape
    _ptr(g); _ptr(z, numel=M * H); _ptr(bias_grad, numel=H)
    ws = _ws(None, "silu_bwd", g.device, (M, H), lib().rr_mlp_silu_backward_workspace_bytes(M, H))
    _check(lib().rr_mlp_silu_backward(g.data_ptr(), z.data_ptr(), M, H, g.data_ptr(), z.data_ptr(), bias_grad.data_ptr(), ws.data_ptr(), ws.numel() * 4,
                                      C.c_void_p(torch.cuda.current_stream(g.device).cuda_stream)))
    return g, z


def mlp_value_backward(grad_value, head_weight, hidden_weights_t, pre_act, bias_grads, bufs=None):
    """Delta chain of the value network's hidden stack on the matrix cores (C ABI `rr_mlp_value_backward`).

    grad_value [M]; head_weight [1, 256] or [256]; hidden_weights_t: list, entry j >= 1 = W_j.t().contiguous() (entry 0 ignored);
    pre_act [nh, M, 256] (rr_mlp_forward's value_pre; overwritten by silu(z)); bias_grads: list of nh [256] tensors (written).
    Returns (delta [nh, M, 256], h = pre_act)."""
    nh, M, H = pre_act.shape
    if H != 256 or len(bias_grads) != nh or len(hidden_weights_t) != nh:
        raise ValueError("rr_mlp_value_backward: inconsistent shapes")
    _ptr(grad_value, numel=M); _ptr(head_weight, numel=256); _ptr(pre_act)
    for j in range(nh):
        _ptr(bias_grads[j], numel=256)
        if j > 0:
            _ptr(hidden_weights_t[j], numel=256 * 256)
    dev, bufs = pre_act.device, {} if bufs is None else bufs      # no `bufs`: a fresh delta per call (it is an output)
    ws = _ws(bufs, "value_bwd", dev, (M, nh), lib().rr_mlp_value_backward_workspace_bytes(M, nh))
    delta = _ws(bufs, "value_bwd_delta", dev, (M, nh), 0, shape=pre_act.shape)
    wt = (C.c_void_p * nh)(*[hidden_weights_t[j].data_ptr() if j > 0 else None for j in range(nh)])
    bg = (C.c_void_p * nh)(*[b.data_ptr() for b in bias_grads])
    _check(lib().rr_mlp_value_backward(grad_value.data_ptr(), head_weight.data_ptr(), wt, nh, M, pre_act.data_ptr(), delta.data_ptr(), bg,
                                       ws.data_ptr(), ws.numel() * 4, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return delta, pre_act


def mlp_policy_backward(grad_logits, head_weight_t, hidden_weights_t, pre_act, bias_grads, bufs=None):
    """Delta chain of a 256-wide policy network's hidden stack on the matrix cores (C ABI `rr_mlp_policy_backward`).

    grad_logits [n, P], P <= 128; head_weight_t [256, P] = W_head.t().contiguous(); hidden_weights_t: list, entry j >= 1 =
    W_j.t().contiguous() (entry 0 ignored); pre_act [nh, M >= n, 256] (rr_mlp_forward's policy_pre; the first n rows of each layer are
    overwritten by silu(z), the rows behind them -- a minibatch's bootstrap rows -- are left alone); bias_grads: list of nh [256] tensors
    (written).  Returns (delta [nh, n, 256], h = pre_act).  `bufs`: persistent buffers (a captured HIP graph sees the same addresses)."""
    nh, M, H = pre_act.shape
    n, P = grad_logits.shape
    if H != 256 or M < n or len(bias_grads) != nh or len(hidden_weights_t) != nh or head_weight_t.shape != (256, P):
        raise ValueError("rr_mlp_policy_backward: inconsistent shapes")
    _ptr(grad_logits); _ptr(head_weight_t); _ptr(pre_act)
    for j in range(nh):
        _ptr(bias_grads[j], numel=256)
        if j > 0:
            _ptr(hidden_weights_t[j], numel=256 * 256)
    dev, bufs = pre_act.device, {} if bufs is None else bufs      # no `bufs`: a fresh delta per call (it is an output)
    ws = _ws(bufs, "policy256_bwd", dev, (n, nh), lib().rr_mlp_policy_backward_workspace_bytes(n, nh))
    delta = _ws(bufs, "policy256_bwd_delta", dev, (n, nh), 0, shape=(nh, n, 256))
    wt = (C.c_void_p * nh)(*[hidden_weights_t[j].data_ptr() if j > 0 else None for j in range(nh)])
    bg = (C.c_void_p * nh)(*[b.data_ptr() for b in bias_grads])
    _check(lib().rr_mlp_policy_backward(grad_logits.data_ptr(), head_weight_t.data_ptr(), wt, nh, n, M, P, pre_act.data_ptr(), delta.data_ptr(), bg,
                                        ws.data_ptr(), ws.numel() * 4, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return delta, pre_act


DW_MAX_ITEMS = 12      # RR_DW_MAXB in csrc/rr_mlp.h: products per `rr_mlp_weight_grad_batch` call


def mlp_weight_grad(delta, act, out, rows=None, mean=None, std=None, delta_colsum=None):
    """out[o, i] = sum_m delta[m, o] * x[m, i] (C ABI `rr_mlp_weight_grad`): x = act[m] or, with `rows`, act[rows[m]]; with
    mean / std (and delta_colsum [O] = the column sums of delta), x = (act - mean) / std.  delta [M, O], act [R, I],
    out [O, I]: contiguous float32."""
    M, O = delta.shape
    I = act.shape[1]
    _ptr(delta); _ptr(act); _ptr(out, numel=O * I)
    if rows is not None:
        _ptr(rows, torch.int64, M)
    elif act.shape[0] < M:
        raise ValueError("rr_mlp_weight_grad: fewer activation rows than delta rows")
    ws = _ws(None, "weight_grad", delta.device, (M, O, I), lib().rr_mlp_weight_grad_workspace_bytes(M, O, I))
    _check(lib().rr_mlp_weight_grad(delta.data_ptr(), act.data_ptr(), _dp(rows), _ptr(mean, numel=I), _ptr(std, numel=I),
                                    _ptr(delta_colsum, numel=O) if mean is not None else None, M, O, I, out.data_ptr(), ws.data_ptr(), ws.numel() * 4,
                                    C.c_void_p(torch.cuda.current_stream(delta.device).cuda_stream)))
    return out


def obs_moments(obs, T: int, mean, bufs=None):
    """S1 = sum (x - mean), S2 = sum (x - mean)^2 per observation column (float64 [2, K]) over the rows t < T of every sequence of
    `obs` [..., Tp1, K] (contiguous float32 device tensor; C ABI `rr_obs_moments`): the normaliser update's sums in one pass."""
    K, Tp1 = obs.shape[-1], obs.shape[-2]
    nseq = obs.numel() // (Tp1 * K)
    _ptr(obs); _ptr(mean, numel=K)
    ws = _ws(bufs, "obs_moments", obs.device, (nseq, T, K), lib().rr_obs_moments_workspace_bytes(nseq, T, K), torch.float64)
    sums = torch.empty(2, K, dtype=torch.float64, device=obs.device)
    _check(lib().rr_obs_moments(obs.data_ptr(), nseq, Tp1, T, K, mean.data_ptr(), sums.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream)))
    return sums


def clipped_adam_partials(n: int) -> int:
    """Partial sums the norm of an n-element gradient is formed from (C ABI `rr_clipped_adam_partials`): a function of n alone."""
    return _check(lib().rr_clipped_adam_partials(int(n)))


class ClippedAdamBuffers:
    """Everything one `rr_clipped_adam_step` reads besides the tensors, kept by the caller so that a captured HIP graph sees the same
    addresses for the life of the object: `cfg` (device float64 [8]: lr, b1, b2, eps, max_grad_norm), `state` (device float64 [16]: t, the
    last norm / scale / skip flag / bias corrections and the counters; `training.optim` names the slots), the workspace of the partial sums
    and the tensor table.  `params`: contiguous float32 device tensors in the order of their segments of `grad_flat`; `m_flat` / `v_flat`:
    the moments, laid out as the gradient is.  `step()` launches on the current stream."""

    def __init__(self, params, grad_flat, m_flat, v_flat, *, lr, b1, b2, eps, max_grad_norm, n=None, kl=None, kl_cfg=None):
        self.params, self.grad, self.m, self.v = list(params), grad_flat, m_flat, v_flat
        dev = grad_flat.device
        self.n = int(grad_flat.numel() if n is None else n)
        for t in (grad_flat, m_flat, v_flat):
            _ptr(t)
        self.table = (RRAdamTensor * max(len(self.params), 1))()
        off = 0
        for k, p in enumerate(self.params):
            self.table[k] = RRAdamTensor(_ptr(p), off, p.numel())
            off += p.numel()
        self.cfg = torch.tensor([lr, b1, b2, eps, max_grad_norm, 0.0, 0.0, 0.0], dtype=torch.float64, device=dev)
        self.state = torch.zeros(16, dtype=torch.float64, device=dev)
        self.workspace = torch.empty(max(lib().rr_clipped_adam_workspace_bytes(self.n) // 8, 1), dtype=torch.float64, device=dev)
        # `kl` (one float32 element on the device: the minibatch's approx_kl) and `kl_cfg` (stop threshold, desired_kl, lr_lo, lr_hi; 0 = off):
        # the step goes through `rr_clipped_adam_step_kl`, which decides the target-KL stop and the KL-adaptive learning rate on the device
        self.kl, self.kl_cfg = kl, None
        if kl is not None:
            _ptr(kl, numel=1)
            self.kl_cfg = torch.tensor([float(x) for x in kl_cfg], dtype=torch.float64, device=dev)
            if self.kl_cfg.numel() != 4:
                raise ValueError("ClippedAdamBuffers: kl_cfg is (stop threshold, desired_kl, lr_lo, lr_hi)")

    def step(self):
        if self.kl is not None:
            _check(lib().rr_clipped_adam_step_kl(self.table, len(self.params), self.grad.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.n,
                                                 self.cfg.data_ptr(), self.state.data_ptr(), self.kl.data_ptr(), self.kl_cfg.data_ptr(),
                                                 self.workspace.data_ptr(), C.c_void_p(torch.cuda.current_stream(self.grad.device).cuda_stream)))
            return
        _check(lib().rr_clipped_adam_step(self.table, len(self.params), self.grad.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.n,
                                          self.cfg.data_ptr(), self.state.data_ptr(), self.workspace.data_ptr(),
                                          C.c_void_p(torch.cuda.current_stream(self.grad.device).cuda_stream)))


def policy_sample(logits, noise, min_std: float):
    """(action, raw_action, log_prob) of the tanh-normal policy head in one launch (C ABI `rr_policy_sample`).
    logits [N, 2A], noise [N, A]: contiguous float32 device tensors."""
    N, P2 = logits.shape
    A = P2 // 2
    _ptr(logits); _ptr(noise, numel=N * A)
    action, raw, lp = torch.empty(N, A, device=logits.device), torch.empty(N, A, device=logits.device), torch.empty(N, device=logits.device)
    _check(lib().rr_policy_sample(logits.data_ptr(), noise.data_ptr(), N, A, min_std, action.data_ptr(), raw.data_ptr(), lp.data_ptr(),
                                  C.c_void_p(torch.cuda.current_stream(logits.device).cuda_stream)))
    return action, raw, lp


def policy_backward(grad_logits, head_weight, hidden_weights, pre_act, bias_grads, bufs=None):
    """Delta chain of the policy network's 32-wide hidden stack in one launch (C ABI `rr_policy_backward`).

    grad_logits [M, P], P <= 128; head_weight [P, 32]; hidden_weights: list, entry j >= 1 = W_j [32, 32] (entry 0 ignored); pre_act
    [nh, >= M, 32] (rr_mlp_forward's policy_pre; the first M rows of each layer are overwritten by silu(z)); bias_grads: list of
    nh [32] tensors.  Returns (delta [nh, M, 32], h = pre_act)."""
    nh = pre_act.shape[0]
    M, P = grad_logits.shape
    if pre_act.shape[2] != 32 or pre_act.shape[1] < M or len(bias_grads) != nh or len(hidden_weights) != nh or head_weight.shape != (P, 32):
        raise ValueError("rr_policy_backward: inconsistent shapes")
    _ptr(grad_logits); _ptr(head_weight); _ptr(pre_act)
    for j in range(nh):
        _ptr(bias_grads[j], numel=32)
        if j > 0:
            _ptr(hidden_weights[j], numel=1024)
    dev, bufs = pre_act.device, {} if bufs is None else bufs      # no `bufs`: a fresh delta per call (it is an output)
    ws = _ws(bufs, "policy_bwd", dev, (M, nh), lib().rr_policy_backward_workspace_bytes(M, nh))
    delta = _ws(bufs, "policy_bwd_delta", dev, (M, nh), 0, shape=(nh, M, 32))
    wt = (C.c_void_p * nh)(*[hidden_weights[j].data_ptr() if j > 0 else None for j in range(nh)])
    bg = (C.c_void_p * nh)(*[b.data_ptr() for b in bias_grads])
    _check(lib().rr_policy_backward(grad_logits.data_ptr(), head_weight.data_ptr(), wt, nh, M, P, pre_act.data_ptr(), pre_act.shape[1], delta.data_ptr(), bg,
                                    ws.data_ptr(), ws.numel() * 4, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return delta, pre_act


def policy_act(obs, mean, std, policy, noise, min_std: float, want_logits: bool = False, rows=None):
    """The rollout's actor step in two launches (C ABI `rr_policy_act`): obs [M, K] (or obs[rows]) -> normalise -> policy MLP ->
    tanh-normal head (A <= 64).  noise [M, A] or None (deterministic: action = tanh(loc)).  Returns (action, raw_action | None,
    log_prob | None, logits | None)."""
    M, K = obs.shape
    _ptr(obs)
    if rows is not None:
        M = rows.numel()
        _ptr(rows, torch.int64)
    pn, keep = _mlp_net(*policy)
    A = policy[0][-1].shape[0] // 2
    dev = obs.device
    action = torch.empty(M, A, device=dev)
    raw = lp = logits = None
    if noise is not None:
        _ptr(noise, numel=M * A)
        raw, lp = torch.empty(M, A, device=dev), torch.empty(M, device=dev)
    if want_logits:
        logits = torch.empty(M, 2 * A, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    ws = _ws(None, "policy_act", dev, M, lib().rr_policy_act_workspace_bytes(M))      # per stream: sub-batches on several streams run this concurrently
    _check(lib().rr_policy_act(obs.data_ptr(), _dp(rows), M, K, _ptr(mean, numel=K), _ptr(std, numel=K), C.byref(pn), _dp(noise), min_std, action.data_ptr(),
                               _dp(raw), _dp(lp), _dp(logits), ws.data_ptr(), ws.numel() * 4, C.c_void_p(stream)))
    return action, raw, lp, logits


def mlp_weight_grad_batch(items):
    """Several weight gradients in one call (C ABI `rr_mlp_weight_grad_batch`, at most 12): `items` = dicts with the arguments of
    `mlp_weight_grad` (delta, act, out, and optionally rows, mean, std, delta_colsum).  Products of one tile shape share a launch,
    one reduction launch sums all partial tiles."""
    n = len(items)
    arr = (RRDwItem * n)()
    dev = items[0]["delta"].device
    shape_key = []
    for i, it in enumerate(items):
        delta, act, out = it["delta"], it["act"], it["out"]
        M, O = delta.shape
        I = act.shape[1]
        _ptr(delta); _ptr(act); _ptr(out, numel=O * I)
        rows, mean, std, cs = it.get("rows"), it.get("mean"), it.get("std"), it.get("delta_colsum")
        if rows is not None:
            _ptr(rows, torch.int64, M)
        elif act.shape[0] < M:
            raise ValueError("rr_mlp_weight_grad_batch: fewer activation rows than delta rows")
        arr[i] = RRDwItem(delta.data_ptr(), act.data_ptr(), _dp(rows), _ptr(mean, numel=I), _ptr(std, numel=I),
                          _ptr(cs, numel=O) if mean is not None else None, M, O, I, out.data_ptr())
        shape_key.append((M, O, I))
    ws = _ws(None, "weight_grad_batch", dev, tuple(shape_key), lib().rr_mlp_weight_grad_batch_workspace_bytes(arr, n))
    _check(lib().rr_mlp_weight_grad_batch(arr, n, ws.data_ptr(), ws.numel() * 4, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
