/* rodent_rr.h -- C ABI of librodent_hip.so: the MI355X-native replacement for the one hot path of
 * talmolab/Brax-Rodent-Run, the batched `Rodent.step()` / `pipeline_step` physics
 * [REF Rodent_Env_Brax.py:87 pipeline_init, :101 pipeline_step, :98-136 step, :138-158 _get_obs].
 *
 * In the reference that path is `PipelineEnv.pipeline_init/pipeline_step` dispatching to the backend
 * module pair `brax.mjx.pipeline.init(sys,q,qd,act,ctrl)` / `step(sys,state,act)` (selected by
 * `backend='mjx'` [REF Rodent_Env_Brax.py:58]).  This header is what a ctypes/cffi binding of a fifth
 * backend would bind (INTEGRATION.md shows the stub).
 *
 * Conventions
 *  - Every `float*` / `int32_t*` data argument is a CALLER-OWNED DEVICE pointer (e.g. torch tensor
 *    storage on the batch's HIP device), env-major row-major `[num_envs][width]`, valid until the
 *    work enqueued on the batch's stream has completed.  Nothing is copied to the host.
 *  - All work is enqueued asynchronously on the `hipStream_t` given at rr_batch_create.
 *  - Return value: 0 on success, negative rr_status on error; message via rr_last_error()
 *    (thread-local).  No exceptions cross the ABI; no abort().
 *  - rr_model is immutable and may be shared by batches on several devices; an rr_batch is not
 *    thread-safe.  The library keeps no per-env state: all state lives in the caller's buffers.
 */
#ifndef RODENT_RR_H
#define RODENT_RR_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rr_model rr_model;
typedef struct rr_batch rr_batch;

enum rr_status { RR_OK = 0, RR_EINVAL = -1, RR_EIO = -2, RR_EHIP = -3, RR_EUNSUPPORTED = -4 };

/* model dimensions (what `sys.nq/nv/nu`, obs size etc. are in the reference) */
typedef struct rr_dims {
  int32_t nq, nv, nu, na, nbody, njnt, ngeom, nM, ncon, nlimit, nefc, obs_dim;
  int32_t iterations, ls_iterations; /* opt.iterations / opt.ls_iterations [REF Rodent_Env_Brax.py:46-47] */
  int32_t lds_bytes;                 /* dynamic LDS one environment (= one wavefront) uses */
  int32_t dbg_floats;                /* floats per env of the debug dump (rr_debug_layout) */
  float timestep;
  int32_t solver;                    /* 1 = CG, 2 = Newton (mjtSolver; opt.solver [REF Rodent_Env_Brax.py:42-45]) */
  int32_t fixed_instance;            /* 1: stepped by a kernel instance compiled for these dimensions; 0: the generic instance (same results, slower) */
} rr_dims;

/* physics state of the batch: what survives between `pipeline_step` calls (mjx.Data qpos, qvel, act,
 * qacc_warmstart).  All in/out, [N][nq], [N][nv], [N][na], [N][nv]. */
typedef struct rr_state {
  float* qpos;
  float* qvel;
  float* act;
  float* qacc_warmstart;
} rr_state;

/* optional per-step outputs read by the reference env (`data.cinert, data.cvel, data.qfrc_actuator,
 * data.xmat, data.xpos` [REF Rodent_Env_Brax.py:151-155,161]); any pointer may be NULL.
 * Values are those of the LAST forward pass (before the last integration), as in mjx.step. */
typedef struct rr_outputs {
  float* cinert;        /* [N][nbody*10] */
  float* cvel;          /* [N][nbody*6]  */
  float* qfrc_actuator; /* [N][nv]       */
  float* xpos;          /* [N][nbody*3]  */
  float* xmat;          /* [N][nbody*9]  */
  float* subtree_com;   /* [N][3]  (root 0) */
  float* debug;         /* [N][dims.dbg_floats], see rr_debug_layout; NULL in production */
  /* contact geometry of the last forward pass (mjx.Data.contact.{dist,pos,frame}; brax State.contact
   * [NB mjcf.ipynb:917-921]); the integer fields geom1 / geom2 / link_idx are static: rr_model_table.
   * Models with candidate-pair contacts (rodent_cpu.xml): ncon is the number of candidate pairs and every pair has its entry, in
   * penetration or not, as in MJX -- the values of the very pair_geometry evaluation whose sign selects the pairs that take a slot.
   * `debug` and these three are served by the debug-dump instance, single-step launches only (rr_pipeline_step, rr_env_step,
   * rr_env_reset); the multi-step forms, the profile build and the Newton solver refuse them. */
  float* contact_dist;  /* [N][ncon]   */
  float* contact_pos;   /* [N][ncon*3] */
  float* contact_frame; /* [N][ncon*9]: rows normal, tangent 1, tangent 2 */
} rr_outputs;

/* reference-env epilogue fused into the step kernel [REF Rodent_Env_Brax.py:98-136]; all NULL = physics only */
typedef struct rr_env_io {
  const float* track_pos; /* [T][3] device; with `clip` set: [num_clips][T][3] */
  int32_t track_len;      /* T */
  int32_t* cur_frame;     /* [N] in/out: info['cur_frame'] */
  float* obs;             /* [N][obs_dim] out */
  float* reward;          /* [N] out */
  float* done;            /* [N] out */
  float* metrics;         /* [N][3] out: pos_reward, reward_quadctrl, reward_alive */
  float healthy_reward, ctrl_cost_weight, healthy_z_min, healthy_z_max;
  int32_t terminate_when_unhealthy;
  /* Bad-state check (MuJoCo's mj_checkPos / mj_checkVel; mjMAXVAL = 1e10), 0 = off (a zero-initialised struct keeps the unchecked
   * behaviour); negative or NaN: RR_EINVAL.  After an env step -- once per step, on the state after the last substep, never at reset and
   * never in rr_pipeline_step -- env e is BAD iff some element x of its qpos or qvel fails fabsf(x) <= bad_state_max, so NaN and +-inf
   * are bad.  That step then writes done = 1 (whatever terminate_when_unhealthy is), reward = 0 and the three metrics = 0, and adds 1
   * to the batch's counter (rr_batch_bad_states).  The state and the observation of the bad step are NOT sanitised. */
  float bad_state_max;
  /* Multi-clip tracking, NULL = one clip (a zero-initialised struct keeps the single-clip behaviour and num_clips is not read).  With
   * `clip` set, track_pos is [num_clips][track_len][3] and env e tracks clip clip[e]: its reward reads track_pos[clip[e]][old_frame], its
   * observation track_pos[clip[e]][new_frame + 1], both frames clamped into [0, track_len - 1] WITHIN the clip.  The kernel clamps
   * clip[e] into [0, num_clips - 1]; num_clips < 1 with clip set: RR_EINVAL.  Every launch form and rr_env_reset honour it; the ids are
   * only read (a wrapped form's restore leaves them alone, as it leaves cur_frame). */
  const int32_t* clip;    /* [N] device, nullable */
  int32_t num_clips;      /* C */
} rr_env_io;

/* -- model ------------------------------------------------------------------------------------- */
/* Load a compiled model blob ('RRM1', written by rodent_amd.mjcf.save_blob).  Replaces
 * mujoco.MjModel.from_xml_path + brax.io.mjcf.load_model -> mjx.put_model [REF Rodent_Env_Brax.py:41,51]. */
int rr_model_load(const char* blob_path, rr_model** out);
int rr_model_dims(const rr_model* m, rr_dims* out);
/* opt.iterations / opt.ls_iterations override [REF Rodent_Env_Brax.py:46-47] (before rr_batch_create) */
int rr_model_set_solver(rr_model* m, int32_t iterations, int32_t ls_iterations);
/* opt.solver = {'cg': 1, 'newton': 2} [REF Rodent_Env_Brax.py:42-45] (before rr_batch_create).  Newton: H = M + J' diag(D active) J
 * has M's tree sparsity for these models and runs through the same factorisation schedules in a second LDS array (csrc/rr_kernel.h
 * newton_hessian); available for the single-rodent models (RR_EUNSUPPORTED otherwise); ~40 KB of LDS per environment. */
int rr_model_set_solver_type(rr_model* m, int32_t solver);
void rr_model_destroy(rr_model* m);
/* Static model tables as the LOADED model holds them (the integer ids the reference exposes through `sys` / `Contact`:
 * "con_geom1", "con_geom2" = Contact.geom1 / geom2 [NB mjcf.ipynb:917-921], "con_body1", "con_body2" (+1 of brax's
 * contact.link_idx), "geom_bodyid", "dof_bodyid", "dof_parentid", "body_parentid", "jnt_qposadr", "jnt_dofadr",
 * "actuator_dofadr", ... -- any entry of the blob by its MuJoCo field name).  Returns a borrowed HOST pointer valid for
 * the model's lifetime; *dtype: 0 = float32, 1 = int32; *count = number of elements.  RR_EINVAL for an unknown name. */
int rr_model_table(const rr_model* m, const char* name, const void** host_ptr, size_t* count, int32_t* dtype);

/* -- batch ------------------------------------------------------------------------------------- */
/* Upload the model tables to `hip_device` and bind `hip_stream` (a hipStream_t, may be NULL = default). */
int rr_batch_create(const rr_model* m, int32_t num_envs, int32_t hip_device, void* hip_stream, rr_batch** out);
void rr_batch_destroy(rr_batch* b);

/* brax.mjx.pipeline.init(sys, q, qd) = make_data + mjx.forward [REF Rodent_Env_Brax.py:87].
 * Reads st->qpos/qvel/act (act normally zero), writes st->qacc_warmstart and the outputs. */
int rr_pipeline_init(rr_batch* b, const rr_state* st, const rr_outputs* out);

/* brax.mjx.pipeline.step(sys, state, act) x n_frames [REF Rodent_Env_Brax.py:101, :53-57]:
 * ctrl [N][nu] is held over the n_frames substeps; st is updated in place. */
int rr_pipeline_step(rr_batch* b, const rr_state* st, const float* ctrl, int32_t n_frames, const rr_outputs* out);

/* Rodent.step fused: pipeline_step + reward/done/obs/metrics + cur_frame increment
 * [REF Rodent_Env_Brax.py:98-136]. `action` plays the role of ctrl. */
int rr_env_step(rr_batch* b, const rr_state* st, const float* action, int32_t n_frames, const rr_env_io* env,
                const rr_outputs* out);

/* With env->bad_state_max > 0 a bad env (see rr_env_io) leaves rr_env_step / rr_env_step_to flagged by done = 1 with reward and metrics 0,
 * but its qpos / qvel / obs are returned as they are (possibly non-finite): the caller -- AutoReset, rr_wrap_episode_autoreset -- restores. */
/* Out-of-place variants: read the state from `in` (and info['cur_frame'] from `cur_frame_in`), write the stepped state to
 * `out_state` (and env->cur_frame).  brax states are immutable values [REF Rodent_Env_Brax.py:98-136 returns a new State]:
 * a caller that keeps the previous state (rollout buffers, AutoReset's first state) needs no copies.  `in` and
 * `out_state` may alias field by field (then it is the in-place call). */
int rr_pipeline_step_to(rr_batch* b, const rr_state* in, const rr_state* out_state, const float* ctrl, int32_t n_frames,
                        const rr_outputs* out);
int rr_env_step_to(rr_batch* b, const rr_state* in, const rr_state* out_state, const float* action, int32_t n_frames,
                   const rr_env_io* env, const int32_t* cur_frame_in, const rr_outputs* out);

/* A multi-step rollout in ONE launch: num_steps x [Rodent.step, then EpisodeWrapper + AutoResetWrapper with action_repeat 1] --
 * the `lax.scan` over env.step of brax.training.acting.generate_unroll / a jitted random-action rollout [UP; REF
 * brax_rodent_run_ppo.py:141-151].  actions [num_steps][N][nu].  The environments of the launch do not wait for each other between
 * steps and the state stays on chip; results are those of num_steps calls of rr_env_step_to + rr_wrap_episode_autoreset, bit for
 * bit.  `in` / `out_state` / `env` / `cur_frame_in` as rr_env_step_to (obs, reward, done, metrics, cur_frame of the LAST step are
 * written); `wrap`: the stored first state and first observation (restored where an episode ends), the wrappers' state before the
 * launch (prev_done, steps_in [N]) and after it (steps_out, truncation_out [N]; the final done goes to env->done).
 * Production instance only (no rr_outputs).  Models with a multi-step instance (CG solver): the single-rodent floor-contact models
 * (rodent_optimized / rodent_new and any model of their slot counts) and the candidate-pair models (rodent_cpu.xml:
 * self-collisions, tendon transmissions).  RR_EUNSUPPORTED for the Newton solver and for models of other slot counts (rodent_pair.xml);
 * rr_batch_unroll_supported tells.
 * Bad-state check (env->bad_state_max > 0): a bad step counts as a finished episode with done_env = 1 -- truncation 0, and the stored first
 * state and first observation come back, so nothing non-finite survives the step; cur_frame and steps behave as at any other done. */
/* Models whose contact list is a list of candidate pairs (contacts between two moving bodies, e.g. rodent_cpu.xml [REF models/rodent_cpu.xml]):
 * the kernel keeps the pairs in penetration in 64 contact slots per environment; pairs beyond that are DROPPED for that substep.  *events = the
 * number of (environment, step) events in which that happened since the batch was created, a step being one launch of rr_pipeline_step /
 * rr_env_step (all its n_frames substeps) or ONE of the num_steps env steps of rr_env_unroll / rr_env_unroll_policy: a multi-step launch
 * adds exactly what the same steps as single launches add.  Synchronises the batch's stream.  Always 0 for the floor-contact models,
 * whose every contact has its own slot. */
int rr_batch_contact_overflow(rr_batch* b, int64_t* events);
/* *events = the number of (environment, env step) events in which the bad-state check (rr_env_io::bad_state_max) found a bad env since the
 * batch was created, counted like the events above: one launch of rr_env_step is one step, a multi-step launch adds exactly what the same
 * steps as single launches add.  The counter is owned by the batch.  Always 0 while the check is off.  Synchronises the batch's stream. */
int rr_batch_bad_states(rr_batch* b, int64_t* events);

/* 1 when this batch's model / solver has a multi-step kernel instance (with_actor != 0: the one with the actor inside), else 0. */
int rr_batch_unroll_supported(const rr_batch* b, int32_t with_actor);
typedef struct rr_unroll_io {
  rr_state first;
  const float* first_obs;
  const float* prev_done;
  const float* steps_in;
  float* steps_out;
  float* truncation_out;
  float episode_length;
} rr_unroll_io;
int rr_env_unroll(rr_batch* b, const rr_state* in, const rr_state* out_state, const float* actions, int32_t num_steps, int32_t n_frames,
                  const rr_env_io* env, const int32_t* cur_frame_in, const rr_unroll_io* wrap);

/* rr_env_unroll with the actor inside: brax.training.acting.generate_unroll -- num_steps x [policy(obs) -> sample -> wrapped env
 * step], transitions recorded -- in ONE launch [UP acting.generate_unroll / actor_step; SURVEY.md a22, a23].  Per env and step the
 * wave evaluates the policy MLP (obs -> 32 x nhidden -> 2A, SiLU; optional normaliser) on the observation of that step, samples
 * the tanh-normal action with the given noise, steps, applies the wrappers, and writes the transition into the learner's trajectory
 * arrays: traj_obs [N][T+1][obs] (row t = observation of step t, row T = the bootstrap observation), traj_raw_action [N][T][A],
 * traj_log_prob / traj_reward / traj_discount (= 1 - done) / traj_truncation [N][T] (with segment_length L < T: U = T / L such
 * blocks one after the other -- a whole rollout phase of U unrolls in one launch); actions_out [T][N][A] receives tanh(raw).
 * Weights: w0 [32][obs] and b0 [32] as torch holds them; hidden_wt[l-1] (l = 1 .. nhidden-1) TRANSPOSED [32 in][32 out];
 * head_wt TRANSPOSED (column j = logit j: columns 0 .. A-1 the location logits, A .. 2A-1 the scale logits) and zero-padded, head_b
 * padded alike, in one of TWO layouts chosen by the model's action count A = nu: A <= 32: head_wt [32][64], head_b [64] (one pass of
 * the wave over the head); 32 < A <= 64: head_wt [32][128], head_b [128] (two passes; rodent_cpu.xml, A = 38).  The kernel reads the
 * whole padded width, so the arrays must have it.  A > 64: RR_EUNSUPPORTED.  noise [T][N][A] standard normal draws.
 * The final observation is traj_obs[:, T] (env->obs is not written).  Instances for the models rr_env_unroll serves
 * (rr_batch_unroll_supported(b, 1)).
 * Bad-state check: at a bad transition traj_reward = 0, traj_discount = 0 (no bootstrap from the bad step), traj_truncation = 0, and the next
 * observation row is the stored first observation. */
typedef struct rr_actor_io {
  const float* obs_in; const float* mean; const float* std;
  const float* w0; const float* b0;
  const float* hidden_wt[4]; const float* hidden_b[4];
  const float* head_wt; const float* head_b;
  const float* noise;
  float* actions_out;
  float* traj_obs; float* traj_raw_action; float* traj_log_prob; float* traj_reward; float* traj_discount; float* traj_truncation;
  float min_std;
  int32_t nhidden;
  int32_t segment_length;   /* L: num_steps = U * L consecutive steps recorded as U trajectories, the traj_* arrays are [U][N][L(+1)][...]
                             * and the last observation row of a segment is repeated as row 0 of the next; 0 = one segment (L = num_steps) */
} rr_actor_io;
int rr_env_unroll_policy(rr_batch* b, const rr_state* in, const rr_state* out_state, int32_t num_steps, int32_t n_frames, const rr_env_io* env,
                         const int32_t* cur_frame_in, const rr_unroll_io* wrap, const rr_actor_io* actor);

/* Evaluation in ONE launch: rr_env_unroll_policy without the trajectory, in the two forms a training run evaluates in.
 * WRAPPED (raw_env = 0) is brax.training.acting.Evaluator's unroll -- num_steps x [policy(obs) -> action -> Rodent.step -> EpisodeWrapper
 * + AutoResetWrapper -> EvalWrapper]: per env step, after the wrappers and before the restore of a finished episode,
 *   episode_steps += active;  sum_k += metric_k * active for k = pos_reward, reward_quadctrl, reward_alive, reward;  active *= 1 - done
 * on eval_metrics [N][6] = (episode_steps, active_episodes, the four sums), read and written in place, so launches chain (nullable:
 * no bookkeeping).  RAW (raw_env = 1) is the launcher's evaluation rollout [REF brax_rodent_run_ppo.py:141-151], a loop over the
 * unwrapped env.step: no step count, no truncation, no restore -- the env keeps stepping past `done`; `wrap` may then be NULL.
 * `actor` as for rr_env_unroll_policy, except: noise may be NULL (the deterministic policy, action = tanh(loc); equal bit for bit to an
 * all-zero noise array), actions_out [num_steps][N][A] may be NULL (not recorded) and the traj_* members and segment_length are ignored.
 * obs_ring [N][2][obs]: the only observation storage of the launch -- step t reads row t & 1 and writes row (t + 1) & 1, so the final
 * observation of env e is obs_ring[e][num_steps & 1] (env->obs is not written).  qpos_out (nullable) [num_steps + 1][N][nq]: row 0 the
 * incoming qpos, row t + 1 the qpos after step t (wrapped form: before a restore).  Everything else (final state, reward / done /
 * metrics / cur_frame of the last step, steps_out / truncation_out in the wrapped form) as rr_env_unroll.
 * Instances: the models rr_env_unroll_policy serves, CG solver.  RR_EUNSUPPORTED (rr_last_error says why) for the Newton solver, two-tree
 * models served by the two-wave pair instance, other slot counts, batches that carry per-env parameters (rr_batch_set_env_params),
 * observations wider than 1280, more than 64 actions and diagnostic batches; those evaluate step by step.  rr_batch_eval_supported: 1 / 0.
 * Bad-state check: a bad step adds zeros to the sums and ends the episode (active *= 0).  The WRAPPED form restores the first state; the
 * RAW form has no restore, so it flags the env by done = 1, counts the event and goes on stepping the bad state as it is. */
typedef struct rr_eval_io {
  float* eval_metrics;
  float* obs_ring;
  float* qpos_out;
  int32_t raw_env;
} rr_eval_io;
int rr_batch_eval_supported(const rr_batch* b);
int rr_env_unroll_eval(rr_batch* b, const rr_state* in, const rr_state* out_state, int32_t num_steps, int32_t n_frames, const rr_env_io* env,
                       const int32_t* cur_frame_in, const rr_unroll_io* wrap, const rr_actor_io* actor, const rr_eval_io* eval);

/* obs of Rodent.reset: after rr_pipeline_init, obs = _get_obs(data, 0, cur_frame) [REF :89];
 * implemented as rr_pipeline_init + obs epilogue in one launch. Only env->obs/track_pos/cur_frame are used,
 * and env->clip/num_clips where set (the observation holds track_pos[clip[e]][cur_frame + 1]). */
int rr_env_reset(rr_batch* b, const rr_state* st, const rr_env_io* env, const rr_outputs* out);

/* Pose tracking: the env step also rewards the clip's root orientation and joint angles.  The block is set on the BATCH (rr_env_io is
 * closed: its layout ends with the clip members) and read by every later env step of it -- rr_env_step(_to), rr_env_unroll and
 * rr_env_unroll_policy -- until it is replaced or cleared; a launch takes the pointers as they are when it is issued, so the caller may
 * hand a fresh pose_metrics array before each launch.  NULL, or both pointers NULL: off, the position-only reward (a batch starts that way).
 * track_pose is [T][nq - 3] -- with rr_env_io::clip set [num_clips][T][nq - 3] -- one row per frame: the clip's root quaternion
 * (w, x, y, z; unit length) then its nq - 7 joint angles, with the launch's track_len / clip / num_clips, indexed like track_pos.  An env
 * step (never a reset) reads the row of the clip and frame its position reward reads and, with q = qpos[3:7] and j = qpos[7:nq] of the
 * stepped state, r_q and r_j the row's two parts:
 *   d = conj(r_q) (x) q,   theta = 2 atan2(|d.xyz|, |d.w|)      (the sign and the scale of q do not matter)
 *   quat_reward  = quat_reward_weight  * exp(-quat_reward_scale  * theta^2)
 *   joint_reward = joint_reward_weight * exp(-joint_reward_scale * sum_i (j_i - r_j,i)^2)
 *   reward = (reward without pose + quat_reward) + joint_reward       (float32, rounded in that order)
 * pose_metrics[e] = (quat_reward, joint_reward); a bad step (bad_state_max) zeroes both.  done, cur_frame, obs and metrics are what they
 * are without pose; in rr_env_unroll_policy traj_reward holds the new total.  rr_env_reset ignores the block.
 * rr_batch_set_pose: one pointer without the other, or a negative or non-finite weight or scale: RR_EINVAL.  RR_EUNSUPPORTED with the
 * reason where the batch has no pose instance -- there are some for the CG solver on the single-rodent floor-contact models (fixed-dimension
 * or generic (2,2,1) slot counts) with shared tables: none for the Newton solver, models with candidate-pair contacts, two-tree models
 * served by the two-wave pair instance and batches that carry per-env parameters (rr_batch_set_env_params refuses in turn while a pose
 * block is set).  With a block set, rr_env_unroll_eval and launches with a debug dump, contact-geometry outputs or the profile build
 * refuse (RR_EUNSUPPORTED).  rr_batch_pose_supported: 1 / 0, with 0 rr_last_error holds the reason. */
typedef struct rr_pose_io {
  const float* track_pose;
  float* pose_metrics;    /* [N][2] out */
  float quat_reward_weight, quat_reward_scale, joint_reward_weight, joint_reward_scale;
} rr_pose_io;
int rr_batch_set_pose(rr_batch* b, const rr_pose_io* pose);
int rr_batch_pose_supported(const rr_batch* b);

/* Reference observation: the policy sees what the pose reward scores.  rr_batch_set_reference_obs(b, H), H = 1 .. 16, on a batch whose
 * pose block is set (rr_batch_set_pose; rr_env_io and rr_pose_io are closed, so the count rides on the batch like the block) makes every
 * observation row of the batch
 *   [ the model's observation (obs_dim) | block_1 | ... | block_H ],   rr_batch_obs_width(b) = obs_dim + H * nq entries,
 * written wherever an observation is written -- by rr_env_reset, which then reads the pose block too, and by every env step of
 * rr_env_step(_to), rr_env_unroll and rr_env_unroll_policy, a bad step included.  EVERY array this header documents as [obs] wide is
 * rr_batch_obs_width(b) wide on such a batch: rr_env_io::obs, rr_unroll_io::first_obs, rr_actor_io::traj_obs, obs_in, mean, std and the
 * rows of w0 (the library cannot check the callers' lengths).  H = 0 (a batch starts that way): the width is obs_dim and nothing changes.
 * block_h = (p_h[3], q_h[4], j_h[nq - 7]) reads frame f_h = clamp(frame + h, 0, track_len - 1) of the env's clip (the id clamped as
 * everywhere), `frame` being the frame the observation's track entry counts from: the stepped cur_frame after a step, cur_frame at a
 * reset.  With x the world quaternion of body 1 (whose matrix is the xmat[1] of the track entry) and (r_q, r_j) track_pose's row:
 *   p_h = xmat[1] @ (track_pos[f_h] - qpos[:3])        p_1 equals the last three entries of the model's observation bit for bit
 *   q_h = s * (conj(x) (x) r_q),  s = -1 where that product's w is negative, else +1 (so q_h.w >= 0); float32, every product and sum
 *         rounded on its own:  w = ((xw rw + xx rx) + xy ry) + xz rz,  x = ((xw rx - xx rw) - xy rz) + xz ry,
 *                              y = ((xw ry + xx rz) - xy rw) - xz rx,  z = ((xw rz - xx ry) + xy rx) - xz rw
 *   j_h = r_j - qpos[7:nq]                             one float32 subtraction per entry
 * Under the AutoReset wrapper of the multi-step forms the stored first observation comes back verbatim at the full width.
 * rr_batch_set_reference_obs: frames outside 0 .. 16, or frames > 0 without a pose block: RR_EINVAL; RR_EUNSUPPORTED with the reason
 * wherever pose tracking is unsupported.  While frames > 0, rr_batch_set_pose(b, NULL) is RR_EINVAL (set the frames to 0 first) and
 * rr_env_unroll_eval refuses (no evaluation instance writes the blocks; evaluate step by step).  The in-kernel actor of these instances
 * reads 26 entries per lane, a row of at most 1664: rr_env_unroll_policy refuses a wider one (RR_EUNSUPPORTED) -- on the shipped
 * floor-contact models (obs_dim 1279 / 1263, nq 74) that is H <= 5 -- while the forms without the actor serve every H.
 * rr_batch_reference_obs_supported(b, frames, with_actor): 1 / 0 -- whether the batch serves that many frames (with_actor != 0: also in
 * rr_env_unroll_policy); with 0 rr_last_error holds the reason.  It does not need the pose block to be set. */
int rr_batch_set_reference_obs(rr_batch* b, int32_t frames);
int32_t rr_batch_obs_width(const rr_batch* b);
int rr_batch_reference_obs_supported(const rr_batch* b, int32_t frames, int32_t with_actor);

/* Pose termination: an env step whose pose has strayed from the clip ends the episode.  The block is set on the BATCH, next to the pose
 * block it needs (rr_env_io and rr_pose_io are closed), and read by every later env step of it -- rr_env_step(_to), rr_env_unroll and
 * rr_env_unroll_policy -- until it is replaced or cleared (NULL; a batch starts without one); a launch takes `fail` as it is when it is
 * issued.  An env step (never a reset) compares the stepped qpos with the row of the clip and frame its position and pose rewards read:
 *   e_pos   = |qpos[:3] - track_pos[c][f]|_2
 *   e_quat  = theta of rr_pose_io               (2 atan2(|d.xyz|, |d.w|), d = conj(r_q) (x) q)
 *   e_joint = sqrt(sum_i (qpos[7+i] - r_j,i)^2)
 *   code = 1 (e_pos > max_pos) | 2 (e_quat > max_quat) | 4 (e_joint > max_joint);   fail[e] = (float)code;   done = max(done, code != 0)
 * +INFINITY switches a criterion off (x > inf is false); a NaN error sets no bit (bad_state_max ends such a step).  The failing step
 * changes nothing but done: reward, metrics, pose_metrics, cur_frame, obs and the state are what they are without the block, and the
 * rule does not ask terminate_when_unhealthy.  A bad step stores code 0 next to its done = 1.  In the multi-step forms the code enters
 * the env's done before the Episode and AutoReset wrappers: a pose failure is a termination -- truncation 0, traj_discount 0, the first
 * state and first observation restored -- and steps_out counts from there.  rr_env_reset ignores the block.
 * rr_batch_set_pose_termination: no pose block on the batch (rr_batch_set_pose first), a NULL fail, or a threshold that is NaN or <= 0:
 * RR_EINVAL; RR_EUNSUPPORTED with the reason wherever pose tracking is unsupported.  While the block is set, rr_batch_set_pose(b, NULL)
 * is RR_EINVAL (clear this block first), and what refuses a pose block refuses here: rr_env_unroll_eval, per-env parameters, the debug
 * dump, contact-geometry outputs and the profile build.  The env steps run the reference-observation instances' code whatever the frame
 * count (0 .. 16), so rr_env_unroll_policy serves rows of up to 1664 entries.
 * rr_batch_pose_termination_supported(b, with_actor): 1 / 0 -- whether the batch serves the block with its current frame count
 * (with_actor != 0: also in rr_env_unroll_policy); with 0 rr_last_error holds the reason.  It does not need the pose block to be set. */
typedef struct rr_pose_term_io {
  float* fail;            /* [N] out: the code as a float, 0 .. 7 */
  float max_pos, max_quat, max_joint;
  int32_t pad;
} rr_pose_term_io;
int rr_batch_set_pose_termination(rr_batch* b, const rr_pose_term_io* term);
int rr_batch_pose_termination_supported(const rr_batch* b, int32_t with_actor);

/* Body tracking: the reward also scores the clip's body positions, and a sharper term its end effectors.  The block is set on the BATCH,
 * next to the pose block it needs (rr_env_io, rr_pose_io and rr_pose_term_io are closed), and read by every later env step of it --
 * rr_env_step(_to), rr_env_unroll and rr_env_unroll_policy -- until it is replaced or cleared (NULL; a batch starts without one); a
 * launch takes the pointers as they are when it is issued.  track_bodies is [T][nbody][3] (with clip ids [num_clips][T][nbody][3]),
 * global body-frame origins, indexed like track_pose; body_weights is [2][nbody] floats, row 0 the 0 / 1 mask of the tracked bodies B,
 * row 1 that of the end effectors E (entry 0, the world, is not read).  An env step (never a reset) forms, with xpos the body positions
 * of its last forward pass -- what rr_outputs.xpos returns: the pose before the last substep's integration -- and r the row of the clip
 * and frame its position and pose rewards read:
 *   S_B = sum_{b in B} |xpos[b] - r[b]|^2,   S_E = the same over E
 *   body_reward   = body_reward_weight   exp(-body_reward_scale   S_B)
 *   endeff_reward = endeff_reward_weight exp(-endeff_reward_scale S_E)
 *   reward = (((plain + quat_reward) + joint_reward) + body_reward) + endeff_reward;   body_metrics[e] = (body_reward, endeff_reward)
 * every product and sum rounded to float32 on its own.  done, cur_frame, obs, the state, metrics, pose_metrics and pose_fail are what they
 * are without the block; a bad step (bad_state_max) zeroes body_metrics with the others.  rr_env_reset ignores the block.
 * rr_batch_set_body_tracking: no pose block on the batch (rr_batch_set_pose first), a NULL pointer, or a weight or scale that is negative
 * or not finite: RR_EINVAL; RR_EUNSUPPORTED with the reason wherever pose tracking is unsupported.  While the block is set,
 * rr_batch_set_pose(b, NULL) is RR_EINVAL (clear this block first), and what refuses a pose block refuses here: rr_env_unroll_eval,
 * per-env parameters, the debug dump, contact-geometry outputs and the profile build.  The env steps run the reference-observation
 * instances' code whatever the frame count (0 .. 16), so rr_env_unroll_policy serves rows of up to 1664 entries; a pose-termination
 * block may stand next to this one or not.
 * rr_batch_body_tracking_supported(b, with_actor): 1 / 0 -- whether the batch serves the block with its current frame count
 * (with_actor != 0: also in rr_env_unroll_policy); with 0 rr_last_error holds the reason.  It does not need the pose block to be set. */
typedef struct rr_body_io {
  const float* track_bodies;   /* [(C)][T][nbody][3] */
  const float* body_weights;   /* [2][nbody]: row 0 the mask of B, row 1 that of E */
  float* body_metrics;         /* [N][2] out: (body_reward, endeff_reward) */
  float body_reward_weight, body_reward_scale, endeff_reward_weight, endeff_reward_scale;
} rr_body_io;
int rr_batch_set_body_tracking(rr_batch* b, const rr_body_io* body);
int rr_batch_body_tracking_supported(const rr_batch* b, int32_t with_actor);

/* Clip restarts: a restarted episode rejoins its clip at a drawn frame.  Upstream's AutoReset brings back the first state and the first
 * observation and leaves info -- cur_frame -- alone; a tracking env then compares the restored pose with frames it never started at.  With
 * this block set on the BATCH (next to the pose block it needs; the structs above are closed) the multi-step launches -- rr_env_unroll and
 * rr_env_unroll_policy; single steps have no restore in the kernel and ignore the block -- read rr_unroll_io::first and first_obs as a
 * BANK of K = num_slots start states, [K][N][width] each ([K][N][rr_batch_obs_width] for first_obs), `frames` [K][N] the frame each entry
 * was formed at and slot_in [N] the entry each env restored last (0 after a reset).  Per wrapped env step, with done_env the env's own done
 * (pose failure and bad state included), new_frame = old_frame + 1 and T = rr_env_io::track_len:
 *   steps' = (prev_done ? 0 : steps) + 1
 *   over   = steps' >= episode_length  ||  (end_at_clip_end && new_frame >= T - 1)
 *   done   = over ? 1 : done_env;   truncation = over ? 1 - done_env : 0
 *   done:  slot' = (slot + 1) mod K;  state, obs <- bank[slot'];  cur_frame <- frames[slot'];     else slot' = slot, cur_frame = new_frame
 * new_frame >= T - 1: the new state's observation has no next frame left to read without clamping; the clip's end is a truncation like
 * episode_length.  The step that ends the episode is untouched: reward, metrics, pose_fail and the trajectory read old_frame as without the
 * block.  env->cur_frame and slot_out [N] receive the frame and the slot after the launch's last step, so launches chain.  A launch takes
 * the pointers as they are when it is issued.  num_slots = 1: the frame comes back with the one stored state.
 * rr_batch_set_clip_restarts: NULL clears (a batch starts without one); num_slots outside 1 .. 64, a NULL pointer, or no pose block on the
 * batch (rr_batch_set_pose first): RR_EINVAL; RR_EUNSUPPORTED with the reason wherever pose tracking is unsupported.  While the block is
 * set, rr_batch_set_pose(b, NULL) is RR_EINVAL (clear this block first) and rr_env_unroll_eval refuses, as for any pose block.  The
 * launches run the reference-observation instances' code whatever the frame count, so rr_env_unroll_policy serves rows of up to 1664
 * entries; pose-termination and body-tracking blocks may stand next to this one or not.
 * rr_batch_clip_restarts_supported(b, with_actor): 1 / 0 -- whether rr_env_unroll (with_actor != 0: rr_env_unroll_policy) serves the block
 * on this batch at its current frame count; with 0 rr_last_error holds the reason.  It does not need the pose block to be set. */
typedef struct rr_clip_restart_io {
  const int32_t* frames;       /* [K][N]: the start frame of each bank entry */
  const int32_t* slot_in;      /* [N] */
  int32_t* slot_out;           /* [N] out */
  int32_t num_slots;           /* K: 1 .. 64 */
  int32_t end_at_clip_end;     /* != 0: the clip's end truncates the episode */
} rr_clip_restart_io;
int rr_batch_set_clip_restarts(rr_batch* b, const rr_clip_restart_io* restart);
int rr_batch_clip_restarts_supported(const rr_batch* b, int32_t with_actor);

/* Velocity tracking: the reward also scores the clip's velocities, so a policy that holds the right pose at the wrong speed no longer
 * earns full reward.  The block is set on the BATCH, next to the pose block it needs (the structs above are closed), and read by every
 * later env step of it -- rr_env_step(_to), rr_env_unroll and rr_env_unroll_policy -- until it is replaced or cleared (NULL; a batch
 * starts without one); a launch takes the pointers as they are when it is issued.  track_vel is [T][nv] (with clip ids
 * [num_clips][T][nv]), indexed like track_pose, a row in qvel layout: the world-frame linear velocity of the free joint [3], the angular
 * velocity in the root's own frame [3], the joint velocities [nv - 6].  An env step (never a reset) forms, with d = qvel - r on the
 * stepped qvel and r the row of the clip and frame its position and pose rewards read:
 *   S_lin = sum d[0:3]^2,   S_ang = sum d[3:6]^2,   S_joint = sum d[6:]^2
 *   lin_vel_reward   = lin_weight   exp(-lin_scale   S_lin)
 *   ang_vel_reward   = ang_weight   exp(-ang_scale   S_ang)
 *   joint_vel_reward = joint_weight exp(-joint_scale S_joint)
 *   reward = ((r_0 + lin_vel_reward) + ang_vel_reward) + joint_vel_reward;   vel_metrics[e] = the three terms
 * r_0 the reward with the pose terms (and the body terms where the batch carries that block); every product and sum rounded to float32
 * on its own.  done, cur_frame, obs, the state, metrics, pose_metrics, pose_fail and body_metrics are what they are without the block; a
 * bad step (bad_state_max) zeroes vel_metrics with the others.  rr_env_reset ignores the block.
 * rr_batch_set_velocity_tracking: no pose block on the batch (rr_batch_set_pose first), a NULL pointer, or a weight or scale that is
 * negative or not finite: RR_EINVAL; RR_EUNSUPPORTED with the reason wherever pose tracking is unsupported.  While the block is set,
 * rr_batch_set_pose(b, NULL) is RR_EINVAL (clear this block first), and what refuses a pose block refuses here: rr_env_unroll_eval,
 * per-env parameters, the debug dump, contact-geometry outputs and the profile build.  The env steps run the body-tracking instances
 * whatever else the batch carries, so rr_env_unroll_policy serves rows of up to 1664 entries.
 * rr_batch_velocity_tracking_supported(b, with_actor): 1 / 0 -- whether the batch serves the block with its current frame count
 * (with_actor != 0: also in rr_env_unroll_policy); with 0 rr_last_error holds the reason.  It does not need the pose block to be set. */
typedef struct rr_vel_io {
  const float* track_vel;      /* [(C)][T][nv] */
  float* vel_metrics;          /* [N][3] out: (lin_vel_reward, ang_vel_reward, joint_vel_reward) */
  float lin_weight, lin_scale, ang_weight, ang_scale, joint_weight, joint_scale;
} rr_vel_io;
int rr_batch_set_velocity_tracking(rr_batch* b, const rr_vel_io* vel);
int rr_batch_velocity_tracking_supported(const rr_batch* b, int32_t with_actor);

/* Clip library: clips keep their own length, and a restarted episode may move to another clip.  The block is set on the BATCH, next to
 * the pose block it needs (the structs above are closed), and read by every later env launch of it until it is replaced or cleared
 * (NULL; a batch starts without one); a launch takes the pointers as they are when it is issued.
 * clip_lengths [num_clips] (one entry for an env io without clip ids): clip c consists of rows 0 .. L_c - 1 of track_pos, track_pose,
 * track_bodies and track_vel, L_c = clip_lengths[c] clamped into 1 .. track_len; the rows behind them are padding that no launch reads
 * (the row stride stays track_len).  Wherever an env on clip c clamps a frame into 0 .. track_len - 1 without the block -- the position
 * reward's row, the observation's track entry (frame + 1), the reference blocks (frame + h), the pose reward and pose-termination row,
 * the body rows, the velocity rows -- it clamps into 0 .. L_c - 1, and end_at_clip_end of rr_clip_restart_io becomes new_frame >=
 * L_c - 1.  Env steps read it, and the resets of a batch with reference frames; a reset without them reads frame + 1 unclamped by the
 * clip, so the caller starts every env at a frame <= L_c - 2.  NULL: every clip has track_len frames.
 * bank_clips [num_slots][N] (needs a clip-restart block and env io clip ids): the clip of each bank entry.  rr_clip_restart_io's rule
 * gains one line,
 *   done:  clip <- bank_clips[slot'] (clamped into 0 .. num_clips - 1);   else the clip the env is on,
 * in rr_env_unroll and rr_env_unroll_policy: the launch reads the env io's clip [N] once, every step reads the rows of the clip the
 * env is on, and clip_out [N] receives the clip each env is on after the last step (the env io's clip is left alone; the two may not
 * alias).  Single steps (rr_env_step(_to)) have no restore in the kernel: rr_wrap_clip_library below.  NULL: every entry on the env's
 * clip.
 * Nothing else of a step changes: with lengths equal to track_len and every bank entry on the env's clip the results are those without
 * the block, bit for bit.
 * rr_batch_set_clip_library: no pose block on the batch, both pointers NULL, bank_clips without a clip-restart block or without
 * clip_out: RR_EINVAL; RR_EUNSUPPORTED with the reason wherever pose tracking is unsupported.  While the block is set,
 * rr_batch_set_pose(b, NULL) is RR_EINVAL, and with bank_clips so is rr_batch_set_clip_restarts(b, NULL): clear this block first.  What
 * refuses a pose block refuses here: rr_env_unroll_eval, per-env parameters, the debug dump, contact-geometry outputs and the profile
 * build.  The env steps of a batch with the block run the body-tracking instances (the restart instances in the multi-step forms with a
 * clip-restart block) whatever else the batch carries.
 * rr_batch_clip_library_supported(b, with_actor): 1 / 0 -- whether the batch serves the block with its current frame count (with_actor
 * != 0: also in rr_env_unroll_policy); with 0 rr_last_error holds the reason.  It does not need the pose block to be set. */
typedef struct rr_clip_library_io {
  const int32_t* clip_lengths;  /* [C] or NULL: every clip has T frames */
  const int32_t* bank_clips;    /* [K][N] or NULL: every bank entry on the env's clip */
  int32_t* clip_out;            /* [N] out; required with bank_clips: the clip each env is on after a multi-step launch */
} rr_clip_library_io;
int rr_batch_set_clip_library(rr_batch* b, const rr_clip_library_io* lib);
int rr_batch_clip_library_supported(const rr_batch* b, int32_t with_actor);

/* Clip sampling: per-clip outcome counters, and restores that draw their bank entry by per-clip weights.  The block is set on the BATCH,
 * next to the clip-restart block it needs, and read by every later rr_env_unroll / rr_env_unroll_policy of it until it is replaced or
 * cleared (NULL; a batch starts without one); a launch takes the pointers as they are when it is issued, and reads the tables' CONTENT
 * when it runs, so weights rewritten in place reach the next launch (and a replayed graph).  Integers only: the composed wrappers, the
 * per-step wrapper below and the multi-step launches agree bit for bit.  With done_env, over, done as in rr_clip_restart_io's rule and c
 * the clip the step was made on (before any restore; 0 without clip ids):
 * outcomes [num_clips][5] int64, added to and never cleared by a launch:
 *   col 4 += 1 for every wrapped step made on c;
 *   done:  col 0 += 1, and exactly one of
 *          col 1 += 1   the step's pose-termination code is nonzero,
 *          col 2 += 1   else done_env (unhealthy, bad state),
 *          col 3 += 1   else (over alone: a truncation by episode_length or the clip's end),
 * so columns 1 + 2 + 3 = column 0.  A launch adds an episode segment's steps in one atomic add at the segment's end (the episode's end
 * or the launch's last step); totals after whole launches do not depend on how the steps were split into launches.  NULL: no counting.
 * clip_weights [num_clips] int32, entries 0 .. 65535 (the low 16 bits are read), needs a clip-library block with bank_clips:
 *   q_k = clip_weights[clamp(bank_clips[k][env], 0, num_clips - 1)], k = 0 .. num_slots - 1;   S = sum q_k;
 *   h = fmix32(fmix32(seed ^ (uint32(env) * 0x9E3779B1)) + uint32(n)), fmix32 = MurmurHash3's finaliser (h ^= h >> 16; h *= 0x85EBCA6B;
 *       h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16, mod 2^32), n = the env's restore count;
 *   r = (uint64(h) * S) >> 32;   done:  slot' = the smallest k with q_0 + .. + q_k > r;   S == 0:  slot' = (slot + 1) mod num_slots.
 * A slot whose clip has weight 0 is never drawn while S > 0; slot' == slot is allowed.  State, observation, frame and clip then come
 * from entry slot' as before.  n = draws_in[env] at the launch's first step, grows by one at every restore (drawn or cyclic) and goes to
 * draws_out[env] after the last step, as slot_out does (the two may not alias).  NULL: the cyclic rule.
 * rr_batch_set_clip_sampling: no clip-restart block on the batch, clip_weights and outcomes both NULL, clip_weights without a
 * clip-library block with bank_clips or without draws_in / draws_out: RR_EINVAL; RR_EUNSUPPORTED with the reason wherever pose tracking
 * is unsupported.  While the block is set, rr_batch_set_clip_restarts(b, NULL) is RR_EINVAL, and with clip_weights so is clearing
 * bank_clips (rr_batch_set_clip_library): clear this block first.  No new instance: the launches run the restart instances they ran;
 * single steps (rr_env_step(_to)) ignore the block: rr_wrap_clip_sampling below.
 * rr_batch_clip_sampling_supported(b, with_actor): 1 / 0 as for the other blocks; with 0 rr_last_error holds the reason. */
typedef struct rr_clip_sampling_io {
  const int32_t* clip_weights;  /* [C], 0 .. 65535, or NULL: the cyclic rule */
  const int32_t* draws_in;      /* [N] restores of each env so far; required with clip_weights */
  int32_t* draws_out;           /* [N] out; required with clip_weights */
  int64_t* outcomes;            /* [C][5] or NULL: no counting */
  uint32_t seed;
} rr_clip_sampling_io;
int rr_batch_set_clip_sampling(rr_batch* b, const rr_clip_sampling_io* sampling);
int rr_batch_clip_sampling_supported(const rr_batch* b, int32_t with_actor);

/* Reference restarts: a restore of rr_env_unroll / rr_env_unroll_policy that reads NO bank entry but draws a clip and a start frame,
 * builds the start state from the clip's rows plus noise and forms its observation by a forward-only pass inside the launch (what
 * rr_env_reset computes for that state, not counted as a step).  Set on the BATCH next to the pose and clip-restart blocks it needs,
 * like the blocks above; NULL clears it.  Integer hashing only, no float transcendental.  With n = draws_in[env] before the restore
 * (it grows by one per restore and goes to draws_out[env] after the launch's last step; these replace the clip-sampling block's pair),
 *   base = fmix32(fmix32(seed ^ (uint32(env) * 0x9E3779B1)) + n);   h(p, i) = fmix32(base ^ (((p << 16) | i) * 0x9E3779B1))   (mod 2^32)
 *   clip:   across_clips and clip ids given: over all num_clips clips -- with clip_weights of sum S > 0 the smallest c with
 *           q_0 + .. + q_c > (uint64(h(1, 0)) * S) >> 32 (a clip of weight 0 is never drawn), else (uint64(h(1, 0)) * num_clips) >> 32;
 *           otherwise the clip the env is on.  num_clips <= 65536.
 *   frame:  d = frame_lo + ((uint64(h(2, 0)) * (frame_hi - frame_lo)) >> 32);  f = d mod (L_c - 1) with per-clip lengths (clip library),
 *           else d;  the rows are read at clamp(f, 0, L_c - 1): none at or behind the clip's end.
 *   state:  qpos = [track_pos[c][f], track_pose[c][f]], qvel = track_vel[c][f] with a velocity block, else 0; to element i of qpos is added
 *           noise_scale * s(h(3, i)), to element i of qvel noise_scale * s(h(4, i)), s(h) = (h >> 8) * 2^-23 - 1 (exact in float32), one
 *           rounded product and one rounded sum.  act = 0, qacc_warmstart = 0 going into the pass.  cur_frame <- f, clip <- c (clip_out
 *           of the clip library).  The slot advances cyclically and selects nothing; the bank's arrays are not read.
 * rr_batch_set_reference_restart: no pose block or no clip-restart block on the batch, NULL draws_in / draws_out or the two aliased,
 * frame_lo < 0 or frame_hi <= frame_lo, a noise_scale that is negative or not finite: RR_EINVAL; RR_EUNSUPPORTED with the reason where
 * there is no restart instance (as rr_batch_set_clip_restarts).  The launches run the restart instances; single steps ignore the block
 * (the per-step wrappers restore through rr_env_reset).  rr_batch_reference_restart_supported(b, with_actor): 1 / 0 as for the others. */
typedef struct rr_reference_restart_io {
  const int32_t* clip_weights;  /* [C], 0 .. 65535, or NULL: the uniform draw */
  const int32_t* draws_in;      /* [N] restores of each env so far */
  int32_t* draws_out;           /* [N] out */
  uint32_t seed;
  int32_t frame_lo, frame_hi;   /* frames are drawn in [frame_lo, frame_hi) */
  int32_t across_clips;         /* != 0: a restore draws its clip over the whole library */
  float noise_scale;
  int32_t pad;
} rr_reference_restart_io;
int rr_batch_set_reference_restart(rr_batch* b, const rr_reference_restart_io* r);
int rr_batch_reference_restart_supported(const rr_batch* b, int32_t with_actor);

/* Generalised advantage estimation of one PPO minibatch, the reverse scan of brax.training.agents.ppo.losses.compute_gae
 * [UP; SURVEY.md Appendix E], one thread per trajectory.  All arrays time-major [T][B] device float32; bootstrap [B];
 * outputs vs [T][B] and advantages [T][B].  `stream` is a hipStream_t (NULL = default stream). */
int rr_compute_gae(const float* truncation, const float* termination, const float* rewards, const float* values,
                   const float* bootstrap_value, int32_t T, int32_t B, float lambda_, float discount, float* vs,
                   float* advantages, void* stream);

/* Fused actor / critic MLP forward on the f32 matrix cores (v_mfma_f32_32x32x2_f32 / 16x16x4_f32; csrc/rr_mlp.h): what
 * `ppo.networks.make_inference_fn` (normalise, policy MLP) and the forward half of `ppo.losses.compute_ppo_loss` (policy and
 * value MLP on the same observations) compute [UP brax.training; REF brax_rodent_run_ppo.py:97-114], for
 * the `make_ppo_networks` default shapes: policy obs -> 32 x (nlayers-1) -> out (<= 128; more than 64
 * logits run as two passes over column halves of 64), value obs -> 256 x (nlayers-1) -> 1,
 * SiLU on hidden layers, float32 throughout.  A network is described by HOST arrays of DEVICE pointers: weights[l] is
 * [sizes[l+1]][sizes[l]] row-major (torch.nn.Linear.weight), biases[l] is [sizes[l+1]]; sizes has nlayers + 1 entries.
 * Either network may be NULL (skipped).  obs_rows (device int64 [M], nullable): sample m is row obs_rows[m] of `obs` (a minibatch
 * addressed inside the unroll buffer, no gathered copy).  mean / std (device, [K]) may both be NULL (no normalisation), else
 * x <- (x - mean) / std.  Outputs: policy_out [M][sizes[nlayers]], value_out [M]; optional PRE-activation dumps of the
 * hidden layers (for a backward pass): policy_pre [nlayers-1][M][32], value_pre [nlayers-1][M][256] (NULL = not written).
 * A policy whose hidden layers are ALL 256 wide (1 .. 7 of them, head 1 .. 128 logits) is taken too: it runs as a launch of its own
 * next to the value network's (the same launch whether or not `value` is given, so a row's logits do not depend on the call's other
 * arguments or row count), policy_pre is then [nlayers-1][M][256], and its backward pass is rr_mlp_policy_backward.  rr_policy_act,
 * rr_policy_backward and the in-kernel actor of rr_env_unroll_policy stay 32-wide only.
 * RR_EUNSUPPORTED for other shapes (mixed hidden widths or widths other than 32 / 256 included). */
typedef struct rr_mlp_net {
  const float* const* weights;
  const float* const* biases;
  const int32_t* sizes;
  int32_t nlayers;
} rr_mlp_net;
int rr_mlp_forward(const float* obs, const int64_t* obs_rows, int32_t M, int32_t K, const float* mean, const float* std, const rr_mlp_net* policy,
                   const rr_mlp_net* value, float* policy_out, float* value_out, float* policy_pre, float* value_pre, void* stream);


/* The loss half of `brax.training.agents.ppo.losses.compute_ppo_loss` [UP; REF
 * brax_rodent_run_ppo.py:97-114] and its gradient with respect to the network outputs, in three launches without atomics
 * (csrc/rr_ppo.h): truncation-aware GAE, device-local advantage normalisation (population std + 1e-8), tanh-normal log-prob
 * (scale = softplus + min_std), clipped surrogate, value loss 0.25 mean((vs - v)^2), entropy estimated with one normal draw
 * per action dimension.  Inputs (device float32): policy_logits [(T+1)*B][2A] and values [(T+1)*B], the networks' outputs on
 * the gathered minibatch, TIME-major (row t*B + b; rows T*B.. belong to the bootstrap observation); the batch leaves
 * raw_action [R][T][A], log_prob / reward / discount / truncation [R][T] batch-major as collected, addressed through idx [B]
 * (int64 rows of the minibatch; NULL = rows 0..B-1); noise [T*B][A] standard normal draws.  Outputs: grad_logits
 * [(T+1)*B][2A] and grad_values [(T+1)*B] (d total_loss / d output; bootstrap rows zero), metrics[4] = total_loss,
 * policy_loss, v_loss, entropy_loss.  workspace: rr_ppo_loss_workspace_bytes(T, B) bytes of device memory, 8-byte aligned. */
typedef struct rr_ppo_cfg {
  float entropy_cost, discounting, reward_scaling, gae_lambda, clipping_epsilon, min_std;
  int32_t normalize_advantage;
} rr_ppo_cfg;
size_t rr_ppo_loss_workspace_bytes(int32_t T, int32_t B);
int rr_ppo_loss(const float* policy_logits, const float* values, const float* raw_action, const float* log_prob, const float* reward,
                const float* discount, const float* truncation, const int64_t* idx, const float* noise, int32_t T, int32_t B, int32_t A,
                const rr_ppo_cfg* cfg, float* grad_logits, float* grad_values, float* metrics, void* workspace, size_t workspace_bytes,
                void* stream);
/* rr_ppo_loss with the learner's diagnostics (the DIAG instances of the loss and metrics kernels; gradients and metrics[4] are bitwise
 * rr_ppo_loss's).  Five more block sums, fixed order, no atomics, give per minibatch
 *   approx_kl          = mean(expm1(d) - d), d = log_prob_new - log_prob_behaviour in float32, the term in double (k3 estimator, >= 0)
 *   clip_fraction      = share of samples with rho outside [1 - eps, 1 + eps]
 *   explained_variance = 1 - Var(vs - v) / Var(vs), population variances from double sums; 0 where Var(vs) == 0
 *   entropy            = mean sampled entropy
 * diag: device double [16], 8-byte aligned, written by one thread with plain stores: [0..3] the four figures of this minibatch in that
 *   order; accumulators since the caller last cleared them: [8] minibatches, [9] sum of approx_kl, [10] largest approx_kl, [11] sum of
 *   clip_fraction, [12] sum of explained_variance, [13] sum of entropy.  A replayed graph keeps adding to them.
 * kl_out: device float, nullable: approx_kl rounded to float32 once -- the input of rr_clipped_adam_step_kl (the first slot behind the
 *   parameters in the flat gradient buffer, so that the ranks' all-reduce averages it with the gradients).
 * workspace: rr_ppo_loss_diag_workspace_bytes(T, B) bytes, 8-byte aligned. */
size_t rr_ppo_loss_diag_workspace_bytes(int32_t T, int32_t B);
int rr_ppo_loss_diag(const float* policy_logits, const float* values, const float* raw_action, const float* log_prob, const float* reward,
                     const float* discount, const float* truncation, const int64_t* idx, const float* noise, int32_t T, int32_t B, int32_t A,
                     const rr_ppo_cfg* cfg, float* grad_logits, float* grad_values, float* metrics, double* diag, float* kl_out,
                     void* workspace, size_t workspace_bytes, void* stream);

/* The rollout's actor step, acting.actor_step -> make_inference_fn [UP; SURVEY.md a22], in two launches: observations (optionally
 * through obs_rows, optionally normalised by mean / std) -> policy network (as rr_mlp_forward takes it: 32-wide hidden layers,
 * head 2 x action_size <= 128; an odd or wider head: RR_EUNSUPPORTED) -> tanh-normal head.  noise [M][A] standard normal draws: raw_action = loc + (softplus(scale) + min_std)
 * * noise, action = tanh(raw_action), log_prob [M]; noise NULL: the deterministic policy, action = tanh(loc).  raw_action, log_prob,
 * logits [M][2A] are optional outputs (NULL = not written).  The first layer is split over the observation width across
 * workgroups (the batch alone is 64 row tiles for 256 CUs).  workspace: rr_policy_act_workspace_bytes(M) bytes of device memory. */
size_t rr_policy_act_workspace_bytes(int32_t M);
int rr_policy_act(const float* obs, const int64_t* obs_rows, int32_t M, int32_t K, const float* mean, const float* std,
                  const rr_mlp_net* policy, const float* noise, float min_std, float* action, float* raw_action, float* log_prob,
                  float* logits, void* workspace, size_t workspace_bytes, void* stream);

/* The actor's head on the rollout path, `NormalTanhDistribution` of brax.training.distribution as acting.actor_step uses it [UP;
 * SURVEY.md a22]: logits [N][2A] = (loc | pre-softplus scale), noise [N][A] standard normal draws ->
 * raw_action = loc + (softplus(scale) + min_std) * noise, action = tanh(raw_action), log_prob [N] of raw_action under the
 * distribution (Normal log-density minus the tanh log-det-Jacobian, summed over the action dimensions).  One launch. */
int rr_policy_sample(const float* logits, const float* noise, int32_t N, int32_t A, float min_std, float* action, float* raw_action,
                     float* log_prob, void* stream);

/* Backward pass of the policy network's hidden stack (32-wide SiLU layers) in one launch: delta_{nh-1} = (g W_head) *
 * silu'(z_{nh-1}), delta_{j-1} = (delta_j W_j) * silu'(z_{j-1}).  grad_logits [M][P] (P <= 128; wider: RR_EUNSUPPORTED) = d loss / d logits; head_weight
 * [P][32]; hidden_weights: HOST array of nhidden device pointers, entry j (1 <= j < nhidden) = W_j [32 out][32 in]
 * (torch.nn.Linear.weight), entry 0 unused; pre_act [nhidden][pre_act_rows >= M][32] = rr_mlp_forward's policy_pre, rows 0..M-1 of
 * each layer overwritten by silu(z) (a minibatch may carry bootstrap rows, which have no policy gradient, behind the M used ones);
 * delta [nhidden][M][32] out; bias_grads: HOST array of nhidden device pointers, db_j [32] (fixed-order sums).  The weight
 * gradients (rr_mlp_weight_grad on these outputs) stay with the caller. */
size_t rr_policy_backward_workspace_bytes(int32_t M, int32_t nhidden);
int rr_policy_backward(const float* grad_logits, const float* head_weight, const float* const* hidden_weights, int32_t nhidden, int32_t M,
                       int32_t P, float* pre_act, int32_t pre_act_rows, float* delta, float* const* bias_grads, void* workspace,
                       size_t workspace_bytes, void* stream);

/* Elementwise half of the backward pass of one hidden SiLU layer of the networks above (the matrix products stay with the
 * caller): with g = delta_l W_l [M][H] and the layer's pre-activations z [M][H] (rr_mlp_forward's dumps),
 * delta = g * silu'(z), h = silu(z) (the operand of dW_l = delta_l' h) and bias_grad[n] = sum_m delta[m][n], in one pass
 * (plus a fixed-order column reduction; no atomics).  `delta` may alias `g` and `h` may alias `z`.  H must divide 256.
 * workspace: rr_mlp_silu_backward_workspace_bytes(M, H) bytes of device memory. */
size_t rr_mlp_silu_backward_workspace_bytes(int32_t M, int32_t H);
int rr_mlp_silu_backward(const float* g, const float* z, int32_t M, int32_t H, float* delta, float* h, float* bias_grad,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Backward pass of the value network's hidden stack (256-wide SiLU layers, as rr_mlp_forward takes them) on the f32 matrix
 * cores: delta_{nh-1} = g w_head * silu'(z_{nh-1}), delta_{j-1} = (delta_j W_j) * silu'(z_{j-1}) with the delta tile resident in
 * LDS between layers.  grad_value [M] = d loss / d value; head_weight [256]; hidden_weights_t: HOST array of nhidden device
 * pointers, entry j (1 <= j < nhidden) = W_j TRANSPOSED ([in][out] row-major), entry 0 unused; pre_act [nhidden][M][256] =
 * rr_mlp_forward's value_pre, overwritten by silu(z) (the operands h_j of dW_{j+1} = delta_{j+1}' h_j); delta [nhidden][M][256]
 * out; bias_grads: HOST array of nhidden device pointers, db_j [256] = column sums of delta_j (fixed-order reduction).  The
 * weight gradients are matrix products of these outputs (dW_0 = delta_0' x) and stay with the caller. */
size_t rr_mlp_value_backward_workspace_bytes(int32_t M, int32_t nhidden);
int rr_mlp_value_backward(const float* grad_value, const float* head_weight, const float* const* hidden_weights_t, int32_t nhidden,
                          int32_t M, float* pre_act, float* delta, float* const* bias_grads, void* workspace, size_t workspace_bytes,
                          void* stream);

/* Backward pass of a 256-wide policy network's hidden stack (as rr_mlp_forward takes it), the value network's chain with a product at
 * the head: delta_{nh-1} = (G W_head) * silu'(z_{nh-1}), delta_{j-1} = (delta_j W_j) * silu'(z_{j-1}).  grad_logits [n][P] (1 <= P <= 128;
 * else RR_EUNSUPPORTED) = d loss / d logits of the first n <= M rows; head_weight_t [256][P] = the head's weight TRANSPOSED;
 * hidden_weights_t as for rr_mlp_value_backward; nhidden 1 .. 7 (else RR_EUNSUPPORTED); pre_act [nhidden][M][256] = rr_mlp_forward's
 * policy_pre, rows 0 .. n-1 of each layer overwritten by silu(z), rows n .. M-1 (a minibatch's bootstrap rows, which carry no policy
 * gradient) neither read nor written; delta [nhidden][n][256] out; bias_grads: HOST array of nhidden device pointers, db_j [256]
 * (fixed-order sums).  The weight gradients (rr_mlp_weight_grad_batch on these outputs; dW_head = grad_logits' h_{nh-1}) stay with the
 * caller.  workspace: rr_mlp_policy_backward_workspace_bytes(n, nhidden) bytes of device memory. */
size_t rr_mlp_policy_backward_workspace_bytes(int32_t n, int32_t nhidden);
int rr_mlp_policy_backward(const float* grad_logits, const float* head_weight_t, const float* const* hidden_weights_t, int32_t nhidden,
                           int32_t n, int32_t M, int32_t P, float* pre_act, float* delta, float* const* bias_grads, void* workspace,
                           size_t workspace_bytes, void* stream);

/* Weight gradient of one layer, grad[o][i] = sum_m delta[m][o] * x[m][i], on the f32 matrix cores with the row range split
 * over workgroups (the output is small, the reduction ~2e4 rows long) and a fixed-order sum of the partial tiles.  delta
 * [M][O]; act: the layer's input, [M][I] (h = silu(z)) -- or, for the first layer, the RAW observations with act_rows [M]
 * (int64, nullable) = the row of sample m inside `act` (the minibatch addressed in place, no gathered copy) and mean / std
 * [I] (nullable, together with delta_colsum [O] = sum_m delta[m][o], the layer's bias gradient) for x = (act - mean) / std,
 * applied to the sum: grad = (delta' act - delta_colsum mean') / std.  grad [O][I] row-major (torch.nn.Linear.weight.grad).
 * workspace: rr_mlp_weight_grad_workspace_bytes(M, O, I) bytes of device memory. */
size_t rr_mlp_weight_grad_workspace_bytes(int32_t M, int32_t O, int32_t I);
int rr_mlp_weight_grad(const float* delta, const float* act, const int64_t* act_rows, const float* mean, const float* std,
                       const float* delta_colsum, int32_t M, int32_t O, int32_t I, float* grad, void* workspace, size_t workspace_bytes,
                       void* stream);

/* Several weight gradients in one call (up to 12: the eleven layers of the two networks): the products of one tile shape share
 * a launch (item = grid z) and all partial tiles are summed by ONE reduction launch -- 4 launches instead of 22 per minibatch.
 * Items as rr_mlp_weight_grad's arguments. */
typedef struct rr_dw_item {
  const float* delta; const float* act; const int64_t* act_rows; const float* mean; const float* std; const float* delta_colsum;
  int32_t M, O, I;
  float* grad;
} rr_dw_item;
size_t rr_mlp_weight_grad_batch_workspace_bytes(const rr_dw_item* items, int32_t n);
int rr_mlp_weight_grad_batch(const rr_dw_item* items, int32_t n, void* workspace, size_t workspace_bytes, void* stream);

/* The sums of the observation normaliser's update, brax.training.acme.running_statistics.update [UP; SURVEY.md a24, Appendix E;
 * normalize_observations=True in REF brax_rodent_run_ppo.py:103], in one pass over the transitions of a training step: per observation
 * column k,  sums[k] = sum_x (x_k - mean_k)  and  sums[K + k] = sum_x (x_k - mean_k)^2  (double), over the rows t < T of every
 * sequence of `obs` [nseq][Tp1][K] (the unroll buffer: row T of a sequence is the bootstrap observation, not a transition; Tp1 = T for
 * a plain [rows][K] batch).  The update then is  mean' = mean + S1 / count',  summed_variance += S2 - (mean' - mean) S1  -- what upstream
 * forms as sum (x - mean)(x - mean') -- with S1, S2 all-reduced over the ranks.  Fixed-order reductions, no atomics.
 * workspace: rr_obs_moments_workspace_bytes(nseq, T, K) bytes of device memory, 8-byte aligned; sums: device double [2 K]. */
size_t rr_obs_moments_workspace_bytes(int64_t nseq, int32_t T, int32_t K);
int rr_obs_moments(const float* obs, int64_t nseq, int32_t Tp1, int32_t T, int32_t K, const float* mean, double* sums, void* workspace,
                   size_t workspace_bytes, void* stream);

/* One optimiser step of optax.chain(optax.clip_by_global_norm(max_grad_norm), optax.adam(lr)) [UP brax.training.agents.ppo.train,
 * `max_grad_norm`] on a flat gradient buffer, three launches, with an update whose norm is not finite skipped (an extension over optax):
 *   norm = float32(sqrt(sum_i g_i^2)), the squares summed in double in an order that depends on n alone (no atomics);
 *   norm not finite: nothing but state[1], state[3] = 1 and state[12] += 1 is written;
 *   s = norm <= max_grad_norm ? 1 : max_grad_norm / norm;  g^ = g where s = 1, else s * g;  t += 1;
 *   m = b1 m + (1 - b1) g^;  v = b2 v + (1 - b2) g^^2;  p -= lr (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps).
 * table: HOST array of `ntensors` (<= 64) entries, the parameter tensors (device float32) in the order of their segments of the flat
 *   buffers: offset[0] = 0, offset[k + 1] = offset[k] + numel[k], sum of numel = n.  It is checked on the host and travels in the kernel
 *   arguments, so a captured graph keeps it; the parameters stay where they are.
 * grad_flat / m_flat / v_flat: device float32 [n], 16-byte aligned; the moments are laid out as the gradient is.
 * cfg_dev: device double [8]: lr, b1, b2, eps, max_grad_norm (inf: never clip), 3 unused.
 * state_dev: device double [16], zero before the first step: [0] t, [1] norm of the last step (pre-clip, float32 value), [2] its s,
 *   [3] 1 if it was skipped, [4] 1 - b1^t, [5] 1 - b2^t (float32 values); statistics since the caller last cleared them: [8] sum of the
 *   applied updates' norms, [9] their largest, [10] applied updates, [11] those with s < 1, [12] skipped updates.  Everything a replay
 *   of a captured graph must see lives here and in cfg_dev, not in the call's arguments.
 * workspace: rr_clipped_adam_workspace_bytes(n) bytes of device memory, 8-byte aligned (the partial sums).
 * rr_clipped_adam_partials(n): how many partial sums the norm of n elements is formed from (a function of n alone; 0 for n <= 0).
 * RR_EINVAL: more than 64 tensors, a null pointer, misaligned buffers, segments that do not follow each other, n different from their sum. */
typedef struct {
  float* param;
  int64_t offset;      /* of the tensor's segment in the flat buffers, in elements */
  int64_t numel;
} rr_adam_tensor;
size_t rr_clipped_adam_workspace_bytes(int64_t n);
int32_t rr_clipped_adam_partials(int64_t n);
int rr_clipped_adam_step(const rr_adam_tensor* table, int32_t ntensors, const float* grad_flat, float* m_flat, float* v_flat, int64_t n,
                         const double* cfg_dev, double* state_dev, void* workspace, void* stream);
/* rr_clipped_adam_step behind two controls driven by the minibatch's approx_kl, decided on the device by the finalisation kernel so that
 * a captured graph replays the decision (the rule: training/optim.py kl_control_rule).  kl_dev: device float, the KL measured before this
 * update.  klcfg_dev: device double [4]: stop threshold (1.5 x target_kl, the factor of Spinning Up and Stable-Baselines3), desired_kl,
 * lr_lo, lr_hi; 0 switches the stop (slot 0) or the schedule (slot 1) off.  In this order:
 *   state[6] != 0 (sticky stop flag; the caller clears it at the start of a training step's learner phase): state[13] += 1, state[3] = 1,
 *     nothing else moves -- not the norm statistics either;
 *   state[7] = kl;  threshold > 0 and not kl <= threshold (a NaN KL too): state[6] = 1, state[3] = 1, state[13] += 1, return;
 *   norm not finite: skipped as in rr_clipped_adam_step, the learning rate is left alone;
 *   desired_kl > 0 (rsl_rl's schedule, in double on cfg_dev[0], before this update): kl > 2 desired: lr = max(lr_lo, lr / 1.5);
 *     0 < kl < desired / 2: lr = min(lr_hi, lr * 1.5);
 *   then the step of rr_clipped_adam_step.
 * The update kernel's blocks return on state[3], which a stop sets as a skip does; parameters, both moments and t keep their bits.
 * cfg_dev is written (slot 0); the layouts of cfg_dev and state_dev are rr_clipped_adam_step's, with state slots 6, 7 and 13 in use. */
int rr_clipped_adam_step_kl(const rr_adam_tensor* table, int32_t ntensors, const float* grad_flat, float* m_flat, float* v_flat, int64_t n,
                            double* cfg_dev, double* state_dev, const float* kl_dev, const double* klcfg_dev, void* workspace, void* stream);

/* brax.envs.wrappers.training.EpisodeWrapper + AutoResetWrapper [UP; SURVEY.md 3.4] after an env step, in one launch:
 * steps' = (prev_done ? 0 : prev_steps) + action_repeat; over = steps' >= episode_length; done <- over ? 1 : done;
 * truncation = over ? 1 - done_env : 0; and for every env with done != 0 the rows of the `narr` (<= 12) arrays `cur[i]`
 * ([N][widths[i]], overwritten in place) are replaced by the rows of `first[i]` (the state stored at reset).  `first`, `cur`,
 * `widths` are HOST arrays of device pointers / ints; everything else is device memory.  `info` is not restored (as upstream). */
int rr_wrap_episode_autoreset(int32_t num_envs, int32_t narr, const float* const* first, float* const* cur, const int32_t* widths,
                              const float* prev_done, const float* prev_steps, float* done, float* steps, float* truncation,
                              float episode_length, float action_repeat, void* stream);
/* The same for an env with clip restarts (rr_clip_restart_io's rule on one env step; the entry above is unchanged): `first[i]` are banks
 * [num_slots][N][widths[i]], cur_frame [N] holds the stepped frame and is finished in place (the bank entry's frame where done),
 * bank_frames [num_slots][N], slot_in / slot_out [N] (they may alias), track_len = T, end_at_clip_end the flag. */
int rr_wrap_clip_restart(int32_t num_envs, int32_t narr, const float* const* first, float* const* cur, const int32_t* widths,
                         const float* prev_done, const float* prev_steps, float* done, float* steps, float* truncation,
                         float episode_length, float action_repeat, int32_t* cur_frame, const int32_t* bank_frames,
                         const int32_t* slot_in, int32_t* slot_out, int32_t num_slots, int32_t track_len, int32_t end_at_clip_end,
                         void* stream);
/* The same with the clip library (rr_clip_library_io's rule on one env step; the entry above is unchanged): rr_wrap_clip_restart's
 * arguments, then clip [N], the clip each env made the step on, finished in place (the bank entry's clip where done; NULL with a NULL
 * bank_clips and at most one clip), bank_clips [num_slots][N] or NULL (every entry on the env's clip), clip_lengths [num_clips] or NULL
 * (every clip has track_len frames): the clip's end is new_frame >= L - 1, L = clip_lengths[clip] clamped into 1 .. track_len.  The
 * ids in clip and bank_clips must lie in 0 .. num_clips - 1 (this entry does not know num_clips). */
int rr_wrap_clip_library(int32_t num_envs, int32_t narr, const float* const* first, float* const* cur, const int32_t* widths,
                         const float* prev_done, const float* prev_steps, float* done, float* steps, float* truncation,
                         float episode_length, float action_repeat, int32_t* cur_frame, const int32_t* bank_frames,
                         const int32_t* slot_in, int32_t* slot_out, int32_t num_slots, int32_t track_len, int32_t end_at_clip_end,
                         int32_t* clip, const int32_t* bank_clips, const int32_t* clip_lengths, void* stream);
/* The same with clip sampling (rr_clip_sampling_io's rule on one env step; the entries above are unchanged): rr_wrap_clip_library's
 * arguments, then num_clips (ids in clip and bank_clips are clamped into 0 .. num_clips - 1), pose_fail [N] or NULL, the
 * pose-termination codes of the step (what rr_pose_term_io's fail received), and the block: the step's outcomes are added at once, and
 * where done the slot is drawn with n = draws_in[env]; draws_out[env] receives n, or n + 1 where done. */
int rr_wrap_clip_sampling(int32_t num_envs, int32_t narr, const float* const* first, float* const* cur, const int32_t* widths,
                          const float* prev_done, const float* prev_steps, float* done, float* steps, float* truncation,
                          float episode_length, float action_repeat, int32_t* cur_frame, const int32_t* bank_frames,
                          const int32_t* slot_in, int32_t* slot_out, int32_t num_slots, int32_t track_len, int32_t end_at_clip_end,
                          int32_t* clip, const int32_t* bank_clips, const int32_t* clip_lengths, int32_t num_clips,
                          const float* pose_fail, const rr_clip_sampling_io* sampling, void* stream);

/* Scheduling of the environments on the GPU (results are unaffected: environments are independent).  `env_map` (device,
 * [N] int32, a permutation of 0..N-1, or NULL = identity): workgroup w steps environment env_map[w]; `cost_cycles` (device,
 * [N] uint32, or NULL): every launch writes a work estimate of environment e (line-search point evaluations, the quantity
 * that separates slow from fast environments; NOT cycles, which depend on the SIMD neighbour) to cost_cycles[e].  With N equal to
 * one resident round (2 waves per SIMD: N = 8 x number of CUs) workgroups w and w + N/2 share a SIMD, and a launch lasts as
 * long as its slowest environment: pairing the costliest environments of the previous step with the cheapest ones shortens
 * it (rodent_amd/envs/base.py: PipelineEnv._rebalance).  Both pointers are read at every later launch of this batch. */
int rr_batch_set_schedule(rr_batch* b, const int32_t* env_map, uint32_t* cost_cycles);

/* Domain randomisation: per-environment model parameters.  Three float tables of the kernel hold the cells people randomise first --
 * `dof_f` [N][nv][16] (cell 0 armature, 1 damping), `act_f` [N][nu][8] (cell 0 gain, 1..3 bias), `con_f` [N][ncon][26] (cell 16
 * friction mu, 17 the contact's effective inverse weight) -- laid out like the model's k_dof_f / k_act_f / k_con_f with a leading
 * environment axis (rodent_amd/ktables.py env_param_tables builds them).  Each pointer is nullable: a null table stays the
 * model's shared one.  The batch copies the data (device memory) into allocations it owns, on its stream, and frees a previous copy;
 * a NULL `p`, or three null pointers, clears the parameters.  From then on every launch of the batch runs the instance that reads
 * environment e's rows [e] (same arithmetic; rr_kernel.h rr_rand_kernel); such a batch refuses the debug dump, the contact-geometry
 * outputs and the profile build.  RR_EUNSUPPORTED (rr_last_error says why) for models with candidate-pair contacts, two-tree
 * models on the two-wave instance, the Newton solver and slot counts other than (2,2,1).  Synchronises the batch's stream. */
typedef struct rr_env_params {
  const float* dof_f;     /* nullable */
  const float* act_f;     /* nullable */
  const float* con_f;     /* nullable */
  int32_t dof_rows, act_rows, con_rows;   /* rows per environment: the model's nv, nu, ncon */
  int32_t num_envs;                       /* the batch's */
} rr_env_params;
int rr_batch_set_env_params(rr_batch* b, const rr_env_params* p);
/* 1 when rr_batch_set_env_params can serve this batch's model / solver, 0 otherwise */
int rr_batch_env_params_supported(const rr_batch* b);

/* Debug dump layout: names[i] begins at float offsets[i] of each env's debug row; returns the field count.
 * Models with candidate-pair contacts keep the shared layout, with the contact sections per CANDIDATE PAIR (ncon pairs): con_dist, con_pos
 * and con_frame of every pair, bit for bit what rr_outputs.contact_* receive; con_D and con_aref (4 rows; a condim-1 pair has one, its
 * other three cells hold 0) of the pairs that hold a contact slot, 0 for every other pair.  Two sections follow kernarg_ok for these models
 * only: pen_count (1: the pairs in penetration BEFORE the clamp to the 64 slots) and slot_pair (64: the pair id held by each slot, -1
 * beyond the count).  Integers are stored as floats (exact: ids are below 2^24). */
int rr_debug_layout(const rr_batch* b, const char*** names, const int32_t** offsets, const int32_t** sizes);

/* Diagnostic, debug-dump launches only (rr_outputs.debug or the contact-geometry outputs): the line search leaves its bracketing loop
 * after an iteration that left the bracket bitwise unchanged, because every later one would repeat it (rr_kernel.h RR_LS_REPEAT_EXIT).
 * enable = 0 makes the debug-dump instance run those iterations anyway, so that a test can compare the two bit for bit; the dump
 * field `ls_iters` holds the bracketing iterations the last substep executed and those the exit left out.  Default 1.  Every other
 * instance always takes the exit and carries no code for this switch. */
int rr_batch_set_ls_repeat_exit(rr_batch* b, int32_t enable);

/* Diagnostic, debug-dump launches only: the solver makes its exit test before it solves for Mgrad = M^-1 grad (Newton: before the Hessian,
 * its factorisation and the solve) and forms the next search direction, evaluates the warm-start candidate at qacc_smooth for its cost
 * alone (no J' f walk over the contacts), and reuses that candidate's constraint rows where it is chosen -- work whose results nothing
 * reads (rr_kernel.h Wave::solve).  enable = 0 makes the debug-dump instance do all of it anyway, in the order the reference has, so that
 * a test can compare the two bit for bit.  The dump field `solver_end` holds, for the last substep, [0] 1 where the context at qacc_smooth
 * was chosen (0: at qacc_warmstart) and [1] how the loop ended: a sum of 1 = iteration cap, 2 = improvement below the tolerance,
 * 4 = gradient below the tolerance.  Default 1.  Every other instance always runs trimmed and carries no code for this switch. */
int rr_batch_set_solver_trim(rr_batch* b, int32_t enable);

/* Diagnostic, debug-dump launches only: the line search forms once per substep what does not change inside it -- the compacted positions
 * of the active constraint rows, their count and their D column (rr_kernel.h RR_LS_STAGE_ONCE).  enable = 0 makes the debug-dump instance
 * form and stage them in every line search, so that a test can compare the two bit for bit.  Default 1.  Every other instance always
 * stages once and carries no code for this switch.  (The once-per-substep load of the solve-job descriptors, RR_JOBS_RESIDENT, has no
 * second path to switch.) */
int rr_batch_set_solver_batch(rr_batch* b, int32_t enable);

/* A/B switch of the production code, for tests: the fixed-dimension instances hold this lane's entries of the inverse factor's M half in
 * registers from the inversion to the end of the substep, and the undamped M^-1 solves multiply from there (rr_kernel.h
 * RR_SOLVE_MAT_RESIDENT).  enable = 0 makes the batch's production single-step launches (rr_pipeline_step, rr_env_step and their _to forms)
 * run the same instance built with the entries left in LDS, so that a test can compare the two bit for bit.  Only for models of the
 * rodent_optimized dimensions with the CG solver (RR_EUNSUPPORTED otherwise); while it is off, multi-step, actor and evaluation launches
 * and every launch that needs another instance (debug dump, contact geometry, profile, per-env parameters, pose tracking) are refused.
 * Default 1. */
int rr_batch_set_solve_resident(rr_batch* b, int32_t enable);
/* RR_OK where rr_batch_set_solve_resident(b, 0) would be accepted on a batch of this model, else its error code with its words in
 * rr_last_error (needs no device). */
int rr_model_solve_resident_switch(const rr_model* m);

/* A/B switch of the production code, for tests: for a model of one tree whose root body holds the only free joint and that has at most
 * two bodies beyond the 64 lanes (rodent_optimized), the fixed-dimension instances run the tree phases with the 64 other bodies in the
 * first body slot and the root alone in the second (rr_kernel.h RR_ROOT_SLOT).  enable = 0 makes the batch's production single-step
 * launches (rr_pipeline_step, rr_env_step and their _to forms) run the same instance built with the plain map body = lane + 64 * slot,
 * so that a test can compare the two bit for bit.  Only for such a model with the CG solver (RR_EUNSUPPORTED otherwise); while it is
 * off, multi-step, actor and evaluation launches and every launch that needs another instance (debug dump, contact geometry, profile,
 * per-env parameters, pose tracking) are refused, and so is a launch with rr_batch_set_solve_resident(b, 0) on the same batch.
 * Default 1. */
int rr_batch_set_root_slot(rr_batch* b, int32_t enable);
/* RR_OK where rr_batch_set_root_slot(b, 0) would be accepted on a batch of this model, else its error code with its words in
 * rr_last_error (needs no device). */
int rr_model_root_slot_switch(const rr_model* m);

/* ms of the most recent step-kernel launches on this batch measured with hipEvents on its stream
 * (enable with rr_batch_set_timing(b,1); each launch is then bracketed by events) */
int rr_batch_set_timing(rr_batch* b, int32_t enable);
int rr_batch_kernel_time(rr_batch* b, double* total_ms, int64_t* launches);

/* Diagnostic only (never in a timed run): route launches to the s_memtime-instrumented build of the kernel, which
 * writes per-phase cycle sums of each env into dev_cycles [N][24] (uint64, device; RR_NPH slots).  Slots 20 and 21 are counts, not cycles:
 * the bracketing iterations the env's line searches executed, and those the repeat exit left out.  NULL switches back. */
int rr_batch_set_profile(rr_batch* b, uint64_t* dev_cycles);

/* Build-consistency probe (tests): byte offset and size of the I/O block inside the step kernel's argument segment as the
 * HOST code assumes them (the kernel re-reads that block through the kernarg segment pointer; tools/kernel_meta.py reads the
 * offsets the device compiler actually assigned from the code object's metadata and tests/test_abi_and_oracle.py compares). */
int rr_kernarg_layout(int32_t* io_offset, int32_t* io_size, int32_t* total_size);

const char* rr_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
