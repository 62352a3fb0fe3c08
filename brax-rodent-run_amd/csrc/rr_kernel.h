// rr_kernel.h -- fused per-environment physics step for gfx950 (MI355X): ONE 64-lane wavefront per
// environment, the whole working set of an environment resident in LDS for all n_frames substeps.
//
// Path replaced: brax.mjx.pipeline.step -> mujoco.mjx.step (kinematics, com_pos, crb, factor_m,
// collision, make_constraint, com_vel, passive, rne, fwd_actuation, fwd_acceleration, CG solve, euler)
// [REF Rodent_Env_Brax.py:101 -> UP mjx; SURVEY.md Appendix A], plus the env epilogue
// [REF Rodent_Env_Brax.py:103-158].
//
// Mapping: lanes run over bodies / dofs / contacts (element e -> lane e%64, slot e/64,
// slot counts are template parameters so per-lane arrays stay in registers).  Kinematic-tree
// recursions are pointer-doubling / DFS-range sweeps; the sparse L'DL factorisation and its explicit
// inverse run as list-scheduled row programs (rodent_amd/levelsched.py), the solves and M*x as balanced per-lane jobs
// (rodent_amd/ktables.py); J*x and J'f are Jacobian-free.  No LDS atomics: every update has one owner
// lane.  Reductions over dofs / rows are DPP wave sums in a fixed order.  Inactive constraint rows
// contribute exactly zero in the reference formulation, so they are skipped.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rr_tanh_normal.h"

#define RR_LANES 64
// debug dump of the candidate-pair models: where pen_count and slot_pair lie, in floats behind kernarg_ok (RRDims carries no offset for
// them; layout() in rr_api.hip appends the two sections in this order and asserts it)
constexpr int RR_DBG_PEN_COUNT = 1, RR_DBG_SLOT_PAIR = 2;
#define RR_DOFI 12   // ints per dof in k_dof_i
#define RR_BODYI 12  // ints per body in k_body_i
#ifndef RR_WIDE
#define RR_WIDE 1
#endif
#ifndef RR_RING
#define RR_RING 6    // table rows of a row program in flight (<= ktables RING = 8, the empty rows behind a program); round 2: 8 (12 / 16: 2-3 % slower);
                     // with the shorter round-3 programs 6 is best under the driver protocol (2: +0.2 %, 3-5: +1.0 %, 6: +1.5 % against 8)
#endif

#define RR_NPH 24    // phases of the diagnostic (s_memtime) build
#ifndef RR_W1                // contacts in penetration from which an environment's waves run at priority 1 / 2 / 3
#define RR_W1 2
#define RR_W2 6
#define RR_W3 12
#endif
#ifndef RR_ENV_PRIO
#define RR_ENV_PRIO 1      // graded wave priority by contacts in penetration (see the kernel body)
#endif
#ifndef RR_FACTOR_PRIO
#define RR_FACTOR_PRIO 1   // top priority during the level schedules
#endif
#ifndef RR_DPP_BLOCK
#define RR_DPP_BLOCK 1     // one s_nop per row-broadcast stage instead of one per value (-0.6 % launch time, bit-identical)
#endif
#ifndef RR_LS_REPEAT_EXIT
#define RR_LS_REPEAT_EXIT 1   // the line search leaves its bracketing loop after an iteration that changed nothing (Wave::linesearch; bit-identical results)
#endif
#ifndef RR_JOBS_RESIDENT
#define RR_JOBS_RESIDENT 1    // the solve-job descriptors are loaded once per substep and held in registers (Wave::jobs_res; bit-identical results)
#endif
#ifndef RR_SOLVE_MAT_RESIDENT
#define RR_SOLVE_MAT_RESIDENT 1   // the M-half inverse-factor entries of this lane's solve jobs are read once per substep and held in registers (Wave::mres_c / mres_r; bit-identical results)
#endif
#ifndef RR_ROOT_SLOT
#define RR_ROOT_SLOT 1        // models of one free-jointed root and <= 66 bodies: the 64 other bodies fill body slot 0, the root stands alone in slot 1 (Wave::ROOT; bit-identical results)
#endif
#ifndef RR_LS_STAGE_ONCE
#define RR_LS_STAGE_ONCE 1    // the line search's compacted row positions and its D values are staged once per substep (Wave::ls_stage; bit-identical results)
#endif
#define RR_MINVAL 1e-15f
#define RR_MINIMP 0.0001f
#define RR_MAXIMP 0.9999f

struct RRDims {
  int nq, nv, nu, nbody, njnt, nM, ncon, dmax, nroot;
  int obs_dim, iterations, ls_iterations, nfac, nround, ninv, lmax, cmax, rmax;
  float dt, gx, gy, gz, tolerance, ls_tolerance, meaninertia;
  // LDS offsets (floats)
  int o_qpos, o_qvel, o_act, o_ctrl, o_xpos, o_xquat, o_cinert, o_cdof, o_cvel,
      o_qLD, o_vec, o_x, o_arm, o_warm, o_qact, o_jlist, lds_floats;
  // Newton instance only (solver == 2): pair arrays of the Hessian and of a copy of M, ancestor-id bytes; 0 otherwise
  int o_H, o_Mp, o_anc, solver;
  // nv_scale: the dof count the solver's tolerances are scaled by (= nv; a PAIR instance runs one replica of nv dofs per wavefront of a
  // 2 nv-dof model).  fac_stride / inv_stride (ints): PAIR instances hold a second copy of each level schedule behind the first, its
  // LDS addresses moved to the second wavefront's region.  lds_bytes_rep: LDS bytes of one replica's region
  int nv_scale, fac_stride, inv_stride, lds_bytes_rep;
  int nalias;      // alias cells (pairs) of the factorisation schedule, at the head of the pose cells (levelsched.py); 0 for the Newton instances
  // debug dump offsets (floats)
  int g_xpos, g_xquat, g_xmat, g_com, g_cinert, g_crb, g_cdof, g_cvel, g_cfrc, g_qM, g_qLD, g_dinv, g_bias, g_passive,
      g_actuator, g_smooth, g_qacc_smooth, g_con_dist, g_con_pos, g_con_frame, g_con_D, g_con_aref, g_lim, g_qacc,
      g_qfrc_constraint, g_misc, g_ls_iters, g_solver_end, g_kaok, dbg_floats;
};

// LDS layout of one environment (float offsets).  One constexpr function serves the host (rr_api.hip layout) and the
// kernel instance compiled for fixed model dimensions.
struct RRLayout {
  int o_qpos, o_qvel, o_act, o_ctrl, o_xpos, o_xquat, o_cinert, o_cdof, o_cvel, o_qLD, o_vec, o_x, o_arm, o_warm, o_qact, o_jlist, lds_floats;
  int o_H, o_Mp, o_anc;
};
constexpr int rr_imax(int a, int b) { return a > b ? a : b; }
constexpr int rr_up4(int n) { return (n + 3) & ~3; }
constexpr RRLayout rr_layout(int nq, int nv, int nu, int nbody, int nM, int ncon, bool newton = false) {
  RRLayout k{};
  int o = 0;
  k.o_qpos = o; o += rr_up4(nq);
  k.o_qvel = o; o += rr_up4(nv + 1);         // cell nv holds 0 (padding of the J*x jobs)
  k.o_act = o; o += rr_up4(nu);
  k.o_ctrl = o; o += rr_up4(nu);
  // pose cells (xpos | xquat) are recycled as the 6*nv scratch of the mass-matrix build and as solver staging
  k.o_xpos = o; o += rr_up4(rr_imax(7 * nbody + 4, 6 * nv));
  k.o_xquat = k.o_xpos + rr_up4(3 * nbody);
  k.o_cinert = o; o += rr_up4(10 * nbody);      // composite inertia accumulates in place
  k.o_cdof = o; o += rr_up4(6 * nv + 6);     // + a zero motion vector for dof id nv (padding of the J*x jobs)
  k.o_cvel = o; o += rr_up4(6 * nbody);
  // sparse-matrix array of PAIRS (M | M + dt*diag(damping), then their factors, then their inverse factors): nM entries,
  // the cells ZERO, ONE, TRASH, MINUS_ONE of the row programs, 16 zero cells padded row jobs read on.  Before the mass
  // matrix is built its first cells hold cacc | cfrc and the sin/cos scratch.
  k.o_qLD = o; o += rr_up4(rr_imax(rr_imax(2 * (nM + 20), 12 * nbody), 2 * nv));
  k.o_vec = o; o += rr_up4(nv + 16);         // vector cells nv.. hold 0 (padding of the job descriptors; padded column steps read on)
  k.o_x = o; o += rr_up4(nv + 16);
  k.o_arm = o; o += rr_up4(2 * nv);
  k.o_warm = o; o += rr_up4(nv);
  k.o_qact = o; o += rr_up4(nv);
  k.o_jlist = o; o += rr_up4(ncon);      // ids of the contacts in penetration, by rank (J*x jobs)
  if (newton) {   // Newton solver: the Hessian H = M + J'DJ has M's tree sparsity (every constraint row lives on ONE ancestor chain),
                  // so it is held, factorised and inverted exactly like M: a second pair array; plus M itself (for M*search)
    k.o_H = o; o += rr_up4(rr_imax(rr_imax(2 * (nM + 20), 12 * nbody), 2 * nv));
    k.o_Mp = o; o += rr_up4(rr_imax(rr_imax(2 * (nM + 20), 12 * nbody), 2 * nv));
    k.o_anc = o; o += rr_up4((nM + 3) / 4 + 1);       // p-th ancestor of dof i at byte Madr[i] + p
  }
  k.lds_floats = o;
  return k;
}

// Dimensions of the benchmark model family (rodent_optimized.xml) as compile-time constants: the instance built on them
// has its loop bounds, bounds checks and LDS addresses as immediates instead of ~40 scalar registers (the generic instance
// spills hundreds of SGPRs to VGPR lanes).  Members of the same name hide the run-time fields of RRDims; everything else
// (solver options, table row counts, debug offsets) stays run-time.  The host selects it only when every constant matches.
template <int NBODY_, int NCON_, int OBS_>
struct RRDimsFixed : RRDims {
  static constexpr int nq = 74, nv = 73, nu = 30, nbody = NBODY_, njnt = 68, nM = 1119, ncon = NCON_, dmax = 35, nroot = 1, obs_dim = OBS_, nround = 6, lmax = 12, cmax = 6, rmax = 3;
  static constexpr RRLayout LY = rr_layout(nq, nv, nu, nbody, nM, ncon);
  static constexpr int o_qpos = LY.o_qpos, o_qvel = LY.o_qvel, o_act = LY.o_act, o_ctrl = LY.o_ctrl, o_xpos = LY.o_xpos, o_xquat = LY.o_xquat,
                       o_cinert = LY.o_cinert, o_cdof = LY.o_cdof, o_cvel = LY.o_cvel, o_qLD = LY.o_qLD, o_vec = LY.o_vec,
                       o_x = LY.o_x, o_arm = LY.o_arm, o_warm = LY.o_warm, o_qact = LY.o_qact, o_jlist = LY.o_jlist,
                       lds_floats = LY.lds_floats;
  __host__ __device__ RRDimsFixed(const RRDims& d) : RRDims(d) {}
  static bool matches(const RRDims& d) {
    const RRDims& r = d;
    return r.nq == nq && r.nv == nv && r.nu == nu && r.nbody == nbody && r.njnt == njnt && r.nM == nM && r.ncon == ncon && r.dmax == dmax &&
           r.nroot == nroot && r.obs_dim == obs_dim && r.nround == nround && r.lmax == lmax && r.cmax == cmax && r.rmax == rmax && r.o_qpos == o_qpos && r.o_qvel == o_qvel && r.o_act == o_act &&
           r.o_ctrl == o_ctrl && r.o_xpos == o_xpos && r.o_xquat == o_xquat && r.o_cinert == o_cinert && r.o_cdof == o_cdof &&
           r.o_cvel == o_cvel && r.o_qLD == o_qLD && r.o_vec == o_vec && r.o_x == o_x && r.o_arm == o_arm &&
           r.o_warm == o_warm && r.o_qact == o_qact && r.o_jlist == o_jlist && r.lds_floats == lds_floats;
  }
};
typedef RRDimsFixed<66, 59, 1263> RRDimsRodent;       // rodent_optimized.xml (the benchmark model)
// ROOT SLOT (RR_ROOT_SLOT; Wave::ROOT): which dims types run the tree phases with the root body alone in the second body slot.  The
// dimensions alone do not say that a model has the shape this needs; the host checks the rest against the blob (rr_api.hip root_slot_ok)
// before it selects an instance of such a type.
template <class DT> struct rr_root_slot { static constexpr bool value = false; };
template <> struct rr_root_slot<RRDimsFixed<66, 59, 1263>> { static constexpr bool value = RR_ROOT_SLOT != 0; };
typedef RRDimsFixed<67, 57, 1279> RRDimsRodentNew;    // rodent_new.xml (the env's default model [REF Rodent_Env_Brax.py:16]) == one replica of rodent_pair.xml

// Table pointers carry the global address space in their type, so every table access is a global_load (never flat).
typedef const int __attribute__((address_space(1)))* rr_gi;
typedef const float __attribute__((address_space(1)))* rr_gf;
struct RRTables {
  rr_gi factor3, linv, coljob, rowjob, jobown, body_i, jnt_i, dof_i, M_ij_k, body_anc, con_chain_rows, con_i, anc4;
  rr_gf body_f, jnt_f, dof_f, act_f, con_f, root_mass;
  rr_gi act_i, act_m_i;      // transmission (DYN instances): per actuator (first moment entry, count); per entry (dof, qpos address)
  rr_gf act_m_f;             // ... coefficient per entry
};
// The tables the solver's loops read (level schedules, solve jobs, contact chains): the only table pointers a wave keeps in scalar
// registers.  Every other table is read through load_tables() at the head of the phase that uses it (see RRKArgs).
struct RRLoopTables { rr_gi factor3, linv, coljob, rowjob, jobown, con_chain_rows; };
static __device__ __forceinline__ RRTables load_tables();      // defined with RRKArgs below
static __device__ __forceinline__ RRDims load_dims();
static __device__ __forceinline__ RRTables load_env_tables(int env, int nv, int nu, int ncon);      // RAND instances (per-environment parameter rows)
// A table row as (wave-uniform base, unsigned 32-bit byte offset of the row, element offset inside it): the address the device's
// global_load takes as SGPR pair + 32-bit VGPR + immediate.  Indexing a table pointer with an `int` instead makes every lane carry a
// 64-bit address built by sign extension, a 64-bit multiply-add and register-pair copies (3-5 vector instructions per row).
// Row and element indices are non-negative by construction (ids of bodies / dofs / joints / contacts / actuators).
typedef const char __attribute__((address_space(1)))* rr_gc;
template <class E>
struct rr_row {
  rr_gc base; unsigned off; int k0;
  __device__ __forceinline__ E operator[](int k) const { return *(const E __attribute__((address_space(1)))*)(base + (size_t)off + (ptrdiff_t)sizeof(E) * (k0 + k)); }
  __device__ __forceinline__ rr_row operator+(int k) const { return rr_row{base, off, k0 + k}; }
};
__device__ __forceinline__ rr_row<int> row_at(rr_gi t, int stride, int idx) { return rr_row<int>{(rr_gc)t, (unsigned)idx * (4u * (unsigned)stride), 0}; }
__device__ __forceinline__ rr_row<float> row_at(rr_gf t, int stride, int idx) { return rr_row<float>{(rr_gc)t, (unsigned)idx * (4u * (unsigned)stride), 0}; }

#define RR_EVAL_RAW 1
#define RR_EVAL_ACTIONS 2
struct RRIO {
  float *qpos, *qvel, *act, *warm;                         // state written by the launch
  const float *qpos_in, *qvel_in, *act_in, *warm_in;       // state read (== the above for an in-place step)
  const int* cur_frame_in;
  const float* ctrl;
  float *o_cinert, *o_cvel, *o_qfrc_actuator, *o_xpos, *o_xmat, *o_com, *dbg;
  float *o_cdist, *o_cpos, *o_cframe;                      // contact geometry of the last forward pass (optional)
  // env epilogue
  const float* track_pos;
  int track_len;
  int* cur_frame;
  float *obs, *reward, *done, *metrics;
  float healthy_reward, ctrl_cost_weight, z_min, z_max;
  int terminate_when_unhealthy;
  unsigned long long* prof;  // diagnostic build only: [N][RR_NPH] cycle sums per phase
  const int* env_map;        // nullable [N]: workgroup -> environment (SIMD pairing of heavy with light environments, rr_batch_set_schedule)
  unsigned* cost;            // nullable [N]: work estimate of this launch per environment (line-search point evaluations x row blocks)
  // multi-step rollout (UNROLL instances, rr_env_unroll): unroll_T env steps in one launch, the Episode + AutoReset training wrappers
  // applied in place between them; ctrl is then [unroll_T][N][nu]
  const float *first_qpos, *first_qvel, *first_act, *first_warm, *first_obs;   // the stored first state (restored where done)
  const float *prev_done, *steps_in;                                           // wrapper state before the launch [N]
  float *steps_out, *trunc_out;                                                // ... and after it
  float episode_length;
  int unroll_T;
  // ... with the actor inside (ACTOR instances, rr_env_unroll_policy): the action of step t is sampled in-kernel from the policy MLP
  // on the observation of step t, and the transitions go straight into the trajectory buffers [N][T(+1)][...] of the learner
  const float *a_obs_in;                          // [N][obs]  observation of the state before the launch
  const float *a_mean, *a_std;                    // nullable: observation normaliser
  const float *a_W0, *a_b0;                       // first layer [32][obs] (torch layout), [32]
  const float *a_Wt[4], *a_b[4];                  // hidden layers l = 1 .. a_nh-1: TRANSPOSED [32 in][32 out], [32]
  const float *a_Wth, *a_bh;                      // head TRANSPOSED and zero-padded: [32 in][64], [64] for A <= 32; [32 in][128], [128] for 32 < A <= 64
  const float *a_noise;                           // [T][N][A] standard normal draws
  float *a_actions;                               // [T][N][nu] out: the actions taken (also what the step reads as ctrl)
  float *t_obs, *t_raw, *t_logp, *t_reward, *t_discount, *t_trunc;     // [N][T+1][obs], [N][T][A], [N][T] x 4
  float a_min_std;
  int a_nh;
  int a_seg, a_pad;                               // trajectory segment length L (unroll_T = U * L): the buffers are [U][N][L(+1)][...]
                                                  // a_pad: EVAL instances only -- bit 0 (RR_EVAL_RAW): no Episode / AutoReset wrappers between the steps;
                                                  // bit 1 (RR_EVAL_ACTIONS): a_actions is [unroll_T][N][nu] (else one row set [N][nu], reused by every step)
  // PACING of a multi-step launch (nullable): one counter per launch, zeroed by the host; every environment adds 1 per finished env
  // step, so counter / num_envs is the launch's average progress.  An environment behind it by more than a fraction of a step raises
  // its wave priority (Wave::env_prio): the launch ends when its SLOWEST environment does, and a wave that outranks its SIMD partner
  // runs at close to single-wave speed while the partner, which is ahead, has slack.  Timing only -- results are unaffected.
  unsigned* progress;
  unsigned* dyn_overflow;            // DYN instances (nullable): counts (env, env step) events -- an env step in one of whose substeps more pairs were in
                                     // penetration than the wave has contact slots; a multi-step launch adds one per such step, as its single launches would
  unsigned* bad_states;              // counts (env, env step) events of the bad-state check below, with the same semantics; read only where the check is on
  float pace_t1, pace_t2, pace_t3;   // env steps behind the average for priority levels 1, 2, 3
  int pace_mode;                     // bits 0-1: 0 max(weight level, lag level), 1 lag level only, 2 sum capped at 3; bit 2 (4): progress counted
                                     // per SUBSTEP (ten times finer); bit 3 (8): the factor-phase priority is 3 for laggards, 2 otherwise
  // DOMAIN RANDOMISATION (RAND instances, rr_batch_set_env_params): per-environment copies of the three float tables that hold the
  // randomisable cells (friction mu / invweight; damping, armature; actuator gain and bias).  Each nullable: a null pointer leaves the
  // model's shared table in place.  Environment e reads rows [e][..]; everything else of the model stays shared.
  const float* env_dof_f;            // [N][nv][16]
  const float* env_act_f;            // [N][nu][8]
  const float* env_con_f;            // [N][ncon][26]
  // EVALUATION (EVAL instances, rr_env_unroll_eval: rr_eval_kernel): the multi-step form with the actor inside, without the trajectory.
  // t_obs is then a ring of two observation rows per environment, [N][2][obs] (step t reads row t & 1 and writes row (t + 1) & 1), the
  // other t_* arrays are not touched, a_noise may be null (the deterministic policy) and a_pad carries the flags below.
  float* e_metrics;                  // nullable [N][6], read and written: episode_steps, active_episodes, then the sums of pos_reward, reward_quadctrl,
                                     // reward_alive, reward over the env's active steps (brax EvalWrapper's eval_metrics)
  float* e_qpos_out;                 // nullable [unroll_T + 1][N][nq]: row 0 the incoming qpos, row t + 1 the qpos after step t (before a restore)
  int mode;  // 0 = forward only (pipeline_init), 1 = step; bit 1 (2) = env epilogue as reset (obs only)
  // BAD-STATE CHECK of the env epilogue (rr_step_body.inc), 0 = off: after an env step the env is bad when some element x of its qpos / qvel
  // fails |x| <= bad_state_max (so NaN and +-inf are bad).  Then done = 1, reward = 0, the metrics = 0 (actor instances: traj_reward = 0)
  // and bad_states += 1; the wrapped forms restore the first state as for any finished episode.  State and observation of the bad step are
  // NOT sanitised: the bare step and the raw evaluation form return them, flagged by done.
  float bad_state_max;
  // debug-dump instance only, a set of flags; no other instance reads it.  Each one makes that instance do work the production code leaves
  // out because nothing reads its result -- the A side of a bitwise test.
  //   RR_DBG_LS_RUN_REPEATS (rr_batch_set_ls_repeat_exit(b, 0)): the line search runs its repeated bracketing iterations instead of
  //     leaving the loop (RR_LS_REPEAT_EXIT);
  //   RR_DBG_SOLVER_UNTRIMMED (rr_batch_set_solver_trim(b, 0)): the solver solves for Mgrad and forms the next search direction BEFORE its
  //     exit test, walks the contacts (J' f) in the cost-only context at qacc_smooth, and rebuilds that context's rows where it is chosen.
  //   RR_DBG_SOLVER_UNBATCHED (rr_batch_set_solver_batch(b, 0)): the line search stages its compacted positions and D values in every
  //     call instead of once per substep (RR_LS_STAGE_ONCE).
  int dbg_flags;
  // MULTI-CLIP TRACKING (env epilogue): with `clip` set, track_pos is [num_clips][track_len][3] and environment e tracks clip clip[e]
  // (clamped into [0, num_clips - 1]); the frame clamp stays per clip.  A null `clip` is the single-clip path: track_pos [track_len][3].
  int num_clips;               // (also keeps sizeof(RRIO) a multiple of 8, RRKArgs)
  const int* clip;             // nullable [N]
  // POSE TRACKING (env epilogue of the POSE instances, rr_pose_kernel; no other instance reads these): the clip's root quaternion and
  // joint angles next to its root position.  track_pose is [T][nq - 3] (with `clip` set [num_clips][T][nq - 3]), a row = quaternion
  // (w, x, y, z) then the nq - 7 joints, indexed by the clip and frame the position reward reads.  With q = qpos[3:7], j = qpos[7:]:
  //   d = conj(r_q) (x) q,  theta = 2 atan2(|d.xyz|, |d.w|)      (invariant to the sign and the scale of q, well conditioned at 0)
  //   quat_reward = pose_quat_w exp(-pose_quat_k theta^2),  joint_reward = pose_joint_w exp(-pose_joint_k sum_i (j_i - r_j,i)^2)
  //   reward = (plain reward + quat_reward) + joint_reward;  pose_metrics[env] = (quat_reward, joint_reward), zeroed by a bad step
  // All six are fetched by narrow loads where they are used (load_io_member), never through load_io().
  const float* track_pose;
  float* pose_metrics;         // [N][2]
  float pose_quat_w, pose_quat_k, pose_joint_w, pose_joint_k;
  // REFERENCE OBSERVATION (REFOBS instances, rr_poseterm_kernel, rr_body_kernel and rr_restart_kernel; no other instance reads it): the observation row carries the clip's next
  // ref_frames = H >= 1 frames behind today's obs_dim entries, [ obs (obs_dim) | block_1 | ... | block_H ], row width obs_dim + H nq --
  // the stride of obs, t_obs, a_obs_in and first_obs in those instances (rr_obs_width).  block_h = (p_h[3], q_h[4], j_h[nq - 7]) at frame
  // f_h = clamp(new_frame + h, 0, track_len - 1) of the env's clip, new_frame the frame the track entry of the observation counts from:
  //   p_h = xmat[1] @ (track_pos[f_h] - qpos[:3])            (p_1 IS the track entry, bit for bit)
  //   q_h = s (conj(x) (x) r_q[f_h]), x = xquat[1], s = -1 where the w component is negative (q and -q are one rotation)
  //   j_h = r_j[f_h] - qpos[7:]
  // with r_q, r_j the parts of track_pose's row.  Written where the observation is written: at reset and after every env step.
  // Fetched by a narrow load where it is used (load_io_member), never through load_io().
  int ref_frames;
  int ref_pad;                 // keeps sizeof(RRIO) a multiple of 8 (RRKArgs)
  // POSE TERMINATION (PTERM instances, rr_poseterm_kernel, rr_body_kernel and rr_restart_kernel; no other instance reads it): an env step whose stepped qpos strays from the
  // clip's row at (clip[env], old_frame) -- the row the position and pose rewards read -- ends the episode.  Lane 0 forms
  //   e_pos = |qpos[:3] - track_pos[f]|, e_quat = theta of POSE TRACKING, e_joint = sqrt(sum (qpos[7+i] - r_j,i)^2),
  //   code = 1 (e_pos > pose_max_pos) | 2 (e_quat > pose_max_quat) | 4 (e_joint > pose_max_joint)      (+inf: off; a NaN error: no bit)
  // stores (float)code in pose_fail[env] and done = max(done, code != 0); a bad step stores code 0.  Never at reset.  Nothing else of the
  // step changes.  Fetched by narrow loads where they are used (load_io_member), never through load_io().
  float* pose_fail;            // [N]
  float pose_max_pos, pose_max_quat, pose_max_joint;
  int pterm_pad;               // keeps sizeof(RRIO) a multiple of 8 (RRKArgs)
  // BODY TRACKING (BODY instances, rr_body_kernel and rr_restart_kernel; no other instance reads these): the clip's global body positions next to its pose.
  // track_bodies is [T][nbody][3] (with `clip` set [num_clips][T][nbody][3]), indexed by the clip and frame the position and pose rewards
  // read; body_weights is [2][nbody], row 0 the 0 / 1 mask of the tracked bodies B, row 1 that of the end effectors E (entry 0, the
  // world, is not read).  With xpos the body positions of the step's LAST FORWARD PASS (the pose before the last substep's integration,
  // what rr_outputs.xpos holds) and r the row:
  //   S_B = sum_{b in B} |xpos[b] - r[b]|^2,  S_E = the same over E        (every product and sum rounded on its own, ascending b per lane)
  //   body_reward = body_w exp(-body_k S_B),  endeff_reward = endeff_w exp(-endeff_k S_E)
  //   reward = (((plain reward + quat_reward) + joint_reward) + body_reward) + endeff_reward
  //   body_metrics[env] = (body_reward, endeff_reward), zeroed by a bad step.  Never at reset.
  // xpos lives in LDS only between kinematics() and the recycling of its cells in the last substep, so S_B and S_E are formed THERE and
  // parked in body_metrics[env] by lane 0, which reads them back in the epilogue and overwrites them with the two terms: nothing lives
  // across the solver.  All fetched by narrow loads where they are used (load_io_member), never through load_io().
  const float* track_bodies;
  const float* body_weights;   // [2][nbody]
  float* body_metrics;         // [N][2]
  float body_w, body_k, endeff_w, endeff_k;
  // CLIP RESTARTS (RESTART instances, rr_restart_kernel; no other instance reads these): a restarted episode rejoins its clip.  The
  // first_* arrays of the launch are then a BANK of restart_K start states, [K][N][width] each, restart_frames [K][N] the frame each was
  // formed at, and the env carries a slot (wave-uniform, next to u_steps / u_frame).  Per wrapped env step, new_frame = old_frame + 1:
  //   over = steps' >= episode_length || (restart_end && new_frame >= track_len - 1)
  //   done: slot' = (slot + 1) mod K, state and observation <- bank[slot'], cur_frame <- restart_frames[slot'];  else slot, new_frame
  // The step that ends the episode is untouched (its reward, metrics and pose_fail read old_frame); cur_frame and the slot of the
  // launch's last step go out with the final state.  Fetched by narrow loads where they are used (load_io_member).
  const int* restart_frames;   // [K][N]
  const int* restart_slot_in;  // [N]
  int* restart_slot_out;       // [N]
  int restart_K;               // 1 .. 64
  int restart_end;             // != 0: the clip's end (no next frame left to read without clamping) truncates the episode
  // VELOCITY TRACKING (BODY instances, rr_body_kernel and rr_restart_kernel; no other instance reads these): the clip's velocities next
  // to its pose.  track_vel is [T][nv] (with `clip` set [num_clips][T][nv]), a row in qvel layout, indexed by the clip and frame the
  // position and pose rewards read.  With d = qvel - row on the stepped qvel:
  //   S_lin = sum d[0:3]^2,  S_ang = sum d[3:6]^2,  S_joint = sum d[6:]^2      (every product and sum rounded on its own: per lane the
  //                                                                              dofs in ascending order, then the wave sum)
  //   lin = vel_lin_w exp(-vel_lin_k S_lin),  ang = vel_ang_w exp(-vel_ang_k S_ang),  joint = vel_joint_w exp(-vel_joint_k S_joint)
  //   reward = ((reward so far + lin) + ang) + joint;  vel_metrics[env] = (lin, ang, joint), zeroed by a bad step.  Never at reset.
  // A null track_vel: no such terms (one scalar load and a branch).  All fetched by narrow loads where they are used (load_io_member).
  const float* track_vel;
  float* vel_metrics;          // [N][3]
  float vel_lin_w, vel_lin_k, vel_ang_w, vel_ang_k, vel_joint_w, vel_joint_k;
  // CLIP LIBRARY (BODY instances, rr_body_kernel and rr_restart_kernel; no other instance reads these; rr_batch_set_clip_library).
  // clip_len [num_clips] (one entry without `clip`): clip c consists of rows 0 .. clip_len[c] - 1 of every [num_clips][track_len][..]
  // array, the rows behind them are padding that nothing reads.  Wherever an env on clip c clamps a frame into 0 .. track_len - 1 it
  // clamps into 0 .. L - 1 instead, L = clip_len[c] clamped into 1 .. track_len (rr_clip_frames), and the clip's end of CLIP RESTARTS is
  // new_frame >= L - 1.  The row stride stays track_len.  A null clip_len: every clip has track_len frames.
  // bank_clips [K][N] (RESTART instances, next to restart_frames): the clip of each bank entry.  The rule gains one line,
  //   done: clip <- bank_clips[slot'] (clamped into 0 .. num_clips - 1);  else the clip the env is on,
  // the launch reads clip[env] once, carries the id wave-uniform through its steps and stores it to clip_out[env] after the last one
  // (`clip` itself is read only).  A null bank_clips: every entry on the env's clip, nothing stored.
  // Only integer bounds and row bases change: no reward expression gains a use.  Fetched by narrow loads where they are used.
  const int* clip_len;
  const int* bank_clips;
  int* clip_out;               // [N]
  // CLIP SAMPLING (RESTART instances, rr_restart_kernel; no other instance reads these; rr_batch_set_clip_sampling).  Integers only.
  // outcomes [num_clips][5] int64, added to and never cleared by a launch.  With c the clip a wrapped step was made on (before any
  // restore): col 4 += 1; where done: col 0 += 1 and exactly one of col 1 (the step's pose-termination code is nonzero), col 2 (else the
  // env's own done: unhealthy, bad state), col 3 (else: `over` alone, a truncation by episode_length or the clip's end).  The launch
  // counts the steps of the running episode segment in a wave-uniform register and flushes it with the episode's end and with the
  // launch's last step: one 64-bit atomic add per flush (lane 0, agent scope, relaxed, like `progress`).  Null: no counting.
  // clip_weights [num_clips] int32, entries 0 .. 65535 (needs bank_clips): a restore draws its slot instead of taking the next one,
  //   q_k = clip_weights[clamp(bank_clips[k][env])], k = 0 .. K - 1;  S = sum q_k;
  //   h = fmix32(fmix32(sample_seed ^ (uint32(env) * 0x9E3779B1)) + uint32(n)), n = the env's restore count;  r = (uint64(h) * S) >> 32;
  //   slot' = the smallest k with q_0 + .. + q_k > r;   S == 0: slot' = (slot + 1) mod K.
  // Lane k < K loads q_k, an inclusive wave scan of six steps, a ballot of prefix > r and its lowest set bit: wave-uniform, and run only
  // at a restore.  n is read from draws_in[env] once, grows by one at every restore either way and goes to draws_out[env] after the
  // launch's last step (null draws_in: n starts at 0 and is not stored).  Null clip_weights: the cyclic rule.
  const int* clip_weights;
  const int* draws_in;
  int* draws_out;              // [N]
  long long* outcomes;         // [num_clips][5]
  unsigned sample_seed;
  // REFERENCE RESTARTS (RESTART instances, rr_restart_kernel; no other instance reads these; rr_batch_set_reference_restart).  rref_on
  // != 0: a restore reads no bank entry.  With n the env's restore count before the restore (draws_in / draws_out as above) and
  //   base = fmix32(fmix32(rref_seed ^ (uint32(env) * 0x9E3779B1)) + n);  h(p, i) = fmix32(base ^ (((p << 16) | i) * 0x9E3779B1))
  // it draws, wave-uniform and in integers,
  //   clip  c = rref_across ? (clip_weights with S > 0 ? the smallest c with q_0 + .. + q_c > (h(1, 0) * S) >> 32, the scan in chunks of 64
  //             : (h(1, 0) * num_clips) >> 32) : the clip the env is on
  //   frame d = rref_lo + ((h(2, 0) * (rref_hi - rref_lo)) >> 32);  f = clip_len ? d mod (L_c - 1) : d;  rows at clamp(f, 0, L_c - 1)
  // builds qpos = [track_pos[c][f], track_pose[c][f]] + rref_noise * s(h(3, i)), qvel = (track_vel ? track_vel[c][f] : 0) + rref_noise *
  // s(h(4, i)), s(h) = (h >> 8) * 2^-23 - 1 (exact; then one rounded product and one rounded sum), zeroes act and the warm start, sets
  // cur_frame = f and clip = c, and the launch runs ONE forward-only pass of the loop body on that state (mode 2: no substep, the reset
  // epilogue) before the next step, which writes the observation where the ended step's stood.  The bank's arrays are not read; the
  // slot advances cyclically and means nothing.  Fetched by narrow loads where they are used.
  unsigned rref_seed;
  int rref_on, rref_lo, rref_hi, rref_across;
  float rref_noise;
  int rref_pad;
};

// ------------------------------------------------------------------------------------------ small math
#define RR_DBG_LS_RUN_REPEATS 1
#define RR_DBG_SOLVER_UNTRIMMED 2
#define RR_DBG_SOLVER_UNBATCHED 4
struct v3 { float x, y, z; };
__device__ __forceinline__ v3 mk3(float x, float y, float z) { v3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ __forceinline__ v3 ld3(const float* p) { return mk3(p[0], p[1], p[2]); }
__device__ __forceinline__ v3 ld3(const float __attribute__((address_space(1)))* p) { return mk3(p[0], p[1], p[2]); }
__device__ __forceinline__ v3 ld3(const rr_row<float>& p) { return mk3(p[0], p[1], p[2]); }
__device__ __forceinline__ void st3(float* p, v3 a) { p[0] = a.x; p[1] = a.y; p[2] = a.z; }
__device__ __forceinline__ v3 operator+(v3 a, v3 b) { return mk3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ v3 operator-(v3 a, v3 b) { return mk3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ v3 operator*(v3 a, float s) { return mk3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ float dot(v3 a, v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ v3 cross(v3 a, v3 b) { return mk3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }

__device__ __forceinline__ void quat_mul(float* r, const float* a, const float* b) {
  float w = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  float x = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  float y = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  float z = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
  r[0] = w; r[1] = x; r[2] = y; r[3] = z;
}
__device__ __forceinline__ void quat_to_mat(float* m, const float* q) {
  float w = q[0], x = q[1], y = q[2], z = q[3];
  m[0] = w * w + x * x - y * y - z * z; m[1] = 2 * (x * y - w * z); m[2] = 2 * (x * z + w * y);
  m[3] = 2 * (x * y + w * z); m[4] = w * w - x * x + y * y - z * z; m[5] = 2 * (y * z - w * x);
  m[6] = 2 * (x * z - w * y); m[7] = 2 * (y * z + w * x); m[8] = w * w - x * x - y * y + z * z;
}
__device__ __forceinline__ v3 mat_vec(const float* m, v3 v) {
  return mk3(m[0] * v.x + m[1] * v.y + m[2] * v.z, m[3] * v.x + m[4] * v.y + m[5] * v.z, m[6] * v.x + m[7] * v.y + m[8] * v.z);
}
__device__ __forceinline__ void quat_normalize(float* q) {
  float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  if (n < RR_MINVAL) { q[0] = 1; q[1] = q[2] = q[3] = 0; return; }
  const float inv = 1.0f / n;
  q[0] *= inv; q[1] *= inv; q[2] *= inv; q[3] *= inv;
}
// spatial inertia (xx yy zz xy xz yz, m*off(3), m) times motion vector (ang; lin)
__device__ __forceinline__ void mul_inert_vec(float* res, const float* i, const float* v) {
  res[0] = i[0] * v[0] + i[3] * v[1] + i[4] * v[2] - i[8] * v[4] + i[7] * v[5];
  res[1] = i[3] * v[0] + i[1] * v[1] + i[5] * v[2] + i[8] * v[3] - i[6] * v[5];
  res[2] = i[4] * v[0] + i[5] * v[1] + i[2] * v[2] - i[7] * v[3] + i[6] * v[4];
  res[3] = i[8] * v[1] - i[7] * v[2] + i[9] * v[3];
  res[4] = i[6] * v[2] - i[8] * v[0] + i[9] * v[4];
  res[5] = i[7] * v[0] - i[6] * v[1] + i[9] * v[5];
}
__device__ __forceinline__ void cross_motion(float* res, const float* vel, const float* v) {
  res[0] = -vel[2] * v[1] + vel[1] * v[2];
  res[1] = vel[2] * v[0] - vel[0] * v[2];
  res[2] = -vel[1] * v[0] + vel[0] * v[1];
  res[3] = -vel[2] * v[4] + vel[1] * v[5] - vel[5] * v[1] + vel[4] * v[2];
  res[4] = vel[2] * v[3] - vel[0] * v[5] + vel[5] * v[0] - vel[3] * v[2];
  res[5] = -vel[1] * v[3] + vel[0] * v[4] - vel[4] * v[0] + vel[3] * v[1];
}
__device__ __forceinline__ void cross_force(float* res, const float* vel, const float* f) {
  res[0] = -vel[2] * f[1] + vel[1] * f[2] - vel[5] * f[4] + vel[4] * f[5];
  res[1] = vel[2] * f[0] - vel[0] * f[2] + vel[5] * f[3] - vel[3] * f[5];
  res[2] = -vel[1] * f[0] + vel[0] * f[1] - vel[4] * f[3] + vel[3] * f[4];
  res[3] = -vel[2] * f[4] + vel[1] * f[5];
  res[4] = vel[2] * f[3] - vel[0] * f[5];
  res[5] = -vel[1] * f[3] + vel[0] * f[4];
}
__device__ __forceinline__ float dot6(const float* a, const float* b) {
  float s = a[0] * b[0];
  s += a[1] * b[1]; s += a[2] * b[2]; s += a[3] * b[3]; s += a[4] * b[4]; s += a[5] * b[5];
  return s;
}
// Wavefront sum, result in every lane.  Four DPP adds give each 16-lane row its total (no LDS crossbar), two row
// broadcasts fold the rows into lane 63, one v_readlane returns it: a fixed order (deterministic), 7 issues per value.
__device__ __forceinline__ float dpp_add(float v, const int ctrl_tag) {
  int x = __float_as_int(v), y;
  switch (ctrl_tag) {
    case 0: y = __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true); break;    // quad_perm [1,0,3,2]
    case 1: y = __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, true); break;    // quad_perm [2,3,0,1]
    case 2: y = __builtin_amdgcn_update_dpp(0, x, 0x141, 0xF, 0xF, true); break;   // row_half_mirror
    case 3: y = __builtin_amdgcn_update_dpp(0, x, 0x140, 0xF, 0xF, true); break;   // row_mirror: every lane holds its row's sum
    // the two row broadcasts as single DPP adds (the compiler emits v_mov_b32_dpp + v_add_f32 for the masked form):
    // enabled rows add the broadcast lane, the other rows keep their value; s_nop covers the VALU-write -> DPP-read hazard
    case 4: asm("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf" : "+v"(v)); return v;   // rows 1, 3 += rows 0, 2
    case 5: asm("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf" : "+v"(v)); return v;   // rows 2, 3 += rows 0+1
    default: return v;
  }
  return v + __int_as_float(y);
}
// sum over the 64 lanes, returned wave-uniform: six DPP adds leave the total in lane 63
__device__ __forceinline__ float wave_sum(float v) {
  v = dpp_add(v, 0); v = dpp_add(v, 1); v = dpp_add(v, 2); v = dpp_add(v, 3); v = dpp_add(v, 4); v = dpp_add(v, 5);
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
// the two row-broadcast steps of K >= 3 values as ONE asm block each: a single s_nop covers the VALU-write -> DPP-read hazard of
// the first value, the K - 1 >= 2 instructions in between cover it for the others (dpp_add pays one s_nop per value)
template <int K>
__device__ __forceinline__ void dpp_bcast_stage(float* v) {
  static_assert(K == 3 || K == 4 || K == 6, "instantiated widths");
  if constexpr (K == 3)
    asm("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\tv_add_f32_dpp %1, %1, %1 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
        "v_add_f32_dpp %2, %2, %2 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
        "v_add_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\tv_add_f32_dpp %1, %1, %1 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
        "v_add_f32_dpp %2, %2, %2 row_bcast:31 row_mask:0xc bank_mask:0xf"
        : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]));
  else if constexpr (K == 4)
    asm("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\tv_add_f32_dpp %1, %1, %1 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
        "v_add_f32_dpp %2, %2, %2 row_bcast:15 row_mask:0xa bank_mask:0xf\n\tv_add_f32_dpp %3, %3, %3 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
        "v_add_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\tv_add_f32_dpp %1, %1, %1 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
        "v_add_f32_dpp %2, %2, %2 row_bcast:31 row_mask:0xc bank_mask:0xf\n\tv_add_f32_dpp %3, %3, %3 row_bcast:31 row_mask:0xc bank_mask:0xf"
        : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]));
  else
    asm("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\tv_add_f32_dpp %1, %1, %1 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
        "v_add_f32_dpp %2, %2, %2 row_bcast:15 row_mask:0xa bank_mask:0xf\n\tv_add_f32_dpp %3, %3, %3 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
        "v_add_f32_dpp %4, %4, %4 row_bcast:15 row_mask:0xa bank_mask:0xf\n\tv_add_f32_dpp %5, %5, %5 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
        "v_add_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\tv_add_f32_dpp %1, %1, %1 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
        "v_add_f32_dpp %2, %2, %2 row_bcast:31 row_mask:0xc bank_mask:0xf\n\tv_add_f32_dpp %3, %3, %3 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
        "v_add_f32_dpp %4, %4, %4 row_bcast:31 row_mask:0xc bank_mask:0xf\n\tv_add_f32_dpp %5, %5, %5 row_bcast:31 row_mask:0xc bank_mask:0xf"
        : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]));
}
template <int K>
__device__ __forceinline__ void wave_sum_n(float* v) {
  constexpr bool BLOCK = RR_DPP_BLOCK && (K == 3 || K == 4 || K == 6);
#pragma unroll
  for (int st = 0; st < (BLOCK ? 4 : 6); ++st)
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = dpp_add(v[k], st);
  if constexpr (BLOCK) dpp_bcast_stage<K>(v);
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[k]), 63));
}

// solver impedance [UP mjx constraint._kbi]
__device__ __forceinline__ void kbi(float dt, float sr0, float sr1, const float* si, float pos, float& k, float& b, float& imp) {
  float timeconst = fmaxf(sr0, 2.0f * dt);
  float dmin = fminf(fmaxf(si[0], RR_MINIMP), RR_MAXIMP), dmax = fminf(fmaxf(si[1], RR_MINIMP), RR_MAXIMP);
  float width = fmaxf(RR_MINVAL, si[2]);
  float mid = fminf(fmaxf(si[3], RR_MINIMP), RR_MAXIMP);
  float power = fmaxf(1.0f, si[4]);
  k = 1.0f / (dmax * dmax * timeconst * timeconst * sr1 * sr1);
  b = 2.0f / (dmax * timeconst);
  if (sr0 <= 0) k = -sr0 / (dmax * dmax);
  if (sr1 <= 0) b = -sr1 / dmax;
  float x = fabsf(pos) / width;
  float a_, bb;
  if (power == 2.0f) {            // the exponent of every constraint of the rodent models: squares instead of four powf
    a_ = (1.0f / mid) * (x * x);
    bb = 1.0f - (1.0f / (1.0f - mid)) * ((1.0f - x) * (1.0f - x));
  } else if (power == 1.0f) {
    a_ = x;
    bb = 1.0f - (1.0f - x);
  } else {
    a_ = (1.0f / powf(mid, power - 1.0f)) * powf(x, power);
    bb = 1.0f - (1.0f / powf(1.0f - mid, power - 1.0f)) * powf(1.0f - x, power);
  }
  float y = x < mid ? a_ : bb;
  imp = dmin + y * (dmax - dmin);
  imp = fminf(fmaxf(imp, dmin), dmax);
  if (x > 1.0f) imp = dmax;
}

struct LSPoint { float alpha, cost, d0, d1; };
// a / b by v_rcp_f32 and one Newton step (<= 1 ulp from the IEEE quotient; the IEEE sequence is 13 instructions and the
// line search, which sets the length of the slowest environments, does two per bracketing iteration)
__device__ __forceinline__ float div_nr(float a, float b) { float r = __builtin_amdgcn_rcpf(b); r = r * (2.0f - b * r); return a * r; }

// Table loads in the hot loops must be GLOBAL loads: when the optimiser loses the address space of a table pointer it
// emits flat_load, which also counts on lgkmcnt -- every LDS wait would then drain the table prefetch as well.
__device__ __forceinline__ int g_int(const int __attribute__((address_space(1)))* base, int idx) { return base[idx]; }
__device__ __forceinline__ int g_int32(rr_gi base, int idx) { return row_at(base, 1, idx)[0]; }      // ... through a 32-bit offset (idx >= 0)

// Identity the optimiser cannot see through: stops loop-invariant code motion from unpacking every packed index
// table entry once, ahead of the solver loops, and keeping hundreds of unpacked indices / addresses alive in
// registers (the unpack is 2 VALU ops; the registers are what limits residency).
__device__ __forceinline__ int opaque(int x) { asm volatile("" : "+v"(x)); return x; }

// Per-body model constants of the tree sweeps.  For bodies 0..63 (slot 0) they live in registers for the whole
// launch; a body's 2nd/3rd joint (a dozen bodies have one) and bodies >= 64 reload from the L2-resident tables.
struct BodyC {
  int parent, depth, sib, dofadr, dofnum, jn, jadr;
  int jtype0, jqa0, jda0;
  float pos[3], quat[4], jpos0[3], jaxis0[3], jq00;
};
__device__ __forceinline__ BodyC load_bodyc(const RRTables& T, int b, int nbody) {
  BodyC c;
  const bool ok = b >= 1 && b < nbody;
  auto bi = row_at(T.body_i, RR_BODYI, ok ? b : 0);
  auto bf = row_at(T.body_f, 18, ok ? b : 0);
  c.parent = bi[0]; c.jadr = bi[1]; c.jn = ok ? bi[2] : 0; c.dofadr = bi[3]; c.dofnum = bi[4];
  c.depth = ok ? bi[8] : -1; c.sib = bi[9];
#pragma unroll
  for (int k = 0; k < 3; ++k) c.pos[k] = bf[k];
#pragma unroll
  for (int k = 0; k < 4; ++k) c.quat[k] = bf[3 + k];
  const int j = c.jn > 0 ? c.jadr : 0;
  auto ji = row_at(T.jnt_i, 4, j);
  auto jf = row_at(T.jnt_f, 8, j);
  c.jtype0 = c.jn > 0 ? ji[0] : 3; c.jqa0 = ji[1]; c.jda0 = ji[2];
#pragma unroll
  for (int k = 0; k < 3; ++k) { c.jpos0[k] = jf[k]; c.jaxis0[k] = jf[3 + k]; }
  c.jq00 = jf[6];
  return c;
}

// ------------------------------------------------------------------------------------------ the wave
// ---- diagnostic builds only (tools/rep_bench.py): run a phase REP extra times to read its marginal in-situ cost
#ifndef RR_REP_SOLVE
#define RR_REP_SOLVE 0
#endif
#ifndef RR_REP_LS
#define RR_REP_LS 0
#endif
#ifndef RR_REP_UC
#define RR_REP_UC 0
#endif
#ifndef RR_REP_JAC
#define RR_REP_JAC 0
#endif
#ifndef RR_REP_MM
#define RR_REP_MM 0
#endif
#ifndef RR_REP_KIN
#define RR_REP_KIN 0
#endif
typedef float rr_f2 __attribute__((ext_vector_type(2)));
template <class A, class B> struct rr_same { static constexpr bool value = false; };
template <class A> struct rr_same<A, A> { static constexpr bool value = true; };
// PAIR: the model is two identical trees that share no constraint (rodent_pair.xml: M block-diagonal, floor contacts only); the
// workgroup is TWO wavefronts, wave r steps replica r on the tables of one replica in its own LDS region, and the only coupling is the
// CG solver's scalars (cost, gradient norm, line-search sums, Polak-Ribiere beta): every such wave sum is followed by an exchange
// through LDS (solver_sum_n), after which both waves hold the same totals and take the same branches.
// DYN (rodent_cpu.xml): the model's contact list is a list of CANDIDATE pairs of two moving geoms (sphere / capsule); every
// substep the wave scans it, keeps the pairs in penetration in its 64 * NCS contact slots (in list order, by ballot), and works on those:
// J = jac(body2) - jac(body1) through SIGNED dof chains (the dofs on exactly one of the two ancestor chains; J x) and a two-interval
// membership test (J' f); contacts of condim 1 carry one row (rows 1..3 of the slot get D = 0); transmissions with several joints (fixed
// tendons) go through per-actuator sums.  Production physics + env epilogue: single-step, multi-step (UNROLL) and multi-step with the
// actor inside (UNROLL + ACTOR); everything DYN-specific is re-derived per substep, so the multi-step loop carries nothing extra for it.
// One diagnostic instance, DBG x DYN, single-step: the dump with the contact sections per candidate pair (contact_geometry_dyn).
// JRES: this instance may hold the solve-job descriptors in registers for the substep (RR_JOBS_RESIDENT; not the debug-dump instances, whose
// dump paths leave no room for them)
// MRES: how much of the inverse factor this instance may hold in registers next to them (RR_SOLVE_MAT_RESIDENT; Wave::MAT_RES): 0 nothing,
// 1 the entries of its column jobs, 2 those of its column and row jobs.  Chosen per entry point by its register figures.
// ROOT (RR_ROOT_SLOT; rr_root_slot<DT>): the lane <-> body map of the tree phases for a model of ONE tree whose root (body 1, child of the
// world) holds the model's only free joint and that has at most 66 bodies.  Slot 0 then holds the 64 bodies that are not the root -- lanes
// 2 .. 63 their own number, lanes 0 and 1 bodies 64 and 65 -- and slot 1 the root alone, on lane 1.  Every body stays on the lane it has
// under the plain map b = lane + 64 s, so the per-lane partial sums of the subtree COM stand where they stood.  Slot 0's code then carries
// no free-joint branch; slot 1's carries no hinge, no pointer-doubling round (the root has no ancestor) and no table read (its joint is
// qpos[0 .. 6], its dofs 0 .. 5: host-checked), and its subtree sum is spread over 16 lanes (backward_sweep).
template <int NBS, int NVS, int NCS, class DT, bool NEWTON = false, bool PAIR = false, bool DYN = false, bool RAND = false, bool JRES = true, int MRES = 0, bool ROOT = false>
struct Wave {
  static_assert(!ROOT || (NBS == 2 && !PAIR && !DYN), "ROOT: one-tree models of 65 or 66 bodies");
  const DT& D;
  RRLoopTables TL;
  int renv = 0;           // RAND: the environment whose parameter rows this wave reads (wave-uniform; re-derived with `lane`)
  int lane;               // re-derived (opaquely) at the head of every substep: see RR_FRAME_LOCAL in the kernel
  float* const lds;
  int rep = 0;            // PAIR: this wave's replica (wave-uniform)
  int lag_mode = 0;       // how lag_prio combines with the weight-based level (RRIO::pace_mode)
  int lag_prio = 0;       // multi-step launches: priority level of an environment that is behind the launch's average progress (wave-uniform)
  int xpar = 0;           // PAIR: parity of the next exchange (two buffers: a wave may be one exchange ahead of its partner)
  float* s_xc = nullptr;  // PAIR: exchange cells [2 parities][2 waves][8] behind the two replicas' regions
  // LDS regions.  Aliases (liveness): s_crb == s_cinert (accumulated in place once cinert has been
  // consumed / written out), s_cacc|s_cfrc and the sin/cos scratch live in the region that later holds qLD,
  // s_buf reuses xpos|xquat after the contact geometry has been taken.
  float *s_qpos, *s_qvel, *s_act, *s_ctrl, *s_xpos, *s_xquat, *s_cinert, *s_crb, *s_cdof, *s_cvel, *s_cacc,
      *s_cfrc, *s_buf, *s_sc, *s_qLD, *s_vec, *s_x, *s_arm, *s_warm, *s_qact;
  float *s_H, *s_Mp;      // Newton instance: Hessian pairs, copy of the M pairs
  unsigned char* s_anc;   // Newton instance: ancestor ids along the rows of M
  float dinvH[NVS];       // Newton instance: 1/D of the Hessian's factor
  int* s_jlist;           // contact ids by rank (J*x jobs)

  static constexpr int W = NVS * RR_LANES;
  static constexpr int WC = NCS * RR_LANES;

  // ---- model constants held in registers for the whole launch (loaded once, reused by all substeps)
  BodyC bc0, bc1;         // constants of bodies `lane` (slot 0) and `lane + 64` (slot 1); further slots are loaded at use (ROOT: of body_at(0); bc1 unused)
  int banc[NBS][2];       // 2^k-th ancestors of the slot's body, k = 0..7, one byte each (0 = none)
  int blast[NBS];         // last body of the subtree (bodies are in DFS order)
  int dofc0[NVS], dofc1[NVS];   // packed per-dof constants: depth | kind<<8 | root<<12 | body<<16 | parent-of-body<<24 ; Madr | last_desc<<16
  // J*x jobs (contact_jobs): the ancestor chains of the contacts in penetration are cut into pieces, one per lane
  static constexpr int JW = DYN ? 10 : 9;       // ints of a chain row (4 ids each)
  int jch[NCS][JW];       // dof ids of this lane's piece, 4 per register (DYN: bit 7 = the dof enters with a minus sign)
  int con_rank[NCS];      // rank of this lane's contact among the contacts in penetration
  int con_leaf[NCS];      // last dof of the contact's chain
  int con_leaf1[NCS];     // DYN: last dof of body1's chain (-1: world)
  int con_pid[NCS];       // DYN: candidate pair held by this slot
  int con_nrow[NCS];      // DYN: rows of the slot's contact (4 = pyramid, 1 = frictionless)
  int dyn_overflow = 0;   // DYN: pairs in penetration beyond the slots in a substep of this env step (dropped; counted per env step, RRIO::cost bit 31)
  int jP, jLp, jnact;     // wave-uniform: lanes per contact (4 / 2 / 1), ids per piece (12 / 20 / 36), contacts in penetration
  // per-dof registers (slot s -> dof lane + 64 s)
  float dinv[NVS], dinvB[NVS];   // 1/D of M's factor, and of the eulerdamp matrix M + dt*diag(damping)
  float Ma_warm[NVS];            // M * qacc_warmstart, taken before the cells of qM are given to the second factor
  float qfrc_smooth[NVS], qacc_smooth[NVS];
  float qacc[NVS], Ma[NVS], grad[NVS], Mgrad[NVS], search[NVS], mv[NVS], qfrc_con[NVS];
  // limit rows (one per limited hinge dof)
  float lim_sign[NVS], lim_D[NVS], lim_aref[NVS], lim_jar[NVS], lim_jv[NVS];
  bool lim_act[NVS];
  // contact rows (4 pyramid rows per contact slot)
  bool con_act[NCS];
  float con_mu[NCS], con_D[NCS], con_aref[NCS][4], con_jar[NCS][4], con_jv[NCS][4];
  float con_kk[NCS], con_b[NCS];                 // k*imp*dist and b of the contact's reference acceleration
  float con_off[NCS][3], con_fr[NCS][9];         // contact point relative to the tree's COM; frame rows n, t1, t2
  int con_nanc[NCS];
  float com0[3], com1[3];
  float gauss, cost, prev_cost;
  // solver options, read from the kernel arguments at the head of solve() and held in scalar registers through its loops only
  float so_tolerance, so_ls_tolerance, so_meaninertia;
  int so_iterations, so_ls_iterations, so_nv_scale;
  int dbg_flags = 0, dbg_ls_ran = 0, dbg_ls_left = 0;      // debug-dump instance only: RRIO::dbg_flags; bracketing iterations executed / left out in this substep
  int dbg_solver_end = 0;           // debug-dump instance only, this substep's solve(): bit 0 the context at qacc_smooth was chosen; how the loop ended: bit 1 cap, bit 2 improvement, bit 3 gradient
  int work;               // wave-uniform count of line-search point evaluations, weighted by row blocks: the scheduling cost estimate (rr_batch_set_schedule)
  unsigned long long pt_last, pt[RR_NPH];
  template <bool PROF> __device__ __forceinline__ void stamp(int i) {
    if (PROF) { const unsigned long long t = __builtin_readcyclecounter(); pt[i] += t - pt_last; pt_last = t; }
  }

  // Run-time dimensions for one phase.  The fixed-dimension instances read the few scalars a phase needs (dt, gravity, schedule
  // lengths) from the kernel arguments at its head, so none of them is held -- or spilled -- across the substep; the generic
  // instances index by dozens of run-time dimensions in every phase and keep the resident copy.
  __device__ __forceinline__ DT phase_dims() const {
    if constexpr (rr_same<DT, RRDims>::value) return D;
    else return DT(load_dims());
  }
  // The model tables for one phase.  RAND instances: dof_f / act_f / con_f advanced to this environment's rows (scalar arithmetic on the
  // wave-uniform id, once per phase), so that every row_at() below stays SGPR base + 32-bit offset + immediate.
  __device__ __forceinline__ RRTables tables() const {
    if constexpr (RAND) return load_env_tables(renv, D.nv, D.nu, D.ncon);
    else return load_tables();
  }
  __device__ Wave(const DT& d, const RRTables& t, float* l)
      : D(d), TL{t.factor3, t.linv, t.coljob, t.rowjob, t.jobown, t.con_chain_rows}, lane(threadIdx.x & (RR_LANES - 1)), lds(l) {
    s_qpos = l + d.o_qpos; s_qvel = l + d.o_qvel; s_act = l + d.o_act; s_ctrl = l + d.o_ctrl;
    s_xpos = l + d.o_xpos; s_xquat = l + d.o_xquat; s_cinert = l + d.o_cinert; s_crb = s_cinert;
    s_cdof = l + d.o_cdof; s_cvel = l + d.o_cvel; s_qLD = l + d.o_qLD;
    s_cacc = s_qLD; s_cfrc = s_qLD + 6 * d.nbody; s_sc = s_qLD; s_buf = s_xpos;
    s_vec = l + d.o_vec; s_x = l + d.o_x; s_arm = l + d.o_arm; s_warm = l + d.o_warm; s_qact = l + d.o_qact;
    s_jlist = (int*)(l + d.o_jlist);
    s_H = l + d.o_H; s_Mp = l + d.o_Mp; s_anc = (unsigned char*)(l + d.o_anc);
    // plain values from here on: as loads from the argument block the allocator re-issues them (a scalar load and its wait) inside the
    // solver's loops instead of keeping them
    asm("" : "+s"(TL.coljob), "+s"(TL.rowjob), "+s"(TL.jobown));
  }

  // One wavefront owns the environment: its LDS instructions execute in program order, so a cross-lane hand-off through LDS
  // needs no s_barrier and no lgkmcnt drain -- only that the compiler keeps the program order of the LDS accesses around this
  // point ("memory" clobber).  Rounds 1-2 also retired the wave's LDS operations here (s_waitcnt lgkmcnt(0), a leftover of the
  // float atomics); without it the results are bit-identical and the launch 1.2 % shorter (tools/variant_bench.py).
#ifndef RR_SYNC_WAIT
#define RR_SYNC_WAIT 0      // 1: also retire the LDS operations at every hand-off (round 1-2 behaviour; bit-identical results, +1.2 % launch time)
#endif
  __device__ __forceinline__ void sync() {
#if RR_SYNC_WAIT
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#else
    asm volatile("" ::: "memory");
#endif
    __builtin_amdgcn_wave_barrier();
  }
  __device__ __forceinline__ v3 get_com(int r) const {
    return mk3(r ? com1[0] : com0[0], r ? com1[1] : com0[1], r ? com1[2] : com0[2]);
  }
  // wave priority of the throughput-bound phases: by the environment's weight (contacts in penetration), see the kernel body
  __device__ __forceinline__ void env_prio() const {
#if !RR_ENV_PRIO
    __builtin_amdgcn_s_setprio(0);
    return;
#endif
    // ... raised for an environment that has fallen behind the others of a multi-step launch (lag_prio, set by the kernel per env step)
    const int by_weight = jnact >= RR_W3 ? 3 : (jnact >= RR_W2 ? 2 : (jnact >= RR_W1 ? 1 : 0));
    int p = by_weight > lag_prio ? by_weight : lag_prio;
    if ((lag_mode & 3) == 1) p = lag_prio;                                         // progress only
    else if ((lag_mode & 3) == 2) p = by_weight + lag_prio > 3 ? 3 : by_weight + lag_prio;
    if (p >= 3) __builtin_amdgcn_s_setprio(3);          // (s_setprio takes an immediate)
    else if (p == 2) __builtin_amdgcn_s_setprio(2);
    else if (p == 1) __builtin_amdgcn_s_setprio(1);
    else __builtin_amdgcn_s_setprio(0);
  }
  // wave-uniform predicate -> scalar branch
  static __device__ __forceinline__ bool uni(bool p) { return __builtin_amdgcn_readfirstlane((int)p) != 0; }
  // A sum the SOLVER branches on (cost, gradient norm, line-search sums, beta): the wave sum, and for PAIR instances the total of the two
  // replicas' wave sums, formed as [wave 0] + [wave 1] by BOTH waves (identical bits, hence identical branches and matching barriers).
  // One s_barrier per exchange: the cells alternate between two buffers, and a wave can reach exchange k + 2 (same buffer as k) only
  // after its partner has passed the barrier of k + 1, i.e. has read the cells of k.
  template <int K>
  __device__ __forceinline__ void solver_sum_n(float* v) {
    wave_sum_n<K>(v);
    if (PAIR) {
      static_assert(K <= 8, "exchange cells");
      float* mine = s_xc + 16 * xpar + 8 * rep;
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) mine[k] = v[k];
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      const float* c = s_xc + 16 * xpar;
#pragma unroll
      for (int k = 0; k < K; ++k) v[k] = c[k] + c[8 + k];
      xpar ^= 1;
    }
  }
  __device__ __forceinline__ float solver_sum(float v) { float t[1] = {v}; solver_sum_n<1>(t); return t[0]; }

  // ---------------------------------------------------------------- A-1 kinematics (pointer doubling)
  // Every body first builds its LOCAL transform (parent frame -> body, all joints applied) in parallel; world
  // poses are then the prefix products along the tree, formed in ceil(log2(depth)) pointer-doubling rounds
  // T[b] <- T[anc_k(b)] o T[b], anc_{k+1} = anc_k o anc_k (ancestor tables in registers), all bodies busy every
  // round, instead of one serial step per tree level (38-39 of them, a handful of active lanes each).
  // Joint anchors / axes are kept in the parent frame (raw, in the cdof cells) and mapped to the world in com_pos.
  // the body of this lane in slot s (0: none)
  __device__ __forceinline__ int body_at(int s) const {
    if constexpr (ROOT) return s == 0 ? (lane < 2 ? lane + RR_LANES : lane) : (lane == 1 ? 1 : 0);
    else return lane + RR_LANES * s;
  }
  __device__ __forceinline__ BodyC bodyc(const RRTables& T, int s) const { return s == 0 ? bc0 : (s == 1 ? bc1 : load_bodyc(T, lane + RR_LANES * s, D.nbody)); }
  // k is a run-time round counter: select the word instead of indexing the register array (a dynamic index would
  // push the whole object into scratch memory)
  __device__ __forceinline__ int anc_at(int s, int k) const { const int wd = k < 4 ? banc[s][0] : banc[s][1]; return (wd >> (8 * (k & 3))) & 255; }

  __device__ __forceinline__ void kinematics() {
    const RRTables T = tables();
#pragma unroll
    for (int s = 0; s < NBS; ++s) {
      const int b = body_at(s);
      if (ROOT && s == 1) {      // the root: its pose is the free joint's coordinates, qpos[0 .. 6]
        if (b == 1) {
          float quat[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) quat[k] = s_qpos[3 + k];
          quat_normalize(quat);
          st3(s_xpos + 3, ld3(s_qpos));
#pragma unroll
          for (int k = 0; k < 4; ++k) s_xquat[4 + k] = quat[k];
        }
        continue;
      }
      if (s > 0 && !__any(b < D.nbody)) continue;
      const BodyC c = bodyc(T, s);
      if (b >= 1 && b < D.nbody) {
        float quat[4], mat[9];
        v3 pos = mk3(c.pos[0], c.pos[1], c.pos[2]);
#pragma unroll
        for (int k = 0; k < 4; ++k) quat[k] = c.quat[k];
#pragma unroll
        for (int jj = 0; jj < 3; ++jj) {     // at most 3 joints per body (checked by the model compiler); unrolled so the
          if (jj >= c.jn) break;             // table reads of joints 1, 2 are requested together, ahead of joint 0's arithmetic
          int jt, qa, da;
          v3 jp, ja;
          float q0;
          if (jj == 0) {
            jt = c.jtype0; qa = c.jqa0; da = c.jda0; q0 = c.jq00;
            jp = mk3(c.jpos0[0], c.jpos0[1], c.jpos0[2]); ja = mk3(c.jaxis0[0], c.jaxis0[1], c.jaxis0[2]);
          } else {   // 2nd / 3rd joint of a multi-joint body: parameters from the tables
            auto ji = row_at(T.jnt_i, 4, c.jadr + jj);
            auto jf = row_at(T.jnt_f, 8, c.jadr + jj);
            jt = ji[0]; qa = ji[1]; da = ji[2]; q0 = jf[6];
            jp = ld3(jf); ja = ld3(jf + 3);
          }
          if (!ROOT && jt == 0) {  // free joint: the pose is the generalised coordinate itself (parent = world)
            pos = ld3(s_qpos + qa);
#pragma unroll
            for (int k = 0; k < 4; ++k) quat[k] = s_qpos[qa + 3 + k];
            quat_normalize(quat);
          } else {  // hinge
            quat_to_mat(mat, quat);
            const v3 anchor = mat_vec(mat, jp) + pos;
            const v3 axis = mat_vec(mat, ja);
            st3(s_cdof + 6 * da, axis);        // raw, parent frame: axis ; anchor
            st3(s_cdof + 6 * da + 3, anchor);
            const float ang = (s_qpos[qa] - q0) * 0.5f;
            float sn, cs;
            sincosf(ang, &sn, &cs);
            float ql[4] = {cs, ja.x * sn, ja.y * sn, ja.z * sn}, qn[4];
            quat_mul(qn, quat, ql);
#pragma unroll
            for (int k = 0; k < 4; ++k) quat[k] = qn[k];
            quat_to_mat(mat, quat);
            pos = anchor - mat_vec(mat, jp);
          }
        }
        st3(s_xpos + 3 * b, pos);
#pragma unroll
        for (int k = 0; k < 4; ++k) s_xquat[4 * b + k] = quat[k];
      }
    }
    sync();
    for (int k = 0; k < D.nround; ++k) {
      float np[NBS][3], nq[NBS][4];
      bool upd[NBS];
#pragma unroll
      for (int s = 0; s < (ROOT ? 1 : NBS); ++s) {      // ROOT: the root has no ancestor
        const int b = body_at(s);
        const int a = anc_at(s, k);
        upd[s] = b >= 1 && b < D.nbody && a != 0;
        if (upd[s]) {
          float qa_[4], qb[4], mat[9];
#pragma unroll
          for (int i = 0; i < 4; ++i) { qa_[i] = s_xquat[4 * a + i]; qb[i] = s_xquat[4 * b + i]; }
          quat_to_mat(mat, qa_);
          const v3 p = ld3(s_xpos + 3 * a) + mat_vec(mat, ld3(s_xpos + 3 * b));
          np[s][0] = p.x; np[s][1] = p.y; np[s][2] = p.z;
          quat_mul(nq[s], qa_, qb);
        }
      }
      sync();
#pragma unroll
      for (int s = 0; s < (ROOT ? 1 : NBS); ++s) {
        if (upd[s]) {
          const int b = body_at(s);
          st3(s_xpos + 3 * b, mk3(np[s][0], np[s][1], np[s][2]));
#pragma unroll
          for (int i = 0; i < 4; ++i) s_xquat[4 * b + i] = nq[s][i];
        }
      }
      sync();
    }
#pragma unroll
    for (int s = 0; s < NBS; ++s) {   // xquat is kept normalised, as the reference does per body
      const int b = body_at(s);
      if (b >= 1 && b < D.nbody) {
        float q[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) q[i] = s_xquat[4 * b + i];
        quat_normalize(q);
#pragma unroll
        for (int i = 0; i < 4; ++i) s_xquat[4 * b + i] = q[i];
      }
    }
    sync();
  }

  // ---------------------------------------------------------------- A-2 com_pos: subtree COM per root, cinert, cdof
  __device__ __forceinline__ void com_pos() {
    const RRTables T = tables();
    float acc[2][3] = {{0, 0, 0}, {0, 0, 0}};
    float xip[NBS][3];
#pragma unroll
    for (int s_ = 0; s_ < NBS; ++s_) {
      // ROOT: slot 1 first, so that lane 1 adds the root's term and then body 65's, the order of the plain map (the += is a fused
      // multiply-add: the order of the two terms decides the rounding)
      const int s = ROOT ? NBS - 1 - s_ : s_;
      const int b = body_at(s);
      xip[s][0] = xip[s][1] = xip[s][2] = 0;
      if (b >= 1 && b < D.nbody) {
        auto bf = row_at(T.body_f, 18, b);
        float bq[4], R[9];
#pragma unroll
        for (int k = 0; k < 4; ++k) bq[k] = s_xquat[4 * b + k];
        quat_to_mat(R, bq);
        v3 xi = ld3(s_xpos + 3 * b) + mat_vec(R, ld3(bf + 7));
        xip[s][0] = xi.x; xip[s][1] = xi.y; xip[s][2] = xi.z;
        const float mass = bf[14];
        if (row_at(T.body_i, RR_BODYI, b)[5] == 0) { acc[0][0] += mass * xi.x; acc[0][1] += mass * xi.y; acc[0][2] += mass * xi.z; }
        else                { acc[1][0] += mass * xi.x; acc[1][1] += mass * xi.y; acc[1][2] += mass * xi.z; }
      }
    }
    wave_sum_n<6>(&acc[0][0]);
    {
      const float rm0 = T.root_mass[0], rm1 = D.nroot > 1 ? T.root_mass[1] : 1.0f;
      for (int k = 0; k < 3; ++k) { com0[k] = acc[0][k] / rm0; com1[k] = acc[1][k] / rm1; }
    }
#pragma unroll
    for (int s = 0; s < NBS; ++s) {
      const int b = body_at(s);
      if (b >= 1 && b < D.nbody) {
        auto bf = row_at(T.body_f, 18, b);
        float q[4], bq[4], iq[4], R[9];
#pragma unroll
        for (int k = 0; k < 4; ++k) { bq[k] = s_xquat[4 * b + k]; iq[k] = bf[10 + k]; }
        quat_mul(q, bq, iq);
        quat_to_mat(R, q);
        const float mass = bf[14];
        const float I0 = bf[15], I1 = bf[16], I2 = bf[17];
        const v3 cm = get_com(row_at(T.body_i, RR_BODYI, b)[5]);
        const float d0 = xip[s][0] - cm.x, d1 = xip[s][1] - cm.y, d2 = xip[s][2] - cm.z;
        float t[9];
#pragma unroll
        for (int rr = 0; rr < 3; ++rr) { t[3 * rr] = R[3 * rr] * I0; t[3 * rr + 1] = R[3 * rr + 1] * I1; t[3 * rr + 2] = R[3 * rr + 2] * I2; }
        float* c = s_cinert + 10 * b;
        c[0] = t[0] * R[0] + t[1] * R[1] + t[2] * R[2] + mass * (d1 * d1 + d2 * d2);
        c[1] = t[3] * R[3] + t[4] * R[4] + t[5] * R[5] + mass * (d0 * d0 + d2 * d2);
        c[2] = t[6] * R[6] + t[7] * R[7] + t[8] * R[8] + mass * (d0 * d0 + d1 * d1);
        c[3] = t[0] * R[3] + t[1] * R[4] + t[2] * R[5] - mass * d0 * d1;
        c[4] = t[0] * R[6] + t[1] * R[7] + t[2] * R[8] - mass * d0 * d2;
        c[5] = t[3] * R[6] + t[4] * R[7] + t[5] * R[8] - mass * d1 * d2;
        c[6] = mass * d0; c[7] = mass * d1; c[8] = mass * d2; c[9] = mass;
      }
    }
    // cdof [mju_dofCom]: hinge raw (axis; anchor) is in the parent frame of the joint's body -> world, then
    // (axis; axis x (com - anchor)); free joint: translations along the world axes, rotations about the body axes
#pragma unroll
    for (int s = 0; s < NVS; ++s) {
      const int d = lane + RR_LANES * s;
      if (d < D.nv) {
        const int kind = ((opaque(dofc0[s]) >> 8) & 15);
        float* c = s_cdof + 6 * d;
        if (kind < 3) {
          c[0] = c[1] = c[2] = 0;
          c[3] = kind == 0; c[4] = kind == 1; c[5] = kind == 2;
        } else {
          const int fb = kind < 6 ? ((opaque(dofc0[s]) >> 16) & 255) : ((opaque(dofc0[s]) >> 24) & 255);     // frame the raw data is expressed in
          float q[4], R[9];
#pragma unroll
          for (int k = 0; k < 4; ++k) q[k] = s_xquat[4 * fb + k];
          quat_to_mat(R, q);
          v3 ax, anchor;
          if (kind < 6) {
            ax = mk3(R[kind - 3], R[3 + kind - 3], R[6 + kind - 3]);
            anchor = ld3(s_xpos + 3 * fb);
          } else {
            ax = mat_vec(R, ld3(c));
            anchor = ld3(s_xpos + 3 * fb) + mat_vec(R, ld3(c + 3));
          }
          st3(c, ax);
          st3(c + 3, cross(ax, get_com(((opaque(dofc0[s]) >> 12) & 15)) - anchor));
        }
      }
    }
    sync();
  }

  // ---------------------------------------------------------------- A-6 com_vel + rne (prefix sums over the tree)
  // cvel[b] = sum over the ancestor chain of each body's own sum(cdof * qvel): an inclusive tree prefix sum by the
  // same pointer-doubling rounds as the kinematics; cdof_dot then needs only the parent's cvel (lane-local loop over
  // the body's dofs), and cacc is a second prefix sum of sum(cdof_dot * qvel) on top of the world's -gravity.
  __device__ __forceinline__ void tree_prefix6(float* arr) {
    for (int k = 0; k < D.nround; ++k) {
      float add[NBS][6];
      bool upd[NBS];
#pragma unroll
      for (int s = 0; s < (ROOT ? 1 : NBS); ++s) {      // ROOT: the root has no ancestor
        const int b = body_at(s);
        const int a = anc_at(s, k);
        upd[s] = b >= 1 && b < D.nbody && a != 0;
        if (upd[s]) {
#pragma unroll
          for (int i = 0; i < 6; ++i) add[s][i] = arr[6 * a + i];
        }
      }
      sync();
#pragma unroll
      for (int s = 0; s < (ROOT ? 1 : NBS); ++s) {
        if (upd[s]) {
          const int b = body_at(s);
#pragma unroll
          for (int i = 0; i < 6; ++i) arr[6 * b + i] += add[s][i];
        }
      }
      sync();
    }
  }

  __device__ __forceinline__ void velocity_sweep() {
    const RRTables T = tables();
    const DT D = phase_dims();   // the run-time scalars this phase reads (dt, gravity, schedule lengths): local to it, like T
    // own contribution of every body
#pragma unroll
    for (int s = 0; s < NBS; ++s) {
      const int b = body_at(s);
      if (ROOT && s == 1) {      // the root: dofs 0 .. 5
        if (b == 1) {
          float v[6] = {0, 0, 0, 0, 0, 0};
          for (int k = 0; k < 6; ++k) {
            const float qv = s_qvel[k];
#pragma unroll
            for (int i = 0; i < 6; ++i) v[i] += s_cdof[6 * k + i] * qv;
          }
#pragma unroll
          for (int i = 0; i < 6; ++i) s_cvel[6 + i] = v[i];
        }
        continue;
      }
      if (s > 0 && !__any(b < D.nbody)) continue;
      const BodyC c = bodyc(T, s);
      if (b >= 1 && b < D.nbody) {
        float v[6] = {0, 0, 0, 0, 0, 0};
        for (int k = 0; k < c.dofnum; ++k) {
          const float qv = s_qvel[c.dofadr + k];
#pragma unroll
          for (int i = 0; i < 6; ++i) v[i] += s_cdof[6 * (c.dofadr + k) + i] * qv;
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) s_cvel[6 * b + i] = v[i];
      }
    }
    sync();
    tree_prefix6(s_cvel);
    // cdof_dot (lane-local) -> own acceleration contribution
#pragma unroll
    for (int s = 0; s < NBS; ++s) {
      const int b = body_at(s);
      if (ROOT && s == 1 && b != 1) continue;
      if (!ROOT && s > 0 && !__any(b < D.nbody)) continue;
      BodyC c;
      if (ROOT && s == 1) { c.parent = 0; c.dofadr = 0; c.dofnum = 6; c.jn = 1; c.jtype0 = 0; }      // the root: child of the world, dofs 0 .. 5
      else c = bodyc(T, s);
      if (b >= 1 && b < D.nbody) {
        const int p = c.parent, da = c.dofadr, dn = c.dofnum;
        float v[6], a[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] = s_cvel[6 * p + k];
        const bool is_free = ROOT ? s == 1 : (c.jn > 0 && c.jtype0 == 0);
        if (is_free) {
          for (int k = 0; k < 3; ++k) {
            const float qv = s_qvel[da + k];
            for (int i = 0; i < 6; ++i) v[i] += s_cdof[6 * (da + k) + i] * qv;
          }
          for (int k = 0; k < 3; ++k) {   // all three rotational cdof_dot use the velocity after the translations
            float cd[6];
            cross_motion(cd, v, s_cdof + 6 * (da + 3 + k));
            const float qv = s_qvel[da + 3 + k];
            for (int i = 0; i < 6; ++i) a[i] += cd[i] * qv;
          }
        } else {
          for (int k = 0; k < dn; ++k) {
            float cd[6];
            cross_motion(cd, v, s_cdof + 6 * (da + k));
            const float qv = s_qvel[da + k];
            for (int i = 0; i < 6; ++i) { v[i] += s_cdof[6 * (da + k) + i] * qv; a[i] += cd[i] * qv; }
          }
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) s_cacc[6 * b + i] = a[i];
      }
    }
    sync();
    tree_prefix6(s_cacc);
    // body forces: cfrc = I (cacc - g) + cvel x* (I cvel)
#pragma unroll
    for (int s = 0; s < NBS; ++s) {
      const int b = body_at(s);
      if (b >= 1 && b < D.nbody) {
        float v[6], a[6], t[6], t1[6], t2[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) { v[k] = s_cvel[6 * b + k]; a[k] = s_cacc[6 * b + k]; }
        a[3] -= D.gx; a[4] -= D.gy; a[5] -= D.gz;
        mul_inert_vec(t, s_cinert + 10 * b, v);
        cross_force(t1, v, t);
        mul_inert_vec(t2, s_cinert + 10 * b, a);
#pragma unroll
        for (int k = 0; k < 6; ++k) s_cfrc[6 * b + k] = t2[k] + t1[k];
      }
    }
    sync();
  }

  // ---------------------------------------------------------------- crb + cfrc: subtree sums over DFS ranges
  // Bodies are in depth-first order, so the subtree of b is the contiguous range [b, blast[b]]: every lane sums its
  // own range straight from LDS (no level steps, no hand-offs), keeps the 16 sums in registers, and the results are
  // written back in place after all reads.
  __device__ __forceinline__ void backward_sweep() {
    // Bodies are in DFS order, so a subtree is the contiguous range [b, blast]; the root's range is the whole tree (65
    // terms on one lane while most lanes have a handful).  Two levels: sums of aligned blocks of 8 bodies first (all lanes
    // busy, into the dead pose cells), then every lane adds <= 7 head bodies, <= nbody/8 whole blocks and <= 7 tail bodies.
    constexpr int BS = 8;
    const int nblk = (D.nbody + BS - 1) / BS;
    for (int p = lane; p < 10 * nblk; p += RR_LANES) {
      const int blk = p / 10, k = p - 10 * blk;
      float sum = 0.0f;
#pragma unroll
      for (int j = 0; j < BS; ++j) { const int d = blk * BS + j; if (d >= 1 && d < D.nbody) sum += s_cinert[10 * d + k]; }
      s_buf[16 * blk + k] = sum;
    }
    for (int p = lane; p < 6 * nblk; p += RR_LANES) {
      const int blk = p / 6, k = p - 6 * blk;
      float sum = 0.0f;
#pragma unroll
      for (int j = 0; j < BS; ++j) { const int d = blk * BS + j; if (d >= 1 && d < D.nbody) sum += s_cfrc[6 * d + k]; }
      s_buf[16 * blk + 10 + k] = sum;
    }
    sync();
    float acc[NBS][16];
#pragma unroll
    for (int s = 0; s < (ROOT ? 1 : NBS); ++s) {
      const int b = body_at(s);
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[s][k] = 0.0f;
      if (b >= 1 && b < D.nbody) {
        const int e = blast[s] + 1;                                   // range [b, e)
        int d = b;
        const int hb = ((b + BS - 1) & ~(BS - 1)) < e ? ((b + BS - 1) & ~(BS - 1)) : e;
        for (; d < hb; ++d) {
#pragma unroll
          for (int k = 0; k < 10; ++k) acc[s][k] += s_cinert[10 * d + k];
#pragma unroll
          for (int k = 0; k < 6; ++k) acc[s][10 + k] += s_cfrc[6 * d + k];
        }
        for (; d + BS <= e; d += BS) {
          const float* S = s_buf + 2 * d;                             // 16 * (d / 8)
#pragma unroll
          for (int k = 0; k < 16; ++k) acc[s][k] += S[k];
        }
        for (; d < e; ++d) {
#pragma unroll
          for (int k = 0; k < 10; ++k) acc[s][k] += s_cinert[10 * d + k];
#pragma unroll
          for (int k = 0; k < 6; ++k) acc[s][10 + k] += s_cfrc[6 * d + k];
        }
      }
    }
    // ROOT: the root's range is the whole tree, bodies [1, nbody).  One lane would walk it in 16 steps of 16 additions, alone in its slot;
    // lanes 0 .. 15 take one of the 16 components each and make the same additions in the same order: the head bodies up to the first
    // block boundary, the whole blocks, the tail bodies.
    float racc = 0.0f;
    if constexpr (ROOT) {
      if (lane < 16) {
        const bool ci = lane < 10;                                    // components 0 .. 9: cinert, 10 .. 15: cfrc
        const float* one = ci ? s_cinert + lane : s_cfrc + (lane - 10);
        const int st = ci ? 10 : 6;
        int d = 1;
        for (; d < BS && d < D.nbody; ++d) racc += one[st * d];
        for (; d + BS <= D.nbody; d += BS) racc += s_buf[2 * d + lane];
        for (; d < D.nbody; ++d) racc += one[st * d];
      }
    }
    sync();
#pragma unroll
    for (int s = 0; s < (ROOT ? 1 : NBS); ++s) {
      const int b = body_at(s);
      if (b >= 1 && b < D.nbody) {
#pragma unroll
        for (int k = 0; k < 10; ++k) s_crb[10 * b + k] = acc[s][k];
#pragma unroll
        for (int k = 0; k < 6; ++k) s_cfrc[6 * b + k] = acc[s][10 + k];
      }
    }
    if constexpr (ROOT) {
      if (lane < 16) *(lane < 10 ? s_crb + 10 + lane : s_cfrc + 6 + (lane - 10)) = racc;
    }
    sync();
  }

  static constexpr int NME = NVS == 1 ? 10 : (NVS == 2 ? 18 : 35);   // sparse-M entries per lane (nM <= 64*NME)
  __device__ __forceinline__ void load_ment(int* ment) {
    const RRTables T = tables();
    const int ol = opaque(lane);
#pragma unroll
    for (int it = 0; it < NME; ++it) ment[it] = g_int32(T.M_ij_k, ol + RR_LANES * it);
  }
  // ---------------------------------------------------------------- A-3 qM (sparse) from crb and cdof
  __device__ __forceinline__ void mass_matrix() {
#pragma unroll
    for (int s = 0; s < NVS; ++s) {
      const int d = lane + RR_LANES * s;
      if (d < D.nv) mul_inert_vec(s_buf + 6 * d, s_crb + 10 * ((opaque(dofc0[s]) >> 16) & 255), s_cdof + 6 * d);
    }
    int ment[NME];          // entry e = lane + 64*it of qM: row i | col j << 8, -1 beyond nM (table padded to whole rows)
    load_ment(ment);
    sync();
#pragma unroll
    for (int it = 0; it < NME; ++it) {
      const int ij = ment[it];
      if (ij >= 0) {
        const int i = ij & 255, j = ij >> 8;
        float v = dot6(s_cdof + 6 * j, s_buf + 6 * i);
        if (i == j) v = s_arm[i] + v;
        *(rr_f2*)(s_qLD + 2 * (lane + RR_LANES * it)) = rr_f2{v, v};     // pair: M | (damped copy, see factor); one 8-byte store
      }
    }
    sync();
  }

  // Executor of the row schedules of the factorisation and the inversion (rodent_amd/levelsched.py).  A table row is 64
  // independent QUAD operations on the sparse-matrix array s_qLD: four targets d_j -= a * b_j [/ piv], b_j four consecutive
  // entries (the targets of one source row are consecutive entries of an ancestor row, so one shared operand, one reciprocal
  // and one run of four feed four multiply-adds), applied as plain read-modify-writes: no two operations of a row share a
  // target.  NO HAND-OFF BETWEEN ROWS: the LDS instructions of a wavefront execute in program order, so the reads of a row see
  // every write of the rows before it, and all reads of a row are issued before its writes -- the host list-schedules the
  // operations of a whole factorisation as one dependency graph under exactly these two rules (rounds 1-2 ran them level by
  // level of the tree with a hand-off per level: 97 + 63 rows for the rodent, now 57 + 44).  The side branches of a fork
  // accumulate into ALIAS copies of their ancestors' rows (pose cells, dead here), which one merge operation per quad folds
  // in before the row is eliminated -- otherwise the free joint's rows, which every dof updates, serialise the schedule.
  // ATOMIC-FREE: an LDS float atomic costs ~10x a plain read-modify-write on gfx950 and >1000 cycles with every wave of the
  // CU issuing them.  PREDICATE-FREE: the host turns the table's element indices into LDS byte addresses at upload, and
  // empty operations / the unused targets of short runs address the cells ZERO (0.0), ONE (1.0) and TRASH kept behind the
  // nM entries (MINUS_ONE (-1.0) is the shared operand of a merge).
  // 1/piv: v_rcp_f32 refined by one Newton step (the row scaling by 1/D after the sweep uses the exact quotient).
  // Rows (16 B per lane) are prefetched RR_RING ahead; the table ends with 8 >= RR_RING empty rows.
  typedef float __attribute__((address_space(3)))* rr_lf;
  static __device__ __forceinline__ float lds_ld(int byte_adr) { return *(rr_lf)(size_t)(unsigned)byte_adr; }
  static __device__ __forceinline__ void lds_st(int byte_adr, float v) { *(rr_lf)(size_t)(unsigned)byte_adr = v; }
  typedef int rr_v4i __attribute__((ext_vector_type(4)));
  // PAIRS: the step factorises two matrices of identical sparsity every substep -- M for the solver and
  // M + dt*diag(damping) for eulerdamp.  They are stored interleaved (float2 per entry), so one 8-byte LDS operation
  // serves both: the table stream, the address extraction and the LDS round trip of a row are shared.
  typedef rr_f2 __attribute__((address_space(3)))* rr_lf2;
  static __device__ __forceinline__ rr_f2 lds_ld2(int byte_adr) { return *(rr_lf2)(size_t)(unsigned)byte_adr; }
  static __device__ __forceinline__ void lds_st2(int byte_adr, rr_f2 v) { *(rr_lf2)(size_t)(unsigned)byte_adr = v; }
  // SHIFT: the schedules' LDS addresses are baked for the pair array at o_qLD; `delta` (bytes) moves them to another pair array
  // (alias-free schedules only: the alias cells are not part of the array)
  struct RowAdr { int a8, p8, b8, d8[4]; };
  template <bool DIV, bool SHIFT>
  static __device__ __forceinline__ RowAdr row_adr(const rr_v4i& e, int delta) {
    const int sh = SHIFT ? delta : 0;
    RowAdr r;
    r.a8 = (e.x & 0xFFFF) + sh; r.b8 = (int)((unsigned)e.x >> 16) + sh;
    r.p8 = DIV ? r.a8 - e.w + 8 : 0;
    r.d8[0] = (e.y & 0xFFFF) + sh; r.d8[1] = (int)((unsigned)e.y >> 16) + sh; r.d8[2] = (e.z & 0xFFFF) + sh; r.d8[3] = (int)((unsigned)e.z >> 16) + sh;
    return r;
  }
  template <bool DIV, bool SHIFT = false>
  __device__ __forceinline__ void run_levels(rr_gi table, int nrows, int delta = 0) {
    typedef const rr_v4i __attribute__((address_space(1)))* rr_gv4;
    typedef const char __attribute__((address_space(1)))* rr_gc;
    const rr_gc tab = (rr_gc)table;                         // wave-uniform base + 16 * lane: the row's address needs no vector arithmetic
    const unsigned lane16 = 16u * (unsigned)lane;
    constexpr int ROWB = RR_LANES * 16;
    rr_v4i ring[RR_RING];
#pragma unroll
    for (int u = 0; u < RR_RING; ++u) ring[u] = *(rr_gv4)(tab + u * ROWB + lane16);
    RowAdr cur = row_adr<DIV, SHIFT>(ring[0], delta);
    for (int r0 = 0; r0 < nrows; r0 += RR_RING) {
      const rr_gc nxt_rows = tab + (size_t)(r0 + RR_RING) * ROWB;
#pragma unroll
#if RR_WIDE == 2
      // EXPERIMENT: table rows in pairs -- the reads of both rows before the writes of either (a row of 128 operations, two per lane)
      for (int u = 0; u < RR_RING; u += 2) {
        if (u && r0 + u >= nrows) break;
        const RowAdr c0 = cur, c1 = row_adr<DIV, SHIFT>(ring[u + 1], delta);
        const rr_f2 va0 = lds_ld2(c0.a8), va1 = lds_ld2(c1.a8);
        rr_f2 vp0 = {1.0f, 1.0f}, vp1 = {1.0f, 1.0f};
        if (DIV) { vp0 = lds_ld2(c0.p8); vp1 = lds_ld2(c1.p8); }
        rr_f2 vb0[4], vo0[4], vb1[4], vo1[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) vb0[j] = lds_ld2(c0.b8 + 8 * j);
#pragma unroll
        for (int j = 0; j < 4; ++j) vo0[j] = lds_ld2(c0.d8[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) vb1[j] = lds_ld2(c1.b8 + 8 * j);
#pragma unroll
        for (int j = 0; j < 4; ++j) vo1[j] = lds_ld2(c1.d8[j]);
        ring[u] = *(rr_gv4)(nxt_rows + u * ROWB + lane16);
        ring[u + 1] = *(rr_gv4)(nxt_rows + (u + 1) * ROWB + lane16);
        const RowAdr nxt = row_adr<DIV, SHIFT>(ring[(u + 2) % RR_RING], delta);
        rr_f2 t0 = va0, t1 = va1;
        if (DIV) {
          rr_f2 r0_ = {__builtin_amdgcn_rcpf(vp0.x), __builtin_amdgcn_rcpf(vp0.y)}, r1_ = {__builtin_amdgcn_rcpf(vp1.x), __builtin_amdgcn_rcpf(vp1.y)};
          r0_ = r0_ * (2.0f - vp0 * r0_); r1_ = r1_ * (2.0f - vp1 * r1_);
          t0 *= r0_; t1 *= r1_;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) lds_st2(c0.d8[j], vo0[j] - vb0[j] * t0);
#pragma unroll
        for (int j = 0; j < 4; ++j) lds_st2(c1.d8[j], vo1[j] - vb1[j] * t1);
        cur = nxt;
      }
      if (true) continue;
#endif
      for (int u = 0; u < RR_RING; ++u) {
        if (u && r0 + u >= nrows) break;            // wave-uniform: the schedule need not fill its last ring
        const rr_f2 va = lds_ld2(cur.a8);
        rr_f2 vp = {1.0f, 1.0f};
        if (DIV) vp = lds_ld2(cur.p8);
        rr_f2 vb[4], vo[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) vb[j] = lds_ld2(cur.b8 + 8 * j);
#pragma unroll
        for (int j = 0; j < 4; ++j) vo[j] = lds_ld2(cur.d8[j]);
        // under the latency of these reads: the ring's refill and the NEXT row's addresses (ring[u + 1] arrived rows ago)
        ring[u] = *(rr_gv4)(nxt_rows + u * ROWB + lane16);
        const RowAdr nxt = row_adr<DIV, SHIFT>(ring[(u + 1) % RR_RING], delta);
        rr_f2 t = va;
        if (DIV) {
          rr_f2 r = {__builtin_amdgcn_rcpf(vp.x), __builtin_amdgcn_rcpf(vp.y)};
          r = r * (2.0f - vp * r);
          t *= r;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) lds_st2(cur.d8[j], vo[j] - vb[j] * t);
        cur = nxt;
      }
    }
  }

  // sparse L'DL in place in s_qLD  [MuJoCo mj_factorM]; damp = dt for the eulerdamp matrix M + dt*diag(damping).
  // The rank-1 updates M[anc_p][anc_q] -= M[k][anc_p] M[k][anc_q] / M[k][k] of all dofs k, as quad operations in the row order
  // of k_factor3 (run_levels); rows are scaled by 1/D afterwards.
  // Both matrices at once: entry e of the array is the pair (M_e, M_e + dt*damping on the diagonal); mass_matrix has
  // written both halves, the damping is added here.  (M itself is not needed afterwards: the one product with M of the
  // substep, M * qacc_warmstart, is taken before.)
  __device__ __forceinline__ void factor() {
    int ment[NME];          // for the row scaling at the end; requested now, local to this call (not held across the solver)
    load_ment(ment);
    const RRTables T = tables();
    const DT D = phase_dims();   // the run-time scalars this phase reads (dt, gravity, schedule lengths): local to it, like T
    if (lane < 8) s_qLD[2 * D.nM + lane] = (lane >> 1) == 1 ? 1.0f : ((lane >> 1) == 3 ? -1.0f : 0.0f);     // cells ZERO, ONE, TRASH, MINUS_ONE of the row schedules
    for (int c = lane; c < 2 * D.nalias; c += RR_LANES) s_buf[c] = 0.0f;      // alias copies of the hot rows (levelsched.py): pose cells, dead from here to the row scaling
#pragma unroll
    for (int s = 0; s < NVS; ++s) {
      const int d = lane + RR_LANES * s;
      if (d < D.nv) s_qLD[2 * (opaque(dofc1[s]) & 0xFFFF) + 1] += D.dt * row_at(T.dof_f, 16, d)[1];
    }
    sync();
    run_levels<true>(PAIR ? TL.factor3 + rep * D.fac_stride : TL.factor3, D.nfac);
    sync();
#pragma unroll
    for (int s = 0; s < NVS; ++s) {
      const int d = lane + RR_LANES * s;
      const rr_f2 dd = d < D.nv ? *(const rr_f2*)(s_qLD + 2 * (opaque(dofc1[s]) & 0xFFFF)) : rr_f2{1.0f, 1.0f};
      dinv[s] = d < D.nv ? 1.0f / dd.x : 0.0f;
      dinvB[s] = d < D.nv ? 1.0f / dd.y : 0.0f;
      if (d < D.nv) *(rr_f2*)(s_buf + 2 * d) = rr_f2{dinv[s], dinvB[s]};   // 1/D pairs per dof for the row scaling below (dead pose cells)
    }
    sync();
#pragma unroll
    for (int it = 0; it < NME; ++it) {
      const int ij = ment[it];
      if (ij >= 0) {
        const int i = ij & 255, j = ij >> 8;
        if (i != j) *(rr_f2*)(s_qLD + 2 * (lane + RR_LANES * it)) *= *(const rr_f2*)(s_buf + 2 * i);
      }
    }
    sync();
  }

  // W = I - L^-1 (strictly lower part) in place of L: L^-1 has the tree sparsity of L (non-zero only for j an ancestor of
  // i).  The triangular solves of mj_solveLD are chains of ~2*depth dependent LDS hand-offs each and the step makes 11
  // of them per factorisation; with W they become two independent sparse products (ldl_solve).  Gauss-Jordan, shallow dofs
  // first (k_linv, a row program like the factorisation's): for dof k every descendant row i does W_ia -= W_ik W_ka over the
  // strict ancestors a of k; W_ik must still hold L_ik (deeper dofs overwrite it later) and row k must be final.
  __device__ __forceinline__ void invert() {
    const DT D = phase_dims();   // the run-time scalars this phase reads (dt, gravity, schedule lengths): local to it, like T
    run_levels<false>(PAIR ? TL.linv + rep * D.inv_stride : TL.linv, D.ninv);
  }

  // x <- (L' D L)^-1 x = U D^-1 U' x  [MuJoCo mj_solveLD] with the explicit inverse factor U = I - W (see invert): no
  // dependent chain, no atomics.  U' b sums column j over its descendants i (a contiguous DFS range, entry (i, j) at
  // base[i] - depth[j]); U y sums row i over its ancestors (entry (i, p) at Madr[i] + p).  Both products are nM - nv
  // multiply-adds but the longest column / row is ~nv / ~depth long, so each is cut into balanced pieces of at most
  // D.lmax (<= 16) entries, one piece per lane and job slot (k_coljob / k_rowjob); the piece sums go through the (dead)
  // pose cells s_buf and the owner lane of the column / row adds up its pieces.  Lane d owns x_d.
  static constexpr int NJS = NVS >= 3 ? NVS + 1 : NVS;      // job slots per lane (ktables: nslot)
  // This lane's jobs (rodent_amd/ktables.py), loaded from the L2-resident tables (once per substep, or with RR_JOBS_RESIDENT 0
  // per call: see jobs_res below).  PREDICATE-FREE: every job runs D.lmax steps; a column job lists the byte offsets of its matrix
  // entries (padding: the matrix array's ZERO cell) and walks the vector from i0, a row job lists its ancestor dof ids
  // (padding: vector cell nv, which always holds 0) and walks the matrix row from byte offset ra.
  struct Jobs { int cw[NJS][8], ci0[NJS], rb[NJS][4], ra[NJS], own[NVS]; };
  __device__ __forceinline__ void load_jobs(Jobs& j) { load_jobs(j, TL.coljob, TL.rowjob, TL.jobown); }
  template <class P, bool CW = true>
  __device__ __forceinline__ void load_jobs(Jobs& j, P coljob, P rowjob, P jobown) {
    constexpr int WJ = NJS * RR_LANES;
    const int ol = opaque(lane);
    const rr_row<int> cj = row_at(coljob, 1, ol), rj = row_at(rowjob, 1, ol), jo = row_at(jobown, 1, ol);   // one 32-bit lane offset, the rest immediates
#pragma unroll
    for (int s = 0; s < NJS; ++s) {
#pragma unroll
      for (int k = 0; k < 8; ++k) if (CW) j.cw[s][k] = 2 * k < D.lmax ? cj[k * WJ + s * RR_LANES] : 0;
      j.ci0[s] = cj[8 * WJ + s * RR_LANES];
#pragma unroll
      for (int k = 0; k < 4; ++k) j.rb[s][k] = 4 * k < D.lmax ? rj[k * WJ + s * RR_LANES] : 0;
      j.ra[s] = rj[4 * WJ + s * RR_LANES];
    }
#pragma unroll
    for (int s = 0; s < NVS; ++s) j.own[s] = ol + RR_LANES * s < D.nv ? jo[RR_LANES * s] : 0;
  }
  // RR_JOBS_RESIDENT: the descriptors depend on the lane alone, and a substep uses them 11-12 times (M * qacc_warmstart, the solve for
  // qacc_smooth, one solve per CG iteration, the eulerdamp solve).  Each reload is ~30 global loads whose L2 round trip the first
  // product of the call waits for.  The instances now sit well below the register cap (the reload dates from when they sat on it), so
  // the substep loads them once, ahead of M * qacc_warmstart (load_jobs_resident), and every solve / product up to euler() reads
  // this copy.  The opaque lane id in load_jobs keeps the load inside the substep: nothing is carried across the tree phases.
  // The three table pointers are then read from the kernel arguments where the load stands, once per substep, instead of living in
  // scalar registers through the launch for the per-call reloads.  The debug-dump instances (JRES false) keep the reload: with their
  // dump paths the resident copy does not fit their registers.
  static constexpr bool JOBS_RES = RR_JOBS_RESIDENT != 0 && JRES;
  static constexpr bool MAT_RES = RR_SOLVE_MAT_RESIDENT != 0 && MRES > 0 && !NEWTON && !PAIR && JOBS_RES && !rr_same<DT, RRDims>::value;      // see below
  static constexpr bool CW_RES = !MAT_RES;      // the column jobs' matrix offsets stay resident only where the solver still reads them
  Jobs jobs_res;
  __device__ __forceinline__ void load_jobs_resident() {
    if constexpr (JOBS_RES) { const RRTables T = load_tables(); load_jobs<rr_gi, CW_RES>(jobs_res, T.coljob, T.rowjob, T.jobown); }
  }
  // !CW_RES (see MAT_RES below): the column jobs' matrix offsets are not held; the three calls that still gather through them (mul_m, the
  // loader of the resident entries, the damped solve of euler()) load them into the same members first, and they are dead in between.
  __device__ __forceinline__ void load_cw() {
    if constexpr (JOBS_RES && !CW_RES) {
      constexpr int WJ = NJS * RR_LANES;
      const RRTables T = load_tables();
      const rr_row<int> cj = row_at(T.coljob, 1, opaque(lane));
#pragma unroll
      for (int s = 0; s < NJS; ++s) {
#pragma unroll
        for (int k = 0; k < 8; ++k) jobs_res.cw[s][k] = 2 * k < D.lmax ? cj[k * WJ + s * RR_LANES] : 0;
      }
    }
  }
  // The resident copy as values the optimiser has not seen before (in place: no instruction, no register).  Without this it takes the
  // unpacked offsets and ids of one call for those of the next, keeps them all alive across the solver and runs out of registers.
  // Fixed dimensions: the entries beyond lmax are constants and stay so; run-time dimensions: every entry (no branch around nothing).
  __device__ __forceinline__ void jobs_fresh() {
    constexpr bool ALL = rr_same<DT, RRDims>::value;
#pragma unroll
    for (int s = 0; s < NJS; ++s) {
#pragma unroll
      for (int k = 0; k < 8; ++k) if (CW_RES && (ALL || 2 * k < D.lmax)) asm volatile("" : "+v"(jobs_res.cw[s][k]));
      asm volatile("" : "+v"(jobs_res.ci0[s]));
#pragma unroll
      for (int k = 0; k < 4; ++k) if (ALL || 4 * k < D.lmax) asm volatile("" : "+v"(jobs_res.rb[s][k]));
      asm volatile("" : "+v"(jobs_res.ra[s]));
    }
#pragma unroll
    for (int s = 0; s < NVS; ++s) asm volatile("" : "+v"(jobs_res.own[s]));
  }
  // RR_SOLVE_MAT_RESIDENT: the inverse factor W stands still from invert() to the next substep's mass_matrix(), and about nine of the
  // substep's solves are with its M half (qacc_smooth, one per CG iteration).  Each of them gathered this lane's lmax entries per job
  // and side from LDS again -- the costliest reads of the solve by bank conflicts (every M-half entry lies on an even dword: 16 banks),
  // the column side with two instructions of offset arithmetic per entry on top.  The substep reads them once, after invert()
  // (load_mat_resident: the addresses of col_piece / row_piece), and ldl_solve_on<false> multiplies from registers, in the same order
  // from the same 0.0f.  A padded column step holds the ZERO cell's 0.0f, a padded row step whatever finite entry follows the row
  // (its vector cell is the zero at nv), as in LDS: the loops stay predicate-free.  The damped solve of euler(), mul_m (on M, before
  // the factorisation) and every Newton / PAIR / debug / run-time-dimension instance keep the gathers.  MRES picks the sides by the
  // instance's registers: +12 values per side and job slot, and the solver no longer reads the column jobs' matrix offsets, so they
  // leave the resident descriptors (CW_RES, load_cw: -12).  Timed instance: 217 -> 253 VGPRs with both sides, 229 with the column side.
  static constexpr bool MAT_RES_ROW = MAT_RES && MRES > 1;
  static constexpr int MRL = 12;      // == D.lmax of the fixed-dimension instances
  float mres_c[NJS][MRL], mres_r[NJS][MRL];
  __device__ __forceinline__ void load_mat_resident() {
    if constexpr (MAT_RES) {
      static_assert(DT::lmax == MRL, "resident matrix entries: one register per step of a job");
      sync();     // the inversion's last rows were written by other lanes
      jobs_fresh();
      load_cw();
#pragma unroll
      for (int s = 0; s < NJS; ++s) {
#pragma unroll
        for (int t = 0; t < MRL; ++t) mres_c[s][t] = *(const float*)((const char*)s_qLD + ((jobs_res.cw[s][t >> 1] >> (16 * (t & 1))) & 0xFFFF));
        if constexpr (MAT_RES_ROW) {
          const float* m_ = (const float*)((const char*)s_qLD + jobs_res.ra[s]);
#pragma unroll
          for (int t = 0; t < MRL; ++t) mres_r[s][t] = m_[2 * t];
        }
      }
    }
  }
  // The resident entries as values the optimiser has not seen before, like jobs_fresh(): nothing derived from them outlives a call.
  __device__ __forceinline__ void mat_fresh() {
#pragma unroll
    for (int s = 0; s < NJS; ++s) {
#pragma unroll
      for (int t = 0; t < MRL; ++t) {
        asm volatile("" : "+v"(mres_c[s][t]));
        if constexpr (MAT_RES_ROW) asm volatile("" : "+v"(mres_r[s][t]));
      }
    }
  }
  __device__ __forceinline__ float col_piece_res(int s, const float* vec) const {
    const float* v = vec + jobs_res.ci0[s];
    float vv[MRL], acc = 0.0f;      // every read ahead of the first multiply-add: see row_piece_res
#pragma unroll
    for (int t = 0; t < MRL; ++t) vv[t] = v[t];
#pragma unroll
    for (int t = 0; t < MRL; ++t) acc += mres_c[s][t] * vv[t];
    return acc;
  }
  __device__ __forceinline__ float row_piece_res(int s, const float* vec) const {
    // With the resident values live the solver runs close to the register cap, and there the instruction scheduler leaves a region as
    // it found it.  Written as read, multiply-add, read ... the products came out in that order, one exposed LDS round trip per pair of
    // entries (measured: +1.8 % launch time against the gathers), so the source has the vector reads first.
    float vv[MRL], acc = 0.0f;
#pragma unroll
    for (int t = 0; t < MRL; ++t) vv[t] = vec[(jobs_res.rb[s][t >> 2] >> (8 * (t & 3))) & 255];
#pragma unroll
    for (int t = 0; t < MRL; ++t) acc += mres_r[s][t] * vv[t];
    return acc;
  }
  // column piece: sum_t mat[cw_t] * vec[i0 + t];  row piece: sum_t mat[ra + t] * vec[rb_t]   (mat = one half of the pair array)
  __device__ __forceinline__ float col_piece(const Jobs& j, int s, const float* mat, const float* vec) const {
    const float* v = vec + j.ci0[s];
    float acc = 0.0f;
#pragma unroll
    for (int t = 0; t < 16; ++t)
      if (t < D.lmax) acc += *(const float*)((const char*)mat + ((j.cw[s][t >> 1] >> (16 * (t & 1))) & 0xFFFF)) * v[t];
    return acc;
  }
  __device__ __forceinline__ float row_piece(const Jobs& j, int s, const float* mat, const float* vec) const {
    const float* m_ = (const float*)((const char*)mat + j.ra[s]);
    float acc = 0.0f;
#pragma unroll
    for (int t = 0; t < 16; ++t)
      if (t < D.lmax) acc += m_[2 * t] * vec[(j.rb[s][t >> 2] >> (8 * (t & 3))) & 255];
    return acc;
  }
  // sum of the c <= cmax consecutive piece sums of this lane's column / row (fixed trip count, reads masked by select)
  static __device__ __forceinline__ float merge_pieces(const float* part, int t0, int c, int cmax) {
    float sum = 0.0f;
#pragma unroll
    for (int r = 0; r < 8; ++r)
      if (r < cmax) { const float v = part[t0 + r]; sum += r < c ? v : 0.0f; }
    return sum;
  }
  // DAMPED = true: the factor of M + dt*diag(damping) (second half of the pairs, dinvB)
  template <bool DAMPED = false>
  __device__ __forceinline__ void ldl_solve(float* x) { ldl_solve_on<DAMPED>(x, s_qLD + (DAMPED ? 1 : 0), DAMPED ? dinvB : dinv); }
  // mat: one half of a pair array holding an inverse factor; di: its 1/D
  template <bool DAMPED = false>
  __device__ __forceinline__ void ldl_solve_on(float* x, const float* mat, const float* di) {
    Jobs jl;
    if constexpr (!JOBS_RES) load_jobs(jl);
    else jobs_fresh();
    const Jobs& jb = JOBS_RES ? jobs_res : jl;
    // the undamped solves of a MAT_RES instance are all with W's M half in s_qLD (its Newton instances, which solve with s_H, have none)
    constexpr bool RES = MAT_RES && !DAMPED;
    if constexpr (RES) mat_fresh();
    else load_cw();
#pragma unroll
    for (int s = 0; s < NVS; ++s) { const int d = lane + RR_LANES * s; if (d < D.nv) s_x[d] = x[s]; }
    sync();
#pragma unroll
    for (int s = 0; s < NJS; ++s) s_buf[s * RR_LANES + lane] = RES ? col_piece_res(s, s_x) : col_piece(jb, s, mat, s_x);
    sync();
    float y[NVS];
#pragma unroll
    for (int s = 0; s < NVS; ++s) {
      y[s] = (x[s] - merge_pieces(s_buf, jb.own[s] & 255, (jb.own[s] >> 8) & 255, D.cmax)) * di[s];
    }
    // every lane has taken its column pieces of x (hand-off above): the vector cells can take y
#pragma unroll
    for (int s = 0; s < NVS; ++s) { const int d = lane + RR_LANES * s; if (d < D.nv) s_x[d] = y[s]; }
    sync();
#pragma unroll
    for (int s = 0; s < NJS; ++s) s_buf[s * RR_LANES + lane] = (RES && MAT_RES_ROW) ? row_piece_res(s, s_x) : row_piece(jb, s, mat, s_x);
    sync();
#pragma unroll
    for (int s = 0; s < NVS; ++s) {
      x[s] = y[s] - merge_pieces(s_buf, (jb.own[s] >> 16) & 255, (int)((unsigned)jb.own[s] >> 24), D.rmax);
    }
    sync();     // s_buf is reused by the next solve
  }

  // y = M * s_vec (s_vec must be visible).  Row i of the symmetric product is its ancestor part (entries of row i) plus
  // its descendant part (entries (k, i) of the rows below): the two sparse products of ldl_solve on the same vector, with
  // the same balanced jobs (k_coljob / k_rowjob), on the first half of the pairs while it still holds M.  No atomics.
  __device__ __forceinline__ void mul_m(float* y) { mul_m_on(y, s_qLD); }
  __device__ __forceinline__ void mul_m_on(float* y, const float* mp) {
    constexpr int WJ = NJS * RR_LANES;
    Jobs jl;
    if constexpr (!JOBS_RES) load_jobs(jl);
    else jobs_fresh();
    load_cw();
    const Jobs& jb = JOBS_RES ? jobs_res : jl;
#pragma unroll
    for (int s = 0; s < NJS; ++s) {
      s_buf[s * RR_LANES + lane] = col_piece(jb, s, mp, s_vec);
      s_buf[WJ + s * RR_LANES + lane] = row_piece(jb, s, mp, s_vec);
    }
    sync();
#pragma unroll
    for (int s = 0; s < NVS; ++s) {
      const int d = lane + RR_LANES * s;
      float sum = 0.0f;
      if (d < D.nv) {
        sum = mp[2 * (opaque(dofc1[s]) & 0xFFFF)] * s_vec[d];
        sum += merge_pieces(s_buf, jb.own[s] & 255, (jb.own[s] >> 8) & 255, D.cmax);
        sum += merge_pieces(s_buf + WJ, (jb.own[s] >> 16) & 255, (int)((unsigned)jb.own[s] >> 24), D.rmax);
      }
      y[s] = sum;
    }
    sync();
  }

  __device__ __forceinline__ void put_vec(const float* x) {
    sync();  // previous readers of s_vec are done
#pragma unroll
    for (int s = 0; s < NVS; ++s) {
      const int d = lane + RR_LANES * s;
      if (d < D.nv) s_vec[d] = x[s];
    }
    sync();
  }

  // ---------------------------------------------------------------- passive + actuation + qfrc_smooth (per dof)
  __device__ __forceinline__ void smooth_forces(float* bias_out, float* passive_out) {
    const RRTables T = tables();
    if (DYN) {      // transmission with several joints per actuator (fixed tendons [REF models/rodent_cpu.xml:505-560]; UP mjx smooth.transmission):
                    // lane = actuator: length = sum coef qpos, velocity = sum coef qvel, force -> the (dead) pose cells, read per dof below
      if (lane < D.nu) {
        const int u = lane, e0 = T.act_i[2 * u], ne = T.act_i[2 * u + 1];
        float len = 0.0f, vel = 0.0f;
        for (int e = 0; e < ne; ++e) {
          const float c = T.act_m_f[e0 + e];
          len += c * s_qpos[T.act_m_i[2 * (e0 + e) + 1]];
          vel += c * s_qvel[T.act_m_i[2 * (e0 + e)]];
        }
        auto af = row_at(T.act_f, 8, u);
        s_buf[u] = af[0] * s_act[u] + af[1] + af[2] * len + af[3] * vel;
      }
      sync();
    }
#pragma unroll
    for (int s = 0; s < NVS; ++s) {
      const int d = lane + RR_LANES * s;
      qfrc_smooth[s] = 0.0f;
      bias_out[s] = passive_out[s] = 0.0f;
      if (d < D.nv) {
        auto di = row_at(T.dof_i, RR_DOFI, d);
        auto df = row_at(T.dof_f, 16, d);
        const float qv = s_qvel[d];
        float passive = -df[1] * qv;
        if (di[2] == 6) passive -= df[2] * (s_qpos[di[6]] - df[3]);
        const float bias = dot6(s_cdof + 6 * d, s_cfrc + 6 * ((opaque(dofc0[s]) >> 16) & 255));
        float actf = 0.0f;
        const int u = di[7];
        if (u >= 0) {
          if (DYN) {
            actf = df[14] * s_buf[u];          // moment coefficient of this dof x the actuator's force
          } else {
            auto af = row_at(T.act_f, 8, u);
            const float a = s_act[u];
            actf = af[0] * a + af[1] + af[2] * s_qpos[di[6]] + af[3] * qv;
          }
        }
        s_qact[d] = actf;
        qfrc_smooth[s] = passive - bias + actf;
        bias_out[s] = bias; passive_out[s] = passive;
      }
    }
    if (DYN) sync();      // every lane has read the actuator forces before the pose cells are reused
  }

  // ---------------------------------------------------------------- A-4 collision: contact geometry -> registers
  // Runs right after com_pos while xpos / xquat are still live; the Jacobian is never materialised: a contact keeps
  // its offset from the tree COM and its frame, and J x / J' f are evaluated on the fly from cdof (J-free products).
  __device__ __forceinline__ void contact_geometry(float* dbg, float* o_dist = nullptr, float* o_pos = nullptr, float* o_frame = nullptr) {
    const RRTables T = tables();
    const DT D = phase_dims();   // the run-time scalars this phase reads (dt, gravity, schedule lengths): local to it, like T
#pragma unroll
    for (int cs = 0; cs < NCS; ++cs) {
      const int c = lane + RR_LANES * cs;
      con_act[cs] = false; con_mu[cs] = 0; con_D[cs] = 0; con_nanc[cs] = 0; con_kk[cs] = 0; con_b[cs] = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) { con_aref[cs][k] = 0; con_jar[cs][k] = 0; con_jv[cs][k] = 0; }
#pragma unroll
      for (int k = 0; k < 3; ++k) con_off[cs][k] = 0;
#pragma unroll
      for (int k = 0; k < 9; ++k) con_fr[cs][k] = 0;
      if (c < D.ncon) {
        auto ci = row_at(T.con_i, 8, c);
        auto cf = row_at(T.con_f, 26, c);
        const int kind = ci[0], b = ci[1], r = ci[2];
        float gq[4], bq[4], q[4], gm[9], xm[9];
#pragma unroll
        for (int k = 0; k < 4; ++k) { bq[k] = s_xquat[4 * b + k]; gq[k] = cf[3 + k]; }
        quat_to_mat(xm, bq);
        v3 gp = ld3(s_xpos + 3 * b) + mat_vec(xm, ld3(cf));
        quat_mul(q, bq, gq);
        quat_to_mat(gm, q);
        const v3 size = ld3(cf + 7), n = ld3(cf + 10), pp = ld3(cf + 13);
        v3 fb, pos;
        float dist;
        v3 yb = (n.y > -0.5f && n.y < 0.5f) ? mk3(0, 1, 0) : mk3(0, 0, 1);   // default tangent of make_frame(n)
        if (kind == 3) {  // plane - ellipsoid
          v3 sdir = mk3((gm[0] * n.x + gm[3] * n.y + gm[6] * n.z) * size.x, (gm[1] * n.x + gm[4] * n.y + gm[7] * n.z) * size.y,
                        (gm[2] * n.x + gm[5] * n.y + gm[8] * n.z) * size.z);
          const float nn = sqrtf(dot(sdir, sdir));
          const float inv = nn < RR_MINVAL ? 0.0f : -1.0f / nn;
          v3 sp = mk3(sdir.x * inv * size.x, sdir.y * inv * size.y, sdir.z * inv * size.z);
          v3 pt = mat_vec(gm, sp) + gp;
          dist = dot(n, pt - pp);
          pos = pt - n * (dist * 0.5f);
          v3 bb = yb - n * dot(n, yb);
          fb = bb * (1.0f / sqrtf(dot(bb, bb)));
        } else {
          v3 center = gp;
          const float radius = size.x;
          if (kind == 0) {
            v3 bb = yb - n * dot(n, yb);
            fb = bb * (1.0f / sqrtf(dot(bb, bb)));
          } else {
            const v3 axis = mk3(gm[2], gm[5], gm[8]);
            v3 bb = axis - n * dot(n, axis);
            const float bn = sqrtf(dot(bb, bb));
            fb = bn < 0.5f ? yb : bb * (1.0f / bn);
            center = center + axis * ((kind == 1 ? 1.0f : -1.0f) * size.y);
          }
          dist = dot(center - pp, n) - radius;
          pos = center - n * (radius + 0.5f * dist);
        }
        const v3 fc = cross(n, fb);
        if (dbg) {
          dbg[D.g_con_dist + c] = dist;
          st3(dbg + D.g_con_pos + 3 * c, pos);
          st3(dbg + D.g_con_frame + 9 * c, n); st3(dbg + D.g_con_frame + 9 * c + 3, fb); st3(dbg + D.g_con_frame + 9 * c + 6, fc);
        }
        if (o_dist) o_dist[c] = dist;
        if (o_pos) st3(o_pos + 3 * c, pos);
        if (o_frame) { st3(o_frame + 9 * c, n); st3(o_frame + 9 * c + 3, fb); st3(o_frame + 9 * c + 6, fc); }
        if (dist < 0) {
          con_act[cs] = true;
          float k, bcoef, imp;
          { const float si_[5] = {cf[20], cf[21], cf[22], cf[23], cf[24]}; kbi(D.dt, cf[18], cf[19], si_, dist, k, bcoef, imp); }
          const float rr = fmaxf(cf[17] * (1.0f - imp) / imp, RR_MINVAL);
          con_mu[cs] = cf[16]; con_D[cs] = 1.0f / rr; con_nanc[cs] = ci[4];
          con_kk[cs] = k * imp * dist; con_b[cs] = bcoef;
          const v3 off = pos - get_com(r);
          con_off[cs][0] = off.x; con_off[cs][1] = off.y; con_off[cs][2] = off.z;
          con_fr[cs][0] = n.x; con_fr[cs][1] = n.y; con_fr[cs][2] = n.z;
          con_fr[cs][3] = fb.x; con_fr[cs][4] = fb.y; con_fr[cs][5] = fb.z;
          con_fr[cs][6] = fc.x; con_fr[cs][7] = fc.y; con_fr[cs][8] = fc.z;
        }
        if (dbg) dbg[D.g_con_D + c] = con_D[cs];
      }
    }
  }

  // ---------------------------------------------------------------- DYN: candidate pairs of two moving geoms [UP mjx collision_primitive]
  // closest point of segment [a, b] to pt: t = (pt - a).ab / (ab.ab + 1e-6), clipped  [UP mjx math.closest_segment_point]
  static __device__ __forceinline__ v3 seg_point(v3 a, v3 b, v3 pt) {
    const v3 ab = b - a;
    float t = dot(pt - a, ab) / (dot(ab, ab) + 1e-6f);
    t = fminf(fmaxf(t, 0.0f), 1.0f);
    return a + ab * t;
  }
  // closest points of two segments [UP mjx math.closest_segment_to_segment_points]: line-line solution from the mid-points (denominator
  // + 1e-6), clipped; then each clipped point re-projected on the other segment and the closer pair kept
  static __device__ __forceinline__ void seg_seg(v3 a0, v3 a1, v3 b0, v3 b1, v3& pa, v3& pb) {
    v3 da = a1 - a0, db = b1 - b0;
    const float la = sqrtf(dot(da, da)), lb = sqrtf(dot(db, db));
    da = da * (la > 0.0f ? 1.0f / la : 0.0f); db = db * (lb > 0.0f ? 1.0f / lb : 0.0f);
    const float ha = 0.5f * la, hb = 0.5f * lb;
    const v3 am = a0 + da * ha, bm = b0 + db * hb, tr = am - bm;
    const float dab = dot(da, db), dat = dot(da, tr), dbt = dot(db, tr);
    float ta = (-dat + dab * dbt) / (1.0f - dab * dab + 1e-6f);
    float tb = dbt + ta * dab;
    ta = fminf(fmaxf(ta, -ha), ha);
    tb = fminf(fmaxf(tb, -hb), hb);
    pa = am + da * ta; pb = bm + db * tb;
    const v3 na = seg_point(a0, a1, pb), nb = seg_point(b0, b1, pa);
    const v3 e1 = na - pb, e2 = nb - pa;
    if (dot(e1, e1) < dot(e2, e2)) pa = na; else pb = nb;
  }
  // pair p: signed distance, contact point, normal (geom1 -> geom2); kinds 4 sphere-sphere, 5 sphere-capsule, 6 capsule-capsule
  __device__ __forceinline__ float pair_geometry(const RRTables& T, int p, v3& pos, v3& n) const {
    auto ci = row_at(T.con_i, 8, p);
    auto cf = row_at(T.con_f, 32, p);
    const int kind = ci[0], b1 = ci[1], b2 = ci[2];
    v3 c[2], ax[2];
    float rad[2], hl[2];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const int b = g ? b2 : b1;
      float bq[4], gq[4], q[4], xm[9], gm[9];
#pragma unroll
      for (int k = 0; k < 4; ++k) { bq[k] = s_xquat[4 * b + k]; gq[k] = cf[10 * g + 3 + k]; }
      quat_to_mat(xm, bq);
      c[g] = ld3(s_xpos + 3 * b) + mat_vec(xm, ld3(cf + 10 * g));
      quat_mul(q, bq, gq);
      quat_to_mat(gm, q);
      ax[g] = mk3(gm[2], gm[5], gm[8]);
      rad[g] = cf[10 * g + 7]; hl[g] = cf[10 * g + 8];
    }
    v3 pa = c[0], pb = c[1];
    if (kind == 5) pb = seg_point(c[1] - ax[1] * hl[1], c[1] + ax[1] * hl[1], c[0]);
    else if (kind == 6) seg_seg(c[0] - ax[0] * hl[0], c[0] + ax[0] * hl[0], c[1] - ax[1] * hl[1], c[1] + ax[1] * hl[1], pa, pb);
    const v3 d = pb - pa;
    const float len = sqrtf(dot(d, d));
    n = len == 0.0f ? mk3(1, 0, 0) : d * (1.0f / len);
    const float dist = len - (rad[0] + rad[1]);
    pos = pa + n * (rad[0] + 0.5f * dist);
    return dist;
  }
  // dbg / o_dist / o_pos / o_frame: the debug-dump instance only (compile-time null in every other one).  The dump's contact sections
  // are per CANDIDATE PAIR: dist / pos / frame of every pair come from the scan's own pair_geometry() call, the one whose sign selects the
  // pair; con_D / con_aref of a pair that holds a slot are its slot's (written below and in constraint_rows), of every other pair 0.
  // Behind kernarg_ok: pen_count (pairs in penetration before the clamp to the slots) and slot_pair[WC] (pair id by slot, -1 beyond).
  __device__ __forceinline__ void contact_geometry_dyn(float* dbg = nullptr, float* o_dist = nullptr, float* o_pos = nullptr, float* o_frame = nullptr) {
    const RRTables T = tables();
    const DT D = phase_dims();   // the run-time scalars this phase reads (dt, gravity, schedule lengths): local to it, like T
    int count = 0;
    for (int p0 = 0; p0 < D.ncon; p0 += RR_LANES) {          // scan: which candidate pairs are in penetration
      const int p = p0 + lane;
      bool pen = false;
      if (p < D.ncon) {
        v3 pos_, n_;
        const float dist_ = pair_geometry(T, p, pos_, n_);
        pen = dist_ < 0.0f;
        if (dbg || o_dist || o_pos || o_frame) {
          const v3 yb = (n_.y > -0.5f && n_.y < 0.5f) ? mk3(0, 1, 0) : mk3(0, 0, 1);       // make_frame(n), as the slots form it below
          v3 fb = yb - n_ * dot(n_, yb);
          fb = fb * (1.0f / sqrtf(dot(fb, fb)));
          const v3 fc = cross(n_, fb);
          if (dbg) {
            dbg[D.g_con_dist + p] = dist_;
            st3(dbg + D.g_con_pos + 3 * p, pos_);
            st3(dbg + D.g_con_frame + 9 * p, n_); st3(dbg + D.g_con_frame + 9 * p + 3, fb); st3(dbg + D.g_con_frame + 9 * p + 6, fc);
          }
          if (o_dist) o_dist[p] = dist_;
          if (o_pos) st3(o_pos + 3 * p, pos_);
          if (o_frame) { st3(o_frame + 9 * p, n_); st3(o_frame + 9 * p + 3, fb); st3(o_frame + 9 * p + 6, fc); }
        }
      }
      const unsigned long long mk = __ballot(pen);
      bool slotted = false;
      if (pen) {
        const int slot = count + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mk, 0u));
        if (slot < WC) s_jlist[slot] = p;
        slotted = slot < WC;
      }
      if (dbg && p < D.ncon && !slotted) {      // no cell is written twice: a slotted pair's cells are its slot's to write
        dbg[D.g_con_D + p] = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) dbg[D.g_con_aref + 4 * p + k] = 0.0f;
      }
      count += __popcll(mk);
    }
    if (dbg && lane == 0) dbg[D.g_kaok + RR_DBG_PEN_COUNT] = (float)count;
    dyn_overflow |= count > WC ? 1 : 0;
    if (count > WC) count = WC;
    sync();
    if (dbg) for (int slot = lane; slot < WC; slot += RR_LANES) dbg[D.g_kaok + RR_DBG_SLOT_PAIR + slot] = slot < count ? (float)s_jlist[slot] : -1.0f;
#pragma unroll
    for (int cs = 0; cs < NCS; ++cs) {
      const int slot = lane + RR_LANES * cs;
      con_act[cs] = false; con_mu[cs] = 0; con_D[cs] = 0; con_nanc[cs] = 0; con_kk[cs] = 0; con_b[cs] = 0;
      con_pid[cs] = 0; con_leaf[cs] = 0; con_leaf1[cs] = -1; con_nrow[cs] = 4;
#pragma unroll
      for (int k = 0; k < 4; ++k) { con_aref[cs][k] = 0; con_jar[cs][k] = 0; con_jv[cs][k] = 0; }
#pragma unroll
      for (int k = 0; k < 3; ++k) con_off[cs][k] = 0;
#pragma unroll
      for (int k = 0; k < 9; ++k) con_fr[cs][k] = 0;
      if (slot < count) {
        const int p = s_jlist[slot];
        auto ci = row_at(T.con_i, 8, p);
        auto cf = row_at(T.con_f, 32, p);
        v3 pos, n;
        const float dist = pair_geometry(T, p, pos, n);
        const v3 yb = (n.y > -0.5f && n.y < 0.5f) ? mk3(0, 1, 0) : mk3(0, 0, 1);       // make_frame(n)
        v3 fb = yb - n * dot(n, yb);
        fb = fb * (1.0f / sqrtf(dot(fb, fb)));
        const v3 fc = cross(n, fb);
        con_act[cs] = true;           // the scan selected it: dist < 0 (same arithmetic)
        con_pid[cs] = p; con_leaf1[cs] = ci[5]; con_leaf[cs] = ci[6]; con_nrow[cs] = ci[7]; con_nanc[cs] = ci[4];
        float k, bcoef, imp;
        { const float si_[5] = {cf[24], cf[25], cf[26], cf[27], cf[28]}; kbi(D.dt, cf[22], cf[23], si_, dist, k, bcoef, imp); }
        const float rr = fmaxf(cf[21] * (1.0f - imp) / imp, RR_MINVAL);
        con_mu[cs] = con_nrow[cs] == 1 ? 0.0f : cf[20]; con_D[cs] = 1.0f / rr;
        con_kk[cs] = k * imp * dist; con_b[cs] = bcoef;
        if (dbg) dbg[D.g_con_D + p] = con_D[cs];
        const v3 off = pos - get_com(ci[3]);
        con_off[cs][0] = off.x; con_off[cs][1] = off.y; con_off[cs][2] = off.z;
        con_fr[cs][0] = n.x; con_fr[cs][1] = n.y; con_fr[cs][2] = n.z;
        con_fr[cs][3] = fb.x; con_fr[cs][4] = fb.y; con_fr[cs][5] = fb.z;
        con_fr[cs][6] = fc.x; con_fr[cs][7] = fc.y; con_fr[cs][8] = fc.z;
      }
    }
    sync();
  }

  // ---------------------------------------------------------------- A-5 constraint rows (limits; contact aref)
  __device__ __forceinline__ void constraint_rows(float* dbg) {
    const RRTables T = tables();
    const DT D = phase_dims();   // the run-time scalars this phase reads (dt, gravity, schedule lengths): local to it, like T
#pragma unroll
    for (int s = 0; s < NVS; ++s) {
      const int d = lane + RR_LANES * s;
      lim_act[s] = false; lim_sign[s] = 0; lim_D[s] = 0; lim_aref[s] = 0; lim_jar[s] = 0; lim_jv[s] = 0;
      if (d < D.nv) {
        auto di = row_at(T.dof_i, RR_DOFI, d);
        if (di[8]) {
          auto df = row_at(T.dof_f, 16, d);
          const float q = s_qpos[di[6]];
          const float dmin_ = q - df[4], dmax_ = df[5] - q;
          const float pos = fminf(dmin_, dmax_);
          if (pos < 0) {
            float k, b, imp;
            { const float si_[5] = {df[8], df[9], df[10], df[11], df[12]}; kbi(D.dt, df[6], df[7], si_, pos, k, b, imp); }
            const float r = fmaxf(df[13] * (1.0f - imp) / imp, RR_MINVAL);
            lim_act[s] = true;
            lim_sign[s] = dmin_ < dmax_ ? 1.0f : -1.0f;
            lim_D[s] = 1.0f / r;
            lim_aref[s] = -b * (lim_sign[s] * s_qvel[d]) - k * imp * pos;
          }
          if (dbg) { dbg[D.g_lim + 3 * d] = pos; dbg[D.g_lim + 3 * d + 1] = lim_D[s]; dbg[D.g_lim + 3 * d + 2] = lim_aref[s]; }
        }
      }
    }
    float jq[NCS][4];
    jac_mul(jq, s_qvel);      // J * qvel, pyramid rows
#pragma unroll
    for (int cs = 0; cs < NCS; ++cs) {
      if (con_act[cs]) {
#pragma unroll
        for (int k = 0; k < 4; ++k) con_aref[cs][k] = -con_b[cs] * jq[cs][k] - con_kk[cs];
      }
      const int c = DYN ? con_pid[cs] : lane + RR_LANES * cs;      // DYN: the dump is per candidate pair; the pairs without a slot hold 0 (contact_geometry_dyn)
      if (dbg && (DYN ? con_act[cs] : c < D.ncon)) {
#pragma unroll
        for (int k = 0; k < 4; ++k) dbg[D.g_con_aref + 4 * c + k] = (!DYN || k < con_nrow[cs]) ? con_aref[cs][k] : 0.0f;
      }
    }
  }

  // J * vec is needed only for the contacts in penetration (typically 5-15 of ncon), each a walk of up to 36 dofs along
  // the ancestor chain of its body -- with one lane per contact most lanes idle through 36 dependent LDS rounds.  Once
  // per substep the chains of the contacts in penetration are cut into pieces of 12 / 20 / 36 dofs, 4 / 2 / 1 lanes per
  // contact (as many as fit 64 * NCS lanes), the lanes of a contact adjacent so that a quad DPP add joins the pieces.
  __device__ __forceinline__ void contact_jobs() {
    const RRTables T = tables();
    int n_act = 0;
#pragma unroll
    for (int cs = 0; cs < NCS; ++cs) {
      const unsigned long long m = __ballot(con_act[cs]);
      con_rank[cs] = n_act + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
      n_act += __popcll(m);
    }
    jnact = n_act;
    jP = 4 * n_act <= RR_LANES * NCS ? 4 : (2 * n_act <= RR_LANES * NCS ? 2 : 1);
    jLp = jP == 4 ? 12 : (jP == 2 ? 20 : (DYN ? 40 : 36));
    const int sh = jP == 4 ? 2 : (jP == 2 ? 1 : 0);
#pragma unroll
    for (int cs = 0; cs < NCS; ++cs) {
      const int c = lane + RR_LANES * cs;
      if (DYN) continue;           // DYN: the slots ARE the contacts in penetration (rank = slot) and s_jlist already holds their pair ids
      if (con_act[cs]) s_jlist[con_rank[cs]] = c;
      con_leaf[cs] = c < D.ncon ? (g_int32(TL.con_chain_rows, 9 * c) & 255) : 0;
    }
    sync();
#pragma unroll
    for (int js = 0; js < NCS; ++js) {
      const int J = lane + RR_LANES * js, r = J >> sh, p = J & (jP - 1);
      const int pad = D.nv * 0x01010101;      // dof id nv: zero motion vector, zero vector cell
#pragma unroll
      for (int k = 0; k < JW; ++k) jch[js][k] = pad;
      if (r < n_act) {
        const int c = s_jlist[r], start = p * jLp;
        const int left = row_at(T.con_i, 8, c)[4] - start;
        const int n = left < 0 ? 0 : (left > jLp ? jLp : left);
        const rr_row<int> chain = row_at(TL.con_chain_rows, 1, JW * c + (start >> 2));
#pragma unroll
        for (int k = 0; k < JW; ++k) {
          if (4 * k < jLp) {
            const int v = chain[k];   // the table has a slack row
            const int keep = n - 4 * k;                                          // ids of this int that belong to the piece
            const unsigned msk = keep >= 4 ? 0xFFFFFFFFu : (keep <= 0 ? 0u : (1u << (8 * keep)) - 1u);
            jch[js][k] = (v & msk) | (pad & ~msk);
          }
        }
      }
    }
  }

  // pyramid rows of J * vec for this lane's contacts, J-free: the spatial velocity of the contact body induced by `vec`
  // (sum of cdof * vec over the ancestor chain, by the jobs above: pieces joined by a quad DPP add, handed to the
  // contact's lane through the dead pose cells), taken at the contact point and projected on the frame
  __device__ __forceinline__ void jac_mul(float (*out)[4], const float* vec) {
    const int sh = jP == 4 ? 2 : (jP == 2 ? 1 : 0);
    // LDS byte address of cdof as ONE scalar the optimiser cannot split: a motion vector's address is then a single multiply-add
    // (24 * id + base) and its three 8-byte reads differ by immediates.  Left to itself the optimiser shares 4 * id with the vector
    // read and rebuilds 24 * id + base from it in three instructions per id (shift-add, multiply-add, add of the region offset).
    int cdof8 = (int)(unsigned)(size_t)(rr_lf)s_cdof;
    asm("" : "+s"(cdof8));
#pragma unroll
    for (int js = 0; js < NCS; ++js) {
      float w[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int t0 = 0; t0 < 4 * JW; t0 += 4) {
        if (t0 < jLp) {     // wave-uniform; no per-lane predicate: ids beyond the piece are nv (zero vector)
          const int ids = opaque(jch[js][t0 >> 2]);     // one opaque copy per register of four ids
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int id = (ids >> (8 * u)) & 255;
            const int dd = DYN ? (id & 127) : id;
            float xv = vec[dd];
            if (DYN && (id & 128)) xv = -xv;           // a dof of body1's chain: J = jac(body2) - jac(body1)
            const int ca = cdof8 + 24 * dd;            // rows of cdof are 24 bytes from a 16-byte aligned base: 8-byte reads
            const rr_f2 c01 = lds_ld2(ca), c23 = lds_ld2(ca + 8), c45 = lds_ld2(ca + 16);
            const float cd[6] = {c01.x, c01.y, c23.x, c23.y, c45.x, c45.y};
#pragma unroll
            for (int i = 0; i < 6; ++i) w[i] += cd[i] * xv;
          }
        }
      }
      if (jP >= 2) {
#pragma unroll
        for (int i = 0; i < 6; ++i) w[i] = dpp_add(w[i], 0);
      }
      if (jP == 4) {
#pragma unroll
        for (int i = 0; i < 6; ++i) w[i] = dpp_add(w[i], 1);
      }
      const int J = lane + RR_LANES * js;
      if ((J & (jP - 1)) == 0 && (J >> sh) < jnact) {
#pragma unroll
        for (int i = 0; i < 6; ++i) s_buf[6 * (J >> sh) + i] = w[i];
      }
    }
    sync();
#pragma unroll
    for (int cs = 0; cs < NCS; ++cs) {
      out[cs][0] = out[cs][1] = out[cs][2] = out[cs][3] = 0.0f;
      if (con_act[cs]) {
        const float* w = s_buf + 6 * con_rank[cs];
        const v3 pv = mk3(w[3], w[4], w[5]) + cross(mk3(w[0], w[1], w[2]), mk3(con_off[cs][0], con_off[cs][1], con_off[cs][2]));
        const float jn_ = dot(mk3(con_fr[cs][0], con_fr[cs][1], con_fr[cs][2]), pv);
        const float j1 = dot(mk3(con_fr[cs][3], con_fr[cs][4], con_fr[cs][5]), pv);
        const float j2 = dot(mk3(con_fr[cs][6], con_fr[cs][7], con_fr[cs][8]), pv);
        const float mu = con_mu[cs];
        out[cs][0] = jn_ + mu * j1; out[cs][1] = jn_ - mu * j1; out[cs][2] = jn_ + mu * j2; out[cs][3] = jn_ - mu * j2;
      }
    }
    sync();     // the pose cells are reused (solve partial sums, line-search staging)
  }

  // constraint state at the current Jaref: forces, qfrc_constraint, cost  [UP mjx solver._update_constraint]
  // `walk` (wave-uniform) false: cost only -- no contact is broadcast, and qfrc_con holds the limit forces alone (solve(), context at qacc_smooth)
  __device__ __forceinline__ void update_constraint(bool walk = true) {
    float part[2] = {0.0f, 0.0f};  // [0] = sum D*Jaref^2 over active rows, [1] = gauss dot
    // J' f without a Jacobian and without atomics: a contact pushes with the spatial force (tau about the tree COM, F)
    // on every dof of its body's ancestor chain, qfrc_d += cdof_d . (tau, F).  The wave walks the contacts that carry
    // force (ballot), broadcasts each one's force and leaf dof (readlane), and every dof lane tests "am I on that chain"
    // by the DFS interval  d <= leaf <= last_desc(d).
    float qc[NVS], cd[NVS][6];
#pragma unroll
    for (int s = 0; s < NVS; ++s) {
      const int d = lane + RR_LANES * s;
      qc[s] = 0.0f;
#pragma unroll
      for (int k = 0; k < 6; ++k) cd[s][k] = d < D.nv ? s_cdof[6 * d + k] : 0.0f;
    }
#pragma unroll
    for (int cs = 0; cs < NCS; ++cs) {
      float W[6] = {0, 0, 0, 0, 0, 0};
      bool has = false;
      if (con_act[cs]) {
        float f[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float jr = con_jar[cs][k];
          if (jr < 0 && (!DYN || k < con_nrow[cs])) { f[k] = -con_D[cs] * jr; part[0] += con_D[cs] * jr * jr; }
        }
        const float mu = con_mu[cs];
        const float fn = f[0] + f[1] + f[2] + f[3], f1 = mu * (f[0] - f[1]), f2 = mu * (f[2] - f[3]);
        if (walk && fn != 0.0f) {
          has = true;
          const v3 F = mk3(con_fr[cs][0], con_fr[cs][1], con_fr[cs][2]) * fn + mk3(con_fr[cs][3], con_fr[cs][4], con_fr[cs][5]) * f1 +
                       mk3(con_fr[cs][6], con_fr[cs][7], con_fr[cs][8]) * f2;
          const v3 tau = cross(mk3(con_off[cs][0], con_off[cs][1], con_off[cs][2]), F);
          W[0] = tau.x; W[1] = tau.y; W[2] = tau.z; W[3] = F.x; W[4] = F.y; W[5] = F.z;
        }
      }
      const int leaf = con_leaf[cs];
      unsigned long long mask = __ballot(has);
      while (mask) {
        const int l = __builtin_ctzll(mask);
        mask &= mask - 1;
        float w[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) w[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(W[k]), l));
        const int ld = __builtin_amdgcn_readlane(leaf, l);
        const int ld1 = DYN ? __builtin_amdgcn_readlane(con_leaf1[cs], l) : -1;
#pragma unroll
        for (int s = 0; s < NVS; ++s) {
          if (s > 0 && ld < RR_LANES * s && ld1 < RR_LANES * s) continue;      // wave-uniform: the chains (dofs <= leaf) have no dof in this slot
          const int d = lane + RR_LANES * s;
          if (!DYN) {
            if (d <= ld && ld <= (opaque(dofc1[s]) >> 16))
              qc[s] += cd[s][0] * w[0] + cd[s][1] * w[1] + cd[s][2] * w[2] + cd[s][3] * w[3] + cd[s][4] * w[4] + cd[s][5] * w[5];
          } else {
            const int last = opaque(dofc1[s]) >> 16;
            const bool on2 = d <= ld && ld <= last;
            const bool on1 = ld1 >= 0 && d <= ld1 && ld1 <= last;          // body1's chain: the force enters with a minus sign
            if (on2 != on1) {       // a dof on both chains gets +t - t = 0
              const float t = cd[s][0] * w[0] + cd[s][1] * w[1] + cd[s][2] * w[2] + cd[s][3] * w[3] + cd[s][4] * w[4] + cd[s][5] * w[5];
              qc[s] += on2 ? t : -t;
            }
          }
        }
      }
    }
#pragma unroll
    for (int s = 0; s < NVS; ++s) {
      float qcs = qc[s];
      if (lim_act[s] && lim_jar[s] < 0) {
        const float f = -lim_D[s] * lim_jar[s];
        part[0] += lim_D[s] * lim_jar[s] * lim_jar[s];
        qcs += lim_sign[s] * f;
      }
      qfrc_con[s] = qcs;
      part[1] += (Ma[s] - qfrc_smooth[s]) * (qacc[s] - qacc_smooth[s]);
    }
    solver_sum_n<2>(part);
    gauss = 0.5f * part[1];
    prev_cost = cost;
    cost = 0.5f * part[0] + gauss;
  }

  // ---------------------------------------------------------------- Newton solver [UP mjx solver, SolverType.NEWTON; REF Rodent_Env_Brax.py:42-45]
  // H = M + J' diag(D * active) J.  Every constraint row of these models lives on ONE ancestor chain (a contact's body, a limited
  // dof), so J' D J couples a dof only with its own ancestors: H has exactly M's tree sparsity (entry Madr[i] + p <-> dof i and
  // its p-th ancestor) and is held as a second pair array, factorised and inverted by the SAME level schedules (address shift),
  // and solved by the same balanced jobs.  The contacts in penetration are walked like J' f (ballot + readlane broadcast of the
  // contact's frame); every dof lane on the chain forms its four pyramid-row entries, the rows go through the pose cells, and the
  // lane adds D_k r_k[i] r_k[anc_p(i)] along its own row of H.
  __device__ __forceinline__ void newton_hessian() {
    const int RS = (D.nv + 3) & ~3;                      // row stride in the pose cells: 4 rows of nv floats (4 nv <= 7 nbody + 4, host check)
    for (int e = lane; e < D.nM + 20; e += RR_LANES) *(rr_f2*)(s_H + 2 * e) = *(const rr_f2*)(s_Mp + 2 * e);     // H <- M (with the schedule cells)
    float cd[NVS][6];
#pragma unroll
    for (int s = 0; s < NVS; ++s) {
      const int d = lane + RR_LANES * s;
#pragma unroll
      for (int k = 0; k < 6; ++k) cd[s][k] = d < D.nv ? s_cdof[6 * d + k] : 0.0f;
    }
    sync();
#pragma unroll
    for (int s = 0; s < NVS; ++s) {        // limit rows: J = +-e_d
      if (lim_act[s] && lim_jar[s] < 0) { rr_f2* h = (rr_f2*)(s_H + 2 * (opaque(dofc1[s]) & 0xFFFF)); *h += rr_f2{lim_D[s], lim_D[s]}; }
    }
#pragma unroll
    for (int cs = 0; cs < NCS; ++cs) {
      unsigned long long mask = __ballot(con_act[cs]);
      while (mask) {
        const int l = __builtin_ctzll(mask);
        mask &= mask - 1;
        auto bc = [&](float v) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); };
        const float mu = bc(con_mu[cs]), Dc = bc(con_D[cs]);
        const v3 off = mk3(bc(con_off[cs][0]), bc(con_off[cs][1]), bc(con_off[cs][2]));
        const v3 fn = mk3(bc(con_fr[cs][0]), bc(con_fr[cs][1]), bc(con_fr[cs][2])), f1 = mk3(bc(con_fr[cs][3]), bc(con_fr[cs][4]), bc(con_fr[cs][5])),
                 f2 = mk3(bc(con_fr[cs][6]), bc(con_fr[cs][7]), bc(con_fr[cs][8]));
        float a[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] = bc(con_jar[cs][k]) < 0 ? Dc : 0.0f;
        const int ld = __builtin_amdgcn_readlane(con_leaf[cs], l);
        float r[NVS][4];
        bool on[NVS];
#pragma unroll
        for (int s = 0; s < NVS; ++s) {
          const int d = lane + RR_LANES * s;
          on[s] = d < D.nv && d <= ld && ld <= (opaque(dofc1[s]) >> 16);
          const v3 jp = mk3(cd[s][3], cd[s][4], cd[s][5]) + cross(mk3(cd[s][0], cd[s][1], cd[s][2]), off);
          const float jn = dot(fn, jp), j1 = dot(f1, jp), j2 = dot(f2, jp);
          r[s][0] = on[s] ? jn + mu * j1 : 0.0f; r[s][1] = on[s] ? jn - mu * j1 : 0.0f;
          r[s][2] = on[s] ? jn + mu * j2 : 0.0f; r[s][3] = on[s] ? jn - mu * j2 : 0.0f;
          if (d < D.nv) {
#pragma unroll
            for (int k = 0; k < 4; ++k) s_buf[k * RS + d] = r[s][k];
          }
        }
        sync();
#pragma unroll
        for (int s = 0; s < NVS; ++s) {
          if (s > 0 && ld < RR_LANES * s) continue;            // wave-uniform: no chain dof in this slot
          if (on[s]) {
            const int madr = opaque(dofc1[s]) & 0xFFFF, dep = opaque(dofc0[s]) & 255;
            const float w0 = a[0] * r[s][0], w1 = a[1] * r[s][1], w2 = a[2] * r[s][2], w3 = a[3] * r[s][3];
            for (int p = 0; p <= dep; ++p) {
              const int j = s_anc[madr + p];
              const float v = w0 * s_buf[j] + w1 * s_buf[RS + j] + w2 * s_buf[2 * RS + j] + w3 * s_buf[3 * RS + j];
              rr_f2* h = (rr_f2*)(s_H + 2 * (madr + p));
              *h += rr_f2{v, v};
            }
          }
        }
        sync();       // the row cells are rewritten by the next contact
      }
    }
  }
  // factor + inverse factor of H in its pair array (both halves hold H), 1/D in dinvH
  __device__ __forceinline__ void newton_factor() {
    const int delta = (int)((D.o_H - D.o_qLD) * sizeof(float));
    int ment[NME];
    load_ment(ment);
    if (lane < 8) s_H[2 * D.nM + lane] = (lane >> 1) == 1 ? 1.0f : 0.0f;     // cells ZERO, ONE, TRASH (+ pad)
    sync();
    run_levels<true, true>(TL.factor3, D.nfac, delta);
    sync();
#pragma unroll
    for (int s = 0; s < NVS; ++s) {
      const int d = lane + RR_LANES * s;
      dinvH[s] = d < D.nv ? 1.0f / s_H[2 * (opaque(dofc1[s]) & 0xFFFF)] : 0.0f;
      if (d < D.nv) *(rr_f2*)(s_buf + 2 * d) = rr_f2{dinvH[s], dinvH[s]};
    }
    sync();
#pragma unroll
    for (int it = 0; it < NME; ++it) {
      const int ij = ment[it];
      if (ij >= 0) {
        const int i = ij & 255, j = ij >> 8;
        if (i != j) *(rr_f2*)(s_H + 2 * (lane + RR_LANES * it)) *= *(const rr_f2*)(s_buf + 2 * i);
      }
    }
    sync();
    run_levels<false, true>(TL.linv, D.ninv, delta);
    sync();
  }

  // [UP mjx solver._update_gradient] in two halves: the exit test of solve() needs grad alone and stands between them
  __device__ __forceinline__ void form_gradient() {
#pragma unroll
    for (int s = 0; s < NVS; ++s) grad[s] = Ma[s] - qfrc_smooth[s] - qfrc_con[s];
  }
  __device__ __forceinline__ void solve_gradient() {
#pragma unroll
    for (int s = 0; s < NVS; ++s) Mgrad[s] = grad[s];
    for (int rep = 0; rep < RR_REP_SOLVE; ++rep) { float t_[NVS]; for (int s = 0; s < NVS; ++s) t_[s] = grad[s]; ldl_solve(t_); }
    if (NEWTON) {            // Mgrad = H^-1 grad
      newton_hessian();
      newton_factor();
      ldl_solve_on(Mgrad, s_H, dinvH);
    } else {
      ldl_solve(Mgrad);
    }
  }

  // search direction from grad / Mgrad: steepest descent on the first pass, Polak-Ribiere after it (pm, gg: Mgrad and grad . Mgrad of the pass before)
  __device__ __forceinline__ void direction(int niter, const float* pm, float gg) {
    if (niter == 0) {
#pragma unroll
      for (int s = 0; s < NVS; ++s) { search[s] = -Mgrad[s]; mv[s] = -grad[s]; }
    } else {
      float bt[2] = {0.0f, gg};
#pragma unroll
      for (int s = 0; s < NVS; ++s) bt[0] += grad[s] * (Mgrad[s] - pm[s]);
      solver_sum_n<2>(bt);
      const float beta = NEWTON ? 0.0f : fmaxf(0.0f, bt[0] / fmaxf(RR_MINVAL, bt[1]));      // Newton: search = -Mgrad
#pragma unroll
      for (int s = 0; s < NVS; ++s) { search[s] = -Mgrad[s] + beta * search[s]; mv[s] = -grad[s] + beta * mv[s]; }
    }
  }

  // [UP mjx solver._Context.create]: Jaref, Ma, constraint state (and gradient/search) at `qacc`
  // `at_smooth`: qacc == qacc_smooth, where Ma = M qacc_smooth = qfrc_smooth by construction (no product needed)
  // `rows_kept`: con_jar / lim_jar already hold the rows at this qacc (solve(), ph 2); `walk`: see update_constraint.  All three wave-uniform.
  __device__ __forceinline__ void ctx_create(bool at_smooth, bool rows_kept, bool walk) {
    if (!rows_kept) {
      put_vec(qacc);
      jac_mul(con_jar, s_vec);
#pragma unroll
      for (int cs = 0; cs < NCS; ++cs)
#pragma unroll
        for (int k = 0; k < 4; ++k) con_jar[cs][k] -= con_aref[cs][k];
#pragma unroll
      for (int s = 0; s < NVS; ++s) lim_jar[s] = lim_sign[s] * qacc[s] - lim_aref[s];
    }
    if (at_smooth) {
#pragma unroll
      for (int s = 0; s < NVS; ++s) Ma[s] = qfrc_smooth[s];
    } else {
#pragma unroll
      for (int s = 0; s < NVS; ++s) Ma[s] = Ma_warm[s];     // M * qacc_warmstart (taken before the factorisations)
    }
    cost = INFINITY; prev_cost = 0.0f;
    update_constraint(walk);
  }

  // line-search point(s): cost and derivatives of the piecewise-quadratic 1-D cost at alpha, over the COMPACTED active
  // rows (see linesearch): row r*64 + lane of the first R rows; padding rows are (0, 0, 0) and never active
  static constexpr int KR = 4 * NCS + NVS;     // row slots per lane if every contact / limit row were active
  // COST = false: derivatives only (the bracketing iterations never look at the cost; the costs of the two final points
  // are evaluated once after the loop, at the same alphas, by the same sums -- identical values, 3 fewer wave sums / point)
  template <int NP, bool COST>
  __device__ __forceinline__ void ls_eval(const float* alpha, const float* qg, LSPoint* out, int R, const float* rjr, const float* rjv,
                                          const float* rD) {
    constexpr int NQ = COST ? 3 : 2;
    float q[NQ * NP];
#pragma unroll
    for (int i = 0; i < NQ * NP; ++i) q[i] = 0.0f;
#pragma unroll
    for (int r = 0; r < KR; ++r) {
      if (r * RR_LANES < R) {
        const float jr = rjr[r], jv = rjv[r], Dv = rD[r];
        const float q0 = 0.5f * jr * jr * Dv, q1 = jv * jr * Dv, q2 = 0.5f * jv * jv * Dv;
#pragma unroll
        for (int i = 0; i < NP; ++i)
          if (jr + alpha[i] * jv < 0) { q[NQ * i] += q1; q[NQ * i + 1] += q2; if (COST) q[NQ * i + 2] += q0; }
      }
    }
    solver_sum_n<NQ * NP>(q);
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const float q1 = qg[1] + q[NQ * i], q2 = qg[2] + q[NQ * i + 1];
      const float a = alpha[i];
      out[i].alpha = a;
      out[i].cost = COST ? a * a * q2 + a * q1 + (qg[0] + q[NQ * i + (COST ? 2 : 0)]) : 0.0f;
      out[i].d0 = 2.0f * a * q2 + q1;
      out[i].d1 = 2.0f * q2 + (q2 == 0.0f ? RR_MINVAL : 0.0f);
    }
  }

  // [UP mjx solver._linesearch].  Only the ACTIVE constraint rows (contacts in penetration x 4 pyramid rows, violated
  // limits) enter the 1-D cost, typically a few dozen of the 4*ncon + nv candidates, scattered over the lanes.  Their
  // (Jaref, Jv, D) triples are compacted once per line search through LDS (positions by ballot / mbcnt; the staging cells
  // are the dead cinert / cvel / pose regions), so that every evaluation of the up to 2 + 3*ls_iterations points costs one
  // row per lane instead of 4*NCS + NVS.
  // RR_LS_STAGE_ONCE: which rows are active (con_act, lim_act) and their D are fixed from constraint_rows() to the end of the substep,
  // so the compacted positions of this lane's rows, the row count R and the D column are formed ONCE, at the head of solve(): a line
  // search then stages and reads back Jaref and Jv alone.  Same positions, same values, same evaluation code (ls_eval).
  int ls_R = 0;                       // wave-uniform
  int ls_cpos[NCS], ls_lpos[NVS];     // first compacted row of this lane's contact slot / its limit row
  float ls_rD[KR];
  __device__ __forceinline__ void ls_stage() {
    int R = 0;
#pragma unroll
    for (int cs = 0; cs < NCS; ++cs) {
      const unsigned long long m = __ballot(con_act[cs]);
      const int pos = R + 4 * (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
      R += 4 * __popcll(m);
      ls_cpos[cs] = pos;
      if (con_act[cs]) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s_buf[pos + k] = (!DYN || k < con_nrow[cs]) ? con_D[cs] : 0.0f;
      }
    }
#pragma unroll
    for (int s = 0; s < NVS; ++s) {
      const unsigned long long m = __ballot(lim_act[s]);
      const int pos = R + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
      R += __popcll(m);
      ls_lpos[s] = pos;
      if (lim_act[s]) s_buf[pos] = lim_D[s];
    }
    ls_R = __builtin_amdgcn_readfirstlane(R);
    sync();
#pragma unroll
    for (int r = 0; r < KR; ++r) {
      ls_rD[r] = 0.0f;
      if (r * RR_LANES < R) {
        const int idx = r * RR_LANES + lane;
        if (idx < R) ls_rD[r] = s_buf[idx];
      }
    }
    sync();     // the pose cells are reused (J * x hand-off)
  }

  template <bool PROF, bool DBG = false>
  __device__ __forceinline__ void linesearch() {
    float red[4] = {0, 0, 0, 0};
    put_vec(search);   // CG: mv = M search is carried by the caller's recurrence; Newton: an explicit product with the copy of M
    if (NEWTON) mul_m_on(mv, s_Mp);
    for (int rep = 0; rep < RR_REP_JAC; ++rep) { float t_[NCS][4]; jac_mul(t_, s_vec); asm volatile("" :: "v"(t_[0][0]), "v"(t_[0][1]), "v"(t_[0][2]), "v"(t_[0][3]) : "memory"); }
    jac_mul(con_jv, s_vec);
    stamp<PROF>(16);
#pragma unroll
    for (int s = 0; s < NVS; ++s) {
      lim_jv[s] = lim_sign[s] * search[s];
      red[0] += search[s] * search[s];
      red[1] += search[s] * Ma[s];
      red[2] += search[s] * qfrc_smooth[s];
      red[3] += search[s] * mv[s];
    }
    int R = 0;
    bool stage_all = !RR_LS_STAGE_ONCE;
    if constexpr (DBG) stage_all |= (dbg_flags & RR_DBG_SOLVER_UNBATCHED) != 0;
    if (!stage_all) {
      float* const st_jr = s_cinert; float* const st_jv = s_cvel;
      // the staged values as values the optimiser has not seen before (in place: no instruction): it would otherwise hoist every mask and
      // address derived from them out of the solver loop and hold them across it
      asm volatile("" : "+s"(ls_R));
#pragma unroll
      for (int cs = 0; cs < NCS; ++cs) asm volatile("" : "+v"(ls_cpos[cs]));
#pragma unroll
      for (int s = 0; s < NVS; ++s) asm volatile("" : "+v"(ls_lpos[s]));
#pragma unroll
      for (int r = 0; r < KR; ++r) asm volatile("" : "+v"(ls_rD[r]));
      R = ls_R;
#pragma unroll
      for (int cs = 0; cs < NCS; ++cs) {
        if (con_act[cs]) {
#pragma unroll
          for (int k = 0; k < 4; ++k) { st_jr[ls_cpos[cs] + k] = con_jar[cs][k]; st_jv[ls_cpos[cs] + k] = con_jv[cs][k]; }
        }
      }
#pragma unroll
      for (int s = 0; s < NVS; ++s)
        if (lim_act[s]) { st_jr[ls_lpos[s]] = lim_jar[s]; st_jv[ls_lpos[s]] = lim_jv[s]; }
    } else {
      float* const st_jr = s_cinert; float* const st_jv = s_cvel; float* const st_D = s_buf;
#pragma unroll
      for (int cs = 0; cs < NCS; ++cs) {
        const unsigned long long m = __ballot(con_act[cs]);
        const int pos = R + 4 * (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        R += 4 * __popcll(m);
        if (con_act[cs]) {
#pragma unroll
          for (int k = 0; k < 4; ++k) { st_jr[pos + k] = con_jar[cs][k]; st_jv[pos + k] = con_jv[cs][k]; st_D[pos + k] = (!DYN || k < con_nrow[cs]) ? con_D[cs] : 0.0f; }
        }
      }
#pragma unroll
      for (int s = 0; s < NVS; ++s) {
        const unsigned long long m = __ballot(lim_act[s]);
        const int pos = R + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        R += __popcll(m);
        if (lim_act[s]) { st_jr[pos] = lim_jar[s]; st_jv[pos] = lim_jv[s]; st_D[pos] = lim_D[s]; }
      }
    }
    sync();
    float rjr[KR], rjv[KR], rD[KR];
#pragma unroll
    for (int r = 0; r < KR; ++r) {
      rjr[r] = rjv[r] = rD[r] = 0.0f;
      if (r * RR_LANES < R) {
        const int idx = r * RR_LANES + lane;
        if (idx < R) { rjr[r] = s_cinert[idx]; rjv[r] = s_cvel[idx]; if (stage_all) rD[r] = s_buf[idx]; }
      }
      if (!stage_all) rD[r] = ls_rD[r];
    }
    solver_sum_n<4>(red);
    const float smag = sqrtf(red[0]) * so_meaninertia * (float)so_nv_scale;
    const float gtol = so_tolerance * so_ls_tolerance * smag;
    const float qg[3] = {gauss, red[1] - red[2], 0.5f * red[3]};
    stamp<PROF>(17);
    LSPoint p0, lo, hi, tmp3[3];
    float a1[1] = {0.0f};
    ls_eval<1, true>(a1, qg, &p0, R, rjr, rjv, rD);
    a1[0] = p0.alpha - div_nr(p0.d0, p0.d1);
    ls_eval<1, false>(a1, qg, &lo, R, rjr, rjv, rD);
    if (lo.d0 < p0.d0) { hi = p0; } else { hi = lo; lo = p0; }
    stamp<PROF>(18);
    bool swap = true;
    work += 4 * (1 + (R > RR_LANES ? 1 : 0));          // the four evaluations outside the bracketing loop
    // REPEAT EXIT (RR_LS_REPEAT_EXIT).  One iteration is a function of (lo, hi) and of values the loop does not change (the compacted rows,
    // qg, gtol), and every iteration runs this one machine-code body (hence nounroll).  An iteration that leaves lo and hi bitwise what they
    // were at its head -- alpha, d0 and d1 of both -- is therefore followed by identical ones: with `swap` false the next loop head ends
    // the loop anyway, with `swap` true nothing changes up to the cap.  In float32 with contracted FMAs that second case is the common
    // one: both ends on one side of the root keep swap_lo_next / swap_hi_next true although the Newton step no longer moves alpha, and gtol
    // lies far below one ulp of d0.  Leaving at once gives the same lo, hi, final costs and alpha.  `work` counts the loop heads the full loop
    // would have visited (after the loop, from `it`: an addition inside the loop costs the single-step instance an SGPR spill).  PAIR: both
    // waves compare the same totals, so they leave in the same iteration and their barriers still match.
    int it = 0, ls_ran = 0, ls_left = 0;               // DBG / PROF: bracketing iterations executed / left out by the exit
#pragma nounroll
    for (; it < so_ls_iterations; ++it) {
#if !RR_LS_REPEAT_EXIT
      work += 3 * (1 + (R > RR_LANES ? 1 : 0));        // the bracketing loop is what separates slow from fast environments
#endif
      bool done = !swap;
      done |= (lo.d0 < 0) && (lo.d0 > -gtol);
      done |= (hi.d0 > 0) && (hi.d0 < gtol);
      if (uni(done)) break;
      if constexpr (PROF || DBG) ++ls_ran;
#if RR_LS_REPEAT_EXIT
      const LSPoint lo_head = lo, hi_head = hi;
#endif
      const float a3[3] = {lo.alpha - div_nr(lo.d0, lo.d1), hi.alpha - div_nr(hi.d0, hi.d1), 0.5f * (lo.alpha + hi.alpha)};
      ls_eval<3, false>(a3, qg, tmp3, R, rjr, rjv, rD);
      const LSPoint lo_next = tmp3[0], hi_next = tmp3[1], mid = tmp3[2];
      const bool swap_lo_next = (lo.d0 > 0) || (lo.d0 < lo_next.d0);
      if (swap_lo_next) lo = lo_next;
      const bool swap_lo_mid = (mid.d0 < 0) && (lo.d0 < mid.d0);
      if (swap_lo_mid) lo = mid;
      const bool swap_hi_next = (hi.d0 < 0) || (hi.d0 > hi_next.d0);
      if (swap_hi_next) hi = hi_next;
      const bool swap_hi_mid = (mid.d0 > 0) && (hi.d0 > mid.d0);
      if (swap_hi_mid) hi = mid;
      swap = swap_lo_next || swap_lo_mid || swap_hi_next || swap_hi_mid;
#if RR_LS_REPEAT_EXIT
      bool same = swap;        // without a swap the next loop head leaves (and counts itself in `work`)
      same &= __float_as_int(lo.alpha) == __float_as_int(lo_head.alpha) && __float_as_int(lo.d0) == __float_as_int(lo_head.d0) && __float_as_int(lo.d1) == __float_as_int(lo_head.d1);
      same &= __float_as_int(hi.alpha) == __float_as_int(hi_head.alpha) && __float_as_int(hi.d0) == __float_as_int(hi_head.d0) && __float_as_int(hi.d1) == __float_as_int(hi_head.d1);
      if constexpr (DBG) same &= (dbg_flags & RR_DBG_LS_RUN_REPEATS) == 0;      // debug-dump instance: run the repeats anyway (rr_batch_set_ls_repeat_exit)
      if (uni(same)) {
        if constexpr (PROF || DBG) ls_left = so_ls_iterations - 1 - it;
        it = so_ls_iterations;
        break;
      }
#endif
    }
#if RR_LS_REPEAT_EXIT
    work += 3 * (1 + (R > RR_LANES ? 1 : 0)) * (it < so_ls_iterations ? it + 1 : it);      // the bracketing loop is what separates slow from fast environments
#endif
    if constexpr (PROF) { pt[20] += (unsigned)ls_ran; pt[21] += (unsigned)ls_left; }
    if constexpr (DBG) { dbg_ls_ran += ls_ran; dbg_ls_left += ls_left; }
    {   // costs of the bracket's end points
      const float a2[2] = {lo.alpha, hi.alpha};
      LSPoint f2[2];
      ls_eval<2, true>(a2, qg, f2, R, rjr, rjv, rD);
      lo.cost = f2[0].cost; hi.cost = f2[1].cost;
    }
    stamp<PROF>(19);
    const bool improved = uni((lo.cost < p0.cost) || (hi.cost < p0.cost));
    const float alpha = lo.cost < hi.cost ? lo.alpha : hi.alpha;
    if (improved) {
#pragma unroll
      for (int s = 0; s < NVS; ++s) { qacc[s] += search[s] * alpha; Ma[s] += mv[s] * alpha; lim_jar[s] += lim_jv[s] * alpha; }
#pragma unroll
      for (int cs = 0; cs < NCS; ++cs)
#pragma unroll
        for (int k = 0; k < 4; ++k) con_jar[cs][k] += con_jv[cs][k] * alpha;
    }
  }

  // [UP mjx solver.solve] primal CG with warm start; returns the iteration count
  template <bool PROF, bool DBG = false>
  __device__ __forceinline__ int solve() {
    {
      const DT Dl = phase_dims();
      so_tolerance = Dl.tolerance; so_ls_tolerance = Dl.ls_tolerance; so_meaninertia = Dl.meaninertia;
      so_iterations = Dl.iterations; so_ls_iterations = Dl.ls_iterations; so_nv_scale = Dl.nv_scale;
    }
    const float scale = 1.0f / (so_meaninertia * (float)so_nv_scale);
    // warm start [UP mjx solver.solve]: cost at qacc_smooth, cost at qacc_warmstart, then the full context at the cheaper
    // of the two.  One copy of the evaluation code, driven by a wave-uniform phase counter, so the two costs that are compared come from
    // the same instructions.  Of ph 0 only the cost is ever read: its qfrc_con is overwritten by ph 1 or formed again by ph 2.  So ph 0
    // skips the contact walk (update_constraint(false): same force and cost arithmetic, empty ballot), and its rows Jaref are kept in
    // registers for ph 2, which would compute the same J * qacc_smooth - aref by the same code: ph 2 restores them and walks.
    const bool untrimmed = DBG && (dbg_flags & RR_DBG_SOLVER_UNTRIMMED) != 0;      // debug-dump instance: walk in ph 0, rebuild in ph 2, solve before the exit test
    const bool unbatched = DBG && (dbg_flags & RR_DBG_SOLVER_UNBATCHED) != 0;      // debug-dump instance: the line search stages positions and D in every call
    if (RR_LS_STAGE_ONCE && !unbatched) ls_stage();
    float cost_smooth = 0.0f;
    bool use_smooth = false;
    float jar0[NCS][4], ljar0[NVS];
#pragma unroll
    for (int cs = 0; cs < NCS; ++cs)
#pragma unroll
      for (int k = 0; k < 4; ++k) jar0[cs][k] = 0.0f;
#pragma unroll
    for (int s = 0; s < NVS; ++s) ljar0[s] = 0.0f;
#pragma nounroll
    for (int ph = 0; ph < 3; ++ph) {
      if (ph == 2 && !use_smooth) break;        // the context already is the one at qacc_warmstart
#pragma unroll
      for (int s = 0; s < NVS; ++s) qacc[s] = ph != 1 ? qacc_smooth[s] : (lane + RR_LANES * s < D.nv ? s_warm[lane + RR_LANES * s] : 0.0f);
      const bool rows_kept = ph == 2 && !untrimmed;
      if (rows_kept) {
#pragma unroll
        for (int cs = 0; cs < NCS; ++cs)
#pragma unroll
          for (int k = 0; k < 4; ++k) con_jar[cs][k] = jar0[cs][k];
#pragma unroll
        for (int s = 0; s < NVS; ++s) lim_jar[s] = ljar0[s];
      }
      ctx_create(ph != 1, rows_kept, ph != 0 || untrimmed);
      if (ph == 0) {
        cost_smooth = cost;
#pragma unroll
        for (int cs = 0; cs < NCS; ++cs)
#pragma unroll
          for (int k = 0; k < 4; ++k) jar0[cs][k] = con_jar[cs][k];
#pragma unroll
        for (int s = 0; s < NVS; ++s) ljar0[s] = lim_jar[s];
      }
      if (ph == 1) use_smooth = uni(!(cost < cost_smooth));
    }
    if constexpr (DBG) dbg_solver_end = use_smooth ? 1 : 0;
    // THE EXIT TEST STANDS BEFORE THE SOLVE.  The loop below is the reference's  linesearch -> update_constraint -> update_gradient ->
    // direction -> ++niter -> test  rotated by half a turn: the test reads niter, prev_cost and cost (final after update_constraint) and
    // |grad|, never Mgrad.  So on the pass that ends the loop -- every forward pass has one -- the solve Mgrad = M^-1 grad (Newton: Hessian,
    // factorisation and solve), the beta sums and the new search / mv would be computed and never read: after the loop only niter, cost,
    // qacc, qfrc_con and s_warm are.  Here grad is formed, niter counted and the test made first; the solve and the direction follow only
    // when another line search does.  One copy of the test, of the solve and of the direction serves the first pass (niter == 0: search =
    // -Mgrad, mv = -grad) and the later ones.  gg and pm are taken from grad / Mgrad before update_constraint, as ever.  PAIR: both waves
    // test identical totals, so they leave together and their barriers still match.
    form_gradient();
    int niter = 0;
    float pm[NVS], gg = 0.0f;
#pragma unroll
    for (int s = 0; s < NVS; ++s) pm[s] = 0.0f;
    while (true) {
      if (untrimmed) { solve_gradient(); direction(niter, pm, gg); }      // debug-dump instance, switch off: the reference's order
      const float improvement = (prev_cost - cost) * scale;
      float g2 = 0.0f;
#pragma unroll
      for (int s = 0; s < NVS; ++s) g2 += grad[s] * grad[s];
      const float gradient = sqrtf(solver_sum(g2)) * scale;
      bool done = niter >= so_iterations;
      done |= improvement < so_tolerance;
      done |= gradient < so_tolerance;
      if (uni(done)) {
        if constexpr (DBG) dbg_solver_end |= (niter >= so_iterations ? 2 : 0) | (uni(improvement < so_tolerance) ? 4 : 0) | (uni(gradient < so_tolerance) ? 8 : 0);
        break;
      }
      if constexpr (PROF) { if (niter) stamp<PROF>(12); }       // cg_misc: grad, the test (and the direction below)
      if (!untrimmed) {
        solve_gradient();
        if constexpr (PROF) { if (niter) stamp<PROF>(11); }     // update_gradient: the solve; the first one belongs to solver_init
        // search = -Mgrad, and mv = M search = -grad because Mgrad = M^-1 grad: the product the reference recomputes every
        // iteration [UP mjx solver._linesearch: mv = M @ search] follows the search-direction recurrence exactly
        direction(niter, pm, gg);
      }
      if constexpr (PROF) { if (niter) stamp<PROF>(12); else stamp<PROF>(8); }
      for (int rep = 0; rep < RR_REP_LS; ++rep) linesearch<false>();
      linesearch<PROF, DBG>();
      stamp<PROF>(9);
      gg = 0.0f;
#pragma unroll
      for (int s = 0; s < NVS; ++s) { gg += grad[s] * Mgrad[s]; pm[s] = Mgrad[s]; }
      for (int rep = 0; rep < RR_REP_UC; ++rep) { const float pc = prev_cost, c0 = cost; update_constraint(); prev_cost = pc; cost = c0; }
      update_constraint();
      stamp<PROF>(10);
      form_gradient();
      ++niter;
    }
#pragma unroll
    for (int s = 0; s < NVS; ++s) { const int d = lane + RR_LANES * s; if (d < D.nv) s_warm[d] = qacc[s]; }
    return niter;
  }

  // ---------------------------------------------------------------- A-8 euler (+eulerdamp) and position integration
  __device__ __forceinline__ void euler() {
    float qa[NVS];
#pragma unroll
    for (int s = 0; s < NVS; ++s) qa[s] = qfrc_smooth[s] + qfrc_con[s];
    ldl_solve<true>(qa);
    const RRTables T = tables();
    const DT D = phase_dims();   // the run-time scalars this phase reads (dt, gravity, schedule lengths): local to it, like T
#pragma unroll
    for (int s = 0; s < NVS; ++s) {
      const int d = lane + RR_LANES * s;
      if (d < D.nv) {
        const int u = DYN ? -1 : row_at(T.dof_i, RR_DOFI, d)[7];      // DYN: an actuator may drive several dofs -- integrated per actuator below
        if (u >= 0) {   // filter activation dynamics: act_dot = (clamp(ctrl) - act) / tau
          auto af = row_at(T.act_f, 8, u);
          const float c = fminf(fmaxf(s_ctrl[u], af[5]), af[6]);
          s_act[u] += D.dt * ((c - s_act[u]) / fmaxf(af[4], RR_MINVAL));
        }
        s_qvel[d] += D.dt * qa[s];
      }
    }
    if (DYN && lane < D.nu) {
      auto af = row_at(T.act_f, 8, lane);
      const float c = fminf(fmaxf(s_ctrl[lane], af[5]), af[6]);
      s_act[lane] += D.dt * ((c - s_act[lane]) / fmaxf(af[4], RR_MINVAL));
    }
    sync();
#pragma unroll
    for (int s = 0; s < NVS; ++s) {
      const int d = lane + RR_LANES * s;
      if (d < D.nv) {
        const int kind = row_at(T.dof_i, RR_DOFI, d)[2], qadr = row_at(T.dof_i, RR_DOFI, d)[6];
        if (kind == 6 || kind < 3) {
          s_qpos[qadr] += D.dt * s_qvel[d];
        } else if (kind == 3) {  // quaternion of the free joint: q <- normalize(q * exp(dt*w/2)), w in the body frame
          const v3 w = ld3(s_qvel + d);
          const float n = sqrtf(dot(w, w));
          v3 ax = mk3(0, 0, 0);
          if (n > RR_MINVAL) ax = w * (1.0f / n);
          const float ang = D.dt * n;
          float sn, cs;
          sincosf(ang * 0.5f, &sn, &cs);
          float qr[4] = {cs, ax.x * sn, ax.y * sn, ax.z * sn}, q0[4], qn[4];
          for (int k = 0; k < 4; ++k) q0[k] = s_qpos[qadr + k];
          quat_mul(qn, q0, qr);
          quat_normalize(qn);
          for (int k = 0; k < 4; ++k) s_qpos[qadr + k] = qn[k];
        }
      }
    }
    sync();
  }
};

// ------------------------------------------------------------------------------------------ kernel
// The kernel's explicit arguments as they lie in the kernarg segment.  The ~20 pointers of RRIO are needed only before the
// first and after the last substep; read through the (opaque) kernarg pointer where they are used, they do not occupy
// scalar registers -- or their spill lanes -- during the substeps.
// ASSUMPTION (AMDGPU kernel ABI): explicit by-value arguments are laid out in the kernarg segment in declaration order,
// each at its natural alignment -- i.e. like the members of this struct.  Guards: the static_asserts below pin the struct's
// own layout rules; tests/test_abi_and_oracle.py compares rr_kernarg_layout() with the argument offsets the device compiler
// recorded in the code object (tools/kernel_meta.py); and the debug-dump instance compares the block it re-reads with the
// real `io_kernarg` parameter on every launch (dump field `kernarg_ok`).
struct RRKArgs { RRDims D; RRTables T; RRIO io; int num_envs, n_frames; };
constexpr size_t rr_align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
static_assert(alignof(RRDims) == 4 && alignof(RRTables) == 8 && alignof(RRIO) == 8, "argument alignments the kernarg layout relies on");
static_assert(offsetof(RRKArgs, T) == rr_align_up(sizeof(RRDims), alignof(RRTables)), "RRTables follows RRDims at its natural alignment");
static_assert(offsetof(RRKArgs, io) == rr_align_up(offsetof(RRKArgs, T) + sizeof(RRTables), alignof(RRIO)), "RRIO follows RRTables at its natural alignment");
static_assert(offsetof(RRKArgs, num_envs) == offsetof(RRKArgs, io) + sizeof(RRIO) && sizeof(RRIO) % 8 == 0, "scalars follow RRIO without padding");
static_assert(offsetof(RRIO, clip) % 8 == 0 && offsetof(RRIO, clip) + sizeof(const int*) == offsetof(RRIO, track_pose), "the pose members follow the clip ids without padding");
static_assert(offsetof(RRIO, pose_joint_k) + sizeof(float) == offsetof(RRIO, ref_frames), "the reference-observation members follow the pose members without padding");
static_assert(offsetof(RRIO, ref_pad) + sizeof(int) == offsetof(RRIO, pose_fail) && offsetof(RRIO, pose_fail) % 8 == 0, "the pose-termination members follow the reference-observation members without padding");
static_assert(offsetof(RRIO, pose_fail) + sizeof(float*) == offsetof(RRIO, pose_max_pos), "the thresholds follow pose_fail without padding");
static_assert(offsetof(RRIO, pterm_pad) + sizeof(int) == offsetof(RRIO, track_bodies) && offsetof(RRIO, track_bodies) % 8 == 0, "the body-tracking members follow the pose-termination members without padding");
static_assert(offsetof(RRIO, track_bodies) + 3 * sizeof(float*) == offsetof(RRIO, body_w), "the weights and scales follow the three body-tracking pointers without padding");
static_assert(offsetof(RRIO, endeff_k) + sizeof(float) == offsetof(RRIO, restart_frames) && offsetof(RRIO, restart_frames) % 8 == 0, "the clip-restart members follow the body-tracking members without padding");
static_assert(offsetof(RRIO, restart_frames) + 3 * sizeof(int*) == offsetof(RRIO, restart_K), "the slot count follows the three clip-restart pointers without padding");
static_assert(offsetof(RRIO, restart_end) + sizeof(int) == offsetof(RRIO, track_vel) && offsetof(RRIO, track_vel) % 8 == 0, "the velocity-tracking members follow the clip-restart members without padding");
static_assert(offsetof(RRIO, track_vel) + 2 * sizeof(float*) == offsetof(RRIO, vel_lin_w), "the weights and scales follow the two velocity-tracking pointers without padding");
static_assert(offsetof(RRIO, vel_joint_k) + sizeof(float) == offsetof(RRIO, clip_len) && offsetof(RRIO, clip_len) % 8 == 0, "the clip-library members follow the velocity-tracking members without padding");
static_assert(offsetof(RRIO, clip_len) + 3 * sizeof(int*) == offsetof(RRIO, clip_weights), "the clip-sampling members follow the three clip-library pointers without padding");
static_assert(offsetof(RRIO, clip_weights) + 4 * sizeof(int*) == offsetof(RRIO, sample_seed), "the seed follows the four clip-sampling pointers without padding");
static_assert(offsetof(RRIO, sample_seed) + sizeof(unsigned) == offsetof(RRIO, rref_seed), "the reference-restart members follow the seed without padding (rref_seed takes the word that was tail padding)");
static_assert(offsetof(RRIO, rref_pad) + sizeof(int) == sizeof(RRIO) && offsetof(RRIO, rref_seed) + 7 * sizeof(int) == sizeof(RRIO), "the reference-restart members close RRIO without padding");
// ... and so are the model tables outside the solver's loops: RRTables is re-read at the head of each phase that indexes a table
// (narrow scalar loads next to an existing hand-off; the unused members' loads are dead), so no table pointer is held across the
// substep.  The loops' own tables are the exception (RRLoopTables, taken once from the parameter).
static __device__ __forceinline__ RRTables load_tables() {
#if defined(__HIP_DEVICE_COMPILE__)
  const char __attribute__((address_space(4)))* p = (const char __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return *(const RRTables __attribute__((address_space(4)))*)(p + offsetof(RRKArgs, T));
#else
  return RRTables{};
#endif
}
static __device__ __forceinline__ RRDims load_dims() {
#if defined(__HIP_DEVICE_COMPILE__)
  const char __attribute__((address_space(4)))* p = (const char __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return *(const RRDims __attribute__((address_space(4)))*)(p + offsetof(RRKArgs, D));
#else
  return RRDims{};
#endif
}
static __device__ __forceinline__ RRIO load_io() {
#if defined(__HIP_DEVICE_COMPILE__)
  const char __attribute__((address_space(4)))* p = (const char __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return *(const RRIO __attribute__((address_space(4)))*)(p + offsetof(RRKArgs, io));
#else
  return RRIO{};
#endif
}

// One member of the I/O block, read where it is used (a narrow scalar load with a short live range; `load_io` fetches the whole block)
template <class T>
static __device__ __forceinline__ T load_io_member(size_t member_offset) {
#if defined(__HIP_DEVICE_COMPILE__)
  const char __attribute__((address_space(4)))* p = (const char __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return *(const T __attribute__((address_space(4)))*)(p + offsetof(RRKArgs, io) + member_offset);
#else
  return T{};
#endif
}

// Width of an observation row = the stride of obs, t_obs, a_obs_in and first_obs.  REFOBS instances (rr_poseterm_kernel, rr_body_kernel, rr_restart_kernel): the model's obs_dim
// plus RRIO::ref_frames blocks of nq entries, the count read where the width is used; every other instance: D.obs_dim itself.
template <bool REFOBS, class DT>
static __device__ __forceinline__ int rr_obs_width(const DT& D) {
  if constexpr (REFOBS) return D.obs_dim + load_io_member<int>(offsetof(RRIO, ref_frames)) * D.nq;
  else return D.obs_dim;
}

// Frames of clip `c` (already clamped into 0 .. num_clips - 1) = the exclusive upper bound of every frame clamp of an env on it.  BODY
// instances (RRIO, CLIP LIBRARY): clip_len[c] clamped into 1 .. track_len, so no frame addresses outside a clip's rows; a null clip_len,
// and every other instance: track_len itself, the expression those instances had before.  `c` is wave-uniform: a scalar load, read where
// it is used.
template <bool BODY>
static __device__ __forceinline__ int rr_clip_frames(int c, int track_len) {
  if constexpr (BODY) {
    const int* cl = load_io_member<const int*>(offsetof(RRIO, clip_len));
    if (!cl) return track_len;
    const int n = __builtin_amdgcn_readfirstlane(cl[c]);
    return n < 1 ? 1 : (n > track_len ? track_len : n);
  } else {
    return track_len;
  }
}

// MurmurHash3's 32-bit finaliser, the hash of the weighted restore (RRIO, CLIP SAMPLING)
static __device__ __host__ __forceinline__ unsigned rr_fmix32(unsigned h) {
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  return h;
}

// The slot a weighted restore of `env` draws (RRIO, CLIP SAMPLING), or -1 where every entry of the env's bank has weight 0.  Called by
// the whole wave with wave-uniform arguments; K <= 64 = one lane per entry.  Lanes >= K carry the total, so the ballot's lowest set bit
// is a slot of the bank whenever S > r, which r's definition guarantees.
static __device__ __forceinline__ int rr_weighted_slot(const int* cw, const int* bcl, int K, int nc, int env, int num_envs, unsigned seed, unsigned n, int lane) {
  unsigned p = 0;
  if (lane < K) {
    int c = bcl[(size_t)lane * (size_t)num_envs + (size_t)env];
    c = c < 0 ? 0 : (c > nc - 1 ? nc - 1 : c);
    p = (unsigned)cw[c] & 0xFFFFu;      // entries are 0 .. 65535 by contract: the mask keeps S within 32 bits whatever the table holds
  }
#pragma unroll
  for (int d = 1; d < RR_LANES; d <<= 1) { const unsigned t = __shfl_up(p, d, RR_LANES); if (lane >= d) p += t; }
  const unsigned S = (unsigned)__builtin_amdgcn_readlane((int)p, RR_LANES - 1);
  if (S == 0) return -1;
  const unsigned h = rr_fmix32(rr_fmix32(seed ^ ((unsigned)env * 0x9E3779B1u)) + n);
  const unsigned r = (unsigned)(((unsigned long long)h * (unsigned long long)S) >> 32);
  const unsigned long long m = __ballot(p > r);
  const int k = (int)__builtin_ctzll(m | (1ull << (K - 1)));      // (the guard bit is never the lowest: slot K - 1 has prefix S > r)
  return __builtin_amdgcn_readfirstlane(k);
}

// The hashes of a reference restart (RRIO, REFERENCE RESTARTS): `base` per (seed, env, restore count), one hash per purpose p and element i
static __device__ __host__ __forceinline__ unsigned rr_ref_base(unsigned seed, int env, unsigned n) { return rr_fmix32(rr_fmix32(seed ^ ((unsigned)env * 0x9E3779B1u)) + n); }
static __device__ __host__ __forceinline__ unsigned rr_ref_hash(unsigned base, unsigned p, unsigned i) { return rr_fmix32(base ^ (((p << 16) | i) * 0x9E3779B1u)); }
// s(h) = (h >> 8) * 2^-23 - 1 in [-1, 1): both operations exact in float32
static __device__ __host__ __forceinline__ float rr_ref_unit(unsigned h) { return (float)(h >> 8) * 0x1p-23f - 1.0f; }

// The clip a reference restart draws over all `nc` clips with the hash `h` (RRIO, REFERENCE RESTARTS).  Called by the whole wave with
// wave-uniform arguments.  With a weight table `cw` of sum S > 0: the smallest c with q_0 + .. + q_c > r = (h * S) >> 32, found chunk of
// 64 clips by chunk -- lane l holds q_(c0 + l), an inclusive wave scan on top of the chunks before, a ballot of prefix > r.  r < S, so
// some chunk has a set bit; a clip of weight 0 repeats its predecessor's prefix and is never the lowest one.  Otherwise uniform.
// The host keeps nc <= 65536, so S stays within 32 bits.
static __device__ __forceinline__ int rr_ref_clip(const int* cw, int nc, unsigned h, int lane) {
  if (cw) {
    unsigned S = 0;
    for (int c0 = 0; c0 < nc; c0 += RR_LANES) {
      unsigned p = c0 + lane < nc ? ((unsigned)cw[c0 + lane] & 0xFFFFu) : 0u;
#pragma unroll
      for (int d = 1; d < RR_LANES; d <<= 1) { const unsigned t = __shfl_up(p, d, RR_LANES); if (lane >= d) p += t; }
      S += (unsigned)__builtin_amdgcn_readlane((int)p, RR_LANES - 1);
    }
    if (S != 0) {
      const unsigned r = (unsigned)(((unsigned long long)h * (unsigned long long)S) >> 32);
      unsigned before = 0;
      for (int c0 = 0; c0 < nc; c0 += RR_LANES) {
        unsigned p = c0 + lane < nc ? ((unsigned)cw[c0 + lane] & 0xFFFFu) : 0u;
#pragma unroll
        for (int d = 1; d < RR_LANES; d <<= 1) { const unsigned t = __shfl_up(p, d, RR_LANES); if (lane >= d) p += t; }
        const unsigned long long m = __ballot(before + p > r);
        if (m != 0) {
          const int c = c0 + (int)__builtin_ctzll(m);
          return __builtin_amdgcn_readfirstlane(c > nc - 1 ? nc - 1 : c);
        }
        before += (unsigned)__builtin_amdgcn_readlane((int)p, RR_LANES - 1);
      }
      return nc - 1;      // not reached (r < S)
    }
  }
  return (int)(((unsigned long long)h * (unsigned long long)(unsigned)nc) >> 32);
}

// RAND instances: the tables with the three randomisable ones advanced to environment `env`'s rows.  `env` is wave-uniform, the
// pointers come from the argument block, so the address arithmetic is scalar (a 64-bit multiply-add per table).
static __device__ __forceinline__ RRTables load_env_tables(int env, int nv, int nu, int ncon) {
  RRTables T = load_tables();
#if defined(__HIP_DEVICE_COMPILE__)
  const char __attribute__((address_space(4)))* p = (const char __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  typedef const char* const __attribute__((address_space(4)))* slot_t;
  const char* const df = *(slot_t)(p + offsetof(RRKArgs, io) + offsetof(RRIO, env_dof_f));
  const char* const af = *(slot_t)(p + offsetof(RRKArgs, io) + offsetof(RRIO, env_act_f));
  const char* const cf = *(slot_t)(p + offsetof(RRKArgs, io) + offsetof(RRIO, env_con_f));
  const size_t e = (size_t)(unsigned)env;
  if (df) T.dof_f = (rr_gf)(df + e * ((size_t)nv * 16 * sizeof(float)));
  if (af) T.act_f = (rr_gf)(af + e * ((size_t)nu * 8 * sizeof(float)));
  if (cf) T.con_f = (rr_gf)(cf + e * ((size_t)ncon * 26 * sizeof(float)));
#endif
  return T;
}

// The actor of a multi-step rollout, one wave = one env: policy MLP (obs -> 32 x a_nh -> 2A, SiLU) on the observation of step `ut`,
// tanh-normal sample with the given noise, action into a_actions (where the step reads its ctrl), raw action and log-prob into the
// trajectory buffers.  Head: lane = logit.  A <= 32: one pass over the 64 padded columns, lane a fetches its scale logit from lane A + a.
// 32 < A <= 64 (rodent_cpu.xml: 38 actuators, 76 logits): two passes over 128 padded columns, location logit a and scale logit A + a both
// formed by lane a.  The choice is wave-uniform (A is a model dimension).  First layer: lane l holds the normalised observation entries l, l+64, ..; for each of the 32 units the 64
// partial dot products are summed over the wave (four units per DPP reduction).  Later layers: lane n = unit n, the activation
// vector handed around by shuffles, weights transposed so that the lanes read consecutive floats.
// trajectory addressing: step s of the launch is step t = s % L of segment u = s / L; rows [u][env][t]
struct RRTraj { int u, t; };
static __device__ __forceinline__ RRTraj rr_traj(const RRIO& io, int s) { RRTraj r; r.u = s / io.a_seg; r.t = s - r.u * io.a_seg; return r; }
static __device__ __forceinline__ size_t rr_traj_obs(const RRIO& io, int N, int env, int u, int t) { return ((size_t)u * N + env) * (io.a_seg + 1) + t; }   // row index
static __device__ __forceinline__ size_t rr_traj_at(const RRIO& io, int N, int env, int s) { const RRTraj r = rr_traj(io, s); return ((size_t)r.u * N + env) * io.a_seg + r.t; }
// EVAL (rr_eval_kernel): the observation comes from the env's two-row ring, a null noise pointer is the deterministic policy (raw = loc,
// formed as loc + scale * 0 so that it equals the sampled form under all-zero noise bit for bit), and nothing but the action is recorded.
// JM: observation entries per lane, so the row is at most 64 JM wide (host check, actor_limit): RR_ACTOR_JM = 20 (1280) everywhere but in
// the REFOBS instances, whose row is rr_obs_width wide and which read RR_ACTOR_JM_REFOBS = 26 per lane (1664: up to five reference
// frames on the shipped floor-contact models, 1279 + 5 x 74 = 1649 and 1263 + 5 x 74 = 1633).
#define RR_ACTOR_JM 20
#define RR_ACTOR_JM_REFOBS 26
template <bool EVAL = false, int JM = RR_ACTOR_JM, bool REFOBS = false, class DT>
__device__ __forceinline__ void rr_actor_step(const RRIO& io, const DT& D, int lane, int env, int ut, int num_envs) {
  const int K = rr_obs_width<REFOBS>(D), A = D.nu;
  const float* ob;
  if constexpr (EVAL) ob = io.t_obs + ((size_t)env * 2 + (ut & 1)) * K;
  else { const RRTraj tr = rr_traj(io, ut); ob = io.t_obs + rr_traj_obs(io, num_envs, env, tr.u, tr.t) * K; }
  float x[JM];
#pragma unroll
  for (int j = 0; j < JM; ++j) {
    const int k = lane + RR_LANES * j, kc = k < K ? k : K - 1;
    float v = ob[kc];
    if (io.a_mean) v = (v - io.a_mean[kc]) / io.a_std[kc];
    x[j] = k < K ? v : 0.0f;
  }
  // all 32 units at once: every observation entry meets 32 independent loads (one per unit, 256 contiguous bytes each across the
  // wave), so the memory system always has a full batch in flight; the 32 wave sums follow, four per DPP reduction
  float p[32];
#pragma unroll
  for (int n = 0; n < 32; ++n) p[n] = 0.0f;
#pragma unroll 2
  for (int j = 0; j < JM; ++j) {
    const int k = lane + RR_LANES * j, kc = k < K ? k : K - 1;
    const float xj = x[j];
#pragma unroll
    for (int n = 0; n < 32; ++n) p[n] = fmaf(xj, io.a_W0[(size_t)n * K + kc], p[n]);
  }
  float z1 = 0.0f;
#pragma unroll
  for (int n0 = 0; n0 < 32; n0 += 4) {
    wave_sum_n<4>(p + n0);
#pragma unroll
    for (int u = 0; u < 4; ++u) z1 = lane == n0 + u ? p[n0 + u] : z1;
  }
  const int l32 = lane & 31;
  float h = z1 + io.a_b0[l32];
  h = h / (1.0f + expf(-h));
#pragma unroll
  for (int l = 1; l < 5; ++l) {             // constant indices into the kernel-argument arrays (they live in scalar registers)
    if (l < io.a_nh) {
      const float* wt = io.a_Wt[l - 1];
      float acc = io.a_b[l - 1][l32];
#pragma unroll
      for (int k = 0; k < 32; ++k) acc = fmaf(__shfl(h, k, RR_LANES), wt[k * 32 + l32], acc);
      h = acc / (1.0f + expf(-acc));
    }
  }
  float o, s_raw;
  if (A <= 32) {
    o = io.a_bh[lane];
#pragma unroll
    for (int k = 0; k < 32; ++k) o = fmaf(__shfl(h, k, RR_LANES), io.a_Wth[k * 64 + lane], o);
    s_raw = __shfl(o, (A + lane) & 63, RR_LANES);      // lane a: logits[A + a]
  } else {             // host check: A <= 64, so column A + lane <= 127 lies inside the 128 padded columns for every lane
    o = io.a_bh[lane];
    s_raw = io.a_bh[A + lane];
#pragma unroll
    for (int k = 0; k < 32; ++k) {
      const float hk = __shfl(h, k, RR_LANES);
      o = fmaf(hk, io.a_Wth[k * 128 + lane], o);
      s_raw = fmaf(hk, io.a_Wth[k * 128 + A + lane], s_raw);
    }
  }
  if constexpr (EVAL) {
    if (lane < A) {
      const float scale = rr_tn_scale(s_raw, io.a_min_std);
      const float nz = io.a_noise ? io.a_noise[((size_t)ut * num_envs + env) * A + lane] : 0.0f;
      const float raw = rr_tn_raw(o, scale, nz);
      io.a_actions[((size_t)((io.a_pad & RR_EVAL_ACTIONS) ? ut : 0) * num_envs + env) * A + lane] = tanhf(raw);
    }
    return;
  }
  float lp = 0.0f;
  if (lane < A) {
    const float scale = rr_tn_scale(s_raw, io.a_min_std);
    const float raw = rr_tn_raw(o, scale, io.a_noise[((size_t)ut * num_envs + env) * A + lane]);
    lp = rr_tn_logp(o, scale, raw);
    io.a_actions[((size_t)ut * num_envs + env) * A + lane] = tanhf(raw);
    io.t_raw[rr_traj_at(io, num_envs, env, ut) * A + lane] = raw;
  }
  lp = wave_sum(lp);
  if (lane == 0) io.t_logp[rr_traj_at(io, num_envs, env, ut)] = lp;
}

// UNROLL: io.unroll_T env steps per launch.  The environments of a launch never wait for each other between steps (a synchronised
// step lasts as long as its slowest environment; over ten unsynchronised steps the slowest SUM is 6.5 % below ten slowest steps,
// tools/tail_probe.py), the state stays in LDS from step to step, and the Episode + AutoReset wrappers
// (brax.envs.wrappers.training; rr_wrap_episode_autoreset is their one-launch form) are applied in place.
// PAIR (see Wave): 128 threads = one wavefront per replica of a two-tree model; Dk / T describe ONE replica (nv_scale = the model's
// dof count), the state arrays are the model's ([N][2 nq] ...: replica r of environment e is row 2 e + r of an [2 N][nq] array).
// Physics only (pipeline_init / pipeline_step: no env epilogue, no optional outputs, no debug dump).
// RAND (rr_rand_kernel below): the environments of the launch carry their own parameter rows (RRIO::env_dof_f / env_act_f / env_con_f).
// The arithmetic is the same; only the base of three tables depends on the environment (Wave::tables).
// The body is shared between the two entries as TEXT (rr_step_body.inc).  As a __device__ __forceinline__ function template it is optimised
// once on its own and a second time after it has been inlined into the entry, and that moved the register allocation of every existing
// instance (SGPR spills 67 / 83 / 158 -> 63 / 77 / 147 in the fixed-dimension ones, 68 bytes of scratch in the (2,2,1) debug and the (3,3,2)
// production instance; profiles/r05_a_kernel_meta_function_form.txt).  Included as text, rr_step_kernel compiles the token stream it always
// had, and its instances keep their code (profiles/r05_a_kernel_meta_parent.txt against r05_a_kernel_meta_rand.txt).
template <int NBS, int NVS, int NCS, bool PROF, bool DBG, class DT, bool NEWTON = false, bool UNROLL = false, bool ACTOR = false, bool PAIR = false, bool DYN = false>
__global__ __launch_bounds__((PAIR ? 2 : 1) * RR_LANES, (NVS >= 3 ? 1 : 2)) void rr_step_kernel(const RRDims Dk, const RRTables Tk, const RRIO io_kernarg, const int num_envs,
                                                           const int n_frames) {
  constexpr bool RAND = false, EVAL = false, POSE = false, REFOBS = false, PTERM = false, BODY = false, RESTART = false;
  constexpr bool ROOTSLOT = rr_root_slot<DT>::value && NBS == 2 && !NEWTON && !PAIR && !DYN;      // the root body alone in the second body slot (Wave::ROOT)
  constexpr int MRES = ACTOR ? 1 : 2;      // resident inverse-factor entries (Wave::MAT_RES): both sides at 245-253 registers (timed: -1.4 % against the column side alone); with the actor the column side (233)
#include "rr_step_body.inc"
}
// Per-environment parameters: the same argument list (load_io / load_tables / load_dims find the block at the same offsets), production
// CG instances of the (2,2,1) slot counts only -- single-step, multi-step, multi-step with the actor.
template <class DT, bool UNROLL = false, bool ACTOR = false>
__global__ __launch_bounds__(RR_LANES, 2) void rr_rand_kernel(const RRDims Dk, const RRTables Tk, const RRIO io_kernarg, const int num_envs, const int n_frames) {
  constexpr int NBS = 2, NVS = 2, NCS = 1;
  constexpr bool PROF = false, DBG = false, NEWTON = false, PAIR = false, DYN = false, RAND = true, EVAL = false, POSE = false, REFOBS = false, PTERM = false, BODY = false, RESTART = false;
  constexpr int MRES = 1;      // resident inverse-factor entries (Wave::MAT_RES): the column side (229-237 registers; both sides reach the cap of 256 here)
  constexpr bool ROOTSLOT = rr_root_slot<DT>::value;
#include "rr_step_body.inc"
}
// Evaluation (rr_env_unroll_eval): the multi-step form with the actor inside as brax's Evaluator and the launcher's evaluation rollout
// use it -- EvalWrapper's sums kept in place, the policy deterministic on request, no trajectory (a two-row observation ring), optionally
// without the Episode / AutoReset wrappers, optionally with the qpos of every step (RRIO::e_*).  A third entry for the same reason
// rr_rand_kernel is one: the instances of the other two keep their token stream, every `if (EVAL)` in the body folds away there.
// Production CG instances of the (2,2,1) slot counts: fixed-dimension, generic, generic with candidate-pair contacts (DYN).
template <class DT, bool DYN = false>
__global__ __launch_bounds__(RR_LANES, 2) void rr_eval_kernel(const RRDims Dk, const RRTables Tk, const RRIO io_kernarg, const int num_envs, const int n_frames) {
  constexpr int NBS = 2, NVS = 2, NCS = 1;
  constexpr bool PROF = false, DBG = false, NEWTON = false, PAIR = false, RAND = false, UNROLL = true, ACTOR = true, EVAL = true, POSE = false, REFOBS = false, PTERM = false, BODY = false, RESTART = false;
  constexpr int MRES = 1;      // resident inverse-factor entries (Wave::MAT_RES): the column side (229-237 registers; both sides reach the cap of 256 here)
  constexpr bool ROOTSLOT = rr_root_slot<DT>::value;
#include "rr_step_body.inc"
}
// Pose tracking (rr_batch_set_pose, rr_pose_io): the env epilogue also rewards the clip's root orientation and joint angles (RRIO, POSE TRACKING).
// A fourth entry for the reason the two above are entries of their own: the instances of the other three keep their code, every
// `if (POSE)` in the body folds away there.  Production CG instances of the (2,2,1) slot counts, shared tables: single-step, multi-step,
// multi-step with the actor.
template <class DT, bool UNROLL = false, bool ACTOR = false>
__global__ __launch_bounds__(RR_LANES, 2) void rr_pose_kernel(const RRDims Dk, const RRTables Tk, const RRIO io_kernarg, const int num_envs, const int n_frames) {
  constexpr int NBS = 2, NVS = 2, NCS = 1;
  constexpr bool PROF = false, DBG = false, NEWTON = false, PAIR = false, DYN = false, RAND = false, EVAL = false, POSE = true, REFOBS = false, PTERM = false, BODY = false, RESTART = false;
  constexpr int MRES = 1;      // resident inverse-factor entries (Wave::MAT_RES): the column side (229-237 registers; both sides reach the cap of 256 here)
  constexpr bool ROOTSLOT = rr_root_slot<DT>::value;
#include "rr_step_body.inc"
}
// Pose termination (rr_batch_set_pose_termination) without body tracking: the env steps of a batch that carries a termination block and
// no body block, at any frame count -- rr_body_kernel below with BODY off.  REFOBS is on, so ref_frames = 0 is the same code with zero
// blocks and the actor inside reads RR_ACTOR_JM_REFOBS entries per lane.  rr_body_kernel computes the same bits for these launches
// (tests/test_gpu_pose_family.py); the entry is kept for the one-launch rollout with the actor inside, which ran 0.27 % slower on
// rr_body_kernel in six of six pairs.  The same nine forms as rr_pose_kernel.
template <class DT, bool UNROLL = false, bool ACTOR = false>
__global__ __launch_bounds__(RR_LANES, 2) void rr_poseterm_kernel(const RRDims Dk, const RRTables Tk, const RRIO io_kernarg, const int num_envs, const int n_frames) {
  constexpr int NBS = 2, NVS = 2, NCS = 1;
  constexpr bool PROF = false, DBG = false, NEWTON = false, PAIR = false, DYN = false, RAND = false, EVAL = false, POSE = true, REFOBS = true, PTERM = true, BODY = false, RESTART = false;
  constexpr int MRES = 1;      // resident inverse-factor entries (Wave::MAT_RES): the column side, as in rr_pose_kernel
  constexpr bool ROOTSLOT = rr_root_slot<DT>::value;
#include "rr_step_body.inc"
}
// The options of pose tracking -- reference frames (rr_batch_set_reference_obs; RRIO, REFERENCE OBSERVATION), pose termination
// (rr_batch_set_pose_termination; POSE TERMINATION) and body tracking (rr_batch_set_body_tracking; BODY TRACKING) -- in ONE set of
// instances: POSE, REFOBS, PTERM and BODY are all on, and this entry serves every combination of the three on a batch.  What a batch
// does not carry reaches the kernel switched off at run time: ref_frames = 0 is the same code with zero blocks (the row is rr_obs_width =
// obs_dim wide), no termination block is +inf thresholds and a null pose_fail, no body block a null track_bodies.  Velocity tracking
// (rr_batch_set_velocity_tracking; VELOCITY TRACKING) rides here too, under `if (BODY)`: no such block is a null track_vel.  Env steps of
// a batch with any of the four run it; the single-step form also serves the RESETS of a batch with ref_frames > 0 (they write the blocks; the
// step-only code is not reached at reset).  A batch with the pose block alone stays on rr_pose_kernel, whose actor reads the narrower
// row.  An entry of its own for the reason the others are: every `if (REFOBS)`, `if (PTERM)` and `if (BODY)` in the body folds away in
// their instances.  The same nine forms as rr_pose_kernel; the actor inside reads RR_ACTOR_JM_REFOBS entries per lane whatever the frame
// count.
template <class DT, bool UNROLL = false, bool ACTOR = false>
__global__ __launch_bounds__(RR_LANES, 2) void rr_body_kernel(const RRDims Dk, const RRTables Tk, const RRIO io_kernarg, const int num_envs, const int n_frames) {
  constexpr int NBS = 2, NVS = 2, NCS = 1;
  constexpr bool PROF = false, DBG = false, NEWTON = false, PAIR = false, DYN = false, RAND = false, EVAL = false, POSE = true, REFOBS = true, PTERM = true, BODY = true, RESTART = false;
  constexpr int MRES = 1;      // resident inverse-factor entries (Wave::MAT_RES): the column side, as in rr_pose_kernel
  constexpr bool ROOTSLOT = rr_root_slot<DT>::value;
#include "rr_step_body.inc"
}
// Clip restarts (rr_batch_set_clip_restarts): the multi-step rr_body_kernel instances with the AutoReset restore drawn from a bank of start
// states, the restored frame and the clip-end truncation (RRIO, CLIP RESTARTS), served to the multi-step launches of a batch that carries
// the block.  An entry of its own for the reason the others are: every `if (RESTART)` in the body folds away in their instances.  POSE,
// REFOBS, PTERM and BODY are on -- a superset instance: ref_frames = 0 is that code with zero blocks, no termination block is +inf
// thresholds and a null pose_fail, no body block a null track_bodies, no velocity block a null track_vel.  Multi-step forms only (a single step has no restore in the
// kernel): without and with the actor, which reads RR_ACTOR_JM_REFOBS entries per lane whatever the frame count.
template <class DT, bool ACTOR = false>
__global__ __launch_bounds__(RR_LANES, 2) void rr_restart_kernel(const RRDims Dk, const RRTables Tk, const RRIO io_kernarg, const int num_envs, const int n_frames) {
  constexpr int NBS = 2, NVS = 2, NCS = 1;
  constexpr bool PROF = false, DBG = false, NEWTON = false, UNROLL = true, PAIR = false, DYN = false, RAND = false, EVAL = false, POSE = true, REFOBS = true, PTERM = true, BODY = true, RESTART = true;
  constexpr int MRES = 1;      // resident inverse-factor entries (Wave::MAT_RES): the column side, as in rr_pose_kernel
  constexpr bool ROOTSLOT = rr_root_slot<DT>::value;
#include "rr_step_body.inc"
}
// The production single-step instance with the inverse factor's entries left in LDS (MRES 0), whatever RR_SOLVE_MAT_RESIDENT says: the other
// arm of an exact A/B inside one library (rr_batch_set_solve_resident(b, 0); tests/test_gpu_solve_resident.py).  An entry of its own so
// that the instances of the other seven keep their code.
template <class DT>
__global__ __launch_bounds__(RR_LANES, 2) void rr_matlds_kernel(const RRDims Dk, const RRTables Tk, const RRIO io_kernarg, const int num_envs, const int n_frames) {
  constexpr int NBS = 2, NVS = 2, NCS = 1, MRES = 0;
  constexpr bool ROOTSLOT = rr_root_slot<DT>::value;
  constexpr bool PROF = false, DBG = false, NEWTON = false, UNROLL = false, ACTOR = false, PAIR = false, DYN = false, RAND = false, EVAL = false, POSE = false, REFOBS = false, PTERM = false, BODY = false, RESTART = false;
#include "rr_step_body.inc"
}
// The production single-step instance with the tree phases on the plain lane <-> body map b = lane + 64 s (Wave::ROOT off), whatever
// RR_ROOT_SLOT says: the other arm of an exact A/B inside one library (rr_batch_set_root_slot(b, 0); tests/test_gpu_root_slot.py).  An
// entry of its own so that the instances of the other eight keep their code.
template <class DT>
__global__ __launch_bounds__(RR_LANES, 2) void rr_twoslot_kernel(const RRDims Dk, const RRTables Tk, const RRIO io_kernarg, const int num_envs, const int n_frames) {
  constexpr int NBS = 2, NVS = 2, NCS = 1, MRES = 2;
  constexpr bool ROOTSLOT = false;
  constexpr bool PROF = false, DBG = false, NEWTON = false, UNROLL = false, ACTOR = false, PAIR = false, DYN = false, RAND = false, EVAL = false, POSE = false, REFOBS = false, PTERM = false, BODY = false, RESTART = false;
#include "rr_step_body.inc"
}
