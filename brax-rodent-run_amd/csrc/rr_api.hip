// rr_api.hip -- host side of librodent_hip.so: model blob loader, device upload of the kernel
// tables, LDS / debug layouts and the launch wrappers behind the C ABI of include/rodent_rr.h.
#include "../../include/rodent_rr.h"
#include "rr_kernel.h"
#include "rr_mlp.h"
#include "rr_ppo.h"

#include <atomic>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) { g_err = msg; return code; }
extern "C" const char* rr_last_error(void) { return g_err.c_str(); }

#define HIPCHK(x)                                                                                  \
  do {                                                                                             \
    hipError_t e_ = (x);                                                                           \
    if (e_ != hipSuccess) return fail(RR_EHIP, std::string(#x) + ": " + hipGetErrorString(e_));   \
  } while (0)

typedef void (*kern_t)(const RRDims, const RRTables, const RRIO, const int, const int);
// ------------------------------------------------------------------------------------------ model
struct Entry { int dtype, ndim, dims[4]; size_t count; const void* data; };

struct rr_model {
  std::vector<unsigned char> raw;
  std::map<std::string, Entry> e;
  rr_dims dims;
  RRDims kd;
  std::vector<std::string> dbg_names;
  std::vector<int32_t> dbg_off, dbg_size;
  std::vector<const char*> dbg_cnames;
  int NBS, NVS, NCS;
  bool stage_ok = true;
  int solver = 1;          // 1 = CG, 2 = Newton [REF Rodent_Env_Brax.py:42-45]
  // two identical trees (rodent_pair.xml): dims / LDS layout of ONE replica for the two-wave instance (rr_kernel.h PAIR), from the
  // blob's h_* tables; pair_ok = the blob carries them and a PAIR kernel instance matches
  bool pair_ok = false;
  RRDims kd_rep;
  bool dyn = false;        // candidate-pair contacts between moving bodies / condim 1 / tendon transmissions (rr_kernel.h DYN; blob k_dyn)
  mutable std::atomic<int> live_batches{0};     // batches bake the model's LDS layout at creation: the solver type is fixed while any exist

  const Entry* find(const char* n) const { auto it = e.find(n); return it == e.end() ? nullptr : &it->second; }
  int iscalar(const char* n) const { const Entry* x = find(n); return x ? ((const int32_t*)x->data)[0] : 0; }
  float fscalar(const char* n, int i = 0) const { const Entry* x = find(n); return x ? ((const float*)x->data)[i] : 0.f; }
};

// ------------------------------------------------------------------------------------------ kernel instances
// One function maps (model, launch form, variant) to the kernel instance that serves it, or to the reason there is none: launch(),
// the support queries and the attribute loop of rr_batch_create all ask it, so none of them can disagree about what exists.
enum Form { F_STEP, F_UNROLL, F_ACTOR, F_EVAL, N_FORMS };                        // single step | multi-step | ... with the actor | evaluation
enum Variant { V_PROD, V_DEBUG, V_PROFILE, V_RAND, V_PAIR, V_POSE, V_MATLDS, V_POSETERM, V_TWOSLOT, V_BODY, V_RESTART, N_VARIANTS }; // production | debug dump | cycle-stamp profile | per-env parameters | two-wave pair | pose tracking, the pose block alone | production, inverse factor read from LDS | pose tracking with pose termination and no body tracking (V_BODY computes the same; kept for its speed with the actor inside) | production, tree phases on the plain lane <-> body map | pose tracking with any of reference frames, pose termination and body tracking | ... with the restore from the bank of start states (multi-step forms only; a superset of V_BODY)
struct Instance { kern_t kern; const char* why = nullptr; bool fixed = false; };      // why: the reason when kern is null (multi-step forms: with the entry point that reports it); fixed: compiled for the model's dimensions

// The shape the root-slot tree phases need beyond the dimensions (rr_kernel.h Wave::ROOT): one tree; body 1 is the child of the world and
// holds the model's only free joint, on qpos[0 .. 6] and dofs 0 .. 5; its subtree is every body; at most two bodies beyond the 64 lanes.
static bool root_slot_ok(const rr_model* m) {
  const int nbody = m->dims.nbody, njnt = m->dims.njnt;
  if (m->kd.nroot != 1 || nbody < 2 || nbody - RR_LANES > 2) return false;
  const int32_t* bi = (const int32_t*)m->find("k_body_i")->data;
  const int32_t* ji = (const int32_t*)m->find("k_jnt_i")->data;
  if ((int)m->find("k_body_i")->count < RR_BODYI * nbody || (int)m->find("k_jnt_i")->count < 4 * njnt) return false;
  const int32_t* r = bi + RR_BODYI;      // parent, jadr, jn, dofadr, dofnum, root, .., .., depth, sib, last
  if (r[0] != 0 || r[2] != 1 || r[3] != 0 || r[4] != 6 || r[10] != nbody - 1 || r[1] < 0 || r[1] >= njnt) return false;
  if (ji[4 * r[1]] != 0 || ji[4 * r[1] + 1] != 0 || ji[4 * r[1] + 2] != 0) return false;
  for (int j = 0; j < njnt; ++j) if (j != r[1] && ji[4 * j] == 0) return false;
  for (int b = 2; b < nbody; ++b) if (bi[RR_BODYI * b] < 1) return false;
  return true;
}
// the fixed-dimension instances of the rodent_optimized dimensions serve this model: the dimensions match, and where those instances
// run the root-slot tree phases (RR_ROOT_SLOT) the model has the shape for them; a model that has not runs the generic instances
static bool rodent_fixed(const rr_model* m) { return RRDimsRodent::matches(m->kd) && (!rr_root_slot<RRDimsRodent>::value || root_slot_ok(m)); }

// The sentence with which rr_env_unroll_eval refuses a pose batch, worded after the most specific block the batch carries (defined with
// the batch's option checks below).  Null batch: the pose block alone.
static const char* pose_eval_refusal(const rr_batch* b);

// b: the batch whose blocks word the evaluation refusal of the pose variants; it decides nothing else
static Instance select(const rr_model* m, Form form, Variant v, const rr_batch* b = nullptr) {
  const bool s111 = m->NBS == 1 && m->NVS == 1 && m->NCS == 1, s221 = m->NBS == 2 && m->NVS == 2 && m->NCS == 1, s332 = m->NBS == 3 && m->NVS == 3 && m->NCS == 2;
  const bool newton = m->solver == 2, eval = form == F_EVAL, unroll = form != F_STEP, actor = form == F_ACTOR;
  const char *no_diag = "no diagnostic kernel instance for this model", *no_slots = "no kernel instance for this model's slot counts";
  auto no = [](const char* why) { return Instance{nullptr, why}; };
  // rr_step_kernel<NBS, NVS, NCS, PROF, DBG, dims, NEWTON, UNROLL, ACTOR, PAIR, DYN>, rr_rand_kernel<dims, UNROLL, ACTOR>, rr_eval_kernel<dims, DYN>,
  // rr_pose_kernel<dims, UNROLL, ACTOR>, rr_poseterm_kernel<dims, UNROLL, ACTOR>, rr_body_kernel<dims, UNROLL, ACTOR>, rr_restart_kernel<dims, ACTOR>, rr_matlds_kernel<dims>, rr_twoslot_kernel<dims>
  if (v == V_PAIR && (unroll || newton || !RRDimsRodentNew::matches(m->kd_rep))) return no("no two-wave pair instance for this model / launch form");
  if (v == V_PAIR) return {rr_step_kernel<2, 2, 1, false, false, RRDimsRodentNew, false, false, false, true>, nullptr, true};      // one replica = the rodent_new dims
  if (v == V_MATLDS) {      // rr_batch_set_solve_resident(b, 0): the production single-step instance of the benchmark model's dimensions, solves from LDS
    if (newton || m->dyn || m->pair_ok || !s221 || !rodent_fixed(m))
      return no("rr_batch_set_solve_resident: only the fixed-dimension CG instance of the rodent_optimized dimensions has a form that solves from LDS");
    if (unroll) return no("rr_batch_set_solve_resident(b, 0): the instance that solves from LDS is single-step; no multi-step, actor or evaluation launch on this batch");
    return {rr_matlds_kernel<RRDimsRodent>, nullptr, true};
  }
  if (v == V_TWOSLOT) {      // rr_batch_set_root_slot(b, 0): the production single-step instance of the benchmark model, tree phases on the plain map
    if (newton || m->dyn || m->pair_ok || !s221 || !rodent_fixed(m))
      return no("rr_batch_set_root_slot: only the fixed-dimension CG instance of the rodent_optimized model runs the tree phases with the root body in a slot of its own");
    if (unroll) return no("rr_batch_set_root_slot(b, 0): the instance with the plain lane-to-body map is single-step; no multi-step, actor or evaluation launch on this batch");
    return {rr_twoslot_kernel<RRDimsRodent>, nullptr, true};
  }
  // Eligibility first.  Multi-step instances: the single-rodent floor-contact models (fixed-dimension or generic) and the candidate-pair models
  // (DYN, generic dimensions), CG only, no diagnostics.  None for the Newton solver, the two-wave pair instance and other slot counts.
  if (unroll && (v == V_DEBUG || v == V_PROFILE)) return no("rr_env_unroll: no diagnostic outputs in a multi-step rollout");
  if (eval) {
    // Evaluation instances (rr_eval_kernel): the production CG multi-step form with the actor of the (2,2,1) slot counts, fixed-dimension,
    // generic or generic with candidate-pair contacts; shared tables only
    if (newton) return no("rr_env_unroll_eval: the Newton solver has no multi-step instance");
    if (m->pair_ok) return no("rr_env_unroll_eval: two-tree models served by the two-wave pair instance have no multi-step instance");
    if (!s221) return no("rr_env_unroll_eval: only the (2,2,1) slot counts have an evaluation instance");
    if (v == V_RAND) return no("rr_env_unroll_eval: no evaluation instance reads per-env parameters (this batch carries some)");
    if (v == V_POSE || v == V_POSETERM || v == V_BODY || v == V_RESTART) return no(pose_eval_refusal(b));
  } else if (v == V_POSE || v == V_POSETERM || v == V_BODY || v == V_RESTART) {
    // Pose tracking (rr_pose_kernel: the pose block alone; rr_body_kernel: with any of reference frames, pose termination and body
    // tracking; rr_poseterm_kernel: pose termination without body tracking; rr_restart_kernel: with clip restarts): the same models and
    // launch forms as the per-env parameters below, shared tables
    if (m->dyn) return no("pose tracking: models with candidate-pair contacts (DYN instances) have no pose instance");
    if (m->pair_ok) return no("pose tracking: two-tree models served by the two-wave pair instance have no pose instance");
    if (newton) return no("pose tracking: the Newton solver's instances have no pose instance");
    if (!s221) return no("pose tracking: only the (2,2,1) slot counts have pose instances");
    if (v == V_RESTART && !unroll) return no("clip restarts: the restore lives in the multi-step instances (rr_env_unroll, rr_env_unroll_policy); a single step has none");
  } else if (v == V_RAND) {
    // Per-environment parameters (rr_rand_kernel): the production CG instances of the single-rodent floor-contact models -- fixed-dimension
    // or generic (2,2,1) -- as single-step, multi-step and multi-step with the actor
    if (m->dyn) return no("models with candidate-pair contacts (DYN instances) have none");
    if (m->pair_ok) return no("two-tree models served by the two-wave pair instance have none");
    if (newton) return no("the Newton solver's instances have none");
    if (!s221) return no("only the (2,2,1) slot counts have instances with per-env parameters");
  } else if (unroll && (newton || !s221))
    return no("rr_env_unroll: no multi-step kernel instance for this model / solver");
  if (m->dyn) {      // candidate-pair contacts: the production instances and the single-step debug dump (generic dimensions); no profile build
    if (v != V_PROD && (v != V_DEBUG || newton || !s221)) return no(no_diag);
    if (newton || !s221) return no(no_slots);
    if (v == V_DEBUG) return Instance{rr_step_kernel<2, 2, 1, false, true, RRDims, false, false, false, false, true>};      // multi-step forms: refused above
    if (eval) return Instance{rr_eval_kernel<RRDims, true>};
    return Instance{actor ? rr_step_kernel<2, 2, 1, false, false, RRDims, false, true, true, false, true>
                    : (unroll ? rr_step_kernel<2, 2, 1, false, false, RRDims, false, true, false, false, true> : rr_step_kernel<2, 2, 1, false, false, RRDims, false, false, false, false, true>)};
  }
  // Single step besides production: debug dump (generic dims; selected per launch when rr_outputs.debug is given), cycle-stamp profile
  // (diagnostic, rodent dims or generic 2,2,1)
  if (v == V_PROFILE && (newton || !s221)) return no(no_diag);
  if (v == V_PROFILE) return rodent_fixed(m) ? Instance{rr_step_kernel<2, 2, 1, true, false, RRDimsRodent>, nullptr, true} : Instance{rr_step_kernel<2, 2, 1, true, false, RRDims>};
  if (newton)     // Newton: the (2,2,1) generic instances only (rr_model_set_solver_type checks)
    return Instance{v == V_DEBUG ? rr_step_kernel<2, 2, 1, false, true, RRDims, true> : rr_step_kernel<2, 2, 1, false, false, RRDims, true>};
  if (v == V_DEBUG)
    return s111 ? Instance{rr_step_kernel<1, 1, 1, false, true, RRDims>} : (s221 ? Instance{rr_step_kernel<2, 2, 1, false, true, RRDims>} : (s332 ? Instance{rr_step_kernel<3, 3, 2, false, true, RRDims>} : no(no_diag)));
  if (!s221) return s111 ? Instance{rr_step_kernel<1, 1, 1, false, false, RRDims>} : (s332 ? Instance{rr_step_kernel<3, 3, 2, false, false, RRDims>} : no(no_slots));
  auto family = [&](auto* t) -> kern_t {      // the (2,2,1) CG production family: one set per dims type
    typedef typename std::remove_pointer<decltype(t)>::type DT;      // t: a null pointer that names the dims type
    if (eval) return rr_eval_kernel<DT>;
    if (v == V_RAND) return actor ? rr_rand_kernel<DT, true, true> : (unroll ? rr_rand_kernel<DT, true> : rr_rand_kernel<DT>);
    if (v == V_POSE) return actor ? rr_pose_kernel<DT, true, true> : (unroll ? rr_pose_kernel<DT, true> : rr_pose_kernel<DT>);
    if (v == V_POSETERM) return actor ? rr_poseterm_kernel<DT, true, true> : (unroll ? rr_poseterm_kernel<DT, true> : rr_poseterm_kernel<DT>);
    if (v == V_BODY) return actor ? rr_body_kernel<DT, true, true> : (unroll ? rr_body_kernel<DT, true> : rr_body_kernel<DT>);
    if (v == V_RESTART) return actor ? rr_restart_kernel<DT, true> : rr_restart_kernel<DT>;
    return actor ? rr_step_kernel<2, 2, 1, false, false, DT, false, true, true> : (unroll ? rr_step_kernel<2, 2, 1, false, false, DT, false, true> : rr_step_kernel<2, 2, 1, false, false, DT>);
  };
  if (rodent_fixed(m)) return {family((RRDimsRodent*)nullptr), nullptr, true};      // fixed-dimension instances (rr_kernel.h RRDimsFixed)
  if (RRDimsRodentNew::matches(m->kd)) return {family((RRDimsRodentNew*)nullptr), nullptr, true};
  return Instance{family((RRDims*)nullptr)};
}

static void set_layout(RRDims& k, const RRLayout& L) {
  k.o_qpos = L.o_qpos; k.o_qvel = L.o_qvel; k.o_act = L.o_act; k.o_ctrl = L.o_ctrl; k.o_xpos = L.o_xpos; k.o_xquat = L.o_xquat;
  k.o_cinert = L.o_cinert; k.o_cdof = L.o_cdof; k.o_cvel = L.o_cvel; k.o_qLD = L.o_qLD; k.o_vec = L.o_vec; k.o_x = L.o_x;
  k.o_arm = L.o_arm; k.o_warm = L.o_warm; k.o_qact = L.o_qact; k.o_jlist = L.o_jlist; k.lds_floats = L.lds_floats;
  k.o_H = L.o_H; k.o_Mp = L.o_Mp; k.o_anc = L.o_anc;      // 0 unless Newton
}
// staging of the line search's compacted rows: cinert | cvel | pose regions each hold 4*ncon + nv floats; the alias cells share the pose cells
static bool stage_fits(int nbody, int nv, int con_slots, int nalias) {
  const int pose = std::max(7 * nbody + 4, 6 * nv);
  return 2 * (nalias + 4) <= pose && 2 * (nbody + 8) <= pose && 6 * con_slots <= pose && 4 * con_slots + nv <= std::min(std::min(10 * nbody, 6 * nbody), pose);
}
// the solve job tables `prefix`k_coljob / k_rowjob against the job slots and loop bounds of the kernel instance
static bool solve_jobs_fit(const rr_model* m, const char* prefix, int njs, const RRDims& k) {
  return (int)m->find((std::string(prefix) + "k_coljob").c_str())->count == 9 * njs && (int)m->find((std::string(prefix) + "k_rowjob").c_str())->count == 5 * njs &&
         k.lmax <= 16 && k.lmax >= 1 && k.cmax <= 8 && k.rmax <= 8 && k.cmax >= 1;
}

static void layout(rr_model* m) {
  RRDims& k = m->kd;
  const rr_dims& d = m->dims;
  const int con_slots = m->dyn ? m->NCS * RR_LANES : d.ncon;      // DYN: the wave holds the pairs in penetration in its contact slots
  const RRLayout L = rr_layout(d.nq, d.nv, d.nu, d.nbody, d.nM, con_slots, m->solver == 2);
  set_layout(k, L);
  k.solver = m->solver;
  // factorisation schedule: with alias copies of the hot rows in the pose cells (levelsched.py); the Newton instances reuse the schedule
  // on the Hessian's array through an address shift, which the alias cells would not follow, so they run the alias-free one
  k.nfac = m->iscalar(m->solver == 2 ? "k_factor3p_rows" : "k_factor3_rows");
  k.nalias = m->solver == 2 ? 0 : m->iscalar("k_nalias");
  m->dbg_names.clear(); m->dbg_off.clear(); m->dbg_size.clear(); m->dbg_cnames.clear();      // layout() may run again (rr_model_set_solver_type)
  m->stage_ok = stage_fits(d.nbody, d.nv, con_slots, k.nalias);
  if (m->dyn && d.nu > std::max(7 * d.nbody + 4, 6 * d.nv)) m->stage_ok = false;      // actuator forces go through the pose cells
  // debug dump
  int g = 0;
  auto dbg = [&](const char* name, int n) { int r = g; m->dbg_names.push_back(name); m->dbg_off.push_back(g); m->dbg_size.push_back(n); g += n; return r; };
  k.g_xpos = dbg("xpos", 3 * d.nbody); k.g_xquat = dbg("xquat", 4 * d.nbody); k.g_xmat = dbg("xmat", 9 * d.nbody);
  k.g_com = dbg("subtree_com", 6); k.g_cinert = dbg("cinert", 10 * d.nbody); k.g_crb = dbg("crb", 10 * d.nbody);
  k.g_cdof = dbg("cdof", 6 * d.nv); k.g_cvel = dbg("cvel", 6 * d.nbody); k.g_cfrc = dbg("cfrc", 6 * d.nbody);
  k.g_qM = dbg("qM", d.nM); k.g_qLD = dbg("qLD", d.nM); k.g_dinv = dbg("qLDiagInv", d.nv);
  k.g_bias = dbg("qfrc_bias", d.nv); k.g_passive = dbg("qfrc_passive", d.nv); k.g_actuator = dbg("qfrc_actuator", d.nv);
  k.g_smooth = dbg("qfrc_smooth", d.nv); k.g_qacc_smooth = dbg("qacc_smooth", d.nv);
  k.g_con_dist = dbg("con_dist", d.ncon); k.g_con_pos = dbg("con_pos", 3 * d.ncon); k.g_con_frame = dbg("con_frame", 9 * d.ncon);
  k.g_con_D = dbg("con_D", d.ncon); k.g_con_aref = dbg("con_aref", 4 * d.ncon); k.g_lim = dbg("limit_pos_D_aref", 3 * d.nv);
  k.g_qacc = dbg("qacc", d.nv); k.g_qfrc_constraint = dbg("qfrc_constraint", d.nv); k.g_misc = dbg("niter_cost", 2);
  k.g_ls_iters = dbg("ls_iters", 2);      // bracketing iterations of the last substep's line searches: executed, left out by the repeat exit
  // the last substep's solve(): [0] 1 = the context at qacc_smooth was chosen, 0 = the one at qacc_warmstart; [1] how the loop ended, a sum of
  // 1 = iteration cap, 2 = improvement below the tolerance, 4 = gradient below the tolerance
  k.g_solver_end = dbg("solver_end", 2);
  k.g_kaok = dbg("kernarg_ok", 1);
  // candidate-pair models: the scan's count before the clamp to the slots, and the pair id held by each slot (-1 beyond the count); the
  // kernel finds both behind kernarg_ok (contact_geometry_dyn), so RRDims carries no offset for them
  static_assert(RR_DBG_PEN_COUNT == 1 && RR_DBG_SLOT_PAIR == RR_DBG_PEN_COUNT + 1, "pen_count (1 float) and slot_pair follow kernarg_ok (1 float) in this order");
  if (m->dyn) { dbg("pen_count", 1); dbg("slot_pair", m->NCS * RR_LANES); }
  k.dbg_floats = g;
  for (auto& s : m->dbg_names) m->dbg_cnames.push_back(s.c_str());
  m->dims.lds_bytes = L.lds_floats * (int)sizeof(float);
  m->dims.dbg_floats = g;
  m->dims.solver = m->solver;
  // 1: the production launches of this model run an instance compiled for its dimensions (rr_kernel.h RRDimsFixed); 0: the generic
  // instance (same results, ~10 % slower).  The constants cover the schedule-table parameters, so a compiler change that moves
  // them shows up here (tests/test_abi_and_oracle.py) instead of as a silent slowdown.
  m->dims.fixed_instance = select(m, F_STEP, V_PROD).fixed ? 1 : 0;
}

// Two-wave (PAIR) instance: dims of one replica from the blob's h_* tables (rodent_amd/ktables.py replica_model).  RR_PAIR_WAVES=0
// keeps such models on the generic one-wave instance (A/B runs).
static void setup_replica(rr_model* m) {
  m->pair_ok = false;
  const char* sw = getenv("RR_PAIR_WAVES");
  if (sw && sw[0] == '0') return;
  static const char* need[] = {"h_dims", "h_k_slots", "h_k_body_i", "h_k_body_f", "h_k_jnt_i", "h_k_jnt_f", "h_k_dof_i", "h_k_dof_f", "h_k_act_f", "h_k_M_ij_k",
                               "h_k_body_anc", "h_k_nround", "h_k_factor3", "h_k_factor3_rows", "h_k_linv", "h_k_linv_rows", "h_k_coljob", "h_k_rowjob", "h_k_jobown",
                               "h_k_solve_lmax", "h_k_solve_cmax", "h_k_solve_rmax", "h_k_nalias", "h_k_con_i", "h_k_con_f", "h_k_con_chain_rows", "h_k_root_mass"};
  for (const char* n : need) if (!m->find(n)) return;
  const int32_t* hd = (const int32_t*)m->find("h_dims")->data;       // nq nv nu nbody njnt nM ncon dmax
  const int32_t* sl = (const int32_t*)m->find("h_k_slots")->data;
  if (m->find("h_dims")->count < 8 || sl[0] != 2 || sl[1] != 2 || sl[2] != 1) return;
  if (2 * hd[0] != m->dims.nq || 2 * hd[1] != m->dims.nv || 2 * hd[2] != m->dims.nu || 2 * hd[6] != m->dims.ncon || m->dims.na != m->dims.nu) return;
  RRDims k = m->kd;          // options, gravity, tolerances, meaninertia: the model's
  k.nq = hd[0]; k.nv = hd[1]; k.nu = hd[2]; k.nbody = hd[3]; k.njnt = hd[4]; k.nM = hd[5]; k.ncon = hd[6]; k.dmax = hd[7];
  k.nroot = (int)m->find("h_k_root_mass")->count;
  k.nround = m->iscalar("h_k_nround"); k.ninv = m->iscalar("h_k_linv_rows"); k.nfac = m->iscalar("h_k_factor3_rows"); k.nalias = m->iscalar("h_k_nalias");
  k.lmax = m->iscalar("h_k_solve_lmax"); k.cmax = m->iscalar("h_k_solve_cmax"); k.rmax = m->iscalar("h_k_solve_rmax");
  k.obs_dim = k.nq + k.nv + 16 * (k.nbody - 1) + k.nv + 3;
  const RRLayout L = rr_layout(k.nq, k.nv, k.nu, k.nbody, k.nM, k.ncon, false);
  set_layout(k, L);
  k.solver = 1;
  k.nv_scale = m->dims.nv;                          // the solver's tolerances scale with the MODEL's dof count
  k.lds_bytes_rep = L.lds_floats * 4;
  k.fac_stride = (int)m->find("h_k_factor3")->count; k.inv_stride = (int)m->find("h_k_linv")->count;
  if (!solve_jobs_fit(m, "h_", 2 * RR_LANES, k)) return;
  if (k.nM > RR_LANES * 18 || k.nroot != 1) return;
  if (!stage_fits(k.nbody, k.nv, k.ncon, k.nalias) || 2 * k.lds_bytes_rep + 128 > 64 * 1024) return;
  m->kd_rep = k;
  m->pair_ok = select(m, F_STEP, V_PAIR).kern != nullptr;
}

extern "C" int rr_model_load(const char* path, rr_model** out) {
  if (!path || !out) return fail(RR_EINVAL, "rr_model_load: null argument");
  FILE* f = fopen(path, "rb");
  if (!f) return fail(RR_EIO, std::string("rr_model_load: cannot open ") + path);
  fseek(f, 0, SEEK_END);
  long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  rr_model* m = new rr_model();
  m->raw.resize(n);
  size_t got = fread(m->raw.data(), 1, n, f);
  fclose(f);
  if ((long)got != n || n < 8 || memcmp(m->raw.data(), "RRM1", 4)) { delete m; return fail(RR_EIO, "rr_model_load: not an RRM1 blob"); }
  const unsigned char* raw = m->raw.data();
  uint32_t ne = *(const uint32_t*)(raw + 4);
  if (8 + (size_t)ne * 72 > (size_t)n) { delete m; return fail(RR_EIO, "rr_model_load: truncated header"); }
  const unsigned char* p = raw + 8;
  for (uint32_t i = 0; i < ne; ++i, p += 72) {
    Entry e;
    char name[33] = {0};
    memcpy(name, p, 32);
    e.dtype = *(const uint32_t*)(p + 32);
    e.ndim = *(const uint32_t*)(p + 36);
    for (int k = 0; k < 4; ++k) e.dims[k] = *(const uint32_t*)(p + 40 + 4 * k);
    uint64_t off = *(const uint64_t*)(p + 56), nb = *(const uint64_t*)(p + 64);
    if (off + nb > (uint64_t)n) { delete m; return fail(RR_EIO, "rr_model_load: entry out of range"); }
    e.count = nb / 4;
    e.data = raw + off;
    m->e[name] = e;
  }
  static const char* need[] = {"nq", "nv", "nu", "nbody", "njnt", "ngeom", "nM", "ncon", "nlimit", "nefc", "obs_dim", "k_slots",
                               "k_body_i", "k_body_f", "k_jnt_i", "k_jnt_f", "k_dof_i", "k_dof_f", "k_act_f", "k_M_ij_k", "k_body_anc",
                               "k_nround", "k_factor3", "k_factor3_rows", "k_factor3p", "k_factor3p_rows", "k_nalias", "k_linv", "k_linv_rows", "k_coljob", "k_rowjob",
                               "k_jobown", "k_solve_lmax", "k_solve_cmax", "k_solve_rmax", "k_con_i", "k_con_f", "k_con_chain_packed", "k_con_chain_rows", "k_root_mass",
                               "k_act_i", "k_act_m_i", "k_act_m_f",
                               "dof_depth", "body_depth", "opt_timestep", "opt_gravity", "stat_meaninertia"};
  for (const char* nme : need)
    if (!m->find(nme)) { std::string s = std::string("rr_model_load: blob lacks '") + nme + "'"; delete m; return fail(RR_EIO, s); }
  rr_dims& d = m->dims;
  memset(&d, 0, sizeof(d));
  d.nq = m->iscalar("nq"); d.nv = m->iscalar("nv"); d.nu = m->iscalar("nu"); d.na = m->iscalar("na"); d.nbody = m->iscalar("nbody");
  d.njnt = m->iscalar("njnt"); d.ngeom = m->iscalar("ngeom"); d.nM = m->iscalar("nM"); d.ncon = m->iscalar("ncon");
  d.nlimit = m->iscalar("nlimit"); d.nefc = m->iscalar("nefc"); d.obs_dim = m->iscalar("obs_dim");
  d.iterations = m->iscalar("opt_iterations"); d.ls_iterations = m->iscalar("opt_ls_iterations");
  d.timestep = m->fscalar("opt_timestep");
  const int32_t* sl = (const int32_t*)m->find("k_slots")->data;
  m->NBS = sl[0]; m->NVS = sl[1]; m->NCS = sl[2];
  m->dyn = m->iscalar("k_dyn") != 0;
  if (m->dyn && (m->find("k_con_i")->dims[1] != 8 || m->find("k_con_f")->dims[1] != 32 || (int)m->find("k_con_chain_rows")->count != 10 * (d.ncon + 1) || d.nv >= 128 || d.nu > RR_LANES)) {
    delete m; return fail(RR_EIO, "rr_model_load: candidate-pair tables do not match the DYN kernel instance (stale blob)"); }
  RRDims& k = m->kd;
  memset(&k, 0, sizeof(k));
  k.nq = d.nq; k.nv = d.nv; k.nu = d.nu; k.nbody = d.nbody; k.njnt = d.njnt; k.nM = d.nM; k.ncon = d.ncon;
  int dmax = 0;
  { const Entry* dd = m->find("dof_depth"); for (size_t i = 0; i < dd->count; ++i) dmax = std::max(dmax, ((const int32_t*)dd->data)[i]); }
  k.dmax = dmax;
  k.nroot = (int)m->find("k_root_mass")->count;
  k.nround = m->iscalar("k_nround");
  k.ninv = m->iscalar("k_linv_rows");
  if (d.nM > RR_LANES * (m->NVS == 1 ? 10 : (m->NVS == 2 ? 18 : 35))) { delete m; return fail(RR_EUNSUPPORTED, "rr_model_load: more mass-matrix entries than the kernel's register table"); }
  k.lmax = m->iscalar("k_solve_lmax"); k.cmax = m->iscalar("k_solve_cmax"); k.rmax = m->iscalar("k_solve_rmax");
  if (!solve_jobs_fit(m, "", (m->NVS >= 3 ? m->NVS + 1 : m->NVS) * RR_LANES, k)) {     // Wave::NJS job slots
    delete m; return fail(RR_EIO, "rr_model_load: solve job tables do not match the kernel instance (stale blob)"); }
  k.obs_dim = d.obs_dim; k.iterations = d.iterations; k.ls_iterations = d.ls_iterations;
  k.dt = d.timestep; k.gx = m->fscalar("opt_gravity", 0); k.gy = m->fscalar("opt_gravity", 1); k.gz = m->fscalar("opt_gravity", 2);
  k.tolerance = m->fscalar("opt_tolerance"); k.ls_tolerance = m->fscalar("opt_ls_tolerance");
  k.meaninertia = m->fscalar("stat_meaninertia");
  if (k.nroot > 2) { delete m; return fail(RR_EUNSUPPORTED, "rr_model_load: more than 2 kinematic trees"); }
  if (m->find("k_dof_i")->dims[1] != RR_DOFI) { delete m; return fail(RR_EIO, "rr_model_load: k_dof_i width mismatch (stale blob)"); }
  if (m->find("k_body_i")->dims[1] != RR_BODYI) { delete m; return fail(RR_EIO, "rr_model_load: k_body_i width mismatch (stale blob)"); }
  if (d.nv > 256 || (!m->dyn && d.ncon > 256)) { delete m; return fail(RR_EUNSUPPORTED, "rr_model_load: nv/ncon above the 8-bit table index"); }
  if (m->find("k_con_chain_packed")->dims[1] != m->NCS * RR_LANES) { delete m; return fail(RR_EIO, "rr_model_load: lane-table width mismatch"); }
  k.nv_scale = d.nv > 1 ? d.nv : 1;
  layout(m);
  setup_replica(m);
  *out = m;
  return RR_OK;
}

extern "C" int rr_model_dims(const rr_model* m, rr_dims* out) {
  if (!m || !out) return fail(RR_EINVAL, "rr_model_dims: null argument");
  *out = m->dims;
  return RR_OK;
}
extern "C" int rr_model_set_solver(rr_model* m, int32_t it, int32_t ls) {
  if (!m || it < 0 || ls < 0) return fail(RR_EINVAL, "rr_model_set_solver: bad argument");
  m->dims.iterations = m->kd.iterations = it;
  m->dims.ls_iterations = m->kd.ls_iterations = ls;
  return RR_OK;
}
extern "C" int rr_model_set_solver_type(rr_model* m, int32_t solver) {
  if (!m || (solver != 1 && solver != 2)) return fail(RR_EINVAL, "rr_model_set_solver_type: solver must be 1 (cg) or 2 (newton)");
  if (solver != m->solver && m->live_batches.load() > 0)
    return fail(RR_EINVAL, "rr_model_set_solver_type: batches of this model exist (they hold the LDS layout of the current solver); set the solver before rr_batch_create");
  if (solver == 2 && (!(m->NBS == 2 && m->NVS == 2 && m->NCS == 1) || m->dyn))
    return fail(RR_EUNSUPPORTED, "rr_model_set_solver_type: the Newton instance exists for the single-rodent models only");
  if (solver == 2 && 4 * ((m->dims.nv + 3) & ~3) > std::max(7 * m->dims.nbody + 4, 6 * m->dims.nv))
    return fail(RR_EUNSUPPORTED, "rr_model_set_solver_type: the four Hessian rows do not fit the pose cells");
  m->solver = solver;
  layout(m);
  return RR_OK;
}
extern "C" void rr_model_destroy(rr_model* m) { delete m; }
extern "C" int rr_model_table(const rr_model* m, const char* name, const void** host_ptr, size_t* count, int32_t* dtype) {
  if (!m || !name || !host_ptr) return fail(RR_EINVAL, "rr_model_table: null argument");
  const Entry* e = m->find(name);
  if (!e) return fail(RR_EINVAL, std::string("rr_model_table: the model has no table '") + name + "'");
  *host_ptr = e->data;
  if (count) *count = e->count;
  if (dtype) *dtype = e->dtype;
  return RR_OK;
}
extern "C" int rr_kernarg_layout(int32_t* io_offset, int32_t* io_size, int32_t* total_size) {
  if (io_offset) *io_offset = (int32_t)offsetof(RRKArgs, io);
  if (io_size) *io_size = (int32_t)sizeof(RRIO);
  if (total_size) *total_size = (int32_t)sizeof(RRKArgs);
  return RR_OK;
}

// ------------------------------------------------------------------------------------------ batch
struct rr_batch {
  const rr_model* m;
  int N, device;
  hipStream_t stream;
  RRDims kd;
  RRTables T;
  RRTables T_rep;                       // tables of one replica (two-wave instance of a two-tree model; m->pair_ok)
  std::vector<void*> dev_allocs;
  bool timing = false;
  std::vector<hipEvent_t> ev0, ev1;     // ring of event pairs: launches are timed without a host sync per launch
  int npending = 0, ring_head = 0;      // pending pairs are ring_head .. ring_head + npending - 1 (mod the ring size)
  double total_ms = 0;
  int64_t launches = 0;
  unsigned long long* prof = nullptr;   // diagnostic phase-cycle buffer (rr_batch_set_profile)
  const int32_t* env_map = nullptr;     // rr_batch_set_schedule
  uint32_t* cost = nullptr;
  bool counted = false;                 // this batch is in m->live_batches
  unsigned* dyn_overflow = nullptr;     // DYN models: (env, env step) events in which more pairs penetrated than the wave has contact slots (rr_batch_contact_overflow)
  unsigned* bad_states = nullptr;       // (env, env step) events of the bad-state check (rr_env_io::bad_state_max; rr_batch_bad_states)
  unsigned* progress = nullptr;         // pacing counter of multi-step launches (RRIO::progress); RR_PACE=0 turns pacing off
  float *env_dof_f = nullptr, *env_act_f = nullptr, *env_con_f = nullptr;     // per-env parameter rows, owned (rr_batch_set_env_params)
  int dbg_flags = 0;                    // debug-dump launches, RRIO::dbg_flags: RR_DBG_LS_RUN_REPEATS (rr_batch_set_ls_repeat_exit(b, 0)), RR_DBG_SOLVER_UNTRIMMED (rr_batch_set_solver_trim(b, 0)), RR_DBG_SOLVER_UNBATCHED (rr_batch_set_solver_batch(b, 0))
  float* eval_actions = nullptr;        // [N][nu]: where an evaluation launch without actions_out keeps the current action (rr_env_unroll_eval)
  rr_pose_io pose = {};                 // pose tracking of the env steps (rr_batch_set_pose); track_pose null: off
  int ref_frames = 0;                   // reference frames in every observation row (rr_batch_set_reference_obs); > 0 only with a pose block
  int obs_width() const { return m->dims.obs_dim + ref_frames * m->dims.nq; }      // of obs, first_obs, traj_obs, obs_in, mean, std, w0's rows
  rr_pose_term_io pterm = {};           // pose termination of the env steps (rr_batch_set_pose_termination); fail null: off; set only with a pose block
  bool plain_slots = false;             // rr_batch_set_root_slot(b, 0): production single-step launches run rr_twoslot_kernel
  rr_body_io body = {};                 // body tracking of the env steps (rr_batch_set_body_tracking); track_bodies null: off; set only with a pose block
  rr_clip_restart_io restart = {};      // clip restarts of the multi-step launches (rr_batch_set_clip_restarts); frames null: off; set only with a pose block
  bool solve_lds = false;               // rr_batch_set_solve_resident(b, 0): production single-step launches run rr_matlds_kernel
  rr_vel_io vel = {};                   // velocity tracking of the env steps (rr_batch_set_velocity_tracking); track_vel null: off; set only with a pose block
  rr_clip_library_io lib = {};          // clip library of the env launches (rr_batch_set_clip_library); both pointers null: off; set only with a pose block
  bool has_clip_library() const { return lib.clip_lengths || lib.bank_clips; }
  rr_clip_sampling_io samp = {};        // clip sampling of the multi-step launches (rr_batch_set_clip_sampling); clip_weights and outcomes null: off; set only with a clip-restart block
  bool has_clip_sampling() const { return samp.clip_weights || samp.outcomes; }
  rr_reference_restart_io refr = {};    // reference restarts of the multi-step launches (rr_batch_set_reference_restart); draws_in null: off; set only with a clip-restart block
  bool has_env_params() const { return env_dof_f || env_act_f || env_con_f; }
};

static const char* pose_eval_refusal(const rr_batch* b) {
  if (b && b->has_clip_library()) return "rr_env_unroll_eval: no evaluation instance reads per-clip lengths or moves an env to another clip (rr_batch_set_clip_library is on); evaluate step by step";
  if (b && b->restart.frames) return "rr_env_unroll_eval: no evaluation instance restores from the bank of start states (rr_batch_set_clip_restarts is on); evaluate step by step";
  if (b && b->body.track_bodies) return "rr_env_unroll_eval: no evaluation instance rewards the body positions (rr_batch_set_body_tracking is on); evaluate step by step";
  if (b && b->vel.track_vel) return "rr_env_unroll_eval: no evaluation instance rewards the velocities (rr_batch_set_velocity_tracking is on); evaluate step by step";
  if (b && b->pterm.fail) return "rr_env_unroll_eval: no evaluation instance ends episodes on the pose error (rr_batch_set_pose_termination is on); evaluate step by step";
  if (b && b->ref_frames > 0) return "rr_env_unroll_eval: no evaluation instance writes the reference observation (rr_batch_set_reference_obs is on); evaluate step by step";
  return "rr_env_unroll_eval: no evaluation instance rewards the pose (this env io carries track_pose); evaluate step by step";
}

// hipMalloc recorded in the batch (rr_batch_destroy frees it), filled from `host` when given
template <typename Ptr>
static int dev_alloc(rr_batch* b, size_t bytes, Ptr* dst, const void* host = nullptr, size_t host_bytes = 0) {
  void* p = nullptr;
  HIPCHK(hipMalloc(&p, bytes));
  b->dev_allocs.push_back(p);
  if (host_bytes) HIPCHK(hipMemcpy(p, host, host_bytes, hipMemcpyHostToDevice));
  *dst = (Ptr)p;
  return RR_OK;
}
template <typename Ptr>
static int upload(rr_batch* b, const char* name, Ptr* dst) {
  const Entry* e = b->m->find(name);
  return dev_alloc(b, std::max<size_t>(e->count, 1) * 4, dst, e->data, e->count * 4);
}

// Row schedules (k_factor3, k_linv): element indices -> LDS byte addresses (rr_kernel.h run_levels).  Indices below nM + 4 are cells of
// the sparse-matrix array at `base`; the alias cells nM + 4 .. live at `alias_base` (the pose cells).
// `copies` = 2 (two-wave instance): a second copy behind the first, addressed into the second wavefront's LDS region (+ rep_bytes).
static int upload_levels(rr_batch* b, const char* name, rr_gi* dst, uint32_t base, uint32_t alias_base, uint32_t nM, int copies = 1, uint32_t rep_bytes = 0) {
  const Entry* e = b->m->find(name);
  std::vector<uint32_t> t((size_t)copies * e->count);
  for (int c = 0; c < copies; ++c) {
    const uint32_t* src = (const uint32_t*)e->data;
    uint32_t* tc = t.data() + (size_t)c * e->count;
    const uint32_t cb = base + (uint32_t)c * rep_bytes, ab = alias_base + (uint32_t)c * rep_bytes;
    for (size_t i = 0; i + 3 < e->count; i += 4) {        // x = a | b0 << 16, y = d0 | d1 << 16, z = d2 | d3 << 16, w = q
      uint32_t f[6] = {src[i] & 0xFFFFu, src[i] >> 16, src[i + 1] & 0xFFFFu, src[i + 1] >> 16, src[i + 2] & 0xFFFFu, src[i + 2] >> 16};
      for (uint32_t& v : f) {                              // 8 bytes per entry: pairs
        v = v < nM + 4u ? v * 8u + cb : (v - (nM + 4u)) * 8u + ab;
        if (v > 0xFFFFu) return fail(RR_EUNSUPPORTED, "level schedule does not fit the 16-bit LDS address fields");
      }
      const uint32_t q = src[i + 3];
      if (q > 255u) return fail(RR_EIO, "level schedule: pivot offset out of range (stale blob)");
      tc[i] = f[0] | (f[1] << 16); tc[i + 1] = f[2] | (f[3] << 16); tc[i + 2] = f[4] | (f[5] << 16);
      tc[i + 3] = q * 8u;
    }
  }
  return dev_alloc(b, t.size() * 4, dst, t.data(), t.size() * 4);
}

static int lds_bytes(const rr_model* m, Variant v) { return v == V_PAIR ? 2 * m->kd_rep.lds_bytes_rep + 128 : m->dims.lds_bytes; }      // of a launch of select(m, form, v)

extern "C" int rr_batch_create(const rr_model* m, int32_t num_envs, int32_t device, void* stream, rr_batch** out) {
  if (!m || !out || num_envs <= 0) return fail(RR_EINVAL, "rr_batch_create: bad argument");
  const Instance prod = select(m, F_STEP, V_PROD);
  if (!prod.kern) return fail(RR_EUNSUPPORTED, std::string("rr_batch_create: ") + prod.why);
  HIPCHK(hipSetDevice(device));
  std::unique_ptr<rr_batch, void (*)(rr_batch*)> guard(new rr_batch(), rr_batch_destroy);      // every early return below destroys the batch
  rr_batch* b = guard.get();
  b->m = m; b->N = num_envs; b->device = device; b->stream = (hipStream_t)stream; b->kd = m->kd;
  int rc = 0;
  // the model's tables; T_rep: those of one replica (blob prefix h_) -- all but the transmission tables, which only DYN instances read
#define UP(T, prefix, field) if ((rc = upload(b, prefix "k_" #field, &T.field))) return rc;
#define UP_REPLICA_TABLES(T, prefix)                                                                                                \
  UP(T, prefix, body_i) UP(T, prefix, jnt_i) UP(T, prefix, dof_i) UP(T, prefix, M_ij_k) UP(T, prefix, body_anc)                     \
  UP(T, prefix, con_chain_rows) UP(T, prefix, coljob) UP(T, prefix, rowjob) UP(T, prefix, jobown) UP(T, prefix, con_i)              \
  UP(T, prefix, body_f) UP(T, prefix, jnt_f) UP(T, prefix, dof_f) UP(T, prefix, act_f) UP(T, prefix, con_f) UP(T, prefix, root_mass)
  UP_REPLICA_TABLES(b->T, "")
  UP(b->T, "", act_i) UP(b->T, "", act_m_i) UP(b->T, "", act_m_f)
  const uint32_t qb = (uint32_t)m->kd.o_qLD * 4u, ab = (uint32_t)m->kd.o_xpos * 4u, nM = (uint32_t)m->dims.nM;
  if ((rc = upload_levels(b, m->solver == 2 ? "k_factor3p" : "k_factor3", &b->T.factor3, qb, ab, nM)) || (rc = upload_levels(b, "k_linv", &b->T.linv, qb, ab, nM))) return rc;
  memset(&b->T_rep, 0, sizeof(b->T_rep));
  if (m->pair_ok) {      // tables of one replica; the level schedules twice (second copy addressed into the second wavefront's region)
    UP_REPLICA_TABLES(b->T_rep, "h_")
    const uint32_t base = (uint32_t)m->kd_rep.o_qLD * 4u, rb = (uint32_t)m->kd_rep.lds_bytes_rep;
    const uint32_t abase = (uint32_t)m->kd_rep.o_xpos * 4u, hnM = (uint32_t)m->kd_rep.nM;
    if ((rc = upload_levels(b, "h_k_factor3", &b->T_rep.factor3, base, abase, hnM, 2, rb)) || (rc = upload_levels(b, "h_k_linv", &b->T_rep.linv, base, abase, hnM, 2, rb))) return rc;
    b->T_rep.anc4 = b->T_rep.M_ij_k;     // unused (Newton only); a valid pointer
  }
#undef UP_REPLICA_TABLES
#undef UP
  {   // ancestor ids along the rows of M (Newton): byte Madr[i] + p = the p-th ancestor of dof i (p = 0: i itself)
    const Entry *an = m->find("dof_anc"), *ad = m->find("dof_ancadr"), *ma = m->find("dof_Madr");
    std::vector<unsigned char> bytes(((size_t)m->dims.nM + 3) / 4 * 4 + 4, 0);
    if (an && ad && ma) {
      const int32_t *anc = (const int32_t*)an->data, *adr = (const int32_t*)ad->data, *madr = (const int32_t*)ma->data;
      for (int i = 0; i < m->dims.nv; ++i) {
        const int n = adr[i + 1] - adr[i];                 // chain root .. self
        for (int p = 0; p < n; ++p) bytes[madr[i] + p] = (unsigned char)anc[adr[i] + n - 1 - p];
      }
    } else if (m->solver == 2) return fail(RR_EIO, "rr_batch_create: blob lacks the ancestor tables the Newton solver needs");
    if ((rc = dev_alloc(b, bytes.size(), &b->T.anc4, bytes.data(), bytes.size()))) return rc;
  }
  if (!m->stage_ok) return fail(RR_EUNSUPPORTED, "rr_batch_create: 4*ncon + nv exceeds the line-search staging cells (6*nbody)");
  if (m->dims.lds_bytes > 64 * 1024) return fail(RR_EUNSUPPORTED, "rr_batch_create: per-env working set exceeds the 64 KiB of LDS one workgroup may address");
  for (int f = 0; f < N_FORMS; ++f)
    for (int v = 0; v < N_VARIANTS; ++v) {      // every instance a launch may pick
      const kern_t kk = select(m, (Form)f, (Variant)v).kern;
      if (!kk) continue;
      HIPCHK(hipFuncSetAttribute((const void*)kk, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes(m, (Variant)v)));
      // the level schedules address LDS by absolute byte address, so the dynamic segment must begin at LDS address 0: no static LDS
      hipFuncAttributes fa;
      HIPCHK(hipFuncGetAttributes(&fa, (const void*)kk));
      if (fa.sharedSizeBytes != 0) return fail(RR_EUNSUPPORTED, "rr_batch_create: a step-kernel instance has static LDS (the level schedules need the dynamic segment at address 0)");
    }
  if (m->dyn && (rc = dev_alloc(b, 64, &b->dyn_overflow))) return rc;
  if (m->dyn) HIPCHK(hipMemset(b->dyn_overflow, 0, 64));
  if ((rc = dev_alloc(b, 64, &b->bad_states))) return rc;
  HIPCHK(hipMemset(b->bad_states, 0, 64));
  const char* pace = getenv("RR_PACE");
  if (!(pace && pace[0] == '0') && (rc = dev_alloc(b, 64, &b->progress))) return rc;
  m->live_batches.fetch_add(1);
  b->counted = true;
  *out = guard.release();
  return RR_OK;
}

extern "C" void rr_batch_destroy(rr_batch* b) {
  if (!b) return;
  if (b->counted) b->m->live_batches.fetch_sub(1);
  for (void* p : b->dev_allocs) (void)hipFree(p);
  for (float* p : {b->env_dof_f, b->env_act_f, b->env_con_f, b->eval_actions}) if (p) (void)hipFree(p);
  for (hipEvent_t e : b->ev0) (void)hipEventDestroy(e);
  for (hipEvent_t e : b->ev1) (void)hipEventDestroy(e);
  delete b;
}

#define RR_TIMING_RING 256
// Fold finished event pairs into the totals.  `all`: wait for every pending launch (rr_batch_kernel_time).  Otherwise (the ring is
// full at a launch) only pairs that HAVE finished are taken, oldest first, without blocking -- a blocking drain stalled the host
// for the length of the launch in flight, long enough with multi-step launches for a second stream to run dry -- and if none has,
// the oldest one is waited for.
static int collect_timing(rr_batch* b, bool all = true) {
  bool first = true;
  while (b->npending > 0) {
    const int i = b->ring_head;
    if (all || (first && hipEventQuery(b->ev1[i]) != hipSuccess)) HIPCHK(hipEventSynchronize(b->ev1[i]));
    else if (hipEventQuery(b->ev1[i]) != hipSuccess) break;
    first = false;
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, b->ev0[i], b->ev1[i]));
    b->total_ms += ms;
    b->launches += 1;
    b->ring_head = (i + 1) % RR_TIMING_RING;
    b->npending -= 1;
  }
  (void)hipGetLastError();      // hipEventQuery reports "not ready" through the sticky last-error slot
  return RR_OK;
}

// One launch of the step kernel as an ABI entry point describes it (fields named at the call: designated initialisers, in this order).
struct Launch {
  int mode = 1;                                     // 0 = forward pass only, 1 = step, 2 = reset
  const rr_state *st = nullptr, *st_in = nullptr;   // the state written; the one read (null: st)
  const float* ctrl = nullptr;
  int n_frames = 1;
  const rr_env_io* env = nullptr;
  const int32_t* cur_frame_in = nullptr;            // null: env->cur_frame is read and written
  const rr_outputs* out = nullptr;
  const rr_unroll_io* un = nullptr;                 // multi-step forms: the wrappers' state, unroll_T steps
  int unroll_T = 0;
  const rr_actor_io* ac = nullptr;                  // ... with the actor
  const rr_eval_io* ev = nullptr;                   // ... as an evaluation
};
static int check_wrap(const char* who, const rr_unroll_io* w, const char* note = "") {
  if (!w || !w->first.qpos || !w->first.qvel || !w->first.act || !w->first.qacc_warmstart || !w->first_obs || !w->prev_done || !w->steps_in ||
      !w->steps_out || !w->truncation_out)
    return fail(RR_EINVAL, std::string(who) + ": null wrapper pointer" + note);
  return RR_OK;
}
// Columns the actor's head is padded to, in the kernel arguments (rr_actor_step) and in LDS (rr_policy_tail_kernel): 64 up to 64 logits,
// 128 above.  A head fits when P <= head_cols(P).
static int head_cols(int P) { return P <= 64 ? 64 : 128; }
// traj: the form that samples and records transitions (noise, actions and the trajectory arrays are required)
static int check_actor(const char* who, const rr_actor_io* a, bool traj) {
  if (!a->obs_in || !a->w0 || !a->b0 || !a->head_wt || !a->head_b || (a->mean == nullptr) != (a->std == nullptr) ||
      (traj && (!a->noise || !a->actions_out || !a->traj_obs || !a->traj_raw_action || !a->traj_log_prob || !a->traj_reward || !a->traj_discount ||
                !a->traj_truncation)))
    return fail(RR_EINVAL, std::string(who) + ": null actor pointer");
  for (int l = 1; l < a->nhidden && l < 5; ++l)
    if (!a->hidden_wt[l - 1] || !a->hidden_b[l - 1]) return fail(RR_EINVAL, std::string(who) + ": null hidden layer");
  return RR_OK;
}
// What the in-kernel actor cannot serve, or null.  ac null: the limits on the model alone (rr_batch_eval_supported).  ref_frames: of the
// batch; the actor of the selected instance reads 64 x JM entries of the row (rr_actor_step: 1280, REFOBS instances 1664).  wide: the
// launch runs a REFOBS instance (V_POSETERM, V_BODY, V_RESTART) whatever ref_frames is
static const char* actor_limit(const rr_model* m, const rr_actor_io* ac, int ref_frames = 0, bool wide = false) {
  static_assert(RR_ACTOR_JM == 20 && RR_ACTOR_JM_REFOBS == 26, "the two texts below name 64 x JM");
  if ((ref_frames > 0 || wide) && m->dims.obs_dim + ref_frames * m->dims.nq > 64 * RR_ACTOR_JM_REFOBS)
    return "rr_env_unroll_policy: observation with its reference frames wider than 1664 (the in-kernel actor of the reference-observation instances reads 26 entries per lane: at most 5 frames on the rodent models)";
  if (!wide && m->dims.obs_dim > 64 * RR_ACTOR_JM) return "rr_env_unroll_policy: observation wider than 1280";
  if (ac && (ac->nhidden < 1 || ac->nhidden > 5)) return "rr_env_unroll_policy: 1 .. 5 hidden layers";
  if (2 * m->dims.nu > head_cols(2 * m->dims.nu)) return "rr_env_unroll_policy: more than 64 actions (the in-kernel actor's head is at most 2 x 64 logits)";
  return nullptr;
}

// launch() step 1: RRIO from the state, the env io and the outputs
static int fill_io(const Launch& L, RRIO& io) {
  const rr_state *st = L.st, *st_in = L.st_in;
  if (!st || !st->qpos || !st->qvel || !st->act || !st->qacc_warmstart) return fail(RR_EINVAL, "launch: null state pointer");
  if (st_in && (!st_in->qpos || !st_in->qvel || !st_in->act || !st_in->qacc_warmstart)) return fail(RR_EINVAL, "launch: null input state pointer");
  if ((L.mode & 1) && ((!L.ctrl && !L.ev) || L.n_frames <= 0)) return fail(RR_EINVAL, "launch: step needs ctrl and n_frames > 0");      // ev: the batch's own action rows
  memset(&io, 0, sizeof(io));
  io.qpos = st->qpos; io.qvel = st->qvel; io.act = st->act; io.warm = st->qacc_warmstart; io.ctrl = L.ctrl;
  const rr_state* si = st_in ? st_in : st;
  io.qpos_in = si->qpos; io.qvel_in = si->qvel; io.act_in = si->act; io.warm_in = si->qacc_warmstart;
  if (const rr_outputs* out = L.out) {
    io.o_cinert = out->cinert; io.o_cvel = out->cvel; io.o_qfrc_actuator = out->qfrc_actuator; io.o_xpos = out->xpos;
    io.o_xmat = out->xmat; io.o_com = out->subtree_com; io.dbg = out->debug;
    io.o_cdist = out->contact_dist; io.o_cpos = out->contact_pos; io.o_cframe = out->contact_frame;
  }
  if (const rr_env_io* env = L.env) {
    if (!env->obs || !env->track_pos || !env->cur_frame || env->track_len <= 0) return fail(RR_EINVAL, "launch: env io needs obs, track_pos, cur_frame");
    if ((L.mode & 1) && (!env->reward || !env->done || !env->metrics)) return fail(RR_EINVAL, "launch: env step needs reward, done, metrics");
    io.track_pos = env->track_pos; io.track_len = env->track_len; io.cur_frame = env->cur_frame; io.obs = env->obs;
    io.cur_frame_in = L.cur_frame_in ? L.cur_frame_in : env->cur_frame;
    io.reward = env->reward; io.done = env->done; io.metrics = env->metrics;
    io.healthy_reward = env->healthy_reward; io.ctrl_cost_weight = env->ctrl_cost_weight; io.z_min = env->healthy_z_min;
    io.z_max = env->healthy_z_max; io.terminate_when_unhealthy = env->terminate_when_unhealthy;
    if (!(env->bad_state_max >= 0.0f)) return fail(RR_EINVAL, "launch: env io bad_state_max must be >= 0 (0 = no bad-state check)");
    io.bad_state_max = env->bad_state_max;
    if (env->clip && env->num_clips < 1) return fail(RR_EINVAL, "launch: env io clip needs num_clips >= 1");
    io.clip = env->clip; io.num_clips = env->num_clips;
  }
  io.mode = L.mode;
  return RR_OK;
}

// launch() step 3: the fields of the multi-step forms -- wrappers' state, actor, evaluation, pacing
// wide: the launch runs V_POSETERM, V_BODY or V_RESTART, whose actor reads the wider row
static int fill_unroll(rr_batch* b, const Launch& L, RRIO& io, bool wide) {
  if (const rr_actor_io* ac = L.ac) {
    if (const char* limit = actor_limit(b->m, ac, io.ref_frames, wide)) return fail(RR_EUNSUPPORTED, limit);
    io.a_obs_in = ac->obs_in; io.a_mean = ac->mean; io.a_std = ac->std; io.a_W0 = ac->w0; io.a_b0 = ac->b0;
    for (int l = 1; l < ac->nhidden; ++l) { io.a_Wt[l - 1] = ac->hidden_wt[l - 1]; io.a_b[l - 1] = ac->hidden_b[l - 1]; }
    io.a_Wth = ac->head_wt; io.a_bh = ac->head_b; io.a_noise = ac->noise; io.a_actions = ac->actions_out; io.ctrl = ac->actions_out;
    io.t_obs = ac->traj_obs; io.t_raw = ac->traj_raw_action; io.t_logp = ac->traj_log_prob; io.t_reward = ac->traj_reward;
    io.t_discount = ac->traj_discount; io.t_trunc = ac->traj_truncation; io.a_min_std = ac->min_std; io.a_nh = ac->nhidden;
    io.a_seg = ac->segment_length > 0 ? ac->segment_length : L.unroll_T;
    if (L.unroll_T % io.a_seg) return fail(RR_EINVAL, "rr_env_unroll_policy: num_steps must be a multiple of segment_length");
    io.obs = ac->traj_obs;
    if (const rr_eval_io* ev = L.ev) {
      io.t_obs = io.obs = ev->obs_ring; io.e_metrics = ev->eval_metrics; io.e_qpos_out = ev->qpos_out; io.a_seg = L.unroll_T;
      io.a_pad = (ev->raw_env ? RR_EVAL_RAW : 0) | (ac->actions_out ? RR_EVAL_ACTIONS : 0);
      if (!ac->actions_out) {
        if (!b->eval_actions) HIPCHK(hipMalloc((void**)&b->eval_actions, (size_t)b->N * b->m->dims.nu * sizeof(float)));
        io.a_actions = b->eval_actions; io.ctrl = b->eval_actions;
      }
    }
  }
  io.first_qpos = L.un->first.qpos; io.first_qvel = L.un->first.qvel; io.first_act = L.un->first.act; io.first_warm = L.un->first.qacc_warmstart;
  io.first_obs = L.un->first_obs; io.prev_done = L.un->prev_done; io.steps_in = L.un->steps_in; io.steps_out = L.un->steps_out;
  io.trunc_out = L.un->truncation_out; io.episode_length = L.un->episode_length; io.unroll_T = L.unroll_T;
  if (b->progress && L.unroll_T > 1) {
    HIPCHK(hipMemsetAsync(b->progress, 0, 4, b->stream));
    io.progress = b->progress;
    static const struct Pace { float t[3]; int mode; } pace = [] {        // RR_PACE_T="t1,t2,t3", RR_PACE_MODE: tuning switches (tools/)
      Pace p = {{0.3f, 0.6f, 1.0f}, 0};
      if (const char* e = getenv("RR_PACE_T")) sscanf(e, "%f,%f,%f", &p.t[0], &p.t[1], &p.t[2]);
      if (const char* e = getenv("RR_PACE_MODE")) p.mode = atoi(e);
      return p;
    }();
    io.pace_t1 = pace.t[0]; io.pace_t2 = pace.t[1]; io.pace_t3 = pace.t[2]; io.pace_mode = pace.mode;
  }
  return RR_OK;
}

static int launch(rr_batch* b, const Launch& L) {
  if (!b) return fail(RR_EINVAL, "launch: null state pointer");
  RRIO io;
  int rc = fill_io(L, io);
  if (rc) return rc;
  HIPCHK(hipSetDevice(b->device));
  // step 2: the instance that serves the launch on this batch, or the refusal
  const rr_model* m = b->m;
  const bool geom = io.o_cdist || io.o_cpos || io.o_cframe, params = b->has_env_params();
  // per-env parameters: the RAND instance of the same launch form; production instances only (a batch takes them only where those exist)
  if (params && io.dbg) return fail(RR_EUNSUPPORTED, "launch: no debug dump on a batch with per-env parameters (the debug instance reads the model's shared tables)");
  if (params && geom) return fail(RR_EUNSUPPORTED, "launch: no contact-geometry outputs on a batch with per-env parameters (they are served by the debug instance)");
  if (params && b->prof) return fail(RR_EUNSUPPORTED, "launch: no profile build on a batch with per-env parameters");
  // pose tracking (rr_batch_set_pose): an env step's reward terms -- a reset has no reward and ignores the block -- served by the POSE
  // instance of the same launch form; shared tables, production instances only.  The options on top of the block:
  //   reference frames (rr_batch_set_reference_obs): env steps AND resets write the blocks, and every row is obs_width() wide;
  //   pose termination (rr_batch_set_pose_termination), body tracking (rr_batch_set_body_tracking) and velocity tracking
  //   (rr_batch_set_velocity_tracking): env steps only -- a reset has neither done nor reward and stays on the variant it uses without them;
  //   clip restarts (rr_batch_set_clip_restarts): the multi-step launches of the training wrappers only -- single steps have no restore
  //   in the kernel, the evaluation form none from a bank.
  // Any of the first four selects V_BODY, clip restarts V_RESTART (rr_kernel.h rr_body_kernel: one instance for every combination);
  // an env step with a termination block and neither a body nor a velocity block runs V_POSETERM, the same computation without the
  // `if (BODY)` code.  An option the batch does not carry reaches the kernel as zero frames, thresholds that no error exceeds with a
  // null pose_fail, a null track_bodies, a null track_vel.  The clip library (rr_batch_set_clip_library) counts as an option of the env
  // steps too: only the BODY instances read clip_len, bank_clips and clip_out, so such a batch never runs V_POSE or V_POSETERM.  The
  // lengths also go to the resets that run V_BODY (reference frames); the other resets stay on their variant and read none
  const bool pose_step = b->pose.track_pose && L.env && L.mode == 1;
  const bool refobs = b->ref_frames > 0 && b->pose.track_pose && L.env;
  const bool pose = pose_step || refobs;
  const bool pterm = b->pterm.fail && pose_step, body = b->body.track_bodies && pose_step, restart = b->restart.frames && pose_step && L.un && !L.ev;
  const bool vel = b->vel.track_vel && pose_step;
  const bool library = b->has_clip_library() && pose_step;
  const bool options = refobs || pterm || body || restart || vel || library;
  if (options) io.pose_max_pos = io.pose_max_quat = io.pose_max_joint = INFINITY;
  if (refobs) io.ref_frames = b->ref_frames;
  if (restart) {
    io.restart_frames = b->restart.frames; io.restart_slot_in = b->restart.slot_in; io.restart_slot_out = b->restart.slot_out;
    io.restart_K = b->restart.num_slots; io.restart_end = b->restart.end_at_clip_end ? 1 : 0;
  }
  if (body) {
    io.track_bodies = b->body.track_bodies; io.body_weights = b->body.body_weights; io.body_metrics = b->body.body_metrics;
    io.body_w = b->body.body_reward_weight; io.body_k = b->body.body_reward_scale; io.endeff_w = b->body.endeff_reward_weight; io.endeff_k = b->body.endeff_reward_scale;
  }
  if (vel) {
    io.track_vel = b->vel.track_vel; io.vel_metrics = b->vel.vel_metrics;
    io.vel_lin_w = b->vel.lin_weight; io.vel_lin_k = b->vel.lin_scale; io.vel_ang_w = b->vel.ang_weight; io.vel_ang_k = b->vel.ang_scale;
    io.vel_joint_w = b->vel.joint_weight; io.vel_joint_k = b->vel.joint_scale;
  }
  if (b->has_clip_library() && (pose_step || refobs)) io.clip_len = b->lib.clip_lengths;
  if (library && restart && b->lib.bank_clips) {
    if (!io.clip) return fail(RR_EINVAL, "launch: clip library: bank_clips needs the env io's clip ids");
    if (io.clip == b->lib.clip_out) return fail(RR_EINVAL, "launch: clip library: clip_out may not alias the env io's clip");
    io.bank_clips = b->lib.bank_clips; io.clip_out = b->lib.clip_out;
  }
  if (restart && b->has_clip_sampling()) {      // only the RESTART instances read these; single steps ignore the block (rr_wrap_clip_sampling)
    io.outcomes = (long long*)b->samp.outcomes; io.sample_seed = b->samp.seed;
    if (b->samp.clip_weights) {
      if (!io.bank_clips) return fail(RR_EINVAL, "launch: clip sampling: clip_weights needs the clip library's bank_clips");
      io.clip_weights = b->samp.clip_weights;
    }
    io.draws_in = b->samp.draws_in; io.draws_out = b->samp.draws_out;
    if (io.draws_in && io.draws_in == io.draws_out) return fail(RR_EINVAL, "launch: clip sampling: draws_out may not alias draws_in");
  }
  if (restart && b->refr.draws_in) {      // only the RESTART instances read these; single steps ignore the block
    if (b->refr.across_clips && io.clip && !io.clip_out) return fail(RR_EINVAL, "launch: reference restarts: across_clips needs the clip library's bank_clips and clip_out (the clip an env moves to goes out there)");
    if (io.clip && io.num_clips > 65536) return fail(RR_EINVAL, "launch: reference restarts: num_clips must be <= 65536 (the weights' sum stays within 32 bits)");
    io.rref_on = 1; io.rref_seed = b->refr.seed; io.rref_lo = b->refr.frame_lo; io.rref_hi = b->refr.frame_hi;
    io.rref_across = b->refr.across_clips ? 1 : 0; io.rref_noise = b->refr.noise_scale;
    io.clip_weights = b->refr.clip_weights; io.draws_in = b->refr.draws_in; io.draws_out = b->refr.draws_out;
  }
  if (pterm) { io.pose_fail = b->pterm.fail; io.pose_max_pos = b->pterm.max_pos; io.pose_max_quat = b->pterm.max_quat; io.pose_max_joint = b->pterm.max_joint; }
  if (pose) {
    io.track_pose = b->pose.track_pose; io.pose_metrics = b->pose.pose_metrics;
    io.pose_quat_w = b->pose.quat_reward_weight; io.pose_quat_k = b->pose.quat_reward_scale;
    io.pose_joint_w = b->pose.joint_reward_weight; io.pose_joint_k = b->pose.joint_reward_scale;
  }
  if (pose && params) return fail(RR_EUNSUPPORTED, "launch: pose tracking: no pose instance reads per-env parameters (this batch carries some)");
  if (pose && (io.dbg || geom || b->prof)) return fail(RR_EUNSUPPORTED, "launch: pose tracking: no debug dump, contact-geometry outputs or profile build with track_pose (diagnostic instances have no pose form)");
  Variant v = b->prof ? V_PROFILE : ((io.dbg || geom) ? V_DEBUG : (params ? V_RAND : (restart ? V_RESTART : (pterm && !body && !vel && !library ? V_POSETERM : (options ? V_BODY : (pose ? V_POSE : V_PROD))))));
  // two-tree model, physics only, no diagnostics: one wavefront per replica (rr_kernel.h PAIR)
  const bool pair = m->pair_ok && v == V_PROD && !L.env && !L.out && !L.un && !b->env_map && !b->cost && m->solver != 2;
  if (pair) v = V_PAIR;
  if (b->solve_lds) {      // rr_batch_set_solve_resident(b, 0): production launches only, and select() refuses the multi-step forms
    if (v != V_PROD) return fail(RR_EUNSUPPORTED, "launch: rr_batch_set_solve_resident(b, 0) serves production launches only (no debug dump, contact-geometry outputs, profile build, per-env parameters or pose tracking on this batch)");
    v = V_MATLDS;
  }
  if (b->plain_slots) {      // rr_batch_set_root_slot(b, 0): production launches only, and select() refuses the multi-step forms
    if (b->solve_lds) return fail(RR_EUNSUPPORTED, "launch: rr_batch_set_root_slot(b, 0) and rr_batch_set_solve_resident(b, 0) select different comparison instances; one of the two per batch");
    if (v != V_PROD) return fail(RR_EUNSUPPORTED, "launch: rr_batch_set_root_slot(b, 0) serves production launches only (no debug dump, contact-geometry outputs, profile build, per-env parameters or pose tracking on this batch)");
    v = V_TWOSLOT;
  }
  const Instance in = select(m, L.ev ? F_EVAL : (L.ac ? F_ACTOR : (L.un ? F_UNROLL : F_STEP)), v, b);
  if (!in.kern) return fail(RR_EUNSUPPORTED, std::string(L.un ? "" : "launch: ") + in.why);
  if (L.un && (rc = fill_unroll(b, L, io, options))) return rc;
  io.env_dof_f = b->env_dof_f; io.env_act_f = b->env_act_f; io.env_con_f = b->env_con_f;      // null without per-env parameters
  io.prof = b->prof; io.env_map = b->env_map; io.cost = b->cost; io.dyn_overflow = b->dyn_overflow; io.bad_states = b->bad_states;
  if (v == V_DEBUG) io.dbg_flags = b->dbg_flags;      // the only instance that reads it
  // step 4: the launch itself, between the event pair of the timing ring
  RRDims kd = pair ? m->kd_rep : b->kd;
  kd.iterations = m->kd.iterations; kd.ls_iterations = m->kd.ls_iterations;
  if (b->timing) {
    if (b->npending == RR_TIMING_RING && (rc = collect_timing(b, false))) return rc;
    HIPCHK(hipEventRecord(b->ev0[(b->ring_head + b->npending) % RR_TIMING_RING], b->stream));
  }
  hipLaunchKernelGGL(in.kern, dim3(b->N), dim3((pair ? 2 : 1) * RR_LANES), (size_t)lds_bytes(m, v), b->stream, kd, pair ? b->T_rep : b->T, io, b->N, L.n_frames);
  HIPCHK(hipGetLastError());
  if (b->timing) {
    HIPCHK(hipEventRecord(b->ev1[(b->ring_head + b->npending) % RR_TIMING_RING], b->stream));
    b->npending += 1;
  }
  return RR_OK;
}

extern "C" int rr_pipeline_step_to(rr_batch* b, const rr_state* in, const rr_state* outst, const float* ctrl, int32_t n_frames, const rr_outputs* out) {
  if (!in) return fail(RR_EINVAL, "rr_pipeline_step_to: null input state");
  return launch(b, {.st = outst, .st_in = in, .ctrl = ctrl, .n_frames = n_frames, .out = out});
}
extern "C" int rr_env_step_to(rr_batch* b, const rr_state* in, const rr_state* outst, const float* action, int32_t n_frames, const rr_env_io* env,
                              const int32_t* cur_frame_in, const rr_outputs* out) {
  if (!env) return fail(RR_EINVAL, "rr_env_step_to: env io required");
  if (!in || !cur_frame_in) return fail(RR_EINVAL, "rr_env_step_to: null input state");
  return launch(b, {.st = outst, .st_in = in, .ctrl = action, .n_frames = n_frames, .env = env, .cur_frame_in = cur_frame_in, .out = out});
}
extern "C" int rr_batch_contact_overflow(rr_batch* b, int64_t* events) {
  if (!b || !events) return fail(RR_EINVAL, "rr_batch_contact_overflow: null argument");
  *events = 0;
  if (!b->dyn_overflow) return RR_OK;                // static-slot models hold every contact of the model: nothing can overflow
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipStreamSynchronize(b->stream));
  unsigned v = 0;
  HIPCHK(hipMemcpy(&v, b->dyn_overflow, sizeof(v), hipMemcpyDeviceToHost));
  *events = (int64_t)v;
  return RR_OK;
}
extern "C" int rr_batch_bad_states(rr_batch* b, int64_t* events) {
  if (!b || !events) return fail(RR_EINVAL, "rr_batch_bad_states: null argument");
  *events = 0;
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipStreamSynchronize(b->stream));
  unsigned v = 0;
  HIPCHK(hipMemcpy(&v, b->bad_states, sizeof(v), hipMemcpyDeviceToHost));
  *events = (int64_t)v;
  return RR_OK;
}
extern "C" int rr_batch_unroll_supported(const rr_batch* b, int32_t with_actor) {
  if (!b) return fail(RR_EINVAL, "rr_batch_unroll_supported: null batch");
  return select(b->m, with_actor ? F_ACTOR : F_UNROLL, V_PROD).kern ? 1 : 0;
}
extern "C" int rr_env_unroll(rr_batch* b, const rr_state* in, const rr_state* outst, const float* actions, int32_t num_steps, int32_t n_frames,
                             const rr_env_io* env, const int32_t* cur_frame_in, const rr_unroll_io* wrap) {
  if (!env || !in || !cur_frame_in || !wrap || !actions || num_steps <= 0) return fail(RR_EINVAL, "rr_env_unroll: bad argument");
  if (int rc = check_wrap("rr_env_unroll", wrap)) return rc;
  return launch(b, {.st = outst, .st_in = in, .ctrl = actions, .n_frames = n_frames, .env = env, .cur_frame_in = cur_frame_in, .un = wrap, .unroll_T = num_steps});
}
extern "C" int rr_env_unroll_policy(rr_batch* b, const rr_state* in, const rr_state* outst, int32_t num_steps, int32_t n_frames, const rr_env_io* env,
                                    const int32_t* cur_frame_in, const rr_unroll_io* wrap, const rr_actor_io* actor) {
  if (!env || !in || !cur_frame_in || !wrap || !actor || num_steps <= 0) return fail(RR_EINVAL, "rr_env_unroll_policy: bad argument");
  int rc = check_wrap("rr_env_unroll_policy", wrap);
  if (rc || (rc = check_actor("rr_env_unroll_policy", actor, true))) return rc;
  rr_env_io e = *env;
  e.obs = actor->traj_obs;                   // the observations of the launch go to the trajectory
  return launch(b, {.st = outst, .st_in = in, .ctrl = actor->actions_out, .n_frames = n_frames, .env = &e, .cur_frame_in = cur_frame_in, .un = wrap,
                    .unroll_T = num_steps, .ac = actor});
}
extern "C" int rr_batch_eval_supported(const rr_batch* b) {
  if (!b) return fail(RR_EINVAL, "rr_batch_eval_supported: null batch");
  const bool options = b->ref_frames > 0 || b->pterm.fail || b->body.track_bodies || b->restart.frames || b->vel.track_vel || b->has_clip_library();      // of the pose family: none has an evaluation instance
  const Variant v = b->prof ? V_PROFILE : (b->has_env_params() ? V_RAND : (options ? V_BODY : V_PROD));
  return (select(b->m, F_EVAL, v, b).kern && !actor_limit(b->m, nullptr)) ? 1 : 0;
}
extern "C" int rr_env_unroll_eval(rr_batch* b, const rr_state* in, const rr_state* outst, int32_t num_steps, int32_t n_frames, const rr_env_io* env,
                                  const int32_t* cur_frame_in, const rr_unroll_io* wrap, const rr_actor_io* actor, const rr_eval_io* ev) {
  if (!env || !in || !cur_frame_in || !actor || !ev || num_steps <= 0) return fail(RR_EINVAL, "rr_env_unroll_eval: bad argument");
  if (!ev->obs_ring) return fail(RR_EINVAL, "rr_env_unroll_eval: null observation ring");
  int rc = ev->raw_env ? RR_OK : check_wrap("rr_env_unroll_eval", wrap, " (only the raw form runs without the wrappers' state)");
  if (rc || (rc = check_actor("rr_env_unroll_eval", actor, false))) return rc;
  rr_unroll_io none;
  memset(&none, 0, sizeof(none));
  rr_env_io e = *env;
  e.obs = ev->obs_ring;                      // the observations of the launch live in the ring
  return launch(b, {.st = outst, .st_in = in, .ctrl = actor->actions_out, .n_frames = n_frames, .env = &e, .cur_frame_in = cur_frame_in,
                    .un = ev->raw_env ? &none : wrap, .unroll_T = num_steps, .ac = actor, .ev = ev});
}
extern "C" int rr_pipeline_init(rr_batch* b, const rr_state* st, const rr_outputs* out) { return launch(b, {.mode = 0, .st = st, .out = out}); }
extern "C" int rr_pipeline_step(rr_batch* b, const rr_state* st, const float* ctrl, int32_t n_frames, const rr_outputs* out) {
  return launch(b, {.st = st, .ctrl = ctrl, .n_frames = n_frames, .out = out});
}
extern "C" int rr_env_step(rr_batch* b, const rr_state* st, const float* action, int32_t n_frames, const rr_env_io* env, const rr_outputs* out) {
  if (!env) return fail(RR_EINVAL, "rr_env_step: env io required");
  return launch(b, {.st = st, .ctrl = action, .n_frames = n_frames, .env = env, .out = out});
}
extern "C" int rr_env_reset(rr_batch* b, const rr_state* st, const rr_env_io* env, const rr_outputs* out) {
  if (!env) return fail(RR_EINVAL, "rr_env_reset: env io required");
  return launch(b, {.mode = 2, .st = st, .env = env, .out = out});
}

// ------------------------------------------------------------------------------------------ PPO: GAE
__global__ void rr_gae_kernel(const float* __restrict__ trunc, const float* __restrict__ term, const float* __restrict__ rew,
                              const float* __restrict__ val, const float* __restrict__ boot, int T, int B, float lam, float disc,
                              float* __restrict__ vs, float* __restrict__ adv) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float acc = 0.0f;
  const float vb = boot[b];
  for (int t = T - 1; t >= 0; --t) {     // vs_t - v_t = delta_t + gamma (1-term_t)(1-trunc_t) lambda (vs_{t+1} - v_{t+1})
    const size_t i = (size_t)t * B + b;
    const float mask = 1.0f - trunc[i], nt = 1.0f - term[i];
    const float vnext = t == T - 1 ? vb : val[i + B];
    const float delta = (rew[i] + disc * nt * vnext - val[i]) * mask;
    acc = delta + disc * nt * mask * lam * acc;
    vs[i] = acc + val[i];
  }
  for (int t = 0; t < T; ++t) {          // advantages use vs_{t+1} (bootstrap at the end)
    const size_t i = (size_t)t * B + b;
    const float vsn = t == T - 1 ? vb : vs[i + B];
    adv[i] = (rew[i] + disc * (1.0f - term[i]) * vsn - val[i]) * (1.0f - trunc[i]);
  }
}

extern "C" int rr_compute_gae(const float* truncation, const float* termination, const float* rewards, const float* values,
                              const float* bootstrap_value, int32_t T, int32_t B, float lambda_, float discount, float* vs,
                              float* advantages, void* stream) {
  if (!truncation || !termination || !rewards || !values || !bootstrap_value || !vs || !advantages || T <= 0 || B <= 0)
    return fail(RR_EINVAL, "rr_compute_gae: bad argument");
  hipLaunchKernelGGL(rr_gae_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, truncation, termination, rewards,
                     values, bootstrap_value, T, B, lambda_, discount, vs, advantages);
  HIPCHK(hipGetLastError());
  return RR_OK;
}

// ------------------------------------------------------------------------------------------ PPO: loss + gradient w.r.t. the network outputs
static void ppo_blocks(int T, int B, int* nblk1, int* nblk2) {
  *nblk1 = (B + 255) / 256;
  const long n = (long)T * B;
  *nblk2 = (int)std::min<long>((n + 7) / 8, 1024);
}
extern "C" size_t rr_ppo_loss_workspace_bytes(int32_t T, int32_t B) {
  if (T <= 0 || B <= 0) return 0;
  int n1, n2;
  ppo_blocks(T, B, &n1, &n2);
  return rr_align_up((size_t)2 * T * B * sizeof(float), 8) + ((size_t)2 * n1 + (size_t)3 * n2) * sizeof(double);
}
extern "C" size_t rr_ppo_loss_diag_workspace_bytes(int32_t T, int32_t B) {
  if (T <= 0 || B <= 0) return 0;
  int n1, n2;
  ppo_blocks(T, B, &n1, &n2);
  return rr_ppo_loss_workspace_bytes(T, B) + (size_t)5 * n2 * sizeof(double);
}
// diag != NULL: the DIAG instances of the loss and metrics kernels (rr_ppo_loss_diag)
static int ppo_loss_launch(const float* policy_logits, const float* values, const float* raw_action, const float* log_prob, const float* reward,
                           const float* discount, const float* truncation, const int64_t* idx, const float* noise, int32_t T, int32_t B, int32_t A,
                           const rr_ppo_cfg* cfg, float* grad_logits, float* grad_values, float* metrics, double* diag, float* kl_out,
                           void* workspace, size_t workspace_bytes, void* stream) {
  const std::string who = diag ? "rr_ppo_loss_diag" : "rr_ppo_loss";                         // the entry the caller used, for its error text
  if (!policy_logits || !values || !raw_action || !log_prob || !reward || !discount || !truncation || !noise || !cfg || !grad_logits ||
      !grad_values || !metrics || !workspace || T <= 0 || B <= 0 || A <= 0)
    return fail(RR_EINVAL, who + ": bad argument");
  if (workspace_bytes < (diag ? rr_ppo_loss_diag_workspace_bytes(T, B) : rr_ppo_loss_workspace_bytes(T, B)) || ((uintptr_t)workspace & 7))
    return fail(RR_EINVAL, who + ": workspace too small (rr_ppo_loss_workspace_bytes / rr_ppo_loss_diag_workspace_bytes) or not 8-byte aligned");
  if (diag && (((uintptr_t)diag & 7) || ((uintptr_t)kl_out & 3)))
    return fail(RR_EINVAL, "rr_ppo_loss_diag: diag must be 8-byte aligned, kl_out 4-byte aligned");
  RRPpoArgs P;
  memset(&P, 0, sizeof(P));
  P.logits = policy_logits; P.values = values; P.raw_action = raw_action; P.log_prob = log_prob; P.reward = reward; P.discount = discount;
  P.truncation = truncation; P.idx = idx; P.noise = noise; P.T = T; P.B = B; P.A = A;
  P.entropy_cost = cfg->entropy_cost; P.discounting = cfg->discounting; P.reward_scaling = cfg->reward_scaling; P.gae_lambda = cfg->gae_lambda;
  P.clipping_epsilon = cfg->clipping_epsilon; P.min_std = cfg->min_std; P.normalize_advantage = cfg->normalize_advantage;
  P.grad_logits = grad_logits; P.grad_values = grad_values; P.metrics = metrics;
  ppo_blocks(T, B, &P.nblk1, &P.nblk2);
  char* w = (char*)workspace;
  P.vs = (float*)w; P.adv = P.vs + (size_t)T * B;
  P.part_adv = (double*)(w + rr_align_up((size_t)2 * T * B * sizeof(float), 8));
  P.part_loss = P.part_adv + 2 * P.nblk1;
  if (diag) { P.part_diag = P.part_loss + 3 * P.nblk2; P.diag = diag; P.kl_out = kl_out; }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(rr_ppo_gae_kernel, dim3(P.nblk1), dim3(256), 0, st, P);
  if (diag) {
    hipLaunchKernelGGL(rr_ppo_loss_kernel<true>, dim3(P.nblk2), dim3(256), 0, st, P);
    hipLaunchKernelGGL(rr_ppo_metrics_kernel<true>, dim3(1), dim3(64), 0, st, P);
  } else {
    hipLaunchKernelGGL(rr_ppo_loss_kernel<false>, dim3(P.nblk2), dim3(256), 0, st, P);
    hipLaunchKernelGGL(rr_ppo_metrics_kernel<false>, dim3(1), dim3(64), 0, st, P);
  }
  HIPCHK(hipGetLastError());
  return RR_OK;
}
extern "C" int rr_ppo_loss(const float* policy_logits, const float* values, const float* raw_action, const float* log_prob, const float* reward,
                           const float* discount, const float* truncation, const int64_t* idx, const float* noise, int32_t T, int32_t B, int32_t A,
                           const rr_ppo_cfg* cfg, float* grad_logits, float* grad_values, float* metrics, void* workspace, size_t workspace_bytes,
                           void* stream) {
  return ppo_loss_launch(policy_logits, values, raw_action, log_prob, reward, discount, truncation, idx, noise, T, B, A, cfg, grad_logits,
                         grad_values, metrics, nullptr, nullptr, workspace, workspace_bytes, stream);
}
extern "C" int rr_ppo_loss_diag(const float* policy_logits, const float* values, const float* raw_action, const float* log_prob,
                                const float* reward, const float* discount, const float* truncation, const int64_t* idx, const float* noise,
                                int32_t T, int32_t B, int32_t A, const rr_ppo_cfg* cfg, float* grad_logits, float* grad_values, float* metrics,
                                double* diag, float* kl_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!diag) return fail(RR_EINVAL, "rr_ppo_loss_diag: diag is NULL");
  return ppo_loss_launch(policy_logits, values, raw_action, log_prob, reward, discount, truncation, idx, noise, T, B, A, cfg, grad_logits,
                         grad_values, metrics, diag, kl_out, workspace, workspace_bytes, stream);
}

extern "C" int rr_policy_sample(const float* logits, const float* noise, int32_t N, int32_t A, float min_std, float* action, float* raw_action,
                                float* log_prob, void* stream) {
  if (!logits || !noise || !action || !raw_action || !log_prob || N <= 0 || A <= 0) return fail(RR_EINVAL, "rr_policy_sample: bad argument");
  hipLaunchKernelGGL(rr_policy_sample_kernel, dim3((N + 7) / 8), dim3(256), 0, (hipStream_t)stream, logits, noise, N, A, min_std, action,
                     raw_action, log_prob);
  HIPCHK(hipGetLastError());
  return RR_OK;
}

// policy network backward: the delta chain of the 32-wide stack in one launch (csrc/rr_ppo.h)
static int pol_bwd_blocks(int M) { return std::max(1, std::min(1024, (M + 7) / 8)); }     // latency-bound per row: many small blocks (256 blocks: 76 us, 1024: 35 us)
extern "C" size_t rr_policy_backward_workspace_bytes(int32_t M, int32_t nhidden) {
  if (M <= 0 || nhidden <= 0) return 0;
  return (size_t)nhidden * pol_bwd_blocks(M) * 32 * sizeof(float);
}
extern "C" int rr_policy_backward(const float* grad_logits, const float* head_weight, const float* const* hidden_weights, int32_t nhidden, int32_t M,
                                  int32_t P, float* pre_act, int32_t pre_act_rows, float* delta, float* const* bias_grads, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  if (!grad_logits || !head_weight || !hidden_weights || !pre_act || !delta || !bias_grads || !workspace || M <= 0 || pre_act_rows < M)
    return fail(RR_EINVAL, "rr_policy_backward: bad argument");
  if (nhidden < 1 || nhidden > RR_POL_MAXL) return fail(RR_EUNSUPPORTED, "rr_policy_backward: 1 .. 8 hidden layers");
  if (P < 1 || P > 128) return fail(RR_EUNSUPPORTED, "rr_policy_backward: a head of " + std::to_string(P) + " logits (1 .. 128 are supported)");
  if (workspace_bytes < rr_policy_backward_workspace_bytes(M, nhidden)) return fail(RR_EINVAL, "rr_policy_backward: workspace too small");
  RRPolBwdArgs A;
  memset(&A, 0, sizeof(A));
  A.g = grad_logits; A.w_head = head_weight; A.z = pre_act; A.delta = delta; A.part = (float*)workspace; A.M = M; A.P = P; A.nh = nhidden; A.zrows = pre_act_rows;
  A.nblk = pol_bwd_blocks(M);
  for (int j = 0; j < nhidden; ++j) {
    if (!bias_grads[j] || (j > 0 && !hidden_weights[j])) return fail(RR_EINVAL, "rr_policy_backward: null layer pointer");
    A.bgrad[j] = bias_grads[j];
    A.W[j] = j > 0 ? hidden_weights[j] : nullptr;
  }
  const size_t lds = ((size_t)P * 32 + (size_t)(nhidden - 1) * 1024) * sizeof(float);      // head [P][32] (16 KB at P = 128) + hidden layers
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(rr_policy_backward_kernel, dim3(A.nblk), dim3(256), lds, st, A);
  hipLaunchKernelGGL(rr_policy_colsum_kernel, dim3(nhidden), dim3(1024), 0, st, A);
  HIPCHK(hipGetLastError());
  return RR_OK;
}

// elementwise half of a hidden SiLU layer's backward (csrc/rr_ppo.h)
static int silu_bwd_blocks(int M, int* rows_per_block) {
  const int target = 512;                                   // blocks: two per CU
  *rows_per_block = std::max(8, (M + target - 1) / target);
  return (M + *rows_per_block - 1) / *rows_per_block;
}
extern "C" size_t rr_mlp_silu_backward_workspace_bytes(int32_t M, int32_t H) {
  if (M <= 0 || H <= 0) return 0;
  int rpb;
  return (size_t)silu_bwd_blocks(M, &rpb) * H * sizeof(float);
}
extern "C" int rr_mlp_silu_backward(const float* g, const float* z, int32_t M, int32_t H, float* delta, float* h, float* bias_grad,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  if (!g || !z || !delta || !h || !bias_grad || !workspace || M <= 0 || H <= 0) return fail(RR_EINVAL, "rr_mlp_silu_backward: bad argument");
  if (H > 256 || 256 % H) return fail(RR_EUNSUPPORTED, "rr_mlp_silu_backward: the layer width must divide 256");
  if (workspace_bytes < rr_mlp_silu_backward_workspace_bytes(M, H)) return fail(RR_EINVAL, "rr_mlp_silu_backward: workspace too small");
  int rpb;
  const int nblk = silu_bwd_blocks(M, &rpb);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(rr_silu_bwd_kernel, dim3(nblk), dim3(256), 0, st, g, z, M, H, rpb, delta, h, (float*)workspace);
  hipLaunchKernelGGL(rr_colsum_kernel, dim3((H + 15) / 16), dim3(256), 0, st, (const float*)workspace, nblk, H, bias_grad);
  HIPCHK(hipGetLastError());
  return RR_OK;
}

// ------------------------------------------------------------------------------------------ PPO: fused MLP forward (MFMA f32)
// A launch with `bytes` of dynamic LDS needs the kernel's limit raised first.  The attribute belongs to the (kernel, device) pair, so
// that is what is remembered (rr_batch_create does the same for the step-kernel instances of its batch's device).
static int dyn_lds(const void* kernel, size_t bytes) {
  static std::mutex mu;
  static std::map<std::pair<const void*, int>, size_t> set_to;
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  size_t& have = set_to[{kernel, dev}];
  if (have < bytes) {
    HIPCHK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    have = bytes;
  }
  return RR_OK;
}
static int mlp_net(const rr_mlp_net* n, int K, int hidden, bool is_value, RRMlpNet* out, const char* who, const char* fn = "rr_mlp_forward",
                   const char* widths = nullptr) {
  memset(out, 0, sizeof(*out));
  if (!n) return RR_OK;
  if (!n->weights || !n->biases || !n->sizes || n->nlayers < 2 || n->nlayers > RR_MLP_MAXL) return fail(RR_EINVAL, std::string(fn) + ": bad " + who + " network description");
  if (n->sizes[0] != K) return fail(RR_EINVAL, std::string(fn) + ": " + who + " input width differs from the observation width");
  for (int l = 1; l < n->nlayers; ++l)
    if (n->sizes[l] != hidden) return fail(RR_EUNSUPPORTED, std::string(fn) + ": " + who + " hidden width must be " + (widths ? std::string(widths) : std::to_string(hidden)));
  const int od = n->sizes[n->nlayers];
  if (is_value ? od != 1 : (od < 1 || od > 128))
    return fail(RR_EUNSUPPORTED, std::string(fn) + ": unsupported " + who + " output width " + std::to_string(od) + (is_value ? " (the value head is 1 wide)" : " (1 .. 128 logits are supported)"));
  for (int l = 0; l < n->nlayers; ++l) {
    if (!n->weights[l] || !n->biases[l]) return fail(RR_EINVAL, std::string(fn) + ": null " + who + " parameter");
    out->W[l] = n->weights[l]; out->b[l] = n->biases[l];
  }
  out->nlayers = n->nlayers; out->out_dim = od;
  return RR_OK;
}

extern "C" int rr_mlp_forward(const float* obs, const int64_t* obs_rows, int32_t M, int32_t K, const float* mean, const float* std_, const rr_mlp_net* policy,
                              const rr_mlp_net* value, float* policy_out, float* value_out, float* policy_pre, float* value_pre, void* stream) {
  if (!obs || M <= 0 || K <= 0 || (!policy && !value)) return fail(RR_EINVAL, "rr_mlp_forward: bad argument");
  if ((mean == nullptr) != (std_ == nullptr)) return fail(RR_EINVAL, "rr_mlp_forward: mean and std must be given together");
  if ((policy && !policy_out) || (value && !value_out)) return fail(RR_EINVAL, "rr_mlp_forward: missing output buffer");
  RRMlpArgs A;
  memset(&A, 0, sizeof(A));
  int rc;
  // a policy whose first hidden layer is 256 wide is held to 256 in every hidden layer and runs as a launch of its own
  // (rr_mlp_policy256_forward_kernel) next to the value network's; any other policy is held to 32 and shares the value network's launch
  const bool wide = policy && policy->sizes && policy->nlayers >= 2 && policy->sizes[1] == RR_MLP_VH;
  if ((rc = mlp_net(policy, K, wide ? RR_MLP_VH : RR_MLP_PH, false, &A.pol, "policy", "rr_mlp_forward", "32 or 256, the same in every hidden layer")) ||
      (rc = mlp_net(value, K, RR_MLP_VH, true, &A.val, "value"))) return rc;
  A.obs = obs; A.rows = obs_rows; A.M = M; A.K = K; A.mean = mean; A.std_ = std_;
  A.pol_out = policy_out; A.val_out = value_out; A.pol_act = policy ? policy_pre : nullptr; A.val_act = value ? value_pre : nullptr;
  const size_t lds = RR_MLP_LDS_FLOATS * sizeof(float);
  if (wide) {
    RRMlpArgs W = A;
    memset(&W.val, 0, sizeof(W.val));
    W.val_out = W.val_act = nullptr;
    if ((rc = dyn_lds((const void*)rr_mlp_policy256_forward_kernel, lds))) return rc;
    hipLaunchKernelGGL(rr_mlp_policy256_forward_kernel, dim3((M + RR_MLP_BM - 1) / RR_MLP_BM), dim3(256), lds, (hipStream_t)stream, W);
    HIPCHK(hipGetLastError());
    if (!value) return RR_OK;
    memset(&A.pol, 0, sizeof(A.pol));           // the value network: the launch a value-only call makes
    A.pol_out = A.pol_act = nullptr;
    policy = nullptr;
  }
  typedef void (*fwd_t)(const RRMlpArgs);
  const fwd_t kern = policy && value ? (fwd_t)rr_mlp_forward_kernel<true, true> : (value ? (fwd_t)rr_mlp_forward_kernel<true, false> : (fwd_t)rr_mlp_forward_kernel<false, true>);
  if ((rc = dyn_lds((const void*)kern, lds))) return rc;
  // diagnostic (RR_MLP_PROF=<file>, eager calls only): shader-clock stamps per phase and workgroup, summarised into the file after every call
  static const char* prof_path = getenv("RR_MLP_PROF");
  static unsigned long long* prof_dev = nullptr;
  const int nwg = (M + RR_MLP_BM - 1) / RR_MLP_BM;
  if (prof_path && nwg <= 4096) {
    if (!prof_dev) HIPCHK(hipMalloc((void**)&prof_dev, 4096 * 16 * sizeof(unsigned long long)));
    HIPCHK(hipMemsetAsync(prof_dev, 0, (size_t)nwg * 16 * sizeof(unsigned long long), (hipStream_t)stream));
    A.prof = prof_dev;
  }
  hipLaunchKernelGGL(kern, dim3(nwg), dim3(256), lds, (hipStream_t)stream, A);
  HIPCHK(hipGetLastError());
  if (A.prof) {
    std::vector<unsigned long long> h((size_t)nwg * 16);
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    HIPCHK(hipMemcpy(h.data(), prof_dev, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (FILE* f = fopen(prof_path, "a")) {
      unsigned long long t0 = ~0ull, t1 = 0;
      double sum[16] = {0};
      for (int w = 0; w < nwg; ++w) {
        t0 = std::min(t0, h[(size_t)w * 16]); t1 = std::max(t1, h[(size_t)w * 16 + 12]);
        unsigned long long prev = h[(size_t)w * 16];
        for (int i = 1; i <= 12; ++i) { const unsigned long long v = h[(size_t)w * 16 + i]; if (v) { sum[i] += (double)(v - prev); prev = v; } }
      }
      fprintf(f, "M %d workgroups %d span %llu ticks; mean ticks per workgroup: layer1_loop %.0f layer1_store %.0f policy %.0f", M, nwg, t1 - t0, sum[1] / nwg, sum[2] / nwg, sum[3] / nwg);
      for (int l = 1; l <= 4; ++l) fprintf(f, " | hidden%d loop %.0f store %.0f", l, sum[2 + 2 * l] / nwg, sum[3 + 2 * l] / nwg);
      fprintf(f, " | head %.0f\n", sum[12] / nwg);
      fclose(f);
    }
  }
  return RR_OK;
}

// the rollout's actor in two launches: first policy layer split over k, then the remaining layers + the tanh-normal head
#define RR_POL_KSLICES 8
extern "C" size_t rr_policy_act_workspace_bytes(int32_t M) { return M > 0 ? (size_t)RR_POL_KSLICES * M * RR_MLP_PH * sizeof(float) : 0; }
extern "C" int rr_policy_act(const float* obs, const int64_t* obs_rows, int32_t M, int32_t K, const float* mean, const float* std_,
                             const rr_mlp_net* policy, const float* noise, float min_std, float* action, float* raw_action, float* log_prob,
                             float* logits, void* workspace, size_t workspace_bytes, void* stream) {
  if (!obs || !policy || !action || !workspace || M <= 0 || K <= 0) return fail(RR_EINVAL, "rr_policy_act: bad argument");
  if ((mean == nullptr) != (std_ == nullptr)) return fail(RR_EINVAL, "rr_policy_act: mean and std must be given together");
  RRMlpNet net;
  int rc = mlp_net(policy, K, RR_MLP_PH, false, &net, "policy", "rr_policy_act");
  if (rc) return rc;
  const int nh = net.nlayers - 1, P = net.out_dim, A_ = P / 2;
  if ((P & 1) || P > head_cols(P) || nh > RR_POL_MAXL - 1)
    return fail(RR_EUNSUPPORTED, "rr_policy_act: a head of " + std::to_string(P) + " logits (it must be 2 x action_size <= 128 wide, at most 7 hidden layers)");
  if (workspace_bytes < rr_policy_act_workspace_bytes(M)) return fail(RR_EINVAL, "rr_policy_act: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  RRPolL1Args L;
  memset(&L, 0, sizeof(L));
  L.obs = obs; L.rows = obs_rows; L.mean = mean; L.std_ = std_; L.W = net.W[0]; L.M = M; L.K = K; L.part = (float*)workspace;
  const int nchunk = (K + RR_MLP_KC - 1) / RR_MLP_KC;
  L.chunks_per_slice = (nchunk + RR_POL_KSLICES - 1) / RR_POL_KSLICES;
  const int nslice = (nchunk + L.chunks_per_slice - 1) / L.chunks_per_slice;
  hipLaunchKernelGGL(rr_policy_l1_kernel, dim3((M + RR_MLP_BM - 1) / RR_MLP_BM, nslice), dim3(256), 0, st, L);
  RRPolTailArgs T;
  memset(&T, 0, sizeof(T));
  T.part = (const float*)workspace; T.nslice = nslice; T.M = M; T.P = P; T.A = A_; T.nh = nh; T.noise = noise; T.min_std = min_std;
  T.action = action; T.raw = raw_action; T.logp = log_prob; T.logits = logits;
  for (int l = 1; l <= nh; ++l) T.W[l] = net.W[l];
  for (int l = 0; l <= nh; ++l) T.b[l] = net.b[l];
  const int HW = head_cols(P);
  const size_t lds = ((size_t)(nh - 1) * 1024 + (size_t)32 * HW + (size_t)nh * 32 + HW) * sizeof(float);
  const dim3 grid(std::max(1, std::min(256, (M + 7) / 8)));
  if (HW == 64) hipLaunchKernelGGL(rr_policy_tail_kernel<64>, grid, dim3(256), lds, st, T);
  else hipLaunchKernelGGL(rr_policy_tail_kernel<128>, grid, dim3(256), lds, st, T);
  HIPCHK(hipGetLastError());
  return RR_OK;
}

// value network backward: the delta chain on the matrix cores (csrc/rr_mlp.h)
extern "C" size_t rr_mlp_value_backward_workspace_bytes(int32_t M, int32_t nhidden) {
  if (M <= 0 || nhidden <= 0) return 0;
  return (size_t)nhidden * ((M + RR_MLP_BM - 1) / RR_MLP_BM) * RR_MLP_VH * sizeof(float);
}
extern "C" int rr_mlp_value_backward(const float* grad_value, const float* head_weight, const float* const* hidden_weights_t, int32_t nhidden,
                                     int32_t M, float* pre_act, float* delta, float* const* bias_grads, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  if (!grad_value || !head_weight || !hidden_weights_t || !pre_act || !delta || !bias_grads || !workspace || M <= 0)
    return fail(RR_EINVAL, "rr_mlp_value_backward: bad argument");
  if (nhidden < 1 || nhidden > RR_MLP_MAXL) return fail(RR_EUNSUPPORTED, "rr_mlp_value_backward: unsupported number of hidden layers");
  if (workspace_bytes < rr_mlp_value_backward_workspace_bytes(M, nhidden)) return fail(RR_EINVAL, "rr_mlp_value_backward: workspace too small");
  RRMlpBwdArgs A;
  memset(&A, 0, sizeof(A));
  A.g = grad_value; A.w_head = head_weight; A.z = pre_act; A.delta = delta; A.part = (float*)workspace; A.M = M; A.nh = nhidden;
  A.nblk = (M + RR_MLP_BM - 1) / RR_MLP_BM;
  for (int j = 0; j < nhidden; ++j) {
    if (!bias_grads[j] || (j > 0 && !hidden_weights_t[j])) return fail(RR_EINVAL, "rr_mlp_value_backward: null layer pointer");
    A.bgrad[j] = bias_grads[j];
    A.Wt[j] = j > 0 ? hidden_weights_t[j] : nullptr;
  }
  const size_t lds = RR_MLP_BWD_LDS_FLOATS * sizeof(float);
  if (const int rc = dyn_lds((const void*)rr_mlp_value_backward_kernel, lds)) return rc;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(rr_mlp_value_backward_kernel, dim3(A.nblk), dim3(256), lds, st, A);
  hipLaunchKernelGGL(rr_mlp_colsum_kernel, dim3(RR_MLP_VH / 16, nhidden), dim3(256), 0, st, A);
  HIPCHK(hipGetLastError());
  return RR_OK;
}

// 256-wide policy network backward: the value chain with a [n x P] . [P x 256] product at the head (csrc/rr_mlp.h)
extern "C" size_t rr_mlp_policy_backward_workspace_bytes(int32_t n, int32_t nhidden) { return rr_mlp_value_backward_workspace_bytes(n, nhidden); }
extern "C" int rr_mlp_policy_backward(const float* grad_logits, const float* head_weight_t, const float* const* hidden_weights_t, int32_t nhidden,
                                      int32_t n, int32_t M, int32_t P, float* pre_act, float* delta, float* const* bias_grads, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  if (!grad_logits || !head_weight_t || !hidden_weights_t || !pre_act || !delta || !bias_grads || !workspace || n <= 0 || M < n)
    return fail(RR_EINVAL, "rr_mlp_policy_backward: bad argument");
  if (P < 1 || P > 128) return fail(RR_EUNSUPPORTED, "rr_mlp_policy_backward: a head of " + std::to_string(P) + " logits (1 .. 128 are supported)");
  if (nhidden < 1 || nhidden > RR_MLP_MAXL - 1)
    return fail(RR_EUNSUPPORTED, "rr_mlp_policy_backward: " + std::to_string(nhidden) + " hidden layers (1 .. 7 are supported)");
  if (workspace_bytes < rr_mlp_policy_backward_workspace_bytes(n, nhidden)) return fail(RR_EINVAL, "rr_mlp_policy_backward: workspace too small");
  RRPol256BwdArgs A;
  RRMlpBwdArgs S;                                // what rr_mlp_colsum_kernel reads: part, nblk, bgrad
  memset(&A, 0, sizeof(A));
  memset(&S, 0, sizeof(S));
  A.g = grad_logits; A.wt_head = head_weight_t; A.z = pre_act; A.delta = delta; A.part = (float*)workspace; A.n = n; A.M = M; A.P = P; A.nh = nhidden;
  A.nblk = (n + RR_MLP_BM - 1) / RR_MLP_BM;
  S.part = A.part; S.nblk = A.nblk; S.M = n; S.nh = nhidden;
  for (int j = 0; j < nhidden; ++j) {
    if (!bias_grads[j] || (j > 0 && !hidden_weights_t[j])) return fail(RR_EINVAL, "rr_mlp_policy_backward: null layer pointer");
    S.bgrad[j] = bias_grads[j];
    A.Wt[j] = j > 0 ? hidden_weights_t[j] : nullptr;
  }
  const size_t lds = RR_MLP_BWD_LDS_FLOATS * sizeof(float);
  if (const int rc = dyn_lds((const void*)rr_mlp_policy256_backward_kernel, lds)) return rc;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(rr_mlp_policy256_backward_kernel, dim3(A.nblk), dim3(256), lds, st, A);
  hipLaunchKernelGGL(rr_mlp_colsum_kernel, dim3(RR_MLP_VH / 16, nhidden), dim3(256), 0, st, S);
  HIPCHK(hipGetLastError());
  return RR_OK;
}

// weight gradient dW = delta' h as a split-row matrix-core product (csrc/rr_mlp.h)
#ifndef RR_DW_KC128
#define RR_DW_KC128 16      // rows of a staged chunk of the 128 x 128-tile weight-gradient kernel (32: half the LDS hand-offs, twice the bytes in flight)
#endif
struct DwPlan { int to, ti, kc, rows_per_slice, nslice; };
// `group_tiles`: output tiles of ALL products that share this product's launch (rr_mlp_weight_grad_batch runs the products of one tile
// shape as one launch, item = grid z); 0 = the product is launched alone.  The slices are cut so that the LAUNCH has ~target workgroups:
// planned per product (round 2), the four 256 x 256 hidden-layer products of a minibatch were cut into 128 slices each although their
// launch already holds 36 tiles -- 134 MB of partial tiles written and read back where 29 MB do.
static DwPlan dw_plan(int M, int O, int I, int group_tiles = 0) {
  DwPlan p;
  p.to = O <= 32 ? 32 : (O <= 64 ? 64 : 128);
  p.ti = O <= 32 ? 128 : (O <= 64 ? 64 : 128);
  p.kc = O <= 32 ? 64 : (O <= 64 ? 32 : RR_DW_KC128);    // equal matrix-core work per LDS hand-off in the three tile shapes
  const int tiles = group_tiles > 0 ? group_tiles : ((O + p.to - 1) / p.to) * ((I + p.ti - 1) / p.ti);
  static const int target = [] { const char* e = getenv("RR_DW_TARGET_WGS"); const int v = e ? atoi(e) : 0; return v > 0 ? v : 512; }();   // workgroups per product
  static const int target_batch = [] { const char* e = getenv("RR_DW_TARGET_WGS_BATCH"); const int v = e ? atoi(e) : 0; return v > 0 ? v : 1024; }();   // ... per batched launch: two resident rounds
  const int want = std::max(1, std::min((group_tiles > 0 ? target_batch : target) / tiles, M / (2 * p.kc)));
  p.rows_per_slice = ((M + want - 1) / want + p.kc - 1) / p.kc * p.kc;
  p.nslice = (M + p.rows_per_slice - 1) / p.rows_per_slice;
  return p;
}
extern "C" size_t rr_mlp_weight_grad_batch_workspace_bytes(const rr_dw_item* items, int32_t n);
extern "C" size_t rr_mlp_weight_grad_workspace_bytes(int32_t M, int32_t O, int32_t I) {      // a single product = a batch of one
  if (M <= 0 || O <= 0 || I <= 0) return 0;
  rr_dw_item it;
  memset(&it, 0, sizeof(it));
  it.M = M; it.O = O; it.I = I;
  return rr_mlp_weight_grad_batch_workspace_bytes(&it, 1);
}
template <int GO, int GI, int WO, int WI, int KC>
static int dw_launch(const RRDwBatch& B, dim3 grid, hipStream_t st) {
  constexpr int TO = GO * WO * 32, TI = GI * WI * 32;
  constexpr size_t lds = (size_t)KC * ((TO + (TO % 64 == 0 ? 32 : 0)) + (TI + (TI % 64 == 0 ? 32 : 0))) * sizeof(float);
  if (const int rc = dyn_lds((const void*)rr_mlp_dw_kernel<GO, GI, WO, WI, KC>, lds)) return rc;
  hipLaunchKernelGGL((rr_mlp_dw_kernel<GO, GI, WO, WI, KC>), grid, dim3(256), lds, st, B);
  return RR_OK;
}
// tiles of each tile-shape group of a batch (the products of one shape share a launch)
static void dw_group_tiles(const rr_dw_item* items, int n, int* gt) {
  gt[0] = gt[1] = gt[2] = 0;
  for (int i = 0; i < n; ++i) {
    const DwPlan p = dw_plan(items[i].M, items[i].O, items[i].I);
    gt[p.to == 32 ? 0 : (p.to == 64 ? 1 : 2)] += ((items[i].O + p.to - 1) / p.to) * ((items[i].I + p.ti - 1) / p.ti);
  }
}
static DwPlan dw_plan_batch(const rr_dw_item& it, const int* gt) {
  const DwPlan p = dw_plan(it.M, it.O, it.I);
  return dw_plan(it.M, it.O, it.I, gt[p.to == 32 ? 0 : (p.to == 64 ? 1 : 2)]);
}
extern "C" size_t rr_mlp_weight_grad_batch_workspace_bytes(const rr_dw_item* items, int32_t n) {
  size_t t = 0;
  int gt[3];
  if (!items || n <= 0) return 0;
  for (int i = 0; i < n; ++i) if (items[i].M <= 0 || items[i].O <= 0 || items[i].I <= 0) return 0;
  dw_group_tiles(items, n, gt);
  for (int i = 0; i < n; ++i) t += rr_align_up((size_t)dw_plan_batch(items[i], gt).nslice * items[i].O * items[i].I * sizeof(float), 256);
  return t;
}
extern "C" int rr_mlp_weight_grad_batch(const rr_dw_item* items, int32_t n, void* workspace, size_t workspace_bytes, void* stream) {
  if (!items || n <= 0 || !workspace) return fail(RR_EINVAL, "rr_mlp_weight_grad_batch: bad argument");
  if (n > RR_DW_MAXB) return fail(RR_EUNSUPPORTED, "rr_mlp_weight_grad_batch: at most 12 products per call");
  if (workspace_bytes < rr_mlp_weight_grad_batch_workspace_bytes(items, n)) return fail(RR_EINVAL, "rr_mlp_weight_grad_batch: workspace too small");
  RRDwBatch all, grp[3];
  memset(&all, 0, sizeof(all));
  memset(grp, 0, sizeof(grp));
  dim3 ggrid[3] = {dim3(0, 0, 0), dim3(0, 0, 0), dim3(0, 0, 0)};
  unsigned red_blocks = 0;
  char* w = (char*)workspace;
  int gt[3];
  for (int i = 0; i < n; ++i)
    if (!items[i].delta || !items[i].act || !items[i].grad || items[i].M <= 0 || items[i].O <= 0 || items[i].I <= 0) return fail(RR_EINVAL, "rr_mlp_weight_grad_batch: bad item");
  dw_group_tiles(items, n, gt);
  for (int i = 0; i < n; ++i) {
    const rr_dw_item& it = items[i];
    if ((it.mean == nullptr) != (it.std == nullptr) || (it.mean && !it.delta_colsum))
      return fail(RR_EINVAL, "rr_mlp_weight_grad_batch: mean, std and delta_colsum must be given together");
    const DwPlan p = dw_plan_batch(it, gt);
    RRDwArgs A;
    memset(&A, 0, sizeof(A));
    A.rows_per_slice = p.rows_per_slice; A.nslice = p.nslice;
    A.a = it.delta; A.b = it.act; A.rows = it.act_rows; A.mean = it.mean; A.std_ = it.std; A.bsum = it.delta_colsum; A.M = it.M; A.O = it.O; A.I = it.I;
    A.part = (float*)w; A.out = it.grad;
    w += rr_align_up((size_t)p.nslice * it.O * it.I * sizeof(float), 256);
    all.it[all.n++] = A;
    const int g = p.to == 32 ? 0 : (p.to == 64 ? 1 : 2);
    grp[g].it[grp[g].n++] = A;
    ggrid[g].x = std::max<unsigned>(ggrid[g].x, ((it.O + p.to - 1) / p.to) * ((it.I + p.ti - 1) / p.ti));
    ggrid[g].y = std::max<unsigned>(ggrid[g].y, (unsigned)p.nslice);
    ggrid[g].z = grp[g].n;
    red_blocks = std::max<unsigned>(red_blocks, (unsigned)(((size_t)it.O * it.I + 1023) / 1024));
  }
  hipStream_t st = (hipStream_t)stream;
  int rc = RR_OK;
  if (grp[2].n) rc = dw_launch<2, 2, 2, 2, RR_DW_KC128>(grp[2], ggrid[2], st);      // the big tiles first: they are the long ones
  if (!rc && grp[1].n) rc = dw_launch<2, 2, 1, 1, 32>(grp[1], ggrid[1], st);
  if (!rc && grp[0].n) rc = dw_launch<1, 4, 1, 1, 64>(grp[0], ggrid[0], st);
  if (rc) return rc;
  hipLaunchKernelGGL(rr_mlp_dw_reduce_kernel, dim3(red_blocks, all.n), dim3(256), 0, st, all);
  HIPCHK(hipGetLastError());
  return RR_OK;
}
extern "C" int rr_mlp_weight_grad(const float* delta, const float* act, const int64_t* act_rows, const float* mean, const float* std_,
                                  const float* delta_colsum, int32_t M, int32_t O, int32_t I, float* grad, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  if (!delta || !act || !grad || !workspace || M <= 0 || O <= 0 || I <= 0) return fail(RR_EINVAL, "rr_mlp_weight_grad: bad argument");
  if (workspace_bytes < rr_mlp_weight_grad_workspace_bytes(M, O, I)) return fail(RR_EINVAL, "rr_mlp_weight_grad: workspace too small (rr_mlp_weight_grad_workspace_bytes)");
  rr_dw_item it;
  memset(&it, 0, sizeof(it));
  it.delta = delta; it.act = act; it.act_rows = act_rows; it.mean = mean; it.std = std_; it.delta_colsum = delta_colsum; it.M = M; it.O = O; it.I = I;
  it.grad = grad;
  return rr_mlp_weight_grad_batch(&it, 1, workspace, rr_align_up(workspace_bytes, 256), stream);
}

// ------------------------------------------------------------------------------------------ observation normaliser sums (csrc/rr_ppo.h)
static void mom_plan(long long nrows, int* rows_per_block, int* nblk) {
  const long long target = 2048;                              // blocks: one resident round of 8 per CU
  long long rpb = (nrows + target - 1) / target;
  if (rpb < 16) rpb = 16;
  *rows_per_block = (int)rpb;
  *nblk = (int)((nrows + rpb - 1) / rpb);
}
extern "C" size_t rr_obs_moments_workspace_bytes(int64_t nseq, int32_t T, int32_t K) {
  if (nseq <= 0 || T <= 0 || K <= 0) return 0;
  int rpb, nblk;
  mom_plan((long long)nseq * T, &rpb, &nblk);
  return (size_t)nblk * 2 * K * sizeof(double);
}
extern "C" int rr_obs_moments(const float* obs, int64_t nseq, int32_t Tp1, int32_t T, int32_t K, const float* mean, double* sums, void* workspace,
                              size_t workspace_bytes, void* stream) {
  if (!obs || !mean || !sums || !workspace || nseq <= 0 || T <= 0 || Tp1 < T || K <= 0) return fail(RR_EINVAL, "rr_obs_moments: bad argument");
  if (workspace_bytes < rr_obs_moments_workspace_bytes(nseq, T, K) || ((uintptr_t)workspace & 7) || ((uintptr_t)sums & 7))
    return fail(RR_EINVAL, "rr_obs_moments: workspace too small (rr_obs_moments_workspace_bytes) or not 8-byte aligned");
  RRMomArgs A;
  memset(&A, 0, sizeof(A));
  A.obs = obs; A.mean = mean; A.nrows = (long long)nseq * T; A.Tp1 = Tp1; A.T = T; A.K = K; A.part = (double*)workspace; A.out = sums;
  mom_plan(A.nrows, &A.rows_per_block, &A.nblk);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(rr_obs_moments_kernel, dim3(A.nblk), dim3(256), 0, st, A);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(rr_obs_moments_reduce_kernel, dim3((2 * K + 255) / 256), dim3(256), 0, st, A);
  HIPCHK(hipGetLastError());
  return RR_OK;
}

// ------------------------------------------------------------------------------------------ Adam behind a global-norm clip
extern "C" int32_t rr_clipped_adam_partials(int64_t n) {
  if (n <= 0) return 0;
  const int64_t k = (n + RR_ADAM_PART_ELEMS - 1) / RR_ADAM_PART_ELEMS;
  return (int32_t)(k < RR_ADAM_MAX_PARTIALS ? k : RR_ADAM_MAX_PARTIALS);
}
extern "C" size_t rr_clipped_adam_workspace_bytes(int64_t n) { return (size_t)rr_clipped_adam_partials(n) * sizeof(double); }
// kl_dev != NULL: the KL instance of the finalisation (rr_clipped_adam_step_kl), which writes cfg_dev[0]
static int clipped_adam_launch(const rr_adam_tensor* table, int32_t ntensors, const float* grad_flat, float* m_flat, float* v_flat, int64_t n,
                               double* cfg_dev, double* state_dev, const float* kl_dev, const double* klcfg_dev, void* workspace, void* stream) {
  const std::string who = kl_dev ? "rr_clipped_adam_step_kl" : "rr_clipped_adam_step";       // the entry the caller used, for its error text
  if (ntensors > RR_ADAM_MAX_TENSORS) return fail(RR_EINVAL, who + ": more than 64 tensors");
  if (!table || ntensors <= 0 || !grad_flat || !m_flat || !v_flat || !cfg_dev || !state_dev || !workspace || n <= 0)
    return fail(RR_EINVAL, who + ": bad argument");
  if ((((uintptr_t)grad_flat | (uintptr_t)m_flat | (uintptr_t)v_flat) & 15) || (((uintptr_t)cfg_dev | (uintptr_t)state_dev | (uintptr_t)workspace) & 7))
    return fail(RR_EINVAL, who + ": the flat buffers must be 16-byte aligned, cfg / state / workspace 8-byte aligned");
  RRAdamTable T;
  memset(&T, 0, sizeof(T));
  int64_t sum = 0, blocks = 0;
  for (int k = 0; k < ntensors; ++k) {           // the segments tile [0, n) in table order: every access of the flat buffers is in range
    const rr_adam_tensor& e = table[k];
    if (!e.param || ((uintptr_t)e.param & 3)) return fail(RR_EINVAL, who + ": null or misaligned parameter pointer in the table");
    if (e.numel <= 0 || e.offset != sum || e.numel > n - sum)
      return fail(RR_EINVAL, who + ": the table's segments must follow each other from offset 0 and sum to n");
    T.t[k].p = e.param; T.t[k].off = e.offset; T.t[k].numel = e.numel;
    int64_t head = (4 - (e.offset & 3)) & 3;
    if (head > e.numel) head = e.numel;
    const int64_t nb = (e.numel - head) >> 2, nblk = nb ? (nb + 255) / 256 : 1;
    T.first_block[k] = (int)blocks;
    blocks += nblk;
    if (blocks > INT_MAX) return fail(RR_EINVAL, who + ": too many elements");
    sum += e.numel;
  }
  if (sum != n) return fail(RR_EINVAL, who + ": n differs from the sum of the table's element counts");
  for (int k = ntensors; k <= RR_ADAM_MAX_TENSORS; ++k) T.first_block[k] = (int)blocks;
  T.ntensors = ntensors;
  const int nparts = rr_clipped_adam_partials(n);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(rr_adam_sumsq_kernel, dim3(nparts), dim3(256), 0, st, grad_flat, (long long)n, (double*)workspace);
  HIPCHK(hipGetLastError());
  if (kl_dev)
    hipLaunchKernelGGL(rr_adam_finalize_kernel<true>, dim3(1), dim3(64), 0, st, (const double*)workspace, nparts, cfg_dev, state_dev, kl_dev, klcfg_dev);
  else
    hipLaunchKernelGGL(rr_adam_finalize_kernel<false>, dim3(1), dim3(64), 0, st, (const double*)workspace, nparts, (const double*)cfg_dev, state_dev,
                       (const float*)nullptr, (const double*)nullptr);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(rr_adam_apply_kernel, dim3((unsigned)blocks), dim3(256), 0, st, T, grad_flat, m_flat, v_flat, (const double*)cfg_dev,
                     (const double*)state_dev);
  HIPCHK(hipGetLastError());
  return RR_OK;
}
extern "C" int rr_clipped_adam_step(const rr_adam_tensor* table, int32_t ntensors, const float* grad_flat, float* m_flat, float* v_flat, int64_t n,
                                    const double* cfg_dev, double* state_dev, void* workspace, void* stream) {
  return clipped_adam_launch(table, ntensors, grad_flat, m_flat, v_flat, n, const_cast<double*>(cfg_dev), state_dev, nullptr, nullptr, workspace,
                             stream);
}
extern "C" int rr_clipped_adam_step_kl(const rr_adam_tensor* table, int32_t ntensors, const float* grad_flat, float* m_flat, float* v_flat,
                                       int64_t n, double* cfg_dev, double* state_dev, const float* kl_dev, const double* klcfg_dev,
                                       void* workspace, void* stream) {
  if (!kl_dev || !klcfg_dev || ((uintptr_t)kl_dev & 3) || ((uintptr_t)klcfg_dev & 7))
    return fail(RR_EINVAL, "rr_clipped_adam_step_kl: kl_dev (4-byte aligned) and klcfg_dev (8-byte aligned) must be given");
  return clipped_adam_launch(table, ntensors, grad_flat, m_flat, v_flat, n, cfg_dev, state_dev, kl_dev, klcfg_dev, workspace, stream);
}

// ------------------------------------------------------------------------------------------ training wrappers, fused
// brax.envs.wrappers.training: EpisodeWrapper (step count, truncation, done at episode end) followed by AutoResetWrapper
// (restore the stored first state where done) -- ~15 elementwise launches per env step when composed from tensor ops;
// here one launch, one 256-thread block per env.  Arrays are row-major [N][width]; `cur` is overwritten in place.
#define RR_WRAP_MAX 12
struct RRWrapArgs { const float* first[RR_WRAP_MAX]; float* cur[RR_WRAP_MAX]; int width[RR_WRAP_MAX]; int narr; };
// What the rule gains level by level; each level has the ones below it, and its own members of RRWrapClip (by value, like RRWrapArgs):
//   RESTART  (rr_clip_restart_io's rule, one env step): `first[i]` are banks [num_slots][N][widths[i]], the clip's end joins `over`, and
//            where done the next bank entry and its frame come back.  cur_frame holds the stepped frame and is finished in place.
//   LIBRARY  (rr_clip_library_io's): the clip's end is taken at the length of the clip the step was made on, and where done the bank
//            entry's clip comes back with its frame.  clip is finished in place; null pointers switch the two additions off one by one.
//   SAMPLING (rr_clip_sampling_io's): the outcome counters of the step -- on the clip it was made on, flushed every step -- and, where
//            done, the slot drawn by the env's bank weights instead of the next one.  pose_fail: the step's pose-termination codes (null:
//            none).  Null outcomes / clip_weights switch the two additions off one by one.  This level knows num_clips and clamps every
//            clip id into 0 .. num_clips - 1; LIBRARY clamps the id it indexes clip_lengths with below only and hands a bank entry's on.
enum { RR_WRAP_PLAIN, RR_WRAP_RESTART, RR_WRAP_LIBRARY, RR_WRAP_SAMPLING };
struct RRWrapClip {
  int* cur_frame; const int* bank_frames; const int* slot_in; int* slot_out; int num_slots, track_len, end_at_clip_end;      // RESTART
  int* clip; const int* bank_clips; const int* clip_lengths;                                                                 // LIBRARY
  int num_clips; const float* pose_fail; const int* clip_weights; const int* draws_in; int* draws_out; long long* outcomes;  // SAMPLING
  unsigned seed;
};
template <int LEVEL>
__global__ void rr_wrap_kernel(const RRWrapArgs A, const RRWrapClip K, const float* __restrict__ prev_done, const float* __restrict__ prev_steps,
                               float* __restrict__ done, float* __restrict__ steps, float* __restrict__ truncation,
                               float episode_length, float action_repeat) {
  const int e = blockIdx.x, N = gridDim.x;
  auto clip_id = [&](int c) {            // a clip id as the level takes it
    c = c < 0 ? 0 : c;
    if constexpr (LEVEL >= RR_WRAP_SAMPLING) c = c > K.num_clips - 1 ? K.num_clips - 1 : c;
    return c;
  };
  // AutoReset (before the step): steps <- 0 where the incoming state was done;  Episode: steps += action_repeat, done at the
  // episode end, truncation = over & !terminated;  AutoReset (after): first state where done
  const float s0 = prev_done[e] != 0.0f ? 0.0f : prev_steps[e];
  const float s1 = s0 + action_repeat;
  bool over = s1 >= episode_length;
  int new_frame = 0, c = 0;
  if constexpr (LEVEL >= RR_WRAP_RESTART) {
    new_frame = K.cur_frame[e];
    int len = K.track_len;
    if constexpr (LEVEL >= RR_WRAP_LIBRARY) {
      c = clip_id(K.clip ? K.clip[e] : 0);
      if (K.clip_lengths) { len = K.clip_lengths[c]; len = len < 1 ? 1 : (len > K.track_len ? K.track_len : len); }
    }
    over = over || (K.end_at_clip_end && new_frame >= len - 1);
  }
  const int c_step = c;                  // the clip the step was made on
  const float d_env = done[e];
  const float d_out = over ? 1.0f : d_env;
  size_t row = e;                        // the row of `first` that comes back where done
  int frame = 0, slot = 0;
  bool failed = false;
  unsigned n = 0;
  if constexpr (LEVEL >= RR_WRAP_RESTART) {
    if constexpr (LEVEL >= RR_WRAP_SAMPLING) {
      failed = K.pose_fail && K.pose_fail[e] != 0.0f;
      n = K.draws_in ? (unsigned)K.draws_in[e] : 0u;
    }
    slot = K.slot_in[e];
    slot = slot < 0 ? 0 : (slot > K.num_slots - 1 ? K.num_slots - 1 : slot);      // clamped into the bank
    if (d_out != 0.0f) {
      int drawn = -1;
      if constexpr (LEVEL >= RR_WRAP_SAMPLING) {
        if (K.clip_weights && K.bank_clips) {      // the K entries one after the other: every thread of the block forms the same slot
          auto weight = [&](int k) { return (unsigned)K.clip_weights[clip_id(K.bank_clips[(size_t)k * N + e])] & 0xFFFFu; };
          unsigned S = 0;
          for (int k = 0; k < K.num_slots; ++k) S += weight(k);
          if (S != 0) {
            const unsigned h = rr_fmix32(rr_fmix32(K.seed ^ ((unsigned)e * 0x9E3779B1u)) + n);
            const unsigned r = (unsigned)(((unsigned long long)h * (unsigned long long)S) >> 32);
            unsigned p = 0;
            drawn = K.num_slots - 1;
            for (int k = 0; k < K.num_slots; ++k) {
              p += weight(k);
              if (p > r) { drawn = k; break; }
            }
          }
        }
        n = n + 1u;
      }
      slot = drawn >= 0 ? drawn : (slot + 1 >= K.num_slots ? 0 : slot + 1);
    }
    row = (size_t)slot * N + e;
    frame = d_out != 0.0f ? K.bank_frames[row] : new_frame;
    if constexpr (LEVEL >= RR_WRAP_LIBRARY) {
      if (d_out != 0.0f && K.bank_clips) c = LEVEL >= RR_WRAP_SAMPLING ? clip_id(K.bank_clips[row]) : K.bank_clips[row];
    }
  }
  __syncthreads();                       // every thread has read done[e], cur_frame[e] and clip[e] before thread 0 rewrites them
  if (threadIdx.x == 0) {
    steps[e] = s1; truncation[e] = over ? 1.0f - d_env : 0.0f; done[e] = d_out;
    if constexpr (LEVEL >= RR_WRAP_RESTART) { K.cur_frame[e] = frame; K.slot_out[e] = slot; }
    if constexpr (LEVEL >= RR_WRAP_LIBRARY) {
      if (K.clip) K.clip[e] = c;
    }
    if constexpr (LEVEL >= RR_WRAP_SAMPLING) {
      if (K.draws_out) K.draws_out[e] = (int)n;
      if (K.outcomes) {
        long long* orow = K.outcomes + 5 * (size_t)c_step;
        __hip_atomic_fetch_add(orow + 4, 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (d_out != 0.0f) {
          __hip_atomic_fetch_add(orow, 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_fetch_add(orow + (failed ? 1 : (d_env != 0.0f ? 2 : 3)), 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
  }
  if (d_out != 0.0f) {
    for (int a = 0; a < A.narr; ++a) {
      const int w = A.width[a];
      const float* src = A.first[a] + row * w;
      float* dst = A.cur[a] + (size_t)e * w;
      for (int i = threadIdx.x; i < w; i += blockDim.x) dst[i] = src[i];
    }
  }
}

// The checks of every entry `who` in their one order -- the scalar arguments and required pointers, num_slots, the entry's own refusal
// `why` (null: none), the arrays -- and the launch.
template <int LEVEL>
static int wrap_launch(const char* who, int32_t num_envs, int32_t narr, const float* const* first, float* const* cur, const int32_t* widths,
                       const float* prev_done, const float* prev_steps, float* done, float* steps, float* truncation,
                       float episode_length, float action_repeat, const RRWrapClip& K, const char* why, void* stream) {
  const std::string name = std::string(who) + ": ";
  if (num_envs <= 0 || narr < 0 || narr > RR_WRAP_MAX || !prev_done || !prev_steps || !done || !steps || !truncation ||
      (LEVEL >= RR_WRAP_RESTART && (!K.cur_frame || !K.bank_frames || !K.slot_in || !K.slot_out || K.track_len <= 0)) ||
      (LEVEL >= RR_WRAP_SAMPLING && K.num_clips < 1) || (LEVEL >= RR_WRAP_LIBRARY && K.bank_clips && !K.clip))
    return fail(RR_EINVAL, name + "bad argument");
  if (LEVEL >= RR_WRAP_RESTART && (K.num_slots < 1 || K.num_slots > 64)) return fail(RR_EINVAL, name + "num_slots must lie in 1 .. 64");
  if (why) return fail(RR_EINVAL, name + why);
  RRWrapArgs A;
  memset(&A, 0, sizeof(A));
  A.narr = narr;
  for (int i = 0; i < narr; ++i) {
    if (!first[i] || !cur[i] || widths[i] <= 0) return fail(RR_EINVAL, name + "null array");
    A.first[i] = first[i]; A.cur[i] = cur[i]; A.width[i] = widths[i];
  }
  hipLaunchKernelGGL(rr_wrap_kernel<LEVEL>, dim3(num_envs), dim3(256), 0, (hipStream_t)stream, A, K, prev_done, prev_steps, done, steps, truncation,
                     episode_length, action_repeat);
  HIPCHK(hipGetLastError());
  return RR_OK;
}

extern "C" int rr_wrap_episode_autoreset(int32_t num_envs, int32_t narr, const float* const* first, float* const* cur, const int32_t* widths,
                                         const float* prev_done, const float* prev_steps, float* done, float* steps, float* truncation,
                                         float episode_length, float action_repeat, void* stream) {
  return wrap_launch<RR_WRAP_PLAIN>("rr_wrap_episode_autoreset", num_envs, narr, first, cur, widths, prev_done, prev_steps, done, steps, truncation,
                                    episode_length, action_repeat, RRWrapClip{}, nullptr, stream);
}

extern "C" int rr_wrap_clip_restart(int32_t num_envs, int32_t narr, const float* const* first, float* const* cur, const int32_t* widths,
                                    const float* prev_done, const float* prev_steps, float* done, float* steps, float* truncation,
                                    float episode_length, float action_repeat, int32_t* cur_frame, const int32_t* bank_frames,
                                    const int32_t* slot_in, int32_t* slot_out, int32_t num_slots, int32_t track_len, int32_t end_at_clip_end,
                                    void* stream) {
  const RRWrapClip K = {cur_frame, bank_frames, slot_in, slot_out, num_slots, track_len, end_at_clip_end};
  return wrap_launch<RR_WRAP_RESTART>("rr_wrap_clip_restart", num_envs, narr, first, cur, widths, prev_done, prev_steps, done, steps, truncation,
                                      episode_length, action_repeat, K, nullptr, stream);
}

extern "C" int rr_wrap_clip_library(int32_t num_envs, int32_t narr, const float* const* first, float* const* cur, const int32_t* widths,
                                    const float* prev_done, const float* prev_steps, float* done, float* steps, float* truncation,
                                    float episode_length, float action_repeat, int32_t* cur_frame, const int32_t* bank_frames,
                                    const int32_t* slot_in, int32_t* slot_out, int32_t num_slots, int32_t track_len, int32_t end_at_clip_end,
                                    int32_t* clip, const int32_t* bank_clips, const int32_t* clip_lengths, void* stream) {
  const RRWrapClip K = {cur_frame, bank_frames, slot_in, slot_out, num_slots, track_len, end_at_clip_end, clip, bank_clips, clip_lengths};
  return wrap_launch<RR_WRAP_LIBRARY>("rr_wrap_clip_library", num_envs, narr, first, cur, widths, prev_done, prev_steps, done, steps, truncation,
                                      episode_length, action_repeat, K, nullptr, stream);
}

extern "C" int rr_wrap_clip_sampling(int32_t num_envs, int32_t narr, const float* const* first, float* const* cur, const int32_t* widths,
                                     const float* prev_done, const float* prev_steps, float* done, float* steps, float* truncation,
                                     float episode_length, float action_repeat, int32_t* cur_frame, const int32_t* bank_frames,
                                     const int32_t* slot_in, int32_t* slot_out, int32_t num_slots, int32_t track_len, int32_t end_at_clip_end,
                                     int32_t* clip, const int32_t* bank_clips, const int32_t* clip_lengths, int32_t num_clips,
                                     const float* pose_fail, const rr_clip_sampling_io* sampling, void* stream) {
  if (!sampling) return fail(RR_EINVAL, "rr_wrap_clip_sampling: bad argument");      // (the first check's answer, whatever else is wrong)
  const rr_clip_sampling_io& s = *sampling;
  const char* why = !s.clip_weights && !s.outcomes ? "null clip_weights and outcomes"
                    : s.clip_weights && (!bank_clips || !s.draws_in || !s.draws_out) ? "clip_weights needs bank_clips, draws_in and draws_out"
                    : s.outcomes && num_clips > 1 && !clip ? "outcomes of several clips need clip" : nullptr;
  const RRWrapClip K = {cur_frame, bank_frames, slot_in, slot_out, num_slots, track_len, end_at_clip_end, clip, bank_clips, clip_lengths,
                        num_clips, pose_fail, s.clip_weights, s.draws_in, s.draws_out, (long long*)s.outcomes, s.seed};
  return wrap_launch<RR_WRAP_SAMPLING>("rr_wrap_clip_sampling", num_envs, narr, first, cur, widths, prev_done, prev_steps, done, steps, truncation,
                                       episode_length, action_repeat, K, why, stream);
}

extern "C" int rr_debug_layout(const rr_batch* b, const char*** names, const int32_t** offsets, const int32_t** sizes) {
  if (!b) return fail(RR_EINVAL, "rr_debug_layout: null batch");
  if (names) *names = const_cast<const char**>(b->m->dbg_cnames.data());
  if (offsets) *offsets = b->m->dbg_off.data();
  if (sizes) *sizes = b->m->dbg_size.data();
  return (int)b->m->dbg_names.size();
}

extern "C" int rr_batch_set_profile(rr_batch* b, uint64_t* dev_cycles) {
  if (!b) return fail(RR_EINVAL, "rr_batch_set_profile: null batch");
  if (dev_cycles) {
    const Instance in = select(b->m, F_STEP, V_PROFILE);      // rr_batch_create has set its LDS attribute
    if (!in.kern) return fail(RR_EUNSUPPORTED, std::string("rr_batch_set_profile: ") + in.why);
    if (b->has_env_params()) return fail(RR_EUNSUPPORTED, "rr_batch_set_profile: no profile build on a batch with per-env parameters");
  }
  b->prof = (unsigned long long*)dev_cycles;
  return RR_OK;
}

extern "C" int rr_batch_env_params_supported(const rr_batch* b) {
  if (!b) return fail(RR_EINVAL, "rr_batch_env_params_supported: null batch");
  return select(b->m, F_STEP, V_RAND).kern ? 1 : 0;
}
// the answer of a rr_batch_*_supported query: 1, or 0 with `who: why` as the last error
static int supported(const char* who, const char* why) {
  if (why) (void)fail(RR_EUNSUPPORTED, std::string(who) + ": " + why);
  return why ? 0 : 1;
}
extern "C" int rr_batch_pose_supported(const rr_batch* b) {
  if (!b) return fail(RR_EINVAL, "rr_batch_pose_supported: null batch");
  const Instance in = select(b->m, F_STEP, V_POSE);
  const char* why = in.kern ? nullptr : in.why;
  if (!why && b->has_env_params()) why = "pose tracking: no pose instance reads per-env parameters (this batch carries some)";
  if (!why && b->prof) why = "pose tracking: no profile build with track_pose";
  return supported("rr_batch_pose_supported", why);
}
extern "C" int rr_batch_set_pose(rr_batch* b, const rr_pose_io* p) {
  if (!b) return fail(RR_EINVAL, "rr_batch_set_pose: null batch");
  if (!p || (!p->track_pose && !p->pose_metrics)) {
    if (b->ref_frames > 0) return fail(RR_EINVAL, "rr_batch_set_pose: the batch carries reference frames (rr_batch_set_reference_obs), whose rows come from the pose block: set them to 0 first");
    if (b->has_clip_library()) return fail(RR_EINVAL, "rr_batch_set_pose: the batch carries a clip-library block (rr_batch_set_clip_library), which serves pose envs only: clear it first");
    if (b->restart.frames) return fail(RR_EINVAL, "rr_batch_set_pose: the batch carries a clip-restart block (rr_batch_set_clip_restarts), which serves pose envs only: clear it first");
    if (b->vel.track_vel) return fail(RR_EINVAL, "rr_batch_set_pose: the batch carries a velocity-tracking block (rr_batch_set_velocity_tracking), whose rows are indexed like the pose block's: clear it first");
    if (b->body.track_bodies) return fail(RR_EINVAL, "rr_batch_set_pose: the batch carries a body-tracking block (rr_batch_set_body_tracking), whose rows are indexed like the pose block's: clear it first");
    if (b->pterm.fail) return fail(RR_EINVAL, "rr_batch_set_pose: the batch carries a pose-termination block (rr_batch_set_pose_termination), whose errors come from the pose block: clear it first");
    b->pose = rr_pose_io{};
    return RR_OK;
  }
  if (!p->track_pose || !p->pose_metrics) return fail(RR_EINVAL, "rr_batch_set_pose: track_pose and pose_metrics go together");
  for (float x : {p->quat_reward_weight, p->quat_reward_scale, p->joint_reward_weight, p->joint_reward_scale})
    if (!(x >= 0.0f) || !std::isfinite(x)) return fail(RR_EINVAL, "rr_batch_set_pose: pose reward weights and scales must be finite and >= 0");
  if (rr_batch_pose_supported(b) != 1) return RR_EUNSUPPORTED;      // the reason is in place
  b->pose = *p;
  return RR_OK;
}
// What keeps an option of the pose family off this batch, or null.  form: F_STEP for the options that rr_body_kernel serves in every
// launch form (reference frames, pose termination, body tracking), F_UNROLL for clip restarts (rr_restart_kernel: multi-step forms
// only).  frames: the reference frames the batch carries or is about to, 0 .. 16; with_actor also asks the width the in-kernel actor of
// these instances reads
static const char* pose_option_limit(const rr_batch* b, Form form, int frames, bool with_actor) {
  const Instance in = select(b->m, with_actor ? F_ACTOR : form, form == F_STEP ? V_BODY : V_RESTART);
  if (!in.kern) return in.why;
  if (b->has_env_params()) return "pose tracking: no pose instance reads per-env parameters (this batch carries some)";
  if (b->prof) return "pose tracking: no profile build with track_pose";
  return with_actor ? actor_limit(b->m, nullptr, frames, true) : nullptr;
}
extern "C" int rr_batch_reference_obs_supported(const rr_batch* b, int32_t frames, int32_t with_actor) {
  if (!b) return fail(RR_EINVAL, "rr_batch_reference_obs_supported: null batch");
  if (frames < 0 || frames > 16) return supported("rr_batch_reference_obs_supported", "reference observation: frames must lie in 0 .. 16");
  // no frames: the model's own row in the instances the batch launches anyway
  return supported("rr_batch_reference_obs_supported", frames == 0 ? (with_actor ? actor_limit(b->m, nullptr) : nullptr) : pose_option_limit(b, F_STEP, frames, with_actor != 0));
}
extern "C" int rr_batch_set_reference_obs(rr_batch* b, int32_t frames) {
  if (!b) return fail(RR_EINVAL, "rr_batch_set_reference_obs: null batch");
  if (frames < 0 || frames > 16) return fail(RR_EINVAL, "rr_batch_set_reference_obs: frames must lie in 0 .. 16");
  if (frames > 0 && !b->pose.track_pose) return fail(RR_EINVAL, "rr_batch_set_reference_obs: frames > 0 need a pose block (rr_batch_set_pose) first: the rows come from track_pose");
  if (const char* why = frames > 0 ? pose_option_limit(b, F_STEP, frames, false) : nullptr) return fail(RR_EUNSUPPORTED, std::string("rr_batch_set_reference_obs: ") + why);
  b->ref_frames = frames;
  return RR_OK;
}
extern "C" int rr_batch_pose_termination_supported(const rr_batch* b, int32_t with_actor) {
  if (!b) return fail(RR_EINVAL, "rr_batch_pose_termination_supported: null batch");
  return supported("rr_batch_pose_termination_supported", pose_option_limit(b, F_STEP, b->ref_frames, with_actor != 0));
}
extern "C" int rr_batch_set_pose_termination(rr_batch* b, const rr_pose_term_io* t) {
  if (!b) return fail(RR_EINVAL, "rr_batch_set_pose_termination: null batch");
  if (!t) { b->pterm = rr_pose_term_io{}; return RR_OK; }
  if (const char* why = pose_option_limit(b, F_STEP, b->ref_frames, false)) return fail(RR_EUNSUPPORTED, std::string("rr_batch_set_pose_termination: ") + why);
  if (!b->pose.track_pose) return fail(RR_EINVAL, "rr_batch_set_pose_termination: needs a pose block (rr_batch_set_pose) first: the errors are taken against track_pose's rows");
  if (!t->fail) return fail(RR_EINVAL, "rr_batch_set_pose_termination: null fail array");
  for (float x : {t->max_pos, t->max_quat, t->max_joint})
    if (!(x > 0.0f)) return fail(RR_EINVAL, "rr_batch_set_pose_termination: thresholds must be > 0 and not NaN (INFINITY switches a criterion off)");
  b->pterm = *t;
  return RR_OK;
}
extern "C" int rr_batch_body_tracking_supported(const rr_batch* b, int32_t with_actor) {
  if (!b) return fail(RR_EINVAL, "rr_batch_body_tracking_supported: null batch");
  return supported("rr_batch_body_tracking_supported", pose_option_limit(b, F_STEP, b->ref_frames, with_actor != 0));
}
extern "C" int rr_batch_set_body_tracking(rr_batch* b, const rr_body_io* t) {
  if (!b) return fail(RR_EINVAL, "rr_batch_set_body_tracking: null batch");
  if (!t) { b->body = rr_body_io{}; return RR_OK; }
  if (const char* why = pose_option_limit(b, F_STEP, b->ref_frames, false)) return fail(RR_EUNSUPPORTED, std::string("rr_batch_set_body_tracking: ") + why);
  if (!b->pose.track_pose) return fail(RR_EINVAL, "rr_batch_set_body_tracking: needs a pose block (rr_batch_set_pose) first: track_bodies is indexed like track_pose");
  if (!t->track_bodies || !t->body_weights || !t->body_metrics) return fail(RR_EINVAL, "rr_batch_set_body_tracking: null track_bodies, body_weights or body_metrics");
  for (float x : {t->body_reward_weight, t->body_reward_scale, t->endeff_reward_weight, t->endeff_reward_scale})
    if (!(x >= 0.0f) || !std::isfinite(x)) return fail(RR_EINVAL, "rr_batch_set_body_tracking: weights and scales must be finite and >= 0");
  b->body = *t;
  return RR_OK;
}
extern "C" int rr_batch_velocity_tracking_supported(const rr_batch* b, int32_t with_actor) {
  if (!b) return fail(RR_EINVAL, "rr_batch_velocity_tracking_supported: null batch");
  return supported("rr_batch_velocity_tracking_supported", pose_option_limit(b, F_STEP, b->ref_frames, with_actor != 0));
}
extern "C" int rr_batch_set_velocity_tracking(rr_batch* b, const rr_vel_io* t) {
  if (!b) return fail(RR_EINVAL, "rr_batch_set_velocity_tracking: null batch");
  if (!t) { b->vel = rr_vel_io{}; return RR_OK; }
  if (const char* why = pose_option_limit(b, F_STEP, b->ref_frames, false)) return fail(RR_EUNSUPPORTED, std::string("rr_batch_set_velocity_tracking: ") + why);
  if (!b->pose.track_pose) return fail(RR_EINVAL, "rr_batch_set_velocity_tracking: needs a pose block (rr_batch_set_pose) first: track_vel is indexed like track_pose");
  if (!t->track_vel || !t->vel_metrics) return fail(RR_EINVAL, "rr_batch_set_velocity_tracking: null track_vel or vel_metrics");
  for (float x : {t->lin_weight, t->lin_scale, t->ang_weight, t->ang_scale, t->joint_weight, t->joint_scale})
    if (!(x >= 0.0f) || !std::isfinite(x)) return fail(RR_EINVAL, "rr_batch_set_velocity_tracking: weights and scales must be finite and >= 0");
  b->vel = *t;
  return RR_OK;
}
extern "C" int rr_batch_clip_restarts_supported(const rr_batch* b, int32_t with_actor) {
  if (!b) return fail(RR_EINVAL, "rr_batch_clip_restarts_supported: null batch");
  return supported("rr_batch_clip_restarts_supported", pose_option_limit(b, F_UNROLL, b->ref_frames, with_actor != 0));
}
extern "C" int rr_batch_set_clip_restarts(rr_batch* b, const rr_clip_restart_io* r) {
  if (!b) return fail(RR_EINVAL, "rr_batch_set_clip_restarts: null batch");
  if (!r) {
    if (b->refr.draws_in) return fail(RR_EINVAL, "rr_batch_set_clip_restarts: the batch carries a reference-restart block (rr_batch_set_reference_restart), which replaces this block's restores: clear it first");
    if (b->has_clip_sampling()) return fail(RR_EINVAL, "rr_batch_set_clip_restarts: the batch carries a clip-sampling block (rr_batch_set_clip_sampling), which counts and draws this block's restores: clear it first");
    if (b->lib.bank_clips) return fail(RR_EINVAL, "rr_batch_set_clip_restarts: the batch carries a clip-library block with bank_clips (rr_batch_set_clip_library), the clips of this block's entries: clear it first");
    b->restart = rr_clip_restart_io{};
    return RR_OK;
  }
  if (const char* why = pose_option_limit(b, F_UNROLL, b->ref_frames, false)) return fail(RR_EUNSUPPORTED, std::string("rr_batch_set_clip_restarts: ") + why);
  if (!b->pose.track_pose) return fail(RR_EINVAL, "rr_batch_set_clip_restarts: needs a pose block (rr_batch_set_pose) first: clip restarts serve pose envs only");
  if (!r->frames || !r->slot_in || !r->slot_out) return fail(RR_EINVAL, "rr_batch_set_clip_restarts: null frames, slot_in or slot_out");
  if (r->num_slots < 1 || r->num_slots > 64) return fail(RR_EINVAL, "rr_batch_set_clip_restarts: num_slots must lie in 1 .. 64");
  b->restart = *r;
  return RR_OK;
}
extern "C" int rr_batch_clip_library_supported(const rr_batch* b, int32_t with_actor) {
  if (!b) return fail(RR_EINVAL, "rr_batch_clip_library_supported: null batch");
  return supported("rr_batch_clip_library_supported", pose_option_limit(b, F_STEP, b->ref_frames, with_actor != 0));
}
extern "C" int rr_batch_set_clip_library(rr_batch* b, const rr_clip_library_io* l) {
  if (!b) return fail(RR_EINVAL, "rr_batch_set_clip_library: null batch");
  if (!l || !l->bank_clips) {
    if (b->samp.clip_weights) return fail(RR_EINVAL, "rr_batch_set_clip_library: the batch carries a clip-sampling block with clip_weights (rr_batch_set_clip_sampling), which weighs this block's bank_clips: clear it first");
  }
  if (!l) { b->lib = rr_clip_library_io{}; return RR_OK; }
  if (const char* why = pose_option_limit(b, F_STEP, b->ref_frames, false)) return fail(RR_EUNSUPPORTED, std::string("rr_batch_set_clip_library: ") + why);
  if (!b->pose.track_pose) return fail(RR_EINVAL, "rr_batch_set_clip_library: needs a pose block (rr_batch_set_pose) first: lengths and clip changes serve pose envs only");
  if (!l->clip_lengths && !l->bank_clips) return fail(RR_EINVAL, "rr_batch_set_clip_library: null clip_lengths and bank_clips (NULL clears the block)");
  if (l->bank_clips && !b->restart.frames) return fail(RR_EINVAL, "rr_batch_set_clip_library: bank_clips needs a clip-restart block (rr_batch_set_clip_restarts) first: they are the clips of its entries");
  if (l->bank_clips && !l->clip_out) return fail(RR_EINVAL, "rr_batch_set_clip_library: bank_clips needs clip_out");
  b->lib = *l;
  return RR_OK;
}
extern "C" int rr_batch_clip_sampling_supported(const rr_batch* b, int32_t with_actor) {
  if (!b) return fail(RR_EINVAL, "rr_batch_clip_sampling_supported: null batch");
  return supported("rr_batch_clip_sampling_supported", pose_option_limit(b, F_UNROLL, b->ref_frames, with_actor != 0));
}
extern "C" int rr_batch_set_clip_sampling(rr_batch* b, const rr_clip_sampling_io* s) {
  if (!b) return fail(RR_EINVAL, "rr_batch_set_clip_sampling: null batch");
  if (!s) { b->samp = rr_clip_sampling_io{}; return RR_OK; }
  if (const char* why = pose_option_limit(b, F_UNROLL, b->ref_frames, false)) return fail(RR_EUNSUPPORTED, std::string("rr_batch_set_clip_sampling: ") + why);
  if (!b->restart.frames) return fail(RR_EINVAL, "rr_batch_set_clip_sampling: needs a clip-restart block (rr_batch_set_clip_restarts) first: it counts and draws that block's restores");
  if (!s->clip_weights && !s->outcomes) return fail(RR_EINVAL, "rr_batch_set_clip_sampling: null clip_weights and outcomes (NULL clears the block)");
  if (s->clip_weights && !b->lib.bank_clips) return fail(RR_EINVAL, "rr_batch_set_clip_sampling: clip_weights needs a clip-library block with bank_clips (rr_batch_set_clip_library) first: the weights are those of the entries' clips");
  if (s->clip_weights && (!s->draws_in || !s->draws_out)) return fail(RR_EINVAL, "rr_batch_set_clip_sampling: clip_weights needs draws_in and draws_out");
  if (s->draws_in && s->draws_in == s->draws_out) return fail(RR_EINVAL, "rr_batch_set_clip_sampling: draws_out may not alias draws_in");
  b->samp = *s;
  return RR_OK;
}
extern "C" int rr_batch_reference_restart_supported(const rr_batch* b, int32_t with_actor) {
  if (!b) return fail(RR_EINVAL, "rr_batch_reference_restart_supported: null batch");
  return supported("rr_batch_reference_restart_supported", pose_option_limit(b, F_UNROLL, b->ref_frames, with_actor != 0));
}
extern "C" int rr_batch_set_reference_restart(rr_batch* b, const rr_reference_restart_io* r) {
  if (!b) return fail(RR_EINVAL, "rr_batch_set_reference_restart: null batch");
  if (!r) { b->refr = rr_reference_restart_io{}; return RR_OK; }
  if (const char* why = pose_option_limit(b, F_UNROLL, b->ref_frames, false)) return fail(RR_EUNSUPPORTED, std::string("rr_batch_set_reference_restart: ") + why);
  if (!b->pose.track_pose) return fail(RR_EINVAL, "rr_batch_set_reference_restart: needs a pose block (rr_batch_set_pose) first: the start state is built from the clip's pose rows");
  if (!b->restart.frames) return fail(RR_EINVAL, "rr_batch_set_reference_restart: needs a clip-restart block (rr_batch_set_clip_restarts) first: it replaces that block's restores");
  if (!r->draws_in || !r->draws_out) return fail(RR_EINVAL, "rr_batch_set_reference_restart: null draws_in or draws_out");
  if (r->draws_in == r->draws_out) return fail(RR_EINVAL, "rr_batch_set_reference_restart: draws_out may not alias draws_in");
  if (r->frame_lo < 0 || r->frame_hi <= r->frame_lo) return fail(RR_EINVAL, "rr_batch_set_reference_restart: needs 0 <= frame_lo < frame_hi");
  if (!(r->noise_scale >= 0.0f) || !std::isfinite(r->noise_scale)) return fail(RR_EINVAL, "rr_batch_set_reference_restart: noise_scale must be finite and >= 0");
  b->refr = *r;
  return RR_OK;
}
extern "C" int32_t rr_batch_obs_width(const rr_batch* b) {
  if (!b) return fail(RR_EINVAL, "rr_batch_obs_width: null batch");
  return b->obs_width();
}
extern "C" int rr_batch_set_env_params(rr_batch* b, const rr_env_params* p) {
  if (!b) return fail(RR_EINVAL, "rr_batch_set_env_params: null batch");
  const rr_dims& d = b->m->dims;
  const bool any = p && (p->dof_f || p->act_f || p->con_f);
  if (any) {
    const Instance in = select(b->m, F_STEP, V_RAND);
    if (!in.kern) return fail(RR_EUNSUPPORTED, std::string("rr_batch_set_env_params: no kernel instance with per-env parameters: ") + in.why);
    if (b->prof) return fail(RR_EUNSUPPORTED, "rr_batch_set_env_params: no profile build on a batch with per-env parameters (rr_batch_set_profile is on)");
    if (b->pose.track_pose) return fail(RR_EUNSUPPORTED, "rr_batch_set_env_params: pose tracking: no pose instance reads per-env parameters (rr_batch_set_pose is on)");
    if (p->num_envs != b->N) return fail(RR_EINVAL, "rr_batch_set_env_params: num_envs differs from the batch's");
    if ((p->dof_f && p->dof_rows != d.nv) || (p->act_f && p->act_rows != d.nu) || (p->con_f && p->con_rows != d.ncon))
      return fail(RR_EINVAL, "rr_batch_set_env_params: row counts must be the model's nv (dof_f), nu (act_f), ncon (con_f)");
  }
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipStreamSynchronize(b->stream));       // launches in flight read the copy that is about to be freed
  float** own[3] = {&b->env_dof_f, &b->env_act_f, &b->env_con_f};
  for (float** o : own) { if (*o) { HIPCHK(hipFree(*o)); *o = nullptr; } }
  if (!any) return RR_OK;
  const float* src[3] = {p->dof_f, p->act_f, p->con_f};
  const size_t bytes[3] = {(size_t)b->N * d.nv * 16 * 4, (size_t)b->N * d.nu * 8 * 4, (size_t)b->N * d.ncon * 26 * 4};
  for (int i = 0; i < 3; ++i) {
    if (!src[i] || !bytes[i]) continue;
    void* q = nullptr;
    HIPCHK(hipMalloc(&q, bytes[i]));
    *own[i] = (float*)q;
    HIPCHK(hipMemcpyAsync(q, src[i], bytes[i], hipMemcpyDeviceToDevice, b->stream));
  }
  HIPCHK(hipStreamSynchronize(b->stream));       // the caller's buffers are free again on return
  return RR_OK;
}

extern "C" int rr_batch_set_schedule(rr_batch* b, const int32_t* env_map, uint32_t* cost_cycles) {
  if (!b) return fail(RR_EINVAL, "rr_batch_set_schedule: null batch");
  b->env_map = env_map; b->cost = cost_cycles;
  return RR_OK;
}

extern "C" int rr_batch_set_ls_repeat_exit(rr_batch* b, int32_t enable) {
  if (!b) return fail(RR_EINVAL, "rr_batch_set_ls_repeat_exit: null batch");
  b->dbg_flags = enable ? (b->dbg_flags & ~RR_DBG_LS_RUN_REPEATS) : (b->dbg_flags | RR_DBG_LS_RUN_REPEATS);
  return RR_OK;
}

extern "C" int rr_batch_set_solver_trim(rr_batch* b, int32_t enable) {
  if (!b) return fail(RR_EINVAL, "rr_batch_set_solver_trim: null batch");
  b->dbg_flags = enable ? (b->dbg_flags & ~RR_DBG_SOLVER_UNTRIMMED) : (b->dbg_flags | RR_DBG_SOLVER_UNTRIMMED);
  return RR_OK;
}

extern "C" int rr_batch_set_solver_batch(rr_batch* b, int32_t enable) {
  if (!b) return fail(RR_EINVAL, "rr_batch_set_solver_batch: null batch");
  b->dbg_flags = enable ? (b->dbg_flags & ~RR_DBG_SOLVER_UNBATCHED) : (b->dbg_flags | RR_DBG_SOLVER_UNBATCHED);
  return RR_OK;
}

extern "C" int rr_model_solve_resident_switch(const rr_model* m) {
  if (!m) return fail(RR_EINVAL, "rr_model_solve_resident_switch: null model");
  const Instance in = select(m, F_STEP, V_MATLDS);
  return in.kern ? RR_OK : fail(RR_EUNSUPPORTED, in.why);
}
extern "C" int rr_batch_set_solve_resident(rr_batch* b, int32_t enable) {
  if (!b) return fail(RR_EINVAL, "rr_batch_set_solve_resident: null batch");
  if (!enable) {
    const int rc = rr_model_solve_resident_switch(b->m);
    if (rc) return rc;
  }
  b->solve_lds = enable == 0;
  return RR_OK;
}

extern "C" int rr_model_root_slot_switch(const rr_model* m) {
  if (!m) return fail(RR_EINVAL, "rr_model_root_slot_switch: null model");
  const Instance in = select(m, F_STEP, V_TWOSLOT);
  return in.kern ? RR_OK : fail(RR_EUNSUPPORTED, in.why);
}
extern "C" int rr_batch_set_root_slot(rr_batch* b, int32_t enable) {
  if (!b) return fail(RR_EINVAL, "rr_batch_set_root_slot: null batch");
  if (!enable) {
    const int rc = rr_model_root_slot_switch(b->m);
    if (rc) return rc;
  }
  b->plain_slots = enable == 0;
  return RR_OK;
}

extern "C" int rr_batch_set_timing(rr_batch* b, int32_t enable) {
  if (!b) return fail(RR_EINVAL, "rr_batch_set_timing: null batch");
  HIPCHK(hipSetDevice(b->device));
  if (enable && b->ev0.empty()) {
    for (int i = 0; i < RR_TIMING_RING; ++i) {
      hipEvent_t a, c;
      HIPCHK(hipEventCreate(&a)); b->ev0.push_back(a);
      HIPCHK(hipEventCreate(&c)); b->ev1.push_back(c);
    }
  }
  b->timing = enable != 0;
  b->total_ms = 0; b->launches = 0; b->npending = 0; b->ring_head = 0;
  return RR_OK;
}
extern "C" int rr_batch_kernel_time(rr_batch* b, double* total_ms, int64_t* launches) {
  if (!b) return fail(RR_EINVAL, "rr_batch_kernel_time: null batch");
  int rc = collect_timing(b);
  if (rc) return rc;
  if (total_ms) *total_ms = b->total_ms;
  if (launches) *launches = b->launches;
  return RR_OK;
}
