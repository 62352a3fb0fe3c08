// rr_step_body.inc -- the body of the step kernel, included by each of its __global__ entries in rr_kernel.h (rr_step_kernel,
// rr_rand_kernel, rr_eval_kernel, rr_pose_kernel, rr_poseterm_kernel, rr_body_kernel, rr_restart_kernel, rr_matlds_kernel, rr_twoslot_kernel).  In scope where it is included: the kernel's five arguments (Dk, Tk, io_kernarg, num_envs, n_frames) and the
// compile-time switches NBS, NVS, NCS, PROF, DBG, DT, NEWTON, UNROLL, ACTOR, PAIR, DYN, RAND, EVAL, POSE, REFOBS, PTERM, BODY, RESTART, MRES, ROOTSLOT.
// Why text and not a function: see the note above rr_step_kernel.
  static_assert(!PAIR || (!PROF && !DBG && !NEWTON && !UNROLL && !ACTOR), "PAIR: production physics instance only");
  static_assert(!DYN || (!PROF && !NEWTON && !PAIR && (!DBG || (!UNROLL && !ACTOR))), "DYN: production instances (single-step, multi-step, multi-step with the actor) and the single-step debug dump");
  static_assert(!ACTOR || UNROLL, "the actor lives in the multi-step instances");
  static_assert(!POSE || (!RAND && !EVAL && !PROF && !DBG && !NEWTON && !PAIR && !DYN), "POSE: production CG instances of the floor-contact models only");
  static_assert(!REFOBS || POSE, "REFOBS: a form of the pose instances (the blocks are rows of track_pose)");
  static_assert(!PTERM || REFOBS, "PTERM: a form of the reference-observation instances (ref_frames 0: no blocks)");
  static_assert(!BODY || PTERM, "BODY: a form of the pose-termination instances (+inf thresholds and a null pose_fail: no termination)");
  static_assert(!RESTART || (BODY && UNROLL), "RESTART: a form of the multi-step body-tracking instances (a null track_bodies: no body terms)");
  static_assert(!EVAL || (ACTOR && !RAND && !PROF && !DBG && !NEWTON && !PAIR), "EVAL: a form of the production multi-step instance with the actor");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  int env = blockIdx.x;
  if (env >= num_envs) return;
  // the level schedules address LDS by absolute byte address: the dynamic segment must start at 0, i.e. the kernel has no static
  // LDS -- checked on the HOST for every instance a batch may launch (rr_batch_create: hipFuncGetAttributes().sharedSizeBytes == 0)
  const DT D(Dk);
  const int wrep = PAIR ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : 0;
  Wave<NBS, NVS, NCS, DT, NEWTON, PAIR, DYN, RAND, !DBG, MRES, ROOTSLOT> w(D, Tk, PAIR ? lds + wrep * (D.lds_bytes_rep >> 2) : lds);
  int lane = threadIdx.x & (RR_LANES - 1);
  if (PAIR) { w.rep = wrep; w.s_xc = lds + 2 * (D.lds_bytes_rep >> 2); }
  RRIO io = load_io();
  if (io.env_map) {          // a permutation of 0 .. num_envs-1 (host-checked length); environments are independent, so the mapping
    env = __builtin_amdgcn_readfirstlane(io.env_map[env]);   // only decides which two of them share a SIMD
    if ((unsigned)env >= (unsigned)num_envs) return;
  }
  if (RAND) w.renv = env;
  if (DBG) {   // the re-read block must be the real parameter, word for word; on a mismatch say so in the dump and touch nothing else
    const RRIO ref_io = io_kernarg;
    bool same = true;
    for (unsigned i = 0; i < sizeof(RRIO) / sizeof(int); ++i) same &= ((const int*)&io)[i] == ((const int*)&ref_io)[i];
    if (ref_io.dbg && lane == 0) ref_io.dbg[(size_t)env * D.dbg_floats + D.g_kaok] = same ? 1.0f : 0.0f;
    if (!same) return;
  }
  int mode = io.mode;            // bits 0-1: RRIO::mode; bit 2 (4): the bad-state flag of the env step being finished (set and cleared below)
  // the debug dump (parity tests) is a separate instance: its paths keep dozens of values alive across the solver
  float* dbg = (DBG && io.dbg) ? io.dbg + (size_t)env * D.dbg_floats : nullptr;     // DBG instance without a dump buffer: contact outputs only

  // wrapper state of a multi-step rollout, wave-uniform
  const int nsteps = UNROLL ? io.unroll_T : 1;
  float u_steps = 0.0f, u_prev_done = 0.0f;
  int u_frame = 0;
  int u_slot = 0;                // RESTART: the bank entry the env's next restore follows (RRIO, CLIP RESTARTS)
  int u_clip = 0;                // RESTART: the clip the env is on, clamped; a restore may move it (RRIO, CLIP LIBRARY); 0 without clip ids
  unsigned u_draws = 0;          // RESTART: restores of the env so far, the counter of the weighted draw's hash (RRIO, CLIP SAMPLING)
  int u_seg = 0;                 // RESTART: wrapped steps of the running episode segment not yet added to the outcome table
  int u_ref = 0;                 // RESTART: a reference restart has staged its start state in LDS, and the next trip of the loop is its forward pass (RRIO, REFERENCE RESTARTS)
  unsigned u_work = 0;
  int u_overflow = 0;            // DYN: some step of this launch dropped pairs (RRIO::cost bit 31 of a multi-step launch)
  if (UNROLL) {
    if (!EVAL || !(io.a_pad & RR_EVAL_RAW)) {      // EVAL without the wrappers: no wrapper state (the pointers may be null)
    u_steps = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(io.steps_in[env])));
    u_prev_done = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(io.prev_done[env])));
    }
    u_frame = __builtin_amdgcn_readfirstlane(io.cur_frame_in[env]);
    if (RESTART) {      // clamped into the bank, so no slot addresses outside it
      const int rk = load_io_member<int>(offsetof(RRIO, restart_K));
      u_slot = __builtin_amdgcn_readfirstlane(load_io_member<const int*>(offsetof(RRIO, restart_slot_in))[env]);
      u_slot = u_slot < 0 ? 0 : (u_slot > rk - 1 ? rk - 1 : u_slot);
      if (const int* cp = load_io_member<const int*>(offsetof(RRIO, clip))) {      // read once: the epilogues below take the id from here
        const int nc = load_io_member<int>(offsetof(RRIO, num_clips));
        u_clip = __builtin_amdgcn_readfirstlane(cp[env]);
        u_clip = u_clip < 0 ? 0 : (u_clip > nc - 1 ? nc - 1 : u_clip);
      }
      if (const int* di = load_io_member<const int*>(offsetof(RRIO, draws_in))) u_draws = (unsigned)__builtin_amdgcn_readfirstlane(di[env]);
    }
  }
  int niter = 0;
  float xq1[4] = {1, 0, 0, 0};   // xquat of body 1 at the last forward pass (obs: xmat[1])
 // A TRIP OF THIS LOOP MAY REPEAT AT THE SAME `ut` (RESTART instances only; RRIO, REFERENCE RESTARTS): a step whose episode ends with a
 // reference restart sets u_ref and takes `ut` back by one at its end, and the next trip (`refpass` below) is the restore's forward pass at
 // that step's index -- mode 2, no actor, no state load, no bad-state check, no wrappers.  Whatever a trip does ONCE PER ENV STEP (counters,
 // pacing, trajectory rows, step bookkeeping) must therefore stand where `refpass` does not reach, i.e. in the wrapper block's `else` arm
 // or behind `!refpass`; today only u_work (the cost report, which counts the pass as the work it is) and the harmless rewrite of the
 // segment's opening row and of the final state see both trips.
 for (int ut = 0; ut < nsteps; ++ut) {
  if (UNROLL) { lane = opaque(lane); w.lane = lane; asm volatile("" : "+s"(env)); if (RAND) w.renv = env; io = load_io(); }
  // REFERENCE RESTARTS: this trip is the forward pass of a restore -- the loop body in mode 2 (no substep, no actor, no wrappers, the
  // reset epilogue) on the state the ended step left in LDS, at the step's own index `ut`, so the observation lands where the step's stood
  const bool refpass = RESTART && u_ref != 0;
  if (RESTART) mode = refpass ? 2 : load_io_member<int>(offsetof(RRIO, mode));
  const RRTables T = w.tables();
  const int senv = PAIR ? 2 * env + wrep : env;      // row of this wave's replica in the state arrays (from the step's own copy of env: see RR_FRAME_LOCAL)
  const size_t ctrl_at = UNROLL ? ((size_t)((EVAL && !(io.a_pad & RR_EVAL_ACTIONS)) ? 0 : ut) * num_envs + env) * D.nu : (size_t)senv * D.nu;
  if (ACTOR && !refpass) {
    if (ut == 0) {       // the observation the rollout starts from is row 0 of the env's trajectory (EVAL: of its two-row ring)
      const int ow = rr_obs_width<REFOBS>(D);      // row stride (REFOBS: with the reference blocks)
      for (int i = lane; i < ow; i += RR_LANES) io.t_obs[(EVAL ? (size_t)env * 2 : rr_traj_obs(io, num_envs, env, 0, 0)) * ow + i] = io.a_obs_in[(size_t)env * ow + i];
      if (EVAL && io.e_qpos_out) for (int i = lane; i < D.nq; i += RR_LANES) io.e_qpos_out[(size_t)env * D.nq + i] = io.qpos_in[(size_t)env * D.nq + i];
    }
    // ORDERING through global memory inside one wave: the observation row the actor reads was written by OTHER lanes of this wave (the
    // previous step's epilogue / the copy above), and the action it writes (lanes < A) is read back as ctrl by all lanes below.  Same-wave
    // vector memory operations complete in order, but the compiler must not move them across each other either: a wavefront-scope fence on
    // both sides states the dependency (guarded by tests/test_gpu_ppo.py::test_one_launch_unroll_with_the_actor_inside, bitwise).
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    rr_actor_step<EVAL, REFOBS ? RR_ACTOR_JM_REFOBS : RR_ACTOR_JM, REFOBS>(io, D, lane, env, ut, num_envs);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  }
  // ---- load state (a multi-step rollout keeps it in LDS after its first step)
  if (!UNROLL || (ut == 0 && !refpass)) {
    for (int i = lane; i < D.nq; i += RR_LANES) w.s_qpos[i] = io.qpos_in[(size_t)senv * D.nq + i];
    for (int i = lane; i < D.nv; i += RR_LANES) w.s_qvel[i] = io.qvel_in[(size_t)senv * D.nv + i];
    for (int i = lane; i < D.nu; i += RR_LANES) w.s_act[i] = io.act_in[(size_t)senv * D.nu + i];
  }
  for (int i = lane; i < D.nu; i += RR_LANES) w.s_ctrl[i] = (io.ctrl && !refpass) ? io.ctrl[ctrl_at + i] : 0.0f;
#pragma unroll
  for (int s = 0; s < NVS; ++s) {
    const int d = lane + RR_LANES * s;
    if ((!UNROLL || (ut == 0 && !refpass)) && d < D.nv) w.s_warm[d] = io.warm_in[(size_t)senv * D.nv + d];
    if (d < D.nv) {
      auto di = row_at(T.dof_i, RR_DOFI, d);
      w.dofc0[s] = (di[3] & 255) | ((di[2] & 15) << 8) | ((di[9] & 15) << 12) | ((di[0] & 255) << 16) | ((row_at(T.body_i, RR_BODYI, di[0])[0] & 255) << 24);
      w.dofc1[s] = (di[4] & 0xFFFF) | (di[10] << 16);
    } else {
      w.dofc0[s] = 255 | (6 << 8);
      w.dofc1[s] = 0;
    }
    w.qacc[s] = w.Ma[s] = w.grad[s] = w.Mgrad[s] = w.search[s] = w.mv[s] = w.qfrc_con[s] = 0.0f;
  }
  w.work = 0;
  if (UNROLL && DYN) w.dyn_overflow = 0;       // per env step: the counter below then counts what the single-step launches would count
  for (int i = lane; i < D.nv; i += RR_LANES) w.s_arm[i] = row_at(T.dof_f, 16, i)[0];
  if (NEWTON) for (int i = lane; i < (D.nM + 3) / 4; i += RR_LANES) ((int*)w.s_anc)[i] = T.anc4[i];
  if (lane < 6) w.s_cdof[6 * D.nv + lane] = 0.0f;
  if (lane == 0) w.s_qvel[D.nv] = 0.0f;
  if (lane < 40) w.s_qLD[2 * D.nM + lane] = 0.0f;        // cells ZERO .. pad, and the 16 zero cells behind them (pairs)
  if (lane < 16) { w.s_vec[D.nv + lane] = 0.0f; w.s_x[D.nv + lane] = 0.0f; }   // zero cells the job descriptors pad with / padded steps read
  w.sync();

  if (PROF) { for (int i = 0; i < RR_NPH; ++i) w.pt[i] = 0; w.pt_last = __builtin_readcyclecounter(); }
  const int frames = (mode & 1) ? n_frames : 1;
  for (int f = 0; f < frames; ++f) {
    // RR_FRAME_LOCAL: everything derived from the lane id / env id (per-lane table addresses, output offsets) is loop-invariant,
    // so the optimiser hoists it out of the substep loop and -- with 256 registers taken -- spills it to scratch at the loop head
    // (45 dwords per lane in round 1's build, reloaded one by one inside every substep).  Re-deriving the two ids through an
    // opaque copy per substep keeps those values local to their phase.
    lane = opaque(lane); w.lane = lane;
    asm volatile("" : "+s"(env));
    if (RAND) w.renv = env;
    const bool last = f == frames - 1;
    if (last) io = load_io();
    float* dg = last ? dbg : nullptr;
    float bias[NVS], passive[NVS];
    w.template stamp<PROF>(15);
    // ---- per-substep (re)load of the model constants from the L2-resident tables.  Holding them in registers across
    // the solver made the allocator spill them to scratch (HBM-side write traffic ~80x the algorithmic bytes); a plain
    // reload costs the same read and no write.  `opaque` keeps the loads inside the substep loop.
    {
      const RRTables T = w.tables();
      const int ol = opaque(lane);
      // ROOTSLOT (Wave::ROOT): slot 0 holds bodies 64 and 65 on lanes 0 and 1; the root, alone in slot 1, needs none of these
      w.bc0 = load_bodyc(T, ROOTSLOT && ol < 2 ? ol + RR_LANES : ol, D.nbody);
      if (NBS > 1 && !ROOTSLOT) w.bc1 = load_bodyc(T, ol + RR_LANES, D.nbody);
#pragma unroll
      for (int s = 0; s < (ROOTSLOT ? 1 : NBS); ++s) {
        const int b = ROOTSLOT && ol < 2 ? ol + RR_LANES : ol + RR_LANES * s;
        const bool ok = b >= 1 && b < D.nbody;
        w.banc[s][0] = ok ? row_at(T.body_anc, 2, b)[0] : 0;
        w.banc[s][1] = ok ? row_at(T.body_anc, 2, b)[1] : 0;
        w.blast[s] = ok ? row_at(T.body_i, RR_BODYI, b)[10] : 0;
      }
    }
    if (lane == 0) {  // world body entries (their LDS cells are reused by later phases of every substep)
      for (int k = 0; k < 6; ++k) w.s_cvel[k] = 0.0f;
      for (int k = 0; k < 10; ++k) w.s_cinert[k] = 0.0f;
      for (int k = 0; k < 3; ++k) w.s_xpos[k] = 0.0f;
      w.s_xquat[0] = 1.0f; w.s_xquat[1] = w.s_xquat[2] = w.s_xquat[3] = 0.0f;
    }
    for (int rep = 0; rep < RR_REP_KIN; ++rep) w.kinematics();
    w.kinematics();
    w.template stamp<PROF>(0);
    w.com_pos();
    w.template stamp<PROF>(1);
    if (last) {   // pose outputs of the last forward pass, before the pose cells are recycled
#pragma unroll
      for (int k = 0; k < 4; ++k) xq1[k] = w.s_xquat[4 + k];
      if (io.o_xpos) for (int e = lane; e < 3 * D.nbody; e += RR_LANES) io.o_xpos[(size_t)env * 3 * D.nbody + e] = w.s_xpos[e];
      if (io.o_xmat || dg) {
        for (int b = lane; b < D.nbody; b += RR_LANES) {
          float q[4], mm[9];
          for (int k = 0; k < 4; ++k) q[k] = w.s_xquat[4 * b + k];
          quat_to_mat(mm, q);
          for (int k = 0; k < 9; ++k) {
            if (io.o_xmat) io.o_xmat[(size_t)env * 9 * D.nbody + 9 * b + k] = mm[k];
            if (dg) dg[D.g_xmat + 9 * b + k] = mm[k];
          }
        }
      }
      if (io.o_com && lane == 0) for (int k = 0; k < 3; ++k) io.o_com[(size_t)env * 3 + k] = w.com0[k];
      // ---- BODY TRACKING, capture (BODY instances, RRIO::track_bodies): the squared distances of the body positions to the clip's row, env
      // steps only.  It stands HERE because s_xpos exists only up to the recycling of its cells later in this substep; the epilogue's
      // terms need S_B and S_E alone, and those travel through body_metrics[env] -- stored by lane 0 now, read back by lane 0 in the
      // epilogue (same thread, program order, as the REFOBS block reads back p_1) -- so nothing of this lives across the solver.  The
      // lanes walk bodies lane, lane + 64, .. from 1 in ascending order; differences, squares, masked products and sums are rounded one by
      // one (contraction off, see POSE TRACKING below).  Clip and frame -- the row the position and pose rewards of this step read -- are
      // clamped before the offset is formed, so no row lies outside track_bodies.  Every member comes by a narrow load.
      if (BODY) {
        const float* tbod = load_io_member<const float*>(offsetof(RRIO, track_bodies));
        if (tbod && !(mode & 2)) {
#pragma clang fp contract(off)
          const float* bwt = load_io_member<const float*>(offsetof(RRIO, body_weights));
          const int blen = load_io_member<int>(offsetof(RRIO, track_len));
          int bc = 0;
          if (const int* bclip = load_io_member<const int*>(offsetof(RRIO, clip))) {
            const int nc = load_io_member<int>(offsetof(RRIO, num_clips));
            bc = RESTART ? u_clip : bclip[env];
            bc = bc < 0 ? 0 : (bc > nc - 1 ? nc - 1 : bc);
          }
          const int bcl = rr_clip_frames<BODY>(bc, blen);      // the clip's own frames; the row stride below stays blen
          int bf = UNROLL ? u_frame : load_io_member<const int*>(offsetof(RRIO, cur_frame_in))[env];
          bf = bf < 0 ? 0 : (bf > bcl - 1 ? bcl - 1 : bf);
          const float* brow = tbod + ((size_t)bc * (size_t)blen + (size_t)bf) * (size_t)(3 * D.nbody);
          float sb = 0.0f, se = 0.0f;
          for (int b = lane; b < D.nbody; b += RR_LANES) {
            if (b >= 1) {
              const float ex = w.s_xpos[3 * b] - brow[3 * b], ey = w.s_xpos[3 * b + 1] - brow[3 * b + 1], ez = w.s_xpos[3 * b + 2] - brow[3 * b + 2];
              const float xx = ex * ex, yy = ey * ey, zz = ez * ez;
              const float e2 = (xx + yy) + zz;
              const float tb = bwt[b] * e2, te = bwt[D.nbody + b] * e2;
              sb = sb + tb; se = se + te;
            }
          }
          sb = wave_sum(sb);
          se = wave_sum(se);
          if (lane == 0) { float* bm = load_io_member<float*>(offsetof(RRIO, body_metrics)) + 2 * (size_t)env; bm[0] = sb; bm[1] = se; }
        }
      }
      if (dg) {
        for (int e = lane; e < 3 * D.nbody; e += RR_LANES) dg[D.g_xpos + e] = w.s_xpos[e];
        for (int e = lane; e < 4 * D.nbody; e += RR_LANES) dg[D.g_xquat + e] = w.s_xquat[e];
        for (int e = lane; e < 10 * D.nbody; e += RR_LANES) dg[D.g_cinert + e] = w.s_cinert[e];
        for (int e = lane; e < 6 * D.nv; e += RR_LANES) dg[D.g_cdof + e] = w.s_cdof[e];
        if (lane == 0) { for (int k = 0; k < 3; ++k) { dg[D.g_com + k] = w.com0[k]; dg[D.g_com + 3 + k] = w.com1[k]; } }
      }
    }
    {   // contact geometry outputs (on request only) are served by the debug-dump instance: the production instances carry no code for them
      float *od = nullptr, *op = nullptr, *of = nullptr;
      if (DBG && last) {
        od = io.o_cdist ? io.o_cdist + (size_t)env * D.ncon : nullptr;
        op = io.o_cpos ? io.o_cpos + (size_t)env * 3 * D.ncon : nullptr;
        of = io.o_cframe ? io.o_cframe + (size_t)env * 9 * D.ncon : nullptr;
      }
      if (DYN) w.contact_geometry_dyn(dg, od, op, of);
      else w.contact_geometry(dg, od, op, of);
    }
    w.velocity_sweep();
    w.template stamp<PROF>(2);
    if (last) {   // cinert / cvel of the last forward pass go out now: cinert's cells become the composite inertia next
      if (io.o_cinert) for (int e = lane; e < 10 * D.nbody; e += RR_LANES) io.o_cinert[(size_t)env * 10 * D.nbody + e] = w.s_cinert[e];
      if (io.o_cvel) for (int e = lane; e < 6 * D.nbody; e += RR_LANES) io.o_cvel[(size_t)env * 6 * D.nbody + e] = w.s_cvel[e];
      if (io.obs) {
        const int ow = rr_obs_width<REFOBS>(D);
        float* ob = (EVAL ? io.t_obs + ((size_t)env * 2 + ((ut + 1) & 1)) * ow : ACTOR ? io.t_obs + rr_traj_obs(io, num_envs, env, rr_traj(io, ut).u, rr_traj(io, ut).t + 1) * ow : io.obs + (size_t)env * ow) + D.nq + D.nv;
        for (int i = lane; i < 10 * (D.nbody - 1); i += RR_LANES) ob[i] = w.s_cinert[10 + i];
        ob += 10 * (D.nbody - 1);
        for (int i = lane; i < 6 * (D.nbody - 1); i += RR_LANES) ob[i] = w.s_cvel[6 + i];
      }
      if (dg) for (int e = lane; e < 6 * D.nbody; e += RR_LANES) dg[D.g_cvel + e] = w.s_cvel[e];
    }
    w.backward_sweep();
    w.template stamp<PROF>(3);
    w.smooth_forces(bias, passive);     // needs cfrc, whose cells the factorisation overwrites
    if (dg) {
      for (int e = lane; e < 10 * D.nbody; e += RR_LANES) dg[D.g_crb + e] = w.s_crb[e];
      // the world body has no cfrc: nothing writes or reads its row, and its cells hold whatever LDS held (the previous substep's qLD, or at the
      // first substep of a launch the previous kernel's data) -- the dump says 0, so that two launches from one state dump the same bits
      for (int e = lane; e < 6 * D.nbody; e += RR_LANES) dg[D.g_cfrc + e] = e < 6 ? 0.0f : w.s_cfrc[e];
    }
    w.contact_jobs();     // J*x jobs of the contacts in penetration: needed from here to the end of the substep
    // WAVE PRIORITY.  2048 environments are exactly one resident round, so a launch lasts as long as its slowest environment,
    // and an environment is slow when many contacts carry force (more J'f terms, more line-search rows).  The heavier of the two
    // waves that share a SIMD issues first; the lighter one has slack.  Four graded levels (0 / 2+ / 6+ / 12+ contacts in
    // penetration): -4.6 % launch time, bit-identical results (tools/variant_bench.py; a two-level split gave -3.1 %).
    w.env_prio();
    w.sync();
    for (int rep = 0; rep < RR_REP_MM; ++rep) w.mass_matrix();
    w.mass_matrix();
    w.template stamp<PROF>(4);
    if (dg) for (int e = lane; e < D.nM; e += RR_LANES) dg[D.g_qM + e] = w.s_qLD[2 * e];
    if (NEWTON) {      // M itself is needed all through the Newton iterations (M * search, H = M + ...): keep a copy of the pair array
      for (int e = lane; e < D.nM + 20; e += RR_LANES) *(rr_f2*)(w.s_Mp + 2 * e) = *(const rr_f2*)(w.s_qLD + 2 * e);
      w.sync();
    }
    {   // the substep's only product with M itself: M * qacc_warmstart, for the solver's warm-start context
      float wv[NVS];
#pragma unroll
      for (int s = 0; s < NVS; ++s) { const int d = lane + RR_LANES * s; wv[s] = d < D.nv ? w.s_warm[d] : 0.0f; }
      w.put_vec(wv);
      w.load_jobs_resident();     // the solve-job descriptors of this substep: read by every product / solve from here to euler()
      w.mul_m(w.Ma_warm);
    }
    // ... and by phase: the two level schedules are one long dependent chain of LDS round trips that issues little; at top priority
    // its instructions go out the moment they are ready (-1.2 ... -1.6 % launch time; the same for the solves, the line-search
    // iterations or the tree sweeps measured +0.3 ... +0.6 % each and +3 % together)
#if RR_FACTOR_PRIO
    if ((w.lag_mode & 8) && w.lag_prio == 0) __builtin_amdgcn_s_setprio(2);
    else __builtin_amdgcn_s_setprio(3);
#endif
    w.factor();
    if (dg) for (int e = lane; e < D.nM; e += RR_LANES) dg[D.g_qLD + e] = w.s_qLD[2 * e];
    w.invert();
    w.env_prio();
    w.load_mat_resident();      // this lane's entries of the inverse factor's M half: read by every undamped solve of the substep
    w.template stamp<PROF>(5);
#pragma unroll
    for (int s = 0; s < NVS; ++s) w.qacc_smooth[s] = w.qfrc_smooth[s];
    w.ldl_solve(w.qacc_smooth);
    w.template stamp<PROF>(6);
    if (dg) {
#pragma unroll
      for (int s = 0; s < NVS; ++s) {
        const int d = lane + RR_LANES * s;
        if (d < D.nv) {
          dg[D.g_dinv + d] = w.dinv[s]; dg[D.g_bias + d] = bias[s]; dg[D.g_passive + d] = passive[s];
          dg[D.g_actuator + d] = w.s_qact[d]; dg[D.g_smooth + d] = w.qfrc_smooth[s];
          dg[D.g_qacc_smooth + d] = w.qacc_smooth[s];
        }
      }
    }
    w.constraint_rows(dg);
    w.template stamp<PROF>(7);
    if (DBG) { w.dbg_flags = io.dbg_flags; w.dbg_ls_ran = w.dbg_ls_left = 0; }
    niter = w.template solve<PROF, DBG>();
    w.template stamp<PROF>(12);
    if (dg) {
#pragma unroll
      for (int s = 0; s < NVS; ++s) {
        const int d = lane + RR_LANES * s;
        if (d < D.nv) { dg[D.g_qacc + d] = w.qacc[s]; dg[D.g_qfrc_constraint + d] = w.qfrc_con[s]; }
      }
      if (lane == 0) {
        dg[D.g_misc] = (float)niter; dg[D.g_misc + 1] = w.cost;
        dg[D.g_ls_iters] = (float)w.dbg_ls_ran; dg[D.g_ls_iters + 1] = (float)w.dbg_ls_left;
        dg[D.g_solver_end] = (float)(w.dbg_solver_end & 1); dg[D.g_solver_end + 1] = (float)(w.dbg_solver_end >> 1);
      }
    }
    if (mode & 1) w.euler();
    w.template stamp<PROF>(13);
    if (UNROLL && !last) {       // pacing at substep granularity (RRIO::pace_mode bit 2)
      const RRIO iop = load_io();
      if (iop.progress && (iop.pace_mode & 4)) {
        unsigned seen = 0;
        if (lane == 0) seen = __hip_atomic_fetch_add(iop.progress, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u;
        seen = (unsigned)__builtin_amdgcn_readfirstlane((int)seen);
        const float behind = ((float)seen / (float)num_envs - (float)(ut * frames + f + 1)) / (float)frames;      // in env steps
        w.lag_prio = behind > iop.pace_t3 ? 3 : (behind > iop.pace_t2 ? 2 : (behind > iop.pace_t1 ? 1 : 0));
        w.lag_mode = iop.pace_mode;
      }
    }
  }

  w.template stamp<PROF>(14);
  lane = opaque(lane); w.lane = lane;
  asm volatile("" : "+s"(env));
  if (RAND) w.renv = env;
  // ---- BAD-STATE CHECK (RRIO::bad_state_max > 0; MuJoCo's mj_checkPos / mj_checkVel): once per env step, on the state after the last
  // substep, never at reset.  The env is bad when some element x of its qpos / qvel fails |x| <= bad_state_max -- written that way round,
  // so NaN and +-inf are bad.  One pass of the lanes over the two LDS vectors and one ballot; the flag is wave-uniform and travels in
  // bit 2 of `mode`, a register that is live anyway, up to the two places below that form `done`.  It stands HERE, before the epilogue
  // re-reads the I/O block, and takes its two members by narrow loads: formed in the observation loops below with the members read from
  // `io`, the flag met the epilogue's register peak and the fixed-dimension multi-step instances went from 83 / 158 to 105 / 172 spilled
  // SGPRs (DESIGN.md section 4i).  Physics-only launches carry no threshold (the host sets it with the env io only).
  if (!PAIR) {
    const float bad_max = load_io_member<float>(offsetof(RRIO, bad_state_max));
    mode &= 3;
    if (bad_max > 0.0f && !(mode & 2)) {
      bool b = false;
      for (int i = lane; i < D.nq; i += RR_LANES) b |= !(fabsf(w.s_qpos[i]) <= bad_max);
      for (int i = lane; i < D.nv; i += RR_LANES) b |= !(fabsf(w.s_qvel[i]) <= bad_max);
      if (__builtin_amdgcn_ballot_w64(b) != 0) {
        mode |= 4;
        if (lane == 0) __hip_atomic_fetch_add(load_io_member<unsigned*>(offsetof(RRIO, bad_states)), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  io = load_io();
  if (PROF && io.prof && lane == 0) for (int i = 0; i < RR_NPH; ++i) io.prof[(size_t)env * RR_NPH + i] = w.pt[i];
  if (UNROLL) u_work += (unsigned)w.work;        // a multi-step launch reports the work of all its steps
  if (UNROLL && DYN) u_overflow |= w.dyn_overflow;
  if (io.cost && lane == 0 && wrep == 0) io.cost[env] = (UNROLL ? u_work : (unsigned)w.work) | (DYN && (UNROLL ? u_overflow : w.dyn_overflow) ? 0x80000000u : 0u);
  if (DYN && w.dyn_overflow && io.dyn_overflow && lane == 0) __hip_atomic_fetch_add(io.dyn_overflow, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // ---- write back state (a multi-step rollout writes it once, after the wrappers of its last step: see below)
  if (!UNROLL) {
    for (int i = lane; i < D.nq; i += RR_LANES) io.qpos[(size_t)senv * D.nq + i] = w.s_qpos[i];
    for (int i = lane; i < D.nv; i += RR_LANES) io.qvel[(size_t)senv * D.nv + i] = w.s_qvel[i];
    for (int i = lane; i < D.nu; i += RR_LANES) io.act[(size_t)senv * D.nu + i] = w.s_act[i];
#pragma unroll
    for (int s = 0; s < NVS; ++s) {
      const int d = lane + RR_LANES * s;
      if (d < D.nv) {
        io.warm[(size_t)senv * D.nv + d] = w.s_warm[d];
        if (io.o_qfrc_actuator) io.o_qfrc_actuator[(size_t)senv * D.nv + d] = w.s_qact[d];
      }
    }
  }

  // ---- reference env epilogue [REF Rodent_Env_Brax.py:103-158]
  if (io.obs) {
    const bool is_reset = (mode & 2) != 0;
    const int old_frame = UNROLL ? u_frame : io.cur_frame_in[env];
    const int new_frame = is_reset ? old_frame : old_frame + 1;
    // multi-clip tracking: the env's clip as the base of both track reads below.  clip[env] is wave-uniform: one load per env step next
    // to cur_frame_in's, the clamp and the offset on the scalar unit, re-read in each epilogue (nothing lives across the solver).  The id
    // is clamped, so none addresses outside the array; the frame clamp below stays per clip.  Null clip: io.track_pos as it is.
    const float* track = io.track_pos;
    if (io.clip) {
      int c = RESTART ? u_clip : io.clip[env];
      c = c < 0 ? 0 : (c > io.num_clips - 1 ? io.num_clips - 1 : c);
      track += (size_t)3 * (size_t)io.track_len * (size_t)c;
    }
    // CLIP LIBRARY (BODY instances): frames of the env's clip, the bound of the two position clamps below and of the clip's end.  Every
    // clamp of this epilogue keeps the expression it has in the other instances, and a BODY instance lowers the result to the clip's
    // last frame behind it (L <= track_len, so the two clamps are one clamp into 0 .. L - 1): the code shared with the other
    // instances is theirs token for token.
    int tlen = io.track_len;
    if (BODY) {
      int tc = 0;
      if (io.clip) { tc = RESTART ? u_clip : io.clip[env]; tc = tc < 0 ? 0 : (tc > io.num_clips - 1 ? io.num_clips - 1 : tc); }
      tlen = rr_clip_frames<BODY>(tc, io.track_len);
    }
    const int ow = rr_obs_width<REFOBS>(D);      // row stride of obs / t_obs / first_obs (REFOBS: with the reference blocks)
    float* ob = EVAL ? io.t_obs + ((size_t)env * 2 + ((ut + 1) & 1)) * ow : ACTOR ? io.t_obs + rr_traj_obs(io, num_envs, env, rr_traj(io, ut).u, rr_traj(io, ut).t + 1) * ow : io.obs + (size_t)env * ow;
    int o = 0;
    for (int i = lane; i < D.nq; i += RR_LANES) ob[o + i] = w.s_qpos[i];
    o += D.nq;
    for (int i = lane; i < D.nv; i += RR_LANES) ob[o + i] = w.s_qvel[i];
    o += D.nv;
    o += 16 * (D.nbody - 1);   // cinert[1:], cvel[1:] were written right after the last forward pass
#pragma unroll
    for (int s = 0; s < NVS; ++s) {
      const int d = lane + RR_LANES * s;
      if (d < D.nv) ob[o + d] = w.s_qact[d];
    }
    o += D.nv;
    if (lane < 3) {  // xmat[1] @ (track_pos[frame + 1] - qpos[:3]); JAX clamps the gather index
      int fi = new_frame + 1;
      fi = fi < 0 ? 0 : (fi > io.track_len - 1 ? io.track_len - 1 : fi);
      if (BODY) fi = fi > tlen - 1 ? tlen - 1 : fi;
      const v3 v = ld3(track + 3 * fi) - ld3(w.s_qpos);
      float m1[9];
      quat_to_mat(m1, xq1);
      // row `lane` of xmat[1] by selects (indexing a register array by the lane id would put it into scratch memory)
      const float r0 = m1[0] * v.x + m1[1] * v.y + m1[2] * v.z, r1 = m1[3] * v.x + m1[4] * v.y + m1[5] * v.z, r2 = m1[6] * v.x + m1[7] * v.y + m1[8] * v.z;
      ob[o + lane] = lane == 0 ? r0 : (lane == 1 ? r1 : r2);
    }
    // ---- REFERENCE OBSERVATION (REFOBS instances, RRIO::ref_frames = H): H blocks of nq entries behind the obs_dim entries above, block h
    // = (p_h[3], q_h[4], j_h[nq - 7]) from the clip's frame f_h = clamp(new_frame + h) -- at reset and after every step alike, a bad step
    // included.  The lanes write the joint part coalesced (one subtraction each); lanes 0 .. 6 form p_h and q_h and pick their entry by
    // selects.  p_h is the track entry's expression at frame f_h.  p_1 is not formed again: lanes 0 .. 2 read back the track entry they
    // have just stored, so the two are the same bits whatever the optimiser contracts.  q_h stands under contraction OFF (see POSE
    // TRACKING below): every product and sum rounded on its own.  Clip and frame are clamped before the row offset is formed, so no row
    // lies outside track_pose; H and the table come by narrow loads here and nothing of this lives across the solver.
    // ISOLATION: the block shares no value with the track entry above -- lane id, row pointer and quaternion pass through opaque copies.
    // Sharing them (one rotation matrix for both, the track entry kept in a register) gave the products of the track entry further uses,
    // and the backend then contracted it differently from every other instance: one ulp in obs[obs_dim - 3 ..], measured against the
    // pose instances.  Apart, the track entry above compiles from the tokens and the uses it has everywhere else.
    if (REFOBS) {
      const int H = load_io_member<int>(offsetof(RRIO, ref_frames));
      const float* tpose = load_io_member<const float*>(offsetof(RRIO, track_pose));
      if (tpose) {
        const int rl = opaque(lane);
        float* rob = ob;
        asm volatile("" : "+s"(rob) : : "memory");
        int rc = 0;
        if (io.clip) { rc = RESTART ? u_clip : io.clip[env]; rc = rc < 0 ? 0 : (rc > io.num_clips - 1 ? io.num_clips - 1 : rc); }
        int rcl = io.track_len;
        if (BODY) rcl = rr_clip_frames<BODY>(rc, io.track_len);
        float xo[4], m1[9];
#pragma unroll
        for (int k = 0; k < 4; ++k) { xo[k] = xq1[k]; asm volatile("" : "+v"(xo[k])); }
        quat_to_mat(m1, xo);
        const float p1 = rl < 3 ? rob[D.obs_dim - 3 + rl] : 0.0f;      // the track entry this lane stored above (same thread: program order)
        for (int h = 1; h <= H; ++h) {
          int fh = new_frame + h;
          fh = fh < 0 ? 0 : (fh > io.track_len - 1 ? io.track_len - 1 : fh);
          if (BODY) fh = fh > rcl - 1 ? rcl - 1 : fh;
          const float* rrow = tpose + ((size_t)rc * (size_t)io.track_len + (size_t)fh) * (size_t)(D.nq - 3);
          float* blk = rob + D.obs_dim + (h - 1) * D.nq;
          for (int i = rl; i < D.nq - 7; i += RR_LANES) blk[7 + i] = rrow[4 + i] - w.s_qpos[7 + i];
          if (rl < 7) {
            const v3 v = ld3(track + 3 * fh) - ld3(w.s_qpos);
            const float r0 = m1[0] * v.x + m1[1] * v.y + m1[2] * v.z, r1 = m1[3] * v.x + m1[4] * v.y + m1[5] * v.z, r2 = m1[6] * v.x + m1[7] * v.y + m1[8] * v.z;
            float qw, qx, qy, qz;
            {
#pragma clang fp contract(off)
              const float xw = xo[0], xx = xo[1], xy = xo[2], xz = xo[3];
              const float rw = rrow[0], rx = rrow[1], ry = rrow[2], rz = rrow[3];
              const float dw = ((xw * rw + xx * rx) + xy * ry) + xz * rz;
              const float d1 = ((xw * rx - xx * rw) - xy * rz) + xz * ry;
              const float d2 = ((xw * ry + xx * rz) - xy * rw) - xz * rx;
              const float d3 = ((xw * rz - xx * ry) + xy * rx) - xz * rw;
              const float sg = dw < 0.0f ? -1.0f : 1.0f;
              qw = sg * dw; qx = sg * d1; qy = sg * d2; qz = sg * d3;
            }
            const float p = h == 1 ? p1 : (rl == 0 ? r0 : (rl == 1 ? r1 : r2));
            const float q = rl == 3 ? qw : (rl == 4 ? qx : (rl == 5 ? qy : qz));
            blk[rl] = rl < 3 ? p : q;
          }
        }
      }
    }
    int pterm_code = 0;      // PTERM instances: the pose-termination code of this step, decided on lane 0, wave-uniform after the lane-0 block
    if (!is_reset) {
      float a2 = 0.0f;
      for (int i = lane; i < D.nu; i += RR_LANES) { const float a = io.ctrl[ctrl_at + i]; a2 += a * a; }
      a2 = wave_sum(a2);
      // ---- POSE TRACKING (POSE instances, RRIO::track_pose): the clip's row [quaternion, joints] at the clip and frame of the position
      // reward.  The lanes read the joint part coalesced, the squared errors are rounded one by one and summed over the wave; lane 0 forms
      // the two terms below.  The members come by narrow loads HERE, for the reason given at the bad-state check above.
      // Roundings: the pose arithmetic stands in blocks with floating-point contraction OFF and uses the plain operators.  __fmul_rn /
      // __fadd_rn are `x * y` / `x + y` in an inline function and carry the translation unit's contraction licence with them: the
      // backend fused weight * exp(..) into the sum that forms the reward (one ulp off the stored metric) until the pragma stood here.
      const float* prow = nullptr;
      float pe2 = 0.0f;
      if (POSE) {
        const float* tpose = load_io_member<const float*>(offsetof(RRIO, track_pose));
        if (tpose) {
#pragma clang fp contract(off)
          int pc = 0;
          if (io.clip) { pc = RESTART ? u_clip : io.clip[env]; pc = pc < 0 ? 0 : (pc > io.num_clips - 1 ? io.num_clips - 1 : pc); }
          int pf = old_frame < 0 ? 0 : (old_frame > io.track_len - 1 ? io.track_len - 1 : old_frame);
          if (BODY) { const int pcl = rr_clip_frames<BODY>(pc, io.track_len); pf = pf > pcl - 1 ? pcl - 1 : pf; }
          prow = tpose + ((size_t)pc * (size_t)io.track_len + (size_t)pf) * (size_t)(D.nq - 3);
          for (int i = lane; i < D.nq - 7; i += RR_LANES) { const float e = w.s_qpos[7 + i] - prow[4 + i]; const float ee = e * e; pe2 = pe2 + ee; }
          pe2 = wave_sum(pe2);
        }
      }
      // ---- VELOCITY TRACKING, sums (BODY instances, RRIO::track_vel): the squared differences of the stepped qvel to the clip's row at
      // the clip and frame of the other rewards, in three sums by dof range -- 0 .. 2 linear, 3 .. 5 angular, 6 .. nv - 1 joints.  The
      // lanes read their dofs of both coalesced (nv = 73: dofs 64 .. 72 are a lane's second pass); every difference, square and sum is
      // rounded on its own (contraction off), a dof outside a range adds +0 to that range's sum, which changes no bit of a sum of
      // squares; one wave sum for the three.  Clip and frame are clamped before the offset is formed, so no row lies outside track_vel.
      // A batch without the block pays the one scalar load and the branch.  ISOLATION: the lane id passes through an opaque copy and
      // nothing here is shared with the pose sums above.
      float vs[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (BODY) {
        const float* tvel = load_io_member<const float*>(offsetof(RRIO, track_vel));
        if (tvel) {
#pragma clang fp contract(off)
          int vc = 0;
          if (io.clip) { vc = RESTART ? u_clip : io.clip[env]; vc = vc < 0 ? 0 : (vc > io.num_clips - 1 ? io.num_clips - 1 : vc); }
          const int vcl = rr_clip_frames<BODY>(vc, io.track_len);
          const int vf = old_frame < 0 ? 0 : (old_frame > vcl - 1 ? vcl - 1 : old_frame);
          const float* vrow = tvel + ((size_t)vc * (size_t)io.track_len + (size_t)vf) * (size_t)D.nv;
          const int vl = opaque(lane);
          for (int i = vl; i < D.nv; i += RR_LANES) {
            const float e = w.s_qvel[i] - vrow[i];
            const float ee = e * e;
            vs[0] = vs[0] + (i < 3 ? ee : 0.0f);
            vs[1] = vs[1] + (i >= 3 && i < 6 ? ee : 0.0f);
            vs[2] = vs[2] + (i >= 6 ? ee : 0.0f);
          }
          wave_sum_n<4>(vs);
        }
      }
      if (lane == 0) {
        int fi = old_frame < 0 ? 0 : (old_frame > io.track_len - 1 ? io.track_len - 1 : old_frame);
        if (BODY) fi = fi > tlen - 1 ? tlen - 1 : fi;
        const v3 dx = ld3(w.s_qpos) - ld3(track + 3 * fi);
        // explicit roundings (no fused multiply-add left to the optimiser), so that the instances of the kernel form the reward from the
        // same operations: single-step and multi-step instances agree bit for bit (tests/test_gpu_env.py); the actor-inside instance to
        // ONE ulp -- `expf` below is expanded inline per instance and its expansion there rounds differently
        // (tests/test_gpu_ppo.py::test_one_launch_unroll_with_the_actor_inside allows exactly that)
        const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx.x, dx.x), __fmul_rn(dx.y, dx.y)), __fmul_rn(dx.z, dx.z));
        const float pos_reward = expf(__fmul_rn(-100.0f, sqrtf(d2)));
        const float z = w.s_qpos[2];
        float healthy = z < io.z_min ? 0.0f : 1.0f;
        if (z > io.z_max) healthy = 0.0f;
        const float hr = io.terminate_when_unhealthy ? io.healthy_reward : __fmul_rn(io.healthy_reward, healthy);
        const float cc = __fmul_rn(io.ctrl_cost_weight, a2);     // explicit roundings: every instance of the kernel forms the reward identically
        const float plain_rew = __fsub_rn(__fadd_rn(pos_reward, hr), cc);   // (left to the optimiser, one instance fused the product into the sum: 1 ulp)
        float rew = plain_rew;
        if (POSE) {
          if (prow) {      // d = conj(r_q) (x) q, theta = 2 atan2(|d.xyz|, |d.w|); every product and sum rounded on its own (contraction off)
#pragma clang fp contract(off)
            const float rw = prow[0], rx = prow[1], ry = prow[2], rz = prow[3];
            const float qw = w.s_qpos[3], qx = w.s_qpos[4], qy = w.s_qpos[5], qz = w.s_qpos[6];
            const float dw = ((rw * qw + rx * qx) + ry * qy) + rz * qz;
            const float dq1 = ((rw * qx - rx * qw) - ry * qz) + rz * qy;
            const float dq2 = ((rw * qy + rx * qz) - ry * qw) - rz * qx;
            const float dq3 = ((rw * qz - rx * qy) + ry * qx) - rz * qw;
            const float dv = sqrtf((dq1 * dq1 + dq2 * dq2) + dq3 * dq3);
            const float theta = 2.0f * atan2f(dv, fabsf(dw));
            const float xq = load_io_member<float>(offsetof(RRIO, pose_quat_k)) * (theta * theta);
            const float quat_rew = load_io_member<float>(offsetof(RRIO, pose_quat_w)) * expf(-xq);
            const float xj = load_io_member<float>(offsetof(RRIO, pose_joint_k)) * pe2;
            const float joint_rew = load_io_member<float>(offsetof(RRIO, pose_joint_w)) * expf(-xj);
            rew = (plain_rew + quat_rew) + joint_rew;
            float* pm = load_io_member<float*>(offsetof(RRIO, pose_metrics)) + 2 * (size_t)env;
            pm[0] = quat_rew; pm[1] = joint_rew;
            // ---- POSE TERMINATION (PTERM instances, RRIO::pose_fail): the three errors against the thresholds.  ISOLATION: d2, theta and
            // pe2 pass through opaque copies, so the reward's expressions above keep the uses -- and with them the contraction -- they
            // have in the pose and reference-observation instances; the compared values are formed again from the copies, contraction
            // off.  `x > +inf` and `NaN > x` are false: an infinite threshold is off, a NaN error belongs to the bad-state check.
            if (PTERM) {
              float cd2 = d2, cth = theta, cpe = pe2;
              asm volatile("" : "+v"(cd2), "+v"(cth), "+v"(cpe));
              const float e_pos = sqrtf(cd2), e_joint = sqrtf(cpe);
              pterm_code = (e_pos > load_io_member<float>(offsetof(RRIO, pose_max_pos)) ? 1 : 0) | (cth > load_io_member<float>(offsetof(RRIO, pose_max_quat)) ? 2 : 0) |
                           (e_joint > load_io_member<float>(offsetof(RRIO, pose_max_joint)) ? 4 : 0);
            }
          }
        }
        // ---- BODY TRACKING, terms (BODY instances): lane 0 reads back the S_B and S_E it parked in body_metrics[env] after the last
        // forward pass and overwrites them with the two terms.  ISOLATION: the reward formed above passes through an opaque copy, so its
        // expressions keep the uses -- and the contraction -- they have in the pose instances; the two sums stand under contraction off.
        if (BODY) {
          if (load_io_member<const float*>(offsetof(RRIO, track_bodies))) {
#pragma clang fp contract(off)
            float* bm = load_io_member<float*>(offsetof(RRIO, body_metrics)) + 2 * (size_t)env;
            float rb = rew;
            asm volatile("" : "+v"(rb));
            const float xb = load_io_member<float>(offsetof(RRIO, body_k)) * bm[0];
            const float body_rew = load_io_member<float>(offsetof(RRIO, body_w)) * expf(-xb);
            const float xe = load_io_member<float>(offsetof(RRIO, endeff_k)) * bm[1];
            const float endeff_rew = load_io_member<float>(offsetof(RRIO, endeff_w)) * expf(-xe);
            rew = (rb + body_rew) + endeff_rew;
            bm[0] = body_rew; bm[1] = endeff_rew;
          }
        }
        // ---- VELOCITY TRACKING, terms (BODY instances): lane 0 forms the three terms from the wave sums above.  ISOLATION as for the
        // body terms: the reward so far passes through an opaque copy, the terms stand under contraction off.
        if (BODY) {
          if (load_io_member<const float*>(offsetof(RRIO, track_vel))) {
#pragma clang fp contract(off)
            float* vm = load_io_member<float*>(offsetof(RRIO, vel_metrics)) + 3 * (size_t)env;
            float rv = rew;
            asm volatile("" : "+v"(rv));
            const float xl = load_io_member<float>(offsetof(RRIO, vel_lin_k)) * vs[0];
            const float lin_rew = load_io_member<float>(offsetof(RRIO, vel_lin_w)) * expf(-xl);
            const float xa = load_io_member<float>(offsetof(RRIO, vel_ang_k)) * vs[1];
            const float ang_rew = load_io_member<float>(offsetof(RRIO, vel_ang_w)) * expf(-xa);
            const float xv = load_io_member<float>(offsetof(RRIO, vel_joint_k)) * vs[2];
            const float jvel_rew = load_io_member<float>(offsetof(RRIO, vel_joint_w)) * expf(-xv);
            rew = ((rv + lin_rew) + ang_rew) + jvel_rew;
            vm[0] = lin_rew; vm[1] = ang_rew; vm[2] = jvel_rew;
          }
        }
        io.reward[env] = rew;
        if (ACTOR && !EVAL) io.t_reward[rr_traj_at(io, num_envs, env, ut)] = rew;
        io.done[env] = io.terminate_when_unhealthy ? 1.0f - healthy : 0.0f;
        io.metrics[3 * env] = pos_reward; io.metrics[3 * env + 1] = -cc; io.metrics[3 * env + 2] = hr;
        io.cur_frame[env] = new_frame;
        // a bad state ends the episode with reward 0 and metrics 0, whatever terminate_when_unhealthy is (state and observation stay as they
        // are).  Written OVER the step's values by a branch of its own: the arithmetic above keeps the code it had without the check
        if (mode & 4) {
          io.reward[env] = 0.0f;
          if (ACTOR && !EVAL) io.t_reward[rr_traj_at(io, num_envs, env, ut)] = 0.0f;
          io.done[env] = 1.0f;
          io.metrics[3 * env] = 0.0f; io.metrics[3 * env + 1] = 0.0f; io.metrics[3 * env + 2] = 0.0f;
          if (POSE) {
            if (prow) { float* pm = load_io_member<float*>(offsetof(RRIO, pose_metrics)) + 2 * (size_t)env; pm[0] = 0.0f; pm[1] = 0.0f; }
          }
          if (BODY) {
            if (load_io_member<const float*>(offsetof(RRIO, track_bodies))) { float* bm = load_io_member<float*>(offsetof(RRIO, body_metrics)) + 2 * (size_t)env; bm[0] = 0.0f; bm[1] = 0.0f; }
            if (load_io_member<const float*>(offsetof(RRIO, track_vel))) { float* vm = load_io_member<float*>(offsetof(RRIO, vel_metrics)) + 3 * (size_t)env; vm[0] = 0.0f; vm[1] = 0.0f; vm[2] = 0.0f; }
          }
          if (PTERM) pterm_code = 0;      // a bad step: done = 1 from the check above, code 0
        }
        // pose termination changes nothing but done: raised OVER the step's value, as the bad-state branch does
        if (PTERM) {
          if (float* pf = load_io_member<float*>(offsetof(RRIO, pose_fail))) pf[env] = (float)pterm_code;
          if (pterm_code != 0) io.done[env] = 1.0f;
        }
      }
      if (PTERM) pterm_code = __builtin_amdgcn_readfirstlane(pterm_code);      // lane 0's value in every lane: done_env below is formed by all of them
    }
    if (RESTART && refpass) {
      // REFERENCE RESTARTS: the pass has written the restored state's observation over the ended step's; what that step left to it
      // follows -- the row that opens the next segment, and the state of the launch's last step (after the pass, as a reset stores it)
      u_ref = 0;
      if (ACTOR && !EVAL) {
        const RRTraj tr = rr_traj(io, ut);
        if (tr.t + 1 == io.a_seg && ut + 1 < nsteps) {
          float* nx = io.t_obs + rr_traj_obs(io, num_envs, env, tr.u + 1, 0) * ow;
          for (int i = lane; i < ow; i += RR_LANES) nx[i] = ob[i];
        }
      }
      if (ut == nsteps - 1) {
        for (int i = lane; i < D.nq; i += RR_LANES) io.qpos[(size_t)env * D.nq + i] = w.s_qpos[i];
        for (int i = lane; i < D.nv; i += RR_LANES) { io.qvel[(size_t)env * D.nv + i] = w.s_qvel[i]; io.warm[(size_t)env * D.nv + i] = w.s_warm[i]; }
        for (int i = lane; i < D.nu; i += RR_LANES) io.act[(size_t)env * D.nu + i] = w.s_act[i];
      }
    } else if (UNROLL) {
      // EpisodeWrapper + AutoResetWrapper on the step just made (action_repeat 1), as rr_wrap_kernel applies them:
      // steps' = (prev_done ? 0 : steps) + 1; over = steps' >= episode_length; done <- over ? 1 : done; truncation = over ? 1 - done_env : 0;
      // where done, the stored first state and first observation come back (info -- cur_frame, steps -- is not restored)
      // RESTART: the clip's end joins `over`, and the state, the observation AND the frame come back from the next entry of the bank
      const float z = w.s_qpos[2];
      const float healthy = (z < io.z_min || z > io.z_max) ? 0.0f : 1.0f;
      const float done_own = (mode & 4) ? 1.0f : (io.terminate_when_unhealthy ? 1.0f - healthy : 0.0f);
      const float done_env = (PTERM && pterm_code != 0) ? 1.0f : done_own;      // PTERM: a pose failure is a termination (trunc 0, discount 0, restore)
      const bool wrapped = !EVAL || !(io.a_pad & RR_EVAL_RAW);      // EVAL without the wrappers: the env's own done, no step count, no restore
      if (wrapped) u_steps = (u_prev_done != 0.0f ? 0.0f : u_steps) + 1.0f;
      bool over = wrapped && u_steps >= io.episode_length;
      if (RESTART) {      // new_frame >= L - 1, L the frames of the clip the step was made on: the new state's observation has no next frame left to read without clamping
        if (load_io_member<int>(offsetof(RRIO, restart_end)) != 0 && new_frame >= tlen - 1) over = true;
      }
      const float done2 = over ? 1.0f : done_env, trunc = over ? 1.0f - done_env : 0.0f;
      u_prev_done = done2;
      u_frame = new_frame;
      if (ACTOR && !EVAL && lane == 0) { const size_t at = rr_traj_at(io, num_envs, env, ut); io.t_discount[at] = 1.0f - done2; io.t_trunc[at] = trunc; }
      if (EVAL) {
        // brax EvalWrapper on the step just made, in place: episode_steps += active; sums += metric * active; active *= 1 - done (the
        // wrapped done).  Lane 0 reads the step's metrics back from where it has just stored them and updates the env's six cells in
        // memory: nothing of this lives across the solver.  Products and sums rounded one by one -- the operations torch performs.
        if (io.e_metrics && lane == 0) {
          float* em = io.e_metrics + (size_t)env * 6;
          const float active = em[1];
          em[0] = __fadd_rn(em[0], active);
          em[2] = __fadd_rn(em[2], __fmul_rn(io.metrics[3 * env], active));
          em[3] = __fadd_rn(em[3], __fmul_rn(io.metrics[3 * env + 1], active));
          em[4] = __fadd_rn(em[4], __fmul_rn(io.metrics[3 * env + 2], active));
          em[5] = __fadd_rn(em[5], __fmul_rn(io.reward[env], active));
          em[1] = __fmul_rn(active, __fsub_rn(1.0f, done2));
        }
        if (io.e_qpos_out) for (int i = lane; i < D.nq; i += RR_LANES) io.e_qpos_out[((size_t)(ut + 1) * num_envs + env) * D.nq + i] = w.s_qpos[i];
      }
      if (RESTART) {
        const bool ended = __builtin_amdgcn_readfirstlane(__float_as_int(done2)) != 0;
        // CLIP SAMPLING, outcome counters: on the clip the step was made on (u_clip moves below).  The segment's steps are flushed with the
        // episode's end and with the launch's last step
        if (long long* oc = load_io_member<long long*>(offsetof(RRIO, outcomes))) {
          u_seg = u_seg + 1;
          if (ended || ut == nsteps - 1) {
            if (lane == 0) {
              long long* row = oc + 5 * (size_t)u_clip;
              __hip_atomic_fetch_add(row + 4, (long long)u_seg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              if (ended) {
                const int col = (PTERM && pterm_code != 0) ? 1 : (done_env != 0.0f ? 2 : 3);
                __hip_atomic_fetch_add(row, 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_add(row + col, 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              }
            }
            u_seg = 0;
          }
        }
        if (ended) {
          // CLIP SAMPLING, weighted restore: the slot drawn by the env's bank weights; the next slot without a table or with S == 0
          const bool refr = load_io_member<int>(offsetof(RRIO, rref_on)) != 0;      // REFERENCE RESTARTS: no bank entry is read
          const unsigned rn = u_draws;
          int drawn = -1;
          if (!refr) {      // (a reference restart draws a clip, not a slot: the weights are read below)
            if (const int* cw = load_io_member<const int*>(offsetof(RRIO, clip_weights))) {
              if (const int* wbc = load_io_member<const int*>(offsetof(RRIO, bank_clips)))
                drawn = rr_weighted_slot(cw, wbc, load_io_member<int>(offsetof(RRIO, restart_K)), load_io_member<int>(offsetof(RRIO, num_clips)), env, num_envs,
                                         load_io_member<unsigned>(offsetof(RRIO, sample_seed)), u_draws, lane);
            }
          }
          u_draws = u_draws + 1u;
          u_slot = u_slot + 1;
          if (u_slot >= load_io_member<int>(offsetof(RRIO, restart_K))) u_slot = 0;
          if (drawn >= 0) u_slot = drawn;
          if (refr) {
            // REFERENCE RESTARTS (RRIO): clip and frame drawn here, wave-uniform and in integers; the start state built in LDS from the
            // clip's rows plus noise; the forward pass and the observation are the next trip of the loop (refpass).  Clip and frame are
            // clamped before a row offset is formed, so no row lies outside the arrays or at or behind the clip's own end.
            const unsigned base = rr_ref_base(load_io_member<unsigned>(offsetof(RRIO, rref_seed)), env, rn);
            const int nc = load_io_member<int>(offsetof(RRIO, num_clips));
            int c = u_clip;
            if (load_io_member<int>(offsetof(RRIO, rref_across)) != 0 && load_io_member<const int*>(offsetof(RRIO, clip)) && nc >= 1)
              c = rr_ref_clip(load_io_member<const int*>(offsetof(RRIO, clip_weights)), nc, rr_ref_hash(base, 1u, 0u), opaque(lane));
            const int flo = load_io_member<int>(offsetof(RRIO, rref_lo)), fhi = load_io_member<int>(offsetof(RRIO, rref_hi));
            int f = flo + (int)(((unsigned long long)rr_ref_hash(base, 2u, 0u) * (unsigned long long)(unsigned)(fhi - flo)) >> 32);
            const int tl = load_io_member<int>(offsetof(RRIO, track_len));
            const int cl = rr_clip_frames<BODY>(c, tl);
            if (load_io_member<const int*>(offsetof(RRIO, clip_len))) f = cl > 1 ? (int)((unsigned)f % (unsigned)(cl - 1)) : 0;
            const int fr = f < 0 ? 0 : (f > cl - 1 ? cl - 1 : f);
            u_clip = c; u_frame = f;
            const size_t rrow = (size_t)c * (size_t)tl + (size_t)fr;
            const float* rp = load_io_member<const float*>(offsetof(RRIO, track_pos)) + rrow * 3;
            const float* rq = load_io_member<const float*>(offsetof(RRIO, track_pose)) + rrow * (size_t)(D.nq - 3);
            const float* rv = load_io_member<const float*>(offsetof(RRIO, track_vel));
            const float ns = load_io_member<float>(offsetof(RRIO, rref_noise));
            const int rl = opaque(lane);
            w.sync();
            {      // one rounded product and one rounded sum per element: contraction off and the plain operators (__fmul_rn / __fadd_rn carry the
                   // translation unit's contraction licence, see POSE TRACKING above), and the product passes through an opaque copy
#pragma clang fp contract(off)
              for (int i = rl; i < D.nq; i += RR_LANES) {
                const float row = i < 3 ? rp[i] : rq[i - 3];
                float nz = ns * rr_ref_unit(rr_ref_hash(base, 3u, (unsigned)i));
                asm volatile("" : "+v"(nz));
                w.s_qpos[i] = row + nz;
              }
              for (int i = rl; i < D.nv; i += RR_LANES) {
                const float row = rv ? rv[rrow * (size_t)D.nv + i] : 0.0f;
                float nz = ns * rr_ref_unit(rr_ref_hash(base, 4u, (unsigned)i));
                asm volatile("" : "+v"(nz));
                w.s_qvel[i] = row + nz;
                w.s_warm[i] = 0.0f;
              }
            }
            for (int i = rl; i < D.nu; i += RR_LANES) w.s_act[i] = 0.0f;
            w.sync();
            u_ref = 1;
          } else {      // the bank restore: state, observation, frame and clip of entry u_slot
            const size_t re = (size_t)u_slot * (size_t)num_envs + (size_t)env;      // row of the bank entry in every [K][N][width] array
            u_frame = __builtin_amdgcn_readfirstlane(load_io_member<const int*>(offsetof(RRIO, restart_frames))[re]);
            if (const int* bcl = load_io_member<const int*>(offsetof(RRIO, bank_clips))) {      // CLIP LIBRARY: the entry's clip, clamped
              const int nc = load_io_member<int>(offsetof(RRIO, num_clips));
              const int c = __builtin_amdgcn_readfirstlane(bcl[re]);
              u_clip = c < 0 ? 0 : (c > nc - 1 ? nc - 1 : c);
            }
            w.sync();
            for (int i = lane; i < D.nq; i += RR_LANES) w.s_qpos[i] = io.first_qpos[re * D.nq + i];
            for (int i = lane; i < D.nv; i += RR_LANES) { w.s_qvel[i] = io.first_qvel[re * D.nv + i]; w.s_warm[i] = io.first_warm[re * D.nv + i]; }
            for (int i = lane; i < D.nu; i += RR_LANES) w.s_act[i] = io.first_act[re * D.nu + i];
            for (int i = lane; i < ow; i += RR_LANES) ob[i] = io.first_obs[re * ow + i];
            w.sync();
          }
        }
      } else if (wrapped && __builtin_amdgcn_readfirstlane(__float_as_int(done2)) != 0) {
        w.sync();
        for (int i = lane; i < D.nq; i += RR_LANES) w.s_qpos[i] = io.first_qpos[(size_t)env * D.nq + i];
        for (int i = lane; i < D.nv; i += RR_LANES) { w.s_qvel[i] = io.first_qvel[(size_t)env * D.nv + i]; w.s_warm[i] = io.first_warm[(size_t)env * D.nv + i]; }
        for (int i = lane; i < D.nu; i += RR_LANES) w.s_act[i] = io.first_act[(size_t)env * D.nu + i];
        for (int i = lane; i < ow; i += RR_LANES) ob[i] = io.first_obs[(size_t)env * ow + i];
        w.sync();
      }
      if (ACTOR && !EVAL) {      // the last observation of a segment is also the first of the next one (the learner's trajectories overlap by one row)
        const RRTraj tr = rr_traj(io, ut);
        if (tr.t + 1 == io.a_seg && ut + 1 < nsteps) {
          float* nx = io.t_obs + rr_traj_obs(io, num_envs, env, tr.u + 1, 0) * ow;
          for (int i = lane; i < ow; i += RR_LANES) nx[i] = ob[i];
        }
      }
      if (io.progress && ut + 1 < nsteps) {
        unsigned seen = 0;
        if (lane == 0) seen = __hip_atomic_fetch_add(io.progress, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u;
        seen = (unsigned)__builtin_amdgcn_readfirstlane((int)seen);
        const float per_step = (io.pace_mode & 4) ? (float)frames : 1.0f;          // the counter's units per env step
        const float behind = ((float)seen / (float)num_envs) / per_step - (float)(ut + 1);      // env steps behind the average environment
        w.lag_prio = behind > io.pace_t3 ? 3 : (behind > io.pace_t2 ? 2 : (behind > io.pace_t1 ? 1 : 0));
        w.lag_mode = io.pace_mode;
      }
      if (ut == nsteps - 1) {
        if (lane == 0) { io.done[env] = done2; if (wrapped) { io.steps_out[env] = u_steps; io.trunc_out[env] = trunc; } }
        if (RESTART) {      // the frame and the slot the next launch goes on from (lane 0 stored new_frame above: program order)
          if (lane == 0) { io.cur_frame[env] = u_frame; load_io_member<int*>(offsetof(RRIO, restart_slot_out))[env] = u_slot; }
          if (lane == 0) { if (int* co = load_io_member<int*>(offsetof(RRIO, clip_out))) co[env] = u_clip; }      // CLIP LIBRARY: the clip the next launch goes on from
          if (lane == 0) { if (int* dro = load_io_member<int*>(offsetof(RRIO, draws_out))) dro[env] = (int)u_draws; }      // CLIP SAMPLING: the restore count likewise
        }
        for (int i = lane; i < D.nq; i += RR_LANES) io.qpos[(size_t)env * D.nq + i] = w.s_qpos[i];
        for (int i = lane; i < D.nv; i += RR_LANES) { io.qvel[(size_t)env * D.nv + i] = w.s_qvel[i]; io.warm[(size_t)env * D.nv + i] = w.s_warm[i]; }
        for (int i = lane; i < D.nu; i += RR_LANES) io.act[(size_t)env * D.nu + i] = w.s_act[i];
      }
      // REFERENCE RESTARTS: the restore's forward pass is the next trip, at this step's index (what the three blocks above wrote of the
      // ended step's state and observation, the pass writes again)
      if (RESTART) { if (u_ref != 0) ut = ut - 1; }
    }
  }
 }     // ut
