// pbhc_closed_loop.h — what the closed-loop simulators' kernels (k_joint_sim, k_articulated_sim) share: everything in front of the joint law
// and behind it, and their entries' argument checks.  Included after pbhc_env_step.h (PBHC_G, at, clampf, frame_blend, slerp, rng_*).
//
// Both kernels run 32 lanes per env, 8 envs per 256-thread workgroup, the tail workgroup's missing envs clamped to env N - 1 and masked at the
// stores; they differ in the dof a lane holds (`dc`: min(lane, D - 1) in k_joint_sim; min(max(lane - 1, 0), D - 1) in k_articulated_sim, where
// lane = body).  They read what the previous step left — dof_state, the action queue and delay index (PEEKED: the step still owns and shifts
// the queue), the DR scales, the per-env default angles — and the new actions.  Every load is issued before the first dependent use, in three
// phases: cl_load_env and the kernel's own loads, a __builtin_amdgcn_sched_barrier(0) in the kernel, cl_load_rows, another barrier.
// The units that include this file are built with the step kernel's flags: cl_torque is the step's `torques`, operation for operation.
#pragma once

#define CL_EPB 8                                            // envs per 256-thread workgroup: 32 lanes per env
#define CL_MAX_DECIMATION 64

typedef const PbhcEnvConfig __attribute__((address_space(4))) ClCfg;

struct ClFront {                                            // what a lane holds in front of the joint law
  int D, B, Bx, NF, Q;                                      // the config's sizes, read in front of the first barrier
  int lane, env, envc, dc, mid, sl, foot;                   // envc: the env clamped to N - 1; dc: the lane's dof, clamped
  bool valid;
  unsigned int eDc, step_ctr;                               // eDc = envc * D
  long long ep1, adelay;
  float start, org, a_in, q, v, kp, kd, rfs, ras, u_inj, n_inj, k_dp, tl, k_pg, k_dg, k_as, lo, hi, qold[PBHC_MAX_QUEUE];
  float blend, rr0, rr1, cc0, cc1;                          // the root component and the contact source of the rows round tref
  float blend_p, ss0, ss1;                                  // PREV only: the root component of the rows round tref - dt
  float u_rfi, n_ps, a_sc;                                  // cl_control
};

// the lane's place, then phases (1) and (2) of the loads
__device__ __forceinline__ void cl_load_env(ClFront& F, ClCfg& c, const PbhcStepIO& io, const double* __restrict__ glob, int N, int lane, int dc) {
  typedef unsigned int u32;
  const int D = c.skel.num_dof, B = c.skel.num_bodies, Bx = c.skel.num_bodies_ext, NF = c.num_feet, Q = max(c.queue_len, 1);
  F.D = D; F.B = B; F.Bx = Bx; F.NF = NF; F.Q = Q;
  const int env = blockIdx.x * CL_EPB + (int)(threadIdx.x / PBHC_G), envc = env < N ? env : N - 1;
  const u32 eDc = (u32)envc * (u32)D;
  F.lane = lane; F.env = env; F.valid = env < N; F.envc = envc; F.dc = dc; F.eDc = eDc;
  // (1) the env scalars the reference rows' addresses hang on
  F.ep1 = (long long)io.episode_length_buf[envc] + 1;
  F.start = io.motion_start_times[envc];
  F.mid = (int)io.motion_ids[envc];
  // (2) everything that depends on the env index only
  F.step_ctr = (uint32_t)glob[PBHC_G_STEP_COUNTER];
  F.adelay = io.action_delay_idx[envc];
  F.org = at(io.env_origins, (u32)envc * 3u + (u32)min(lane, 2));
  F.a_in = at(io.actions_in, eDc + dc);
  F.q = at(io.dof_state, (eDc + dc) * 2); F.v = at(io.dof_state, (eDc + dc) * 2 + 1);
  F.kp = at(io.kp_scale, eDc + dc); F.kd = at(io.kd_scale, eDc + dc); F.rfs = at(io.rfi_lim_scale, eDc + dc); F.ras = at(io.rao_scale, eDc + dc);
  F.u_inj = at(io.u_rfi ? io.u_rfi : io.actions_in, eDc + dc);
  F.k_dp = io.default_dof_pos ? at(io.default_dof_pos, eDc + dc) : c.default_dof_pos[dc];
#pragma unroll
  for (int k = 0; k < PBHC_MAX_QUEUE; ++k) F.qold[k] = at(io.action_queue, (u32)envc * (u32)(Q * D) + (u32)(min(k, Q - 1) * D) + (u32)dc);
  F.sl = c.ps_tau ? c.ps_tau_slot[dc] : -1;
  F.n_inj = (F.sl >= 0 && io.ovr_ps_tau) ? at(io.ovr_ps_tau, (u32)envc * (u32)c.ps_tau_num + (u32)F.sl) : 0.0f;
  F.tl = c.torque_limits[dc]; F.k_pg = c.p_gains[dc]; F.k_dg = c.d_gains[dc]; F.k_as = c.action_scale[dc];
  F.lo = c.hard_dof_pos_limits[dc][0]; F.hi = c.hard_dof_pos_limits[dc][1];
  F.foot = c.feet[min(lane, max(NF, 1) - 1)];
}

// phase (3), once (1) is back: one root component per lane (lanes 0..12), one contact source per lane (lanes < NF), of the two rows round the
// step's reference time; PREV: the root component of the two rows round tref - dt as well (the articulated base's accelerations)
template <bool PREV>
__device__ __forceinline__ void cl_load_rows(ClFront& F, ClCfg& c, const PbhcMotionTable& tbl) {
  const int D = F.D, Bx = F.Bx, lane = F.lane;
  const int o_pos = 2 * D + 2, o_rot = o_pos + 3 * Bx, o_vel = o_rot + 4 * Bx, o_ang = o_vel + 3 * Bx;     // columns of a packed motion-table row
  float m_len = tbl.single_len, m_dt = tbl.single_dt;
  int m_nf = tbl.single_num_frames, m_row0 = 0;
  if (tbl.num_motions != 1) { m_len = tbl.motion_len[F.mid]; m_nf = tbl.num_frames[F.mid]; m_dt = tbl.motion_dt[F.mid]; m_row0 = tbl.length_starts[F.mid]; }
  const float tref = (float)(F.ep1 + 1) * c.dt + F.start;     // the step's own reference time (motion_tracking.py:554,588), from the pre-step counter
  int f0, f1, g0 = 0, g1 = 0;
  frame_blend(tref, m_len, m_nf, m_dt, &f0, &f1, &F.blend);
  if (PREV) frame_blend(tref - c.dt, m_len, m_nf, m_dt, &g0, &g1, &F.blend_p);
  const float* r0 = tbl.frames + (size_t)(m_row0 + f0) * tbl.row;
  const float* r1 = tbl.frames + (size_t)(m_row0 + f1) * tbl.row;
  const int lr = min(lane, 12);
  const int rcol = lr < 3 ? o_pos + lr : (lr < 7 ? o_rot + (lr - 3) : (lr < 10 ? o_vel + (lr - 7) : o_ang + (lr - 10)));     // body 0 of the row
  const int ccol = c.has_contact_mask ? 2 * D + min(lane, 1) : o_pos + 3 * F.foot + 2;
  F.rr0 = r0[rcol]; F.rr1 = r1[rcol]; F.cc0 = r0[ccol]; F.cc1 = r1[ccol];
  if (PREV) {
    const float* s0 = tbl.frames + (size_t)(m_row0 + g0) * tbl.row;
    const float* s1 = tbl.frames + (size_t)(m_row0 + g1) * tbl.row;
    F.ss0 = s0[rcol]; F.ss1 = s1[rcol];
  }
}

// the draws of this control step (computed while the loads fly), held over the sub-steps: Philox stream 1 (RFI) and 19 (parallel_serial_tau)
// keyed (seed, env, step counter, stream, dof) as the step itself will draw them, the step counter read from the globals where k_env_step
// reads it (the launch sits in front of the step on its stream), or the injected io.u_rfi / io.ovr_ps_tau.  The key's dof is the CLAMPED
// `dc`: on every lane whose result is stored that is the lane's dof.  Then the action the step will apply (pbhc_env_step.h,
// _pre_physics_step), scaled: clipped, then the queue entry the delay index names AFTER the step's shift — the new action for index 0, else
// the entry one place in front of it as the queue stands now.
__device__ __forceinline__ void cl_control(ClFront& F, ClCfg& c, const PbhcStepIO& io) {
  typedef unsigned int u32;
  F.u_rfi = 0.5f; F.n_ps = 0.0f;
  if (c.randomize_torque_rfi) F.u_rfi = io.u_rfi ? F.u_inj : rng_uniform(c.seed, (u32)F.env, F.step_ctr, 1, (u32)F.dc);
  if (F.sl >= 0) F.n_ps = io.ovr_ps_tau ? F.n_inj : rng_normal(c.seed, (u32)F.env, F.step_ctr, 19, (u32)F.dc);
  float delayed = clampf(F.a_in, -c.action_clip_value, c.action_clip_value);
  if (c.randomize_ctrl_delay) {
    const int didx = (int)F.adelay;
#pragma unroll
    for (int k = 1; k < PBHC_MAX_QUEUE; ++k)
      if (k < F.Q && k == didx) delayed = F.qold[k - 1];
  }
  F.a_sc = delayed * F.k_as;
}

// the torque law of one sub-step (legged_robot_base.py:795-838), from the current (q, v): k_env_step's expression, operation for operation
__device__ __forceinline__ float cl_torque(const ClFront& F, ClCfg& c, float q, float v) {
  float tq;
  if (c.control_type == 0) tq = F.kp * F.k_pg * (F.a_sc + F.k_dp - q) - F.kd * F.k_dg * v;
  else tq = F.a_sc;                                            // "T" ("V" is refused by the host)
  if (c.randomize_torque_rfi) tq = tq + (F.u_rfi * 2.0f - 1.0f) * c.rfi_lim * F.rfs * F.tl;
  if (F.sl >= 0) tq = tq + (c.ps_tau_rfi_lim * F.tl) * F.n_ps;
  if (c.use_rao) tq = tq + F.ras * F.tl;
  if (c.clip_torques) tq = clampf(tq, -F.tl, F.tl);
  return tq;
}

// root state: lerp / slerp of the root body's two rows, exactly motion_lookup's expressions (k_motion_state): lanes 0..12 each hold one
// component of the row (pos 3, rot 4, vel 3, ang 3), the quaternion is handed round by __shfl.  -> the lane's component; `qs`: the slerp
__device__ __forceinline__ float cl_root(const ClFront& F, f4& qs) {
  const float al = 1.0f - F.blend, blend = F.blend, rr0 = F.rr0, rr1 = F.rr1;
  const f4 q0 = mk4(__shfl(rr0, 3, PBHC_G), __shfl(rr0, 4, PBHC_G), __shfl(rr0, 5, PBHC_G), __shfl(rr0, 6, PBHC_G));
  const f4 q1 = mk4(__shfl(rr1, 3, PBHC_G), __shfl(rr1, 4, PBHC_G), __shfl(rr1, 5, PBHC_G), __shfl(rr1, 6, PBHC_G));
  qs = slerp(q0, q1, blend);
  if (F.lane < 3) return al * rr0 + blend * rr1 + F.org;
  if (F.lane < 7) return F.lane == 3 ? qs.x : (F.lane == 4 ? qs.y : (F.lane == 5 ? qs.z : qs.w));
  return al * rr0 + blend * rr1;
}

// the frame (the window is the simulator's own: one frame, [1, N, ...]), plain vector stores.  `own`: the lane holds a dof of the robot, `dc`
// unclamped.  Contact: the clip's lerped mask, or the foot's reference height where the library has no masks.
__device__ __forceinline__ void cl_store_frame(const ClFront& F, ClCfg& c, const PbhcStepIO& io, bool own, float q, float v, float tq0, float* tau0,
                                               float rootv, float foot_height_threshold, float contact_force) {
  typedef unsigned int u32;
  const float cl = (1.0f - F.blend) * F.cc0 + F.blend * F.cc1;
  const bool touch = c.has_contact_mask ? cl > 0.5f : cl < foot_height_threshold;
  if (!F.valid) return;
  if (own) {
    at(const_cast<float*>(io.frame_dof_pos), F.eDc + (u32)F.dc) = q;
    at(const_cast<float*>(io.frame_dof_vel), F.eDc + (u32)F.dc) = v;
    if (tau0) at(tau0, F.eDc + (u32)F.dc) = tq0;
  }
  if (F.lane < 13) at(const_cast<float*>(io.frame_root), (u32)F.envc * 13u + (u32)F.lane) = rootv;
  if (F.lane < F.NF)
    at(const_cast<float*>(io.frame_contact), (u32)F.envc * (u32)(F.B * 3) + (u32)(3 * F.foot + 2)) = touch ? contact_force : 0.0f;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
extern thread_local char g_pbhc_err[512];
extern "C" int pbhc_env_parts(PbhcEnv* e, const PbhcEnvConfig** host_cfg, const PbhcEnvConfig** dev_cfg, const PbhcMotionTable** tbl,
                              double** glob);                  // pbhc_kernels.hip

#define CL_CHECK(cnd)                                                                                              \
  do {                                                                                                             \
    if (!(cnd)) {                                                                                                  \
      snprintf(g_pbhc_err, sizeof(g_pbhc_err), "%s:%d bad argument: %s", __FILE__, __LINE__, #cnd);                \
      return PBHC_EINVAL;                                                                                          \
    }                                                                                                              \
  } while (0)

// what both pbhc_*_sim_step entries ask of their arguments before anything of their own; -> the env's parts
static int cl_check_step(PbhcEnv* e, const PbhcStepIO* io, int decimation, const PbhcEnvConfig** hc, const PbhcEnvConfig** dcfg,
                         const PbhcMotionTable** tbl, double** glob) {
  CL_CHECK(e && io);
  const int rc = pbhc_env_parts(e, hc, dcfg, tbl, glob);
  if (rc != PBHC_OK) return rc;
  CL_CHECK(io->actions_in && io->frame_root && io->frame_dof_pos && io->frame_dof_vel && io->frame_contact && io->num_frames == 1);
  CL_CHECK(io->dof_state && io->action_queue && io->action_delay_idx && io->kp_scale && io->kd_scale && io->rfi_lim_scale && io->rao_scale);
  CL_CHECK(io->episode_length_buf && io->motion_start_times && io->motion_ids && io->env_origins);
  CL_CHECK(((((uintptr_t)io->episode_length_buf | (uintptr_t)io->motion_ids | (uintptr_t)io->action_delay_idx) & 7) == 0));     // int64 elements
  CL_CHECK(decimation >= 1 && decimation <= CL_MAX_DECIMATION);
  CL_CHECK((*hc)->control_type == 0 || (*hc)->control_type == 2);      // "V" needs last_dof_vel per sub-step: refused
  const int D = (*hc)->skel.num_dof, B = (*hc)->skel.num_bodies, N = (*hc)->num_envs, NF = (*hc)->num_feet;
  CL_CHECK(N >= 1 && D >= 1 && NF >= 0 && NF <= PBHC_MAX_FEET);
  for (int f = 0; f < NF; ++f) CL_CHECK((*hc)->feet[f] >= 0 && (*hc)->feet[f] < B);
  CL_CHECK((uint64_t)N * (uint64_t)(3 * B > 2 * D ? 3 * B : 2 * D) < (1ull << 30));          // 32-bit row offsets in the kernels
  return PBHC_OK;
}
