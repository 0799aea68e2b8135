// pbhc_joint_sim.hip — the closed-loop joint-space simulator (pbhc_amd/simulator/joint_sim.py JointSpaceSim).
//
//   k_joint_sim   one launch per control step on the stepping stream, directly in front of k_env_step (and in front of k_dof_far_any, which
//                 reads the frame the step will read).  It writes the ONE-frame replay window that the unchanged step kernel then consumes
//                 through its frame_* pointers: the robot hangs on a gantry — the root is carried along the clip's own root trajectory at the
//                 step's reference time — and every joint obeys  I_d q'' = tau_d - b_d q'  under the env's own PD law, integrated over the
//                 control_decimation physics sub-steps with the torque re-evaluated in every sub-step, as the reference's _physics_step does
//                 (legged_robot_base.py:287-295,795-838).  No gravity, no coupling between joints, no contact dynamics: this is NOT a physics
//                 engine, it closes the loop action -> torque -> joint state -> observation.
//
// What it reads is what the previous step left (post-reset): dof_state, the action queue and delay index (PEEKED: the step still owns and shifts
// the queue), the DR scales, the per-env default angles; and the new actions.  The per-control-step torque noise is the draw the step itself
// will make — Philox stream 1 (RFI) and 19 (parallel_serial_tau) keyed (seed, env, step counter, stream, dof), the step counter read from the
// globals where k_env_step reads it (the launch sits in front of the step on its stream: the same ordering guarantees), or the injected
// io.u_rfi / io.ovr_ps_tau — held over the sub-steps.  So the first sub-step's torque is the step's `torques` output, operation for operation.
//
// Mapping, as k_dof_far_any: 32 lanes per env, lane = dof, 8 envs per 256-thread workgroup, the tail workgroup's missing envs clamped to env
// N - 1 and masked at the stores.  Every load is issued before the first dependent use: (1) the env scalars the table rows' addresses hang on,
// (2) everything that depends on the env index only, (3) — once (1) is back — the two table rows.  Lanes 0..12 each hold one component of the
// root body's row (pos 3, rot 4, vel 3, ang 3); the quaternion is handed round by __shfl for the slerp.  Outputs are plain vector stores.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <math.h>

#include "../../include/pbhc_hip.h"
#include "pbhc_math.h"

using namespace pbhc;

extern thread_local char g_pbhc_err[512];
extern "C" int pbhc_env_parts(PbhcEnv* e, const PbhcEnvConfig** host_cfg, const PbhcEnvConfig** dev_cfg, const PbhcMotionTable** tbl,
                              double** glob);                  // pbhc_kernels.hip

#undef PBHC_STAMPS                                          // (the phase stamps of the diagnostic build belong to the step kernel's unit)
#include "pbhc_env_step.h"                                  // PBHC_G, at, clampf, frame_blend, slerp, rng_uniform / rng_normal

#define JSIM_EPB 8                                          // envs per 256-thread workgroup: 32 lanes per env
#define JSIM_MAX_DECIMATION 64

__global__ __launch_bounds__(PBHC_G* JSIM_EPB) void k_joint_sim(const PbhcEnvConfig* __restrict__ cfgp, PbhcMotionTable tbl, PbhcStepIO io, PbhcJointSimParams p,
                                                                const double* __restrict__ glob, int N) {
  typedef const PbhcEnvConfig __attribute__((address_space(4))) ConstCfg;
  ConstCfg& c = *(ConstCfg*)cfgp;
  typedef unsigned int u32;
  const int D = c.skel.num_dof, B = c.skel.num_bodies, Bx = c.skel.num_bodies_ext, NF = c.num_feet, Q = max(c.queue_len, 1);
  const int lane = threadIdx.x & (PBHC_G - 1);
  const int env = blockIdx.x * JSIM_EPB + (int)(threadIdx.x / PBHC_G);
  const bool valid = env < N;
  const int envc = valid ? env : N - 1;
  const int dc = min(lane, D - 1);
  const u32 eDc = (u32)envc * (u32)D;
  const int o_pos = 2 * D + 2, o_rot = o_pos + 3 * Bx, o_vel = o_rot + 4 * Bx, o_ang = o_vel + 3 * Bx;     // columns of a packed motion-table row

  // (1) the env scalars the reference rows' addresses hang on
  const long long ep1 = (long long)io.episode_length_buf[envc] + 1;
  const float start = io.motion_start_times[envc];
  const int mid = (int)io.motion_ids[envc];
  // (2) everything that depends on the env index only
  const uint32_t step_ctr = (uint32_t)glob[PBHC_G_STEP_COUNTER];
  const long long adelay = io.action_delay_idx[envc];
  const float org = at(io.env_origins, (u32)envc * 3u + (u32)min(lane, 2));
  const float a_in = at(io.actions_in, eDc + dc);
  float q = at(io.dof_state, (eDc + dc) * 2), v = at(io.dof_state, (eDc + dc) * 2 + 1);
  const float kp = at(io.kp_scale, eDc + dc), kd = at(io.kd_scale, eDc + dc), rfs = at(io.rfi_lim_scale, eDc + dc), ras = at(io.rao_scale, eDc + dc);
  const float u_inj = at(io.u_rfi ? io.u_rfi : io.actions_in, eDc + dc);
  const float k_dp = io.default_dof_pos ? at(io.default_dof_pos, eDc + dc) : c.default_dof_pos[dc];
  float qold[PBHC_MAX_QUEUE];
#pragma unroll
  for (int k = 0; k < PBHC_MAX_QUEUE; ++k) qold[k] = at(io.action_queue, (u32)envc * (u32)(Q * D) + (u32)(min(k, Q - 1) * D) + (u32)dc);
  const int sl = c.ps_tau ? c.ps_tau_slot[dc] : -1;
  const float n_inj = (sl >= 0 && io.ovr_ps_tau) ? at(io.ovr_ps_tau, (u32)envc * (u32)c.ps_tau_num + (u32)sl) : 0.0f;
  const float tl = c.torque_limits[dc], k_pg = c.p_gains[dc], k_dg = c.d_gains[dc], k_as = c.action_scale[dc];
  const float lim_lo = c.hard_dof_pos_limits[dc][0], lim_hi = c.hard_dof_pos_limits[dc][1];
  const float inertia = p.inertia[dc], damping = p.damping[dc];
  const int foot = c.feet[min(lane, max(NF, 1) - 1)];
  __builtin_amdgcn_sched_barrier(0);
  // (3) the two table rows: one root component per lane (lanes 0..12), one contact source per lane (lanes < NF)
  float m_len = tbl.single_len, m_dt = tbl.single_dt;
  int m_nf = tbl.single_num_frames, m_row0 = 0;
  if (tbl.num_motions != 1) { m_len = tbl.motion_len[mid]; m_nf = tbl.num_frames[mid]; m_dt = tbl.motion_dt[mid]; m_row0 = tbl.length_starts[mid]; }
  const float tref = (float)(ep1 + 1) * c.dt + start;         // the step's own reference time (motion_tracking.py:554,588), from the pre-step counter
  int f0, f1;
  float blend;
  frame_blend(tref, m_len, m_nf, m_dt, &f0, &f1, &blend);
  const float* r0 = tbl.frames + (size_t)(m_row0 + f0) * tbl.row;
  const float* r1 = tbl.frames + (size_t)(m_row0 + f1) * tbl.row;
  const int lr = min(lane, 12);
  const int rcol = lr < 3 ? o_pos + lr : (lr < 7 ? o_rot + (lr - 3) : (lr < 10 ? o_vel + (lr - 7) : o_ang + (lr - 10)));     // body 0 of the row
  const int ccol = c.has_contact_mask ? 2 * D + min(lane, 1) : o_pos + 3 * foot + 2;
  const float rr0 = r0[rcol], rr1 = r1[rcol], cc0 = r0[ccol], cc1 = r1[ccol];
  __builtin_amdgcn_sched_barrier(0);

  // ---- the draws of this control step (computed while the loads fly), held over the sub-steps
  float u_rfi = 0.5f, n_ps = 0.0f;
  if (c.randomize_torque_rfi) u_rfi = io.u_rfi ? u_inj : rng_uniform(c.seed, (u32)env, step_ctr, 1, (u32)lane);
  if (sl >= 0) n_ps = io.ovr_ps_tau ? n_inj : rng_normal(c.seed, (u32)env, step_ctr, 19, (u32)lane);

  // ---- the action the step will apply (pbhc_env_step.h, _pre_physics_step): clipped, then the queue entry the delay index names AFTER the
  // step's shift — the new action for index 0, else the entry one place in front of it as the queue stands now
  const float a = clampf(a_in, -c.action_clip_value, c.action_clip_value);
  float delayed = a;
  if (c.randomize_ctrl_delay) {
    const int didx = (int)adelay;
#pragma unroll
    for (int k = 1; k < PBHC_MAX_QUEUE; ++k)
      if (k < Q && k == didx) delayed = qold[k - 1];
  }
  const float a_sc = delayed * k_as;

  // ---- the sub-steps (legged_robot_base.py:287-295): torque from the current (q, v), semi-implicit Euler with the passive damping implicit
  const float h = c.sim_dt;
  const float den = 1.0f + h * damping / inertia;
  float tq0 = 0.0f;
  for (int s = 0; s < p.decimation; ++s) {
    float tq;
    if (c.control_type == 0) tq = kp * k_pg * (a_sc + k_dp - q) - kd * k_dg * v;
    else tq = a_sc;                                            // "T" ("V" is refused by the host)
    if (c.randomize_torque_rfi) tq = tq + (u_rfi * 2.0f - 1.0f) * c.rfi_lim * rfs * tl;
    if (sl >= 0) tq = tq + (c.ps_tau_rfi_lim * tl) * n_ps;
    if (c.use_rao) tq = tq + ras * tl;
    if (c.clip_torques) tq = clampf(tq, -tl, tl);
    if (s == 0) tq0 = tq;
    v = (v + h * tq / inertia) / den;
    q = q + h * v;
    if (p.enforce_limits) {
      if (q < lim_lo) { q = lim_lo; if (v < 0.0f) v = 0.0f; }
      else if (q > lim_hi) { q = lim_hi; if (v > 0.0f) v = 0.0f; }
    }
  }

  // ---- root state: lerp / slerp of the root body's two rows, exactly motion_lookup's expressions (k_motion_state)
  const float al = 1.0f - blend;
  const f4 q0 = mk4(__shfl(rr0, 3, PBHC_G), __shfl(rr0, 4, PBHC_G), __shfl(rr0, 5, PBHC_G), __shfl(rr0, 6, PBHC_G));
  const f4 q1 = mk4(__shfl(rr1, 3, PBHC_G), __shfl(rr1, 4, PBHC_G), __shfl(rr1, 5, PBHC_G), __shfl(rr1, 6, PBHC_G));
  const f4 qs = slerp(q0, q1, blend);
  float rootv;
  if (lane < 3) rootv = al * rr0 + blend * rr1 + org;
  else if (lane < 7) rootv = lane == 3 ? qs.x : (lane == 4 ? qs.y : (lane == 5 ? qs.z : qs.w));
  else rootv = al * rr0 + blend * rr1;
  // ---- contact: the clip's lerped mask, or the foot's reference height where the library has no masks
  const float cl = al * cc0 + blend * cc1;
  const bool touch = c.has_contact_mask ? cl > 0.5f : cl < p.foot_height_threshold;

  float* f_root = const_cast<float*>(io.frame_root);           // the window is the simulator's own: one frame, [1, N, ...]
  float* f_q = const_cast<float*>(io.frame_dof_pos);
  float* f_qd = const_cast<float*>(io.frame_dof_vel);
  float* f_c = const_cast<float*>(io.frame_contact);
  if (valid) {
    if (lane < D) {
      at(f_q, eDc + (u32)lane) = q;
      at(f_qd, eDc + (u32)lane) = v;
      if (p.tau0) at(p.tau0, eDc + (u32)lane) = tq0;
    }
    if (lane < 13) at(f_root, (u32)envc * 13u + (u32)lane) = rootv;
    if (lane < NF) at(f_c, (u32)envc * (u32)(B * 3) + (u32)(3 * foot + 2)) = touch ? p.contact_force : 0.0f;
  }
}

extern "C" int pbhc_sizeof_joint_sim_params(void) { return (int)sizeof(PbhcJointSimParams); }

#define JSIM_CHECK(cnd)                                                                                            \
  do {                                                                                                             \
    if (!(cnd)) {                                                                                                  \
      snprintf(g_pbhc_err, sizeof(g_pbhc_err), "%s:%d bad argument: %s", __FILE__, __LINE__, #cnd);                \
      return PBHC_EINVAL;                                                                                          \
    }                                                                                                              \
  } while (0)

extern "C" int pbhc_joint_sim_step(PbhcEnv* e, const PbhcStepIO* io, const PbhcJointSimParams* p, void* stream) {
  JSIM_CHECK(e && io && p);
  const PbhcEnvConfig *hc = nullptr, *dcfg = nullptr;
  const PbhcMotionTable* tbl = nullptr;
  double* glob = nullptr;
  const int rc = pbhc_env_parts(e, &hc, &dcfg, &tbl, &glob);
  if (rc != PBHC_OK) return rc;
  JSIM_CHECK(io->actions_in && io->frame_root && io->frame_dof_pos && io->frame_dof_vel && io->frame_contact && io->num_frames == 1);
  JSIM_CHECK(io->dof_state && io->action_queue && io->action_delay_idx && io->kp_scale && io->kd_scale && io->rfi_lim_scale && io->rao_scale);
  JSIM_CHECK(io->episode_length_buf && io->motion_start_times && io->motion_ids && io->env_origins);
  JSIM_CHECK(p->decimation >= 1 && p->decimation <= JSIM_MAX_DECIMATION);
  JSIM_CHECK(hc->control_type == 0 || hc->control_type == 2);          // "V" needs last_dof_vel per sub-step: refused
  const int D = hc->skel.num_dof, B = hc->skel.num_bodies, N = hc->num_envs;
  JSIM_CHECK(N >= 1 && D >= 1 && D <= PBHC_G && hc->num_feet >= 0 && hc->num_feet <= PBHC_MAX_FEET);
  for (int f = 0; f < hc->num_feet; ++f) JSIM_CHECK(hc->feet[f] >= 0 && hc->feet[f] < B);
  for (int d = 0; d < D; ++d) JSIM_CHECK(p->inertia[d] > 0.0f && p->damping[d] >= 0.0f);
  JSIM_CHECK((uint64_t)N * (uint64_t)(3 * B > 2 * D ? 3 * B : 2 * D) < (1ull << 30));          // 32-bit row offsets in the kernel
  hipLaunchKernelGGL(k_joint_sim, dim3((N + JSIM_EPB - 1) / JSIM_EPB), dim3(PBHC_G * JSIM_EPB), 0, (hipStream_t)stream, dcfg, *tbl, *io, *p,
                     (const double*)glob, N);
  if (hipGetLastError() != hipSuccess) {
    snprintf(g_pbhc_err, sizeof(g_pbhc_err), "pbhc_joint_sim_step: launch failed");
    return PBHC_EHIP;
  }
  return PBHC_OK;
}
