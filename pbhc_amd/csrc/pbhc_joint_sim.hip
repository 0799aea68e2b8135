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
// Everything but the joint law — the loads, the draws, the delayed action, the torque, the root row, the contact rule, the stores and the
// entry's argument checks — is pbhc_closed_loop.h, shared with k_articulated_sim.  Here lane = dof.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <math.h>

#include "../../include/pbhc_hip.h"
#include "pbhc_math.h"

using namespace pbhc;

#undef PBHC_STAMPS                                          // (the phase stamps of the diagnostic build belong to the step kernel's unit)
#include "pbhc_env_step.h"                                  // PBHC_G, at, clampf, frame_blend, slerp, rng_uniform / rng_normal
#include "pbhc_closed_loop.h"

__global__ __launch_bounds__(PBHC_G* CL_EPB) void k_joint_sim(const PbhcEnvConfig* __restrict__ cfgp, PbhcMotionTable tbl, PbhcStepIO io, PbhcJointSimParams p,
                                                              const double* __restrict__ glob, int N) {
  ClCfg& c = *(ClCfg*)cfgp;
  const int D = c.skel.num_dof;
  const int lane = threadIdx.x & (PBHC_G - 1);
  ClFront F;
  cl_load_env(F, c, io, glob, N, lane, min(lane, D - 1));
  const float inertia = p.inertia[F.dc], damping = p.damping[F.dc];
  __builtin_amdgcn_sched_barrier(0);
  cl_load_rows<false>(F, c, tbl);
  __builtin_amdgcn_sched_barrier(0);
  cl_control(F, c, io);

  // ---- the sub-steps (legged_robot_base.py:287-295): torque from the current (q, v), semi-implicit Euler with the passive damping implicit
  float q = F.q, v = F.v;
  const float h = c.sim_dt;
  const float den = 1.0f + h * damping / inertia;
  float tq0 = 0.0f;
  for (int s = 0; s < p.decimation; ++s) {
    const float tq = cl_torque(F, c, q, v);
    if (s == 0) tq0 = tq;
    v = (v + h * tq / inertia) / den;
    q = q + h * v;
    if (p.enforce_limits) {
      if (q < F.lo) { q = F.lo; if (v < 0.0f) v = 0.0f; }
      else if (q > F.hi) { q = F.hi; if (v > 0.0f) v = 0.0f; }
    }
  }

  f4 qs;
  const float rootv = cl_root(F, qs);
  cl_store_frame(F, c, io, lane < D, q, v, tq0, p.tau0, rootv, p.foot_height_threshold, p.contact_force);
}

extern "C" int pbhc_sizeof_joint_sim_params(void) { return (int)sizeof(PbhcJointSimParams); }

extern "C" int pbhc_joint_sim_step(PbhcEnv* e, const PbhcStepIO* io, const PbhcJointSimParams* p, void* stream) {
  CL_CHECK(p);
  const PbhcEnvConfig *hc = nullptr, *dcfg = nullptr;
  const PbhcMotionTable* tbl = nullptr;
  double* glob = nullptr;
  const int rc = cl_check_step(e, io, p->decimation, &hc, &dcfg, &tbl, &glob);
  if (rc != PBHC_OK) return rc;
  const int D = hc->skel.num_dof, N = hc->num_envs;
  CL_CHECK(D <= PBHC_G);
  for (int d = 0; d < D; ++d) CL_CHECK(p->inertia[d] > 0.0f && p->damping[d] >= 0.0f);
  hipLaunchKernelGGL(k_joint_sim, dim3((N + CL_EPB - 1) / CL_EPB), dim3(PBHC_G * CL_EPB), 0, (hipStream_t)stream, dcfg, *tbl, *io, *p,
                     (const double*)glob, N);
  if (hipGetLastError() != hipSuccess) {
    snprintf(g_pbhc_err, sizeof(g_pbhc_err), "pbhc_joint_sim_step: launch failed");
    return PBHC_EHIP;
  }
  return PBHC_OK;
}
