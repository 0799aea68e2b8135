// pbhc_articulated_sim.hip — the articulated rigid-body simulator (pbhc_amd/simulator/articulated_sim.py ArticulatedSim).
//
//   k_articulated_sim   one launch per control step, where k_joint_sim sits (directly in front of k_env_step on the stepping stream), writing the
//                       same one-frame replay window.  Root, contact, the delayed-action peek, the torque law and its draws are k_joint_sim's:
//                       the shared part lives in pbhc_closed_loop.h (here lane = body and lane b owns dof b - 1).  Only the joint law differs:
//                       every sub-step solves  (M(q) + diag(armature + h b)) dv = h (tau - b v - c(q, v; base))  on the robot's tree with the
//                       MJCF's masses, centres of mass and inertia tensors; the base (the root row this kernel writes) is prescribed.
//   k_art_debug         test-only: the same device function (art_substep) under a constant torque.
//
// The forward dynamics (art_substep<false>: the base prescribed) is shared with the floating-base simulator: pbhc_art_dynamics.h.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <math.h>

#include "../../include/pbhc_hip.h"
#include "pbhc_math.h"

using namespace pbhc;

#undef PBHC_STAMPS                                          // (the phase stamps of the diagnostic build belong to the step kernel's unit)
#include "pbhc_env_step.h"                                  // PBHC_G, at, clampf, frame_blend, slerp, rng_uniform / rng_normal
#include "pbhc_closed_loop.h"                               // CL_EPB, ClFront and the cl_* pieces, CL_CHECK, cl_check_step

#include "pbhc_art_dynamics.h"                             // sym3 / mat3, ArtTree, ArtSkel, ArtLane, ArtBase, art_substep, art_tree, art_skel

__global__ __launch_bounds__(PBHC_G* CL_EPB) void k_articulated_sim(const PbhcEnvConfig* __restrict__ cfgp, PbhcMotionTable tbl, PbhcStepIO io,
                                                                    PbhcArticulatedParams p, ArtTree tree, const double* __restrict__ glob, int N) {
  ClCfg& c = *(ClCfg*)cfgp;
  typedef unsigned int u32;
  const int D = c.skel.num_dof, B = c.skel.num_bodies;
  const int lane = threadIdx.x & (PBHC_G - 1);
  const bool joint = lane >= 1 && lane < B;                  // lane = body; its hinge is dof lane - 1
  ClFront F;
  cl_load_env(F, c, io, glob, N, lane, min(max(lane - 1, 0), D - 1));
  const int dc = F.dc;
  const float h = c.sim_dt;
  ArtLane L;
  L.lo = F.lo; L.hi = F.hi;
  L.parent = max(c.skel.parent[lane], 0);
  L.depth = joint ? c.skel.depth[lane] : (lane == 0 ? 0 : -1);
  L.first_child = tree.first_child[lane]; L.next_sibling = tree.next_sibling[lane];
  L.off = mk3(c.skel.offset[lane][0], c.skel.offset[lane][1], c.skel.offset[lane][2]);
  L.lq = mk4(c.skel.local_rot_wxyz[lane][1], c.skel.local_rot_wxyz[lane][2], c.skel.local_rot_wxyz[lane][3], c.skel.local_rot_wxyz[lane][0]);
  {
    const f3 ax = mk3(c.skel.dof_axis[dc][0], c.skel.dof_axis[dc][1], c.skel.dof_axis[dc][2]);     // normalised as the FK's (skel_word)
    L.axis = mul3(ax, 1.0f / fmaxf(norm3(ax), 1e-9f));
  }
  art_lane_inertial(L, p, lane, dc, h);
  __builtin_amdgcn_sched_barrier(0);
  cl_load_rows<true>(F, c, tbl);                             // with the rows at tref - dt, for the base acceleration
  __builtin_amdgcn_sched_barrier(0);
  cl_control(F, c, io);

  // ---- the base: R_0, w_0 of the root row; a_0, alpha_0 from the row one control step earlier (lanes 7..12: one component each)
  f4 qs;
  const float rootv = cl_root(F, qs);
  const float racc = p.base_acceleration ? (rootv - ((1.0f - F.blend_p) * F.ss0 + F.blend_p * F.ss1)) / c.dt : 0.0f;
  ArtBase base;
  base.R0 = quat_unit_fast(qs);
  base.w0 = mk3(shf(rootv, 10), shf(rootv, 11), shf(rootv, 12));
  base.alpha0 = mk3(shf(racc, 10), shf(racc, 11), shf(racc, 12));
  base.a0g = mk3(shf(racc, 7) - p.gravity[0], shf(racc, 8) - p.gravity[1], shf(racc, 9) - p.gravity[2]);

  // ---- the sub-steps (legged_robot_base.py:287-295): torque from the current (q, v), then the tree's forward dynamics
  float q = F.q, v = F.v;
  if (!joint) { q = 0.0f; v = 0.0f; }
  float tq0 = 0.0f;
  ArtFloat none;                                             // (the floating base's part: not touched with FREE = false)
  for (int s = 0; s < p.decimation; ++s) {
    const float tq = cl_torque(F, c, q, v);
    if (s == 0) tq0 = tq;
    art_substep<false>(L, tree, base, none, lane, h, tq, p.enforce_limits != 0, q, v);
  }

  cl_store_frame(F, c, io, joint, q, v, tq0, p.tau0, rootv, p.foot_height_threshold, p.contact_force);
  if (F.valid && p.base_acc && lane >= 7 && lane < 13) at(p.base_acc, (u32)F.envc * 6u + (u32)(lane - 7)) = racc;
}

__global__ __launch_bounds__(PBHC_G* CL_EPB) void k_art_debug(ArtSkel sk, PbhcArticulatedParams p, ArtTree tree, const float* __restrict__ basep,
                                                               const float* __restrict__ qp, const float* __restrict__ vp, const float* __restrict__ taup,
                                                               int n, int steps, float h, int enforce_limits, float* __restrict__ out_q,
                                                               float* __restrict__ out_v, float* __restrict__ out_qdd0) {
  typedef unsigned int u32;
  const int B = sk.num_bodies, D = B - 1;
  const int lane = threadIdx.x & (PBHC_G - 1);
  const int env = blockIdx.x * CL_EPB + (int)(threadIdx.x / PBHC_G);
  const bool valid = env < n;
  const int envc = valid ? env : n - 1;
  const int dc = min(max(lane - 1, 0), D - 1);
  const bool joint = lane >= 1 && lane < B;
  const u32 eDc = (u32)envc * (u32)D;
  ArtLane L;
  L.lo = sk.limits[lane][0]; L.hi = sk.limits[lane][1];
  L.parent = max(sk.parent[lane], 0);
  L.depth = joint ? sk.depth[lane] : (lane == 0 ? 0 : -1);
  L.first_child = tree.first_child[lane]; L.next_sibling = tree.next_sibling[lane];
  L.off = mk3(sk.offset[lane][0], sk.offset[lane][1], sk.offset[lane][2]);
  L.lq = mk4(sk.lq_xyzw[lane][0], sk.lq_xyzw[lane][1], sk.lq_xyzw[lane][2], sk.lq_xyzw[lane][3]);
  L.axis = mk3(sk.axis[lane][0], sk.axis[lane][1], sk.axis[lane][2]);
  art_lane_inertial(L, p, lane, dc, h);
  const float* bp = basep + (size_t)envc * 13;
  ArtBase base;
  base.R0 = quat_unit_fast(mk4(bp[0], bp[1], bp[2], bp[3]));
  base.w0 = mk3(bp[4], bp[5], bp[6]);
  base.alpha0 = mk3(bp[7], bp[8], bp[9]);
  base.a0g = mk3(bp[10] - p.gravity[0], bp[11] - p.gravity[1], bp[12] - p.gravity[2]);
  float q = at(qp, eDc + dc), v = at(vp, eDc + dc);
  const float tau = at(taup, eDc + dc);
  if (!joint) { q = 0.0f; v = 0.0f; }
  float qdd0 = 0.0f;
  ArtFloat none;
  for (int s = 0; s < steps; ++s) {
    const float qdd = art_substep<false>(L, tree, base, none, lane, h, tau, enforce_limits != 0, q, v);
    if (s == 0) qdd0 = qdd;
  }
  if (valid && joint) {
    at(out_q, eDc + (u32)dc) = q;
    at(out_v, eDc + (u32)dc) = v;
    at(out_qdd0, eDc + (u32)dc) = qdd0;
  }
}

extern "C" int pbhc_sizeof_articulated_params(void) { return (int)sizeof(PbhcArticulatedParams); }

// the kernel arguments travel by value: the largest set (the debug kernel's) must fit the 4 KB kernarg segment
static_assert(sizeof(ArtSkel) + sizeof(PbhcArticulatedParams) + sizeof(ArtTree) + 12 * 8 <= 4096, "k_art_debug: kernel arguments over 4 KB");
static_assert(sizeof(PbhcStepIO) + sizeof(PbhcMotionTable) + sizeof(PbhcArticulatedParams) + sizeof(ArtTree) + 4 * 8 <= 4096,
              "k_articulated_sim: kernel arguments over 4 KB");

static int art_check_params(const PbhcArticulatedParams* p, int B) {
  for (int b = 0; b < B; ++b) CL_CHECK(p->mass[b] >= 0.0f);
  for (int d = 0; d < B - 1; ++d) CL_CHECK(p->armature[d] >= 0.0f && p->damping[d] >= 0.0f);
  return PBHC_OK;
}

extern "C" int pbhc_articulated_sim_step(PbhcEnv* e, const PbhcStepIO* io, const PbhcArticulatedParams* p, void* stream) {
  CL_CHECK(p);
  const PbhcEnvConfig *hc = nullptr, *dcfg = nullptr;
  const PbhcMotionTable* tbl = nullptr;
  double* glob = nullptr;
  int rc = cl_check_step(e, io, p->decimation, &hc, &dcfg, &tbl, &glob);
  if (rc != PBHC_OK) return rc;
  const int D = hc->skel.num_dof, B = hc->skel.num_bodies, N = hc->num_envs;
  CL_CHECK(B <= PBHC_ART_MAX_BODIES && D == B - 1);
  if ((rc = art_check_params(p, B)) != PBHC_OK) return rc;
  ArtTree tree;
  if ((rc = art_tree(hc->skel, &tree)) != PBHC_OK) return rc;
  hipLaunchKernelGGL(k_articulated_sim, dim3((N + CL_EPB - 1) / CL_EPB), dim3(PBHC_G * CL_EPB), 0, (hipStream_t)stream, dcfg, *tbl, *io, *p, tree,
                     (const double*)glob, N);
  if (hipGetLastError() != hipSuccess) {
    snprintf(g_pbhc_err, sizeof(g_pbhc_err), "pbhc_articulated_sim_step: launch failed");
    return PBHC_EHIP;
  }
  return PBHC_OK;
}

extern "C" int pbhc_debug_articulated_substeps(const PbhcSkeleton* skel, const PbhcArticulatedParams* p, const float* base, const float* q, const float* v,
                                               const float* tau, int n, int steps, float h, int enforce_limits, const float* limits, float* out_q,
                                               float* out_v, float* out_qdd0, void* stream) {
  CL_CHECK(skel && p && base && q && v && tau && out_q && out_v && out_qdd0);
  CL_CHECK(n >= 1 && steps >= 1 && steps <= ART_MAX_DEBUG_STEPS && h > 0.0f && (!enforce_limits || limits));
  ArtTree tree;
  int rc = art_tree(*skel, &tree);
  if (rc != PBHC_OK) return rc;
  const int B = skel->num_bodies;
  if ((rc = art_check_params(p, B)) != PBHC_OK) return rc;
  CL_CHECK((uint64_t)n * (uint64_t)B < (1ull << 28));
  ArtSkel sk;
  art_skel(*skel, enforce_limits ? limits : nullptr, &sk);
  hipLaunchKernelGGL(k_art_debug, dim3((n + CL_EPB - 1) / CL_EPB), dim3(PBHC_G * CL_EPB), 0, (hipStream_t)stream, sk, *p, tree, base, q, v, tau, n,
                     steps, h, enforce_limits, out_q, out_v, out_qdd0);
  if (hipGetLastError() != hipSuccess) {
    snprintf(g_pbhc_err, sizeof(g_pbhc_err), "pbhc_debug_articulated_substeps: launch failed");
    return PBHC_EHIP;
  }
  return PBHC_OK;
}
