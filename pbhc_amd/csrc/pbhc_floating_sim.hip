// pbhc_floating_sim.hip — the floating-base simulator (pbhc_amd/simulator/floating_sim.py FloatingBaseSim).
//
//   k_floating_sim   one launch per control step, where k_articulated_sim sits (directly in front of k_env_step on the stepping stream), writing
//                    the same one-frame replay window.  The delayed-action peek, the torque law and its draws are the shared front's
//                    (pbhc_closed_loop.h; lane = body and lane b owns dof b - 1); the clip's rows are NOT loaded: the root is the state
//                    io->root_states holds (what the previous step left, resets included), six more degrees of freedom of the tree, and the
//                    ground pushes back at contact points on the links.  Definition: include/pbhc_hip.h, PbhcFloatingParams.
//   k_float_debug    test-only: the same device functions (art_substep<true>, art_integrate_root) under a constant torque.
//
// The forward dynamics is pbhc_art_dynamics.h's, FREE = true.  The root's state is held on every lane of the env (13 registers, the same
// values); the contact points of a body are the body's lane's, read from a small device table with plain loads in front of the sub-steps.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <math.h>

#include "../../include/pbhc_hip.h"
#include "pbhc_math.h"

using namespace pbhc;

#undef PBHC_STAMPS                                          // (the phase stamps of the diagnostic build belong to the step kernel's unit)
#include "pbhc_env_step.h"                                  // PBHC_G, at, clampf, rng_uniform / rng_normal
#include "pbhc_closed_loop.h"                               // CL_EPB, ClFront and the cl_* pieces, CL_CHECK, cl_check_step
#include "pbhc_art_dynamics.h"                              // ArtTree, ArtSkel, ArtLane, ArtBase, ArtFloat, art_substep, art_integrate_root

static_assert(PBHC_FLOAT_MAX_POINTS == ART_MAX_POINTS, "the point table's width");

// the lane's contact points and the contact law
// (`env_friction` [N], or NULL: in place of the params' one coefficient; `envc`: the env, clamped)
__device__ __forceinline__ void float_lane_contact(ArtFloat& X, const PbhcFloatingParams& p, int lane, const float* __restrict__ env_friction, int envc) {
  X.npts = p.num_points[lane];
  const float* r = p.points + lane * (ART_MAX_POINTS * 3);  // the table has PBHC_ART_MAX_BODIES rows: every lane's loads are in bounds
  X.r0 = mk3(r[0], r[1], r[2]); X.r1 = mk3(r[3], r[4], r[5]); X.r2 = mk3(r[6], r[7], r[8]); X.r3 = mk3(r[9], r[10], r[11]);
  const f3 zero = mk3(0.0f, 0.0f, 0.0f);
  X.f0 = zero; X.f1 = zero; X.f2 = zero; X.f3_ = zero;
  X.stiffness = p.stiffness; X.normal_damping = p.normal_damping; X.friction = env_friction ? env_friction[envc] : p.friction; X.slip_velocity = p.slip_velocity;
  X.ground_height = p.ground_height;
  X.g = mk3(p.gravity[0], p.gravity[1], p.gravity[2]);
  X.a0 = zero; X.alpha0 = zero;
}

// the lane's row of env_inertial ([N, PBHC_ART_MAX_BODIES, 4]; NULL without the table)
__device__ __forceinline__ const float* float_env_row(const PbhcFloatingParams& p, int envc, int lane) {
  return p.env_inertial ? p.env_inertial + ((size_t)envc * PBHC_ART_MAX_BODIES + (size_t)lane) * 4 : nullptr;
}

// push_robots (include/pbhc_hip.h, PbhcFloatingParams.push_counter): the env's words, loaded in front of the sub-steps with the other per-env
// loads (the same addresses on every lane of the env: the root's state lives on every lane, so every lane evaluates the same test) ...
struct FloatPush { int counter, interval; float u0, u1, u2; };
__device__ __forceinline__ void float_push_load(FloatPush& P, const PbhcFloatingParams& p, int envc) {
  typedef unsigned int u32;
  P.counter = 0; P.interval = 0; P.u0 = P.u1 = P.u2 = 0.0f;
  if (!p.push_counter) return;
  // (a ragged last workgroup's missing envs load env N - 1's words from other waves while that env's lane 0 stores them: whatever they
  // read, their results are discarded and they never store)
  P.counter = p.push_counter[envc]; P.interval = p.push_interval[envc];
  if (p.u_push) { P.u0 = at(p.u_push, (u32)envc * 3u); P.u1 = at(p.u_push, (u32)envc * 3u + 1u); P.u2 = at(p.u_push, (u32)envc * 3u + 2u); }
}
// ... and the push itself, on the root's linear velocity in registers before the first sub-step.  `just_reset`: the previous step reset the
// env (its counter and interval are renewed and the draws consumed, the velocity is the reset's).  Lane 0 alone stores, plain vector stores.
__device__ __forceinline__ void float_push(ArtFloat& X, FloatPush P, const PbhcFloatingParams& p, uint64_t seed, unsigned int env, int envc,
                                           unsigned int step_ctr, float dt, bool just_reset, bool store) {
  typedef unsigned int u32;
  if (!p.push_counter) return;
  const bool fire = P.counter == (int)((float)P.interval / dt);
  float pvx = 0.0f, pvy = 0.0f;
  if (fire) {
    if (!p.u_push) {
      float u[4];
      rng_uniform4(seed, env, step_ctr, PBHC_RNG_STREAM_PUSH, 0u, u);
      P.u0 = u[0]; P.u1 = u[1]; P.u2 = u[2];
    }
    P.counter = 0;
    P.interval = min(p.push_lo + (int)floorf(P.u0 * (float)(p.push_hi - p.push_lo)), p.push_hi - 1);
    pvx = (2.0f * P.u1 - 1.0f) * p.max_push_vel_xy;
    pvy = (2.0f * P.u2 - 1.0f) * p.max_push_vel_xy;
    if (!just_reset) {
      X.v0.x = p.push_fixed ? X.v0.x + pvx : pvx;
      X.v0.y = p.push_fixed ? X.v0.y + pvy : pvy;
    }
  }
  if (!store) return;
  p.push_counter[envc] = P.counter + 1;
  p.push_interval[envc] = P.interval;
  if (fire) { at(p.push_vel, (u32)envc * 2u) = pvx; at(p.push_vel, (u32)envc * 2u + 1u) = pvy; }
}

// the root's 13 words (one per lane 0..12, `rs`) onto every lane
__device__ __forceinline__ void float_root_state(ArtBase& base, ArtFloat& X, float rs) {
  X.p0 = mk3(shf(rs, 0), shf(rs, 1), shf(rs, 2));
  base.R0 = quat_unit_fast(mk4(shf(rs, 3), shf(rs, 4), shf(rs, 5), shf(rs, 6)));
  X.v0 = mk3(shf(rs, 7), shf(rs, 8), shf(rs, 9));
  base.w0 = mk3(shf(rs, 10), shf(rs, 11), shf(rs, 12));
  base.alpha0 = mk3(0.0f, 0.0f, 0.0f);
  base.a0g = mk3(0.0f, 0.0f, 0.0f);
}

// word `lane` (0..12) of the root's state; the operands by VALUE (a select between members of a struct held by reference becomes a select
// between addresses, and the struct goes to scratch)
__device__ __forceinline__ float float_root_word(f3 p0, f4 R0, f3 v0, f3 w0, int lane) {
  float w = p0.x;
  w = lane == 1 ? p0.y : w; w = lane == 2 ? p0.z : w;
  w = lane == 3 ? R0.x : w; w = lane == 4 ? R0.y : w; w = lane == 5 ? R0.z : w; w = lane == 6 ? R0.w : w;
  w = lane == 7 ? v0.x : w; w = lane == 8 ? v0.y : w; w = lane == 9 ? v0.z : w;
  w = lane == 10 ? w0.x : w; w = lane == 11 ? w0.y : w; w = lane == 12 ? w0.z : w;
  return w;
}
// word `lane` (0..5) of [a_0, alpha_0]
__device__ __forceinline__ float float_acc_word(f3 a0, f3 alpha0, int lane) {
  float w = a0.x;
  w = lane == 1 ? a0.y : w; w = lane == 2 ? a0.z : w; w = lane == 3 ? alpha0.x : w; w = lane == 4 ? alpha0.y : w; w = lane == 5 ? alpha0.z : w;
  return w;
}

// DR: a per-env operand of the params is non-NULL (env_inertial, env_friction, push_counter).  DR = false is the kernel without them: the
// entry launches it when every one is NULL, so a simulator with the randomisation off runs the instructions it ran before there was any.
template <bool DR>
__global__ __launch_bounds__(PBHC_G* CL_EPB) void k_floating_sim(const PbhcEnvConfig* __restrict__ cfgp, PbhcStepIO io, PbhcFloatingParams p, ArtTree tree,
                                                                 const double* __restrict__ glob, int N) {
  ClCfg& c = *(ClCfg*)cfgp;
  typedef unsigned int u32;
  const int D = c.skel.num_dof, B = c.skel.num_bodies;
  const int lane = threadIdx.x & (PBHC_G - 1);
  const bool joint = lane >= 1 && lane < B;                  // lane = body; its hinge is dof lane - 1
  ClFront F;
  cl_load_env(F, c, io, glob, N, lane, min(max(lane - 1, 0), D - 1));
  const int dc = F.dc;
  const float h = c.sim_dt;
  const float rs = at(io.root_states, (u32)F.envc * 13u + (u32)min(lane, 12));
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
  art_lane_inertial(L, p, lane, dc, h, DR ? float_env_row(p, F.envc, lane) : nullptr);
  ArtFloat X;
  float_lane_contact(X, p, lane, DR ? p.env_friction : nullptr, F.envc);
  FloatPush push;
  if (DR) float_push_load(push, p, F.envc);
  __builtin_amdgcn_sched_barrier(0);
  cl_control(F, c, io);
  ArtBase base;
  float_root_state(base, X, rs);
  if (DR) float_push(X, push, p, c.seed, (u32)F.env, F.envc, F.step_ctr, c.dt, F.ep1 == 1, F.valid && lane == 0);

  // ---- the sub-steps: torque from the current (q, v), contact from the current state, the free tree's forward dynamics, the step
  float q = F.q, v = F.v;
  if (!joint) { q = 0.0f; v = 0.0f; }
  float tq0 = 0.0f;
  for (int s = 0; s < p.decimation; ++s) {
    const float tq = cl_torque(F, c, q, v);
    if (s == 0) tq0 = tq;
    art_substep<true>(L, tree, base, X, lane, h, tq, p.enforce_limits != 0, q, v);
    art_integrate_root(base, X, h);
  }

  // ---- the frame ([1, N, ...]), plain vector stores
  if (!F.valid) return;
  if (joint) {
    at(const_cast<float*>(io.frame_dof_pos), F.eDc + (u32)dc) = q;
    at(const_cast<float*>(io.frame_dof_vel), F.eDc + (u32)dc) = v;
    if (p.tau0) at(p.tau0, F.eDc + (u32)dc) = tq0;
  }
  if (lane < 13) at(const_cast<float*>(io.frame_root), (u32)F.envc * 13u + (u32)lane) = float_root_word(X.p0, base.R0, X.v0, base.w0, lane);
  if (lane < B && X.npts > 0) {
    const f3 sum = add3(add3(add3(X.f0, X.f1), X.f2), X.f3_);
    float* fc = const_cast<float*>(io.frame_contact) + ((u32)F.envc * (u32)(B * 3) + (u32)(3 * lane));
    fc[0] = sum.x; fc[1] = sum.y; fc[2] = sum.z;
  }
  if (p.root_acc && lane < 6) at(p.root_acc, (u32)F.envc * 6u + (u32)lane) = float_acc_word(X.a0, X.alpha0, lane);
}

__global__ __launch_bounds__(PBHC_G* CL_EPB) void k_float_debug(ArtSkel sk, PbhcFloatingParams p, ArtTree tree, const float* __restrict__ rootp,
                                                                 const float* __restrict__ qp, const float* __restrict__ vp, const float* __restrict__ taup,
                                                                 int n, int steps, float h, int enforce_limits, float* __restrict__ out_root,
                                                                 float* __restrict__ out_q, float* __restrict__ out_v, float* __restrict__ out_acc0,
                                                                 float* __restrict__ out_force) {
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
  art_lane_inertial(L, p, lane, dc, h, float_env_row(p, envc, lane));
  ArtFloat X;
  float_lane_contact(X, p, lane, p.env_friction, envc);
  ArtBase base;
  float_root_state(base, X, at(rootp, (u32)envc * 13u + (u32)min(lane, 12)));
  float q = at(qp, eDc + dc), v = at(vp, eDc + dc);
  const float tau = at(taup, eDc + dc);
  if (!joint) { q = 0.0f; v = 0.0f; }
  float acc0 = 0.0f;
  f3 g0 = mk3(0.0f, 0.0f, 0.0f), g1 = g0, g2 = g0, g3 = g0;   // the first sub-step's point forces
  for (int s = 0; s < steps; ++s) {
    const float qdd = art_substep<true>(L, tree, base, X, lane, h, tau, enforce_limits != 0, q, v);
    if (s == 0) {
      // lanes 0..5 keep [a_0, alpha_0] (words 0..5 of the row), the joints' lanes their q'' (word 6 + dof = 5 + lane, stored at the end)
      acc0 = qdd;
      g0 = X.f0; g1 = X.f1; g2 = X.f2; g3 = X.f3_;
      if (valid && lane < 6) at(out_acc0, (u32)envc * (u32)(6 + D) + (u32)lane) = float_acc_word(X.a0, X.alpha0, lane);
    }
    art_integrate_root(base, X, h);
  }
  if (!valid) return;
  if (joint) {
    at(out_q, eDc + (u32)dc) = q;
    at(out_v, eDc + (u32)dc) = v;
    at(out_acc0, (u32)envc * (u32)(6 + D) + (u32)(6 + dc)) = acc0;
  }
  if (lane < 13) at(out_root, (u32)envc * 13u + (u32)lane) = float_root_word(X.p0, base.R0, X.v0, base.w0, lane);
  if (lane < B) {
    float* fo = out_force + ((u32)envc * (u32)B + (u32)lane) * (u32)(ART_MAX_POINTS * 3);
    fo[0] = g0.x; fo[1] = g0.y; fo[2] = g0.z; fo[3] = g1.x; fo[4] = g1.y; fo[5] = g1.z;
    fo[6] = g2.x; fo[7] = g2.y; fo[8] = g2.z; fo[9] = g3.x; fo[10] = g3.y; fo[11] = g3.z;
  }
}

extern "C" int pbhc_sizeof_floating_params(void) { return (int)sizeof(PbhcFloatingParams); }

// the kernel arguments travel by value: both sets must fit the 4 KB kernarg segment (which is why the points are a device table)
static_assert(sizeof(ArtSkel) + sizeof(PbhcFloatingParams) + sizeof(ArtTree) + 14 * 8 <= 4096, "k_float_debug: kernel arguments over 4 KB");
static_assert(sizeof(PbhcStepIO) + sizeof(PbhcFloatingParams) + sizeof(ArtTree) + 4 * 8 <= 4096, "k_floating_sim: kernel arguments over 4 KB");

static int float_check_params(const PbhcFloatingParams* p, int B) {
  CL_CHECK(p->points);
  for (int b = 0; b < B; ++b) CL_CHECK(p->mass[b] >= 0.0f);
  CL_CHECK(p->mass[0] > 0.0f);
  for (int d = 0; d < B - 1; ++d) CL_CHECK(p->armature[d] >= 0.0f && p->damping[d] >= 0.0f);
  CL_CHECK(p->stiffness >= 0.0f && p->normal_damping >= 0.0f && p->friction >= 0.0f && p->slip_velocity > 0.0f);
  for (int b = 0; b < PBHC_ART_MAX_BODIES; ++b) CL_CHECK(p->num_points[b] >= 0 && p->num_points[b] <= (b < B ? PBHC_FLOAT_MAX_POINTS : 0));
  CL_CHECK(((uintptr_t)p->env_inertial & 15) == 0);        // one 16-byte load per lane
  CL_CHECK(((uintptr_t)p->env_friction & 3) == 0);
  return PBHC_OK;
}

// push_robots: the three state pointers together or not at all, the draws' buffer only with them
static int float_check_push(const PbhcFloatingParams* p) {
  if (!p->push_counter) {
    CL_CHECK(!p->push_interval && !p->push_vel && !p->u_push);
    return PBHC_OK;
  }
  CL_CHECK(p->push_interval && p->push_vel);
  CL_CHECK(((((uintptr_t)p->push_counter | (uintptr_t)p->push_interval | (uintptr_t)p->push_vel | (uintptr_t)p->u_push) & 3) == 0));
  CL_CHECK(p->push_lo >= 0 && p->push_hi > p->push_lo && p->max_push_vel_xy >= 0.0f);
  return PBHC_OK;
}

extern "C" int pbhc_floating_sim_step(PbhcEnv* e, const PbhcStepIO* io, const PbhcFloatingParams* p, void* stream) {
  CL_CHECK(p);
  const PbhcEnvConfig *hc = nullptr, *dcfg = nullptr;
  const PbhcMotionTable* tbl = nullptr;
  double* glob = nullptr;
  int rc = cl_check_step(e, io, p->decimation, &hc, &dcfg, &tbl, &glob);
  if (rc != PBHC_OK) return rc;
  CL_CHECK(io->root_states);
  const int D = hc->skel.num_dof, B = hc->skel.num_bodies, N = hc->num_envs;
  CL_CHECK(B <= PBHC_ART_MAX_BODIES && D == B - 1);
  if ((rc = float_check_params(p, B)) != PBHC_OK) return rc;
  if ((rc = float_check_push(p)) != PBHC_OK) return rc;
  ArtTree tree;
  if ((rc = art_tree(hc->skel, &tree)) != PBHC_OK) return rc;
  const dim3 grid((N + CL_EPB - 1) / CL_EPB), block(PBHC_G * CL_EPB);
  if (p->env_inertial || p->env_friction || p->push_counter)
    hipLaunchKernelGGL(k_floating_sim<true>, grid, block, 0, (hipStream_t)stream, dcfg, *io, *p, tree, (const double*)glob, N);
  else
    hipLaunchKernelGGL(k_floating_sim<false>, grid, block, 0, (hipStream_t)stream, dcfg, *io, *p, tree, (const double*)glob, N);
  if (hipGetLastError() != hipSuccess) {
    snprintf(g_pbhc_err, sizeof(g_pbhc_err), "pbhc_floating_sim_step: launch failed");
    return PBHC_EHIP;
  }
  return PBHC_OK;
}

extern "C" int pbhc_debug_floating_substeps(const PbhcSkeleton* skel, const PbhcFloatingParams* p, const float* root, const float* q, const float* v,
                                            const float* tau, int n, int steps, float h, int enforce_limits, const float* limits, float* out_root,
                                            float* out_q, float* out_v, float* out_acc0, float* out_force, void* stream) {
  CL_CHECK(skel && p && root && q && v && tau && out_root && out_q && out_v && out_acc0 && out_force);
  CL_CHECK(n >= 1 && steps >= 1 && steps <= ART_MAX_DEBUG_STEPS && h > 0.0f && (!enforce_limits || limits));
  ArtTree tree;
  int rc = art_tree(*skel, &tree);
  if (rc != PBHC_OK) return rc;
  const int B = skel->num_bodies;
  if ((rc = float_check_params(p, B)) != PBHC_OK) return rc;
  CL_CHECK(!p->push_counter && !p->push_interval && !p->push_vel && !p->u_push);      // no control step here: no push
  CL_CHECK((uint64_t)n * (uint64_t)B * (uint64_t)(PBHC_FLOAT_MAX_POINTS * 3) < (1ull << 30));
  ArtSkel sk;
  art_skel(*skel, enforce_limits ? limits : nullptr, &sk);
  hipLaunchKernelGGL(k_float_debug, dim3((n + CL_EPB - 1) / CL_EPB), dim3(PBHC_G * CL_EPB), 0, (hipStream_t)stream, sk, *p, tree, root, q, v, tau, n,
                     steps, h, enforce_limits, out_root, out_q, out_v, out_acc0, out_force);
  if (hipGetLastError() != hipSuccess) {
    snprintf(g_pbhc_err, sizeof(g_pbhc_err), "pbhc_debug_floating_substeps: launch failed");
    return PBHC_EHIP;
  }
  return PBHC_OK;
}
