// pbhc_articulated_sim.hip — the articulated rigid-body simulator (pbhc_amd/simulator/articulated_sim.py ArticulatedSim).
//
//   k_articulated_sim   one launch per control step, where k_joint_sim sits (directly in front of k_env_step on the stepping stream), writing the
//                       same one-frame replay window.  Root, contact, the delayed-action peek, the torque law and its draws are k_joint_sim's:
//                       the shared part lives in pbhc_closed_loop.h (here lane = body and lane b owns dof b - 1).  Only the joint law differs:
//                       every sub-step solves  (M(q) + diag(armature + h b)) dv = h (tau - b v - c(q, v; base))  on the robot's tree with the
//                       MJCF's masses, centres of mass and inertia tensors; the base (the root row this kernel writes) is prescribed.
//   k_art_debug         test-only: the same device function (art_substep) under a constant torque.
//
// The forward dynamics is the articulated-body algorithm in three level-synchronous passes over the tree's depth.  Every link's spatial
// quantities are expressed in WORLD axes about the link's OWN origin (so the hinge is S_b = [a; 0] and no lever longer than a link enters an
// inertia: about one common point the distal links' m r^2 swamped their own 4e-4 kg m^2 and float32 lost three digits).  Between a link and its
// parent only the reference point moves, by d_b = R_parent offset_b; nothing is rotated and no position is ever formed, so the env origin never
// enters the arithmetic:
//   pass 1 (root -> leaves)  orientation, d_b, axis a, velocity v_b = shift(v_parent) + S_b qd_b, velocity-product acceleration
//                            c_b = shift(v_parent) x S_b qd_b; then per lane the link's spatial inertia and its bias v x* (I v)
//   pass 2 (leaves -> root)  U = I^A S, D = S.U + armature + h b, u = tau - b qd - S.p^A, I^a = I^A - U U^T / D, p^a = p^A + I^a c + U u / D,
//                            moved to the parent's origin and summed into the parent: 27 words, 21 of the symmetric articulated inertia and 6
//                            of the bias force (the sum into the prescribed root is skipped)
//   pass 3 (root -> leaves)  a' = shift(a_parent) + c, qdd = (u - U.a') / D, a = a' + S qdd;  the root's a = [alpha_0; a_0 - g]
// (The base's linear velocity is left out: a constant velocity of the whole frame changes no joint acceleration.)
// Per-lane state lives in registers; parent -> child and child -> parent traffic goes by __shfl inside the env's 32 lanes (always the same
// wave): a parent reads its children one after the other through a first-child / next-sibling list, in index order, so the sums are
// reproducible.  No LDS, no runtime-indexed per-thread arrays.
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

#define ART_MAX_DEBUG_STEPS 4096
static_assert(PBHC_ART_MAX_BODIES == PBHC_G, "one body per lane of an env group");

struct sym3 { float xx, yy, zz, xy, xz, yz; };
struct mat3 { float m00, m01, m02, m10, m11, m12, m20, m21, m22; };
__device__ __forceinline__ f3 sym3_mv(const sym3& s, f3 v) {
  return mk3(s.xx * v.x + s.xy * v.y + s.xz * v.z, s.xy * v.x + s.yy * v.y + s.yz * v.z, s.xz * v.x + s.yz * v.y + s.zz * v.z);
}
__device__ __forceinline__ f3 mat3_mv(const mat3& m, f3 v) {
  return mk3(m.m00 * v.x + m.m01 * v.y + m.m02 * v.z, m.m10 * v.x + m.m11 * v.y + m.m12 * v.z, m.m20 * v.x + m.m21 * v.y + m.m22 * v.z);
}
__device__ __forceinline__ f3 mat3_tmv(const mat3& m, f3 v) {   // m^T v
  return mk3(m.m00 * v.x + m.m10 * v.y + m.m20 * v.z, m.m01 * v.x + m.m11 * v.y + m.m21 * v.z, m.m02 * v.x + m.m12 * v.y + m.m22 * v.z);
}
__device__ __forceinline__ float shf(float x, int src) { return __shfl(x, src, PBHC_G); }
__device__ __forceinline__ f3 shf3(f3 v, int src) { return mk3(shf(v.x, src), shf(v.y, src), shf(v.z, src)); }
__device__ __forceinline__ f4 shf4(f4 v, int src) { return mk4(shf(v.x, src), shf(v.y, src), shf(v.z, src), shf(v.w, src)); }

// the tree's child lists, built on the host from the skeleton's parents (art_tree): a parent walks first_child -> next_sibling
struct ArtTree {
  int32_t first_child[PBHC_ART_MAX_BODIES], next_sibling[PBHC_ART_MAX_BODIES];
  int32_t nchild[PBHC_MAX_DEPTH + 2];                       // [L]: the most children any body of depth L - 1 has at depth L
  int32_t max_depth;
};
// the debug kernel's copy of what the sim kernel reads from the env's config
struct ArtSkel {
  int32_t num_bodies;
  int32_t parent[PBHC_ART_MAX_BODIES], depth[PBHC_ART_MAX_BODIES];
  float offset[PBHC_ART_MAX_BODIES][3], lq_xyzw[PBHC_ART_MAX_BODIES][4], axis[PBHC_ART_MAX_BODIES][3];      // axis: of the hinge that drives the body, unit
  float limits[PBHC_ART_MAX_BODIES][2];
};
// one lane's constants (lane = body; its hinge is dof lane - 1)
struct ArtLane {
  int parent, depth, first_child, next_sibling;             // parent clamped to >= 0; depth -1: no body in this lane
  f3 off, axis, com;
  f4 lq;
  float mass;
  sym3 inertia;
  float arm_h, damping;                                     // armature + h b, b
  float lo, hi;
};
struct ArtBase { f4 R0; f3 w0, alpha0, a0g; };              // a0g = a_0 - g

// One sub-step of the definition: (q, v) of the lane's hinge under the torque `tau`; returns dv / h.
__device__ __forceinline__ float art_substep(const ArtLane& L, const ArtTree& T, const ArtBase& base, int lane, float h, float tau, bool enforce_limits,
                                             float& q, float& v) {
  const f3 zero = mk3(0.0f, 0.0f, 0.0f);
  const bool body = L.depth >= 1;
  // ---- pass 1: orientation, offset from the parent's origin, axis, velocity (of the link's own origin), velocity-product acceleration
  const f4 relq = quat_mul(L.lq, quat_from_angle_unit_axis(q, L.axis));
  f4 R = base.R0;
  f3 d = zero, vw = base.w0, vl = zero, cw = zero, cl = zero, Sa = zero;
  for (int lev = 1; lev <= T.max_depth; ++lev) {
    const f4 Rp = shf4(R, L.parent);
    const f3 vwp = shf3(vw, L.parent), vlp = shf3(vl, L.parent);
    if (L.depth == lev) {
      d = fk_rotate(Rp, L.off);                              // the FK's own chain (fk_walk): the product renormalised at every level — without
      R = fk_mul_unit(Rp, relq);                             // it the quaternion's norm drifts by ~1e-6 down a limb and |S|^2 with it
      Sa = fk_rotate(R, L.axis);
      const f3 jw = mul3(Sa, v);
      vw = add3(vwp, jw);
      vl = add3(vlp, cross3(vwp, d));
      cw = cross3(vwp, jw);
      cl = cross3(vl, jw);
    }
  }
  // ---- the link's spatial inertia about its own origin in world axes:  f_ang = A w + H v,  f_lin = H^T w + M v
  sym3 A, M;
  mat3 H;
  f3 pw, pl;                                                 // bias force
  {
    const fkm33 r = fk_matrix(R);
    const f3 c = mk3(r.m00 * L.com.x + r.m01 * L.com.y + r.m02 * L.com.z, r.m10 * L.com.x + r.m11 * L.com.y + r.m12 * L.com.z,
                     r.m20 * L.com.x + r.m21 * L.com.y + r.m22 * L.com.z);
    const sym3& I = L.inertia;
    // t = r I  (rows of r times the symmetric I), then r I r^T
    const float t00 = r.m00 * I.xx + r.m01 * I.xy + r.m02 * I.xz, t01 = r.m00 * I.xy + r.m01 * I.yy + r.m02 * I.yz, t02 = r.m00 * I.xz + r.m01 * I.yz + r.m02 * I.zz;
    const float t10 = r.m10 * I.xx + r.m11 * I.xy + r.m12 * I.xz, t11 = r.m10 * I.xy + r.m11 * I.yy + r.m12 * I.yz, t12 = r.m10 * I.xz + r.m11 * I.yz + r.m12 * I.zz;
    const float t20 = r.m20 * I.xx + r.m21 * I.xy + r.m22 * I.xz, t21 = r.m20 * I.xy + r.m21 * I.yy + r.m22 * I.yz, t22 = r.m20 * I.xz + r.m21 * I.yz + r.m22 * I.zz;
    const float m = body ? L.mass : 0.0f, cc = dot3(c, c);
    A.xx = t00 * r.m00 + t01 * r.m01 + t02 * r.m02 + m * (cc - c.x * c.x);
    A.yy = t10 * r.m10 + t11 * r.m11 + t12 * r.m12 + m * (cc - c.y * c.y);
    A.zz = t20 * r.m20 + t21 * r.m21 + t22 * r.m22 + m * (cc - c.z * c.z);
    A.xy = t00 * r.m10 + t01 * r.m11 + t02 * r.m12 - m * (c.x * c.y);
    A.xz = t00 * r.m20 + t01 * r.m21 + t02 * r.m22 - m * (c.x * c.z);
    A.yz = t10 * r.m20 + t11 * r.m21 + t12 * r.m22 - m * (c.y * c.z);
    if (!body) A.xx = A.yy = A.zz = A.xy = A.xz = A.yz = 0.0f;
    const f3 mc = mul3(c, m);
    H.m00 = 0.0f; H.m01 = -mc.z; H.m02 = mc.y;
    H.m10 = mc.z; H.m11 = 0.0f; H.m12 = -mc.x;
    H.m20 = -mc.y; H.m21 = mc.x; H.m22 = 0.0f;
    M.xx = M.yy = M.zz = m; M.xy = M.xz = M.yz = 0.0f;
    const f3 fw = add3(sym3_mv(A, vw), mat3_mv(H, vl)), fl = add3(mat3_tmv(H, vw), sym3_mv(M, vl));
    pw = add3(cross3(vw, fw), cross3(vl, fl));
    pl = cross3(vw, fl);
  }
  // ---- pass 2: articulated inertias and bias forces, leaves -> root
  f3 Uw = zero, Ul = zero;
  float Dj = 1.0f, uj = 0.0f;
  int cur = L.first_child;
  sym3 As = A;                                               // what the parent receives: (I^a, p^a) moved to the parent's origin
  mat3 Hs = H;
  f3 pws = pw;
  for (int lev = T.max_depth; lev >= 1; --lev) {
    if (L.depth == lev) {
      Uw = sym3_mv(A, Sa);                                   // S = [a; 0]: the axis passes through the link's own origin
      Ul = mat3_tmv(H, Sa);
      Dj = dot3(Sa, Uw) + L.arm_h;
      uj = tau - L.damping * v - dot3(Sa, pw);
      const f3 Gw = mul3(Uw, 1.0f / Dj), Gl = mul3(Ul, 1.0f / Dj);          // U / D
      A.xx -= Uw.x * Gw.x; A.yy -= Uw.y * Gw.y; A.zz -= Uw.z * Gw.z; A.xy -= Uw.x * Gw.y; A.xz -= Uw.x * Gw.z; A.yz -= Uw.y * Gw.z;
      M.xx -= Ul.x * Gl.x; M.yy -= Ul.y * Gl.y; M.zz -= Ul.z * Gl.z; M.xy -= Ul.x * Gl.y; M.xz -= Ul.x * Gl.z; M.yz -= Ul.y * Gl.z;
      H.m00 -= Uw.x * Gl.x; H.m01 -= Uw.x * Gl.y; H.m02 -= Uw.x * Gl.z;
      H.m10 -= Uw.y * Gl.x; H.m11 -= Uw.y * Gl.y; H.m12 -= Uw.y * Gl.z;
      H.m20 -= Uw.z * Gl.x; H.m21 -= Uw.z * Gl.y; H.m22 -= Uw.z * Gl.z;
      pw = add3(pw, add3(add3(sym3_mv(A, cw), mat3_mv(H, cl)), mul3(Gw, uj)));
      pl = add3(pl, add3(add3(mat3_tmv(H, cw), sym3_mv(M, cl)), mul3(Gl, uj)));
      // the reference point moves by d to the parent's origin: with D = [d]x,  M' = M,  H' = H + D M,  A' = A - (H D + (H D)^T) - D M D,
      // n' = n + d x f.  Row i of X D is (row i of X) x d; column j of D X is d x (column j of X).
      const f3 h0 = cross3(mk3(H.m00, H.m01, H.m02), d), h1 = cross3(mk3(H.m10, H.m11, H.m12), d), h2 = cross3(mk3(H.m20, H.m21, H.m22), d);      // rows of H D
      const f3 m0 = cross3(d, mk3(M.xx, M.xy, M.xz)), m1 = cross3(d, mk3(M.xy, M.yy, M.yz)), m2 = cross3(d, mk3(M.xz, M.yz, M.zz));              // columns of D M
      // rows of D M: (m0.x m1.x m2.x), (m0.y m1.y m2.y), (m0.z m1.z m2.z); rows of (D M) D
      const f3 e0 = cross3(mk3(m0.x, m1.x, m2.x), d), e1 = cross3(mk3(m0.y, m1.y, m2.y), d), e2 = cross3(mk3(m0.z, m1.z, m2.z), d);
      As.xx = A.xx - (h0.x + h0.x) - e0.x; As.yy = A.yy - (h1.y + h1.y) - e1.y; As.zz = A.zz - (h2.z + h2.z) - e2.z;
      As.xy = A.xy - (h0.y + h1.x) - e0.y; As.xz = A.xz - (h0.z + h2.x) - e0.z; As.yz = A.yz - (h1.z + h2.y) - e1.z;
      Hs.m00 = H.m00 + m0.x; Hs.m01 = H.m01 + m1.x; Hs.m02 = H.m02 + m2.x;
      Hs.m10 = H.m10 + m0.y; Hs.m11 = H.m11 + m1.y; Hs.m12 = H.m12 + m2.y;
      Hs.m20 = H.m20 + m0.z; Hs.m21 = H.m21 + m1.z; Hs.m22 = H.m22 + m2.z;
      pws = add3(pw, cross3(d, pl));
    }
    if (lev >= 2) {                                          // (the root is prescribed: nothing is summed into it)
      const int nc = T.nchild[lev];
      for (int it = 0; it < nc; ++it) {
        const bool take = L.depth == lev - 1 && cur >= 0;
        const int src = take ? cur : lane;
#define ART_ACC(x, y) { const float t_ = shf(y, src); if (take) x += t_; }
        ART_ACC(A.xx, As.xx) ART_ACC(A.yy, As.yy) ART_ACC(A.zz, As.zz) ART_ACC(A.xy, As.xy) ART_ACC(A.xz, As.xz) ART_ACC(A.yz, As.yz)
        ART_ACC(M.xx, M.xx) ART_ACC(M.yy, M.yy) ART_ACC(M.zz, M.zz) ART_ACC(M.xy, M.xy) ART_ACC(M.xz, M.xz) ART_ACC(M.yz, M.yz)
        ART_ACC(H.m00, Hs.m00) ART_ACC(H.m01, Hs.m01) ART_ACC(H.m02, Hs.m02) ART_ACC(H.m10, Hs.m10) ART_ACC(H.m11, Hs.m11) ART_ACC(H.m12, Hs.m12)
        ART_ACC(H.m20, Hs.m20) ART_ACC(H.m21, Hs.m21) ART_ACC(H.m22, Hs.m22)
        ART_ACC(pw.x, pws.x) ART_ACC(pw.y, pws.y) ART_ACC(pw.z, pws.z) ART_ACC(pl.x, pl.x) ART_ACC(pl.y, pl.y) ART_ACC(pl.z, pl.z)
#undef ART_ACC
        const int nxt = __shfl(L.next_sibling, src, PBHC_G);
        if (take) cur = nxt;
      }
    }
  }
  // ---- pass 3: accelerations (of each link's own origin), root -> leaves
  f3 aw = base.alpha0, al = base.a0g;
  float qdd = 0.0f;
  for (int lev = 1; lev <= T.max_depth; ++lev) {
    const f3 awp = shf3(aw, L.parent), alp = shf3(al, L.parent);
    if (L.depth == lev) {
      const f3 bw = add3(awp, cw), bl = add3(add3(alp, cross3(awp, d)), cl);
      qdd = (uj - (dot3(Uw, bw) + dot3(Ul, bl))) / Dj;
      aw = add3(bw, mul3(Sa, qdd)); al = bl;
    }
  }
  // ---- the step
  v = v + h * qdd;
  q = q + h * v;
  if (enforce_limits) {
    if (q < L.lo) { q = L.lo; if (v < 0.0f) v = 0.0f; }
    else if (q > L.hi) { q = L.hi; if (v > 0.0f) v = 0.0f; }
  }
  return qdd;
}

__device__ __forceinline__ void art_lane_inertial(ArtLane& L, const PbhcArticulatedParams& p, int lane, int dcl, float h) {
  L.mass = p.mass[lane];
  L.com = mk3(p.com[lane][0], p.com[lane][1], p.com[lane][2]);
  L.inertia.xx = p.inertia[lane][0]; L.inertia.yy = p.inertia[lane][1]; L.inertia.zz = p.inertia[lane][2];
  L.inertia.xy = p.inertia[lane][3]; L.inertia.xz = p.inertia[lane][4]; L.inertia.yz = p.inertia[lane][5];
  L.damping = p.damping[dcl];
  L.arm_h = p.armature[dcl] + h * L.damping;
}

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
  for (int s = 0; s < p.decimation; ++s) {
    const float tq = cl_torque(F, c, q, v);
    if (s == 0) tq0 = tq;
    art_substep(L, tree, base, lane, h, tq, p.enforce_limits != 0, q, v);
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
  for (int s = 0; s < steps; ++s) {
    const float qdd = art_substep(L, tree, base, lane, h, tau, enforce_limits != 0, q, v);
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

// child lists from the parents (bodies are in DFS order: a parent comes before its children); refuses a tree the kernel cannot walk
static int art_tree(const PbhcSkeleton& sk, ArtTree* t) {
  const int B = sk.num_bodies;
  CL_CHECK(B >= 2 && B <= PBHC_ART_MAX_BODIES && sk.num_dof == B - 1 && sk.max_depth >= 1 && sk.max_depth <= PBHC_MAX_DEPTH);
  memset(t, 0, sizeof(*t));
  int last[PBHC_ART_MAX_BODIES], count[PBHC_ART_MAX_BODIES];
  for (int b = 0; b < PBHC_ART_MAX_BODIES; ++b) { t->first_child[b] = t->next_sibling[b] = last[b] = -1; count[b] = 0; }
  CL_CHECK(sk.parent[0] < 0 && sk.depth[0] == 0);
  int maxd = 0;
  for (int b = 1; b < B; ++b) {
    const int pa = sk.parent[b];
    CL_CHECK(pa >= 0 && pa < b && sk.depth[b] == sk.depth[pa] + 1 && sk.depth[b] <= PBHC_MAX_DEPTH);
    if (last[pa] < 0) t->first_child[pa] = b; else t->next_sibling[last[pa]] = b;
    last[pa] = b;
    count[pa] += 1;
    if (count[pa] > t->nchild[sk.depth[b]]) t->nchild[sk.depth[b]] = count[pa];
    if (sk.depth[b] > maxd) maxd = sk.depth[b];
  }
  t->max_depth = maxd;
  return PBHC_OK;
}

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
  memset(&sk, 0, sizeof(sk));
  sk.num_bodies = B;
  for (int b = 0; b < B; ++b) {
    sk.parent[b] = skel->parent[b]; sk.depth[b] = skel->depth[b];
    for (int k = 0; k < 3; ++k) sk.offset[b][k] = skel->offset[b][k];
    for (int k = 0; k < 4; ++k) sk.lq_xyzw[b][k] = skel->local_rot_wxyz[b][(k + 1) & 3];
    if (b >= 1) {
      const float* ax = skel->dof_axis[b - 1];
      const float nrm = fmaxf(sqrtf(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]), 1e-9f);
      for (int k = 0; k < 3; ++k) sk.axis[b][k] = ax[k] / nrm;
      if (enforce_limits) { sk.limits[b][0] = limits[2 * (b - 1)]; sk.limits[b][1] = limits[2 * (b - 1) + 1]; }
    }
  }
  hipLaunchKernelGGL(k_art_debug, dim3((n + CL_EPB - 1) / CL_EPB), dim3(PBHC_G * CL_EPB), 0, (hipStream_t)stream, sk, *p, tree, base, q, v, tau, n,
                     steps, h, enforce_limits, out_q, out_v, out_qdd0);
  if (hipGetLastError() != hipSuccess) {
    snprintf(g_pbhc_err, sizeof(g_pbhc_err), "pbhc_debug_articulated_substeps: launch failed");
    return PBHC_EHIP;
  }
  return PBHC_OK;
}
