// pbhc_art_dynamics.h — the tree's forward dynamics, shared by the articulated simulator (pbhc_articulated_sim.hip: the base prescribed,
// FREE = false) and the floating-base simulator (pbhc_floating_sim.hip: the root six more degrees of freedom of the same tree and ground
// contact at points on the links, FREE = true).  Included after pbhc_math.h, pbhc_env_step.h (PBHC_G) and pbhc_closed_loop.h (CL_CHECK).
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
//                            of the bias force (the sum into a prescribed root is skipped)
//   pass 3 (root -> leaves)  a' = shift(a_parent) + c, qdd = (u - U.a') / D, a = a' + S qdd;  the root's a = [alpha_0; a_0 - g]
// (The base's linear velocity is left out: a constant velocity of the whole frame changes no joint acceleration.)
// FREE adds: in pass 1 the link origin's position relative to the root's origin (the sum of the d's: for the contact points' heights); after
// pass 1 the contact points' forces from the state at the start of the sub-step, which enter the link's bias force as p -= [r x f; f] about
// the link's own origin, in point order; in pass 2 the sum into the root as well, whose own mass and inertia count, and the root's symmetric
// 6 x 6 system I^A_0 a = -p^A_0 by an unrolled LDL^T in registers (the linear block first: its pivots are masses, and what is left for the
// angular block is the inertia about the centre of mass); pass 3 starts from that a.  Gravity enters both variants the same way: the root's
// linear acceleration is a_0 - g, so the solved one gets g added back.  The root's linear velocity enters the points' velocities only.
// Per-lane state lives in registers; parent -> child and child -> parent traffic goes by __shfl inside the env's 32 lanes (always the same
// wave): a parent reads its children one after the other through a first-child / next-sibling list, in index order, so the sums are
// reproducible.  No LDS, no runtime-indexed per-thread arrays.
#pragma once

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
// the debug kernels' copy of what the sim kernels read from the env's config
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
struct ArtBase { f4 R0; f3 w0, alpha0, a0g; };              // a0g = a_0 - g (FREE: R0, w0 are the root's state; alpha0, a0g are not read)
// FREE only: the lane's contact points, the contact law, the rest of the root's state (the same on every lane of the env), and what one
// sub-step leaves: its points' forces and the root's accelerations
#define ART_MAX_POINTS 4
struct ArtFloat {
  int npts;
  f3 r0, r1, r2, r3;                                        // body frame (named, not an array: every member stays in registers)
  float stiffness, normal_damping, friction, slip_velocity, ground_height;
  f3 g;
  f3 p0, v0;                                                // world position and linear velocity of the root's origin
  f3 f0, f1, f2, f3_;                                       // out: world force on each point (0 for a point the lane does not have)
  f3 a0, alpha0;                                            // out: d v_0 / dt, d w_0 / dt
};

// x of the symmetric positive definite 6 x 6 system K x = b, K given by its lower triangle: LDL^T, every index a compile-time constant
__device__ __forceinline__ void art_ldl6(float (&K)[6][6], float (&b)[6]) {
#pragma unroll
  for (int j = 0; j < 6; ++j) {
#pragma unroll
    for (int k = 0; k < j; ++k) K[j][j] -= K[j][k] * K[j][k] * K[k][k];
    const float rd = 1.0f / K[j][j];
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
#pragma unroll
      for (int k = 0; k < j; ++k) K[i][j] -= K[i][k] * K[j][k] * K[k][k];
      K[i][j] *= rd;
    }
  }
#pragma unroll
  for (int i = 1; i < 6; ++i) {
#pragma unroll
    for (int k = 0; k < i; ++k) b[i] -= K[i][k] * b[k];
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) b[i] /= K[i][i];
#pragma unroll
  for (int i = 4; i >= 0; --i) {
#pragma unroll
    for (int k = i + 1; k < 6; ++k) b[i] -= K[k][i] * b[k];
  }
}

// One sub-step of the definition: (q, v) of the lane's hinge under the torque `tau`; returns dv / h.  FREE: the root's state (base.R0, base.w0,
// X.p0, X.v0) is read, X.f, X.a0, X.alpha0 are written; the caller integrates the root (art_integrate_root).
template <bool FREE>
__device__ __forceinline__ float art_substep(const ArtLane& L, const ArtTree& T, const ArtBase& base, ArtFloat& X, int lane, float h, float tau,
                                             bool enforce_limits, float& q, float& v) {
  const f3 zero = mk3(0.0f, 0.0f, 0.0f);
  const bool body = FREE ? L.depth >= 0 : L.depth >= 1;
  // ---- pass 1: orientation, offset from the parent's origin, axis, velocity (of the link's own origin), velocity-product acceleration
  const f4 relq = quat_mul(L.lq, quat_from_angle_unit_axis(q, L.axis));
  f4 R = base.R0;
  f3 d = zero, vw = base.w0, vl = zero, cw = zero, cl = zero, Sa = zero;
  f3 pos = zero;                                             // FREE: the link's origin relative to the root's
  for (int lev = 1; lev <= T.max_depth; ++lev) {
    const f4 Rp = shf4(R, L.parent);
    const f3 vwp = shf3(vw, L.parent), vlp = shf3(vl, L.parent);
    f3 posp = zero;
    if (FREE) posp = shf3(pos, L.parent);
    if (L.depth == lev) {
      d = fk_rotate(Rp, L.off);                              // the FK's own chain (fk_walk): the product renormalised at every level — without
      R = fk_mul_unit(Rp, relq);                             // it the quaternion's norm drifts by ~1e-6 down a limb and |S|^2 with it
      Sa = fk_rotate(R, L.axis);
      const f3 jw = mul3(Sa, v);
      vw = add3(vwp, jw);
      vl = add3(vlp, cross3(vwp, d));
      cw = cross3(vwp, jw);
      cl = cross3(vl, jw);
      if (FREE) pos = add3(posp, d);
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
    if (FREE) {
      // ---- the lane's contact points, from the state at the start of the sub-step, in point order
#define ART_POINT(k, rk, fk)                                                                                                                   \
  {                                                                                                                                            \
    const f3 rw = mk3(r.m00 * rk.x + r.m01 * rk.y + r.m02 * rk.z, r.m10 * rk.x + r.m11 * rk.y + r.m12 * rk.z,                                  \
                      r.m20 * rk.x + r.m21 * rk.y + r.m22 * rk.z);                                                                             \
    const f3 xd = add3(add3(X.v0, vl), cross3(vw, rw));                                                                                        \
    const float delta = X.ground_height - ((X.p0.z + pos.z) + rw.z);                                                                           \
    f3 f = zero;                                                                                                                               \
    if (k < X.npts && delta > 0.0f) {                                                                                                          \
      const float fn = fmaxf(0.0f, X.stiffness * delta - X.normal_damping * xd.z);                                                             \
      const float sc = (X.friction * fn) / fmaxf(sqrtf(xd.x * xd.x + xd.y * xd.y), X.slip_velocity);                                           \
      f = mk3(-(sc * xd.x), -(sc * xd.y), fn);                                                                                                 \
    }                                                                                                                                          \
    fk = f;                                                                                                                                    \
    pw = sub3(pw, cross3(rw, f));                                                                                                              \
    pl = sub3(pl, f);                                                                                                                          \
  }
      ART_POINT(0, X.r0, X.f0) ART_POINT(1, X.r1, X.f1) ART_POINT(2, X.r2, X.f2) ART_POINT(3, X.r3, X.f3_)
#undef ART_POINT
    }
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
    if (FREE || lev >= 2) {                                  // (a prescribed root: nothing is summed into it)
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
  if (FREE) {
    // the root's own system  [M H^T; H A] [a_0 - g; alpha_0] = -[p_lin; p_ang]  (on every lane; lane 0's is the root's)
    float K[6][6], b[6];
    K[0][0] = M.xx; K[1][0] = M.xy; K[1][1] = M.yy; K[2][0] = M.xz; K[2][1] = M.yz; K[2][2] = M.zz;
    K[3][0] = H.m00; K[3][1] = H.m01; K[3][2] = H.m02; K[4][0] = H.m10; K[4][1] = H.m11; K[4][2] = H.m12;
    K[5][0] = H.m20; K[5][1] = H.m21; K[5][2] = H.m22;
    K[3][3] = A.xx; K[4][3] = A.xy; K[4][4] = A.yy; K[5][3] = A.xz; K[5][4] = A.yz; K[5][5] = A.zz;
    b[0] = -pl.x; b[1] = -pl.y; b[2] = -pl.z; b[3] = -pw.x; b[4] = -pw.y; b[5] = -pw.z;
    art_ldl6(K, b);
    al = mk3(shf(b[0], 0), shf(b[1], 0), shf(b[2], 0));
    aw = mk3(shf(b[3], 0), shf(b[4], 0), shf(b[5], 0));
    X.a0 = add3(al, X.g);
    X.alpha0 = aw;
  }
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

// FREE: the root's part of the step, from the accelerations art_substep left:  v_0 += h a_0,  w_0 += h alpha_0,  p_0 += h v_0,
// R_0 <- exp(h w_0) R_0 (the world-frame exponential map as a quaternion, renormalised)
__device__ __forceinline__ void art_integrate_root(ArtBase& base, ArtFloat& X, float h) {
  X.v0 = add3(X.v0, mul3(X.a0, h));
  base.w0 = add3(base.w0, mul3(X.alpha0, h));
  X.p0 = add3(X.p0, mul3(X.v0, h));
  const f3 hw = mul3(base.w0, 0.5f * h);                     // half the rotation vector
  const float th = norm3(hw);
  float s, c;
  sincos_cw(th, &s, &c);
  const float sc = th > 1e-6f ? s / th : 1.0f;
  base.R0 = quat_unit_fast(fk_mul(mk4(hw.x * sc, hw.y * sc, hw.z * sc, c), base.R0));
}

// `env_row` (FREE, per-env randomisation; else NULL): the lane's 16-byte aligned (mass, com_x, com_y, com_z) of this env, one 16-byte load,
// in place of p.mass[lane] and p.com[lane]; the inertia about the centre of mass stays the params'
template <typename P>
__device__ __forceinline__ void art_lane_inertial(ArtLane& L, const P& p, int lane, int dcl, float h, const float* __restrict__ env_row = nullptr) {
  if (env_row) {
    const float4 r = *reinterpret_cast<const float4*>(env_row);
    L.mass = r.x;
    L.com = mk3(r.y, r.z, r.w);
  } else {
    L.mass = p.mass[lane];
    L.com = mk3(p.com[lane][0], p.com[lane][1], p.com[lane][2]);
  }
  L.inertia.xx = p.inertia[lane][0]; L.inertia.yy = p.inertia[lane][1]; L.inertia.zz = p.inertia[lane][2];
  L.inertia.xy = p.inertia[lane][3]; L.inertia.xz = p.inertia[lane][4]; L.inertia.yz = p.inertia[lane][5];
  L.damping = p.damping[dcl];
  L.arm_h = p.armature[dcl] + h * L.damping;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
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

// the debug kernels' skeleton from the ABI's (limits: HOST [D,2] or NULL)
static void art_skel(const PbhcSkeleton& skel, const float* limits, ArtSkel* out) {
  ArtSkel& sk = *out;
  memset(&sk, 0, sizeof(sk));
  const int B = skel.num_bodies;
  sk.num_bodies = B;
  for (int b = 0; b < B; ++b) {
    sk.parent[b] = skel.parent[b]; sk.depth[b] = skel.depth[b];
    for (int k = 0; k < 3; ++k) sk.offset[b][k] = skel.offset[b][k];
    for (int k = 0; k < 4; ++k) sk.lq_xyzw[b][k] = skel.local_rot_wxyz[b][(k + 1) & 3];
    if (b >= 1) {
      const float* ax = skel.dof_axis[b - 1];
      const float nrm = fmaxf(sqrtf(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]), 1e-9f);
      for (int k = 0; k < 3; ++k) sk.axis[b][k] = ax[k] / nrm;
      if (limits) { sk.limits[b][0] = limits[2 * (b - 1)]; sk.limits[b][1] = limits[2 * (b - 1) + 1]; }
    }
  }
}
