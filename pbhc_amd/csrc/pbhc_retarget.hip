// pbhc_retarget.hip — fit robot joint angles to key-point targets at ingestion (reference: smpl_retarget/phc_retarget/fit_smpl_motion.py
// :137-179, gradient descent through Humanoid_Batch.fk_batch; restated in DESIGN §8 "Retargeting").  Two launches per iteration:
//
//   k_retarget_frame  one wave per frame (RT_FPB frames per workgroup), lane = body.  Every body lane forms its local rotation
//                     (k_motion_fk's own functions on pose_aa = axis * dof), the local matrices meet in LDS, every lane walks its own chain
//                     root -> body: positions equal k_motion_fk's bit for bit.  Lanes < P form the unit residuals u of the picks; body lane
//                     b then sums (p_pick - p_b) x u over the picks of its subtree (a 64-bit pick mask per body, pick order) — the hinge
//                     gradient is that sum dotted with the world axis, the root's is J_l(w)^T applied to it (lane 0, in double).  In the
//                     fitting form the same lanes take the Adadelta / Adam step and the clamp; lanes 40..43 write the frame's four partial
//                     sums (u.x, u.y, u.z, |diff|) in pick order.
//   k_retarget_clip   one workgroup per clip: the frame partials of the clip, thread t taking frames t, t + 256, ... of the clip and an LDS
//                     tree over the threads — an order that depends on the clip's frame count only — then the loss, the Adam step of the
//                     clip's root offset, and the 5-tap edge-replicated Gaussian filter of the clamped joints (read from the pre-filter
//                     buffer the frame launch wrote, written to the state).  ONE workgroup walks the whole clip: fine for clips of hundreds
//                     of frames (19 us for 256 x 300); a single clip of very many frames would serialise its N * D * 5 loads on one CU.
//   k_retarget_finish the final clamp and the outputs (pose_aa, root translation, root quaternion), once.
//
// No atomics; nothing depends on where a clip lies in the batch but its own frame count and its own root offset, so a clip fitted alone and
// inside a batch gives the same bits.  All iterations are enqueued back to back: the bias corrections of Adam are kernel arguments.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <stdio.h>

#include "../../include/pbhc_hip.h"
#include "pbhc_math.h"

using namespace pbhc;

extern thread_local char g_pbhc_err[512];
extern "C" int pbhc_check_skel(const PbhcSkeleton* sk);            // pbhc_kernels.hip

#define RT_THREADS 256
#define RT_FPB (RT_THREADS / 64)                                   // frames per workgroup: one wave each
#define RT_SUM_LANE 40                                             // lanes 40..43: the frame's partial sums (PBHC_MAX_BODIES <= 40)
static_assert(PBHC_MAX_BODIES <= RT_SUM_LANE && PBHC_MAX_BODIES <= 64, "lane roles");

// what the kernels read of the skeleton and the parameters, by value (2.6 KB; PbhcSkeleton + PbhcRetargetParams would not fit a kernarg)
struct RtTables {
  float offset[PBHC_MAX_BODIES][3];
  float lrot[PBHC_MAX_BODIES][4];                                  // wxyz
  float axis[PBHC_MAX_DOF][3];
  float limits[PBHC_MAX_DOF][2];
  unsigned long long desc[PBHC_MAX_BODIES];                        // bit l: pick l lies in the subtree of body b (body 0: every pick)
  uint8_t chain_len[PBHC_MAX_BODIES];
  uint8_t chain[PBHC_MAX_BODIES][PBHC_MAX_DEPTH];
  uint8_t pick[PBHC_MAX_BODIES];
  int32_t Bx, B, D, P, taps;
  float dof_lr, root_lr, rho, ad_eps, beta1, beta2, adam_eps;
  float w[5];
};

struct RtIO {
  const float* kp;                                                 // [total, P, 3]
  const float* trans;                                              // [total, 3]
  const float* dof;                                                // [total, D]
  float* root_rot;                                                 // [total, 3] (fit: updated in place; loss_grad: read only)
  const float* root_off;                                           // [M, 3]
  const int32_t* starts;                                           // [M + 1] device
  float* part;                                                     // [total, 4]
  float* o_dof;                                                    // fit: the clamped joints before the filter; loss_grad: g_dof
  float* o_root;                                                   // loss_grad: g_root_rot
  float *sq, *acc, *rm, *rv;                                       // fit: optimiser state
  float* body_pos;                                                 // [total, Bx, 3] or NULL
  int32_t total, M;
  float bc1, bc2s;                                                 // fit: 1 - beta1^t, sqrt(1 - beta2^t)
};

__device__ __forceinline__ int rt_clip_of(const int32_t* __restrict__ starts, int M, int f) {
  int lo = 0, hi = M;                                              // starts[lo] <= f < starts[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (starts[mid] <= f) lo = mid; else hi = mid;
  }
  return lo;
}

// torch.optim.Adam, one element: -> the new parameter
__device__ __forceinline__ float rt_adam(float p, float g, float* m, float* v, float lr, float b1, float b2, float eps, float bc1, float bc2s) {
  *m = b1 * *m + (1.0f - b1) * g;
  *v = b2 * *v + (1.0f - b2) * g * g;
  const float denom = sqrtf(*v) / bc2s + eps;
  return p - (lr / bc1) * (*m / denom);
}

template <bool UPDATE>
__global__ __launch_bounds__(RT_THREADS) void k_retarget_frame(RtTables t, RtIO io) {
  __shared__ float sM[RT_FPB][PBHC_MAX_BODIES][9];
  __shared__ float sP[RT_FPB][PBHC_MAX_BODIES][3];
  __shared__ float sU[RT_FPB][PBHC_MAX_BODIES][4];
  const int w = threadIdx.x >> 6, b = threadIdx.x & 63;
  const int f = blockIdx.x * RT_FPB + w;
  const bool valid = f < io.total;
  const size_t fi = valid ? f : io.total - 1;                      // a wave past the end recomputes the last frame and stores nothing
  const int c = rt_clip_of(io.starts, io.M, (int)fi);
  const int Nc = io.starts[c + 1] - io.starts[c];
  const float inv = 1.0f / (float)(Nc * t.P);
  const int Bx = t.Bx, D = t.D;
  float q = 0.0f, rr[3] = {0.0f, 0.0f, 0.0f};
  if (b < Bx) {
    float aa[3] = {0.0f, 0.0f, 0.0f};
    if (b == 0) {
      rr[0] = io.root_rot[fi * 3 + 0]; rr[1] = io.root_rot[fi * 3 + 1]; rr[2] = io.root_rot[fi * 3 + 2];
      aa[0] = rr[0]; aa[1] = rr[1]; aa[2] = rr[2];
    } else if (b <= D) {
      q = io.dof[fi * D + (b - 1)];
      aa[0] = t.axis[b - 1][0] * q; aa[1] = t.axis[b - 1][1] * q; aa[2] = t.axis[b - 1][2] * q;
    }
    float qw[4];
    axis_angle_to_quat_wxyz(aa[0], aa[1], aa[2], qw);
    m33 J = quat_wxyz_to_matrix(qw[0], qw[1], qw[2], qw[3]);
    if (b > 0) J = matmul33(quat_wxyz_to_matrix(t.lrot[b][0], t.lrot[b][1], t.lrot[b][2], t.lrot[b][3]), J);
#pragma unroll
    for (int k = 0; k < 9; ++k) sM[w][b][k] = J.m[k];
  }
  __syncthreads();
  m33 R;
  float P[3] = {0.0f, 0.0f, 0.0f};
  if (b < Bx) {
#pragma unroll
    for (int k = 0; k < 9; ++k) R.m[k] = sM[w][0][k];
    // (+ 0 is exact: with a zero offset the root is `trans` itself, as the build's FK has it)
    P[0] = io.trans[fi * 3 + 0] + io.root_off[c * 3 + 0];
    P[1] = io.trans[fi * 3 + 1] + io.root_off[c * 3 + 1];
    P[2] = io.trans[fi * 3 + 2] + io.root_off[c * 3 + 2];
    const int len = t.chain_len[b] + (b >= t.B ? 1 : 0);           // an extended body: its parent's chain, then itself
    for (int k = 0; k < len; ++k) {
      const int i = k < t.chain_len[b] ? t.chain[b][k] : b;
      const float* o = t.offset[i];
      const float px = R.m[0] * o[0] + R.m[1] * o[1] + R.m[2] * o[2] + P[0];
      const float py = R.m[3] * o[0] + R.m[4] * o[1] + R.m[5] * o[2] + P[1];
      const float pz = R.m[6] * o[0] + R.m[7] * o[1] + R.m[8] * o[2] + P[2];
      P[0] = px; P[1] = py; P[2] = pz;
      m33 L;
#pragma unroll
      for (int e = 0; e < 9; ++e) L.m[e] = sM[w][i][e];
      R = matmul33(R, L);
    }
    sP[w][b][0] = P[0]; sP[w][b][1] = P[1]; sP[w][b][2] = P[2];
    if (io.body_pos && valid) {
      float* bp = io.body_pos + (fi * Bx + b) * 3;
      bp[0] = P[0]; bp[1] = P[1]; bp[2] = P[2];
    }
  }
  __syncthreads();
  if (b < t.P) {
    const int pb = t.pick[b];
    const float* tg = io.kp + (fi * t.P + b) * 3;
    const float dx = sP[w][pb][0] - tg[0], dy = sP[w][pb][1] - tg[1], dz = sP[w][pb][2] - tg[2];
    const float n = sqrtf(dx * dx + dy * dy + dz * dz);
    const bool nz = n > 0.0f;
    sU[w][b][0] = nz ? dx / n : 0.0f; sU[w][b][1] = nz ? dy / n : 0.0f; sU[w][b][2] = nz ? dz / n : 0.0f; sU[w][b][3] = n;
  }
  __syncthreads();
  if (b >= RT_SUM_LANE && b < RT_SUM_LANE + 4) {                   // the frame's partial sums, in pick order
    float s = 0.0f;
    for (int l = 0; l < t.P; ++l) s += sU[w][l][b - RT_SUM_LANE];
    if (valid) io.part[fi * 4 + (b - RT_SUM_LANE)] = s;
  }
  if (b >= t.B) return;
  float tau[3] = {0.0f, 0.0f, 0.0f};                               // sum over the picks of this body's subtree of (p_pick - p_b) x u
  const unsigned long long mask = t.desc[b];
  for (int l = 0; l < t.P; ++l) {
    if (!((mask >> l) & 1ull)) continue;
    const int pb = t.pick[l];
    const float rx = sP[w][pb][0] - P[0], ry = sP[w][pb][1] - P[1], rz = sP[w][pb][2] - P[2];
    const float ux = sU[w][l][0], uy = sU[w][l][1], uz = sU[w][l][2];
    tau[0] += ry * uz - rz * uy; tau[1] += rz * ux - rx * uz; tau[2] += rx * uy - ry * ux;
  }
  if (b == 0) {
    // J_l(w)^T tau = tau - A (w x tau) + Bc w x (w x tau), A = (1 - cos th) / th^2, Bc = (th - sin th) / th^3; in double, series below 1e-2
    const double wx = rr[0], wy = rr[1], wz = rr[2], t2 = wx * wx + wy * wy + wz * wz, th = sqrt(t2);
    double A, Bc;
    if (th < 1e-2) {
      A = 0.5 - t2 / 24.0 + t2 * t2 / 720.0;
      Bc = 1.0 / 6.0 - t2 / 120.0 + t2 * t2 / 5040.0;
    } else {
      A = (1.0 - cos(th)) / t2;
      Bc = (th - sin(th)) / (t2 * th);
    }
    const double tx = tau[0], ty = tau[1], tz = tau[2];
    const double c1x = wy * tz - wz * ty, c1y = wz * tx - wx * tz, c1z = wx * ty - wy * tx;
    const double c2x = wy * c1z - wz * c1y, c2y = wz * c1x - wx * c1z, c2z = wx * c1y - wy * c1x;
    const float g[3] = {(float)(tx - A * c1x + Bc * c2x) * inv, (float)(ty - A * c1y + Bc * c2y) * inv, (float)(tz - A * c1z + Bc * c2z) * inv};
    if (!valid) return;
    if constexpr (UPDATE) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        float m = io.rm[fi * 3 + k], v = io.rv[fi * 3 + k];
        io.root_rot[fi * 3 + k] = rt_adam(rr[k], g[k], &m, &v, t.root_lr, t.beta1, t.beta2, t.adam_eps, io.bc1, io.bc2s);
        io.rm[fi * 3 + k] = m; io.rv[fi * 3 + k] = v;
      }
    } else {
      io.o_root[fi * 3 + 0] = g[0]; io.o_root[fi * 3 + 1] = g[1]; io.o_root[fi * 3 + 2] = g[2];
    }
    return;
  }
  const int j = b - 1;
  const float* a = t.axis[j];                                      // world axis of hinge j: W_b a (the hinge's own turn leaves a where it is)
  const float wx = R.m[0] * a[0] + R.m[1] * a[1] + R.m[2] * a[2], wy = R.m[3] * a[0] + R.m[4] * a[1] + R.m[5] * a[2],
              wz = R.m[6] * a[0] + R.m[7] * a[1] + R.m[8] * a[2];
  const float g = (wx * tau[0] + wy * tau[1] + wz * tau[2]) * inv;
  if (!valid) return;
  const size_t e = fi * D + j;
  if constexpr (UPDATE) {                                          // torch.optim.Adadelta, then the clamp
    const float sq = t.rho * io.sq[e] + (1.0f - t.rho) * g * g;
    const float ac = io.acc[e];
    const float delta = sqrtf(ac + t.ad_eps) / sqrtf(sq + t.ad_eps) * g;
    io.sq[e] = sq;
    io.acc[e] = t.rho * ac + (1.0f - t.rho) * delta * delta;
    io.o_dof[e] = fminf(fmaxf(q - t.dof_lr * delta, t.limits[j][0]), t.limits[j][1]);
  } else {
    io.o_dof[e] = g;
  }
}

struct RtClipIO {
  const float* part;                                               // [total, 4]
  const int32_t* starts;
  float* loss;                                                     // [M]: loss_history row / loss_out
  float* root_off;                                                 // fit: [M, 3] updated; loss_grad: g_root_off
  float *om, *ov;                                                  // fit: Adam state of the offset
  const float* pre;                                                // fit: clamped joints before the filter
  float* dof;                                                      // fit: the state's joints
  float bc1, bc2s;
};

template <bool UPDATE>
__global__ __launch_bounds__(RT_THREADS) void k_retarget_clip(RtTables t, RtClipIO io) {
  __shared__ float red[RT_THREADS][4];
  const int c = blockIdx.x, tid = threadIdx.x;
  const int a = io.starts[c], N = io.starts[c + 1] - a;
  float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int i = tid; i < N; i += RT_THREADS) {
    const float* p = io.part + (size_t)(a + i) * 4;
    s[0] += p[0]; s[1] += p[1]; s[2] += p[2]; s[3] += p[3];
  }
  red[tid][0] = s[0]; red[tid][1] = s[1]; red[tid][2] = s[2]; red[tid][3] = s[3];
  __syncthreads();
  for (int h = RT_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) { red[tid][0] += red[tid + h][0]; red[tid][1] += red[tid + h][1]; red[tid][2] += red[tid + h][2]; red[tid][3] += red[tid + h][3]; }
    __syncthreads();
  }
  if (tid < 4) {
    const float inv = 1.0f / (float)(N * t.P);
    const float v = red[0][tid] * inv;
    if (tid == 3) {
      io.loss[c] = v;
    } else if constexpr (UPDATE) {
      float m = io.om[c * 3 + tid], vv = io.ov[c * 3 + tid];
      io.root_off[c * 3 + tid] = rt_adam(io.root_off[c * 3 + tid], v, &m, &vv, t.root_lr, t.beta1, t.beta2, t.adam_eps, io.bc1, io.bc2s);
      io.om[c * 3 + tid] = m; io.ov[c * 3 + tid] = vv;
    } else {
      io.root_off[c * 3 + tid] = v;
    }
  }
  if constexpr (UPDATE) {
    const int D = t.D;
    for (int e = tid; e < N * D; e += RT_THREADS) {
      const int i = e / D, d = e - i * D;
      float v;
      if (t.taps == 5) {                                           // edge-replicated at the clip's own first and last frame
        v = 0.0f;
#pragma unroll
        for (int k = 0; k < 5; ++k) v += t.w[k] * io.pre[(size_t)(a + min(max(i + k - 2, 0), N - 1)) * D + d];
      } else {
        v = io.pre[(size_t)(a + i) * D + d];
      }
      // (a weighted mean of clamped values lies inside the limits; clamping it again only takes off what rounding added)
      io.dof[(size_t)(a + i) * D + d] = fminf(fmaxf(v, t.limits[d][0]), t.limits[d][1]);
    }
  }
}

// the final clamp and the outputs: one thread per (frame, body)
__global__ __launch_bounds__(RT_THREADS) void k_retarget_finish(RtTables t, const float* __restrict__ trans, const int32_t* __restrict__ starts, int M,
                                                                int total, float* __restrict__ dof, const float* __restrict__ root_rot,
                                                                const float* __restrict__ root_off, float* __restrict__ pose,
                                                                float* __restrict__ out_trans, float* __restrict__ out_quat) {
  const size_t g = (size_t)blockIdx.x * RT_THREADS + threadIdx.x;
  if (g >= (size_t)total * t.Bx) return;
  const size_t f = g / t.Bx;
  const int b = (int)(g - f * t.Bx);
  float v[3] = {0.0f, 0.0f, 0.0f};
  if (b == 0) {
    v[0] = root_rot[f * 3 + 0]; v[1] = root_rot[f * 3 + 1]; v[2] = root_rot[f * 3 + 2];
    const int c = rt_clip_of(starts, M, (int)f);
    for (int k = 0; k < 3; ++k) out_trans[f * 3 + k] = trans[f * 3 + k] + root_off[c * 3 + k];
    float qw[4];
    axis_angle_to_quat_wxyz(v[0], v[1], v[2], qw);
    out_quat[f * 4 + 0] = qw[1]; out_quat[f * 4 + 1] = qw[2]; out_quat[f * 4 + 2] = qw[3]; out_quat[f * 4 + 3] = qw[0];
  } else if (b <= t.D) {
    const int j = b - 1;
    const float q = fminf(fmaxf(dof[f * t.D + j], t.limits[j][0]), t.limits[j][1]);
    dof[f * t.D + j] = q;
    v[0] = t.axis[j][0] * q; v[1] = t.axis[j][1] * q; v[2] = t.axis[j][2] * q;
  }
  pose[g * 3 + 0] = v[0]; pose[g * 3 + 1] = v[1]; pose[g * 3 + 2] = v[2];
}

#define RT_FAIL(...)                                         \
  do {                                                       \
    snprintf(g_pbhc_err, sizeof(g_pbhc_err), __VA_ARGS__);   \
    return PBHC_EINVAL;                                      \
  } while (0)

// every refusal of the exports, and the by-value tables; no GPU call
static int rt_prepare(const char* who, const PbhcSkeleton* sk, const PbhcRetargetParams* p, int total, int num_clips, const int32_t* starts,
                      RtTables* t) {
  const int rc = pbhc_check_skel(sk);                              // Bx <= PBHC_MAX_BODIES, D == B - 1 <= PBHC_MAX_DOF, the chain tables
  if (rc) return rc;
  if (!p || !starts) RT_FAIL("%s: bad argument (NULL params or starts)", who);
  if (p->num_picks < 1 || p->num_picks > PBHC_MAX_BODIES) RT_FAIL("%s: bad argument (num_picks %d outside 1..%d)", who, p->num_picks, PBHC_MAX_BODIES);
  for (int l = 0; l < p->num_picks; ++l)
    if (p->pick[l] < 0 || p->pick[l] >= sk->num_bodies_ext)
      RT_FAIL("%s: bad argument (pick %d is body %d, outside [0, %d))", who, l, p->pick[l], sk->num_bodies_ext);
  if (p->filter_taps != 0 && p->filter_taps != 5) RT_FAIL("%s: bad argument (filter_taps %d, not 0 or 5)", who, p->filter_taps);
  if (p->filter_taps == 5 && !(p->filter_sigma > 0.0f && p->filter_sigma < 1e6f)) RT_FAIL("%s: bad argument (filter_sigma %g)", who, p->filter_sigma);
  for (int d = 0; d < sk->num_dof; ++d)
    if (!(p->limits[d][0] <= p->limits[d][1])) RT_FAIL("%s: bad argument (limits of dof %d: lo %g > hi %g)", who, d, p->limits[d][0], p->limits[d][1]);
  if (num_clips < 1 || total < 1 || starts[0] != 0) RT_FAIL("%s: bad argument (%d clips, %d frames, starts[0] %d)", who, num_clips, total, starts[0]);
  for (int c = 0; c < num_clips; ++c)
    if (starts[c + 1] <= starts[c]) RT_FAIL("%s: bad argument (clip %d has %d frames)", who, c, starts[c + 1] - starts[c]);
  if (starts[num_clips] != total) RT_FAIL("%s: bad argument (total %d is not starts[%d] = %d)", who, total, num_clips, starts[num_clips]);
  if ((long long)total * sk->num_bodies_ext * 3 >= (1ll << 31)) RT_FAIL("%s: bad argument (%d frames: over 2^31 pose elements)", who, total);
  memset(t, 0, sizeof(*t));
  t->Bx = sk->num_bodies_ext; t->B = sk->num_bodies; t->D = sk->num_dof; t->P = p->num_picks; t->taps = p->filter_taps;
  t->dof_lr = p->dof_lr; t->root_lr = p->root_lr; t->rho = p->rho; t->ad_eps = p->adadelta_eps;
  t->beta1 = p->beta1; t->beta2 = p->beta2; t->adam_eps = p->adam_eps;
  for (int b = 0; b < t->Bx; ++b) {
    for (int k = 0; k < 3; ++k) t->offset[b][k] = sk->offset[b][k];
    for (int k = 0; k < 4; ++k) t->lrot[b][k] = sk->local_rot_wxyz[b][k];
    t->chain_len[b] = (uint8_t)sk->chain_len[b];
    for (int k = 0; k < sk->chain_len[b]; ++k) t->chain[b][k] = (uint8_t)sk->chain[b][k];
  }
  for (int d = 0; d < t->D; ++d) {
    for (int k = 0; k < 3; ++k) t->axis[d][k] = sk->dof_axis[d][k];
    t->limits[d][0] = p->limits[d][0]; t->limits[d][1] = p->limits[d][1];
  }
  for (int l = 0; l < t->P; ++l) {
    const int pb = p->pick[l];
    t->pick[l] = (uint8_t)pb;
    t->desc[0] |= 1ull << l;
    for (int k = 0; k < sk->chain_len[pb]; ++k) t->desc[sk->chain[pb][k]] |= 1ull << l;
  }
  if (t->taps == 5) {
    double w[5], sum = 0.0;
    for (int k = 0; k < 5; ++k) { w[k] = exp(-(double)((k - 2) * (k - 2)) / (2.0 * (double)p->filter_sigma * (double)p->filter_sigma)); sum += w[k]; }
    for (int k = 0; k < 5; ++k) t->w[k] = (float)(w[k] / sum);
  }
  return PBHC_OK;
}

extern "C" int pbhc_sizeof_retarget_params(void) { return (int)sizeof(PbhcRetargetParams); }
extern "C" int pbhc_sizeof_retarget_state(void) { return (int)sizeof(PbhcRetargetState); }

extern "C" int pbhc_retarget_loss_grad(const PbhcSkeleton* skel, const PbhcRetargetParams* params, const float* keypoints, const float* trans,
                                       const float* dof, const float* root_rot, const float* root_off, int total, int num_clips,
                                       const int32_t* starts, const int32_t* d_starts, float* loss_out, float* g_dof, float* g_root_rot,
                                       float* g_root_off, float* body_pos_out, float* scratch, void* stream) {
  RtTables t;
  const int rc = rt_prepare("pbhc_retarget_loss_grad", skel, params, total, num_clips, starts, &t);
  if (rc) return rc;
  if (!keypoints || !trans || !dof || !root_rot || !root_off || !d_starts || !loss_out || !g_dof || !g_root_rot || !g_root_off || !scratch)
    RT_FAIL("pbhc_retarget_loss_grad: bad argument (NULL pointer)");
  RtIO io{};
  io.kp = keypoints; io.trans = trans; io.dof = dof; io.root_rot = const_cast<float*>(root_rot); io.root_off = root_off; io.starts = d_starts;
  io.part = scratch; io.o_dof = g_dof; io.o_root = g_root_rot; io.body_pos = body_pos_out; io.total = total; io.M = num_clips;
  RtClipIO cio{};
  cio.part = scratch; cio.starts = d_starts; cio.loss = loss_out; cio.root_off = g_root_off;
  hipLaunchKernelGGL(k_retarget_frame<false>, dim3((total + RT_FPB - 1) / RT_FPB), dim3(RT_THREADS), 0, (hipStream_t)stream, t, io);
  hipLaunchKernelGGL(k_retarget_clip<false>, dim3(num_clips), dim3(RT_THREADS), 0, (hipStream_t)stream, t, cio);
  if (hipGetLastError() != hipSuccess) return PBHC_EHIP;
  return PBHC_OK;
}

static int rt_state_ok(const char* who, const PbhcRetargetState* s) {
  if (!s || !s->dof || !s->dof_sq || !s->dof_acc || !s->root_rot || !s->root_m || !s->root_v || !s->root_off || !s->off_m || !s->off_v || !s->scratch ||
      s->step < 0)
    RT_FAIL("%s: bad argument (NULL state buffer or a negative step count)", who);
  return PBHC_OK;
}

extern "C" int pbhc_retarget_fit(const PbhcSkeleton* skel, const PbhcRetargetParams* params, const float* keypoints, const float* trans, int total,
                                 int num_clips, const int32_t* starts, const int32_t* d_starts, PbhcRetargetState* state, int iterations,
                                 float* loss_history, void* stream) {
  RtTables t;
  int rc = rt_prepare("pbhc_retarget_fit", skel, params, total, num_clips, starts, &t);
  if (rc) return rc;
  if ((rc = rt_state_ok("pbhc_retarget_fit", state))) return rc;
  if (!keypoints || !trans || !d_starts || !loss_history || iterations < 1) RT_FAIL("pbhc_retarget_fit: bad argument (NULL pointer or %d iterations)", iterations);
  RtIO io{};
  io.kp = keypoints; io.trans = trans; io.dof = state->dof; io.root_rot = state->root_rot; io.root_off = state->root_off; io.starts = d_starts;
  io.part = state->scratch; io.o_dof = state->scratch + (size_t)total * 4; io.sq = state->dof_sq; io.acc = state->dof_acc;
  io.rm = state->root_m; io.rv = state->root_v; io.total = total; io.M = num_clips;
  RtClipIO cio{};
  cio.part = io.part; cio.starts = d_starts; cio.root_off = state->root_off; cio.om = state->off_m; cio.ov = state->off_v; cio.pre = io.o_dof;
  cio.dof = state->dof;
  for (int it = 0; it < iterations; ++it) {
    const double step = (double)(state->step + it + 1);
    io.bc1 = cio.bc1 = (float)(1.0 - pow((double)params->beta1, step));
    io.bc2s = cio.bc2s = (float)sqrt(1.0 - pow((double)params->beta2, step));
    cio.loss = loss_history + (size_t)it * num_clips;
    hipLaunchKernelGGL(k_retarget_frame<true>, dim3((total + RT_FPB - 1) / RT_FPB), dim3(RT_THREADS), 0, (hipStream_t)stream, t, io);
    hipLaunchKernelGGL(k_retarget_clip<true>, dim3(num_clips), dim3(RT_THREADS), 0, (hipStream_t)stream, t, cio);
  }
  if (hipGetLastError() != hipSuccess) return PBHC_EHIP;
  state->step += iterations;
  return PBHC_OK;
}

extern "C" int pbhc_retarget_finish(const PbhcSkeleton* skel, const PbhcRetargetParams* params, const float* trans, int total, int num_clips,
                                    const int32_t* starts, const int32_t* d_starts, PbhcRetargetState* state, float* pose_aa_out,
                                    float* root_trans_out, float* root_quat_out, void* stream) {
  RtTables t;
  int rc = rt_prepare("pbhc_retarget_finish", skel, params, total, num_clips, starts, &t);
  if (rc) return rc;
  if ((rc = rt_state_ok("pbhc_retarget_finish", state))) return rc;
  if (!trans || !d_starts || !pose_aa_out || !root_trans_out || !root_quat_out) RT_FAIL("pbhc_retarget_finish: bad argument (NULL pointer)");
  const size_t n = (size_t)total * t.Bx;
  hipLaunchKernelGGL(k_retarget_finish, dim3((unsigned)((n + RT_THREADS - 1) / RT_THREADS)), dim3(RT_THREADS), 0, (hipStream_t)stream, t, trans, d_starts,
                     num_clips, total, state->dof, state->root_rot, state->root_off, pose_aa_out, root_trans_out, root_quat_out);
  if (hipGetLastError() != hipSuccess) return PBHC_EHIP;
  return PBHC_OK;
}
