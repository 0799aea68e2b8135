// pbhc_motion_screen.hip — contact masks and a stability screen for the source clips of a library, at ingestion (robot.motion.contact_detection,
// robot.motion.screening), before the augmentation, the extension and the build.
//
//   k_motion_screen_ground  one wave per CLIP: the FK of its first frame, lane b < B body b; ground[c] = the lowest real-body origin z
//   k_motion_screen_frames  one wave per source FRAME (SCR_FPW frames per workgroup): lane b < Bx walks chain[b] for body b's world position
//                           and rotation with the arithmetic of the build's k_motion_fk (matrices, parent before child), so a foot
//                           position here is the one the tables will hold.  The two foot lanes store foot_pos[frame][2][3]; the wave adds
//                           up the sums below (butterfly over the 64 lanes, every lane the same total), lane 0 stores dist[frame]
//   k_motion_screen_clips   one workgroup per clip: mask rows from foot_pos, the report row from dist
//
// Contact (the reference's foot_detect, motion_source/count_pkl_contact_mask.py:18-38): frame 0 of a clip is 1; frame f >= 1 is 1 iff
// dx^2 + dy^2 + dz^2 < vel_threshold (float squares and sum of p_f - p_(f-1), compared in double as numpy compares a float32 array with a
// float64 threshold) and p_f.z < height_threshold.  The velocity threshold is a squared displacement per FRAME, as there.
//
// Stability distance (compute_com_cop / compute_diff of smpl_retarget/motion_filter/utils/motion_filter.py in robot space, z up; body
// origins stand in for mesh vertices, link masses for part volumes), over the real bodies b < B, sums in double:
//   com = sum m_b (p_b + R_b c_b) / sum m_b       z_b = p_b.z - ground[clip]       w_b = z_b >= 0 ? exp(-cop_w z_b) : 1 - cop_k z_b
//   cop = sum w_b p_b / (sum w_b + 1e-6)           d = |(com - cop)_xy|
// Verdict (check_conditions :60-72): frame f is stable iff d_f is finite and d_f < epsilon_stab; the clip is stable iff its first and last
// frame are and, if F > N, no two consecutive stable frames lie >= N frames apart.
// No atomics; every store is an ordinary per-lane store.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>

#include "../../include/pbhc_hip.h"
#include "pbhc_math.h"

using namespace pbhc;

extern thread_local char g_pbhc_err[512];
extern "C" int pbhc_check_skel(const PbhcSkeleton* sk);            // pbhc_kernels.hip

#define SCR_THREADS 256
#define SCR_FPW (SCR_THREADS / 64)                                 // frames per workgroup: one wave each

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_min_f32(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

// World position P and rotation W of body b (< Bx) of one frame: pose [Bx,3] rotation vectors, tr [3].  Op for op k_motion_fk's step
// P_i = W_p o_i + P_p, W_i = W_p (L_i J_i), taken along chain[b] (the real bodies from below the root down to b, or down to the parent of an
// extended b, which then takes one step of its own).
__device__ __forceinline__ void screen_fk(const PbhcSkeleton& sk, const float* __restrict__ pose, const float* __restrict__ tr, int b, float P[3],
                                          m33& W) {
  float qw[4];
  axis_angle_to_quat_wxyz(pose[0], pose[1], pose[2], qw);
  W = quat_wxyz_to_matrix(qw[0], qw[1], qw[2], qw[3]);
  P[0] = tr[0]; P[1] = tr[1]; P[2] = tr[2];
  const int len = sk.chain_len[b], steps = len + (b >= sk.num_bodies ? 1 : 0);
  for (int k = 0; k < steps; ++k) {
    const int i = k < len ? sk.chain[b][k] : b;
    const float* o = sk.offset[i];
    const float x = W.m[0] * o[0] + W.m[1] * o[1] + W.m[2] * o[2] + P[0];
    const float y = W.m[3] * o[0] + W.m[4] * o[1] + W.m[5] * o[2] + P[1];
    const float z = W.m[6] * o[0] + W.m[7] * o[1] + W.m[8] * o[2] + P[2];
    P[0] = x; P[1] = y; P[2] = z;
    axis_angle_to_quat_wxyz(pose[3 * i], pose[3 * i + 1], pose[3 * i + 2], qw);
    const m33 J = quat_wxyz_to_matrix(qw[0], qw[1], qw[2], qw[3]);
    const m33 L = quat_wxyz_to_matrix(sk.local_rot_wxyz[i][0], sk.local_rot_wxyz[i][1], sk.local_rot_wxyz[i][2], sk.local_rot_wxyz[i][3]);
    W = matmul33(W, matmul33(L, J));
  }
}

// start arrays that do not describe the input index nothing: clip c holds frames [ib, ib + F) of the `total` uploaded ones
__device__ __forceinline__ bool clip_ok(int ib, int F, int total) { return ib >= 0 && F >= 1 && F <= total - ib; }

__global__ __launch_bounds__(SCR_THREADS) void k_motion_screen_ground(PbhcSkeleton sk, const float* __restrict__ pose_aa,
                                                                      const float* __restrict__ trans, int total, int M,
                                                                      const int32_t* __restrict__ in_start, float* __restrict__ ground) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * SCR_FPW + (threadIdx.x >> 6);        // clip of this wave
  if (c >= M) return;
  const int ib = in_start[c], F = in_start[c + 1] - ib;
  if (!clip_ok(ib, F, total)) return;
  float z = INFINITY;
  if (lane < sk.num_bodies) {
    float P[3];
    m33 W;
    screen_fk(sk, pose_aa + (size_t)ib * sk.num_bodies_ext * 3, trans + (size_t)ib * 3, lane, P, W);
    z = P[2];
  }
  z = wave_min_f32(z);
  if (lane == 0) ground[c] = z;
}

__global__ __launch_bounds__(SCR_THREADS) void k_motion_screen_frames(PbhcSkeleton sk, const float* __restrict__ pose_aa,
                                                                      const float* __restrict__ trans, int total, int M,
                                                                      const int32_t* __restrict__ in_start, PbhcMotionScreen p,
                                                                      const float* __restrict__ body_mass, const float* __restrict__ body_com,
                                                                      const float* __restrict__ ground, float* __restrict__ foot_pos,
                                                                      float* __restrict__ dist) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * SCR_FPW + (threadIdx.x >> 6);        // source frame of this wave
  if (g >= total) return;
  int lo = 0, hi = M;                                             // the clip of frame g: in_start[lo] <= g < in_start[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (in_start[mid] <= g) lo = mid; else hi = mid;
  }
  const int ib = in_start[lo], F = in_start[lo + 1] - ib;
  if (!clip_ok(ib, F, total) || g < ib || g - ib >= F) return;
  const int B = sk.num_bodies, Bx = sk.num_bodies_ext;
  float P[3] = {0.0f, 0.0f, 0.0f};
  m33 W;
  if (lane < Bx) screen_fk(sk, pose_aa + (size_t)g * Bx * 3, trans + (size_t)g * 3, lane, P, W);
  if (foot_pos && lane < Bx) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
      if (lane == p.foot[j]) {
        float* o = foot_pos + (size_t)g * 6 + 3 * j;
        o[0] = P[0]; o[1] = P[1]; o[2] = P[2];
      }
  }
  if (!dist) return;                                              // (uniform: no lane leaves before the butterfly on its own)
  double sm = 0.0, smx = 0.0, smy = 0.0, sw = 0.0, swx = 0.0, swy = 0.0;
  if (lane < B) {
    const float* c = body_com + 3 * lane;
    const float cx = W.m[0] * c[0] + W.m[1] * c[1] + W.m[2] * c[2] + P[0];
    const float cy = W.m[3] * c[0] + W.m[4] * c[1] + W.m[5] * c[2] + P[1];
    sm = (double)body_mass[lane];
    smx = sm * (double)cx; smy = sm * (double)cy;
    const double z = (double)P[2] - (double)ground[lo];
    sw = z >= 0.0 ? exp(-p.cop_w * z) : 1.0 - p.cop_k * z;        // (a NaN height takes the second branch and stays NaN)
    swx = sw * (double)P[0]; swy = sw * (double)P[1];
  }
  sm = wave_sum_f64(sm); smx = wave_sum_f64(smx); smy = wave_sum_f64(smy);
  sw = wave_sum_f64(sw); swx = wave_sum_f64(swx); swy = wave_sum_f64(swy);
  if (lane == 0) {
    const double dx = smx / sm - swx / (sw + 1e-6), dy = smy / sm - swy / (sw + 1e-6);
    dist[g] = (float)sqrt(dx * dx + dy * dy);
  }
}

// what a contiguous run of frames tells the verdict: its first and last stable frame (clip-relative, -1: none) and the largest distance
// between two consecutive stable frames inside it; plus its unstable frames and its largest distance
struct ScrRun { int first, last, gap, unstable; float maxd; };

__global__ __launch_bounds__(SCR_THREADS) void k_motion_screen_clips(const float* __restrict__ foot_pos, const float* __restrict__ dist, int total,
                                                                     int M, const int32_t* __restrict__ in_start,
                                                                     const int32_t* __restrict__ derive, PbhcMotionScreen p,
                                                                     float* __restrict__ mask, float* __restrict__ report) {
  __shared__ ScrRun s_run[SCR_THREADS];
  const int c = blockIdx.x, t = threadIdx.x;
  const int ib = in_start[c], F = in_start[c + 1] - ib;
  if (!clip_ok(ib, F, total)) return;                             // (uniform over the workgroup)
  if (mask && derive[c] != 0) {
    for (int f = t; f < F; f += SCR_THREADS) {
      const float* a = foot_pos + ((size_t)ib + f) * 6;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        float v = 1.0f;
        if (f > 0) {                                              // frame f reads frame f - 1 of its own clip only
          const float dx = a[3 * j] - a[3 * j - 6], dy = a[3 * j + 1] - a[3 * j - 5], dz = a[3 * j + 2] - a[3 * j - 4];
          const float d2 = dx * dx + dy * dy + dz * dz;
          v = ((double)d2 < p.vel_threshold && (double)a[3 * j + 2] < p.height_threshold) ? 1.0f : 0.0f;
        }
        mask[((size_t)ib + f) * 2 + j] = v;
      }
    }
  }
  if (!report) return;                                            // (uniform)
  const int per = (F + SCR_THREADS - 1) / SCR_THREADS;
  const int f0 = (int)min((long long)t * per, (long long)F), f1 = (int)min((long long)f0 + per, (long long)F);
  ScrRun r = {-1, -1, 0, 0, 0.0f};
  for (int f = f0; f < f1; ++f) {
    const float d = dist[(size_t)ib + f];
    const bool fin = isfinite(d);
    r.maxd = fmaxf(r.maxd, fin ? d : INFINITY);
    if (fin && (double)d < p.epsilon_stab) {
      if (r.first < 0) r.first = f; else r.gap = max(r.gap, f - r.last);
      r.last = f;
    } else {
      r.unstable += 1;
    }
  }
  s_run[t] = r;
  __syncthreads();
  if (t != 0) return;
  ScrRun a = s_run[0];                                            // the runs in order: a gap may span any number of runs without a stable frame
  for (int k = 1; k < SCR_THREADS; ++k) {
    const ScrRun b = s_run[k];
    a.unstable += b.unstable;
    a.maxd = fmaxf(a.maxd, b.maxd);
    if (b.first < 0) continue;
    if (a.first < 0) a.first = b.first; else a.gap = max(a.gap, b.first - a.last);
    a.gap = max(a.gap, b.gap);
    a.last = b.last;
  }
  const bool stable = a.first == 0 && a.last == F - 1 && !(F > p.epsilon_stab_frames && a.gap >= p.epsilon_stab_frames);
  float* o = report + (size_t)c * PBHC_SCREEN_REPORT;
  o[0] = stable ? 1.0f : 0.0f;
  o[1] = dist[ib];
  o[2] = dist[(size_t)ib + F - 1];
  o[3] = a.maxd;
  o[4] = (float)((double)a.unstable / (double)F);
  o[5] = (float)a.gap;
  o[6] = 0.0f; o[7] = 0.0f;
}

static bool screen_counts_ok(int total, int num_clips, const int32_t* in_start) { return in_start && num_clips >= 1 && total >= num_clips; }

extern "C" int pbhc_motion_screen_frames(const PbhcSkeleton* skel, const float* pose_aa, const float* trans, int total, int num_clips,
                                         const int32_t* in_start, PbhcMotionScreen params, const float* body_mass, const float* body_com,
                                         float* ground, float* foot_pos, float* dist, void* stream) {
  const int rc = pbhc_check_skel(skel);                           // Bx <= PBHC_MAX_BODIES (one lane per body), the chain tables screen_fk walks
  if (rc) return rc;
  if (!pose_aa || !trans || !screen_counts_ok(total, num_clips, in_start) || (!foot_pos && !dist) || (dist && (!body_mass || !body_com || !ground))) {
    snprintf(g_pbhc_err, sizeof(g_pbhc_err),
             "pbhc_motion_screen_frames: bad argument (NULL pointer, neither foot_pos nor dist, dist without body_mass / body_com / ground, %d "
             "clips, %d frames)", num_clips, total);
    return PBHC_EINVAL;
  }
  if (foot_pos)
    for (int j = 0; j < 2; ++j)
      if (params.foot[j] < 0 || params.foot[j] >= skel->num_bodies_ext) {
        snprintf(g_pbhc_err, sizeof(g_pbhc_err), "pbhc_motion_screen_frames: bad argument (foot %d is body %d, the skeleton has %d)", j, params.foot[j],
                 skel->num_bodies_ext);
        return PBHC_EINVAL;
      }
  if (dist && !(isfinite(params.cop_w) && isfinite(params.cop_k))) {
    snprintf(g_pbhc_err, sizeof(g_pbhc_err), "pbhc_motion_screen_frames: bad argument (cop_w %g, cop_k %g)", params.cop_w, params.cop_k);
    return PBHC_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  if (dist)
    hipLaunchKernelGGL(k_motion_screen_ground, dim3((num_clips + SCR_FPW - 1) / SCR_FPW), dim3(SCR_THREADS), 0, st, *skel, pose_aa, trans, total,
                       num_clips, in_start, ground);
  hipLaunchKernelGGL(k_motion_screen_frames, dim3((total + SCR_FPW - 1) / SCR_FPW), dim3(SCR_THREADS), 0, st, *skel, pose_aa, trans, total, num_clips,
                     in_start, params, body_mass, body_com, ground, foot_pos, dist);
  if (hipGetLastError() != hipSuccess) return PBHC_EHIP;
  return PBHC_OK;
}

extern "C" int pbhc_motion_screen_clips(const float* foot_pos, const float* dist, int total, int num_clips, const int32_t* in_start,
                                        const int32_t* derive, PbhcMotionScreen params, float* mask, float* report, void* stream) {
  if (!screen_counts_ok(total, num_clips, in_start) || (foot_pos == nullptr) != (mask == nullptr) || (dist == nullptr) != (report == nullptr) ||
      (!mask && !report) || (mask && !derive)) {
    snprintf(g_pbhc_err, sizeof(g_pbhc_err),
             "pbhc_motion_screen_clips: bad argument (NULL pointer, foot_pos without mask, dist without report, mask without derive, %d clips, %d "
             "frames)", num_clips, total);
    return PBHC_EINVAL;
  }
  if ((mask && !(params.vel_threshold == params.vel_threshold && params.height_threshold == params.height_threshold)) ||
      (report && (!(params.epsilon_stab == params.epsilon_stab) || params.epsilon_stab_frames < 1))) {
    snprintf(g_pbhc_err, sizeof(g_pbhc_err),
             "pbhc_motion_screen_clips: bad argument (vel_threshold %g, height_threshold %g, epsilon_stab %g, epsilon_stab_frames %d)",
             params.vel_threshold, params.height_threshold, params.epsilon_stab, params.epsilon_stab_frames);
    return PBHC_EINVAL;
  }
  hipLaunchKernelGGL(k_motion_screen_clips, dim3(num_clips), dim3(SCR_THREADS), 0, (hipStream_t)stream, foot_pos, dist, total, num_clips, in_start,
                     derive, params, mask, report);
  if (hipGetLastError() != hipSuccess) return PBHC_EHIP;
  return PBHC_OK;
}
