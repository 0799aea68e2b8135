// pbhc_motion_extend.hip — lead-in / lead-out frames between a default pose and every clip of a library, at ingestion, in one launch.
//
//   k_motion_extend   one wave per OUTPUT frame (EXT_FPW frames per workgroup), lanes over the 3 Bx floats of the frame's pose_aa rows.
//                     A frame inside the original clip is copied bit for bit; the start_frames + end_frames synthetic frames of a clip are
//                     computed from the clip's first / last frame and the default pose.
//
// What the synthetic frames hold (reference: robot_motion_process/motion_interpolation_pkl.py, interpolate_motion / lower_dof_interpolation
// and the contact-mask block of its __main__; restated in DESIGN §8).  With n = start_frames, m = end_frames, (p, q, d) the clip's first and
// (p', q', d') its last root translation / root rotation / joint values, (z0, q0, d0) the default pose:
//   lead-in  i < n : z = linspace(z0, p.z, n)[i], x, y held;  joints linspace(d0, d, n + 1, endpoint=False)[i + 1];
//                    rotation slerp(A, B, linspace(0, 1, n)[i]) with B = R_ZYX(yaw q, pitch q, roll q), A = R_ZYX(yaw q, pitch q0, roll q0)
//   lead-out i < m : z = linspace(p'.z, z0, m)[i];            joints linspace(d', d0, m + 1)[i + 1] (the last frame IS d0);
//                    rotation slerp(A', B', linspace(1, 0, m)[i])
//   knee_modify    : dofs 0..5 move in the first h = N / 2 synthetic frames and then hold, dofs 6..11 hold and move in the last h, both by
//                    linspace(s, e, h + 1, endpoint=False)[r + 1]; dofs 3 and 9 go to 1.0 rad in k = h / 2 frames and come back in k + 1
//                    (both ends inclusive; 2 k + 1 == h is checked on the host).  Contact: (1,1) at the ends (and in the middle of an odd
//                    count), (0,1) in the first half, (1,0) in the second; without knee_modify the fill value.
// The joint value of a clip frame is dot(pose_aa[j + 1], dof_axis[j]); a synthetic joint row is dof_axis[j] * value, the extended bodies'
// rows are zero.  The root row is formed in double by lane 0 of the frame's wave — rotation vector -> quaternion -> ZYX angles -> slerp ->
// rotation vector — and rounded to float once.  No atomics, no LDS; every store is a vector store of one dword per lane, consecutive lanes
// to consecutive addresses.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "../../include/pbhc_hip.h"
#include "pbhc_dquat.h"
#include "pbhc_math.h"

using namespace pbhc;

extern thread_local char g_pbhc_err[512];
extern "C" int pbhc_check_skel(const PbhcSkeleton* sk);            // pbhc_kernels.hip

#define EXT_THREADS 256
#define EXT_FPW (EXT_THREADS / 64)                                 // frames per workgroup: one wave each

struct ExtAxes { float a[PBHC_MAX_DOF][3]; };                     // the one table of the skeleton this kernel reads (384 of its 3.6 KB)

// np.linspace(a, b, num, endpoint=False)[i] and np.linspace(a, b, num)[i] as numpy forms them: a + i * step, and the last sample of the
// closed form is b itself (num == 1: a).
__device__ __forceinline__ double lin_open(double a, double b, int i, int num) { return a + (double)i * ((b - a) / (double)num); }
__device__ __forceinline__ double lin_closed(double a, double b, int i, int num) {
  if (num <= 1) return a;
  if (i == num - 1) return b;
  return a + (double)i * ((b - a) / (double)(num - 1));
}

// joint j of synthetic frame i of N, interpolated from s to e (lead-in: default -> clip, open at both ends; lead-out: clip -> default, closed at e)
__device__ __forceinline__ double ext_joint(double s, double e, int j, int i, int N, bool lead_in, bool knee) {
  if (knee && j < 12) {
    const int h = N / 2, k = h / 2, jj = j < 6 ? j : j - 6;
    const int r = j < 6 ? min(i, h - 1) : max(i - (N - h), 0);
    if (jj == 3) return r < k ? lin_closed(s, 1.0, r, k) : lin_closed(1.0, e, r - k, k + 1);
    return lin_open(s, e, r + 1, h + 1);
  }
  return lead_in ? lin_open(s, e, i + 1, N + 1) : lin_closed(s, e, i + 1, N + 1);
}

// intrinsic Z-Y'-X'' angles of a unit quaternion: R = Rz(yaw) Ry(pitch) Rx(roll)
__device__ __forceinline__ void dq_to_zyx(d4 q, double& yaw, double& pitch, double& roll) {
  yaw = atan2(2.0 * (q.w * q.z + q.x * q.y), 1.0 - 2.0 * (q.y * q.y + q.z * q.z));
  pitch = asin(fmin(fmax(2.0 * (q.w * q.y - q.z * q.x), -1.0), 1.0));
  roll = atan2(2.0 * (q.w * q.x + q.y * q.z), 1.0 - 2.0 * (q.x * q.x + q.y * q.y));
}

__device__ __forceinline__ d4 dq_from_zyx(double yaw, double pitch, double roll) {
  const double cy = cos(0.5 * yaw), sy = sin(0.5 * yaw), cp = cos(0.5 * pitch), sp = sin(0.5 * pitch), cr = cos(0.5 * roll), sr = sin(0.5 * roll);
  return d4{sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy};
}

__global__ __launch_bounds__(EXT_THREADS) void k_motion_extend(ExtAxes ax, int Bx, int D, const float* __restrict__ pose_aa,
                                                               const float* __restrict__ trans, const float* __restrict__ contact, int total_in,
                                                               int M, const int32_t* __restrict__ in_start, const int32_t* __restrict__ out_start,
                                                               int total_out, PbhcMotionExtend p, float* __restrict__ out_pose,
                                                               float* __restrict__ out_trans, float* __restrict__ out_contact) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * EXT_FPW + (threadIdx.x >> 6);        // output frame of this wave
  if (g >= total_out) return;
  int lo = 0, hi = M;                                             // the clip of frame g: out_start[lo] <= g < out_start[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (out_start[mid] <= g) lo = mid; else hi = mid;
  }
  const int n = p.start_frames, m = p.end_frames;
  const int ib = in_start[lo], F = in_start[lo + 1] - ib, ob = out_start[lo], k = g - ob;
  // start arrays that do not describe "every clip grows by n + m frames" index nothing: the frame is left as it was
  if (ib < 0 || F < 1 || F > total_in - ib || out_start[lo + 1] - ob != F + n + m || k < 0 || k >= F + n + m) return;
  const int row = 3 * Bx;
  float* op = out_pose + (size_t)g * row;
  if (k >= n && k < n + F) {                                      // a frame of the clip itself
    const size_t src = (size_t)ib + (k - n);
    for (int e = lane; e < row; e += 64) op[e] = pose_aa[src * row + e];
    if (lane < 3) out_trans[(size_t)g * 3 + lane] = trans[src * 3 + lane];
    if (lane < 2 && out_contact) out_contact[(size_t)g * 2 + lane] = contact[src * 2 + lane];
    return;
  }
  const bool lead_in = k < n;
  const int i = lead_in ? k : k - n - F, N = lead_in ? n : m;
  const size_t edge = lead_in ? (size_t)ib : (size_t)ib + F - 1;  // the clip frame this end starts from / arrives at
  const float* ep = pose_aa + edge * row;
  float root[3] = {0.0f, 0.0f, 0.0f}, z = 0.0f;
  if (lane == 0) {
    const d4 q = dq_from_rotvec((double)ep[0], (double)ep[1], (double)ep[2]);
    const double qn = sqrt((double)p.default_quat_xyzw[0] * p.default_quat_xyzw[0] + (double)p.default_quat_xyzw[1] * p.default_quat_xyzw[1] +
                           (double)p.default_quat_xyzw[2] * p.default_quat_xyzw[2] + (double)p.default_quat_xyzw[3] * p.default_quat_xyzw[3]);
    const d4 q0 = d4{p.default_quat_xyzw[0] / qn, p.default_quat_xyzw[1] / qn, p.default_quat_xyzw[2] / qn, p.default_quat_xyzw[3] / qn};
    double yaw, pitch, roll, yaw0, pitch0, roll0;
    dq_to_zyx(q, yaw, pitch, roll);
    dq_to_zyx(q0, yaw0, pitch0, roll0);                           // yaw0 is not used: the clip's heading is held
    const double t = lead_in ? lin_closed(0.0, 1.0, i, N) : lin_closed(1.0, 0.0, i, N);
    const d4 r = dq_slerp(dq_from_zyx(yaw, pitch0, roll0), dq_from_zyx(yaw, pitch, roll), t);
    double rv[3];
    rotvec_from_quat<double>(r.x, r.y, r.z, r.w, rv);
    root[0] = (float)rv[0]; root[1] = (float)rv[1]; root[2] = (float)rv[2];
    const double ze = (double)trans[edge * 3 + 2], z0 = (double)p.default_height;
    z = (float)(lead_in ? lin_closed(z0, ze, i, N) : lin_closed(ze, z0, i, N));
  }
  root[0] = __shfl(root[0], 0, 64); root[1] = __shfl(root[1], 0, 64); root[2] = __shfl(root[2], 0, 64);
  z = __shfl(z, 0, 64);
  for (int e = lane; e < row; e += 64) {
    const int b = e / 3, c = e - 3 * b;
    float v = 0.0f;                                               // the extended bodies' rows
    if (b == 0) {
      v = c == 0 ? root[0] : (c == 1 ? root[1] : root[2]);
    } else if (b <= D) {
      const int j = b - 1;
      const float* pj = ep + 3 * b;
      const double dc = (double)(pj[0] * ax.a[j][0] + pj[1] * ax.a[j][1] + pj[2] * ax.a[j][2]), d0 = (double)p.default_dof[j];
      v = ax.a[j][c] * (float)ext_joint(lead_in ? d0 : dc, lead_in ? dc : d0, j, i, N, lead_in, p.knee_modify != 0);
    }
    op[e] = v;
  }
  if (lane < 3) out_trans[(size_t)g * 3 + lane] = lane == 2 ? z : trans[edge * 3 + lane];
  if (lane < 2 && out_contact) {
    float cm = p.contact_fill;
    if (p.knee_modify) {
      const int h = N / 2;
      if (i == 0 || i == N - 1 || ((N & 1) && i == h)) cm = 1.0f;
      else cm = (i < h) == (lane == 1) ? 1.0f : 0.0f;             // first half (0, 1), second half (1, 0)
    }
    out_contact[(size_t)g * 2 + lane] = cm;
  }
}

// the frame counts lower_dof_interpolation accepts: its two knee ramps of k and k + 1 samples must fill the h = N / 2 moving frames
static bool knee_count_ok(int N) { return N == 0 || 2 * ((N / 2) / 2) + 1 == N / 2; }

extern "C" int pbhc_motion_extend_batch(const PbhcSkeleton* skel, const float* pose_aa, const float* trans, const float* contact, int total_in,
                                        int num_clips, const int32_t* in_start, const int32_t* out_start, int total_out, PbhcMotionExtend params,
                                        float* out_pose_aa, float* out_trans, float* out_contact, void* stream) {
  const int rc = pbhc_check_skel(skel);                           // Bx <= PBHC_MAX_BODIES, D == B - 1 <= PBHC_MAX_DOF
  if (rc) return rc;
  const long long grown = (long long)total_in + (long long)num_clips * ((long long)params.start_frames + params.end_frames);
  if (!pose_aa || !trans || !in_start || !out_start || !out_pose_aa || !out_trans || !params.default_dof || (contact == nullptr) != (out_contact == nullptr) ||
      num_clips < 1 || total_in < num_clips || params.start_frames < 0 || params.end_frames < 0 || grown != (long long)total_out) {
    snprintf(g_pbhc_err, sizeof(g_pbhc_err),
             "pbhc_motion_extend_batch: bad argument (NULL pointer, contact in without contact out, %d clips, %d frames in, %d out, %d + %d added per clip)",
             num_clips, total_in, total_out, params.start_frames, params.end_frames);
    return PBHC_EINVAL;
  }
  if (params.knee_modify && (skel->num_dof < 12 || !knee_count_ok(params.start_frames) || !knee_count_ok(params.end_frames))) {
    snprintf(g_pbhc_err, sizeof(g_pbhc_err),
             "pbhc_motion_extend_batch: bad argument (knee_modify needs 12 leg dofs, has %d, and frame counts N with 2 (N / 2 / 2) + 1 == N / 2, got %d and %d)",
             skel->num_dof, params.start_frames, params.end_frames);
    return PBHC_EINVAL;
  }
  const float* q0 = params.default_quat_xyzw;
  const float q0n = q0[0] * q0[0] + q0[1] * q0[1] + q0[2] * q0[2] + q0[3] * q0[3];
  if (!(q0n > 1e-12f && q0n < 1e12f) || !(params.default_height == params.default_height)) {
    snprintf(g_pbhc_err, sizeof(g_pbhc_err), "pbhc_motion_extend_batch: bad argument (default root quaternion of squared norm %g, height %g)", q0n,
             params.default_height);
    return PBHC_EINVAL;
  }
  ExtAxes ax;
  for (int j = 0; j < PBHC_MAX_DOF; ++j)
    for (int c = 0; c < 3; ++c) ax.a[j][c] = j < skel->num_dof ? skel->dof_axis[j][c] : 0.0f;
  hipLaunchKernelGGL(k_motion_extend, dim3((total_out + EXT_FPW - 1) / EXT_FPW), dim3(EXT_THREADS), 0, (hipStream_t)stream, ax, skel->num_bodies_ext,
                     skel->num_dof, pose_aa, trans, contact, total_in, num_clips, in_start, out_start, total_out, params, out_pose_aa, out_trans,
                     out_contact);
  if (hipGetLastError() != hipSuccess) return PBHC_EHIP;
  return PBHC_OK;
}
