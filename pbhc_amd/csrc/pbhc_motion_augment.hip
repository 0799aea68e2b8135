// pbhc_motion_augment.hip — mirrored and time-scaled copies of every clip of a library, at ingestion, in one launch (robot.motion.augmentation).
//
//   k_motion_augment  one wave per OUTPUT frame (AUG_FPW frames per workgroup), lanes over the 3 Bx floats of the frame's pose_aa rows.
//                     Output clip c is variant v = c % V of source clip c / V; v = speed index * (mirror ? 2 : 1) + mirrored, speed index 0
//                     is speed 1.0.  Variant 0 is the source, copied bit for bit.
//
// Speed s (the clip keeps its fps): a clip of F frames gives F' = floor((F - 1) / s) + 1 frames (aug_frames, the same arithmetic on the host
// and here); output frame k samples the source at x = k s, formed in double: i0 = min(floor(x), F - 1), i1 = min(i0 + 1, F - 1), t = x - i0.
//   t == 0 : frame i0, bit for bit
//   else   : translation and every row but the root's a + t (b - a) in double, rounded to float once (the build runs with -ffp-contract=off:
//            no fused multiply-add); the extended bodies' rows are zero in a clip and stay zero under that; the root row is rotation vector
//            -> quaternion -> short-way slerp -> rotation vector in double by lane 0 of the frame's wave, rounded once, as k_motion_extend
//            forms its root row; the contact mask is that of the nearer source frame, i0 for t < 0.5, else i1
// Mirror (a reflection across the x-z plane, applied after the resampling): translation (x, -y, z); pose_aa row b = (-a_x, a_y, -a_z) of row
// perm[b], the root included (perm[0] == 0); the two contact columns swapped.  perm exchanges the left and right bodies; that the skeleton is
// its own mirror image under it is checked on the host (pbhc_amd/motion_augment.py).
// No atomics, no LDS; every store is a vector store of one dword per lane, consecutive lanes to consecutive addresses.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>

#include "../../include/pbhc_hip.h"
#include "pbhc_dquat.h"
#include "pbhc_math.h"

using namespace pbhc;

extern thread_local char g_pbhc_err[512];
extern "C" int pbhc_check_skel(const PbhcSkeleton* sk);            // pbhc_kernels.hip

#define AUG_THREADS 256
#define AUG_FPW (AUG_THREADS / 64)                                 // frames per workgroup: one wave each
#define AUG_SPEED_MIN 0.25
#define AUG_SPEED_MAX 4.0

// frames of a clip of F >= 1 frames played at speed s: the last sample (F' - 1) s must not pass the last source frame F - 1
__host__ __device__ __forceinline__ int aug_frames(int F, double s) {
  int Fo = (int)floor((double)(F - 1) / s) + 1;
  if ((double)(Fo - 1) * s > (double)(F - 1)) Fo -= 1;
  return Fo;
}

__global__ __launch_bounds__(AUG_THREADS) void k_motion_augment(int Bx, const float* __restrict__ pose_aa, const float* __restrict__ trans,
                                                                const float* __restrict__ contact, int total_in, int M,
                                                                const int32_t* __restrict__ in_start, const int32_t* __restrict__ out_start,
                                                                int total_out, PbhcMotionAugment p, const int32_t* __restrict__ perm,
                                                                float* __restrict__ out_pose, float* __restrict__ out_trans,
                                                                float* __restrict__ out_contact) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * AUG_FPW + (threadIdx.x >> 6);        // output frame of this wave
  if (g >= total_out) return;
  const int V = p.num_variants;
  int lo = 0, hi = M * V;                                         // the output clip of frame g: out_start[lo] <= g < out_start[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (out_start[mid] <= g) lo = mid; else hi = mid;
  }
  const int src = lo / V, v = lo - src * V;
  const bool mir = p.mirror != 0 && (v & 1) != 0;
  const int si = p.mirror != 0 ? v >> 1 : v;
  const double s = si == 0 ? 1.0 : p.speeds[si - 1];
  const int ib = in_start[src], F = in_start[src + 1] - ib, ob = out_start[lo], k = g - ob;
  // start arrays that do not describe "variant v of clip src has aug_frames(F, s) frames" index nothing: the frame is left as it was
  if (ib < 0 || F < 1 || F > total_in - ib || k < 0 || out_start[lo + 1] - ob != aug_frames(F, s) || k >= out_start[lo + 1] - ob) return;
  const double x = (double)k * s;
  const int i0 = min((int)floor(x), F - 1), i1 = min(i0 + 1, F - 1);
  const double t = x - (double)i0;
  const bool copy = t == 0.0;
  const int row = 3 * Bx;
  const float* pa = pose_aa + ((size_t)ib + i0) * row;
  const float* pb = pose_aa + ((size_t)ib + i1) * row;
  float root[3] = {0.0f, 0.0f, 0.0f};
  if (!copy) {
    if (lane == 0) {
      const d4 r = dq_slerp(dq_from_rotvec((double)pa[0], (double)pa[1], (double)pa[2]), dq_from_rotvec((double)pb[0], (double)pb[1], (double)pb[2]), t);
      double rv[3];
      rotvec_from_quat<double>(r.x, r.y, r.z, r.w, rv);
      root[0] = (float)rv[0]; root[1] = (float)rv[1]; root[2] = (float)rv[2];
    }
    root[0] = __shfl(root[0], 0, 64); root[1] = __shfl(root[1], 0, 64); root[2] = __shfl(root[2], 0, 64);
  }
  float* op = out_pose + (size_t)g * row;
  for (int e = lane; e < row; e += 64) {
    const int b = e / 3, c = e - 3 * b;
    const int sb = mir ? perm[b] : b;                             // the body whose row lands in row b
    if ((unsigned)sb >= (unsigned)Bx || (b == 0) != (sb == 0)) continue;   // not a permutation that holds the root: nothing is read or written
    const int se = 3 * sb + c;
    float val;
    if (copy) val = pa[se];
    else if (b == 0) val = c == 0 ? root[0] : (c == 1 ? root[1] : root[2]);
    else val = (float)((double)pa[se] + t * ((double)pb[se] - (double)pa[se]));
    op[e] = mir && c != 1 ? -val : val;
  }
  if (lane < 3) {
    const float a = trans[((size_t)ib + i0) * 3 + lane];
    const float val = copy ? a : (float)((double)a + t * ((double)trans[((size_t)ib + i1) * 3 + lane] - (double)a));
    out_trans[(size_t)g * 3 + lane] = mir && lane == 1 ? -val : val;
  }
  if (lane < 2 && out_contact) out_contact[(size_t)g * 2 + lane] = contact[((size_t)ib + (t < 0.5 ? i0 : i1)) * 2 + (mir ? 1 - lane : lane)];
}

extern "C" int pbhc_motion_augment_batch(const PbhcSkeleton* skel, const float* pose_aa, const float* trans, const float* contact, int total_in,
                                         int num_clips, const int32_t* in_start, const int32_t* out_start, int total_out, PbhcMotionAugment params,
                                         const int32_t* perm, float* out_pose_aa, float* out_trans, float* out_contact, void* stream) {
  const int rc = pbhc_check_skel(skel);                           // Bx <= PBHC_MAX_BODIES, D == B - 1 <= PBHC_MAX_DOF
  if (rc) return rc;
  const int S = 1 + params.num_speeds, V = params.num_variants;
  if (!pose_aa || !trans || !in_start || !out_start || !out_pose_aa || !out_trans || (params.mirror && !perm) ||
      (contact == nullptr) != (out_contact == nullptr) || num_clips < 1 || total_in < num_clips || V < 1 || params.num_speeds < 0 ||
      params.num_speeds > PBHC_MAX_SPEEDS || V != S * (params.mirror ? 2 : 1) || (long long)num_clips * V > 0x7fffffffLL) {
    snprintf(g_pbhc_err, sizeof(g_pbhc_err),
             "pbhc_motion_augment_batch: bad argument (NULL pointer, mirror without perm, contact in without contact out, %d clips, %d frames in, "
             "%d variants for %d speeds besides 1.0 (at most %d)%s)",
             num_clips, total_in, V, params.num_speeds, PBHC_MAX_SPEEDS, params.mirror ? " and the mirror" : "");
    return PBHC_EINVAL;
  }
  // The per-clip frame counts live on the device.  What the scalars imply: with Y = total_in - num_clips, speed s turns the total_in frames
  // of num_clips clips into more than Y / s and at most Y / s + num_clips frames, so into floor(Y / s) + 1 ... floor(Y / s) + num_clips
  // (a relative 1e-12 of room for a quotient that rounds onto an integer); speed 1.0 into exactly total_in.
  long long lo = total_in, hi = total_in;
  for (int i = 0; i < params.num_speeds; ++i) {
    const double s = params.speeds[i];
    if (!(s >= AUG_SPEED_MIN && s <= AUG_SPEED_MAX)) {
      snprintf(g_pbhc_err, sizeof(g_pbhc_err), "pbhc_motion_augment_batch: bad argument (speed %d is %g, outside [%g, %g])", i, s, AUG_SPEED_MIN,
               AUG_SPEED_MAX);
      return PBHC_EINVAL;
    }
    const double y = (double)(total_in - num_clips) / s;
    lo += (long long)floor(y * (1.0 - 1e-12)) + 1;
    hi += (long long)floor(y * (1.0 + 1e-12)) + num_clips;
  }
  const int mult = params.mirror ? 2 : 1;
  if (total_out < 1 || total_out % mult != 0 || total_out / mult < lo || total_out / mult > hi) {
    snprintf(g_pbhc_err, sizeof(g_pbhc_err),
             "pbhc_motion_augment_batch: bad argument (%d frames out: the %d variants of %d frames in %d clips hold between %lld and %lld)", total_out,
             V, total_in, num_clips, lo * mult, hi * mult);
    return PBHC_EINVAL;
  }
  hipLaunchKernelGGL(k_motion_augment, dim3((total_out + AUG_FPW - 1) / AUG_FPW), dim3(AUG_THREADS), 0, (hipStream_t)stream, skel->num_bodies_ext,
                     pose_aa, trans, contact, total_in, num_clips, in_start, out_start, total_out, params, perm, out_pose_aa, out_trans, out_contact);
  if (hipGetLastError() != hipSuccess) return PBHC_EHIP;
  return PBHC_OK;
}
