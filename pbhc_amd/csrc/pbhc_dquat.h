// pbhc_dquat.h — double-precision quaternion helpers (x, y, z, w) of the ingestion kernels that form a root rotation once per frame and
// round it to float once: k_motion_extend (pbhc_motion_extend.hip) and k_motion_augment (pbhc_motion_augment.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace pbhc {

struct d4 { double x, y, z, w; };

__device__ __forceinline__ d4 dq_mul(d4 a, d4 b) {
  return d4{a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x,
            a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
}

// scipy's Rotation.from_rotvec: (v sin(a/2) / a, cos(a/2)), the series 1/2 - a^2/48 + a^4/3840 for a <= 1e-3
__device__ __forceinline__ d4 dq_from_rotvec(double x, double y, double z) {
  const double a = sqrt(x * x + y * y + z * z);
  const double s = a <= 1e-3 ? 0.5 - a * a / 48.0 + a * a * a * a / 3840.0 : sin(0.5 * a) / a;
  return d4{s * x, s * y, s * z, cos(0.5 * a)};
}

// scipy's Slerp([0, 1], [A, B])(t): A * exp(t * log(A^-1 B)), the relative rotation taken the short way round
__device__ __forceinline__ d4 dq_slerp(d4 A, d4 B, double t) {
  d4 rel = dq_mul(d4{-A.x, -A.y, -A.z, A.w}, B);
  if (rel.w < 0.0) rel = d4{-rel.x, -rel.y, -rel.z, -rel.w};
  const double nv = sqrt(rel.x * rel.x + rel.y * rel.y + rel.z * rel.z);
  if (!(nv > 0.0)) return A;
  const double half = t * atan2(nv, rel.w), s = sin(half) / nv;
  return dq_mul(A, d4{s * rel.x, s * rel.y, s * rel.z, cos(half)});
}

}  // namespace pbhc
