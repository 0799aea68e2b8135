// pbhc_clip_track.hip — per-clip tracking error of the library sweep (env.library_sweep), accumulated on the device.
//
//   k_clip_track   one launch per control step of a sweep, after the fused step and after k_clip_stats on the same stream: every active env
//                  that did NOT reset in this step adds one scored frame to row slot_clip[env] of `track_window [M,4]` int64 =
//                  (frames, sum of e_g * 2^20, sum of e_l * 2^20, sum of e_j * 2^20), with the per-frame errors of
//                  pbhc_amd/eval/metrics.py eval_accuracy over the B real bodies and the D joints:
//                    e_g = mean_b |p_b - r_b|                      (E_gmpbpe, metres)
//                    e_l = mean_b |(p_b - p_0) - (r_b - r_0)|      (E_mpbpe, metres)
//                    e_j = |q - q_ref|_2                           (E_mpjpe, radians)
//                  p: the simulator FK of the state the step left (fk_walk, as k_sim_fk calls it), r / q_ref: the reference at ref_time[env]
//                  (motion_lookup with the step's own table entry, offset by the env's origin).
//
// Every column is an integer ON PURPOSE, as in pbhc_clip_stats.hip: integer atomic sums do not depend on the order in which the adds arrive,
// so the table is bit-reproducible.  An error goes in as llrintf(e * 2^20): at most 2^-21 (0.5 um / 0.5 urad) of rounding per frame, and an
// int64 holds 2^43 metres of it.
//
// There is no combine stage (k_clip_stats has one for N adds onto one row): in a sweep a clip belongs to at most one env per wave of clips,
// so all adds of a launch hit distinct rows.  Called outside a sweep with a clip shared by several envs the sums are still exact, only
// serialised per row.
//
// Which frames count.  An env that reset in this step is not scored: its post-step buffers already hold the NEW episode's state, so the
// terminal frame of an episode has no state left to score (k_clip_stats has counted the episode).  With `retire` given, such an env's
// retire[env] becomes -1; the sweep passes its slot -> clip array as both slot_clip and retire, so a clip is scored on its first episode
// only.  A frame whose three errors are not all finite is skipped entirely (not counted).  A slot_clip outside [0, M) — an idle or retired
// env — is skipped and never used as an index, and so is a table entry outside the motion table.
//
// Raw pointers only: the step kernel, its config-specialised builds, PbhcEnvConfig and PbhcStepIO do not know this kernel exists.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <math.h>

#include "../../include/pbhc_hip.h"
#include "pbhc_math.h"

using namespace pbhc;

extern thread_local char g_pbhc_err[512];
extern "C" int pbhc_check_skel(const PbhcSkeleton* sk);            // pbhc_kernels.hip

#undef PBHC_STAMPS                                          // (the phase stamps of the diagnostic build belong to the step kernel's unit)
#include "pbhc_env_step.h"                                  // PBHC_G / PBHC_EPB, stage_skeleton, fk_walk, motion_lookup, group_sum

#define TRACK_SCALE 1048576.0f                              // 2^20

// floats of LDS per env: root 16, q / qd 64, the FK's pos3 quat4 vel3 ang3 + relative quaternions 17 per body (as k_sim_fk), then the
// reference: dof / dof vel 64, contact 8, pos3 quat4 vel3 ang3 13 per body (as k_motion_state)
#define TRACK_FK_WORDS (16 + 64 + PBHC_MAX_BODIES * 17)
#define TRACK_ENV_WORDS (TRACK_FK_WORDS + 64 + 8 + PBHC_MAX_BODIES * 13)

// One env per PBHC_G lanes, PBHC_EPB envs per workgroup.  fk_walk's barriers span the workgroup, so no wave leaves on its own: a
// workgroup with no frame to score returns as a whole before it stages the skeleton or loads any state, and inside a scoring workgroup a
// wave with nothing to score loads no state and does no arithmetic (`score` false on all its lanes), it only keeps the barriers company.
__global__ __launch_bounds__(PBHC_G* PBHC_EPB) void k_clip_track(PbhcSkeleton sk, PbhcMotionTable tbl, const float* __restrict__ root_states,
                                                                const float* __restrict__ dof_state, const float* __restrict__ ref_time,
                                                                const float* __restrict__ env_origins, const int64_t* __restrict__ motion_ids,
                                                                const int64_t* __restrict__ reset_buf, const int64_t* slot_clip, int64_t* retire,
                                                                int N, int M, unsigned long long* __restrict__ window) {
  __shared__ float sm[PBHC_EPB][TRACK_ENV_WORDS];
  __shared__ float skc[SKC_WORDS];
  const int lane = threadIdx.x & (PBHC_G - 1), le = threadIdx.x / PBHC_G, env = blockIdx.x * PBHC_EPB + le;
  const int D = sk.num_dof, B = sk.num_bodies, Bx = sk.num_bodies_ext;

  bool score = false;
  int clip = 0, mid = 0;
  if (env < N) {
    const int64_t c = slot_clip[env];                       // (every lane of the env: the retire store below comes after this load has returned)
    if (c >= 0 && c < (int64_t)M) {
      if (reset_buf[env] != 0) {
        if (retire != nullptr && lane == 0) retire[env] = -1;
      } else {
        const int64_t m = motion_ids[env];
        if (m >= 0 && m < (int64_t)tbl.num_motions) { score = true; clip = (int)c; mid = (int)m; }
      }
    }
  }
  if (!__syncthreads_or(score ? 1 : 0)) return;             // workgroup-uniform

  float* root = sm[le];
  float *q = root + 16, *qd = q + 32, *bp = qd + 32, *bq = bp + 3 * PBHC_MAX_BODIES, *bv = bq + 4 * PBHC_MAX_BODIES, *bw = bv + 3 * PBHC_MAX_BODIES;
  float* relq = bw + 3 * PBHC_MAX_BODIES;
  float* rdof = root + TRACK_FK_WORDS;
  float *rdofv = rdof + 32, *rc = rdofv + 32, *rp = rc + 8, *rq = rp + 3 * PBHC_MAX_BODIES, *rv = rq + 4 * PBHC_MAX_BODIES, *rw = rv + 3 * PBHC_MAX_BODIES;
  stage_skeleton(sk, skc);

  if (score) {
    if (lane < 13) root[lane] = root_states[(size_t)env * 13 + lane];
    for (int d = lane; d < D; d += PBHC_G) {
      const float2 s = *(const float2*)(dof_state + ((size_t)env * D + d) * 2);       // [N,D,2]: (position, velocity)
      q[d] = s.x;
      qd[d] = s.y;
    }
    motion_lookup(tbl, D, Bx, lane, mid, ref_time[env], ld3(env_origins + (size_t)env * 3), true, rdof, rdofv, rc, rp, rq, rv, rw);
  }
  __syncthreads();
  fk_walk(skc, B, B, lane, score, root, q, qd, relq, bp, bq, bv, bw);       // (ends on a barrier: bp and rp of every lane are visible below)

  // per-lane partial sums; the differences are formed in double so that e_l keeps its relative accuracy when it is small next to the
  // distances it is a difference of (a policy that tracks well), then rounded once to float32
  float sg = 0.0f, sl = 0.0f, sj = 0.0f;
  if (score) {
    for (int b = lane; b < B; b += PBHC_G) {
      const double gx = (double)bp[3 * b] - (double)rp[3 * b], gy = (double)bp[3 * b + 1] - (double)rp[3 * b + 1],
                   gz = (double)bp[3 * b + 2] - (double)rp[3 * b + 2];
      const double lx = ((double)bp[3 * b] - (double)bp[0]) - ((double)rp[3 * b] - (double)rp[0]);
      const double ly = ((double)bp[3 * b + 1] - (double)bp[1]) - ((double)rp[3 * b + 1] - (double)rp[1]);
      const double lz = ((double)bp[3 * b + 2] - (double)bp[2]) - ((double)rp[3 * b + 2] - (double)rp[2]);
      sg += norm3(mk3((float)gx, (float)gy, (float)gz));
      sl += norm3(mk3((float)lx, (float)ly, (float)lz));
    }
    for (int d = lane; d < D; d += PBHC_G) {
      const float dj = q[d] - rdof[d];
      sj += dj * dj;
    }
  }
  sg = group_sum(sg);                                       // (every lane of the wave: an idle env's lanes add zeros among themselves)
  sl = group_sum(sl);
  sj = group_sum(sj);
  if (score && lane == 0) {
    const float e_g = sg / (float)B, e_l = sl / (float)B, e_j = sqrtf(sj);
    if (isfinite(e_g) && isfinite(e_l) && isfinite(e_j)) {
      unsigned long long* row = window + 4 * (size_t)clip;
      atomicAdd(row + 0, 1ull);
      atomicAdd(row + 1, (unsigned long long)llrintf(e_g * TRACK_SCALE));
      atomicAdd(row + 2, (unsigned long long)llrintf(e_l * TRACK_SCALE));
      atomicAdd(row + 3, (unsigned long long)llrintf(e_j * TRACK_SCALE));
    }
  }
}

extern "C" int pbhc_clip_track(const PbhcSkeleton* skel, const PbhcMotionTable* tbl, const float* root_states, const float* dof_state,
                               const float* ref_time, const float* env_origins, const int64_t* motion_ids, const int64_t* reset_buf,
                               const int64_t* slot_clip, int64_t* retire, int N, int M, int64_t* track_window, void* stream) {
  if (!skel || !tbl || !tbl->frames || !tbl->length_starts || !tbl->num_frames || !tbl->motion_dt || !tbl->motion_len || !root_states ||
      !dof_state || !ref_time || !env_origins || !motion_ids || !reset_buf || !slot_clip || !track_window || N < 1 || M < 1) {
    snprintf(g_pbhc_err, sizeof(g_pbhc_err), "pbhc_clip_track: bad argument (NULL pointer, N %d, M %d)", N, M);
    return PBHC_EINVAL;
  }
  const int rc = pbhc_check_skel(skel);                     // the kernel maxima and the chain tables fk_walk indexes LDS with
  if (rc) return rc;
  if (tbl->num_motions < 1 || tbl->row != 2 * skel->num_dof + 2 + 13 * skel->num_bodies_ext) {
    snprintf(g_pbhc_err, sizeof(g_pbhc_err), "pbhc_clip_track: bad argument (motion table of %d entries, row %d for %d dofs and %d bodies)",
             tbl->num_motions, tbl->row, skel->num_dof, skel->num_bodies_ext);
    return PBHC_EINVAL;
  }
  hipLaunchKernelGGL(k_clip_track, dim3((N + PBHC_EPB - 1) / PBHC_EPB), dim3(PBHC_G * PBHC_EPB), 0, (hipStream_t)stream, *skel, *tbl, root_states,
                     dof_state, ref_time, env_origins, motion_ids, reset_buf, slot_clip, retire, N, M, (unsigned long long*)track_window);
  if (hipGetLastError() != hipSuccess) return PBHC_EHIP;
  return PBHC_OK;
}
