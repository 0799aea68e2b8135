// pbhc_kernels.hip — hand-written gfx950 (CDNA4) kernels + the C ABI of include/pbhc_hip.h.
//
// Hot path: one fused launch per control step (k_env_step) + a 1-block finalize.  Mapping:
// 32 lanes (half a wave64) own one env, lane <-> body / dof / obs element; PBHC_EPB envs per
// 128-thread workgroup, so 4096 envs = 1024 workgroups = 4 per CU.  Per-env rows are read and
// written as contiguous rows (reference [N,C] layouts, which is also what the MLP GEMMs consume);
// the joint chain, the reference frames and the feature row are staged in LDS.
// This is HBM-bound float work: no MFMA on purpose.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <new>
#include <dlfcn.h>

#include "../../include/pbhc_hip.h"
#include "pbhc_math.h"

using namespace pbhc;



thread_local char g_pbhc_err[512] = "";
#define g_err g_pbhc_err

#define HIP_CHECK(x)                                                                          \
  do {                                                                                        \
    hipError_t e_ = (x);                                                                      \
    if (e_ != hipSuccess) {                                                                   \
      snprintf(g_err, sizeof(g_err), "%s:%d %s -> %s", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
      return PBHC_EHIP;                                                                       \
    }                                                                                         \
  } while (0)
#define ARG_CHECK(c)                                                                    \
  do {                                                                                  \
    if (!(c)) {                                                                         \
      snprintf(g_err, sizeof(g_err), "%s:%d bad argument: %s", __FILE__, __LINE__, #c); \
      return PBHC_EINVAL;                                                               \
    }                                                                                   \
  } while (0)


#include "pbhc_env_step.h"

// =================================================================================================
//  k_env_finalize: the scalars the reference updates on the host each step
// =================================================================================================
#include "pbhc_env_finalize.h"      // env_finalize_body: shared with the rider workgroup of the rollout's policy launch (pbhc_mlp.hip)
__global__ __launch_bounds__(64 * PBHC_FIN_CHUNKS) void k_env_finalize(const PbhcEnvConfig* __restrict__ cfgp, double* __restrict__ glob, const float* __restrict__ partials, int nblocks, int32_t* frame_cursor, int num_frames,
                                                                    const double* __restrict__ ext_tot, double* __restrict__ tot_out, double n_total) {
  __shared__ double acc[PBHC_FIN_CHUNKS * 64];
  __shared__ double tot[PBHC_NP];
  env_finalize_body<64 * PBHC_FIN_CHUNKS>(acc, tot, cfgp, glob, partials, nblocks, frame_cursor, num_frames, ext_tot, tot_out, n_total);
}

// =================================================================================================
//  k_dof_far_any: the batch-global decision of termination.terminate_when_dof_far (motion_tracking.py:343-349,
//  torch.any(norm(dif_joint_angles, dim=-1) > threshold) over the ENV axis: one env past the threshold resets every env of the step).
//  A pre-pass on the step's stream right before k_env_step, launched only when the switch is on: k_env_step's workgroups are not
//  co-resident at large env counts, so the decision cannot be exchanged inside it (a grid barrier there would deadlock).  Per env it
//  evaluates |ref dof_pos - dof_pos| exactly as k_env_step's role B does — the replay frame the step will read, the reference at the
//  step's pre-reset time (ep_len + 2) dt + start with frame_blend and the same lerp, the same 32-lane reduction — so that the decision
//  agrees bit for bit with the norm the step logs.  One device-scope atomic per workgroup sets PBHC_G_DOF_FAR_HIT; k_env_step reads it
//  once, k_env_finalize clears it (stream order: finalize of step t precedes the pre-pass of step t + 1, in a captured graph too).
// =================================================================================================
#define DOF_FAR_EPB 8                                             // envs per 256-thread workgroup: 32 lanes per env
__global__ __launch_bounds__(PBHC_G * DOF_FAR_EPB) void k_dof_far_any(const long long* __restrict__ ep_len, const float* __restrict__ start,
                                                                       const float* __restrict__ frame_q, const int32_t* __restrict__ cursor,
                                                                       int frame_index, int num_frames, int N, int D, float dt, PbhcMotionTable tbl,
                                                                       const int64_t* __restrict__ motion_ids, double* __restrict__ glob) {
  const int lane = threadIdx.x & (PBHC_G - 1);
  const int env = blockIdx.x * DOF_FAR_EPB + (int)(threadIdx.x / PBHC_G);
  const bool valid = env < N;
  const int envc = valid ? env : N - 1;
  const int dc = min(lane, D - 1);
  const size_t fk = (size_t)(frame_index >= 0 ? frame_index : cursor[0] % num_frames) * (size_t)N;
  const int mid = (int)motion_ids[envc];
  float m_len = tbl.single_len, m_dt = tbl.single_dt;
  int m_nf = tbl.single_num_frames, m_row0 = 0;
  if (tbl.num_motions != 1) { m_len = tbl.motion_len[mid]; m_nf = tbl.num_frames[mid]; m_dt = tbl.motion_dt[mid]; m_row0 = tbl.length_starts[mid]; }
  const long long ep1 = ep_len[envc] + 1;
  const float tref = (float)(ep1 + 1) * dt + start[envc];
  int f0, f1;
  float blend;
  frame_blend(tref, m_len, m_nf, m_dt, &f0, &f1, &blend);
  const float rd0 = tbl.frames[(size_t)(m_row0 + f0) * tbl.row + dc], rd1 = tbl.frames[(size_t)(m_row0 + f1) * tbl.row + dc];
  const float q = frame_q[fk * D + (size_t)envc * D + dc];
  const float a = 1.0f - blend;
  const float dj = (a * rd0 + blend * rd1) - q;
  float s = 0.0f;
  if (lane < D) s += dj * dj;
  s = group_sum(s);
  const bool far = valid && sqrtf(s) > (float)glob[PBHC_G_DOF_FAR_THR];
  if (__syncthreads_or(far) && threadIdx.x == 0)
    __hip_atomic_store(glob + PBHC_G_DOF_FAR_HIT, 1.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// =================================================================================================
//  k_record_motion: one frame of the evaluation recorder (env.config.save_motion; motion_tracking.py:861-938 keeps twelve python lists of
//  .cpu() copies and a scipy call per control step).  Launched right after k_env_step, only when the recorder is on; it copies the step's
//  post-reset state into [N, T, ...] buffers whose frame index comes from a device-side counter, so a captured graph replays it.
//  Layout: env n's T frames of a key are contiguous (what the reference's stack + transpose(0, 1) produces), i.e. a step writes N rows of
//  `row` floats with a stride of T * row.  Mapping: the frame of one env is W = 546 words (v1 / 23 dof: actor_obs 380, pose_aa 81, dof,
//  dof_vel, action 23 each, root 13, contacts 2, one scalar slot); ONE WORD PER LANE-ITEM over the flat index env * W + j, REC_ITEMS items
//  per thread a block apart.  Consecutive lanes hold consecutive words of one destination row and run on into the env's next key, so a
//  wave store is 64 dwords in one or two contiguous segments (one 256-B segment inside an actor_obs row of 1520 B) and the sources — [N, row]
//  tensors — are read coalesced; every thread issues the loads of all its items before its first store, and with ~2 k workgroups at 4096
//  envs the latency of the short rows is hidden by occupancy instead of by a loop (a first version — 8 envs per workgroup, key after key —
//  was a chain of ~25 dependent round trips per wave: 0.9 TB/s).  Offsets are 64-bit: N * T * row passes 2^31 bytes.
//  The counter: every workgroup reads it first; the LAST one to finish advances it.  "Last" is a two-level arrival ticket — PBHC_REC_SHARDS
//  shard words on lines of their own, then one top word — because ~25 ns per same-address atomic made a single ticket word the whole cost
//  of the kernel (124 us at 32 768 envs with 4096 workgroups, measured).
// =================================================================================================
#define REC_TPB 256
#define REC_ITEMS 4
struct RecSrc {
  const float* root; const float* dof_state; const float* actions; const float* contacts_filt; const float* origins; const float* start;
  const float* obs; const long long* ep_len; const long long* reset;
  int obs_pitch, obs_dim;
};
__global__ __launch_bounds__(REC_TPB) void k_record_motion(RecSrc s, PbhcRecordIO r, const PbhcEnvConfig* __restrict__ cfgp, int N, int D, int Bx, float dt) {
  __shared__ int s_cnt, s_last;
  const int tid = threadIdx.x;
  if (tid == 0) s_cnt = __hip_atomic_load(r.counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  const int cnt = s_cnt, T = r.total_steps;
  const int f = cnt - 3;                                    // the reference drops its first three records (v[3:])
  if (f >= 0 && f < T) {
    const int prow = Bx * 3;
    const int W = s.obs_dim + prow + 3 * D + 16;            // + root_rot 4, root_trans_offset / lin vel / ang vel 3 each, contact 2, scalars 1
    const unsigned total = (unsigned)N * (unsigned)W;       // (< 2^31: checked by pbhc_record_motion; only the DESTINATION offsets need 64 bits)
    const unsigned base = blockIdx.x * (unsigned)(REC_TPB * REC_ITEMS) + tid;
    int env0 = (int)(base / (unsigned)W), j0 = (int)(base - (unsigned)env0 * (unsigned)W);      // one division per thread, then steps of REC_TPB
    float* dst[REC_ITEMS];
    float val[REC_ITEMS];
    long long term = 0;
    long long* dst_term = nullptr;
#pragma unroll
    for (int it = 0; it < REC_ITEMS; ++it) {
      const unsigned i = base + (unsigned)it * REC_TPB;
      dst[it] = nullptr;
      val[it] = 0.0f;
      const int env = env0;
      int j = j0;
      j0 += REC_TPB;
      while (j0 >= W) { j0 -= W; ++env0; }
      if (i >= total) continue;
      const size_t ef = (size_t)env * (size_t)T + (size_t)f;  // row index of (env, frame) in every [N, T, row] buffer
      const float* root = s.root + (size_t)env * 13;
      if (j < s.obs_dim) { dst[it] = r.actor_obs + ef * s.obs_dim + j; val[it] = s.obs[(size_t)env * s.obs_pitch + j]; continue; }
      j -= s.obs_dim;
      if (j < prow) {
        const int b = j / 3, a = j - 3 * b;
        float v = 0.0f;
        if (b == 0) {
          float rv[3];
          rotvec_from_quat<float>(root[3], root[4], root[5], root[6], rv);
          v = a == 0 ? rv[0] : (a == 1 ? rv[1] : rv[2]);
        } else if (b <= D) {
          v = cfgp->skel.dof_axis[b - 1][a] * s.dof_state[((size_t)env * D + (b - 1)) * 2];
        }
        dst[it] = r.pose_aa + ef * prow + j; val[it] = v; continue;
      }
      j -= prow;
      if (j < D) { dst[it] = r.dof + ef * D + j; val[it] = s.dof_state[((size_t)env * D + j) * 2]; continue; }
      j -= D;
      if (j < D) { dst[it] = r.dof_vel + ef * D + j; val[it] = s.dof_state[((size_t)env * D + j) * 2 + 1]; continue; }
      j -= D;
      if (j < D) { dst[it] = r.action + ef * D + j; val[it] = s.actions[(size_t)env * D + j]; continue; }
      j -= D;
      if (j < 4) { dst[it] = r.root_rot + ef * 4 + j; val[it] = root[3 + j]; continue; }
      j -= 4;
      if (j < 3) { dst[it] = r.root_trans_offset + ef * 3 + j; val[it] = root[j] - s.origins[(size_t)env * 3 + j]; continue; }
      j -= 3;
      if (j < 3) { dst[it] = r.root_lin_vel + ef * 3 + j; val[it] = root[7 + j]; continue; }
      j -= 3;
      if (j < 3) { dst[it] = r.root_ang_vel + ef * 3 + j; val[it] = root[10 + j]; continue; }
      j -= 3;
      if (j < 2) { dst[it] = r.contact_mask + ef * 2 + j; val[it] = s.contacts_filt[(size_t)env * 2 + j]; continue; }
      // the scalar slot: motion_times here, terminate (int64) beside it
      dst[it] = r.motion_times + ef; val[it] = (float)s.ep_len[env] * dt + s.start[env];
      dst_term = (long long*)r.terminate + ef; term = s.reset[env];
    }
#pragma unroll
    for (int it = 0; it < REC_ITEMS; ++it)
      if (dst[it]) *dst[it] = val[it];
    if (dst_term) *dst_term = term;
  }
  // every workgroup has read the counter (above, before its barrier) by the time it arrives here: the last arrival advances it
  if (tid == 0) {
    const int nb = (int)gridDim.x, shard = (int)blockIdx.x % PBHC_REC_SHARDS;
    const int in_shard = (nb - shard + PBHC_REC_SHARDS - 1) / PBHC_REC_SHARDS, shards = nb < PBHC_REC_SHARDS ? nb : PBHC_REC_SHARDS;
    int last = 0;
    if (__hip_atomic_fetch_add(r.counter + 32 * (2 + shard), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == in_shard - 1)
      last = __hip_atomic_fetch_add(r.counter + 32, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == shards - 1;
    s_last = last;
  }
  __syncthreads();
  if (s_last) {                                             // tickets back to zero for the next launch, then the counter itself
    for (int k = tid; k < PBHC_REC_SHARDS + 1; k += REC_TPB) __hip_atomic_store(r.counter + 32 * (1 + k), 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid == 0) __hip_atomic_store(r.counter, cnt < T + 3 ? cnt + 1 : cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// =================================================================================================
//  standalone kernels: sim FK, motion state, load-time motion build
// =================================================================================================
__global__ __launch_bounds__(PBHC_G* PBHC_EPB) void k_sim_fk(PbhcSkeleton sk, const float* __restrict__ root_states, const float* __restrict__ dof_pos,
                                                            const float* __restrict__ dof_vel, int dof_stride, int n, float* __restrict__ out) {
  __shared__ float sm[PBHC_EPB][16 + 64 + PBHC_MAX_BODIES * 17];
  __shared__ float skc[SKC_WORDS];
  const int lane = threadIdx.x & (PBHC_G - 1), le = threadIdx.x / PBHC_G, env = blockIdx.x * PBHC_EPB + le;
  const bool valid = env < n;
  float* root = sm[le];
  float *q = root + 16, *qd = q + 32, *bp = qd + 32, *bq = bp + 3 * PBHC_MAX_BODIES, *bv = bq + 4 * PBHC_MAX_BODIES, *bw = bv + 3 * PBHC_MAX_BODIES;
  float* relq = bw + 3 * PBHC_MAX_BODIES;
  stage_skeleton(sk, skc);

  if (valid) {
    if (lane < 13) root[lane] = root_states[(size_t)env * 13 + lane];
    for (int d = lane; d < sk.num_dof; d += PBHC_G) {
      q[d] = dof_pos[((size_t)env * sk.num_dof + d) * dof_stride];
      qd[d] = dof_vel[((size_t)env * sk.num_dof + d) * dof_stride];
    }
  }
  __syncthreads();
  fk_walk(skc, sk.num_bodies, sk.num_bodies, lane, valid, root, q, qd, relq, bp, bq, bv, bw);
  if (valid)
    for (int b = lane; b < sk.num_bodies; b += PBHC_G) {
      float* o = out + ((size_t)env * sk.num_bodies + b) * 13;
      st3(o, ld3(bp + 3 * b)); st4(o + 3, ld4(bq + 4 * b)); st3(o + 7, ld3(bv + 3 * b)); st3(o + 10, ld3(bw + 3 * b));
    }
}

__global__ __launch_bounds__(PBHC_G* PBHC_EPB) void k_motion_state(PbhcMotionTable tbl, int Bx, int D, const int64_t* __restrict__ ids, const float* __restrict__ times,
                                                                  const float* __restrict__ offset, int n, float* __restrict__ out) {
  __shared__ float sm[PBHC_EPB][64 + 8 + PBHC_MAX_BODIES * 13];
  const int lane = threadIdx.x & (PBHC_G - 1), le = threadIdx.x / PBHC_G, i = blockIdx.x * PBHC_EPB + le;
  const bool valid = i < n;
  float* rdof = sm[le];
  float *rdofv = rdof + 32, *rc = rdofv + 32, *rp = rc + 8, *rq = rp + 3 * PBHC_MAX_BODIES, *rv = rq + 4 * PBHC_MAX_BODIES, *rw = rv + 3 * PBHC_MAX_BODIES;
  if (valid) {
    f3 off = offset ? ld3(offset + (size_t)i * 3) : mk3(0.f, 0.f, 0.f);
    motion_lookup(tbl, D, Bx, lane, (int)ids[i], times[i], off, true, rdof, rdofv, rc, rp, rq, rv, rw);
  }
  __syncthreads();
  if (!valid) return;
  float* o = out + (size_t)i * tbl.row;
  for (int d = lane; d < D; d += PBHC_G) { o[d] = rdof[d]; o[D + d] = rdofv[d]; }
  if (lane < 2) o[2 * D + lane] = rc[lane];
  int o_pos = 2 * D + 2, o_rot = o_pos + 3 * Bx, o_vel = o_rot + 4 * Bx, o_ang = o_vel + 3 * Bx;
  for (int k = lane; k < 3 * Bx; k += PBHC_G) { o[o_pos + k] = rp[k]; o[o_vel + k] = rv[k]; o[o_ang + k] = rw[k]; }
  for (int k = lane; k < 4 * Bx; k += PBHC_G) o[o_rot + k] = rq[k];
}

// load-time FK: one thread per frame walks the chain (Humanoid_Batch.fk_batch +
// forward_kinematics_batch, torch_humanoid_batch.py:168-269)
__global__ void k_motion_fk(PbhcSkeleton sk, const float* __restrict__ pose_aa, const float* __restrict__ trans, int F,
                            float* __restrict__ pos, float* __restrict__ rot) {
  int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  const int Bx = sk.num_bodies_ext;
  m33 W[PBHC_MAX_BODIES];
  float P[PBHC_MAX_BODIES][3];
  for (int i = 0; i < Bx; ++i) {
    const float* aa = pose_aa + ((size_t)f * Bx + i) * 3;
    float qw[4];
    axis_angle_to_quat_wxyz(aa[0], aa[1], aa[2], qw);
    m33 J = quat_wxyz_to_matrix(qw[0], qw[1], qw[2], qw[3]);
    int p = sk.parent[i];
    if (p < 0) {
      W[i] = J;
      P[i][0] = trans[f * 3 + 0]; P[i][1] = trans[f * 3 + 1]; P[i][2] = trans[f * 3 + 2];
    } else {
      const float* o = sk.offset[i];
      const m33& Rp = W[p];
      P[i][0] = Rp.m[0] * o[0] + Rp.m[1] * o[1] + Rp.m[2] * o[2] + P[p][0];
      P[i][1] = Rp.m[3] * o[0] + Rp.m[4] * o[1] + Rp.m[5] * o[2] + P[p][1];
      P[i][2] = Rp.m[6] * o[0] + Rp.m[7] * o[1] + Rp.m[8] * o[2] + P[p][2];
      m33 Lm = quat_wxyz_to_matrix(sk.local_rot_wxyz[i][0], sk.local_rot_wxyz[i][1], sk.local_rot_wxyz[i][2], sk.local_rot_wxyz[i][3]);
      W[i] = matmul33(Rp, matmul33(Lm, J));
    }
    float* po = pos + ((size_t)f * Bx + i) * 3;
    po[0] = P[i][0]; po[1] = P[i][1]; po[2] = P[i][2];
    st4(rot + ((size_t)f * Bx + i) * 4, matrix_to_quat_xyzw(W[i]));
  }
}

// raw velocities: np.gradient/dt and angle-axis of q_{t+1} * conj(q_t) (torch_humanoid_batch.py:272-290)
// `frame_clip` / `clip_start` / `clip_dt` (may be NULL: one clip of F frames): frame -> clip, first frame of every clip (+ the total),
// frame time per clip — the batched build of a whole library in one launch set (pbhc_motion_build_batch)
__global__ void k_motion_rawvel(const float* __restrict__ pos, const float* __restrict__ rot, int Ftot, int Bx, float dt1,
                                const int32_t* __restrict__ frame_clip, const int32_t* __restrict__ clip_start, const float* __restrict__ clip_dt,
                                float* __restrict__ vel, float* __restrict__ ang) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Ftot * Bx) return;
  int fg = i / Bx, b = i % Bx;
  int base = 0, F = Ftot;
  float dt = dt1;
  if (frame_clip) { const int cidx = frame_clip[fg]; base = clip_start[cidx]; F = clip_start[cidx + 1] - base; dt = clip_dt[cidx]; }
  const int f = fg - base;
  auto P = [&](int ff, int k) { return pos[((size_t)(base + ff) * Bx + b) * 3 + k]; };
  for (int k = 0; k < 3; ++k) {
    float g;
    if (F == 1) g = 0.0f;
    else if (f == 0) g = (P(1, k) - P(0, k)) / 1.0f;
    else if (f == F - 1) g = (P(F - 1, k) - P(F - 2, k)) / 1.0f;
    else g = (P(f + 1, k) - P(f - 1, k)) / 2.0f;
    vel[(size_t)i * 3 + k] = g / dt;
  }
  f4 dq = mk4(0.f, 0.f, 0.f, 1.f);
  if (f < F - 1) dq = quat_unit(quat_mul(ld4(rot + ((size_t)(fg + 1) * Bx + b) * 4), quat_conj(ld4(rot + ((size_t)fg * Bx + b) * 4))));
  float s = 2.0f * (dq.w * dq.w) - 1.0f;
  float angle = acosf(clampf(s, -1.0f, 1.0f));
  float n = fmaxf(sqrtf(dq.x * dq.x + dq.y * dq.y + dq.z * dq.z), 1e-9f);
  ang[(size_t)i * 3 + 0] = dq.x / n * angle / dt;
  ang[(size_t)i * 3 + 1] = dq.y / n * angle / dt;
  ang[(size_t)i * 3 + 2] = dq.z / n * angle / dt;
}

// scipy.ndimage.gaussian_filter1d(sigma=2, mode="nearest", truncate=4) along time, double accumulation,
// then pack the frame rows
__global__ void k_motion_pack(PbhcSkeleton sk, const float* __restrict__ pose_aa, const float* __restrict__ contact, const float* __restrict__ pos,
                              const float* __restrict__ rot, const float* __restrict__ vel, const float* __restrict__ ang, int Ftot, float dt1, int row,
                              const int32_t* __restrict__ frame_clip, const int32_t* __restrict__ clip_start, const float* __restrict__ clip_dt,
                              float* __restrict__ out) {
  const int Bx = sk.num_bodies_ext, D = sk.num_dof, B = sk.num_bodies;
  const int fg = blockIdx.x;
  int base = 0, F = Ftot;
  float dt = dt1;
  if (frame_clip) { const int cidx = frame_clip[fg]; base = clip_start[cidx]; F = clip_start[cidx + 1] - base; dt = clip_dt[cidx]; }
  const int f = fg - base;
  // everything below indexes frames of THIS clip: shift the per-frame arrays to its first frame
  pose_aa += (size_t)base * Bx * 3; pos += (size_t)base * Bx * 3; rot += (size_t)base * Bx * 4; vel += (size_t)base * Bx * 3; ang += (size_t)base * Bx * 3;
  if (contact) contact += (size_t)base * 2;
  float* o = out + (size_t)fg * row;
  double w[9];
  double wsum = 0.0;
  for (int k = 0; k <= 8; ++k) { w[k] = exp(-0.5 * (double)(k * k) / 4.0); wsum += (k == 0 ? 1.0 : 2.0) * w[k]; }
  const int o_pos = 2 * D + 2, o_rot = o_pos + 3 * Bx, o_vel = o_rot + 4 * Bx, o_ang = o_vel + 3 * Bx;
  for (int i = threadIdx.x; i < Bx * 3; i += blockDim.x) {
    double av = 0.0, aw = 0.0;
    for (int k = -8; k <= 8; ++k) {
      int ff = min(max(f + k, 0), F - 1);
      double wk = w[k < 0 ? -k : k] / wsum;
      av += wk * (double)vel[(size_t)ff * Bx * 3 + i];
      aw += wk * (double)ang[(size_t)ff * Bx * 3 + i];
    }
    o[o_vel + i] = (float)av; o[o_ang + i] = (float)aw;
    o[o_pos + i] = pos[(size_t)f * Bx * 3 + i];
  }
  for (int i = threadIdx.x; i < Bx * 4; i += blockDim.x) o[o_rot + i] = rot[(size_t)f * Bx * 4 + i];
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    auto dofp = [&](int ff) {
      const float* aa = pose_aa + ((size_t)ff * Bx + (d + 1)) * 3;
      return aa[0] + aa[1] + aa[2];                                   // pose_aa.sum(-1)[1:B]  (:216)
    };
    o[d] = dofp(f);
    float dv;
    if (F < 2) dv = 0.0f;
    else if (f < F - 1) dv = (dofp(f + 1) - dofp(f)) / dt;
    else { int g = F >= 3 ? F - 3 : 0; dv = (dofp(g + 1) - dofp(g)) / dt; }   // `dof_vel[:, -2:-1]`, sic (:224)
    o[D + d] = dv;
  }
  if (threadIdx.x < 2) o[2 * D + threadIdx.x] = contact ? contact[(size_t)f * 2 + threadIdx.x] : 0.0f;
  (void)B;
}

// =================================================================================================
//  GAE (MHPPO._compute_returns mh_ppo.py:348-395)
// =================================================================================================
#define GAE_TPB 256
__global__ __launch_bounds__(GAE_TPB) void k_gae(const float* __restrict__ rewards, const float* __restrict__ values, const uint8_t* __restrict__ dones,
                                                 const float* __restrict__ last_values, int T, int N, int R, float gamma, float lam,
                                                 float* __restrict__ returns) {
  // thread <-> (env, head): consecutive threads walk consecutive floats of every [t] slab
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)N * R) return;
  int n = (int)(i / R);
  float adv = 0.0f;
  float next = last_values[i];
  for (int t = T - 1; t >= 0; --t) {
    size_t o = (size_t)t * N * R + i;
    float nt = 1.0f - (dones[(size_t)t * N + n] ? 1.0f : 0.0f);
    float v = values[o];
    float delta = rewards[o] + nt * gamma * next - v;
    adv = delta + nt * gamma * lam * adv;
    returns[o] = adv + v;
    next = v;
  }
}
// advantages = sum over heads of (returns - values); block partial sums of x and x^2 (double)
__global__ __launch_bounds__(GAE_TPB) void k_adv_sum(const float* __restrict__ returns, const float* __restrict__ values, size_t TN, int R,
                                                     float* __restrict__ adv, double* __restrict__ part) {
  __shared__ double s1[GAE_TPB], s2[GAE_TPB];
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  double a = 0.0;
  if (i < TN) {
    float s = 0.0f;
    for (int r = 0; r < R; ++r) s += returns[i * R + r] - values[i * R + r];
    adv[i] = s;
    a = (double)s;
  }
  s1[threadIdx.x] = a; s2[threadIdx.x] = a * a;
  __syncthreads();
  for (int st = GAE_TPB / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) { s1[threadIdx.x] += s1[threadIdx.x + st]; s2[threadIdx.x] += s2[threadIdx.x + st]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = s1[0]; part[2 * blockIdx.x + 1] = s2[0]; }
}
// mean / unbiased std of the advantages from the block partials, then the normalisation — in ONE launch: every block re-sums the (few hundred)
// partial pairs itself, all in the same fixed order (thread i takes partials i, i + 256, ...; then a tree), so every block normalises with the
// same two numbers; block 0 also leaves them behind the partials (part[2 nblocks], part[2 nblocks + 1]: the data-parallel path re-normalises
// with the all-rank moments).  (Was a one-thread serial sum, 34 us, and a launch of its own.)
__global__ __launch_bounds__(GAE_TPB) void k_adv_norm(float* __restrict__ adv, size_t TN, double* __restrict__ part, int nblocks) {
  __shared__ double s1[GAE_TPB], s2[GAE_TPB];
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += GAE_TPB) { a += part[2 * i]; b += part[2 * i + 1]; }
  s1[threadIdx.x] = a; s2[threadIdx.x] = b;
  __syncthreads();
  for (int st = GAE_TPB / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) { s1[threadIdx.x] += s1[threadIdx.x + st]; s2[threadIdx.x] += s2[threadIdx.x + st]; }
    __syncthreads();
  }
  const double n = (double)TN;
  const double mean_d = s1[0] / n;
  const double var = (s2[0] - n * mean_d * mean_d) / (n - 1.0);       // torch.std: unbiased
  const double sd_d = sqrt(var < 0.0 ? 0.0 : var);                    // (T*N = 1: 0 / 0 stays NaN, as torch.std of one element)
  if (blockIdx.x == 0 && threadIdx.x == 0) { part[2 * nblocks] = mean_d; part[2 * nblocks + 1] = sd_d; }
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= TN) return;
  const float mean = (float)mean_d, sd = (float)sd_d;
  adv[i] = (adv[i] - mean) / (sd + 1e-8f);
}

// =================================================================================================
//  C ABI
// =================================================================================================
// LDS slot of the reduction row that IS the raw value of a reward term, or -1 for the terms computed by a case of the kernel's switch
static int term_source(int id) {
  switch (id) {
    case PBHC_R_TELEOP_MAX_JOINT_POSITION: return R_EXP0 + PBHC_S_MAX_JOINT_POS;
    case PBHC_R_TELEOP_VR_3POINT: return R_EXP0 + PBHC_S_VR_3POINT_POS;
    case PBHC_R_TELEOP_BODY_POSITION_FEET: return R_EXP0 + PBHC_S_FEET_POS;
    case PBHC_R_TELEOP_BODY_ROTATION_EXTEND: return R_EXP0 + PBHC_S_BODY_ROT;
    case PBHC_R_TELEOP_BODY_ANG_VELOCITY_EXTEND: return R_EXP0 + PBHC_S_BODY_ANG_VEL;
    case PBHC_R_TELEOP_BODY_VELOCITY_EXTEND: return R_EXP0 + PBHC_S_BODY_VEL;
    case PBHC_R_TELEOP_JOINT_POSITION: return R_EXP0 + PBHC_S_JOINT_POS;
    case PBHC_R_TELEOP_JOINT_VELOCITY: return R_EXP0 + PBHC_S_JOINT_VEL;
    case PBHC_R_PENALTY_TORQUES: return R_TAU2;
    case PBHC_R_PENALTY_DOF_VEL: return R_QD2;
    case PBHC_R_PENALTY_DOF_ACC: return R_QACC2;
    case PBHC_R_PENALTY_ACTION_RATE: return R_ARATE;
    case PBHC_R_LIMITS_DOF_POS: return R_LIMPOS;
    case PBHC_R_LIMITS_DOF_VEL: return R_LIMVEL;
    case PBHC_R_LIMITS_TORQUE: return R_LIMTAU;
    case PBHC_R_COLLISION: return R_COLL;
    case PBHC_R_TELEOP_KEY_BODY_POSITION: return R_EXP0 + PBHC_S_KEY_BODY_POS;
    case PBHC_R_TELEOP_ANCHOR_BODY_POSITION: return R_EXP0 + PBHC_S_ANCHOR_BODY_POS;
    case PBHC_R_TELEOP_ANCHOR_BODY_ROTATION: return R_EXP0 + PBHC_S_ANCHOR_BODY_ROT;
    case PBHC_R_LOCAL_KEY_BODY_POSITION: return R_EXP0 + PBHC_S_LOCAL_KEY_BODY_POS;
    case PBHC_R_LOCAL_KEY_BODY_ROTATION: return R_EXP0 + PBHC_S_LOCAL_KEY_BODY_ROT;
    case PBHC_R_KEY_BODY_VELOCITY: return R_EXP0 + PBHC_S_KEY_BODY_VEL;
    case PBHC_R_KEY_BODY_ANG_VELOCITY: return R_EXP0 + PBHC_S_KEY_BODY_ANG_VEL;
    case PBHC_R_TELEOP_ROOT_VEL: return R_EXP0 + PBHC_S_ROOT_VEL;
    case PBHC_R_TELEOP_ROOT_POSE: return R_EXP0 + PBHC_S_ROOT_POSE;
    default: return -1;
  }
}

struct PbhcEnv {
  PbhcEnvConfig cfg;
  PbhcEnvConfig* d_cfg;
  PbhcMotionTable tbl;
  double* d_glob;
  float* d_partials;
  float* d_skc;
  float* d_skj;              // per-body rows of the pointer-jumping chain (fk_jump_wave: skj_word)
  int nblocks;
  int lds_stride;
  size_t lds_bytes;
  uint32_t step_ctr;
  int profile;
  int prof_count;
  hipEvent_t ev0[PBHC_PROFILE_RING], ev1[PBHC_PROFILE_RING];
  const void* spec_fn;       // config-specialised k_env_step (pbhc_env_attach_specialised), or nullptr: the generic kernel
  void* spec_dl;
  int spec_lds_stride;       // ... and its own LDS plan (step_lds_plan)
  size_t spec_lds_bytes;
  int spec_hist_wide;        // ... which may read the history rows 16 bytes per lane
};

extern "C" {

int pbhc_abi_version(void) { return PBHC_ABI_VERSION; }
#ifdef PBHC_STAMPS
int pbhc_debug_read_stamps(unsigned long long* out, int n) {
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * (n < 64 ? n : 64)));
  return PBHC_OK;
}
int pbhc_debug_read_wg_times(unsigned long long* out, int num_workgroups) {
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wg_times), sizeof(unsigned long long) * 2 * (num_workgroups < 4096 ? num_workgroups : 4096)));
  return PBHC_OK;
}
#endif
const char* pbhc_last_error(void) { return g_err; }
int pbhc_sizeof_env_config(void) { return (int)sizeof(PbhcEnvConfig); }
int pbhc_sizeof_step_io(void) { return (int)sizeof(PbhcStepIO); }
int pbhc_sizeof_record_io(void) { return (int)sizeof(PbhcRecordIO); }

// (not in the header: shared with pbhc_clip_track.hip, whose kernel indexes LDS with the same chain tables)
int pbhc_check_skel(const PbhcSkeleton* sk) {
  ARG_CHECK(sk != nullptr);
  ARG_CHECK(sk->num_bodies >= 1 && sk->num_bodies <= sk->num_bodies_ext && sk->num_bodies_ext <= PBHC_MAX_BODIES);
  ARG_CHECK(sk->num_dof == sk->num_bodies - 1 && sk->num_dof <= PBHC_MAX_DOF);
  ARG_CHECK(sk->parent[0] == -1);
  for (int i = 1; i < sk->num_bodies_ext; ++i) ARG_CHECK(sk->parent[i] >= 0 && sk->parent[i] < i && sk->parent[i] < sk->num_bodies);
  for (int i = 1; i < sk->num_bodies; ++i) ARG_CHECK(sk->depth[i] == sk->depth[sk->parent[i]] + 1 && sk->depth[i] <= sk->max_depth);
  for (int b = 0; b < sk->num_bodies_ext; ++b) {
    const int node = b < sk->num_bodies ? b : sk->parent[b];
    ARG_CHECK(sk->chain_len[b] == sk->depth[node] && sk->chain_len[b] <= PBHC_MAX_DEPTH);
    int cur = node;
    for (int k = sk->chain_len[b] - 1; k >= 0; --k) { ARG_CHECK(sk->chain[b][k] == cur && cur >= 1 && cur < sk->num_bodies); cur = sk->parent[cur]; }
    ARG_CHECK(cur == 0);
  }
  return PBHC_OK;
}

int pbhc_motion_build(const PbhcSkeleton* skel, const float* pose_aa, const float* trans, const float* contact, int F, float dt,
                      float* out_rows, float* scratch, void* stream) {
  int rc = pbhc_check_skel(skel);
  if (rc) return rc;
  ARG_CHECK(pose_aa && trans && out_rows && scratch && F >= 1 && dt > 0.0f);
  hipStream_t st = (hipStream_t)stream;
  const int Bx = skel->num_bodies_ext, D = skel->num_dof;
  const int row = 2 * D + 2 + 13 * Bx;
  float* pos = scratch;
  float* rot = pos + (size_t)F * Bx * 3;
  float* vel = rot + (size_t)F * Bx * 4;
  float* ang = vel + (size_t)F * Bx * 3;
  hipLaunchKernelGGL(k_motion_fk, dim3((F + 63) / 64), dim3(64), 0, st, *skel, pose_aa, trans, F, pos, rot);
  hipLaunchKernelGGL(k_motion_rawvel, dim3((F * Bx + 127) / 128), dim3(128), 0, st, pos, rot, F, Bx, dt, (const int32_t*)nullptr, (const int32_t*)nullptr,
                     (const float*)nullptr, vel, ang);
  hipLaunchKernelGGL(k_motion_pack, dim3(F), dim3(128), 0, st, *skel, pose_aa, contact, pos, rot, vel, ang, F, dt, row, (const int32_t*)nullptr,
                     (const int32_t*)nullptr, (const float*)nullptr, out_rows);
  HIP_CHECK(hipGetLastError());
  return PBHC_OK;
}

int pbhc_motion_build_batch(const PbhcSkeleton* skel, const float* pose_aa, const float* trans, const float* contact, int total_frames, int num_clips,
                            const int32_t* frame_clip, const int32_t* clip_start, const float* clip_dt, float* out_rows, float* scratch, void* stream) {
  int rc = pbhc_check_skel(skel);
  if (rc) return rc;
  ARG_CHECK(pose_aa && trans && out_rows && scratch && frame_clip && clip_start && clip_dt && total_frames >= 1 && num_clips >= 1 && num_clips <= total_frames);
  hipStream_t st = (hipStream_t)stream;
  const int Bx = skel->num_bodies_ext, D = skel->num_dof, F = total_frames;
  const int row = 2 * D + 2 + 13 * Bx;
  float* pos = scratch;
  float* rot = pos + (size_t)F * Bx * 3;
  float* vel = rot + (size_t)F * Bx * 4;
  float* ang = vel + (size_t)F * Bx * 3;
  hipLaunchKernelGGL(k_motion_fk, dim3((F + 63) / 64), dim3(64), 0, st, *skel, pose_aa, trans, F, pos, rot);
  hipLaunchKernelGGL(k_motion_rawvel, dim3((unsigned)(((size_t)F * Bx + 127) / 128)), dim3(128), 0, st, pos, rot, F, Bx, 0.0f, frame_clip, clip_start, clip_dt, vel, ang);
  hipLaunchKernelGGL(k_motion_pack, dim3(F), dim3(128), 0, st, *skel, pose_aa, contact, pos, rot, vel, ang, F, 0.0f, row, frame_clip, clip_start, clip_dt, out_rows);
  HIP_CHECK(hipGetLastError());
  return PBHC_OK;
}

int pbhc_motion_state(const PbhcMotionTable* tbl, int Bx, int D, const int64_t* ids, const float* times, const float* offset, int n,
                      float* out, void* stream) {
  ARG_CHECK(tbl && tbl->frames && ids && times && out && n >= 0);
  ARG_CHECK(((uintptr_t)ids & 7) == 0);                                   // int64 elements; every float buffer: 4-byte alignment
  ARG_CHECK(Bx >= 1 && Bx <= PBHC_MAX_BODIES && D >= 1 && D <= PBHC_MAX_DOF && tbl->row == 2 * D + 2 + 13 * Bx);
  if (n == 0) return PBHC_OK;
  hipLaunchKernelGGL(k_motion_state, dim3((n + PBHC_EPB - 1) / PBHC_EPB), dim3(PBHC_G * PBHC_EPB), 0, (hipStream_t)stream, *tbl, Bx, D, ids, times, offset, n, out);
  HIP_CHECK(hipGetLastError());
  return PBHC_OK;
}

int pbhc_sim_fk(const PbhcSkeleton* skel, const float* root_states, const float* dof_pos, const float* dof_vel, int dof_stride, int n,
                float* out, void* stream) {
  int rc = pbhc_check_skel(skel);
  if (rc) return rc;
  ARG_CHECK(root_states && dof_pos && dof_vel && out && n >= 0 && dof_stride >= 1);
  if (n == 0) return PBHC_OK;
  hipLaunchKernelGGL(k_sim_fk, dim3((n + PBHC_EPB - 1) / PBHC_EPB), dim3(PBHC_G * PBHC_EPB), 0, (hipStream_t)stream, *skel, root_states, dof_pos, dof_vel, dof_stride, n, out);
  HIP_CHECK(hipGetLastError());
  return PBHC_OK;
}

// Test-only: the rigid-body state of every body INCLUDING the extended ones by either form of the chain — method 0 the walk (fk_walk, what
// pbhc_sim_fk runs), 1 pointer jumping (fk_jump_wave, what the step kernel runs for robots of <= 32 bodies) — on any skeleton: random trees of
// every depth class (1..4 rounds) in tests/test_gpu_fk.py, where the envs' config-driven tests only reach the G1's three rounds.
__global__ __launch_bounds__(PBHC_G* PBHC_EPB) void k_debug_fk(PbhcSkeleton sk, const float* __restrict__ root_states, const float* __restrict__ dof_pos,
                                                              const float* __restrict__ dof_vel, int n, int method, float* __restrict__ out) {
  __shared__ float sm[PBHC_EPB][16 + 64 + PBHC_MAX_BODIES * 17];
  __shared__ float skc[SKC_WORDS];
  const int lane = threadIdx.x & (PBHC_G - 1), le = threadIdx.x / PBHC_G, env = blockIdx.x * PBHC_EPB + le;
  const bool valid = env < n;
  float* root = sm[le];
  float *q = root + 16, *qd = q + 32, *bp = qd + 32, *bq = bp + 3 * PBHC_MAX_BODIES, *bv = bq + 4 * PBHC_MAX_BODIES, *bw = bv + 3 * PBHC_MAX_BODIES;
  float* relq = bw + 3 * PBHC_MAX_BODIES;
  stage_skeleton(sk, skc);
  if (valid) {
    if (lane < 13) root[lane] = root_states[(size_t)env * 13 + lane];
    for (int d = lane; d < sk.num_dof; d += PBHC_G) { q[d] = dof_pos[(size_t)env * sk.num_dof + d]; qd[d] = dof_vel[(size_t)env * sk.num_dof + d]; }
  }
  __syncthreads();
  const int B = sk.num_bodies, Bx = sk.num_bodies_ext;
  if (method == 0) {
    fk_walk(skc, B, Bx, lane, valid, root, q, qd, relq, bp, bq, bv, bw);
  } else {
    float4 kr[5];
    const int lb = min(lane, Bx - 1);
#pragma unroll
    for (int u = 0; u < 5; ++u) kr[u] = make_float4(skj_word(sk, SKJ_W * lb + 4 * u), skj_word(sk, SKJ_W * lb + 4 * u + 1), skj_word(sk, SKJ_W * lb + 4 * u + 2), skj_word(sk, SKJ_W * lb + 4 * u + 3));
    fk_jump_wave(kr, skel_fk_rounds(sk.max_depth), B, Bx, lane, valid, root, q, qd, bp, bq, bv, bw);
    __syncthreads();
  }
  if (valid)
    for (int b = lane; b < Bx; b += PBHC_G) {
      float* o = out + ((size_t)env * Bx + b) * 13;
      st3(o, ld3(bp + 3 * b)); st4(o + 3, ld4(bq + 4 * b)); st3(o + 7, ld3(bv + 3 * b)); st3(o + 10, ld3(bw + 3 * b));
    }
}
extern "C" int pbhc_debug_fk(const PbhcSkeleton* skel, const float* root_states, const float* dof_pos, const float* dof_vel, int n, int method, float* out, void* stream) {
  ARG_CHECK(skel);
  int rc = pbhc_check_skel(skel);
  if (rc) return rc;
  ARG_CHECK(root_states && dof_pos && dof_vel && out && n >= 0 && (method == 0 || method == 1));
  if (method == 1 && !skel_fk_jump(skel->num_bodies_ext, skel->max_depth)) {
    snprintf(g_err, sizeof(g_err), "pbhc_debug_fk: pointer jumping needs <= %d bodies and a chain of <= 15 joints", PBHC_G);
    return PBHC_EINVAL;
  }
  if (n == 0) return PBHC_OK;
  hipLaunchKernelGGL(k_debug_fk, dim3((n + PBHC_EPB - 1) / PBHC_EPB), dim3(PBHC_G * PBHC_EPB), 0, (hipStream_t)stream, *skel, root_states, dof_pos, dof_vel, n, method, out);
  HIP_CHECK(hipGetLastError());
  return PBHC_OK;
}

// Validation + the members pbhc_env_create derives (term_src, sum_col_term, whether the compact observation maps fit in LDS): host
// arithmetic only, so that a specialised kernel can be generated for a config without a device at hand (pbhc_env_config_finalize).
static int finalize_config(const PbhcEnvConfig* cfg, PbhcEnvConfig* fin, int* lds_stride, size_t* lds_bytes) {
  ARG_CHECK(cfg && fin && lds_stride && lds_bytes);
  ARG_CHECK(cfg->abi_version == PBHC_ENV_CONFIG_VERSION);
  int rc = pbhc_check_skel(&cfg->skel);
  if (rc) return rc;
  const int Bx = cfg->skel.num_bodies_ext;
  ARG_CHECK(cfg->num_envs >= 1);
  ARG_CHECK(cfg->num_feet >= 1 && cfg->num_feet <= PBHC_MAX_FEET);
  ARG_CHECK(cfg->num_terms >= 0 && cfg->num_terms <= PBHC_MAX_TERMS && cfg->num_terms <= PBHC_G && cfg->num_rew_cols <= PBHC_G);
  ARG_CHECK(cfg->num_groups >= 1 && cfg->num_groups <= PBHC_MAX_GROUPS);
  ARG_CHECK(cfg->num_term_contact >= 0 && cfg->num_term_contact <= PBHC_MAX_IDX);
  for (int i = 0; i < cfg->num_term_contact; ++i) ARG_CHECK(cfg->term_contact[i] >= 0 && cfg->term_contact[i] < cfg->skel.num_bodies);
  ARG_CHECK(cfg->queue_len >= 1 && cfg->queue_len <= PBHC_MAX_QUEUE);
  // parallel_serial_*: every listed joint a dof of the skeleton, one column of the [N,J] draws each
  ARG_CHECK(cfg->ps_pd_num >= 0 && cfg->ps_pd_num <= cfg->skel.num_dof && cfg->ps_tau_num >= 0 && cfg->ps_tau_num <= cfg->skel.num_dof);
  for (int d = 0; d < PBHC_MAX_DOF; ++d) {       // (the slot tables are read only when their switch is on)
    if (cfg->ps_pd) ARG_CHECK(cfg->ps_pd_slot[d] >= -1 && cfg->ps_pd_slot[d] < cfg->ps_pd_num && (d < cfg->skel.num_dof || cfg->ps_pd_slot[d] == -1));
    if (cfg->ps_tau) ARG_CHECK(cfg->ps_tau_slot[d] >= -1 && cfg->ps_tau_slot[d] < cfg->ps_tau_num && (d < cfg->skel.num_dof || cfg->ps_tau_slot[d] == -1));
  }
  // the optional features / terms: flags within their ranges, the v1-only ones refused for general tracking
  ARG_CHECK((cfg->obs_extra & ~7) == 0 && (cfg->radial_terms & ~3) == 0);
  ARG_CHECK(cfg->future_ref_steps >= 0 && cfg->future_ref_steps <= PBHC_MAX_FUTURE);
  ARG_CHECK(cfg->tracking_mode == 0 || (cfg->future_ref_steps == 0 && cfg->radial_terms == 0 && (cfg->obs_extra & 1) == 0));
  ARG_CHECK(cfg->feat_dim > 0 && cfg->feat_dim < 16384);
  // the step kernel addresses every per-env tensor with 32-bit element offsets from its base pointer
  ARG_CHECK((uint64_t)cfg->num_envs * (uint64_t)(cfg->skel.num_bodies * 13 > cfg->hist_dim + 64 ? cfg->skel.num_bodies * 13 : cfg->hist_dim + 64) < (1ull << 30));
  for (int g = 0; g < cfg->num_groups; ++g) ARG_CHECK(cfg->groups[g].dim > 0 && cfg->groups[g].src && cfg->groups[g].scale && cfg->groups[g].noise);
  for (int i = 0; i < PBHC_F_NUM; ++i) ARG_CHECK(cfg->feat_off[i] >= 0 && cfg->feat_off[i] < cfg->feat_dim);
  *fin = *cfg;
  for (int i = 0; i < PBHC_MAX_TERMS; ++i) fin->term_src[i] = i < cfg->num_terms ? term_source(cfg->term_id[i]) : -1;
  ARG_CHECK(cfg->num_sum_cols >= 1 && cfg->num_sum_cols <= 32);
  for (int i = 0; i < 32; ++i) fin->sum_col_term[i] = -1;
  for (int i = 0; i < cfg->num_terms; ++i) {
    ARG_CHECK(cfg->term_sum_col[i] >= 0 && cfg->term_sum_col[i] < cfg->num_sum_cols && fin->sum_col_term[cfg->term_sum_col[i]] == -1);
    fin->sum_col_term[cfg->term_sum_col[i]] = i;
  }
  ARG_CHECK(cfg->tracking_mode == 0 || cfg->tracking_mode == 1);
  if (cfg->tracking_mode) {
    ARG_CHECK(cfg->num_key >= 1 && cfg->num_key <= PBHC_MAX_IDX && cfg->anchor_index >= 0 && cfg->anchor_index < Bx);
    ARG_CHECK(cfg->future_num_steps >= 0 && cfg->future_num_steps <= PBHC_MAX_FUTURE);
    for (int k = 0; k < cfg->num_key; ++k) ARG_CHECK(cfg->key[k] >= 0 && cfg->key[k] < Bx);
    for (int k = 0; k < cfg->future_num_steps; ++k) ARG_CHECK(cfg->future_steps[k] >= 0);
  }
  *lds_stride = Lds(Bx, cfg->tracking_mode).feat + ((cfg->feat_dim + 3) & ~3);
  ARG_CHECK(cfg->map_lds_words >= 0);
  if (cfg->map_lds_words > 0) {
    int need = 0;
    for (int g = 0; g < cfg->num_groups; ++g) {
      ARG_CHECK(cfg->groups[g].dst == nullptr && cfg->groups[g].lds_off == need && cfg->groups[g].map_words >= PBHC_MAP_HDR + ((cfg->groups[g].dim + 1) >> 1));
      need += cfg->groups[g].map_words;
    }
    ARG_CHECK(need == cfg->map_lds_words && cfg->feat_dim <= 4096 && cfg->map_image != nullptr);
  }
  {
    // the compact maps must not cost a resident workgroup per CU (160 KB LDS): otherwise the per-element maps stay in global memory
    const size_t base = ((size_t)PBHC_EPB * *lds_stride + (size_t)((Bx * SKC_W + 3) & ~3)) * sizeof(float);
    const size_t with = base + (size_t)cfg->map_lds_words * sizeof(float);
    if (cfg->map_lds_words > 0 && (160 * 1024) / with < (160 * 1024) / base) fin->map_lds_words = 0;
    *lds_bytes = fin->map_lds_words > 0 ? with : base;
  }
  if (*lds_bytes > 160 * 1024) { snprintf(g_err, sizeof(g_err), "feature row too large for LDS"); return PBHC_EINVAL; }
  return PBHC_OK;
}

// `out` = `cfg` as pbhc_env_create would store it.  No device is touched.
int pbhc_env_config_finalize(const PbhcEnvConfig* cfg, PbhcEnvConfig* out) {
  int lds_stride = 0;
  size_t lds_bytes = 0;
  return finalize_config(cfg, out, &lds_stride, &lds_bytes);
}

// dynamic LDS of one k_env_step workgroup (4 envs) for this config, or a negative error code.  No device is touched.
int pbhc_env_config_lds_bytes(const PbhcEnvConfig* cfg) {
  PbhcEnvConfig fin;
  int lds_stride = 0;
  size_t lds_bytes = 0;
  const int rc = finalize_config(cfg, &fin, &lds_stride, &lds_bytes);
  return rc != PBHC_OK ? -rc : (int)lds_bytes;
}

int pbhc_env_create(const PbhcEnvConfig* cfg, const PbhcMotionTable* tbl, double* globals, PbhcEnv** out) {
  ARG_CHECK(cfg && tbl && globals && out);
  PbhcEnv* e = new (std::nothrow) PbhcEnv();
  if (!e) return PBHC_ENOMEM;
  int rc = finalize_config(cfg, &e->cfg, &e->lds_stride, &e->lds_bytes);
  if (rc == PBHC_OK && !(tbl->row == 2 * cfg->skel.num_dof + 2 + 13 * cfg->skel.num_bodies_ext && tbl->frames && tbl->num_motions >= 1)) {
    snprintf(g_err, sizeof(g_err), "pbhc_env_create: motion table does not match the skeleton (row %d)", tbl->row);
    rc = PBHC_EINVAL;
  }
  if (rc != PBHC_OK) { delete e; return rc; }
  const int Bx = cfg->skel.num_bodies_ext;
  e->tbl = *tbl;
  e->d_glob = globals;
  e->nblocks = (cfg->num_envs + PBHC_EPB - 1) / PBHC_EPB;
  e->step_ctr = 0;
  e->profile = 0;
  e->prof_count = 0;
  e->spec_fn = nullptr;
  e->spec_dl = nullptr;
  e->spec_lds_stride = 0;
  e->spec_lds_bytes = 0;
  e->spec_hist_wide = 0;
  if (hipMalloc(&e->d_cfg, sizeof(PbhcEnvConfig)) != hipSuccess) { delete e; return PBHC_ENOMEM; }
  if (hipMalloc(&e->d_partials, (size_t)e->nblocks * 2 * PBHC_NP * sizeof(float)) != hipSuccess) { (void)hipFree(e->d_cfg); delete e; return PBHC_ENOMEM; }
  if (hipMalloc(&e->d_skc, SKC_WORDS * sizeof(float)) != hipSuccess) { (void)hipFree(e->d_cfg); (void)hipFree(e->d_partials); delete e; return PBHC_ENOMEM; }
  {
    float img[SKC_WORDS];
    for (int i = 0; i < SKC_WORDS; ++i) img[i] = i < Bx * SKC_W ? skel_word(cfg->skel, i) : 0.0f;
    HIP_CHECK(hipMemcpy(e->d_skc, img, sizeof(img), hipMemcpyHostToDevice));
  }
  if (hipMalloc(&e->d_skj, PBHC_MAX_BODIES * SKJ_W * sizeof(float)) != hipSuccess) { (void)hipFree(e->d_cfg); (void)hipFree(e->d_partials); (void)hipFree(e->d_skc); delete e; return PBHC_ENOMEM; }
  {
    float img[PBHC_MAX_BODIES * SKJ_W];
    for (int i = 0; i < PBHC_MAX_BODIES * SKJ_W; ++i) img[i] = i < Bx * SKJ_W ? skj_word(cfg->skel, i) : 0.0f;
    HIP_CHECK(hipMemcpy(e->d_skj, img, sizeof(img), hipMemcpyHostToDevice));
  }
  HIP_CHECK(hipMemcpy(e->d_cfg, &e->cfg, sizeof(PbhcEnvConfig), hipMemcpyHostToDevice));
  if (e->lds_bytes > 64 * 1024)
    HIP_CHECK(hipFuncSetAttribute(cfg->tracking_mode ? (const void*)k_env_step<1> : (const void*)k_env_step<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)e->lds_bytes));
  *out = e;
  return PBHC_OK;
}

// the config as pbhc_env_create finalised it (term_src, sum_col_term, map_lds_words): what a specialised kernel is generated from
int pbhc_env_get_config(PbhcEnv* e, PbhcEnvConfig* out) {
  ARG_CHECK(e && out);
  *out = e->cfg;
  return PBHC_OK;
}

// for the library's other units (pbhc_joint_sim.hip; not part of the ABI): the parts of an env handle that a launch of theirs in front of the
// step needs — the finalised config on the host and on the device, the motion table, the globals
int pbhc_env_parts(PbhcEnv* e, const PbhcEnvConfig** host_cfg, const PbhcEnvConfig** dev_cfg, const PbhcMotionTable** tbl, double** glob) {
  ARG_CHECK(e && host_cfg && dev_cfg && tbl && glob);
  *host_cfg = &e->cfg; *dev_cfg = e->d_cfg; *tbl = &e->tbl; *glob = e->d_glob;
  return PBHC_OK;
}

// config without the members k_env_step reads from the run-time copy even when specialised (pointers, env count, seed, reference yaw)
static void strip_runtime_members(PbhcEnvConfig* c) {
  c->num_envs = 0; c->seed = 0; c->ref_init_yaw = 0.0f; c->map_image = nullptr;
  for (int g = 0; g < PBHC_MAX_GROUPS; ++g) { c->groups[g].dst = nullptr; c->groups[g].src = nullptr; c->groups[g].scale = nullptr; c->groups[g].noise = nullptr; }
}

// Attach a config-specialised build of k_env_step (csrc/pbhc_env_step_spec.hip compiled with this env's config as constants).  The
// object is accepted only if the config baked into it equals this env's, member by member; afterwards pbhc_env_step launches it
// instead of the generic kernel.  `so_path` = NULL detaches.
int pbhc_env_attach_specialised(PbhcEnv* e, const char* so_path) {
  ARG_CHECK(e);
  if (!so_path) { e->spec_fn = nullptr; return PBHC_OK; }          // (the object stays loaded: another env may share it)
  void* dl = dlopen(so_path, RTLD_NOW | RTLD_LOCAL);
  if (!dl) { snprintf(g_err, sizeof(g_err), "pbhc_env_attach_specialised: dlopen(%s): %s", so_path, dlerror()); return PBHC_EINVAL; }
  typedef int (*fn_i)(void);
  typedef const PbhcEnvConfig* (*fn_c)(void);
  typedef const void* (*fn_k)(void);
  fn_i abi = (fn_i)dlsym(dl, "pbhc_spec_abi_version"), mode = (fn_i)dlsym(dl, "pbhc_spec_mode");
  fn_c cfgf = (fn_c)dlsym(dl, "pbhc_spec_config");
  fn_k kern = (fn_k)dlsym(dl, "pbhc_spec_kernel");
  fn_i lds_stride = (fn_i)dlsym(dl, "pbhc_spec_lds_stride"), lds_bytes = (fn_i)dlsym(dl, "pbhc_spec_lds_bytes"), hist_wide = (fn_i)dlsym(dl, "pbhc_spec_hist_wide");
  if (!abi || !mode || !cfgf || !kern || !lds_stride || !lds_bytes || !hist_wide || abi() != PBHC_ABI_VERSION) {
    dlclose(dl);
    snprintf(g_err, sizeof(g_err), "pbhc_env_attach_specialised: %s is not a specialised step kernel of this ABI version", so_path);
    return PBHC_EINVAL;
  }
  PbhcEnvConfig* a = new (std::nothrow) PbhcEnvConfig;
  PbhcEnvConfig* b = new (std::nothrow) PbhcEnvConfig;
  if (!a || !b) { delete a; delete b; dlclose(dl); return PBHC_ENOMEM; }
  memcpy(a, cfgf(), sizeof(PbhcEnvConfig));
  memcpy(b, &e->cfg, sizeof(PbhcEnvConfig));
  strip_runtime_members(a); strip_runtime_members(b);
  const bool same = mode() == e->cfg.tracking_mode && memcmp(a, b, sizeof(PbhcEnvConfig)) == 0;
  delete a; delete b;
  if (!same) {
    dlclose(dl);
    snprintf(g_err, sizeof(g_err), "pbhc_env_attach_specialised: %s was built from a different config", so_path);
    return PBHC_EINVAL;
  }
  const void* fn = kern();
  e->spec_lds_stride = lds_stride();
  e->spec_lds_bytes = (size_t)lds_bytes();
  e->spec_hist_wide = hist_wide();
  if (e->spec_lds_bytes > 64 * 1024) HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)e->spec_lds_bytes));
  e->spec_fn = fn;
  e->spec_dl = dl;
  return PBHC_OK;
}
int pbhc_env_is_specialised(PbhcEnv* e) { return e && e->spec_fn ? 1 : 0; }

void pbhc_env_destroy(PbhcEnv* e) {
  if (!e) return;
  if (e->profile)
    for (int i = 0; i < PBHC_PROFILE_RING; ++i) { (void)hipEventDestroy(e->ev0[i]); (void)hipEventDestroy(e->ev1[i]); }
  (void)hipFree(e->d_cfg);
  (void)hipFree(e->d_partials);
  (void)hipFree(e->d_skc);
  (void)hipFree(e->d_skj);
  delete e;
}

int pbhc_env_profile(PbhcEnv* e, int enable) {
  ARG_CHECK(e);
  if (enable && !e->profile) {
    for (int i = 0; i < PBHC_PROFILE_RING; ++i) { HIP_CHECK(hipEventCreate(&e->ev0[i])); HIP_CHECK(hipEventCreate(&e->ev1[i])); }
    e->profile = 1;
  }
  if (!enable && e->profile) {
    for (int i = 0; i < PBHC_PROFILE_RING; ++i) { (void)hipEventDestroy(e->ev0[i]); (void)hipEventDestroy(e->ev1[i]); }
    e->profile = 0;
  }
  e->prof_count = 0;
  return PBHC_OK;
}

// One wave that spins for `ticks` of the 100 MHz wall clock: a kernel of KNOWN duration, to calibrate the dispatch-attached event pair
__global__ void k_profile_spin(long long ticks, long long* sink) {
  const long long t0 = wall_clock64();
  long long t = t0;
  while (t - t0 < ticks) t = wall_clock64();          // bounded: the wall clock always advances
  if (sink && threadIdx.x == 0) *sink = t - t0;
}
int pbhc_env_profile_overhead(PbhcEnv* e, void* stream, float* overhead_ms) {
  ARG_CHECK(e && overhead_ms && e->profile);
  hipStream_t st = (hipStream_t)stream;
  hipEvent_t a, b;
  HIP_CHECK(hipEventCreate(&a));
  HIP_CHECK(hipEventCreate(&b));
  float v[33];
  const long long ticks = 2000;                             // 20 us
  for (int i = 0; i < 33; ++i) {
    hipExtLaunchKernelGGL(k_profile_spin, dim3(1), dim3(64), 0, st, a, b, 0, ticks, (long long*)nullptr);
    HIP_CHECK(hipEventSynchronize(b));
    HIP_CHECK(hipEventElapsedTime(&v[i], a, b));
  }
  (void)hipEventDestroy(a); (void)hipEventDestroy(b);
  for (int i = 1; i < 33; ++i) { float x = v[i]; int j = i - 1; while (j >= 0 && v[j] > x) { v[j + 1] = v[j]; --j; } v[j + 1] = x; }
  *overhead_ms = v[16] - 0.020f;                            // median reading minus the spin's own 20 us
  return PBHC_OK;
}
int pbhc_env_profile_read(PbhcEnv* e, float* ms_out, int max_count, int* count) {
  ARG_CHECK(e && ms_out && count && e->profile);
  int n = e->prof_count < PBHC_PROFILE_RING ? e->prof_count : PBHC_PROFILE_RING;
  if (n > max_count) n = max_count;
  for (int i = 0; i < n; ++i) {
    int slot = (e->prof_count - n + i) % PBHC_PROFILE_RING;
    HIP_CHECK(hipEventSynchronize(e->ev1[slot]));
    HIP_CHECK(hipEventElapsedTime(&ms_out[i], e->ev0[slot], e->ev1[slot]));
  }
  *count = n;
  return PBHC_OK;
}

static int env_step_check(PbhcEnv* e, const PbhcStepIO* io) {
  ARG_CHECK(e && io);
  ARG_CHECK(io->actions_in && io->frame_root && io->frame_dof_pos && io->frame_dof_vel && io->frame_contact && io->frame_cursor && io->num_frames >= 1);
  ARG_CHECK(io->root_states && io->dof_state && io->actions && io->last_actions && io->actions_after_delay && io->action_queue);
  ARG_CHECK(io->last_dof_pos && io->last_dof_vel && io->torques && io->feet_air_time && io->contacts && io->contacts_filt);
  ARG_CHECK(io->last_contacts && io->last_contacts_filt && io->kp_scale && io->kd_scale && io->rfi_lim_scale && io->rao_scale);
  ARG_CHECK(io->motion_start_times && io->motion_len && io->end_time_ratio_buf && io->episode_sums && io->hist);
  ARG_CHECK(io->episode_length_buf && io->last_episode_length_buf && io->reset_buf && io->action_delay_idx && io->motion_ids && io->time_out_buf);
  ARG_CHECK(io->env_origins && io->dr_base_com && io->dr_link_mass && io->dr_friction && io->rew_buf);
  for (int g = 0; g < e->cfg.num_groups; ++g) {
    ARG_CHECK(io->obs[g] != nullptr && (io->obs_pitch[g] == 0 || io->obs_pitch[g] >= e->cfg.groups[g].pitch));
    ARG_CHECK((uint64_t)e->cfg.num_envs * (uint64_t)(io->obs_pitch[g] ? io->obs_pitch[g] : e->cfg.groups[g].pitch) < (1ull << 30));   // 32-bit row offsets in the kernel
  }
  ARG_CHECK(io->hist_pitch == 0 || io->hist_pitch >= e->cfg.hist_dim);
  ARG_CHECK(!e->cfg.noise_process || io->ou_state);
  // the 64-bit counters and indices are read and written as one 8-byte element (every other buffer of the step needs 4-byte alignment only;
  // the history rows of a specialised kernel: pbhc_env_step_launch)
  if ((((uintptr_t)io->episode_length_buf | (uintptr_t)io->last_episode_length_buf | (uintptr_t)io->reset_buf | (uintptr_t)io->action_delay_idx |
        (uintptr_t)io->motion_ids | (uintptr_t)io->ovr_delay) & 7) != 0) {
    snprintf(g_err, sizeof(g_err), "pbhc_env_step: the int64 buffers (episode_length_buf, last_episode_length_buf, reset_buf, action_delay_idx, motion_ids, "
                                   "ovr_delay) must be 8-byte aligned");
    return PBHC_EINVAL;
  }
  ARG_CHECK(((uintptr_t)io->totals_out & 7) == 0);                        // doubles (written by the step's second half)
  return PBHC_OK;
}

// first half of a step: the fused launch (per-env work + per-workgroup partial sums)
int pbhc_env_step_launch(PbhcEnv* e, const PbhcStepIO* io, void* stream) {
  const int rc = env_step_check(e, io);
  if (rc != PBHC_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int slot = e->prof_count % PBHC_PROFILE_RING;
  // profiling: the event pair is attached to the dispatch itself (hipExtLaunchKernelGGL: start / stop taken from the kernel's own
  // begin / end timestamps), so the reading is the kernel's execution time, without the dispatch gap a hipEventRecord pair would add
  hipEvent_t pe0 = e->profile ? e->ev0[slot] : nullptr, pe1 = e->profile ? e->ev1[slot] : nullptr;
  // (profiling off: the plain launch calls — what a stream capture of the whole rollout records; the dispatch-attached event pair of the
  // hipExt forms exists for bench.py's per-launch timing only)
  const PbhcEnvConfig* a_cfg = e->d_cfg;
  const double* a_glob = e->d_glob;
  const float* a_skc = e->d_skc;
  const uint32_t* a_map = e->cfg.map_image;
  const float* a_skj = e->d_skj;
  if (e->spec_fn && e->spec_hist_wide) {
    const int hp = io->hist_pitch ? io->hist_pitch : e->cfg.hist_dim;
    if (((uintptr_t)io->hist & 15) != 0 || (hp & 3) != 0 || hp < ((e->cfg.hist_dim + 3) & ~3)) {
      snprintf(g_err, sizeof(g_err), "pbhc_env_step: the specialised kernel reads history rows 16 bytes per lane: io.hist must be 16-byte aligned with a pitch that is a "
                                     "multiple of 4 floats >= hist_dim rounded up to 4 (pad the rows, or detach the specialised kernel)");
      return PBHC_EINVAL;
    }
  }
  int a_stride = e->spec_fn ? e->spec_lds_stride : e->lds_stride;
  const size_t a_lds = e->spec_fn ? e->spec_lds_bytes : e->lds_bytes;
  const long long* a_ep = (const long long*)io->episode_length_buf;
  const float* a_st = io->motion_start_times;
  const float *a_fr = io->frame_root, *a_fq = io->frame_dof_pos, *a_fqd = io->frame_dof_vel;
  const int32_t* a_cur = io->frame_cursor;
  int a_fi = io->frame_index, a_n = e->cfg.num_envs;
  void* args[] = {(void*)&a_ep, (void*)&a_st, (void*)&a_fr, (void*)&a_fq, (void*)&a_fqd, (void*)&a_cur, (void*)&a_fi, (void*)&a_n, (void*)&a_cfg, (void*)&e->tbl, (void*)io, (void*)&a_glob, (void*)&e->d_partials, (void*)&a_stride, (void*)&a_skc, (void*)&a_map, (void*)&a_skj};
  const void* fn = e->spec_fn ? e->spec_fn : (e->cfg.tracking_mode ? (const void*)k_env_step<1> : (const void*)k_env_step<0>);
  if (e->cfg.terminate_when_dof_far)          // the batch-global dof-far decision, ahead of the step's reset path (k_dof_far_any)
    hipLaunchKernelGGL(k_dof_far_any, dim3((a_n + DOF_FAR_EPB - 1) / DOF_FAR_EPB), dim3(PBHC_G * DOF_FAR_EPB), 0, st, a_ep, a_st, a_fq, a_cur, a_fi,
                       io->num_frames, a_n, e->cfg.skel.num_dof, e->cfg.dt, e->tbl, (const int64_t*)io->motion_ids, e->d_glob);
  if (e->profile) HIP_CHECK(hipExtLaunchKernel(fn, dim3(e->nblocks), dim3(PBHC_TPB), args, a_lds, st, pe0, pe1, 0));
  else HIP_CHECK(hipLaunchKernel(fn, dim3(e->nblocks), dim3(PBHC_TPB), args, a_lds, st));
  if (e->profile) e->prof_count++;
  e->step_ctr++;
  HIP_CHECK(hipGetLastError());
  return PBHC_OK;
}

// second half: the one-workgroup reduction of the partial sums into the globals (adaptive sigma, curricula, log means, step counter) — or,
// with io->totals_out, into this shard's totals for the ranks' exchange.  `stream` may differ from the launch's: the caller orders it
// after the fused launch and before the next one (the rollout runs it next to the policy forward, off the step -> policy -> step chain).
int pbhc_env_step_finish(PbhcEnv* e, const PbhcStepIO* io, void* stream) {
  ARG_CHECK(e && io && io->frame_cursor && io->num_frames >= 1);
  ARG_CHECK(((uintptr_t)io->totals_out & 7) == 0);                        // doubles
  hipLaunchKernelGGL(k_env_finalize, dim3(1), dim3(64 * PBHC_FIN_CHUNKS), 0, (hipStream_t)stream, e->d_cfg, e->d_glob, e->d_partials, 2 * e->nblocks, io->frame_cursor,
                     io->num_frames, (const double*)nullptr, io->totals_out, 0.0);
  HIP_CHECK(hipGetLastError());
  return PBHC_OK;
}

// the same reduction (single-process form only) as a descriptor instead of a launch: the caller hands it to a launch of its own that follows
// the fused launch on its stream (pbhc_mlp_fwd_*_riders: one more workgroup of the rollout's policy forward).  Nothing is launched here.
int pbhc_env_finalize_rider(PbhcEnv* e, const PbhcStepIO* io, PbhcRider* r) {
  ARG_CHECK(e && io && r && io->frame_cursor && io->num_frames >= 1);
  ARG_CHECK(io->totals_out == nullptr);              // (the data-parallel halves exchange their sums between two launches)
  r->cfg = e->d_cfg; r->globals = e->d_glob; r->partials = e->d_partials; r->frame_cursor = io->frame_cursor;
  r->num_partial_rows = 2 * e->nblocks; r->num_frames = io->num_frames;
  r->has_finalize = 1;
  return PBHC_OK;
}

// test aid: k_env_finalize (single-process form) on a rider's finalize half, i.e. on partial rows, globals and a cursor of the caller's choice
int pbhc_debug_env_finalize(const PbhcRider* r, void* stream) {
  ARG_CHECK(r && r->has_finalize && r->cfg && r->globals && r->partials && r->frame_cursor && r->num_partial_rows >= 1 && r->num_frames >= 1);
  hipLaunchKernelGGL(k_env_finalize, dim3(1), dim3(64 * PBHC_FIN_CHUNKS), 0, (hipStream_t)stream, r->cfg, r->globals, r->partials, r->num_partial_rows, r->frame_cursor,
                     r->num_frames, (const double*)nullptr, (double*)nullptr, 0.0);
  HIP_CHECK(hipGetLastError());
  return PBHC_OK;
}

// the evaluation recorder's frame of the step just launched on `stream` (k_record_motion)
int pbhc_record_motion(PbhcEnv* e, const PbhcStepIO* io, const PbhcRecordIO* rec, void* stream) {
  ARG_CHECK(e && io && rec);
  ARG_CHECK(e->cfg.tracking_mode == 0);            // the reference's general-tracking env has no recorder
  ARG_CHECK(rec->total_steps >= 1 && rec->obs_group >= 0 && rec->obs_group < e->cfg.num_groups && rec->counter);
  ARG_CHECK(rec->root_trans_offset && rec->root_rot && rec->root_lin_vel && rec->root_ang_vel && rec->dof && rec->dof_vel && rec->contact_mask);
  ARG_CHECK(rec->pose_aa && rec->action && rec->actor_obs && rec->terminate && rec->motion_times);
  ARG_CHECK(io->root_states && io->dof_state && io->actions && io->contacts_filt && io->env_origins && io->motion_start_times);
  ARG_CHECK(io->episode_length_buf && io->reset_buf && io->obs[rec->obs_group]);
  ARG_CHECK(((((uintptr_t)rec->terminate | (uintptr_t)io->episode_length_buf | (uintptr_t)io->reset_buf) & 7) == 0));    // int64 elements
  const int g = rec->obs_group, N = e->cfg.num_envs;
  RecSrc s;
  s.root = io->root_states; s.dof_state = io->dof_state; s.actions = io->actions; s.contacts_filt = io->contacts_filt;
  s.origins = io->env_origins; s.start = io->motion_start_times; s.obs = io->obs[g];
  s.ep_len = (const long long*)io->episode_length_buf; s.reset = (const long long*)io->reset_buf;
  s.obs_dim = e->cfg.groups[g].dim;
  s.obs_pitch = io->obs_pitch[g] ? io->obs_pitch[g] : e->cfg.groups[g].pitch;
  ARG_CHECK((uint64_t)N * (uint64_t)(s.obs_dim + 3 * e->cfg.skel.num_bodies_ext + 3 * e->cfg.skel.num_dof + 16) < (1ull << 31) - REC_TPB * REC_ITEMS);   // 32-bit item index
  const size_t items = (size_t)N * (size_t)(s.obs_dim + 3 * e->cfg.skel.num_bodies_ext + 3 * e->cfg.skel.num_dof + 16);
  const size_t per_block = (size_t)REC_TPB * REC_ITEMS;
  hipLaunchKernelGGL(k_record_motion, dim3((unsigned)((items + per_block - 1) / per_block)), dim3(REC_TPB), 0, (hipStream_t)stream, s, *rec, (const PbhcEnvConfig*)e->d_cfg, N,
                     e->cfg.skel.num_dof, e->cfg.skel.num_bodies_ext, e->cfg.dt);
  HIP_CHECK(hipGetLastError());
  return PBHC_OK;
}

int pbhc_env_step(PbhcEnv* e, const PbhcStepIO* io, void* stream) {
  const int rc = pbhc_env_step_launch(e, io, stream);
  return rc != PBHC_OK ? rc : pbhc_env_step_finish(e, io, stream);
}

int pbhc_env_finalize(PbhcEnv* e, const double* totals, double num_envs_total, void* stream) {
  ARG_CHECK(e && totals && num_envs_total >= 1.0);
  ARG_CHECK(((uintptr_t)totals & 7) == 0);                                // doubles
  hipLaunchKernelGGL(k_env_finalize, dim3(1), dim3(64 * PBHC_FIN_CHUNKS), 0, (hipStream_t)stream, e->d_cfg, e->d_glob, (const float*)nullptr, 0, (int32_t*)nullptr, 1,
                     totals, (double*)nullptr, num_envs_total);
  HIP_CHECK(hipGetLastError());
  return PBHC_OK;
}

int pbhc_gae(const float* rewards, const float* values, const uint8_t* dones, const float* last_values, int T, int N, int R, float gamma,
             float lam, float* returns, float* advantages, double* stats, void* stream) {
  ARG_CHECK(rewards && values && dones && last_values && returns && advantages && stats && T >= 1 && N >= 1 && R >= 1);
  hipStream_t st = (hipStream_t)stream;
  size_t NR = (size_t)N * R, TN = (size_t)T * N;
  int nb = (int)((TN + GAE_TPB - 1) / GAE_TPB);
  hipLaunchKernelGGL(k_gae, dim3((unsigned)((NR + GAE_TPB - 1) / GAE_TPB)), dim3(GAE_TPB), 0, st, rewards, values, dones, last_values, T, N, R, gamma, lam, returns);
  hipLaunchKernelGGL(k_adv_sum, dim3(nb), dim3(GAE_TPB), 0, st, returns, values, TN, R, advantages, stats);
  hipLaunchKernelGGL(k_adv_norm, dim3(nb), dim3(GAE_TPB), 0, st, advantages, TN, stats, nb);
  HIP_CHECK(hipGetLastError());
  return PBHC_OK;
}

}  // extern "C"
