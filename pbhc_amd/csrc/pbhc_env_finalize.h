// pbhc_env_finalize.h — the env step's one-workgroup reduction (the scalars the reference updates on the host each step) as a device
// function, so that it can run as k_env_finalize (pbhc_kernels.hip, 1024 threads) or as one more workgroup of a launch that is on the
// rollout's step -> policy -> step chain anyway (k_mlp_fwd's rider workgroup, pbhc_mlp.hip, 512 threads).  Both callers add the partial rows
// up in the SAME order and run the same scalar chains: the globals they leave are equal bit for bit (tests/test_gpu_rollout_riders.py).
// Expects <hip/hip_runtime.h> and include/pbhc_hip.h before it.
#pragma once

#include "pbhc_partials.h"

#define PBHC_FIN_CHUNKS 16
#define PBHC_FIN_LDS_DOUBLES (PBHC_FIN_CHUNKS * 64 + PBHC_NP)      // acc [PBHC_FIN_CHUNKS][64] + tot [PBHC_NP]

// NT: threads of the calling workgroup, a multiple of 64 that divides 64 * PBHC_FIN_CHUNKS and is > 320 (the scalar chains' lanes); every
// thread of the workgroup calls it.  acc: PBHC_FIN_CHUNKS * 64 doubles of LDS, tot: PBHC_NP doubles of LDS.
// three uses: (partials) reduce + apply [single process]; (partials, tot_out) reduce only, sums to tot_out [data-parallel, first half];
// (ext_tot) apply sums that the caller has added up over ranks [second half]
template <int NT>
__device__ __forceinline__ void env_finalize_body(double* __restrict__ acc, double* __restrict__ tot, const PbhcEnvConfig* __restrict__ cfgp, double* __restrict__ glob,
                                                  const float* __restrict__ partials, int nblocks, int32_t* frame_cursor, int num_frames,
                                                  const double* __restrict__ ext_tot, double* __restrict__ tot_out, double n_total) {
  static_assert(NT % 64 == 0 && (64 * PBHC_FIN_CHUNKS) % NT == 0 && NT > 320, "workgroup size");
  const PbhcEnvConfig& c = *cfgp;
  const int k = threadIdx.x & 63;
  // column sums of the workgroup partials in a FIXED order (chunk-strided, then chunk order): deterministic.  Chunk c adds rows c, c + 16,
  // c + 32, ... one after the other into one double; how many of its loads are in flight does not change that order.  A wave owns CPW chunks
  // (wave, wave + NT / 64): their loads go out together — a 512-thread caller has 2 x FIN_U loads in flight per lane and makes as few
  // round trips to memory as 1024 threads with 8 each (two chunks one after the other doubled the rider's time next to the policy stack)
  constexpr int CPW = 64 * PBHC_FIN_CHUNKS / NT, HOP = NT / 64, FIN_U = CPW == 1 ? 8 : 16;
  const int wave = threadIdx.x >> 6;
  double s[CPW];
#pragma unroll
  for (int q = 0; q < CPW; ++q) s[q] = 0.0;
  if (k < PBHC_NP && !ext_tot) {
    int b = wave;
    if (CPW > 1) {
      for (; b + (CPW - 1) * HOP + (FIN_U - 1) * PBHC_FIN_CHUNKS < nblocks; b += FIN_U * PBHC_FIN_CHUNKS) {
        float v[CPW][FIN_U];
#pragma unroll
        for (int q = 0; q < CPW; ++q)
#pragma unroll
          for (int u = 0; u < FIN_U; ++u) v[q][u] = partials[(size_t)(b + q * HOP + u * PBHC_FIN_CHUNKS) * PBHC_NP + k];
#pragma unroll
        for (int q = 0; q < CPW; ++q)
#pragma unroll
          for (int u = 0; u < FIN_U; ++u) s[q] += (double)v[q][u];
      }
    }
#pragma unroll
    for (int q = 0; q < CPW; ++q) {
      int bq = b + q * HOP;
      for (; bq + 7 * PBHC_FIN_CHUNKS < nblocks; bq += 8 * PBHC_FIN_CHUNKS) {       // 8 independent loads in flight, summed in the same fixed order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = partials[(size_t)(bq + u * PBHC_FIN_CHUNKS) * PBHC_NP + k];
#pragma unroll
        for (int u = 0; u < 8; ++u) s[q] += (double)v[u];
      }
      for (; bq < nblocks; bq += PBHC_FIN_CHUNKS) s[q] += (double)partials[(size_t)bq * PBHC_NP + k];
    }
  }
#pragma unroll
  for (int q = 0; q < CPW; ++q) acc[(wave + q * HOP) * 64 + k] = s[q];
  __syncthreads();
  if (threadIdx.x < PBHC_NP) {
    double t = 0.0;
    for (int ch = 0; ch < PBHC_FIN_CHUNKS; ++ch) t += acc[ch * 64 + threadIdx.x];
    if (ext_tot) t = ext_tot[threadIdx.x];
    tot[threadIdx.x] = t;
    if (tot_out) tot_out[threadIdx.x] = t;
  }
  __syncthreads();
  // the scalar updates are independent chains of dependent global loads / double divisions: one lane (of different waves) per chain
  const double N = ext_tot ? n_total : (double)c.num_envs;
  const int tid = threadIdx.x;
  if (tot_out) {                                     // reduce-only half: the per-launch counters still advance here
    if (tid == 64) {
      if (c.terminate_when_dof_far) glob[PBHC_G_DOF_FAR_HIT] = 0.0;
      glob[PBHC_G_STEP_COUNTER] += 1.0;
      frame_cursor[0] = (frame_cursor[0] + 1) % num_frames;
    }
    return;
  }
  // adaptive sigma (motion_tracking.py:1030-1048, general_tracking.py:972-996): lane i of wave 0 owns term i
  if (tid < PBHC_NUM_SIGMA) {
    const int i = tid;
    if (c.adaptive_sigma && c.sigma_active[i]) {
      double mean = (double)(float)(tot[P_ERR + i] / N);
      double ema = glob[PBHC_G_EMA + i] * (1.0 - (double)c.adaptive_alpha) + mean * (double)c.adaptive_alpha;
      glob[PBHC_G_EMA + i] = ema;
      const double sg = glob[PBHC_G_SIGMA + i];
      double nsg;
      switch (c.adaptive_type) {
        case 1: nsg = (fmin(ema, sg) + ema) / 2.0; break;
        case 2: nsg = fmin(ema * (double)c.adaptive_scale, sg); break;
        case 3: nsg = ema; break;
        default: nsg = fmin(ema, sg);
      }
      glob[PBHC_G_SIGMA + i] = nsg;
    }
    return;
  }
  double* L = glob + PBHC_G_LOG;
  const double nreset = tot[P_RESET_CNT];
  const double rfrac = nreset / N;
  if (tid == 64) {
    L[PBHC_L_UPPER_BODY_DIFF_NORM] = tot[P_UPPER_NORM] / N; L[PBHC_L_LOWER_BODY_DIFF_NORM] = tot[P_LOWER_NORM] / N;
    L[PBHC_L_VR_3POINT_DIFF_NORM] = tot[P_VR_NORM] / N; L[PBHC_L_JOINT_POS_DIFF_NORM] = tot[P_JOINT_NORM] / N;
    L[PBHC_L_ACTION_CLIP_FRAC] = tot[P_CLIP_CNT] / (N * (double)c.skel.num_dof);
    L[PBHC_L_RESET_FRAC] = rfrac; L[PBHC_L_NUM_RESETS] = nreset;
    L[PBHC_L_REW_MEAN] = tot[P_REW_SUM] / N;
    if (!ext_tot) {
      glob[PBHC_G_STEP_COUNTER] += 1.0;
      frame_cursor[0] = (frame_cursor[0] + 1) % num_frames;
    }
  } else if (tid == 128) {
    L[PBHC_L_TERM_GRAVITY] = (tot[P_TERM_GRAVITY] / N) / (rfrac + 1e-15); L[PBHC_L_TERM_MOTION_FAR] = (tot[P_TERM_FAR] / N) / (rfrac + 1e-15);
    L[PBHC_L_TERM_TIME_OUT] = (tot[P_TERM_TIMEOUT] / N) / (rfrac + 1e-15); L[PBHC_L_TERM_MOTION_END] = (tot[P_TERM_END] / N) / (rfrac + 1e-15);
    L[PBHC_L_TERM_CONTACT] = (tot[P_TERM_CONTACT] / N) / (rfrac + 1e-15); L[PBHC_L_TERM_LOW_HEIGHT] = (tot[P_TERM_LOWH] / N) / (rfrac + 1e-15);
    L[PBHC_L_TERM_DOF_POS_LIMIT] = (tot[P_TERM_POSLIM] / N) / (rfrac + 1e-15); L[PBHC_L_TERM_DOF_VEL_LIMIT] = (tot[P_TERM_VELLIM] / N) / (rfrac + 1e-15);
    L[PBHC_L_TERM_TORQUE_LIMIT] = (tot[P_TERM_TAULIM] / N) / (rfrac + 1e-15);
    if (c.terminate_when_dof_far) {     // motion_tracking.py:346: a scalar flag, its env-mean is the flag itself; cleared for the next pre-pass
      L[PBHC_L_TERM_DOF_FAR] = glob[PBHC_G_DOF_FAR_HIT] / (rfrac + 1e-15);
      glob[PBHC_G_DOF_FAR_HIT] = 0.0;
    }
    if (c.tracking_mode) {
      L[PBHC_L_TERM_REF_POS_Z] = (tot[P_TERM_REFZ] / N) / (rfrac + 1e-15); L[PBHC_L_TERM_REF_ORI] = (tot[P_TERM_REFORI] / N) / (rfrac + 1e-15);
      L[PBHC_L_TERM_BODY_Z] = (tot[P_TERM_BODYZ] / N) / (rfrac + 1e-15);
    }
  } else if (tid == 192) {
    if (c.tracking_mode) {
      L[PBHC_L_KEY_BODY_DIFF_NORM] = tot[P_KEY_NORM] / N; L[PBHC_L_LOCAL_UPPER_BODY_DIFF_NORM] = tot[P_LUP_NORM] / N;
      L[PBHC_L_LOCAL_LOWER_BODY_DIFF_NORM] = tot[P_LLO_NORM] / N; L[PBHC_L_LOCAL_VR_3POINT_DIFF_NORM] = tot[P_LVR_NORM] / N;
      L[PBHC_L_LOCAL_KEY_BODY_DIFF_NORM] = tot[P_LKEY_NORM] / N;
    }
  } else if (tid == 256) {
    // the threshold this step's termination test used (logged by _update_reset_buf before the curriculum below moves it)
    if (c.terminate_when_dof_far) L[PBHC_L_DOF_FAR_THR] = glob[PBHC_G_DOF_FAR_THR];
    if (nreset > 0.0) {
    // _update_average_episode_length (legged_robot_base.py:875-879), fp32 like the reference's 0-dim tensor
    float cur = (float)(tot[P_RESET_EPLEN] / nreset);
    double frac = nreset / (double)c.num_compute_average_epl;
    float avg = (float)glob[PBHC_G_AVG_EP_LEN] * (float)(1.0 - frac) + cur * (float)frac;
    glob[PBHC_G_AVG_EP_LEN] = (double)avg;
    if (c.penalty_curriculum) {           // legged_robot_base.py:882-900
      double p = glob[PBHC_G_PENALTY_SCALE];
      if (avg < c.penalty_down) p *= (1.0 - (double)c.penalty_degree);
      else if (avg > c.penalty_up) p *= (1.0 + (double)c.penalty_degree);
      glob[PBHC_G_PENALTY_SCALE] = fmin(fmax(p, (double)c.penalty_min), (double)c.penalty_max);
    }
    {                                     // _update_reward_limits_curriculum, legged_robot_base.py:902-939 (python floats: double)
      const int on[3] = {c.soft_pos_curriculum, c.soft_vel_curriculum, c.soft_tau_curriculum};
      const int slot[3] = {PBHC_G_SOFT_POS_VAL, PBHC_G_SOFT_VEL_VAL, PBHC_G_SOFT_TAU_VAL};
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        if (!on[q]) continue;
        double v = glob[slot[q]];
        if (avg < c.soft_cur_down[q]) v *= (1.0 + (double)c.soft_cur_degree[q]);
        else if (avg > c.soft_cur_up[q]) v *= (1.0 - (double)c.soft_cur_degree[q]);
        glob[slot[q]] = fmin(fmax(v, (double)c.soft_cur_min[q]), (double)c.soft_cur_max[q]);
      }
    }
    if (c.noise_curriculum) {             // _update_obs_noise_curriculum, legged_robot_base.py:1117-1126 (after the penalty / limit curricula)
      double v = glob[PBHC_G_NOISE_CURRICULUM];
      if (avg < c.noise_down) v *= (1.0 - (double)c.noise_degree);
      else if (avg > c.noise_up) v *= (1.0 + (double)c.noise_degree);
      glob[PBHC_G_NOISE_CURRICULUM] = fmin(fmax(v, (double)c.noise_min), (double)c.noise_max);
    }
    if (c.terminate_when_motion_far && c.motion_far_curriculum) {   // motion_tracking.py:309-317
      double t = glob[PBHC_G_MOTION_FAR_THR];
      if (avg < c.motion_far_down) t *= (1.0 + (double)c.motion_far_degree);
      else if (avg > c.motion_far_up) t *= (1.0 - (double)c.motion_far_degree);
      glob[PBHC_G_MOTION_FAR_THR] = fmin(fmax(t, (double)c.motion_far_min), (double)c.motion_far_max);
    }
    if (c.terminate_when_dof_far && c.dof_far_curriculum) {         // motion_tracking.py:283-292, the same call site
      double t = glob[PBHC_G_DOF_FAR_THR];
      if (avg < c.dof_far_down) t *= (1.0 + (double)c.dof_far_degree);
      else if (avg > c.dof_far_up) t *= (1.0 - (double)c.dof_far_degree);
      glob[PBHC_G_DOF_FAR_THR] = fmin(fmax(t, (double)c.dof_far_min), (double)c.dof_far_max);
    }
    }
  } else if (tid == 320 && nreset > 0.0) {
    double mean = tot[P_ETR_SUM] / N;
    L[PBHC_L_END_TIME_RATIO] = mean;
    double var = (tot[P_ETR_SQ] - N * mean * mean) / (N - 1.0);
    L[PBHC_L_END_TIME_RATIO_STD] = var > 0.0 ? sqrt(var) : 0.0;
  }
}
