// pbhc_rollout_post.h — the rollout's done / episode-statistics book-keeping of one control step (mh_ppo.py:300-323) as a device function:
// k_rollout_post (pbhc_ppo.hip) runs it with 8 envs per 256-thread workgroup, the rider workgroups of the rollout's policy launch
// (k_mlp_fwd, pbhc_mlp.hip) with 16 envs per 512-thread workgroup.  32 lanes per env; the per-env arithmetic is the same in both.
// Expects <hip/hip_runtime.h> before it.
#pragma once
#include <stdint.h>

__device__ __forceinline__ float gsum32(float v) {
#pragma unroll
  for (int m = 16; m >= 1; m >>= 1) v += __shfl_xor(v, m, 32);
  return v;
}

// ROWS: envs per workgroup (blockDim.x == 32 * ROWS); block: the workgroup's index among those that run this body; sh: 3 * ROWS doubles of LDS
template <int ROWS>
__device__ __forceinline__ void rollout_post_body(double* __restrict__ sh, int block, const float* __restrict__ rew, const float* __restrict__ values,
                                                  const int64_t* __restrict__ reset_buf, const uint8_t* __restrict__ time_outs, int N, int R, float gamma,
                                                  float* __restrict__ rewards_out, uint8_t* __restrict__ dones_out, float* __restrict__ cur_rew,
                                                  float* __restrict__ cur_len, double* __restrict__ ep_stats, uint8_t* __restrict__ time_outs_out) {
  const int lane = threadIdx.x & 31, lr = threadIdx.x >> 5, row = block * ROWS + lr;
  const bool valid = row < N;
  float r = 0.0f;
  const float to = valid ? (time_outs[row] ? 1.0f : 0.0f) : 0.0f;
  if (valid && lane < R) {
    const size_t i = (size_t)row * R + lane;
    r = rew[i];
    rewards_out[i] = values ? r + gamma * values[i] * to : r;      // values == NULL: the caller adds the time-out bootstrap later (batched critic)
  }
  const float rsum = gsum32(r);
  double a = 0.0, b = 0.0, c = 0.0;
  if (valid && lane == 0) {
    const bool done = reset_buf[row] > 0;
    dones_out[row] = done ? 1 : 0;
    if (time_outs_out) time_outs_out[row] = time_outs[row];
    const float cr = cur_rew[row] + rsum, cl = cur_len[row] + 1.0f;
    if (done) { a = (double)cr; b = (double)cl; c = 1.0; }
    cur_rew[row] = done ? 0.0f : cr;
    cur_len[row] = done ? 0.0f : cl;
  }
  if (lane == 0) { sh[lr] = a; sh[ROWS + lr] = b; sh[2 * ROWS + lr] = c; }
  __syncthreads();
  if (threadIdx.x < 3) {
    double t = 0.0;
    for (int k = 0; k < ROWS; ++k) t += sh[threadIdx.x * ROWS + k];
    if (t != 0.0) atomicAdd(&ep_stats[threadIdx.x], t);        // logging statistics only
  }
}
