// pbhc_clip_stats.hip — per-clip episode statistics and failure-weighted clip sampling, all on the device.
//
//   k_clip_stats            one launch per control step, right after the fused step: every env that reset adds its finished episode to row
//                           slot_clip[env] of `window [M,4]` int64 = (episodes, failures, sum of end_time_ratio * 2^24, sum of lengths).
//   k_clip_sampling_update  once per resample: folds the window into the reference's four hook tensors (_sampling_history,
//                           _termination_history, _success_rate, _sampling_prob; motion_lib_base.py:109-118), writes the CDF, clears the window.
//   k_clip_sample_slots     slot -> clip multinomial draw with replacement from that CDF, keyed by Philox stream 20.
//
// Every column of the window is an integer ON PURPOSE: integer atomic sums do not depend on the order in which the adds arrive, so the
// table is bit-reproducible and a captured rollout graph gives exactly the table of the eager loop.  The end_time_ratio goes in as the
// fixed-point value llrintf(ratio * 2^24): a float32 in [0.5, 2) is a multiple of 2^-24 (2^-23 from 1 on), so nothing is lost there; below
// 0.5 the rounding loses at most 2^-25 per episode.  (A non-finite ratio adds 0.)
//
// The step kernel and its config-specialised builds do not know these kernels exist (as with the evaluation recorder): they read what a
// step left in the env's buffers.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "../../include/pbhc_hip.h"
#include "pbhc_math.h"

using namespace pbhc;

extern thread_local char g_pbhc_err[512];

#define CLIP_THREADS 256

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

#define STATS_THREADS 1024
#define STATS_WAVES (STATS_THREADS / 64)

// reset_all() and a collapsing policy reset every env in one step; with one clip that is N adds onto one row, and same-row atomics run one
// after the other (about 12 ns each, profiles/clip_sampling.txt).  So the adds are combined first: a wave whose resetting lanes share a clip
// sums inside the wave, and a workgroup whose waves share that clip sums those once more through LDS and adds once per column.  A wave with
// several clips falls back to per-lane 64-bit integer atomics, a workgroup with several clips to one set per wave (all still
// order-independent).  A slot_clip outside [0, M) is skipped, never used as an index.
__global__ __launch_bounds__(STATS_THREADS) void k_clip_stats(const int64_t* __restrict__ reset_buf, const uint8_t* __restrict__ time_out_buf,
                                                              const float* __restrict__ end_time_ratio_buf,
                                                              const int64_t* __restrict__ last_episode_length_buf,
                                                              const int64_t* __restrict__ slot_clip, int N, int M,
                                                              unsigned long long* __restrict__ window) {
  __shared__ long long s_sum[STATS_WAVES][4];
  __shared__ int s_clip[STATS_WAVES];                         // the clip a wave's sums belong to, -1: the wave has nothing to hand over
  const int i = blockIdx.x * STATS_THREADS + threadIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  bool act = false;
  int clip = 0;
  long long fail = 0, ratio = 0, len = 0;
  if (i < N && reset_buf[i] != 0) {
    const int64_t c = slot_clip[i];
    if (c >= 0 && c < (int64_t)M) {
      act = true;
      clip = (int)c;
      fail = time_out_buf[i] == 0 ? 1 : 0;
      const float r = end_time_ratio_buf[i] * 16777216.0f;
      ratio = isfinite(r) ? llrintf(r) : 0;
      len = last_episode_length_buf[i];
    }
  }
  const unsigned long long mask = __ballot(act);
  int wclip = -1;
  long long e = 0, f = 0, r = 0, l = 0;
  if (mask != 0ull) {                                         // wave-uniform
    const int clip0 = __shfl(clip, __ffsll((long long)mask) - 1, 64);
    if (__ballot(act && clip != clip0) == 0ull) {             // wave-uniform: one clip in this wave
      wclip = clip0;
      e = __popcll(mask); f = wave_sum_i64(fail); r = wave_sum_i64(ratio); l = wave_sum_i64(len);
    } else if (act) {
      unsigned long long* row = window + 4 * (size_t)clip;
      atomicAdd(row + 0, 1ull);
      atomicAdd(row + 1, (unsigned long long)fail);
      atomicAdd(row + 2, (unsigned long long)ratio);
      atomicAdd(row + 3, (unsigned long long)len);
    }
  }
  if (lane == 0) {
    s_clip[wave] = wclip;
    s_sum[wave][0] = e; s_sum[wave][1] = f; s_sum[wave][2] = r; s_sum[wave][3] = l;
  }
  __syncthreads();
  if (wave != 0) return;
  // wave 0: lane w holds what wave w handed over
  const bool has = lane < STATS_WAVES && s_clip[lane] >= 0;
  const int c = has ? s_clip[lane] : 0;
  const unsigned long long hmask = __ballot(has);
  if (hmask == 0ull) return;
  const int lead = __ffsll((long long)hmask) - 1;
  const int c0 = __shfl(c, lead, 64);
  if (__ballot(has && c != c0) == 0ull) {                     // one clip in this workgroup
#pragma unroll
    for (int col = 0; col < 4; ++col) {
      const long long v = wave_sum_i64(has ? s_sum[lane][col] : 0ll);
      if (lane == lead) atomicAdd(window + 4 * (size_t)c0 + col, (unsigned long long)v);
    }
  } else if (has) {
#pragma unroll
    for (int col = 0; col < 4; ++col) atomicAdd(window + 4 * (size_t)c + col, (unsigned long long)s_sum[lane][col]);
  }
}

// sum of one double per thread over the workgroup, returned to every thread (red: CLIP_THREADS doubles of LDS)
__device__ double block_sum(double v, double* red) {
  const int t = threadIdx.x;
  __syncthreads();
  red[t] = v;
  __syncthreads();
  for (int s = CLIP_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  return red[0];
}

// cdf[i] = sum_{j <= i} double(p[j]), by one workgroup: every thread owns a contiguous chunk (sum, exclusive scan of the chunk sums, rewrite)
__device__ void block_cdf(const float* p, double* __restrict__ cdf, int M, double* red) {
  const int t = threadIdx.x;
  const int chunk = (M + CLIP_THREADS - 1) / CLIP_THREADS;
  const int a = min(t * chunk, M), b = min(a + chunk, M);
  double s = 0.0;
  for (int i = a; i < b; ++i) s += (double)p[i];
  __syncthreads();
  red[t] = s;
  __syncthreads();
  if (t == 0) {
    double run = 0.0;
    for (int k = 0; k < CLIP_THREADS; ++k) {
      const double x = red[k];
      red[k] = run;
      run += x;
    }
  }
  __syncthreads();
  double run = red[t];
  for (int i = a; i < b; ++i) {
    run += (double)p[i];
    cdf[i] = run;
  }
}

// One workgroup (not a hot path: once per resample).  Arithmetic in double on the float32 hook tensors; E and F are rounded to float32
// BEFORE the ratio is formed, so the rule is a function of what the tensors hold.
__global__ __launch_bounds__(CLIP_THREADS) void k_clip_sampling_update(int64_t* __restrict__ window, float* __restrict__ hist_E,
                                                                       float* __restrict__ hist_F, float* __restrict__ success,
                                                                       float* prob, double* __restrict__ cdf, int M, double decay,
                                                                       double prior, double floor_) {
  __shared__ double red[CLIP_THREADS];
  const int t = threadIdx.x;
  double part = 0.0;
  for (int i = t; i < M; i += CLIP_THREADS) {
    const float E = (float)(decay * (double)hist_E[i] + (double)window[4 * (size_t)i + 0]);
    const float F = (float)(decay * (double)hist_F[i] + (double)window[4 * (size_t)i + 1]);
    hist_E[i] = E;
    hist_F[i] = F;
    success[i] = E > 0.0f ? (float)(1.0 - (double)F / (double)E) : 0.0f;
    part += ((double)F + prior) / ((double)E + prior);
    window[4 * (size_t)i + 0] = 0; window[4 * (size_t)i + 1] = 0; window[4 * (size_t)i + 2] = 0; window[4 * (size_t)i + 3] = 0;
  }
  const double total = block_sum(part, red);
  const double keep = 1.0 - floor_, uni = floor_ / (double)M;
  for (int i = t; i < M; i += CLIP_THREADS) {       // (each thread re-reads the E, F it wrote itself)
    const double r = ((double)hist_F[i] + prior) / ((double)hist_E[i] + prior);
    prob[i] = (float)(keep * r / total + uni);
  }
  __syncthreads();                                  // prob[] of the other threads (global memory, one workgroup)
  block_cdf(prob, cdf, M, red);
}

// slot j: u = u01(philox4x32(seed; j, draw_index, 20, 0)[0]); clip = first i with cdf[i] > u * cdf[M-1], clamped to M-1.  A clip of
// probability 0 has cdf[i] == cdf[i-1] and is never the FIRST index past the target.
__global__ __launch_bounds__(CLIP_THREADS) void k_clip_sample_slots(const double* __restrict__ cdf, int M, uint64_t seed, uint32_t draw_index,
                                                                    int64_t* __restrict__ slot_clip, int N) {
  const int j = blockIdx.x * CLIP_THREADS + threadIdx.x;
  if (j >= N) return;
  uint32_t o[4];
  philox4x32((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)j, draw_index, PBHC_RNG_STREAM_CLIP_SAMPLING, 0u, o);
  const double target = (double)u01(o[0]) * cdf[M - 1];
  int lo = 0, hi = M;                               // first index in [0, M) with cdf > target, M if none
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cdf[mid] > target) hi = mid; else lo = mid + 1;
  }
  slot_clip[j] = (int64_t)min(lo, M - 1);
}

static int bad(const char* fn, int N, int M) {
  snprintf(g_pbhc_err, sizeof(g_pbhc_err), "%s: bad argument (NULL pointer, N %d, M %d)", fn, N, M);
  return PBHC_EINVAL;
}

extern "C" int pbhc_clip_stats(const int64_t* reset_buf, const uint8_t* time_out_buf, const float* end_time_ratio_buf,
                               const int64_t* last_episode_length_buf, const int64_t* slot_clip, int N, int M, int64_t* window, void* stream) {
  if (!reset_buf || !time_out_buf || !end_time_ratio_buf || !last_episode_length_buf || !slot_clip || !window || N < 1 || M < 1)
    return bad("pbhc_clip_stats", N, M);
  hipLaunchKernelGGL(k_clip_stats, dim3((N + STATS_THREADS - 1) / STATS_THREADS), dim3(STATS_THREADS), 0, (hipStream_t)stream, reset_buf, time_out_buf,
                     end_time_ratio_buf, last_episode_length_buf, slot_clip, N, M, (unsigned long long*)window);
  if (hipGetLastError() != hipSuccess) return PBHC_EHIP;
  return PBHC_OK;
}

extern "C" int pbhc_clip_sampling_update(int64_t* window, float* sampling_history, float* termination_history, float* success_rate,
                                         float* sampling_prob, double* cdf, int M, double decay, double prior_episodes, double uniform_floor,
                                         void* stream) {
  if (!window || !sampling_history || !termination_history || !success_rate || !sampling_prob || !cdf || M < 1)
    return bad("pbhc_clip_sampling_update", 0, M);
  if (!(decay >= 0.0 && decay <= 1.0) || !(prior_episodes > 0.0) || !(uniform_floor >= 0.0 && uniform_floor <= 1.0)) {
    snprintf(g_pbhc_err, sizeof(g_pbhc_err), "pbhc_clip_sampling_update: bad argument (decay %g, prior_episodes %g, uniform_floor %g)", decay,
             prior_episodes, uniform_floor);
    return PBHC_EINVAL;
  }
  hipLaunchKernelGGL(k_clip_sampling_update, dim3(1), dim3(CLIP_THREADS), 0, (hipStream_t)stream, window, sampling_history, termination_history,
                     success_rate, sampling_prob, cdf, M, decay, prior_episodes, uniform_floor);
  if (hipGetLastError() != hipSuccess) return PBHC_EHIP;
  return PBHC_OK;
}

extern "C" int pbhc_clip_sample_slots(const double* cdf, int M, uint64_t seed, uint32_t draw_index, int64_t* slot_clip, int N, void* stream) {
  if (!cdf || !slot_clip || N < 1 || M < 1) return bad("pbhc_clip_sample_slots", N, M);
  hipLaunchKernelGGL(k_clip_sample_slots, dim3((N + CLIP_THREADS - 1) / CLIP_THREADS), dim3(CLIP_THREADS), 0, (hipStream_t)stream, cdf, M, seed,
                     draw_index, slot_clip, N);
  if (hipGetLastError() != hipSuccess) return PBHC_EHIP;
  return PBHC_OK;
}
