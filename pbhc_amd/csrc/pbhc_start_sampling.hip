// pbhc_start_sampling.hip — failure-weighted start-time sampling ("adaptive reference-state initialisation"), all on the device.
//
//   k_start_stats            one launch per control step, right after the fused step: every env that reset adds its finished episode to the
//                            K phase bins of clip slot_clip[env] in `window [M,K,2]` int64 = (visit difference, failures).
//   k_start_sampling_update  off the hot path, one workgroup per clip: folds the window into the decayed histories, forms the look-ahead
//                            weights, the start-bin probabilities and their CDF, clears the window.
//   k_start_draw             start_time[env] = (bin + u2) / K * clip_len with bin drawn from that CDF, keyed by Philox stream 21 and the
//                            device-side step counter: the fused step reads it through PbhcStepIO.ovr_start_time at the env's next reset.
//
// Column 0 of the window is a start / stop DIFFERENCE: +1 in the bin an episode started in, -1 behind the bin it ended in.  Its prefix sum
// over the bins is the number of episodes that visited each bin, for two adds per episode instead of up to K.  Both columns are integers ON
// PURPOSE: integer atomic sums do not depend on arrival order, so a captured rollout graph gives exactly the table of the eager loop.
//
// The step kernel and its config-specialised builds do not know these kernels exist (as with k_clip_stats): they read what a step left in
// the env's buffers and write a buffer the step already knows how to read.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "../../include/pbhc_hip.h"
#include "pbhc_math.h"

using namespace pbhc;

extern thread_local char g_pbhc_err[512];

#define START_THREADS 256
#define START_WAVES (START_THREADS / 64)
#define KB PBHC_START_MAX_BINS

static_assert(2 * KB <= START_THREADS, "k_start_stats zeroes and flushes its 2 x PBHC_START_MAX_BINS counters with one thread each");

// A collapsing policy and reset_all() finish every env's episode in one step, and the v1 configs have ONE clip: all of those adds then land on
// 2 K counters, and same-address atomics run one after the other (about 12 ns each, profiles/clip_sampling.txt).  So a workgroup keeps an LDS
// histogram for ONE clip — the clip of its first finished episode — and flushes the non-zero counters with one 64-bit atomic each; an episode
// of any other clip goes to memory directly (per-lane atomics; with many clips they spread over M K rows).  Both are integer adds: the table
// does not depend on which path an episode took.  A slot_clip outside [0, M) is skipped, never used as an index.
__global__ __launch_bounds__(START_THREADS) void k_start_stats(const int64_t* __restrict__ reset_buf, const uint8_t* __restrict__ time_out_buf,
                                                               const float* __restrict__ end_time_ratio_buf,
                                                               const int64_t* __restrict__ last_episode_length_buf,
                                                               const int64_t* __restrict__ slot_clip, const float* __restrict__ clip_len, double dt,
                                                               int N, int M, int K, unsigned long long* __restrict__ window) {
  __shared__ int s_hist[2][KB];                               // [0]: visit difference, [1]: failures, of the workgroup's home clip
  __shared__ int s_clip[START_WAVES];                         // the clip of a wave's first finished episode, -1: none
  const int t = threadIdx.x, i = blockIdx.x * START_THREADS + t;
  const int wave = t >> 6, lane = t & 63;
  (&s_hist[0][0])[t] = 0;                                     // (2 KB == START_THREADS)
  bool act = false;
  int clip = 0, s = 0, e = 0, fail = 0;
  if (i < N && reset_buf[i] != 0) {
    const int64_t c = slot_clip[i];
    if (c >= 0 && c < (int64_t)M) {
      const double pe = (double)end_time_ratio_buf[i];
      const double ps = pe - ((double)last_episode_length_buf[i] * dt) / (double)clip_len[c];
      if (isfinite(pe) && isfinite(ps)) {
        const double kmax = (double)(K - 1);
        e = (int)fmin(fmax(floor(pe * (double)K), 0.0), kmax);
        s = (int)fmin(fmax(floor(ps * (double)K), 0.0), (double)e);
        act = true;
        clip = (int)c;
        fail = time_out_buf[i] == 0 ? 1 : 0;
      }
    }
  }
  const unsigned long long mask = __ballot(act);
  if (lane == 0) s_clip[wave] = mask != 0ull ? __shfl(clip, __ffsll((long long)mask) - 1, 64) : -1;
  __syncthreads();
  int home = -1;
#pragma unroll
  for (int w = START_WAVES - 1; w >= 0; --w) home = s_clip[w] >= 0 ? s_clip[w] : home;
  if (home < 0) return;                                       // workgroup-uniform: nothing finished here
  if (act) {
    if (clip == home) {
      atomicAdd(&s_hist[0][s], 1);
      if (e + 1 < K) atomicAdd(&s_hist[0][e + 1], -1);
      if (fail) atomicAdd(&s_hist[1][e], 1);
    } else {
      unsigned long long* row = window + 2 * (size_t)clip * K;
      atomicAdd(row + 2 * s, 1ull);
      if (e + 1 < K) atomicAdd(row + 2 * (e + 1), ~0ull);     // -1
      if (fail) atomicAdd(row + 2 * e + 1, 1ull);
    }
  }
  __syncthreads();
  if (t < 2 * K) {                                            // thread t -> (bin t / 2, column t % 2): consecutive lanes, consecutive words
    const int v = s_hist[t & 1][t >> 1];
    if (v != 0) atomicAdd(window + 2 * (size_t)home * K + t, (unsigned long long)(long long)v);
  }
}

// One workgroup per clip, thread b = bin b (not a hot path: once per fold).  Arithmetic in double on the float32 state tensors; V and F are
// rounded to float32 BEFORE the ratio is formed, so the rule is a function of what the tensors hold.  Every sum runs in ascending bin order.
__global__ __launch_bounds__(KB) void k_start_sampling_update(int64_t* __restrict__ window, float* __restrict__ hist_V, float* __restrict__ hist_F,
                                                              float* __restrict__ prob, double* __restrict__ cdf, int K, double decay, double prior,
                                                              double floor_, int H, double lambda) {
  __shared__ long long s_d[KB];
  __shared__ double s_x[KB];                                  // r, then double(prob)
  __shared__ double s_w[KB];
  const int b = threadIdx.x;
  const size_t row = (size_t)blockIdx.x * K;
  long long f = 0;
  if (b < K) {
    s_d[b] = window[2 * (row + b)];
    f = window[2 * (row + b) + 1];
    window[2 * (row + b)] = 0;
    window[2 * (row + b) + 1] = 0;
  }
  __syncthreads();
  if (b < K) {
    long long v = 0;
    for (int i = 0; i <= b; ++i) v += s_d[i];                 // episodes that visited bin b
    const float V = (float)(decay * (double)hist_V[row + b] + (double)v);
    const float F = (float)(decay * (double)hist_F[row + b] + (double)f);
    hist_V[row + b] = V;
    hist_F[row + b] = F;
    s_x[b] = ((double)F + prior) / ((double)V + prior);
  }
  __syncthreads();
  if (b < K) {                                                // a start bin is credited with the failures of the H bins it leads into
    double w = 0.0, pw = 1.0;
    for (int u = 0; u < H && b + u < K; ++u) {
      w += pw * s_x[b + u];
      pw *= lambda;
    }
    s_w[b] = w;
  }
  __syncthreads();
  double total = 0.0;
  for (int i = 0; i < K; ++i) total += s_w[i];
  __syncthreads();                                            // s_x is rewritten below
  if (b < K) {
    const float p = (float)((1.0 - floor_) * s_w[b] / total + floor_ / (double)K);
    prob[row + b] = p;
    s_x[b] = (double)p;
  }
  __syncthreads();
  if (b < K) {
    double run = 0.0;
    for (int i = 0; i <= b; ++i) run += s_x[i];
    cdf[row + b] = run;
  }
}

// env j: (u1, u2) = u01 of words 0, 1 of philox4x32(seed; j, (uint32)counter[0], 21, salt) — or ovr_u[j][0..1] —; bin = first b with
// cdf[c][b] > u1 * cdf[c][K-1], clamped to K-1 (a bin of probability 0 has cdf[b] == cdf[b-1] and is never the FIRST index past the target).
__global__ __launch_bounds__(START_THREADS) void k_start_draw(const double* __restrict__ cdf, const float* __restrict__ clip_len,
                                                              const int64_t* __restrict__ slot_clip, const int64_t* __restrict__ reset_buf,
                                                              const float* __restrict__ ovr_u, int N, int M, int K, uint64_t seed,
                                                              const double* __restrict__ counter, uint32_t salt, float* __restrict__ start_time) {
  const int j = blockIdx.x * START_THREADS + threadIdx.x;
  if (j >= N || (reset_buf && reset_buf[j] == 0)) return;
  const int64_t c = slot_clip[j];
  if (c < 0 || c >= (int64_t)M) return;
  float u1, u2;
  if (ovr_u) {
    u1 = ovr_u[2 * (size_t)j];
    u2 = ovr_u[2 * (size_t)j + 1];
  } else {
    uint32_t o[4];
    philox4x32((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)j, (uint32_t)counter[0], PBHC_RNG_STREAM_START_SAMPLING, salt, o);
    u1 = u01(o[0]);
    u2 = u01(o[1]);
  }
  const double* row = cdf + (size_t)c * K;
  const double target = (double)u1 * row[K - 1];
  int lo = 0, hi = K;                                         // first index in [0, K) with cdf > target, K if none
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (row[mid] > target) hi = mid; else lo = mid + 1;
  }
  const int bin = min(lo, K - 1);
  const float len = clip_len[c];
  // (K - 1 + u2) / K rounds to 1 in float32 for u2 close to 1: sample_time (motion_lib_base.py:486-495) is [0, len)
  const float top = len > 0.0f ? nextafterf(len, 0.0f) : 0.0f;
  start_time[j] = fminf((float)((((double)bin + (double)u2) / (double)K) * (double)len), top);
}

static int bad(const char* fn, int N, int M, int K) {
  snprintf(g_pbhc_err, sizeof(g_pbhc_err), "%s: bad argument (NULL pointer, N %d, M %d, K %d not in [1, %d])", fn, N, M, K, PBHC_START_MAX_BINS);
  return PBHC_EINVAL;
}

static bool bins_ok(int K) { return K >= 1 && K <= PBHC_START_MAX_BINS; }

extern "C" int pbhc_start_stats(const int64_t* reset_buf, const uint8_t* time_out_buf, const float* end_time_ratio_buf,
                                const int64_t* last_episode_length_buf, const int64_t* slot_clip, const float* clip_len, double dt, int N, int M, int K,
                                int64_t* window, void* stream) {
  if (!reset_buf || !time_out_buf || !end_time_ratio_buf || !last_episode_length_buf || !slot_clip || !clip_len || !window || N < 1 || M < 1 ||
      !bins_ok(K))
    return bad("pbhc_start_stats", N, M, K);
  if (!(dt > 0.0 && dt < 1e30)) {
    snprintf(g_pbhc_err, sizeof(g_pbhc_err), "pbhc_start_stats: bad argument (dt %g)", dt);
    return PBHC_EINVAL;
  }
  hipLaunchKernelGGL(k_start_stats, dim3((N + START_THREADS - 1) / START_THREADS), dim3(START_THREADS), 0, (hipStream_t)stream, reset_buf,
                     time_out_buf, end_time_ratio_buf, last_episode_length_buf, slot_clip, clip_len, dt, N, M, K, (unsigned long long*)window);
  if (hipGetLastError() != hipSuccess) return PBHC_EHIP;
  return PBHC_OK;
}

extern "C" int pbhc_start_sampling_update(int64_t* window, float* hist_V, float* hist_F, float* prob, double* cdf, int M, int K, double decay,
                                          double prior_episodes, double uniform_floor, int lookahead_bins, double lookahead_decay, void* stream) {
  if (!window || !hist_V || !hist_F || !prob || !cdf || M < 1 || !bins_ok(K)) return bad("pbhc_start_sampling_update", 0, M, K);
  if (!(decay >= 0.0 && decay <= 1.0) || !(prior_episodes > 0.0 && prior_episodes < 1e300) || !(uniform_floor >= 0.0 && uniform_floor <= 1.0) ||
      lookahead_bins < 1 || lookahead_bins > K || !(lookahead_decay >= 0.0 && lookahead_decay <= 1.0)) {
    snprintf(g_pbhc_err, sizeof(g_pbhc_err),
             "pbhc_start_sampling_update: bad argument (decay %g, prior_episodes %g, uniform_floor %g, lookahead_bins %d of %d, lookahead_decay %g)",
             decay, prior_episodes, uniform_floor, lookahead_bins, K, lookahead_decay);
    return PBHC_EINVAL;
  }
  hipLaunchKernelGGL(k_start_sampling_update, dim3(M), dim3(KB), 0, (hipStream_t)stream, window, hist_V, hist_F, prob, cdf, K, decay, prior_episodes,
                     uniform_floor, lookahead_bins, lookahead_decay);
  if (hipGetLastError() != hipSuccess) return PBHC_EHIP;
  return PBHC_OK;
}

extern "C" int pbhc_start_draw(const double* cdf, const float* clip_len, const int64_t* slot_clip, const int64_t* reset_buf, const float* ovr_u, int N,
                               int M, int K, uint64_t seed, const double* counter, uint32_t salt, float* start_time, void* stream) {
  if (!cdf || !clip_len || !slot_clip || !counter || !start_time || N < 1 || M < 1 || !bins_ok(K)) return bad("pbhc_start_draw", N, M, K);
  hipLaunchKernelGGL(k_start_draw, dim3((N + START_THREADS - 1) / START_THREADS), dim3(START_THREADS), 0, (hipStream_t)stream, cdf, clip_len,
                     slot_clip, reset_buf, ovr_u, N, M, K, seed, counter, salt, start_time);
  if (hipGetLastError() != hipSuccess) return PBHC_EHIP;
  return PBHC_OK;
}
