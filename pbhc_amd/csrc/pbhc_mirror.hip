// pbhc_mirror.hip — the left <-> right mirror of update-sized observation batches, and the mirror-symmetry loss of the policy mean
// (algo.config.symmetry; semantics: DESIGN §8, the maps: pbhc_amd/envs/obs_mirror.py).
//
//   k_mirror_rows     dst[r * dst_pitch + j] = sign[j] * src[r * src_pitch + index[j]] for several jobs in ONE launch: blockIdx.y is the job,
//                     a workgroup takes MIR_ROWS consecutive rows of it.  The job's table is staged in LDS once per workgroup (index as 16
//                     bits, clamped to the row: a bad table cannot read outside its row); a wave then walks its rows, lane j element j (or
//                     elements 4j .. 4j + 3 with one 16-byte store where the destination allows): the gather stays inside one contiguous source
//                     row, the stores go to consecutive dwords.  A sign flip and a copy: bit-exact.
//   k_symmetry_loss   d = mu_m[b, a] - act_sign[a] * mu[b, act_index[a]]; grad_mu_m = k * d with k = 2 coef / (B A) rounded once on the host;
//                     every thread adds up d * d of its elements (element e of thread t of block g: (g + i * gridDim) * SYM_THREADS + t, i
//                     ascending), the block sums its threads (butterfly inside a wave, the waves in order) into partial[g]
//   k_symmetry_final  one block: the partials in the same way -> scalar_out = float(double(sum) * coef / (B A)); acc_out += it
// No atomics: the grid is a function of B * A alone and every sum has a fixed order, so two runs agree bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/pbhc_hip.h"

extern thread_local char g_pbhc_err[512];

#define MIR_FAIL(...) do { snprintf(g_pbhc_err, sizeof(g_pbhc_err), __VA_ARGS__); return PBHC_EINVAL; } while (0)
#define MIR_ARG(c) do { if (!(c)) MIR_FAIL("%s:%d bad argument: %s", __FILE__, __LINE__, #c); } while (0)

#define MIR_THREADS 256
#define MIR_ROWS 16                                               // rows per workgroup: four per wave; the table is staged once for all of them

struct MirrorJobs { PbhcMirrorJob job[PBHC_MAX_MIRROR_JOBS]; int vec[PBHC_MAX_MIRROR_JOBS]; };

__global__ __launch_bounds__(MIR_THREADS) void k_mirror_rows(MirrorJobs J, int nrows) {
  __shared__ uint16_t s_index[PBHC_MIRROR_MAX_WIDTH];
  __shared__ float s_sign[PBHC_MIRROR_MAX_WIDTH];
  const PbhcMirrorJob job = J.job[blockIdx.y];
  const int width = job.width;
  for (int j = threadIdx.x; j < width; j += MIR_THREADS) {
    const uint32_t i = (uint32_t)job.index[j];
    s_index[j] = (uint16_t)(i < (uint32_t)width ? i : (uint32_t)(width - 1));
    s_sign[j] = job.sign[j];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row0 = blockIdx.x * MIR_ROWS;
  const bool vec4 = J.vec[blockIdx.y] == 4;
  for (int r = row0 + wave; r < row0 + MIR_ROWS && r < nrows; r += MIR_THREADS / 64) {
    const float* __restrict__ src = job.src + (size_t)r * job.src_pitch;
    float* __restrict__ dst = job.dst + (size_t)r * job.dst_pitch;
    if (vec4) {
      const int nv = width >> 2;
      for (int c = lane; c < nv; c += 64) {
        const int j = 4 * c;
        float4 v;
        v.x = s_sign[j] * src[s_index[j]];
        v.y = s_sign[j + 1] * src[s_index[j + 1]];
        v.z = s_sign[j + 2] * src[s_index[j + 2]];
        v.w = s_sign[j + 3] * src[s_index[j + 3]];
        reinterpret_cast<float4*>(dst)[c] = v;
      }
      for (int j = 4 * nv + lane; j < width; j += 64) dst[j] = s_sign[j] * src[s_index[j]];
    } else {
      for (int j = lane; j < width; j += 64) dst[j] = s_sign[j] * src[s_index[j]];
    }
  }
}

// ---- the symmetry loss ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float sym_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// the sum of one value per thread of a block of NT threads, on thread 0: butterfly inside a wave, then the waves in order
template <int NT>
__device__ __forceinline__ float sym_block_sum(float v, float* s_wave) {
  v = sym_wave_sum(v);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
  __syncthreads();
  float total = s_wave[0];
  for (int w = 1; w < NT / 64; ++w) total += s_wave[w];
  return total;
}

__global__ __launch_bounds__(PBHC_SYM_THREADS) void k_symmetry_loss(const float* __restrict__ mu, const float* __restrict__ mu_m,
                                                                      const int32_t* __restrict__ act_index, const float* __restrict__ act_sign, int n,
                                                                      int A, float k, float* __restrict__ grad_mu_m, float* __restrict__ partial) {
  __shared__ int s_index[PBHC_MAX_DOF];
  __shared__ float s_sign[PBHC_MAX_DOF];
  __shared__ float s_wave[PBHC_SYM_THREADS / 64];
  if (threadIdx.x < A) {
    const uint32_t i = (uint32_t)act_index[threadIdx.x];
    s_index[threadIdx.x] = (int)(i < (uint32_t)A ? i : (uint32_t)(A - 1));
    s_sign[threadIdx.x] = act_sign[threadIdx.x];
  }
  __syncthreads();
  float acc = 0.0f;
  const int stride = gridDim.x * PBHC_SYM_THREADS;
  for (int e = blockIdx.x * PBHC_SYM_THREADS + threadIdx.x; e < n; e += stride) {
    const int b = e / A, a = e - b * A;
    const float d = mu_m[e] - s_sign[a] * mu[b * A + s_index[a]];
    grad_mu_m[e] = k * d;
    acc += d * d;
  }
  const float total = sym_block_sum<PBHC_SYM_THREADS>(acc, s_wave);
  if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

__global__ __launch_bounds__(PBHC_SYM_MAX_BLOCKS) void k_symmetry_final(const float* __restrict__ partial, int nb, double scale,
                                                                          float* __restrict__ scalar_out, float* __restrict__ acc_out) {
  __shared__ float s_wave[PBHC_SYM_MAX_BLOCKS / 64];
  const float total = sym_block_sum<PBHC_SYM_MAX_BLOCKS>((int)threadIdx.x < nb ? partial[threadIdx.x] : 0.0f, s_wave);
  if (threadIdx.x == 0) {
    const float loss = (float)((double)total * scale);
    scalar_out[0] = loss;
    if (acc_out) acc_out[0] += loss;
  }
}

extern "C" {

int pbhc_mirror_rows(const PbhcMirrorJob* jobs, int num_jobs, int nrows, void* stream) {
  MIR_ARG(jobs && num_jobs >= 1 && num_jobs <= PBHC_MAX_MIRROR_JOBS && nrows >= 1);
  MirrorJobs J;
  for (int j = 0; j < num_jobs; ++j) {
    const PbhcMirrorJob& q = jobs[j];
    MIR_ARG(q.src && q.dst && q.index && q.sign);
    MIR_ARG(q.width >= 1 && q.width <= PBHC_MIRROR_MAX_WIDTH && q.src_pitch >= q.width && q.dst_pitch >= q.width);
    J.job[j] = q;
    J.vec[j] = ((q.dst_pitch & 3) == 0 && ((uintptr_t)q.dst & 15) == 0) ? 4 : 1;
  }
  hipLaunchKernelGGL(k_mirror_rows, dim3((nrows + MIR_ROWS - 1) / MIR_ROWS, num_jobs), dim3(MIR_THREADS), 0, (hipStream_t)stream, J, nrows);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(g_pbhc_err, sizeof(g_pbhc_err), "pbhc_mirror_rows: %s", hipGetErrorString(e));
    return PBHC_EHIP;
  }
  return PBHC_OK;
}

int pbhc_symmetry_loss(const float* mu, const float* mu_m, const int32_t* act_index, const float* act_sign, int B, int A, float coef, float* grad_mu_m,
                       float* scratch, float* scalar_out, float* acc_out, void* stream) {
  MIR_ARG(mu && mu_m && act_index && act_sign && grad_mu_m && scratch && scalar_out);
  MIR_ARG(B >= 1 && A >= 1 && A <= PBHC_MAX_DOF && (long long)B * A < (1ll << 31) - (long long)PBHC_SYM_MAX_BLOCKS * PBHC_SYM_THREADS);
  const int n = B * A;
  int nb = (n + PBHC_SYM_THREADS * PBHC_SYM_ELEMS - 1) / (PBHC_SYM_THREADS * PBHC_SYM_ELEMS);
  if (nb > PBHC_SYM_MAX_BLOCKS) nb = PBHC_SYM_MAX_BLOCKS;
  const double per = (double)coef / (double)n;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_symmetry_loss, dim3(nb), dim3(PBHC_SYM_THREADS), 0, st, mu, mu_m, act_index, act_sign, n, A, (float)(2.0 * per), grad_mu_m, scratch);
  hipLaunchKernelGGL(k_symmetry_final, dim3(1), dim3(PBHC_SYM_MAX_BLOCKS), 0, st, scratch, nb, per, scalar_out, acc_out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(g_pbhc_err, sizeof(g_pbhc_err), "pbhc_symmetry_loss: %s", hipGetErrorString(e));
    return PBHC_EHIP;
  }
  return PBHC_OK;
}

}  // extern "C"
