// stein_thin_dev.h -- what the two kernels that evaluate ONE row of the Stein-kernel matrix per launch share: k_thin_step
// (stein_thin.hip, Stein thinning) and k_weights_step (stein_weights.hip, Stein importance weights).  Both take the row of an
// index that only the device knows, stage x_s and g_s in LDS and let a group of lg lanes take THIN_RB rows j at once.
//   thin_less / thin_block_argmin   the (value, index) order -- lowest index on equal value -- and its workgroup reduction
//   thin_group_sum, thin_up         a lane group's sum; u_p in fp32 from the three sums of one pair
//   thin_row_sums<VEC>              D, cross and gg of THIN_RB rows against the staged row, from the differences
//   thin_lane_group                 (host) the lane-group width rule and the choice between 16-byte and 4-byte units
#pragma once

#include "stein_host.h"

constexpr int THIN_THREADS = 256;
constexpr int THIN_CHUNK = 512;     // columns of x_s and of g_s in LDS at a time (4 KB)
constexpr int THIN_RB = 4;          // rows a lane group holds at once: 2 x THIN_RB loads in flight per lane
constexpr int THIN_MAX_PARTS = 1024;
// k_thin_step runs up to 1024 workgroups of four waves on 256 CUs: four waves per SIMD, which the register file grants at 128
// VGPRs.  k_thin_step<true> needs 127 with its row loop written out in the kernel and drifted to 137 with the loop in
// thin_row_sums -- three waves per SIMD, a third of the step's rate lost at 16384 x 256 -- so its launch bound names the
// occupancy.  (k_weights_step<true> holds its fp64 update on top: 154 registers, and 20 spills under the same bound; it runs
// at three waves per SIMD.)
constexpr int THIN_WAVES_PER_SIMD = 4;

__device__ __forceinline__ bool thin_less(double v, long long j, double bv, long long bj) {
  return v < bv || (v == bv && j < bj);
}

// (v, j) of the workgroup's least value, lowest index on equal value, in every thread
__device__ __forceinline__ void thin_block_argmin(double& v, long long& j, double* sv, long long* sj) {
  for (int o = 32; o; o >>= 1) {
    const double ov = __shfl_xor(v, o);
    const long long oj = __shfl_xor(j, o);
    if (thin_less(ov, oj, v, j)) { v = ov; j = oj; }
  }
  __syncthreads();   // (the arrays' previous readers)
  if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = v; sj[threadIdx.x >> 6] = j; }
  __syncthreads();
  v = sv[0]; j = sj[0];
  for (int w = 1; w < THIN_THREADS / 64; ++w)
    if (thin_less(sv[w], sj[w], v, j)) { v = sv[w]; j = sj[w]; }
}

__device__ __forceinline__ float thin_group_sum(float x, int lg) {
  for (int o = lg >> 1; o; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// u_p from the three sums of one pair
__device__ __forceinline__ float thin_up(int kernel, float D, float cross, float gg, float h2, float fd) {
  if (kernel == STEIN_KERNEL_IMQ) {
    const float c2 = 2.0f * h2;
    const float k = rsqrtf(1.0f + D / c2);
    const float k3 = k * k * k, k5 = k3 * k * k;
    return k * gg + k3 * cross / c2 + fd * k3 / c2 - 3.0f * k5 * D / (c2 * c2);
  }
  const float k = expf(-D / (2.0f * h2));
  return k * (gg + cross / h2 + fd / h2 - D / (h2 * h2));
}

// The rows of batch `batch` that this thread's lane group holds (row[r]; for a fixed r the wave's groups read gpw consecutive
// rows; rows >= n are evaluated as row n - 1 and must be masked by the caller) and their three sums against row s: D = |x_s -
// x_j|^2, C = (g_s - g_j).(x_s - x_j), G = g_s.g_j, from the differences in fp32: this lane's share (thin_group_sum adds the group's).
// one_chunk (d <= THIN_CHUNK): the caller has staged x_s and g_s in sx / sg once; else they are staged here, THIN_CHUNK columns
// at a time, behind barriers -- so every thread of the workgroup must call this with the same batch count.
template <bool VEC>
__device__ __forceinline__ void thin_row_sums(const float* theta, const float* score, const float* xs, const float* gs, float* sx,
                                              float* sg, long long n, long long d, long long batch, long long rows_per_batch,
                                              int lg, int gl, int grp, int gpw, int wave, int tid, bool one_chunk,
                                              long long (&row)[THIN_RB], float (&D)[THIN_RB], float (&C)[THIN_RB],
                                              float (&G)[THIN_RB]) {
  const float* xr[THIN_RB];
  const float* gr[THIN_RB];
#pragma unroll
  for (int r = 0; r < THIN_RB; ++r) {
    row[r] = batch * rows_per_batch + ((long long)wave * THIN_RB + r) * gpw + grp;
    const long long rc = row[r] < n ? row[r] : n - 1;
    xr[r] = theta + rc * d;
    gr[r] = score + rc * d;
    D[r] = C[r] = G[r] = 0.0f;
  }
  for (long long c0 = 0; c0 < d; c0 += THIN_CHUNK) {
    const int len = (int)(d - c0 < THIN_CHUNK ? d - c0 : THIN_CHUNK);
    if (!one_chunk) {
      __syncthreads();   // (the previous chunk's readers)
      for (int c = tid; c < len; c += THIN_THREADS) { sx[c] = xs[c0 + c]; sg[c] = gs[c0 + c]; }
      __syncthreads();
    }
    if (VEC) {   // 16-byte units: d % 4 == 0 and both bases aligned, so every row and every chunk starts aligned
      for (int u = gl; u < len / 4; u += lg) {
        const float4 x0 = reinterpret_cast<const float4*>(sx)[u], g0 = reinterpret_cast<const float4*>(sg)[u];
        float4 x[THIN_RB], g[THIN_RB];
#pragma unroll
        for (int r = 0; r < THIN_RB; ++r) {
          x[r] = reinterpret_cast<const float4*>(xr[r] + c0)[u];
          g[r] = reinterpret_cast<const float4*>(gr[r] + c0)[u];
        }
#pragma unroll
        for (int r = 0; r < THIN_RB; ++r) {
          const float dx0 = x0.x - x[r].x, dx1 = x0.y - x[r].y, dx2 = x0.z - x[r].z, dx3 = x0.w - x[r].w;
          D[r] = fmaf(dx0, dx0, D[r]); D[r] = fmaf(dx1, dx1, D[r]); D[r] = fmaf(dx2, dx2, D[r]); D[r] = fmaf(dx3, dx3, D[r]);
          C[r] = fmaf(g0.x - g[r].x, dx0, C[r]); C[r] = fmaf(g0.y - g[r].y, dx1, C[r]);
          C[r] = fmaf(g0.z - g[r].z, dx2, C[r]); C[r] = fmaf(g0.w - g[r].w, dx3, C[r]);
          G[r] = fmaf(g0.x, g[r].x, G[r]); G[r] = fmaf(g0.y, g[r].y, G[r]);
          G[r] = fmaf(g0.z, g[r].z, G[r]); G[r] = fmaf(g0.w, g[r].w, G[r]);
        }
      }
    } else {     // 4-byte units: any d, any alignment
      for (int u = gl; u < len; u += lg) {
        const float x0 = sx[u], g0 = sg[u];
        float x[THIN_RB], g[THIN_RB];
#pragma unroll
        for (int r = 0; r < THIN_RB; ++r) { x[r] = xr[r][c0 + u]; g[r] = gr[r][c0 + u]; }
#pragma unroll
        for (int r = 0; r < THIN_RB; ++r) {
          const float dx = x0 - x[r];
          D[r] = fmaf(dx, dx, D[r]);
          C[r] = fmaf(g0 - g[r], dx, C[r]);
          G[r] = fmaf(g0, g[r], G[r]);
        }
      }
    }
  }
}

// A row is taken by the power-of-two group of lanes (1 .. 64) that covers its 16-byte units -- or, where d % 4 != 0 or a base
// pointer is not 16-byte aligned (*vec = false), its 4-byte units -- so that narrow rows do not idle a wave.
static inline int thin_lane_group(int64_t d, const void* theta, const void* score, bool* vec) {
  *vec = d % 4 == 0 && (((uintptr_t)theta | (uintptr_t)score) & 15) == 0;
  const int64_t units = *vec ? d / 4 : d;
  int lg = 1;
  while (lg < 64 && lg < units) lg <<= 1;
  return lg;
}
static inline int64_t thin_rows_per_batch(int lg) { return (int64_t)(THIN_THREADS / 64) * (64 / lg) * THIN_RB; }
