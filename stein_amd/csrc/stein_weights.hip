// stein_weights.hip -- Stein importance weights (black-box importance sampling, Liu & Lee 2017): the weights w on the simplex
// that minimise w^T U w, the KSD^2 of the weighted sample, U the Stein-kernel matrix of stein_thin / stein_ksd_boot
// (include/steinhip.h, stein_weights).  Frank-Wolfe with an exact line search from the uniform weights:
//   g = U w,  f = sum_j w_j g_j,  s = argmin_j g_j  (lowest index on equal value)
//   num = f - g_s,  den = f - 2 g_s + u_p(s, s),  gamma = 0 if num <= 0 or den <= 0, else min(1, num / den)
//   w <- (1 - gamma) w + gamma e_s,   g <- (1 - gamma) g + gamma U[s, :]
// A step needs ONE row of U, the row of an index that only the device knows -- what Stein thinning evaluates (thinning is this
// iteration with step 1 / (t + 1) from the empty set); the lane-group code is shared with it (stein_thin_dev.h).
//
//   k_weights_uniform     the float row 1 / n
//   stein_ksd_matmul      g_0 = U w_0 as floats (stein_boot.hip)
//   k_weights_finish<1>   f(uniform) = sum_j g_0[j] / n -> stats_out[2]
//   k_weights_step        launched iters + 1 times.  Launch 0: g, w (fp64) from g_0 and 1 / n, the first partials.  Launch t:
//     1. every workgroup reduces launch t - 1's partials (min g, index, sum w_j g_j; at most 1024: one pass by its 256 threads,
//        the same order in every workgroup) to s, f and, with u_p(s, s) = |g_s|^2 + d / c summed in fp64, gamma; workgroup 0
//        writes idx_out[t - 1] and gamma_out[t - 1]
//     2. x_s and g_s are staged in LDS, THIN_CHUNK columns at a time; 3. lane groups evaluate u_p(s, j) in fp32 from the
//        differences (thin_row_sums, thin_up); g_j and w_j are updated in fp64; 4. the new partials
//     gamma = 0 is a fixed point (nothing moves, every later step is 0 too): the partials are copied and no row is evaluated
//   stein_cast_f64_to_f32, stein_ksd_matmul   a fresh g = U w from the final weights
//   k_weights_finish<0>   one workgroup: w_out, f(w) and the gap w^T g - min g from the FRESH product, not the running g: the
//                         certificate does not inherit the iteration's drift
// Partials belong to VIRTUAL workgroups: virtual workgroup v takes the row batches v, v + nparts, ... in that order, nparts =
// min(1024, batches) -- a function of n and the lane-group width alone.  By default one workgroup runs each; a forced grid
// (stein_debug_weights_grid) only changes which workgroup runs which, so the fp64 sums -- and with them every bit of the
// result -- do not depend on the grid.  The partial buffers alternate and the launch boundary is the only barrier between
// workgroups: no cooperative launch, no spin loop, no atomics.  Every load is plain C++; every index read from memory is
// clamped to [0, n) before it addresses anything; every loop bound is an argument.

#include "stein_thin_dev.h"

struct WeightsPart { double v; long long j; double f; };   // min g, its index, sum w_j g_j over the virtual workgroup's rows

struct WeightsArgs {
  const float* theta; const float* score; const float* h2;
  const float* g0;                   // launch 0: U w_0 as floats
  long long n, d, t;
  int kernel, lg, nparts;            // nparts: virtual workgroups = partials per launch
  double* g; double* w;              // [n] each
  WeightsPart* parts;                // [2][THIN_MAX_PARTS]
  long long* idx_out; double* gamma_out;
};

template <bool VEC>
__global__ __launch_bounds__(THIN_THREADS) void k_weights_step(WeightsArgs a) {
  __shared__ __attribute__((aligned(16))) float sx[THIN_CHUNK];
  __shared__ __attribute__((aligned(16))) float sg[THIN_CHUNK];
  __shared__ double sv[THIN_THREADS / 64];
  __shared__ long long sj[THIN_THREADS / 64];
  __shared__ double red[3][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lg = a.lg, gpw = 64 / lg, gl = lane & (lg - 1), grp = lane / lg;
  const long long n = a.n, d = a.d;
  const float h2 = *a.h2;
  const float fd = (float)d;
  const WeightsPart* prev = a.parts + ((a.t - 1) & 1) * THIN_MAX_PARTS;
  WeightsPart* next = a.parts + (a.t & 1) * THIN_MAX_PARTS;
  long long s = 0;
  double gamma = 0.0, keep = 1.0;

  if (a.t > 0) {   // 1. the previous launch's partials -> this step's vertex and length
    double bv = INFINITY;
    long long bj = n;
    double fs[1] = {0.0};
    for (int p = tid; p < a.nparts; p += THIN_THREADS) {
      const WeightsPart q = prev[p];
      if (thin_less(q.v, q.j, bv, bj)) { bv = q.v; bj = q.j; }
      fs[0] += q.f;
    }
    thin_block_argmin(bv, bj, sv, sj);
    block_sum256(fs, red[0]);
    s = bj < 0 || bj >= n ? 0 : bj;   // (no finite g at all, h2 = 0 for one: still a row that exists)
    const float* gs = a.score + s * d;
    double dd[1] = {0.0};
    for (long long c = tid; c < d; c += THIN_THREADS) { const double x = (double)gs[c]; dd[0] = fma(x, x, dd[0]); }
    block_sum256(dd, red[1]);
    const double uss = dd[0] + (double)d / (a.kernel == STEIN_KERNEL_IMQ ? 2.0 * (double)h2 : (double)h2);
    const double f = fs[0], num = f - bv, den = (f - 2.0 * bv) + uss;
    if (num > 0.0 && den > 0.0) gamma = fmin(1.0, num / den);   // (a NaN fails both comparisons: no step)
    keep = 1.0 - gamma;
    if (blockIdx.x == 0 && tid == 0) {
      if (a.idx_out) a.idx_out[a.t - 1] = s;
      if (a.gamma_out) a.gamma_out[a.t - 1] = gamma;
    }
  }

  const long long rows_per_batch = (long long)(THIN_THREADS / 64) * gpw * THIN_RB;
  const long long nbatch = (n + rows_per_batch - 1) / rows_per_batch;
  const bool moves = a.t > 0 && gamma != 0.0;
  const float* xs = a.theta + s * d;
  const float* gs = a.score + s * d;
  const bool one_chunk = d <= THIN_CHUNK;
  if (moves && one_chunk) {   // 2. the vertex's row, once
    for (int c = tid; c < (int)d; c += THIN_THREADS) { sx[c] = xs[c]; sg[c] = gs[c]; }
    __syncthreads();
  }
  const double w0 = 1.0 / (double)n;

  for (int vb = blockIdx.x; vb < a.nparts; vb += gridDim.x) {   // (uniform per workgroup: barriers inside)
    if (a.t > 0 && !moves) {   // gamma = 0: g and w stay, and so does the partial
      if (tid == 0) next[vb] = prev[vb];
      continue;
    }
    double bv = INFINITY;
    long long bj = n;
    double fs[1] = {0.0};
    for (long long batch = vb; batch < nbatch; batch += a.nparts) {
      long long row[THIN_RB];
      if (a.t == 0) {   // g = g_0, w = 1 / n: the rows in the places the steps will keep them
#pragma unroll
        for (int r = 0; r < THIN_RB; ++r) {
          row[r] = batch * rows_per_batch + ((long long)wave * THIN_RB + r) * gpw + grp;
          if (row[r] < n && gl == 0) {
            const double gj = (double)a.g0[row[r]];
            a.g[row[r]] = gj;
            a.w[row[r]] = w0;
            if (thin_less(gj, row[r], bv, bj)) { bv = gj; bj = row[r]; }
            fs[0] = fma(w0, gj, fs[0]);
          }
        }
      } else {
        float D[THIN_RB], C[THIN_RB], G[THIN_RB];   // 3.
        thin_row_sums<VEC>(a.theta, a.score, xs, gs, sx, sg, n, d, batch, rows_per_batch, lg, gl, grp, gpw, wave, tid, one_chunk,
                           row, D, C, G);
#pragma unroll
        for (int r = 0; r < THIN_RB; ++r) {
          const float Dr = thin_group_sum(D[r], lg), Cr = thin_group_sum(C[r], lg), Gr = thin_group_sum(G[r], lg);
          if (row[r] < n && gl == 0) {
            const double u = (double)thin_up(a.kernel, Dr, Cr, Gr, h2, fd);
            const double gj = fma(keep, a.g[row[r]], gamma * u);
            const double wj = fma(keep, a.w[row[r]], row[r] == s ? gamma : 0.0);
            a.g[row[r]] = gj;
            a.w[row[r]] = wj;
            if (thin_less(gj, row[r], bv, bj)) { bv = gj; bj = row[r]; }   // 4.
            fs[0] = fma(wj, gj, fs[0]);
          }
        }
      }
    }
    thin_block_argmin(bv, bj, sv, sj);   // (its first barrier stands between red[2]'s readers and the next writers)
    block_sum256(fs, red[2]);
    if (tid == 0) next[vb] = WeightsPart{bv, bj, fs[0]};
  }
}

__global__ __launch_bounds__(256) void k_weights_uniform(float* __restrict__ wf, long long n) {
  const float v = (float)(1.0 / (double)n);
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += gridDim.x * 256ll) wf[i] = v;
}

// One workgroup: f = sum_j w_j g_j and min_j g_j of the float product g.  UNIFORM: w_j = 1 / n, stats[2] = f and nothing else
// is written; else w is the iteration's, w_out = w, stats[0] = f, stats[1] = f - min g.
template <bool UNIFORM>
__global__ __launch_bounds__(256) void k_weights_finish(const double* __restrict__ w, const float* __restrict__ g, long long n,
                                                        double* __restrict__ w_out, double* __restrict__ stats) {
  __shared__ double red[4];
  __shared__ double smin[4];
  const int tid = threadIdx.x;
  const double w0 = 1.0 / (double)n;
  double fs[1] = {0.0};
  double mn = INFINITY;
  for (long long j = tid; j < n; j += 256) {
    const double gj = (double)g[j];
    const double wj = UNIFORM ? w0 : w[j];
    if (!UNIFORM) w_out[j] = wj;
    fs[0] = fma(wj, gj, fs[0]);
    mn = fmin(mn, gj);
  }
  block_sum256(fs, red);
  if (UNIFORM) {
    if (tid == 0) stats[2] = fs[0];
    return;
  }
  for (int o = 32; o; o >>= 1) mn = fmin(mn, __shfl_xor(mn, o));
  if ((tid & 63) == 0) smin[tid >> 6] = mn;
  __syncthreads();
  if (tid == 0) {
    mn = fmin(fmin(smin[0], smin[1]), fmin(smin[2], smin[3]));
    stats[0] = fs[0];
    stats[1] = fs[0] - mn;
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------

static thread_local int g_weights_grid = 0;   // stein_debug_weights_grid: 0 = one workgroup per virtual workgroup

extern "C" int stein_debug_weights_grid(int blocks) {
  if (blocks < 0 || blocks > 65535) return fail(STEIN_E_BADARG, "blocks %d", blocks);
  g_weights_grid = blocks;
  return STEIN_OK;
}

// the matmul's workspace for one row | g | w (fp64) | w as floats | U w as floats | the partials
struct WeightsLayout { size_t mm_bytes, mm, g, w, wf, gf, parts, total; };

static int weights_check_shape(int64_t n, int64_t d, int dtype, int flags) {
  if (dtype == STEIN_BF16 || dtype == STEIN_F64)
    return fail(STEIN_E_UNSUPPORTED, "stein_weights takes fp32 inputs (STEIN_F32), not bf16 or f64");
  if (dtype != STEIN_F32) return fail(STEIN_E_UNSUPPORTED, "dtype %d", dtype);
  if (flags != 0) return fail(STEIN_E_BADARG, "stein_weights takes no flags, got 0x%x", flags);
  if (n < 2 || d < 1) return fail(STEIN_E_SHAPE, "bad shape n=%lld d=%lld: need n >= 2 and d >= 1", (long long)n, (long long)d);
  return stein_check_size(n, d);
}

static int weights_layout(int64_t n, int64_t d, WeightsLayout* L) {
  *L = WeightsLayout{};
  if (int rc = stein_ksd_matmul_workspace_bytes(n, d, 1, STEIN_F32, 0, &L->mm_bytes)) return rc;
  size_t at = 0;
  auto put = [&](size_t bytes) { const size_t o = at; at = align_up(at + bytes, 256); return o; };
  L->mm = put(L->mm_bytes);
  L->g = put((size_t)n * 8);
  L->w = put((size_t)n * 8);
  L->wf = put((size_t)n * 4);
  L->gf = put((size_t)n * 4);
  L->parts = put((size_t)2 * THIN_MAX_PARTS * sizeof(WeightsPart));
  L->total = at;
  return STEIN_OK;
}

extern "C" int stein_weights_workspace_bytes(int64_t n, int64_t d, int dtype, int flags, size_t* out_bytes) {
  if (!out_bytes) return fail(STEIN_E_BADARG, "out_bytes is NULL");
  int rc = weights_check_shape(n, d, dtype, flags);
  if (rc) return rc;
  WeightsLayout L;
  if ((rc = weights_layout(n, d, &L))) return rc;
  *out_bytes = L.total;
  return STEIN_OK;
}

extern "C" int stein_weights(const void* theta, const void* score, int64_t n, int64_t d, int dtype, const float* h2_in, int kernel,
                             int64_t iters, double* w_out, double* stats_out, int64_t* idx_out, double* gamma_out,
                             void* workspace, size_t ws_bytes, int flags, void* stream) {
  if (!theta || !score || !h2_in || !w_out || !stats_out || !workspace) return fail(STEIN_E_BADARG, "NULL pointer");
  if ((uintptr_t)workspace & 15) return fail(STEIN_E_BADARG, "the workspace must be 16-byte aligned");
  int rc = weights_check_shape(n, d, dtype, flags);
  if (rc) return rc;
  if (iters < 0 || iters > (1ll << 30)) return fail(STEIN_E_SHAPE, "bad iteration count iters=%lld", (long long)iters);
  if (kernel != STEIN_KERNEL_RBF && kernel != STEIN_KERNEL_IMQ) return fail(STEIN_E_BADARG, "unknown kernel id %d", kernel);
  WeightsLayout L;
  if ((rc = weights_layout(n, d, &L))) return rc;
  if (ws_bytes < L.total) return fail(STEIN_E_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, L.total);
  if ((rc = stein_take_device_error())) return rc;

  bool vec;
  const int lg = thin_lane_group(d, theta, score, &vec);
  const int64_t rows_per_batch = thin_rows_per_batch(lg);
  int64_t nparts = (n + rows_per_batch - 1) / rows_per_batch;
  if (nparts > THIN_MAX_PARTS) nparts = THIN_MAX_PARTS;
  int64_t blocks = g_weights_grid > 0 ? g_weights_grid : nparts;
  if (blocks > THIN_MAX_PARTS) blocks = THIN_MAX_PARTS;

  char* ws = (char*)workspace;
  float* wf = (float*)(ws + L.wf);
  float* gf = (float*)(ws + L.gf);
  WeightsArgs a{};
  a.theta = (const float*)theta; a.score = (const float*)score; a.h2 = h2_in; a.g0 = gf;
  a.n = n; a.d = d;
  a.kernel = kernel; a.lg = lg; a.nparts = (int)nparts;
  a.g = (double*)(ws + L.g); a.w = (double*)(ws + L.w); a.parts = (WeightsPart*)(ws + L.parts);
  a.idx_out = (long long*)idx_out; a.gamma_out = gamma_out;
  const hipStream_t s = (hipStream_t)stream;

  hipLaunchKernelGGL(k_weights_uniform, dim3((unsigned)grid_for(n, 1024)), dim3(256), 0, s, wf, (long long)n);
  LAUNCH_CHECK("k_weights_uniform");
  if ((rc = stein_ksd_matmul(theta, score, n, d, dtype, h2_in, kernel, wf, 1, gf, ws + L.mm, L.mm_bytes, 0, stream))) return rc;
  hipLaunchKernelGGL(k_weights_finish<true>, dim3(1), dim3(256), 0, s, (const double*)nullptr, gf, (long long)n,
                     (double*)nullptr, stats_out);
  LAUNCH_CHECK("k_weights_finish");
  for (int64_t t = 0; t <= iters; ++t) {
    a.t = t;
    if (vec) hipLaunchKernelGGL(k_weights_step<true>, dim3((unsigned)blocks), dim3(THIN_THREADS), 0, s, a);
    else hipLaunchKernelGGL(k_weights_step<false>, dim3((unsigned)blocks), dim3(THIN_THREADS), 0, s, a);
    LAUNCH_CHECK("k_weights_step");
  }
  if ((rc = stein_cast_f64_to_f32(a.w, wf, n, stream))) return rc;
  if ((rc = stein_ksd_matmul(theta, score, n, d, dtype, h2_in, kernel, wf, 1, gf, ws + L.mm, L.mm_bytes, 0, stream))) return rc;
  hipLaunchKernelGGL(k_weights_finish<false>, dim3(1), dim3(256), 0, s, a.w, gf, (long long)n, w_out, stats_out);
  LAUNCH_CHECK("k_weights_finish");
  return STEIN_OK;
}
