// stein_thin.hip -- Stein thinning (Riabiz et al. 2022): greedily pick, m times and with replacement, the particle that most
// lowers the kernelized Stein discrepancy of the picked set (include/steinhip.h, stein_thin).
//   obj_t[j] = u_p(j, j) / 2 + sum_{i < t} u_p(x_{s_i}, x_j),   s_t = argmin_j obj_t[j]  (lowest index on equal value)
//   S_t = S_{t-1} + 2 obj_t[s_t],   KSD^2_V of the first t picks = S_t / t^2
// with the Stein kernel u_p of the IMQ or the RBF kernel at the caller's bandwidth (c2 = 2 h2, D = |x - y|^2,
// cross = (g_x - g_y).(x - y), gg = g_x.g_y):
//   IMQ  k = (1 + D / c2)^(-1/2):  u_p = k gg + k^3 cross / c2 + d k^3 / c2 - 3 k^5 D / c2^2,   u_p(j, j) = |g_j|^2 + d / c2
//   RBF  k = exp(-D / c2):         u_p = k (gg + cross / h2 + d / h2 - D / h2^2),               u_p(j, j) = |g_j|^2 + d / h2
// A pick needs ONE row of the n x n Stein-kernel matrix, the row of an index that only the device knows; the matrix is never
// formed.  Work O(m n d), workspace O(n).
//
// One kernel, k_thin_step, launched m + 1 times on the caller's stream.  Launch t:
//   1. every workgroup reduces launch t - 1's per-workgroup (value, index) partials (at most 1024: one pass by its 256 threads)
//      to the pick s_t; workgroup 0 writes idx_out[t - 1] and ksd2_out[t - 1] and keeps S
//   2. x_s and g_s are staged in LDS, THIN_CHUNK columns at a time
//   3. a group of lg lanes (lg = 1 .. 64: the power of two that covers a row's 16-byte -- or, where d % 4 != 0 or a base is
//      not 16-byte aligned, 4-byte -- units, so that narrow rows do not idle a wave) takes THIN_RB rows j at once: D, cross
//      and gg from the DIFFERENCES (a matrix-vector product can afford them; better conditioned than r_i + r_j - 2 x.y),
//      reduced over the group by shuffles, u_p in fp32, added to obj[j] in fp64 -- one add per row and pick against 2 d
//      loads, and the error does not grow with the sum
//   4. each workgroup reduces its rows' (obj, index) to one partial
// Launch 0 writes obj = u_p(j, j) / 2 (fp64 sums) and the first partials; launch m is one workgroup and does step 1 only.
// The partials alternate between two buffers: a workgroup of launch t may write its partial while another still reads
// launch t - 1's.  The launch boundary is the only barrier between workgroups: no cooperative launch, no spin loop, no
// atomics -- every workgroup reduces the same partials in the same order, so a repeated call is bit-identical, and the value
// of u_p(s, j) does not depend on which lanes computed it (duplicated rows get equal objectives: the lower index wins).
// Every load is plain C++; every index read from memory is clamped to [0, n) before it addresses anything.

#include "stein_thin_dev.h"   // the constants, the (value, index) order, thin_up and the row sums: shared with stein_weights.hip

struct ThinPart { double v; long long j; };

struct ThinArgs {
  const float* theta; const float* score; const float* h2;
  long long n, d, t, m;
  int kernel, lg, nparts;            // nparts: workgroups of the previous launch
  double* obj; ThinPart* parts;      // obj [n]; parts [2][THIN_MAX_PARTS]
  double* S;
  long long* idx_out; double* ksd2_out;
};

template <bool VEC>
__global__ __launch_bounds__(THIN_THREADS, THIN_WAVES_PER_SIMD) void k_thin_step(ThinArgs a) {
  __shared__ __attribute__((aligned(16))) float sx[THIN_CHUNK];
  __shared__ __attribute__((aligned(16))) float sg[THIN_CHUNK];
  __shared__ double sv[THIN_THREADS / 64];
  __shared__ long long sj[THIN_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lg = a.lg, gpw = 64 / lg, gl = lane & (lg - 1), grp = lane / lg;
  const long long n = a.n, d = a.d;
  const float h2 = *a.h2;
  const float fd = (float)d;
  long long s = 0;

  if (a.t > 0) {   // 1. the previous launch's partials -> this pick
    const ThinPart* prev = a.parts + ((a.t - 1) & 1) * THIN_MAX_PARTS;
    double bv = INFINITY;
    long long bj = n;
    for (int p = tid; p < a.nparts; p += THIN_THREADS) {
      const ThinPart q = prev[p];
      if (thin_less(q.v, q.j, bv, bj)) { bv = q.v; bj = q.j; }
    }
    thin_block_argmin(bv, bj, sv, sj);
    s = bj < 0 || bj >= n ? 0 : bj;   // (no finite objective at all, h2 = 0 for one: still a row that exists)
    if (blockIdx.x == 0 && tid == 0) {
      const double S = (a.t > 1 ? *a.S : 0.0) + 2.0 * bv;
      *a.S = S;
      a.idx_out[a.t - 1] = s;
      if (a.ksd2_out) a.ksd2_out[a.t - 1] = S / ((double)a.t * (double)a.t);
    }
    if (a.t == a.m) return;
  }

  double bv = INFINITY;
  long long bj = n;
  const long long rows_per_batch = (long long)(THIN_THREADS / 64) * gpw * THIN_RB;
  const long long nbatch = (n + rows_per_batch - 1) / rows_per_batch;

  if (a.t == 0) {   // obj = u_p(j, j) / 2, in fp64
    const double dterm = (double)d / (a.kernel == STEIN_KERNEL_IMQ ? 2.0 * (double)h2 : (double)h2);
    const long long groups = (long long)gridDim.x * (THIN_THREADS / lg);
    const long long g0 = (long long)blockIdx.x * (THIN_THREADS / lg) + tid / lg;
    for (long long base = 0; base < n; base += groups) {   // (the same trip count in every lane: shuffles inside)
      const long long row = base + g0, rc = row < n ? row : n - 1;
      const float* g = a.score + rc * d;
      double acc = 0.0;
      for (long long c = gl; c < d; c += lg) { const double x = (double)g[c]; acc = fma(x, x, acc); }
      for (int o = lg >> 1; o; o >>= 1) acc += __shfl_xor(acc, o);
      if (row < n && gl == 0) {
        const double o = 0.5 * (acc + dterm);
        a.obj[row] = o;
        if (thin_less(o, row, bv, bj)) { bv = o; bj = row; }
      }
    }
  } else {
    const float* xs = a.theta + s * d;
    const float* gs = a.score + s * d;
    const bool one_chunk = d <= THIN_CHUNK;
    if (one_chunk) {   // 2. the picked row, once
      for (int c = tid; c < (int)d; c += THIN_THREADS) { sx[c] = xs[c]; sg[c] = gs[c]; }
      __syncthreads();
    }
    for (long long batch = blockIdx.x; batch < nbatch; batch += gridDim.x) {   // (uniform per workgroup: barriers inside)
      long long row[THIN_RB];
      float D[THIN_RB], C[THIN_RB], G[THIN_RB];   // 3. (thin_row_sums: 16-byte or 4-byte units)
      thin_row_sums<VEC>(a.theta, a.score, xs, gs, sx, sg, n, d, batch, rows_per_batch, lg, gl, grp, gpw, wave, tid, one_chunk,
                         row, D, C, G);
#pragma unroll
      for (int r = 0; r < THIN_RB; ++r) {
        const float Dr = thin_group_sum(D[r], lg), Cr = thin_group_sum(C[r], lg), Gr = thin_group_sum(G[r], lg);
        if (row[r] < n && gl == 0) {
          const double o = a.obj[row[r]] + (double)thin_up(a.kernel, Dr, Cr, Gr, h2, fd);
          a.obj[row[r]] = o;
          if (thin_less(o, row[r], bv, bj)) { bv = o; bj = row[r]; }   // 4.
        }
      }
    }
  }
  thin_block_argmin(bv, bj, sv, sj);
  if (tid == 0) a.parts[(a.t & 1) * THIN_MAX_PARTS + blockIdx.x] = ThinPart{bv, bj};
}

// ---- host ------------------------------------------------------------------------------------------------------------

static thread_local int g_thin_grid = 0;   // stein_debug_thin_grid: 0 = the rule of thin_plan

extern "C" int stein_debug_thin_grid(int blocks) {
  if (blocks < 0 || blocks > 65535) return fail(STEIN_E_BADARG, "blocks %d", blocks);
  g_thin_grid = blocks;
  return STEIN_OK;
}

struct ThinLayout { size_t obj, parts, S, total; };

static int thin_check_shape(int64_t n, int64_t d, int dtype, int flags) {
  if (dtype == STEIN_BF16 || dtype == STEIN_F64)
    return fail(STEIN_E_UNSUPPORTED, "stein_thin takes fp32 inputs (STEIN_F32), not bf16 or f64");
  if (dtype != STEIN_F32) return fail(STEIN_E_UNSUPPORTED, "dtype %d", dtype);
  if (flags != 0) return fail(STEIN_E_BADARG, "stein_thin takes no flags, got 0x%x", flags);
  if (n < 1 || d < 1) return fail(STEIN_E_SHAPE, "bad shape n=%lld d=%lld", (long long)n, (long long)d);
  return stein_check_size(n, d);
}

static ThinLayout thin_layout(int64_t n) {
  ThinLayout L{};
  size_t at = 0;
  auto put = [&](size_t bytes) { const size_t o = at; at = align_up(at + bytes, 256); return o; };
  L.obj = put((size_t)n * 8);
  L.parts = put((size_t)2 * THIN_MAX_PARTS * sizeof(ThinPart));
  L.S = put(8);
  L.total = at;
  return L;
}

extern "C" int stein_thin_workspace_bytes(int64_t n, int64_t d, int dtype, int flags, size_t* out_bytes) {
  if (!out_bytes) return fail(STEIN_E_BADARG, "out_bytes is NULL");
  int rc = thin_check_shape(n, d, dtype, flags);
  if (rc) return rc;
  *out_bytes = thin_layout(n).total;
  return STEIN_OK;
}

extern "C" int stein_thin(const void* theta, const void* score, int64_t n, int64_t d, int dtype, const float* h2_in, int kernel,
                          int64_t m, int64_t* idx_out, double* ksd2_out, void* workspace, size_t ws_bytes, int flags,
                          void* stream) {
  if (!theta || !score || !h2_in || !idx_out || !workspace) return fail(STEIN_E_BADARG, "NULL pointer");
  if ((uintptr_t)workspace & 15) return fail(STEIN_E_BADARG, "the workspace must be 16-byte aligned");
  int rc = thin_check_shape(n, d, dtype, flags);
  if (rc) return rc;
  if (m < 1 || m > (1ll << 30)) return fail(STEIN_E_SHAPE, "bad pick count m=%lld", (long long)m);
  if (kernel != STEIN_KERNEL_RBF && kernel != STEIN_KERNEL_IMQ) return fail(STEIN_E_BADARG, "unknown kernel id %d", kernel);
  const ThinLayout L = thin_layout(n);
  if (ws_bytes < L.total) return fail(STEIN_E_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, L.total);
  if ((rc = stein_take_device_error())) return rc;

  bool vec;
  const int lg = thin_lane_group(d, theta, score, &vec);
  const int64_t rows_per_batch = thin_rows_per_batch(lg);
  int64_t blocks = (n + rows_per_batch - 1) / rows_per_batch;
  if (g_thin_grid > 0) blocks = g_thin_grid;
  if (blocks > THIN_MAX_PARTS) blocks = THIN_MAX_PARTS;

  char* ws = (char*)workspace;
  ThinArgs a{};
  a.theta = (const float*)theta; a.score = (const float*)score; a.h2 = h2_in;
  a.n = n; a.d = d; a.m = m;
  a.kernel = kernel; a.lg = lg; a.nparts = (int)blocks;
  a.obj = (double*)(ws + L.obj); a.parts = (ThinPart*)(ws + L.parts); a.S = (double*)(ws + L.S);
  a.idx_out = (long long*)idx_out; a.ksd2_out = ksd2_out;
  const hipStream_t s = (hipStream_t)stream;
  for (int64_t t = 0; t <= m; ++t) {
    a.t = t;
    const dim3 grid(t == m ? 1u : (unsigned)blocks);
    if (vec) hipLaunchKernelGGL(k_thin_step<true>, grid, dim3(THIN_THREADS), 0, s, a);
    else hipLaunchKernelGGL(k_thin_step<false>, grid, dim3(THIN_THREADS), 0, s, a);
    LAUNCH_CHECK("k_thin_step");
  }
  return STEIN_OK;
}
