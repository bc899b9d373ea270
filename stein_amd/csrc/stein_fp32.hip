// stein_fp32.hip -- the fp32-input MFMA path (calls without the split operand planes): the distance pass k_distance and
// the contraction k_phi_partial on the fp32 matrix cores (32x32x2), with the host functions that launch them.  The split
// path (stein_x3.hip) replaces both when the planes are given.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stein_host.h"

constexpr int LDK = BK + 4;    // LDS row stride (floats) of a [rows][k] fp32 tile: +16 B keeps ds_read_b128 conflict-free

// Row-of-k tile loader: rows `rbase + lr + 32p`, k range [k0 + lc, +4).  VEC requires d % 4 == 0.
template <bool VEC>
__device__ __forceinline__ void load_rows_k(const float* __restrict__ M, int nrows, int d, int rbase, int k0,
                                            int lr, int lc, float4 (&v)[4]) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int row = rbase + lr + 32 * p;
    const int k = k0 + lc;
    if (VEC) {
      v[p] = ld4_or_zero(M + (size_t)row * d + k, row < nrows && k < d);
    } else {
      const float* src = M + (size_t)row * d + k;
      const bool rok = row < nrows;
      v[p].x = (rok && k + 0 < d) ? src[0] : 0.f;
      v[p].y = (rok && k + 1 < d) ? src[1] : 0.f;
      v[p].z = (rok && k + 2 < d) ? src[2] : 0.f;
      v[p].w = (rok && k + 3 < d) ? src[3] : 0.f;
    }
  }
}

__device__ __forceinline__ void store_rows_k(float* S, int lr, int lc, const float4 (&v)[4]) {
#pragma unroll
  for (int p = 0; p < 4; ++p) *reinterpret_cast<float4*>(S + (lr + 32 * p) * LDK + lc) = v[p];
}

__device__ __forceinline__ float comp(const float4& v, int t) {
  return t == 0 ? v.x : (t == 1 ? v.y : (t == 2 ? v.z : v.w));
}

// ------------------------------------------------------------------------------------------------
// k_distance: D = r_i + r_j - 2 T T^T on the fp32 matrix cores.
//   A operand = rows of the row block, B operand = rows of the column block, both k-contiguous, so both
//   tiles live in LDS as [row][k] and a lane fetches 4 consecutive k with one ds_read_b128.  The k order
//   inside an MFMA step is permuted identically for A and B (lane half h, step t <-> k = 8kk + 4h + t).
//   Every D_ij runs the same k-ordered fma chain with the operands swapped for D_ji, so D is bitwise
//   symmetric.  SYM (the block is the whole n x n matrix): only tiles on or above the diagonal are
//   computed and each off-diagonal tile is also stored transposed -- half the MFMA work.
//   hist0 != NULL: the level-0 radix-select histogram (top 11 key bits) is taken from the accumulators
//   here instead of re-reading D; a mirrored tile counts twice.
// ------------------------------------------------------------------------------------------------
template <bool VEC, bool SYM>
__global__ __launch_bounds__(NTHREADS, 2) void k_distance(const float* __restrict__ T, const float* __restrict__ r,
                                                       float* __restrict__ D, int n, int d, int row0, int n_local,
                                                       long ldD, int tiles_m, int tiles_n, u64* __restrict__ hist0,
                                                       SpecState* __restrict__ spec, u64* __restrict__ spec_buf) {
  constexpr int kStage = (BM + BN) * LDK, kEpi = EPI_LDS_BYTES / 4;   // main loop tiles; the epilogue reuses the array
  __shared__ __attribute__((aligned(16))) float smem[kStage > kEpi ? kStage : kEpi];
  float* As = smem;
  float* Bs = smem + BM * LDK;

  int tile_m, tile_n;
  if (!distance_tile<SYM>(xcd_remap(blockIdx.x, gridDim.x), tiles_m, tiles_n, tile_m, tile_n)) return;

  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int wy = wid >> 1, wx = wid & 1;
  const int lr = t >> 3, lc = (t & 7) * 4;
  const int arow0 = row0 + tile_m * BM;  // global particle index of the tile's first row
  const int brow0 = tile_n * BN;
  const EpiPrefetch pf = distance_epilogue_prefetch(r, n, row0, n_local, tile_m, tile_n, spec);

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  float4 ra[4], rb[4];
  load_rows_k<VEC>(T, n, d, arow0, 0, lr, lc, ra);
  load_rows_k<VEC>(T, n, d, brow0, 0, lr, lc, rb);

  const int l31 = lane & 31, h4 = (lane >> 5) * 4;
  for (int k0 = 0; k0 < d; k0 += BK) {
    store_rows_k(As, lr, lc, ra);
    store_rows_k(Bs, lr, lc, rb);
    __syncthreads();
    if (k0 + BK < d) {  // next tile's loads fly under this tile's MFMAs
      load_rows_k<VEC>(T, n, d, arow0, k0 + BK, lr, lc, ra);
      load_rows_k<VEC>(T, n, d, brow0, k0 + BK, lr, lc, rb);
    }
#pragma unroll
    for (int kk = 0; kk < BK / 8; ++kk) {
      float4 a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[i] = *reinterpret_cast<const float4*>(As + (wy * 64 + i * 32 + l31) * LDK + kk * 8 + h4);
        b[i] = *reinterpret_cast<const float4*>(Bs + (wx * 64 + i * 32 + l31) * LDK + kk * 8 + h4);
      }
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(comp(a[i], s), comp(b[j], s), acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }

  // the staging tiles are dead (every wave is past the loop's last barrier): 8 KB of them hold the level-0 histogram
  distance_epilogue<SYM>(acc, reinterpret_cast<u32*>(smem), D, n, n_local, ldD, tile_m, tile_n, hist0, pf, 2.f,
                         spec, spec_buf);
}

// ------------------------------------------------------------------------------------------------
// k_phi_partial: O[z] = P[:, jrange(z)] . V[jrange(z), cblock],  P = exp2(c D) built tile by tile.
//   A operand = P tile [128 rows][32 j], written to LDS as [row][j] right after the exp, read back with
//   ds_read_b128 (same k permutation as k_distance).  B operand = V tile [32 j][128 c], row-major in LDS;
//   a lane reads V[j = 8kk + 4h + s][c = lane & 31] with ds_read_b32 (32 consecutive floats per half wave).
//   The thread that stages P(row, 4 j) keeps the running rowsum for that row.
// ------------------------------------------------------------------------------------------------
template <bool VEC>
__device__ __forceinline__ void load_v_tile(const float* __restrict__ V, int n, int d, int j0, int jend, int c0,
                                            int vr, int vc, float4 (&v)[4]) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int j = j0 + vr + 8 * p;
    const int c = c0 + vc;
    const bool jok = j < jend;
    if (VEC) {
      v[p] = ld4_or_zero(V + (size_t)j * d + c, jok && c < d);
    } else {
      const float* src = V + (size_t)j * d + c;
      v[p].x = (jok && c + 0 < d) ? src[0] : 0.f;
      v[p].y = (jok && c + 1 < d) ? src[1] : 0.f;
      v[p].z = (jok && c + 2 < d) ? src[2] : 0.f;
      v[p].w = (jok && c + 3 < d) ? src[3] : 0.f;
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(NTHREADS) void k_phi_partial(const float* __restrict__ D, long ldD,
                                                          const float* __restrict__ G, const float* __restrict__ T,
                                                          const float* __restrict__ h2p, float* __restrict__ OG,
                                                          float* __restrict__ OT, float* __restrict__ RS, int n, int d,
                                                          int n_local, int tiles_m, int cblocks, int split, int jchunk) {
  __shared__ __attribute__((aligned(16))) float smem[BM * LDK + BK * BN];
  float* As = smem;
  float* Bs = smem + BM * LDK;

  const int logical = xcd_remap(blockIdx.x, gridDim.x);
  const int ncb = 2 * cblocks;
  const int cb = logical % ncb;
  const int tile_m = (logical / ncb) % tiles_m;
  const int z = logical / (ncb * tiles_m);
  const bool isT = cb >= cblocks;
  const float* __restrict__ V = isT ? T : G;
  float* __restrict__ O = isT ? OT : OG;
  const int c0 = (isT ? cb - cblocks : cb) * BN;

  const int jbeg = z * jchunk;
  const int jend = min(n, jbeg + jchunk);

  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int wy = wid >> 1, wx = wid & 1;
  const int lr = t >> 3, lc = (t & 7) * 4;   // P staging: rows lr + 32p, 4 consecutive j
  const int vr = t >> 5, vc = (t & 31) * 4;  // V staging: j rows vr + 8p, 4 consecutive c
  const int i0 = tile_m * BM;

  const float cexp = -1.44269504088896341f / (2.f * *h2p);  // exp(-D/(2 h2)) = exp2(cexp * D)

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  float rs[4] = {0.f, 0.f, 0.f, 0.f};

  float4 rd[4], rv[4];
  // the D tile (tile_m, j0 / 32) is one contiguous [128][32] block (rows are padded to 128 in memory)
  const float* __restrict__ drow = D + (size_t)tile_m * (ldD >> 5) * DT_ELEMS;
  auto load_d = [&](int j0) {
    const float* tile = drow + (size_t)(j0 >> 5) * DT_ELEMS;
#pragma unroll
    for (int p = 0; p < 4; ++p) rd[p] = *reinterpret_cast<const float4*>(tile + (lr + 32 * p) * DT_COLS + lc);
  };
  if (jbeg < jend) {
    load_d(jbeg);
    load_v_tile<VEC>(V, n, d, jbeg, jend, c0, vr, vc, rv);
  }

  const int l31 = lane & 31, h4 = (lane >> 5) * 4;
  for (int j0 = jbeg; j0 < jend; j0 += BK) {
    // P = exp2(cexp * D) for in-range j, 0 outside; stage to LDS, keep the rowsum
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int j = j0 + lc;
      float4 pv;
      pv.x = (j + 0 < jend) ? __builtin_amdgcn_exp2f(cexp * rd[p].x) : 0.f;
      pv.y = (j + 1 < jend) ? __builtin_amdgcn_exp2f(cexp * rd[p].y) : 0.f;
      pv.z = (j + 2 < jend) ? __builtin_amdgcn_exp2f(cexp * rd[p].z) : 0.f;
      pv.w = (j + 3 < jend) ? __builtin_amdgcn_exp2f(cexp * rd[p].w) : 0.f;
      if (i0 + lr + 32 * p >= n_local) pv = make_float4(0.f, 0.f, 0.f, 0.f);
      rs[p] += (pv.x + pv.y) + (pv.z + pv.w);
      *reinterpret_cast<float4*>(As + (lr + 32 * p) * LDK + lc) = pv;
      *reinterpret_cast<float4*>(Bs + (vr + 8 * p) * BN + vc) = rv[p];
    }
    __syncthreads();
    if (j0 + BK < jend) {
      load_d(j0 + BK);
      load_v_tile<VEC>(V, n, d, j0 + BK, jend, c0, vr, vc, rv);
    }
#pragma unroll
    for (int kk = 0; kk < BK / 8; ++kk) {
      float4 a[2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
        a[i] = *reinterpret_cast<const float4*>(As + (wy * 64 + i * 32 + l31) * LDK + kk * 8 + h4);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        float b[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) b[j] = Bs[(kk * 8 + h4 + s) * BN + wx * 64 + j * 32 + l31];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(comp(a[i], s), b[j], acc[i][j], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  phi_epilogue(acc, rs, O + (size_t)z * n_local * d, RS + (size_t)z * n_local, d, n_local, i0, c0, cb == 0);
}

template <bool VEC, bool SYM>
static void launch_distance(long nblk, hipStream_t s, const float* T, const float* r, float* D, int n, int d, int row0,
                            int n_local, long ld, int tiles_m, int tiles_n, u64* hist0, SpecState* spec, u64* spec_buf) {
  hipLaunchKernelGGL((k_distance<VEC, SYM>), dim3((unsigned)nblk), dim3(NTHREADS), 0, s, T, r, D, n, d, row0, n_local,
                     ld, tiles_m, tiles_n, hist0, spec, spec_buf);
}

int stein_fp32_distance(const StepViews& v, const BlockShape& b, const float* T, bool sym, bool window, hipStream_t s) {
  const int tiles_m = (int)((b.n_local + BM - 1) / BM), tiles_n = (int)((b.n + BN - 1) / BN);
  const long nblk = distance_grid(sym, tiles_m, tiles_n);
  if (nblk > 0x7fffffffl) return stein_fail(STEIN_E_SHAPE, "too many tiles");
  const bool vec = (b.d % 4 == 0) && (((uintptr_t)T & 15) == 0);
  SpecState* spec = window ? v.spec : nullptr;
  u64* spec_buf = window ? v.spec_buf : nullptr;
#define FP32_DIST(VEC, SYM) launch_distance<VEC, SYM>(nblk, s, T, v.r, v.D, (int)b.n, (int)b.d, (int)b.row0, (int)b.n_local, (long)v.L.ld_dist, tiles_m, tiles_n, v.hist, spec, spec_buf)
  if (vec && sym) FP32_DIST(true, true);
  else if (vec) FP32_DIST(true, false);
  else if (sym) FP32_DIST(false, true);
  else FP32_DIST(false, false);
#undef FP32_DIST
  LAUNCH_CHECK("k_distance");
  return STEIN_OK;
}

int stein_fp32_contract_partial(const StepViews& v, const BlockShape& b, const float* T, const float* G, const float* h2_dev,
                                hipStream_t s) {
  const SteinLayout& L = v.L;
  const long nblk = (long)L.tiles_m * 2 * L.cblocks * v.nsplit;
  if (nblk > 0x7fffffffl) return stein_fail(STEIN_E_SHAPE, "too many tiles");
  const bool vec = (b.d % 4 == 0) && (((uintptr_t)T & 15) == 0) && (((uintptr_t)G & 15) == 0);
  if (vec)
    hipLaunchKernelGGL(k_phi_partial<true>, dim3((unsigned)nblk), dim3(NTHREADS), 0, s, v.D, (long)L.ld_dist, G, T, h2_dev,
                       v.OG, v.OT, v.RS, (int)b.n, (int)b.d, (int)b.n_local, (int)L.tiles_m, (int)L.cblocks, v.nsplit, v.jchunk);
  else
    hipLaunchKernelGGL(k_phi_partial<false>, dim3((unsigned)nblk), dim3(NTHREADS), 0, s, v.D, (long)L.ld_dist, G, T, h2_dev,
                       v.OG, v.OT, v.RS, (int)b.n, (int)b.d, (int)b.n_local, (int)L.tiles_m, (int)L.cblocks, v.nsplit, v.jchunk);
  LAUNCH_CHECK("k_phi_partial");
  return STEIN_OK;
}
