// stein_boot.hip -- the quadratic forms of the KSD goodness-of-fit test without the n x n Stein-kernel matrix:
//   Q_b = sum_ij w_bi w_bj u_p(x_i, x_j)   for every row w_b of the caller's weights [reps][n]
// (include/steinhip.h, stein_ksd_boot).  The Stein-kernel matrix U is formed tile by tile in
// registers, split into hi + lo fp16 into the LDS image of the streaming step and contracted with ALL rows' weights at once:
// T = U Omega^T is accumulated per workgroup, multiplied by w_bi in the tail and reduced over its rows; nothing of size
// n x n or n x reps reaches memory.
//
//   stein_rownorms, k_colmax, k_make_scales, k_split (row-major image only)   as they are (stein_x3.hip), three times:
//                       theta -> T3;  the score-side operand M (RBF: W = G - theta / h2, IMQ: G) -> M3;  the weights, read as
//                       a matrix of reps "particles" x n "parameters" -> their row-major image, which IS the transposed image
//                       of Omega^T the contraction's B operand wants (rows = replicates, k = particles)
//   k_boot_canon        per row of weights: the row times the sign of its first nonzero entry.  Q_b is even in the row, but
//                       the matrix cores' accumulation is not sign-symmetric (observed: Q(-w) one ulp of a partial from
//                       Q(w)), so w and -w are made the SAME operand: negating a row leaves its bits unchanged by construction
//   k_boot_rows         per particle: b_i (RBF: g_i.x_i / h2 - r_i / (2 h2^2); IMQ: g_i.x_i), |m_i|^2, |g_i|^2 (fp64); RBF: row i of W
//   k_boot_scale        one workgroup: a bound on |u_p| -> the power-of-two scale of the image; sum_i u_p(i, i) -> diag_out;
//                       a non-finite per-row sum (a NaN or Inf in theta or the score) or h2 = 0 / NaN -> a NaN out-scale:
//                       every output is NaN (the element function's clamp would otherwise turn it into a finite +-60000)
//   k_ksd_boot<Kern>    the streaming kernel (below)
//   k_boot_sum          adds the (j range, row tile) partials of every replicate in fixed order in fp64 -> q_out
// stein_ksd_matmul (out = V U, the products Stein importance weights and control variates need) is the
// same sequence without k_boot_canon, with k_ksd_boot<Kern, true> -- the same j loop, whose tail stores the accumulators as
// this j range's partial of T instead of reducing them -- and k_boot_product_sum, which adds the ranges in fp64 -> out.
//
// k_ksd_boot: k_phi_stream's shape (stein_stream.hip).  A 512-thread workgroup owns 128 rows x one group of 256 weight
// columns (replicates) x one range of 128-column j tiles; the LDS image is double-buffered, one barrier per j tile.  Per tile:
//   Gram         S = T_j T_i^T (st_distance_tile), S1 = M_j M_i^T, and for the IMQ kernel S2 = T_j M_i^T + M_j T_i^T, the
//                symmetric cross term as ONE Gram of depth 2 d over the operands [g | x] and [x | g] -- which are the planes
//                already there, read in the other order
//   element      u_p from D (0 on the diagonal by a select), the Gram values and the per-particle b (RbfBoot / ImqBoot), times the image scale, clamped to the
//                fp16 range, columns j >= n forced to 0 by a select; hi + lo fp16 into the image (st_split4, st_stage4)
//   contraction  st_contract_ktile, unchanged: A the u image, B the weights' planes
// Tail: the wave's 128 x 32 accumulator times w_bi (the canonical floats), rows >= n masked by a select, summed over the
// rows: one float per (j range, row tile, replicate).  No atomics; every (range, tile, replicate < reps) slot is written
// by exactly one wave, so the result does not depend on what the workspace held and a repeated call is bit-identical.
// Every load is plain C++; no workgroup waits for another; every loop bound is an argument.

#include "stein_x3.h"

#include "stein_x3_dev.h"
#include "stein_stream_tile.h"

// ---- the element functions ---------------------------------------------------------------------------------------------
// u(dv, g1, g2, bi, bj): the Stein kernel of one pair from D, the Gram values and the two particles' b.
// RBF (h = h2, w = g - x / h, b_i = g_i.x_i / h - r_i / (2 h^2)):  u = k (w_i.w_j - D / (2 h^2) + b_i + b_j + d / h)
struct RbfBoot {
  static constexpr bool CROSS = false;
  static constexpr int ID = STEIN_KERNEL_RBF;
  float cexp, i2h2, dh;
  __device__ RbfBoot(float h2, int d) : cexp(-1.44269504088896341f / (2.f * h2)), i2h2(0.5f / (h2 * h2)), dh((float)d / h2) {}
  __device__ float u(float dv, float ww, float, float bi, float bj) const {
    const float k = __builtin_amdgcn_exp2f(cexp * dv);
    return k * ((ww - dv * i2h2) + (bi + bj) + dh);
  }
};
// IMQ (c2 = 2 h2, a_i = g_i.x_i):  u = k g_i.g_j + k^3 [ (a_i + a_j - cross) / c2 + d / c2 - 3 k^2 D / c2^2 ]
struct ImqBoot {
  static constexpr bool CROSS = true;
  static constexpr int ID = STEIN_KERNEL_IMQ;
  float ic2, dic2;
  __device__ ImqBoot(float h2, int d) : ic2(1.f / (2.f * h2)), dic2((float)d / (2.f * h2)) {}
  __device__ float u(float dv, float gg, float cross, float ai, float aj) const {
    dv = __builtin_fmaxf(dv, 0.f);
    const float e = dv * ic2;
    const float k = __builtin_amdgcn_rsqf(1.f + e);
    const float k2 = k * k;
    return k * gg + (k2 * k) * ((((ai + aj) - cross) * ic2 + dic2) - 3.f * k2 * e * ic2);
  }
};

// s += B_j A_i^T over ntk k tiles: st_distance_tile's loop without the zeroing (the cross term adds two Grams into one set)
__device__ __forceinline__ void boot_gram_add(const u16* __restrict__ ta, const u16* __restrict__ tb, int ntk, f32x4 (&s)[4][2]) {
  for (int kt = 0; kt < ntk; ++kt) {
    u32x4 fa[2][3], fb[4][3];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
#pragma unroll
      for (int ib = 0; ib < 2; ++ib)
        fa[ib][p] = *reinterpret_cast<const u32x4*>(ta + ((size_t)kt * 3 + p) * XTILE_E + ib * 512);
#pragma unroll
      for (int jb = 0; jb < 4; ++jb)
        fb[jb][p] = *reinterpret_cast<const u32x4*>(tb + ((size_t)kt * 3 + p) * XTILE_E + jb * 512);
    }
#pragma unroll
    for (int jb = 0; jb < 4; ++jb)
#pragma unroll
      for (int ib = 0; ib < 2; ++ib) s[jb][ib] = x3_products16<2>(fb[jb], fa[ib], s[jb][ib]);
  }
}

constexpr float BOOT_CLAMP = 60000.f;   // the scaled image stays inside fp16 (65504) whatever the rounding did to the bound

// st[0]: the image's in-scale 2^su; st[1]: the out-scale 2^-su / (the weights' in-scale)
// PRODUCT (stein_ksd_matmul): the same j loop with the other tail -- T itself is stored, `weights` is not read
template <class Kern, bool PRODUCT>
__global__ __launch_bounds__(ST_THREADS) void k_ksd_boot(const u16* __restrict__ T3, const u16* __restrict__ M3, int ntk,
                                                         const u16* __restrict__ Wt3, long ntj, const float* __restrict__ r,
                                                         const float* __restrict__ rowb, const float* __restrict__ sct,
                                                         const float* __restrict__ scm, int dc, const float* __restrict__ st,
                                                         const float* __restrict__ h2p, const float* __restrict__ weights,
                                                         float* __restrict__ part, int n, int d, int reps, int repsp,
                                                         int row_tiles, int col_groups, int cblocks, int jtiles,
                                                         int jtiles_per) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * ST_BUF];
  // column group fastest: the workgroups of one row tile are neighbours (same XCD, same panels in its L2)
  const int logical = xcd_remap(blockIdx.x, gridDim.x);
  const int cg = logical % col_groups;
  const int tile_m = (logical / col_groups) % row_tiles;
  const int z = logical / (col_groups * row_tiles);
  const int i0 = tile_m * ST_ROWS;
  const int jt0 = z * jtiles_per, jt1 = min(jtiles, jt0 + jtiles_per);

  const StRoles ro = st_roles();
  const int lane = ro.lane, w = ro.w, l15 = ro.l15, lq = ro.lq, wr = ro.wr, wc = ro.wc, wcol = ro.wcol;
  // contraction role: the 32 replicates at wcol of 128-column block g; a block past the last has nothing to contract
  const int g = 2 * cg + (w >> 2);
  const bool live = g < cblocks;
  const int gl = min(g, cblocks - 1);

  const Kern kern(*h2p, d);
  const float two_s = sct[4 * dc + 1];                       // x_i.x_j = S two_s / 2
  const float gm = 0.5f * scm[4 * dc + 1];                   // m_i.m_j = S1 gm
  const float gc = 1.f / (sct[4 * dc] * scm[4 * dc]);        // x_j.m_i + m_j.x_i = S2 gc (powers of two: exact)
  const float us = st[0];
  float ri[2], bi[2];
  int irow[2];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    irow[a] = i0 + wr * 32 + a * 16 + l15;
    ri[a] = r[i0 + wr * 32 + a * 16 + l15];      // (r and rowb are padded to the row tiles; rows >= n are masked in the tail)
    bi[a] = rowb[i0 + wr * 32 + a * 16 + l15];
  }

  f32x4 acc[8][2];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const size_t frag_i = (size_t)tile_m * ntk * 3 * XTILE_E + (wr * 2) * 512 + lane * 8;
  const u16* __restrict__ ta = T3 + frag_i;
  const u16* __restrict__ ma = M3 + frag_i;
  const u16* __restrict__ wb = Wt3 + (size_t)gl * ntj * 3 * XTILE_E + wcol * 32 + lane * 8;
  const int aoff = l15 * XROW + pswz(l15, lq);

  for (int jt = jt0; jt < jt1; ++jt) {
    unsigned char* buf = smem + ((jt - jt0) & 1) * ST_BUF;
    const int j0 = jt * ST_JT;
    // ---- Gram: S^T blocks [4 j blocks][2 i blocks] of this wave
    const size_t frag_j = (size_t)jt * ntk * 3 * XTILE_E + (wc * 4) * 512 + lane * 8;
    const u16* __restrict__ tb = T3 + frag_j;
    const u16* __restrict__ mb = M3 + frag_j;
    f32x4 s[4][2], s1[4][2], s2[4][2];
    st_distance_tile(ta, tb, ntk, s);
    st_distance_tile(ma, mb, ntk, s1);
    if constexpr (Kern::CROSS) {
      st_distance_tile(ma, tb, ntk, s2);   // x_j.m_i
      boot_gram_add(ta, mb, ntk, s2);      // + m_j.x_i
    }
    // ---- element function, split, stage: lane holds S^T[j = 16 jb + 4 lq + e][i = 16 ib + l15]
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) {
      const int jc = wc * 64 + jb * 16 + 4 * lq;          // first of this lane's 4 columns inside the tile
      const float4 rj4 = *reinterpret_cast<const float4*>(r + j0 + jc);      // (padded; columns >= n are masked below)
      const float4 bj4 = *reinterpret_cast<const float4*>(rowb + j0 + jc);
      const float rj[4] = {rj4.x, rj4.y, rj4.z, rj4.w};
      const float bj[4] = {bj4.x, bj4.y, bj4.z, bj4.w};
#pragma unroll
      for (int ib = 0; ib < 2; ++ib) {
        float q[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          // D_ii = 0, not the rounding error of r_i + r_i - 2 x_i.x_i: one ulp of 2 r_i there moves k by r_i 2^-23 / (2 h2),
          // 0.2 % of u_ii for a particle 100 sigma out, whose diagonal term is all it contributes
          const float dv = (j0 + jc + e == irow[ib]) ? 0.f : (ri[ib] + rj[e]) - two_s * s[jb][ib][e];
          float g2 = 0.f;
          if constexpr (Kern::CROSS) g2 = gc * s2[jb][ib][e];
          const float uv = kern.u(dv, gm * s1[jb][ib][e], g2, bi[ib], bj[e]) * us;
          // (masked by a select: r's padding, and with it dv, may hold anything there, NaN included)
          q[e] = (j0 + jc + e < n) ? __builtin_amdgcn_fmed3f(uv, -BOOT_CLAMP, BOOT_CLAMP) : 0.f;
        }
        const StSplit4 p = st_split4(q);
        st_stage4(st_image_dst(buf, wr * 32 + ib * 16 + l15, jc), p);
      }
    }
    __syncthreads();
    // ---- contraction: T += U . Omega_j^T over the tile's (up to) four 32-deep k tiles
    for (int kt = 0; live && kt < ST_JT / 32; ++kt) {
      if (j0 + kt * 32 >= n) break;   // the image is zero there
      st_contract_ktile(acc, buf + kt * ST_KTB + aoff, wb + ((size_t)jt * (ST_JT / 32) + kt) * 3 * XTILE_E);
    }
  }

  if (!live) return;
  if constexpr (PRODUCT) {
    // ---- tail: this j range's partial of T, part[z][b][row]: one float per (j range, replicate, row < n).  A lane holds four
    // consecutive rows: one 16-byte store (the rows are padded to the tiles and the block is 256-byte aligned) unless they
    // straddle n, where the rows < n go out one by one; rows >= n and replicates >= reps are not written
    const size_t rows = (size_t)row_tiles * ST_ROWS;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int b = g * 128 + wcol + j * 16 + l15;
      if (b >= reps) continue;
      float* __restrict__ dst = part + ((size_t)z * repsp + b) * rows;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int row = i0 + i * 16 + 4 * lq;
        if (row + 3 < n) {
          *reinterpret_cast<f32x4*>(dst + row) = acc[i][j];
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (row + e < n) dst[row + e] = acc[i][j][e];
        }
      }
    }
    return;
  }
  // ---- tail: sum_i w_bi T_ib over this tile's rows, one float per (j range, row tile, replicate)
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int b = g * 128 + wcol + j * 16 + l15;
    const float* __restrict__ wrow = weights + (size_t)min(b, reps - 1) * n;
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = i0 + i * 16 + 4 * lq + e;
        const bool in = row < n;
        t = __builtin_fmaf(in ? acc[i][j][e] : 0.f, in ? wrow[row] : 0.f, t);
      }
    t += __shfl_xor(t, 16);
    t += __shfl_xor(t, 32);
    if (lq == 0 && b < reps) part[((size_t)z * row_tiles + tile_m) * repsp + b] = t;
  }
}

// ---- per particle: b_i, |m_i|^2 (for the bound), |g_i|^2 in fp64 (for the diagonal); RBF: row i of W ------------------------
// One wave per row; rows n .. rows - 1 of rowb / rown are written zero (the kernel reads them as the padding of a j tile).
template <int KERNEL>
__global__ __launch_bounds__(256) void k_boot_rows(const float* __restrict__ T, const float* __restrict__ G,
                                                   const float* __restrict__ r, const float* __restrict__ h2p,
                                                   float* __restrict__ W, float* __restrict__ rowb, float* __restrict__ rown,
                                                   double* __restrict__ rowdiag, int n, int d, int rows) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  if (row >= n) {
    if (lane == 0) { rowb[row] = 0.f; rown[row] = 0.f; rowdiag[row] = 0.0; }
    return;
  }
  const float ih = 1.f / *h2p;
  const float* __restrict__ th = T + (size_t)row * d;
  const float* __restrict__ gr = G + (size_t)row * d;
  float gx = 0.f, mm = 0.f;
  double gg = 0.0;
  for (int c = lane; c < d; c += 64) {
    const float x = th[c], gv = gr[c];
    gx = __builtin_fmaf(gv, x, gx);
    gg += (double)gv * (double)gv;
    if (KERNEL == STEIN_KERNEL_RBF) {
      const float wv = __builtin_fmaf(-x, ih, gv);
      W[(size_t)row * d + c] = wv;
      mm = __builtin_fmaf(wv, wv, mm);
    } else {
      mm = __builtin_fmaf(gv, gv, mm);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    gx += __shfl_xor(gx, o);
    mm += __shfl_xor(mm, o);
    gg += __shfl_xor(gg, o);
  }
  if (lane == 0) {
    rowb[row] = KERNEL == STEIN_KERNEL_RBF ? gx * ih - 0.5f * r[row] * ih * ih : gx;
    rown[row] = mm;
    rowdiag[row] = gg;
  }
}

// ---- per row of weights: the canonical sign (one wave per row) ------------------------------------------------------------
// Wc[b] = s_b W[b], s_b = the sign of the first nonzero entry of the row (1 for a row of zeros).  Exact; w and -w give the
// same Wc, and everything downstream (the split, the contraction, the tail) reads Wc.
__global__ __launch_bounds__(256) void k_boot_canon(const float* __restrict__ W, float* __restrict__ Wc, int n, int reps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= reps) return;
  const float* __restrict__ w = W + (size_t)row * n;
  int first = n;
  for (int i = lane; i < n; i += 64)
    if (w[i] != 0.f) { first = i; break; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o));
  const float sgn = (first < n && (__float_as_uint(w[first]) >> 31)) ? -1.f : 1.f;
  for (int i = lane; i < n; i += 64) Wc[(size_t)row * n + i] = sgn * w[i];
}

// ---- one workgroup: the image's scale from a bound on |u_p|, and the diagonal sum ---------------------------------------------
// RBF: |u| <= max|w|^2 + 2 max|b| + (d + 1) / h2   (k <= 1, k D / (2 h2^2) <= 1 / (e h2))
// IMQ: |u| <= max|g|^2 + max|g| / sqrt(c2) + (d + 3) / c2   (k^3 sqrt(D) / c2 <= 0.385 / sqrt(c2), k^5 D / c2 <= 1)
// The scale puts the bound into [2^13, 2^14): the image's entries stay below 2^14 and an entry's absolute error is 2^-25 of
// the scaled unit, 2^-38 of the bound.
template <int KERNEL>
__global__ __launch_bounds__(256) void k_boot_scale(const float* __restrict__ rown, const float* __restrict__ rowb,
                                                    const float* __restrict__ r, const double* __restrict__ rowdiag, const float* __restrict__ h2p,
                                                    const float* __restrict__ scw_all, float* __restrict__ st,
                                                    double* __restrict__ diag_out, int n, int d) {
  __shared__ float mx[2][256];
  __shared__ double red[4];
  const int t = threadIdx.x;
  float mn = 0.f, mb = 0.f;
  double dg[1] = {0.0};
  // fmaxf drops a NaN: a row whose |m_i|^2 or b_i is NaN counts as +inf, so that the bound sees it (below)
  auto seen = [](float v) { return v == v ? v : __builtin_inff(); };
  for (int i = t; i < n; i += 256) {
    mn = fmaxf(mn, seen(rown[i]));
    mb = fmaxf(mb, seen(fabsf(rowb[i])));
    if (!(r[i] < __builtin_inff())) mb = __builtin_inff();   // |x_i|^2 beyond fp32 (or NaN): D, and with it k, is lost
    dg[0] += rowdiag[i];
  }
  mx[0][t] = mn;
  mx[1][t] = mb;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
      mx[0][t] = fmaxf(mx[0][t], mx[0][t + o]);
      mx[1][t] = fmaxf(mx[1][t], mx[1][t + o]);
    }
    __syncthreads();
  }
  block_sum256(dg, red);
  if (t == 0) {
    const float h2 = *h2p;
    const float ih = KERNEL == STEIN_KERNEL_RBF ? 1.f / h2 : 0.5f / h2;   // 1 / h2 or 1 / c2
    const float bound = KERNEL == STEIN_KERNEL_RBF ? mx[0][0] + 2.f * mx[1][0] + (float)(d + 1) * ih
                                                   : mx[0][0] + sqrtf(mx[0][0] * ih) + (float)(d + 3) * ih;
    const int se = scale_exp(__float_as_uint(bound), 100);
    // A non-finite theta or score entry makes its row's |m_i|^2, b_i or r_i non-finite (k_boot_rows, stein_rownorms), h2 = 0
    // or NaN the bound itself.  The element function would clamp such an entry into the image as a finite value, so the OUT-scale is
    // poisoned here, off the j loop: every q_out[b] / out[b][i] and diag_out come out NaN (include/steinhip.h).
    // (the IMQ bound does not hold max |b_i| = max |g_i.x_i|, the one per-row sum of that kernel theta enters: it is asked too)
    const bool finite = bound < __builtin_inff() && mx[1][0] < __builtin_inff();
    const float nan = __uint_as_float(0x7fc00000u);
    st[0] = pow2i(se);
    st[1] = finite ? pow2i(-se) / *scw_all : nan;
    if (diag_out)
      *diag_out = finite ? dg[0] + (double)n * (double)d * (KERNEL == STEIN_KERNEL_RBF ? 1.0 : 0.5) / (double)h2 : (double)nan;
  }
}

// ---- the partials of every replicate in fixed order (j range, then row tile) in fp64, unscaled -> q_out --------------------
__global__ __launch_bounds__(256) void k_boot_sum(const float* __restrict__ part, const float* __restrict__ st, int slots,
                                                  int repsp, int reps, double* __restrict__ q_out) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= reps) return;
  double s = 0.0;
  for (int k = 0; k < slots; ++k) s += (double)part[(size_t)k * repsp + b];
  q_out[b] = s * (double)st[1];
}

// ---- stein_ksd_matmul: the j ranges' partials of T in range order in fp64, unscaled -> out [reps][n] as float ----------------
__global__ __launch_bounds__(256) void k_boot_product_sum(const float* __restrict__ part, const float* __restrict__ st, int jsplit,
                                                          int repsp, long rows, int n, long total, float* __restrict__ out) {
  const double os = (double)st[1];
  for (long at = blockIdx.x * 256L + threadIdx.x; at < total; at += gridDim.x * 256L) {
    const long b = at / n, i = at - b * n;
    double s = 0.0;
    for (int z = 0; z < jsplit; ++z) s += (double)part[((size_t)z * repsp + b) * rows + i];
    out[at] = (float)(s * os);
  }
}

// ================================================================================================
// host side
// ================================================================================================
static thread_local int g_boot_jsplit = 0;   // stein_debug_boot_jsplit: 0 = the plan's own rule

extern "C" int stein_debug_boot_jsplit(int jsplit) {
  if (jsplit < 0) return fail(STEIN_E_BADARG, "jsplit < 0");
  g_boot_jsplit = jsplit;
  return STEIN_OK;
}

// r | theta's scales | T3 | W (RBF) | M's scales | M3 | the weights' scales | their planes | b | |m|^2 | |g|^2 | state | partials |
// the sign-canonical weights
struct BootLayout {
  int64_t row_tiles, col_groups, cblocks, jsplit, jtiles_per;
  int64_t rows, dk, dc, repsc, repsp;
  size_t r, sct, t3, w, scm, m3, scw, w3, rowb, rown, rowdiag, st, part, wc, total;
};

static int boot_check_shape(int64_t n, int64_t d, int64_t reps, int dtype, int flags, const char* who = "stein_ksd_boot") {
  if (dtype == STEIN_BF16 || dtype == STEIN_F64)
    return fail(STEIN_E_UNSUPPORTED, "%s takes fp32 inputs (STEIN_F32), not bf16 or f64", who);
  if (dtype != STEIN_F32) return fail(STEIN_E_UNSUPPORTED, "dtype %d", dtype);
  if (flags != 0) return fail(STEIN_E_BADARG, "%s takes no flags, got 0x%x", who, flags);
  if (n < 2 || d < 1) return fail(STEIN_E_SHAPE, "bad shape n=%lld d=%lld: need n >= 2 and d >= 1", (long long)n, (long long)d);
  if (reps < 1) return fail(STEIN_E_SHAPE, "bad replicate count reps=%lld: need reps >= 1", (long long)reps);
  if (int rc = stein_check_size(n, d)) return rc;
  return stein_check_size(reps, n);   // the weights are split as a reps x n matrix
}

// The plan: one workgroup per (row tile, group of 256 replicates, j range); the j ranges fill the resident grid by the
// streaming step's rule (stream_make_layout) with the replicate groups in the place of its column groups.
// product (stein_ksd_matmul): the partial block holds T itself, [jsplit][repsp][rows], and there are no canonical weights.
static int boot_make_layout(int64_t n, int64_t d, int64_t reps, BootLayout* L, bool product = false) {
  *L = BootLayout{};
  L->row_tiles = (n + ST_ROWS - 1) / ST_ROWS;
  L->cblocks = (reps + 127) / 128;
  L->col_groups = (reps + 255) / 256;
  const int64_t jtiles = L->row_tiles;
  int64_t want = g_boot_jsplit > 0 ? g_boot_jsplit : (int64_t)(RESIDENT_ONE_PER_CU / (double)(L->row_tiles * L->col_groups));
  if (want < 1) want = 1;
  if (want > jtiles) want = jtiles;
  L->jtiles_per = (jtiles + want - 1) / want;
  L->jsplit = (jtiles + L->jtiles_per - 1) / L->jtiles_per;
  L->rows = L->row_tiles * ST_ROWS;
  L->dk = (int64_t)align_up((size_t)d, 32);
  L->dc = (int64_t)align_up((size_t)d, 128);
  L->repsc = L->cblocks * 128;
  L->repsp = (int64_t)align_up((size_t)reps, 32);
  size_t at = 0;
  auto put = [&](size_t bytes) { const size_t o = at; at = align_up(at + bytes, 256); return o; };
  L->r = put((size_t)L->rows * 4);
  L->sct = put((size_t)(6 * L->dc + 4) * 4);
  L->t3 = put((size_t)3 * L->rows * L->dk * 2);
  L->w = put((size_t)n * d * 4);
  L->scm = put((size_t)(6 * L->dc + 4) * 4);
  L->m3 = put((size_t)3 * L->rows * L->dk * 2);
  L->scw = put((size_t)(6 * L->rows + 4) * 4);
  L->w3 = put((size_t)3 * L->repsc * L->rows * 2);
  L->rowb = put((size_t)L->rows * 4);
  L->rown = put((size_t)L->rows * 4);
  L->rowdiag = put((size_t)L->rows * 8);
  L->st = put(256);
  L->part = put((size_t)L->jsplit * (product ? L->rows : L->row_tiles) * L->repsp * 4);
  L->wc = put(product ? 0 : (size_t)reps * n * 4);
  L->total = at;
  if (L->row_tiles * L->col_groups * L->jsplit > 0x7fffffffll) return fail(STEIN_E_SHAPE, "too many tiles");
  return STEIN_OK;
}

extern "C" int stein_ksd_boot_workspace_bytes(int64_t n, int64_t d, int64_t reps, int dtype, int flags, size_t* out_bytes) {
  if (!out_bytes) return fail(STEIN_E_BADARG, "out_bytes is NULL");
  int rc = boot_check_shape(n, d, reps, dtype, flags);
  if (rc) return rc;
  BootLayout L;
  if ((rc = boot_make_layout(n, d, reps, &L))) return rc;
  *out_bytes = L.total;
  return STEIN_OK;
}

extern "C" int stein_ksd_boot_plan(int64_t n, int64_t d, int64_t reps, int* row_tiles, int* col_groups, int* jsplit) {
  if (!row_tiles || !col_groups || !jsplit) return fail(STEIN_E_BADARG, "NULL output");
  int rc = boot_check_shape(n, d, reps, STEIN_F32, 0);
  if (rc) return rc;
  BootLayout L;
  if ((rc = boot_make_layout(n, d, reps, &L))) return rc;
  *row_tiles = (int)L.row_tiles;
  *col_groups = (int)L.col_groups;
  *jsplit = (int)L.jsplit;
  return STEIN_OK;
}

// The views the split launchers take for one row-major image of an [rows_in][cols_in] matrix: planes at `planes`, scales area
// at `sc` (column maxima behind it), padded to prow x pcol (pcol a multiple of 128: the scales area is sized by it)
static StepViews boot_split_views(char* ws, size_t sc, size_t planes, int64_t prow, int64_t pk, int64_t pcol) {
  StepViews v{};
  v.L.x3_rows = prow; v.L.x3_nk = prow; v.L.x3_dk = pk; v.L.x3_dc = pcol;
  v.planes = ws;
  v.T3 = (unsigned short*)(ws + planes);
  v.sc = (float*)(ws + sc);
  v.cmax = (u32*)(v.sc + x3_sc_cmax(pcol));
  v.two_s = v.sc + x3_sc_two_s(pcol);
  return v;
}

// One matrix -> its scales and row-major planes (no second matrix: its half of the column maxima is zeroed here, as the
// streaming median does, so that k_make_scales reads nothing the workspace held)
static int boot_split_one(const StepViews& v, const void* X, int64_t rows_in, int64_t cols_in, hipStream_t s) {
  HIP_TRY(hipMemsetAsync(v.cmax, 0, (size_t)v.L.x3_dc * sizeof(u32), s));
  const SplitFused only_rows{nullptr, nullptr, 1};
  return stein_x3_split(v, X, nullptr, STEIN_F32, rows_in, cols_in, s, &only_rows);
}

// PRODUCT: `weights` is V, contracted as given (no canonical sign), and T goes to prod_out [reps][n]; q_out, diag_out unused
template <class Kern, bool PRODUCT = false>
static int boot_launch(const BootLayout& L, char* ws, const float* theta, const float* score, int64_t n, int64_t d,
                       const float* h2_in, const float* weights, int64_t reps, double* q_out, double* diag_out, hipStream_t s,
                       float* prod_out = nullptr) {
  float* r = (float*)(ws + L.r);
  float* W = (float*)(ws + L.w);
  float* rowb = (float*)(ws + L.rowb);
  float* rown = (float*)(ws + L.rown);
  double* rowdiag = (double*)(ws + L.rowdiag);
  float* st = (float*)(ws + L.st);
  float* part = (float*)(ws + L.part);
  const float* Wc = weights;
  int rc;
  // 1. row norms; theta's scales and planes (the score only feeds column maxima nothing here reads)
  if ((rc = stein_rownorms(theta, n, d, STEIN_F32, r, (void*)s))) return rc;
  const StepViews vt = boot_split_views(ws, L.sct, L.t3, L.rows, L.dk, L.dc);
  const SplitFused only_rows{nullptr, nullptr, 1};
  if ((rc = stein_x3_split(vt, theta, score, STEIN_F32, n, d, s, &only_rows))) return rc;
  // 2. per particle: b, |m|^2, |g|^2; RBF: W
  hipLaunchKernelGGL(k_boot_rows<Kern::ID>, dim3((unsigned)((L.rows + 3) / 4)), dim3(256), 0, s, theta, score, r, h2_in, W, rowb,
                     rown, rowdiag, (int)n, (int)d, (int)L.rows);
  LAUNCH_CHECK("k_boot_rows");
  // 3. the score-side operand's planes; 4. the weights in canonical sign, their planes: [reps][n] row-major = the transposed image of Omega^T
  const StepViews vm = boot_split_views(ws, L.scm, L.m3, L.rows, L.dk, L.dc);
  if ((rc = boot_split_one(vm, Kern::ID == STEIN_KERNEL_RBF ? W : score, n, d, s))) return rc;
  const StepViews vw = boot_split_views(ws, L.scw, L.w3, L.repsc, L.rows, L.rows);
  if (!PRODUCT) {
    float* canon = (float*)(ws + L.wc);
    hipLaunchKernelGGL(k_boot_canon, dim3((unsigned)((reps + 3) / 4)), dim3(256), 0, s, weights, canon, (int)n, (int)reps);
    LAUNCH_CHECK("k_boot_canon");
    Wc = canon;
  }
  if ((rc = boot_split_one(vw, Wc, reps, n, s))) return rc;
  // 5. the image's scale (after the weights' scale exists), the diagonal sum
  hipLaunchKernelGGL(k_boot_scale<Kern::ID>, dim3(1), dim3(256), 0, s, rown, rowb, r, rowdiag, h2_in, vw.sc + 4 * L.rows, st, diag_out,
                     (int)n, (int)d);
  LAUNCH_CHECK("k_boot_scale");
  // 6. the streaming kernel; 7. the partials in fixed order
  const unsigned nblk = (unsigned)(L.row_tiles * L.col_groups * L.jsplit);
  hipLaunchKernelGGL((k_ksd_boot<Kern, PRODUCT>), dim3(nblk), dim3(ST_THREADS), 0, s, vt.T3, vm.T3, (int)(L.dk / 32), vw.T3,
                     (long)(L.rows / 32), r, rowb, vt.sc, vm.sc, (int)L.dc, st, h2_in, Wc, part, (int)n, (int)d, (int)reps,
                     (int)L.repsp, (int)L.row_tiles, (int)L.col_groups, (int)L.cblocks, (int)L.row_tiles, (int)L.jtiles_per);
  LAUNCH_CHECK("k_ksd_boot");
  if (PRODUCT) {
    const long total = (long)reps * (long)n;
    hipLaunchKernelGGL(k_boot_product_sum, dim3((unsigned)grid_for(total, 1 << 20)), dim3(256), 0, s, part, st,
                       (int)L.jsplit, (int)L.repsp, (long)L.rows, (int)n, total, prod_out);
    LAUNCH_CHECK("k_boot_product_sum");
    return STEIN_OK;
  }
  hipLaunchKernelGGL(k_boot_sum, dim3((unsigned)((reps + 255) / 256)), dim3(256), 0, s, part, st,
                     (int)(L.jsplit * L.row_tiles), (int)L.repsp, (int)reps, q_out);
  LAUNCH_CHECK("k_boot_sum");
  return STEIN_OK;
}

extern "C" int stein_ksd_boot(const void* theta, const void* score, int64_t n, int64_t d, int dtype, const float* h2_in,
                              int kernel, const float* weights, int64_t reps, double* q_out, double* diag_out, void* workspace,
                              size_t ws_bytes, int flags, void* stream) {
  if (!theta || !score || !h2_in || !weights || !q_out || !workspace) return fail(STEIN_E_BADARG, "NULL pointer");
  if ((uintptr_t)workspace & 15) return fail(STEIN_E_BADARG, "the workspace must be 16-byte aligned");
  int rc = boot_check_shape(n, d, reps, dtype, flags);
  if (rc) return rc;
  if (kernel != STEIN_KERNEL_RBF && kernel != STEIN_KERNEL_IMQ) return fail(STEIN_E_BADARG, "unknown kernel id %d", kernel);
  BootLayout L;
  if ((rc = boot_make_layout(n, d, reps, &L))) return rc;
  if (ws_bytes < L.total) return fail(STEIN_E_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, L.total);
  if ((rc = stein_take_device_error())) return rc;
  const hipStream_t s = (hipStream_t)stream;
  if (kernel == STEIN_KERNEL_RBF)
    return boot_launch<RbfBoot>(L, (char*)workspace, (const float*)theta, (const float*)score, n, d, h2_in, weights, reps, q_out,
                                diag_out, s);
  return boot_launch<ImqBoot>(L, (char*)workspace, (const float*)theta, (const float*)score, n, d, h2_in, weights, reps, q_out,
                              diag_out, s);
}

// ---- stein_ksd_matmul: out = V U, the same launches with the product tail --------------------------------------------------
extern "C" int stein_ksd_matmul_workspace_bytes(int64_t n, int64_t d, int64_t reps, int dtype, int flags, size_t* out_bytes) {
  if (!out_bytes) return fail(STEIN_E_BADARG, "out_bytes is NULL");
  int rc = boot_check_shape(n, d, reps, dtype, flags, "stein_ksd_matmul");
  if (rc) return rc;
  BootLayout L;
  if ((rc = boot_make_layout(n, d, reps, &L, true))) return rc;
  *out_bytes = L.total;
  return STEIN_OK;
}

extern "C" int stein_ksd_matmul(const void* theta, const void* score, int64_t n, int64_t d, int dtype, const float* h2_in,
                                int kernel, const float* V, int64_t reps, float* out, void* workspace, size_t ws_bytes, int flags,
                                void* stream) {
  if (!theta || !score || !h2_in || !V || !out || !workspace) return fail(STEIN_E_BADARG, "NULL pointer");
  if ((uintptr_t)workspace & 15) return fail(STEIN_E_BADARG, "the workspace must be 16-byte aligned");
  int rc = boot_check_shape(n, d, reps, dtype, flags, "stein_ksd_matmul");
  if (rc) return rc;
  if (kernel != STEIN_KERNEL_RBF && kernel != STEIN_KERNEL_IMQ) return fail(STEIN_E_BADARG, "unknown kernel id %d", kernel);
  BootLayout L;
  if ((rc = boot_make_layout(n, d, reps, &L, true))) return rc;
  if (ws_bytes < L.total) return fail(STEIN_E_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, L.total);
  if ((rc = stein_take_device_error())) return rc;
  const hipStream_t s = (hipStream_t)stream;
  if (kernel == STEIN_KERNEL_RBF)
    return boot_launch<RbfBoot, true>(L, (char*)workspace, (const float*)theta, (const float*)score, n, d, h2_in, V, reps, nullptr,
                                      nullptr, s, out);
  return boot_launch<ImqBoot, true>(L, (char*)workspace, (const float*)theta, (const float*)score, n, d, h2_in, V, reps, nullptr,
                                    nullptr, s, out);
}
