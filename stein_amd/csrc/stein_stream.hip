// stein_stream.hip -- the SVGD direction at a bandwidth the caller supplies, without the n x n distance image.
//
// With h2 known before the step starts nothing needs all of D at once: the folded operand W = G - theta / h2 (stein_x3.hip,
// "folded operand") is built first, and a tile of D is exponentiated and contracted with W the moment its accumulators are
// complete, then dropped.  The workspace is O(n d): row norms, scales, theta's row-major planes, W's transposed planes and
// the partial sums (stein_stream_make_layout below).
//
//   stein_rownorms, k_colmax, k_make_scales, k_split (theta, row-major image only), k_split_w   as they are (stein_x3.hip)
//   k_phi_stream        distance tile -> P = exp2(c D + 14) -> O += P.W, running rowsum(P); D and K never reach memory
//   k_stream_finish     sums the j ranges in order, phi = (K.W + rowsum(K) theta / h2) / n, |phi|^2 block partials (fp64)
//   k_stream_sqsum      one workgroup: the block partials -> sqnorm_out
// stein_svgd_phi_stream_ksd, the step with the Stein discrepancy sums at its own bandwidth (include/steinhip.h), launches
// the KSD forms of the same bodies: k_phi_stream_ksd (a second running row sum, rd = rowsum(P o D)), k_stream_finish_ksd
// (reads the score rows too; three sets of block partials) and k_stream_sqsum3.  No K.theta, no further column space.
// The P image's swizzle, the fp16 split and the exponent offset (pswz, cvt_pk_f16, f16_resid_lo / _hi, PEXP_H2) are
// stein_x3_dev.h's, the ones the stored-D contraction uses; the size limits, align_up and the resident-workgroup count are
// stein_host.h's, shared with stein_make_layout.  The finish pass stays a kernel of this file although k_phi_finish's FOLD
// form (steinhip.hip) gives the same bits: at 8 j ranges that kernel takes its generic loop and the step measured slower
// ("streaming step").
//
// k_phi_stream: a 512-thread workgroup (8 waves, two per SIMD) owns 128 rows of particles x one column group of W (two
// 128-column blocks) x one range of 128-column j tiles.  Per j tile:
//   distance     wave w computes the 32 rows x 64 columns (w >> 1, w & 1) of S^T = T_j T_i^T on 16x16x32 fp16 MFMAs, three
//                products per fragment pair (x3_products16), both operands read in fragment order straight from theta's
//                planes T3 (1 KB coalesced loads; the row tile's panel stays in the L2).  Transposed, so that a lane
//                holds FOUR CONSECUTIVE j of one row i: one 8-byte LDS store per plane.
//   exp / split  D = (r_i + r_j) - two_s S, P = exp2(c D + 14), columns j >= n forced to 0, hi = fp16(P), lo = fp16(P - hi)
//                into the LDS image the stored-D contraction uses ([k tile][plane][128 rows][64 B], pswz); rowsum += P
//   barrier      (one per j tile: the P image is double-buffered)
//   contraction  wave w owns all 128 rows x the 32 columns (w & 3) of 128-column block w >> 2: A fragments (P) by
//                ds_read_b128, B fragments (W) by coalesced 1 KB loads from W's planes, three products each
// Every load is plain C++ (the compiler counts its own waits); no workgroup waits for another; every loop bound is an
// argument.  The partial sums of the j ranges go to [jsplit][n][d] / [jsplit][n] and are added in range order by the finish
// pass: no float atomics, a repeated call is bit-identical.
// Resources (hipcc, gfx950): recorded in DESIGN.md, "streaming step".
//
// The streaming median (stein_stream_median): the exact median-heuristic bandwidth of the same particles in the same O(n d)
// workspace.  The n^2 distances are never stored: the 3-level radix select of stein_select.hip (11 + 11 + 10 key bits)
// recomputes the distance tiles once per level and counts them straight from the MFMA accumulators.
//   stein_rownorms, k_colmax, k_make_scales, k_split (theta, row-major image only)   as in the step: the same r, T3, two_s
//   k_sel_init, then per level:  k_stream_hist<LEVEL>  distance tile -> digit of LEVEL -> LDS histogram -> one flush
//                                k_resolve             (stein_select.hip) -> prefixes; level 2: lo, hi, median, h2
// k_stream_hist runs the distance phase of k_phi_stream (st_distance_tile, stein_stream_tile.h: one body for both), so the median is the
// median of the D values the step exponentiates.

#include "stein_x3.h"

#include "stein_x3_dev.h"

// the tile geometry (ST_THREADS, ST_ROWS, ST_JT, ST_PLN, ST_KTB, ST_BUF) and the distance phase st_distance_tile, shared by
// k_phi_stream and k_stream_hist here and by k_phi_imq (stein_imq.hip)
#include "stein_stream_tile.h"

constexpr int ST_COLS = 256;              // columns of W per column group

// The body of k_phi_stream (KSD = false) and of k_phi_stream_ksd (KSD = true: also rd_i = sum_j P_ij D_ij, the second row sum
// the Stein discrepancy needs -- include/steinhip.h, stein_svgd_phi_stream_ksd -- carried beside rs, reduced like rs and
// written to RD like RS).  smem: the kernel's 2 x ST_BUF bytes of LDS.
template <bool KSD>
__device__ __forceinline__ void phi_stream_body(unsigned char* smem, const u16* __restrict__ T3, int ntk,
                                                const u16* __restrict__ Wt3, long ntj, const float* __restrict__ r,
                                                const float* __restrict__ sc, int dc, const float* __restrict__ h2p,
                                                float* __restrict__ O, float* __restrict__ RS, float* __restrict__ RD, int n,
                                                int d, int row_tiles, int col_groups, int cblocks, int jtiles,
                                                int jtiles_per) {
  // column group fastest: the workgroups of one row tile are neighbours (same XCD, same T panels in its L2)
  const int logical = xcd_remap(blockIdx.x, gridDim.x);
  const int cg = logical % col_groups;
  const int tile_m = (logical / col_groups) % row_tiles;
  const int z = logical / (col_groups * row_tiles);
  const int i0 = tile_m * ST_ROWS;
  const int jt0 = z * jtiles_per, jt1 = min(jtiles, jt0 + jtiles_per);

  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  // distance role: rows [32 wr, 32 wr + 32) x columns [64 wc, 64 wc + 64) of the 128 x 128 tile
  const int wr = w >> 1, wc = w & 1;
  // contraction role: all 128 rows x 32 columns at wcol of 128-column block g.  A block past the matrix's last (an odd block
  // count: d <= 128, or the last column group) has nothing to contract: its four waves only take part in the distance
  // tiles and the barriers (wave-uniform test)
  const int g = 2 * cg + (w >> 2);
  const bool live = g < cblocks;
  const int gl = min(g, cblocks - 1);
  const int wcol = (w & 3) * 32;

  const float cexp = -1.44269504088896341f / (2.f * *h2p);   // exp(-D / (2 h2)) = exp2(cexp D)
  const float two_s = sc[4 * dc + 1];
  float ri[2];
#pragma unroll
  for (int a = 0; a < 2; ++a) ri[a] = r[i0 + wr * 32 + a * 16 + l15];   // (r is padded to the row tiles; rows >= n are never stored)
  float rs[2] = {0.f, 0.f};
  float rd[2] = {0.f, 0.f};   // (KSD)

  f32x4 acc[8][2];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const u16* __restrict__ ta = T3 + (size_t)tile_m * ntk * 3 * XTILE_E + (wr * 2) * 512 + lane * 8;
  const u16* __restrict__ wb = Wt3 + (size_t)gl * ntj * 3 * XTILE_E + wcol * 32 + lane * 8;
  const int aoff = l15 * XROW + pswz(l15, lq);

  for (int jt = jt0; jt < jt1; ++jt) {
    unsigned char* buf = smem + ((jt - jt0) & 1) * ST_BUF;
    const int j0 = jt * ST_JT;
    // ---- distance: S^T block [4 j blocks][2 i blocks] of this wave
    f32x4 s[4][2];
    const u16* __restrict__ tb = T3 + (size_t)jt * ntk * 3 * XTILE_E + (wc * 4) * 512 + lane * 8;
    st_distance_tile(ta, tb, ntk, s);
    // ---- exp, split, stage: lane holds S^T[j = 16 jb + 4 lq + e][i = 16 ib + l15]
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) {
      const int jc = wc * 64 + jb * 16 + 4 * lq;          // first of this lane's 4 columns inside the tile
      const float4 rj4 = *reinterpret_cast<const float4*>(r + j0 + jc);   // (padded; columns >= n are masked below)
      const float rj[4] = {rj4.x, rj4.y, rj4.z, rj4.w};
#pragma unroll
      for (int ib = 0; ib < 2; ++ib) {
        float q[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float dv = (ri[ib] + rj[e]) - two_s * s[jb][ib][e];
          q[e] = __builtin_amdgcn_exp2f(__builtin_fmaf(cexp, dv, (float)PEXP_H2));
          q[e] = (j0 + jc + e < n) ? q[e] : 0.f;
          // (the product is masked by itself: r's padding, and with it dv, may hold anything there, NaN included)
          if constexpr (KSD) rd[ib] = __builtin_fmaf(q[e], (j0 + jc + e < n) ? dv : 0.f, rd[ib]);
        }
        rs[ib] += (q[0] + q[1]) + (q[2] + q[3]);
        const u32 h0 = cvt_pk_f16(q[0], q[1]), h1 = cvt_pk_f16(q[2], q[3]);
        const u32 o0 = cvt_pk_f16(f16_resid_lo(h0, q[0]), f16_resid_hi(h0, q[1]));
        const u32 o1 = cvt_pk_f16(f16_resid_lo(h1, q[2]), f16_resid_hi(h1, q[3]));
        const int row = wr * 32 + ib * 16 + l15;
        unsigned char* dst = buf + (jc >> 5) * ST_KTB + row * XROW + pswz(row, (jc & 31) >> 3) + (jc & 4) * 2;
        *reinterpret_cast<uint2*>(dst) = make_uint2(h0, h1);
        *reinterpret_cast<uint2*>(dst + ST_PLN) = make_uint2(o0, o1);
      }
    }
    __syncthreads();
    // ---- contraction: O += P . W_j over the tile's (up to) four 32-deep k tiles
    for (int kt = 0; live && kt < ST_JT / 32; ++kt) {
      if (j0 + kt * 32 >= n) break;   // P is zero there
      u32x4 b[2][3];
      const u16* __restrict__ src = wb + ((size_t)jt * (ST_JT / 32) + kt) * 3 * XTILE_E;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int p = 0; p < 2; ++p) b[j][p] = *reinterpret_cast<const u32x4*>(src + p * XTILE_E + j * 512);
      const unsigned char* As = buf + kt * ST_KTB + aoff;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        u32x4 a[3];
#pragma unroll
        for (int p = 0; p < 2; ++p) a[p] = *reinterpret_cast<const u32x4*>(As + i * 16 * XROW + p * ST_PLN);
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = x3_products16<2>(a, b[j], acc[i][j]);
      }
    }
  }

  // ---- partial O of this j range (out-scaled), partial row sums
  if (live) {
    float* __restrict__ Oz = O + (size_t)z * n * d;
    const float* __restrict__ osc = sc + 2 * dc;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = g * 128 + wcol + j * 16 + l15;
      if (col >= d) continue;
      const float os = osc[col];
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = i0 + i * 16 + 4 * lq + e;
          if (row < n) Oz[(size_t)row * d + col] = acc[i][j][e] * os;
        }
    }
  }
  if (cg == 0) {
    // a row's sum: the four lane groups lq of a wave, then the two waves wc = 0, 1 (through LDS, in that order)
    __syncthreads();   // every wave is past its last read of the P images
    float* red = reinterpret_cast<float*>(smem);   // [2][128] (KSD: rd's [2][128] behind it)
#pragma unroll
    for (int ib = 0; ib < 2; ++ib) {
      float a = rs[ib];
      a += __shfl_xor(a, 16);
      a += __shfl_xor(a, 32);
      if (lq == 0) red[wc * ST_ROWS + wr * 32 + ib * 16 + l15] = a;
      if constexpr (KSD) {
        float b = rd[ib];
        b += __shfl_xor(b, 16);
        b += __shfl_xor(b, 32);
        if (lq == 0) red[(2 + wc) * ST_ROWS + wr * 32 + ib * 16 + l15] = b;
      }
    }
    __syncthreads();
    const int row = i0 + t;
    if (t < ST_ROWS && row < n) RS[(size_t)z * n + row] = (red[t] + red[ST_ROWS + t]) * sc[4 * dc + 2];
    if constexpr (KSD)
      if (t < ST_ROWS && row < n) RD[(size_t)z * n + row] = (red[2 * ST_ROWS + t] + red[3 * ST_ROWS + t]) * sc[4 * dc + 2];
  }
}

__global__ __launch_bounds__(ST_THREADS) void k_phi_stream(const u16* __restrict__ T3, int ntk, const u16* __restrict__ Wt3,
                                                           long ntj, const float* __restrict__ r,
                                                           const float* __restrict__ sc, int dc,
                                                           const float* __restrict__ h2p, float* __restrict__ O,
                                                           float* __restrict__ RS, int n, int d, int row_tiles,
                                                           int col_groups, int cblocks, int jtiles, int jtiles_per) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * ST_BUF];
  phi_stream_body<false>(smem, T3, ntk, Wt3, ntj, r, sc, dc, h2p, O, RS, nullptr, n, d, row_tiles, col_groups, cblocks, jtiles,
                         jtiles_per);
}

// k_phi_stream that also leaves RD[jsplit][n], the partial sums of rd (same registers live, no scratch: __graft_entry__.py)
__global__ __launch_bounds__(ST_THREADS) void k_phi_stream_ksd(const u16* __restrict__ T3, int ntk,
                                                               const u16* __restrict__ Wt3, long ntj,
                                                               const float* __restrict__ r, const float* __restrict__ sc,
                                                               int dc, const float* __restrict__ h2p, float* __restrict__ O,
                                                               float* __restrict__ RS, float* __restrict__ RD, int n, int d,
                                                               int row_tiles, int col_groups, int cblocks, int jtiles,
                                                               int jtiles_per) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * ST_BUF];
  phi_stream_body<true>(smem, T3, ntk, Wt3, ntj, r, sc, dc, h2p, O, RS, RD, n, d, row_tiles, col_groups, cblocks, jtiles,
                        jtiles_per);
}

// ================================================================================================
// the streaming median: radix-select histograms straight from the distance tiles
// ================================================================================================
// One level's digits of one wave's share (32 rows x 64 columns) of tile (ti, tj), tj >= ti, into the LDS histogram
// h[2][STEIN_HIST_BINS]: the semantics of hist_pass_body<LEVEL, true> (stein_select.hip).  PRED = false: an off-diagonal
// tile that lies inside the matrix -- every entry stands for itself and its mirror image (weight 2), no per-entry test.
// PRED = true (diagonal and edge tiles): col > row weighs 2, col == row 1, col < row and everything >= n is skipped.
// Level 0 sees every entry and a handful of bins take them all: the wave-merged hist_add (every lane of the wave gets
// here: the branches around the call are workgroup-uniform).  Levels 1 and 2 see the entries under the prefixes only.
template <int LEVEL, bool PRED>
__device__ __forceinline__ void sh_count(const f32x4 (&s)[4][2], const float (&ri)[2], const float* __restrict__ r, float two_s,
                                         int row0 /* of this lane: + 16 ib */, int col0 /* of this lane: + 16 jb + e */, int n,
                                         u32* h, u32 pa, u32 pb, bool two, int lane) {
#pragma unroll
  for (int jb = 0; jb < 4; ++jb) {
    const int c4 = col0 + jb * 16;
    const float4 rj4 = *reinterpret_cast<const float4*>(r + c4);   // (r is padded to the tiles; columns >= n are not counted)
    const float rj[4] = {rj4.x, rj4.y, rj4.z, rj4.w};
#pragma unroll
    for (int ib = 0; ib < 2; ++ib) {
      const int row = row0 + ib * 16;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int col = c4 + e;
        const float dv = (ri[ib] + rj[e]) - two_s * s[jb][ib][e];   // k_phi_stream's expression, term for term
        const u32 key = f32_key(dv);
        const bool inb = !PRED || (row < n && col < n && col >= row);
        const bool dg = PRED && col == row;
        if (LEVEL == 0) {
          hist_add(h, key >> 21, inb && !dg, lane, 2u);
          if (PRED && inb && dg) atomicAdd(&h[key >> 21], 1u);
        } else {
          const u32 digit = LEVEL == 1 ? ((key >> 10) & 2047u) : (key & 1023u);
          const u32 hi = LEVEL == 1 ? (key >> 21) : (key >> 10);
          const u32 w = dg ? 1u : 2u;
          if (inb && hi == pa) atomicAdd(&h[digit], w);
          if (two && inb && hi == pb) atomicAdd(&h[STEIN_HIST_BINS + digit], w);
        }
      }
    }
  }
}

// A workgroup (512 threads, k_phi_stream's distance roles) owns tiles u = logical id, + grid, + 2 grid, ... of the
// nt (nt + 1) / 2 tiles (ti, tj >= ti) of the symmetric matrix -- useful tiles only, in folded-row order: virtual row v is
// row v (nt - v tiles) followed by row nt - 1 - v (v + 1 tiles), nt + 1 tiles whatever v, and the middle row of an odd nt
// comes last by itself.  Consecutive u share a row tile, and consecutive logical ids an XCD (xcd_remap): the row tile's
// fragments stay in that L2.
// Counts are integers: the u64 adds of the flush commute, so the histogram does not depend on the grid or on the order of
// the workgroups, and a repeated call is bit-identical.  The LDS counters are 32-bit and one tile adds at most
// 128 x 128 x 2 = 32768 to one bin: after flush_tiles <= 65536 tiles (65536 x 32768 = 2^31 < 2^32) the histogram is
// flushed and zeroed again; a workgroup with fewer tiles than that flushes once, at the end.
// Plain C++ loads; no workgroup waits for another; every loop bound is an argument.
constexpr int SH_FLUSH_TILES = 65536;
template <int LEVEL>
__global__ __launch_bounds__(ST_THREADS) void k_stream_hist(const u16* __restrict__ T3, int ntk, const float* __restrict__ r,
                                                            const float* __restrict__ sc, int dc,
                                                            const SelState* __restrict__ st, u64* __restrict__ hist, int n,
                                                            int nt, long tiles, int flush_tiles) {
  __shared__ u32 h[2 * STEIN_HIST_BINS];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  const int wr = w >> 1, wc = w & 1;   // rows [32 wr, 32 wr + 32) x columns [64 wc, 64 wc + 64) of the tile
  const u32 pa = st->prefix[0], pb = st->prefix[1];
  const bool two = LEVEL > 0 && st->diverged != 0u;
  const int nbins = (two ? 2 : 1) * STEIN_HIST_BINS;
  for (int b = t; b < 2 * STEIN_HIST_BINS; b += ST_THREADS) h[b] = 0u;
  __syncthreads();
  const float two_s = sc[4 * dc + 1];
  const long paired = (long)(nt >> 1) * (nt + 1);
  int since = 0;
  for (long u = xcd_remap(blockIdx.x, gridDim.x); u < tiles; u += gridDim.x) {
    int ti, tj;
    if (u < paired) {
      const int v = (int)(u / (nt + 1)), x = (int)(u - (long)v * (nt + 1)), len0 = nt - v;
      if (x < len0) { ti = v; tj = v + x; }
      else { ti = nt - 1 - v; tj = ti + (x - len0); }
    } else {
      ti = nt >> 1;
      tj = ti + (int)(u - paired);
    }
    const int row0 = ti * ST_ROWS + wr * 32 + l15, col0 = tj * ST_JT + wc * 64 + 4 * lq;
    float ri[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) ri[a] = r[row0 + a * 16];   // (padded to the row tiles; rows >= n are not counted)
    const u16* __restrict__ ta = T3 + (size_t)ti * ntk * 3 * XTILE_E + (wr * 2) * 512 + lane * 8;
    const u16* __restrict__ tb = T3 + (size_t)tj * ntk * 3 * XTILE_E + (wc * 4) * 512 + lane * 8;
    f32x4 s[4][2];
    st_distance_tile(ta, tb, ntk, s);
    if (ti != tj && tj * ST_JT + ST_JT <= n) sh_count<LEVEL, false>(s, ri, r, two_s, row0, col0, n, h, pa, pb, two, lane);
    else sh_count<LEVEL, true>(s, ri, r, two_s, row0, col0, n, h, pa, pb, two, lane);
    if (++since == flush_tiles) {   // (workgroup-uniform)
      since = 0;
      __syncthreads();
      for (int b = t; b < nbins; b += ST_THREADS)
        if (h[b]) { atomicAdd(&hist[b], (u64)h[b]); h[b] = 0u; }
      __syncthreads();
    }
  }
  __syncthreads();
  for (int b = t; b < nbins; b += ST_THREADS)
    if (h[b]) atomicAdd(&hist[b], (u64)h[b]);
}

// phi = (sum_z O_z + (sum_z RS_z) theta / h2) / n (the folded finish of k_phi_finish, steinhip.hip) and this workgroup's
// fp64 partial of |phi|^2.  vec (bit 0): d % 4 == 0 and O, T and phi 16-byte aligned; KSD, bit 1: so is G.
// KSD (k_stream_finish_ksd): also this workgroup's partials of the Stein discrepancy sums S and S_diag (include/steinhip.h,
// stein_svgd_phi_stream_ksd) into kpart[0][blocks] and kpart[1][blocks], in fp64 from the fp32 ow = sum_z O_z, rs and
// rd = sum_z RD_z (range order) and the score rows G; the rd term is added once per row, by the thread that holds its
// column 0.  phi may then be NULL: only the store is skipped.
__device__ __forceinline__ void stream_ksd_terms(float g, float ow, float th, float rs, double ih, double& s, double& sd) {
  const double gd = g, t = (double)th * ih, w = gd - t;
  s += w * (double)ow + (double)rs * (t * (2.0 * gd - t) + ih);   // g^2 - w^2 = t (2 g - t), t = theta / h2
  sd += gd * gd + ih;
}

template <bool KSD>
__device__ __forceinline__ void stream_finish_body(const float* __restrict__ O, const float* __restrict__ RS,
                                                   const float* __restrict__ RD, const float* __restrict__ T,
                                                   const float* __restrict__ G, const float* __restrict__ h2p,
                                                   float* __restrict__ phi, double* __restrict__ sqpart,
                                                   double* __restrict__ kpart, int n, int d, int jsplit, int vec) {
  __shared__ double red[KSD ? 12 : 4];
  const float h2 = *h2p;
  const float fn = (float)n;
  const long total = (long)n * d;
  const size_t zs = (size_t)n * d;
  const double ih = 1.0 / (double)h2;   // (KSD)
  double sq = 0.0, ks = 0.0, kd = 0.0;
  if (vec & 1) {
    const long total4 = total >> 2;
    const int d4 = d >> 2;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < total4; q += (long)gridDim.x * 256) {
      const int i = (int)(q / d4);
      const long e = q << 2;
      float4 og = make_float4(0.f, 0.f, 0.f, 0.f);
      float rs = 0.f;
      for (int z = 0; z < jsplit; ++z) {
        const float4 a = *reinterpret_cast<const float4*>(O + z * zs + e);
        og.x += a.x; og.y += a.y; og.z += a.z; og.w += a.w;
        rs += RS[(size_t)z * n + i];
      }
      const float4 th = *reinterpret_cast<const float4*>(T + e);
      float4 ph;
      ph.x = (og.x + rs * th.x / h2) / fn; ph.y = (og.y + rs * th.y / h2) / fn;
      ph.z = (og.z + rs * th.z / h2) / fn; ph.w = (og.w + rs * th.w / h2) / fn;
      if (!KSD || phi) *reinterpret_cast<float4*>(phi + e) = ph;
      sq += ((double)ph.x * (double)ph.x + (double)ph.y * (double)ph.y) + ((double)ph.z * (double)ph.z + (double)ph.w * (double)ph.w);
      if constexpr (KSD) {
        const float4 g = (vec & 2) ? *reinterpret_cast<const float4*>(G + e) : make_float4(G[e], G[e + 1], G[e + 2], G[e + 3]);
        stream_ksd_terms(g.x, og.x, th.x, rs, ih, ks, kd);
        stream_ksd_terms(g.y, og.y, th.y, rs, ih, ks, kd);
        stream_ksd_terms(g.z, og.z, th.z, rs, ih, ks, kd);
        stream_ksd_terms(g.w, og.w, th.w, rs, ih, ks, kd);
        if (q == (long)i * d4) {   // the row's first four columns
          float rd = 0.f;
          for (int z = 0; z < jsplit; ++z) rd += RD[(size_t)z * n + i];
          ks -= 0.5 * ih * ih * (double)rd;
        }
      }
    }
  } else {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
      const int i = (int)(e / d);
      float og = 0.f, rs = 0.f;
      for (int z = 0; z < jsplit; ++z) {
        og += O[z * zs + e];
        rs += RS[(size_t)z * n + i];
      }
      const float th = T[e];
      const float ph = (og + rs * th / h2) / fn;
      if (!KSD || phi) phi[e] = ph;
      sq += (double)ph * (double)ph;
      if constexpr (KSD) {
        stream_ksd_terms(G[e], og, th, rs, ih, ks, kd);
        if (e == (long)i * d) {   // the row's column 0
          float rd = 0.f;
          for (int z = 0; z < jsplit; ++z) rd += RD[(size_t)z * n + i];
          ks -= 0.5 * ih * ih * (double)rd;
        }
      }
    }
  }
  if constexpr (KSD) {
    double part[3] = {sq, ks, kd};
    block_sum256(part, red);
    if (threadIdx.x == 0) {
      sqpart[blockIdx.x] = part[0];
      kpart[blockIdx.x] = part[1];
      kpart[gridDim.x + blockIdx.x] = part[2];
    }
  } else {
    double part[1] = {sq};
    block_sum256(part, red);
    if (threadIdx.x == 0) sqpart[blockIdx.x] = part[0];
  }
}

__global__ __launch_bounds__(256) void k_stream_finish(const float* __restrict__ O, const float* __restrict__ RS,
                                                       const float* __restrict__ T, const float* __restrict__ h2p,
                                                       float* __restrict__ phi, double* __restrict__ sqpart, int n, int d,
                                                       int jsplit, int vec) {
  stream_finish_body<false>(O, RS, nullptr, T, nullptr, h2p, phi, sqpart, nullptr, n, d, jsplit, vec);
}

__global__ __launch_bounds__(256) void k_stream_finish_ksd(const float* __restrict__ O, const float* __restrict__ RS,
                                                           const float* __restrict__ RD, const float* __restrict__ T,
                                                           const float* __restrict__ G, const float* __restrict__ h2p,
                                                           float* __restrict__ phi, double* __restrict__ sqpart,
                                                           double* __restrict__ kpart, int n, int d, int jsplit, int vec) {
  stream_finish_body<true>(O, RS, RD, T, G, h2p, phi, sqpart, kpart, n, d, jsplit, vec);
}

// the block partials of k_stream_finish, in a fixed order -> sqnorm_out[0]
__global__ __launch_bounds__(256) void k_stream_sqsum(const double* __restrict__ part, int count, double* __restrict__ out) {
  __shared__ double red[4];
  double s[1] = {0.0};
  for (int i = threadIdx.x; i < count; i += 256) s[0] += part[i];
  block_sum256(s, red);
  if (threadIdx.x == 0) out[0] = s[0];
}

// the same for k_stream_finish_ksd's three sets, one workgroup each: sqpart[count] -> out[0], kpart[2][count] -> out[1], out[2]
__global__ __launch_bounds__(256) void k_stream_sqsum3(const double* __restrict__ sqpart, const double* __restrict__ kpart,
                                                       int count, double* __restrict__ out) {
  __shared__ double red[4];
  const double* __restrict__ part = blockIdx.x == 0 ? sqpart : kpart + (size_t)(blockIdx.x - 1) * count;
  double s[1] = {0.0};
  for (int i = threadIdx.x; i < count; i += 256) s[0] += part[i];
  block_sum256(s, red);
  if (threadIdx.x == 0) out[blockIdx.x] = s[0];
}

// ================================================================================================
// host side
// ================================================================================================
static thread_local int g_stream_jsplit = 0;   // stein_debug_stream_jsplit: 0 = the plan's own rule

struct StreamLayout {
  int64_t row_tiles, col_groups, cblocks, jsplit, jtiles_per, sq_blocks;
  int64_t rows, dk, dc, nk;                      // padded extents of the planes (the x3_* of SteinLayout)
  size_t r, sc, t3, wt3, o, rs, sq, total;       // byte offsets, 256-byte aligned
};

static int stream_check_shape(int64_t n, int64_t d, int dtype, int flags) {
  if (dtype == STEIN_BF16) return fail(STEIN_E_UNSUPPORTED, "the streaming step takes fp32 inputs (STEIN_F32), not bf16");
  if (dtype != STEIN_F32) return fail(STEIN_E_UNSUPPORTED, "dtype %d", dtype);
  if (flags != 0) return fail(STEIN_E_BADARG, "the streaming step takes no flags, got 0x%x", flags);
  if (n < 1 || d < 1) return fail(STEIN_E_SHAPE, "bad shape n=%lld d=%lld", (long long)n, (long long)d);
  return stein_check_size(n, d);
}

// The plan: one workgroup per (row tile, column group, j range).  The j ranges fill the resident grid (one workgroup per CU)
// when the row tiles and column groups alone do not: jsplit = floor(resident / (row_tiles col_groups)), at most one range
// per 128-column j tile; ranges are whole j tiles and empty tails are dropped.  So jsplit > 1 only while
// jsplit row_tiles col_groups <= resident: the partial sums then hold at most resident x 128 x 256 floats (32 MiB),
// whatever n and d; beyond that there is one range and they are n d floats.
static int stream_make_layout(int64_t n, int64_t d, StreamLayout* L) {
  L->row_tiles = (n + ST_ROWS - 1) / ST_ROWS;
  L->cblocks = (d + 127) / 128;
  L->col_groups = (d + ST_COLS - 1) / ST_COLS;
  const int64_t jtiles = L->row_tiles;
  int64_t want = g_stream_jsplit > 0 ? g_stream_jsplit : (int64_t)(RESIDENT_ONE_PER_CU / (double)(L->row_tiles * L->col_groups));
  if (want < 1) want = 1;
  if (want > jtiles) want = jtiles;
  L->jtiles_per = (jtiles + want - 1) / want;
  L->jsplit = (jtiles + L->jtiles_per - 1) / L->jtiles_per;
  L->rows = L->row_tiles * ST_ROWS;
  L->nk = L->rows;
  L->dk = (int64_t)align_up((size_t)d, 32);
  L->dc = (int64_t)align_up((size_t)d, 128);
  int64_t sqb = (n * d + 1023) / 1024;
  if (sqb > 1024) sqb = 1024;
  L->sq_blocks = sqb;
  size_t at = 0;
  auto put = [&](size_t bytes) { const size_t o = at; at = align_up(at + bytes, 256); return o; };
  L->r = put((size_t)L->rows * 4);
  L->sc = put((size_t)(6 * L->dc + 4) * 4);
  L->t3 = put((size_t)3 * L->rows * L->dk * 2);
  L->wt3 = put((size_t)3 * L->dc * L->nk * 2);
  L->o = put((size_t)L->jsplit * n * d * 4);
  L->rs = put((size_t)L->jsplit * n * 4);
  L->sq = put((size_t)sqb * 8);
  L->total = at;
  if (L->row_tiles * L->col_groups * L->jsplit > 0x7fffffffll) return fail(STEIN_E_SHAPE, "too many tiles");
  return STEIN_OK;
}

// Every address the streaming entry points use, formed once: of a stored-D layout only the planes' extents; the planes the
// split launchers take; and the step's partial sums (K.W of the j ranges in OG, their rowsum(K) in RS, the |phi|^2 block
// partials in SQ; no K.theta: nothing here asks for dK, and the statistic does without it -- StreamKsdLayout).
// The median passes StreamMedianLayout's hist / sel offsets: its histograms and select state lie where the step keeps W's
// planes and partial sums, which that call never touches.
static StepViews stream_views(const StreamLayout& L, void* workspace, size_t hist_at = 0, size_t sel_at = 0) {
  char* ws = (char*)workspace;
  StepViews v{};
  v.L.x3_rows = L.rows; v.L.x3_dk = L.dk; v.L.x3_dc = L.dc; v.L.x3_nk = L.nk;
  v.r = (float*)(ws + L.r);
  v.planes = ws;
  v.T3 = (unsigned short*)(ws + L.t3);
  v.Gt3 = (unsigned short*)(ws + L.wt3);
  v.sc = (float*)(ws + L.sc);
  v.cmax = (u32*)(v.sc + x3_sc_cmax(L.dc));
  v.two_s = v.sc + x3_sc_two_s(L.dc);
  v.OG = (float*)(ws + L.o);
  v.RS = (float*)(ws + L.rs);
  v.SQ = (double*)(ws + L.sq);
  if (sel_at) {
    v.hist = (u64*)(ws + hist_at);
    v.sel = (SelState*)(ws + sel_at);
  }
  return v;
}

// The layout of stein_svgd_phi_stream_ksd: StreamLayout as it is, with RD (the j ranges' partial rd, [jsplit][n] floats) and
// the S / S_diag block partials ([2][sq_blocks] doubles) appended behind its end.  No offset of the plain layout moves:
// a buffer of this size serves the plain step and the median call too.
struct StreamKsdLayout {
  StreamLayout L;
  size_t rd, kpart, total;
};

static int stream_ksd_make_layout(int64_t n, int64_t d, StreamKsdLayout* K) {
  if (int rc = stream_make_layout(n, d, &K->L)) return rc;
  K->rd = K->L.total;
  K->kpart = K->rd + align_up((size_t)K->L.jsplit * n * 4, 256);
  K->total = K->kpart + align_up((size_t)2 * K->L.sq_blocks * 8, 256);
  return STEIN_OK;
}

extern "C" int stein_debug_stream_jsplit(int jsplit) {
  if (jsplit < 0) return fail(STEIN_E_BADARG, "jsplit < 0");
  g_stream_jsplit = jsplit;
  return STEIN_OK;
}
int stein_stream_jsplit_hook(void) { return g_stream_jsplit; }   // (stein_imq.hip's plan honours the same hook)

extern "C" int stein_stream_workspace_bytes(int64_t n, int64_t d, int dtype, int flags, size_t* out_bytes) {
  if (!out_bytes) return fail(STEIN_E_BADARG, "out_bytes is NULL");
  int rc = stream_check_shape(n, d, dtype, flags);
  if (rc) return rc;
  StreamLayout L;
  if ((rc = stream_make_layout(n, d, &L))) return rc;
  *out_bytes = L.total;
  return STEIN_OK;
}

extern "C" int stein_stream_plan(int64_t n, int64_t d, int* row_tiles, int* col_groups, int* jsplit) {
  if (!row_tiles || !col_groups || !jsplit) return fail(STEIN_E_BADARG, "NULL output");
  int rc = stream_check_shape(n, d, STEIN_F32, 0);
  if (rc) return rc;
  StreamLayout L;
  if ((rc = stream_make_layout(n, d, &L))) return rc;
  *row_tiles = (int)L.row_tiles;
  *col_groups = (int)L.col_groups;
  *jsplit = (int)L.jsplit;
  return STEIN_OK;
}

// The launches in front of the contraction, the same for the plain step and the one with the statistic:
// 1. row norms (the padding rows of r are never read into a stored result), column maxima -> scales
// 2. theta's row-major planes (fold form of the split: no transposed image, the score only feeds the maxima)
// 3. W = G - theta / h2 at the caller's bandwidth
static int stream_operands(const StepViews& v, const void* theta, const void* score, int64_t n, int64_t d, int dtype,
                           const float* h2_in, hipStream_t s) {
  int rc;
  if ((rc = stein_rownorms(theta, n, d, dtype, v.r, (void*)s))) return rc;
  const SplitFused only_rows{nullptr, nullptr, 1};
  if ((rc = stein_x3_split(v, theta, score, dtype, n, d, s, &only_rows))) return rc;
  return stein_x3_split_w(v, (const float*)theta, (const float*)score, n, d, h2_in, s);
}

extern "C" int stein_svgd_phi_stream(const void* theta, const void* score, int64_t n, int64_t d, int dtype,
                                     const float* h2_in, float* phi, double* sqnorm_out, void* workspace, size_t ws_bytes,
                                     int flags, void* stream) {
  if (!theta || !score || !h2_in || !phi || !sqnorm_out || !workspace) return fail(STEIN_E_BADARG, "NULL pointer");
  if ((uintptr_t)workspace & 15) return fail(STEIN_E_BADARG, "the workspace must be 16-byte aligned");   // (16-byte loads of its sections)
  int rc = stream_check_shape(n, d, dtype, flags);
  if (rc) return rc;
  StreamLayout L;
  if ((rc = stream_make_layout(n, d, &L))) return rc;
  if (ws_bytes < L.total) return fail(STEIN_E_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, L.total);
  if ((rc = stein_take_device_error())) return rc;   // a kernel of an earlier call on this device gave up: say so now
  hipStream_t s = (hipStream_t)stream;
  const StepViews v = stream_views(L, workspace);
  if ((rc = stream_operands(v, theta, score, n, d, dtype, h2_in, s))) return rc;
  // 4. the streaming contraction
  const long nblk = (long)(L.row_tiles * L.col_groups * L.jsplit);
  hipLaunchKernelGGL(k_phi_stream, dim3((unsigned)nblk), dim3(ST_THREADS), 0, s, v.T3, (int)(L.dk / 32), v.Gt3,
                     (long)(L.nk / 32), v.r, v.sc, (int)L.dc, h2_in, v.OG, v.RS, (int)n, (int)d, (int)L.row_tiles,
                     (int)L.col_groups, (int)L.cblocks, (int)L.row_tiles, (int)L.jtiles_per);
  LAUNCH_CHECK("k_phi_stream");
  // 5. finish
  const int vec = d % 4 == 0 && (((uintptr_t)theta | (uintptr_t)phi) & 15) == 0;
  hipLaunchKernelGGL(k_stream_finish, dim3((unsigned)L.sq_blocks), dim3(256), 0, s, v.OG, v.RS, (const float*)theta, h2_in, phi,
                     v.SQ, (int)n, (int)d, (int)L.jsplit, vec);
  LAUNCH_CHECK("k_stream_finish");
  hipLaunchKernelGGL(k_stream_sqsum, dim3(1), dim3(256), 0, s, v.SQ, (int)L.sq_blocks, sqnorm_out);
  LAUNCH_CHECK("k_stream_sqsum");
  return STEIN_OK;
}

// ---- the streaming step with the Stein discrepancy sums ---------------------------------------------------------------
extern "C" int stein_stream_ksd_workspace_bytes(int64_t n, int64_t d, int dtype, int flags, size_t* out_bytes) {
  if (!out_bytes) return fail(STEIN_E_BADARG, "out_bytes is NULL");
  int rc = stream_check_shape(n, d, dtype, flags);
  if (rc) return rc;
  StreamKsdLayout K;
  if ((rc = stream_ksd_make_layout(n, d, &K))) return rc;
  *out_bytes = K.total;
  return STEIN_OK;
}

extern "C" int stein_svgd_phi_stream_ksd(const void* theta, const void* score, int64_t n, int64_t d, int dtype,
                                         const float* h2_in, float* phi, double* sums_out, void* workspace, size_t ws_bytes,
                                         int flags, void* stream) {
  if (!theta || !score || !h2_in || !sums_out || !workspace) return fail(STEIN_E_BADARG, "NULL pointer");   // (phi may be)
  if ((uintptr_t)workspace & 15) return fail(STEIN_E_BADARG, "the workspace must be 16-byte aligned");
  int rc = stream_check_shape(n, d, dtype, flags);
  if (rc) return rc;
  StreamKsdLayout K;
  if ((rc = stream_ksd_make_layout(n, d, &K))) return rc;
  const StreamLayout& L = K.L;
  if (ws_bytes < K.total) return fail(STEIN_E_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, K.total);
  if ((rc = stein_take_device_error())) return rc;
  hipStream_t s = (hipStream_t)stream;
  const StepViews v = stream_views(L, workspace);
  float* RD = (float*)((char*)workspace + K.rd);
  double* KP = (double*)((char*)workspace + K.kpart);
  if ((rc = stream_operands(v, theta, score, n, d, dtype, h2_in, s))) return rc;
  // 4. the streaming contraction, with the second row sum
  const long nblk = (long)(L.row_tiles * L.col_groups * L.jsplit);
  hipLaunchKernelGGL(k_phi_stream_ksd, dim3((unsigned)nblk), dim3(ST_THREADS), 0, s, v.T3, (int)(L.dk / 32), v.Gt3,
                     (long)(L.nk / 32), v.r, v.sc, (int)L.dc, h2_in, v.OG, v.RS, RD, (int)n, (int)d, (int)L.row_tiles,
                     (int)L.col_groups, (int)L.cblocks, (int)L.row_tiles, (int)L.jtiles_per);
  LAUNCH_CHECK("k_phi_stream_ksd");
  // 5. finish: phi (unless NULL), the three sets of block partials, their sums in a fixed order.  The 16-byte path is chosen
  // as in the plain step (a NULL phi counts as aligned), so that |phi|^2 is summed in the plain step's order; the score's
  // alignment only decides how its rows are loaded on that path (bit 1)
  const int vec = (d % 4 == 0 && (((uintptr_t)theta | (uintptr_t)phi) & 15) == 0 ? 1 : 0) | (((uintptr_t)score & 15) == 0 ? 2 : 0);
  hipLaunchKernelGGL(k_stream_finish_ksd, dim3((unsigned)L.sq_blocks), dim3(256), 0, s, v.OG, v.RS, RD, (const float*)theta,
                     (const float*)score, h2_in, phi, v.SQ, KP, (int)n, (int)d, (int)L.jsplit, vec);
  LAUNCH_CHECK("k_stream_finish_ksd");
  hipLaunchKernelGGL(k_stream_sqsum3, dim3(3), dim3(256), 0, s, v.SQ, KP, (int)L.sq_blocks, sums_out);
  LAUNCH_CHECK("k_stream_sqsum3");
  return STEIN_OK;
}

// ---- the streaming median -------------------------------------------------------------------------------------------
// Workspace: a prefix-compatible subset of StreamLayout.  Row norms, scales and theta's planes sit at the step's own offsets
// (none of them depends on the j split); the three histograms (96 KiB) start where the step keeps W's planes, the select
// state (64 bytes, its own 256) behind them.  W's planes are at least 3 x 128 x 128 x 2 = 96 KiB and the step has three more
// sections of at least 256 bytes behind them, so this layout never reaches past the step's: one buffer serves both calls
// back to back (at the smallest shapes the select state lies in the step's partial-sum area, not in W's planes).
static thread_local int g_stream_median_grid = 0;   // stein_debug_stream_median_grid: 0 = the rule below
// Workgroups per CU the grid is sized for.  k_stream_hist: 90-92 VGPRs (96 allocated), 16 KB of LDS, 8 waves -> the register file
// holds five waves per SIMD, i.e. two whole workgroups (two waves per SIMD each) per CU ("streaming median"); tiles cost the same, so a grid of
// exactly the resident workgroups with strided shares is balanced to within one tile.
constexpr int SH_WG_PER_CU = 2;
constexpr size_t SH_HIST_BYTES = (size_t)STEIN_HIST_LEVELS * 2 * STEIN_HIST_BINS * 8;

struct StreamMedianLayout {
  StreamLayout L;            // r, sc, t3 and the planes' extents
  size_t hist, sel, total;
  int64_t tiles, blocks;
};

static int stream_median_make_layout(int64_t n, int64_t d, int dtype, int flags, StreamMedianLayout* M) {
  int rc = stream_check_shape(n, d, dtype, flags);
  if (rc) return rc;
  if (n < 2) return fail(STEIN_E_SHAPE, "n = %lld: the median-heuristic bandwidth divides by ln n; need n >= 2", (long long)n);
  if ((rc = stream_make_layout(n, d, &M->L))) return rc;
  M->hist = M->L.wt3;
  M->sel = M->hist + align_up(SH_HIST_BYTES, 256);
  M->total = M->sel + 256;
  const int64_t nt = M->L.row_tiles;
  M->tiles = nt * (nt + 1) / 2;
  const int64_t want = g_stream_median_grid > 0 ? g_stream_median_grid : (int64_t)SH_WG_PER_CU * (int64_t)RESIDENT_ONE_PER_CU;
  M->blocks = g_stream_median_grid > 0 ? want : (M->tiles < want ? M->tiles : want);
  return STEIN_OK;
}

extern "C" int stein_debug_stream_median_grid(int blocks) {
  if (blocks < 0 || blocks > 65535) return fail(STEIN_E_BADARG, "blocks %d", blocks);
  g_stream_median_grid = blocks;
  return STEIN_OK;
}

extern "C" int stein_stream_median_workspace_bytes(int64_t n, int64_t d, int dtype, int flags, size_t* out_bytes) {
  if (!out_bytes) return fail(STEIN_E_BADARG, "out_bytes is NULL");
  StreamMedianLayout M;
  if (int rc = stream_median_make_layout(n, d, dtype, flags, &M)) return rc;
  *out_bytes = M.total;
  return STEIN_OK;
}

extern "C" int stein_stream_median_plan(int64_t n, int64_t d, size_t* hist_offset, size_t* state_offset, int64_t* tiles,
                                        int* blocks) {
  if (!hist_offset || !state_offset || !tiles || !blocks) return fail(STEIN_E_BADARG, "NULL output");
  StreamMedianLayout M;
  if (int rc = stream_median_make_layout(n, d, STEIN_F32, 0, &M)) return rc;
  *hist_offset = M.hist;
  *state_offset = M.sel;
  *tiles = M.tiles;
  *blocks = (int)M.blocks;
  return STEIN_OK;
}

template <int LEVEL>
static void launch_stream_hist(const StreamMedianLayout& M, const StepViews& v, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL((k_stream_hist<LEVEL>), dim3((unsigned)M.blocks), dim3(ST_THREADS), 0, s, v.T3, (int)(M.L.dk / 32), v.r,
                     v.sc, (int)M.L.dc, v.sel, v.hist + (size_t)LEVEL * 2 * STEIN_HIST_BINS, (int)n, (int)M.L.row_tiles,
                     (long)M.tiles, SH_FLUSH_TILES);
}

extern "C" int stein_stream_median(const void* theta, int64_t n, int64_t d, int dtype, float* h2_out, float* median_out,
                                   void* workspace, size_t ws_bytes, int flags, void* stream) {
  if (!theta || !h2_out || !workspace) return fail(STEIN_E_BADARG, "NULL pointer");
  if ((uintptr_t)workspace & 15) return fail(STEIN_E_BADARG, "the workspace must be 16-byte aligned");
  StreamMedianLayout M;
  int rc = stream_median_make_layout(n, d, dtype, flags, &M);
  if (rc) return rc;
  const StreamLayout& L = M.L;
  if (ws_bytes < M.total) return fail(STEIN_E_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, M.total);
  if ((rc = stein_take_device_error())) return rc;
  hipStream_t s = (hipStream_t)stream;
  const StepViews v = stream_views(L, workspace, M.hist, M.sel);
  // 1. row norms; 2. theta's scales and row-major planes, as the step builds them.  There is no score: the split takes a
  // NULL score as "leave that half of the column maxima alone", and k_make_scales reads both halves -- the score's only
  // feed scales this call never uses, but they are zeroed here so that nothing reads what the workspace held.
  if ((rc = stein_rownorms(theta, n, d, dtype, v.r, stream))) return rc;
  HIP_TRY(hipMemsetAsync(v.cmax, 0, (size_t)L.dc * sizeof(u32), s));
  const SplitFused only_rows{nullptr, nullptr, 1};
  if ((rc = stein_x3_split(v, theta, nullptr, dtype, n, d, s, &only_rows))) return rc;
  // 3. select state for n^2 entries, histograms zeroed; 4. three levels, k_resolve between them
  if ((rc = stein_median_begin(v.hist, v.sel, n * n, stream))) return rc;
  launch_stream_hist<0>(M, v, n, s);
  LAUNCH_CHECK("k_stream_hist<0>");
  if ((rc = stein_median_resolve(v.hist, 0, n, v.sel, h2_out, median_out, stream))) return rc;
  launch_stream_hist<1>(M, v, n, s);
  LAUNCH_CHECK("k_stream_hist<1>");
  if ((rc = stein_median_resolve(v.hist, 1, n, v.sel, h2_out, median_out, stream))) return rc;
  launch_stream_hist<2>(M, v, n, s);
  LAUNCH_CHECK("k_stream_hist<2>");
  return stein_median_resolve(v.hist, 2, n, v.sel, h2_out, median_out, stream);
}
