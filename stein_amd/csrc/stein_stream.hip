// stein_stream.hip -- the SVGD direction at a bandwidth the caller supplies, without the n x n distance image.
//
// With h2 known before the step starts nothing needs all of D at once: the folded operand W = G - theta / h2 (stein_x3.hip,
// "folded operand") is built first, and a tile of D is exponentiated and contracted with W the moment its accumulators are
// complete, then dropped.  The workspace is O(n d): row norms, scales, theta's row-major planes, W's transposed planes and
// the partial sums (stream_make_layout, stein_stream_host.h).
//
//   stein_rownorms, k_colmax, k_make_scales, k_split (theta, row-major image only), k_split_w   as they are (stein_x3.hip)
//   k_phi_stream        distance tile -> P = exp2(c D + 14) -> O += P.W, running rowsum(P); D and K never reach memory
//   k_stream_finish     sums the j ranges in order, phi = (K.W + rowsum(K) theta / h2) / n, |phi|^2 block partials (fp64)
//   k_stream_sum        (stein_stream_tile.h) one workgroup: the block partials -> sqnorm_out
// stein_svgd_phi_stream_ksd, the step with the Stein discrepancy sums at its own bandwidth (include/steinhip.h), launches
// the KSD forms of the same bodies: k_phi_stream_ksd (a second running row sum, rd = rowsum(P o D)), k_stream_finish_ksd
// (reads the score rows too; three sets of block partials) and k_stream_sum on a grid of three.  No K.theta, no further
// column space.
// The P image's swizzle, the fp16 split and the exponent offset (pswz, cvt_pk_f16, f16_resid_lo / _hi, PEXP_H2) are
// stein_x3_dev.h's, the ones the stored-D contraction uses; the size limits, align_up and the resident-workgroup count are
// stein_host.h's, shared with stein_make_layout.  The tile phases other than the element function, the frame of the finish
// pass (st_finish_body) and k_stream_sum are stein_stream_tile.h's, and the host side around the launches is
// stein_stream_host.h's: the IMQ step (stein_imq.hip) runs the same code.  The finish pass stays a kernel of this file
// although k_phi_finish's FOLD form (steinhip.hip) gives the same bits: at 8 j ranges that kernel takes its generic loop and
// the step measured slower ("streaming step").
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
// k_stream_hist runs the distance phase of k_phi_stream (st_distance_tile, stein_stream_tile.h: one body for both), so the
// median is the median of the D values the step exponentiates.

#include "stein_x3.h"

#include "stein_x3_dev.h"

// the tile geometry (ST_THREADS, ST_ROWS, ST_JT, ST_PLN, ST_KTB, ST_BUF) and the tile phases (stein_stream_tile.h), the layout
// and the entry points' prologue: shared with the IMQ step (stein_imq.hip)
#include "stein_stream_host.h"

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

  const StRoles ro = st_roles();
  const int lane = ro.lane, w = ro.w, l15 = ro.l15, lq = ro.lq, wr = ro.wr, wc = ro.wc, wcol = ro.wcol;
  // contraction role: the 32 columns at wcol of 128-column block g.  A block past the matrix's last (an odd block count:
  // d <= 128, or the last column group) has nothing to contract: its four waves only take part in the distance tiles and
  // the barriers (wave-uniform test)
  const int g = 2 * cg + (w >> 2);
  const bool live = g < cblocks;
  const int gl = min(g, cblocks - 1);

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
        const StSplit4 p = st_split4(q);
        st_stage4(st_image_dst(buf, wr * 32 + ib * 16 + l15, jc), p);
      }
    }
    __syncthreads();
    // ---- contraction: O += P . W_j over the tile's (up to) four 32-deep k tiles
    for (int kt = 0; live && kt < ST_JT / 32; ++kt) {
      if (j0 + kt * 32 >= n) break;   // P is zero there
      st_contract_ktile(acc, buf + kt * ST_KTB + aoff, wb + ((size_t)jt * (ST_JT / 32) + kt) * 3 * XTILE_E);
    }
  }

  // ---- partial O of this j range (out-scaled), partial row sums
  if (live) st_store_partial(O + (size_t)z * n * d, sc + 2 * dc, acc, g * 128 + wcol, i0, lq, l15, n, d);
  if (cg == 0) st_reduce_rows<KSD>(smem, rs, rd, RS, RD, z, i0, n, sc + 4 * dc + 2, ro);
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
  const StRoles ro = st_roles();   // (the distance role only)
  const int t = ro.t, lane = ro.lane, l15 = ro.l15, lq = ro.lq, wr = ro.wr, wc = ro.wc;
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

// The RBF step's part of the finish pass (st_finish_body, stein_stream_tile.h): one operand, ow = sum_z O_z;
// phi = (ow + rs theta / h2) / n (the folded finish of k_phi_finish, steinhip.hip); the statistic's terms (include/steinhip.h,
// stein_svgd_phi_stream_ksd) per element, and per row -rd / (2 h2^2).
struct RbfFinish {
  static constexpr int NO = 1;
  float h2, fn;
  double ih;   // (KSD)
  __device__ RbfFinish(const float* __restrict__ h2p, int n, int) : h2(*h2p), fn((float)n), ih(1.0 / (double)*h2p) {}
  __device__ float phi(const float (&o)[NO], float th, float rs) const { return (o[0] + rs * th / h2) / fn; }
  __device__ void ksd_terms(float g, const float (&o)[NO], float th, float rs, double& s, double& sd) const {
    const double gd = g, t = (double)th * ih, w = gd - t;
    s += w * (double)o[0] + (double)rs * (t * (2.0 * gd - t) + ih);   // g^2 - w^2 = t (2 g - t), t = theta / h2
    sd += gd * gd + ih;
  }
  __device__ double row_term(float, float rd) const { return -0.5 * ih * ih * (double)rd; }
};

__global__ __launch_bounds__(256) void k_stream_finish(const float* __restrict__ O, const float* __restrict__ RS,
                                                       const float* __restrict__ T, const float* __restrict__ h2p,
                                                       float* __restrict__ phi, double* __restrict__ sqpart, int n, int d,
                                                       int jsplit, int vec) {
  st_finish_body<RbfFinish, false>(O, nullptr, RS, nullptr, T, nullptr, h2p, phi, sqpart, nullptr, n, d, jsplit, vec);
}

__global__ __launch_bounds__(256) void k_stream_finish_ksd(const float* __restrict__ O, const float* __restrict__ RS,
                                                           const float* __restrict__ RD, const float* __restrict__ T,
                                                           const float* __restrict__ G, const float* __restrict__ h2p,
                                                           float* __restrict__ phi, double* __restrict__ sqpart,
                                                           double* __restrict__ kpart, int n, int d, int jsplit, int vec) {
  st_finish_body<RbfFinish, true>(O, nullptr, RS, RD, T, G, h2p, phi, sqpart, kpart, n, d, jsplit, vec);
}

// ================================================================================================
// host side
// ================================================================================================
// (shape check, layout, views, sizes, plan, the entry points' prologue and last launch: stein_stream_host.h, the IMQ step's too)
static thread_local int g_stream_jsplit = 0;   // stein_debug_stream_jsplit: 0 = the plan's own rule

extern "C" int stein_debug_stream_jsplit(int jsplit) {
  if (jsplit < 0) return fail(STEIN_E_BADARG, "jsplit < 0");
  g_stream_jsplit = jsplit;
  return STEIN_OK;
}
int stein_stream_jsplit_hook(void) { return g_stream_jsplit; }   // (stream_make_layout reads it in either step's file)

extern "C" int stein_stream_workspace_bytes(int64_t n, int64_t d, int dtype, int flags, size_t* out_bytes) {
  return stream_workspace_bytes(STREAM_RBF, false, n, d, dtype, flags, out_bytes);
}

extern "C" int stein_stream_ksd_workspace_bytes(int64_t n, int64_t d, int dtype, int flags, size_t* out_bytes) {
  return stream_workspace_bytes(STREAM_RBF, true, n, d, dtype, flags, out_bytes);
}

extern "C" int stein_stream_plan(int64_t n, int64_t d, int* row_tiles, int* col_groups, int* jsplit) {
  return stream_plan(STREAM_RBF, n, d, row_tiles, col_groups, jsplit);
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
  StreamCall c;
  int rc = stream_begin(STREAM_RBF, false, theta, score, n, d, dtype, h2_in, phi, sqnorm_out, workspace, ws_bytes, flags, stream, &c);
  if (rc) return rc;
  const StreamLayout& L = c.L;
  const StepViews& v = c.v;
  if ((rc = stream_operands(v, theta, score, n, d, dtype, h2_in, c.s))) return rc;
  // 4. the streaming contraction
  hipLaunchKernelGGL(k_phi_stream, dim3(c.nblk), dim3(ST_THREADS), 0, c.s, v.T3, (int)(L.dk / 32), v.Gt3, (long)(L.nk / 32),
                     v.r, v.sc, (int)L.dc, h2_in, v.OG, v.RS, (int)n, (int)d, (int)L.row_tiles, (int)L.col_units,
                     (int)L.cblocks, (int)L.row_tiles, (int)L.jtiles_per);
  LAUNCH_CHECK("k_phi_stream");
  // 5. finish: phi, the |phi|^2 block partials, their sum in a fixed order
  hipLaunchKernelGGL(k_stream_finish, dim3((unsigned)L.sq_blocks), dim3(256), 0, c.s, v.OG, v.RS, (const float*)theta, h2_in,
                     phi, v.SQ, (int)n, (int)d, (int)L.jsplit, c.vec);
  LAUNCH_CHECK("k_stream_finish");
  return stream_sum(c, sqnorm_out);
}

// ---- the streaming step with the Stein discrepancy sums ---------------------------------------------------------------
extern "C" int stein_svgd_phi_stream_ksd(const void* theta, const void* score, int64_t n, int64_t d, int dtype,
                                         const float* h2_in, float* phi, double* sums_out, void* workspace, size_t ws_bytes,
                                         int flags, void* stream) {
  StreamCall c;
  int rc = stream_begin(STREAM_RBF, true, theta, score, n, d, dtype, h2_in, phi, sums_out, workspace, ws_bytes, flags, stream, &c);
  if (rc) return rc;
  const StreamLayout& L = c.L;
  const StepViews& v = c.v;
  if ((rc = stream_operands(v, theta, score, n, d, dtype, h2_in, c.s))) return rc;
  // 4. the streaming contraction, with the second row sum
  hipLaunchKernelGGL(k_phi_stream_ksd, dim3(c.nblk), dim3(ST_THREADS), 0, c.s, v.T3, (int)(L.dk / 32), v.Gt3,
                     (long)(L.nk / 32), v.r, v.sc, (int)L.dc, h2_in, v.OG, v.RS, c.RD, (int)n, (int)d, (int)L.row_tiles,
                     (int)L.col_units, (int)L.cblocks, (int)L.row_tiles, (int)L.jtiles_per);
  LAUNCH_CHECK("k_phi_stream_ksd");
  // 5. finish: phi (unless NULL), the three sets of block partials, their sums in a fixed order
  hipLaunchKernelGGL(k_stream_finish_ksd, dim3((unsigned)L.sq_blocks), dim3(256), 0, c.s, v.OG, v.RS, c.RD, (const float*)theta,
                     (const float*)score, h2_in, phi, v.SQ, c.KP, (int)n, (int)d, (int)L.jsplit, c.vec);
  LAUNCH_CHECK("k_stream_finish_ksd");
  return stream_sum(c, sums_out);
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
  int rc = stream_check_shape(STREAM_RBF, n, d, dtype, flags);
  if (rc) return rc;
  if (n < 2) return fail(STEIN_E_SHAPE, "n = %lld: the median-heuristic bandwidth divides by ln n; need n >= 2", (long long)n);
  if ((rc = stream_make_layout(STREAM_RBF, n, d, &M->L))) return rc;
  M->hist = M->L.planes[0];
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
