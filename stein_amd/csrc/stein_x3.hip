// stein_x3.hip -- both GEMMs of the SVGD step on the 16-bit matrix cores with fp32-level accuracy.
//
// gfx950 runs the 16-bit-input MFMAs at 16x the rate of the fp32-input MFMA.  Every fp32 operand x is split into a
// short sum of 16-bit terms whose pairwise products are exact in fp32 (the MFMA accumulates in fp32), and a product
// a*b is formed from the term pairs that matter.  KIND selects the split:
//   KIND 2 (fp32 inputs)           x * 2^s = hi + lo, two fp16 terms (hi = fp16(x'), lo = fp16(x' - hi), the subtraction
//          is exact: 22 significant bits); products lo*hi, hi*lo, hi*hi (the dropped lo*lo is 2^-22 relative).  fp16 has
//          a 5-bit exponent, so operands are pre-scaled by powers of two (exact, undone exactly in the epilogues):
//          theta^T and score^T per column to a column maximum in [2^13, 2^14), theta for the distance GEMM by one factor
//          for the whole matrix, and P = exp2(c D + 14) in (0, 2^14].  An entry far below its column's maximum keeps
//          an ABSOLUTE error of 2^-25 of the scaled unit, i.e. 2^-38 of the column maximum -- the same norm-wise
//          guarantee an fp32 GEMM gives.
//          (A three-term bf16 split, six products and no scaling, was measured in round 1: same accuracy, twice the
//          matrix-core time; it is no longer built.)
//   KIND 1 (bf16 inputs)           the value itself; one product.
//
//   k_colmax, k_make_scales   column maxima -> power-of-two scales (KIND 2; all ones otherwise)
//   k_split         theta, score -> 16-bit operand tiles ("planes", layout below)
//   k_split_rows    theta -> its row-major planes alone, scaled by max|theta| as the fused call's prologue found it (the folded
//                   step that is asked for phi alone: it launches neither k_colmax nor k_make_scales -- the column maxima are
//                   taken by the select launch's slice, stein_select.hip, and turned into scales by k_split_w)
//   k_split_w       theta, score, h2 -> the planes of W = score - theta / h2 (the fused call's folded operand, behind the median);
//                   W's column scales and theta's, from the column maxima
//   k_distance_x3   S = T T^T from the planes; shares the fp32 kernel's epilogue (D, level-0 histogram or window counting).
//                   Single rank: only the 128 x 128 tiles on and above the diagonal are computed AND stored
//   k_phi_x3fs      warp-specialised contraction: producer waves build P = exp2(c D) (split on the fly) in LDS -- a k tile
//                   left of the row tile's diagonal block from its mirror image D[j][i] --, consumer waves stream the V
//                   fragments from L2 and issue the MFMAs
//
// Both GEMMs are "row x row" products (C[i][c] = sum_k A[i][k] B[c][k]) with k contiguous for both operands.
//
// Operand tile = 128 rows x 32 k of one plane = [128][32] x 16 bit = 8 KB; a tile has three plane slots (24 KB, KIND of
// them used; the third is a leftover of the three-term split) and tiles are stored tile-major:  tile(rb, kt) at ((rb * ntk + kt) * 3 + plane) * 4096 elements.
// One wave-wide 16-byte-per-lane load therefore covers 1 KB of consecutive memory (row-major planes made every
// 64-byte row piece its own cache-line visit: the producers spent 2900 cycles per k tile issuing loads).
//   T3   rows = particles, k = parameters   (distance operands)
//   Vt3  rows = parameters, k = particles   (theta^T and score^T: the contraction's B operand; never staged in LDS)
//   Each plane of a tile is stored in MFMA fragment order [row / 16][chunk][row % 16][8] (vfrag_offset), so the operand
//   fragment of a 16-row block is ONE coalesced 1 KB load, lane l reading bytes 16 l .. 16 l + 15.  k_distance_x3 stages
//   T3 through LDS chunk by chunk (its tile's rows may straddle two row blocks when a rank's row0 is not a multiple of
//   128); k_distance_panel (stein_dpanel.hip) copies fragments into LDS and streams them into registers as they are.
//
// LDS image of a plane: [128 rows][64 B], chunk c of row r at 16 * (c ^ ((r >> 2) & 3)).  Conflict-free for
//   ds_read_b128 fragments (16-lane groups {0-3,12-15,20-27}..., 64 banks): (4 row + chunk') mod 16 distinct in a group
//   ds_write_b128 staging  (8 consecutive lanes = 2 rows x 4 chunks, 32 banks): even row -> bytes 0..63, odd -> 64..127
//   ds_write_b64 of P      (16 consecutive lanes = 2 rows x 8 half-chunks): same split
// (an 80-byte padded row made every write 2-way conflicted.)  Lane l of a 32x32x16 MFMA reads the 8 consecutive k
// of row (l & 31) at k offset 8 (l >> 5).
//
// Scales area (floats at planes + L.x3_sc; dc = roundup(d, 128)):
//   [0, dc)       in-scale of the score columns       Gt3 = split(G * in)
//   [dc, 2dc)     in-scale of the theta columns       Tt3 = split(theta * in)
//   [2dc, 3dc)    out-scale of the K.G columns        = 1 / (in * 2^PEXP)
//   [3dc, 4dc)    out-scale of the K.theta columns
//   [4dc + 0]     in-scale of theta for T3 (one factor: S = T T^T mixes the columns)
//   [4dc + 1]     two_s = 2 / in^2:  D = r_i + r_j - two_s * S'
//   [4dc + 2]     2^-PEXP, the rowsum(K) unscale
//   then u32 [2][dc]: bit patterns of the column maxima of |score|, |theta| (k_colmax, or the slice of k_spec_select)

#include "stein_x3.h"

#include <stdlib.h>

#include "stein_x3_dev.h"
template <int KIND> struct SplitTraits { static constexpr int pexp = KIND == 2 ? PEXP_H2 : 0; };

#include <type_traits>

__device__ __forceinline__ int xswz(int row, int chunk) { return (chunk ^ ((row >> 2) & 3)) * 16; }

// ------------------------------------------------------------------------------------------------
// splitting
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ u32 cvt_pk_bf16(float lo, float hi) {   // round-to-nearest-even, lo -> bits 15:0
  u32 r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}

// two fp32 values -> KIND packed 16-bit pairs w[0..KIND) (x in the low half), most significant term first
template <int KIND>
__device__ __forceinline__ void split_pair(float x, float y, u32 (&w)[3]) {
  if (KIND == 2) {
    w[0] = cvt_pk_f16(x, y);
    w[1] = cvt_pk_f16(f16_resid_lo(w[0], x), f16_resid_hi(w[0], y));
  } else {
    w[0] = cvt_pk_bf16(x, y);   // bf16 inputs: exact
  }
}

// ------------------------------------------------------------------------------------------------
// scales (KIND 2)
// ------------------------------------------------------------------------------------------------
// (abs_bits: stein_common.h; pow2i and scale_exp: stein_x3_dev.h, the bootstrap kernel scales its image with them too)

// the three entries behind the column scales (see the header) from the exponent of theta's one scale
__device__ __forceinline__ void write_global_scales(float* __restrict__ sc, int dc, int sa, int pexp) {
  sc[4 * dc + 0] = pow2i(sa);
  sc[4 * dc + 1] = pow2i(1 - 2 * sa);
  sc[4 * dc + 2] = pow2i(-pexp);
}

// maxima -> the scales area (see the header), by the first 256 threads of one workgroup (every thread of it must call:
// barriers inside; red: 256 words).  enable = 0 writes the neutral scales.
__device__ __forceinline__ void make_scales_body(const u32* cmax, int dc, float* __restrict__ sc, int pexp, int enable,
                                                 u32* red) {
  const int t = threadIdx.x;
  if (t < 256) {
    u32 m = 0u;
    for (int c = t; c < dc; c += 256) {
      const u32 mg = load_fresh(cmax + c), mt = load_fresh(cmax + dc + c);
      const int sg = enable ? scale_exp(mg, 100) : 0, st = enable ? scale_exp(mt, 100) : 0;
      sc[c] = pow2i(sg);
      sc[dc + c] = pow2i(st);
      sc[2 * dc + c] = pow2i(-sg - pexp);
      sc[3 * dc + c] = pow2i(-st - pexp);
      m = max(m, mt);
    }
    red[t] = m;
  }
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] = max(red[t], red[t + o]);
    __syncthreads();
  }
  if (t == 0) write_global_scales(sc, dc, enable ? scale_exp(red[0], 60) : 0, pexp);
}

// column maxima of |X| [n][d] as bit patterns (non-negative floats order like unsigned integers): colmax_scan and
// colmax_commit of stein_common.h on a grid of (column blocks, row groups, matrices)
// blockIdx.z = 0: X0 -> cmax[0, dc), 1: X1 -> cmax[dc, 2 dc)
// done != NULL (fused call: both matrices given, completion counters zeroed by the prologue): the last workgroup to finish
// also turns the maxima into the scales, which saves the k_make_scales launch (round 4: a two-level count, so whatever the grid).
// V4 (fp32, d % 4 == 0, 16-byte aligned rows; 1024 threads): a lane reads four columns at once, so a wave's load is one full
// KB of a row instead of 256 bytes, sixteen waves walk sixteen rows at a time, and the workgroup's maxima are added by 256
// threads, one column each (coalesced atomics, and a quarter as many per column as with 256-thread workgroups: the
// same-address atomic chains were the larger part of the 4-byte form's 14-16 us at C3).
// The folded step that is asked for phi alone does not launch this kernel: the same body runs in the select launch's slice
// (k_spec_select, stein_select.hip); only under stein_debug_no_warm does it launch, with done = NULL.
template <typename TIN, bool V4>
__global__ __launch_bounds__(V4 ? 1024 : 256) void k_colmax(const TIN* __restrict__ X0, const TIN* __restrict__ X1, int n, int d,
                                                            u32* __restrict__ cmax0, int dc, int zbase, float* __restrict__ sc,
                                                            int pexp, HistSync* done) {
  const int z = blockIdx.z + zbase;
  constexpr int CW = V4 ? 4 : 1;                 // columns per lane
  constexpr int NW = V4 ? 16 : 4;                // waves = rows in flight per workgroup
  __shared__ u32 red[256];                       // (64 CW words for the maxima, 256 for make_scales_body)
  const int t = threadIdx.x, cx = t & 63, ry = t >> 6;
  const TIN* const X[1] = {z ? X1 : X0};
  u32 m[1][CW];
  colmax_scan<TIN, V4, 1>(X, n, d, ((int)blockIdx.x * 64 + cx) * CW, (long)blockIdx.y * NW + ry, (long)gridDim.y * NW, m);
  colmax_commit<CW, 1>(m, cx, (int)blockIdx.x, d, red, cmax0 + (z ? dc : 0), dc);
  if (done) {
    __shared__ u32 s_last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's maxima have been acknowledged
    __syncthreads();
    if (t == 0) {
      const u32 id = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
      s_last = tree_report_done(done->cm_leaf, &done->cm_top, id, gridDim.x * gridDim.y * gridDim.z) ? 1u : 0u;
    }
    __syncthreads();
    if (s_last) make_scales_body(cmax0, dc, sc, pexp, 1, red);
  }
}

// one workgroup: maxima -> the scales area
__global__ __launch_bounds__(256) void k_make_scales(const u32* __restrict__ cmax, int dc, float* __restrict__ sc, int pexp,
                                                     int enable) {
  __shared__ u32 red[256];
  make_scales_body(cmax, dc, sc, pexp, enable, red);
}

// One 64x64 tile of X [n][d] per workgroup.
//   R  != NULL: tile-major image with rows = X rows (dk / 32 k tiles per row block), fragment order, rows < r_rows, k < dk
//   Tt != NULL: tile-major image with rows = X columns (nk / 32 k tiles per row block), pre-swizzled, rows < dc, k < nk
// The grid covers the padded extents; out-of-range source entries are written as zero.
// TIN = float (KIND 2 or 3) or u16 = bf16 bits (KIND 1).  sc_all scales the row-major image, sc_col[c] column c of the
// transposed one (both powers of two; 1 unless KIND 2).
// blockIdx.z = 0: theta (row-major image R and transposed image Tt0), 1: score (transposed image Tt1 only; the grid is
// sized for theta's padded extents, blocks outside the score's exit at once)
// PRO (bf16 inputs in the fused call): the grid has one more z slice, whose workgroups do the fused call's prologue
// (prologue_body, stein_common.h: row norms, median state, tickets, neutral scales) -- bf16 planes need no scales, so
// nothing here waits for it, and the step is one launch shorter.  The split slices then must not READ the scales (the
// prologue slice writes them in the same launch): they are 1 by definition for KIND 1.
// LDS image of a transposed 64 x 64 tile, one per plane: [64 columns][32 particle pairs] of u32 (particle 2p in the low half,
// 2p + 1 in the high one: a pair is one word of the k-contiguous operand), no padding; the 16-byte slot p >> 2 of column c
// sits at slot ^ ((c >> 2) & 7).
//   ds_write_b32 (banks mod 32, 32-lane groups): a group holds the 16 column quads twice; the quads 0-7 write pairs
//     p & 3 = {0, 1}, the quads 8-15 {2, 3} (tp_pair) into eight distinct slots each: 32 distinct banks.
//   ds_read_b128 (banks mod 64, lane groups {0-3,12-15,20-27}, ...): a group holds the columns {0,3,5,6} or {1,2,4,7} (+ 8)
//     with four slots 2 quarter + e each; the two columns of equal parity differ in c >> 2, so in the slot's low bit: 16
//     distinct slots of the 256-byte bank row.
// (The image used to be [64][66] u16 written and read one half-word at a time: 32 LDS stores and 32 loads per thread and
// plane, and the kernels ran at 2.3 TB/s.)
constexpr int TP_WORDS = 64 * 32;
__device__ __forceinline__ int tp_index(int c, int p) { return c * 32 + ((((p >> 2) ^ (c >> 2)) & 7) << 2) + (p & 3); }
// the particle pair (rows 2 p, 2 p + 1 of the tile) thread t converts in pass 0 or 1; its columns are 4 (t & 15) ..+3.  Eight
// consecutive lanes still read 128 consecutive bytes of a row.
__device__ __forceinline__ int tp_pair(int t, int pass) { return 16 * pass + 4 * (t >> 6) + (((t >> 4) & 3) ^ ((t >> 2) & 2)); }

// four consecutive entries of row `row` from column `col` (col % 4 == 0), zero outside the matrix.  vec (host: fp32,
// d % 4 == 0, the matrix on a 16-byte boundary): one 16-byte load instead of four
template <typename TIN>
__device__ __forceinline__ void load_row4(const TIN* __restrict__ X, int row, int col, int n, int d, int vec, float (&v)[4]) {
  if constexpr (std::is_same<TIN, float>::value) {
    if (vec) {
      const float4 x = (row < n && col < d) ? *reinterpret_cast<const float4*>(X + (size_t)row * d + col) : make_float4(0.f, 0.f, 0.f, 0.f);
      v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
      return;
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) v[q] = (row < n && col + q < d) ? elem_f32(X + (size_t)row * d + col + q) : 0.f;
}

// the image -> the transposed planes: thread -> (parameter c = t >> 2, the 16 particles starting at j = row0 + 16 (t & 3)) =
// two 8-element chunks of the k tile, written in MFMA fragment order (vfrag_offset)
template <int KIND>
__device__ __forceinline__ void tp_store(const u32 (*tile)[TP_WORDS], u16* __restrict__ Tt, long ntk_t, int dc, long nk,
                                         int row0, int col0, int t) {
  const int c = col0 + (t >> 2), j = row0 + (t & 3) * 16;
  if (c < dc && j < nk) {   // nk % 32 == 0 and j % 16 == 0: both fragments stay inside one k tile
    const int rowc = c & 127, ch0 = (j & 31) >> 3;
#pragma unroll
    for (int s = 0; s < KIND; ++s) {
      const uint4 w0 = *reinterpret_cast<const uint4*>(&tile[s][tp_index(t >> 2, (t & 3) * 8)]);
      const uint4 w1 = *reinterpret_cast<const uint4*>(&tile[s][tp_index(t >> 2, (t & 3) * 8 + 4)]);
      u16* base = Tt + (((size_t)(c >> 7) * ntk_t + (j >> 5)) * 3 + s) * XTILE_E;
      *reinterpret_cast<uint4*>(base + vfrag_offset(rowc, ch0)) = w0;
      *reinterpret_cast<uint4*>(base + vfrag_offset(rowc, ch0 + 1)) = w1;
    }
  }
}

template <typename TIN, int KIND, bool PRO = false>
__global__ __launch_bounds__(256) void k_split(const TIN* __restrict__ X0, const TIN* __restrict__ X1, int n, int d,
                                               u16* __restrict__ R0, long r_rows, int dk, u16* __restrict__ Tt0,
                                               u16* __restrict__ Tt1, int dc, long nk, const float* __restrict__ sc,
                                               int zbase, PrologueArgs pro, int vec) {
  if (PRO && blockIdx.z == gridDim.z - 1) {
    prologue_body<TIN>(X0, pro, (int)(blockIdx.y * gridDim.x + blockIdx.x), (int)(gridDim.x * gridDim.y));
    return;
  }
  const bool score = blockIdx.z + zbase != 0;
  if (score && ((int)blockIdx.x * 64 >= dc || (long)blockIdx.y * 64 >= nk)) return;
  const TIN* __restrict__ X = score ? X1 : X0;
  u16* __restrict__ R = score ? nullptr : R0;
  u16* __restrict__ Tt = score ? Tt1 : Tt0;
  const float* __restrict__ sc_all = sc + 4 * dc;                 // scale of the row-major theta image
  const float* __restrict__ sc_col = sc + (score ? 0 : dc);       // per-column scales of this matrix
  __shared__ __attribute__((aligned(16))) u32 tile[KIND][TP_WORDS];
  const int t = threadIdx.x;
  const int row0 = blockIdx.y * 64, col0 = blockIdx.x * 64;
  const int lc = (t & 15) * 4;
  const long ntk_r = dk >> 5, ntk_t = nk >> 5;
  const float sa = (R && !PRO) ? *sc_all : 1.f;
  float scq[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) scq[q] = (!PRO && Tt && col0 + lc + q < dc) ? sc_col[col0 + lc + q] : 1.f;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int pr = tp_pair(t, p), col = col0 + lc;
    float v[2][4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = row0 + 2 * pr + h;
      load_row4(X, row, col, n, d, vec, v[h]);
      if (R && row < r_rows && col < dk) {   // col % 4 == 0: the 4 entries stay inside one 32-wide k tile
        u32 wa[3], wb[3];
        split_pair<KIND>(v[h][0] * sa, v[h][1] * sa, wa);
        split_pair<KIND>(v[h][2] * sa, v[h][3] * sa, wb);
        u16* dst = R + (((size_t)(row >> 7) * ntk_r + (col >> 5)) * 3) * XTILE_E + vfrag_offset(row & 127, (col & 31) >> 3) + (col & 7);
#pragma unroll
        for (int s = 0; s < KIND; ++s) *reinterpret_cast<uint2*>(dst + s * XTILE_E) = make_uint2(wa[s], wb[s]);
      }
    }
    if (Tt) {   // a column's two particles make one word: the terms are the same element by element
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        u32 w[3];
        split_pair<KIND>(v[0][q] * scq[q], v[1][q] * scq[q], w);
#pragma unroll
        for (int s = 0; s < KIND; ++s) tile[s][tp_index(lc + q, pr)] = w[s];
      }
    }
  }
  if (!Tt) return;
  __syncthreads();
  tp_store<KIND>(tile, Tt, ntk_t, dc, nk, row0, col0, t);
}

// k_split for the folded step that is asked for phi alone (fp32): theta's row-major image R and nothing else -- no
// transposed image, so no LDS tile -- with the image's one scale formed here instead of read: the prologue left max|theta| of
// each of its nwg workgroups in wgmax (PrologueArgs::wgmax), every workgroup reduces the words (issued in front of its row
// loads, so the two latencies overlap) to sa = scale_exp(max, 60), the value make_scales_body forms from the maximum over
// theta's column maxima, and workgroup (0, 0) writes sc[4 dc + 0 .. 2] for the distance pass, the contraction and the
// finish pass to find.  Tiles, thread mapping and arithmetic are k_split's: R keeps its bits.
__global__ __launch_bounds__(256) void k_split_rows(const float* __restrict__ X, int n, int d, u16* __restrict__ R, long r_rows,
                                                    int dk, int dc, float* __restrict__ sc, int vec,
                                                    const u32* __restrict__ wgmax, int nwg) {
  __shared__ u32 s_wmax[4];
  const int t = threadIdx.x;
  const int row0 = blockIdx.y * 64, col = blockIdx.x * 64 + (t & 15) * 4;
  const long ntk_r = dk >> 5;
  u32 m = 0u;
  for (int i = t; i < nwg; i += 256) m = max(m, wgmax[i]);
  float v[2][2][4];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int h = 0; h < 2; ++h) load_row4(X, row0 + 2 * tp_pair(t, p) + h, col, n, d, vec, v[p][h]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (u32)__shfl_xor((int)m, o));
  if ((t & 63) == 0) s_wmax[t >> 6] = m;
  __syncthreads();
  const int sae = scale_exp(max(max(s_wmax[0], s_wmax[1]), max(s_wmax[2], s_wmax[3])), 60);
  const float sa = pow2i(sae);
  if (t == 0 && blockIdx.x == 0 && blockIdx.y == 0) write_global_scales(sc, dc, sae, PEXP_H2);
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = row0 + 2 * tp_pair(t, p) + h;
      if (row < r_rows && col < dk) {   // col % 4 == 0: the 4 entries stay inside one 32-wide k tile
        u32 wa[3], wb[3];
        split_pair<2>(v[p][h][0] * sa, v[p][h][1] * sa, wa);
        split_pair<2>(v[p][h][2] * sa, v[p][h][3] * sa, wb);
        u16* dst = R + (((size_t)(row >> 7) * ntk_r + (col >> 5)) * 3) * XTILE_E + vfrag_offset(row & 127, (col & 31) >> 3) + (col & 7);
#pragma unroll
        for (int s = 0; s < 2; ++s) *reinterpret_cast<uint2*>(dst + s * XTILE_E) = make_uint2(wa[s], wb[s]);
      }
    }
}

// The folded operand (fused call, fp32 inputs; stein_fold_pays): phi_i = (sum_j K_ij w_j + rowsum_i theta_i / h2) / n with
// w_j = g_j - theta_j / h2, so the contraction multiplies K with ONE matrix.  W depends on h2: this kernel runs between the
// median and the contraction.  One 64 x 64 tile of W per workgroup, written like k_split's transposed image into Wt (the
// score's plane storage).  Column c's in-scale puts the bound max_c|g| + max_c|theta| / h2 (from the column maxima: no
// pass over the inputs) into [2^13, 2^14); it replaces the score's scales ([0, dc) and [2dc, 3dc) of the scales area).  The
// bound can be twice the true maximum of |w| and more where the terms cancel: the absolute error stays 2^-38 of the bound,
// which is what K.G and K.theta / h2 carry separately on the unfolded path.  h2 = 0: 1 / h2 = inf, the bound is inf or NaN,
// the scale 1, W holds inf / NaN and phi comes out NaN as on every other path.
__global__ __launch_bounds__(256) void k_split_w(const float* __restrict__ T, const float* __restrict__ G, int n, int d,
                                                 u16* __restrict__ Wt, int dc, long nk, float* __restrict__ sc,
                                                 const u32* __restrict__ cmax, const float* __restrict__ h2p, int vec) {
  __shared__ __attribute__((aligned(16))) u32 tile[2][TP_WORDS];
  const int t = threadIdx.x;
  const int row0 = blockIdx.y * 64, col0 = blockIdx.x * 64;
  const int lc = (t & 15) * 4;
  const long ntk_t = nk >> 5;
  const float ih = 1.f / *h2p;
  float scq[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c = col0 + lc + q;
    int se = 0;
    if (c < dc) se = scale_exp(__float_as_uint(__builtin_fmaf(__uint_as_float(cmax[dc + c]), ih, __uint_as_float(cmax[c]))), 100);
    scq[q] = pow2i(se);
    if (blockIdx.y == 0 && (t >> 4) == 0 && c < dc) {
      sc[c] = scq[q];
      sc[2 * dc + c] = pow2i(-se - PEXP_H2);
      // theta's own column scales, as make_scales_body writes them: the folded step that takes its maxima in the select
      // launch has nobody else to (elsewhere these stores repeat what is there)
      const int st = scale_exp(cmax[dc + c], 100);
      sc[dc + c] = pow2i(st);
      sc[3 * dc + c] = pow2i(-st - PEXP_H2);
    }
  }
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int pr = tp_pair(t, p), col = col0 + lc;
    float v[2][4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = row0 + 2 * pr + h;
      float th[4], g[4];
      load_row4(T, row, col, n, d, vec, th);
      load_row4(G, row, col, n, d, vec, g);
#pragma unroll
      for (int q = 0; q < 4; ++q) v[h][q] = (row < n && col + q < d) ? __builtin_fmaf(-th[q], ih, g[q]) : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      u32 w[3];
      split_pair<2>(v[0][q] * scq[q], v[1][q] * scq[q], w);
#pragma unroll
      for (int s = 0; s < 2; ++s) tile[s][tp_index(lc + q, pr)] = w[s];
    }
  }
  __syncthreads();
  tp_store<2>(tile, Wt, ntk_t, dc, nk, row0, col0, t);
}

// ------------------------------------------------------------------------------------------------
// k_distance_x3
//   Thread t stages chunk t and chunk t + 256 (row += 64) of every plane.  The tile's rows may straddle two row
//   blocks of T3, so each thread keeps its two source pointers; k tile / plane steps are uniform immediates.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ const u16* t3_chunk_ptr(const u16* __restrict__ T3, long ntk, long grow, int c16) {
  return T3 + ((size_t)(grow >> 7) * ntk * 3) * XTILE_E + vfrag_offset((int)(grow & 127), c16);
}

template <int NP>
__device__ __forceinline__ void t3_load(const u16* __restrict__ p0, const u16* __restrict__ p1, int kt, u32x4 (&reg)[6]) {
#pragma unroll
  for (int s = 0; s < NP; ++s) {
    reg[s * 2 + 0] = *reinterpret_cast<const u32x4*>(p0 + ((size_t)kt * 3 + s) * XTILE_E);
    reg[s * 2 + 1] = *reinterpret_cast<const u32x4*>(p1 + ((size_t)kt * 3 + s) * XTILE_E);
  }
}

template <int NP>
__device__ __forceinline__ void x3_store_swz(unsigned char* oper, int t, const u32x4 (&reg)[6]) {
#pragma unroll
  for (int s = 0; s < NP; ++s)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int chunk = t + 256 * q;
      *reinterpret_cast<u32x4*>(oper + s * XPLANE + (chunk >> 2) * XROW + xswz(chunk >> 2, chunk & 3)) = reg[s * 2 + q];
    }
}

// The products of one fragment pair on the 32x32x16 shape, smallest first (plane 0 = most significant term; NP planes:
// 2 -> three fp16 products, 1 -> one bf16 product).  X3_BF / X3_HF and the 16x16x32 form: stein_x3_dev.h
template <int NP>
__device__ __forceinline__ f32x16 x3_products(const u32x4 (&a)[3], const u32x4 (&b)[3], f32x16 c) {
  if (NP == 2) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(X3_HF(a[1]), X3_HF(b[0]), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(X3_HF(a[0]), X3_HF(b[1]), c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(X3_HF(a[0]), X3_HF(b[0]), c, 0, 0, 0);
  }
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(X3_BF(a[0]), X3_BF(b[0]), c, 0, 0, 0);
}


// one 32-deep k tile already in LDS: 2 k16 steps x (2x2 tiles) x NP-dependent products
template <int NP>
__device__ __forceinline__ void x3_mma_tile(const unsigned char* As, const unsigned char* Bs, int wy, int wx, int lane,
                                            f32x16 (&acc)[2][2]) {
  const int l31 = lane & 31, h = lane >> 5;
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    u32x4 a[2][3], b[2][3];
    const int co = xswz(l31, 2 * ks + h);   // (row >> 2) & 3 only depends on row mod 16 = l31 mod 16
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int s = 0; s < NP; ++s) {
        a[i][s] = *reinterpret_cast<const u32x4*>(As + s * XPLANE + (wy * 64 + i * 32 + l31) * XROW + co);
        b[i][s] = *reinterpret_cast<const u32x4*>(Bs + s * XPLANE + (wx * 64 + i * 32 + l31) * XROW + co);
      }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = x3_products<NP>(a[i], b[j], acc[i][j]);
  }
}

template <bool SYM, int NP>
__global__ __launch_bounds__(NTHREADS, 3) void k_distance_x3(const u16* __restrict__ T3, int ntk,
                                                             const float* __restrict__ r, float* __restrict__ D, int n,
                                                             int row0, int n_local, long ldD, int tiles_m, int tiles_n,
                                                             u64* __restrict__ hist0, const float* __restrict__ two_s,
                                                             SpecState* __restrict__ spec, u64* __restrict__ spec_buf) {
  // two operand tiles in the main loop; the epilogue reuses the array (EPI_LDS_BYTES)
  constexpr int OP = NP * XPLANE;   // one operand tile: NP planes
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * OP > EPI_LDS_BYTES ? 2 * OP : EPI_LDS_BYTES];
  unsigned char* As = smem;
  unsigned char* Bs = smem + OP;
  int tile_m, tile_n;
  if (!distance_tile<SYM>(xcd_remap(blockIdx.x, gridDim.x), tiles_m, tiles_n, tile_m, tile_n)) return;
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int wy = wid >> 1, wx = wid & 1;
  const long arow0 = row0 + (long)tile_m * BM, brow0 = (long)tile_n * BN;
  const EpiPrefetch pf = distance_epilogue_prefetch(r, n, row0, n_local, tile_m, tile_n, spec);
  const float two_s_v = *two_s;

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const u16* __restrict__ pa0 = t3_chunk_ptr(T3, ntk, arow0 + (t >> 2), t & 3);
  const u16* __restrict__ pa1 = t3_chunk_ptr(T3, ntk, arow0 + (t >> 2) + 64, t & 3);
  const u16* __restrict__ pb0 = t3_chunk_ptr(T3, ntk, brow0 + (t >> 2), t & 3);
  const u16* __restrict__ pb1 = t3_chunk_ptr(T3, ntk, brow0 + (t >> 2) + 64, t & 3);
  // the next k tile's operands are prefetched into registers under the MFMAs (a second register set, two tiles
  // ahead, bought nothing and costs the third workgroup per CU)
  u32x4 ra[6], rb[6];
  t3_load<NP>(pa0, pa1, 0, ra);
  t3_load<NP>(pb0, pb1, 0, rb);
  for (int kt = 0; kt < ntk; ++kt) {
    x3_store_swz<NP>(As, t, ra);
    x3_store_swz<NP>(Bs, t, rb);
    __syncthreads();
    if (kt + 1 < ntk) {
      t3_load<NP>(pa0, pa1, kt + 1, ra);
      t3_load<NP>(pb0, pb1, kt + 1, rb);
    }
    x3_mma_tile<NP>(As, Bs, wy, wx, lane, acc);
    __syncthreads();
  }
  // SYM: only the tiles on and above the diagonal are stored (the contraction reads the others transposed)
  distance_epilogue<SYM, false>(acc, reinterpret_cast<u32*>(smem), D, n, n_local, ldD, tile_m, tile_n, hist0, pf,
                                two_s_v, spec, spec_buf);
}

// ------------------------------------------------------------------------------------------------
// k_phi_x3fs: the contraction, warp-specialised, V fragments streamed straight from L2.
//   History (measured with per-phase cycle stamps): a monolithic kernel (every wave stages, then every wave multiplies)
//   fell into lockstep phases; a producer/consumer split that staged P AND the V tiles through LDS was bound by its
//   producers (64 KB of loads per k tile accepted at the vector-L1 rate while they also ran the exp/split VALU work).
//   Here a 768-thread workgroup owns a 128 x 256 tile of [K.G | K.theta]:
//     waves 0-3   PRODUCERS  load the D tile, P = exp2(c D), split into 16-bit planes, fill LDS stage (it+1) & 1
//     waves 4-11  CONSUMERS  each owns all 128 rows x 32 columns: A fragments (P) by ds_read from LDS stage it & 1,
//                            B fragments (V) by one coalesced 1 KB global load each, issued one k tile ahead right
//                            after the registers' last use; 48 MFMAs per k tile and wave
//   Every SIMD holds one producer and two consumers.  V never touches LDS and is fetched exactly once per workgroup
//   (no two waves share a B fragment).  One barrier per pipeline stage (four k tiles)
//   hands the P stages over.
//   Column space: the 128-column blocks of [G | theta] (each matrix padded to dc = roundup(d, 128)) are paired up,
//   block cb covers pair (2cb, 2cb+1); consumer wave cw takes half cw >> 2, 32-column block cw & 3.
// ------------------------------------------------------------------------------------------------
constexpr int FS_THREADS = 768;

// ---- streamed loads with hand-counted waits ---------------------------------------------------------------------
// The contraction's two roles each keep global loads in flight ACROSS loop iterations (D tiles four k tiles ahead -- two on
// the folded path, see PD --, V fragments one k tile ahead).  hipcc counts its own loads' s_waitcnt conservatively across
// a loop back-edge: in front of the first use of a tile it emitted vmcnt(3) ... vmcnt(0), which also waits for the loads
// issued a moment earlier for LATER tiles -- every k tile then paid a full memory latency and the "prefetch" was one tile
// deep at best (round-2 finding: the producers needed 1900 cycles per k tile for 500 cycles of work, the matrix waves
// idled 40 % of the time).
// So these loads are inline asm, which the compiler neither counts nor waits for (cdna_hip_programming.md 5.7), and the
// waits are written by hand: stream_wait<N> lets the N youngest loads of the wave stay in flight; the scheduling fence
// behind it keeps every use of the loaded registers below the wait (an MFMA is not a memory operation: "memory" alone
// does not hold it, cdna_hip_programming.md 5.4 rule 18).  The registers are deliberately NOT operands of the wait: tied
// "+v" operands made the compiler copy the (not yet landed) registers in front of the wait.  Loads complete in issue
// order per wave.  After every change here: check in the .s that no v_mov / spill touches a destination register between
// its load and its wait.
// (stream_load16 / stream_wait: stein_x3_dev.h)
// The workgroup's tile: 128 rows x 256 columns of [G | theta].  A matrix wave owns the 8 sixteen-row blocks x 2
// sixteen-column blocks of its 32 columns (8 x 2 x products = 48 MFMAs per k tile and wave for NP 2); a producer thread
// holds 4 rows x 4 columns of every k tile.  (A 64-row x 512-column form, which builds the P tile once per 512 columns,
// was measured in round 2 -- equal within 1 % -- and removed)
constexpr int FS_KT = 4;                 // k tiles per pipeline stage (even: tile parity picks the register set)
constexpr int FS_ROWS = 128;
constexpr int FS_IB = FS_ROWS / 16;      // 16-row blocks of the tile
constexpr int CJ = 2;                    // 16-column blocks per matrix wave (8 waves: 256 columns)
constexpr int PR = FS_ROWS / 32;         // producer: rows lr + 32 p per thread and tile (4 columns each)
constexpr int PLN = FS_ROWS * XROW;      // one plane of one k tile in LDS: [128][64 B]

//   FOLD (the fused call's folded operand, fp32 inputs): the column space is ONE matrix of `cblocks` 128-column blocks,
//   W = G - theta / h2 (Gt3 holds its planes), paired into wpm = ceil(cblocks / 2) workgroups per row tile (an odd count
//   leaves the last with one block: its second half of matrix waves repeats the first block and stores nothing), times
//   `split` j ranges.  When dK or the Stein discrepancy is asked for, the grid carries tiles_m x wpm more workgroups behind
//   those: the same for theta (Tt3 -> OT), each over the whole j range.  The workgroups of W do not know whether they are
//   there: same ids, same k order, so phi is the same to the bit with and without dK_out.
template <int NP, bool FOLD = false>
__global__ __launch_bounds__(FS_THREADS) void k_phi_x3fs(const float* __restrict__ D, long ldD,
                                                         const u16* __restrict__ Gt3, const u16* __restrict__ Tt3,
                                                         long ntj, const float* __restrict__ h2p,
                                                         float* __restrict__ OG, float* __restrict__ OT,
                                                         float* __restrict__ RS, int n, int d, int n_local,
                                                         int tiles_m, int cblocks, int split, int jchunk,
                                                         const float* __restrict__ sc, int dc, int upper) {
  // cblocks: 128-column blocks per matrix; wpm: workgroups per row tile and j range (not FOLD: = cblocks, a workgroup takes
  // one block pair of [G | theta])
  const int wpm = FOLD ? (cblocks + 1) >> 1 : cblocks;
  constexpr int FS_KTB = NP * PLN;            // one k tile in LDS: NP planes, packed
  constexpr int FS_STAGE = FS_KT * FS_KTB;    // 2 stages x FS_KT x NP x 8 KB: 128 KB (NP 2), 64 KB (NP 1)
  // (+ 1 KB behind the stages: the row-sum exchange of the `up` path, which the output image below does not cover)
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * FS_STAGE + 1024];

  const int logical = xcd_remap(blockIdx.x, gridDim.x);
  // Which (row tile, column block) a workgroup takes.  An XCD runs 32 consecutive logical ids at a time (one workgroup per
  // CU) and its 4 MB L2 is what they share: the workgroups of one row tile read the same D tiles, the workgroups of one
  // column block the same V fragments.  With R row tiles x C column blocks resident, a launch pulls D (16 / C) times and V
  // (tiles_m / R) times from beyond the L2.  Up to 4 column blocks (d <= 256) all of a row tile's workgroups are neighbours
  // anyway; a wide [G | theta] (C4: 16 column blocks) dealt that way made an XCD 2 row tiles x 16 blocks -- V, 134 MB, came
  // in 32 times (4.8 GB of HBM traffic per launch by the counters); 8 row tiles x 4 blocks asks for both four to eight times.
  int cb, tile_m;
  const int plane = wpm * tiles_m;
  const int half = FOLD && logical >= plane * split ? 1 : 0;   // FOLD: the workgroups behind W's are theta's (one j range)
  const int lw = FOLD ? logical - half * plane * split : logical;
  const int l2 = lw % plane;
  const int z = lw / plane;
  if (wpm > 4 && (wpm & 3) == 0 && (tiles_m & 7) == 0) {
    const int sb = l2 >> 5, in = l2 & 31, cgroups = wpm >> 2;
    cb = (sb % cgroups) * 4 + (in & 3);
    tile_m = (sb / cgroups) * 8 + (in >> 2);
  } else {
    cb = l2 % wpm;
    tile_m = l2 / wpm;
  }
  const int i0 = tile_m * FS_ROWS;
  const int jbeg = z * jchunk;
  const int jend = half ? n : min(n, jbeg + jchunk);
  const int ntile = jend > jbeg ? (jend - jbeg + BK - 1) / BK : 0;
  // Visit order of the k tiles inside a pipeline stage.  The `cblocks` workgroups of a row tile all stream the same D row
  // block.  Walking it in step, each of them waits out the full HBM latency of every tile (a request that arrives while
  // another workgroup's fill of the same line is in flight waits for that fill), and a CU holds only ~25 KB of misses in
  // flight.  So workgroup cb walks the FS_KT tiles of a full stage rotated by rot = cb * FS_KT / min(cblocks, FS_KT): at any
  // time the workgroups of a row tile request DIFFERENT tiles, each tile is pulled from HBM by one of them and found in
  // the XCD's L2 a tile or two later by the others (a lag of whole stages, 64 KB per workgroup, did not survive in the
  // 4 MB L2 that 32 CUs share: measured slower).  Slot u of the LDS stage holds tile stage * FS_KT + ((u + rot) % FS_KT);
  // the partial last stage keeps its order.  (The order of the k tiles inside the fp32 accumulation changes with it --
  // deterministically.)
  const int nstage = (ntile + FS_KT - 1) / FS_KT;
  const int rot = (cb % FS_KT) * (wpm >= FS_KT ? 1 : FS_KT / wpm) % FS_KT;
  // Visit order of the STAGES (upper, one workgroup per row tile and column block over the whole j range, a power-of-two number
  // of row tiles): stage v of the row tiles that share an XCD (`group` consecutive ones: 32 logical ids / cblocks) is the
  // 128-column block v ^ (tile_m & ~(group - 1)).  Every stored tile D[I][J] is read twice, by row tile I as itself and by
  // row tile J as its mirror image; in the plain order 0, 1, 2 ... the two reads lie |I - J| stages apart (43 on average,
  // 16 MB of D traffic per stage: the second read comes from HBM again), in this order |I % group - J % group| < group
  // stages apart (5 on average), where the memory-side cache still holds the tile.  The row tiles of an XCD keep walking the
  // SAME block at the same time, so V is shared in their L2 as before.
  // FOLD: the halved grid is split over j to fill the chip (C3: two ranges of 64 stages), and every range is walked this way:
  // stage v of a range is its block v ^ (tile_m & ~(group - 1) & (nstage - 1)).  The two reads of a stored tile, by row tiles
  // I and J in whichever ranges, are then (I ^ J) & (group - 1) < group stages apart as before, all ranges running at once.
  // (Folded C3 has wpm = 1, group = 32: the two reads lie 10.7 stages apart on average.  Groups of 16 and of 8 row tiles
  // halve and quarter that and were measured equal and 1 % slower: the launch's 1.13 GB from beyond the L2 are every D
  // tile twice plus V, whatever the order, and the launch does not wait for where they come from;
  // profiles/contract_feed_ab.txt, 1. and 3.)
  const int group = wpm <= 32 ? 32 / wpm : 1;
  const bool permute = upper != 0 && (FOLD || (jbeg == 0 && jend == n && nstage == tiles_m)) && (wpm & (wpm - 1)) == 0 &&
                       wpm <= 4 && nstage * FS_KT == ntile && (nstage & (nstage - 1)) == 0 && nstage >= 2 * group;
  const int xmask = permute ? (tile_m & ~(group - 1) & (nstage - 1)) : 0;
  auto stage_of = [&](int v) { return v ^ xmask; };   // (v = nstage, "the stage after the last", stays out of range)
  auto tile_at = [&](int stage, int u) {     // u may run past the stage: u >= FS_KT continues in the next stage
    const int st2 = stage_of(stage + u / FS_KT), u2 = u % FS_KT;
    return st2 * FS_KT + ((st2 + 1) * FS_KT <= ntile ? ((u2 + rot) & (FS_KT - 1)) : u2);
  };

  // upper (single rank, D holds only the 128 x 128 tiles on and above the diagonal): the k tiles left of this row tile's
  // diagonal block are read from their mirror image D[j][i].  The producers gather such a tile with a row-per-lane-group
  // map (below) that leaves every thread holding 4 consecutive j of 4 rows i, so it is written into the SAME natural LDS
  // image with the same number of 8-byte stores: the matrix waves do not know the difference.  The choice is per pipeline
  // stage (FS_KT k tiles = 128 columns; the host keeps jbeg a multiple of 128, so a stage never straddles the diagonal
  // block): the first ntr stages of the j range are mirrored ones.
  const bool up = upper != 0;
  const int ntr = up ? max(0, min(nstage, (i0 - jbeg) / (FS_KT * BK))) : 0;

  const int t = threadIdx.x;
  // ---- the output tail: the partial sums leave through LDS in whole lines ------------------------------------------------
  // An accumulator is four ROWS of one column, so a matrix wave's own store is a dword per lane and touches four 64-byte
  // half lines per instruction: 64 such stores per lane, 128 KB per workgroup, while the producers idle -- and the tail of a
  // kernel that runs one workgroup per CU in a single round is all exposed.  Instead: behind the loop's last barrier the
  // stage buffers are dead; the matrix waves write their scaled accumulators (the same multiplication as before: the same
  // bits) into an image of the workgroup's tile there, one barrier, and all twelve waves store the image row-major with
  // 16-byte stores, eight consecutive lanes to a 128-byte line.
  //   Image: unit (c, rg) = the 16 bytes { rows 4 rg .. 4 rg + 3 of image column c } at byte rg * IMG_PITCH +
  //   16 * (c ^ (rg & 3)): row-group-major, one row group = IMG_COLS units.  NP 2: all 256 columns, 128 KB = both stages;
  //   NP 1 (64 KB of stages): 128 columns, the two halves of the matrix waves one after the other (two more barriers).
  //   Writes (ds_write_b128: groups of 8 contiguous lanes, 32 banks): the lanes of a group are 8 consecutive columns of one row
  //   group, and the XOR permutes inside aligned fours: 8 distinct 16-byte slots of a 128-byte bank row.  Reads, 16-byte form
  //   (ds_read_b128: lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31} and the same + 32, 64 banks): lane l reads column
  //   4 (l & 7) + k of row group R + (l >> 3), so a group holds every (l & 3) once in each of four row groups with four
  //   different rg & 3: slot ((4 (l & 3) + k) ^ (rg & 3)) & 15 takes all 16 values.  4-byte form: a wave reads 64 consecutive
  //   columns of one row group, a lane group sees 16 different c & 15 under one XOR.  No conflicts in any of the three.
  //   The row-sum exchange of the `up` path has 1 KB of its own behind the stages, so it needs no barrier of its own any
  //   more: the image's barrier orders it, on every path both roles pass 1 (NP 2) or 3 (NP 1) barriers behind the loop.
  constexpr int IMG_COLS = NP == 2 ? 256 : 128;
  constexpr int IMG_PITCH = IMG_COLS * 16;
  constexpr int IMG_PASSES = 256 / IMG_COLS;
  static_assert(32 * IMG_PITCH <= 2 * FS_STAGE, "the output image lives in the stage buffers");
  // 16-byte stores need rows on 16-byte boundaries (d % 4 == 0 makes every z slice and row start one if the bases are).
  // OG and OT are workspace sections, each a multiple of 256 bytes from the workspace's base (stein_make_layout), so the
  // pointer half of this test only fails for a workspace that is itself off a 16-byte boundary -- which no allocation of the
  // package is, and which finish_stage (steinhip.hip) allows for in the same way.  The loop it then takes is the one every
  // d % 4 != 0 call takes.
  const bool vec16 = (d & 3) == 0 && ((((size_t)OG) | ((size_t)OT)) & 15) == 0;
  auto image_store = [&](int ps) {   // all twelve waves; ps: which half of the column pair the image holds (NP 1)
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6), ln = t & 63;
    if (vec16) {
      // task = 8 row groups (32 rows) x 32 columns: four reads and four stores per lane, a store = 8 rows x one whole line
      constexpr int MB = IMG_COLS / 32, NT = 4 * MB;
#pragma unroll
      for (int q = 0; q < (NT + 11) / 12; ++q) {
        const int task = wv + 12 * q;
        if (task >= NT) break;
        const int mb = task % MB, rg = (task / MB) * 8 + (ln >> 3);
        const int g = 2 * cb + (NP == 2 ? mb >> 2 : ps);
        if (FOLD && g >= cblocks) continue;   // (an odd block count: this half stores nothing)
        const bool first = FOLD ? half == 0 : g < cblocks;
        float* __restrict__ Oz = (first ? OG : OT) + (size_t)z * n_local * d;
        const int c = 32 * mb + 4 * (ln & 7);
        const int col = (FOLD || first ? g : g - cblocks) * BN + (c & (BN - 1));
        const int row = i0 + 4 * rg;
        if (col < d && row < n_local) {
          const unsigned char* src = smem + rg * IMG_PITCH;
          f32x4 u[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) u[k] = *reinterpret_cast<const f32x4*>(src + (((c + k) ^ (rg & 3)) * 16));
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (row + e < n_local)
              *reinterpret_cast<f32x4*>(Oz + (size_t)(row + e) * d + col) = f32x4{u[0][e], u[1][e], u[2][e], u[3][e]};
        }
      }
    } else {
      // item = one row group x 64 columns: one read and four dword stores per lane, a store = 256 consecutive bytes of a row
      constexpr int CH = IMG_COLS / 64, NI = 32 * CH;
      for (int item = wv; item < NI; item += 12) {
        const int ch = item % CH, rg = item / CH;
        const int g = 2 * cb + (NP == 2 ? ch >> 1 : ps);
        if (FOLD && g >= cblocks) continue;
        const bool first = FOLD ? half == 0 : g < cblocks;
        float* __restrict__ Oz = (first ? OG : OT) + (size_t)z * n_local * d;
        const int c = 64 * ch + ln;
        const int col = (FOLD || first ? g : g - cblocks) * BN + (c & (BN - 1));
        const int row = i0 + 4 * rg;
        if (col < d && row < n_local) {
          const f32x4 u = *reinterpret_cast<const f32x4*>(smem + rg * IMG_PITCH + ((c ^ (rg & 3)) * 16));
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (row + e < n_local) Oz[(size_t)(row + e) * d + col] = u[e];
        }
      }
    }
  };
  // The two roles run separate loops (so neither carries the other's registers) with the same number of
  // barriers: one after the prologue, one per k tile.  The role test is wave-uniform (waves 0-3 / 4-11).
  if (t < 256) {
    // ================================ PRODUCER ================================
    const int pt = t;
    const int lr = pt >> 3, lc = (pt & 7) * 4;   // P staging: rows lr + 32p, 4 consecutive j
    float rs[PR];
#pragma unroll
    for (int p = 0; p < PR; ++p) rs[p] = 0.f;
    // PD register sets (tile index mod PD picks the set): the loads of tile t + PD are issued as soon as tile t has been
    // turned into LDS data.  D streams from beyond the L2, so the loads need more than one tile of lead -- and no more than
    // the CU can hold in flight.  FOLD: 2.  A folded workgroup is the only reader of its D tiles on its XCD (unfolded,
    // `rot` lets the workgroups of a row tile find every other tile in the L2), so all 16 KB per k tile come from beyond
    // the L2; four tiles ahead that is 64 KB per CU, and the launch was 17 us (4.7 %) SLOWER at C3 than two tiles ahead
    // (one tile ahead: 1 % slower than four; profiles/contract_feed_ab.txt, 3.).  Unfolded the lead stays at 4: 8192 x 128
    // measured 1 % slower with 2.
    constexpr int PD = FOLD ? 2 : FS_KT;   // FS_KT % PD == 0 keeps the set index static
    f32x4g rd[PD][PR];
    u32 doff[PR];
    const float cexp = -1.44269504088896341f / (2.f * *h2p);   // exp(-D/(2 h2)) = exp2(cexp * D)
    constexpr float pofs = (float)SplitTraits<NP>::pexp;        // P carries 2^pexp (undone by the out-scales)
    // the D tile (tile_m, j0 / 32) is one contiguous [128][32] block of the tile-major distance image (rows past
    // n_local exist as padding and only feed accumulator rows that are never stored)
#pragma unroll
    for (int p = 0; p < PR; ++p) doff[p] = (u32)(((i0 & (DT_ROWS - 1)) + lr + 32 * p) * DT_COLS + lc);
    const float* __restrict__ drow = D + (size_t)(i0 / DT_ROWS) * (ldD >> 5) * DT_ELEMS;
    // mirrored source (upper): wave w gathers from mirror tile w (columns i0 + 32 w .. + 31); thread (c = pt & 7,
    // jq = (pt >> 3) & 7) loads D[j0 + 4 jq + u][i0 + 4 ig .. + 3], ig = 8 w + c, u = 0..3: a quarter wave reads two full
    // 128-byte lines, like the natural map (lanes along j first made every quarter wave touch eight lines: the producers
    // took 2500 instead of 1500 cycles per k tile).  Afterwards the thread holds P(i = 4 ig + e, j = 4 jq + u): four
    // consecutive j of four rows = one 8-byte LDS store per row and plane at row 4 ig + e, byte 8 jq of the natural image
    const int jq = (pt >> 3) & 7, ig = (pt >> 6) * 8 + (pt & 7);
    u32 doff_tr[PR];
#pragma unroll
    for (int u = 0; u < PR; ++u) doff_tr[u] = (u32)((ig >> 3) * DT_ELEMS + (4 * jq + u) * DT_COLS + 4 * (ig & 7)) * 4u;
    const long ntc_d = ldD >> 5;
    float rst[4] = {0.f, 0.f, 0.f, 0.f};   // row sums over the mirrored tiles: rows i0 + 4 ig + e
    // one call site for both sources (base and offsets selected first): a load instruction in each arm of a branch would
    // let the compiler reconcile the two destination registers with copies of registers that are still in flight
    auto request = [&](int j0, bool tr, f32x4g (&rd)[PR]) {
      const float* tile = tr ? D + ((size_t)(j0 >> 7) * ntc_d + 4 * (size_t)(i0 / DT_ROWS)) * DT_ELEMS + (j0 & 127) * DT_COLS
                             : drow + (size_t)(j0 >> 5) * DT_ELEMS;
#pragma unroll
      for (int p = 0; p < PR; ++p) stream_load16(rd[p], tile, tr ? doff_tr[p] : doff[p] * 4u);
    };
    // before tile number v (in visit order) of the ntile is turned into LDS data: its PR loads must have landed, the loads
    // of the up to PD - 1 later tiles already requested (PR each) stay in flight
    auto wait_loads = [&](int v, f32x4g (&rd)[PR]) {
      const int later = ntile - v - 1;
      (void)rd;
      // (nested, the loosest wait first and unconditional: every path from a request to its use passes a wait, which is
      // what stein_amd/csrc/isa_check.py verifies on the assembly)
      if constexpr (PD == 4) {
        stream_wait<3 * PR>();
        if (later < 3) {
          stream_wait<2 * PR>();
          if (later < 2) {
            stream_wait<PR>();
            if (later < 1) stream_wait<0>();
          }
        }
      } else {
        static_assert(PD == 2 || PD == 4, "wait_loads is written out for these two leads");
        stream_wait<PR>();
        if (later < 1) stream_wait<0>();
      }
    };
    // registers of tile j0 -> LDS stage `buf`
    // One k tile: 16 entries per thread, done phase by phase over all 16 (fma, exp, row sums, hi terms, residuals, lo
    // terms, stores) with scheduling fences between the phases.  Entry by entry the stream is a chain of dependent
    // instructions (cvt -> fma_mix -> cvt -> store), and next to two matrix waves on the SIMD a dependent instruction waits
    // for the next free issue window: measured ~16 cycles per instruction.  Sixteen independent instructions per phase
    // fill the windows.
    auto produce = [&](int j0, unsigned char* buf, const f32x4g (&rd)[PR]) {
      const bool full = j0 + BK <= jend;
      float q[PR][4];
#pragma unroll
      for (int p = 0; p < PR; ++p)
#pragma unroll
        for (int e = 0; e < 4; ++e) q[p][e] = __builtin_fmaf(cexp, rd[p][e], pofs);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int p = 0; p < PR; ++p)
#pragma unroll
        for (int e = 0; e < 4; ++e) q[p][e] = __builtin_amdgcn_exp2f(q[p][e]);
      __builtin_amdgcn_sched_barrier(0);
      if (!full) {   // columns past jend hold whatever the padding holds: force P = 0 there
        const int j = j0 + lc;
#pragma unroll
        for (int p = 0; p < PR; ++p)
#pragma unroll
          for (int e = 0; e < 4; ++e) q[p][e] = (j + e < jend) ? q[p][e] : 0.f;
      }
      if (NP >= 2) {
        u32 hi[PR][2], lo[PR][2];
        float r[PR][4];
#pragma unroll
        for (int p = 0; p < PR; ++p) rs[p] += (q[p][0] + q[p][1]) + (q[p][2] + q[p][3]);
#pragma unroll
        for (int p = 0; p < PR; ++p) { hi[p][0] = cvt_pk_f16(q[p][0], q[p][1]); hi[p][1] = cvt_pk_f16(q[p][2], q[p][3]); }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int p = 0; p < PR; ++p) {
          r[p][0] = f16_resid_lo(hi[p][0], q[p][0]); r[p][1] = f16_resid_hi(hi[p][0], q[p][1]);
          r[p][2] = f16_resid_lo(hi[p][1], q[p][2]); r[p][3] = f16_resid_hi(hi[p][1], q[p][3]);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int p = 0; p < PR; ++p) { lo[p][0] = cvt_pk_f16(r[p][0], r[p][1]); lo[p][1] = cvt_pk_f16(r[p][2], r[p][3]); }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int p = 0; p < PR; ++p) {
          unsigned char* dst = buf + (lr + 32 * p) * XROW + pswz(lr, lc >> 3) + (lc & 4) * 2;   // (lr+32p)>>2&3 == lr>>2&3
          *reinterpret_cast<uint2*>(dst) = make_uint2(hi[p][0], hi[p][1]);
          *reinterpret_cast<uint2*>(dst + PLN) = make_uint2(lo[p][0], lo[p][1]);
        }
      } else {
#pragma unroll
        for (int p = 0; p < PR; ++p) {
          // bf16 operands: K is rounded to bf16 once and BOTH uses of it (K.theta in the MFMA and rowsum(K) here) see
          // the rounded value, so the repulsion term sum_j K_ij (theta_i - theta_j) stays consistent
          unsigned char* dst = buf + (lr + 32 * p) * XROW + pswz(lr, lc >> 3) + (lc & 4) * 2;
          const u32 h0 = cvt_pk_bf16(q[p][0], q[p][1]), h1 = cvt_pk_bf16(q[p][2], q[p][3]);
          rs[p] += (__uint_as_float(h0 << 16) + __uint_as_float(h0 & 0xffff0000u)) +
                   (__uint_as_float(h1 << 16) + __uint_as_float(h1 & 0xffff0000u));
          *reinterpret_cast<uint2*>(dst) = make_uint2(h0, h1);
        }
      }
    };
    // the same for a tile read from its mirror image (always a full tile): rd[u][e] = D[j = 4 jq + u][i = 4 ig + e].
    // (The row sums below run along e, i.e. over adjacent registers: under plain -O3 the SLP vectoriser turned them into
    // v_pk_add_f32, and eight packed adds per k tile beside the MFMAs cost the launch 0.07 ms -- the library is built with
    // -fno-slp-vectorize, __graft_entry__.py.)
    auto produce_tr = [&](unsigned char* buf, const f32x4g (&rd)[PR]) {
      float q[4][4];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) q[u][e] = __builtin_fmaf(cexp, rd[u][e], pofs);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) q[u][e] = __builtin_amdgcn_exp2f(q[u][e]);
      __builtin_amdgcn_sched_barrier(0);
      u32 hi[4][2], lo[4][2];   // [row e][j pair]
      if (NP >= 2) {
        float r[4][4];
#pragma unroll
        for (int e = 0; e < 4; ++e) rst[e] += (q[0][e] + q[1][e]) + (q[2][e] + q[3][e]);
#pragma unroll
        for (int e = 0; e < 4; ++e) { hi[e][0] = cvt_pk_f16(q[0][e], q[1][e]); hi[e][1] = cvt_pk_f16(q[2][e], q[3][e]); }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          r[e][0] = f16_resid_lo(hi[e][0], q[0][e]); r[e][1] = f16_resid_hi(hi[e][0], q[1][e]);
          r[e][2] = f16_resid_lo(hi[e][1], q[2][e]); r[e][3] = f16_resid_hi(hi[e][1], q[3][e]);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int e = 0; e < 4; ++e) { lo[e][0] = cvt_pk_f16(r[e][0], r[e][1]); lo[e][1] = cvt_pk_f16(r[e][2], r[e][3]); }
        __builtin_amdgcn_sched_barrier(0);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {   // bf16: the row sums see the ROUNDED values, as in the natural tiles
          hi[e][0] = cvt_pk_bf16(q[0][e], q[1][e]); hi[e][1] = cvt_pk_bf16(q[2][e], q[3][e]);
          lo[e][0] = lo[e][1] = 0u;
          rst[e] += (__uint_as_float(hi[e][0] << 16) + __uint_as_float(hi[e][0] & 0xffff0000u)) +
                    (__uint_as_float(hi[e][1] << 16) + __uint_as_float(hi[e][1] & 0xffff0000u));
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = 4 * ig + e;   // (row >> 2) & 3 == ig & 3
        unsigned char* dst = buf + row * XROW + pswz(row, jq >> 1) + (jq & 1) * 8;
        *reinterpret_cast<uint2*>(dst) = make_uint2(hi[e][0], hi[e][1]);
        if (NP >= 2) *reinterpret_cast<uint2*>(dst + PLN) = make_uint2(lo[e][0], lo[e][1]);
      }
    };
    auto jt = [&](int tile) { return jbeg + tile * BK; };   // tile index -> first column (jbeg % 32 == 0)
    // A pipeline stage holds FS_KT consecutive k tiles, so the workgroup synchronises once per FS_KT tiles.  The tile's
    // position mod PD picks the register set; a tile's loads are issued PD tiles ahead, right after the set is free.
#pragma unroll
    for (int u = 0; u < PD; ++u)
      if (tile_at(0, u) < ntile) request(jt(tile_at(0, u)), stage_of(0) < ntr, rd[u]);
    // stage st: turn the registers of its tiles into LDS data (slot u <- tile_at(st, u)); behind each, request the tile PD
    // positions on (slot u + PD: of the next stage from u + PD >= FS_KT on, with that stage's source)
    auto produce_stage = [&](int st, unsigned char* buf) {
      const bool tr_now = stage_of(st) < ntr;   // workgroup-uniform
#pragma unroll
      for (int u = 0; u < FS_KT; ++u) {
        const int tile_u = tile_at(st, u), next_u = tile_at(st, u + PD);
        const bool tr_next = stage_of(st + (u + PD) / FS_KT) < ntr;
        if (tile_u < ntile) {
          wait_loads(st * FS_KT + u, rd[u % PD]);   // (tiles are requested in visit order: position = st * FS_KT + u)
          if (tr_now) produce_tr(buf + u * FS_KTB, rd[u % PD]);
          else produce(jt(tile_u), buf + u * FS_KTB, rd[u % PD]);
        }
        if (next_u < ntile) request(jt(next_u), tr_next, rd[u % PD]);
      }
    };
    produce_stage(0, smem);
    __syncthreads();
    // iteration st (consumers are on stage st): fill stage st+1 into the other buffer
    for (int st = 0; st < nstage; ++st) {
      if (st + 1 < nstage) produce_stage(st + 1, smem + ((st + 1) & 1) * FS_STAGE);
      __syncthreads();
    }
    if (up) {
      // natural tiles: rows lr + 32 p, the 8 threads of a row are 8 consecutive lanes; mirrored tiles: rows 4 ig + e, the 8
      // threads of a row are the lanes jq = 0..7 (lane bits 3..5).  The two row sets meet in LDS (behind the stage buffers,
      // where the matrix waves are writing the output image by now; the image's barrier orders the exchange) and are added
      // in a fixed order.
      float* red = reinterpret_cast<float*>(smem + 2 * FS_STAGE);   // [128] natural sums | [128] mirrored sums
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        float a = rs[p], b = rst[p];
        a += __shfl_xor(a, 1); b += __shfl_xor(b, 8);
        a += __shfl_xor(a, 2); b += __shfl_xor(b, 16);
        a += __shfl_xor(a, 4); b += __shfl_xor(b, 32);
        if ((pt & 7) == 0) red[lr + 32 * p] = a;
        if (jq == 0) red[128 + 4 * ig + p] = b;
      }
    } else if (cb == 0 && !half) {   // rowsum: the 8 threads of a row are 8 consecutive lanes
#pragma unroll
      for (int p = 0; p < PR; ++p) {
        float sum = rs[p];
        sum += __shfl_xor(sum, 1);
        sum += __shfl_xor(sum, 2);
        sum += __shfl_xor(sum, 4);
        const int row = i0 + lr + 32 * p;
        if ((pt & 7) == 0 && row < n_local) RS[(size_t)z * n_local + row] = sum * sc[4 * dc + 2];
      }
    }
    __syncthreads();   // the matrix waves have written the output image (and, up: the row sums have met)
    if (up) {
      const float* red = reinterpret_cast<const float*>(smem + 2 * FS_STAGE);
      const int row = i0 + pt;
      if (cb == 0 && !half && pt < 128 && row < n_local) RS[(size_t)z * n_local + row] = (red[pt] + red[128 + pt]) * sc[4 * dc + 2];
    }
    image_store(0);
    if (IMG_PASSES == 2) {   // the second half's image: the same two barriers as the matrix waves
      __syncthreads();
      __syncthreads();
      image_store(1);
    }
  } else {
    // ================================ CONSUMER ================================
    // v_mfma_f32_16x16x32_bf16: one MFMA spans the whole 32-deep k tile.  The chip holds a higher clock on this shape
    // than on 32x32x16 at the same cycles per flop (MI355X_MICROARCH.md, DVFS give-back item 7).
    const int ct = t - 256, lane = ct & 63, cw = ct >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    // this wave's 128-column block of [G | theta] and its CJ 16-column blocks inside it
    // (FOLD: block g of matrix `half`; a block past the matrix's last is computed as that last one and not stored)
    const int g = 2 * cb + (cw >> 2);
    const int gl = FOLD ? min(g, cblocks - 1) : g;
    const int wcol = (cw & 3) * 32;   // first column inside the block (16 CJ columns)
    // B fragment of (k tile kt, plane s, 16-column block jb): vb + ((kt * 3 + s) * 4096 + jb * 512) elements
    // (wave-uniform part, made provably so for the "s" operand of the streamed loads; per-lane byte offsets boff below)
    const u16* vb_wave = (FOLD ? (half ? Tt3 : Gt3) + (size_t)gl * ntj * 3 * XTILE_E
                               : (g < cblocks ? Gt3 + (size_t)g * ntj * 3 * XTILE_E
                                              : Tt3 + (size_t)(g - cblocks) * ntj * 3 * XTILE_E)) +
                         (size_t)(jbeg >> 5) * 3 * XTILE_E + wcol * 32;
    const u16* __restrict__ vb = reinterpret_cast<const u16*>(
        ((unsigned long long)(u32)__builtin_amdgcn_readfirstlane((int)((unsigned long long)vb_wave >> 32)) << 32) |
        (unsigned long long)(u32)__builtin_amdgcn_readfirstlane((int)(unsigned long long)vb_wave));
    u32 boff[CJ][3];
#pragma unroll
    for (int j = 0; j < CJ; ++j)   // j = 16-column block
#pragma unroll
      for (int s = 0; s < 3; ++s) boff[j][s] = (u32)(lane * 8 + s * XTILE_E + j * 512) * 2u;
    const int aoff = l15 * XROW + pswz(l15, lq);   // A fragment of 16-row block ib, plane s: + ib * 1024 + s * PLN
    f32x4 acc[FS_IB][CJ];
#pragma unroll
    for (int i = 0; i < FS_IB; ++i)
#pragma unroll
      for (int j = 0; j < CJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // two B register sets: the fragments of tile it+1 are requested at the top of tile it.  Held as 32-bit vectors
    // (loop-carried bf16 vectors get scalarised into 16-bit pieces by the compiler) and bit-cast at the MFMA.
    u32x4 bX[CJ][3], bY[CJ][3];
    auto load_b = [&](int tile, u32x4 (&b)[CJ][3]) {
      const u16* __restrict__ src = vb + (size_t)tile * 3 * XTILE_E;
#pragma unroll
      for (int j = 0; j < CJ; ++j)
#pragma unroll
        for (int s = 0; s < NP; ++s) stream_load16(b[j][s], src, boff[j][s]);
    };
    // before the MFMAs of a tile: its CJ NP fragment loads must have landed; `younger`: the next tile's CJ NP loads have
    // been requested already and stay in flight
    auto wait_b = [&](bool younger, u32x4 (&b)[CJ][3]) {
      (void)b;
      stream_wait<CJ * NP>();
      if (!younger) stream_wait<0>();
    };
    // A fragments are read one 16-row block ahead of their MFMAs; the scheduling fences keep the compiler from hoisting
    // all 24 reads (96 registers) to the top of the tile
    auto read_a = [&](const unsigned char* As, int i, u32x4 (&a)[3]) {
#pragma unroll
      for (int s = 0; s < NP; ++s) a[s] = *reinterpret_cast<const u32x4*>(As + aoff + i * 16 * XROW + s * PLN);
    };
    auto mma_tile = [&](const unsigned char* As, const u32x4 (&b)[CJ][3]) {
      u32x4 a[2][3];
      read_a(As, 0, a[0]);
#pragma unroll
      for (int i = 0; i < FS_IB; ++i) {
        if (i + 1 < FS_IB) read_a(As, i + 1, a[(i + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < CJ; ++j) acc[i][j] = x3_products16<NP>(a[i & 1], b[j], acc[i][j]);
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    if (ntile > 0) load_b(tile_at(0, 0), bX);
    __syncthreads();
    for (int st = 0; st < nstage; ++st) {
      const unsigned char* As = smem + (st & 1) * FS_STAGE;
      auto after = [&](int u) { return tile_at(st, u); };   // the tile in slot u of this stage (u >= FS_KT: of the next stage)
      constexpr bool kLoadV = true;
#pragma unroll
      for (int u = 0; u < FS_KT; u += 2) {
        if (after(u) >= ntile) break;
        const bool n1 = after(u + 1) < ntile;
        if (kLoadV && n1) load_b(after(u + 1), bY);
        wait_b(kLoadV && n1, bX);
        // The two matrix waves of a SIMD (cw and cw + 4) take turns at the higher issue priority, tile by tile.  At equal
        // priority the older wave wins every arbitration: it ran ahead (1460 vs 2070 cycles per k tile, per-wave stamps)
        // and idled at the stage barrier while the younger one finished alone.  Measured -2 % on the launch.
        if (cw >> 2) __builtin_amdgcn_s_setprio(0); else __builtin_amdgcn_s_setprio(2);
        mma_tile(As + u * FS_KTB, bX);
        if (n1) {
          const bool n2 = after(u + 2) < ntile;
          if (kLoadV && n2) load_b(after(u + 2), bX);
          wait_b(kLoadV && n2, bY);
          if (cw >> 2) __builtin_amdgcn_s_setprio(2); else __builtin_amdgcn_s_setprio(0);
          mma_tile(As + (u + 1) * FS_KTB, bY);
        }
      }
      __syncthreads();
    }
    // the scaled accumulators -> the output image (the tail's comment in front of the role split); a block past the
    // matrix's last (FOLD, odd block count) writes nothing, nor does a column past d: nobody stores those units
    const bool first = FOLD ? half == 0 : g < cblocks;   // this wave's matrix: G (FOLD: W) or theta
    const int cbase = (FOLD || first ? g : g - cblocks) * BN + wcol + l15;
    const float* __restrict__ osc = sc + (first ? 2 : 3) * dc;   // out-scales of this wave's matrix
    // unit (c, rg = 4 i + lq): lq = rg & 3, and the XOR stays inside the low two bits of c, so i and j are immediates
    unsigned char* const img = smem + lq * IMG_PITCH + ((((NP == 2 ? (cw >> 2) * BN : 0) + wcol + l15) ^ lq) * 16);
    auto image_write = [&]() {
      if (FOLD ? g >= cblocks : g >= 2 * cblocks) return;
#pragma unroll
      for (int j = 0; j < CJ; ++j) {
        const int col = cbase + j * 16;
        if (col >= d) continue;
        const float os = osc[col];
#pragma unroll
        for (int i = 0; i < FS_IB; ++i) {
          f32x4 v;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = acc[i][j][e] * os;
          *reinterpret_cast<f32x4*>(img + i * 4 * IMG_PITCH + j * 16 * 16) = v;
        }
      }
    };
    if (NP == 2 || (cw >> 2) == 0) image_write();
    __syncthreads();   // (the producers' row-sum exchange rides on this barrier: same count in both roles)
    image_store(0);
    if (IMG_PASSES == 2) {
      __syncthreads();   // everybody has stored the first half's image
      if ((cw >> 2) == 1) image_write();
      __syncthreads();
      image_store(1);
    }
  }
}

// ================================================================================================
// host side
// ================================================================================================
// split KIND of a call: bf16 inputs -> 1 (the values themselves); fp32 inputs -> 2 (two fp16 terms of the scaled value)
static int split_kind(int dtype) { return dtype == STEIN_BF16 ? 1 : 2; }
int stein_x3_kind(int dtype) { return split_kind(dtype); }

template <typename TIN, int KIND>
static void launch_split(hipStream_t stream, const TIN* theta, const TIN* score, int64_t n, int64_t d,
                         const SteinLayout& L, u16* T3, u16* Tt3, u16* Gt3, const float* sc, const PrologueArgs* pro = nullptr) {
  // grid.z walks [theta, score]; a NULL matrix is left out (its planes keep their contents)
  const unsigned nz = (theta ? 1u : 0u) + (score ? 1u : 0u);
  const int zbase = theta ? 0 : 1;
  // 16-byte loads of the inputs (load_row4): fp32 rows that start on 16-byte boundaries
  const int vec = std::is_same<TIN, float>::value && d % 4 == 0 && (((uintptr_t)theta | (uintptr_t)score) & 15u) == 0;
  const int64_t rows = L.x3_rows > L.x3_nk ? L.x3_rows : L.x3_nk;   // particle extent to cover (both multiples of 32)
  const int64_t cols = L.x3_dk > L.x3_dc ? L.x3_dk : L.x3_dc;      // parameter extent
  if (KIND == 1 && pro && theta) {   // + the prologue slice (fused call, bf16)
    const dim3 grid((unsigned)((cols + 63) / 64), (unsigned)((rows + 63) / 64), nz + 1u);
    hipLaunchKernelGGL((k_split<TIN, KIND, true>), grid, dim3(256), 0, stream, theta, score, (int)n, (int)d, T3,
                       (long)L.x3_rows, (int)L.x3_dk, Tt3, Gt3, (int)L.x3_dc, (long)L.x3_nk, sc, zbase, *pro, vec);
    return;
  }
  const dim3 grid((unsigned)((cols + 63) / 64), (unsigned)((rows + 63) / 64), nz);
  hipLaunchKernelGGL((k_split<TIN, KIND, false>), grid, dim3(256), 0, stream, theta, score, (int)n, (int)d, T3,
                     (long)L.x3_rows, (int)L.x3_dk, Tt3, Gt3, (int)L.x3_dc, (long)L.x3_nk, sc, zbase, PrologueArgs{}, vec);
}

// k_colmax over the matrices given (a NULL one is left out: its half of cmax keeps its values)
static void launch_colmax(const StepViews& v, const float* score_all, const float* theta_all, int64_t n, int64_t d,
                          HistSync* fuse_done, hipStream_t stream) {
  const int dc = (int)v.L.x3_dc;
  const int zbase = score_all ? 0 : 1;
  const unsigned nz = (score_all ? 1u : 0u) + (theta_all ? 1u : 0u);
  int gy = (int)((n + 63) / 64);
  if (gy > 256) gy = 256;
  const bool v4 = d % 4 == 0 && (!score_all || ((uintptr_t)score_all & 15) == 0) && (!theta_all || ((uintptr_t)theta_all & 15) == 0);
  if (v4) {
    const int gy4 = gy > 64 ? 64 : gy;
    const dim3 grid((unsigned)((d + 255) / 256), (unsigned)gy4, nz);
    hipLaunchKernelGGL((k_colmax<float, true>), grid, dim3(1024), 0, stream, score_all, theta_all, (int)n, (int)d, v.cmax, dc,
                       zbase, v.sc, PEXP_H2, fuse_done);
  } else {
    const dim3 grid((unsigned)((d + 63) / 64), (unsigned)gy, nz);
    hipLaunchKernelGGL((k_colmax<float, false>), grid, dim3(256), 0, stream, score_all, theta_all, (int)n, (int)d, v.cmax, dc,
                       zbase, v.sc, PEXP_H2, fuse_done);
  }
}

int stein_x3_split(const StepViews& v, const void* theta_all, const void* score_all, int dtype, int64_t n, int64_t d,
                   hipStream_t stream, const SplitFused* fused) {
  const SteinLayout& L = v.L;
  const int dc = (int)L.x3_dc;
  const int kind = split_kind(dtype);
  HistSync* fuse_done = fused && theta_all && score_all ? fused->done : nullptr;
  const PrologueArgs* prologue = fused ? fused->prologue : nullptr;
  const int fold = fused ? fused->fold : 0;
  // the fused call's folded step, phi alone: no maxima and no scales here -- k_split_rows takes theta's one scale from the
  // prologue's per-workgroup maxima, the column maxima come with the select launch, the column scales with k_split_w
  const u32* wgmax = fused && kind == 2 && fold == 1 ? fused->wgmax : nullptr;
  if (wgmax) {
    const int vec = d % 4 == 0 && ((uintptr_t)theta_all & 15u) == 0;   // 16-byte loads (load_row4)
    const dim3 grid((unsigned)((L.x3_dk + 63) / 64), (unsigned)((L.x3_rows + 63) / 64));
    hipLaunchKernelGGL(k_split_rows, grid, dim3(256), 0, stream, (const float*)theta_all, (int)n, (int)d, v.T3, (long)L.x3_rows,
                       (int)L.x3_dk, dc, v.sc, vec, wgmax, fused->nwg);
    LAUNCH_CHECK("k_split_rows");
    return STEIN_OK;
  }
  if (kind == 2) {   // column maxima of the matrices given (cmax = [score | theta]); the other half keeps its values
    const int zbase = score_all ? 0 : 1;
    const unsigned nz = (score_all ? 1u : 0u) + (theta_all ? 1u : 0u);
    if (!fuse_done) HIP_TRY(hipMemsetAsync(v.cmax + (size_t)zbase * dc, 0, (size_t)nz * dc * sizeof(u32), stream));
    launch_colmax(v, (const float*)score_all, (const float*)theta_all, n, d, fuse_done, stream);
    LAUNCH_CHECK("k_colmax");
  }
  if (kind == 2 ? !fuse_done : !prologue) {   // (bf16 inputs: the fused call's prologue writes the neutral scales)
    hipLaunchKernelGGL(k_make_scales, dim3(1), dim3(256), 0, stream, v.cmax, dc, v.sc, kind == 2 ? PEXP_H2 : 0,
                       kind == 2 ? 1 : 0);
    LAUNCH_CHECK("k_make_scales");
  }
  if (kind == 1) launch_split<u16, 1>(stream, (const u16*)theta_all, (const u16*)score_all, n, d, L, v.T3, v.Tt3, v.Gt3, v.sc, prologue);
  else if (fold)   // the score's planes are built behind the median (stein_x3_split_w); theta^T only if its product is asked for
    launch_split<float, 2>(stream, (const float*)theta_all, (const float*)nullptr, n, d, L, v.T3, fold == 2 ? v.Tt3 : nullptr, v.Gt3, v.sc);
  else launch_split<float, 2>(stream, (const float*)theta_all, (const float*)score_all, n, d, L, v.T3, v.Tt3, v.Gt3, v.sc);
  LAUNCH_CHECK("k_split");
  return STEIN_OK;
}

// Where the folded operand pays by default.  It halves the contraction's MFMAs only when W has at least two 128-column
// blocks: with one (d <= 128) the unfolded kernel already pairs G's block with theta's in one workgroup and the folded one
// would run half its matrix waves for nothing -- measured 2.5 % SLOWER at 8192 x 128 (one more dependent launch, nothing
// saved).  With d > 128 the fused step, fold forced on against off (ms): 4096 x 256 0.129 -> 0.119,
// 8192 x 256 0.275 -> 0.211, 8192 x 2001 1.77 -> 1.22, 16384 x 256 0.87 -> 0.61; run-to-run spread 0.5 %.  The threshold sits
// at the smallest block measured to gain (4096 x 256: n^2 d = 4.3e9); below it the step is a chain of latency-bound launches.
constexpr double FOLD_MIN_WORK = 4.0e9;   // n * n * d
bool stein_fold_pays(int64_t n, int64_t d) { return d > 128 && (double)n * (double)n * (double)d >= FOLD_MIN_WORK; }

int stein_x3_colmax(const StepViews& v, const float* theta_all, const float* score_all, int64_t n, int64_t d,
                    hipStream_t stream) {
  launch_colmax(v, score_all, theta_all, n, d, nullptr, stream);
  LAUNCH_CHECK("k_colmax");
  return STEIN_OK;
}

int stein_x3_split_w(const StepViews& v, const float* theta_all, const float* score_all, int64_t n, int64_t d,
                     const float* h2_dev, hipStream_t stream) {
  const SteinLayout& L = v.L;
  const dim3 grid((unsigned)((L.x3_dc + 63) / 64), (unsigned)((L.x3_nk + 63) / 64));
  const int vec = d % 4 == 0 && (((uintptr_t)theta_all | (uintptr_t)score_all) & 15u) == 0;   // 16-byte loads (load_row4)
  hipLaunchKernelGGL(k_split_w, grid, dim3(256), 0, stream, theta_all, score_all, (int)n, (int)d, v.Gt3, (int)L.x3_dc,
                     (long)L.x3_nk, v.sc, (const u32*)v.cmax, h2_dev, vec);
  LAUNCH_CHECK("k_split_w");
  return STEIN_OK;
}

template <bool SYM, int NP>
static void launch_distance_x3(long nblk, hipStream_t stream, const u16* T3, int ntk, const float* r, float* D, int n,
                               int row0, int n_local, long ld, int tiles_m, int tiles_n, u64* hist0, const float* two_s,
                               SpecState* spec, u64* spec_buf) {
  hipLaunchKernelGGL((k_distance_x3<SYM, NP>), dim3((unsigned)nblk), dim3(NTHREADS), 0, stream, T3, ntk, r, D, n, row0,
                     n_local, ld, tiles_m, tiles_n, hist0, two_s, spec, spec_buf);
}

int stein_x3_distance(const StepViews& v, const BlockShape& b, bool symmetric, bool window, hipStream_t stream, int panel) {
  if (panel >= 0 && stein_dpanel_ok(v, b, panel > 0)) return stein_dpanel_distance(v, b, symmetric, window, stream);
  const SteinLayout& L = v.L;
  const int ntk = (int)(L.x3_dk / 32);
  const int tiles_m = (int)((b.n_local + BM - 1) / BM), tiles_n = (int)((b.n + BN - 1) / BN);
  if (b.row0 + (int64_t)tiles_m * BM > L.x3_rows) return stein_fail(STEIN_E_SHAPE, "row block exceeds the padded planes");
  const long nblk = distance_grid(symmetric, tiles_m, tiles_n);
  if (nblk > 0x7fffffffl) return stein_fail(STEIN_E_SHAPE, "too many tiles");
  SpecState* spec = window ? v.spec : nullptr;
  u64* spec_buf = window ? v.spec_buf : nullptr;
#define X3_DIST(SYM, NP) launch_distance_x3<SYM, NP>(nblk, stream, v.T3, ntk, v.r, v.D, (int)b.n, (int)b.row0, (int)b.n_local, (long)L.ld_dist, tiles_m, tiles_n, v.hist, v.two_s, spec, spec_buf)
  switch (split_kind(b.dtype)) {
    case 1: if (symmetric) X3_DIST(true, 1); else X3_DIST(false, 1); break;
    default: if (symmetric) X3_DIST(true, 2); else X3_DIST(false, 2); break;
  }
#undef X3_DIST
  LAUNCH_CHECK("k_distance_x3");
  return STEIN_OK;
}

int stein_x3_contract_partial(const StepViews& v, const BlockShape& b, const float* h2_dev, hipStream_t stream, bool upper) {
  const SteinLayout& L = v.L;
  const long nblk = (long)L.tiles_m * L.cblocks * v.nsplit;
  if (nblk > 0x7fffffffl) return stein_fail(STEIN_E_SHAPE, "too many tiles");
#define X3_PHI(NP) hipLaunchKernelGGL((k_phi_x3fs<NP>), dim3((unsigned)nblk), dim3(FS_THREADS), 0, stream, v.D, (long)L.ld_dist, v.Gt3, v.Tt3, (long)(L.x3_nk / 32), h2_dev, v.OG, v.OT, v.RS, (int)b.n, (int)b.d, (int)b.n_local, (int)L.tiles_m, (int)L.cblocks, v.nsplit, v.jchunk, v.sc, (int)L.x3_dc, upper ? 1 : 0)
  switch (split_kind(b.dtype)) {
    case 1: X3_PHI(1); break;
    default: X3_PHI(2); break;
  }
#undef X3_PHI
  LAUNCH_CHECK("k_phi_x3fs");
  return STEIN_OK;
}

// the folded contraction of the fused call: K.W in v.nsplit j ranges (with_theta: and K.theta in one) into the fold's
// partial sums (v.OG / v.OT / v.RS of a folding layout)
int stein_x3_contract_fold(const StepViews& v, const float* h2_dev, int64_t n, int64_t d, bool with_theta,
                           hipStream_t stream) {
  const SteinLayout& L = v.L;
  const long per_range = (long)L.tiles_m * ((L.cblocks + 1) / 2);
  const long nblk = per_range * (v.nsplit + (with_theta ? 1 : 0));
  if (nblk > 0x7fffffffl) return stein_fail(STEIN_E_SHAPE, "too many tiles");
  hipLaunchKernelGGL((k_phi_x3fs<2, true>), dim3((unsigned)nblk), dim3(FS_THREADS), 0, stream, v.D, (long)L.ld_dist, v.Gt3,
                     with_theta ? v.Tt3 : (const u16*)nullptr, (long)(L.x3_nk / 32), h2_dev, v.OG, v.OT, v.RS, (int)n, (int)d,
                     (int)n, (int)L.tiles_m, (int)L.cblocks, v.nsplit, v.jchunk, v.sc, (int)L.x3_dc, 1);
  LAUNCH_CHECK("k_phi_x3fs");
  return STEIN_OK;
}
