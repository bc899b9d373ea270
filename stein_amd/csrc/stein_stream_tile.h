// stein_stream_tile.h -- the device code the streaming kernels of stein_stream.hip (k_phi_stream, k_stream_hist) and of
// stein_imq.hip (k_phi_imq) share: the geometry of one 128 x 128 distance tile with its P image in LDS, the phases of one
// tile (distance, fp16 split into the image, contraction), the tail of a workgroup (partial O, row sums), the frame of the
// finish pass and the kernel that adds its block partials.  One body each: every kernel forms every S value and every sum
// in the same order, so the streaming median is the median of the very D values both steps consume, and a fix to a phase
// reaches both steps.  What differs stays in the kernels: buffering and barriers, the element function, which wave
// contracts which operand.
#pragma once
#include "stein_x3_dev.h"

constexpr int ST_THREADS = 512;
constexpr int ST_ROWS = 128;              // particles per row tile
constexpr int ST_JT = 128;                // columns of D per step (4 k tiles of the contraction)
constexpr int ST_PLN = ST_ROWS * XROW;    // one plane of one 32-deep k tile of P in LDS: 8 KB
constexpr int ST_KTB = 2 * ST_PLN;        // hi and lo plane
constexpr int ST_BUF = (ST_JT / 32) * ST_KTB;   // one P image: 64 KB; two of them

// What one thread of the 512 does.  Distance role: wave (wr, wc) owns rows [32 wr, 32 wr + 32) x columns
// [64 wc, 64 wc + 64) of the 128 x 128 tile.  Contraction role: all 128 rows x the 32 columns at wcol of a 128-column block.
struct StRoles {
  int t, lane, w, l15, lq, wr, wc, wcol;
};
__device__ __forceinline__ StRoles st_roles() {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  return StRoles{t, lane, w, lane & 15, lane >> 4, w >> 1, w & 1, (w & 3) * 32};
}

// The distance phase of one 128 x 128 tile.  Wave (wr, wc) of eight: s[jb][ib] = the 16 x 16 block
// S^T[j = 64 wc + 16 jb ..][i = 32 wr + 16 ib ..] over all ntk k tiles; ta / tb: this lane's 16 bytes of the first fragment
// of the row tile's rows 32 wr.. and of the column tile's rows 64 wc..
__device__ __forceinline__ void st_distance_tile(const u16* __restrict__ ta, const u16* __restrict__ tb, int ntk,
                                                 f32x4 (&s)[4][2]) {
#pragma unroll
  for (int jb = 0; jb < 4; ++jb)
#pragma unroll
    for (int ib = 0; ib < 2; ++ib) s[jb][ib] = f32x4{0.f, 0.f, 0.f, 0.f};
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

// Where the four consecutive columns jc .. jc + 3 (jc % 4 == 0) of row `row` lie in the hi plane of a P image: the stored-D
// contraction's layout [k tile][plane][128 rows][64 B] with its swizzle
__device__ __forceinline__ unsigned char* st_image_dst(unsigned char* buf, int row, int jc) {
  return buf + (jc >> 5) * ST_KTB + row * XROW + pswz(row, (jc & 31) >> 3) + (jc & 4) * 2;
}

// q[0..3] -> hi = fp16(q), lo = fp16(q - hi), packed for one 8-byte LDS store per plane.  Two steps, so that each kernel
// keeps the order its inline code had (k_phi_stream splits and then forms the address, k_phi_imq forms the one address
// of its two images first): the compiler's schedule of the stage, and k_phi_imq's register count, follow that order.
struct StSplit4 {
  uint2 hi, lo;
};
__device__ __forceinline__ StSplit4 st_split4(const float (&q)[4]) {
  const u32 h0 = cvt_pk_f16(q[0], q[1]), h1 = cvt_pk_f16(q[2], q[3]);
  const u32 o0 = cvt_pk_f16(f16_resid_lo(h0, q[0]), f16_resid_hi(h0, q[1]));
  const u32 o1 = cvt_pk_f16(f16_resid_lo(h1, q[2]), f16_resid_hi(h1, q[3]));
  return StSplit4{make_uint2(h0, h1), make_uint2(o0, o1)};
}
__device__ __forceinline__ void st_stage4(unsigned char* dst, const StSplit4& p) {
  *reinterpret_cast<uint2*>(dst) = p.hi;
  *reinterpret_cast<uint2*>(dst + ST_PLN) = p.lo;
}

// One 32-deep k tile of the contraction phase: acc += A . B with A this wave's 128 rows of the P image (As: the k tile's
// hi plane at this lane's offset into a row block; fragments by ds_read_b128) and B the operand's 32 columns (src: this
// lane's 16 bytes of the k tile's first fragment; coalesced 1 KB loads), three products each.  The loop over a j tile's
// four k tiles stays in the kernels: inside a helper it compiled k_phi_stream{,_ksd} to another entry test per j tile, and
// the step measured 0.2 - 0.5 % slower at 16384 x 256 (profiles/stream_imq_shared_ab.txt).
__device__ __forceinline__ void st_contract_ktile(f32x4 (&acc)[8][2], const unsigned char* As, const u16* src) {
  u32x4 b[2][3];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int p = 0; p < 2; ++p) b[j][p] = *reinterpret_cast<const u32x4*>(src + p * XTILE_E + j * 512);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    u32x4 a[3];
#pragma unroll
    for (int p = 0; p < 2; ++p) a[p] = *reinterpret_cast<const u32x4*>(As + i * 16 * XROW + p * ST_PLN);
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = x3_products16<2>(a, b[j], acc[i][j]);
  }
}

// This wave's partial O of one j range: rows i0.. x the 32 columns at col0, out-scaled by the operand's column scales osc
__device__ __forceinline__ void st_store_partial(float* Oz, const float* osc,
                                                 const f32x4 (&acc)[8][2], int col0, int i0, int lq, int l15, int n, int d) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = col0 + j * 16 + l15;
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

// The row sums of one j range z: the four lane groups lq of a wave, then the two waves wc = 0, 1 (through LDS, in that
// order), times *scale, into RS[z][n] (KSD: rd the same way into RD).  Every wave of the workgroup calls it.
template <bool KSD>
__device__ __forceinline__ void st_reduce_rows(unsigned char* smem, const float (&rs)[2], const float (&rd)[2],
                                               float* RS, float* RD, int z, int i0, int n, const float* scale,
                                               const StRoles& ro) {
  __syncthreads();   // every wave is past its last read of the P images
  float* red = reinterpret_cast<float*>(smem);   // [2][128] (KSD: rd's [2][128] behind it)
#pragma unroll
  for (int ib = 0; ib < 2; ++ib) {
    float a = rs[ib];
    a += __shfl_xor(a, 16);
    a += __shfl_xor(a, 32);
    if (ro.lq == 0) red[ro.wc * ST_ROWS + ro.wr * 32 + ib * 16 + ro.l15] = a;
    if constexpr (KSD) {
      float b = rd[ib];
      b += __shfl_xor(b, 16);
      b += __shfl_xor(b, 32);
      if (ro.lq == 0) red[(2 + ro.wc) * ST_ROWS + ro.wr * 32 + ib * 16 + ro.l15] = b;
    }
  }
  __syncthreads();
  const int t = ro.t, row = i0 + t;
  if (t < ST_ROWS && row < n) RS[(size_t)z * n + row] = (red[t] + red[ST_ROWS + t]) * *scale;
  if constexpr (KSD)
    if (t < ST_ROWS && row < n) RD[(size_t)z * n + row] = (red[2 * ST_ROWS + t] + red[3 * ST_ROWS + t]) * *scale;
}

// ---- the finish pass ---------------------------------------------------------------------------------------------------
// The frame of k_stream_finish{,_ksd} and k_imq_finish{,_ksd}: o_k = sum_z O_k (k < Kern::NO operands) and rs = sum_z RS in
// range order, phi = kern.phi(o, theta, rs), and this workgroup's fp64 partial of |phi|^2 into sqpart[block].
// vec bit 0: d % 4 == 0 and the O_k, T and phi 16-byte aligned (four elements per thread); bit 1 (KSD): so is G.
// KSD: also this workgroup's partials of the Stein discrepancy sums S and S_diag (include/steinhip.h) into kpart[0][blocks]
// and kpart[1][blocks], in fp64 from the fp32 sums and the score rows G: kern.ksd_terms per element, and kern.row_term
// (with rd = sum_z RD, range order) once per row, by the thread that holds its column 0.  phi may then be NULL: only the
// store is skipped.
// Kern: NO; a constructor from (h2p, n, d); float phi(o[NO], th, rs); void ksd_terms(g, o[NO], th, rs, s, sd);
// double row_term(rs, rd).
template <class Kern, bool KSD>
__device__ __forceinline__ void st_finish_body(const float* __restrict__ O1, const float* __restrict__ O2,
                                               const float* __restrict__ RS, const float* __restrict__ RD,
                                               const float* __restrict__ T, const float* __restrict__ G,
                                               const float* __restrict__ h2p, float* __restrict__ phi,
                                               double* __restrict__ sqpart, double* __restrict__ kpart, int n, int d,
                                               int jsplit, int vec) {
  constexpr int NO = Kern::NO;
  __shared__ double red[KSD ? 12 : 4];
  const Kern kern(h2p, n, d);
  const float* const O[2] = {O1, O2};
  const long total = (long)n * d;
  const size_t zs = (size_t)n * d;
  double sq = 0.0, ks = 0.0, kd = 0.0;
  auto row_term = [&](int i, float rs) {
    float rd = 0.f;
    for (int z = 0; z < jsplit; ++z) rd += RD[(size_t)z * n + i];
    return kern.row_term(rs, rd);
  };
  if (vec & 1) {
    const long total4 = total >> 2;
    const int d4 = d >> 2;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < total4; q += (long)gridDim.x * 256) {
      const int i = (int)(q / d4);
      const long e = q << 2;
      float o[4][NO] = {};
      float rs = 0.f;
      for (int z = 0; z < jsplit; ++z) {
#pragma unroll
        for (int k = 0; k < NO; ++k) {
          const float4 a = *reinterpret_cast<const float4*>(O[k] + z * zs + e);
          o[0][k] += a.x; o[1][k] += a.y; o[2][k] += a.z; o[3][k] += a.w;
        }
        rs += RS[(size_t)z * n + i];
      }
      const float4 th4 = *reinterpret_cast<const float4*>(T + e);
      const float th[4] = {th4.x, th4.y, th4.z, th4.w};
      float ph[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) ph[c] = kern.phi(o[c], th[c], rs);
      if (!KSD || phi) *reinterpret_cast<float4*>(phi + e) = make_float4(ph[0], ph[1], ph[2], ph[3]);
      sq += ((double)ph[0] * (double)ph[0] + (double)ph[1] * (double)ph[1]) + ((double)ph[2] * (double)ph[2] + (double)ph[3] * (double)ph[3]);
      if constexpr (KSD) {
        const float4 g4 = (vec & 2) ? *reinterpret_cast<const float4*>(G + e) : make_float4(G[e], G[e + 1], G[e + 2], G[e + 3]);
        const float g[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) kern.ksd_terms(g[c], o[c], th[c], rs, ks, kd);
        if (q == (long)i * d4) ks += row_term(i, rs);   // the row's first four columns
      }
    }
  } else {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
      const int i = (int)(e / d);
      float o[NO] = {};
      float rs = 0.f;
      for (int z = 0; z < jsplit; ++z) {
#pragma unroll
        for (int k = 0; k < NO; ++k) o[k] += O[k][z * zs + e];
        rs += RS[(size_t)z * n + i];
      }
      const float th = T[e];
      const float ph = kern.phi(o, th, rs);
      if (!KSD || phi) phi[e] = ph;
      sq += (double)ph * (double)ph;
      if constexpr (KSD) {
        kern.ksd_terms(G[e], o, th, rs, ks, kd);
        if (e == (long)i * d) ks += row_term(i, rs);   // the row's column 0
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

// The block partials of a finish pass in a fixed order, one workgroup per set: sqpart[count] -> out[0] (the plain steps:
// a grid of one, kpart NULL); the KSD steps' grid of three: kpart[2][count] -> out[1], out[2].  (static: each file that
// launches it holds its own copy.)
static __global__ __launch_bounds__(256) void k_stream_sum(const double* __restrict__ sqpart, const double* __restrict__ kpart,
                                                           int count, double* __restrict__ out) {
  __shared__ double red[4];
  const double* __restrict__ part = blockIdx.x == 0 ? sqpart : kpart + (size_t)(blockIdx.x - 1) * count;
  double s[1] = {0.0};
  for (int i = threadIdx.x; i < count; i += 256) s[0] += part[i];
  block_sum256(s, red);
  if (threadIdx.x == 0) out[blockIdx.x] = s[0];
}
