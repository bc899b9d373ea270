// stein_imq.hip -- the streaming SVGD direction and Stein discrepancy under the inverse multiquadric (IMQ) kernel
//   k_ij = (1 + D_ij / c2)^(-1/2),   c2 = 2 h2,   D_ij = max(|theta_i - theta_j|^2, 0)
// at a bandwidth the caller supplies, without the n x n distance image (include/steinhip.h, stein_svgd_phi_imq).
//
// The kernel's gradient is not proportional to the kernel: grad_{theta_j} k(theta_j, theta_i) = k3_ij (theta_i - theta_j) / c2
// with k3 = k^3, so the fold W = G - theta / h2 of the RBF paths does not apply and the step contracts two images with two
// operands:
//   n phi_i = (K G)_i + [ rs3_i theta_i - (K3 theta)_i ] / c2,        rs3_i = sum_j k3_ij
// and for the statistic (Stein kernel u_p, k5 = k^5, rd5_i = sum_j k5_ij D_ij):
//   S      = sum_e g_e (K G)_e + (2 / c2) sum_e g_e [ rs3_i theta_e - (K3 theta)_e ] + sum_i [ d rs3_i / c2 - 3 rd5_i / c2^2 ]
//   S_diag = sum_e g_e^2 + n d / c2
// (e runs over the elements (i, column)).
//
//   stein_rownorms, k_colmax, k_make_scales, k_split (unfolded: theta's row-major planes, theta^T's and G^T's)   as they are
//   k_phi_imq           distance tile -> k, k3 (both x 2^14, hi + lo fp16) -> O1 += K.G, O2 += K3.theta, running rs3
//   k_imq_finish        sums the j ranges in order, phi, |phi|^2 block partials (fp64)
//   k_imq_sum           the block partials in a fixed order -> the caller's doubles
// stein_svgd_phi_imq_ksd launches the KSD forms of the same bodies (k_phi_imq_ksd: a second running row sum rd5;
// k_imq_finish_ksd: reads the score rows, three sets of block partials).
//
// k_phi_imq: a 512-thread workgroup (8 waves) owns 128 rows of particles x ONE 128-column block of phi x one range of
// 128-column j tiles.  Per j tile:
//   distance     st_distance_tile (stein_stream_tile.h), the streaming step's and the streaming median's: registers only
//   barrier      every wave has read the previous tile's images
//   kernel/split D = max((r_i + r_j) - two_s S, 0), u = 1 + D / c2, k = rsq(u), k3 = k k k, columns j >= n forced to 0; both
//                times 2^PEXP_H2, split into hi + lo fp16 and stored as TWO P images in the stored-D contraction's swizzled LDS
//                layout (2 x 64 KB: single-buffered, 32 KB of the CU's LDS stay free); rs3 += k3 (KSD: rd5 += k5 D)
//   barrier
//   contraction  waves 0-3: the k image with G^T's planes of the block, waves 4-7: the k3 image with theta^T's planes of
//                the same block; wave w owns all 128 rows x the 32 columns (w & 3): A fragments by ds_read_b128, B
//                fragments by coalesced 1 KB loads, three products each
// Every load is plain C++; no workgroup waits for another; every loop bound is an argument.  The partial sums of the j ranges
// go to [jsplit][n][d] / [jsplit][n] and are added in range order by the finish pass: no float atomics, a repeated call is
// bit-identical.  Resources (hipcc, gfx950): DESIGN.md section 6f.

#include "stein_x3.h"

#include "stein_x3_dev.h"
#include "stein_stream_tile.h"

template <bool KSD>
__device__ __forceinline__ void phi_imq_body(unsigned char* smem, const u16* __restrict__ T3, int ntk,
                                             const u16* __restrict__ Gt3, const u16* __restrict__ Tt3, long ntj,
                                             const float* __restrict__ r, const float* __restrict__ sc, int dc,
                                             const float* __restrict__ h2p, float* __restrict__ O1, float* __restrict__ O2,
                                             float* __restrict__ RS3, float* __restrict__ RD5, int n, int d, int row_tiles,
                                             int cblocks, int jtiles, int jtiles_per) {
  // column block fastest: the workgroups of one row tile are neighbours (same XCD, same T panels in its L2)
  const int logical = xcd_remap(blockIdx.x, gridDim.x);
  const int cb = logical % cblocks;
  const int tile_m = (logical / cblocks) % row_tiles;
  const int z = logical / (cblocks * row_tiles);
  const int i0 = tile_m * ST_ROWS;
  const int jt0 = z * jtiles_per, jt1 = min(jtiles, jt0 + jtiles_per);

  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  // distance role: rows [32 wr, 32 wr + 32) x columns [64 wc, 64 wc + 64) of the 128 x 128 tile
  const int wr = w >> 1, wc = w & 1;
  // contraction role: all 128 rows x 32 columns at wcol of block cb; waves 0-3 K.G, waves 4-7 K3.theta (wave-uniform)
  const bool third = w >= 4;
  const int wcol = (w & 3) * 32;

  const float ic2 = 1.f / (2.f * *h2p);   // 1 / c2
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
  const u16* __restrict__ vb = (third ? Tt3 : Gt3) + (size_t)cb * ntj * 3 * XTILE_E + wcol * 32 + lane * 8;
  const unsigned char* img = smem + (third ? ST_BUF : 0);   // this wave's A operand: the k or the k3 image
  const int aoff = l15 * XROW + pswz(l15, lq);
  const float pscale = (float)(1 << PEXP_H2);

  for (int jt = jt0; jt < jt1; ++jt) {
    const int j0 = jt * ST_JT;
    // ---- distance: S^T block [4 j blocks][2 i blocks] of this wave
    f32x4 s[4][2];
    const u16* __restrict__ tb = T3 + (size_t)jt * ntk * 3 * XTILE_E + (wc * 4) * 512 + lane * 8;
    st_distance_tile(ta, tb, ntk, s);
    __syncthreads();   // every wave is past its reads of the previous tile's images
    // ---- kernel, split, stage: lane holds S^T[j = 16 jb + 4 lq + e][i = 16 ib + l15]
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) {
      const int jc = wc * 64 + jb * 16 + 4 * lq;          // first of this lane's 4 columns inside the tile
      const float4 rj4 = *reinterpret_cast<const float4*>(r + j0 + jc);   // (padded; columns >= n are masked below)
      const float rj[4] = {rj4.x, rj4.y, rj4.z, rj4.w};
#pragma unroll
      for (int ib = 0; ib < 2; ++ib) {
        float q[4], q3[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool inb = j0 + jc + e < n;
          const float dv = __builtin_fmaxf((ri[ib] + rj[e]) - two_s * s[jb][ib][e], 0.f);
          const float u = __builtin_fmaf(dv, ic2, 1.f);
          const float k = __builtin_amdgcn_rsqf(u);
          const float k2 = k * k;
          // (masked by a select: r's padding, and with it dv, may hold anything there, NaN included)
          q[e] = inb ? k * pscale : 0.f;
          q3[e] = inb ? (k2 * k) * pscale : 0.f;
          if constexpr (KSD) rd[ib] = __builtin_fmaf(inb ? q3[e] * k2 : 0.f, inb ? dv : 0.f, rd[ib]);
        }
        rs[ib] += (q3[0] + q3[1]) + (q3[2] + q3[3]);
        const int row = wr * 32 + ib * 16 + l15;
        unsigned char* dst = smem + (jc >> 5) * ST_KTB + row * XROW + pswz(row, (jc & 31) >> 3) + (jc & 4) * 2;
        {
          const u32 h0 = cvt_pk_f16(q[0], q[1]), h1 = cvt_pk_f16(q[2], q[3]);
          const u32 o0 = cvt_pk_f16(f16_resid_lo(h0, q[0]), f16_resid_hi(h0, q[1]));
          const u32 o1 = cvt_pk_f16(f16_resid_lo(h1, q[2]), f16_resid_hi(h1, q[3]));
          *reinterpret_cast<uint2*>(dst) = make_uint2(h0, h1);
          *reinterpret_cast<uint2*>(dst + ST_PLN) = make_uint2(o0, o1);
        }
        {
          const u32 h0 = cvt_pk_f16(q3[0], q3[1]), h1 = cvt_pk_f16(q3[2], q3[3]);
          const u32 o0 = cvt_pk_f16(f16_resid_lo(h0, q3[0]), f16_resid_hi(h0, q3[1]));
          const u32 o1 = cvt_pk_f16(f16_resid_lo(h1, q3[2]), f16_resid_hi(h1, q3[3]));
          *reinterpret_cast<uint2*>(dst + ST_BUF) = make_uint2(h0, h1);
          *reinterpret_cast<uint2*>(dst + ST_BUF + ST_PLN) = make_uint2(o0, o1);
        }
      }
    }
    __syncthreads();
    // ---- contraction: O += image . V_j over the tile's (up to) four 32-deep k tiles
    for (int kt = 0; kt < ST_JT / 32; ++kt) {
      if (j0 + kt * 32 >= n) break;   // both images are zero there
      u32x4 b[2][3];
      const u16* __restrict__ src = vb + ((size_t)jt * (ST_JT / 32) + kt) * 3 * XTILE_E;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int p = 0; p < 2; ++p) b[j][p] = *reinterpret_cast<const u32x4*>(src + p * XTILE_E + j * 512);
      const unsigned char* As = img + kt * ST_KTB + aoff;
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

  // ---- partial O1 / O2 of this j range (out-scaled by the operand's column scale)
  {
    float* __restrict__ Oz = (third ? O2 : O1) + (size_t)z * n * d;
    const float* __restrict__ osc = sc + (third ? 3 : 2) * dc;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = cb * 128 + wcol + j * 16 + l15;
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
  if (cb == 0) {
    // a row's sum: the four lane groups lq of a wave, then the two waves wc = 0, 1 (through LDS, in that order)
    __syncthreads();   // every wave is past its last read of the images
    float* red = reinterpret_cast<float*>(smem);   // [2][128] (KSD: rd5's [2][128] behind it)
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
    if (t < ST_ROWS && row < n) RS3[(size_t)z * n + row] = (red[t] + red[ST_ROWS + t]) * sc[4 * dc + 2];
    if constexpr (KSD)
      if (t < ST_ROWS && row < n) RD5[(size_t)z * n + row] = (red[2 * ST_ROWS + t] + red[3 * ST_ROWS + t]) * sc[4 * dc + 2];
  }
}

__global__ __launch_bounds__(ST_THREADS) void k_phi_imq(const u16* __restrict__ T3, int ntk, const u16* __restrict__ Gt3,
                                                        const u16* __restrict__ Tt3, long ntj, const float* __restrict__ r,
                                                        const float* __restrict__ sc, int dc, const float* __restrict__ h2p,
                                                        float* __restrict__ O1, float* __restrict__ O2,
                                                        float* __restrict__ RS3, int n, int d, int row_tiles, int cblocks,
                                                        int jtiles, int jtiles_per) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * ST_BUF];
  phi_imq_body<false>(smem, T3, ntk, Gt3, Tt3, ntj, r, sc, dc, h2p, O1, O2, RS3, nullptr, n, d, row_tiles, cblocks, jtiles,
                      jtiles_per);
}

// k_phi_imq that also leaves RD5[jsplit][n], the partial sums of rd5 (same registers live, no scratch: __graft_entry__.py)
__global__ __launch_bounds__(ST_THREADS) void k_phi_imq_ksd(const u16* __restrict__ T3, int ntk, const u16* __restrict__ Gt3,
                                                            const u16* __restrict__ Tt3, long ntj,
                                                            const float* __restrict__ r, const float* __restrict__ sc,
                                                            int dc, const float* __restrict__ h2p, float* __restrict__ O1,
                                                            float* __restrict__ O2, float* __restrict__ RS3,
                                                            float* __restrict__ RD5, int n, int d, int row_tiles,
                                                            int cblocks, int jtiles, int jtiles_per) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * ST_BUF];
  phi_imq_body<true>(smem, T3, ntk, Gt3, Tt3, ntj, r, sc, dc, h2p, O1, O2, RS3, RD5, n, d, row_tiles, cblocks, jtiles,
                     jtiles_per);
}

// phi = (sum_z O1_z + ((sum_z RS3_z) theta - sum_z O2_z) / c2) / n and this workgroup's fp64 partial of |phi|^2.
// vec (bit 0): d % 4 == 0 and O1, O2, T and phi 16-byte aligned; KSD, bit 1: so is G.
// KSD (k_imq_finish_ksd): also this workgroup's partials of S and S_diag (the file's header) into kpart[0][blocks] and
// kpart[1][blocks], in fp64 from the fp32 o1 = sum_z O1_z, o2, rs3 and rd5 (range order) and the score rows G; the row's
// own terms are added once per row, by the thread that holds its column 0.  phi may then be NULL: only the store is skipped.
__device__ __forceinline__ float imq_phi(float o1, float o2, float th, float rs3, float c2, float fn) {
  return (o1 + __builtin_fmaf(rs3, th, -o2) / c2) / fn;
}
__device__ __forceinline__ void imq_ksd_terms(float g, float o1, float o2, float th, float rs3, double ic2, double& s,
                                              double& sd) {
  const double gd = g;
  s += gd * ((double)o1 + 2.0 * ic2 * ((double)rs3 * (double)th - (double)o2));
  sd += gd * gd + ic2;
}

template <bool KSD>
__device__ __forceinline__ void imq_finish_body(const float* __restrict__ O1, const float* __restrict__ O2,
                                                const float* __restrict__ RS3, const float* __restrict__ RD5,
                                                const float* __restrict__ T, const float* __restrict__ G,
                                                const float* __restrict__ h2p, float* __restrict__ phi,
                                                double* __restrict__ sqpart, double* __restrict__ kpart, int n, int d,
                                                int jsplit, int vec) {
  __shared__ double red[KSD ? 12 : 4];
  const float c2 = 2.f * *h2p;
  const float fn = (float)n;
  const long total = (long)n * d;
  const size_t zs = (size_t)n * d;
  const double ic2 = 1.0 / (2.0 * (double)*h2p);   // (KSD)
  double sq = 0.0, ks = 0.0, kd = 0.0;
  // the row's own terms of S: d rs3 / c2 - 3 rd5 / c2^2
  auto row_terms = [&](int i, float rs3) {
    float rd5 = 0.f;
    for (int z = 0; z < jsplit; ++z) rd5 += RD5[(size_t)z * n + i];
    return ic2 * ((double)d * (double)rs3 - 3.0 * ic2 * (double)rd5);
  };
  if (vec & 1) {
    const long total4 = total >> 2;
    const int d4 = d >> 2;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < total4; q += (long)gridDim.x * 256) {
      const int i = (int)(q / d4);
      const long e = q << 2;
      float4 o1 = make_float4(0.f, 0.f, 0.f, 0.f), o2 = make_float4(0.f, 0.f, 0.f, 0.f);
      float rs3 = 0.f;
      for (int z = 0; z < jsplit; ++z) {
        const float4 a = *reinterpret_cast<const float4*>(O1 + z * zs + e);
        const float4 b = *reinterpret_cast<const float4*>(O2 + z * zs + e);
        o1.x += a.x; o1.y += a.y; o1.z += a.z; o1.w += a.w;
        o2.x += b.x; o2.y += b.y; o2.z += b.z; o2.w += b.w;
        rs3 += RS3[(size_t)z * n + i];
      }
      const float4 th = *reinterpret_cast<const float4*>(T + e);
      float4 ph;
      ph.x = imq_phi(o1.x, o2.x, th.x, rs3, c2, fn); ph.y = imq_phi(o1.y, o2.y, th.y, rs3, c2, fn);
      ph.z = imq_phi(o1.z, o2.z, th.z, rs3, c2, fn); ph.w = imq_phi(o1.w, o2.w, th.w, rs3, c2, fn);
      if (!KSD || phi) *reinterpret_cast<float4*>(phi + e) = ph;
      sq += ((double)ph.x * (double)ph.x + (double)ph.y * (double)ph.y) + ((double)ph.z * (double)ph.z + (double)ph.w * (double)ph.w);
      if constexpr (KSD) {
        const float4 g = (vec & 2) ? *reinterpret_cast<const float4*>(G + e) : make_float4(G[e], G[e + 1], G[e + 2], G[e + 3]);
        imq_ksd_terms(g.x, o1.x, o2.x, th.x, rs3, ic2, ks, kd);
        imq_ksd_terms(g.y, o1.y, o2.y, th.y, rs3, ic2, ks, kd);
        imq_ksd_terms(g.z, o1.z, o2.z, th.z, rs3, ic2, ks, kd);
        imq_ksd_terms(g.w, o1.w, o2.w, th.w, rs3, ic2, ks, kd);
        if (q == (long)i * d4) ks += row_terms(i, rs3);   // the row's first four columns
      }
    }
  } else {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
      const int i = (int)(e / d);
      float o1 = 0.f, o2 = 0.f, rs3 = 0.f;
      for (int z = 0; z < jsplit; ++z) {
        o1 += O1[z * zs + e];
        o2 += O2[z * zs + e];
        rs3 += RS3[(size_t)z * n + i];
      }
      const float th = T[e];
      const float ph = imq_phi(o1, o2, th, rs3, c2, fn);
      if (!KSD || phi) phi[e] = ph;
      sq += (double)ph * (double)ph;
      if constexpr (KSD) {
        imq_ksd_terms(G[e], o1, o2, th, rs3, ic2, ks, kd);
        if (e == (long)i * d) ks += row_terms(i, rs3);   // the row's column 0
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

__global__ __launch_bounds__(256) void k_imq_finish(const float* __restrict__ O1, const float* __restrict__ O2,
                                                    const float* __restrict__ RS3, const float* __restrict__ T,
                                                    const float* __restrict__ h2p, float* __restrict__ phi,
                                                    double* __restrict__ sqpart, int n, int d, int jsplit, int vec) {
  imq_finish_body<false>(O1, O2, RS3, nullptr, T, nullptr, h2p, phi, sqpart, nullptr, n, d, jsplit, vec);
}

__global__ __launch_bounds__(256) void k_imq_finish_ksd(const float* __restrict__ O1, const float* __restrict__ O2,
                                                        const float* __restrict__ RS3, const float* __restrict__ RD5,
                                                        const float* __restrict__ T, const float* __restrict__ G,
                                                        const float* __restrict__ h2p, float* __restrict__ phi,
                                                        double* __restrict__ sqpart, double* __restrict__ kpart, int n, int d,
                                                        int jsplit, int vec) {
  imq_finish_body<true>(O1, O2, RS3, RD5, T, G, h2p, phi, sqpart, kpart, n, d, jsplit, vec);
}

// the block partials of the finish pass in a fixed order, one workgroup per set: sqpart[count] -> out[0]; the KSD form's
// grid of three: kpart[2][count] -> out[1], out[2]
__global__ __launch_bounds__(256) void k_imq_sum(const double* __restrict__ sqpart, const double* __restrict__ kpart, int count,
                                                 double* __restrict__ out) {
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
struct ImqLayout {
  int64_t row_tiles, cblocks, jsplit, jtiles_per, sq_blocks;
  int64_t rows, dk, dc, nk;                                  // padded extents of the planes (the x3_* of SteinLayout)
  size_t r, sc, t3, tt3, gt3, o1, o2, rs3, sq, total;        // byte offsets, 256-byte aligned
  size_t rd5, kpart, ksd_total;                              // the KSD form's sections, appended behind `total`
};

static int imq_check_shape(int64_t n, int64_t d, int dtype, int flags) {
  if (dtype == STEIN_BF16) return fail(STEIN_E_UNSUPPORTED, "the IMQ step takes fp32 inputs (STEIN_F32), not bf16");
  if (dtype != STEIN_F32) return fail(STEIN_E_UNSUPPORTED, "dtype %d", dtype);
  if (flags != 0) return fail(STEIN_E_BADARG, "the IMQ step takes no flags, got 0x%x", flags);
  if (n < 1 || d < 1) return fail(STEIN_E_SHAPE, "bad shape n=%lld d=%lld", (long long)n, (long long)d);
  return stein_check_size(n, d);
}

// The plan: one workgroup per (row tile, 128-column block, j range); the j ranges fill the resident grid by the streaming
// step's rule (stream_make_layout, stein_stream.hip) with the column blocks in the place of its column groups.  The first
// three sections sit at the streaming layout's own offsets and the planes behind them are larger than the streaming
// median's histograms, so a buffer of this size also serves stein_stream_median.
static int imq_make_layout(int64_t n, int64_t d, ImqLayout* L) {
  L->row_tiles = (n + ST_ROWS - 1) / ST_ROWS;
  L->cblocks = (d + 127) / 128;
  const int64_t jtiles = L->row_tiles;
  const int hook = stein_stream_jsplit_hook();
  int64_t want = hook > 0 ? hook : (int64_t)(RESIDENT_ONE_PER_CU / (double)(L->row_tiles * L->cblocks));
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
  L->tt3 = put((size_t)3 * L->dc * L->nk * 2);
  L->gt3 = put((size_t)3 * L->dc * L->nk * 2);
  L->o1 = put((size_t)L->jsplit * n * d * 4);
  L->o2 = put((size_t)L->jsplit * n * d * 4);
  L->rs3 = put((size_t)L->jsplit * n * 4);
  L->sq = put((size_t)sqb * 8);
  L->total = at;
  L->rd5 = put((size_t)L->jsplit * n * 4);
  L->kpart = put((size_t)2 * sqb * 8);
  L->ksd_total = at;
  if (L->row_tiles * L->cblocks * L->jsplit > 0x7fffffffll) return fail(STEIN_E_SHAPE, "too many tiles");
  return STEIN_OK;
}

// every address the split launchers take (of a stored-D layout only the planes' extents)
static StepViews imq_views(const ImqLayout& L, void* workspace) {
  char* ws = (char*)workspace;
  StepViews v{};
  v.L.x3_rows = L.rows; v.L.x3_dk = L.dk; v.L.x3_dc = L.dc; v.L.x3_nk = L.nk;
  v.r = (float*)(ws + L.r);
  v.planes = ws;
  v.T3 = (unsigned short*)(ws + L.t3);
  v.Tt3 = (unsigned short*)(ws + L.tt3);
  v.Gt3 = (unsigned short*)(ws + L.gt3);
  v.sc = (float*)(ws + L.sc);
  v.cmax = (u32*)(v.sc + x3_sc_cmax(L.dc));
  v.two_s = v.sc + x3_sc_two_s(L.dc);
  v.OG = (float*)(ws + L.o1);
  v.OT = (float*)(ws + L.o2);
  v.RS = (float*)(ws + L.rs3);
  v.SQ = (double*)(ws + L.sq);
  return v;
}

static int imq_workspace_bytes(int64_t n, int64_t d, int dtype, int flags, size_t* out_bytes, bool ksd) {
  if (!out_bytes) return fail(STEIN_E_BADARG, "out_bytes is NULL");
  int rc = imq_check_shape(n, d, dtype, flags);
  if (rc) return rc;
  ImqLayout L;
  if ((rc = imq_make_layout(n, d, &L))) return rc;
  *out_bytes = ksd ? L.ksd_total : L.total;
  return STEIN_OK;
}

extern "C" int stein_imq_workspace_bytes(int64_t n, int64_t d, int dtype, int flags, size_t* out_bytes) {
  return imq_workspace_bytes(n, d, dtype, flags, out_bytes, false);
}

extern "C" int stein_imq_ksd_workspace_bytes(int64_t n, int64_t d, int dtype, int flags, size_t* out_bytes) {
  return imq_workspace_bytes(n, d, dtype, flags, out_bytes, true);
}

extern "C" int stein_imq_plan(int64_t n, int64_t d, int* row_tiles, int* col_blocks, int* jsplit) {
  if (!row_tiles || !col_blocks || !jsplit) return fail(STEIN_E_BADARG, "NULL output");
  int rc = imq_check_shape(n, d, STEIN_F32, 0);
  if (rc) return rc;
  ImqLayout L;
  if ((rc = imq_make_layout(n, d, &L))) return rc;
  *row_tiles = (int)L.row_tiles;
  *col_blocks = (int)L.cblocks;
  *jsplit = (int)L.jsplit;
  return STEIN_OK;
}

// The launches in front of the contraction: row norms (the padding rows of r are never read into a stored result), then the
// unfolded split: column maxima -> scales, theta's row-major planes, theta^T's and G^T's planes
static int imq_operands(const StepViews& v, const void* theta, const void* score, int64_t n, int64_t d, int dtype,
                        hipStream_t s) {
  if (int rc = stein_rownorms(theta, n, d, dtype, v.r, (void*)s)) return rc;
  return stein_x3_split(v, theta, score, dtype, n, d, s, nullptr);
}

extern "C" int stein_svgd_phi_imq(const void* theta, const void* score, int64_t n, int64_t d, int dtype, const float* h2_in,
                                  float* phi, double* sqnorm_out, void* workspace, size_t ws_bytes, int flags, void* stream) {
  if (!theta || !score || !h2_in || !phi || !sqnorm_out || !workspace) return fail(STEIN_E_BADARG, "NULL pointer");
  if ((uintptr_t)workspace & 15) return fail(STEIN_E_BADARG, "the workspace must be 16-byte aligned");   // (16-byte loads of its sections)
  int rc = imq_check_shape(n, d, dtype, flags);
  if (rc) return rc;
  ImqLayout L;
  if ((rc = imq_make_layout(n, d, &L))) return rc;
  if (ws_bytes < L.total) return fail(STEIN_E_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, L.total);
  if ((rc = stein_take_device_error())) return rc;   // a kernel of an earlier call on this device gave up: say so now
  hipStream_t s = (hipStream_t)stream;
  const StepViews v = imq_views(L, workspace);
  if ((rc = imq_operands(v, theta, score, n, d, dtype, s))) return rc;
  const long nblk = (long)(L.row_tiles * L.cblocks * L.jsplit);
  hipLaunchKernelGGL(k_phi_imq, dim3((unsigned)nblk), dim3(ST_THREADS), 0, s, v.T3, (int)(L.dk / 32), v.Gt3, v.Tt3,
                     (long)(L.nk / 32), v.r, v.sc, (int)L.dc, h2_in, v.OG, v.OT, v.RS, (int)n, (int)d, (int)L.row_tiles,
                     (int)L.cblocks, (int)L.row_tiles, (int)L.jtiles_per);
  LAUNCH_CHECK("k_phi_imq");
  const int vec = d % 4 == 0 && (((uintptr_t)theta | (uintptr_t)phi) & 15) == 0;
  hipLaunchKernelGGL(k_imq_finish, dim3((unsigned)L.sq_blocks), dim3(256), 0, s, v.OG, v.OT, v.RS, (const float*)theta, h2_in,
                     phi, v.SQ, (int)n, (int)d, (int)L.jsplit, vec);
  LAUNCH_CHECK("k_imq_finish");
  hipLaunchKernelGGL(k_imq_sum, dim3(1), dim3(256), 0, s, v.SQ, (const double*)nullptr, (int)L.sq_blocks, sqnorm_out);
  LAUNCH_CHECK("k_imq_sum");
  return STEIN_OK;
}

extern "C" int stein_svgd_phi_imq_ksd(const void* theta, const void* score, int64_t n, int64_t d, int dtype,
                                      const float* h2_in, float* phi, double* sums_out, void* workspace, size_t ws_bytes,
                                      int flags, void* stream) {
  if (!theta || !score || !h2_in || !sums_out || !workspace) return fail(STEIN_E_BADARG, "NULL pointer");   // (phi may be)
  if ((uintptr_t)workspace & 15) return fail(STEIN_E_BADARG, "the workspace must be 16-byte aligned");
  int rc = imq_check_shape(n, d, dtype, flags);
  if (rc) return rc;
  ImqLayout L;
  if ((rc = imq_make_layout(n, d, &L))) return rc;
  if (ws_bytes < L.ksd_total) return fail(STEIN_E_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, L.ksd_total);
  if ((rc = stein_take_device_error())) return rc;
  hipStream_t s = (hipStream_t)stream;
  const StepViews v = imq_views(L, workspace);
  float* RD5 = (float*)((char*)workspace + L.rd5);
  double* KP = (double*)((char*)workspace + L.kpart);
  if ((rc = imq_operands(v, theta, score, n, d, dtype, s))) return rc;
  const long nblk = (long)(L.row_tiles * L.cblocks * L.jsplit);
  hipLaunchKernelGGL(k_phi_imq_ksd, dim3((unsigned)nblk), dim3(ST_THREADS), 0, s, v.T3, (int)(L.dk / 32), v.Gt3, v.Tt3,
                     (long)(L.nk / 32), v.r, v.sc, (int)L.dc, h2_in, v.OG, v.OT, v.RS, RD5, (int)n, (int)d, (int)L.row_tiles,
                     (int)L.cblocks, (int)L.row_tiles, (int)L.jtiles_per);
  LAUNCH_CHECK("k_phi_imq_ksd");
  // the 16-byte path is chosen as in the plain step (a NULL phi counts as aligned), so that |phi|^2 is summed in the plain
  // step's order; the score's alignment only decides how its rows are loaded on that path (bit 1)
  const int vec = (d % 4 == 0 && (((uintptr_t)theta | (uintptr_t)phi) & 15) == 0 ? 1 : 0) | (((uintptr_t)score & 15) == 0 ? 2 : 0);
  hipLaunchKernelGGL(k_imq_finish_ksd, dim3((unsigned)L.sq_blocks), dim3(256), 0, s, v.OG, v.OT, v.RS, RD5, (const float*)theta,
                     (const float*)score, h2_in, phi, v.SQ, KP, (int)n, (int)d, (int)L.jsplit, vec);
  LAUNCH_CHECK("k_imq_finish_ksd");
  hipLaunchKernelGGL(k_imq_sum, dim3(3), dim3(256), 0, s, v.SQ, KP, (int)L.sq_blocks, sums_out);
  LAUNCH_CHECK("k_imq_sum");
  return STEIN_OK;
}
