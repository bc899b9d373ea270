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
//   k_stream_sum        (stein_stream_tile.h) the block partials in a fixed order -> the caller's doubles
// stein_svgd_phi_imq_ksd launches the KSD forms of the same bodies (k_phi_imq_ksd: a second running row sum rd5;
// k_imq_finish_ksd: reads the score rows, three sets of block partials).  Everything the step has in common with the RBF
// streaming step (stein_stream.hip) is that step's code: the tile phases other than the element function, the frame of the
// finish pass and k_stream_sum (stein_stream_tile.h), and the host side around the launches (stein_stream_host.h).
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
#include "stein_stream_host.h"

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

  const StRoles ro = st_roles();
  const int lane = ro.lane, l15 = ro.l15, lq = ro.lq, wr = ro.wr, wc = ro.wc, wcol = ro.wcol;
  // contraction role: the 32 columns at wcol of block cb; waves 0-3 K.G, waves 4-7 K3.theta (wave-uniform)
  const bool third = ro.w >= 4;

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
        unsigned char* dst = st_image_dst(smem, wr * 32 + ib * 16 + l15, jc);
        st_stage4(dst, st_split4(q));
        st_stage4(dst + ST_BUF, st_split4(q3));
      }
    }
    __syncthreads();
    // ---- contraction: O += image . V_j over the tile's (up to) four 32-deep k tiles
    for (int kt = 0; kt < ST_JT / 32; ++kt) {
      if (j0 + kt * 32 >= n) break;   // both images are zero there
      st_contract_ktile(acc, img + kt * ST_KTB + aoff, vb + ((size_t)jt * (ST_JT / 32) + kt) * 3 * XTILE_E);
    }
  }

  // ---- partial O1 / O2 of this j range (out-scaled by the operand's column scale), partial row sums
  st_store_partial((third ? O2 : O1) + (size_t)z * n * d, sc + (third ? 3 : 2) * dc, acc, cb * 128 + wcol, i0, lq, l15, n, d);
  if (cb == 0) st_reduce_rows<KSD>(smem, rs, rd, RS3, RD5, z, i0, n, sc + 4 * dc + 2, ro);
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

// The IMQ step's part of the finish pass (st_finish_body, stein_stream_tile.h): two operands, o[0] = sum_z O1_z (K.G) and
// o[1] = sum_z O2_z (K3.theta); phi = (o[0] + (rs3 theta - o[1]) / c2) / n; the statistic's terms (the file's header) per
// element, and per row d rs3 / c2 - 3 rd5 / c2^2.
struct ImqFinish {
  static constexpr int NO = 2;
  float c2, fn;
  double ic2, dd;   // (KSD)
  __device__ ImqFinish(const float* __restrict__ h2p, int n, int d)
      : c2(2.f * *h2p), fn((float)n), ic2(1.0 / (2.0 * (double)*h2p)), dd((double)d) {}
  __device__ float phi(const float (&o)[NO], float th, float rs3) const {
    return (o[0] + __builtin_fmaf(rs3, th, -o[1]) / c2) / fn;
  }
  __device__ void ksd_terms(float g, const float (&o)[NO], float th, float rs3, double& s, double& sd) const {
    const double gd = g;
    s += gd * ((double)o[0] + 2.0 * ic2 * ((double)rs3 * (double)th - (double)o[1]));
    sd += gd * gd + ic2;
  }
  __device__ double row_term(float rs3, float rd5) const { return ic2 * (dd * (double)rs3 - 3.0 * ic2 * (double)rd5); }
};

__global__ __launch_bounds__(256) void k_imq_finish(const float* __restrict__ O1, const float* __restrict__ O2,
                                                    const float* __restrict__ RS3, const float* __restrict__ T,
                                                    const float* __restrict__ h2p, float* __restrict__ phi,
                                                    double* __restrict__ sqpart, int n, int d, int jsplit, int vec) {
  st_finish_body<ImqFinish, false>(O1, O2, RS3, nullptr, T, nullptr, h2p, phi, sqpart, nullptr, n, d, jsplit, vec);
}

__global__ __launch_bounds__(256) void k_imq_finish_ksd(const float* __restrict__ O1, const float* __restrict__ O2,
                                                        const float* __restrict__ RS3, const float* __restrict__ RD5,
                                                        const float* __restrict__ T, const float* __restrict__ G,
                                                        const float* __restrict__ h2p, float* __restrict__ phi,
                                                        double* __restrict__ sqpart, double* __restrict__ kpart, int n, int d,
                                                        int jsplit, int vec) {
  st_finish_body<ImqFinish, true>(O1, O2, RS3, RD5, T, G, h2p, phi, sqpart, kpart, n, d, jsplit, vec);
}

// ================================================================================================
// host side (shape check, layout, views, prologue, last launch: stein_stream_host.h, the RBF streaming step's too)
// ================================================================================================
// The plan: one workgroup per (row tile, 128-column block, j range); the j ranges fill the resident grid by the streaming
// step's rule with the column blocks in the place of its column groups.  The workspace: the streaming step's with two sets
// of transposed planes (theta^T, then G^T) and two sets of partial O; the first three sections are the same code's, so a
// buffer of this size also serves stein_stream_median.
extern "C" int stein_imq_workspace_bytes(int64_t n, int64_t d, int dtype, int flags, size_t* out_bytes) {
  return stream_workspace_bytes(STREAM_IMQ, false, n, d, dtype, flags, out_bytes);
}

extern "C" int stein_imq_ksd_workspace_bytes(int64_t n, int64_t d, int dtype, int flags, size_t* out_bytes) {
  return stream_workspace_bytes(STREAM_IMQ, true, n, d, dtype, flags, out_bytes);
}

extern "C" int stein_imq_plan(int64_t n, int64_t d, int* row_tiles, int* col_blocks, int* jsplit) {
  return stream_plan(STREAM_IMQ, n, d, row_tiles, col_blocks, jsplit);
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
  StreamCall c;
  int rc = stream_begin(STREAM_IMQ, false, theta, score, n, d, dtype, h2_in, phi, sqnorm_out, workspace, ws_bytes, flags, stream, &c);
  if (rc) return rc;
  const StreamLayout& L = c.L;
  const StepViews& v = c.v;
  if ((rc = imq_operands(v, theta, score, n, d, dtype, c.s))) return rc;
  hipLaunchKernelGGL(k_phi_imq, dim3(c.nblk), dim3(ST_THREADS), 0, c.s, v.T3, (int)(L.dk / 32), v.Gt3, v.Tt3,
                     (long)(L.nk / 32), v.r, v.sc, (int)L.dc, h2_in, v.OG, v.OT, v.RS, (int)n, (int)d, (int)L.row_tiles,
                     (int)L.cblocks, (int)L.row_tiles, (int)L.jtiles_per);
  LAUNCH_CHECK("k_phi_imq");
  hipLaunchKernelGGL(k_imq_finish, dim3((unsigned)L.sq_blocks), dim3(256), 0, c.s, v.OG, v.OT, v.RS, (const float*)theta, h2_in,
                     phi, v.SQ, (int)n, (int)d, (int)L.jsplit, c.vec);
  LAUNCH_CHECK("k_imq_finish");
  return stream_sum(c, sqnorm_out);
}

extern "C" int stein_svgd_phi_imq_ksd(const void* theta, const void* score, int64_t n, int64_t d, int dtype,
                                      const float* h2_in, float* phi, double* sums_out, void* workspace, size_t ws_bytes,
                                      int flags, void* stream) {
  StreamCall c;
  int rc = stream_begin(STREAM_IMQ, true, theta, score, n, d, dtype, h2_in, phi, sums_out, workspace, ws_bytes, flags, stream, &c);
  if (rc) return rc;
  const StreamLayout& L = c.L;
  const StepViews& v = c.v;
  if ((rc = imq_operands(v, theta, score, n, d, dtype, c.s))) return rc;
  hipLaunchKernelGGL(k_phi_imq_ksd, dim3(c.nblk), dim3(ST_THREADS), 0, c.s, v.T3, (int)(L.dk / 32), v.Gt3, v.Tt3,
                     (long)(L.nk / 32), v.r, v.sc, (int)L.dc, h2_in, v.OG, v.OT, v.RS, c.RD, (int)n, (int)d, (int)L.row_tiles,
                     (int)L.cblocks, (int)L.row_tiles, (int)L.jtiles_per);
  LAUNCH_CHECK("k_phi_imq_ksd");
  hipLaunchKernelGGL(k_imq_finish_ksd, dim3((unsigned)L.sq_blocks), dim3(256), 0, c.s, v.OG, v.OT, v.RS, c.RD, (const float*)theta,
                     (const float*)score, h2_in, phi, v.SQ, c.KP, (int)n, (int)d, (int)L.jsplit, c.vec);
  LAUNCH_CHECK("k_imq_finish_ksd");
  return stream_sum(c, sums_out);
}
