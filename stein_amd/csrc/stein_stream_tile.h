// stein_stream_tile.h -- what the streaming kernels of stein_stream.hip (k_phi_stream, k_stream_hist) and of stein_imq.hip
// (k_phi_imq) share: the geometry of one 128 x 128 distance tile with its P image in LDS, and the distance phase itself.
// One body for all of them: every kernel forms every S value in the same order, so the streaming median is the median of
// the very D values both steps consume.
#pragma once
#include "stein_x3_dev.h"

constexpr int ST_THREADS = 512;
constexpr int ST_ROWS = 128;              // particles per row tile
constexpr int ST_JT = 128;                // columns of D per step (4 k tiles of the contraction)
constexpr int ST_PLN = ST_ROWS * XROW;    // one plane of one 32-deep k tile of P in LDS: 8 KB
constexpr int ST_KTB = 2 * ST_PLN;        // hi and lo plane
constexpr int ST_BUF = (ST_JT / 32) * ST_KTB;   // one P image: 64 KB; two of them

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
