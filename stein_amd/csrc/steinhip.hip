// steinhip.hip -- gfx950 (MI355X / CDNA4) kernels and C ABI for the SVGD particle update.
//
// Pipeline for one step on one rank (rows [row0, row0+n_local) of n particles, d parameters):
//   k_rownorms      r_i = |theta_i|^2                                   HBM-bound, 4nd bytes
//   k_distance      D = r_i + r_j - 2 theta theta^T  (fp32 MFMA 32x32x2, 128x128 tiles, LDS staged; stein_fp32.hip)
//   k_hist x3       3-level radix select over the fp32 bit patterns of D (exact median; stein_select.hip)
//   k_resolve x3    1-wave kernel that walks the histogram; last level -> median, h^2
//   k_phi_partial   P = exp(-D/2h^2) built on the fly from the D tile, O += P.[G|theta] (fp32 MFMA),
//                   rowsum(P) on the VALU -- K is never materialised (stein_fp32.hip)
//   k_phi_finish    phi = (O_G + (rowsum*theta - O_T)/h^2)/n, per-block partial |phi|^2 (fp64)
//   k_sum_partial_sets  deterministic reduction of the partials
//   k_apply_*       clip + Adagrad/Adam + theta += step, one streaming pass (stein_apply.hip)
// Reference formulae: see include/steinhip.h for the file:line of each stage.
// This file holds the workspace layout, the fused single-rank call, the staged distance / contraction entry points, the
// rank-step segments, the stage timing and the device error word.
//
// Everything is launched on the caller's stream; nothing here synchronises with the host.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <stdarg.h>
#include <string.h>
#include <math.h>

#include "stein_host.h"
#include "stein_x3.h"

#include <type_traits>
#include <vector>

// ------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

int stein_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

extern "C" int stein_version(void) { return STEIN_VERSION; }
extern "C" const char* stein_last_error(void) { return g_err; }

// ------------------------------------------------------------------------------------------------
// k_rownorms: one wave per row
// ------------------------------------------------------------------------------------------------
template <typename TIN>
__global__ __launch_bounds__(256) void k_rownorms(const TIN* __restrict__ T, int n, int d, float* __restrict__ r) {
  const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (wave >= n) return;
  const float s = wave_row_sqnorm(T + (size_t)wave * d, d, lane);
  if (lane == 0) r[wave] = s;
}

// First kernel of the fused call (fp32 inputs; bf16 inputs: the same work rides in k_split's launch, stein_x3.hip): the row
// norms and everything the later kernels expect to find zeroed or set up (prologue_body, stein_common.h).
template <typename TIN>
__global__ __launch_bounds__(256) void k_prologue(const TIN* __restrict__ T, PrologueArgs a) {
  prologue_body<TIN>(T, a, (int)blockIdx.x, (int)gridDim.x);
}

// ------------------------------------------------------------------------------------------------
// k_kernel_matrix: optional K output, K = exp(-D / h2 / 2)
// ------------------------------------------------------------------------------------------------
// upper: D holds only the 128 x 128 tiles on and above the diagonal (the split path's symmetric distance pass); an entry
// of a tile below it is read from its mirror image
__global__ __launch_bounds__(256) void k_kernel_matrix(const float* __restrict__ D, long ldD, int n_local, int n,
                                                       const float* __restrict__ h2p, float* __restrict__ K, long ldK,
                                                       int upper) {
  const float h2 = *h2p;
  const long total = (long)n_local * n;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long row = e / n, col = e - row * n;
    const bool swap = upper && (col >> 7) < (row >> 7);
    K[row * ldK + col] = expf(-D[d_index(swap ? col : row, swap ? row : col, ldD >> 5)] / h2 / 2.f);
  }
}

// ------------------------------------------------------------------------------------------------
// k_phi_finish: sum the split partials, form phi, per-block partial |phi|^2 in fp64
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 theta4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 theta4(const unsigned short* p) {   // four bf16 values (8-byte aligned)
  const uint2 w = *reinterpret_cast<const uint2*>(p);
  return make_float4(__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u), __uint_as_float(w.y << 16),
                     __uint_as_float(w.y & 0xffff0000u));
}
// KSD (STEIN_FLAG_KSD): also this call's shares of the Stein discrepancy sums S and S_diag (ksd_terms) from the score rows
// G; their block partials follow the |phi|^2 partials in sqpart ([3][gridDim.x]) and sq_out is double[3].  The KSD = false
// instantiation is the kernel without the statistic.
// FOLD (the fused call's folded operand, stein_x3.hip): OG holds the partials of K.W, W = G - theta / h2, and
// phi = (ow + rs theta / h2) / n.  OT (K.theta) exists and is read only when dK or the statistic is asked for; phi never
// touches it, so it is the same to the bit with and without them.  The statistic gets og = ow + ot / h2 formed in fp64.
template <typename TIN, bool KSD, bool FOLD = false>
__global__ __launch_bounds__(256) void k_phi_finish(const float* __restrict__ OG, const float* __restrict__ OT,
                                                    const float* __restrict__ RS, const TIN* __restrict__ T,
                                                    const float* __restrict__ h2p, float* __restrict__ phi,
                                                    float* __restrict__ dK, double* __restrict__ sqpart, int n, int d,
                                                    int row0, int n_local, int split, int tsplit, int vec, HistSync* done,
                                                    double* __restrict__ sq_out, const TIN* __restrict__ G) {
  // done != NULL (fused call; its completion counters are zero at launch): the last workgroup out also sums the partials --
  // as k_sum_partial_sets does (block_sum256), so the result is the same to the last bit -- which saves that launch
  constexpr int NS = KSD ? 3 : 1;       // sums: |phi|^2 (, S, S_diag)
  __shared__ double red[4 * NS];
  const float h2 = *h2p;
  const float fn = (float)n;
  const long total = (long)n_local * d;
  const size_t zs = (size_t)n_local * d;
  double sq = 0.0;
  double ks = 0.0, kd = 0.0;            // KSD: this thread's shares of S and S_diag
  const double ih = 1.0 / (double)h2;
  const bool need_t = !FOLD || KSD || dK != nullptr;
  auto kg = [&](float o, float t) { return FOLD ? (double)o + (double)t * ih : (double)o; };   // (K.G)_e for the statistic
  if (vec) {   // host: d % 4 == 0 and every pointer aligned for four columns at a time
    // four consecutive columns of one row per step, 16-byte loads and stores (one entry at a time with an integer
    // division each, the kernel moved its 68 MB at 2.8 TB/s; bf16 inputs took that path until round 4: 19 us at C2)
    const long total4 = total >> 2;
    const int d4 = d >> 2;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < total4; q += (long)gridDim.x * 256) {
      const int i = (int)(q / d4);
      const long e = q << 2;
      float4 og = make_float4(0.f, 0.f, 0.f, 0.f), ot = og;
      float rs = 0.f;
#pragma unroll 8
      for (int z = 0; z < split; ++z) {   // unrolled: the loads of eight slices in flight, the sums in the same order
        const float4 a = *reinterpret_cast<const float4*>(OG + z * zs + e);
        og.x += a.x; og.y += a.y; og.z += a.z; og.w += a.w;
        if (FOLD ? need_t && z < tsplit : true) {   // (FOLD: K.theta comes in tsplit = 1 range)
          const float4 b = *reinterpret_cast<const float4*>(OT + z * zs + e);
          ot.x += b.x; ot.y += b.y; ot.z += b.z; ot.w += b.w;
        }
        rs += RS[(size_t)z * n_local + i];
      }
      const float4 th = theta4(T + (size_t)row0 * d + e);
      float4 dk, ph;
      dk.x = (rs * th.x - ot.x) / h2; dk.y = (rs * th.y - ot.y) / h2; dk.z = (rs * th.z - ot.z) / h2; dk.w = (rs * th.w - ot.w) / h2;
      if constexpr (FOLD) {
        ph.x = (og.x + rs * th.x / h2) / fn; ph.y = (og.y + rs * th.y / h2) / fn;
        ph.z = (og.z + rs * th.z / h2) / fn; ph.w = (og.w + rs * th.w / h2) / fn;
      } else {
        ph.x = (og.x + dk.x) / fn; ph.y = (og.y + dk.y) / fn; ph.z = (og.z + dk.z) / fn; ph.w = (og.w + dk.w) / fn;
      }
      *reinterpret_cast<float4*>(phi + e) = ph;
      if (dK) *reinterpret_cast<float4*>(dK + e) = dk;
      sq += ((double)ph.x * (double)ph.x + (double)ph.y * (double)ph.y) + ((double)ph.z * (double)ph.z + (double)ph.w * (double)ph.w);
      if constexpr (KSD) {
        const float4 g = theta4(G + (size_t)row0 * d + e);
        ksd_terms(g.x, kg(og.x, ot.x), ot.x, th.x, rs, ih, ks, kd);
        ksd_terms(g.y, kg(og.y, ot.y), ot.y, th.y, rs, ih, ks, kd);
        ksd_terms(g.z, kg(og.z, ot.z), ot.z, th.z, rs, ih, ks, kd);
        ksd_terms(g.w, kg(og.w, ot.w), ot.w, th.w, rs, ih, ks, kd);
      }
    }
  } else {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
      const int i = (int)(e / d);
      float og = 0.f, ot = 0.f, rs = 0.f;
      for (int z = 0; z < split; ++z) {
        og += OG[z * zs + e];
        if (FOLD ? need_t && z < tsplit : true) ot += OT[z * zs + e];
        rs += RS[(size_t)z * n_local + i];
      }
      const float th = elem_f32(T + (size_t)row0 * d + e);
      const float dk = (rs * th - ot) / h2;
      const float ph = FOLD ? (og + rs * th / h2) / fn : (og + dk) / fn;
      phi[e] = ph;
      if (dK) dK[e] = dk;
      sq += (double)ph * (double)ph;
      if constexpr (KSD) ksd_terms(elem_f32(G + (size_t)row0 * d + e), kg(og, ot), ot, th, rs, ih, ks, kd);
    }
  }
  double part[NS];                      // this workgroup's partials, set k at sqpart[k * gridDim.x + blockIdx.x]
  part[0] = sq;
  if constexpr (KSD) { part[1] = ks; part[2] = kd; }
  block_sum256(part, red);
  if (!done) {
    if (threadIdx.x == 0)
      for (int k = 0; k < NS; ++k) sqpart[k * gridDim.x + blockIdx.x] = part[k];
    return;
  }
  // the partials cross workgroups: written with device-scope atomics, read with load_fresh (tree_report_done)
  if (threadIdx.x == 0)
    for (int k = 0; k < NS; ++k)
      __hip_atomic_store(reinterpret_cast<u64*>(sqpart) + k * gridDim.x + blockIdx.x, (u64)__double_as_longlong(part[k]),
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  {
    __shared__ u32 s_last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's partial has been acknowledged
    __syncthreads();
    if (threadIdx.x == 0) s_last = tree_report_done(done->fin_leaf, &done->fin_top, blockIdx.x, gridDim.x) ? 1u : 0u;
    __syncthreads();
    if (!s_last) return;
  }
  double tot[NS];                       // every set in the same order: thread t takes partials t, t + 256, ...
  for (int k = 0; k < NS; ++k) {
    tot[k] = 0.0;
    for (int i = threadIdx.x; i < (int)gridDim.x; i += 256)
      tot[k] += __longlong_as_double((long long)load_fresh(reinterpret_cast<const u64*>(sqpart) + k * gridDim.x + i));
  }
  __syncthreads();
  block_sum256(tot, red);
  if (threadIdx.x == 0)
    for (int k = 0; k < NS; ++k) sq_out[k] = tot[k];
}

// the partial sets [gridDim.x][count] of a finish pass (|phi|^2; STEIN_FLAG_KSD: S and S_diag behind it): workgroup k sums
// set k into out[k]
__global__ __launch_bounds__(256) void k_sum_partial_sets(const double* __restrict__ part, int count, double* out) {
  __shared__ double red[4];
  const double* p = part + (size_t)blockIdx.x * count;
  double s[1] = {0.0};
  for (int i = threadIdx.x; i < count; i += 256) s[0] += p[i];
  block_sum256(s, red);
  if (threadIdx.x == 0) out[blockIdx.x] = s[0];
}

// the |phi|^2 partials of a finish pass (and with STEIN_FLAG_KSD the S / S_diag partials behind them) -> sqnorm_out[0 (.. 2)]
static int sum_partials(const double* part, int count, bool ksd, double* out, hipStream_t s) {
  hipLaunchKernelGGL(k_sum_partial_sets, dim3(ksd ? 3 : 1), dim3(256), 0, s, part, count, out);
  LAUNCH_CHECK("k_sum_partial_sets");
  return STEIN_OK;
}

// ================================================================================================
// host side
// ================================================================================================
static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

int stein_make_layout(int64_t n_local, int64_t n, int64_t d, int dtype, int flags, SteinLayout* L) {
  if (n < 2) return fail(STEIN_E_BADARG, "n = %lld: the bandwidth divides by ln(n), need n >= 2", (long long)n);
  if (d < 1 || n_local < 1 || n_local > n) return fail(STEIN_E_SHAPE, "bad shape n_local=%lld n=%lld d=%lld", (long long)n_local, (long long)n, (long long)d);
  if (n > (1ll << 30) || d > (1ll << 24) || n * d > (1ll << 40)) return fail(STEIN_E_SHAPE, "shape too large");
  if (dtype != STEIN_F32 && dtype != STEIN_BF16) return fail(STEIN_E_UNSUPPORTED, "dtype %d", dtype);
  if (flags & ~(STEIN_FLAG_X3 | STEIN_FLAG_TIMING | STEIN_FLAG_TILED | STEIN_FLAG_NO_WINDOW | STEIN_FLAG_RANK_WINDOW | STEIN_FLAG_TILE_DISTANCE | STEIN_FLAG_TIMING_CONTRACT | STEIN_FLAG_KSD | STEIN_FLAG_FOLD | STEIN_FLAG_NO_FOLD)) return fail(STEIN_E_BADARG, "unknown flags 0x%x", flags);
  if ((flags & STEIN_FLAG_FOLD) && (flags & STEIN_FLAG_NO_FOLD)) return fail(STEIN_E_BADARG, "STEIN_FLAG_FOLD and STEIN_FLAG_NO_FOLD exclude each other");
  L->ld_dist = (int64_t)align_up((size_t)n, 64);
  L->tiles_m = (n_local + BM - 1) / BM;
  L->cblocks = (d + BN - 1) / BN;
  // workgroups per unit of split and resident workgroups per round: the fp32 kernel tiles [G | theta] in 128-column
  // blocks at 3 workgroups per CU; the split-precision kernel pairs the blocks up (256 columns) at 1 workgroup per CU
  const bool x3 = (flags & STEIN_FLAG_X3) != 0;
  const int64_t base = x3 ? L->tiles_m * L->cblocks : L->tiles_m * 2 * L->cblocks;
  const int64_t jt = (n + BK - 1) / BK;  // j tiles
  // k_phi_partial runs 3 workgroups per CU (156 registers): 768 resident blocks.  Every block does the same
  // work, so the launch takes ceil(blocks / 768) rounds; pick the j-split that wastes least of the last round
  // (ties -> fewer splits, i.e. less partial traffic), keeping at least 8 j-tiles (256 columns) per split.
  const double resident = x3 ? 256.0 : 768.0;
  int64_t max_split = jt / 8 > 0 ? jt / 8 : 1;
  if (max_split > 16) max_split = 16;
  auto choose_split = [&](int64_t base_wgs, int64_t* jchunk_out) {
    int64_t split = 1;
    double best = -1.0;
    for (int64_t s = 1; s <= max_split; ++s) {
      const double rounds = (double)(base_wgs * s) / resident;
      const double eff = rounds / ceil(rounds) - 0.004 * (double)(s - 1);
      if (eff > best + 1e-9) { best = eff; split = s; }
    }
    int64_t tiles_per = (jt + split - 1) / split;
    if (x3) tiles_per = (tiles_per + 3) / 4 * 4;   // a j range of the split kernel starts on a multiple of 128 columns (its
                                                   // pipeline stages then never straddle a row tile's diagonal block)
    *jchunk_out = tiles_per * BK;
    return (jt + tiles_per - 1) / tiles_per;  // drop empty tails
  };
  const int64_t split = choose_split(base, &L->jchunk);
  L->split = split;
  const int64_t elems = n_local * d;
  int64_t sqb = (elems + 1023) / 1024;
  if (sqb > 1024) sqb = 1024;
  L->sq_blocks = sqb;

  size_t at = 0;
  auto put = [&](int sec, size_t bytes) { L->off[sec] = at; at = align_up(at + bytes, 256); };
  put(STEIN_WS_ROWNORM, (size_t)n * 4);
  put(STEIN_WS_DIST, align_up((size_t)n_local, DT_ROWS) * L->ld_dist * 4);   // tile-major, rows padded to 128
  put(STEIN_WS_HIST, (size_t)STEIN_HIST_LEVELS * 2 * STEIN_HIST_BINS * 8);
  put(STEIN_WS_SELECT, sizeof(SelState) + sizeof(SpecState) + sizeof(FuseState));
  put(STEIN_WS_PART_G, (size_t)split * n_local * d * 4);
  put(STEIN_WS_PART_T, (size_t)split * n_local * d * 4);
  put(STEIN_WS_PART_RS, (size_t)split * n_local * 4);
  {  // k_phi_finish writes sq_blocks partials, the one-kernel small path one per 32 parameter columns; STEIN_FLAG_KSD: three
     // sets of them (|phi|^2, S, S_diag)
    const int64_t small = (d + 31) / 32;
    put(STEIN_WS_SQPART, (size_t)(sqb > small ? sqb : small) * 8 * ((flags & STEIN_FLAG_KSD) ? 3 : 1));
  }
  // slots | entries | rank-summed table.  Empty when the fused call will take the one-kernel path (stein_small.hip never
  // touches it): the reference's own example sizes then carry a few hundred KB of workspace instead of 16.5 MB
  const bool small_path = !(flags & STEIN_FLAG_TILED) && n_local == n && stein_small_ok(n, d, dtype);
  put(STEIN_WS_SPEC, small_path ? 0 : ((size_t)SPEC_CAP + SPEC_SLOTS * 8 + SPEC_TABLE) * 8);
  // split operand planes: always LAST so the offsets above do not depend on the flag
  L->x3_rows = (int64_t)align_up((size_t)n, 128) + 128;   // a rank's last row tile may start past roundup(n, 128) - 128
  L->x3_dk = (int64_t)align_up((size_t)d, 32);
  L->x3_dc = (int64_t)align_up((size_t)d, 128);
  L->x3_nk = (int64_t)align_up((size_t)n, 32);
  const size_t t3 = align_up((size_t)3 * L->x3_rows * L->x3_dk * 2, 256);
  const size_t tt3 = align_up((size_t)3 * L->x3_dc * L->x3_nk * 2, 256);
  L->x3_t3 = 0;
  L->x3_tt3 = t3;
  L->x3_gt3 = t3 + tt3;
  L->x3_sc = t3 + 2 * tt3;   // scales area: float[4 dc + 4] + u32[2 dc]
  const size_t scb = align_up((size_t)(6 * L->x3_dc + 4) * 4, 256);
  // The folded operand (stein_x3.hip): the fused single-rank call on the split path with fp32 inputs, where it pays or is
  // forced.  Its contraction has half the workgroups per row tile (the 128-column blocks of ONE matrix, paired), so it gets a
  // j split of its own by the same rule -- C3: 128 row tiles x 1 workgroup x 2 ranges = one round of the 256 CUs; C5: 1024 x 1
  // = four rounds; C4: 64 x 8 = two.  Its partial sums reuse storage that is dead by then, so a workspace does not grow with
  // the default gate: K.W takes PART_G and PART_T together (half the workgroups per range: rarely more than twice the
  // ranges), K.theta (dK / KSD calls; one range, so that the W half never depends on it) and the row sums take theta's
  // row-major planes, which only the distance pass reads.  Where that does not fit, a forced fold appends the three to the
  // PLANES section and the default gate leaves the call unfolded.
  const bool fold_forced = (flags & STEIN_FLAG_FOLD) != 0;
  L->fold = x3 && dtype == STEIN_F32 && n_local == n && !small_path && !(flags & STEIN_FLAG_NO_FOLD) &&
            (fold_forced || stein_fold_pays(n, d));
  L->fsplit = L->fjchunk = 0;
  size_t fold_extra = 0;
  if (L->fold) {
    L->fsplit = choose_split(L->tiles_m * ((L->cblocks + 1) / 2), &L->fjchunk);
    const size_t ow = align_up((size_t)L->fsplit * n_local * d * 4, 256), ot = align_up((size_t)n_local * d * 4, 256),
                 rs = align_up((size_t)L->fsplit * n_local * 4, 256);
    if (ow <= L->off[STEIN_WS_PART_RS] - L->off[STEIN_WS_PART_G] && ot + rs <= t3) {
      L->fold_ow = L->off[STEIN_WS_PART_G];
      L->fold_ot = at + L->x3_t3;   // (`at`: where the PLANES section is about to be put)
      L->fold_rs = L->fold_ot + ot;
    } else if (fold_forced) {
      L->fold_ow = at + t3 + 2 * tt3 + scb;
      L->fold_ot = L->fold_ow + ow;
      L->fold_rs = L->fold_ot + ot;
      fold_extra = ow + ot + rs;
    } else {
      L->fold = 0;
      L->fsplit = L->fjchunk = 0;
    }
  }
  put(STEIN_WS_PLANES, (flags & STEIN_FLAG_X3) ? t3 + 2 * tt3 + scb + fold_extra : 0);
  L->total = at;
  return STEIN_OK;
}

StepViews stein_step_views(const SteinLayout& L, void* workspace) {
  char* ws = (char*)workspace;
  StepViews v;
  v.L = L;
  v.r = (float*)(ws + L.off[STEIN_WS_ROWNORM]);
  v.D = (float*)(ws + L.off[STEIN_WS_DIST]);
  v.hist = (u64*)(ws + L.off[STEIN_WS_HIST]);
  v.sel = (SelState*)(ws + L.off[STEIN_WS_SELECT]);
  v.spec = spec_of(v.sel);
  v.fuse = fuse_of(v.sel);
  v.spec_buf = (u64*)(ws + L.off[STEIN_WS_SPEC]);
  v.table = spec_table_of(v.spec_buf);
  v.planes = L.total > L.off[STEIN_WS_PLANES] ? ws + L.off[STEIN_WS_PLANES] : nullptr;   // (empty without STEIN_FLAG_X3)
  v.OG = (float*)(ws + L.off[STEIN_WS_PART_G]);
  v.OT = (float*)(ws + L.off[STEIN_WS_PART_T]);
  v.RS = (float*)(ws + L.off[STEIN_WS_PART_RS]);
  v.SQ = (double*)(ws + L.off[STEIN_WS_SQPART]);
  return v;
}

extern "C" int stein_workspace_bytes(int64_t n_local, int64_t n, int64_t d, int dtype, int flags, size_t* out) {
  if (!out) return fail(STEIN_E_BADARG, "out is NULL");
  SteinLayout L;
  int rc = stein_make_layout(n_local, n, d, dtype, flags, &L);
  if (rc) return rc;
  *out = L.total;
  return STEIN_OK;
}

extern "C" int stein_workspace_layout(int64_t n_local, int64_t n, int64_t d, int dtype, int flags, size_t* offsets,
                                      int64_t* extra) {
  if (!offsets || !extra) return fail(STEIN_E_BADARG, "NULL output");
  SteinLayout L;
  int rc = stein_make_layout(n_local, n, d, dtype, flags, &L);
  if (rc) return rc;
  for (int i = 0; i < STEIN_WS_NSECTIONS; ++i) offsets[i] = L.off[i];
  extra[STEIN_WSX_LD_DIST] = L.ld_dist;
  extra[STEIN_WSX_SPLIT] = L.split;
  extra[STEIN_WSX_SQ_BLOCKS] = L.sq_blocks;
  extra[STEIN_WSX_HIST_BINS] = STEIN_HIST_BINS;
  return STEIN_OK;
}

extern "C" int stein_layout_folds(int64_t n_local, int64_t n, int64_t d, int dtype, int flags, int* out) {
  if (!out) return fail(STEIN_E_BADARG, "out is NULL");
  SteinLayout L;
  int rc = stein_make_layout(n_local, n, d, dtype, flags, &L);
  if (rc) return rc;
  *out = (int)L.fold;
  return STEIN_OK;
}

extern "C" int stein_x3_prepare(const void* theta_all, const void* score_all, int64_t n, int64_t d, int dtype,
                                void* x3_planes, size_t planes_bytes, void* stream) {
  if ((!theta_all && !score_all) || !x3_planes) return fail(STEIN_E_BADARG, "NULL pointer");
  SteinLayout L;
  int rc = stein_make_layout(n, n, d, dtype, STEIN_FLAG_X3 | STEIN_FLAG_NO_FOLD, &L);
  if (rc) return rc;
  if (planes_bytes < L.total - L.off[STEIN_WS_PLANES])
    return fail(STEIN_E_WORKSPACE, "planes buffer %zu < %zu bytes", planes_bytes, L.total - L.off[STEIN_WS_PLANES]);
  return stein_x3_split(theta_all, score_all, dtype, n, d, L, (char*)x3_planes, (hipStream_t)stream);
}

extern "C" int stein_rownorms(const void* theta_all, int64_t n, int64_t d, int dtype, float* r_out, void* stream) {
  if (!theta_all || !r_out) return fail(STEIN_E_BADARG, "NULL pointer");
  if (n < 1 || d < 1) return fail(STEIN_E_SHAPE, "bad shape");
  if (dtype != STEIN_F32 && dtype != STEIN_BF16) return fail(STEIN_E_UNSUPPORTED, "rownorms: dtype %d", dtype);
  const int blocks = (int)((n + 3) / 4);
  if (dtype == STEIN_BF16)
    hipLaunchKernelGGL(k_rownorms<unsigned short>, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned short*)theta_all, (int)n, (int)d, r_out);
  else
    hipLaunchKernelGGL(k_rownorms<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const float*)theta_all,
                       (int)n, (int)d, r_out);
  LAUNCH_CHECK("k_rownorms");
  return STEIN_OK;
}

// spec != NULL (single-rank fused call only, needs hist_level0): also feed the speculative median window
static int distance_block_impl(const void* theta_all, const float* r_all, int64_t n, int64_t d, int64_t row0,
                               int64_t n_local, int dtype, float* dist_out, int64_t ld_dist, void* hist_level0,
                               const void* x3_planes, int flags, void* stream, SpecState* spec, u64* spec_buf) {
  if ((!theta_all && !x3_planes) || !r_all || !dist_out) return fail(STEIN_E_BADARG, "NULL pointer");
  if (n < 1 || d < 1 || n_local < 1 || row0 < 0 || row0 + n_local > n) return fail(STEIN_E_SHAPE, "bad row block");
  if (ld_dist < n || (ld_dist & 63)) return fail(STEIN_E_SHAPE, "ld_dist must be >= n and a multiple of 64");
  if (dtype != STEIN_F32 && !(dtype == STEIN_BF16 && x3_planes))
    return fail(STEIN_E_UNSUPPORTED, "distance: dtype %d (bf16 inputs need the operand planes)", dtype);
  const bool sym = (flags & STEIN_STAGE_SYMMETRIC) != 0;
  if (sym && (row0 != 0 || n_local != n || (ld_dist & 63)))
    return fail(STEIN_E_BADARG, "STEIN_STAGE_SYMMETRIC needs the whole matrix (row0 = 0, n_local = n) and ld_dist %% 64 == 0");
  const int tiles_m = (int)((n_local + BM - 1) / BM), tiles_n = (int)((n + BN - 1) / BN);
  const long nblk = distance_grid(sym, tiles_m, tiles_n);
  if (nblk > 0x7fffffffl) return fail(STEIN_E_SHAPE, "too many tiles");
  hipStream_t s = (hipStream_t)stream;
  u64* h0 = (u64*)hist_level0;
  if (x3_planes) {
    SteinLayout L;
    int rc = stein_make_layout(n_local, n, d, dtype, STEIN_FLAG_X3 | STEIN_FLAG_NO_FOLD, &L);
    if (rc) return rc;
    return stein_x3_distance((const char*)x3_planes, L, dtype, r_all, dist_out, n, d, row0, n_local, ld_dist, h0, sym, s,
                             spec, spec_buf, (flags & STEIN_STAGE_TILES) ? -1 : ((flags & STEIN_STAGE_PANEL) ? 1 : 0));
  }
  return stein_fp32_distance((const float*)theta_all, r_all, dist_out, n, d, row0, n_local, ld_dist, h0, sym, s, spec, spec_buf);
}

extern "C" int stein_distance_block(const void* theta_all, const float* r_all, int64_t n, int64_t d, int64_t row0,
                                    int64_t n_local, int dtype, float* dist_out, int64_t ld_dist, void* hist_level0,
                                    const void* x3_planes, int flags, void* stream) {
  return distance_block_impl(theta_all, r_all, n, d, row0, n_local, dtype, dist_out, ld_dist, hist_level0, x3_planes,
                             flags, stream, nullptr, nullptr);
}

extern "C" int stein_distance_block_spec(const void* theta_all, const float* r_all, int64_t n, int64_t d, int64_t row0,
                                         int64_t n_local, int dtype, float* dist_out, int64_t ld_dist, void* hist_level0,
                                         const void* x3_planes, int flags, void* select_state, void* spec_buf,
                                         void* stream) {
  if (!hist_level0 || !select_state || !spec_buf) return fail(STEIN_E_BADARG, "NULL pointer");
  return distance_block_impl(theta_all, r_all, n, d, row0, n_local, dtype, dist_out, ld_dist, hist_level0, x3_planes,
                             flags, stream, spec_of(select_state), (u64*)spec_buf);
}

extern "C" int stein_kernel_matrix(const float* dist, int64_t ld_dist, int64_t n_local, int64_t n,
                                   const float* h2_dev, float* K_out, int64_t ld_K, int dist_flags, void* stream) {
  if (!dist || !h2_dev || !K_out) return fail(STEIN_E_BADARG, "NULL pointer");
  if (ld_dist < n || ld_K < n || n_local < 1) return fail(STEIN_E_SHAPE, "bad shape");
  if (dist_flags & ~(STEIN_STAGE_SYMMETRIC | STEIN_STAGE_UPPER)) return fail(STEIN_E_BADARG, "unknown distance flags 0x%x", dist_flags);
  if ((dist_flags & STEIN_STAGE_UPPER) && n_local != n) return fail(STEIN_E_BADARG, "STEIN_STAGE_UPPER needs the whole matrix");
  hipLaunchKernelGGL(k_kernel_matrix, dim3(grid_for((long)n_local * n, 4096)), dim3(256), 0, (hipStream_t)stream,
                     dist, (long)ld_dist, (int)n_local, (int)n, h2_dev, K_out, (long)ld_K,
                     (dist_flags & STEIN_STAGE_UPPER) ? 1 : 0);
  LAUNCH_CHECK("k_kernel_matrix");
  return STEIN_OK;
}

extern "C" int stein_contract_partial(const float* dist, int64_t ld_dist, const void* theta_all,
                                      const void* score_all, int64_t n, int64_t d, int64_t row0, int64_t n_local,
                                      int dtype, const float* h2_dev, const void* x3_planes, void* workspace,
                                      size_t ws_bytes, int dist_flags, void* stream) {
  if (dist_flags & ~(STEIN_STAGE_SYMMETRIC | STEIN_STAGE_UPPER)) return fail(STEIN_E_BADARG, "unknown distance flags 0x%x", dist_flags);
  const bool upper = (dist_flags & STEIN_STAGE_UPPER) != 0;
  if (upper && (!x3_planes || row0 != 0 || n_local != n))
    return fail(STEIN_E_BADARG, "STEIN_STAGE_UPPER: only the split path's symmetric distance pass stores the upper triangle alone");
  if (!dist || (!x3_planes && (!theta_all || !score_all)) || !h2_dev || !workspace)
    return fail(STEIN_E_BADARG, "NULL pointer");
  if (dtype != STEIN_F32 && !(dtype == STEIN_BF16 && x3_planes))
    return fail(STEIN_E_UNSUPPORTED, "contract: dtype %d (bf16 inputs need the operand planes)", dtype);
  if (row0 < 0 || row0 + n_local > n) return fail(STEIN_E_SHAPE, "bad row block");
  SteinLayout L;
  int rc = stein_make_layout(n_local, n, d, dtype, x3_planes ? STEIN_FLAG_X3 | STEIN_FLAG_NO_FOLD : 0, &L);
  if (rc) return rc;
  if (ws_bytes < L.off[STEIN_WS_PLANES]) return fail(STEIN_E_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, L.off[STEIN_WS_PLANES]);
  if (ld_dist != L.ld_dist) return fail(STEIN_E_SHAPE, "ld_dist %lld != %lld", (long long)ld_dist, (long long)L.ld_dist);
  const StepViews v = stein_step_views(L, workspace);
  hipStream_t s = (hipStream_t)stream;
  const long nblk = (long)L.tiles_m * 2 * L.cblocks * L.split;
  if (nblk > 0x7fffffffl) return fail(STEIN_E_SHAPE, "too many tiles");
  return x3_planes ? stein_x3_contract_partial(dist, ld_dist, (const char*)x3_planes, L, dtype, h2_dev, v.OG, v.OT, v.RS, n, d,
                                               n_local, s, upper)
                   : stein_fp32_contract_partial(dist, ld_dist, (const float*)theta_all, (const float*)score_all, L, h2_dev,
                                                 v.OG, v.OT, v.RS, n, d, n_local, s);
}

// score_all: read only with STEIN_FLAG_KSD in flags (the statistic's score rows; sqnorm_out is then double[3])
static int contract_finish_impl(const void* theta_all, const void* score_all, int64_t n, int64_t d, int64_t row0,
                                int64_t n_local, int dtype, const float* h2_dev, float* phi_local, double* sqnorm_out,
                                float* dK_out, void* workspace, size_t ws_bytes, int flags, void* stream, HistSync* fuse_done) {
  const bool ksd = (flags & STEIN_FLAG_KSD) != 0;
  if (!theta_all || !h2_dev || !phi_local || !sqnorm_out || !workspace || (ksd && !score_all)) return fail(STEIN_E_BADARG, "NULL pointer");
  if (dtype != STEIN_F32 && dtype != STEIN_BF16) return fail(STEIN_E_UNSUPPORTED, "contract: dtype %d", dtype);
  if (row0 < 0 || row0 + n_local > n) return fail(STEIN_E_SHAPE, "bad row block");
  SteinLayout L;
  int rc = stein_make_layout(n_local, n, d, dtype, flags, &L);
  if (rc) return rc;
  if (ws_bytes < L.off[STEIN_WS_PLANES]) return fail(STEIN_E_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, L.off[STEIN_WS_PLANES]);
  StepViews v = stein_step_views(L, workspace);
  if (L.fold) {   // (fused call only: the staged entry points ask for STEIN_FLAG_NO_FOLD) the folded contraction's partials
    if (ws_bytes < L.total) return fail(STEIN_E_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, L.total);
    v.OG = (float*)((char*)workspace + L.fold_ow);
    v.OT = (float*)((char*)workspace + L.fold_ot);
    v.RS = (float*)((char*)workspace + L.fold_rs);
  }
  const int nsplit = (int)(L.fold ? L.fsplit : L.split);
  hipStream_t s = (hipStream_t)stream;
  auto al16 = [](const void* p) { return ((uintptr_t)p & 15u) == 0; };
  const size_t tsz = dtype == STEIN_BF16 ? 2 : 4;
  auto rows_aligned = [&](const void* p) { return (((uintptr_t)p + (size_t)row0 * d * tsz) & (4 * tsz - 1)) == 0; };
  const int vec = (d % 4 == 0) && al16(v.OG) && al16(v.OT) && al16(phi_local) && al16(dK_out) && rows_aligned(theta_all) &&
                  (!ksd || rows_aligned(score_all));
  auto launch = [&](auto tin, auto ksd_tag, auto fold_tag) {
    using TIN = decltype(tin);
    hipLaunchKernelGGL((k_phi_finish<TIN, decltype(ksd_tag)::value, decltype(fold_tag)::value>), dim3((unsigned)L.sq_blocks),
                       dim3(256), 0, s, v.OG, v.OT, v.RS, (const TIN*)theta_all, h2_dev, phi_local, dK_out, v.SQ, (int)n, (int)d,
                       (int)row0, (int)n_local, nsplit, L.fold ? 1 : nsplit, vec, fuse_done, sqnorm_out, (const TIN*)score_all);
  };
  if (L.fold) {   // fp32 inputs by construction
    if (ksd) launch(0.f, std::true_type(), std::true_type());
    else launch(0.f, std::false_type(), std::true_type());
  } else if (dtype == STEIN_BF16) {
    if (ksd) launch((unsigned short)0, std::true_type(), std::false_type());
    else launch((unsigned short)0, std::false_type(), std::false_type());
  } else {
    if (ksd) launch(0.f, std::true_type(), std::false_type());
    else launch(0.f, std::false_type(), std::false_type());
  }
  LAUNCH_CHECK("k_phi_finish");
  return fuse_done ? STEIN_OK : sum_partials(v.SQ, (int)L.sq_blocks, ksd, sqnorm_out, s);
}

extern "C" int stein_contract_finish(const void* theta_all, int64_t n, int64_t d, int64_t row0, int64_t n_local,
                                     int dtype, const float* h2_dev, float* phi_local, double* sqnorm_out,
                                     float* dK_out, void* workspace, size_t ws_bytes, int flags, void* stream) {
  if (flags & STEIN_FLAG_KSD)
    return fail(STEIN_E_BADARG, "STEIN_FLAG_KSD: stein_contract_finish has no score operand; the statistic comes from "
                                "stein_svgd_phi, stein_rank_finish or stein_rank_step");
  // (a staged call finishes what stein_contract_partial left: K.[G | theta], never the folded form)
  return contract_finish_impl(theta_all, nullptr, n, d, row0, n_local, dtype, h2_dev, phi_local, sqnorm_out, dK_out,
                              workspace, ws_bytes, (flags & ~STEIN_FLAG_FOLD) | STEIN_FLAG_NO_FOLD, stream, nullptr);
}

extern "C" int stein_kernel_contract(const float* dist, int64_t ld_dist, const void* theta_all, const void* score_all,
                                     int64_t n, int64_t d, int64_t row0, int64_t n_local, int dtype,
                                     const float* h2_dev, float* phi_local, double* sqnorm_out, float* dK_out,
                                     const void* x3_planes, void* workspace, size_t ws_bytes, int dist_flags,
                                     void* stream) {
  if (dist_flags & STEIN_FLAG_KSD)
    return fail(STEIN_E_BADARG, "STEIN_FLAG_KSD: stein_kernel_contract takes distance flags only; the statistic comes from "
                                "stein_svgd_phi, stein_rank_finish or stein_rank_step");
  int rc = stein_contract_partial(dist, ld_dist, theta_all, score_all, n, d, row0, n_local, dtype, h2_dev, x3_planes,
                                  workspace, ws_bytes, dist_flags, stream);
  if (rc) return rc;
  return stein_contract_finish(theta_all, n, d, row0, n_local, dtype, h2_dev, phi_local, sqnorm_out, dK_out, workspace,
                               ws_bytes, x3_planes ? STEIN_FLAG_X3 : 0, stream);
}

// ------------------------------------------------------------------------------------------------
// rank-step segments: what one rank of a row-sharded run does between two collectives, as ONE call each (the staged calls
// above, chained on the stream).  The host layer issues: all-gather(theta), all-gather(score) | stein_rank_begin |
// all-reduce(window table or level-0 histogram) | stein_rank_pick or stein_rank_radix x3 (an all-reduce before each) |
// stein_rank_finish | all-reduce(|phi|^2).
// ------------------------------------------------------------------------------------------------
static thread_local std::vector<hipEvent_t> g_tevents;   // (STEIN_T_NSTAGES + 1) events per reserved call
static thread_local int g_tcalls_reserved = 0, g_tcalls_used = 0;
static thread_local std::vector<unsigned char> g_tmode;   // per reserved call: 1 = only the contraction was bracketed

// STEIN_FLAG_TIMING: a call claims the next reserved slot while they last, and mark(k) records stage boundary k on the
// stream.  STEIN_FLAG_TIMING_CONTRACT (mode 1): only the two events around the contraction -- an event between two
// kernels costs the step ~3 us of GPU time, scratch/event_cost.py: six of them are 2 % of a C3 step and a quarter of a
// C2 step.
struct StageTimer {
  hipEvent_t* ev = nullptr;   // this call's slot; NULL: not timed
  bool contract_only = false;
  explicit StageTimer(int flags) {
    if (!(flags & STEIN_FLAG_TIMING) || g_tcalls_used >= g_tcalls_reserved) return;
    contract_only = (flags & STEIN_FLAG_TIMING_CONTRACT) != 0;
    g_tmode[(size_t)g_tcalls_used] = contract_only ? 1 : 0;
    ev = &g_tevents[(size_t)(g_tcalls_used++) * (STEIN_T_NSTAGES + 1)];
  }
  int mark(int k, hipStream_t s) const {
    if (ev && (!contract_only || k == STEIN_T_CONTRACT || k == STEIN_T_FINISH)) HIP_TRY(hipEventRecord(ev[k], s));
    return STEIN_OK;
  }
};

static int rank_views(int64_t n, int64_t d, int64_t row0, int64_t n_local, int dtype, void* workspace, size_t ws_bytes,
                      int flags, StepViews* v) {
  if (!workspace) return fail(STEIN_E_BADARG, "NULL pointer");
  if (row0 < 0 || n_local < 1 || row0 + n_local > n) return fail(STEIN_E_SHAPE, "bad row block");
  if (flags & ~(STEIN_FLAG_X3 | STEIN_FLAG_TILED | STEIN_FLAG_RANK_WINDOW | STEIN_FLAG_TIMING | STEIN_FLAG_KSD)) return fail(STEIN_E_BADARG, "unknown flags 0x%x", flags);
  SteinLayout L;
  // (the rank segments keep K.[G | theta]: the score's planes are built while its all-gather overlaps the distance pass,
  // before h2 exists.  The workspace may have been sized with the fold area -- it only adds bytes at the end.)
  int rc = stein_make_layout(n_local, n, d, dtype, (flags & (STEIN_FLAG_X3 | STEIN_FLAG_TILED | STEIN_FLAG_KSD)) | STEIN_FLAG_TILED | STEIN_FLAG_NO_FOLD, &L);
  if (rc) return rc;
  if (dtype == STEIN_BF16 && !(flags & STEIN_FLAG_X3)) return fail(STEIN_E_UNSUPPORTED, "bf16 inputs need STEIN_FLAG_X3");
  if (ws_bytes < L.total) return fail(STEIN_E_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, L.total);
  *v = stein_step_views(L, workspace);
  return STEIN_OK;
}

extern "C" int stein_rank_begin(const void* theta_all, int64_t n, int64_t d, int64_t row0, int64_t n_local, int dtype,
                                void* workspace, size_t ws_bytes, int flags, void* stream) {
  if (!theta_all) return fail(STEIN_E_BADARG, "NULL pointer");
  StepViews v;
  int rc = rank_views(n, d, row0, n_local, dtype, workspace, ws_bytes, flags, &v);
  if (rc) return rc;
  const bool window = (flags & STEIN_FLAG_RANK_WINDOW) != 0;
  if ((rc = stein_rownorms(theta_all, n, d, dtype, v.r, stream))) return rc;
  if (v.planes && (rc = stein_x3_split(theta_all, nullptr, dtype, n, d, v.L, v.planes, (hipStream_t)stream))) return rc;
  if (window) rc = stein_spec_begin(v.hist, v.sel, v.spec_buf, n * n, stream);
  else rc = stein_median_begin(v.hist, v.sel, n * n, stream);
  if (rc) return rc;
  if ((rc = distance_block_impl(theta_all, v.r, n, d, row0, n_local, dtype, v.D, v.L.ld_dist, v.hist, v.planes, 0, stream,
                                window ? v.spec : nullptr, window ? v.spec_buf : nullptr)))
    return rc;
  if (window) rc = stein_spec_tally(v.sel, v.spec_buf, stream);
  return rc;
}

extern "C" int stein_rank_pick(int64_t n, int64_t d, int64_t row0, int64_t n_local, int dtype, void* workspace,
                               size_t ws_bytes, int flags, float* h2_out, float* median_out, void* flags_host,
                               void* stream) {
  if (!h2_out || !flags_host) return fail(STEIN_E_BADARG, "NULL pointer");
  StepViews v;
  int rc = rank_views(n, d, row0, n_local, dtype, workspace, ws_bytes, flags, &v);
  if (rc) return rc;
  if ((rc = stein_spec_pick(v.sel, v.spec_buf, n, h2_out, median_out, stream))) return rc;
  // `hit` (SpecState + 28) .. `skip_l0` (+ 52): 28 bytes, to page-locked host memory the caller polls behind an event
  HIP_TRY(hipMemcpyAsync(flags_host, &v.spec->hit, 28, hipMemcpyDeviceToHost, (hipStream_t)stream));
  return STEIN_OK;
}

extern "C" int stein_rank_radix(int level, int need_pass, int64_t n, int64_t d, int64_t row0, int64_t n_local, int dtype,
                                void* workspace, size_t ws_bytes, int flags, float* h2_out, float* median_out,
                                void* stream) {
  // need_pass: first take this level's histogram of the local block (level 0 after a window miss that skipped it);
  // then (the caller has summed hist[level] over the ranks unless need_pass) ... see include/steinhip.h
  StepViews v;
  int rc = rank_views(n, d, row0, n_local, dtype, workspace, ws_bytes, flags, &v);
  if (rc) return rc;
  if (level < 0 || level >= STEIN_HIST_LEVELS) return fail(STEIN_E_BADARG, "level %d", level);
  if (need_pass) return stein_median_hist_pass(v.D, v.L.ld_dist, n_local, n, level, v.sel, v.hist, 0, stream);
  if ((rc = stein_median_resolve(v.hist, level, n, v.sel, h2_out, median_out, stream))) return rc;
  if (level + 1 < STEIN_HIST_LEVELS)
    rc = stein_median_hist_pass(v.D, v.L.ld_dist, n_local, n, level + 1, v.sel, v.hist, 0, stream);
  return rc;
}

extern "C" int stein_rank_finish(const void* theta_all, const void* score_all, int64_t n, int64_t d, int64_t row0,
                                 int64_t n_local, int dtype, const float* h2_dev, float* phi_local, double* sqnorm_out,
                                 float* dK_out, void* workspace, size_t ws_bytes, int flags, void* stream) {
  if (!theta_all || !score_all || !h2_dev || !phi_local || !sqnorm_out) return fail(STEIN_E_BADARG, "NULL pointer");
  StepViews v;
  int rc = rank_views(n, d, row0, n_local, dtype, workspace, ws_bytes, flags, &v);
  if (rc) return rc;
  if ((flags & STEIN_FLAG_RANK_WINDOW) && (rc = stein_spec_update(v.sel, stream))) return rc;
  // STEIN_FLAG_TIMING: the contraction and the finish pass are bracketed by HIP events on the stream (the earlier
  // stages of the slot read as zero length); read them back with stein_timing_read
  const hipStream_t s = (hipStream_t)stream;
  const StageTimer clk(flags);
  for (int k = 0; k <= STEIN_T_CONTRACT; ++k)
    if ((rc = clk.mark(k, s))) return rc;
  if ((rc = stein_contract_partial(v.D, v.L.ld_dist, theta_all, score_all, n, d, row0, n_local, dtype, h2_dev, v.planes,
                                   workspace, ws_bytes, 0, stream)))
    return rc;
  if ((rc = clk.mark(STEIN_T_FINISH, s))) return rc;
  rc = contract_finish_impl(theta_all, score_all, n, d, row0, n_local, dtype, h2_dev, phi_local, sqnorm_out, dK_out,
                            workspace, ws_bytes, (v.planes ? STEIN_FLAG_X3 : 0) | (flags & STEIN_FLAG_KSD) | STEIN_FLAG_NO_FOLD,
                            stream, nullptr);
  return rc ? rc : clk.mark(STEIN_T_NSTAGES, s);
}

// ------------------------------------------------------------------------------------------------
// device error word: one u32 per device in page-locked host memory that a kernel raises when it had to give up (today
// only k_hist_all's bounded wait).  The host reads it without touching the stream at the start of the next fused call or
// optimizer apply on that device and turns it into STEIN_E_HIP; the step that raised it has already written NaN into its
// bandwidth, so nothing wrong was consumed silently in between.
// ------------------------------------------------------------------------------------------------
static u32* g_errword[MAX_DEVICES];
int stein_device_error_word(u32** out) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= MAX_DEVICES) { *out = nullptr; return STEIN_OK; }
  u32* w = __atomic_load_n(&g_errword[dev], __ATOMIC_ACQUIRE);
  if (!w) {
    void* p = nullptr;
    HIP_TRY(hipHostMalloc(&p, 64, hipHostMallocMapped | hipHostMallocPortable));
    *(volatile u32*)p = 0u;
    u32* expect = nullptr;
    if (!__atomic_compare_exchange_n(&g_errword[dev], &expect, (u32*)p, false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE)) {
      (void)hipHostFree(p);   // another thread was first
      w = expect;
    } else {
      w = (u32*)p;
    }
  }
  *out = w;
  return STEIN_OK;
}
// STEIN_E_HIP if a kernel of an EARLIER call on the current device raised the error word (and lowers it again)
int stein_take_device_error(void) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEVICES) return STEIN_OK;
  u32* w = __atomic_load_n(&g_errword[dev], __ATOMIC_ACQUIRE);
  if (!w || !*(volatile u32*)w) return STEIN_OK;
  *(volatile u32*)w = 0u;
  return fail(STEIN_E_HIP, "an earlier step on device %d gave up inside k_hist_all (bounded wait exhausted): its bandwidth and "
                           "everything computed from it are NaN", dev);
}
extern "C" int stein_debug_raise_device_error(void) {
  u32* w = nullptr;
  int rc = stein_device_error_word(&w);
  if (rc) return rc;
  if (w) *(volatile u32*)w = 1u;
  return STEIN_OK;
}

// ------------------------------------------------------------------------------------------------
// stage timing of the fused call (profiling aid; per calling thread, like the last-error string)
// ------------------------------------------------------------------------------------------------

extern "C" int stein_timing_reserve(int calls) {
  if (calls < 0) return fail(STEIN_E_BADARG, "calls < 0");
  const size_t need = (size_t)calls * (STEIN_T_NSTAGES + 1);
  while (g_tevents.size() < need) {
    hipEvent_t e;
    HIP_TRY(hipEventCreate(&e));
    g_tevents.push_back(e);
  }
  g_tmode.assign((size_t)calls, 0);
  g_tcalls_reserved = calls;
  g_tcalls_used = 0;
  return STEIN_OK;
}

extern "C" int stein_timing_read(float* ms_out, int max_calls, int* calls_out) {
  if (!ms_out || !calls_out) return fail(STEIN_E_BADARG, "NULL pointer");
  const int calls = g_tcalls_used < max_calls ? g_tcalls_used : max_calls;
  for (int c = 0; c < calls; ++c) {
    hipEvent_t* ev = &g_tevents[(size_t)c * (STEIN_T_NSTAGES + 1)];
    if (g_tmode[(size_t)c]) {   // STEIN_FLAG_TIMING_CONTRACT: the other stages were not bracketed
      HIP_TRY(hipEventSynchronize(ev[STEIN_T_FINISH]));
      for (int k = 0; k < STEIN_T_NSTAGES; ++k) ms_out[c * STEIN_T_NSTAGES + k] = -1.f;
      HIP_TRY(hipEventElapsedTime(&ms_out[c * STEIN_T_NSTAGES + STEIN_T_CONTRACT], ev[STEIN_T_CONTRACT], ev[STEIN_T_FINISH]));
      continue;
    }
    HIP_TRY(hipEventSynchronize(ev[STEIN_T_NSTAGES]));
    for (int k = 0; k < STEIN_T_NSTAGES; ++k) HIP_TRY(hipEventElapsedTime(&ms_out[c * STEIN_T_NSTAGES + k], ev[k], ev[k + 1]));
  }
  *calls_out = calls;
  return STEIN_OK;
}

// The fused call's first launch: the row norms and all set-up (PrologueArgs, stein_common.h), and -- split path -- the
// operand planes.  bf16 inputs need no scales, so the split does not depend on the prologue: both ride in ONE launch
// (k_split's grid gets a third slice that does the prologue's work) -- one launch less on the latency-bound sizes this
// dtype is for.
static int fused_prologue(const StepViews& v, const void* theta_all, const void* score_all, int64_t n, int64_t d, int dtype,
                          int flags, hipStream_t s, int fold) {
  const SteinLayout& L = v.L;
  PrologueArgs pa;
  pa.n = (int)n; pa.d = (int)d; pa.r = v.r; pa.st = v.sel; pa.sp = v.spec; pa.fs = v.fuse; pa.total = (u64)(n * n);
  pa.hist = v.hist; pa.slots = v.spec_buf;
  pa.cmax = v.planes ? (u32*)((float*)(v.planes + L.x3_sc) + 4 * L.x3_dc + 4) : nullptr;   // the column maxima behind the
  pa.ncmax = v.planes ? (int)(2 * L.x3_dc) : 0;                                              // scales (stein_x3.hip)
  pa.allow_window = (flags & STEIN_FLAG_NO_WINDOW) ? 0 : 1;
  pa.hsync = (u32*)v.table; pa.hsync_words = (int)(sizeof(HistSync) / 4);
  pa.neutral_sc = (dtype == STEIN_BF16 && v.planes) ? (float*)(v.planes + L.x3_sc) : (float*)nullptr;
  pa.dc = (int)L.x3_dc;
  pa.folded = fold ? 1u : 0u;
  if (dtype == STEIN_BF16 && v.planes)
    return stein_x3_split(theta_all, score_all, dtype, n, d, L, v.planes, s, (HistSync*)v.table, true, &pa);
  const dim3 grid((unsigned)((n + 3) / 4 + PRO_INIT_BLOCKS));
  if (dtype == STEIN_BF16)
    hipLaunchKernelGGL(k_prologue<unsigned short>, grid, dim3(256), 0, s, (const unsigned short*)theta_all, pa);
  else
    hipLaunchKernelGGL(k_prologue<float>, grid, dim3(256), 0, s, (const float*)theta_all, pa);
  LAUNCH_CHECK("k_prologue");
  return v.planes ? stein_x3_split(theta_all, score_all, dtype, n, d, L, v.planes, s, (HistSync*)v.table, false, nullptr, fold)
                  : STEIN_OK;
}

extern "C" int stein_svgd_phi(const void* theta_all, const void* score_all, int64_t n, int64_t d, int64_t row0,
                              int64_t n_local, int dtype, float* phi_local, float* h2_out, double* sqnorm_out,
                              float* K_out, float* dK_out, void* workspace, size_t ws_bytes, int flags, void* stream) {
  if (!theta_all || !score_all || !phi_local || !h2_out || !sqnorm_out || !workspace)
    return fail(STEIN_E_BADARG, "NULL pointer");
  if (row0 != 0 || n_local != n)
    return fail(STEIN_E_BADARG, "stein_svgd_phi is the single-rank path (row0 = 0, n_local = n); use the staged calls");
  SteinLayout L;
  int rc = stein_make_layout(n_local, n, d, dtype, flags, &L);
  if (rc) return rc;
  if ((rc = stein_take_device_error())) return rc;   // a kernel of an earlier call on this device gave up: say so now
  if (dtype == STEIN_BF16 && !(flags & STEIN_FLAG_X3))
    return fail(STEIN_E_UNSUPPORTED, "bf16 inputs run on the bf16-MFMA kernels: pass STEIN_FLAG_X3");
  if (ws_bytes < L.total) return fail(STEIN_E_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, L.total);
  const StepViews v = stein_step_views(L, workspace);
  hipStream_t s = (hipStream_t)stream;
  const StageTimer clk(flags);   // STEIN_FLAG_TIMING: one event per stage boundary
  if ((rc = clk.mark(STEIN_T_PREPARE, s))) return rc;
  if (!(flags & STEIN_FLAG_TILED) && stein_small_ok(n, d, dtype)) {   // the reference's own example sizes: one kernel does it all (stein_small.hip)
    for (int k = STEIN_T_DISTANCE; k <= STEIN_T_CONTRACT; ++k)
      if ((rc = clk.mark(k, s))) return rc;
    int nparts = 0;
    const bool ksd = (flags & STEIN_FLAG_KSD) != 0;
    if ((rc = stein_small_phi((const float*)theta_all, (const float*)score_all, n, d, phi_local, h2_out, v.SQ, K_out,
                              dK_out, &nparts, sqnorm_out, ksd, s)))
      return rc;
    if ((rc = clk.mark(STEIN_T_FINISH, s))) return rc;
    if (nparts && (rc = sum_partials(v.SQ, nparts, ksd, sqnorm_out, s))) return rc;   // d > 32: several workgroups' partials
    return clk.mark(STEIN_T_NSTAGES, s);
  }
  // The prologue carries the row norms and all set-up; kernels let their last workgroup do what a one-workgroup follow-up
  // launch would (scales, |phi|^2 sum); the chained radix select is ONE launch (k_hist_all) and none
  // for n <= SOLO_MAX_N (k_spec_select covers it); bf16 inputs need no scales, so their prologue rides in the split's
  // launch.  fp32 inputs: k_prologue, k_colmax, k_split, distance, k_spec_select, k_hist_all, contraction, k_phi_finish:
  // eight launches whatever n (the last workgroups of k_colmax and k_phi_finish are found with two-level completion counts,
  // HistSync, so no grid is too large for them); bf16 inputs: six.
  // folded operand (L.fold: split path, fp32 inputs, where it pays or is forced): the contraction multiplies K with
  // W = G - theta / h2 alone; with dK_out or the Stein discrepancy, with [W | theta] -- phi comes from the W half either way
  const bool fold_theta = L.fold && (dK_out || (flags & STEIN_FLAG_KSD));
  if ((rc = fused_prologue(v, theta_all, score_all, n, d, dtype, flags, s, L.fold ? (fold_theta ? 2 : 1) : 0))) return rc;
  if ((rc = clk.mark(STEIN_T_DISTANCE, s))) return rc;
  // single rank: the block is the whole symmetric matrix -> upper-triangle distance pass with mirrored stores,
  // level-0 histogram taken in its epilogue, levels 1-2 read the upper triangle only
  const int sf = STEIN_STAGE_SYMMETRIC | ((flags & STEIN_FLAG_TILE_DISTANCE) ? STEIN_STAGE_TILES : 0);
  if ((rc = distance_block_impl(theta_all, v.r, n, d, row0, n_local, dtype, v.D, L.ld_dist, v.hist, v.planes, sf, stream,
                                v.spec, v.spec_buf)))
    return rc;
  if ((rc = clk.mark(STEIN_T_MEDIAN, s))) return rc;
  if ((rc = stein_fused_select(v, n, h2_out, s))) return rc;
  // the split path's symmetric distance pass stores only the tiles on and above the diagonal
  const int df = v.planes ? (STEIN_STAGE_SYMMETRIC | STEIN_STAGE_UPPER) : STEIN_STAGE_SYMMETRIC;
  if (K_out && (rc = stein_kernel_matrix(v.D, L.ld_dist, n_local, n, h2_out, K_out, n, df, stream))) return rc;
  if (L.fold && (rc = stein_x3_split_w((const float*)theta_all, (const float*)score_all, n, d, L, v.planes, h2_out, s))) return rc;
  if ((rc = clk.mark(STEIN_T_CONTRACT, s))) return rc;
  if (L.fold) rc = stein_x3_contract_fold(v.D, L.ld_dist, (char*)workspace, L, h2_out, n, d, fold_theta, s);
  else rc = stein_contract_partial(v.D, L.ld_dist, theta_all, score_all, n, d, row0, n_local, dtype, h2_out, v.planes,
                                   workspace, ws_bytes, df, stream);
  if (rc) return rc;
  if ((rc = clk.mark(STEIN_T_FINISH, s))) return rc;
  const int keep = STEIN_FLAG_KSD | STEIN_FLAG_TILED | STEIN_FLAG_FOLD | STEIN_FLAG_NO_FOLD;   // what the layout depends on
  if ((rc = contract_finish_impl(theta_all, score_all, n, d, row0, n_local, dtype, h2_out, phi_local, sqnorm_out, dK_out,
                                 workspace, ws_bytes, (v.planes ? STEIN_FLAG_X3 : 0) | (flags & keep), stream,
                                 (HistSync*)v.table)))
    return rc;
  return clk.mark(STEIN_T_NSTAGES, s);
}

