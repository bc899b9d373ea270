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
// This file holds the workspace layout and its views, the fused single-rank call, the staged distance / contraction entry
// points, the rank-step segments, the stage timing and the device error word.
// Every extern "C" entry point validates its arguments, derives ONE layout (stein_make_layout, with the flags of its family:
// stein_host.h), builds the call's views from it (stein_step_views) and runs stage functions on them; a stage function or a
// launcher never derives a layout, never forms an address from an offset, and checks the grid it computes.
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
  if (vec == 1) {   // host: d % 4 == 0 and every pointer aligned for four columns at a time
    // four consecutive columns of one row per step, 16-byte loads and stores (one entry at a time with an integer
    // division each, the kernel moved its 68 MB at 2.8 TB/s; bf16 inputs took that path until round 4: 19 us at C2)
    // NZ j ranges of OG and RS and NT of OT known at compile time (NZ = 1, 2, 4, NT = NZ or, folded, 0 or 1; NZ = 0: any
    // numbers, the loop): every load of an element group -- the ranges' OG / OT / RS and theta -- is issued before the first add.  (With the runtime count the unrolled loop was a chain of
    // branches with one 16-byte load between each pair: one or two loads in flight per thread, 67 MB at 3.7 TB/s.)  The
    // sums run in the same order on every form: 0 + a0 + a1 ...
    const long total4 = total >> 2;
    const int d4 = d >> 2;
    auto run = [&](auto nz, auto nt) {
      constexpr int NZ = decltype(nz)::value, NT = decltype(nt)::value;
      for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < total4; q += (long)gridDim.x * 256) {
        const int i = (int)(q / d4);
        const long e = q << 2;
        float4 og = make_float4(0.f, 0.f, 0.f, 0.f), ot = og;
        float rs = 0.f;
        float4 th;
        if constexpr (NZ > 0) {
          float4 a[NZ], b[NT > 0 ? NT : 1];
          float r[NZ];
#pragma unroll
          for (int z = 0; z < NZ; ++z) {
            a[z] = *reinterpret_cast<const float4*>(OG + z * zs + e);
            r[z] = RS[(size_t)z * n_local + i];
          }
          th = theta4(T + (size_t)row0 * d + e);
#pragma unroll
          for (int z = 0; z < NT; ++z) b[z] = *reinterpret_cast<const float4*>(OT + z * zs + e);
#pragma unroll
          for (int z = 0; z < NZ; ++z) {
            og.x += a[z].x; og.y += a[z].y; og.z += a[z].z; og.w += a[z].w;
            if (z < NT) { ot.x += b[z].x; ot.y += b[z].y; ot.z += b[z].z; ot.w += b[z].w; }
            rs += r[z];
          }
        } else {
#pragma unroll 8
          for (int z = 0; z < split; ++z) {   // unrolled: the loads of eight slices in flight, the sums in the same order
            const float4 a = *reinterpret_cast<const float4*>(OG + z * zs + e);
            og.x += a.x; og.y += a.y; og.z += a.z; og.w += a.w;
            if (FOLD ? need_t && z < tsplit : true) {
              const float4 b = *reinterpret_cast<const float4*>(OT + z * zs + e);
              ot.x += b.x; ot.y += b.y; ot.z += b.z; ot.w += b.w;
            }
            rs += RS[(size_t)z * n_local + i];
          }
          th = theta4(T + (size_t)row0 * d + e);
        }
        // rowsum * theta - K.theta, written out the way the single-loop kernel was compiled (folded: the rounded product,
        // which phi shares, then the difference; unfolded: one fma), so that dK does not move with the compiler's choice
        // of contraction in each specialised loop
        auto rt_minus = [&](float t, float o) {
          if constexpr (FOLD) {
#pragma clang fp contract(off)
            const float m = rs * t;
            return m - o;
          } else {
            return __builtin_fmaf(rs, t, -o);
          }
        };
        float4 dk, ph;
        dk.x = rt_minus(th.x, ot.x) / h2; dk.y = rt_minus(th.y, ot.y) / h2; dk.z = rt_minus(th.z, ot.z) / h2; dk.w = rt_minus(th.w, ot.w) / h2;
        if constexpr (FOLD) {
          ph.x = (og.x + rs * th.x / h2) / fn; ph.y = (og.y + rs * th.y / h2) / fn;
          ph.z = (og.z + rs * th.z / h2) / fn; ph.w = (og.w + rs * th.w / h2) / fn;
        } else {
          ph.x = (og.x + dk.x) / fn; ph.y = (og.y + dk.y) / fn; ph.z = (og.z + dk.z) / fn; ph.w = (og.w + dk.w) / fn;
        }
        *reinterpret_cast<float4*>(phi + e) = ph;
        if (dK) *reinterpret_cast<float4*>(dK + e) = dk;
        // (the square of a float is exact in fp64, so a fused and an unfused x * x + y * y round alike: whatever the compiler
        // contracts in one specialised loop and not in another, |phi|^2 is the same to the bit.  The statistic's terms below
        // are not of that kind; nothing compares them bit for bit between the forms.)
        sq += ((double)ph.x * (double)ph.x + (double)ph.y * (double)ph.y) + ((double)ph.z * (double)ph.z + (double)ph.w * (double)ph.w);
        if constexpr (KSD) {
          const float4 g = theta4(G + (size_t)row0 * d + e);
          ksd_terms(g.x, kg(og.x, ot.x), ot.x, th.x, rs, ih, ks, kd);
          ksd_terms(g.y, kg(og.y, ot.y), ot.y, th.y, rs, ih, ks, kd);
          ksd_terms(g.z, kg(og.z, ot.z), ot.z, th.z, rs, ih, ks, kd);
          ksd_terms(g.w, kg(og.w, ot.w), ot.w, th.w, rs, ih, ks, kd);
        }
      }
    };
    using std::integral_constant;
    auto run_nz = [&](auto nz) {   // (FOLD: K.theta comes in ONE range -- stein_step_views -- and only when something asks for it)
      if constexpr (!FOLD) run(nz, nz);
      else if (need_t) run(nz, integral_constant<int, 1>());
      else run(nz, integral_constant<int, 0>());
    };
    if (split == 1) run_nz(integral_constant<int, 1>());
    else if (split == 2) run_nz(integral_constant<int, 2>());
    else if (split == 4) run_nz(integral_constant<int, 4>());
    else run(integral_constant<int, 0>(), integral_constant<int, 0>());
  } else if (vec == 2) {
    // d % 4 == 0 and only the input rows (theta; the score of the statistic) off their 16-byte boundaries -- a view into a
    // larger buffer: the entries one at a time, but a thread takes the four of an element group of the branch above and adds
    // their squares as that branch does, so |phi|^2 is to the bit what aligned inputs give (the branch below deals the
    // entries to the threads one by one and adds them in another order)
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < (total >> 2); q += (long)gridDim.x * 256) {
      const int i = (int)(q / (d >> 2));
      float rs = 0.f;
      for (int z = 0; z < split; ++z) rs += RS[(size_t)z * n_local + i];
      double p2[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const long e = (q << 2) + c;
        float og = 0.f, ot = 0.f;
        for (int z = 0; z < split; ++z) {
          og += OG[z * zs + e];
          if (FOLD ? need_t && z < tsplit : true) ot += OT[z * zs + e];
        }
        const float th = elem_f32(T + (size_t)row0 * d + e);
        const float dk = (rs * th - ot) / h2;
        const float ph = FOLD ? (og + rs * th / h2) / fn : (og + dk) / fn;
        phi[e] = ph;
        if (dK) dK[e] = dk;
        p2[c] = (double)ph * (double)ph;
        if constexpr (KSD) ksd_terms(elem_f32(G + (size_t)row0 * d + e), kg(og, ot), ot, th, rs, ih, ks, kd);
      }
      sq += (p2[0] + p2[1]) + (p2[2] + p2[3]);
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
// test hook (per calling thread; tests/test_gpu_glue.py): j ranges the folded contraction's plan asks for, 0 = its own rule.
// A range still starts on a multiple of 128 columns and empty tails are dropped: stein_layout_fold_ranges tells the outcome.
static thread_local int g_fold_split = 0;
extern "C" int stein_debug_fold_split(int ranges) {
  if (ranges < 0 || ranges > 65535) return fail(STEIN_E_BADARG, "ranges %d", ranges);
  g_fold_split = ranges;
  return STEIN_OK;
}

int stein_make_layout(int64_t n_local, int64_t n, int64_t d, int dtype, int flags, SteinLayout* L) {
  if (n < 2) return fail(STEIN_E_BADARG, "n = %lld: the bandwidth divides by ln(n), need n >= 2", (long long)n);
  if (d < 1 || n_local < 1 || n_local > n) return fail(STEIN_E_SHAPE, "bad shape n_local=%lld n=%lld d=%lld", (long long)n_local, (long long)n, (long long)d);
  if (int rc = stein_check_size(n, d)) return rc;
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
  const double resident = x3 ? RESIDENT_ONE_PER_CU : 768.0;
  int64_t max_split = jt / 8 > 0 ? jt / 8 : 1;
  if (max_split > 16) max_split = 16;
  auto choose_split = [&](int64_t base_wgs, int64_t* jchunk_out, int64_t forced = 0) {
    int64_t split = 1;
    double best = -1.0;
    if (forced > 0) split = forced < jt ? forced : jt;   // (test hook: the ranges asked for; the rounding below still holds)
    for (int64_t s = 1; forced <= 0 && s <= max_split; ++s) {
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
    L->fsplit = choose_split(L->tiles_m * ((L->cblocks + 1) / 2), &L->fjchunk, g_fold_split);
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

StepViews stein_step_views(const SteinLayout& L, void* workspace, void* planes_override) {
  char* ws = (char*)workspace;
  StepViews v{};
  v.L = L;
  v.nsplit = (int)L.split; v.jchunk = (int)L.jchunk; v.tsplit = (int)L.split;
  if (ws) {
    v.r = (float*)(ws + L.off[STEIN_WS_ROWNORM]);
    v.D = (float*)(ws + L.off[STEIN_WS_DIST]);
    v.hist = (u64*)(ws + L.off[STEIN_WS_HIST]);
    v.sel = (SelState*)(ws + L.off[STEIN_WS_SELECT]);
    v.spec = spec_of(v.sel);
    v.fuse = fuse_of(v.sel);
    v.spec_buf = (u64*)(ws + L.off[STEIN_WS_SPEC]);
    v.table = spec_table_of(v.spec_buf);
    v.OG = (float*)(ws + L.off[STEIN_WS_PART_G]);
    v.OT = (float*)(ws + L.off[STEIN_WS_PART_T]);
    v.RS = (float*)(ws + L.off[STEIN_WS_PART_RS]);
    v.SQ = (double*)(ws + L.off[STEIN_WS_SQPART]);
  }
  if (planes_override) v.planes = (char*)planes_override;
  else if (ws && L.total > L.off[STEIN_WS_PLANES]) v.planes = ws + L.off[STEIN_WS_PLANES];   // (empty without STEIN_FLAG_X3)
  if (v.planes) {   // x3_* are offsets inside the planes buffer
    v.T3 = (unsigned short*)(v.planes + L.x3_t3);
    v.Tt3 = (unsigned short*)(v.planes + L.x3_tt3);
    v.Gt3 = (unsigned short*)(v.planes + L.x3_gt3);
    v.sc = (float*)(v.planes + L.x3_sc);
    v.cmax = (u32*)(v.sc + x3_sc_cmax(L.x3_dc));
    v.two_s = v.sc + x3_sc_two_s(L.x3_dc);
  }
  // The folded contraction (fused call only: every other family asks for STEIN_FLAG_NO_FOLD) keeps its partial sums in
  // storage of its own -- fold_* are offsets from the workspace base, part of them inside its PLANES section -- and has its
  // own plan.  OT there holds one range, written and read only when dK or the Stein discrepancy is asked for.
  if (L.fold && ws && !planes_override) {
    v.OG = (float*)(ws + L.fold_ow);
    v.OT = (float*)(ws + L.fold_ot);
    v.RS = (float*)(ws + L.fold_rs);
    v.nsplit = (int)L.fsplit; v.jchunk = (int)L.fjchunk; v.tsplit = 1;
  }
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

extern "C" int stein_layout_fold_ranges(int64_t n_local, int64_t n, int64_t d, int dtype, int flags, int* out) {
  if (!out) return fail(STEIN_E_BADARG, "out is NULL");
  SteinLayout L;
  int rc = stein_make_layout(n_local, n, d, dtype, flags, &L);
  if (rc) return rc;
  *out = L.fold ? (int)L.fsplit : 0;
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
  int rc = stein_make_layout(n, n, d, dtype, stein_staged_flags(true), &L);
  if (rc) return rc;
  if (planes_bytes < L.total - L.off[STEIN_WS_PLANES])
    return fail(STEIN_E_WORKSPACE, "planes buffer %zu < %zu bytes", planes_bytes, L.total - L.off[STEIN_WS_PLANES]);
  return stein_x3_split(stein_step_views(L, nullptr, x3_planes), theta_all, score_all, dtype, n, d, (hipStream_t)stream, nullptr);
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

// The dtype and row-block checks of the entry points that work on a row block.  bf16_ok: the call has what bf16 inputs run
// on (the split operand planes / STEIN_FLAG_X3), or cannot tell (the finish pass only reads the rows).
static int check_block(const char* stage, const BlockShape& b, bool bf16_ok) {
  if (b.dtype != STEIN_F32 && b.dtype != STEIN_BF16) return fail(STEIN_E_UNSUPPORTED, "%s: dtype %d", stage, b.dtype);
  if (b.dtype == STEIN_BF16 && !bf16_ok)
    return fail(STEIN_E_UNSUPPORTED, "%s: bf16 inputs need the operand planes (STEIN_FLAG_X3)", stage);
  if (b.row0 < 0 || b.n_local < 1 || b.row0 + b.n_local > b.n) return fail(STEIN_E_SHAPE, "bad row block");
  return STEIN_OK;
}

// ------------------------------------------------------------------------------------------------
// stage functions: one stage of a step on the call's views.  None derives a layout or validates.
// ------------------------------------------------------------------------------------------------
// v.r -> v.D (leading dimension v.L.ld_dist) and the level-0 counts in v.hist; stage_flags: STEIN_STAGE_*.
// window (needs v.hist): also feed the speculative median window
static int distance_stage(const StepViews& v, const BlockShape& b, const void* theta_all, int stage_flags, bool window,
                          hipStream_t s) {
  const bool sym = (stage_flags & STEIN_STAGE_SYMMETRIC) != 0;
  if (v.planes)
    return stein_x3_distance(v, b, sym, window, s, (stage_flags & STEIN_STAGE_TILES) ? -1 : ((stage_flags & STEIN_STAGE_PANEL) ? 1 : 0));
  return stein_fp32_distance(v, b, (const float*)theta_all, sym, window, s);
}

// K.[G | theta] of the block in v.D into v.OG / v.OT / v.RS
static int contract_stage(const StepViews& v, const BlockShape& b, const void* theta_all, const void* score_all,
                          const float* h2_dev, bool upper, hipStream_t s) {
  return v.planes ? stein_x3_contract_partial(v, b, h2_dev, s, upper)
                  : stein_fp32_contract_partial(v, b, (const float*)theta_all, (const float*)score_all, h2_dev, s);
}

// phi and |phi|^2 from the partial sums.  ksd (STEIN_FLAG_KSD): also the statistic from the score rows; sqnorm_out is then
// double[3].  done: the fused call's completion counters (its prologue zeroed them; the last workgroup sums the partials);
// NULL: k_sum_partial_sets does.
static int finish_stage(const StepViews& v, const BlockShape& b, const void* theta_all, const void* score_all,
                        const float* h2_dev, float* phi_local, double* sqnorm_out, float* dK_out, bool ksd, HistSync* done,
                        hipStream_t s) {
  const SteinLayout& L = v.L;
  auto al16 = [](const void* p) { return ((uintptr_t)p & 15u) == 0; };
  const size_t tsz = b.dtype == STEIN_BF16 ? 2 : 4;
  auto rows_aligned = [&](const void* p) { return (((uintptr_t)p + (size_t)b.row0 * b.d * tsz) & (4 * tsz - 1)) == 0; };
  // 0: one entry at a time; 1: four columns at a time; 2: as 1 with the input rows off their 16-byte boundaries (k_phi_finish)
  const bool group4 = (b.d % 4 == 0) && al16(v.OG) && al16(v.OT) && al16(phi_local) && al16(dK_out);
  const int vec = !group4 ? 0 : (rows_aligned(theta_all) && (!ksd || rows_aligned(score_all))) ? 1 : 2;
  auto launch = [&](auto tin, auto ksd_tag, auto fold_tag) {
    using TIN = decltype(tin);
    hipLaunchKernelGGL((k_phi_finish<TIN, decltype(ksd_tag)::value, decltype(fold_tag)::value>), dim3((unsigned)L.sq_blocks),
                       dim3(256), 0, s, v.OG, v.OT, v.RS, (const TIN*)theta_all, h2_dev, phi_local, dK_out, v.SQ, (int)b.n, (int)b.d,
                       (int)b.row0, (int)b.n_local, v.nsplit, v.tsplit, vec, done, sqnorm_out, (const TIN*)score_all);
  };
  auto launch_ksd = [&](auto tin, auto fold_tag) {
    if (ksd) launch(tin, std::true_type(), fold_tag);
    else launch(tin, std::false_type(), fold_tag);
  };
  if (L.fold) launch_ksd(0.f, std::true_type());   // fp32 inputs by construction
  else if (b.dtype == STEIN_BF16) launch_ksd((unsigned short)0, std::false_type());
  else launch_ksd(0.f, std::false_type());
  LAUNCH_CHECK("k_phi_finish");
  return done ? STEIN_OK : sum_partials(v.SQ, (int)L.sq_blocks, ksd, sqnorm_out, s);
}

// ------------------------------------------------------------------------------------------------
// staged entry points: the caller owns the buffers (and the planes, a separate allocation), so their views are the layout's
// plan and planes with the caller's buffers in place of the workspace's sections
// ------------------------------------------------------------------------------------------------
// spec != NULL (needs hist_level0): also feed the speculative median window
static int distance_block(const void* theta_all, const float* r_all, const BlockShape& b, float* dist_out, int64_t ld_dist,
                          void* hist_level0, const void* x3_planes, int flags, void* stream, SpecState* spec, u64* spec_buf) {
  if ((!theta_all && !x3_planes) || !r_all || !dist_out) return fail(STEIN_E_BADARG, "NULL pointer");
  if (b.n < 1 || b.d < 1) return fail(STEIN_E_SHAPE, "bad row block");
  int rc = check_block("distance", b, x3_planes != nullptr);
  if (rc) return rc;
  if (ld_dist < b.n || (ld_dist & 63)) return fail(STEIN_E_SHAPE, "ld_dist must be >= n and a multiple of 64");
  if ((flags & STEIN_STAGE_SYMMETRIC) && (b.row0 != 0 || b.n_local != b.n))
    return fail(STEIN_E_BADARG, "STEIN_STAGE_SYMMETRIC needs the whole matrix (row0 = 0, n_local = n) and ld_dist %% 64 == 0");
  StepViews v{};
  if (x3_planes) {   // (the fp32 kernels need nothing of a layout)
    SteinLayout L;
    if ((rc = stein_make_layout(b.n_local, b.n, b.d, b.dtype, stein_staged_flags(true), &L))) return rc;
    v = stein_step_views(L, nullptr, const_cast<void*>(x3_planes));
  }
  v.r = const_cast<float*>(r_all); v.D = dist_out; v.L.ld_dist = ld_dist; v.hist = (u64*)hist_level0;
  v.spec = spec; v.spec_buf = spec_buf;
  return distance_stage(v, b, theta_all, flags, spec != nullptr, (hipStream_t)stream);
}

extern "C" int stein_distance_block(const void* theta_all, const float* r_all, int64_t n, int64_t d, int64_t row0,
                                    int64_t n_local, int dtype, float* dist_out, int64_t ld_dist, void* hist_level0,
                                    const void* x3_planes, int flags, void* stream) {
  return distance_block(theta_all, r_all, BlockShape{n, d, row0, n_local, dtype}, dist_out, ld_dist, hist_level0, x3_planes,
                        flags, stream, nullptr, nullptr);
}

extern "C" int stein_distance_block_spec(const void* theta_all, const float* r_all, int64_t n, int64_t d, int64_t row0,
                                         int64_t n_local, int dtype, float* dist_out, int64_t ld_dist, void* hist_level0,
                                         const void* x3_planes, int flags, void* select_state, void* spec_buf,
                                         void* stream) {
  if (!hist_level0 || !select_state || !spec_buf) return fail(STEIN_E_BADARG, "NULL pointer");
  return distance_block(theta_all, r_all, BlockShape{n, d, row0, n_local, dtype}, dist_out, ld_dist, hist_level0, x3_planes,
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

// What stein_contract_partial checks, and its views: the workspace need only reach its PLANES section, the planes are the
// caller's buffer, and dist takes the place of the DIST section.
static int contract_partial_views(const float* dist, int64_t ld_dist, const void* theta_all, const void* score_all,
                                  const BlockShape& b, const float* h2_dev, const void* x3_planes, void* workspace,
                                  size_t ws_bytes, int dist_flags, StepViews* v) {
  if (dist_flags & ~(STEIN_STAGE_SYMMETRIC | STEIN_STAGE_UPPER)) return fail(STEIN_E_BADARG, "unknown distance flags 0x%x", dist_flags);
  if ((dist_flags & STEIN_STAGE_UPPER) && (!x3_planes || b.row0 != 0 || b.n_local != b.n))
    return fail(STEIN_E_BADARG, "STEIN_STAGE_UPPER: only the split path's symmetric distance pass stores the upper triangle alone");
  if (!dist || (!x3_planes && (!theta_all || !score_all)) || !h2_dev || !workspace)
    return fail(STEIN_E_BADARG, "NULL pointer");
  int rc = check_block("contract", b, x3_planes != nullptr);
  if (rc) return rc;
  SteinLayout L;
  if ((rc = stein_make_layout(b.n_local, b.n, b.d, b.dtype, stein_staged_flags(x3_planes != nullptr), &L))) return rc;
  if (ws_bytes < L.off[STEIN_WS_PLANES]) return fail(STEIN_E_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, L.off[STEIN_WS_PLANES]);
  if (ld_dist != L.ld_dist) return fail(STEIN_E_SHAPE, "ld_dist %lld != %lld", (long long)ld_dist, (long long)L.ld_dist);
  *v = stein_step_views(L, workspace, const_cast<void*>(x3_planes));
  v->D = const_cast<float*>(dist);
  return STEIN_OK;
}

extern "C" int stein_contract_partial(const float* dist, int64_t ld_dist, const void* theta_all,
                                      const void* score_all, int64_t n, int64_t d, int64_t row0, int64_t n_local,
                                      int dtype, const float* h2_dev, const void* x3_planes, void* workspace,
                                      size_t ws_bytes, int dist_flags, void* stream) {
  const BlockShape b{n, d, row0, n_local, dtype};
  StepViews v;
  int rc = contract_partial_views(dist, ld_dist, theta_all, score_all, b, h2_dev, x3_planes, workspace, ws_bytes, dist_flags, &v);
  if (rc) return rc;
  return contract_stage(v, b, theta_all, score_all, h2_dev, (dist_flags & STEIN_STAGE_UPPER) != 0, (hipStream_t)stream);
}

static int check_finish(const void* theta_all, const BlockShape& b, const float* h2_dev, float* phi_local, double* sqnorm_out,
                        void* workspace) {
  if (!theta_all || !h2_dev || !phi_local || !sqnorm_out || !workspace) return fail(STEIN_E_BADARG, "NULL pointer");
  return check_block("contract", b, true);
}

extern "C" int stein_contract_finish(const void* theta_all, int64_t n, int64_t d, int64_t row0, int64_t n_local,
                                     int dtype, const float* h2_dev, float* phi_local, double* sqnorm_out,
                                     float* dK_out, void* workspace, size_t ws_bytes, int flags, void* stream) {
  if (flags & STEIN_FLAG_KSD)
    return fail(STEIN_E_BADARG, "STEIN_FLAG_KSD: stein_contract_finish has no score operand; the statistic comes from "
                                "stein_svgd_phi, stein_rank_finish or stein_rank_step");
  const BlockShape b{n, d, row0, n_local, dtype};
  int rc = check_finish(theta_all, b, h2_dev, phi_local, sqnorm_out, workspace);
  if (rc) return rc;
  // (a staged call finishes what stein_contract_partial left: K.[G | theta], never the folded form.  The workspace need
  // only reach its PLANES section, and nothing here touches the planes.)
  SteinLayout L;
  if ((rc = stein_make_layout(n_local, n, d, dtype, (flags & ~STEIN_FLAG_FOLD) | STEIN_FLAG_NO_FOLD, &L))) return rc;
  if (ws_bytes < L.off[STEIN_WS_PLANES]) return fail(STEIN_E_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, L.off[STEIN_WS_PLANES]);
  return finish_stage(stein_step_views(L, workspace), b, theta_all, nullptr, h2_dev, phi_local, sqnorm_out, dK_out, false,
                      nullptr, (hipStream_t)stream);
}

extern "C" int stein_kernel_contract(const float* dist, int64_t ld_dist, const void* theta_all, const void* score_all,
                                     int64_t n, int64_t d, int64_t row0, int64_t n_local, int dtype,
                                     const float* h2_dev, float* phi_local, double* sqnorm_out, float* dK_out,
                                     const void* x3_planes, void* workspace, size_t ws_bytes, int dist_flags,
                                     void* stream) {
  if (dist_flags & STEIN_FLAG_KSD)
    return fail(STEIN_E_BADARG, "STEIN_FLAG_KSD: stein_kernel_contract takes distance flags only; the statistic comes from "
                                "stein_svgd_phi, stein_rank_finish or stein_rank_step");
  const BlockShape b{n, d, row0, n_local, dtype};
  StepViews v;
  int rc = contract_partial_views(dist, ld_dist, theta_all, score_all, b, h2_dev, x3_planes, workspace, ws_bytes, dist_flags, &v);
  if (rc) return rc;
  if ((rc = check_finish(theta_all, b, h2_dev, phi_local, sqnorm_out, workspace))) return rc;
  const hipStream_t s = (hipStream_t)stream;
  if ((rc = contract_stage(v, b, theta_all, score_all, h2_dev, (dist_flags & STEIN_STAGE_UPPER) != 0, s))) return rc;
  return finish_stage(v, b, theta_all, nullptr, h2_dev, phi_local, sqnorm_out, dK_out, false, nullptr, s);
}

// ------------------------------------------------------------------------------------------------
// rank-step segments: what one rank of a row-sharded run does between two collectives, as ONE call each (the stages
// above, chained on the stream).  The host layer issues: all-gather(theta), all-gather(score) | stein_rank_begin |
// all-reduce(window table or level-0 histogram) | stein_rank_pick or stein_rank_radix x3 (an all-reduce before each) |
// stein_rank_finish | all-reduce(|phi|^2).  Each public segment validates and derives its views (stein_rank_views) and
// calls its body (stein_rank_*_on); stein_rank_step (stein_comm.hip) does that once for the whole step.
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

int stein_rank_views(const BlockShape& b, void* workspace, size_t ws_bytes, int flags, StepViews* v) {
  if (!workspace) return fail(STEIN_E_BADARG, "NULL pointer");
  int rc = check_block("rank step", b, (flags & STEIN_FLAG_X3) != 0);
  if (rc) return rc;
  if (flags & ~(STEIN_FLAG_X3 | STEIN_FLAG_TILED | STEIN_FLAG_RANK_WINDOW | STEIN_FLAG_TIMING | STEIN_FLAG_KSD)) return fail(STEIN_E_BADARG, "unknown flags 0x%x", flags);
  SteinLayout L;
  if ((rc = stein_make_layout(b.n_local, b.n, b.d, b.dtype, stein_rank_flags(flags), &L))) return rc;
  if (ws_bytes < L.total) return fail(STEIN_E_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, L.total);
  *v = stein_step_views(L, workspace);
  return STEIN_OK;
}

int stein_rank_begin_on(const StepViews& v, const BlockShape& b, const void* theta_all, bool window, hipStream_t s) {
  int rc;
  if ((rc = stein_rownorms(theta_all, b.n, b.d, b.dtype, v.r, s))) return rc;
  if (v.planes && (rc = stein_x3_split(v, theta_all, nullptr, b.dtype, b.n, b.d, s, nullptr))) return rc;
  if (window) rc = stein_spec_begin(v.hist, v.sel, v.spec_buf, b.n * b.n, s);
  else rc = stein_median_begin(v.hist, v.sel, b.n * b.n, s);
  if (rc) return rc;
  if ((rc = distance_stage(v, b, theta_all, 0, window, s))) return rc;
  if (window) rc = stein_spec_tally(v.sel, v.spec_buf, s);
  return rc;
}

extern "C" int stein_rank_begin(const void* theta_all, int64_t n, int64_t d, int64_t row0, int64_t n_local, int dtype,
                                void* workspace, size_t ws_bytes, int flags, void* stream) {
  if (!theta_all) return fail(STEIN_E_BADARG, "NULL pointer");
  const BlockShape b{n, d, row0, n_local, dtype};
  StepViews v;
  int rc = stein_rank_views(b, workspace, ws_bytes, flags, &v);
  return rc ? rc : stein_rank_begin_on(v, b, theta_all, (flags & STEIN_FLAG_RANK_WINDOW) != 0, (hipStream_t)stream);
}

int stein_rank_pick_on(const StepViews& v, int64_t n, float* h2_out, float* median_out, void* flags_host, hipStream_t s) {
  int rc = stein_spec_pick(v.sel, v.spec_buf, n, h2_out, median_out, s);
  if (rc) return rc;
  // `hit` (SpecState + 28) .. `skip_l0` (+ 52): 28 bytes, to page-locked host memory the caller polls behind an event
  HIP_TRY(hipMemcpyAsync(flags_host, &v.spec->hit, 28, hipMemcpyDeviceToHost, s));
  return STEIN_OK;
}

extern "C" int stein_rank_pick(int64_t n, int64_t d, int64_t row0, int64_t n_local, int dtype, void* workspace,
                               size_t ws_bytes, int flags, float* h2_out, float* median_out, void* flags_host,
                               void* stream) {
  if (!h2_out || !flags_host) return fail(STEIN_E_BADARG, "NULL pointer");
  StepViews v;
  int rc = stein_rank_views(BlockShape{n, d, row0, n_local, dtype}, workspace, ws_bytes, flags, &v);
  return rc ? rc : stein_rank_pick_on(v, n, h2_out, median_out, flags_host, (hipStream_t)stream);
}

// need_pass: first take this level's histogram of the local block (level 0 after a window miss that skipped it);
// then (the caller has summed hist[level] over the ranks unless need_pass) ... see include/steinhip.h
int stein_rank_radix_on(const StepViews& v, const BlockShape& b, int level, int need_pass, float* h2_out, float* median_out,
                        hipStream_t s) {
  if (level < 0 || level >= STEIN_HIST_LEVELS) return fail(STEIN_E_BADARG, "level %d", level);
  if (need_pass) return stein_median_hist_pass(v.D, v.L.ld_dist, b.n_local, b.n, level, v.sel, v.hist, 0, s);
  int rc = stein_median_resolve(v.hist, level, b.n, v.sel, h2_out, median_out, s);
  if (rc) return rc;
  if (level + 1 < STEIN_HIST_LEVELS)
    rc = stein_median_hist_pass(v.D, v.L.ld_dist, b.n_local, b.n, level + 1, v.sel, v.hist, 0, s);
  return rc;
}

extern "C" int stein_rank_radix(int level, int need_pass, int64_t n, int64_t d, int64_t row0, int64_t n_local, int dtype,
                                void* workspace, size_t ws_bytes, int flags, float* h2_out, float* median_out,
                                void* stream) {
  const BlockShape b{n, d, row0, n_local, dtype};
  StepViews v;
  int rc = stein_rank_views(b, workspace, ws_bytes, flags, &v);
  return rc ? rc : stein_rank_radix_on(v, b, level, need_pass, h2_out, median_out, (hipStream_t)stream);
}

int stein_rank_finish_on(const StepViews& v, const BlockShape& b, const void* theta_all, const void* score_all,
                         const float* h2_dev, float* phi_local, double* sqnorm_out, float* dK_out, int flags,
                         hipStream_t s) {
  int rc;
  if ((flags & STEIN_FLAG_RANK_WINDOW) && (rc = stein_spec_update(v.sel, s))) return rc;
  // STEIN_FLAG_TIMING: the contraction and the finish pass are bracketed by HIP events on the stream (the earlier
  // stages of the slot read as zero length); read them back with stein_timing_read
  const StageTimer clk(flags);
  for (int k = 0; k <= STEIN_T_CONTRACT; ++k)
    if ((rc = clk.mark(k, s))) return rc;
  if ((rc = contract_stage(v, b, theta_all, score_all, h2_dev, false, s))) return rc;
  if ((rc = clk.mark(STEIN_T_FINISH, s))) return rc;
  rc = finish_stage(v, b, theta_all, score_all, h2_dev, phi_local, sqnorm_out, dK_out, (flags & STEIN_FLAG_KSD) != 0, nullptr, s);
  return rc ? rc : clk.mark(STEIN_T_NSTAGES, s);
}

extern "C" int stein_rank_finish(const void* theta_all, const void* score_all, int64_t n, int64_t d, int64_t row0,
                                 int64_t n_local, int dtype, const float* h2_dev, float* phi_local, double* sqnorm_out,
                                 float* dK_out, void* workspace, size_t ws_bytes, int flags, void* stream) {
  if (!theta_all || !score_all || !h2_dev || !phi_local || !sqnorm_out) return fail(STEIN_E_BADARG, "NULL pointer");
  const BlockShape b{n, d, row0, n_local, dtype};
  StepViews v;
  int rc = stein_rank_views(b, workspace, ws_bytes, flags, &v);
  return rc ? rc : stein_rank_finish_on(v, b, theta_all, score_all, h2_dev, phi_local, sqnorm_out, dK_out, flags,
                                        (hipStream_t)stream);
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
static int fused_prologue(const StepViews& v, const BlockShape& b, const void* theta_all, const void* score_all, int flags,
                          hipStream_t s, int fold) {
  const bool bf16_split = b.dtype == STEIN_BF16 && v.planes;
  PrologueArgs pa;
  pa.n = (int)b.n; pa.d = (int)b.d; pa.r = v.r; pa.st = v.sel; pa.sp = v.spec; pa.fs = v.fuse; pa.total = (u64)(b.n * b.n);
  pa.hist = v.hist; pa.slots = v.spec_buf;
  pa.cmax = v.cmax;   // the column maxima behind the scales (stein_x3.hip); NULL without the planes
  pa.ncmax = v.planes ? (int)(2 * v.L.x3_dc) : 0;
  pa.allow_window = (flags & STEIN_FLAG_NO_WINDOW) ? 0 : 1;
  pa.hsync = (u32*)v.table; pa.hsync_words = (int)(sizeof(HistSync) / 4);
  pa.neutral_sc = bf16_split ? v.sc : (float*)nullptr;
  pa.dc = (int)v.L.x3_dc;
  pa.folded = fold ? 1u : 0u;
  // fold == 1: no launch of the column maxima in front of the distance pass -- the prologue takes max|theta| (all the
  // distance pass needs of them) and k_split_rows turns it into the scale; the maxima themselves come with the select launch
  pa.wgmax = fold == 1 ? (u32*)((char*)v.table + PRO_WGMAX_AT) : (u32*)nullptr;
  int64_t nwg = (b.n + 3) / 4 + PRO_INIT_BLOCKS;
  if (pa.wgmax && nwg > PRO_MAX_WGS) nwg = PRO_MAX_WGS;   // (every other path keeps its grid)
  const SplitFused fused{(HistSync*)v.table, bf16_split ? &pa : nullptr, fold, pa.wgmax, (int)nwg};
  if (bf16_split) return stein_x3_split(v, theta_all, score_all, b.dtype, b.n, b.d, s, &fused);
  const dim3 grid((unsigned)nwg);
  if (b.dtype == STEIN_BF16)
    hipLaunchKernelGGL(k_prologue<unsigned short>, grid, dim3(256), 0, s, (const unsigned short*)theta_all, pa);
  else
    hipLaunchKernelGGL(k_prologue<float>, grid, dim3(256), 0, s, (const float*)theta_all, pa);
  LAUNCH_CHECK("k_prologue");
  return v.planes ? stein_x3_split(v, theta_all, score_all, b.dtype, b.n, b.d, s, &fused) : STEIN_OK;
}

extern "C" int stein_svgd_phi(const void* theta_all, const void* score_all, int64_t n, int64_t d, int64_t row0,
                              int64_t n_local, int dtype, float* phi_local, float* h2_out, double* sqnorm_out,
                              float* K_out, float* dK_out, void* workspace, size_t ws_bytes, int flags, void* stream) {
  if (!theta_all || !score_all || !phi_local || !h2_out || !sqnorm_out || !workspace)
    return fail(STEIN_E_BADARG, "NULL pointer");
  if (row0 != 0 || n_local != n)
    return fail(STEIN_E_BADARG, "stein_svgd_phi is the single-rank path (row0 = 0, n_local = n); use the staged calls");
  const BlockShape b{n, d, row0, n_local, dtype};
  SteinLayout L;
  int rc = stein_make_layout(n_local, n, d, dtype, flags, &L);   // (the fused family: the caller's flags as they are)
  if (rc) return rc;
  if ((rc = stein_take_device_error())) return rc;   // a kernel of an earlier call on this device gave up: say so now
  if ((rc = check_block("stein_svgd_phi", b, (flags & STEIN_FLAG_X3) != 0))) return rc;   // (bf16 runs on the bf16-MFMA kernels)
  if (ws_bytes < L.total) return fail(STEIN_E_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, L.total);
  const StepViews v = stein_step_views(L, workspace);
  hipStream_t s = (hipStream_t)stream;
  const bool ksd = (flags & STEIN_FLAG_KSD) != 0;
  const StageTimer clk(flags);   // STEIN_FLAG_TIMING: one event per stage boundary
  if ((rc = clk.mark(STEIN_T_PREPARE, s))) return rc;
  if (!(flags & STEIN_FLAG_TILED) && stein_small_ok(n, d, dtype)) {   // the reference's own example sizes: one kernel does it all (stein_small.hip)
    for (int k = STEIN_T_DISTANCE; k <= STEIN_T_CONTRACT; ++k)
      if ((rc = clk.mark(k, s))) return rc;
    int nparts = 0;
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
  // W = G - theta / h2 alone; with dK_out or the Stein discrepancy, with [W | theta] -- phi comes from the W half either way.
  // Its launches: k_prologue, k_colmax, k_split (theta), distance, k_spec_select (+ a slice that reads theta and the score
  // into the cache), k_hist_all, k_split_w, contraction, k_phi_finish.  With nothing but phi asked for (fold == 1) k_colmax
  // leaves: k_prologue, k_split_rows, distance, k_spec_select, k_hist_all, k_split_w, contraction, k_phi_finish -- the prologue
  // takes max|theta| from the rows it reads anyway, k_split_rows makes the distance pass's scale of it, and the select launch's
  // slice takes the column maxima from the bytes it streams anyway, for k_split_w, which writes theta's scales too.
  const bool fold_theta = L.fold && (dK_out || ksd);
  if ((rc = fused_prologue(v, b, theta_all, score_all, flags, s, L.fold ? (fold_theta ? 2 : 1) : 0))) return rc;
  if ((rc = clk.mark(STEIN_T_DISTANCE, s))) return rc;
  // single rank: the block is the whole symmetric matrix -> upper-triangle distance pass with mirrored stores,
  // level-0 histogram taken in its epilogue, levels 1-2 read the upper triangle only
  const int sf = STEIN_STAGE_SYMMETRIC | ((flags & STEIN_FLAG_TILE_DISTANCE) ? STEIN_STAGE_TILES : 0);
  if ((rc = distance_stage(v, b, theta_all, sf, true, s))) return rc;
  if ((rc = clk.mark(STEIN_T_MEDIAN, s))) return rc;
  // fold == 1: the select launch's slice takes the column maxima k_split_w needs; with the slice switched off
  // (stein_debug_no_warm) a k_colmax launch of its own does
  const bool want_maxima = L.fold && !fold_theta;
  bool slice_maxima = false;
  if ((rc = stein_fused_select(v, n, d, h2_out, theta_all, score_all, want_maxima, &slice_maxima, s))) return rc;
  if (want_maxima && !slice_maxima && (rc = stein_x3_colmax(v, (const float*)theta_all, (const float*)score_all, n, d, s)))
    return rc;
  // the split path's symmetric distance pass stores only the tiles on and above the diagonal
  const bool upper = v.planes != nullptr;
  if (K_out && (rc = stein_kernel_matrix(v.D, L.ld_dist, n_local, n, h2_out, K_out, n,
                                         STEIN_STAGE_SYMMETRIC | (upper ? STEIN_STAGE_UPPER : 0), stream)))
    return rc;
  if (L.fold && (rc = stein_x3_split_w(v, (const float*)theta_all, (const float*)score_all, n, d, h2_out, s))) return rc;
  if ((rc = clk.mark(STEIN_T_CONTRACT, s))) return rc;
  if (L.fold) rc = stein_x3_contract_fold(v, h2_out, n, d, fold_theta, s);
  else rc = contract_stage(v, b, theta_all, score_all, h2_out, upper, s);
  if (rc) return rc;
  if ((rc = clk.mark(STEIN_T_FINISH, s))) return rc;
  if ((rc = finish_stage(v, b, theta_all, score_all, h2_out, phi_local, sqnorm_out, dK_out, ksd, (HistSync*)v.table, s)))
    return rc;
  return clk.mark(STEIN_T_NSTAGES, s);
}
