// stein_select.hip -- the median of the n^2 distances, exact: the 3-level radix select over the fp32 keys of D (staged
// passes, and the fused call's chained form in one launch, k_hist_all), the speculative window around the predicted median
// (single rank: k_spec_select; several ranks: tally -> all-reduce(sum) -> pick) and the predictor behind it, with the host
// functions that launch them.  Keys, select state, window state and HistSync live in stein_common.h.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "stein_host.h"

// ------------------------------------------------------------------------------------------------
// radix select (keys, state and hist_add live in stein_common.h)
// ------------------------------------------------------------------------------------------------
__global__ void k_sel_init(SelState* st, u64 total) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const u32 even = (total & 1ull) ? 0u : 1u;
    st->rank[0] = even ? total / 2 - 1 : total / 2;
    st->rank[1] = total / 2;
    st->prefix[0] = st->prefix[1] = 0u;
    st->diverged = 0u;
    st->even = even;
    st->median = st->h2 = st->lo = st->hi = 0.f;
  }
}

// ------------------------------------------------------------------------------------------------
// radix select: histogram pass, resolve
// ------------------------------------------------------------------------------------------------
// ---- chained form of the radix select (fused call only): the histogram passes resolve the earlier levels
// themselves, so the fused call launches no k_resolve between them (and nothing at all between them matters when the
// speculative window hit: every launch is a few microseconds even when it returns at once).
// Block-wide (256 threads): the select state after `levels` resolved levels, computed from the INITIAL state in
// *st (ranks set by k_median_init, prefixes 0 -- nothing writes *st until resolve_all_body) and the global histograms.
// FRESH: the histograms may hold atomics of THIS launch (the last workgroup out, the barrier of k_hist_all): device-scope
// loads.  Otherwise earlier launches wrote them and plain loads do (served by the L2: a few thousand workgroups reading
// the same 16 KB with device-scope loads queued on the handful of memory channels that hold it, ~50 us per pass at C2).
struct ChainState { u32 prefix[2]; u64 rank[2]; bool two; };
template <bool FRESH>
__device__ __attribute__((noinline)) ChainState chain_resolve(const u64* hist_all, int levels, const SelState* st) {
  __shared__ u64 c_part[256];
  __shared__ u32 c_bin[2];
  __shared__ u64 c_rest[2];
  const int t = threadIdx.x;
  ChainState cs;
  cs.prefix[0] = cs.prefix[1] = 0u;
  cs.rank[0] = st->rank[0]; cs.rank[1] = st->rank[1];
  cs.two = false;
  for (int level = 0; level < levels; ++level) {
    const int bits = level == 2 ? 10 : 11;
    const u64* hl = hist_all + (size_t)level * 2 * STEIN_HIST_BINS;
    for (int tg = 0; tg < 2; ++tg) {
      const u64* src = hl + ((cs.two && tg == 1) ? STEIN_HIST_BINS : 0);
      u64 mine[8], sum = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) { mine[k] = FRESH ? load_fresh(src + t * 8 + k) : src[t * 8 + k]; sum += mine[k]; }
      c_part[t] = sum;
      __syncthreads();
      for (int o = 1; o < 256; o <<= 1) {   // inclusive scan
        u64 v = 0;
        if (t >= o) v = c_part[t - o];
        __syncthreads();
        c_part[t] += v;
        __syncthreads();
      }
      const u64 excl = c_part[t] - sum, rank = cs.rank[tg];
      if (t == 255 && rank >= c_part[255]) { c_bin[tg] = (u32)((1 << bits) - 1); c_rest[tg] = 0; }   // cannot happen: counts cover the rank
      if (rank >= excl && rank < excl + sum) {
        u64 cum = excl;
        int k = 0;
        while (k < 7 && cum + mine[k] <= rank) cum += mine[k++];
        c_bin[tg] = (u32)(t * 8 + k);
        c_rest[tg] = rank - cum;
      }
      __syncthreads();
      cs.prefix[tg] = (cs.prefix[tg] << bits) | c_bin[tg];
      cs.rank[tg] = c_rest[tg];
      __syncthreads();
    }
    cs.two = cs.prefix[0] != cs.prefix[1];
  }
  return cs;
}

// SYM (square symmetric block): only columns >= row are read; an off-diagonal entry counts twice.
// Level 0 sees every value and a handful of bins hold them all -> wave-merged adds.  Levels 1-2 only see the
// values inside the selected bin, spread over up to 2048 digits -> plain LDS atomics are cheaper.
// k_hist (staged calls): `hist` is this level's histogram and *st holds the state left by k_resolve.
// k_hist_all (fused call): all levels in one launch; what its last resolver needs to finish the select:
struct HistFinal {
  SelState* st;
  SpecState* sp;
  float* h2_out;
  float ln_n;
};
__device__ __attribute__((noinline)) void resolve_all_body(u64* hist_all, SelState* st, SpecState* sp, float ln_n, float* h2_out);   // below

// one histogram pass of a workgroup over a share of the block (units vb, vb + nvb, ... of "virtual workgroup" vb of nvb):
// digits of LEVEL into the LDS histogram h[2][STEIN_HIST_BINS] (zeroed by the caller), given the prefixes the earlier levels fixed
template <int LEVEL, bool SYM>
__device__ __forceinline__ void hist_pass_body(const float* __restrict__ D, long ldD, int n_local, int n, u32* h, u32 pa, u32 pb,
                                               bool two, long vb, long nvb) {
  const int lane = threadIdx.x & 63;
  // one unit = one [128][32] tile of the tile-major block (16 KB, 4 x 16 B per thread); SYM skips the tiles that lie
  // entirely below the diagonal.  (Keeping the loads of two more units in flight -- three register sets in rotation --
  // changed nothing at C2 or C3: the pass is not bound by the latency of its loads.)
  const long ntc = ldD >> 5;
  const int ntr = (n_local + DT_ROWS - 1) / DT_ROWS, ncol_tiles = (n + DT_COLS - 1) / DT_COLS;
  // SYM: row tile ti only has the units tj >= 4 ti (the others lie wholly below the diagonal).  Enumerated row by row over
  // ALL units and skipped, the strided shares were as uneven as they can be: with nvb a multiple of ncol_tiles every share
  // keeps ONE tj -- the share of the last column strip had 32 units at C3, that of the first none, and the launch lasted as
  // long as the longest (round 3: 0.19 ms per pass, twice the balanced time).  So the rows are folded as in the distance
  // pass: virtual row v = row v, then row ntr - 1 - v: W = 2 ncol_tiles - 4 (ntr - 1) useful units whatever v (the middle
  // row of an odd ntr stands alone), and L = v W + x runs over useful units only.
  const int vrows = SYM ? (ntr + 1) / 2 : ntr;
  const int W = SYM ? 2 * ncol_tiles - 4 * (ntr - 1) : ncol_tiles;
  const long units = (long)vrows * W;
  for (long u = vb; u < units; u += nvb) {
    int ti, tj;
    if (SYM) {
      const int v = (int)(u / W), x = (int)(u - (long)v * W), len0 = ncol_tiles - 4 * v;
      if (x < len0) { ti = v; tj = 4 * v + x; }
      else {
        ti = ntr - 1 - v;
        if (ti == v) continue;                       // the middle row has no partner
        tj = 4 * ti + (x - len0);
      }
      if (tj >= ncol_tiles) continue;                // (cannot happen: len0 + the partner's length = W)
    } else {
      ti = (int)(u / ncol_tiles); tj = (int)(u - (long)ti * ncol_tiles);
    }
    const float* tile = D + ((size_t)ti * ntc + tj) * DT_ELEMS;
    float4 v4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v4[q] = *reinterpret_cast<const float4*>(tile + (threadIdx.x + 256 * q) * 4);
    // Interior unit: every entry exists and (SYM) lies strictly above the diagonal -- no per-entry bounds, no per-entry
    // weight.  All but the O(n / 32) units along the edges and the diagonal take this path (C3, three passes: 0.64 -> 0.57 ms).
    const bool interior = ti * DT_ROWS + DT_ROWS <= n_local && tj * DT_COLS + DT_COLS <= n &&
                          (!SYM || tj * DT_COLS >= ti * DT_ROWS + DT_ROWS);
    if (interior) {
      constexpr u32 WT = SYM ? 2u : 1u;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float x[4] = {v4[q].x, v4[q].y, v4[q].z, v4[q].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const u32 key = f32_key(x[e]);
          if (LEVEL == 0) {
            hist_add(h, key >> 21, true, lane, WT);
          } else {
            const u32 digit = LEVEL == 1 ? ((key >> 10) & 2047u) : (key & 1023u);
            const u32 hi = LEVEL == 1 ? (key >> 21) : (key >> 10);
            if (hi == pa) atomicAdd(&h[digit], WT);
            if (two && hi == pb) atomicAdd(&h[STEIN_HIST_BINS + digit], WT);
          }
        }
      }
      continue;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int f = threadIdx.x + 256 * q;          // float4 index inside the tile: row f / 8, columns 4 (f & 7) ..
      const int row = ti * DT_ROWS + (f >> 3), c0 = tj * DT_COLS + (f & 7) * 4;
      const float x[4] = {v4[q].x, v4[q].y, v4[q].z, v4[q].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int col = c0 + e;
        const bool inb = row < n_local && col < n && (!SYM || col >= row);
        const u32 key = f32_key(x[e]);
        const u32 w = (SYM && col != row) ? 2u : 1u;
        if (LEVEL == 0) {
          if (SYM) {
            hist_add(h, key >> 21, inb && col != row, lane, 2u);
            if (inb && col == row) atomicAdd(&h[key >> 21], 1u);
          } else {
            hist_add(h, key >> 21, inb, lane);
          }
        } else {
          const u32 digit = LEVEL == 1 ? ((key >> 10) & 2047u) : (key & 1023u);
          const u32 hi = LEVEL == 1 ? (key >> 21) : (key >> 10);
          if (inb && hi == pa) atomicAdd(&h[digit], w);
          if (two && inb && hi == pb) atomicAdd(&h[STEIN_HIST_BINS + digit], w);
        }
      }
    }
  }
}

template <int LEVEL, bool SYM>
__global__ __launch_bounds__(256) void k_hist(const float* __restrict__ D, long ldD, int n_local, int n,
                                              const SelState* st, u64* hist, const u32* __restrict__ skip) {
  if (skip && *skip) return;   // the speculative window already produced this step's median
  __shared__ u32 h[2 * STEIN_HIST_BINS];
  for (int b = threadIdx.x; b < 2 * STEIN_HIST_BINS; b += 256) h[b] = 0u;
  __syncthreads();
  const u32 pa = st->prefix[0], pb = st->prefix[1];
  const bool two = st->diverged != 0u;
  hist_pass_body<LEVEL, SYM>(D, ldD, n_local, n, h, pa, pb, two, blockIdx.x, gridDim.x);
  __syncthreads();
  for (int b = threadIdx.x; b < (two ? 2 : 1) * STEIN_HIST_BINS; b += 256)
    if (h[b]) atomicAdd(&hist[b], (u64)h[b]);
}

// The whole chained radix select of the fused symmetric call in ONE launch (round 3: for n <= 4096 only, three chained
// launches above that; round 4: every size -- when the window hit, the usual case, three launches returned at once, a few
// microseconds each).  The workgroups of the one launch meet behind each level.
//
// No workgroup ever waits for one that has not started (round 3's form assumed that the whole grid was resident: two
// processes on a card, or a stream with a CU mask, could leave the resident workgroups spinning for absent ones).  The work
// of a level is cut into nvb "virtual workgroups" (virtual workgroup v takes units v, v + nvb, ... of hist_pass_body's
// enumeration).  Real workgroup b takes virtual workgroup b -- after CLAIMING it (atomic exchange on HistSync::claim, an
// address of its own) -- flushes its LDS histogram into the global one (device-scope atomics, acknowledged: s_waitcnt
// vmcnt(0)) and reports it done: one add on its class's leaf counter, and the add that completes a class adds to the top
// counter; the add that completes the top makes its workgroup the level's resolver: it walks the global histogram once
// (chain_resolve, device-scope loads), publishes the select state and the new generation in all 64 class lines.  The
// others poll the line of their class (32 pollers per line; a line carries the state too).  A workgroup that has waited
// HIST_PATIENCE polls without seeing the level complete starts looking for UNCLAIMED virtual workgroups (their owners have not
// started: the chip is shared, the stream has a CU mask, or the launch is larger than the chip) and takes them over, one
// after the other, before it goes back to waiting.  So a waiting workgroup only ever waits for virtual workgroups that
// somebody running has claimed, and every level completes with one resident workgroup as well as with two thousand; a
// workgroup that starts late finds its own virtual workgroup taken and every level published, and falls through.
// The wait is bounded all the same (a hardware fault is the only way to exhaust it): FuseState::gave_up turns the
// step's bandwidth into NaN -- a wrong median is never returned -- and raises the device's error word in page-locked host
// memory, which the next call of the C ABI on this device reports as STEIN_E_HIP (stein_take_device_error).
constexpr int HIST_SPIN_MAX = 1 << 20;
constexpr int HIST_PATIENCE = 160;     // polls (~0.3 ms in all, hs_wait) before a waiting workgroup looks for abandoned work
constexpr int HIST_BLOCKS = 2048;      // workgroups of a histogram pass (C3, every step a miss: 0.61 ms of select with 2048, 0.77 with 1024, 1.17 with 512)
constexpr int HIST_ALL_SMALL_N = 4096; // up to here k_hist_all runs HIST_ALL_VBLOCKS virtual workgroups, above HIST_BLOCKS
constexpr int HIST_ALL_VBLOCKS = 512;  // ... = its grid, 2 per CU (C2, a miss: 135 us with 512, 165 with 256, 180 with 1024)
static_assert(sizeof(HistSync) <= (size_t)SPEC_TABLE * 8, "HistSync lives in the window table");
static_assert(HIST_BLOCKS <= HS_NV, "HistSync::claim holds one flag per virtual workgroup");

// thread 0: virtual workgroup v of `level` is done (its counts have reached the global histogram) -> is this the last one?
__device__ __forceinline__ bool hs_report_done(HistSync* hs, int level, u32 v, u32 nvb) {
  return tree_report_done(hs->leaf[level], &hs->top[level], v, nvb);
}
// whole workgroup: an unclaimed virtual workgroup of `level`, claimed for the caller; nvb if there is none.  Every thief
// scans from a start of its own (workgroup id x a stride coprime to any nvb <= 2048, + the number of its attempt): a
// thousand thieves that all took the FIRST unclaimed entry fought over one virtual workgroup per round (first form: 19 ms
// for a level with 256 absent owners).
__device__ __attribute__((noinline)) u32 hs_steal(HistSync* hs, int level, u32 nvb) {
  __shared__ u32 s_first, s_got;
  for (u32 attempt = 0;; ++attempt) {
    if (threadIdx.x == 0) s_first = nvb;
    __syncthreads();
    const u32 start = (blockIdx.x * 1021u + attempt * 97u) % nvb;
    u32 mine = nvb;   // position in scan order (0 = start) of this thread's first unclaimed entry
    for (u32 i = threadIdx.x; i < nvb; i += 256) {
      u32 v = start + i;
      if (v >= nvb) v -= nvb;
      if (load_fresh(&hs->claim[level][v]) == 0u) { mine = i; break; }
    }
    if (mine < nvb) atomicMin(&s_first, mine);
    __syncthreads();
    const u32 pos = s_first;
    if (pos >= nvb) return nvb;
    u32 cand = start + pos;
    if (cand >= nvb) cand -= nvb;
    if (threadIdx.x == 0)
      s_got = __hip_atomic_exchange(&hs->claim[level][cand], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u ? 1u : 0u;
    __syncthreads();
    const bool got = s_got != 0u;
    __syncthreads();   // (s_first / s_got are rewritten by the next round)
    if (got) return cand;
  }
}

// thread 0: poll a class line until it carries generation `want`; false when max_polls ran out.  Naps of 0.25 us at first,
// 2 us after the first few dozen polls (a poll is a device-scope load: it goes to the memory side every time).
__device__ __forceinline__ bool hs_wait(const u32* gen, u32 want, int max_polls) {
  int nap = 1;
  for (int spin = 0; spin < max_polls; ++spin) {
    if (load_fresh(gen) >= want) return true;
    for (int k = 0; k < nap; ++k) __builtin_amdgcn_s_sleep(8);
    if (spin >= 32 && nap < 8) nap += nap;
  }
  return false;
}

// (not inlined, one function per level: see resolve_all_body; the three passes in one function took 70 registers, 36 apart)
template <int LEVEL>
__device__ __attribute__((noinline)) void hist_pass_sym(const float* __restrict__ D, long ldD, int n, u32* h, u32 pa, u32 pb,
                                                        bool two, u32 v, u32 nvb) {
  hist_pass_body<LEVEL, true>(D, ldD, n, n, h, pa, pb, two, v, nvb);
}

__global__ __launch_bounds__(256) void k_hist_all(const float* __restrict__ D, long ldD, int n, const SelState* st, u64* hist_all,
                                                  const u32* __restrict__ hit, const u32* __restrict__ skip_l0, HistFinal fin,
                                                  FuseState* fs, HistSync* hs /* zero at launch */, u32 nvb,
                                                  u32* errword /* page-locked host memory, or NULL */) {
  if (*hit) return;   // the speculative window already produced this step's median
  __shared__ u32 h[2 * STEIN_HIST_BINS];
  __shared__ u32 s_v, s_flag;
  const int first = *skip_l0 == 0u ? 0 : 1;   // level 0 may have been taken by the distance kernel (an earlier launch)
  ChainState cs = chain_resolve<false>(hist_all, first, st);
  const HistSync::Line* myline = &hs->line[blockIdx.x % HS_CLASSES];
  for (int level = first; level < STEIN_HIST_LEVELS; ++level) {
    const u32 want = (u32)(level - first + 1);
    // this workgroup's own virtual workgroup, unless somebody has taken it over
    if (threadIdx.x == 0)
      s_v = blockIdx.x < nvb && __hip_atomic_exchange(&hs->claim[level][blockIdx.x], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u
                ? blockIdx.x : nvb;
    bool last = false, thief = false;
    for (;;) {
      for (int b = threadIdx.x; b < 2 * STEIN_HIST_BINS; b += 256) h[b] = 0u;
      __syncthreads();
      const u32 v = s_v;
      if (v < nvb) {
        if (level == 0) hist_pass_sym<0>(D, ldD, n, h, cs.prefix[0], cs.prefix[1], cs.two, v, nvb);
        else if (level == 1) hist_pass_sym<1>(D, ldD, n, h, cs.prefix[0], cs.prefix[1], cs.two, v, nvb);
        else hist_pass_sym<2>(D, ldD, n, h, cs.prefix[0], cs.prefix[1], cs.two, v, nvb);
        __syncthreads();
        u64* hl = hist_all + (size_t)level * 2 * STEIN_HIST_BINS;
        for (int b = threadIdx.x; b < (cs.two ? 2 : 1) * STEIN_HIST_BINS; b += 256)
          if (h[b]) atomicAdd(&hl[b], (u64)h[b]);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's histogram atomics have been acknowledged
        __syncthreads();
        if (threadIdx.x == 0) s_flag = hs_report_done(hs, level, v, nvb) ? 1u : 0u;
        __syncthreads();
        last = s_flag != 0u;
        if (last) break;
      }
      if (!thief) {   // wait for the level to be published -- for a while
        __syncthreads();
        if (threadIdx.x == 0) s_flag = hs_wait(&myline->gen, want, HIST_PATIENCE) ? 1u : 0u;
        __syncthreads();
        if (s_flag) break;
        thief = true;   // out of patience: somebody's virtual workgroup may have no owner
      }
      const u32 more = hs_steal(hs, level, nvb);
      if (more < nvb) {   // an abandoned virtual workgroup, now ours
        if (threadIdx.x == 0) s_v = more;
        __syncthreads();
        continue;
      }
      // nothing is abandoned (any more): whoever claimed the rest is running and will report it
      if (threadIdx.x == 0) {
        const bool ok = hs_wait(&myline->gen, want, HIST_SPIN_MAX);
        if (!ok) __hip_atomic_store(&fs->gave_up, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      __syncthreads();
      break;
    }
    const bool final_level = level + 1 == STEIN_HIST_LEVELS;
    if (last) {   // the level's resolver
      if (final_level) {
        resolve_all_body(hist_all, fin.st, fin.sp, fin.ln_n, fin.h2_out);
        if (threadIdx.x == 0 && load_fresh(&fs->gave_up)) {   // a wait ran out somewhere: no median, and loudly so
          fin.st->median = fin.st->h2 = __builtin_nanf("");
          if (fin.h2_out) *fin.h2_out = __builtin_nanf("");
          if (errword) __hip_atomic_store(errword, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
      } else {
        cs = chain_resolve<true>(hist_all, level + 1, st);
      }
      if (threadIdx.x < HS_CLASSES) {   // one thread per class line: the state first, then (acknowledged) the generation
        HistSync::Line* ln = &hs->line[threadIdx.x];
        const u32 w[6] = {cs.prefix[0], cs.prefix[1], (u32)cs.rank[0], (u32)(cs.rank[0] >> 32), (u32)cs.rank[1], (u32)(cs.rank[1] >> 32)};
#pragma unroll
        for (int k = 0; k < 6; ++k) __hip_atomic_store(&ln->pub[k], w[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(&ln->gen, want, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      continue;   // (behind the final level the loop ends)
    }
    if (final_level) return;   // the select is complete (or, gave_up, declared failed); nobody needs the state any more
    // (a workgroup that started late may read the state of a LATER level here, or a mix of two: then that later level was
    // complete before the read, all of its virtual workgroups are claimed, and the state is never used)
    u32 w[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) w[k] = load_fresh(&myline->pub[k]);
    cs.prefix[0] = w[0]; cs.prefix[1] = w[1];
    cs.rank[0] = (u64)w[2] | ((u64)w[3] << 32); cs.rank[1] = (u64)w[4] | ((u64)w[5] << 32);
    cs.two = w[0] != w[1];
  }
}

// one wave; hist points at this level's [2][STEIN_HIST_BINS] counters (already summed over ranks)
__global__ __launch_bounds__(64) void k_resolve(const u64* __restrict__ hist, int level, SelState* st, float ln_n,
                                                float* h2_out, float* median_out, const u32* __restrict__ skip) {
  if (skip && *skip) return;
  __shared__ u64 bins[STEIN_HIST_BINS];
  __shared__ u64 chunk[64];
  const int lane = threadIdx.x;
  const int bits = level == 2 ? 10 : 11;
  const bool div_in = st->diverged != 0u;
  u32 newp[2];
  u64 newr[2];
  for (int tg = 0; tg < 2; ++tg) {
    const u64* src = hist + ((div_in && tg == 1) ? STEIN_HIST_BINS : 0);
    u64 s = 0;
    for (int b = 0; b < 32; ++b) {
      const u64 c = src[lane * 32 + b];
      bins[lane * 32 + b] = c;
      s += c;
    }
    chunk[lane] = s;
    __syncthreads();
    if (lane == 0) {
      u64 rank = st->rank[tg], cum = 0;
      int c = 0;
      while (c < 63 && cum + chunk[c] <= rank) cum += chunk[c++];
      int b = c * 32;
      const int bend = b + 31;
      while (b < bend && cum + bins[b] <= rank) cum += bins[b++];
      newp[tg] = (st->prefix[tg] << bits) | (u32)b;
      newr[tg] = rank - cum;
    }
    __syncthreads();
  }
  if (lane == 0) {
    st->prefix[0] = newp[0]; st->prefix[1] = newp[1];
    st->rank[0] = newr[0]; st->rank[1] = newr[1];
    st->diverged = (newp[0] != newp[1]) ? 1u : 0u;
    if (level == 2) {
      const float lo = key_f32(newp[0]), hi = key_f32(newp[1]);
      const MedianBw m = median_bandwidth(lo, hi, st->even, ln_n);
      st->lo = lo; st->hi = hi; st->median = m.med; st->h2 = m.h2;
      if (h2_out) *h2_out = m.h2;
      if (median_out) *median_out = m.med;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// speculative median window (SpecState in stein_common.h): begin / select / update, one launch each per step
__global__ __launch_bounds__(256) void k_median_init(SelState* st, SpecState* sp, u64 total, u64* __restrict__ hist,
                                                     u64* __restrict__ slots) {
  median_init_body(blockIdx.x * 256 + threadIdx.x, gridDim.x * 256, st, sp, total, hist, slots);
}
__device__ __attribute__((noinline)) void spec_update_dev(const SelState* st, SpecState* sp);   // below

// All 256 bins of an LDS histogram -> the bin holding 0-based rank `rank` and the rank inside it; *bin = 256 when the
// rank lies past the last bin.  Called by the whole workgroup (>= 256 threads); `scan` is 256 words of LDS scratch.
// Both targets at once: waves 0-3 scan histogram hA (256 bins) for rankA, waves 4-7 histogram hB for rankB, each with
// shuffles; `scan[0..7]` carries the wave totals (2 barriers in all; round 4: four separate locates cost 12 of them, ~1.4 k
// cycles each time, a quarter of this one-workgroup kernel).  bin[k] = 256: rank k lies beyond its histogram.
__device__ __forceinline__ void spec_locate2(const u32* hA, u32 rankA, const u32* hB, u32 rankB, u32* scan, u32* bin, u32* rest) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int side = t >> 8;                       // 0: target A (threads 0..255), 1: target B (256..511)
  u32 c = 0u, incl = 0u;
  if (t < 512) {
    c = (side ? hB : hA)[t & 255];
    incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const u32 v = __shfl_up(incl, o);
      if (lane >= o) incl += v;
    }
    if (lane == 63) scan[wave] = incl;
  }
  if (t < 2) bin[t] = 256u;
  __syncthreads();
  if (t < 512) {
    u32 base = 0u;
    for (int w = side * 4; w < wave; ++w) base += scan[w];
    const u32 excl = base + incl - c, rank = side ? rankB : rankA;
    if (excl <= rank && rank < excl + c) { bin[side] = (u32)(t & 255); rest[side] = rank - excl; }
  }
  __syncthreads();
}

// One workgroup: exact weighted selection of the two median targets among the buffered window entries.
// Entry = key << 2 | weight, offset o = key - lo_key < 65536: pass 1 histograms o >> 8, pass 2 the low byte of the
// entries that share each target's high byte.  Returns (workgroup-uniform) whether the window held both targets.
__device__ __forceinline__ bool spec_select_body(SelState* st, SpecState* sp, const u64* __restrict__ slots, float ln_n,
                                                 float* h2_out, int update) {
  const u64* __restrict__ buf = slots + SPEC_SLOTS * 8;
  __shared__ u32 h1[256], h2a[256], h2b[256], scan[256];
  __shared__ u32 sel[8];   // [0,1] high bytes, [2,3] ranks inside them, [4,5] low bytes, [6,7] scratch
  __shared__ u64 below_s;
  const int t = threadIdx.x;
  const u32 cnt = sp->count, lo = sp->lo_key, width = sp->width;
  if (width == 0u || sp->overflow || cnt > SPEC_CAP || cnt == 0u) return false;   // miss: the radix select runs
  // thread 0 asks now for what it will need at the very end (the result and the predictor update are a chain of dependent
  // loads otherwise: ~3 k cycles behind the last barrier)
  u32 even0 = 0u;
  if (t == 0) even0 = st->even;
  u64 mine = t < (int)SPEC_SLOTS ? slots[t * 8] : 0ull;
  const u64 total = sp->total;
  if (t == 0) below_s = 0ull;
  if (t < 256) { h1[t] = 0u; h2a[t] = 0u; h2b[t] = 0u; }
  __syncthreads();
  {
    // the weights below the window, one slot per thread: summed per wave first (256 same-address 64-bit LDS atomics took
    // 7 k cycles of this kernel's 28 k at C2)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if ((t & 63) == 0 && mine) atomicAdd(reinterpret_cast<unsigned long long*>(&below_s), (unsigned long long)mine);
  }
  __syncthreads();
  const u64 below = below_s;
  const u64 r0 = (total & 1ull) ? total / 2 : total / 2 - 1, r1 = total / 2;
  if (r0 < below || r1 - below > 0xfffffff0ull) return false;   // the target lies below the window
  // Pass 1 histograms the HIGH byte of the offsets: a window of `width` keys occupies (width >> 8) + 1 bins, a handful, and
  // every entry of every wave lands in them.  Up to 16 entries per thread are fetched ONCE, all loads in flight together,
  // and both passes work from the registers (round 4: the loops below paid one memory latency per 1024 entries, twice).
  // With at most eight bins in play the counts are kept in eight registers per thread, summed over the wave with shuffles
  // and added with one atomic per wave and bin (LDS atomics merged by ballots, below, were 1 k cycles per 1024 entries:
  // 7 k of this kernel's 28 k cycles at C2, 15 k of 39 k at C3).
  // (the 8-byte entries come through ONE compute unit: 13 k of them are 108 KB, ~3 k cycles of its load path -- requested
  // any earlier they only delay the slot sums above, which wait behind them in the memory pipeline)
  constexpr int EPT = 16;
  const bool inreg = cnt <= 1024u * EPT;
  const u32 nb = (width >> 8) + 1u;
  u64 er[EPT];
  if (inreg) {
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
      const u32 i = (u32)k * 1024u + (u32)t;
      er[k] = (u32)k * 1024u < cnt && i < cnt ? buf[i] : 0ull;   // (0: weight 0, counted nowhere)
    }
  }
  if (inreg && nb <= 8u) {
    u32 c[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
      if ((u32)k * 1024u < cnt) {                // workgroup-uniform
        const u64 e = er[k];
        const u32 hb = (((u32)(e >> 2) - lo) >> 8) & 255u, w = (u32)e & 3u;
#pragma unroll
        for (int b = 0; b < 8; ++b) c[b] += hb == (u32)b ? w : 0u;
      }
    }
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      if ((u32)b < nb) {                         // workgroup-uniform
        u32 v = c[b];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if ((t & 63) == 0 && v) atomicAdd(&h1[b], v);
      }
    }
  } else if (inreg) {
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
      if ((u32)k * 1024u < cnt) {                // workgroup-uniform: the ballots need every lane of a wave
        const u64 e = er[k];
        const u32 hb = (((u32)(e >> 2) - lo) >> 8) & 255u, w = (u32)e & 3u;
        hist_add(h1, hb, w == 2u, t & 63, 2u);   // (lanes that share the leader's bin are merged into one atomic per wave)
        hist_add(h1, hb, w == 1u, t & 63, 1u);
        if (w == 3u) atomicAdd(&h1[hb], 3u);     // (no producer writes weight 3; kept exact all the same)
      }
    }
  } else {
    for (u32 i0 = 0; i0 < cnt; i0 += 1024) {   // wave-uniform trip count: the ballots need every lane
      const u32 i = i0 + (u32)t;
      const bool ok = i < cnt;
      const u64 e = ok ? buf[i] : 0ull;
      const u32 hb = (((u32)(e >> 2) - lo) >> 8) & 255u, w = (u32)e & 3u;
      hist_add(h1, hb, ok && w == 2u, t & 63, 2u);
      hist_add(h1, hb, ok && w == 1u, t & 63, 1u);
      if (ok && w == 3u) atomicAdd(&h1[hb], 3u);
    }
  }
  __syncthreads();
  spec_locate2(h1, (u32)(r0 - below), h1, (u32)(r1 - below), scan, &sel[0], &sel[2]);
  const u32 ba = sel[0], bb = sel[1];
  if (ba == 256u || bb == 256u) return false;   // a target lies above the window
  const bool two_hb = ba != bb;                 // (both targets in one high byte, the usual case: one low-byte histogram serves both)
  if (inreg) {
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
      if ((u32)k * 1024u < cnt) {                // workgroup-uniform
        const u64 e = er[k];
        const u32 o = (u32)(e >> 2) - lo, w = (u32)e & 3u;
        if (w && (o >> 8) == ba) atomicAdd(&h2a[o & 255u], w);
        if (w && two_hb && (o >> 8) == bb) atomicAdd(&h2b[o & 255u], w);
      }
    }
  } else {
    for (u32 i = t; i < cnt; i += 1024) {
      const u64 e = buf[i];
      const u32 o = (u32)(e >> 2) - lo, w = (u32)e & 3u;
      if ((o >> 8) == ba) atomicAdd(&h2a[o & 255u], w);
      if (two_hb && (o >> 8) == bb) atomicAdd(&h2b[o & 255u], w);
    }
  }
  __syncthreads();
  spec_locate2(h2a, sel[2], two_hb ? h2b : h2a, sel[3], scan, &sel[4], &sel[6]);
  if (t == 0) {
    const float flo = key_f32(lo + ((ba << 8) | sel[4])), fhi = key_f32(lo + ((bb << 8) | sel[5]));
    const MedianBw m = median_bandwidth(flo, fhi, even0, ln_n);
    st->lo = flo; st->hi = fhi; st->median = m.med; st->h2 = m.h2;
    if (h2_out) *h2_out = m.h2;
    sp->hit = 1u;
    sp->skip_l0 = 1u;
    if (update) spec_update_dev(st, sp);   // fused call: no separate k_spec_update launch
  }
  return true;
}

// Small symmetric blocks (fused call, n <= SOLO_MAX_N): when the window misses, this one workgroup runs the whole
// 3-level radix select over the upper triangle of D itself (LDS histograms, digits located by a prefix sum over the
// 2048 bins), so the fused call launches no histogram passes at all -- three launches that, on the usual hit, did
// nothing for 4-5 us each.  A miss costs ~30 us here instead of ~15 us; misses are the first two steps and jumps.
constexpr int SOLO_MAX_N = 512;
__device__ __forceinline__ void solo_locate(const u32* h, u32 rank, u32* wsum, u32* out_bin, u32* out_rest) {
  // 1024 threads, two bins each; *out_bin / *out_rest are LDS words written by the one thread that finds the rank
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const u32 c0 = h[2 * t], c1 = h[2 * t + 1];
  u32 incl = c0 + c1;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u32 v = __shfl_up(incl, o);
    if (lane >= o) incl += v;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  u32 base = 0u;
  for (int w = 0; w < wave; ++w) base += wsum[w];
  const u32 excl = base + incl - (c0 + c1);
  if (rank >= excl && rank < excl + c0 + c1) {
    const u32 b = rank < excl + c0 ? 2u * t : 2u * t + 1u;
    *out_bin = b;
    *out_rest = rank - ((b & 1u) ? excl + c0 : excl);
  }
  __syncthreads();
}
__device__ __forceinline__ void solo_select(const float* __restrict__ D, long ldD, int n, SelState* st, SpecState* sp,
                                            float ln_n, float* h2_out) {
  __shared__ u32 sh[2 * STEIN_HIST_BINS];
  __shared__ u32 s_wsum[16], s_bin[2], s_rest[2];
  const int t = threadIdx.x;
  const long ntc = ldD >> 5;
  const int ntr = (n + DT_ROWS - 1) / DT_ROWS, nct = (n + DT_COLS - 1) / DT_COLS;
  const u32 total = (u32)n * (u32)n;
  u32 prefix[2] = {0u, 0u};
  u32 rank[2] = {(total & 1u) ? total / 2 : total / 2 - 1, total / 2};
  bool two = false;
  for (int level = 0; level < STEIN_HIST_LEVELS; ++level) {
    const int bits = level == 2 ? 10 : 11, shift = level == 0 ? 21 : (level == 1 ? 10 : 0);
    for (int b = t; b < 2 * STEIN_HIST_BINS; b += 1024) sh[b] = 0u;
    __syncthreads();
    for (int ti = 0; ti < ntr; ++ti)
      for (int tj = 0; tj < nct; ++tj) {
        if (tj * DT_COLS + DT_COLS <= ti * DT_ROWS) continue;   // wholly below the diagonal
        const float4 v4 = *reinterpret_cast<const float4*>(D + ((size_t)ti * ntc + tj) * DT_ELEMS + t * 4);
        const int row = ti * DT_ROWS + (t >> 3), c0 = tj * DT_COLS + (t & 7) * 4;
        const float x[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int col = c0 + e;
          if (row < n && col < n && col >= row) {
            const u32 key = f32_key(x[e]), w = col != row ? 2u : 1u;
            const u32 digit = (key >> shift) & ((1u << bits) - 1u);
            const u32 hi = level == 0 ? 0u : key >> (shift + bits);
            if (level == 0 || hi == prefix[0]) atomicAdd(&sh[digit], w);
            if (two && hi == prefix[1]) atomicAdd(&sh[STEIN_HIST_BINS + digit], w);
          }
        }
      }
    __syncthreads();
    solo_locate(sh, rank[0], s_wsum, &s_bin[0], &s_rest[0]);
    solo_locate(sh + (two ? STEIN_HIST_BINS : 0), rank[1], s_wsum, &s_bin[1], &s_rest[1]);
    prefix[0] = (prefix[0] << bits) | s_bin[0];
    prefix[1] = (prefix[1] << bits) | s_bin[1];
    rank[0] = s_rest[0];
    rank[1] = s_rest[1];
    two = prefix[0] != prefix[1];
    __syncthreads();   // s_bin / s_rest are rewritten by the next level
  }
  if (t == 0) {
    st->prefix[0] = prefix[0]; st->prefix[1] = prefix[1];
    st->rank[0] = rank[0]; st->rank[1] = rank[1];
    st->diverged = two ? 1u : 0u;
    const float lo = key_f32(prefix[0]), hi = key_f32(prefix[1]);
    const MedianBw m = median_bandwidth(lo, hi, st->even, ln_n);
    st->lo = lo; st->hi = hi; st->median = m.med; st->h2 = m.h2;
    if (h2_out) *h2_out = m.h2;
    spec_update_dev(st, sp);
  }
}

// D != NULL ("solo", fused call on a small symmetric block): a miss is resolved here by solo_select
// Workgroups 1 .. gridDim.x - 1 (fused call with the folded operand only; the select is workgroup 0, one workgroup on an
// otherwise idle chip) are a slice that reads warm0 and warm1 -- the score and theta: the distance pass has just pushed
// 0.5 GB of D through the memory-side cache, and k_split_w, next but one in the stream, then finds its inputs there again.
// They wait for nothing and the select does not wait for them.
//   slice = SLICE_READ (the step also contracts K with theta: dK / KSD): warm4 16-byte pieces of each, values dropped
//   slice = SLICE_MAX16 / SLICE_MAX4 (phi alone): the same bytes as [n][d] matrices, reduced to their column maxima in
//     cmax = [score | theta] (zeroed by the prologue), which k_split_w turns into W's and theta's scales -- the step has no
//     k_colmax launch.  Workgroup 1 + rg * ncg + cb scans column block cb (256 columns in the 16-byte form for d % 4 == 0
//     and aligned inputs, 64 in the 4-byte form) of the rows 16 rg + wave, + 16 nrg, ... of BOTH matrices: eight loads in
//     flight per lane, and nrg atomics per column (colmax_scan, colmax_commit: stein_common.h)
enum { SLICE_READ = 0, SLICE_MAX16 = 1, SLICE_MAX4 = 2 };
template <bool V4>
__device__ __forceinline__ void slice_maxima(const float* __restrict__ G, const float* __restrict__ T, int n, int d,
                                             u32* __restrict__ cmax, int dc, int ncg, int nrg, u32* red) {
  constexpr int CW = V4 ? 4 : 1;
  const int w = (int)blockIdx.x - 1, cb = w % ncg, rg = w / ncg;
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const float* const X[2] = {G, T};
  u32 m[2][CW];
  colmax_scan<float, V4, 2>(X, n, d, (cb * 64 + cx) * CW, (long)rg * 16 + ry, (long)nrg * 16, m);
  colmax_commit<CW, 2>(m, cx, cb, d, red, cmax, dc);
}

__global__ __launch_bounds__(1024) void k_spec_select(SelState* st, SpecState* sp, const u64* __restrict__ slots,
                                                      float ln_n, float* h2_out, int update,
                                                      const float* __restrict__ D, long ldD, int n,
                                                      const float4* __restrict__ warm0, const float4* __restrict__ warm1,
                                                      long warm4, int slice, int d, u32* __restrict__ cmax, int dc, int ncg,
                                                      int nrg) {
  if (blockIdx.x) {
    if (slice != SLICE_READ) {
      __shared__ u32 red[2 * 256];
      if (slice == SLICE_MAX16)
        slice_maxima<true>((const float*)warm0, (const float*)warm1, n, d, cmax, dc, ncg, nrg, red);
      else
        slice_maxima<false>((const float*)warm0, (const float*)warm1, n, d, cmax, dc, ncg, nrg, red);
      return;
    }
    const long stride = (long)(gridDim.x - 1) * 1024;
    auto keep = [](const float4& a) { asm volatile("" ::"v"(a.x), "v"(a.y), "v"(a.z), "v"(a.w)); };
    long i = (long)(blockIdx.x - 1) * 1024 + threadIdx.x;
    for (; i + 3 * stride < warm4; i += 4 * stride) {   // eight loads in flight per lane, both matrices together
      const float4 a0 = warm0[i], a1 = warm0[i + stride], a2 = warm0[i + 2 * stride], a3 = warm0[i + 3 * stride];
      const float4 b0 = warm1[i], b1 = warm1[i + stride], b2 = warm1[i + 2 * stride], b3 = warm1[i + 3 * stride];
      keep(a0); keep(a1); keep(a2); keep(a3); keep(b0); keep(b1); keep(b2); keep(b3);
    }
    for (; i < warm4; i += stride) {
      const float4 a0 = warm0[i], b0 = warm1[i];
      keep(a0); keep(b0);
    }
    return;
  }
  const bool hit = spec_select_body(st, sp, slots, ln_n, h2_out, update);
  if (!hit && D) {
    __syncthreads();
    solo_select(D, ldD, n, st, sp, ln_n, h2_out);
  }
}

// ---- the window across several ranks: tally -> all-reduce(sum) -> pick ---------------------------------------------
// this rank's window entries -> one counter per key (table[SPEC_TABLE_HDR + key - lo_key]); workgroup 0 also fills the header
__global__ __launch_bounds__(256) void k_spec_tally(const SpecState* __restrict__ sp, const u64* __restrict__ slots,
                                                    u64* __restrict__ table) {
  const u64* __restrict__ buf = slots + SPEC_SLOTS * 8;
  const u32 cnt = sp->count, lo = sp->lo_key;
  const bool bad = sp->width == 0u || sp->overflow || cnt > SPEC_CAP;
  if (blockIdx.x == 0) {
    if (threadIdx.x < (int)SPEC_SLOTS && slots[threadIdx.x * 8])
      atomicAdd(reinterpret_cast<unsigned long long*>(&table[0]), (unsigned long long)slots[threadIdx.x * 8]);
    if (threadIdx.x == 0) {
      if (bad) atomicAdd(reinterpret_cast<unsigned long long*>(&table[1]), 1ull);
      atomicAdd(reinterpret_cast<unsigned long long*>(&table[2]), (unsigned long long)cnt);
    }
  }
  if (bad) return;
  for (u32 i = blockIdx.x * 256 + threadIdx.x; i < cnt; i += gridDim.x * 256) {
    const u64 e = buf[i];
    atomicAdd(reinterpret_cast<unsigned long long*>(&table[SPEC_TABLE_HDR + ((u32)(e >> 2) - lo)]),
              (unsigned long long)(e & 3ull));
  }
}

// one workgroup: the two median targets from the rank-summed table (identical on every rank)
__global__ __launch_bounds__(1024) void k_spec_pick(SelState* st, SpecState* sp, const u64* __restrict__ table,
                                                    float ln_n, float* h2_out, float* median_out) {
  __shared__ u64 part[1024];
  __shared__ u32 found[2];
  const int t = threadIdx.x;
  const u32 width = sp->width, lo = sp->lo_key;
  // k_spec_update sizes the next window from `count`: make it the GLOBAL number of entries so that every rank's
  // predictor stays identical (the local counts differ from rank to rank)
  if (t == 0) sp->count = table[2] > 0xffffffffull ? 0xffffffffu : (u32)table[2];
  if (width == 0u || table[1] != 0ull) return;   // miss on every rank alike
  const u64 total = sp->total, below = table[0];
  const u64 r0 = (total & 1ull) ? total / 2 : total / 2 - 1, r1 = total / 2;
  if (r0 < below) return;
  constexpr int PER = 64;   // 1024 threads x 64 keys >= 65536
  u64 mine = 0ull;
  for (int k = 0; k < PER; ++k) {
    const u32 key = (u32)t * PER + k;
    if (key <= width) mine += table[SPEC_TABLE_HDR + key];
  }
  part[t] = mine;
  if (t < 2) found[t] = 0xffffffffu;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {   // inclusive scan
    u64 v = 0ull;
    if (t >= o) v = part[t - o];
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  const u64 excl = part[t] - mine;
  for (int tg = 0; tg < 2; ++tg) {
    const u64 rank = (tg ? r1 : r0) - below;
    if (excl <= rank && rank < excl + mine) {
      u64 cum = excl;
      for (int k = 0; k < PER; ++k) {
        const u64 c = table[SPEC_TABLE_HDR + (u32)t * PER + k];
        if (rank < cum + c) { found[tg] = (u32)t * PER + k; break; }
        cum += c;
      }
    }
  }
  __syncthreads();
  if (t == 0 && found[0] != 0xffffffffu && found[1] != 0xffffffffu) {
    const float flo = key_f32(lo + found[0]), fhi = key_f32(lo + found[1]);
    const MedianBw m = median_bandwidth(flo, fhi, st->even, ln_n);
    st->lo = flo; st->hi = fhi; st->median = m.med; st->h2 = m.h2;
    if (h2_out) *h2_out = m.h2;
    if (median_out) *median_out = m.med;
    sp->hit = 1u;
    sp->skip_l0 = 1u;
  }
}

// after the median is final (window or radix passes): predict the next one and size its window (one thread)
__device__ __attribute__((noinline)) void spec_update_dev(const SelState* st, SpecState* sp) {
  const u32 key = f32_key(st->lo);
  const bool had_window = sp->width != 0u;
  u32 hw = 4096u, next = key, earned = 0u;
  if (sp->magic == SPEC_MAGIC1 || sp->magic == SPEC_MAGIC2) {
    // linear extrapolation of the VALUE (key space bends at every power of two)
    const float pred = 2.f * st->lo - key_f32(sp->last_key);
    long c = (long)f32_key(pred == pred ? pred : st->lo);
    c = c < 65536l ? 65536l : (c > 0xfffe0000l ? 0xfffe0000l : c);
    next = (u32)c;
    if (sp->magic == SPEC_MAGIC2 && had_window) {   // the window of this step was centred on a real prediction
      const u32 err = key > sp->center ? key - sp->center : sp->center - key;
      hw = err > SPEC_HW_MAX / 4u ? SPEC_HW_MAX : 4u * err + 48u;
      // ... and never below three quarters of the previous one: one lucky prediction (an error of a few keys) used to shrink
      // the window to ~60 keys and the next ordinary error missed it -- 10 % misses under noisy scores and at n = 4096 in
      // bf16; with the floor 1 %, for a window a third wider on average (scratch/window_policy.py replays the rules on
      // recorded runs: profiles/r04_window_policy.txt).  A miss costs a radix select, a wider window a few more entries.
      // (the floor follows EARNED widths only: the 4096-key window of a predictor without a velocity is not one)
      const u32 floor_hw = sp->earned_hw - sp->earned_hw / 4u;
      if (hw < floor_hw) hw = floor_hw;
      earned = hw;
      if (sp->hit && sp->count > SPEC_CAP / 2 && hw > sp->halfwidth / 2u) hw = sp->halfwidth / 2u + 1u;   // keep the buffer small
    }
    sp->magic = SPEC_MAGIC2;
    sp->n_steps += 1u;
    sp->n_hits += sp->hit ? 1u : 0u;
  } else {
    sp->magic = SPEC_MAGIC1;
    sp->n_steps = 1u;
    sp->n_hits = 0u;
  }
  sp->last_key = key;
  sp->center = next;
  sp->halfwidth = hw > SPEC_HW_MAX ? SPEC_HW_MAX : hw;
  sp->earned_hw = earned > SPEC_HW_MAX ? SPEC_HW_MAX : earned;
}
__global__ void k_spec_update(const SelState* st, SpecState* sp) {
  if (threadIdx.x || blockIdx.x) return;
  spec_update_dev(st, sp);
}

// end of the chained radix select (fused call): all three resolves, the median / bandwidth, the predictor update;
// one workgroup of 256 threads
// (not inlined, like chain_resolve and hs_steal: inlined into k_hist_all their constants and addresses were hoisted in front
// of the level loop -- 114 registers, four workgroups per CU instead of eight, for code that one workgroup runs once)
__device__ __attribute__((noinline)) void resolve_all_body(u64* hist_all, SelState* st, SpecState* sp, float ln_n, float* h2_out) {
  const ChainState cs = chain_resolve<true>(hist_all, STEIN_HIST_LEVELS, st);
  if (threadIdx.x == 0) {
    st->prefix[0] = cs.prefix[0]; st->prefix[1] = cs.prefix[1];
    st->rank[0] = cs.rank[0]; st->rank[1] = cs.rank[1];
    st->diverged = cs.two ? 1u : 0u;
    const float lo = key_f32(cs.prefix[0]), hi = key_f32(cs.prefix[1]);
    const MedianBw m = median_bandwidth(lo, hi, st->even, ln_n);
    st->lo = lo; st->hi = hi; st->median = m.med; st->h2 = m.h2;
    if (h2_out) *h2_out = m.h2;
    spec_update_dev(st, sp);
  }
}

// ================================================================================================
// host side: the staged calls (include/steinhip.h) and the fused call's select
// ================================================================================================
extern "C" int stein_median_begin(void* hist, void* select_state, int64_t total, void* stream) {
  if (!hist || !select_state) return fail(STEIN_E_BADARG, "NULL pointer");
  if (total < 1) return fail(STEIN_E_SHAPE, "total < 1");
  HIP_TRY(hipMemsetAsync(hist, 0, (size_t)STEIN_HIST_LEVELS * 2 * STEIN_HIST_BINS * 8, (hipStream_t)stream));
  hipLaunchKernelGGL(k_sel_init, dim3(1), dim3(64), 0, (hipStream_t)stream, (SelState*)select_state,
                     (u64)total);
  LAUNCH_CHECK("k_sel_init");
  return STEIN_OK;
}

template <int LEVEL>
static void launch_hist(bool sym, int blocks, hipStream_t s, const float* dist, long ld, int n_local, int n,
                        const SelState* st, u64* h, const u32* skip) {
  if (sym)
    hipLaunchKernelGGL((k_hist<LEVEL, true>), dim3(blocks), dim3(256), 0, s, dist, ld, n_local, n, st, h, skip);
  else
    hipLaunchKernelGGL((k_hist<LEVEL, false>), dim3(blocks), dim3(256), 0, s, dist, ld, n_local, n, st, h, skip);
}

extern "C" int stein_median_hist_pass(const float* dist, int64_t ld_dist, int64_t n_local, int64_t n, int level,
                                      const void* select_state, void* hist, int flags, void* stream) {
  if (!dist || !select_state || !hist) return fail(STEIN_E_BADARG, "NULL pointer");
  if (level < 0 || level >= STEIN_HIST_LEVELS) return fail(STEIN_E_BADARG, "level %d", level);
  if (ld_dist < n || (ld_dist & 31) || n_local < 1) return fail(STEIN_E_SHAPE, "bad distance block shape (ld_dist must be a multiple of 32)");
  const bool sym = (flags & STEIN_STAGE_SYMMETRIC) != 0;
  if (sym && n_local != n) return fail(STEIN_E_BADARG, "STEIN_STAGE_SYMMETRIC needs a square block");
  const long units = ((n_local + DT_ROWS - 1) / DT_ROWS) * ((n + DT_COLS - 1) / DT_COLS);   // [128][32] tiles
  const int blocks = (int)(units < HIST_BLOCKS ? units : HIST_BLOCKS);
  u64* h = (u64*)hist + (size_t)level * 2 * STEIN_HIST_BINS;
  const SelState* st = (const SelState*)select_state;
  hipStream_t s = (hipStream_t)stream;
  if (level == 0) launch_hist<0>(sym, blocks, s, dist, (long)ld_dist, (int)n_local, (int)n, st, h, nullptr);
  else if (level == 1) launch_hist<1>(sym, blocks, s, dist, (long)ld_dist, (int)n_local, (int)n, st, h, nullptr);
  else launch_hist<2>(sym, blocks, s, dist, (long)ld_dist, (int)n_local, (int)n, st, h, nullptr);
  LAUNCH_CHECK("k_hist");
  return STEIN_OK;
}

extern "C" int stein_median_resolve(const void* hist, int level, int64_t n, void* select_state, float* h2_out,
                                    float* median_out, void* stream) {
  if (!hist || !select_state) return fail(STEIN_E_BADARG, "NULL pointer");
  if (level < 0 || level >= STEIN_HIST_LEVELS) return fail(STEIN_E_BADARG, "level %d", level);
  if (n < 2) return fail(STEIN_E_BADARG, "n = %lld: need n >= 2", (long long)n);
  const u64* h = (const u64*)hist + (size_t)level * 2 * STEIN_HIST_BINS;
  const float ln_n = (float)log((double)n);  // np.log(n) in fp64, cast to fp32 by the tf.float32 graph
  hipLaunchKernelGGL(k_resolve, dim3(1), dim3(64), 0, (hipStream_t)stream, h, level, (SelState*)select_state, ln_n,
                     h2_out, median_out, nullptr);
  LAUNCH_CHECK("k_resolve");
  return STEIN_OK;
}

// ---- speculative window, staged form (several ranks; include/steinhip.h) -------------------------------------------
extern "C" int stein_spec_begin(void* hist, void* select_state, void* spec_buf, int64_t total, void* stream) {
  if (!hist || !select_state || !spec_buf) return fail(STEIN_E_BADARG, "NULL pointer");
  if (total < 1) return fail(STEIN_E_SHAPE, "total < 1");
  hipLaunchKernelGGL(k_median_init, dim3(16), dim3(256), 0, (hipStream_t)stream, (SelState*)select_state,
                     spec_of(select_state), (u64)total, (u64*)hist, (u64*)spec_buf);
  LAUNCH_CHECK("k_median_init");
  return STEIN_OK;
}

extern "C" int stein_spec_tally(void* select_state, void* spec_buf, void* stream) {
  if (!select_state || !spec_buf) return fail(STEIN_E_BADARG, "NULL pointer");
  u64* table = spec_table_of(spec_buf);
  HIP_TRY(hipMemsetAsync(table, 0, (size_t)SPEC_TABLE * 8, (hipStream_t)stream));
  hipLaunchKernelGGL(k_spec_tally, dim3(256), dim3(256), 0, (hipStream_t)stream, spec_of(select_state),
                     (const u64*)spec_buf, table);
  LAUNCH_CHECK("k_spec_tally");
  return STEIN_OK;
}

extern "C" int stein_spec_pick(void* select_state, void* spec_buf, int64_t n, float* h2_out, float* median_out,
                               void* stream) {
  if (!select_state || !spec_buf) return fail(STEIN_E_BADARG, "NULL pointer");
  if (n < 2) return fail(STEIN_E_BADARG, "n = %lld: need n >= 2", (long long)n);
  hipLaunchKernelGGL(k_spec_pick, dim3(1), dim3(1024), 0, (hipStream_t)stream, (SelState*)select_state,
                     spec_of(select_state), (const u64*)spec_table_of(spec_buf), (float)log((double)n), h2_out,
                     median_out);
  LAUNCH_CHECK("k_spec_pick");
  return STEIN_OK;
}

extern "C" int stein_spec_update(void* select_state, void* stream) {
  if (!select_state) return fail(STEIN_E_BADARG, "NULL pointer");
  hipLaunchKernelGGL(k_spec_update, dim3(1), dim3(64), 0, (hipStream_t)stream, (const SelState*)select_state,
                     spec_of(select_state));
  LAUNCH_CHECK("k_spec_update");
  return STEIN_OK;
}

// test hooks (per calling thread; tests/test_gpu_spec.py): launch k_hist_all with this many workgroups instead of one per
// virtual workgroup (0 = default); stein_debug_raise_device_error (steinhip.hip) raises the error word as a kernel would
static thread_local int g_hist_all_grid = 0, g_hist_all_nvb = 0;
constexpr int SPEC_WARM_WGS = 255;
static thread_local int g_no_warm = 0;   // stein_debug_no_warm: 1 = the select launches without its warm slice
extern "C" int stein_debug_no_warm(int off) {
  if (off != 0 && off != 1) return fail(STEIN_E_BADARG, "off %d", off);
  g_no_warm = off;
  return STEIN_OK;
}
extern "C" int stein_debug_hist_all_grid(int blocks) {
  if (blocks < 0 || blocks > 65535) return fail(STEIN_E_BADARG, "blocks %d", blocks);
  g_hist_all_grid = blocks;
  return STEIN_OK;
}
extern "C" int stein_debug_hist_all_vblocks(int nvb) {   // (tuning aid: virtual workgroups per level, 0 = default)
  if (nvb < 0 || nvb > 65535) return fail(STEIN_E_BADARG, "nvb %d", nvb);
  g_hist_all_nvb = nvb;
  return STEIN_OK;
}

// ---- the fused call's select ----------------------------------------------------------------------------------------
int stein_fused_select(const StepViews& v, int64_t n, int64_t d, float* h2_out, const void* theta_all,
                       const void* score_all, bool want_maxima, bool* took_maxima, hipStream_t s) {
  // the window either yields the median now (spec->hit) or the radix-select passes below run; each of them
  // checks the flag on the device, so nothing here waits for the host
  const bool solo = n <= SOLO_MAX_N;   // small block: a miss is resolved inside k_spec_select, no histogram launches
  // the slice (k_spec_select): folded operand, fp32 inputs
  long warm4 = 0;
  int warm_wgs = 0, slice = SLICE_READ, ncg = 1, nrg = 1;
  const bool aligned = (((uintptr_t)theta_all | (uintptr_t)score_all) & 15u) == 0;
  *took_maxima = false;
  if (v.L.fold && !g_no_warm && theta_all && score_all && want_maxima) {
    // column maxima: column blocks x row groups, about SPEC_WARM_WGS workgroups (one per compute unit beside the select's).
    // A wave takes the rows of its slot (n / 16 slots) four at a time: the row groups are as few as make every wave's
    // rows a whole number of such rounds where n allows it -- a fifth row would be a second trip to memory for one load
    // (C3: 1024 slots -> 2 rounds of 128 groups, not 255 groups with a ragged tail) -- and fewer groups are fewer
    // same-address atomics per column
    const bool v4 = aligned && d % 4 == 0;
    slice = v4 ? SLICE_MAX16 : SLICE_MAX4;
    const int64_t cw = v4 ? 256 : 64;
    const int64_t blocks = (d + cw - 1) / cw, slots = (n + 15) / 16;
    const int64_t max_rg = SPEC_WARM_WGS / blocks > 0 ? SPEC_WARM_WGS / blocks : 1;
    const int64_t rounds = (slots + 4 * max_rg - 1) / (4 * max_rg);
    ncg = (int)blocks;
    nrg = (int)((slots + 4 * rounds - 1) / (4 * rounds));
    warm_wgs = ncg * nrg;
    *took_maxima = true;
  } else if (v.L.fold && !g_no_warm && theta_all && score_all && aligned) {
    // the pure reader: 16-byte boundaries only; one workgroup per 128 KB of a matrix, at most SPEC_WARM_WGS
    warm4 = (long)(n * d) >> 2;
    const long want = (warm4 + 8191) / 8192;
    warm_wgs = (int)(want < SPEC_WARM_WGS ? want : SPEC_WARM_WGS);
  }
  // (the slice's matrices in cmax's order: the score first)
  hipLaunchKernelGGL(k_spec_select, dim3(1 + warm_wgs), dim3(1024), 0, s, v.sel, v.spec, v.spec_buf, (float)log((double)n),
                     h2_out, 1, solo ? (const float*)v.D : (const float*)nullptr, (long)v.L.ld_dist, (int)n,
                     (const float4*)score_all, (const float4*)theta_all, warm4, slice, (int)d, v.cmax, (int)v.L.x3_dc, ncg, nrg);
  LAUNCH_CHECK("k_spec_select");
  if (solo) return STEIN_OK;
  // chained radix select, ONE launch whatever n (k_hist_all: in-launch level barriers that need no co-residency; it returns
  // at once when the window hit).  Level 0 comes from the distance epilogue unless this step had a window (then only a
  // miss needs it, and the launch takes it itself: SpecState::skip_l0).
  const HistFinal fin{v.sel, v.spec, h2_out, (float)log((double)n)};
  const long units = ((n + DT_ROWS - 1) / DT_ROWS) * ((n + DT_COLS - 1) / DT_COLS);
  // large blocks: as many virtual workgroups as the chip holds at once (the passes like many loads in flight, and a grid
  // beyond residency would leave the surplus to the thieves); small ones: 512 (measured at C2)
  long want = HIST_ALL_VBLOCKS;
  if (n > HIST_ALL_SMALL_N) {
    static int resident[MAX_DEVICES];   // per device, computed on first use (threads that race store the same value)
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    const bool cached = dev >= 0 && dev < MAX_DEVICES;
    int res = cached ? __atomic_load_n(&resident[dev], __ATOMIC_RELAXED) : 0;
    if (!res) {
      int per_cu = 0, ncu = 0;
      HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_hist_all, 256, 0));
      HIP_TRY(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
      const long r = (long)(per_cu > 0 ? per_cu : 4) * (ncu > 0 ? ncu : 256);
      res = (int)(r > HIST_BLOCKS ? HIST_BLOCKS : r);
      if (cached) __atomic_store_n(&resident[dev], res, __ATOMIC_RELAXED);
    }
    want = res;
  }
  if (g_hist_all_nvb > 0) want = g_hist_all_nvb;
  if (want > HS_NV) want = HS_NV;   // (HistSync::claim holds one flag per virtual workgroup)
  const int nvb = (int)(units < want ? units : want);
  const int blocks = g_hist_all_grid > 0 ? g_hist_all_grid : nvb;   // (test hook: any grid >= 1 must give the same median)
  u32* errword = nullptr;
  if (int rc = stein_device_error_word(&errword)) return rc;
  hipLaunchKernelGGL(k_hist_all, dim3(blocks), dim3(256), 0, s, (const float*)v.D, (long)v.L.ld_dist, (int)n,
                     (const SelState*)v.sel, v.hist, (const u32*)&v.spec->hit, (const u32*)&v.spec->skip_l0, fin, v.fuse,
                     (HistSync*)v.table, (u32)nvb, errword);
  LAUNCH_CHECK("k_hist_all");
  return STEIN_OK;
}
