// stein_predict_ranks.hip -- order statistics of the posterior predictive outputs: credible bands and the ensemble median per
// test point without the [n][batch] matrix (stein_predict_glm_ranks / stein_predict_bnn_ranks of include/steinhip.h).
// The forward passes, the plan and the argument checks are stein_predict.hip's own: this file includes that source up to its
// weight pass (STEIN_PREDICT_SHARED_ONLY), so a counted value is bit for bit the value pred holds, and it is built with the
// same flags.  A source of its own because it sums integer counts with atomics, which the summary kernels must not use.
#define STEIN_PREDICT_SHARED_ONLY
#include "stein_predict.hip"

// ---- order statistics of the outputs (stein_predict_*_ranks) ------------------------------------------------
// out[i][b] = the ranks[i]-th smallest of f_pb over the particles, by a radix select over the 32-bit keys f32_key(f) (every
// NaN mapped to the top key) that recomputes the forward pass once per level of at most PQ_BITS bits and never stores an
// output.  Per (row, rank) the workspace holds the key prefix found so far, the rank that remains among the outputs that
// share it, the first rank of the call with the same prefix (its "leader": ranks that share a prefix share one histogram,
// so the first level counts once whatever n_ranks is) and PQ_BINS totals, all [..][batch] with the row fastest.
// k_predict_ranks_narrow sets them up; then per level a counting kernel -- the geometry of the summary kernels, the forward
// pass above -- adds every output's digit to the totals of each leader whose prefix it matches, and k_predict_ranks_narrow
// picks each rank's digit from its leader's totals and zeroes them for the next level; after the last level it writes
// key_f32(prefix).
// Counting: a lane counts its own row into bytes of LDS words (ds_add, no return, no dependent chain; a counter array in
// registers indexed by the digit would go to scratch, a compare chain over 16 bins and 8 ranks costs more than the forward
// pass).  Lane t's counters start at word t * (R * bins / 4 + 1), an odd stride: 64 lanes on 64 banks.  Every PQ_FLUSH
// passes -- 15 * 16 = 240 <= 255 outputs, so no byte overflows -- and at the slice's end it adds the non-zero counters to the
// global totals with integer atomics: sums of integers, so neither the order nor the slicing can matter.
constexpr int PQ_BITS = 4, PQ_BINS = 1 << PQ_BITS;   // digit bits per level at most (the GLM calls may take 3: see the host side)
constexpr int PQ_FLUSH = 15;                       // passes between two flushes of the byte counters
constexpr int PQ_WORDS = 3 + PQ_BINS;              // workspace words per (row, rank): prefix, remaining rank, leader, totals
constexpr u32 PQ_NAN_KEY = 0xffffffffu;            // no number has it: the top key of a number is f32_key(+inf) = 0xff800000
static_assert(PQ_FLUSH * PR_PASS <= 255, "a byte counter overflows between flushes");

struct PredRanks { int r[STEIN_PRED_RANKS_MAX]; };

__device__ __forceinline__ u32 pq_key(float f) { return f != f ? PQ_NAN_KEY : f32_key(f); }

struct PredCount {
  u32* hist;                              // this lane's counters in LDS: [R][PQ_BINS / 4] words of four byte counters
  u32 prefix[STEIN_PRED_RANKS_MAX];
  u32 lead;                               // bit i: rank i is its own leader (0 for a row past the batch: it counts nothing)
  u32 mask;                               // the key bits above this level's digit
  u32 top;                                // the digit's largest value
  int shift, wpr;                         // the digit's lowest bit; LDS words per rank: a quarter of the level's bins
};

__device__ __forceinline__ void pq_begin(PredCount& pc, u32* hist_lds, const u32* __restrict__ st, int R, int B, int row,
                                         bool live, int shift, int width, int wpr, int t) {
  pc.hist = hist_lds + t * (R * wpr + 1);
  pc.shift = shift;
  pc.wpr = wpr;
  pc.top = (1u << width) - 1u;
  pc.mask = shift + width >= 32 ? 0u : ~0u << (shift + width);
  pc.lead = 0u;
#pragma unroll
  for (int i = 0; i < STEIN_PRED_RANKS_MAX; ++i) {
    pc.prefix[i] = 0u;
    if (i < R) {
      if (live) {
        pc.prefix[i] = st[(size_t)i * B + row];
        if (st[(size_t)(2 * R + i) * B + row] == (u32)i) pc.lead |= 1u << i;
      }
      for (int w = 0; w < wpr; ++w) pc.hist[i * wpr + w] = 0u;
    }
  }
}

__device__ __forceinline__ void pq_count(const PredCount& pc, float f) {
  const u32 key = pq_key(f);
  const u32 dg = (key >> pc.shift) & pc.top;
  const u32 inc = 1u << (8u * (dg & 3u));
  u32* h = pc.hist + (dg >> 2);
#pragma unroll
  for (int i = 0; i < STEIN_PRED_RANKS_MAX; ++i)
    if ((pc.lead >> i & 1u) && ((key ^ pc.prefix[i]) & pc.mask) == 0u) atomicAdd(h + i * pc.wpr, inc);
}

// the lane's non-zero counters added to the totals [R][PQ_BINS][B] and cleared
__device__ __forceinline__ void pq_flush(const PredCount& pc, int R, u32* __restrict__ tot, int B, int row) {
  for (int i = 0; i < R; ++i) {
    if (!(pc.lead >> i & 1u)) continue;
    for (int w = 0; w < pc.wpr; ++w) {
      const u32 v = pc.hist[i * pc.wpr + w];
      if (v == 0u) continue;
      pc.hist[i * pc.wpr + w] = 0u;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const u32 c = (v >> (8 * q)) & 255u;
        if (c) atomicAdd(tot + (size_t)(i * PQ_BINS + 4 * w + q) * B + row, c);
      }
    }
  }
}

// st: the call's workspace, [prefix | remaining | leader][R][B] then the totals [R][PQ_BINS][B].  The dynamic LDS continues
// k_predict_glm's: the X tile, the staged weights, then the counters [PR_ROWS][4 R + 1].
__global__ __launch_bounds__(256) void k_predict_glm_ranks(const float* __restrict__ theta, int n, int d, int kind, int output,
                                                           int w_col, int F, int fc, int ld, const float* __restrict__ X,
                                                           int B, int per, u32* __restrict__ st, int R, int shift, int width,
                                                           int wpr) {
  extern __shared__ float lds[];
  float* xs = lds;                   // [PR_ROWS][ld]
  float* ws = lds + PR_ROWS * ld;    // [fc][PR_PASS]
  const int t = threadIdx.x;
  const int row0 = blockIdx.x * PR_ROWS, row = row0 + t;
  const bool live = row < B;
  const int p_begin = blockIdx.y * per, p_end = min(n, p_begin + per);
  const bool sigmoid = kind == STEIN_GLM_LOGISTIC && output == STEIN_PRED_MEAN;
  u32* tot = st + (size_t)3 * R * B;
  PredCount pc;
  pq_begin(pc, reinterpret_cast<u32*>(ws + fc * PR_PASS), st, R, B, row, live, shift, width, wpr, t);
  pred_glm_slice(
      theta, d, w_col, F, fc, ld, X, B, row0, p_begin, p_end, xs, ws, t, [](int, int) {},
      [&](int p0, int k, float zz) {
        if (k == 0 && p0 > p_begin && ((p0 - p_begin) / PR_PASS) % PQ_FLUSH == 0) pq_flush(pc, R, tot, B, row);
        pq_count(pc, pred_glm_output(zz, sigmoid));
      });
  pq_flush(pc, R, tot, B, row);
}

template <int NIN>
__global__ __launch_bounds__(256) void k_predict_bnn_ranks(const float* __restrict__ theta, int n, int d, int H, PredCols c,
                                                           const float* __restrict__ X, int B, int per, u32* __restrict__ st,
                                                           int R, int shift, int width, int wpr) {
  __shared__ __attribute__((aligned(16))) float lw[PR_PASS * PR_BNN_PW<NIN>];
  __shared__ float lp[PR_PASS][4];
  extern __shared__ u32 hist_lds[];   // [PR_ROWS][4 R + 1]
  const int t = threadIdx.x;
  const int row = blockIdx.x * PR_ROWS + t;
  const bool live = row < B;
  const int p_begin = blockIdx.y * per, p_end = min(n, p_begin + per);
  float x[NIN];
#pragma unroll
  for (int f = 0; f < NIN; ++f) x[f] = live ? X[(size_t)row * NIN + f] : 0.f;
  u32* tot = st + (size_t)3 * R * B;
  PredCount pc;
  pq_begin(pc, hist_lds, st, R, B, row, live, shift, width, wpr, t);
  int since = 0;
  for (int p0 = p_begin; p0 < p_end; p0 += PR_PASS) {
    const int cnt = min(PR_PASS, p_end - p0);
    float z[PR_PASS];
#pragma unroll
    for (int k = 0; k < PR_PASS; ++k) z[k] = 0.f;
    pred_bnn_pass<NIN>(z, theta, d, H, c, x, p0, cnt, lw, lp, t, [](int) {});
#pragma unroll
    for (int k = 0; k < PR_PASS; ++k)
      if (k < cnt) pq_count(pc, z[k] + lp[k][0]);
    if (++since == PQ_FLUSH) {
      pq_flush(pc, R, tot, B, row);
      since = 0;
    }
  }
  pq_flush(pc, R, tot, B, row);
}

// One thread per row, all of its ranks.  width 0 (the call's first launch): prefix 0, the ranks asked for, every rank led by rank 0, totals zero.
// Otherwise each rank takes the digit at which its leader's running total passes the rank that remains; then the totals
// are zeroed and the leaders found again (the first rank with the same prefix).  After the last level (shift 0) the
// prefix is the key of the order statistic.  A level's digit is the key's bits [shift, shift + width).
__global__ __launch_bounds__(256) void k_predict_ranks_narrow(u32* __restrict__ st, int R, int B, int shift, int width,
                                                              PredRanks ranks, float* __restrict__ out) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= B) return;
  const size_t sB = (size_t)B;
  u32* prefix = st + row;
  u32* rem = prefix + (size_t)R * sB;
  u32* leader = rem + (size_t)R * sB;
  u32* tot = leader + (size_t)R * sB;
  u32 pf[STEIN_PRED_RANKS_MAX];
  const bool first_call = width == 0, last = !first_call && shift == 0;
#pragma unroll
  for (int i = 0; i < STEIN_PRED_RANKS_MAX; ++i) {
    pf[i] = 0u;
    if (i >= R) continue;
    if (first_call) {
      rem[i * sB] = (u32)ranks.r[i];
    } else {
      const u32* h = tot + (size_t)leader[i * sB] * PQ_BINS * sB;
      const int bins = 1 << width;
      u32 r = rem[i * sB], dg = (u32)(bins - 1);
      bool found = false;
      for (int b = 0; b < bins; ++b) {
        const u32 cb = h[b * sB];
        if (!found) {
          if (r < cb) {
            dg = (u32)b;
            found = true;
          } else {
            r -= cb;
          }
        }
      }
      pf[i] = prefix[i * sB] | dg << shift;
      rem[i * sB] = r;
    }
  }
#pragma unroll
  for (int i = 0; i < STEIN_PRED_RANKS_MAX; ++i) {
    if (i >= R) continue;
    if (last) {
      out[i * sB + row] = pf[i] == PQ_NAN_KEY ? __builtin_nanf("") : key_f32(pf[i]);
      continue;
    }
    u32 first = (u32)i;
#pragma unroll
    for (int j = STEIN_PRED_RANKS_MAX - 1; j >= 0; --j)
      if (j < i && pf[j] == pf[i]) first = (u32)j;
    prefix[i * sB] = pf[i];
    leader[i * sB] = first;
    for (int b = 0; b < PQ_BINS; ++b) tot[(size_t)(i * PQ_BINS + b) * sB] = 0u;
  }
}

// ---- weighted order statistics (stein_predict_*_ranks_weighted) --------------------------------------------------------
// The same select with every output adding its particle's mass m_p (a u32) in place of 1: out[i][b] is the smallest f_pb of
// a particle with m_p > 0 at which the running mass passes the target max(0, ceil(q_i M) - 1), M = sum m_p < 2^32.  All sums
// are integer sums, so everything the unweighted select promises carries over.  The masses of a pass's PR_PASS particles are
// staged beside the particle data and read at one address by every lane; a particle of mass 0 is skipped.  A lane's counters
// are whole words, [R][2^bits] of them and a word of padding (an odd stride): M < 2^32, so none can overflow and they are
// flushed once, at the slice's end.  The narrow step and the leaders are the unweighted call's own kernel, launched with
// ranks of zero; k_predict_wranks_targets then puts each level's target where that kernel put the rank.  The workspace is
// the unweighted call's behind a header of PQW_MPARTS 64-bit words: the partial sums of the masses that
// k_predict_wranks_msum leaves, and in the last word the poison flag -- M = 0 or M >= 2^32 (the masses are not trusted):
// the counting kernels then count nothing, every level takes its top digit, and the call ends on the NaN key.
constexpr int PQW_MPARTS = 64;   // the header's words: at most PQW_MPARTS - 1 workgroups of k_predict_wranks_msum, then the flag

struct PredLevels { double q[STEIN_PRED_RANKS_MAX]; };

__global__ __launch_bounds__(256) void k_predict_wranks_msum(const u32* __restrict__ masses, int n, u64* __restrict__ mpart) {
  __shared__ u64 sh[256];
  const int t = threadIdx.x;
  u64 a = 0;
  for (size_t p = (size_t)blockIdx.x * 256 + t; p < (size_t)n; p += (size_t)gridDim.x * 256) a += masses[p];
  sh[t] = a;
  for (int half = 128; half > 0; half >>= 1) {
    __syncthreads();
    if (t < half) sh[t] += sh[t + half];
  }
  if (t == 0) mpart[blockIdx.x] = sh[0];
}

// One thread per row, behind the first k_predict_ranks_narrow: the remaining target of every level, max(0, ceil(q M) - 1) by
// one fp64 multiply, M summed from the mparts partial sums; the first thread also writes the poison flag.
__global__ __launch_bounds__(256) void k_predict_wranks_targets(u32* __restrict__ st, int R, int B, PredLevels levels,
                                                                u64* __restrict__ mpart, int mparts) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= B) return;
  u64 M = 0;
  for (int g = 0; g < mparts; ++g) M += mpart[g];
  const bool poisoned = M == 0 || M >> 32 != 0;
  if (row == 0) mpart[PQW_MPARTS - 1] = poisoned ? 1u : 0u;
  u32* rem = st + (size_t)R * B + row;
  for (int i = 0; i < R; ++i) {
    const double c = ceil(levels.q[i] * (double)M);   // <= M < 2^32 unless the call is poisoned
    rem[(size_t)i * B] = (poisoned || c < 1.0) ? 0u : (u32)(c - 1.0);
  }
}

__device__ __forceinline__ void pqw_count(const PredCount& pc, float f, u32 m) {
  if (m == 0u) return;
  const u32 key = pq_key(f);
  u32* h = pc.hist + ((key >> pc.shift) & pc.top);
#pragma unroll
  for (int i = 0; i < STEIN_PRED_RANKS_MAX; ++i)
    if ((pc.lead >> i & 1u) && ((key ^ pc.prefix[i]) & pc.mask) == 0u) atomicAdd(h + i * pc.wpr, m);
}

// the lane's non-zero counters (pc.wpr = the level's bins: a word each) added to the totals [R][PQ_BINS][B]
__device__ __forceinline__ void pqw_flush(const PredCount& pc, int R, u32* __restrict__ tot, int B, int row) {
  for (int i = 0; i < R; ++i) {
    if (!(pc.lead >> i & 1u)) continue;
    for (int b = 0; b < pc.wpr; ++b) {
      const u32 v = pc.hist[i * pc.wpr + b];
      if (v) atomicAdd(tot + (size_t)(i * PQ_BINS + b) * B + row, v);
    }
  }
}

// The dynamic LDS: the X tile, the staged weights, the pass's PR_PASS masses, then the counters [PR_ROWS][R 2^bits + 1].
__global__ __launch_bounds__(256) void k_predict_glm_wranks(const float* __restrict__ theta, int n, int d, int kind, int output,
                                                            int w_col, int F, int fc, int ld, const float* __restrict__ X,
                                                            int B, int per, const u32* __restrict__ masses,
                                                            const u64* __restrict__ poison, u32* __restrict__ st, int R,
                                                            int shift, int width, int bins) {
  if (*poison) return;               // the whole grid: nothing is counted
  extern __shared__ float lds[];
  float* xs = lds;                   // [PR_ROWS][ld]
  float* ws = lds + PR_ROWS * ld;    // [fc][PR_PASS]
  u32* ml = reinterpret_cast<u32*>(ws + fc * PR_PASS);   // [PR_PASS]
  const int t = threadIdx.x;
  const int row0 = blockIdx.x * PR_ROWS, row = row0 + t;
  const bool live = row < B;
  const int p_begin = blockIdx.y * per, p_end = min(n, p_begin + per);
  const bool sigmoid = kind == STEIN_GLM_LOGISTIC && output == STEIN_PRED_MEAN;
  u32* tot = st + (size_t)3 * R * B;
  PredCount pc;
  pq_begin(pc, ml + PR_PASS, st, R, B, row, live, shift, width, bins, t);
  pred_glm_slice(
      theta, d, w_col, F, fc, ld, X, B, row0, p_begin, p_end, xs, ws, t,
      [&](int p0, int cnt) {
        if (t < PR_PASS) ml[t] = t < cnt ? masses[p0 + t] : 0u;
      },
      [&](int, int k, float zz) { pqw_count(pc, pred_glm_output(zz, sigmoid), ml[k]); });
  pqw_flush(pc, R, tot, B, row);
}

template <int NIN>
__global__ __launch_bounds__(256) void k_predict_bnn_wranks(const float* __restrict__ theta, int n, int d, int H, PredCols c,
                                                            const float* __restrict__ X, int B, int per,
                                                            const u32* __restrict__ masses, const u64* __restrict__ poison,
                                                            u32* __restrict__ st, int R, int shift, int width, int bins) {
  if (*poison) return;                // the whole grid: nothing is counted
  __shared__ __attribute__((aligned(16))) float lw[PR_PASS * PR_BNN_PW<NIN>];
  __shared__ float lp[PR_PASS][4];    // per particle: b2, two words of the likelihood (unused here), its mass (as bits)
  extern __shared__ u32 hist_lds[];   // [PR_ROWS][R 2^bits + 1]
  const int t = threadIdx.x;
  const int row = blockIdx.x * PR_ROWS + t;
  const bool live = row < B;
  const int p_begin = blockIdx.y * per, p_end = min(n, p_begin + per);
  float x[NIN];
#pragma unroll
  for (int f = 0; f < NIN; ++f) x[f] = live ? X[(size_t)row * NIN + f] : 0.f;
  u32* tot = st + (size_t)3 * R * B;
  PredCount pc;
  pq_begin(pc, hist_lds, st, R, B, row, live, shift, width, bins, t);
  for (int p0 = p_begin; p0 < p_end; p0 += PR_PASS) {
    const int cnt = min(PR_PASS, p_end - p0);
    float z[PR_PASS];
#pragma unroll
    for (int k = 0; k < PR_PASS; ++k) z[k] = 0.f;
    pred_bnn_pass<NIN>(z, theta, d, H, c, x, p0, cnt, lw, lp, t, [&](int k) { lp[k][3] = __uint_as_float(masses[p0 + k]); });
#pragma unroll
    for (int k = 0; k < PR_PASS; ++k)
      if (k < cnt) pqw_count(pc, z[k] + lp[k][0], __float_as_uint(lp[k][3]));
  }
  pqw_flush(pc, R, tot, B, row);
}

// ---- host side -----------------------------------------------------------------------------------------
static size_t predict_ranks_ws_bytes(int64_t batch, int64_t n_ranks) {
  return (size_t)batch * (size_t)n_ranks * PQ_WORDS * sizeof(u32);
}

extern "C" int stein_predict_ranks_workspace_bytes(int64_t n, int64_t batch, int64_t n_ranks, size_t* out_bytes) {
  if (!out_bytes) return stein_fail(STEIN_E_BADARG, "NULL pointer");
  if (n_ranks < 1) return stein_fail(STEIN_E_BADARG, "n_ranks %lld", (long long)n_ranks);
  if (n < 1 || batch < 1 || n > PR_COUNT_MAX || batch > PR_COUNT_MAX)
    return stein_fail(STEIN_E_SHAPE, "bad shape n=%lld batch=%lld", (long long)n, (long long)batch);
  if (n_ranks > STEIN_PRED_RANKS_MAX)
    return stein_fail(STEIN_E_UNSUPPORTED, "more than %d ranks per call", (int)STEIN_PRED_RANKS_MAX);
  *out_bytes = predict_ranks_ws_bytes(batch, n_ranks);
  return STEIN_OK;
}

// the checks of a ranks call that do not depend on the model, in the header's order: up to and including the shapes ...
static int predict_ranks_check(const float* theta, const float* X, const int64_t* ranks, int64_t n_ranks, const float* out,
                               int64_t n, int64_t d, int64_t batch, int64_t width, int output) {
  if (!theta || !X || !ranks || !out) return stein_fail(STEIN_E_BADARG, "NULL pointer");
  if (n_ranks < 1) return stein_fail(STEIN_E_BADARG, "n_ranks %lld", (long long)n_ranks);
  return predict_check(theta, X, nullptr, n, d, batch, width, output, out, nullptr, nullptr, nullptr,
                       PredWeights{false, nullptr, nullptr});
}

// ... and behind the model's own: the rank count, every rank, the workspace
static int predict_ranks_check_tail(const int64_t* ranks, int64_t n_ranks, int64_t n, int64_t batch, const void* workspace,
                                    size_t ws_bytes, PredRanks& pr) {
  if (n_ranks > STEIN_PRED_RANKS_MAX)
    return stein_fail(STEIN_E_UNSUPPORTED, "more than %d ranks per call", (int)STEIN_PRED_RANKS_MAX);
  for (int64_t i = 0; i < n_ranks; ++i) {
    if (ranks[i] < 0 || ranks[i] >= n)
      return stein_fail(STEIN_E_BADARG, "rank %lld is outside [0, %lld)", (long long)ranks[i], (long long)n);
    pr.r[i] = (int)ranks[i];
  }
  if (!workspace) return stein_fail(STEIN_E_WORKSPACE, "the ranks need a workspace (stein_predict_ranks_workspace_bytes)");
  const size_t need = predict_ranks_ws_bytes(batch, n_ranks);
  if (ws_bytes < need) return stein_fail(STEIN_E_WORKSPACE, "workspace too small: %zu < %zu bytes", ws_bytes, need);
  if ((uintptr_t)workspace % sizeof(u32)) return stein_fail(STEIN_E_WORKSPACE, "the workspace of a ranks call must be 4-byte aligned");
  return STEIN_OK;
}

static int predict_ranks_narrow(u32* st, int R, int64_t batch, int shift, int width, const PredRanks& pr, float* out,
                                hipStream_t s) {
  hipLaunchKernelGGL(k_predict_ranks_narrow, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, s, st, R, (int)batch, shift,
                     width, pr, out);
  LAUNCH_CHECK("k_predict_ranks_narrow");
  return STEIN_OK;
}

static thread_local int g_ranks_slices = 0;   // stein_debug_predict_ranks_slices: 0 = the slices of predict_plan

extern "C" int stein_debug_predict_ranks_slices(int slices) {
  if (slices < 0 || slices > PR_SLICE_CAP) return stein_fail(STEIN_E_BADARG, "slices %d", slices);
  g_ranks_slices = slices;
  return STEIN_OK;
}

// the grid of a ranks call: the summary calls' own plan, or the hook's slice count (no slice of less than one pass)
static PredPlan predict_ranks_plan(int64_t n, int64_t batch) {
  PredPlan p = predict_plan(n, batch);
  if (g_ranks_slices > 0) {
    const int64_t passes = (n + PR_PASS - 1) / PR_PASS;
    const int64_t s = g_ranks_slices < passes ? g_ranks_slices : passes;
    p.per = (int)((n + s - 1) / s);
    p.slices = (int)((n + p.per - 1) / p.per);
  }
  return p;
}

// the counters of a counting workgroup: per lane 2^bits bytes per rank and a word of padding (an odd stride)
static size_t predict_ranks_lds(int R, int bits) { return (size_t)PR_ROWS * (R * ((1 << bits) / 4) + 1) * sizeof(u32); }
constexpr size_t PQ_LDS_HALF_CU = 80 * 1024;   // two workgroups per CU fit below this

extern "C" int stein_predict_glm_ranks(const float* theta, int64_t n, int64_t d, int kind, int output, int64_t w_col,
                                       int64_t n_feats, const float* X, int64_t batch, const int64_t* ranks, int64_t n_ranks,
                                       float* out, void* workspace, size_t ws_bytes, void* stream) {
  if (int rc = predict_ranks_check(theta, X, ranks, n_ranks, out, n, d, batch, n_feats, output)) return rc;
  if (kind != STEIN_GLM_LINEAR && kind != STEIN_GLM_LOGISTIC) return stein_fail(STEIN_E_BADARG, "kind %d", kind);
  if (w_col < 0 || w_col + n_feats > d)
    return stein_fail(STEIN_E_SHAPE, "weights [%lld, %lld) do not fit d=%lld", (long long)w_col, (long long)(w_col + n_feats),
                      (long long)d);
  if (n_feats > PR_WIDTH_MAX) return stein_fail(STEIN_E_UNSUPPORTED, "more than 1024 features per particle");
  PredRanks pr = {};
  if (int rc = predict_ranks_check_tail(ranks, n_ranks, n, batch, workspace, ws_bytes, pr)) return rc;
  const PredPlan pl = predict_ranks_plan(n, batch);
  const int R = (int)n_ranks;
  const int fc = (int)(n_feats <= PR_FC ? n_feats : PR_FC);
  const int ld = fc | 1;
  // The X tile and the counters share the CU's 160 KiB.  With 4 bits a level, five or more ranks beside a wide tile leave
  // room for one workgroup per CU only, which doubled the call's time; 3 bits a level (11 levels instead of 8) halve the
  // counters and keep two.  Both give the same bits of the same order statistic.
  const size_t tile_bytes = ((size_t)PR_ROWS * ld + (size_t)fc * PR_PASS) * sizeof(float);
  const int bits = (tile_bytes + predict_ranks_lds(R, PQ_BITS) > PQ_LDS_HALF_CU &&
                    tile_bytes + predict_ranks_lds(R, PQ_BITS - 1) <= PQ_LDS_HALF_CU) ? PQ_BITS - 1 : PQ_BITS;
  const size_t lds_bytes = tile_bytes + predict_ranks_lds(R, bits);
  // up to 96.5 KB of dynamic LDS, past the default 64 KB: the attribute belongs to the function on one device (as in
  // stein_small_phi: a flag per device id; racing threads at worst set it twice)
  static bool attr_set[64] = {false};
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64 || !attr_set[dev]) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_predict_glm_ranks), hipFuncAttributeMaxDynamicSharedMemorySize,
                                100 * 1024));
    if (dev >= 0 && dev < 64) attr_set[dev] = true;
  }
  hipStream_t s = (hipStream_t)stream;
  u32* st = (u32*)workspace;
  if (int rc = predict_ranks_narrow(st, R, batch, 32, 0, pr, out, s)) return rc;
  for (int hi = 32; hi > 0;) {   // the key's bits from the top, `bits` at a time (the last level takes what is left)
    const int width = bits < hi ? bits : hi, shift = hi - width;
    hipLaunchKernelGGL(k_predict_glm_ranks, dim3((unsigned)pl.row_tiles, (unsigned)pl.slices), dim3(256), lds_bytes, s, theta,
                       (int)n, (int)d, kind, output, (int)w_col, (int)n_feats, fc, ld, X, (int)batch, pl.per, st, R, shift, width,
                       (1 << bits) / 4);
    LAUNCH_CHECK("k_predict_glm_ranks");
    if (int rc = predict_ranks_narrow(st, R, batch, shift, width, pr, out, s)) return rc;
    hi = shift;
  }
  return STEIN_OK;
}

extern "C" int stein_predict_bnn_ranks(const float* theta, int64_t n, int64_t d, int64_t n_in, int64_t n_hidden,
                                       const int64_t* cols, int output, const float* X, int64_t batch, const int64_t* ranks,
                                       int64_t n_ranks, float* out, void* workspace, size_t ws_bytes, void* stream) {
  if (!cols) return stein_fail(STEIN_E_BADARG, "NULL pointer");
  if (int rc = predict_ranks_check(theta, X, ranks, n_ranks, out, n, d, batch, n_hidden, output)) return rc;
  if (n_in < 1) return stein_fail(STEIN_E_SHAPE, "bad shape n_in=%lld", (long long)n_in);
  if (n_in > PR_NIN_MAX) return stein_fail(STEIN_E_UNSUPPORTED, "more than %d input features", PR_NIN_MAX);
  if (n_hidden > PR_WIDTH_MAX) return stein_fail(STEIN_E_UNSUPPORTED, "more than 1024 hidden units");
  if (int rc = predict_check_cols(cols, n_in, n_hidden, d)) return rc;
  PredRanks pr = {};
  if (int rc = predict_ranks_check_tail(ranks, n_ranks, n, batch, workspace, ws_bytes, pr)) return rc;
  const PredPlan pl = predict_ranks_plan(n, batch);
  const int R = (int)n_ranks;
  const PredCols c = {(int)cols[0], (int)cols[1], (int)cols[2], (int)cols[3], (int)cols[5]};
  const size_t lds_bytes = predict_ranks_lds(R, PQ_BITS);   // beside at most 24.8 KB of static LDS: below 64 KB, two per CU
  hipStream_t s = (hipStream_t)stream;
  u32* st = (u32*)workspace;
  if (int rc = predict_ranks_narrow(st, R, batch, 32, 0, pr, out, s)) return rc;
  for (int shift = 32 - PQ_BITS; shift >= 0; shift -= PQ_BITS) {
#define PQ_LAUNCH_BNN(NIN)                                                                                              \
  hipLaunchKernelGGL(k_predict_bnn_ranks<NIN>, dim3((unsigned)pl.row_tiles, (unsigned)pl.slices), dim3(256), lds_bytes, s, \
                     theta, (int)n, (int)d, (int)n_hidden, c, X, (int)batch, pl.per, st, R, shift, PQ_BITS, PQ_BINS / 4)
    if (n_in == 1) PQ_LAUNCH_BNN(1);
    else if (n_in == 2) PQ_LAUNCH_BNN(2);
    else if (n_in == 3) PQ_LAUNCH_BNN(3);
    else PQ_LAUNCH_BNN(4);
#undef PQ_LAUNCH_BNN
    LAUNCH_CHECK("k_predict_bnn_ranks");
    if (int rc = predict_ranks_narrow(st, R, batch, shift, PQ_BITS, pr, out, s)) return rc;
  }
  return STEIN_OK;
}

// ---- weighted order statistics: host side ---------------------------------------------------------------------
static size_t predict_wranks_ws_bytes(int64_t batch, int64_t n_levels) {
  return (size_t)PQW_MPARTS * sizeof(u64) + predict_ranks_ws_bytes(batch, n_levels);
}

extern "C" int stein_predict_ranks_weighted_workspace_bytes(int64_t n, int64_t batch, int64_t n_levels, size_t* out_bytes) {
  if (!out_bytes) return stein_fail(STEIN_E_BADARG, "NULL pointer");
  if (n_levels < 1) return stein_fail(STEIN_E_BADARG, "n_levels %lld", (long long)n_levels);
  if (n < 1 || batch < 1 || n > PR_COUNT_MAX || batch > PR_COUNT_MAX)
    return stein_fail(STEIN_E_SHAPE, "bad shape n=%lld batch=%lld", (long long)n, (long long)batch);
  if (n_levels > STEIN_PRED_RANKS_MAX)
    return stein_fail(STEIN_E_UNSUPPORTED, "more than %d levels per call", (int)STEIN_PRED_RANKS_MAX);
  *out_bytes = predict_wranks_ws_bytes(batch, n_levels);
  return STEIN_OK;
}

static thread_local int g_wranks_bits = 0;   // stein_debug_predict_ranks_weighted_bits: 0 = the rule of predict_wranks_bits

extern "C" int stein_debug_predict_ranks_weighted_bits(int bits) {
  if (bits < 0 || bits > PQ_BITS) return stein_fail(STEIN_E_BADARG, "bits %d", bits);
  g_wranks_bits = bits;
  return STEIN_OK;
}

// the word counters of a weighted counting workgroup: per lane 2^bits words per level and a word of padding
static size_t predict_wranks_lds(int R, int bits) { return (size_t)PR_ROWS * (R * (1 << bits) + 1) * sizeof(u32); }
constexpr size_t PQW_LDS_CU = 160 * 1024;   // what one workgroup can have: the CU's whole LDS
constexpr int PQW_CUS = 256;                // compute units of the card the rule below was measured on

// The digit width of a weighted call, or the hook's.  Measured (profiles/predict_wquantile_ab.txt): a call's time is its
// forward passes, ceil(32 / bits), times a pass's time, and a pass runs 1.9 times faster with two workgroups resident on a
// CU than with one, and no faster with more.  So: the width of the least passes / min(2, workgroups that fit a CU's LDS),
// the wider on a tie; a grid of no more workgroups than CUs has no second workgroup to place and takes the widest width
// that fits.  other_bytes: the LDS beside the counters (the GLM call's tile, the network call's static arrays).
static int predict_wranks_bits(int R, size_t other_bytes, int64_t workgroups) {
  if (g_wranks_bits > 0) return g_wranks_bits;
  int best = 1, best_cost = 1 << 30;
  for (int bits = PQ_BITS; bits >= 1; --bits) {
    const size_t lds = other_bytes + predict_wranks_lds(R, bits);
    if (lds > PQW_LDS_CU) continue;
    const int passes = (32 + bits - 1) / bits;
    const int cost = (workgroups > PQW_CUS && 2 * lds <= PQW_LDS_CU) ? passes : 2 * passes;
    if (cost < best_cost) {
      best = bits;
      best_cost = cost;
    }
  }
  return best;
}

// the checks of a weighted ranks call behind the model's own: the level count, every level, the workspace, the hook's width
static int predict_wranks_check_tail(const double* levels, int64_t n_levels, int64_t batch, const void* workspace,
                                     size_t ws_bytes, size_t lds_total, PredLevels& lv) {
  if (n_levels > STEIN_PRED_RANKS_MAX)
    return stein_fail(STEIN_E_UNSUPPORTED, "more than %d levels per call", (int)STEIN_PRED_RANKS_MAX);
  for (int64_t i = 0; i < n_levels; ++i) {
    if (!(levels[i] >= 0.0 && levels[i] <= 1.0)) return stein_fail(STEIN_E_BADARG, "level %g is outside [0, 1]", levels[i]);
    lv.q[i] = levels[i];
  }
  if (!workspace)
    return stein_fail(STEIN_E_WORKSPACE, "the weighted ranks need a workspace (stein_predict_ranks_weighted_workspace_bytes)");
  const size_t need = predict_wranks_ws_bytes(batch, n_levels);
  if (ws_bytes < need) return stein_fail(STEIN_E_WORKSPACE, "workspace too small: %zu < %zu bytes", ws_bytes, need);
  if ((uintptr_t)workspace % sizeof(u64))
    return stein_fail(STEIN_E_WORKSPACE, "the workspace of a weighted ranks call must be 8-byte aligned");
  if (lds_total > PQW_LDS_CU)
    return stein_fail(STEIN_E_UNSUPPORTED, "%d-bit digits need %zu bytes of LDS, more than a CU has", g_wranks_bits, lds_total);
  return STEIN_OK;
}

// past the default 64 KB of LDS a kernel needs the attribute, which belongs to the function on one device (as above);
// lds_dynamic: the most the kernel can be given beside its static LDS
static int predict_wranks_attr(const void* fn, int slot, size_t lds_dynamic) {
  static bool attr_set[5][64] = {{false}};
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64 || !attr_set[slot][dev]) {
    HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_dynamic));
    if (dev >= 0 && dev < 64) attr_set[slot][dev] = true;
  }
  return STEIN_OK;
}

// the partial sums of the masses, the first narrow launch (every level led by level 0), then the targets from the levels
static int predict_wranks_setup(const u32* masses, int64_t n, u64* mpart, u32* st, int R, int64_t batch, const PredLevels& lv,
                                float* out, hipStream_t s) {
  const int64_t blocks = (n + 255) / 256;
  const int mparts = (int)(blocks < PQW_MPARTS - 1 ? blocks : PQW_MPARTS - 1);
  hipLaunchKernelGGL(k_predict_wranks_msum, dim3((unsigned)mparts), dim3(256), 0, s, masses, (int)n, mpart);
  LAUNCH_CHECK("k_predict_wranks_msum");
  if (int rc = predict_ranks_narrow(st, R, batch, 32, 0, PredRanks{}, out, s)) return rc;
  hipLaunchKernelGGL(k_predict_wranks_targets, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, s, st, R, (int)batch, lv,
                     mpart, mparts);
  LAUNCH_CHECK("k_predict_wranks_targets");
  return STEIN_OK;
}

extern "C" int stein_predict_glm_ranks_weighted(const float* theta, int64_t n, int64_t d, int kind, int output, int64_t w_col,
                                                int64_t n_feats, const float* X, int64_t batch, const uint32_t* masses,
                                                const double* levels, int64_t n_levels, float* out, void* workspace,
                                                size_t ws_bytes, void* stream) {
  if (!theta || !X || !masses || !levels || !out) return stein_fail(STEIN_E_BADARG, "NULL pointer");
  if (n_levels < 1) return stein_fail(STEIN_E_BADARG, "n_levels %lld", (long long)n_levels);
  if (int rc = predict_check(theta, X, nullptr, n, d, batch, n_feats, output, out, nullptr, nullptr, nullptr,
                             PredWeights{false, nullptr, nullptr}))
    return rc;
  if (kind != STEIN_GLM_LINEAR && kind != STEIN_GLM_LOGISTIC) return stein_fail(STEIN_E_BADARG, "kind %d", kind);
  if (w_col < 0 || w_col + n_feats > d)
    return stein_fail(STEIN_E_SHAPE, "weights [%lld, %lld) do not fit d=%lld", (long long)w_col, (long long)(w_col + n_feats),
                      (long long)d);
  if (n_feats > PR_WIDTH_MAX) return stein_fail(STEIN_E_UNSUPPORTED, "more than 1024 features per particle");
  const int R = (int)(n_levels < STEIN_PRED_RANKS_MAX ? n_levels : STEIN_PRED_RANKS_MAX);
  const int fc = (int)(n_feats <= PR_FC ? n_feats : PR_FC);
  const int ld = fc | 1;
  const size_t tile_bytes = ((size_t)PR_ROWS * ld + (size_t)fc * PR_PASS + PR_PASS) * sizeof(float);   // X, weights, masses
  const PredPlan pl = predict_ranks_plan(n, batch);
  const int bits = predict_wranks_bits(R, tile_bytes, (int64_t)pl.row_tiles * pl.slices);
  const size_t lds_bytes = tile_bytes + predict_wranks_lds(R, bits);
  PredLevels lv = {};
  if (int rc = predict_wranks_check_tail(levels, n_levels, batch, workspace, ws_bytes, lds_bytes, lv)) return rc;
  if (int rc = predict_wranks_attr(reinterpret_cast<const void*>(k_predict_glm_wranks), 0, PQW_LDS_CU)) return rc;
  hipStream_t s = (hipStream_t)stream;
  u64* mpart = (u64*)workspace;
  u32* st = (u32*)(mpart + PQW_MPARTS);
  if (int rc = predict_wranks_setup(masses, n, mpart, st, R, batch, lv, out, s)) return rc;
  for (int hi = 32; hi > 0;) {   // the key's bits from the top, `bits` at a time (the last level takes what is left)
    const int width = bits < hi ? bits : hi, shift = hi - width;
    hipLaunchKernelGGL(k_predict_glm_wranks, dim3((unsigned)pl.row_tiles, (unsigned)pl.slices), dim3(256), lds_bytes, s, theta,
                       (int)n, (int)d, kind, output, (int)w_col, (int)n_feats, fc, ld, X, (int)batch, pl.per, masses, mpart + PQW_MPARTS - 1,
                       st, R, shift, width, 1 << bits);
    LAUNCH_CHECK("k_predict_glm_wranks");
    if (int rc = predict_ranks_narrow(st, R, batch, shift, width, PredRanks{}, out, s)) return rc;
    hi = shift;
  }
  return STEIN_OK;
}

extern "C" int stein_predict_bnn_ranks_weighted(const float* theta, int64_t n, int64_t d, int64_t n_in, int64_t n_hidden,
                                                const int64_t* cols, int output, const float* X, int64_t batch,
                                                const uint32_t* masses, const double* levels, int64_t n_levels, float* out,
                                                void* workspace, size_t ws_bytes, void* stream) {
  if (!cols) return stein_fail(STEIN_E_BADARG, "NULL pointer");
  if (!theta || !X || !masses || !levels || !out) return stein_fail(STEIN_E_BADARG, "NULL pointer");
  if (n_levels < 1) return stein_fail(STEIN_E_BADARG, "n_levels %lld", (long long)n_levels);
  if (int rc = predict_check(theta, X, nullptr, n, d, batch, n_hidden, output, out, nullptr, nullptr, nullptr,
                             PredWeights{false, nullptr, nullptr}))
    return rc;
  if (n_in < 1) return stein_fail(STEIN_E_SHAPE, "bad shape n_in=%lld", (long long)n_in);
  if (n_in > PR_NIN_MAX) return stein_fail(STEIN_E_UNSUPPORTED, "more than %d input features", PR_NIN_MAX);
  if (n_hidden > PR_WIDTH_MAX) return stein_fail(STEIN_E_UNSUPPORTED, "more than 1024 hidden units");
  if (int rc = predict_check_cols(cols, n_in, n_hidden, d)) return rc;
  const int R = (int)(n_levels < STEIN_PRED_RANKS_MAX ? n_levels : STEIN_PRED_RANKS_MAX);
  const PredPlan pl = predict_ranks_plan(n, batch);
  const size_t lds_static = ((size_t)PR_PASS * (n_in + 2) * PR_HC + PR_PASS * 4) * sizeof(float);   // lw and lp: at most 24.8 KB
  const int bits = predict_wranks_bits(R, lds_static, (int64_t)pl.row_tiles * pl.slices);
  const size_t lds_bytes = predict_wranks_lds(R, bits);
  PredLevels lv = {};
  if (int rc = predict_wranks_check_tail(levels, n_levels, batch, workspace, ws_bytes, lds_static + lds_bytes, lv)) return rc;
  const PredCols c = {(int)cols[0], (int)cols[1], (int)cols[2], (int)cols[3], (int)cols[5]};
  hipStream_t s = (hipStream_t)stream;
  u64* mpart = (u64*)workspace;
  u32* st = (u32*)(mpart + PQW_MPARTS);
  const void* fn = n_in == 1   ? reinterpret_cast<const void*>(k_predict_bnn_wranks<1>)
                   : n_in == 2 ? reinterpret_cast<const void*>(k_predict_bnn_wranks<2>)
                   : n_in == 3 ? reinterpret_cast<const void*>(k_predict_bnn_wranks<3>)
                               : reinterpret_cast<const void*>(k_predict_bnn_wranks<4>);
  if (int rc = predict_wranks_attr(fn, (int)n_in, PQW_LDS_CU - lds_static)) return rc;
  if (int rc = predict_wranks_setup(masses, n, mpart, st, R, batch, lv, out, s)) return rc;
  for (int hi = 32; hi > 0;) {
    const int width = bits < hi ? bits : hi, shift = hi - width;
#define PQW_LAUNCH_BNN(NIN)                                                                                              \
  hipLaunchKernelGGL(k_predict_bnn_wranks<NIN>, dim3((unsigned)pl.row_tiles, (unsigned)pl.slices), dim3(256), lds_bytes, s, \
                     theta, (int)n, (int)d, (int)n_hidden, c, X, (int)batch, pl.per, masses, mpart + PQW_MPARTS - 1, st, R, shift, width, \
                     1 << bits)
    if (n_in == 1) PQW_LAUNCH_BNN(1);
    else if (n_in == 2) PQW_LAUNCH_BNN(2);
    else if (n_in == 3) PQW_LAUNCH_BNN(3);
    else PQW_LAUNCH_BNN(4);
#undef PQW_LAUNCH_BNN
    LAUNCH_CHECK("k_predict_bnn_wranks");
    if (int rc = predict_ranks_narrow(st, R, batch, shift, width, PredRanks{}, out, s)) return rc;
    hi = shift;
  }
  return STEIN_OK;
}

// ---- masses from weights (stein_predict_rank_masses) ---------------------------------------------------------------
// weights [n] in fp64 -> masses [n] in u32 for the weighted calls above.  STEIN_MASS_NORMALISED: m_p = rint(w_p / W 2^31),
// the quotient in fp64, W the sum of the weights in an order that n alone fixes (PM_BLOCKS strided partial sums folded by
// halving, then the partials folded the same way); STEIN_MASS_COUNTS: m_p = w_p, every weight an integer below 2^32 and
// their sum too.  A negative or non-finite weight, W = 0 or an overflow turns W into NaN: every mass 0, info[0] = NaN.
// No atomic anywhere.  Workspace: per workgroup one double (its part of W) and two u64 (its part of M and of the count).
constexpr int PM_BLOCKS = 256;

__device__ __forceinline__ double pm_fold(double* sh, int t) {   // 256 values folded by halving, in a fixed order
  for (int half = 128; half > 0; half >>= 1) {
    __syncthreads();
    if (t < half) sh[t] += sh[t + half];
  }
  __syncthreads();
  return sh[0];
}

__global__ __launch_bounds__(256) void k_rank_masses_wsum(const double* __restrict__ wts, int n, int counts,
                                                          double* __restrict__ wpart) {
  __shared__ double sh[256];
  const int t = threadIdx.x;
  double a = 0.0;
  bool bad = false;
  for (size_t p = (size_t)blockIdx.x * 256 + t; p < (size_t)n; p += (size_t)gridDim.x * 256) {
    const double v = wts[p];
    bad = bad || !(v >= 0.0 && v < (double)INFINITY) || (counts && (v >= 4294967296.0 || v != floor(v)));
    a += v;
  }
  sh[t] = bad ? (double)NAN : a;
  const double sum = pm_fold(sh, t);
  if (t == 0) wpart[blockIdx.x] = sum;
}

__global__ __launch_bounds__(256) void k_rank_masses_write(const double* __restrict__ wts, int n, int counts, int blocks,
                                                           const double* __restrict__ wpart, u32* __restrict__ masses,
                                                           u64* __restrict__ mpart) {
  __shared__ double sh[256];
  __shared__ u64 shm[2][256];
  const int t = threadIdx.x;
  sh[t] = t < blocks ? wpart[t] : 0.0;
  double W = pm_fold(sh, t);
  if (!(W > 0.0 && W < (counts ? 4294967296.0 : (double)INFINITY))) W = (double)NAN;
  u64 msum = 0, live = 0;
  for (size_t p = (size_t)blockIdx.x * 256 + t; p < (size_t)n; p += (size_t)gridDim.x * 256) {
    u32 m = 0u;
    if (W == W) m = counts ? (u32)wts[p] : (u32)rint(wts[p] / W * 2147483648.0);
    masses[p] = m;
    msum += m;
    live += m != 0u;
  }
  shm[0][t] = msum; shm[1][t] = live;
  for (int half = 128; half > 0; half >>= 1) {
    __syncthreads();
    if (t < half) {
      shm[0][t] += shm[0][t + half];
      shm[1][t] += shm[1][t + half];
    }
  }
  if (t == 0) {
    mpart[2 * blockIdx.x] = shm[0][0];
    mpart[2 * blockIdx.x + 1] = shm[1][0];
  }
}

__global__ __launch_bounds__(64) void k_rank_masses_info(int blocks, const double* __restrict__ wpart,
                                                         const u64* __restrict__ mpart, double* __restrict__ info) {
  if (threadIdx.x != 0) return;
  bool bad = false;
  u64 M = 0, live = 0;
  for (int b = 0; b < blocks; ++b) {
    bad = bad || wpart[b] != wpart[b];
    M += mpart[2 * b];
    live += mpart[2 * b + 1];
  }
  info[0] = (bad || M == 0) ? (double)NAN : (double)M;
  info[1] = (double)live;
}

static int rank_masses_blocks(int64_t n) {
  const int64_t b = (n + 255) / 256;
  return (int)(b < PM_BLOCKS ? b : PM_BLOCKS);
}

extern "C" int stein_predict_rank_masses_workspace_bytes(int64_t n, size_t* out_bytes) {
  if (!out_bytes) return stein_fail(STEIN_E_BADARG, "NULL pointer");
  if (n < 1 || n > PR_COUNT_MAX) return stein_fail(STEIN_E_SHAPE, "bad shape n=%lld", (long long)n);
  *out_bytes = (size_t)rank_masses_blocks(n) * 3 * sizeof(double);
  return STEIN_OK;
}

extern "C" int stein_predict_rank_masses(const double* weights, int64_t n, int mode, uint32_t* masses, double* info,
                                         void* workspace, size_t ws_bytes, void* stream) {
  if (!weights || !masses || !info) return stein_fail(STEIN_E_BADARG, "NULL pointer");
  if (mode != STEIN_MASS_NORMALISED && mode != STEIN_MASS_COUNTS) return stein_fail(STEIN_E_BADARG, "mode %d", mode);
  if (n < 1 || n > PR_COUNT_MAX) return stein_fail(STEIN_E_SHAPE, "bad shape n=%lld", (long long)n);
  if (!workspace) return stein_fail(STEIN_E_WORKSPACE, "the masses need a workspace (stein_predict_rank_masses_workspace_bytes)");
  const int blocks = rank_masses_blocks(n);
  const size_t need = (size_t)blocks * 3 * sizeof(double);
  if (ws_bytes < need) return stein_fail(STEIN_E_WORKSPACE, "workspace too small: %zu < %zu bytes", ws_bytes, need);
  if ((uintptr_t)workspace % sizeof(double)) return stein_fail(STEIN_E_WORKSPACE, "the workspace of the masses must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  double* wpart = (double*)workspace;
  u64* mpart = (u64*)(wpart + blocks);
  const int counts = mode == STEIN_MASS_COUNTS ? 1 : 0;
  hipLaunchKernelGGL(k_rank_masses_wsum, dim3((unsigned)blocks), dim3(256), 0, s, weights, (int)n, counts, wpart);
  LAUNCH_CHECK("k_rank_masses_wsum");
  hipLaunchKernelGGL(k_rank_masses_write, dim3((unsigned)blocks), dim3(256), 0, s, weights, (int)n, counts, blocks, wpart, masses, mpart);
  LAUNCH_CHECK("k_rank_masses_write");
  hipLaunchKernelGGL(k_rank_masses_info, dim3(1), dim3(64), 0, s, blocks, wpart, mpart, info);
  LAUNCH_CHECK("k_rank_masses_info");
  return STEIN_OK;
}
