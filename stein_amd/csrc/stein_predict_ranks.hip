// stein_predict_ranks.hip -- order statistics of the posterior predictive outputs: credible bands and the ensemble median per
// test point without the [n][batch] matrix (stein_predict_glm_ranks / stein_predict_bnn_ranks of include/steinhip.h).
// The forward passes, the plan and the argument checks are the summary kernels' own (stein_predict_fwd.h, which
// stein_predict.hip includes too), so a counted value is bit for bit the value pred holds, and this file is built with the
// same flags.  A source of its own because it sums integer counts with atomics, which the summary kernels must not use.
// One counting kernel per model, k_predict_glm_ranks<MASS, ..> and k_predict_bnn_ranks<NIN, MASS, ..>: MASS = false counts
// every output as 1 (stein_predict_*_ranks), MASS = true adds its particle's integer mass (stein_predict_*_ranks_weighted).
#include "stein_predict_fwd.h"

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

// ---- the counters of a lane and the counting kernels, both selects ----------------------------------------------------------
// MASS = false: four byte counters to an LDS word (pc.wpr = a quarter of the level's bins), the output counts 1.
// MASS = true: a word per bin (pc.wpr = the level's bins), the output adds its particle's mass m; mass 0 is skipped.
template <bool MASS>
__device__ __forceinline__ void pq_count(const PredCount& pc, float f, u32 m) {
  if (MASS && m == 0u) return;
  const u32 key = pq_key(f);
  const u32 dg = (key >> pc.shift) & pc.top;
  const u32 inc = MASS ? m : 1u << (8u * (dg & 3u));
  u32* h = pc.hist + (MASS ? dg : dg >> 2);
#pragma unroll
  for (int i = 0; i < STEIN_PRED_RANKS_MAX; ++i)
    if ((pc.lead >> i & 1u) && ((key ^ pc.prefix[i]) & pc.mask) == 0u) atomicAdd(h + i * pc.wpr, inc);
}

// the lane's non-zero counters added to the totals [R][PQ_BINS][B]; the byte counters are flushed more than once and cleared
template <bool MASS>
__device__ __forceinline__ void pq_flush(const PredCount& pc, int R, u32* __restrict__ tot, int B, int row) {
  for (int i = 0; i < R; ++i) {
    if (!(pc.lead >> i & 1u)) continue;
    for (int w = 0; w < pc.wpr; ++w) {
      const u32 v = pc.hist[i * pc.wpr + w];
      if (v == 0u) continue;
      if constexpr (MASS) {
        atomicAdd(tot + (size_t)(i * PQ_BINS + w) * B + row, v);
      } else {
        pc.hist[i * pc.wpr + w] = 0u;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const u32 c = (v >> (8 * q)) & 255u;
          if (c) atomicAdd(tot + (size_t)(i * PQ_BINS + 4 * w + q) * B + row, c);
        }
      }
    }
  }
}

// the two arguments a counting kernel takes with MASS only (restrict, as kernel arguments are throughout), and their
// accessors out of the kernel's pack (nothing in it: the unweighted kernel)
using PredMasses = const u32* __restrict__;
using PredPoison = const u64* __restrict__;
__device__ __forceinline__ const u32* pq_masses(const u32* masses, const u64*) { return masses; }
__device__ __forceinline__ const u32* pq_masses() { return nullptr; }
__device__ __forceinline__ const u64* pq_poison(const u32*, const u64* poison) { return poison; }

// st: the call's select state, [prefix | remaining | leader][R][B] then the totals [R][PQ_BINS][B].  The dynamic LDS continues
// k_predict_glm's: the X tile, the staged weights, with MASS the pass's PR_PASS masses, then the counters [PR_ROWS][R wpr + 1].
// Mass...: with MASS (PredMasses masses [n], PredPoison poison -- the flag of the workspace's header: the whole grid counts
// nothing), without it no argument at all.  A pack and not two pointers that the unweighted kernels would carry unused, and
// `if constexpr` wherever MASS decides, so that an instantiation names nothing of the other's: with either the generated
// prologue changes, and a prologue two to eight instructions longer cost the GLM kernel 0.5 to 2.7 % of its time
// (profiles/predict_ranks_unify_ab.txt, C).  For the same reason the unweighted counters' address is formed where it is used.
template <bool MASS, class... Mass>
__global__ __launch_bounds__(256) void k_predict_glm_ranks(const float* __restrict__ theta, int n, int d, int kind, int output,
                                                           int w_col, int F, int fc, int ld, const float* __restrict__ X,
                                                           int B, int per, Mass... mass, u32* __restrict__ st, int R,
                                                           int shift, int width, int wpr) {
  static_assert(sizeof...(Mass) == (MASS ? 2 : 0), "masses and poison with MASS, nothing without");
  const u32* __restrict__ masses = pq_masses(mass...);
  if constexpr (MASS) {
    if (*pq_poison(mass...)) return;
  }
  extern __shared__ float lds[];
  float* xs = lds;                   // [PR_ROWS][ld]
  float* ws = lds + PR_ROWS * ld;    // [fc][PR_PASS]
  u32* ml = MASS ? reinterpret_cast<u32*>(ws + fc * PR_PASS) : nullptr;   // [PR_PASS], MASS only
  const int t = threadIdx.x;
  const int row0 = blockIdx.x * PR_ROWS, row = row0 + t;
  const bool live = row < B;
  const int p_begin = blockIdx.y * per, p_end = min(n, p_begin + per);
  const bool sigmoid = kind == STEIN_GLM_LOGISTIC && output == STEIN_PRED_MEAN;
  u32* tot = st + (size_t)3 * R * B;
  PredCount pc;
  pq_begin(pc, MASS ? ml + PR_PASS : reinterpret_cast<u32*>(ws + fc * PR_PASS), st, R, B, row, live, shift, width, wpr, t);
  pred_glm_slice(
      theta, d, w_col, F, fc, ld, X, B, row0, p_begin, p_end, xs, ws, t,
      [&](int p0, int cnt) {
        if constexpr (MASS) {
          if (t < PR_PASS) ml[t] = t < cnt ? masses[p0 + t] : 0u;
        }
      },
      [&](int p0, int k, float zz) {
        if constexpr (!MASS) {   // the byte counters, every PQ_FLUSH passes
          if (k == 0 && p0 > p_begin && ((p0 - p_begin) / PR_PASS) % PQ_FLUSH == 0) pq_flush<MASS>(pc, R, tot, B, row);
        }
        const float f = pred_glm_output(zz, sigmoid);
        if constexpr (MASS) pq_count<MASS>(pc, f, ml[k]);
        else pq_count<MASS>(pc, f, 0u);
      });
  pq_flush<MASS>(pc, R, tot, B, row);
}

// The counters [PR_ROWS][R wpr + 1] are the dynamic LDS; with MASS a particle's mass travels as the bits of lp[k][3].
template <int NIN, bool MASS, class... Mass>
__global__ __launch_bounds__(256) void k_predict_bnn_ranks(const float* __restrict__ theta, int n, int d, int H, PredCols c,
                                                           const float* __restrict__ X, int B, int per, Mass... mass,
                                                           u32* __restrict__ st, int R, int shift, int width, int wpr) {
  static_assert(sizeof...(Mass) == (MASS ? 2 : 0), "masses and poison with MASS, nothing without");
  const u32* __restrict__ masses = pq_masses(mass...);
  if constexpr (MASS) {
    if (*pq_poison(mass...)) return;
  }
  __shared__ __attribute__((aligned(16))) float lw[PR_PASS * PR_BNN_PW<NIN>];
  __shared__ float lp[PR_PASS][4];    // per particle: b2, two words of the likelihood (unused here), MASS: its mass
  extern __shared__ u32 hist_lds[];
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
  int since = 0;   // passes since the byte counters' last flush
  for (int p0 = p_begin; p0 < p_end; p0 += PR_PASS) {
    const int cnt = min(PR_PASS, p_end - p0);
    float z[PR_PASS];
#pragma unroll
    for (int k = 0; k < PR_PASS; ++k) z[k] = 0.f;
    pred_bnn_pass<NIN>(z, theta, d, H, c, x, p0, cnt, lw, lp, t, [&](int k) {
      if constexpr (MASS) lp[k][3] = __uint_as_float(masses[p0 + k]);
    });
#pragma unroll
    for (int k = 0; k < PR_PASS; ++k)
      if (k < cnt) {
        if constexpr (MASS) pq_count<MASS>(pc, z[k] + lp[k][0], __float_as_uint(lp[k][3]));
        else pq_count<MASS>(pc, z[k] + lp[k][0], 0u);
      }
    if constexpr (!MASS) {
      if (++since == PQ_FLUSH) {
        pq_flush<MASS>(pc, R, tot, B, row);
        since = 0;
      }
    }
  }
  pq_flush<MASS>(pc, R, tot, B, row);
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

// the weighted select's header: up to PQW_MPARTS - 1 workgroups leave the partial sums of the masses, folded by halving
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

// the counters of a counting workgroup: per lane and rank 2^bits bytes, or with masses 2^bits words, and per lane a word of
// padding (an odd stride)
static int predict_ranks_wpr(int bits, bool mass) { return mass ? 1 << bits : (1 << bits) / 4; }
static size_t predict_ranks_lds(int R, int bits, bool mass) {
  return (size_t)PR_ROWS * (R * predict_ranks_wpr(bits, mass) + 1) * sizeof(u32);
}
constexpr size_t PQ_LDS_HALF_CU = 80 * 1024;   // two workgroups per CU fit below this
constexpr size_t PQW_LDS_CU = 160 * 1024;   // what one workgroup can have: the CU's whole LDS
constexpr int PQW_CUS = 256;                // compute units of the card the rule below was measured on
// the network kernels' static LDS, lw and lp: at most 24.8 KB
static size_t predict_bnn_lds_static(int64_t n_in) { return ((size_t)PR_PASS * (n_in + 2) * PR_HC + PR_PASS * 4) * sizeof(float); }

static thread_local int g_wranks_bits = 0;   // stein_debug_predict_ranks_weighted_bits: 0 = the rule of predict_wranks_bits

extern "C" int stein_debug_predict_ranks_weighted_bits(int bits) {
  if (bits < 0 || bits > PQ_BITS) return stein_fail(STEIN_E_BADARG, "bits %d", bits);
  g_wranks_bits = bits;
  return STEIN_OK;
}

// The digit width of a weighted call, or the hook's.  Measured (profiles/predict_wquantile_ab.txt): a call's time is its
// forward passes, ceil(32 / bits), times a pass's time, and a pass runs 1.9 times faster with two workgroups resident on a
// CU than with one, and no faster with more.  So: the width of the least passes / min(2, workgroups that fit a CU's LDS),
// the wider on a tie; a grid of no more workgroups than CUs has no second workgroup to place and takes the widest width
// that fits.  other_bytes: the LDS beside the counters (the GLM call's tile, the network call's static arrays).
static int predict_wranks_bits(int R, size_t other_bytes, int64_t workgroups) {
  if (g_wranks_bits > 0) return g_wranks_bits;
  int best = 1, best_cost = 1 << 30;
  for (int bits = PQ_BITS; bits >= 1; --bits) {
    const size_t lds = other_bytes + predict_ranks_lds(R, bits, true);
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

// the checks of a weighted ranks call that do not depend on the model: up to and including the shapes ...
static int predict_wranks_check(const float* theta, const float* X, const uint32_t* masses, const double* levels,
                                int64_t n_levels, const float* out, int64_t n, int64_t d, int64_t batch, int64_t width,
                                int output) {
  if (!theta || !X || !masses || !levels || !out) return stein_fail(STEIN_E_BADARG, "NULL pointer");
  if (n_levels < 1) return stein_fail(STEIN_E_BADARG, "n_levels %lld", (long long)n_levels);
  return predict_check(theta, X, nullptr, n, d, batch, width, output, out, nullptr, nullptr, nullptr,
                       PredWeights{false, nullptr, nullptr});
}

// ... and behind the model's own: the level count, every level, the workspace, the hook's width
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

// ---- the launches of a call past its checks, both selects -------------------------------------------------------------------
// masses = nullptr: the unweighted call -- its ranks in pr, the workspace is the select's state st.  Otherwise the weighted
// call: pr is zero, lv holds its levels, and st lies behind the workspace's header mpart.
struct PredSelect {
  const u32* masses;
  u64* mpart;
  u32* st;
  int R, bits;
  size_t lds_bytes;   // the counting kernel's dynamic LDS
  PredRanks pr;
  PredLevels lv;
  float* out;
  int wpr() const { return predict_ranks_wpr(bits, masses != nullptr); }
};

// Past the default 64 KB of LDS a kernel needs the attribute, which belongs to the function on one device (as in
// stein_small_phi: a flag per device id; racing threads at worst set it twice).  slot: 0 and 1 the GLM kernel without and
// with masses, 1 + n_in the network kernels with masses; lds_dynamic: the most the kernel can be given beside its static LDS.
static int predict_ranks_attr(const void* fn, int slot, size_t lds_dynamic) {
  static bool attr_set[2 + PR_NIN_MAX][64] = {{false}};
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64 || !attr_set[slot][dev]) {
    HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_dynamic));
    if (dev >= 0 && dev < 64) attr_set[slot][dev] = true;
  }
  return STEIN_OK;
}

static int predict_ranks_narrow(const PredSelect& q, int64_t batch, int shift, int width, hipStream_t s) {
  hipLaunchKernelGGL(k_predict_ranks_narrow, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, s, q.st, q.R, (int)batch,
                     shift, width, q.pr, q.out);
  LAUNCH_CHECK("k_predict_ranks_narrow");
  return STEIN_OK;
}

// The first narrow launch (every rank led by rank 0) -- in a weighted call behind the partial sums of the masses and ahead of
// the targets from the levels -- then the key's bits from the top, `bits` at a time (the last level takes what is left):
// count(shift, width) launches the model's counting kernel for one level, and the narrow step is queued behind it.
template <class Count>
static int predict_ranks_run(const PredSelect& q, int64_t n, int64_t batch, hipStream_t s, Count&& count) {
  const int64_t blocks = (n + 255) / 256;
  const int mparts = (int)(blocks < PQW_MPARTS - 1 ? blocks : PQW_MPARTS - 1);
  if (q.masses) {
    hipLaunchKernelGGL(k_predict_wranks_msum, dim3((unsigned)mparts), dim3(256), 0, s, q.masses, (int)n, q.mpart);
    LAUNCH_CHECK("k_predict_wranks_msum");
  }
  if (int rc = predict_ranks_narrow(q, batch, 32, 0, s)) return rc;
  if (q.masses) {
    hipLaunchKernelGGL(k_predict_wranks_targets, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, s, q.st, q.R, (int)batch,
                       q.lv, q.mpart, mparts);
    LAUNCH_CHECK("k_predict_wranks_targets");
  }
  for (int hi = 32; hi > 0;) {
    const int width = q.bits < hi ? q.bits : hi, shift = hi - width;
    if (int rc = count(shift, width)) return rc;
    if (int rc = predict_ranks_narrow(q, batch, shift, width, s)) return rc;
    hi = shift;
  }
  return STEIN_OK;
}

// mass...: what the counting kernel takes in its pack -- nothing (the unweighted call), or the masses and the poison flag
template <class... Mass>
static int predict_glm_select(const float* theta, int64_t n, int64_t d, int kind, int output, int64_t w_col, int64_t n_feats,
                              const float* X, int64_t batch, const PredPlan& pl, const PredGlmTile& tile, const PredSelect& q,
                              hipStream_t s, Mass... mass) {
  constexpr bool MASS = sizeof...(Mass) != 0;
  const auto kernel = k_predict_glm_ranks<MASS, Mass...>;
  // the byte counters beside the tile: up to 96.5 KB of dynamic LDS; the word counters: whatever the CU has
  if (int rc = predict_ranks_attr(reinterpret_cast<const void*>(kernel), MASS ? 1 : 0, MASS ? PQW_LDS_CU : 100 * 1024)) return rc;
  return predict_ranks_run(q, n, batch, s, [&](int shift, int width) -> int {
    hipLaunchKernelGGL(kernel, dim3((unsigned)pl.row_tiles, (unsigned)pl.slices), dim3(256), q.lds_bytes, s, theta, (int)n,
                       (int)d, kind, output, (int)w_col, (int)n_feats, tile.fc, tile.ld, X, (int)batch, pl.per, mass..., q.st,
                       q.R, shift, width, q.wpr());
    LAUNCH_CHECK("k_predict_glm_ranks");
    return STEIN_OK;
  });
}

template <class... Mass>
static int predict_bnn_select(const float* theta, int64_t n, int64_t d, int64_t n_in, int64_t n_hidden, const int64_t* cols,
                              const float* X, int64_t batch, const PredPlan& pl, const PredSelect& q, hipStream_t s,
                              Mass... mass) {
  constexpr bool MASS = sizeof...(Mass) != 0;
  using Kernel = decltype(&k_predict_bnn_ranks<1, MASS, Mass...>);
  static const Kernel kernels[PR_NIN_MAX] = {k_predict_bnn_ranks<1, MASS, Mass...>, k_predict_bnn_ranks<2, MASS, Mass...>,
                                             k_predict_bnn_ranks<3, MASS, Mass...>, k_predict_bnn_ranks<4, MASS, Mass...>};
  const Kernel kernel = kernels[n_in - 1];
  // the byte counters stay below the default 64 KB beside the static LDS (two workgroups per CU): no attribute
  if (MASS)
    if (int rc = predict_ranks_attr(reinterpret_cast<const void*>(kernel), 1 + (int)n_in, PQW_LDS_CU - predict_bnn_lds_static(n_in)))
      return rc;
  const PredCols c = predict_cols(cols);
  return predict_ranks_run(q, n, batch, s, [&](int shift, int width) -> int {
    hipLaunchKernelGGL(kernel, dim3((unsigned)pl.row_tiles, (unsigned)pl.slices), dim3(256), q.lds_bytes, s, theta, (int)n,
                       (int)d, (int)n_hidden, c, X, (int)batch, pl.per, mass..., q.st, q.R, shift, width, q.wpr());
    LAUNCH_CHECK("k_predict_bnn_ranks");
    return STEIN_OK;
  });
}

extern "C" int stein_predict_glm_ranks(const float* theta, int64_t n, int64_t d, int kind, int output, int64_t w_col,
                                       int64_t n_feats, const float* X, int64_t batch, const int64_t* ranks, int64_t n_ranks,
                                       float* out, void* workspace, size_t ws_bytes, void* stream) {
  if (int rc = predict_ranks_check(theta, X, ranks, n_ranks, out, n, d, batch, n_feats, output)) return rc;
  if (int rc = predict_check_glm(kind, w_col, n_feats, d)) return rc;
  PredRanks pr = {};
  if (int rc = predict_ranks_check_tail(ranks, n_ranks, n, batch, workspace, ws_bytes, pr)) return rc;
  const int R = (int)n_ranks;
  const PredGlmTile tile = predict_glm_tile(n_feats, false);
  // The X tile and the counters share the CU's 160 KiB.  With 4 bits a level, five or more ranks beside a wide tile leave
  // room for one workgroup per CU only, which doubled the call's time; 3 bits a level (11 levels instead of 8) halve the
  // counters and keep two.  Both give the same bits of the same order statistic.
  const int bits = (tile.bytes + predict_ranks_lds(R, PQ_BITS, false) > PQ_LDS_HALF_CU &&
                    tile.bytes + predict_ranks_lds(R, PQ_BITS - 1, false) <= PQ_LDS_HALF_CU) ? PQ_BITS - 1 : PQ_BITS;
  const PredSelect q = {nullptr, nullptr, (u32*)workspace, R, bits, tile.bytes + predict_ranks_lds(R, bits, false), pr, {}, out};
  return predict_glm_select(theta, n, d, kind, output, w_col, n_feats, X, batch, predict_ranks_plan(n, batch), tile, q,
                            (hipStream_t)stream);
}

extern "C" int stein_predict_bnn_ranks(const float* theta, int64_t n, int64_t d, int64_t n_in, int64_t n_hidden,
                                       const int64_t* cols, int output, const float* X, int64_t batch, const int64_t* ranks,
                                       int64_t n_ranks, float* out, void* workspace, size_t ws_bytes, void* stream) {
  if (!cols) return stein_fail(STEIN_E_BADARG, "NULL pointer");
  if (int rc = predict_ranks_check(theta, X, ranks, n_ranks, out, n, d, batch, n_hidden, output)) return rc;
  if (int rc = predict_check_bnn(n_in, n_hidden, cols, d)) return rc;
  PredRanks pr = {};
  if (int rc = predict_ranks_check_tail(ranks, n_ranks, n, batch, workspace, ws_bytes, pr)) return rc;
  const int R = (int)n_ranks;
  const PredSelect q = {nullptr, nullptr, (u32*)workspace, R, PQ_BITS, predict_ranks_lds(R, PQ_BITS, false), pr, {}, out};
  return predict_bnn_select(theta, n, d, n_in, n_hidden, cols, X, batch, predict_ranks_plan(n, batch), q, (hipStream_t)stream);
}

extern "C" int stein_predict_glm_ranks_weighted(const float* theta, int64_t n, int64_t d, int kind, int output, int64_t w_col,
                                                int64_t n_feats, const float* X, int64_t batch, const uint32_t* masses,
                                                const double* levels, int64_t n_levels, float* out, void* workspace,
                                                size_t ws_bytes, void* stream) {
  if (int rc = predict_wranks_check(theta, X, masses, levels, n_levels, out, n, d, batch, n_feats, output)) return rc;
  if (int rc = predict_check_glm(kind, w_col, n_feats, d)) return rc;
  const int R = (int)(n_levels < STEIN_PRED_RANKS_MAX ? n_levels : STEIN_PRED_RANKS_MAX);
  const PredGlmTile tile = predict_glm_tile(n_feats, true);   // X, weights, masses
  const PredPlan pl = predict_ranks_plan(n, batch);
  const int bits = predict_wranks_bits(R, tile.bytes, (int64_t)pl.row_tiles * pl.slices);
  const size_t lds_bytes = tile.bytes + predict_ranks_lds(R, bits, true);
  PredLevels lv = {};
  if (int rc = predict_wranks_check_tail(levels, n_levels, batch, workspace, ws_bytes, lds_bytes, lv)) return rc;
  u64* mpart = (u64*)workspace;
  const PredSelect q = {masses, mpart, (u32*)(mpart + PQW_MPARTS), R, bits, lds_bytes, {}, lv, out};
  return predict_glm_select<PredMasses, PredPoison>(theta, n, d, kind, output, w_col, n_feats, X, batch, pl, tile, q,
                                                    (hipStream_t)stream, masses, mpart + PQW_MPARTS - 1);
}

extern "C" int stein_predict_bnn_ranks_weighted(const float* theta, int64_t n, int64_t d, int64_t n_in, int64_t n_hidden,
                                                const int64_t* cols, int output, const float* X, int64_t batch,
                                                const uint32_t* masses, const double* levels, int64_t n_levels, float* out,
                                                void* workspace, size_t ws_bytes, void* stream) {
  if (!cols) return stein_fail(STEIN_E_BADARG, "NULL pointer");
  if (int rc = predict_wranks_check(theta, X, masses, levels, n_levels, out, n, d, batch, n_hidden, output)) return rc;
  if (int rc = predict_check_bnn(n_in, n_hidden, cols, d)) return rc;
  const int R = (int)(n_levels < STEIN_PRED_RANKS_MAX ? n_levels : STEIN_PRED_RANKS_MAX);
  const PredPlan pl = predict_ranks_plan(n, batch);
  const size_t lds_static = predict_bnn_lds_static(n_in);
  const int bits = predict_wranks_bits(R, lds_static, (int64_t)pl.row_tiles * pl.slices);
  const size_t lds_bytes = predict_ranks_lds(R, bits, true);
  PredLevels lv = {};
  if (int rc = predict_wranks_check_tail(levels, n_levels, batch, workspace, ws_bytes, lds_static + lds_bytes, lv)) return rc;
  u64* mpart = (u64*)workspace;
  const PredSelect q = {masses, mpart, (u32*)(mpart + PQW_MPARTS), R, bits, lds_bytes, {}, lv, out};
  return predict_bnn_select<PredMasses, PredPoison>(theta, n, d, n_in, n_hidden, cols, X, batch, pl, q, (hipStream_t)stream,
                                                    masses, mpart + PQW_MPARTS - 1);
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
