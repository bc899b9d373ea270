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
