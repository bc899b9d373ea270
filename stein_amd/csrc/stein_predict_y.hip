// stein_predict_y.hip -- the predictive distribution of y, observation noise included (stein_predict_*_ycdf and
// stein_predict_*_yquantiles of include/steinhip.h): the Gaussian mixture over the particles
//   F_b(t) = sum_p w_p Phi((t - z_pb) sqrt(tau_p)) / W
// evaluated at given points (the probability integral transform, the mass of an interval) and inverted at given levels
// (predictive intervals) without the [n][batch] matrix.  Both are reductions across particles of a per-(particle, row)
// transcendental, so the mapping is the summary kernels': rows on the lanes, a workgroup per (row tile, particle slice), the
// forward passes of stein_predict_fwd.h -- z_pb is bit for bit what pred holds -- a partial result per (slice, row) in the
// workspace and a finish kernel that merges the slices in slice order in fp64.  No atomic anywhere.
//
// One forward kernel per model, in three modes:
//   PY_CDF      A = n_pts running sums of w Phi((t_i - z) s) per lane, s = sqrt(tau)
//   PY_BRACKET  per level the least and the largest widened component quantile z + c_i / s (c_i = Phi^-1(level_i), from the host)
//   PY_REFINE   per level the sums at the PY_K interior points of the row's bracket [lo, hi] (py_point): 7 A running sums
// A pass's PR_PASS linear outputs go through the lane's own 16 words of LDS (zs[k][lane]) and are consumed by a loop over k
// that is NOT unrolled: unrolled, the up to 56 erfcf of a particle would be laid out 16 times, far past the instruction
// cache.  The sums are indexed statically (registers); the points of PY_REFINE are formed where they are used.
// The weights are the weighted summaries': the weight pass of stein_predict.hip (predict_weight_pass) leaves W in the
// workspace's header and the lanes hold pred_norm_weight(w_p, W); a particle of weight zero is skipped.  Without weights
// every particle counts 1 and the finish kernels divide by n.
#include "stein_predict_fwd.h"

constexpr int PY_K = 7;                                  // interior points of a bracket per refinement pass: eight sub-intervals
constexpr int PY_LEVELS = STEIN_PRED_RANKS_MAX;          // levels per call, and points per call (STEIN_PRED_Y_POINTS_MAX)
constexpr int PY_ACC_MAX = PY_LEVELS * PY_K;             // running sums of a lane at most
constexpr int64_t PY_PART_FLOATS = (int64_t)1 << 23;     // the partial sums of a call: the slice count is cut down to fit them
constexpr int PY_ROUND_WGS = 512;                        // workgroups of one round: two resident on each of 256 CUs
constexpr float PY_WIDEN = 4.76837158203125e-07f;        // 2^-21: what a component quantile is moved outward by, relatively
constexpr float PY_RSQRT2 = 0.70710678118654752440f;
static_assert(STEIN_PRED_Y_POINTS_MAX == PY_LEVELS, "one lane state serves points and levels");
enum { PY_CDF = 0, PY_BRACKET = 1, PY_REFINE = 2 };

struct PyConsts { float c[PY_LEVELS]; };      // PY_BRACKET: Phi^-1(level_i)
struct PyLevels { double q[PY_LEVELS]; };     // the levels themselves, for the finish kernel's comparison

__device__ __forceinline__ float py_phi(float x) { return 0.5f * erfcf(-PY_RSQRT2 * x); }

// interior point j (1 .. PY_K) of [lo, hi]: one rounding of lo + (hi - lo) j / 8, so monotone in j, never below lo and, by
// the min, never above hi; the forward kernel and the finish kernel both call this, so they name the same floats
__device__ __forceinline__ float py_point(float lo, float hi, int j) {
  return fminf(fmaf(hi - lo, 0.125f * (float)j, lo), hi);
}

template <int MODE>
struct PyLane {
  static constexpr int NA = MODE == PY_REFINE ? PY_ACC_MAX : MODE == PY_BRACKET ? 2 * PY_LEVELS : PY_LEVELS;
  float acc[NA];
  float u[PY_LEVELS], v[PY_LEVELS];   // PY_CDF: u = t_i of the row; PY_BRACKET: u = c_i; PY_REFINE: [u, v] = the bracket
  int A;                              // points or levels of the call
};

// words of the workspace per (slice, row)
__host__ __device__ constexpr int py_words(int mode, int A) { return mode == PY_REFINE ? PY_K * A : mode == PY_BRACKET ? 2 * A : A; }

// pts: PY_CDF t [A][B]; PY_REFINE the brackets [2][A][B] (lo, then hi); a row past the batch evaluates at 0 and stores nothing
template <int MODE>
__device__ __forceinline__ void py_begin(PyLane<MODE>& ln, const float* __restrict__ pts, const PyConsts& cs, int A, int B,
                                         int row, bool live) {
  ln.A = A;
#pragma unroll
  for (int i = 0; i < PyLane<MODE>::NA; ++i) ln.acc[i] = 0.f;
#pragma unroll
  for (int i = 0; i < PY_LEVELS; ++i) {
    ln.u[i] = ln.v[i] = 0.f;
    if (i >= A) continue;
    if constexpr (MODE == PY_CDF) {
      if (live) ln.u[i] = pts[(size_t)i * B + row];
    } else if constexpr (MODE == PY_BRACKET) {
      ln.u[i] = cs.c[i];
      ln.acc[2 * i] = INFINITY;
      ln.acc[2 * i + 1] = -INFINITY;
    } else {
      if (live) {
        ln.u[i] = pts[(size_t)i * B + row];
        ln.v[i] = pts[(size_t)(A + i) * B + row];
      }
    }
  }
}

// one particle: its linear output f, s = sqrt(tau), rs = 1 / s, and (WEIGHTED) its normalised weight w, lane-uniform
template <int MODE, bool WEIGHTED>
__device__ __forceinline__ void py_add(PyLane<MODE>& ln, float f, float s, float rs, float w) {
#pragma unroll
  for (int i = 0; i < PY_LEVELS; ++i) {
    if (i >= ln.A) continue;
    if constexpr (MODE == PY_CDF) {
      const float ph = py_phi((ln.u[i] - f) * s);
      ln.acc[i] = WEIGHTED ? fmaf(w, ph, ln.acc[i]) : ln.acc[i] + ph;
    } else if constexpr (MODE == PY_BRACKET) {
      const float o = ln.u[i] * rs;
      const float cq = f + o, m = PY_WIDEN * (fabsf(f) + fabsf(o));
      ln.acc[2 * i] = fminf(ln.acc[2 * i], cq - m);
      ln.acc[2 * i + 1] = fmaxf(ln.acc[2 * i + 1], cq + m);
    } else {
#pragma unroll
      for (int j = 0; j < PY_K; ++j) {
        const float ph = py_phi((py_point(ln.u[i], ln.v[i], j + 1) - f) * s);
        ln.acc[i * PY_K + j] = WEIGHTED ? fmaf(w, ph, ln.acc[i * PY_K + j]) : ln.acc[i * PY_K + j] + ph;
      }
    }
  }
}

// part [slice][py_words][B], the row fastest
template <int MODE>
__device__ __forceinline__ void py_store(const PyLane<MODE>& ln, float* __restrict__ part, int slice, int B, int row) {
  constexpr int per_level = MODE == PY_REFINE ? PY_K : MODE == PY_BRACKET ? 2 : 1;
  float* p = part + (size_t)slice * py_words(MODE, ln.A) * B + row;
#pragma unroll
  for (int i = 0; i < PY_LEVELS; ++i) {
    if (i >= ln.A) continue;
#pragma unroll
    for (int j = 0; j < per_level; ++j) p[(size_t)(i * per_level + j) * B] = ln.acc[i * per_level + j];
  }
}

// The dynamic LDS continues k_predict_glm's: the X tile, a pass's staged weights, then the normalised weights of two passes
// [2][PR_PASS] and the lanes' linear outputs of a pass zs [PR_PASS][256].  A pass's outputs are consumed one pass later, in
// the slot pred_glm_slice leaves between the barriers of the next pass's first chunk (and after the slice's last pass): one
// site in the code and not one per unrolled k.  So the weights alternate between two rows: the threads that stage a pass's
// weights may run ahead of the lanes that still read the previous pass's.  zs is each lane's own: no lane reads another's.
template <int MODE, bool WEIGHTED>
__global__ __launch_bounds__(256) void k_predict_glm_y(const float* __restrict__ theta, int n, int d, int w_col, int F, int fc,
                                                       int ld, const float* __restrict__ X, int B, int per, float s, float rs,
                                                       const float* __restrict__ pts, PyConsts cs, int A,
                                                       float* __restrict__ part, const double* __restrict__ wts,
                                                       const double* __restrict__ head) {
  extern __shared__ float lds[];
  float* xs = lds;                    // [PR_ROWS][ld]
  float* ws = lds + PR_ROWS * ld;     // [fc][PR_PASS]
  float* wl = ws + fc * PR_PASS;      // [2][PR_PASS], read WEIGHTED only
  float* zs = wl + 2 * PR_PASS;       // [PR_PASS][256]
  const double wtot = WEIGHTED ? head[0] : 0.0;
  const int t = threadIdx.x;
  const int row0 = blockIdx.x * PR_ROWS, row = row0 + t;
  const bool live = row < B;
  const int p_begin = blockIdx.y * per, p_end = min(n, p_begin + per);
  PyLane<MODE> ln;
  py_begin(ln, pts, cs, A, B, row, live);
  int held = 0, parity = 0;   // outputs of the previous pass waiting in zs, and the row of wl their weights lie in
  auto drain = [&]() __attribute__((always_inline)) {   // (as a call, the lane's sums would travel through scratch)
    const float* wrow = wl + parity * PR_PASS;
#pragma unroll 1
    for (int k = 0; k < held; ++k) {
      const float w = WEIGHTED ? wrow[k] : 1.f;
      if (WEIGHTED && !(w > 0.f)) continue;
      py_add<MODE, WEIGHTED>(ln, zs[k * 256 + t], s, rs, w);
    }
  };
  pred_glm_slice(
      theta, d, w_col, F, fc, ld, X, B, row0, p_begin, p_end, xs, ws, t,
      [&](int p0, int cnt) {
        drain();
        parity ^= 1;
        held = cnt;
        if (WEIGHTED && t < PR_PASS) wl[parity * PR_PASS + t] = t < cnt ? pred_norm_weight(wts[p0 + t], wtot) : 0.f;
      },
      [&](int, int k, float zz) { zs[k * 256 + t] = zz; });
  __syncthreads();   // the last pass's weights, staged by other threads
  drain();
  if (live) py_store(ln, part, blockIdx.y, B, row);
}

// ls per particle of the pass: sqrt(tau_p) = sqrt(exp(lg_p)), its reciprocal, and (WEIGHTED) the normalised weight
template <int NIN, int MODE, bool WEIGHTED>
__global__ __launch_bounds__(256) void k_predict_bnn_y(const float* __restrict__ theta, int n, int d, int H, PredCols c,
                                                       const float* __restrict__ X, int B, int per,
                                                       const float* __restrict__ pts, PyConsts cs, int A,
                                                       float* __restrict__ part, const double* __restrict__ wts,
                                                       const double* __restrict__ head) {
  __shared__ __attribute__((aligned(16))) float lw[PR_PASS * PR_BNN_PW<NIN>];
  __shared__ float lp[PR_PASS][4];        // per particle: b2, 1/2 lg - 1/2 log 2 pi (unused here), 1/2 e^lg
  __shared__ float ls[PR_PASS][4];        // sqrt(e^lg), 1 / sqrt(e^lg), the normalised weight
  __shared__ float zs[PR_PASS * 256];
  const double wtot = WEIGHTED ? head[0] : 0.0;
  const int t = threadIdx.x;
  const int row = blockIdx.x * PR_ROWS + t;
  const bool live = row < B;
  const int p_begin = blockIdx.y * per, p_end = min(n, p_begin + per);
  float x[NIN];
#pragma unroll
  for (int f = 0; f < NIN; ++f) x[f] = live ? X[(size_t)row * NIN + f] : 0.f;
  PyLane<MODE> ln;
  py_begin(ln, pts, cs, A, B, row, live);
  for (int p0 = p_begin; p0 < p_end; p0 += PR_PASS) {
    const int cnt = min(PR_PASS, p_end - p0);
    float z[PR_PASS];
#pragma unroll
    for (int k = 0; k < PR_PASS; ++k) z[k] = 0.f;
    pred_bnn_pass<NIN>(z, theta, d, H, c, x, p0, cnt, lw, lp, t, [&](int k) {
      const float sk = sqrtf(2.f * lp[k][2]);   // lp[k][2] = 1/2 e^lg, just staged by this thread: the doubling is exact
      ls[k][0] = sk;
      ls[k][1] = 1.f / sk;
      ls[k][2] = WEIGHTED ? pred_norm_weight(wts[p0 + k], wtot) : 1.f;
    });
#pragma unroll
    for (int k = 0; k < PR_PASS; ++k) zs[k * 256 + t] = z[k] + lp[k][0];   // k >= cnt: never read
#pragma unroll 1
    for (int k = 0; k < cnt; ++k) {
      const float w = ls[k][2];
      if (WEIGHTED && !(w > 0.f)) continue;
      py_add<MODE, WEIGHTED>(ln, zs[k * 256 + t], ls[k][0], ls[k][1], w);
    }
  }
  if (live) py_store(ln, part, blockIdx.y, B, row);
}

// ---- the finish kernels: the slices merged in slice order, in fp64 --------------------------------------------------------
// head: the weight pass's header of a weighted call (head[0] = W, NaN for bad weights: NaN rows), or NULL: the sums are
// divided by n.
// PY_CDF: one thread per (point, row)
__global__ __launch_bounds__(256) void k_predict_y_finish_cdf(const float* __restrict__ part, int slices, int n, int B, int A,
                                                              float* __restrict__ out, const double* __restrict__ head) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)A * B) return;
  double sum = 0.0;
  for (int s = 0; s < slices; ++s) sum += (double)part[(size_t)s * A * B + idx];
  if (head) out[idx] = head[0] > 0.0 ? (float)sum : __builtin_nanf("");
  else out[idx] = (float)(sum / (double)n);
}

// PY_BRACKET: one thread per (level, row): the least and the largest over the slices (a slice without a live particle left
// +inf and -inf, which change nothing) into the brackets br [2][A][B]
__global__ __launch_bounds__(256) void k_predict_y_finish_bracket(const float* __restrict__ part, int slices, int B, int A,
                                                                  float* __restrict__ br, const double* __restrict__ head) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)A * B) return;
  const int i = (int)(idx / B), row = (int)(idx - (size_t)i * B);
  float lo = INFINITY, hi = -INFINITY;
  for (int s = 0; s < slices; ++s) {
    const float* p = part + ((size_t)s * 2 * A + 2 * i) * B + row;
    lo = fminf(lo, p[0]);
    hi = fmaxf(hi, p[(size_t)B]);
  }
  if (head && !(head[0] > 0.0)) lo = hi = __builtin_nanf("");
  br[idx] = lo;
  br[(size_t)A * B + idx] = hi;
}

// PY_REFINE: a workgroup takes PYF_ROWS rows; thread (j, r) sums F at point j + 1 of row r's bracket over the slices, then the
// thread j = 0 of the row narrows the bracket to the sub-interval that ends at the first point with F >= level (the last
// sub-interval when there is none) -- the points by py_point, the floats the forward kernel evaluated at -- and after the
// call's last pass writes out = hi and out_lo = lo.
constexpr int PYF_ROWS = 32;
__global__ __launch_bounds__(256) void k_predict_y_finish_refine(const float* __restrict__ part, int slices, int n, int B, int A,
                                                                 PyLevels lv, float* __restrict__ br, float* __restrict__ out,
                                                                 float* __restrict__ out_lo, int last,
                                                                 const double* __restrict__ head) {
  __shared__ double sh[PY_K][PYF_ROWS];
  const int r = threadIdx.x % PYF_ROWS, j = threadIdx.x / PYF_ROWS;   // j = 0 .. 7; 7 idles through the sums
  const int row = blockIdx.x * PYF_ROWS + r;
  const bool live = row < B;
  const bool bad = head && !(head[0] > 0.0);
  for (int i = 0; i < A; ++i) {
    if (live && j < PY_K) {
      double sum = 0.0;
      for (int s = 0; s < slices; ++s) sum += (double)part[((size_t)s * PY_K * A + i * PY_K + j) * B + row];
      sh[j][r] = head ? sum : sum / (double)n;
    }
    __syncthreads();
    if (live && j == 0) {
      const size_t at = (size_t)i * B + row;
      const float lo = br[at], hi = br[(size_t)A * B + at];
      float nlo = py_point(lo, hi, PY_K), nhi = hi;
      float below = lo;
      bool found = false;
#pragma unroll
      for (int k = 0; k < PY_K; ++k) {
        const float p = py_point(lo, hi, k + 1);
        if (!found && sh[k][r] >= lv.q[i]) {
          nlo = below;
          nhi = p;
          found = true;
        }
        below = p;
      }
      if (bad) nlo = nhi = __builtin_nanf("");
      br[at] = nlo;
      br[(size_t)A * B + at] = nhi;
      if (last) {
        out[at] = nhi;
        if (out_lo) out_lo[at] = nlo;
      }
    }
    __syncthreads();
  }
}

// ---- host side -----------------------------------------------------------------------------------------
// The summaries' plan with its slice count cut down until slices x (rows of the row tiles) x acc floats fit PY_PART_FLOATS
// (or to one slice); acc: the most words a (slice, row) can hold in a call of this kind -- PY_LEVELS for the distribution
// function, PY_ACC_MAX for the quantiles -- and not what this call holds: the slices decide which fp32 sums are formed, and a
// point's or a level's row must not depend on how many others share its call.
static PredPlan predict_y_plan(int64_t n, int64_t batch, bool quantiles) {
  const int acc = quantiles ? PY_ACC_MAX : PY_LEVELS;
  PredPlan p = predict_plan(n, batch);
  int64_t s = PY_PART_FLOATS / ((int64_t)p.row_tiles * PR_ROWS * acc);
  if (s < 1) s = 1;
  if (p.slices > s) {
    // a cut grid of a few hundred workgroups is whole rounds of the card or it waits on its last one: two of these
    // workgroups are resident per CU, PY_ROUND_WGS a round (measured: 576 workgroups took 1.8 times 512's time per particle)
    const int64_t wgs = s * p.row_tiles;
    if (wgs >= PY_ROUND_WGS) s = wgs / PY_ROUND_WGS * PY_ROUND_WGS / p.row_tiles;
    if (s < 1) s = 1;
    p.per = (int)((n + s - 1) / s);
    p.slices = (int)((n + p.per - 1) / p.per);
  }
  return p;
}

static int64_t predict_y_slices_bound(int64_t n) {
  const int64_t s = (n + PR_PASS - 1) / PR_PASS;
  return s < PR_SLICE_CAP ? s : PR_SLICE_CAP;
}

// the header for the most slices a plan can have, `levels` brackets per row, and an upper bound of slices * batch * acc partial
// sums that is monotone in every argument: slices <= min(passes, PR_SLICE_CAP); slices * batch <= PR_TARGET_WGS * PR_ROWS +
// batch as for the summaries; and by predict_y_plan, which
// plans for at least acc sums, slices * batch * acc <= PY_PART_FLOATS unless it is one slice
static size_t predict_y_ws_bytes(int64_t n, int64_t batch, int64_t acc, int64_t levels) {
  const int64_t s = predict_y_slices_bound(n);
  int64_t floats = s * batch * acc;
  const int64_t by_target = ((int64_t)PR_TARGET_WGS * PR_ROWS + batch) * acc, by_fit = PY_PART_FLOATS + batch * acc;
  if (floats > by_target) floats = by_target;
  if (floats > by_fit) floats = by_fit;
  const size_t bytes = pw_doubles(s) * sizeof(double) + (size_t)(2 * levels * batch + floats) * sizeof(float);
  return (bytes + 7) & ~(size_t)7;
}

static int predict_y_ws_query(int64_t n, int64_t batch, int64_t count, bool quantiles, size_t* out_bytes) {
  if (!out_bytes) return stein_fail(STEIN_E_BADARG, "NULL pointer");
  if (count < 1) return stein_fail(STEIN_E_BADARG, quantiles ? "n_levels %lld" : "n_pts %lld", (long long)count);
  if (n < 1 || batch < 1 || n > PR_COUNT_MAX || batch > PR_COUNT_MAX)
    return stein_fail(STEIN_E_SHAPE, "bad shape n=%lld batch=%lld", (long long)n, (long long)batch);
  if (count > PY_LEVELS)
    return stein_fail(STEIN_E_UNSUPPORTED, quantiles ? "more than %d levels per call" : "more than %d points per call", PY_LEVELS);
  *out_bytes = quantiles ? predict_y_ws_bytes(n, batch, PY_K * count, count) : predict_y_ws_bytes(n, batch, count, 0);
  return STEIN_OK;
}

extern "C" int stein_predict_ycdf_workspace_bytes(int64_t n, int64_t batch, int64_t n_pts, size_t* out_bytes) {
  return predict_y_ws_query(n, batch, n_pts, false, out_bytes);
}

extern "C" int stein_predict_yquantiles_workspace_bytes(int64_t n, int64_t batch, int64_t n_levels, size_t* out_bytes) {
  return predict_y_ws_query(n, batch, n_levels, true, out_bytes);
}

// what a call asks of the mixture: t != NULL the distribution function at n_pts points, else the quantiles at the levels
struct PyAsk {
  const float* t;
  const double* levels;
  int64_t count;
  int passes;
  const double* weights;
  float* out;
  float* out_lo;
  void* workspace;
  size_t ws_bytes;
  bool quantiles() const { return t == nullptr; }
};

// the checks ahead of the model's own: the NULL pointers and the count, then the shapes
static int predict_y_check(const float* theta, const float* X, const PyAsk& ask, bool quantiles, int64_t n, int64_t d,
                           int64_t batch, int64_t width) {
  if (!theta || !X || !(quantiles ? (const void*)ask.levels : (const void*)ask.t) || !ask.out)
    return stein_fail(STEIN_E_BADARG, "NULL pointer");
  if (ask.count < 1) return stein_fail(STEIN_E_BADARG, quantiles ? "n_levels %lld" : "n_pts %lld", (long long)ask.count);
  return predict_check(theta, X, nullptr, n, d, batch, width, STEIN_PRED_LINK, ask.out, nullptr, nullptr, nullptr,
                       PredWeights{false, nullptr, nullptr});
}

// Phi^-1(q) in fp64 for 0 < q < 1: Abramowitz & Stegun 26.2.23 (4.5e-4) polished by Halley steps on Phi(x) = erfc(-x / sqrt 2) / 2,
// taken in the lower tail, where erfc keeps its relative accuracy; the upper half by symmetry (1 - q is exact for q >= 1/2)
static double py_normal_quantile(double q) {
  const double p = q <= 0.5 ? q : 1.0 - q;
  const double r = sqrt(-2.0 * log(p));
  double x = -(r - (2.515517 + r * (0.802853 + r * 0.010328)) / (1.0 + r * (1.432788 + r * (0.189269 + r * 0.001308))));
  for (int it = 0; it < 4; ++it) {
    const double h = (0.5 * erfc(-x * 0.70710678118654752440) - p) / (0.39894228040143267794 * exp(-0.5 * x * x));
    x -= h / (1.0 + 0.5 * x * h);
  }
  return q <= 0.5 ? x : -x;
}

// ... and behind them: the count, every level, the passes, the workspace
static int predict_y_check_tail(const PyAsk& ask, bool quantiles, int64_t n, int64_t batch, PyLevels& lv, PyConsts& cs) {
  if (ask.count > PY_LEVELS)
    return stein_fail(STEIN_E_UNSUPPORTED, quantiles ? "more than %d levels per call" : "more than %d points per call", PY_LEVELS);
  if (quantiles) {
    for (int64_t i = 0; i < ask.count; ++i) {
      const double q = ask.levels[i];
      if (!(q > 0.0 && q < 1.0)) return stein_fail(STEIN_E_BADARG, "level %g is not inside (0, 1)", q);
      lv.q[i] = q;
      cs.c[i] = (float)py_normal_quantile(q);
    }
    if (ask.passes < 1 || ask.passes > STEIN_PRED_Y_PASSES_MAX)
      return stein_fail(STEIN_E_BADARG, "passes %d is outside [1, %d]", ask.passes, (int)STEIN_PRED_Y_PASSES_MAX);
  }
  if (!ask.workspace)
    return stein_fail(STEIN_E_WORKSPACE, quantiles ? "the quantiles of y need a workspace (stein_predict_yquantiles_workspace_bytes)"
                                                   : "the distribution function of y needs a workspace (stein_predict_ycdf_workspace_bytes)");
  const size_t need = quantiles ? predict_y_ws_bytes(n, batch, PY_K * ask.count, ask.count) : predict_y_ws_bytes(n, batch, ask.count, 0);
  if (ask.ws_bytes < need) return stein_fail(STEIN_E_WORKSPACE, "workspace too small: %zu < %zu bytes", ask.ws_bytes, need);
  if ((uintptr_t)ask.workspace % sizeof(double))
    return stein_fail(STEIN_E_WORKSPACE, "the workspace of a predictive call for y must be 8-byte aligned");
  return STEIN_OK;
}

// The launches of a call past its checks.  forward(mode, pts, part, head): the model's forward kernel in one mode.
template <class Forward>
static int predict_y_run(const PyAsk& ask, int64_t n, int64_t batch, const PredPlan& pl, const PyLevels& lv, hipStream_t s,
                         Forward&& forward) {
  const int A = (int)ask.count;
  const bool quantiles = ask.quantiles();
  double* head = (double*)ask.workspace;
  float* br = (float*)(head + pw_doubles(pl.slices));            // [2][A][batch], the quantiles only
  float* part = br + (quantiles ? (size_t)2 * A * batch : 0);
  const double* whead = ask.weights ? head : nullptr;
  if (ask.weights)
    if (int rc = predict_weight_pass(pl, n, PredWeights{true, ask.weights, nullptr}, ask.workspace, s)) return rc;
  const dim3 flat((unsigned)(((size_t)A * batch + 255) / 256));
  if (!quantiles) {
    if (int rc = forward(PY_CDF, ask.t, part, whead)) return rc;
    hipLaunchKernelGGL(k_predict_y_finish_cdf, flat, dim3(256), 0, s, part, pl.slices, (int)n, (int)batch, A, ask.out, whead);
    LAUNCH_CHECK("k_predict_y_finish_cdf");
    return STEIN_OK;
  }
  if (int rc = forward(PY_BRACKET, nullptr, part, whead)) return rc;
  hipLaunchKernelGGL(k_predict_y_finish_bracket, flat, dim3(256), 0, s, part, pl.slices, (int)batch, A, br, whead);
  LAUNCH_CHECK("k_predict_y_finish_bracket");
  for (int pass = 1; pass <= ask.passes; ++pass) {
    if (int rc = forward(PY_REFINE, br, part, whead)) return rc;
    hipLaunchKernelGGL(k_predict_y_finish_refine, dim3((unsigned)((batch + PYF_ROWS - 1) / PYF_ROWS)), dim3(256), 0, s, part,
                       pl.slices, (int)n, (int)batch, A, lv, br, ask.out, ask.out_lo, pass == ask.passes ? 1 : 0, whead);
    LAUNCH_CHECK("k_predict_y_finish_refine");
  }
  return STEIN_OK;
}

// Past the default 64 KB of LDS a kernel needs the attribute, which belongs to the function on one device (as in
// stein_predict_ranks.hip: a flag per device id; racing threads at worst set it twice).
static int predict_y_attr(const void* fn, int slot, size_t lds_dynamic) {
  static bool attr_set[6][64] = {{false}};
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64 || !attr_set[slot][dev]) {
    HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_dynamic));
    if (dev >= 0 && dev < 64) attr_set[slot][dev] = true;
  }
  return STEIN_OK;
}

static int predict_glm_y(const float* theta, int64_t n, int64_t d, int kind, int64_t w_col, int64_t n_feats, const float* X,
                         int64_t batch, double noise_precision, const PyAsk& ask, void* stream) {
  const bool quantiles = ask.quantiles();
  if (int rc = predict_y_check(theta, X, ask, quantiles, n, d, batch, n_feats)) return rc;
  if (int rc = predict_check_glm(kind, w_col, n_feats, d)) return rc;
  if (kind != STEIN_GLM_LINEAR)
    return stein_fail(STEIN_E_UNSUPPORTED, "y of the logistic model is Bernoulli: its predictive probability is the mean of the "
                                           "outputs with STEIN_PRED_MEAN (output=\"mean\")");
  if (!(noise_precision > 0.0 && noise_precision < INFINITY))
    return stein_fail(STEIN_E_BADARG, "noise_precision must be positive and finite");
  PyLevels lv = {};
  PyConsts cs = {};
  if (int rc = predict_y_check_tail(ask, quantiles, n, batch, lv, cs)) return rc;
  const int A = (int)ask.count;
  const PredPlan pl = predict_y_plan(n, batch, quantiles);
  const PredGlmTile tile = predict_glm_tile(n_feats, false);
  const size_t lds = tile.bytes + (size_t)(2 * PR_PASS + PR_PASS * 256) * sizeof(float);   // at most 80 640 bytes: two fit a CU
  const float sq = (float)sqrt(noise_precision), rsq = (float)(1.0 / sqrt(noise_precision));
  hipStream_t s = (hipStream_t)stream;
  using Kernel = decltype(&k_predict_glm_y<PY_CDF, false>);
  static const Kernel kernels[3][2] = {{k_predict_glm_y<PY_CDF, false>, k_predict_glm_y<PY_CDF, true>},
                                       {k_predict_glm_y<PY_BRACKET, false>, k_predict_glm_y<PY_BRACKET, true>},
                                       {k_predict_glm_y<PY_REFINE, false>, k_predict_glm_y<PY_REFINE, true>}};
  return predict_y_run(ask, n, batch, pl, lv, s, [&](int mode, const float* pts, float* part, const double* head) -> int {
    const Kernel kernel = kernels[mode][head ? 1 : 0];
    if (int rc = predict_y_attr(reinterpret_cast<const void*>(kernel), 2 * mode + (head ? 1 : 0), 96 * 1024)) return rc;
    hipLaunchKernelGGL(kernel, dim3((unsigned)pl.row_tiles, (unsigned)pl.slices), dim3(256), lds, s, theta, (int)n, (int)d,
                       (int)w_col, (int)n_feats, tile.fc, tile.ld, X, (int)batch, pl.per, sq, rsq, pts, cs, A, part, ask.weights,
                       head);
    LAUNCH_CHECK("k_predict_glm_y");
    return STEIN_OK;
  });
}

template <int NIN>
static int predict_bnn_y_launch(int mode, bool weighted, dim3 grid, hipStream_t s, const float* theta, int n, int d, int H,
                                PredCols c, const float* X, int B, int per, const float* pts, const PyConsts& cs, int A,
                                float* part, const double* wts, const double* head) {
  using Kernel = decltype(&k_predict_bnn_y<NIN, PY_CDF, false>);
  static const Kernel kernels[3][2] = {{k_predict_bnn_y<NIN, PY_CDF, false>, k_predict_bnn_y<NIN, PY_CDF, true>},
                                       {k_predict_bnn_y<NIN, PY_BRACKET, false>, k_predict_bnn_y<NIN, PY_BRACKET, true>},
                                       {k_predict_bnn_y<NIN, PY_REFINE, false>, k_predict_bnn_y<NIN, PY_REFINE, true>}};
  hipLaunchKernelGGL(kernels[mode][weighted ? 1 : 0], grid, dim3(256), 0, s, theta, n, d, H, c, X, B, per, pts, cs, A, part, wts,
                     head);
  LAUNCH_CHECK("k_predict_bnn_y");
  return STEIN_OK;
}

static int predict_bnn_y(const float* theta, int64_t n, int64_t d, int64_t n_in, int64_t n_hidden, const int64_t* cols,
                         const float* X, int64_t batch, const PyAsk& ask, void* stream) {
  if (!cols) return stein_fail(STEIN_E_BADARG, "NULL pointer");
  const bool quantiles = ask.quantiles();
  if (int rc = predict_y_check(theta, X, ask, quantiles, n, d, batch, n_hidden)) return rc;
  if (int rc = predict_check_bnn(n_in, n_hidden, cols, d)) return rc;
  PyLevels lv = {};
  PyConsts cs = {};
  if (int rc = predict_y_check_tail(ask, quantiles, n, batch, lv, cs)) return rc;
  const int A = (int)ask.count;
  const PredPlan pl = predict_y_plan(n, batch, quantiles);
  const PredCols c = predict_cols(cols);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)pl.row_tiles, (unsigned)pl.slices);
  return predict_y_run(ask, n, batch, pl, lv, s, [&](int mode, const float* pts, float* part, const double* head) -> int {
#define PY_LAUNCH_BNN(NIN)                                                                                              \
  return predict_bnn_y_launch<NIN>(mode, head != nullptr, grid, s, theta, (int)n, (int)d, (int)n_hidden, c, X, (int)batch, \
                                   pl.per, pts, cs, A, part, ask.weights, head)
    if (n_in == 1) PY_LAUNCH_BNN(1);
    if (n_in == 2) PY_LAUNCH_BNN(2);
    if (n_in == 3) PY_LAUNCH_BNN(3);
    PY_LAUNCH_BNN(4);
#undef PY_LAUNCH_BNN
  });
}

extern "C" int stein_predict_glm_ycdf(const float* theta, int64_t n, int64_t d, int kind, int64_t w_col, int64_t n_feats,
                                      const float* X, int64_t batch, double noise_precision, const float* t, int64_t n_pts,
                                      const double* weights, float* out, void* workspace, size_t ws_bytes, void* stream) {
  if (!t) return stein_fail(STEIN_E_BADARG, "NULL pointer");
  return predict_glm_y(theta, n, d, kind, w_col, n_feats, X, batch, noise_precision,
                       PyAsk{t, nullptr, n_pts, 0, weights, out, nullptr, workspace, ws_bytes}, stream);
}

extern "C" int stein_predict_bnn_ycdf(const float* theta, int64_t n, int64_t d, int64_t n_in, int64_t n_hidden,
                                      const int64_t* cols, const float* X, int64_t batch, const float* t, int64_t n_pts,
                                      const double* weights, float* out, void* workspace, size_t ws_bytes, void* stream) {
  if (!t) return stein_fail(STEIN_E_BADARG, "NULL pointer");
  return predict_bnn_y(theta, n, d, n_in, n_hidden, cols, X, batch,
                       PyAsk{t, nullptr, n_pts, 0, weights, out, nullptr, workspace, ws_bytes}, stream);
}

extern "C" int stein_predict_glm_yquantiles(const float* theta, int64_t n, int64_t d, int kind, int64_t w_col, int64_t n_feats,
                                            const float* X, int64_t batch, double noise_precision, const double* levels,
                                            int64_t n_levels, int passes, const double* weights, float* out, float* out_lo,
                                            void* workspace, size_t ws_bytes, void* stream) {
  return predict_glm_y(theta, n, d, kind, w_col, n_feats, X, batch, noise_precision,
                       PyAsk{nullptr, levels, n_levels, passes, weights, out, out_lo, workspace, ws_bytes}, stream);
}

extern "C" int stein_predict_bnn_yquantiles(const float* theta, int64_t n, int64_t d, int64_t n_in, int64_t n_hidden,
                                            const int64_t* cols, const float* X, int64_t batch, const double* levels,
                                            int64_t n_levels, int passes, const double* weights, float* out, float* out_lo,
                                            void* workspace, size_t ws_bytes, void* stream) {
  return predict_bnn_y(theta, n, d, n_in, n_hidden, cols, X, batch,
                       PyAsk{nullptr, levels, n_levels, passes, weights, out, out_lo, workspace, ws_bytes}, stream);
}
