// stein_predict.hip -- posterior predictive producers: the forward pass of the three models the score producers cover
// (stein_score.hip), for every particle, read out as the per-particle outputs pred[n][batch] and / or as per-test-point
// ensemble summaries that never materialise [n][batch].  This is the step immediately AFTER the SVGD update: the reference's
// examples end in function_posterior (stein/samplers/abstract_stein_sampler.py:157-168) and average what it returns.
//
//   z_pb   GLM      x_b . w_p
//          network  sum_h relu(b1_h + sum_f x_bf w1_fh) w2_h + b2          (the pred_b of stein_score.hip)
//   f_pb   STEIN_PRED_LINK: z_pb;  STEIN_PRED_MEAN: sigmoid(z_pb) for the logistic model, z_pb otherwise
//   mean_b = 1/n sum_p f_pb,  var_b = 1/n sum_p (f_pb - mean_b)^2,  lpd_b = log(1/n sum_p exp(l_pb))
//   l_pb   linear    1/2 log tau - 1/2 tau (y_b - z_pb)^2 - 1/2 log 2 pi
//          logistic  y_b z_pb - softplus(z_pb),  softplus(z) = max(z, 0) + log1p(exp(-|z|))
//          network   1/2 lg_p - 1/2 e^lg_p (y_b - z_pb)^2 - 1/2 log 2 pi,   lg_p the particle's log_gamma
//
// Mapping: the reduction a summary needs runs ACROSS PARTICLES, so the rows of X go on the lanes (the score kernels put the
// features there).  A workgroup owns a tile of PR_ROWS rows x one slice of the particles; every lane keeps its row's running
// state (count, mean, M2 by Welford's update; running max and sum exp(l - max)) in registers and walks the slice PR_PASS
// particles at a time, their weights staged in LDS and read at one address by every lane (broadcast, 16 bytes a read).
// No shuffle and no atomic anywhere.  Each (slice, row) writes one partial state to the workspace; k_predict_finish merges
// the slices in slice order (Chan et al.'s pairwise update and a max / rescaled-sum merge, both in fp64, as a fixed tree).  A slice's
// particle count follows from its index, so it is not stored, and every workspace word that is read was written by the
// same call: the workspace may hold anything on entry.
//
// Weighted form (stein_predict_*_weighted; the WEIGHTED instantiations below): per-particle weights w_p >= 0 in fp64, W their
// sum, mean_b = sum_p w_p f_pb / W and so on (include/steinhip.h).  k_predict_wsum / k_predict_wtotal sum the weights per
// slice and in total in fp64, in a fixed order, and poison W with NaN when a weight is negative or not finite or W is 0.
// The forward kernels stage fl32(w_p / W) of a pass's particles beside the particle data (the quotient is taken in fp64, so
// a power-of-two rescaling of w changes no bit; a quotient below 2^-126 counts as zero), every lane reads them at one
// address, and the running state becomes West's weighted update and a running max with sum w exp(l - max); a particle of
// weight zero is skipped.  The first particle with w > 0 sets shift, max and sum.  The state stays five floats: a slice's
// weight W_s / W is per slice, not per row, and comes from the weight pass, which also zeroes the W_s of a slice none of
// whose weights survives the rounding, so the finish kernel skips exactly the slices whose state was never set.
//
// The forward passes themselves (pred_glm_slice, pred_bnn_pass), the plan and the argument checks are stein_predict_fwd.h's:
// the rank-counting kernels of stein_predict_ranks.hip run the same ones.
#include "stein_predict_fwd.h"

// of the particles seen so far (their count is the caller's loop index): the slice's first output as a shift, mean and M2 of
// the outputs minus that shift (a common offset of the outputs then costs no digits), running max and sum exp(l - max)
struct PredState { float shift, mean, m2, mx, se; };
constexpr int PR_STATE = 5;          // floats per (slice, row) of the workspace

// particle number k (0-based) of this lane's slice: its output f and, when the lpd is wanted, its log likelihood l
__device__ __forceinline__ void pred_accumulate(PredState& st, int k, float f, float l, bool want_mv, bool want_lpd) {
  if (want_mv) {   // Welford on g = f - shift: k = 0 gives g = 0, mean = 0, m2 = 0 exactly
    if (k == 0) st.shift = f;
    const float g = f - st.shift;
    const float delta = g - st.mean;
    st.mean = fmaf(delta, 1.f / (float)(k + 1), st.mean);
    st.m2 = fmaf(delta, g - st.mean, st.m2);
  }
  if (want_lpd) {
    if (k == 0) {   // an empty state has no max: no (-inf) - (-inf)
      st.mx = l;
      st.se = 1.f;
    } else {
      const float e = l == st.mx ? 1.f : expf(-fabsf(l - st.mx));
      if (l > st.mx) {
        st.se = fmaf(st.se, e, 1.f);
        st.mx = l;
      } else {
        st.se += e;
      }
    }
  }
}

// The weighted update of one particle of normalised weight w (lane-uniform; 0: skipped) with wk the running sum of the
// weights before it.  West (1979) on g = f - shift: wk += w, mean += (w / wk) delta, M2 += w delta (g - mean).  The first
// particle with w > 0 meets wk = 0: it sets the shift (g = 0, delta = 0: mean and M2 stay exactly 0), max = l and sum = w.
__device__ __forceinline__ void pred_accumulate_weighted(PredState& st, float& wk, float w, float f, float l, bool want_mv,
                                                         bool want_lpd) {
  if (!(w > 0.f)) return;
  const bool first = wk == 0.f;
  wk += w;
  if (want_mv) {
    if (first) st.shift = f;
    const float g = f - st.shift;
    const float delta = g - st.mean;
    st.mean = fmaf(delta, w / wk, st.mean);
    st.m2 = fmaf(w * delta, g - st.mean, st.m2);
  }
  if (want_lpd) {
    if (first) {
      st.mx = l;
      st.se = w;
    } else {
      const float e = l == st.mx ? 1.f : expf(-fabsf(l - st.mx));
      if (l > st.mx) {
        st.se = fmaf(st.se, e, w);
        st.mx = l;
      } else {
        st.se = fmaf(w, e, st.se);
      }
    }
  }
}

__device__ __forceinline__ void pred_store_state(const PredState& st, float* __restrict__ part, int slice, int B, int row,
                                                 bool want_mv, bool want_lpd) {
  float* p = part + (size_t)slice * PR_STATE * B + row;   // [slice][shift, mean, m2, max, sum][B]
  if (want_mv) {
    p[0] = st.shift;
    p[(size_t)B] = st.mean;
    p[2 * (size_t)B] = st.m2;
  }
  if (want_lpd) {
    p[3 * (size_t)B] = st.mx;
    p[4 * (size_t)B] = st.se;
  }
}

// WEIGHTED: wts [n] the weights, head the weight pass's header (head[0] = W); the pass's PR_PASS normalised weights are
// staged behind ws.
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void k_predict_glm(const float* __restrict__ theta, int n, int d, int kind, int output,
                                                     int w_col, int F, int fc, int ld, const float* __restrict__ X,
                                                     const float* __restrict__ y, int B, int per, float half_tau, float c0,
                                                     float* __restrict__ pred, float* __restrict__ part, int want_mv,
                                                     int want_lpd, const double* __restrict__ wts,
                                                     const double* __restrict__ head) {
  extern __shared__ float lds[];
  float* xs = lds;                   // [PR_ROWS][ld]
  float* ws = lds + PR_ROWS * ld;    // [fc][PR_PASS]
  float* wl = ws + fc * PR_PASS;     // [PR_PASS], WEIGHTED only
  float wk = 0.f;
  const double wtot = WEIGHTED ? head[0] : 0.0;
  const int t = threadIdx.x;
  const int row0 = blockIdx.x * PR_ROWS, row = row0 + t;
  const bool live = row < B;
  const int p_begin = blockIdx.y * per, p_end = min(n, p_begin + per);
  const bool logistic = kind == STEIN_GLM_LOGISTIC, sigmoid = logistic && output == STEIN_PRED_MEAN;
  const float yb = (want_lpd && live) ? y[row] : 0.f;
  PredState st = {0.f, 0.f, 0.f, 0.f, 0.f};
  pred_glm_slice(
      theta, d, w_col, F, fc, ld, X, B, row0, p_begin, p_end, xs, ws, t,
      [&](int p0, int cnt) {
        if (WEIGHTED && t < PR_PASS) wl[t] = t < cnt ? pred_norm_weight(wts[p0 + t], wtot) : 0.f;
      },
      [&](int p0, int k, float zz) {
        const float f = pred_glm_output(zz, sigmoid);
        if (pred && live) pred[(size_t)(p0 + k) * B + row] = f;
        float l = 0.f;
        if (want_lpd) {
          if (logistic) {
            l = yb * zz - (fmaxf(zz, 0.f) + log1pf(expf(-fabsf(zz))));
          } else {
            const float r = yb - zz;
            l = fmaf(-half_tau, r * r, c0);
          }
        }
        if constexpr (WEIGHTED) pred_accumulate_weighted(st, wk, wl[k], f, l, want_mv, want_lpd);
        else pred_accumulate(st, p0 - p_begin + k, f, l, want_mv, want_lpd);
      });
  if (live && part) pred_store_state(st, part, blockIdx.y, B, row, want_mv, want_lpd);
}

template <int NIN, bool WEIGHTED>
__global__ __launch_bounds__(256) void k_predict_bnn(const float* __restrict__ theta, int n, int d, int H, PredCols c,
                                                     const float* __restrict__ X, const float* __restrict__ y, int B, int per,
                                                     float* __restrict__ pred, float* __restrict__ part, int want_mv,
                                                     int want_lpd, const double* __restrict__ wts,
                                                     const double* __restrict__ head) {
  __shared__ __attribute__((aligned(16))) float lw[PR_PASS * PR_BNN_PW<NIN>];
  __shared__ float lp[PR_PASS][4];        // per particle: b2, 1/2 lg - 1/2 log 2 pi, 1/2 e^lg; WEIGHTED: its normalised weight
  float wk = 0.f;
  const double wtot = WEIGHTED ? head[0] : 0.0;
  const int t = threadIdx.x;
  const int row = blockIdx.x * PR_ROWS + t;
  const bool live = row < B;
  const int p_begin = blockIdx.y * per, p_end = min(n, p_begin + per);
  float x[NIN];
#pragma unroll
  for (int f = 0; f < NIN; ++f) x[f] = live ? X[(size_t)row * NIN + f] : 0.f;
  const float yb = (want_lpd && live) ? y[row] : 0.f;
  PredState st = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (int p0 = p_begin; p0 < p_end; p0 += PR_PASS) {
    const int cnt = min(PR_PASS, p_end - p0);
    float z[PR_PASS];
#pragma unroll
    for (int k = 0; k < PR_PASS; ++k) z[k] = 0.f;
    pred_bnn_pass<NIN>(z, theta, d, H, c, x, p0, cnt, lw, lp, t, [&](int k) {
      if (WEIGHTED) lp[k][3] = pred_norm_weight(wts[p0 + k], wtot);
    });
#pragma unroll
    for (int k = 0; k < PR_PASS; ++k) {
      if (k < cnt) {
        const float f = z[k] + lp[k][0];
        if (pred && live) pred[(size_t)(p0 + k) * B + row] = f;
        float l = 0.f;
        if (want_lpd) {
          const float r = yb - f;
          l = fmaf(-lp[k][2], r * r, lp[k][1]);
        }
        if constexpr (WEIGHTED) pred_accumulate_weighted(st, wk, lp[k][3], f, l, want_mv, want_lpd);
        else pred_accumulate(st, p0 - p_begin + k, f, l, want_mv, want_lpd);
      }
    }
  }
  if (live && part) pred_store_state(st, part, blockIdx.y, B, row, want_mv, want_lpd);
}

// More than PR_NIN_MAX input features (stein_predict_bnn_wide): the same mapping with the row's inputs in LDS
// (pred_bnn_wide_pass); xs [PR_ROWS][ld] is staged once for the slice, rows past the batch as zeros, lw behind it.
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void k_predict_bnn_wide(const float* __restrict__ theta, int n, int d, int NIN, int H,
                                                          PredCols c, const float* __restrict__ X, const float* __restrict__ y,
                                                          int B, int per, int ld, int ps, int hc, float* __restrict__ pred,
                                                          float* __restrict__ part, int want_mv, int want_lpd,
                                                          const double* __restrict__ wts, const double* __restrict__ head) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xs = lds;                 // [PR_ROWS][ld]
  float* lw = lds + PR_ROWS * ld;  // [ps][NIN + 2][hc]
  __shared__ float lp[PR_PASS][4];
  float wk = 0.f;
  const double wtot = WEIGHTED ? head[0] : 0.0;
  const int t = threadIdx.x;
  const int row0 = blockIdx.x * PR_ROWS, row = row0 + t;
  const bool live = row < B;
  const int p_begin = blockIdx.y * per, p_end = min(n, p_begin + per);
  for (int i = t; i < PR_ROWS * NIN; i += 256) {
    const int r = i / NIN, f = i - r * NIN;
    xs[r * ld + f] = row0 + r < B ? X[(size_t)(row0 + r) * NIN + f] : 0.f;
  }
  const float* xr = xs + t * ld;
  const float yb = (want_lpd && live) ? y[row] : 0.f;
  PredState st = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (int p0 = p_begin; p0 < p_end; p0 += PR_PASS) {
    const int cnt = min(PR_PASS, p_end - p0);
    float z[PR_PASS];
#pragma unroll
    for (int k = 0; k < PR_PASS; ++k) z[k] = 0.f;
    pred_bnn_wide_pass(z, theta, d, NIN, H, c, xr, p0, cnt, ps, hc, lw, lp, t, [&](int k) {
      if (WEIGHTED) lp[k][3] = pred_norm_weight(wts[p0 + k], wtot);
    });
#pragma unroll
    for (int k = 0; k < PR_PASS; ++k) {
      if (k < cnt) {
        const float f = z[k] + lp[k][0];
        if (pred && live) pred[(size_t)(p0 + k) * B + row] = f;
        float l = 0.f;
        if (want_lpd) {
          const float r = yb - f;
          l = fmaf(-lp[k][2], r * r, lp[k][1]);
        }
        if constexpr (WEIGHTED) pred_accumulate_weighted(st, wk, lp[k][3], f, l, want_mv, want_lpd);
        else pred_accumulate(st, p0 - p_begin + k, f, l, want_mv, want_lpd);
      }
    }
  }
  if (live && part) pred_store_state(st, part, blockIdx.y, B, row, want_mv, want_lpd);
}

// The slices' states merged in slice order, in fp64.  A workgroup takes PF_ROWS rows; its PF_GROUPS thread groups each merge
// a contiguous range of the slices in order, then one thread per row merges the groups in order: a fixed tree, so the
// result depends on nothing but the states.  (One thread walking all the slices of a row took longer than the forward
// pass at 512 slices.)
constexpr int PF_ROWS = 16, PF_GROUPS = 16;

//
// WEIGHTED: a slice counts with W_s / W of the weight pass's header in place of its particle count, so the total is 1 and
// nothing is divided at the end; a slice (and then a group) of weight 0 holds no state and is skipped, wherever it lies.
// Bad weights (W = NaN) give NaN rows.
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void k_predict_finish(const float* __restrict__ part, int slices, int per, int n, int B,
                                                        float* __restrict__ mean, float* __restrict__ var,
                                                        float* __restrict__ lpd, const double* __restrict__ head) {
  __shared__ double sh[5][PF_GROUPS][PF_ROWS];   // count, mean, M2, max, sum
  const int r = threadIdx.x % PF_ROWS, g = threadIdx.x / PF_ROWS;
  const int b = blockIdx.x * PF_ROWS + r;
  const int per_g = (slices + PF_GROUPS - 1) / PF_GROUPS;
  const int s0 = g * per_g, s1 = min(slices, s0 + per_g);
  const size_t sB = (size_t)B;
  const double wtot = WEIGHTED ? head[0] : 0.0;
  auto weight = [&](int s) {   // of slice s: not positive (0, or NaN under a poisoned W) = no state
    if constexpr (WEIGHTED) return head[PW_HEAD + s] / wtot;
    else return (double)min(per, n - s * per);
  };
  double cnt = 0.0, m = 0.0, m2 = 0.0, top = 0.0, sum = 0.0;
  if (b < B && s0 < s1) {
    const float* p = part + b;
    if (mean || var) {   // Chan et al.: (count, mean, M2) of the union of two sets
      for (int s = s0; s < s1; ++s) {
        const float* ps = p + (size_t)s * PR_STATE * sB;
        const double cs = weight(s);
        if (WEIGHTED && !(cs > 0.0)) continue;
        const double ms = (double)ps[0] + (double)ps[sB], m2s = ps[2 * sB];
        const double tot = cnt + cs, delta = ms - m;
        m += delta * (cs / tot);
        m2 += m2s + delta * delta * (cnt * cs / tot);
        cnt = tot;
      }
    }
    if constexpr (WEIGHTED) {   // the same sum in the same order, whether or not the loop above ran
      cnt = 0.0;
      for (int s = s0; s < s1; ++s) {
        const double cs = weight(s);
        if (cs > 0.0) cnt += cs;
      }
    } else {
      cnt = (double)(min((long)n, (long)s1 * per) - (long)s0 * per);
    }
    if (lpd) {
      if constexpr (WEIGHTED) {
        bool any = false;
        for (int s = s0; s < s1; ++s) {
          if (!(weight(s) > 0.0)) continue;
          const double mx = p[((size_t)s * PR_STATE + 3) * sB];
          top = any ? fmax(top, mx) : mx;
          any = true;
        }
      } else {
        top = (double)p[((size_t)s0 * PR_STATE + 3) * sB];
        for (int s = s0 + 1; s < s1; ++s) top = fmax(top, (double)p[((size_t)s * PR_STATE + 3) * sB]);
      }
      for (int s = s0; s < s1; ++s) {
        if (WEIGHTED && !(weight(s) > 0.0)) continue;
        const double mx = p[((size_t)s * PR_STATE + 3) * sB], se = p[((size_t)s * PR_STATE + 4) * sB];
        sum += mx == top ? se : se * exp(mx - top);
      }
    }
  }
  sh[0][g][r] = cnt; sh[1][g][r] = m; sh[2][g][r] = m2; sh[3][g][r] = top; sh[4][g][r] = sum;
  __syncthreads();
  if (g != 0 || b >= B) return;
  if (WEIGHTED && !(wtot > 0.0)) {   // a negative or non-finite weight, or W = 0
    const float bad = __builtin_nanf("");
    if (mean) mean[b] = bad;
    if (var) var[b] = bad;
    if (lpd) lpd[b] = bad;
    return;
  }
  for (int k = 1; k < PF_GROUPS; ++k) {   // (unweighted: group 0 is never empty, and no group follows an empty one)
    const double cs = sh[0][k][r];
    if (WEIGHTED) {
      if (!(cs > 0.0)) continue;
      if (cnt == 0.0) {   // the first group that holds anything
        cnt = cs; m = sh[1][k][r]; m2 = sh[2][k][r]; top = sh[3][k][r]; sum = sh[4][k][r];
        continue;
      }
    }
    if (cs == 0.0) break;
    const double tot = cnt + cs, delta = sh[1][k][r] - m;
    m += delta * (cs / tot);
    m2 += sh[2][k][r] + delta * delta * (cnt * cs / tot);
    cnt = tot;
    const double tk = sh[3][k][r], sk = sh[4][k][r];
    if (tk > top) {
      sum = sum * exp(top - tk) + sk;
      top = tk;
    } else {
      sum += tk == top ? sk : sk * exp(tk - top);
    }
  }
  if (mean) mean[b] = (float)m;
  if (var) var[b] = WEIGHTED ? (float)m2 : (float)(m2 / (double)n);
  if (lpd) lpd[b] = WEIGHTED ? (float)(top + log(sum)) : (float)(top + log(sum) - log((double)n));
}

// ---- the weight pass of a weighted call ------------------------------------------------------------------
// 256 partial results per quantity folded by halving, in a fixed order: quantities 0 and 1 are sums, 2 is a maximum
__device__ __forceinline__ void pw_fold(double (*sh)[256], int t, int quantities) {
  for (int half = 128; half > 0; half >>= 1) {
    __syncthreads();
    if (t < half)
      for (int q = 0; q < quantities; ++q) sh[q][t] = q == 2 ? fmax(sh[q][t], sh[q][t + half]) : sh[q][t] + sh[q][t + half];
  }
  __syncthreads();
}

// one workgroup per slice of predict_plan: W_s, sum w^2 and max w of the slice; a weight that is negative or not finite
// turns W_s into NaN, which every later sum keeps
__global__ __launch_bounds__(256) void k_predict_wsum(const double* __restrict__ wts, int n, int per, int slices,
                                                      double* __restrict__ head) {
  __shared__ double sh[3][256];
  const int t = threadIdx.x, s = blockIdx.x;
  const int p_begin = s * per, p_end = min(n, p_begin + per);
  double a = 0.0, q = 0.0, top = 0.0;
  bool bad = false;
  for (int p = p_begin + t; p < p_end; p += 256) {
    const double v = wts[p];
    bad = bad || !(v >= 0.0 && v < (double)INFINITY);
    a += v;
    q += v * v;
    top = fmax(top, v);
  }
  sh[0][t] = bad ? (double)NAN : a; sh[1][t] = q; sh[2][t] = top;
  pw_fold(sh, t, 3);
  if (t == 0) {
    head[PW_HEAD + s] = sh[0][0];
    head[PW_HEAD + slices + s] = sh[1][0];
    head[PW_HEAD + 2 * slices + s] = sh[2][0];
  }
}

// one workgroup: W and sum w^2 over the slices, the poison (W is NaN unless 0 < W < inf), ess = W^2 / sum w^2, and W_s = 0
// for a slice whose largest weight rounds to zero as the forward kernels round it (rounding is monotone: then all do)
__global__ __launch_bounds__(256) void k_predict_wtotal(int slices, double* __restrict__ head, double* __restrict__ ess) {
  __shared__ double sh[2][256];
  const int t = threadIdx.x;
  double a = 0.0, q = 0.0;
  for (int s = t; s < slices; s += 256) {
    a += head[PW_HEAD + s];
    q += head[PW_HEAD + slices + s];
  }
  sh[0][t] = a; sh[1][t] = q;
  pw_fold(sh, t, 2);
  double W = sh[0][0];
  if (!(W > 0.0 && W < (double)INFINITY)) W = (double)NAN;
  for (int s = t; s < slices; s += 256)
    if (!(pred_norm_weight(head[PW_HEAD + 2 * slices + s], W) > 0.f)) head[PW_HEAD + s] = 0.0;
  if (t == 0) {
    head[0] = W;
    head[1] = sh[1][0];
    if (ess) *ess = W * W / sh[1][0];
  }
}

// ---- host side -----------------------------------------------------------------------------------------
// An upper bound of the plan's slices * batch states, monotone in both arguments (the plan's own product is not: a row tile
// more can cost slices).  slices <= passes, <= PR_SLICE_CAP, and <= PR_TARGET_WGS / row_tiles + 1 with row_tiles >= batch /
// PR_ROWS, so slices * batch <= PR_TARGET_WGS * PR_ROWS + batch.
static size_t predict_ws_bytes(int64_t n, int64_t batch) {
  int64_t s = (n + PR_PASS - 1) / PR_PASS;
  if (s > PR_SLICE_CAP) s = PR_SLICE_CAP;
  int64_t states = s * batch;
  const int64_t by_target = (int64_t)PR_TARGET_WGS * PR_ROWS + batch;
  if (states > by_target) states = by_target;
  return (size_t)states * PR_STATE * sizeof(float);
}

extern "C" int stein_predict_workspace_bytes(int64_t n, int64_t batch, size_t* out_bytes) {
  if (!out_bytes) return stein_fail(STEIN_E_BADARG, "NULL pointer");
  if (n < 1 || batch < 1 || n > PR_COUNT_MAX || batch > PR_COUNT_MAX)
    return stein_fail(STEIN_E_SHAPE, "bad shape n=%lld batch=%lld", (long long)n, (long long)batch);
  *out_bytes = predict_ws_bytes(n, batch);
  return STEIN_OK;
}

static size_t predict_wws_bytes(int64_t n, int64_t batch) {   // the states behind the weight pass's header; monotone too
  int64_t s = (n + PR_PASS - 1) / PR_PASS;
  if (s > PR_SLICE_CAP) s = PR_SLICE_CAP;
  return pw_doubles(s) * sizeof(double) + predict_ws_bytes(n, batch);
}

extern "C" int stein_predict_weighted_workspace_bytes(int64_t n, int64_t batch, size_t* out_bytes) {
  if (!out_bytes) return stein_fail(STEIN_E_BADARG, "NULL pointer");
  if (n < 1 || batch < 1 || n > PR_COUNT_MAX || batch > PR_COUNT_MAX)
    return stein_fail(STEIN_E_SHAPE, "bad shape n=%lld batch=%lld", (long long)n, (long long)batch);
  *out_bytes = predict_wws_bytes(n, batch);
  return STEIN_OK;
}

static int predict_check_ws(int64_t n, int64_t batch, bool summary, const void* workspace, size_t ws_bytes,
                            const PredWeights& pw) {
  if (!summary) return STEIN_OK;   // a call that only asks for pred needs no workspace
  if (!workspace)
    return stein_fail(STEIN_E_WORKSPACE, pw.on ? "mean, var, lpd and ess need a workspace (stein_predict_weighted_workspace_bytes)"
                                               : "mean, var and lpd need a workspace (stein_predict_workspace_bytes)");
  const size_t need = pw.on ? predict_wws_bytes(n, batch) : predict_ws_bytes(n, batch);
  if (ws_bytes < need) return stein_fail(STEIN_E_WORKSPACE, "workspace too small: %zu < %zu bytes", ws_bytes, need);
  if (pw.on && (uintptr_t)workspace % sizeof(double))
    return stein_fail(STEIN_E_WORKSPACE, "the workspace of a weighted call must be 8-byte aligned");
  return STEIN_OK;
}

// where a call's states lie in its workspace: at its start, or behind the weight pass's header
static float* predict_states(const PredPlan& pl, void* workspace, const PredWeights& pw) {
  return pw.on ? (float*)((double*)workspace + pw_doubles(pl.slices)) : (float*)workspace;
}

// the weight pass, queued ahead of the forward kernel of a weighted call that asks for any summary (declared in
// stein_predict_fwd.h: the calls of stein_predict_y.hip queue it too)
int predict_weight_pass(const PredPlan& pl, int64_t n, const PredWeights& pw, void* workspace, hipStream_t s) {
  hipLaunchKernelGGL(k_predict_wsum, dim3((unsigned)pl.slices), dim3(256), 0, s, pw.w, (int)n, pl.per, pl.slices, (double*)workspace);
  LAUNCH_CHECK("k_predict_wsum");
  hipLaunchKernelGGL(k_predict_wtotal, dim3(1), dim3(256), 0, s, pl.slices, (double*)workspace, pw.ess);
  LAUNCH_CHECK("k_predict_wtotal");
  return STEIN_OK;
}

static int predict_finish(const PredPlan& pl, int64_t n, int64_t batch, const float* part, float* mean, float* var,
                          float* lpd, const double* head, hipStream_t s) {
  const dim3 grid((unsigned)((batch + PF_ROWS - 1) / PF_ROWS));
  if (head) hipLaunchKernelGGL(k_predict_finish<true>, grid, dim3(256), 0, s, part, pl.slices, pl.per, (int)n, (int)batch, mean, var, lpd, head);
  else hipLaunchKernelGGL(k_predict_finish<false>, grid, dim3(256), 0, s, part, pl.slices, pl.per, (int)n, (int)batch, mean, var, lpd, head);
  LAUNCH_CHECK("k_predict_finish");
  return STEIN_OK;
}

static int predict_glm(const float* theta, int64_t n, int64_t d, int kind, int output, int64_t w_col, int64_t n_feats,
                       const float* X, const float* y, int64_t batch, double noise_precision, float* pred, float* mean,
                       float* var, float* lpd, void* workspace, size_t ws_bytes, void* stream, const PredWeights& pw) {
  if (int rc = predict_check(theta, X, y, n, d, batch, n_feats, output, pred, mean, var, lpd, pw)) return rc;
  if (int rc = predict_check_glm(kind, w_col, n_feats, d)) return rc;
  if (lpd && kind == STEIN_GLM_LINEAR && !(noise_precision > 0.0 && noise_precision < INFINITY))
    return stein_fail(STEIN_E_BADARG, "noise_precision must be positive and finite");
  const bool summary = mean || var || lpd;   // the rows the forward kernel reduces; ess comes from the weight pass alone
  if (int rc = predict_check_ws(n, batch, summary || pw.ess, workspace, ws_bytes, pw)) return rc;
  const PredPlan pl = predict_plan(n, batch);
  const double tau = (lpd && kind == STEIN_GLM_LINEAR) ? noise_precision : 1.0;
  hipStream_t s = (hipStream_t)stream;
  if (pw.on && (summary || pw.ess))
    if (int rc = predict_weight_pass(pl, n, pw, workspace, s)) return rc;
  if (!pred && !summary) return STEIN_OK;   // ess alone
  float* part = summary ? predict_states(pl, workspace, pw) : nullptr;
  const double* head = (pw.on && summary) ? (const double*)workspace : nullptr;
  const PredGlmTile tile = predict_glm_tile(n_feats, head != nullptr);   // weighted: the pass's weights behind the tile
#define PR_LAUNCH_GLM(WEIGHTED, LDS)                                                                                    \
  hipLaunchKernelGGL(k_predict_glm<WEIGHTED>, dim3((unsigned)pl.row_tiles, (unsigned)pl.slices), dim3(256), LDS, s, theta, \
                     (int)n, (int)d, kind, output, (int)w_col, (int)n_feats, tile.fc, tile.ld, X, y, (int)batch, pl.per,  \
                     (float)(0.5 * tau), (float)(0.5 * log(tau) - (double)PR_HALF_LOG_2PI), pred, part,                   \
                     (mean || var) ? 1 : 0, lpd ? 1 : 0, pw.w, head)
  if (head) PR_LAUNCH_GLM(true, tile.bytes);
  else PR_LAUNCH_GLM(false, tile.bytes);
#undef PR_LAUNCH_GLM
  LAUNCH_CHECK("k_predict_glm");
  return summary ? predict_finish(pl, n, batch, part, mean, var, lpd, head, s) : STEIN_OK;
}

static int predict_bnn(const float* theta, int64_t n, int64_t d, int64_t n_in, int64_t n_hidden, const int64_t* cols,
                       int output, const float* X, const float* y, int64_t batch, float* pred, float* mean, float* var,
                       float* lpd, void* workspace, size_t ws_bytes, void* stream, const PredWeights& pw) {
  if (!cols) return stein_fail(STEIN_E_BADARG, "NULL pointer");
  if (int rc = predict_check(theta, X, y, n, d, batch, n_hidden, output, pred, mean, var, lpd, pw)) return rc;
  if (int rc = predict_check_bnn(n_in, n_hidden, cols, d)) return rc;
  const bool summary = mean || var || lpd;
  if (int rc = predict_check_ws(n, batch, summary || pw.ess, workspace, ws_bytes, pw)) return rc;
  const PredPlan pl = predict_plan(n, batch);
  const PredCols c = predict_cols(cols);
  hipStream_t s = (hipStream_t)stream;
  if (pw.on && (summary || pw.ess))
    if (int rc = predict_weight_pass(pl, n, pw, workspace, s)) return rc;
  if (!pred && !summary) return STEIN_OK;   // ess alone
  float* part = summary ? predict_states(pl, workspace, pw) : nullptr;
  const double* head = (pw.on && summary) ? (const double*)workspace : nullptr;
#define PR_LAUNCH_BNN_AS(NIN, WEIGHTED)                                                                                 \
  hipLaunchKernelGGL((k_predict_bnn<NIN, WEIGHTED>), dim3((unsigned)pl.row_tiles, (unsigned)pl.slices), dim3(256), 0, s, \
                     theta, (int)n, (int)d, (int)n_hidden, c, X, y, (int)batch, pl.per, pred, part,                      \
                     (mean || var) ? 1 : 0, lpd ? 1 : 0, pw.w, head)
#define PR_LAUNCH_BNN(NIN)                                                                                              \
  do {                                                                                                                  \
    if (head) PR_LAUNCH_BNN_AS(NIN, true);                                                                              \
    else PR_LAUNCH_BNN_AS(NIN, false);                                                                                  \
  } while (0)
  if (n_in == 1) PR_LAUNCH_BNN(1);
  else if (n_in == 2) PR_LAUNCH_BNN(2);
  else if (n_in == 3) PR_LAUNCH_BNN(3);
  else PR_LAUNCH_BNN(4);
#undef PR_LAUNCH_BNN
#undef PR_LAUNCH_BNN_AS
  LAUNCH_CHECK("k_predict_bnn");
  return summary ? predict_finish(pl, n, batch, part, mean, var, lpd, head, s) : STEIN_OK;
}

// the wide kernels take up to 160 KB of dynamic LDS: raise each one's limit once per device
static int predict_wide_attr(const void* fn, int slot) {
  static bool attr_set[2][64] = {{false}};
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64 || !attr_set[slot][dev]) {
    HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, PR_WIDE_LDS * (int)sizeof(float)));
    if (dev >= 0 && dev < 64) attr_set[slot][dev] = true;
  }
  return STEIN_OK;
}

// stein_predict_bnn_wide / _weighted: up to PR_NIN_MAX features the narrow entry points' own code; past them the same
// checks in the same order with the wide domain, the same plan, workspace, weight pass and finish, and k_predict_bnn_wide
static int predict_bnn_wide(const float* theta, int64_t n, int64_t d, int64_t n_in, int64_t n_hidden, const int64_t* cols,
                            int output, const float* X, const float* y, int64_t batch, float* pred, float* mean, float* var,
                            float* lpd, void* workspace, size_t ws_bytes, void* stream, const PredWeights& pw) {
  if (n_in >= 1 && n_in <= PR_NIN_MAX)
    return predict_bnn(theta, n, d, n_in, n_hidden, cols, output, X, y, batch, pred, mean, var, lpd, workspace, ws_bytes, stream, pw);
  if (!cols) return stein_fail(STEIN_E_BADARG, "NULL pointer");
  if (int rc = predict_check(theta, X, y, n, d, batch, n_hidden, output, pred, mean, var, lpd, pw)) return rc;
  if (int rc = predict_check_bnn_wide(n_in, n_hidden, cols, d)) return rc;
  const bool summary = mean || var || lpd;
  if (int rc = predict_check_ws(n, batch, summary || pw.ess, workspace, ws_bytes, pw)) return rc;
  const PredPlan pl = predict_plan(n, batch);
  const PredCols c = predict_cols(cols);
  hipStream_t s = (hipStream_t)stream;
  if (pw.on && (summary || pw.ess))
    if (int rc = predict_weight_pass(pl, n, pw, workspace, s)) return rc;
  if (!pred && !summary) return STEIN_OK;   // ess alone
  float* part = summary ? predict_states(pl, workspace, pw) : nullptr;
  const double* head = (pw.on && summary) ? (const double*)workspace : nullptr;
  const PredWideTile w = predict_wide_tile(n_in);
#define PR_LAUNCH_WIDE(WEIGHTED, SLOT)                                                                                   \
  do {                                                                                                                   \
    if (int rc = predict_wide_attr(reinterpret_cast<const void*>(k_predict_bnn_wide<WEIGHTED>), SLOT)) return rc;        \
    hipLaunchKernelGGL(k_predict_bnn_wide<WEIGHTED>, dim3((unsigned)pl.row_tiles, (unsigned)pl.slices), dim3(256),        \
                       w.bytes, s, theta, (int)n, (int)d, (int)n_in, (int)n_hidden, c, X, y, (int)batch, pl.per, w.ld,    \
                       w.ps, w.hc, pred, part, (mean || var) ? 1 : 0, lpd ? 1 : 0, pw.w, head);                           \
  } while (0)
  if (head) PR_LAUNCH_WIDE(true, 1);
  else PR_LAUNCH_WIDE(false, 0);
#undef PR_LAUNCH_WIDE
  LAUNCH_CHECK("k_predict_bnn_wide");
  return summary ? predict_finish(pl, n, batch, part, mean, var, lpd, head, s) : STEIN_OK;
}

extern "C" int stein_predict_bnn_wide(const float* theta, int64_t n, int64_t d, int64_t n_in, int64_t n_hidden,
                                      const int64_t* cols /*[6]: w1, b1, w2, b2, log_lambda, log_gamma*/, int output,
                                      const float* X, const float* y, int64_t batch, float* pred, float* mean, float* var,
                                      float* lpd, void* workspace, size_t ws_bytes, void* stream) {
  return predict_bnn_wide(theta, n, d, n_in, n_hidden, cols, output, X, y, batch, pred, mean, var, lpd, workspace, ws_bytes,
                          stream, PredWeights{false, nullptr, nullptr});
}

extern "C" int stein_predict_bnn_wide_weighted(const float* theta, int64_t n, int64_t d, int64_t n_in, int64_t n_hidden,
                                               const int64_t* cols, int output, const float* X, const float* y, int64_t batch,
                                               const double* weights, float* pred, float* mean, float* var, float* lpd,
                                               double* ess, void* workspace, size_t ws_bytes, void* stream) {
  return predict_bnn_wide(theta, n, d, n_in, n_hidden, cols, output, X, y, batch, pred, mean, var, lpd, workspace, ws_bytes,
                          stream, PredWeights{true, weights, ess});
}

extern "C" int stein_predict_glm(const float* theta, int64_t n, int64_t d, int kind, int output, int64_t w_col,
                                 int64_t n_feats, const float* X, const float* y, int64_t batch, double noise_precision,
                                 float* pred, float* mean, float* var, float* lpd, void* workspace, size_t ws_bytes,
                                 void* stream) {
  return predict_glm(theta, n, d, kind, output, w_col, n_feats, X, y, batch, noise_precision, pred, mean, var, lpd, workspace,
                     ws_bytes, stream, PredWeights{false, nullptr, nullptr});
}

extern "C" int stein_predict_glm_weighted(const float* theta, int64_t n, int64_t d, int kind, int output, int64_t w_col,
                                          int64_t n_feats, const float* X, const float* y, int64_t batch,
                                          double noise_precision, const double* weights, float* pred, float* mean, float* var,
                                          float* lpd, double* ess, void* workspace, size_t ws_bytes, void* stream) {
  return predict_glm(theta, n, d, kind, output, w_col, n_feats, X, y, batch, noise_precision, pred, mean, var, lpd, workspace,
                     ws_bytes, stream, PredWeights{true, weights, ess});
}

extern "C" int stein_predict_bnn(const float* theta, int64_t n, int64_t d, int64_t n_in, int64_t n_hidden,
                                 const int64_t* cols /*[6]: w1, b1, w2, b2, log_lambda, log_gamma*/, int output,
                                 const float* X, const float* y, int64_t batch, float* pred, float* mean, float* var,
                                 float* lpd, void* workspace, size_t ws_bytes, void* stream) {
  return predict_bnn(theta, n, d, n_in, n_hidden, cols, output, X, y, batch, pred, mean, var, lpd, workspace, ws_bytes, stream,
                     PredWeights{false, nullptr, nullptr});
}

extern "C" int stein_predict_bnn_weighted(const float* theta, int64_t n, int64_t d, int64_t n_in, int64_t n_hidden,
                                          const int64_t* cols, int output, const float* X, const float* y, int64_t batch,
                                          const double* weights, float* pred, float* mean, float* var, float* lpd,
                                          double* ess, void* workspace, size_t ws_bytes, void* stream) {
  return predict_bnn(theta, n, d, n_in, n_hidden, cols, output, X, y, batch, pred, mean, var, lpd, workspace, ws_bytes, stream,
                     PredWeights{true, weights, ess});
}
