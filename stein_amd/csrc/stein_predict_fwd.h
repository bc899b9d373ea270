// stein_predict_fwd.h -- what the summary kernels (stein_predict.hip) and the rank-counting kernels (stein_predict_ranks.hip)
// of the posterior predictive share: the geometry constants, the forward passes of the models as one body of device code --
// so a counted value is bit for bit the value pred holds -- and on the host side the plan of a call's grid, the GLM
// kernels' tile arithmetic (predict_glm_tile), the argument checks of the entry points and the network's columns as the
// kernels take them (predict_cols).  The models, the outputs and the mapping are described at the head of stein_predict.hip.
#pragma once
#include "stein_common.h"
#include <cfloat>

constexpr int PR_ROWS = 256;         // rows of X per workgroup: one per lane
constexpr int PR_PASS = 16;          // particles per pass: their outputs are 16 registers of every lane
constexpr int PR_SLICE_CAP = 1024;   // particle slices at most: the workspace is 20 bytes per (slice, row)
constexpr int PR_TARGET_WGS = 2048;  // workgroups wanted: eight per CU (the loops wait on LDS, so more resident workgroups
                                     // hide it; DESIGN.md 6e on what was and was not recorded); a small batch is filled
                                     // up with slices
constexpr int PR_FC = 58;            // GLM: features of the X tile per LDS chunk ([256][59] floats = 59 KB)
constexpr int PR_HC = 64;            // network: hidden units of the PR_PASS staged particles per LDS chunk
constexpr int PR_NIN_MAX = 4;        // the score producers' own limits
constexpr int PR_WIDTH_MAX = 1024;
// n and batch at most: the kernels index particles and rows in int and step past the end by less than a slice (p_begin + per
// < 2 n) or a row tile (row < batch + PR_ROWS) before they clamp, so both stay below 2^31
constexpr int64_t PR_COUNT_MAX = (int64_t)1 << 30;
constexpr float PR_HALF_LOG_2PI = 0.91893853320467274178f;

struct PredCols { int w1, b1, w2, b2, loggam; };

// ---- the forward passes ------------------------------------------------------------------------------------------------
// GLM: the walk of one workgroup over its slice [p_begin, p_end) of the particles, PR_PASS at a time.  fc = features per
// chunk (F when the whole X tile fits, else PR_FC), ld = floats per staged row of X (odd: lane t reads xs[t * ld + f], 64
// different banks); xs [PR_ROWS][ld] and ws [fc][PR_PASS] in LDS.  z[k] = x_row . w_(p0 + k) is summed over the features in
// order whatever the chunking.  between(p0, cnt): what the caller stages beside the first chunk's weights of a pass, between
// the two barriers; consume(p0, k, z): the lane's linear output of particle p0 + k, in particle order.  (z stays a local of
// this function: handed to a helper by reference, the inner loop came out with its LDS reads serialised, 7 % slower.)
template <class Between, class Consume>
__device__ __forceinline__ void pred_glm_slice(const float* theta, int d, int w_col, int F, int fc, int ld, const float* X, int B,
                                               int row0, int p_begin, int p_end, float* xs, float* ws, int t, Between&& between,
                                               Consume&& consume) {
  const int nfc = (F + fc - 1) / fc;
  auto stage_x = [&](int f0, int len) {   // rows past the batch are staged as zeros
    for (int i = t; i < PR_ROWS * len; i += 256) {
      const int r = i / len, f = i - r * len;
      xs[r * ld + f] = row0 + r < B ? X[(size_t)(row0 + r) * F + f0 + f] : 0.f;
    }
  };
  if (nfc == 1) stage_x(0, F);   // the whole tile fits: staged once for every particle of the slice
  for (int p0 = p_begin; p0 < p_end; p0 += PR_PASS) {
    const int cnt = min(PR_PASS, p_end - p0);
    float z[PR_PASS];
#pragma unroll
    for (int k = 0; k < PR_PASS; ++k) z[k] = 0.f;
    for (int c = 0; c < nfc; ++c) {
      const int f0 = c * fc, len = min(fc, F - f0);
      __syncthreads();   // every lane is past its last read of ws (and of xs)
      if (nfc > 1) stage_x(f0, len);
      for (int i = t; i < PR_PASS * len; i += 256) {
        const int k = i / len, f = i - k * len;
        ws[f * PR_PASS + k] = k < cnt ? theta[(size_t)(p0 + k) * d + w_col + f0 + f] : 0.f;
      }
      if (c == 0) between(p0, cnt);
      __syncthreads();
      const float* xr = xs + t * ld;
#pragma unroll 2
      for (int f = 0; f < len; ++f) {
        const float x = xr[f];
        const float4* w4 = reinterpret_cast<const float4*>(ws + f * PR_PASS);
#pragma unroll
        for (int q = 0; q < PR_PASS / 4; ++q) {
          const float4 w = w4[q];
          z[4 * q + 0] = fmaf(x, w.x, z[4 * q + 0]);
          z[4 * q + 1] = fmaf(x, w.y, z[4 * q + 1]);
          z[4 * q + 2] = fmaf(x, w.z, z[4 * q + 2]);
          z[4 * q + 3] = fmaf(x, w.w, z[4 * q + 3]);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < PR_PASS; ++k)
      if (k < cnt) consume(p0, k, z[k]);   // a particle past the slice's end is no particle: it is not counted as f = 0
  }
}

// the reported output of a GLM particle from its linear output
__device__ __forceinline__ float pred_glm_output(float zz, bool sigmoid) { return sigmoid ? 1.f / (1.f + expf(-zz)) : zz; }

// Network: z[k] of the cnt particles from p0 WITHOUT b2 (z comes in as zeros; f = z[k] + lp[k][0]).  x: the lane's NIN input
// features in registers; lw: the PR_PASS staged particles' b1, w2 and w1 rows of a chunk of PR_HC hidden units (hidden units
// past H are staged as zeros: relu(0) * 0 adds an exact zero); lp per particle: b2, 1/2 lg - 1/2 log 2 pi, 1/2 e^lg, and
// what extra(t) puts into lp[t][3] beside them (called by the thread that stages particle p0 + t).
template <int NIN>
constexpr int PR_BNN_PW = (NIN + 2) * PR_HC;   // staged floats per particle: b1 [PR_HC], w2 [PR_HC], w1 [NIN][PR_HC]

template <int NIN, class Extra>
__device__ __forceinline__ void pred_bnn_pass(float (&z)[PR_PASS], const float* theta, int d, int H,
                                              const PredCols& c, const float (&x)[NIN], int p0, int cnt,
                                              float* lw, float (*lp)[4], int t, Extra&& extra) {
  constexpr int PW = PR_BNN_PW<NIN>;
  for (int h0 = 0; h0 < H; h0 += PR_HC) {
    const int len = min(PR_HC, H - h0), len4 = (len + 3) & ~3;
    __syncthreads();   // every lane is past its last read of lw and lp
    for (int i = t; i < PR_PASS * len4; i += 256) {
      const int k = i / len4, h = i - k * len4;
      const bool ok = k < cnt && h < len;
      const float* th = theta + (size_t)(p0 + (ok ? k : 0)) * d + h0 + h;
      float* dst = lw + k * PW + h;
      dst[0] = ok ? th[c.b1] : 0.f;
      dst[PR_HC] = ok ? th[c.w2] : 0.f;
#pragma unroll
      for (int f = 0; f < NIN; ++f) dst[(2 + f) * PR_HC] = ok ? th[c.w1 + f * H] : 0.f;
    }
    if (h0 == 0 && t < cnt) {
      const float* th = theta + (size_t)(p0 + t) * d;
      const float lg = th[c.loggam];
      lp[t][0] = th[c.b2];
      lp[t][1] = fmaf(0.5f, lg, -PR_HALF_LOG_2PI);
      lp[t][2] = 0.5f * expf(lg);
      extra(t);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PR_PASS; ++k) {
      if (k < cnt) {
        const float* wk = lw + k * PW;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 2
        for (int h = 0; h < len4; h += 4) {
          float4 v = *reinterpret_cast<const float4*>(wk + h);
          const float4 w2 = *reinterpret_cast<const float4*>(wk + PR_HC + h);
#pragma unroll
          for (int f = 0; f < NIN; ++f) {
            const float4 w1 = *reinterpret_cast<const float4*>(wk + (2 + f) * PR_HC + h);
            v.x = fmaf(x[f], w1.x, v.x);
            v.y = fmaf(x[f], w1.y, v.y);
            v.z = fmaf(x[f], w1.z, v.z);
            v.w = fmaf(x[f], w1.w, v.w);
          }
          a0 = fmaf(fmaxf(v.x, 0.f), w2.x, a0);
          a1 = fmaf(fmaxf(v.y, 0.f), w2.y, a1);
          a2 = fmaf(fmaxf(v.z, 0.f), w2.z, a2);
          a3 = fmaf(fmaxf(v.w, 0.f), w2.w, a3);
        }
        z[k] += (a0 + a1) + (a2 + a3);
      }
    }
  }
}

// Network with more than PR_NIN_MAX input features (up to PR_WIDE_NIN_MAX): the lane's inputs no longer fit its registers, so
// the workgroup's X tile lies in LDS ([PR_ROWS][ld], ld odd; xr = the lane's row) and a particle's hidden units are taken
// PR_WT at a time: PR_WT accumulators start at b1, the features stream through them in ascending order (one own-row read of x
// and four 16-byte broadcasts of w1 per 16 FMAs), and relu(.) . w2 of the tile is summed in one fixed order.  Staging unit: ps
// particles x hc hidden units (hc a multiple of PR_WT; predict_wide_tile: hc = PR_WT, ps shrinks with n_in); per particle
// b1 [hc], w2 [hc], w1 [NIN][hc], hidden units past H staged as zeros.  (hc stays a run-time argument: with the unit fixed at
// PR_WT at compile time and the tile loop gone the kernel came out slower -- 5.21 against 3.88 ms at 90 inputs x 100 hidden x
// 1024 particles x 4000 rows, 2.66 against 2.49 ms at 13 x 50 x 16384 x 4000, profiles/bnn_wide_ab.txt B4; not looked into.)  z, lp and extra as in pred_bnn_pass.  What a particle's output is summed
// from, and in which order, follows from (NIN, H) alone: not from its place in the pass, cnt, or the slicing.
constexpr int PR_WT = 16;
constexpr int PR_WIDE_NIN_MAX = 128;
constexpr int PR_WIDE_W1_MAX = 16384;   // n_in * n_hidden at most
constexpr int PR_WIDE_LDS = 160 * 1024 / 4 - 128;   // floats of dynamic LDS at most (lp and some slack stay free)

template <class Extra>
__device__ __forceinline__ void pred_bnn_wide_pass(float (&z)[PR_PASS], const float* theta, int d, int NIN, int H,
                                                   const PredCols& c, const float* xr, int p0, int cnt, int ps, int hc,
                                                   float* lw, float (*lp)[4], int t, Extra&& extra) {
  const int pw = (NIN + 2) * hc;
  for (int k0 = 0; k0 < cnt; k0 += ps) {
    const int kn = min(ps, cnt - k0);
    for (int h0 = 0; h0 < H; h0 += hc) {
      const int len = min(hc, H - h0), len16 = (len + PR_WT - 1) & ~(PR_WT - 1);
      __syncthreads();   // every lane is past its last read of lw and lp
      for (int i = t; i < kn * len16; i += 256) {
        const int kk = i / len16, h = i - kk * len16;
        const bool ok = h < len;
        const float* th = theta + (size_t)(p0 + k0 + kk) * d + h0 + (ok ? h : 0);
        float* dst = lw + kk * pw + h;
        dst[0] = ok ? th[c.b1] : 0.f;
        dst[hc] = ok ? th[c.w2] : 0.f;
        for (int f = 0; f < NIN; ++f) dst[(2 + f) * hc] = ok ? th[c.w1 + f * H] : 0.f;
      }
      if (k0 == 0 && h0 == 0 && t < cnt) {
        const float* th = theta + (size_t)(p0 + t) * d;
        const float lg = th[c.loggam];
        lp[t][0] = th[c.b2];
        lp[t][1] = fmaf(0.5f, lg, -PR_HALF_LOG_2PI);
        lp[t][2] = 0.5f * expf(lg);
        extra(t);
      }
      __syncthreads();
      for (int kk = 0; kk < kn; ++kk) {
        const float* wk = lw + kk * pw;
        float sp = 0.f;
        for (int j = 0; j < len16; j += PR_WT) {
          float4 a[PR_WT / 4];
#pragma unroll
          for (int q = 0; q < PR_WT / 4; ++q) a[q] = *reinterpret_cast<const float4*>(wk + j + 4 * q);
#pragma unroll 2
          for (int f = 0; f < NIN; ++f) {
            const float x = xr[f];
            const float4* w4 = reinterpret_cast<const float4*>(wk + (2 + f) * hc + j);
#pragma unroll
            for (int q = 0; q < PR_WT / 4; ++q) {
              const float4 w = w4[q];
              a[q].x = fmaf(x, w.x, a[q].x);
              a[q].y = fmaf(x, w.y, a[q].y);
              a[q].z = fmaf(x, w.z, a[q].z);
              a[q].w = fmaf(x, w.w, a[q].w);
            }
          }
          float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
          for (int q = 0; q < PR_WT / 4; ++q) {
            const float4 w2 = *reinterpret_cast<const float4*>(wk + hc + j + 4 * q);
            s0 = fmaf(fmaxf(a[q].x, 0.f), w2.x, s0);
            s1 = fmaf(fmaxf(a[q].y, 0.f), w2.y, s1);
            s2 = fmaf(fmaxf(a[q].z, 0.f), w2.z, s2);
            s3 = fmaf(fmaxf(a[q].w, 0.f), w2.w, s3);
          }
          sp += (s0 + s1) + (s2 + s3);
        }
#pragma unroll
        for (int q = 0; q < PR_PASS; ++q) z[q] = q == k0 + kk ? z[q] + sp : z[q];   // (z stays in registers: no dynamic index)
      }
    }
  }
}

// ---- the weights of a weighted call as the lanes and the workspace hold them ---------------------------------------------------
// The header of a weighted call's workspace, in doubles: W (NaN: bad weights), sum w^2, then per slice W_s (0 after
// k_predict_wtotal when none of the slice's weights survives the rounding to fp32), sum w^2 and max w.  The states follow.
constexpr int PW_HEAD = 2;
__host__ __device__ constexpr size_t pw_doubles(int64_t slices) { return (size_t)(PW_HEAD + 3 * slices); }

// fl32(w / W) as the lanes hold it: below the normal range it counts as zero (whatever the denormal mode); W = NaN gives 0
__device__ __forceinline__ float pred_norm_weight(double w, double W) {
  const float q = (float)(w / W);
  return q >= FLT_MIN ? q : 0.f;
}

// ---- host side: the plan of a call's grid and the checks of the entry points -----------------------------------------------
struct PredPlan { int row_tiles, slices, per; };

static PredPlan predict_plan(int64_t n, int64_t batch) {
  PredPlan p;
  p.row_tiles = (int)((batch + PR_ROWS - 1) / PR_ROWS);
  int64_t s = (PR_TARGET_WGS + p.row_tiles - 1) / p.row_tiles;   // slices that fill the card at this batch
  if (s > PR_SLICE_CAP) s = PR_SLICE_CAP;
  const int64_t passes = (n + PR_PASS - 1) / PR_PASS;            // no slice of less than one pass
  if (s > passes) s = passes;
  p.per = (int)((n + s - 1) / s);
  p.slices = (int)((n + p.per - 1) / p.per);
  return p;
}

// the GLM kernels' LDS beside what a kernel adds of its own: the X tile and a pass's staged weights, and with extra_row the
// PR_PASS words a weighted kernel stages behind them (normalised weights, masses)
struct PredGlmTile { int fc, ld; size_t bytes; };

static PredGlmTile predict_glm_tile(int64_t n_feats, bool extra_row) {
  const int fc = (int)(n_feats <= PR_FC ? n_feats : PR_FC);
  const int ld = fc | 1;
  return {fc, ld, ((size_t)PR_ROWS * ld + (size_t)fc * PR_PASS + (extra_row ? PR_PASS : 0)) * sizeof(float)};
}

// the weights of a weighted call (on = false: an unweighted call, for which every check and launch is what it was)
struct PredWeights { bool on; const double* w; double* ess; };

// the weight pass of a weighted call (stein_predict.hip): W, sum w^2 and the per-slice sums of pl's slices into the header at
// the start of `workspace`, and ess when pw.ess is set; queued ahead of the forward kernel that reads the header
int predict_weight_pass(const PredPlan& pl, int64_t n, const PredWeights& pw, void* workspace, hipStream_t s);

// the checks the entry points share, in the order the header lists them
static int predict_check(const float* theta, const float* X, const float* y, int64_t n, int64_t d, int64_t batch,
                         int64_t width, int output, const float* pred, const float* mean, const float* var,
                         const float* lpd, const PredWeights& pw) {
  if (!theta || !X || (pw.on && !pw.w)) return stein_fail(STEIN_E_BADARG, "NULL pointer");
  if (!pred && !mean && !var && !lpd && !pw.ess)
    return stein_fail(STEIN_E_BADARG, pw.on ? "no output requested: pred, mean, var, lpd and ess are all NULL"
                                            : "no output requested: pred, mean, var and lpd are all NULL");
  if (lpd && !y) return stein_fail(STEIN_E_BADARG, "lpd needs y");
  if (output != STEIN_PRED_LINK && output != STEIN_PRED_MEAN) return stein_fail(STEIN_E_BADARG, "output %d", output);
  if (n < 1 || d < 1 || batch < 1 || width < 1 || n > PR_COUNT_MAX || d > 0x7fffffffl || batch > PR_COUNT_MAX)
    return stein_fail(STEIN_E_SHAPE, "bad shape n=%lld d=%lld batch=%lld width=%lld", (long long)n, (long long)d,
                      (long long)batch, (long long)width);
  return STEIN_OK;
}

// the GLM entry points' own checks, behind predict_check
static int predict_check_glm(int kind, int64_t w_col, int64_t n_feats, int64_t d) {
  if (kind != STEIN_GLM_LINEAR && kind != STEIN_GLM_LOGISTIC) return stein_fail(STEIN_E_BADARG, "kind %d", kind);
  if (w_col < 0 || w_col + n_feats > d)
    return stein_fail(STEIN_E_SHAPE, "weights [%lld, %lld) do not fit d=%lld", (long long)w_col, (long long)(w_col + n_feats),
                      (long long)d);
  if (n_feats > PR_WIDTH_MAX) return stein_fail(STEIN_E_UNSUPPORTED, "more than 1024 features per particle");
  return STEIN_OK;
}

// the network's six column blocks fit d and do not overlap
static int predict_check_cols(const int64_t* cols, int64_t n_in, int64_t n_hidden, int64_t d) {
  const int64_t len[6] = {n_in * n_hidden, n_hidden, n_hidden, 1, 1, 1};
  for (int i = 0; i < 6; ++i) {
    if (cols[i] < 0 || cols[i] + len[i] > d) return stein_fail(STEIN_E_SHAPE, "block %d does not fit d=%lld", i, (long long)d);
    for (int j = 0; j < i; ++j)
      if (cols[i] < cols[j] + len[j] && cols[j] < cols[i] + len[i]) return stein_fail(STEIN_E_SHAPE, "blocks %d and %d overlap", j, i);
  }
  return STEIN_OK;
}

// the network entry points' own checks, behind predict_check (cols != NULL is checked ahead of it)
static int predict_check_bnn(int64_t n_in, int64_t n_hidden, const int64_t* cols, int64_t d) {
  if (n_in < 1) return stein_fail(STEIN_E_SHAPE, "bad shape n_in=%lld", (long long)n_in);
  if (n_in > PR_NIN_MAX) return stein_fail(STEIN_E_UNSUPPORTED, "more than %d input features", PR_NIN_MAX);
  if (n_hidden > PR_WIDTH_MAX) return stein_fail(STEIN_E_UNSUPPORTED, "more than 1024 hidden units");
  return predict_check_cols(cols, n_in, n_hidden, d);
}

// the wide network entry points' own checks (n_in > PR_NIN_MAX), in the place of predict_check_bnn
static int predict_check_bnn_wide(int64_t n_in, int64_t n_hidden, const int64_t* cols, int64_t d) {
  if (n_in < 1) return stein_fail(STEIN_E_SHAPE, "bad shape n_in=%lld", (long long)n_in);
  if (n_in > PR_WIDE_NIN_MAX) return stein_fail(STEIN_E_UNSUPPORTED, "more than %d input features", PR_WIDE_NIN_MAX);
  if (n_hidden > PR_WIDTH_MAX) return stein_fail(STEIN_E_UNSUPPORTED, "more than 1024 hidden units");
  if (n_in * n_hidden > PR_WIDE_W1_MAX)
    return stein_fail(STEIN_E_UNSUPPORTED, "more than %d first-layer weights (n_in * n_hidden)", PR_WIDE_W1_MAX);
  return predict_check_cols(cols, n_in, n_hidden, d);
}

// the wide network kernels' LDS: the X tile [PR_ROWS][ld] and behind it the staging unit of ps particles x hc hidden units:
// one tile of PR_WT hidden units of as many of a pass's PR_PASS particles as the LDS holds beside the X tile -- all of them up
// to n_in = 78, 11 at 90, 3 at 128 (where the X tile alone is 129 KB).  Measured (profiles/bnn_wide_ab.txt): more hidden units
// per unit cost resident workgroups at 13 inputs (16 | 32 | 64 units: 2.33 | 2.65 | 2.99 ms), fewer particles cost barriers at
// 90 (2 | 5 | 11 particles: 6.37 | 4.67 | 3.86 ms).
struct PredWideTile { int ld, ps, hc; size_t bytes; };

static PredWideTile predict_wide_tile(int64_t n_in) {
  PredWideTile w;
  w.hc = PR_WT;
  w.ld = (int)(n_in | 1);
  const int xt = PR_ROWS * w.ld, unit = (int)(n_in + 2) * PR_WT;
  w.ps = (PR_WIDE_LDS - xt) / unit;
  if (w.ps > PR_PASS) w.ps = PR_PASS;
  w.bytes = ((size_t)xt + (size_t)w.ps * unit) * sizeof(float);
  return w;
}

// the network's columns as the kernels take them (log_lambda, cols[4], enters no output)
static PredCols predict_cols(const int64_t* cols) {
  return {(int)cols[0], (int)cols[1], (int)cols[2], (int)cols[3], (int)cols[5]};
}
