// stein_predict_softmax.hip -- posterior predictive of softmax regression (the model of stein_score_softmax.hip): the
// class probabilities of every particle, read out as pred[n][batch][C] and / or as per-test-point summaries that never
// materialise [n][batch][C]:
//   z_pbc  = sum_f x_bf W_p,fc,   p_pb. = softmax(z_pb.) with the row maximum subtracted
//   pred   STEIN_PRED_MEAN: p_pbc;  STEIN_PRED_LINK: z_pbc
//   prob_bc = 1/n sum_p p_pbc                      the posterior predictive class probabilities
//   lpd_b   = log(1/n sum_p p_{pb,y_b})            needs labels; a label outside [0, C) gives NaN in its row
//   ent_b   = 1/n sum_p H(p_pb.)                   H = log s - sum_c p_c t_c with t = z - max z, s = sum_c exp(t_c): this is
//                                                  logsumexp(z) - sum_c p_c z_c with the maximum taken out of both terms
//   label_b = argmax_c prob_bc, ties to the lowest class, taken of the very floats prob receives
//
// Mapping: that of stein_predict.hip -- rows of X on the lanes, a workgroup owns PR_ROWS rows x one slice of the particles
// (predict_plan), the X tile [PR_ROWS][ld] in LDS, whole up to PR_FC features and in chunks of PR_FC past them
// (predict_glm_tile).  A pass stages NA = max(PR_PASS, CP) columns of weights, (particle, class) pairs: PR_PASS / CP
// particles for the padded class count CP = 4, 8, 16 and one particle for CP = 32; every lane reads them at one address,
// 16 bytes a read.  pred_glm_slice itself does not serve: it takes a column's features at stride 1 and here they lie at
// stride C.  The running state is C + 2 fp32 sums per lane (the class probabilities, p at the true label, the entropy): all
// terms are non-negative, so a plain sum per slice.  k_predict_softmax_finish merges the slices in slice order in fp64.  No
// atomics; every workspace word that is read was written by the same call.
//
// Weighted form (stein_predict_softmax_weighted; the WEIGHTED instantiations): per-particle weights w_p >= 0 in fp64, W their
// sum, prob_bc = sum_p w_p p_pbc / W and so on (include/steinhip.h).  The weight pass of stein_predict.hip
// (predict_weight_pass) leaves W at the head of the workspace; the kernel stages the lane weights fl32(w_p / W) of PS_WB
// particles at a time behind the staged model weights -- one fp64 quotient per particle and workgroup, taken by the thread
// that stages it -- and every lane reads them at one address.  The running sums become acc = fmaf(w, q, acc), particles
// ascending; a particle of lane weight zero skips its softmax tail unless pred wants it, and without pred a pass whose
// particles all have lane weight zero is neither staged nor computed (one branch for the whole workgroup: the weights come
// from LDS at one address).  The lane weights sum to 1, so the finish divides by nothing.
#include "stein_predict_fwd.h"

constexpr int PS_C_MIN = 2, PS_C_MAX = 32, PS_FC_MAX = 16384;
constexpr int PS_WB = 64;   // WEIGHTED: particles whose lane weights are staged at a time (a multiple of every PP)

// a value every lane holds alike, as the scalar the branches on it want
__device__ __forceinline__ float ps_uniform(float v) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

// WEIGHTED: wts [n] the weights, head the weight pass's header (head[0] = W)
template <int CP, bool WEIGHTED>
__global__ __launch_bounds__(256) void k_predict_softmax(const float* __restrict__ theta, int n, int d, int w_col, int F, int C,
                                                         int output, int fc, int ld, const float* __restrict__ X,
                                                         const int* __restrict__ labels, int B, int per,
                                                         float* __restrict__ pred, float* __restrict__ part, int want_lpd,
                                                         const double* __restrict__ wts,
                                                         const double* __restrict__ head) {
  constexpr int NA = CP > PR_PASS ? CP : PR_PASS;   // staged columns of a pass
  constexpr int PP = NA / CP;                       // its particles
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xs = lds;                                  // [PR_ROWS][ld]
  float* ws = lds + ((PR_ROWS * ld + 3) & ~3);      // [fc][NA]
  [[maybe_unused]] float* wl = ws + fc * NA;        // [PS_WB], WEIGHTED only
  [[maybe_unused]] double wtot = 0.0;
  if constexpr (WEIGHTED) wtot = head[0];
  const int t = threadIdx.x;
  const int row0 = blockIdx.x * PR_ROWS, row = row0 + t;
  const bool live = row < B;
  const int p_begin = blockIdx.y * per, p_end = min(n, p_begin + per);
  const int yb = (want_lpd && live) ? labels[row] : 0;
  const int nfc = (F + fc - 1) / fc;
  auto stage_x = [&](int f0, int len) {   // rows past the batch are staged as zeros
    for (int i = t; i < PR_ROWS * len; i += 256) {
      const int r = i / len, f = i - r * len;
      xs[r * ld + f] = row0 + r < B ? X[(size_t)(row0 + r) * F + f0 + f] : 0.f;
    }
  };
  if (nfc == 1) stage_x(0, F);            // the whole tile fits: staged once for every particle of the slice
  float acc[CP], acc_y = 0.f, acc_h = 0.f;
#pragma unroll
  for (int c = 0; c < CP; ++c) acc[c] = 0.f;
  for (int p0 = p_begin; p0 < p_end; p0 += PP) {
    const int cnt = min(PP, p_end - p0);
    [[maybe_unused]] int wo = 0;                    // the pass's place in wl
    if constexpr (WEIGHTED) {
      wo = (p0 - p_begin) % PS_WB;
      if (wo == 0) {
        __syncthreads();   // every lane is past its last read of wl
        if (t < PS_WB) wl[t] = p0 + t < p_end ? pred_norm_weight(wts[p0 + t], wtot) : 0.f;
        __syncthreads();
      }
      bool any = false;
#pragma unroll
      for (int pk = 0; pk < PP; ++pk) any = any || ps_uniform(wl[wo + pk]) != 0.f;
      if (!pred && !any) continue;   // a dead pass: nothing of it is staged or computed
    }
    float z[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) z[k] = 0.f;
    for (int ch = 0; ch < nfc; ++ch) {
      const int f0 = ch * fc, len = min(fc, F - f0);
      __syncthreads();   // every lane is past its last read of ws (and of xs)
      if (nfc > 1) stage_x(f0, len);
      for (int i = t; i < len * NA; i += 256) {
        const int f = i / NA, k = i - f * NA, pk = k / CP, c = k - pk * CP;
        ws[i] = (pk < cnt && c < C) ? theta[(size_t)(p0 + pk) * d + w_col + (size_t)(f0 + f) * C + c] : 0.f;
      }
      __syncthreads();
      const float* xr = xs + t * ld;
#pragma unroll 2
      for (int f = 0; f < len; ++f) {
        const float x = xr[f];
        const float4* w4 = reinterpret_cast<const float4*>(ws + f * NA);
#pragma unroll
        for (int q = 0; q < NA / 4; ++q) {
          const float4 w = w4[q];
          z[4 * q + 0] = fmaf(x, w.x, z[4 * q + 0]);
          z[4 * q + 1] = fmaf(x, w.y, z[4 * q + 1]);
          z[4 * q + 2] = fmaf(x, w.z, z[4 * q + 2]);
          z[4 * q + 3] = fmaf(x, w.w, z[4 * q + 3]);
        }
      }
    }
#pragma unroll
    for (int pk = 0; pk < PP; ++pk) {
      [[maybe_unused]] float wv = 0.f;
      if constexpr (WEIGHTED) wv = ps_uniform(wl[wo + pk]);
      if (pk < cnt && (!WEIGHTED || pred || wv != 0.f)) {    // a particle past the slice's end is no particle
        float* out = (pred && live) ? pred + ((size_t)(p0 + pk) * B + row) * C : nullptr;
        float m = z[pk * CP];
#pragma unroll
        for (int c = 1; c < CP; ++c)
          if (c < C) m = fmaxf(m, z[pk * CP + c]);
        if (out && output == STEIN_PRED_LINK) {
#pragma unroll
          for (int c = 0; c < CP; ++c)
            if (c < C) out[c] = z[pk * CP + c];
        }
        float s = 0.f, e[CP];
#pragma unroll
        for (int c = 0; c < CP; ++c) {
          z[pk * CP + c] = c < C ? z[pk * CP + c] - m : 0.f;   // t_c <= 0
          e[c] = c < C ? expf(z[pk * CP + c]) : 0.f;
          s += e[c];
        }
        float pt = 0.f, py = (yb < 0 || yb >= C) ? __builtin_nanf("") : 0.f;
#pragma unroll
        for (int c = 0; c < CP; ++c) {
          const float pc = e[c] / s;
          if (out && output != STEIN_PRED_LINK && c < C) out[c] = pc;
          if constexpr (WEIGHTED) {
            if (wv != 0.f) acc[c] = fmaf(wv, pc, acc[c]);
          } else {
            acc[c] += pc;
          }
          pt = fmaf(pc, z[pk * CP + c], pt);
          py = (c == yb && c < C) ? pc : py;   // (a label in [C, CP) is no class: py stays NaN)
        }
        if constexpr (WEIGHTED) {
          if (wv != 0.f) {   // (weight zero: the particle enters no sum, whatever its probabilities are)
            acc_y = fmaf(wv, py, acc_y);
            acc_h = fmaf(wv, logf(s) - pt, acc_h);
          }
        } else {
          acc_y += py;
          acc_h += logf(s) - pt;
        }
      }
    }
  }
  if (live && part) {    // [slice][C + 2][B]
    float* ps = part + (size_t)blockIdx.y * (C + 2) * B + row;
#pragma unroll
    for (int c = 0; c < CP; ++c)
      if (c < C) ps[(size_t)c * B] = acc[c];
    ps[(size_t)C * B] = acc_y;
    ps[(size_t)(C + 1) * B] = acc_h;
  }
}

// The slices' sums merged in slice order, in fp64: PSF_ROWS rows per workgroup, the C + 2 quantities of a row over eight
// threads; then one thread per row takes the argmax of the floats prob received (through LDS; written whether or not prob
// is wanted).  WEIGHTED: the lane weights sum to 1, so nothing is divided; bad weights (the header's W is NaN) give NaN rows
// and the label -1.
constexpr int PSF_ROWS = 32;

template <bool WEIGHTED>
__global__ __launch_bounds__(256) void k_predict_softmax_finish(const float* __restrict__ part, int slices, int n, int B, int C,
                                                                float* __restrict__ prob, float* __restrict__ lpd,
                                                                float* __restrict__ ent, int* __restrict__ label,
                                                                const double* __restrict__ head) {
  __shared__ float pr[PSF_ROWS][PS_C_MAX + 1];
  [[maybe_unused]] bool bad = false;
  if constexpr (WEIGHTED) bad = !(head[0] > 0.0);   // a negative or non-finite weight, W = 0 or an overflowing W
  const int r = threadIdx.x % PSF_ROWS, ql = threadIdx.x / PSF_ROWS;
  const int b = blockIdx.x * PSF_ROWS + r;
  if (b < B) {
    for (int q = ql; q < C + 2; q += 256 / PSF_ROWS) {
      if ((q == C && !lpd) || (q == C + 1 && !ent) || (q < C && !prob && !label)) continue;
      const float* p = part + (size_t)q * B + b;
      double sum = 0.0;
      for (int s = 0; s < slices; ++s) sum += (double)p[(size_t)s * (C + 2) * B];
      if constexpr (WEIGHTED) {
        if (bad) sum = (double)NAN;
      } else {
        sum /= (double)n;
      }
      if (q < C) {
        const float v = (float)sum;
        pr[r][q] = v;
        if (prob) prob[(size_t)b * C + q] = v;
      } else if (q == C) {
        lpd[b] = (float)log(sum);
      } else {
        ent[b] = (float)sum;
      }
    }
  }
  __syncthreads();
  if (label && ql == 0 && b < B) {
    int best = 0;
    float top = pr[r][0];
    for (int c = 1; c < C; ++c)
      if (pr[r][c] > top) {
        top = pr[r][c];
        best = c;
      }
    if constexpr (WEIGHTED) best = bad ? -1 : best;
    label[b] = best;
  }
}

// (C + 2) floats per state; the states' count is bounded as in stein_predict.hip: monotone in n and batch
static size_t predict_softmax_ws_bytes(int64_t n, int64_t batch, int64_t n_classes) {
  int64_t s = (n + PR_PASS - 1) / PR_PASS;
  if (s > PR_SLICE_CAP) s = PR_SLICE_CAP;
  int64_t states = s * batch;
  const int64_t by_target = (int64_t)PR_TARGET_WGS * PR_ROWS + batch;
  if (states > by_target) states = by_target;
  return (size_t)states * (size_t)(n_classes + 2) * sizeof(float);
}

static int predict_softmax_domain(int64_t n_feats, int64_t n_classes) {
  if (n_classes < PS_C_MIN) return stein_fail(STEIN_E_UNSUPPORTED, "fewer than %d classes", PS_C_MIN);
  if (n_classes > PS_C_MAX) return stein_fail(STEIN_E_UNSUPPORTED, "more than %d classes", PS_C_MAX);
  if (n_feats > PR_WIDTH_MAX) return stein_fail(STEIN_E_UNSUPPORTED, "more than %d features", PR_WIDTH_MAX);
  if (n_feats * n_classes > PS_FC_MAX)
    return stein_fail(STEIN_E_UNSUPPORTED, "more than %d weights (n_feats * n_classes)", PS_FC_MAX);
  return STEIN_OK;
}

// the 32-class kernel takes 66 KB of dynamic LDS at 58 features and more: raise each kernel's limit once per device
static int predict_softmax_attr(const void* fn, int slot) {
  static bool attr_set[8][64] = {{false}};
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64 || !attr_set[slot][dev]) {
    HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024));
    if (dev >= 0 && dev < 64) attr_set[slot][dev] = true;
  }
  return STEIN_OK;
}

// the workspace of a weighted call: the weight pass's header of the slice bound ahead of the states; monotone too
static size_t predict_softmax_wws_bytes(int64_t n, int64_t batch, int64_t n_classes) {
  int64_t s = (n + PR_PASS - 1) / PR_PASS;
  if (s > PR_SLICE_CAP) s = PR_SLICE_CAP;
  return pw_doubles(s) * sizeof(double) + predict_softmax_ws_bytes(n, batch, n_classes);
}

static int predict_softmax_ws_check(int64_t n, int64_t batch, int64_t n_classes, size_t* out_bytes, bool weighted) {
  if (!out_bytes) return stein_fail(STEIN_E_BADARG, "NULL pointer");
  if (n < 1 || batch < 1 || n_classes < 1 || n > PR_COUNT_MAX || batch > PR_COUNT_MAX)
    return stein_fail(STEIN_E_SHAPE, "bad shape n=%lld batch=%lld C=%lld", (long long)n, (long long)batch, (long long)n_classes);
  if (int rc = predict_softmax_domain(1, n_classes)) return rc;
  *out_bytes = weighted ? predict_softmax_wws_bytes(n, batch, n_classes) : predict_softmax_ws_bytes(n, batch, n_classes);
  return STEIN_OK;
}

extern "C" int stein_predict_softmax_workspace_bytes(int64_t n, int64_t batch, int64_t n_classes, size_t* out_bytes) {
  return predict_softmax_ws_check(n, batch, n_classes, out_bytes, false);
}

extern "C" int stein_predict_softmax_weighted_workspace_bytes(int64_t n, int64_t batch, int64_t n_classes, size_t* out_bytes) {
  return predict_softmax_ws_check(n, batch, n_classes, out_bytes, true);
}

// both entry points (pw.on = false: the unweighted call, for which every check and launch is what it was)
static int predict_softmax(const float* theta, int64_t n, int64_t d, int output, int64_t w_col, int64_t n_feats,
                           int64_t n_classes, const float* X, const int32_t* labels, int64_t batch, float* pred, float* prob,
                           float* lpd, float* ent, int32_t* label, void* workspace, size_t ws_bytes, void* stream,
                           const PredWeights& pw) {
  if (!theta || !X || (pw.on && !pw.w)) return stein_fail(STEIN_E_BADARG, "NULL pointer");
  if (!pred && !prob && !lpd && !ent && !label && !pw.ess)
    return stein_fail(STEIN_E_BADARG, pw.on ? "no output requested: pred, prob, lpd, ent, label and ess are all NULL"
                                            : "no output requested: pred, prob, lpd, ent and label are all NULL");
  if (lpd && !labels) return stein_fail(STEIN_E_BADARG, "lpd needs labels");
  if (output != STEIN_PRED_LINK && output != STEIN_PRED_MEAN) return stein_fail(STEIN_E_BADARG, "output %d", output);
  if (n < 1 || d < 1 || batch < 1 || n_feats < 1 || n_classes < 1 || n > PR_COUNT_MAX || d > 0x7fffffffl || batch > PR_COUNT_MAX)
    return stein_fail(STEIN_E_SHAPE, "bad shape n=%lld d=%lld batch=%lld F=%lld C=%lld", (long long)n, (long long)d,
                      (long long)batch, (long long)n_feats, (long long)n_classes);
  if (int rc = predict_softmax_domain(n_feats, n_classes)) return rc;
  if (w_col < 0 || w_col + n_feats * n_classes > d)
    return stein_fail(STEIN_E_SHAPE, "weights [%lld, %lld) do not fit d=%lld", (long long)w_col,
                      (long long)(w_col + n_feats * n_classes), (long long)d);
  const bool summary = prob || lpd || ent || label;   // the rows the forward kernel reduces; ess comes from the weight pass alone
  if (summary || pw.ess) {
    if (!workspace)
      return stein_fail(STEIN_E_WORKSPACE,
                        pw.on ? "prob, lpd, ent, label and ess need a workspace (stein_predict_softmax_weighted_workspace_bytes)"
                              : "prob, lpd, ent and label need a workspace (stein_predict_softmax_workspace_bytes)");
    const size_t need = pw.on ? predict_softmax_wws_bytes(n, batch, n_classes) : predict_softmax_ws_bytes(n, batch, n_classes);
    if (ws_bytes < need) return stein_fail(STEIN_E_WORKSPACE, "workspace too small: %zu < %zu bytes", ws_bytes, need);
    if (pw.on && (uintptr_t)workspace % sizeof(double))
      return stein_fail(STEIN_E_WORKSPACE, "the workspace of a weighted call must be 8-byte aligned");
  }
  const PredPlan pl = predict_plan(n, batch);
  const int C = (int)n_classes, na = C > PR_PASS ? 32 : PR_PASS;
  const int fc = (int)(n_feats <= PR_FC ? n_feats : PR_FC), ld = fc | 1;
  hipStream_t s = (hipStream_t)stream;
  if (pw.on && (summary || pw.ess))
    if (int rc = predict_weight_pass(pl, n, pw, workspace, s)) return rc;
  if (!pred && !summary) return STEIN_OK;   // ess alone
  // a weighted call that only asks for pred runs the unweighted kernel: pred does not depend on the weights
  const double* head = (pw.on && summary) ? (const double*)workspace : nullptr;
  float* part = !summary ? nullptr : head ? (float*)((double*)workspace + pw_doubles(pl.slices)) : (float*)workspace;
  const size_t lds_bytes = ((size_t)((PR_ROWS * ld + 3) & ~3) + (size_t)fc * na + (head ? PS_WB : 0)) * sizeof(float);
#define PS_LAUNCH_AS(CP, WEIGHTED, SLOT)                                                                                 \
  do {                                                                                                                   \
    if (int rc = predict_softmax_attr(reinterpret_cast<const void*>(k_predict_softmax<CP, WEIGHTED>), SLOT)) return rc;  \
    hipLaunchKernelGGL((k_predict_softmax<CP, WEIGHTED>), dim3((unsigned)pl.row_tiles, (unsigned)pl.slices), dim3(256),   \
                       lds_bytes, s, theta, (int)n, (int)d, (int)w_col, (int)n_feats, C, output, fc, ld, X, labels,       \
                       (int)batch, pl.per, pred, part, lpd ? 1 : 0, pw.w, head);                                          \
  } while (0)
#define PS_LAUNCH(CP, SLOT)                                                                                              \
  do {                                                                                                                   \
    if (head) PS_LAUNCH_AS(CP, true, 4 + SLOT);                                                                          \
    else PS_LAUNCH_AS(CP, false, SLOT);                                                                                  \
  } while (0)
  if (C <= 4) PS_LAUNCH(4, 0);
  else if (C <= 8) PS_LAUNCH(8, 1);
  else if (C <= 16) PS_LAUNCH(16, 2);
  else PS_LAUNCH(32, 3);
#undef PS_LAUNCH
#undef PS_LAUNCH_AS
  LAUNCH_CHECK("k_predict_softmax");
  if (!summary) return STEIN_OK;
  const dim3 grid((unsigned)((batch + PSF_ROWS - 1) / PSF_ROWS));
  if (head) hipLaunchKernelGGL(k_predict_softmax_finish<true>, grid, dim3(256), 0, s, part, pl.slices, (int)n, (int)batch, C, prob, lpd, ent, label, head);
  else hipLaunchKernelGGL(k_predict_softmax_finish<false>, grid, dim3(256), 0, s, part, pl.slices, (int)n, (int)batch, C, prob, lpd, ent, label, head);
  LAUNCH_CHECK("k_predict_softmax_finish");
  return STEIN_OK;
}

extern "C" int stein_predict_softmax(const float* theta, int64_t n, int64_t d, int output, int64_t w_col, int64_t n_feats,
                                     int64_t n_classes, const float* X, const int32_t* labels, int64_t batch, float* pred,
                                     float* prob, float* lpd, float* ent, int32_t* label, void* workspace, size_t ws_bytes,
                                     void* stream) {
  return predict_softmax(theta, n, d, output, w_col, n_feats, n_classes, X, labels, batch, pred, prob, lpd, ent, label,
                         workspace, ws_bytes, stream, PredWeights{false, nullptr, nullptr});
}

extern "C" int stein_predict_softmax_weighted(const float* theta, int64_t n, int64_t d, int output, int64_t w_col,
                                              int64_t n_feats, int64_t n_classes, const float* X, const int32_t* labels,
                                              int64_t batch, const double* weights, float* pred, float* prob, float* lpd,
                                              float* ent, int32_t* label, double* ess, void* workspace, size_t ws_bytes,
                                              void* stream) {
  return predict_softmax(theta, n, d, output, w_col, n_feats, n_classes, X, labels, batch, pred, prob, lpd, ent, label,
                         workspace, ws_bytes, stream, PredWeights{true, weights, ess});
}
