// stein_predict_bnn_class.hip -- posterior predictive of the network classifier (the model of stein_score_bnn_class.hip): the
// class probabilities of every particle, read out as pred[n][batch][C] and / or as the per-test-point summaries of
// stein_predict_softmax.hip (prob, lpd, ent, label: their definitions are written at its head), never materialising
// [n][batch][C]:
//   pre_pbh = b1_ph + sum_f x_bf w1_pfh (f ascending),  z_pbc = b2_pc + sum_h relu(pre_pbh) w2_phc (h ascending)
//   p_pb.   = softmax(z_pb.) with the row maximum subtracted;  pred  STEIN_PRED_MEAN: p_pbc;  STEIN_PRED_LINK: z_pbc
//
// Mapping: that of the summary kernels -- rows of X on the lanes, a workgroup owns PR_ROWS rows x one slice of the particles
// (predict_plan), the X tile [PR_ROWS][ld] in LDS as in predict_wide_tile, for every n_in from 1 to 128.  A particle is walked
// in tiles of PR_WT hidden units; the (particle, tile) pairs of the slice form one sequence and a staging unit holds the next
// ps of them (as many as the LDS holds beside the X tile, PR_PASS at most; hidden units past H are staged as zeros), per
// pair b1 [16], w1 [n_in][16], w2 [16][CS] and b2 [CS].  A lane carries the tile's 16 accumulators and CP logits: they start
// at b2 with a particle's first tile, take relu(acc_q) w2[q][c] from 16-byte broadcast reads after every tile, and go
// through the softmax and the C + 2 running sums of k_predict_softmax after its last.  What a particle's outputs are summed
// from, and in which order, follows from (n_in, H, C) alone: not from its place in the unit, the slice or the grid.
// k_predict_bnn_class_finish merges the slices in slice order in fp64.  No atomics; every workspace word that is read was
// written by the same call.
//
// Weighted form (stein_predict_bnn_class_weighted; the WEIGHTED instantiations), as stein_predict_softmax.hip describes it:
// the lane weights fl32(w_p / W) of PC_WB particles at a time lie behind the staging unit (restaged when a unit's last
// particle passes their end), the running sums become acc = fmaf(w, q, acc), and without pred a particle of lane weight
// zero is not computed and a unit all of whose (particle, tile) items belong to such particles is not staged either.  A
// particle whose tiles straddle a skipped unit has weight zero itself; what its remaining tiles would add to the logits is
// never computed, and the next particle's first tile sets the logits to its b2 (tile == 0 below).
#include "stein_predict_fwd.h"

constexpr int PC_NIN_MAX = 128, PC_C_MIN = 2, PC_C_MAX = 32, PC_H_MAX = 512, PC_W_MAX = 16384;

constexpr int PC_WB = 64;   // WEIGHTED: particles whose lane weights are staged at a time (more than a unit's PR_PASS + 1)

struct PredClassCols { int w1, b1, w2, b2; };

// a value every lane holds alike, as the scalar the branches on it want
__device__ __forceinline__ float pc_uniform(float v) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

// floats of a staged (particle, tile) pair
static __host__ __device__ inline int pc_item_floats(int F, int CS) { return (F + 1 + CS) * PR_WT + CS; }

// WEIGHTED: wts [n] the weights, head the weight pass's header (head[0] = W)
template <int CP, bool WEIGHTED>
__global__ __launch_bounds__(256) void k_predict_bnn_class(const float* __restrict__ theta, int n, int d, int F, int H, int C,
                                                           PredClassCols c, int output, int ld, int ps,
                                                           const float* __restrict__ X, const int* __restrict__ labels, int B,
                                                           int per, float* __restrict__ pred, float* __restrict__ part,
                                                           int want_lpd, const double* __restrict__ wts,
                                                           const double* __restrict__ head) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int CS = (C + 3) & ~3, cq = CS / 4, iw = pc_item_floats(F, CS);
  const int o_w1 = PR_WT, o_w2 = o_w1 + F * PR_WT, o_b2 = o_w2 + PR_WT * CS;
  float* xs = lds;                                  // [PR_ROWS][ld]
  float* ws = lds + ((PR_ROWS * ld + 3) & ~3);      // [ps][iw]
  [[maybe_unused]] float* wl = ws + ps * iw;        // [PC_WB], WEIGHTED only
  [[maybe_unused]] double wtot = 0.0;
  if constexpr (WEIGHTED) wtot = head[0];
  [[maybe_unused]] int wb0 = -PC_WB;                // the first particle of wl, counted from p_begin
  const int t = threadIdx.x;
  const int row0 = blockIdx.x * PR_ROWS, row = row0 + t;
  const bool live = row < B;
  const int p_begin = blockIdx.y * per, p_end = min(n, p_begin + per);
  const int yb = (want_lpd && live) ? labels[row] : 0;
  const int nt = (H + PR_WT - 1) / PR_WT;
  const long items = (long)(p_end - p_begin) * nt;
  for (int i = t; i < PR_ROWS * F; i += 256) {      // rows past the batch are staged as zeros
    const int r = i / F, f = i - r * F;
    xs[r * ld + f] = row0 + r < B ? X[(size_t)(row0 + r) * F + f] : 0.f;
  }
  const float* xr = xs + t * ld;
  float acc[CP], acc_y = 0.f, acc_h = 0.f, z[CP];
#pragma unroll
  for (int cc = 0; cc < CP; ++cc) acc[cc] = z[cc] = 0.f;
  for (long j0 = 0; j0 < items; j0 += ps) {
    const int cnt = (int)min((long)ps, items - j0);
    if constexpr (WEIGHTED) {
      const int k0 = (int)(j0 / nt), k1 = (int)((j0 + cnt - 1) / nt);   // the unit's particles
      if (k1 >= wb0 + PC_WB) {
        wb0 = k0;
        __syncthreads();   // every lane is past its last read of wl
        if (t < PC_WB) wl[t] = p_begin + wb0 + t < p_end ? pred_norm_weight(wts[p_begin + wb0 + t], wtot) : 0.f;
        __syncthreads();
      }
      bool any = false;
      for (int k = k0; k <= k1; ++k) any = any || pc_uniform(wl[k - wb0]) != 0.f;
      if (!pred && !any) continue;   // a dead unit: nothing of it is staged or computed
    }
    __syncthreads();     // every lane is past its last read of ws
    for (int i = t; i < cnt * iw; i += 256) {
      const int it = i / iw, o = i - it * iw;
      const long j = j0 + it;
      const int pk = (int)(j / nt), h0 = (int)(j - (long)pk * nt) * PR_WT;
      const float* th = theta + (size_t)(p_begin + pk) * d;
      float v;
      if (o < o_w1) {
        v = h0 + o < H ? th[c.b1 + h0 + o] : 0.f;
      } else if (o < o_w2) {
        const int f = (o - o_w1) / PR_WT, h = h0 + (o - o_w1) % PR_WT;
        v = h < H ? th[c.w1 + f * H + h] : 0.f;
      } else if (o < o_b2) {
        const int q = (o - o_w2) / CS, cc = (o - o_w2) - q * CS, h = h0 + q;
        v = (h < H && cc < C) ? th[c.w2 + h * C + cc] : 0.f;
      } else {
        const int cc = o - o_b2;
        v = cc < C ? th[c.b2 + cc] : 0.f;
      }
      ws[i] = v;
    }
    __syncthreads();
    for (int it = 0; it < cnt; ++it) {
      const long j = j0 + it;
      const int pk = (int)(j / nt), tile = (int)(j - (long)pk * nt);
      const float* wk = ws + it * iw;
      [[maybe_unused]] float wv = 0.f;
      if constexpr (WEIGHTED) {
        wv = pc_uniform(wl[pk - wb0]);
        if (!pred && wv == 0.f) continue;   // a particle of weight zero enters nothing (uniform over the workgroup)
      }
      if (tile == 0) {   // (uniform over the workgroup)
#pragma unroll
        for (int q = 0; q < CP / 4; ++q) {
          if (q < cq) {
            const float4 b = *reinterpret_cast<const float4*>(wk + o_b2 + 4 * q);
            z[4 * q + 0] = b.x; z[4 * q + 1] = b.y; z[4 * q + 2] = b.z; z[4 * q + 3] = b.w;
          }
        }
      }
      float4 a[PR_WT / 4];
#pragma unroll
      for (int q = 0; q < PR_WT / 4; ++q) a[q] = *reinterpret_cast<const float4*>(wk + 4 * q);
#pragma unroll 2
      for (int f = 0; f < F; ++f) {
        const float x = xr[f];
        const float4* w4 = reinterpret_cast<const float4*>(wk + o_w1 + f * PR_WT);
#pragma unroll
        for (int q = 0; q < PR_WT / 4; ++q) {
          const float4 w = w4[q];
          a[q].x = fmaf(x, w.x, a[q].x);
          a[q].y = fmaf(x, w.y, a[q].y);
          a[q].z = fmaf(x, w.z, a[q].z);
          a[q].w = fmaf(x, w.w, a[q].w);
        }
      }
#pragma unroll
      for (int q = 0; q < PR_WT; ++q) {
        const float4 aq4 = a[q / 4];
        const float aq = fmaxf((q & 3) == 0 ? aq4.x : (q & 3) == 1 ? aq4.y : (q & 3) == 2 ? aq4.z : aq4.w, 0.f);
        const float4* w4 = reinterpret_cast<const float4*>(wk + o_w2 + q * CS);
#pragma unroll
        for (int k = 0; k < CP / 4; ++k) {
          if (k < cq) {
            const float4 w = w4[k];
            z[4 * k + 0] = fmaf(aq, w.x, z[4 * k + 0]);
            z[4 * k + 1] = fmaf(aq, w.y, z[4 * k + 1]);
            z[4 * k + 2] = fmaf(aq, w.z, z[4 * k + 2]);
            z[4 * k + 3] = fmaf(aq, w.w, z[4 * k + 3]);
          }
        }
      }
      if (tile == nt - 1) {   // the particle's logits are whole: the softmax and the running sums, as k_predict_softmax
        float* out = (pred && live) ? pred + ((size_t)(p_begin + pk) * B + row) * C : nullptr;
        float m = z[0];
#pragma unroll
        for (int cc = 1; cc < CP; ++cc)
          if (cc < C) m = fmaxf(m, z[cc]);
        if (out && output == STEIN_PRED_LINK) {
#pragma unroll
          for (int cc = 0; cc < CP; ++cc)
            if (cc < C) out[cc] = z[cc];
        }
        float s = 0.f, e[CP];
#pragma unroll
        for (int cc = 0; cc < CP; ++cc) {
          z[cc] = cc < C ? z[cc] - m : 0.f;   // t_c <= 0
          e[cc] = cc < C ? expf(z[cc]) : 0.f;
          s += e[cc];
        }
        float pt = 0.f, py = (yb < 0 || yb >= C) ? __builtin_nanf("") : 0.f;
#pragma unroll
        for (int cc = 0; cc < CP; ++cc) {
          const float pc = e[cc] / s;
          if (out && output != STEIN_PRED_LINK && cc < C) out[cc] = pc;
          if constexpr (WEIGHTED) {
            if (wv != 0.f) acc[cc] = fmaf(wv, pc, acc[cc]);
          } else {
            acc[cc] += pc;
          }
          pt = fmaf(pc, z[cc], pt);
          py = (cc == yb && cc < C) ? pc : py;   // (a label in [C, CP) is no class: py stays NaN)
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
    float* po = part + (size_t)blockIdx.y * (C + 2) * B + row;
#pragma unroll
    for (int cc = 0; cc < CP; ++cc)
      if (cc < C) po[(size_t)cc * B] = acc[cc];
    po[(size_t)C * B] = acc_y;
    po[(size_t)(C + 1) * B] = acc_h;
  }
}

// The slices' sums merged in slice order, in fp64, as k_predict_softmax_finish does: PCF_ROWS rows per workgroup, the C + 2
// quantities of a row over eight threads; then one thread per row takes the argmax of the floats prob received.  WEIGHTED:
// the lane weights sum to 1, so nothing is divided; bad weights (the header's W is NaN) give NaN rows and the label -1.
constexpr int PCF_ROWS = 32;

template <bool WEIGHTED>
__global__ __launch_bounds__(256) void k_predict_bnn_class_finish(const float* __restrict__ part, int slices, int n, int B,
                                                                  int C, float* __restrict__ prob, float* __restrict__ lpd,
                                                                  float* __restrict__ ent, int* __restrict__ label,
                                                                  const double* __restrict__ head) {
  __shared__ float pr[PCF_ROWS][PC_C_MAX + 1];
  [[maybe_unused]] bool bad = false;
  if constexpr (WEIGHTED) bad = !(head[0] > 0.0);   // a negative or non-finite weight, W = 0 or an overflowing W
  const int r = threadIdx.x % PCF_ROWS, ql = threadIdx.x / PCF_ROWS;
  const int b = blockIdx.x * PCF_ROWS + r;
  if (b < B) {
    for (int q = ql; q < C + 2; q += 256 / PCF_ROWS) {
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
    for (int cc = 1; cc < C; ++cc)
      if (pr[r][cc] > top) {
        top = pr[r][cc];
        best = cc;
      }
    if constexpr (WEIGHTED) best = bad ? -1 : best;
    label[b] = best;
  }
}

// (C + 2) floats per state; the states' count is bounded as in stein_predict_softmax.hip: monotone in n and batch
static size_t predict_bnn_class_ws_bytes(int64_t n, int64_t batch, int64_t n_classes) {
  int64_t s = (n + PR_PASS - 1) / PR_PASS;
  if (s > PR_SLICE_CAP) s = PR_SLICE_CAP;
  int64_t states = s * batch;
  const int64_t by_target = (int64_t)PR_TARGET_WGS * PR_ROWS + batch;
  if (states > by_target) states = by_target;
  return (size_t)states * (size_t)(n_classes + 2) * sizeof(float);
}

static int predict_bnn_class_domain(int64_t n_in, int64_t n_hidden, int64_t n_classes) {
  if (n_in > PC_NIN_MAX) return stein_fail(STEIN_E_UNSUPPORTED, "more than %d input features", PC_NIN_MAX);
  if (n_classes < PC_C_MIN) return stein_fail(STEIN_E_UNSUPPORTED, "fewer than %d classes", PC_C_MIN);
  if (n_classes > PC_C_MAX) return stein_fail(STEIN_E_UNSUPPORTED, "more than %d classes", PC_C_MAX);
  if (n_hidden > PC_H_MAX) return stein_fail(STEIN_E_UNSUPPORTED, "more than %d hidden units", PC_H_MAX);
  if ((n_in + ((n_classes + 3) & ~(int64_t)3)) * n_hidden > PC_W_MAX)
    return stein_fail(STEIN_E_UNSUPPORTED, "more than %d weights ((n_in + CS) * n_hidden, CS = n_classes rounded up to 4)",
                      PC_W_MAX);
  return STEIN_OK;
}

// the kernels take up to 160 KB of dynamic LDS (the X tile alone is 129 KB at 128 inputs): raise each one's limit once per device
static int predict_bnn_class_attr(const void* fn, int slot) {
  static bool attr_set[8][64] = {{false}};
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64 || !attr_set[slot][dev]) {
    HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    if (dev >= 0 && dev < 64) attr_set[slot][dev] = true;
  }
  return STEIN_OK;
}

// the workspace of a weighted call: the weight pass's header of the slice bound ahead of the states; monotone too
static size_t predict_bnn_class_wws_bytes(int64_t n, int64_t batch, int64_t n_classes) {
  int64_t s = (n + PR_PASS - 1) / PR_PASS;
  if (s > PR_SLICE_CAP) s = PR_SLICE_CAP;
  return pw_doubles(s) * sizeof(double) + predict_bnn_class_ws_bytes(n, batch, n_classes);
}

static int predict_bnn_class_ws_check(int64_t n, int64_t batch, int64_t n_classes, size_t* out_bytes, bool weighted) {
  if (!out_bytes) return stein_fail(STEIN_E_BADARG, "NULL pointer");
  if (n < 1 || batch < 1 || n_classes < 1 || n > PR_COUNT_MAX || batch > PR_COUNT_MAX)
    return stein_fail(STEIN_E_SHAPE, "bad shape n=%lld batch=%lld C=%lld", (long long)n, (long long)batch, (long long)n_classes);
  if (int rc = predict_bnn_class_domain(1, 1, n_classes)) return rc;
  *out_bytes = weighted ? predict_bnn_class_wws_bytes(n, batch, n_classes) : predict_bnn_class_ws_bytes(n, batch, n_classes);
  return STEIN_OK;
}

extern "C" int stein_predict_bnn_class_workspace_bytes(int64_t n, int64_t batch, int64_t n_classes, size_t* out_bytes) {
  return predict_bnn_class_ws_check(n, batch, n_classes, out_bytes, false);
}

extern "C" int stein_predict_bnn_class_weighted_workspace_bytes(int64_t n, int64_t batch, int64_t n_classes, size_t* out_bytes) {
  return predict_bnn_class_ws_check(n, batch, n_classes, out_bytes, true);
}

// both entry points (pw.on = false: the unweighted call, for which every check and launch is what it was)
static int predict_bnn_class(const float* theta, int64_t n, int64_t d, int output, int64_t n_in, int64_t n_hidden,
                             int64_t n_classes, const int64_t* cols /*[5]: w1, b1, w2, b2; cols[4] is not read*/,
                             const float* X, const int32_t* labels, int64_t batch, float* pred, float* prob, float* lpd,
                             float* ent, int32_t* label, void* workspace, size_t ws_bytes, void* stream, const PredWeights& pw) {
  if (!theta || !cols || !X || (pw.on && !pw.w)) return stein_fail(STEIN_E_BADARG, "NULL pointer");
  if (!pred && !prob && !lpd && !ent && !label && !pw.ess)
    return stein_fail(STEIN_E_BADARG, pw.on ? "no output requested: pred, prob, lpd, ent, label and ess are all NULL"
                                            : "no output requested: pred, prob, lpd, ent and label are all NULL");
  if (lpd && !labels) return stein_fail(STEIN_E_BADARG, "lpd needs labels");
  if (output != STEIN_PRED_LINK && output != STEIN_PRED_MEAN) return stein_fail(STEIN_E_BADARG, "output %d", output);
  if (n < 1 || d < 1 || batch < 1 || n_in < 1 || n_hidden < 1 || n_classes < 1 || n > PR_COUNT_MAX || d > 0x7fffffffl ||
      batch > PR_COUNT_MAX)
    return stein_fail(STEIN_E_SHAPE, "bad shape n=%lld d=%lld batch=%lld n_in=%lld H=%lld C=%lld", (long long)n, (long long)d,
                      (long long)batch, (long long)n_in, (long long)n_hidden, (long long)n_classes);
  if (int rc = predict_bnn_class_domain(n_in, n_hidden, n_classes)) return rc;
  const int64_t len[4] = {n_in * n_hidden, n_hidden, n_hidden * n_classes, n_classes};
  for (int i = 0; i < 4; ++i) {
    if (cols[i] < 0 || cols[i] + len[i] > d) return stein_fail(STEIN_E_SHAPE, "block %d does not fit d=%lld", i, (long long)d);
    for (int j = 0; j < i; ++j)
      if (cols[i] < cols[j] + len[j] && cols[j] < cols[i] + len[i]) return stein_fail(STEIN_E_SHAPE, "blocks %d and %d overlap", j, i);
  }
  const bool summary = prob || lpd || ent || label;   // the rows the forward kernel reduces; ess comes from the weight pass alone
  if (summary || pw.ess) {
    if (!workspace)
      return stein_fail(STEIN_E_WORKSPACE,
                        pw.on ? "prob, lpd, ent, label and ess need a workspace (stein_predict_bnn_class_weighted_workspace_bytes)"
                              : "prob, lpd, ent and label need a workspace (stein_predict_bnn_class_workspace_bytes)");
    const size_t need = pw.on ? predict_bnn_class_wws_bytes(n, batch, n_classes) : predict_bnn_class_ws_bytes(n, batch, n_classes);
    if (ws_bytes < need) return stein_fail(STEIN_E_WORKSPACE, "workspace too small: %zu < %zu bytes", ws_bytes, need);
    if (pw.on && (uintptr_t)workspace % sizeof(double))
      return stein_fail(STEIN_E_WORKSPACE, "the workspace of a weighted call must be 8-byte aligned");
  }
  const PredPlan pl = predict_plan(n, batch);
  const int C = (int)n_classes, F = (int)n_in, H = (int)n_hidden, CS = (C + 3) & ~3;
  PredClassCols c = {(int)cols[0], (int)cols[1], (int)cols[2], (int)cols[3]};
  // the X tile and behind it the staging unit: as many (particle, tile) pairs as the LDS holds, PR_PASS at most
  const int ld = F | 1, xt = (PR_ROWS * ld + 3) & ~3, iw = pc_item_floats(F, CS);
  int ps = (PR_WIDE_LDS - xt) / iw;
  if (ps > PR_PASS) ps = PR_PASS;
  if (ps < 1) return stein_fail(STEIN_E_UNSUPPORTED, "launch plan: no staging unit fits");   // (no shape of the domain gets here)
  hipStream_t s = (hipStream_t)stream;
  if (pw.on && (summary || pw.ess))
    if (int rc = predict_weight_pass(pl, n, pw, workspace, s)) return rc;
  if (!pred && !summary) return STEIN_OK;   // ess alone
  // a weighted call that only asks for pred runs the unweighted kernel: pred does not depend on the weights
  const double* head = (pw.on && summary) ? (const double*)workspace : nullptr;
  float* part = !summary ? nullptr : head ? (float*)((double*)workspace + pw_doubles(pl.slices)) : (float*)workspace;
  // (the PC_WB lane weights go into the 128 floats PR_WIDE_LDS leaves free)
  const size_t lds_bytes = ((size_t)xt + (size_t)ps * iw + (head ? PC_WB : 0)) * sizeof(float);
#define PC_LAUNCH_AS(CP, WEIGHTED, SLOT)                                                                                 \
  do {                                                                                                                   \
    if (int rc = predict_bnn_class_attr(reinterpret_cast<const void*>(k_predict_bnn_class<CP, WEIGHTED>), SLOT)) return rc; \
    hipLaunchKernelGGL((k_predict_bnn_class<CP, WEIGHTED>), dim3((unsigned)pl.row_tiles, (unsigned)pl.slices), dim3(256), \
                       lds_bytes, s, theta, (int)n, (int)d, F, H, C, c, output, ld, ps, X, labels, (int)batch, pl.per,    \
                       pred, part, lpd ? 1 : 0, pw.w, head);                                                              \
  } while (0)
#define PC_LAUNCH(CP, SLOT)                                                                                              \
  do {                                                                                                                   \
    if (head) PC_LAUNCH_AS(CP, true, 4 + SLOT);                                                                          \
    else PC_LAUNCH_AS(CP, false, SLOT);                                                                                  \
  } while (0)
  if (C <= 4) PC_LAUNCH(4, 0);
  else if (C <= 8) PC_LAUNCH(8, 1);
  else if (C <= 16) PC_LAUNCH(16, 2);
  else PC_LAUNCH(32, 3);
#undef PC_LAUNCH
#undef PC_LAUNCH_AS
  LAUNCH_CHECK("k_predict_bnn_class");
  if (!summary) return STEIN_OK;
  const dim3 grid((unsigned)((batch + PCF_ROWS - 1) / PCF_ROWS));
  if (head) hipLaunchKernelGGL(k_predict_bnn_class_finish<true>, grid, dim3(256), 0, s, part, pl.slices, (int)n, (int)batch, C, prob, lpd, ent, label, head);
  else hipLaunchKernelGGL(k_predict_bnn_class_finish<false>, grid, dim3(256), 0, s, part, pl.slices, (int)n, (int)batch, C, prob, lpd, ent, label, head);
  LAUNCH_CHECK("k_predict_bnn_class_finish");
  return STEIN_OK;
}

extern "C" int stein_predict_bnn_class(const float* theta, int64_t n, int64_t d, int output, int64_t n_in, int64_t n_hidden,
                                       int64_t n_classes, const int64_t* cols, const float* X, const int32_t* labels,
                                       int64_t batch, float* pred, float* prob, float* lpd, float* ent, int32_t* label,
                                       void* workspace, size_t ws_bytes, void* stream) {
  return predict_bnn_class(theta, n, d, output, n_in, n_hidden, n_classes, cols, X, labels, batch, pred, prob, lpd, ent, label,
                           workspace, ws_bytes, stream, PredWeights{false, nullptr, nullptr});
}

extern "C" int stein_predict_bnn_class_weighted(const float* theta, int64_t n, int64_t d, int output, int64_t n_in,
                                                int64_t n_hidden, int64_t n_classes, const int64_t* cols, const float* X,
                                                const int32_t* labels, int64_t batch, const double* weights, float* pred,
                                                float* prob, float* lpd, float* ent, int32_t* label, double* ess,
                                                void* workspace, size_t ws_bytes, void* stream) {
  return predict_bnn_class(theta, n, d, output, n_in, n_hidden, n_classes, cols, X, labels, batch, pred, prob, lpd, ent, label,
                           workspace, ws_bytes, stream, PredWeights{true, weights, ess});
}
