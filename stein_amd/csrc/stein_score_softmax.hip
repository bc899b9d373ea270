// stein_score_softmax.hip -- the score of multi-class (softmax) regression for every particle in one launch:
// stein_score_softmax.  theta packs W [F][C] row-major at w_col (W_fc at column w_col + f C + c) and, for the hierarchical
// prior, log alpha at alpha_col; labels are int32 class indices on the device.
//   z_bc  = sum_f x_bf W_fc
//   log p = scale * sum_b [z_{b,y_b} - logsumexp_c z_bc] + sum_fc log N(W_fc; 0, 1/alpha) + log Gamma(alpha; 1, rate)
//           (density at alpha, no Jacobian, as the logistic model of stein_score.hip)
//   d/dW_fc    = scale * sum_b x_bf (1[y_b = c] - p_bc) - alpha W_fc,   p_b. = softmax(z_b.) with the row maximum subtracted
//   d/dlog alpha = F C / 2 - alpha (1/2 sum_fc W_fc^2 + rate)           (alpha_col < 0: alpha = prior_precision, no entry)
// A label outside [0, C) makes its row's residuals NaN, and with them every weight entry of every particle.
//
// Mapping: a workgroup keeps W and its gradient of PPW = 1, 2 or 4 particles in LDS ([F][CS] each, CS = C rounded up to 4, the
// padding zero), LPP = 256 / PPW lanes per particle.  The batch is staged in LDS chunks of crows rows ([crows][ld], ld odd)
// shared by the workgroup's particles, once when it fits whole.  Per chunk two phases and one barrier between them:
//   forward   G lanes per row (G a power of two, 1 when the chunk has a row for every lane): lane j of a row sums the features
//             f = j, j + G, ... ascending into CP logit accumulators in registers (W read 16 bytes at a time, at one address by
//             the lanes of equal j: broadcast), the G lanes are summed by shuffles, and lane 0 evaluates the softmax in
//             registers and writes the residuals r_bc = 1[y_b = c] - p_bc to LDS
//   backward  lanes over the (f, four classes) tiles of the gradient: a tile is read from LDS, takes x_bf r_bc of the chunk's
//             rows in ascending order, and is written back
// All of a particle's batch is reduced where the particle lives: one launch, no workspace, no atomics.  PPW, G and crows follow
// from (F, C, batch) alone, so a particle's row depends on nothing but the particle.  Instantiated over the padded class count
// CP = 4, 8, 16, 32 (the registers of the forward phase); loops over classes stop at CS.  DESIGN.md 6e.
#include "stein_common.h"

constexpr int SM_LDS = 40448;           // floats of dynamic LDS at most (158 KB)
constexpr int SM_WLDS = 24576;          // floats of W and its gradient of a workgroup's particles at most when PPW > 1 (96 KB)
constexpr int SM_ROWS_MAX = 1024;       // rows per LDS chunk at most
constexpr int SM_MAX_WGS = 1024;        // the grid's cap: the particle loop is grid-strided
constexpr int SM_C_MIN = 2, SM_C_MAX = 32, SM_F_MAX = 1024, SM_FC_MAX = 16384;

template <int CP>
__global__ __launch_bounds__(256) void k_score_softmax(const float* __restrict__ theta, int n, int d, int w_col, int F, int C,
                                                       int alpha_col, const float* __restrict__ X,
                                                       const int* __restrict__ labels, int B, int ppw, int G, int crows,
                                                       float scale, float prior_precision, float gamma_rate,
                                                       float* __restrict__ score) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int CS = (C + 3) & ~3, cq = CS / 4, FCS = F * CS, ld = F | 1;
  const int lpp = 256 / ppw;
  float* Ws = lds;                                   // [ppw][F][CS]
  float* Gs = Ws + ppw * FCS;                        // the same
  float* rs = Gs + ppw * FCS;                        // [ppw][crows][CS]
  float* xs = rs + (size_t)ppw * crows * CS;         // [crows][ld]
  int* ys = reinterpret_cast<int*>(xs + (size_t)crows * ld);   // [crows]
  float* red = reinterpret_cast<float*>(ys + crows); // [4 waves]
  const int t = threadIdx.x, sub = t / lpp, l = t - sub * lpp, wave = t >> 6;
  const int j = l % G, rr = l / G, RB = lpp / G;
  const int nchunks = (B + crows - 1) / crows;
  auto stage = [&](int c0) {
    const int rows = min(crows, B - c0);
    for (int i = t; i < rows * F; i += 256) {
      const int r = i / F, f = i - r * F;
      xs[r * ld + f] = X[(size_t)(c0 + r) * F + f];
    }
    for (int i = t; i < rows; i += 256) ys[i] = labels[c0 + i];
  };
  if (nchunks == 1) stage(0);          // the first barrier of the particle loop follows
  float* Wp = Ws + sub * FCS;
  float* Gp = Gs + sub * FCS;
  float* rp = rs + (size_t)sub * crows * CS;
  for (long p0 = (long)blockIdx.x * ppw; p0 < n; p0 += (long)gridDim.x * ppw) {
    const long p = p0 + sub;
    const bool live = p < n;
    const float* th = theta + (size_t)(live ? p : 0) * d;
    __syncthreads();                   // every lane is past the last particle's W and gradient
    for (int i = l; i < FCS; i += lpp) {
      const int f = i / CS, c = i - f * CS;
      Wp[i] = c < C ? th[w_col + f * C + c] : 0.f;
      Gp[i] = 0.f;
    }
    for (int ch = 0; ch < nchunks; ++ch) {
      __syncthreads();                 // W is staged; every lane is past the last chunk's rows and residuals
      if (nchunks > 1) {
        stage(ch * crows);
        __syncthreads();
      }
      const int rows = min(crows, B - ch * crows);
      // forward: the logits of RB rows at a time, their softmax, the residuals
      for (int rb = 0; rb < rows; rb += RB) {
        const int row = rb + rr;
        const float* xr = xs + min(row, rows - 1) * ld;
        float z[CP];
#pragma unroll
        for (int c = 0; c < CP; ++c) z[c] = 0.f;
        for (int f = j; f < F; f += G) {
          const float x = xr[f];
          const float4* w4 = reinterpret_cast<const float4*>(Wp + f * CS);
#pragma unroll
          for (int q = 0; q < CP / 4; ++q) {
            if (q < cq) {
              const float4 w = w4[q];
              z[4 * q + 0] = fmaf(x, w.x, z[4 * q + 0]);
              z[4 * q + 1] = fmaf(x, w.y, z[4 * q + 1]);
              z[4 * q + 2] = fmaf(x, w.z, z[4 * q + 2]);
              z[4 * q + 3] = fmaf(x, w.w, z[4 * q + 3]);
            }
          }
        }
        for (int o = G >> 1; o > 0; o >>= 1) {
#pragma unroll
          for (int c = 0; c < CP; ++c) z[c] += __shfl_xor(z[c], o);
        }
        if (j == 0 && row < rows) {
          const int yb = ys[row];
          float m = z[0];
#pragma unroll
          for (int c = 1; c < CP; ++c)
            if (c < C) m = fmaxf(m, z[c]);
          float s = 0.f;
#pragma unroll
          for (int c = 0; c < CP; ++c) {
            z[c] = c < C ? expf(z[c] - m) : 0.f;
            s += z[c];
          }
          const float bad = (yb < 0 || yb >= C) ? __builtin_nanf("") : 0.f;
          float* ro = rp + row * CS;
#pragma unroll
          for (int c = 0; c < CP; ++c)
            if (c < CS) ro[c] = ((c == yb ? 1.f : 0.f) - z[c] / s) + bad;
        }
      }
      __syncthreads();
      // backward: every tile of the gradient takes the chunk's rows in order
      for (int tile = l; tile < F * cq; tile += lpp) {
        const int f = tile / cq, q = tile - f * cq;
        float4* gp = reinterpret_cast<float4*>(Gp + f * CS + 4 * q);
        float4 g = *gp;
        const float* xc = xs + f;
        const float* rc = rp + 4 * q;
#pragma unroll 4
        for (int r = 0; r < rows; ++r) {
          const float x = xc[r * ld];
          const float4 e = *reinterpret_cast<const float4*>(rc + r * CS);
          g.x = fmaf(x, e.x, g.x);
          g.y = fmaf(x, e.y, g.y);
          g.z = fmaf(x, e.z, g.z);
          g.w = fmaf(x, e.w, g.w);
        }
        *gp = g;
      }
    }
    __syncthreads();                   // the gradient is whole
    float prec = prior_precision, sw2 = 0.f;
    if (alpha_col >= 0) {              // (uniform over the workgroup)
      prec = expf(th[alpha_col]);
      for (int i = l; i < FCS; i += lpp) sw2 = fmaf(Wp[i], Wp[i], sw2);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) sw2 += __shfl_xor(sw2, o);
      if ((t & 63) == 0) red[wave] = sw2;
      __syncthreads();
      const int nw = lpp / 64;         // the particle's waves, in wave order
      sw2 = red[sub * nw];
      for (int w = 1; w < nw; ++w) sw2 += red[sub * nw + w];
    }
    if (live) {
      float* out = score + (size_t)p * d;
      for (int c = l; c < d; c += lpp)   // columns that are neither weights nor log alpha carry no gradient
        if ((c < w_col || c >= w_col + F * C) && c != alpha_col) out[c] = 0.f;
      for (int i = l; i < F * C; i += lpp) {
        const int f = i / C, c = i - f * C;
        out[w_col + i] = scale * Gp[f * CS + c] - prec * Wp[f * CS + c];
      }
      if (alpha_col >= 0 && l == 0) out[alpha_col] = 0.5f * (float)(F * C) - prec * (0.5f * sw2 + gamma_rate);
    }
  }
}

// the kernels take up to 158 KB of dynamic LDS: raise each one's limit once per device
static int score_softmax_attr(const void* fn, int slot) {
  static bool attr_set[4][64] = {{false}};
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64 || !attr_set[slot][dev]) {
    HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    if (dev >= 0 && dev < 64) attr_set[slot][dev] = true;
  }
  return STEIN_OK;
}

static thread_local int g_softmax_lanes = 0;   // stein_debug_score_softmax_lanes: 0 = the rule below

extern "C" int stein_debug_score_softmax_lanes(int lanes) {
  if (lanes < 0 || lanes > 64 || (lanes & (lanes - 1))) return stein_fail(STEIN_E_BADARG, "lanes %d", lanes);
  g_softmax_lanes = lanes;
  return STEIN_OK;
}

extern "C" int stein_score_softmax(const float* theta, int64_t n, int64_t d, int64_t w_col, int64_t n_feats, int64_t n_classes,
                                   int64_t alpha_col, const float* X, const int32_t* labels, int64_t batch, double scale,
                                   double prior_precision, double gamma_rate, float* score, void* stream) {
  if (!theta || !X || !labels || !score) return stein_fail(STEIN_E_BADARG, "NULL pointer");
  if (n < 1 || d < 1 || batch < 1 || n_feats < 1 || n_classes < 1 || n > 0x7fffffffl || d > 0x7fffffffl || batch > 0x7fffffffl)
    return stein_fail(STEIN_E_SHAPE, "bad shape n=%lld d=%lld batch=%lld F=%lld C=%lld", (long long)n, (long long)d,
                      (long long)batch, (long long)n_feats, (long long)n_classes);
  if (n_classes < SM_C_MIN) return stein_fail(STEIN_E_UNSUPPORTED, "fewer than %d classes", SM_C_MIN);
  if (n_classes > SM_C_MAX) return stein_fail(STEIN_E_UNSUPPORTED, "more than %d classes", SM_C_MAX);
  if (n_feats > SM_F_MAX) return stein_fail(STEIN_E_UNSUPPORTED, "more than %d features", SM_F_MAX);
  if (n_feats * n_classes > SM_FC_MAX)
    return stein_fail(STEIN_E_UNSUPPORTED, "more than %d weights (n_feats * n_classes)", SM_FC_MAX);
  const int64_t fc = n_feats * n_classes;
  if (w_col < 0 || w_col + fc > d || alpha_col >= d || (alpha_col >= w_col && alpha_col < w_col + fc))
    return stein_fail(STEIN_E_SHAPE, "weights [%lld, %lld) / log-alpha column %lld do not fit d=%lld", (long long)w_col,
                      (long long)(w_col + fc), (long long)alpha_col, (long long)d);
  const int C = (int)n_classes, F = (int)n_feats, CS = (C + 3) & ~3, fcs = F * CS, ld = F | 1;
  // particles per workgroup: as many as SM_WLDS holds; rows per chunk: what the rest of the LDS holds beside them (a row of
  // X, its label and the particles' residuals), no more than the batch; lanes per row: doubled while the chunk has fewer
  // rows than a particle has lanes (and the features give the lanes something to sum)
  const int ppw = 8 * fcs <= SM_WLDS ? 4 : 4 * fcs <= SM_WLDS ? 2 : 1;
  int64_t crows = (SM_LDS - 2 * ppw * fcs - 8) / (ld + 1 + ppw * CS);
  if (crows > SM_ROWS_MAX) crows = SM_ROWS_MAX;
  if (crows > batch) crows = batch;
  const int lpp = 256 / ppw;
  int g = 1;
  while (g < 64 && lpp / g > crows && g < F) g *= 2;
  if (g_softmax_lanes) g = g_softmax_lanes;   // (the A/B of profiles/softmax_ab.txt: any power of two up to 64 is a valid mapping)
  const size_t lds_bytes = ((size_t)2 * ppw * fcs + (size_t)crows * (ld + 1 + ppw * CS) + 4) * sizeof(float);
  long blocks = (long)((n + ppw - 1) / ppw);
  if (blocks > SM_MAX_WGS) blocks = SM_MAX_WGS;
  hipStream_t s = (hipStream_t)stream;
#define SM_LAUNCH(CP, SLOT)                                                                                              \
  do {                                                                                                                   \
    if (int rc = score_softmax_attr(reinterpret_cast<const void*>(k_score_softmax<CP>), SLOT)) return rc;                \
    hipLaunchKernelGGL((k_score_softmax<CP>), dim3((unsigned)blocks), dim3(256), lds_bytes, s, theta, (int)n, (int)d,     \
                       (int)w_col, F, C, (int)alpha_col, X, labels, (int)batch, ppw, g, (int)crows, (float)scale,        \
                       (float)prior_precision, (float)gamma_rate, score);                                                \
  } while (0)
  if (C <= 4) SM_LAUNCH(4, 0);
  else if (C <= 8) SM_LAUNCH(8, 1);
  else if (C <= 16) SM_LAUNCH(16, 2);
  else SM_LAUNCH(32, 3);
#undef SM_LAUNCH
  LAUNCH_CHECK("k_score_softmax");
  return STEIN_OK;
}
