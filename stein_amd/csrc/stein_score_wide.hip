// stein_score_wide.hip -- the score of the one-hidden-layer network of stein_score.hip (the model, the formulas and the output
// conventions are written at its head) for 5 .. 128 input features: stein_score_bnn_wide.  k_score_bnn keeps w1 and its
// gradient in registers, n_in * KH words each per lane, which stops at four features; here both live in LDS.
//
// Mapping: LH lanes per particle over the hidden units (KH per lane), 256 / LH particles per workgroup.  A particle's w1 and
// gw1 are [n_in][H] in LDS; a lane only ever touches the columns of its own hidden units, so neither needs a barrier.  The
// batch is staged in chunks, transposed in blocks of SW_R rows ([block][f][SW_R]): per feature a lane reads its w1 word once
// and the block's SW_R inputs as two 16-byte broadcasts, for SW_R FMAs.  Per block:
//   forward   z[k][r] = b1 + sum_f x_rf w1_fh (f ascending), the lane's share of pred_r, summed over the particle's lanes by
//             shuffles and -- LH > 64 -- one barrier through LDS, in a fixed order: every lane of the particle holds e_r
//   backward  gw2, gb1 in registers; gw1_fh += sum_r t_r x_rf as one LDS read-modify-write per SW_R FMAs
// All of a particle's batch is reduced where the particle lives: no atomics, no workspace, and a particle's row depends on
// nothing but the particle (its place in the workgroup and the grid change no operation).  DESIGN.md 6e.
#include "stein_common.h"

constexpr int SW_R = 8;                 // batch rows per register block
constexpr int SW_XLDS = 3584;           // floats of X and y per LDS chunk (14 KB): (SW_XLDS / (n_in + 1)) & ~7 rows
constexpr int SW_WLDS = 36 * 1024;      // floats of w1 and gw1 of a workgroup's particles (144 KB): two particles of
                                        // n_in * H <= 9216, which takes in 90 x 100, or four of <= 4608
constexpr int SW_MAX_WGS = 1024;        // the grid's cap: the particle loop is grid-strided
constexpr int SW_NIN_MAX = 128, SW_H_MAX = 1024, SW_W1_MAX = 16384;

struct BnnWideCols { int w1, b1, w2, b2, loglam, loggam; };

template <int LH, int KH>
__global__ __launch_bounds__(256) void k_score_bnn_wide(const float* __restrict__ theta, int n, int d, int F, int H,
                                                        BnnWideCols c, const float* __restrict__ X,
                                                        const float* __restrict__ y, int B, int crows, int wfl, float n_train,
                                                        float ga, float gb, float* __restrict__ score) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int NW = LH / 64;          // waves per particle
  // feature iterations in flight (their LDS reads are issued together).  Measured, 1 | 2 | 4 (profiles/bnn_wide_ab.txt): 13 x 50,
  // four particles per workgroup, n = 16384: 0.289 | 0.279 | 0.356 ms; 90 x 100, two per workgroup: 3.48 | 3.02 | 2.79 ms
  constexpr int FU = KH >= 4 ? 1 : (KH == 2 || LH == 64) ? 2 : 4;
  const int FH = F * H;
  float* w1s = lds;                    // [256 / LH][F][H], wfl floats
  float* g1s = lds + wfl;              // the same
  float* xs = g1s + wfl;               // [crows / SW_R][F][SW_R]
  float* ys = xs + (size_t)crows * F;  // [crows]
  float* red = ys + crows;             // [2][4 waves][SW_R]: the waves' shares of pred_r, double-buffered
  float* red2 = red + 2 * 4 * SW_R;    // [4 waves]: the waves' shares of sum w^2
  const int t = threadIdx.x, lane = t % LH, sub = t / LH, wave = t >> 6;
  const int nchunks = (B + crows - 1) / crows;
  auto stage = [&](int c0) {           // rows past the batch are staged as zeros (their e is forced to 0 below)
    const int rows = min(crows, B - c0), rows8 = (rows + SW_R - 1) & ~(SW_R - 1);
    for (int i = t; i < rows8 * F; i += 256) {
      const int r = i / F, f = i - r * F;
      xs[((r / SW_R) * F + f) * SW_R + (r % SW_R)] = r < rows ? X[(size_t)(c0 + r) * F + f] : 0.f;
    }
    for (int i = t; i < rows8; i += 256) ys[i] = i < rows ? y[c0 + i] : 0.f;
  };
  if (nchunks == 1) {
    stage(0);
    __syncthreads();
  }
  float* w1p = w1s + sub * FH;
  float* g1p = g1s + sub * FH;
  int buf = 0;
  for (long p0 = (long)blockIdx.x * (256 / LH); p0 < n; p0 += (long)gridDim.x * (256 / LH)) {
    const long p = p0 + sub;
    const bool live = p < n;
    const float* th = theta + (size_t)(live ? p : 0) * d;
    float b1[KH], w2[KH], gb1[KH], gw2[KH];
    bool ok[KH];
#pragma unroll
    for (int k = 0; k < KH; ++k) {
      const int h = lane + LH * k;
      ok[k] = h < H;
      b1[k] = ok[k] ? th[c.b1 + h] : 0.f;
      w2[k] = ok[k] ? th[c.w2 + h] : 0.f;
      gb1[k] = 0.f; gw2[k] = 0.f;
      if (ok[k])
        for (int f = 0; f < F; ++f) {
          w1p[f * H + h] = th[c.w1 + f * H + h];
          g1p[f * H + h] = 0.f;
        }
    }
    const float b2 = th[c.b2];
    float se = 0.f, se2 = 0.f;
    for (int ch = 0; ch < nchunks; ++ch) {
      if (nchunks > 1) {
        __syncthreads();
        stage(ch * crows);
        __syncthreads();
      }
      const int rows = min(crows, B - ch * crows);
      for (int r0 = 0; r0 < rows; r0 += SW_R) {
        const float* xb = xs + (size_t)(r0 / SW_R) * F * SW_R;
        float z[KH][SW_R];
#pragma unroll
        for (int k = 0; k < KH; ++k)
#pragma unroll
          for (int r = 0; r < SW_R; ++r) z[k][r] = b1[k];
#pragma unroll FU
        for (int f = 0; f < F; ++f) {
          const float4 xa = *reinterpret_cast<const float4*>(xb + f * SW_R);
          const float4 xc = *reinterpret_cast<const float4*>(xb + f * SW_R + 4);
          const float x[SW_R] = {xa.x, xa.y, xa.z, xa.w, xc.x, xc.y, xc.z, xc.w};
#pragma unroll
          for (int k = 0; k < KH; ++k) {
            const float w = ok[k] ? w1p[f * H + lane + LH * k] : 0.f;
#pragma unroll
            for (int r = 0; r < SW_R; ++r) z[k][r] = fmaf(x[r], w, z[k][r]);
          }
        }
        float e[SW_R];
#pragma unroll
        for (int r = 0; r < SW_R; ++r) {
          float part = 0.f;
#pragma unroll
          for (int k = 0; k < KH; ++k) part = fmaf(fmaxf(z[k][r], 0.f), w2[k], part);
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
          e[r] = part;
        }
        if constexpr (NW > 1) {          // the particle's waves, in wave order
          if ((t & 63) == 0) {
#pragma unroll
            for (int r = 0; r < SW_R; ++r) red[(buf * 4 + wave) * SW_R + r] = e[r];
          }
          __syncthreads();
#pragma unroll
          for (int r = 0; r < SW_R; ++r) {
            float s = red[(buf * 4 + sub * NW) * SW_R + r];
#pragma unroll
            for (int w = 1; w < NW; ++w) s += red[(buf * 4 + sub * NW + w) * SW_R + r];
            e[r] = s;
          }
          buf ^= 1;
        }
#pragma unroll
        for (int r = 0; r < SW_R; ++r) {
          e[r] = r0 + r < rows ? ys[r0 + r] - (e[r] + b2) : 0.f;
          se += e[r];
          se2 = fmaf(e[r], e[r], se2);
        }
#pragma unroll
        for (int k = 0; k < KH; ++k)
#pragma unroll
          for (int r = 0; r < SW_R; ++r) {
            gw2[k] = fmaf(e[r], fmaxf(z[k][r], 0.f), gw2[k]);
            const float tk = z[k][r] > 0.f ? e[r] * w2[k] : 0.f;
            gb1[k] += tk;
            z[k][r] = tk;
          }
#pragma unroll FU
        for (int f = 0; f < F; ++f) {
          const float4 xa = *reinterpret_cast<const float4*>(xb + f * SW_R);
          const float4 xc = *reinterpret_cast<const float4*>(xb + f * SW_R + 4);
          const float x[SW_R] = {xa.x, xa.y, xa.z, xa.w, xc.x, xc.y, xc.z, xc.w};
#pragma unroll
          for (int k = 0; k < KH; ++k) {
            if (ok[k]) {
              float g = g1p[f * H + lane + LH * k];
#pragma unroll
              for (int r = 0; r < SW_R; ++r) g = fmaf(z[k][r], x[r], g);
              g1p[f * H + lane + LH * k] = g;
            }
          }
        }
      }
    }
    float sw2 = 0.f;   // sum of squares of every weight under the N(0, 1/lambda) prior
#pragma unroll
    for (int k = 0; k < KH; ++k) {
      sw2 = fmaf(b1[k], b1[k], fmaf(w2[k], w2[k], sw2));
      if (ok[k])
        for (int f = 0; f < F; ++f) {
          const float w = w1p[f * H + lane + LH * k];
          sw2 = fmaf(w, w, sw2);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sw2 += __shfl_xor(sw2, o);
    if constexpr (NW > 1) {   // (a barrier of the row loop lies between two uses of red2: B >= 1)
      if ((t & 63) == 0) red2[wave] = sw2;
      __syncthreads();
      sw2 = red2[sub * NW];
#pragma unroll
      for (int w = 1; w < NW; ++w) sw2 += red2[sub * NW + w];
    }
    sw2 += b2 * b2;
    if (live) {
      const float lam = expf(th[c.loglam]), gam = expf(th[c.loggam]);
      const float s = n_train / (float)B, cg = s * gam, inv = 1.f / n_train;
      float* out = score + (size_t)p * d;
      for (int j = lane; j < d; j += LH) {   // columns outside the model carry no gradient
        const bool in_model = (j >= c.w1 && j < c.w1 + FH) || (j >= c.b1 && j < c.b1 + H) || (j >= c.w2 && j < c.w2 + H) ||
                              j == c.b2 || j == c.loglam || j == c.loggam;
        if (!in_model) out[j] = 0.f;
      }
#pragma unroll
      for (int k = 0; k < KH; ++k) {
        const int h = lane + LH * k;
        if (ok[k]) {
          out[c.b1 + h] = (cg * gb1[k] - lam * b1[k]) * inv;
          out[c.w2 + h] = (cg * gw2[k] - lam * w2[k]) * inv;
          for (int f = 0; f < F; ++f) out[c.w1 + f * H + h] = (cg * g1p[f * H + h] - lam * w1p[f * H + h]) * inv;
        }
      }
      if (lane == 0) {
        const float P = (float)(FH + 2 * H + 1);
        out[c.b2] = (cg * se - lam * b2) * inv;
        out[c.loggam] = (s * (0.5f * (float)B - 0.5f * gam * se2) + (ga - 1.f) - gb * gam) * inv;
        out[c.loglam] = (0.5f * P - 0.5f * lam * sw2 + (ga - 1.f) - gb * lam) * inv;
      }
    }
  }
}

// the kernels take up to 158 KB of dynamic LDS: raise each one's limit once per device
static int score_wide_attr(const void* fn, int slot) {
  static bool attr_set[5][64] = {{false}};
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64 || !attr_set[slot][dev]) {
    HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    if (dev >= 0 && dev < 64) attr_set[slot][dev] = true;
  }
  return STEIN_OK;
}

extern "C" int stein_score_bnn_wide(const float* theta, int64_t n, int64_t d, int64_t n_in, int64_t n_hidden,
                                    const int64_t* cols /*[6]: w1, b1, w2, b2, log_lambda, log_gamma*/, const float* X,
                                    const float* y, int64_t batch, double n_train, double gamma_a, double gamma_b,
                                    float* score, void* stream) {
  // up to four features: the narrow entry point's own code (and its checks)
  if (n_in >= 1 && n_in <= 4) return stein_score_bnn(theta, n, d, n_in, n_hidden, cols, X, y, batch, n_train, gamma_a, gamma_b, score, stream);
  if (!theta || !cols || !X || !y || !score) return stein_fail(STEIN_E_BADARG, "NULL pointer");
  if (n < 1 || d < 1 || batch < 1 || n_in < 1 || n_hidden < 1 || n > 0x7fffffffl || d > 0x7fffffffl || batch > 0x7fffffffl)
    return stein_fail(STEIN_E_SHAPE, "bad shape");
  if (n_in > SW_NIN_MAX) return stein_fail(STEIN_E_UNSUPPORTED, "more than %d input features", SW_NIN_MAX);
  if (n_hidden > SW_H_MAX) return stein_fail(STEIN_E_UNSUPPORTED, "more than %d hidden units", SW_H_MAX);
  if (n_in * n_hidden > SW_W1_MAX)
    return stein_fail(STEIN_E_UNSUPPORTED, "more than %d first-layer weights (n_in * n_hidden)", SW_W1_MAX);
  const int64_t len[6] = {n_in * n_hidden, n_hidden, n_hidden, 1, 1, 1};
  for (int i = 0; i < 6; ++i) {
    if (cols[i] < 0 || cols[i] + len[i] > d) return stein_fail(STEIN_E_SHAPE, "block %d does not fit d=%lld", i, (long long)d);
    for (int j = 0; j < i; ++j)
      if (cols[i] < cols[j] + len[j] && cols[j] < cols[i] + len[i]) return stein_fail(STEIN_E_SHAPE, "blocks %d and %d overlap", j, i);
  }
  if (!(n_train > 0.0)) return stein_fail(STEIN_E_BADARG, "n_train must be positive");
  BnnWideCols c = {(int)cols[0], (int)cols[1], (int)cols[2], (int)cols[3], (int)cols[4], (int)cols[5]};
  const int fh = (int)(n_in * n_hidden);
  // lanes per particle: the hidden units rounded up to whole waves, and no more particles per workgroup than SW_WLDS holds
  int lh = n_hidden <= 64 ? 64 : n_hidden <= 128 ? 128 : 256;
  while (lh < 256 && (256 / lh) * fh * 2 > SW_WLDS) lh *= 2;
  const int ppw = 256 / lh;
  const int kh = lh < 256 ? 1 : (int)((n_hidden + 255) / 256);
  const int wfl = (ppw * fh + 3) & ~3;
  int64_t crows = (SW_XLDS / (n_in + 1)) & ~(int64_t)(SW_R - 1);
  const int64_t b8 = (batch + SW_R - 1) & ~(int64_t)(SW_R - 1);
  if (crows > b8) crows = b8;
  const size_t lds_bytes = ((size_t)2 * wfl + (size_t)crows * (n_in + 1) + 2 * 4 * SW_R + 4) * sizeof(float);
  long blocks = (long)((n + ppw - 1) / ppw);
  if (blocks > SW_MAX_WGS) blocks = SW_MAX_WGS;
  hipStream_t s = (hipStream_t)stream;
#define SW_LAUNCH(LH, KH, SLOT)                                                                                          \
  do {                                                                                                                   \
    if (int rc = score_wide_attr(reinterpret_cast<const void*>(k_score_bnn_wide<LH, KH>), SLOT)) return rc;              \
    hipLaunchKernelGGL((k_score_bnn_wide<LH, KH>), dim3((unsigned)blocks), dim3(256), lds_bytes, s, theta, (int)n,        \
                       (int)d, (int)n_in, (int)n_hidden, c, X, y, (int)batch, (int)crows, wfl, (float)n_train,            \
                       (float)gamma_a, (float)gamma_b, score);                                                            \
  } while (0)
  if (lh == 64) SW_LAUNCH(64, 1, 0);
  else if (lh == 128) SW_LAUNCH(128, 1, 1);
  else if (kh <= 1) SW_LAUNCH(256, 1, 2);
  else if (kh <= 2) SW_LAUNCH(256, 2, 3);
  else SW_LAUNCH(256, 4, 4);
#undef SW_LAUNCH
  LAUNCH_CHECK("k_score_bnn_wide");
  return STEIN_OK;
}
