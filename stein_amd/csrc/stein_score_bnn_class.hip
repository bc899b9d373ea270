// stein_score_bnn_class.hip -- the score of the network classifier, one hidden ReLU layer with a softmax head, for every
// particle in one launch: stein_score_bnn_class.  theta packs w1 [n_in][H] (row-major, as stein_score_bnn), b1 [H], w2 [H][C]
// (row-major: how an [H, C] variable flattens), b2 [C] and, for the hierarchical prior, log lambda; cols[5] gives the first
// column of each (cols[4] < 0: the fixed prior_precision, no entry).  labels are int32 class indices on the device.
//   pre_bh = b1_h + sum_f x_bf w1_fh (f ascending),  a_bh = relu(pre_bh)
//   z_bc   = b2_c + sum_h a_bh w2_hc (h ascending),   p_b. = softmax(z_b.) with the row maximum subtracted
//   log p  = scale * sum_b [z_{b,y_b} - logsumexp_c z_bc] + sum over the P = n_in H + H + H C + C entries of the four blocks of
//            log N(. ; 0, 1/lambda) + log Gamma(lambda; 1, gamma_rate)   (density at lambda, no Jacobian)
//   r_bc = 1[y_b = c] - p_bc,  m_bh = [pre_bh > 0],  delta_bh = m_bh sum_c r_bc w2_hc (c ascending)
//   d/db2_c = scale sum_b r_bc - lambda b2_c            d/dw2_hc = scale sum_b a_bh r_bc - lambda w2_hc
//   d/db1_h = scale sum_b delta_bh - lambda b1_h        d/dw1_fh = scale sum_b x_bf delta_bh - lambda w1_fh
//   d/dlog lambda = P / 2 - lambda (1/2 sum of squares of the P entries + gamma_rate)
// The prior and the scaling are stein_score_softmax's over all four blocks; stein_score_bnn's division of everything by n_train
// is not taken over.  A label outside [0, C) makes every entry of the four blocks of every particle NaN.
//
// Mapping: LH lanes per particle (64, 128 or 256: the hidden units rounded up to whole waves, KH = 1 or 2 units per lane),
// 256 / LH particles per workgroup.  A particle keeps w1, w2 ([H][CS], CS = C rounded up to 4, the padding zero) and both
// gradients in LDS.  The batch is staged in chunks shared by the workgroup's particles, transposed in blocks of BC_R rows as
// in stein_score_wide.hip.  Per block of BC_R rows four phases with a barrier between them:
//   A  lanes over the hidden units: pre[k][r] in registers (f ascending), a_bh written to LDS as [h][BC_R]
//   B  lanes over the (row, class) pairs, BC_R * CS <= 256: z = b2_c + sum_h a_bh w2_hc, h ascending, written to LDS
//   S  the same lanes: each reads its row's C logits and takes the maximum and the sum of the exponentials in class order
//      (every lane of a row computes the same bits), then writes r_bc to LDS; padded classes and rows past the batch get 0
//   C  lanes over the hidden units again: delta_bh from 16-byte broadcast reads of r_b. and the lane's own w2 row, gw2 as one
//      LDS read-modify-write per 32 FMAs, gb1 in registers, gw1 as the wide kernel's backward; lanes 0 .. C-1 sum gb2
// All of a particle's batch is reduced where the particle lives: one launch, no workspace, no atomics.  LH, KH and the chunk
// rows follow from (n_in, H, C, batch) alone and every sum has a fixed order, so a particle's row depends on nothing but the
// particle.  DESIGN.md 6e.
#include "stein_common.h"

constexpr int BC_R = 8;                 // batch rows per register block
constexpr int BC_LDS = 40448;           // floats of dynamic LDS at most (158 KB)
constexpr int BC_PLDS = 36864;          // floats of a workgroup's particles at most when it holds more than one (144 KB)
constexpr int BC_ROWS_MAX = 1024;       // rows per LDS chunk at most
constexpr int BC_MAX_WGS = 1024;        // the grid's cap: the particle loop is grid-strided
constexpr int BC_NIN_MAX = 128, BC_C_MIN = 2, BC_C_MAX = 32, BC_H_MAX = 512, BC_W_MAX = 16384;

struct BnnClassCols { int w1, b1, w2, b2, loglam; };

// floats of one particle in LDS: w1 and gw1 [n_in H, rounded up to 4], w2 and gw2 [H][CS], a [H][BC_R], z and r [BC_R][CS],
// b2 and gb2 [CS]
static __host__ __device__ inline int bc_particle_floats(int F, int H, int CS) {
  return 2 * (((F * H + 3) & ~3) + H * CS) + BC_R * H + 2 * BC_R * CS + 2 * CS;
}

template <int LH, int KH>
__global__ __launch_bounds__(256) void k_score_bnn_class(const float* __restrict__ theta, int n, int d, int F, int H, int C,
                                                         BnnClassCols c, const float* __restrict__ X,
                                                         const int* __restrict__ labels, int B, int crows, float scale,
                                                         float prior_precision, float gamma_rate, float* __restrict__ score) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int PPW = 256 / LH, NW = LH / 64;
  const int CS = (C + 3) & ~3, cq = CS / 4, FH = F * H, FH4 = (FH + 3) & ~3, HCS = H * CS, HC = H * C;
  const int pf = bc_particle_floats(F, H, CS);
  const int t = threadIdx.x, lane = t % LH, sub = t / LH, wave = t >> 6;
  float* w1p = lds + (size_t)sub * pf;     // [F][H]
  float* w2p = w1p + FH4;                  // [H][CS]
  float* g1p = w2p + HCS;                  // [F][H]
  float* g2p = g1p + FH4;                  // [H][CS]
  float* ap = g2p + HCS;                   // [H][BC_R]
  float* zp = ap + BC_R * H;               // [BC_R][CS]
  float* rp = zp + BC_R * CS;              // [BC_R][CS]
  float* b2p = rp + BC_R * CS;             // [CS]
  float* gb2p = b2p + CS;                  // [CS]
  float* xs = lds + (size_t)PPW * pf;      // [crows / BC_R][F][BC_R]
  int* ys = reinterpret_cast<int*>(xs + (size_t)crows * F);   // [crows]
  float* red = reinterpret_cast<float*>(ys + crows);          // [4 waves]
  const int nchunks = (B + crows - 1) / crows;
  auto stage = [&](int c0) {               // rows past the batch are staged as zeros (their residuals are forced to 0 below)
    const int rows = min(crows, B - c0), rows8 = (rows + BC_R - 1) & ~(BC_R - 1);
    for (int i = t; i < rows8 * F; i += 256) {
      const int r = i / F, f = i - r * F;
      xs[((r / BC_R) * F + f) * BC_R + (r % BC_R)] = r < rows ? X[(size_t)(c0 + r) * F + f] : 0.f;
    }
    for (int i = t; i < rows8; i += 256) ys[i] = i < rows ? labels[c0 + i] : 0;
  };
  if (nchunks == 1) stage(0);              // the barriers of the particle loop follow
  for (long p0 = (long)blockIdx.x * PPW; p0 < n; p0 += (long)gridDim.x * PPW) {
    const long p = p0 + sub;
    const bool live = p < n;
    const float* th = theta + (size_t)(live ? p : 0) * d;
    __syncthreads();                       // every lane is past the last particle's LDS
    for (int i = lane; i < FH; i += LH) {
      w1p[i] = th[c.w1 + i];
      g1p[i] = 0.f;
    }
    for (int i = lane; i < HCS; i += LH) {
      const int h = i / CS, cc = i - h * CS;
      w2p[i] = cc < C ? th[c.w2 + h * C + cc] : 0.f;
      g2p[i] = 0.f;
    }
    if (lane < CS) b2p[lane] = lane < C ? th[c.b2 + lane] : 0.f;
    float b1[KH], gb1[KH], gb2 = 0.f;
    bool ok[KH];
#pragma unroll
    for (int k = 0; k < KH; ++k) {
      const int h = lane + LH * k;
      ok[k] = h < H;
      b1[k] = ok[k] ? th[c.b1 + h] : 0.f;
      gb1[k] = 0.f;
    }
    for (int ch = 0; ch < nchunks; ++ch) {
      __syncthreads();                     // the particle is staged; every lane is past the last chunk's rows
      if (nchunks > 1) {
        stage(ch * crows);
        __syncthreads();
      }
      const int rows = min(crows, B - ch * crows);
      for (int r0 = 0; r0 < rows; r0 += BC_R) {
        const float* xb = xs + (size_t)(r0 / BC_R) * F * BC_R;
        // A: the pre-activations of the lane's hidden units, the activations to LDS
        float z[KH][BC_R];
#pragma unroll
        for (int k = 0; k < KH; ++k)
#pragma unroll
          for (int r = 0; r < BC_R; ++r) z[k][r] = b1[k];
#pragma unroll 2
        for (int f = 0; f < F; ++f) {
          const float4 xa = *reinterpret_cast<const float4*>(xb + f * BC_R);
          const float4 xc = *reinterpret_cast<const float4*>(xb + f * BC_R + 4);
          const float x[BC_R] = {xa.x, xa.y, xa.z, xa.w, xc.x, xc.y, xc.z, xc.w};
#pragma unroll
          for (int k = 0; k < KH; ++k) {
            const float w = ok[k] ? w1p[f * H + lane + LH * k] : 0.f;
#pragma unroll
            for (int r = 0; r < BC_R; ++r) z[k][r] = fmaf(x[r], w, z[k][r]);
          }
        }
#pragma unroll
        for (int k = 0; k < KH; ++k)
          if (ok[k]) {
            float4* ao = reinterpret_cast<float4*>(ap + (lane + LH * k) * BC_R);
            ao[0] = make_float4(fmaxf(z[k][0], 0.f), fmaxf(z[k][1], 0.f), fmaxf(z[k][2], 0.f), fmaxf(z[k][3], 0.f));
            ao[1] = make_float4(fmaxf(z[k][4], 0.f), fmaxf(z[k][5], 0.f), fmaxf(z[k][6], 0.f), fmaxf(z[k][7], 0.f));
          }
        __syncthreads();
        // B: the logits of the block's (row, class) pairs
        for (int pr = lane; pr < BC_R * CS; pr += LH) {
          const int r = pr / CS, cc = pr - r * CS;
          float zz = b2p[cc];
          const float* ar = ap + r;
          const float* wc = w2p + cc;
#pragma unroll 4
          for (int h = 0; h < H; ++h) zz = fmaf(ar[h * BC_R], wc[h * CS], zz);
          zp[pr] = zz;
        }
        __syncthreads();
        // S: the softmax of the pair's row, the residual
        for (int pr = lane; pr < BC_R * CS; pr += LH) {
          const int r = pr / CS, cc = pr - r * CS;
          const float* zr = zp + r * CS;
          float m = zr[0];
          for (int j = 1; j < C; ++j) m = fmaxf(m, zr[j]);
          float s = 0.f;
          for (int j = 0; j < C; ++j) s += expf(zr[j] - m);
          const int yb = ys[r0 + r];
          const float bad = (yb < 0 || yb >= C) ? __builtin_nanf("") : 0.f;
          const float pc = expf(zr[min(cc, C - 1)] - m) / s;
          rp[pr] = (r0 + r < rows && cc < C) ? ((cc == yb ? 1.f : 0.f) - pc) + bad : 0.f;
        }
        __syncthreads();
        // C: delta, gw2 and gb1 of the lane's hidden units, gb2 on the first C lanes, then gw1
#pragma unroll
        for (int k = 0; k < KH; ++k) {
          if (ok[k]) {
            const int h = lane + LH * k;
            float dl[BC_R], a[BC_R];
#pragma unroll
            for (int r = 0; r < BC_R; ++r) {
              dl[r] = 0.f;
              a[r] = fmaxf(z[k][r], 0.f);
            }
            for (int q = 0; q < cq; ++q) {
              const float4 w = *reinterpret_cast<const float4*>(w2p + h * CS + 4 * q);
              float4* gp = reinterpret_cast<float4*>(g2p + h * CS + 4 * q);
              float4 g = *gp;
#pragma unroll
              for (int r = 0; r < BC_R; ++r) {
                const float4 e = *reinterpret_cast<const float4*>(rp + r * CS + 4 * q);
                dl[r] = fmaf(e.x, w.x, dl[r]);
                dl[r] = fmaf(e.y, w.y, dl[r]);
                dl[r] = fmaf(e.z, w.z, dl[r]);
                dl[r] = fmaf(e.w, w.w, dl[r]);
                g.x = fmaf(a[r], e.x, g.x);
                g.y = fmaf(a[r], e.y, g.y);
                g.z = fmaf(a[r], e.z, g.z);
                g.w = fmaf(a[r], e.w, g.w);
              }
              *gp = g;
            }
#pragma unroll
            for (int r = 0; r < BC_R; ++r) {
              const float tk = z[k][r] > 0.f ? dl[r] : 0.f;
              gb1[k] += tk;
              z[k][r] = tk;
            }
          }
        }
        if (lane < C) {
#pragma unroll
          for (int r = 0; r < BC_R; ++r) gb2 += rp[r * CS + lane];
        }
#pragma unroll 2
        for (int f = 0; f < F; ++f) {
          const float4 xa = *reinterpret_cast<const float4*>(xb + f * BC_R);
          const float4 xc = *reinterpret_cast<const float4*>(xb + f * BC_R + 4);
          const float x[BC_R] = {xa.x, xa.y, xa.z, xa.w, xc.x, xc.y, xc.z, xc.w};
#pragma unroll
          for (int k = 0; k < KH; ++k) {
            if (ok[k]) {
              float g = g1p[f * H + lane + LH * k];
#pragma unroll
              for (int r = 0; r < BC_R; ++r) g = fmaf(z[k][r], x[r], g);
              g1p[f * H + lane + LH * k] = g;
            }
          }
        }
      }
    }
    // the sum of squares of the four blocks: the lane's strided share, the lanes of a wave, the particle's waves in order
    float sw2 = 0.f;
    for (int i = lane; i < FH; i += LH) sw2 = fmaf(w1p[i], w1p[i], sw2);
    for (int i = lane; i < HCS; i += LH) sw2 = fmaf(w2p[i], w2p[i], sw2);
#pragma unroll
    for (int k = 0; k < KH; ++k) sw2 = fmaf(b1[k], b1[k], sw2);
    if (lane < CS) sw2 = fmaf(b2p[lane], b2p[lane], sw2);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sw2 += __shfl_xor(sw2, o);
    if ((t & 63) == 0) red[wave] = sw2;
    if (lane < C) gb2p[lane] = gb2;
    __syncthreads();                       // the gradients, gb2 and the waves' sums are whole
    sw2 = red[sub * NW];
#pragma unroll
    for (int w = 1; w < NW; ++w) sw2 += red[sub * NW + w];
    if (live) {
      const float prec = c.loglam >= 0 ? expf(th[c.loglam]) : prior_precision;
      const float poison = gb2p[0] != gb2p[0] ? __builtin_nanf("") : 0.f;   // a label outside [0, C): r_b0 is NaN
      float* out = score + (size_t)p * d;
      for (int j = lane; j < d; j += LH) {   // columns outside the model carry no gradient
        const bool in_model = (j >= c.w1 && j < c.w1 + FH) || (j >= c.b1 && j < c.b1 + H) || (j >= c.w2 && j < c.w2 + HC) ||
                              (j >= c.b2 && j < c.b2 + C) || j == c.loglam;
        if (!in_model) out[j] = 0.f;
      }
      for (int i = lane; i < FH; i += LH) out[c.w1 + i] = (scale * g1p[i] - prec * w1p[i]) + poison;
      for (int i = lane; i < HC; i += LH) {
        const int h = i / C, cc = i - h * C;
        out[c.w2 + i] = (scale * g2p[h * CS + cc] - prec * w2p[h * CS + cc]) + poison;
      }
#pragma unroll
      for (int k = 0; k < KH; ++k)
        if (ok[k]) out[c.b1 + lane + LH * k] = (scale * gb1[k] - prec * b1[k]) + poison;
      if (lane < C) out[c.b2 + lane] = (scale * gb2p[lane] - prec * b2p[lane]) + poison;
      if (c.loglam >= 0 && lane == 0)
        out[c.loglam] = 0.5f * (float)(FH + H + HC + C) - prec * (0.5f * sw2 + gamma_rate);
    }
  }
}

// the kernels take up to 158 KB of dynamic LDS: raise each one's limit once per device
static int score_bnn_class_attr(const void* fn, int slot) {
  static bool attr_set[4][64] = {{false}};
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64 || !attr_set[slot][dev]) {
    HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    if (dev >= 0 && dev < 64) attr_set[slot][dev] = true;
  }
  return STEIN_OK;
}

extern "C" int stein_score_bnn_class(const float* theta, int64_t n, int64_t d, int64_t n_in, int64_t n_hidden, int64_t n_classes,
                                     const int64_t* cols /*[5]: w1, b1, w2, b2, log_lambda (< 0: none)*/, const float* X,
                                     const int32_t* labels, int64_t batch, double scale, double prior_precision,
                                     double gamma_rate, float* score, void* stream) {
  if (!theta || !cols || !X || !labels || !score) return stein_fail(STEIN_E_BADARG, "NULL pointer");
  if (n < 1 || d < 1 || batch < 1 || n_in < 1 || n_hidden < 1 || n_classes < 1 || n > 0x7fffffffl || d > 0x7fffffffl ||
      batch > 0x7fffffffl)
    return stein_fail(STEIN_E_SHAPE, "bad shape n=%lld d=%lld batch=%lld n_in=%lld H=%lld C=%lld", (long long)n, (long long)d,
                      (long long)batch, (long long)n_in, (long long)n_hidden, (long long)n_classes);
  if (n_in > BC_NIN_MAX) return stein_fail(STEIN_E_UNSUPPORTED, "more than %d input features", BC_NIN_MAX);
  if (n_classes < BC_C_MIN) return stein_fail(STEIN_E_UNSUPPORTED, "fewer than %d classes", BC_C_MIN);
  if (n_classes > BC_C_MAX) return stein_fail(STEIN_E_UNSUPPORTED, "more than %d classes", BC_C_MAX);
  if (n_hidden > BC_H_MAX) return stein_fail(STEIN_E_UNSUPPORTED, "more than %d hidden units", BC_H_MAX);
  const int C = (int)n_classes, F = (int)n_in, H = (int)n_hidden, CS = (C + 3) & ~3;
  if ((F + CS) * H > BC_W_MAX)
    return stein_fail(STEIN_E_UNSUPPORTED, "more than %d weights ((n_in + CS) * n_hidden, CS = n_classes rounded up to 4)",
                      BC_W_MAX);
  const int64_t len[5] = {n_in * n_hidden, n_hidden, n_hidden * n_classes, n_classes, 1};
  for (int i = 0; i < 5; ++i) {
    if (i == 4 && cols[4] < 0) break;      // no log-lambda entry
    if (cols[i] < 0 || cols[i] + len[i] > d) return stein_fail(STEIN_E_SHAPE, "block %d does not fit d=%lld", i, (long long)d);
    for (int j = 0; j < i; ++j)
      if (cols[i] < cols[j] + len[j] && cols[j] < cols[i] + len[i]) return stein_fail(STEIN_E_SHAPE, "blocks %d and %d overlap", j, i);
  }
  BnnClassCols c = {(int)cols[0], (int)cols[1], (int)cols[2], (int)cols[3], cols[4] < 0 ? -1 : (int)cols[4]};
  // lanes per particle: the hidden units rounded up to whole waves, and no more particles per workgroup than BC_PLDS holds;
  // rows per chunk: what the rest of the LDS holds (a row of X and its label), whole blocks of BC_R, no more than the batch
  const int pf = bc_particle_floats(F, H, CS);
  int lh = H <= 64 ? 64 : H <= 128 ? 128 : 256;
  while (lh < 256 && (256 / lh) * pf > BC_PLDS) lh *= 2;
  const int ppw = 256 / lh;
  const int kh = (H + lh - 1) / lh;
  int64_t crows = ((BC_LDS - ppw * pf - 8) / (F + 1)) & ~(int64_t)(BC_R - 1);
  if (crows > BC_ROWS_MAX) crows = BC_ROWS_MAX;
  const int64_t b8 = (batch + BC_R - 1) & ~(int64_t)(BC_R - 1);
  if (crows > b8) crows = b8;
  if (crows < BC_R || kh > 2)   // (no shape of the domain gets here: tests/test_netclass_cases.py walks all of them)
    return stein_fail(STEIN_E_UNSUPPORTED, "launch plan: %lld chunk rows, %d units per lane", (long long)crows, kh);
  const size_t lds_bytes = ((size_t)ppw * pf + (size_t)crows * (F + 1) + 4) * sizeof(float);
  long blocks = (long)((n + ppw - 1) / ppw);
  if (blocks > BC_MAX_WGS) blocks = BC_MAX_WGS;
  hipStream_t s = (hipStream_t)stream;
#define BC_LAUNCH(LH, KH, SLOT)                                                                                          \
  do {                                                                                                                   \
    if (int rc = score_bnn_class_attr(reinterpret_cast<const void*>(k_score_bnn_class<LH, KH>), SLOT)) return rc;        \
    hipLaunchKernelGGL((k_score_bnn_class<LH, KH>), dim3((unsigned)blocks), dim3(256), lds_bytes, s, theta, (int)n,       \
                       (int)d, F, H, C, c, X, labels, (int)batch, (int)crows, (float)scale, (float)prior_precision,       \
                       (float)gamma_rate, score);                                                                         \
  } while (0)
  if (lh == 64) BC_LAUNCH(64, 1, 0);
  else if (lh == 128) BC_LAUNCH(128, 1, 1);
  else if (kh <= 1) BC_LAUNCH(256, 1, 2);
  else BC_LAUNCH(256, 2, 3);
#undef BC_LAUNCH
  LAUNCH_CHECK("k_score_bnn_class");
  return STEIN_OK;
}
