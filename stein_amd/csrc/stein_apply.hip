// stein_apply.hip -- the optimizer step behind phi (clip by |phi|, Adagrad or Adam, theta += step, one streaming pass
// each) and the dtype casts of the host layer, with their C ABI entry points.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>
#include <math.h>
#include <type_traits>

#include "stein_host.h"

// ------------------------------------------------------------------------------------------------
// optimizer apply (clip + map + theta += step); arithmetic in fp64, storage S = float or double
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double clip_scale_of(const double* sq, double host_scale, double thr) {
  if (!sq) return host_scale;
  const double nrm = sqrt(*sq);
  return thr / (nrm > thr ? nrm : thr);
}

// one element of the Adagrad map (adagrad_gradient_descent.py:37-44), the same instruction sequence on every path
// (no compiler-chosen fma contraction: the 16-byte and the scalar loops must agree to the last bit)
template <typename C>
__device__ __forceinline__ C adagrad_elem(C p, C h, int first, C a, C na, C ep, C l, C* hs_out) {
#pragma clang fp contract(off)
  const C pp = p * p;
  const C hs = first ? pp : a * h + na * pp;
  *hs_out = hs;
  return p / (ep + sqrt(hs)) * l;
}

template <typename S, typename P>
__global__ __launch_bounds__(256) void k_apply_adagrad(S* __restrict__ theta, const P* __restrict__ phi,
                                                       S* __restrict__ hist, long count, const double* sq,
                                                       double host_scale, double thr, double lr, double alpha,
                                                       double eps, int first, S* __restrict__ step_out, int vec) {
  // arithmetic in the storage type: fp64 state -> fp64 (the reference's NumPy arithmetic), fp32 state -> fp32 (the
  // results are rounded to fp32 anyway, and the fp64 square root and division made the kernel compute-bound: 25 us
  // for 80 MB at C3)
  typedef typename std::conditional<sizeof(S) == 4, float, double>::type C;
  const C scale = (C)clip_scale_of(sq, host_scale, thr);
  const C a = (C)alpha, na = (C)(1.0 - alpha), ep = (C)eps, l = (C)lr;
  if (sizeof(S) == 4 && sizeof(P) == 4 && vec) {   // host: count % 4 == 0, theta present, every pointer 16-byte aligned, no step_out
    float4* th4 = reinterpret_cast<float4*>(theta);
    float4* hi4 = reinterpret_cast<float4*>(hist);
    const float4* ph4 = reinterpret_cast<const float4*>(phi);
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < (count >> 2); q += (long)gridDim.x * 256) {
      const float4 pv = ph4[q], hv = hi4[q];
      float4 tv = th4[q], ho;
      const float pp[4] = {pv.x, pv.y, pv.z, pv.w}, hh[4] = {hv.x, hv.y, hv.z, hv.w};
      float tt[4] = {tv.x, tv.y, tv.z, tv.w}, oo[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float hs;
        const float step = adagrad_elem<float>(pp[k] * (float)scale, hh[k], first, (float)a, (float)na, (float)ep, (float)l, &hs);
        oo[k] = hs;
        tt[k] = tt[k] + step;
      }
      ho = make_float4(oo[0], oo[1], oo[2], oo[3]);
      tv = make_float4(tt[0], tt[1], tt[2], tt[3]);
      hi4[q] = ho;
      th4[q] = tv;
    }
    return;
  }
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < count; e += (long)gridDim.x * 256) {
    C hs;
    const C step = adagrad_elem<C>((C)phi[e] * scale, (C)hist[e], first, a, na, ep, l, &hs);
    hist[e] = (S)hs;
    if (step_out) step_out[e] = (S)step;
    if (theta) theta[e] = (S)((C)theta[e] + step);
  }
}

template <typename S, typename P>
__global__ __launch_bounds__(256) void k_apply_adam(S* __restrict__ theta, const P* __restrict__ phi,
                                                    S* __restrict__ mu, S* __restrict__ nu, long count,
                                                    const double* sq, double host_scale, double thr, double lr,
                                                    double b1, double b2, double eps, int first, double corr1,
                                                    double corr2, S* __restrict__ step_out) {
  typedef typename std::conditional<sizeof(S) == 4, float, double>::type C;   // as in k_apply_adagrad
  const C scale = (C)clip_scale_of(sq, host_scale, thr);
  const C c1 = (C)b1, n1 = (C)(1.0 - b1), c2 = (C)b2, n2 = (C)(1.0 - b2), ep = (C)eps, l = (C)lr;
  const C k1 = (C)corr1, k2 = (C)corr2;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < count; e += (long)gridDim.x * 256) {
    const C p = (C)phi[e] * scale;
    const C m = first ? p : c1 * (C)mu[e] + n1 * p;
    const C v = first ? p * p : c2 * (C)nu[e] + n2 * p * p;
    mu[e] = (S)m;
    nu[e] = (S)v;
    const C step = (m / k1) / (ep + sqrt(v / k2)) * l;
    if (step_out) step_out[e] = (S)step;
    if (theta) theta[e] = (S)((C)theta[e] + step);
  }
}

__global__ __launch_bounds__(256) void k_cast_f64_f32(const double* __restrict__ s, float* __restrict__ o, long count) {
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < count; e += (long)gridDim.x * 256) o[e] = (float)s[e];
}
__global__ __launch_bounds__(256) void k_cast_f32_bf16(const float* __restrict__ s, __hip_bfloat16* __restrict__ o,
                                                       long count) {
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < count; e += (long)gridDim.x * 256)
    o[e] = __float2bfloat16(s[e]);
}

template <typename S, typename P>
static int apply_adagrad_t(void* theta, const void* phi, void* hist, int64_t count, const double* sq, double hs,
                           double thr, double lr, double alpha, double eps, int first, void* step_out, void* stream) {
  auto al16 = [](const void* p) { return ((uintptr_t)p & 15u) == 0; };
  const int vec = sizeof(S) == 4 && sizeof(P) == 4 && count % 4 == 0 && theta && !step_out && al16(theta) && al16(phi) && al16(hist);
  hipLaunchKernelGGL((k_apply_adagrad<S, P>), dim3(grid_for(vec ? count / 4 : count, 2048)), dim3(256), 0, (hipStream_t)stream,
                     (S*)theta, (const P*)phi, (S*)hist, (long)count, sq, hs, thr, lr, alpha, eps, first, (S*)step_out, vec);
  LAUNCH_CHECK("k_apply_adagrad");
  return STEIN_OK;
}

// phi_dtype STEIN_F64 needs fp64 state: the reference's pure-fp64 `gd.update(phi)` (no rounding of phi to fp32)
static int check_apply_dtypes(int state_dtype, int phi_dtype) {
  if (state_dtype != STEIN_F32 && state_dtype != STEIN_F64) return fail(STEIN_E_UNSUPPORTED, "state dtype %d", state_dtype);
  if (phi_dtype != STEIN_F32 && phi_dtype != STEIN_F64) return fail(STEIN_E_UNSUPPORTED, "phi dtype %d", phi_dtype);
  if (phi_dtype == STEIN_F64 && state_dtype != STEIN_F64) return fail(STEIN_E_UNSUPPORTED, "fp64 phi needs fp64 optimizer state");
  return STEIN_OK;
}

extern "C" int stein_apply_adagrad(void* theta, const void* phi, int phi_dtype, void* hist, int64_t count, int state_dtype,
                                   const double* sqnorm_dev, double clip_scale_host, double clip_threshold, double lr,
                                   double alpha, double eps, int first_step, void* step_out, void* stream) {
  if (!phi || !hist) return fail(STEIN_E_BADARG, "NULL pointer");
  if (count < 1) return fail(STEIN_E_SHAPE, "count < 1");
  if (int rc = check_apply_dtypes(state_dtype, phi_dtype)) return rc;
  if (int rc = stein_take_device_error()) return rc;
  if (state_dtype == STEIN_F32)
    return apply_adagrad_t<float, float>(theta, phi, hist, count, sqnorm_dev, clip_scale_host, clip_threshold, lr, alpha, eps,
                                         first_step, step_out, stream);
  if (phi_dtype == STEIN_F32)
    return apply_adagrad_t<double, float>(theta, phi, hist, count, sqnorm_dev, clip_scale_host, clip_threshold, lr, alpha,
                                          eps, first_step, step_out, stream);
  return apply_adagrad_t<double, double>(theta, phi, hist, count, sqnorm_dev, clip_scale_host, clip_threshold, lr, alpha,
                                         eps, first_step, step_out, stream);
}

template <typename S, typename P>
static int apply_adam_t(void* theta, const void* phi, void* mu, void* nu, int64_t count, const double* sq, double hs,
                        double thr, double lr, double b1, double b2, double eps, int64_t t, void* step_out,
                        void* stream) {
  const double corr1 = 1.0 - pow(b1, (double)t), corr2 = 1.0 - pow(b2, (double)t);
  hipLaunchKernelGGL((k_apply_adam<S, P>), dim3(grid_for(count, 2048)), dim3(256), 0, (hipStream_t)stream, (S*)theta,
                     (const P*)phi, (S*)mu, (S*)nu, (long)count, sq, hs, thr, lr, b1, b2, eps, t == 1 ? 1 : 0, corr1, corr2,
                     (S*)step_out);
  LAUNCH_CHECK("k_apply_adam");
  return STEIN_OK;
}

extern "C" int stein_apply_adam(void* theta, const void* phi, int phi_dtype, void* mu, void* nu, int64_t count,
                                int state_dtype, const double* sqnorm_dev, double clip_scale_host, double clip_threshold,
                                double lr, double beta1, double beta2, double eps, int64_t t, void* step_out, void* stream) {
  if (!phi || !mu || !nu) return fail(STEIN_E_BADARG, "NULL pointer");
  if (count < 1 || t < 1) return fail(STEIN_E_SHAPE, "count < 1 or t < 1");
  if (int rc = check_apply_dtypes(state_dtype, phi_dtype)) return rc;
  if (int rc = stein_take_device_error()) return rc;
  if (state_dtype == STEIN_F32)
    return apply_adam_t<float, float>(theta, phi, mu, nu, count, sqnorm_dev, clip_scale_host, clip_threshold, lr, beta1,
                                      beta2, eps, t, step_out, stream);
  if (phi_dtype == STEIN_F32)
    return apply_adam_t<double, float>(theta, phi, mu, nu, count, sqnorm_dev, clip_scale_host, clip_threshold, lr, beta1,
                                       beta2, eps, t, step_out, stream);
  return apply_adam_t<double, double>(theta, phi, mu, nu, count, sqnorm_dev, clip_scale_host, clip_threshold, lr, beta1,
                                      beta2, eps, t, step_out, stream);
}

extern "C" int stein_cast_f64_to_f32(const double* src, float* dst, int64_t count, void* stream) {
  if (!src || !dst) return fail(STEIN_E_BADARG, "NULL pointer");
  if (count < 1) return fail(STEIN_E_SHAPE, "count < 1");
  hipLaunchKernelGGL(k_cast_f64_f32, dim3(grid_for(count, 2048)), dim3(256), 0, (hipStream_t)stream, src, dst,
                     (long)count);
  LAUNCH_CHECK("k_cast_f64_f32");
  return STEIN_OK;
}

extern "C" int stein_cast_f32_to_bf16(const float* src, void* dst, int64_t count, void* stream) {
  if (!src || !dst) return fail(STEIN_E_BADARG, "NULL pointer");
  if (count < 1) return fail(STEIN_E_SHAPE, "count < 1");
  hipLaunchKernelGGL(k_cast_f32_bf16, dim3(grid_for(count, 2048)), dim3(256), 0, (hipStream_t)stream, src,
                     (__hip_bfloat16*)dst, (long)count);
  LAUNCH_CHECK("k_cast_f32_bf16");
  return STEIN_OK;
}
