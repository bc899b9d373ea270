// stein_host.h -- host-side declarations shared by the library's translation units (internal: the ABI is include/steinhip.h)
#pragma once

#include "stein_common.h"

#define fail stein_fail

constexpr int MAX_DEVICES = 64;   // per-device host state (the error word, k_hist_all's residency) for devices 0 .. 63

static inline int grid_for(long count, int cap) {
  long b = (count + 255) / 256;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

// addresses inside the SELECT section (SelState | SpecState | FuseState) and the SPEC section (slots | entries | table)
static inline SpecState* spec_of(void* select_state) { return (SpecState*)((char*)select_state + sizeof(SelState)); }
static inline FuseState* fuse_of(void* select_state) { return (FuseState*)((char*)spec_of(select_state) + sizeof(SpecState)); }
static inline u64* spec_table_of(void* spec_buf) { return (u64*)spec_buf + SPEC_TABLE_AT; }

// every section of one workspace (stein_workspace_layout) as a pointer; planes is NULL when the layout has none
struct StepViews {
  SteinLayout L;
  float* r; float* D; u64* hist;
  SelState* sel; SpecState* spec; FuseState* fuse;
  u64* spec_buf; u64* table;   // the SPEC section and its rank-summed window table (k_hist_all's HistSync in the fused call)
  char* planes;
  float* OG; float* OT; float* RS; double* SQ;
};
StepViews stein_step_views(const SteinLayout& L, void* workspace);

// steinhip.hip: the device error word (one u32 per device in page-locked host memory that a kernel raises when it gave up)
int stein_device_error_word(u32** out);
int stein_take_device_error(void);

// stein_select.hip: the fused call's median behind its distance pass (k_spec_select, then k_hist_all unless n is small)
int stein_fused_select(const StepViews& v, int64_t n, float* h2_out, hipStream_t stream);

// stein_fp32.hip: the fp32-input MFMA kernels, for calls without the split planes (what stein_x3_distance and
// stein_x3_contract_partial are for the split path)
int stein_fp32_distance(const float* theta_all, const float* r_all, float* dist_out, int64_t n, int64_t d, int64_t row0,
                        int64_t n_local, int64_t ld_dist, u64* hist0, bool symmetric, hipStream_t stream, SpecState* spec,
                        u64* spec_buf);
int stein_fp32_contract_partial(const float* dist, int64_t ld_dist, const float* theta_all, const float* score_all,
                                const SteinLayout& L, const float* h2_dev, float* OG, float* OT, float* RS, int64_t n,
                                int64_t d, int64_t n_local, hipStream_t stream);

// stein_small.hip: the whole phi computation in one kernel for n <= 160 (the reference's own example sizes)
bool stein_small_ok(int64_t n, int64_t d, int dtype);
int stein_small_phi(const float* theta, const float* score, int64_t n, int64_t d, float* phi, float* h2_out,
                    double* sqpart /* one partial |phi|^2 per workgroup, *nparts of them (<= ceil(d / 32)) */,
                    float* K_out, float* dK_out, int* nparts /* 0: a single workgroup wrote *sqnorm_out itself */,
                    double* sqnorm_out, bool ksd /* STEIN_FLAG_KSD: [3][nparts] partials, sqnorm_out double[3] */,
                    hipStream_t stream);
