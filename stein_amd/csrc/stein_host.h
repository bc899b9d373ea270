// stein_host.h -- host-side declarations shared by the library's translation units (internal: the ABI is include/steinhip.h):
// the views of one call (StepViews), the layout flags of each family of entry point, and the stage functions that take them
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

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Workgroups the chip holds at once of a kernel that runs one per CU (128 KB of LDS each: the split-precision contraction,
// k_phi_stream).  The MI355X's 256 CUs, as a constant: the plans and the workspace sizes are host arithmetic.
constexpr double RESIDENT_ONE_PER_CU = 256.0;

// the size limits every layout shares: int indices of rows and columns, and n d elements within 2^40
static inline int stein_check_size(int64_t n, int64_t d) {
  if (n > (1ll << 30) || d > (1ll << 24) || n * d > (1ll << 40)) return fail(STEIN_E_SHAPE, "shape too large");
  return STEIN_OK;
}

// addresses inside the SELECT section (SelState | SpecState | FuseState) and the SPEC section (slots | entries | table)
static inline SpecState* spec_of(void* select_state) { return (SpecState*)((char*)select_state + sizeof(SelState)); }
static inline FuseState* fuse_of(void* select_state) { return (FuseState*)((char*)spec_of(select_state) + sizeof(SpecState)); }
static inline u64* spec_table_of(void* spec_buf) { return (u64*)spec_buf + SPEC_TABLE_AT; }

// rows [row0, row0 + n_local) of n particles with d parameters, inputs of dtype (STEIN_F32 / STEIN_BF16)
struct BlockShape { int64_t n, d, row0, n_local; int dtype; };

// The scales area at SteinLayout::x3_sc of the planes buffer (stein_x3.hip): float sc[4 dc + 4], then the u32 column
// maxima [score | theta] the scales are made from.  As float indices from sc:
static inline size_t x3_sc_two_s(int64_t dc) { return (size_t)(4 * dc + 1); }   // the distance pass's scale, 2^(1 - 2 sa)
static inline size_t x3_sc_cmax(int64_t dc) { return (size_t)(4 * dc + 4); }    // where the column maxima start

// Every address one C call uses, formed once (stein_step_views) from the one layout that call derives: the workspace's
// sections, the split planes with their parts typed, and the partial sums of the contraction in use with its plan.
// An entry point validates, derives its layout, builds these and hands them to the stage functions, which never derive a
// layout themselves.  Layout flags by family of entry point:
//   fused call (stein_svgd_phi)                 the caller's flags
//   staged calls (stein_distance_block*, stein_contract_partial, stein_kernel_contract, stein_x3_prepare)
//                                               stein_staged_flags: (planes ? X3 : 0) | NO_FOLD
//   rank segments (stein_rank_*)                stein_rank_flags: (flags & (X3 | KSD)) | TILED | NO_FOLD
// (stein_contract_finish has no planes argument: it takes the caller's layout flags with NO_FOLD in place of FOLD.)
struct StepViews {
  SteinLayout L;
  float* r; float* D; u64* hist;
  SelState* sel; SpecState* spec; FuseState* fuse;
  u64* spec_buf; u64* table;   // the SPEC section and its rank-summed window table (k_hist_all's HistSync in the fused call)
  // the split planes: the workspace's PLANES section, or the staged ABI's separately allocated buffer.  All NULL without them.
  char* planes;
  unsigned short* T3; unsigned short* Tt3; unsigned short* Gt3;   // theta row-major | theta^T | score^T (folded: W^T)
  float* sc; u32* cmax; float* two_s;   // the scales area, its column maxima and the distance pass's scale
  // partial sums of the contraction: PART_G / PART_T / PART_RS; with L.fold the fold's storage, K.W in OG
  float* OG; float* OT; float* RS; double* SQ;
  int nsplit, jchunk, tsplit;           // j ranges of OG and RS, columns per range, ranges of OT (folded: one)
};
// workspace == NULL (a staged call without one): no section pointers.  planes_override: the staged ABI's planes buffer; the
// plane pointers then come from it and never from the workspace, which need not reach its PLANES section.
StepViews stein_step_views(const SteinLayout& L, void* workspace, void* planes_override = nullptr);
static inline int stein_staged_flags(bool x3) { return (x3 ? STEIN_FLAG_X3 : 0) | STEIN_FLAG_NO_FOLD; }
// (the rank segments keep K.[G | theta]: the score's planes are built while its all-gather overlaps the distance pass,
// before h2 exists.  The workspace may have been sized with the fold area -- it only adds bytes at the end.)
static inline int stein_rank_flags(int flags) {
  return (flags & (STEIN_FLAG_X3 | STEIN_FLAG_KSD)) | STEIN_FLAG_TILED | STEIN_FLAG_NO_FOLD;
}

// steinhip.hip: the rank segments on views (the public stein_rank_* wrap them; stein_rank_step derives once and calls them)
int stein_rank_views(const BlockShape& b, void* workspace, size_t ws_bytes, int flags, StepViews* v);   // validates too
int stein_rank_begin_on(const StepViews& v, const BlockShape& b, const void* theta_all, bool window, hipStream_t stream);
int stein_rank_pick_on(const StepViews& v, int64_t n, float* h2_out, float* median_out, void* flags_host, hipStream_t stream);
int stein_rank_radix_on(const StepViews& v, const BlockShape& b, int level, int need_pass, float* h2_out, float* median_out,
                        hipStream_t stream);
int stein_rank_finish_on(const StepViews& v, const BlockShape& b, const void* theta_all, const void* score_all,
                         const float* h2_dev, float* phi_local, double* sqnorm_out, float* dK_out, int flags,
                         hipStream_t stream);

// steinhip.hip: the device error word (one u32 per device in page-locked host memory that a kernel raises when it gave up)
int stein_device_error_word(u32** out);
int stein_take_device_error(void);

// stein_stream.hip: the j ranges stein_debug_stream_jsplit asked for on this thread, 0 = the plan's own rule (read by
// stream_make_layout, stein_stream_host.h: the plan of the RBF streaming step and of the IMQ step, stein_imq.hip)
int stein_stream_jsplit_hook(void);

// stein_select.hip: the fused call's median behind its distance pass (k_spec_select, then k_hist_all unless n is small)
// theta_all / score_all: the call's inputs, read by the select launch's slice when the operand is folded: dropped, or --
// want_maxima -- reduced to the column maxima in v.cmax (zeroed by the prologue).  *took_maxima: whether the slice ran and
// did so (not under stein_debug_no_warm: the caller then launches the column maxima itself)
int stein_fused_select(const StepViews& v, int64_t n, int64_t d, float* h2_out, const void* theta_all, const void* score_all,
                       bool want_maxima, bool* took_maxima, hipStream_t stream);

// stein_fp32.hip: the fp32-input MFMA kernels, for calls without the split planes (what stein_x3_distance and
// stein_x3_contract_partial are for the split path).  window: also feed the speculative median window (v.spec, v.spec_buf)
int stein_fp32_distance(const StepViews& v, const BlockShape& b, const float* theta_all, bool symmetric, bool window,
                        hipStream_t stream);
int stein_fp32_contract_partial(const StepViews& v, const BlockShape& b, const float* theta_all, const float* score_all,
                                const float* h2_dev, hipStream_t stream);

// stein_small.hip: the whole phi computation in one kernel for n <= 160 (the reference's own example sizes)
bool stein_small_ok(int64_t n, int64_t d, int dtype);
int stein_small_phi(const float* theta, const float* score, int64_t n, int64_t d, float* phi, float* h2_out,
                    double* sqpart /* one partial |phi|^2 per workgroup, *nparts of them (<= ceil(d / 32)) */,
                    float* K_out, float* dK_out, int* nparts /* 0: a single workgroup wrote *sqnorm_out itself */,
                    double* sqnorm_out, bool ksd /* STEIN_FLAG_KSD: [3][nparts] partials, sqnorm_out double[3] */,
                    hipStream_t stream);
