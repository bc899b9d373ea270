// stein_x3.h -- host entry points of the split-precision ("x3") kernels in stein_x3.hip.  Each takes the call's views
// (StepViews, stein_host.h: the planes' typed parts, the partial sums and the contraction plan), never a layout to unpack,
// and checks the grid it computes.
#pragma once
#include "stein_host.h"

// dtype = STEIN_F32: fp32 inputs, two fp16 planes, three products; STEIN_BF16: bf16 inputs, one plane, one product
int stein_x3_kind(int dtype);   // 1 or 2
// what the fused call adds to the split: it has zeroed the column maxima and the completion counters `done`, and gives both
// matrices, so the column-maxima kernel's last workgroup writes the scales itself
struct SplitFused {
  HistSync* done;
  const PrologueArgs* prologue;   // bf16 inputs: the launch also does the prologue's work (which writes the neutral scales)
  int fold;   // folded operand: the score only feeds the column maxima; 1: no theta^T planes either, 2: with them
  // fold == 1: no column maxima here at all.  The prologue left max|theta| of each of its nwg workgroups in wgmax, and
  // k_split_rows makes the scale of theta's row-major planes (and sc[4 dc + 0 .. 2]) of them; the maxima come with the select
  const u32* wgmax; int nwg;
};
int stein_x3_split(const StepViews& v, const void* theta_all, const void* score_all, int dtype, int64_t n, int64_t d,
                   hipStream_t stream, const SplitFused* fused);
// the folded operand of the fused call (fp32 inputs): W = G - theta / h2 replaces the score in the contraction
bool stein_fold_pays(int64_t n, int64_t d);   // the default gate (STEIN_FLAG_FOLD / STEIN_FLAG_NO_FOLD override it)
int stein_x3_split_w(const StepViews& v, const float* theta_all, const float* score_all, int64_t n, int64_t d,
                     const float* h2_dev, hipStream_t stream);   // after the median, before the contraction
// the column maxima of both matrices into v.cmax (zeroed by the caller's prologue), no scales: the folded step's fallback
// when the select launch runs without its slice
int stein_x3_colmax(const StepViews& v, const float* theta_all, const float* score_all, int64_t n, int64_t d,
                    hipStream_t stream);
int stein_x3_contract_fold(const StepViews& v, const float* h2_dev, int64_t n, int64_t d, bool with_theta,
                           hipStream_t stream);
// window: also feed the speculative median window (v.spec, v.spec_buf; needs v.hist)
int stein_x3_distance(const StepViews& v, const BlockShape& b, bool symmetric, bool window, hipStream_t stream,
                      int panel /* -1: never the panel-resident kernel, 1: whenever it can run, 0: where it pays */);
// stein_dpanel.hip: the panel-resident distance kernel and the test that picks it (stein_x3_distance applies it)
bool stein_dpanel_ok(const StepViews& v, const BlockShape& b, bool any_size);
int stein_dpanel_distance(const StepViews& v, const BlockShape& b, bool symmetric, bool window, hipStream_t stream);
int stein_x3_contract_partial(const StepViews& v, const BlockShape& b, const float* h2_dev, hipStream_t stream,
                              bool upper /* v.D holds only the tiles on and above the diagonal of a symmetric block (what
                              stein_x3_distance(symmetric) stores) */);
