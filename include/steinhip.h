/* steinhip.h -- C ABI of libsteinhip.so, the MI355X (gfx950) SVGD particle-update engine.
 *
 * The reference (JamesBrofos/Stein, pure Python) has no FFI layer; its seams on this path are
 * Python duck-typed calls.  Every entry point below names the reference call it replaces
 * (file:line relative to the reference tree).  INTEGRATION.md shows the ctypes stub a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (row-major, contiguous) unless the name ends in _host;
 *     the library never allocates or frees caller memory.  Scratch comes from a caller-owned
 *     workspace sized by stein_workspace_bytes() and described by stein_workspace_layout().
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*); none of them
 *     synchronises with the host.
 *   - return value: 0 on success, a negative STEIN_E_* code otherwise; stein_last_error()
 *     returns a per-thread message for the last failure.
 *   - n = total number of particles, d = parameters per particle.  A rank owns rows
 *     [row0, row0 + n_local) of theta / score / phi / optimizer state; single GPU: row0 = 0,
 *     n_local = n.
 */
#ifndef STEINHIP_H
#define STEINHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STEIN_VERSION 100 /* 0.1.0 */

enum {
  STEIN_OK = 0,
  STEIN_E_BADARG = -1,
  STEIN_E_SHAPE = -2,
  STEIN_E_WORKSPACE = -3,
  STEIN_E_HIP = -4,
  STEIN_E_RCCL = -5, /* an RCCL call of the library's own communicator failed (stein_comm_*, stein_rank_step) */
  STEIN_E_UNSUPPORTED = -6
};

/* element types of caller buffers */
enum { STEIN_F32 = 0, STEIN_BF16 = 1, STEIN_F64 = 2 };

/* flags for stein_svgd_phi / stein_workspace_bytes */
enum {
  STEIN_FLAG_NONE = 0,
  STEIN_FLAG_X3 = 1, /* run both GEMMs on the 16-bit matrix cores at fp32-level accuracy: every fp32 operand is scaled
                        by a power of two and split into two fp16 terms, three products per pair; see
                        stein_amd/csrc/stein_x3.hip.  bf16 inputs use one bf16 product.  Adds the PLANES section to
                        the workspace. */
  STEIN_FLAG_TIMING = 4, /* stein_svgd_phi only: record a HIP event at every stage boundary (see stein_timing_reserve) */
  STEIN_FLAG_TILED = 8,  /* stein_svgd_phi only: never take the one-kernel path for n <= 160 (stein_small.hip); the
                            tiled kernels then also leave D, the histograms and the planes in the workspace */
  STEIN_FLAG_NO_WINDOW = 16, /* stein_svgd_phi only: never grant the speculative median window, i.e. run the radix-select
                                passes over D on every call (same result; what a window miss costs, for measurements) */
  STEIN_FLAG_RANK_WINDOW = 32, /* stein_rank_* only: this step uses the cross-rank speculative window (tally / pick) instead
                                  of the radix-select histograms */
  STEIN_FLAG_TILE_DISTANCE = 64, /* stein_svgd_phi only: run the distance pass with the per-tile kernel even where the
                                    panel-resident form (STEIN_STAGE_TILES below) would be taken; for A/B measurements */
  STEIN_FLAG_TIMING_CONTRACT = 128, /* stein_svgd_phi, with STEIN_FLAG_TIMING: record only the two events that bracket the
                                       contraction (an event between two kernels costs the step ~3 us of GPU time: six of
                                       them perturb what they time); stein_timing_read reports -1 for the other stages */
  STEIN_FLAG_FOLD = 512, /* stein_svgd_phi (and stein_workspace_bytes / _layout): take the folded contraction wherever it is
                            eligible, whatever the size.  Eligible: STEIN_FLAG_X3, fp32 inputs, not the one-kernel path.  The
                            contraction then multiplies K with W = G - theta / h2 alone (phi = (K.W + rowsum(K) theta / h2) / n:
                            half the matrix-core work; W's planes are built behind the median); with dK_out or
                            STEIN_FLAG_KSD, with [W | theta] -- phi, h2 and |phi|^2 are the same to the bit either way.
                            Without either flag the library takes the form where it pays (large blocks).  The staged calls
                            and the rank segments never do.  The fold's partial sums reuse PART_G, PART_T and theta's row-major
                            planes; where they do not fit, this flag appends them to the PLANES section (no other offset
                            moves) and the default leaves the call unfolded.  Every tiled fused call records what it did in
                            the workspace: the uint32 at byte 140 of the SELECT section is 1 after a folded call, else 0. */
  STEIN_FLAG_NO_FOLD = 1024, /* the same calls: never take the folded contraction (A/B measurements; a workspace that only
                                ever serves the staged calls does not need the fold's partial sums either) */
  STEIN_FLAG_KSD = 256 /* stein_svgd_phi, stein_rank_finish, stein_rank_step (and stein_workspace_bytes / _layout, whose
                          SQPART section then holds three partials per block): also the kernelized Stein discrepancy of
                          the particles under the step's own RBF kernel and median bandwidth.  sqnorm_out then points to
                          double[3] = { |phi|^2, S, S_diag } with
                            u_ij = k_ij [ g_i.g_j + (g_i - g_j).(x_i - x_j)/h2 + d/h2 - D_ij/h2^2 ],  k_ij = exp(-D_ij / 2 h2)
                            S = this call's rows' share of  sum_ij u_ij,   S_diag = its share of  sum_i u_ii
                          (x = theta, g = score, h2 = *h2_out), so that  KSD^2_V = S / n^2  and
                          KSD^2_U = (S - S_diag) / (n (n - 1)).  The share is taken per element (i, c) of the rows by an
                          identity that uses the symmetry of K: a rank's S is NOT sum_{i in its rows, j} u_ij;
                          only the sum over all ranks is the statistic (stein_rank_step all-reduces all three doubles).
                          [0] keeps its meaning, so the apply calls read it unchanged; phi, h2 and |phi|^2 are
                          bit-identical to a call without the flag.  stein_contract_finish / stein_kernel_contract have no
                          score operand and refuse the flag (STEIN_E_BADARG).  The flag moves the workspace sections
                          behind SQPART: pass it to every stein_rank_* segment of a step alike. */
};
/* flags for the staged distance / histogram calls */
enum {
  STEIN_STAGE_SYMMETRIC = 1, /* the block is the whole n x n matrix (row0 = 0, n_local = n): compute / count only the
                                upper triangle; the histograms weigh off-diagonal entries by 2.  On the fp32-MFMA path
                                (x3_planes = NULL) the distance pass stores each off-diagonal tile twice (mirrored): a
                                full image.  On the split path it stores ONLY the 128 x 128 tiles on and above the
                                diagonal; pass STEIN_STAGE_UPPER with that image to its readers.  Results are identical. */
  STEIN_STAGE_UPPER = 2,     /* readers of a distance image (stein_contract_partial, stein_kernel_contract,
                                stein_kernel_matrix): the image holds only the tiles on and above the diagonal of the
                                whole symmetric matrix, as stein_distance_block(STEIN_STAGE_SYMMETRIC) with x3_planes
                                leaves it; entries of the other tiles are read from their mirror images */
  STEIN_STAGE_TILES = 4,     /* stein_distance_block*: always the per-tile kernel (one 128 x 128 tile per workgroup).  Without
                                it, large blocks on the split path whose n, n_local and row0 are multiples of 128 take the
                                panel-resident kernels (stein_amd/csrc/stein_dpanel.hip: the operand panel of a row tile in
                                LDS, whole for d <= 256 with fp32 inputs / 512 with bf16, a chunk of K at a time beyond that):
                                the same formula, entries may differ from the per-tile kernel's in the last bit */
  STEIN_STAGE_PANEL = 8      /* stein_distance_block*: take the panel-resident kernel whenever its restrictions hold, however
                                small the block (tests) */
};

/* Workspace sections reported by stein_workspace_layout (byte offsets into the workspace). */
enum {
  STEIN_WS_ROWNORM = 0,  /* float  [n]                      r_i = |theta_i|^2                     */
  STEIN_WS_DIST = 1,     /* float  [n_local][ld_dist]       squared distances, row block          */
  STEIN_WS_HIST = 2,     /* int64  [3 levels][2][2048]      radix-select histograms               */
  STEIN_WS_SELECT = 3,   /* 192 B  select state (ranks, prefixes, median, h2) + the speculative-window state,
                            which must persist from one stein_svgd_phi call to the next, + 64 B of
                            launch tickets private to stein_svgd_phi                                  */
  STEIN_WS_PART_G = 4,   /* float  [split][n_local][d]      partial K.G                           */
  STEIN_WS_PART_T = 5,   /* float  [split][n_local][d]      partial K.theta                       */
  STEIN_WS_PART_RS = 6,  /* float  [split][n_local]         partial rowsum(K)                     */
  STEIN_WS_SQPART = 7,   /* double [sq_blocks]              per-block partial |phi|^2 (STEIN_FLAG_KSD: [3][sq_blocks],
                                                            the S and S_diag partials behind them)  */
  STEIN_WS_SPEC = 8,     /* 16 MB  entries caught by the speculative median window (stein_svgd_phi only)  */
  STEIN_WS_PLANES = 9,   /* split-precision operand planes + scales (STEIN_FLAG_X3 only; empty otherwise), always last */
  STEIN_WS_NSECTIONS = 10
};
/* extra[] entries reported by stein_workspace_layout */
enum { STEIN_WSX_LD_DIST = 0, STEIN_WSX_SPLIT = 1, STEIN_WSX_SQ_BLOCKS = 2, STEIN_WSX_HIST_BINS = 3, STEIN_WSX_N = 4 };

#define STEIN_HIST_BINS 2048
#define STEIN_HIST_LEVELS 3

int stein_version(void);
const char* stein_last_error(void);

/* Workspace sizing. */
int stein_workspace_bytes(int64_t n_local, int64_t n, int64_t d, int dtype, int flags, size_t* out_bytes);
int stein_workspace_layout(int64_t n_local, int64_t n, int64_t d, int dtype, int flags,
                           size_t* offsets /*[STEIN_WS_NSECTIONS]*/, int64_t* extra /*[STEIN_WSX_N]*/);

/* *out = 1 if stein_svgd_phi with these arguments takes the folded contraction (STEIN_FLAG_FOLD), else 0.  Host arithmetic. */
int stein_layout_folds(int64_t n_local, int64_t n, int64_t d, int dtype, int flags, int* out);
/* *out = the j ranges of that call's folded contraction (what its finish pass sums), 0 if it does not fold.  Host arithmetic.
 * stein_debug_fold_split(k) (test hook, per calling thread): k > 0 asks the plan for k ranges instead of its own rule, 0
 * restores the rule.  A range still starts on a multiple of 128 columns and empty tails are dropped, so fewer may come out;
 * the workspace size depends on it: set it before sizing the workspace and keep it through the calls.  Results do not
 * depend on the ranges beyond the order of the fp32 sums over them. */
int stein_layout_fold_ranges(int64_t n_local, int64_t n, int64_t d, int dtype, int flags, int* out);
int stein_debug_fold_split(int ranges);

/* ---- fused single-rank path ------------------------------------------------------------------
 * Replaces AbstractSteinSampler.compute_phi (stein/samplers/abstract_stein_sampler.py:100-105)
 * together with everything it calls: SquaredExponentialKernel.kernel_and_grad
 * (stein/kernels/squared_exponential_kernel.py:25-35), the distance / bandwidth graph
 * (stein/kernels/abstract_kernel.py:30-40) and compute_median (stein/utilities/compute_median.py:4-16).
 *   theta_all, score_all : [n][d] of `dtype` (STEIN_F32 or STEIN_BF16)
 *   phi_local            : [n_local][d] float, rows row0..row0+n_local      (unclipped phi)
 *   h2_out               : float[1], receives bandwidth^2
 *   sqnorm_out           : double[1], receives sum(phi_local^2) (the rank-local part of |phi|_F^2); with
 *                          STEIN_FLAG_KSD double[3]: |phi|^2, S, S_diag (see the flag)
 *   K_out / dK_out       : optional (may be NULL): [n_local][n] float / [n_local][d] float
 * row0 / n_local: this is the SINGLE-RANK entry -- row0 must be 0 and n_local must equal n (one rank sees every row, so
 * the median is global), anything else returns STEIN_E_BADARG.  The two arguments stay in the signature because SURVEY.md
 * section 8(b) fixes it (a binding written against that table keeps working); a rank of a sharded run calls
 * stein_rank_step, or the stein_rank_* segments with its own collectives between them (below).
 * The workspace carries state from one call to the next: the SELECT section keeps the median of the two previous
 * calls and, from the third call on, the distance pass counts the entries below a narrow window around the
 * extrapolated median and collects the entries inside it; when both median ranks fall inside the window an exact
 * selection among the collected entries replaces the two radix-select passes over D, otherwise those run.  The
 * result is identical either way (and for any workspace contents), only the time differs: keep ONE workspace per
 * particle set.
 */
int stein_svgd_phi(const void* theta_all, const void* score_all, int64_t n, int64_t d,
                   int64_t row0, int64_t n_local, int dtype,
                   float* phi_local, float* h2_out, double* sqnorm_out,
                   float* K_out, float* dK_out,
                   void* workspace, size_t ws_bytes, int flags, void* stream);

/* ---- streaming single-rank path: the bandwidth is the caller's, the workspace is O(n d) --------------------------
 * The same reference lines as stein_svgd_phi with SquaredExponentialKernel's bandwidth GIVEN (Liu & Wang's
 * svgd_kernel(theta, h) with h > 0) instead of taken from the median of all n^2 distances:
 *   phi = (K.G + (rowsum(K) theta - K.theta) / h2) / n,   K_ij = exp(-|theta_i - theta_j|^2 / (2 h2)),   h2 = *h2_in
 * With h2 known up front neither the median select nor the n x n distance image is needed: W = G - theta / h2 is built
 * first and every 128 x 128 tile of D is exponentiated and contracted with W as soon as it is complete, then dropped
 * (stein_amd/csrc/stein_stream.hip; same split-fp16 arithmetic per entry as STEIN_FLAG_X3 | STEIN_FLAG_FOLD).
 *   theta, score : [n][d] float (dtype must be STEIN_F32; STEIN_BF16 returns STEIN_E_UNSUPPORTED)
 *   h2_in        : DEVICE float[1], bandwidth^2, read by the kernels of this call: the caller may rewrite it on the stream
 *                  between calls (an annealing schedule, another workspace's h2_out) without a host round trip.  The host
 *                  cannot validate a device scalar: h2 = 0 gives NaN phi, as on every other path.
 *   phi          : [n][d] float (unclipped);  sqnorm_out: double[1] = sum(phi^2), what stein_apply_* read
 *   flags        : must be 0 (STEIN_E_BADARG otherwise).  n >= 1 (no ln n here), d >= 1.
 * Limits of this entry: fp32 inputs, one rank (all n rows), no K_out / dK_out; the Stein discrepancy at this bandwidth is
 * stein_svgd_phi_stream_ksd's, below.  d > 256 is taken
 * in ceil(d / 256) column groups, each of which recomputes the distance tiles: correct for any d, but the
 * stored-D path is the one for wide particles.
 * The workspace must be 16-byte aligned (STEIN_E_BADARG otherwise; hipMalloc and PyTorch allocations are).  It carries
 * nothing from call to call and its contents on entry do not matter.  Its size has no term in n^2:
 *   stein_stream_workspace_bytes = 4 N + 4 (6 dc + 4) + 6 N dk + 6 N dc + 4 jsplit n d + 4 jsplit n + 8 min(1024, ceil(n d / 1024)),
 *   N = roundup(n, 128), dk = roundup(d, 32), dc = roundup(d, 128), every term rounded up to 256 bytes
 *   (row norms | scales | theta's planes | W's planes | partial K.W | partial rowsum(K) | |phi|^2 block partials).
 * stein_stream_plan (host arithmetic): row_tiles = ceil(n / 128), col_groups = ceil(d / 256) and the number of j ranges
 * jsplit = clamp(floor(256 / (row_tiles col_groups)), 1, row_tiles) with empty tails dropped -- one workgroup per
 * (row tile, column group, j range); the ranges' partial sums are added in range order, no float atomics: a repeated call
 * is bit-identical.  The 256 is the MI355X's CU count, built in as a constant (the plan and with it the workspace size stay
 * host arithmetic; on a part with another count the plan is still correct, only less well filled).
 * jsplit > 1 only while the whole grid fits the 256 CUs, so the partial sums hold at most 32 MiB more
 * than n d floats.  stein_debug_stream_jsplit(k) (test hook, per calling thread): k > 0 replaces the floor(...) above in
 * the plan, the workspace size and the call alike; 0 restores the rule. */
int stein_stream_workspace_bytes(int64_t n, int64_t d, int dtype, int flags, size_t* out_bytes);
int stein_stream_plan(int64_t n, int64_t d, int* row_tiles, int* col_groups, int* jsplit);
int stein_svgd_phi_stream(const void* theta, const void* score, int64_t n, int64_t d, int dtype,
                          const float* h2_in, float* phi, double* sqnorm_out,
                          void* workspace, size_t ws_bytes, int flags, void* stream);
int stein_debug_stream_jsplit(int jsplit);

/* ---- streaming step with the kernelized Stein discrepancy at its own bandwidth -------------------------------------
 * stein_svgd_phi_stream and, from the same contraction, the two sums of STEIN_FLAG_KSD (S = sum_ij u_ij, S_diag =
 * sum_i u_ii) of the particles under K at *h2_in.  K.theta is not formed.  With x = theta, g = score, w = g - x / h2 (the
 * operand the step contracts), r_i = |x_i|^2 and D_ij = r_i + r_j - 2 x_i.x_j,
 *   u_ij / k_ij = w_i.w_j - D_ij / (2 h2^2) + b_i + b_j + d / h2,      b_i = g_i.x_i / h2 - r_i / (2 h2^2)
 * and summed over the pairs, per element e = (i, c) with ow = (K.W)_e, rs_i = sum_j k_ij, rd_i = sum_j k_ij D_ij:
 *   S      = sum_e [ w_e ow_e + rs_i (g_e^2 - w_e^2 + 1 / h2) ] - sum_i rd_i / (2 h2^2)
 *   S_diag = sum_e [ g_e^2 + 1 / h2 ]
 * rd is a second running row sum of the contraction's exp phase (k_phi_stream_ksd: one multiply-add per entry of K on
 * values it holds anyway); the finish pass reads the score rows once more and sums in fp64 from the fp32 ow, rs, rd.
 *   phi        : [n][d] float, or NULL: the statistic alone (nothing else changes; the three sums are the same bits)
 *   sums_out   : DEVICE double[3] = |phi|^2, S, S_diag.  KSD^2_V = S / n^2, KSD^2_U = (S - S_diag) / (n (n - 1)).
 *   everything else as stein_svgd_phi_stream: fp32 only (STEIN_BF16: STEIN_E_UNSUPPORTED), flags == 0, a 16-byte-aligned
 *   workspace whose contents on entry do not matter.  phi and sums_out[0] are stein_svgd_phi_stream's to the bit.
 *   stein_stream_ksd_workspace_bytes = stein_stream_workspace_bytes + 4 jsplit n + 16 min(1024, ceil(n d / 1024)), both
 *   terms rounded up to 256 (partial rd | the S and S_diag block partials), appended behind the plain layout: no offset
 *   of it moves, so a buffer of this size serves stein_svgd_phi_stream, stein_stream_median and this call alike. */
int stein_stream_ksd_workspace_bytes(int64_t n, int64_t d, int dtype, int flags, size_t* out_bytes);
int stein_svgd_phi_stream_ksd(const void* theta, const void* score, int64_t n, int64_t d, int dtype,
                              const float* h2_in, float* phi /* may be NULL */,
                              double* sums_out /* [3]: |phi|^2, S, S_diag */,
                              void* workspace, size_t ws_bytes, int flags, void* stream);

/* ---- streaming median: the median-heuristic bandwidth in the streaming step's workspace -----------------------------
 * h2 = median(D) / ln n over all n^2 squared distances (compute_median.py:12-15, abstract_kernel.py:40), exact, without
 * the n x n image: the 3-level radix select of the other paths (11 + 11 + 10 key bits) with the 128 x 128 distance tiles
 * recomputed once per level and counted straight from the matrix-core accumulators (k_stream_hist, stein_stream.hip).
 * The tiles run the distance code of stein_svgd_phi_stream on the same row norms, scales and planes, so the median is
 * that of the D values the step exponentiates; the final arithmetic (median_bandwidth) is every other path's.
 * Chain, all on `stream`, no host read: row norms; theta's scales and row-major planes; select state and histograms
 * zeroed; per level one histogram launch and one resolve.
 *   theta      : [n][d] float (STEIN_F32; STEIN_BF16 returns STEIN_E_UNSUPPORTED)
 *   h2_out     : DEVICE float[1];  median_out: DEVICE float[1] or NULL
 *   flags      : must be 0.  n >= 2 (n = 1: STEIN_E_SHAPE, ln 1 = 0), d >= 1 (any d: the k loop covers ceil(d / 32) tiles)
 * The workspace must be 16-byte aligned; it carries nothing between calls and its contents on entry do not matter.
 *   stein_stream_median_workspace_bytes = 4 N + 4 (6 dc + 4) + 6 N dk (each rounded up to 256, as above) + 98304 + 256
 *   (row norms | scales | theta's planes at the streaming step's own offsets, then 3 x 2 x 2048 u64 histograms and the
 *   64-byte select state where the step keeps W's planes).  It is never larger than stein_stream_workspace_bytes(n, d):
 *   one buffer serves stein_stream_median and then stein_svgd_phi_stream, h2_out handed over as h2_in; the step rebuilds
 *   its planes itself.
 * Counts are integers added with 64-bit atomics: the result does not depend on the grid and a repeated call is
 * bit-identical.  Grid: min(tiles, 2 x 256) workgroups, tiles = nt (nt + 1) / 2, nt = ceil(n / 128) (two 512-thread
 * workgroups fit a CU; 256 = the MI355X's CU count, a constant as in stein_stream_plan).
 * stein_stream_median_plan (host arithmetic): byte offsets of the histograms and of the select state inside the
 * workspace (lo and hi are the floats at state_offset + 40 and + 44), the number of tiles and the grid.
 * stein_debug_stream_median_grid(k) (test hook, per calling thread): k > 0 launches exactly k workgroups, 0 restores the
 * rule. */
int stein_stream_median_workspace_bytes(int64_t n, int64_t d, int dtype, int flags, size_t* out_bytes);
int stein_stream_median_plan(int64_t n, int64_t d, size_t* hist_offset, size_t* state_offset, int64_t* tiles, int* blocks);
int stein_stream_median(const void* theta, int64_t n, int64_t d, int dtype,
                        float* h2_out, float* median_out /* may be NULL */,
                        void* workspace, size_t ws_bytes, int flags, void* stream);
int stein_debug_stream_median_grid(int blocks);   /* test hook, per calling thread; 0 = default */

/* ---- streaming step and Stein discrepancy under the inverse multiquadric (IMQ) kernel ------------------------------
 * The SVGD direction with the heavy-tailed kernel
 *   k_ij = (1 + D_ij / c2)^(-1/2),   c2 = 2 h2,   h2 = *h2_in,   D_ij = max(|theta_i - theta_j|^2, 0)
 * in place of the RBF exp(-D_ij / (2 h2)): the same bandwidth (the same h2 tensor, the same median heuristic -- take it
 * with stein_stream_median), the exponent fixed at -1/2.  Under the RBF kernel the Stein discrepancy does not control
 * convergence for d >= 3; under this one it does (Gorham & Mackey 2017), so this is the path for the KERNEL, not a faster
 * one: by instruction count it costs about twice stein_svgd_phi_stream (measured: README.md, profiles/imq_ab.txt).
 * With k3 = k^3, k5 = k^5:  grad_{theta_j} k(theta_j, theta_i) = k3_ij (theta_i - theta_j) / c2, and
 *   n phi_i = (K G)_i + [ rs3_i theta_i - (K3 theta)_i ] / c2,          rs3_i = sum_j k3_ij
 * The gradient is not proportional to the kernel, so no folded operand exists: every 128 x 128 tile of D is turned into
 * two images, k and k3, and contracted with G and with theta at once, then dropped (stein_amd/csrc/stein_imq.hip; the
 * distance tiles are stein_svgd_phi_stream's and stein_stream_median's, value for value).
 *   theta, score, h2_in, phi, sqnorm_out, flags, workspace, stream: exactly as stein_svgd_phi_stream -- fp32 only
 *   (STEIN_BF16: STEIN_E_UNSUPPORTED), flags == 0 (STEIN_E_BADARG), n >= 1, d >= 1 (STEIN_E_SHAPE), h2_in a DEVICE float[1]
 *   read on the device in every call, a 16-byte-aligned workspace (STEIN_E_BADARG) of at least the size below
 *   (STEIN_E_WORKSPACE) whose contents on entry do not matter.  No K_out / dK_out, one rank.
 * stein_svgd_phi_imq_ksd: the step and the Stein discrepancy sums under this kernel at *h2_in.  Stein kernel
 *   u_p(i,j) = k_ij g_i.g_j + k3_ij (g_i - g_j).(theta_i - theta_j) / c2 + d k3_ij / c2 - 3 k5_ij D_ij / c2^2
 * and summed over the pairs, per element e = (i, column), with rd5_i = sum_j k5_ij D_ij:
 *   S      = sum_e g_e (K G)_e + (2 / c2) sum_e g_e [ rs3_i theta_e - (K3 theta)_e ] + sum_i [ d rs3_i / c2 - 3 rd5_i / c2^2 ]
 *   S_diag = sum_e g_e^2 + n d / c2
 *   phi        : [n][d] float, or NULL: the statistic alone (the three sums are the same bits)
 *   sums_out   : DEVICE double[3] = |phi|^2, S, S_diag.  KSD^2_V = S / n^2, KSD^2_U = (S - S_diag) / (n (n - 1)).
 *   phi and sums_out[0] are stein_svgd_phi_imq's to the bit.
 * Sizes, N = roundup(n, 128), dk = roundup(d, 32), dc = roundup(d, 128), every term rounded up to 256 bytes:
 *   stein_imq_workspace_bytes = 4 N + 4 (6 dc + 4) + 6 N dk + 2 x 6 N dc + 2 x 4 jsplit n d + 4 jsplit n + 8 min(1024, ceil(n d / 1024))
 *   (row norms | scales | theta's planes | theta^T's planes | G^T's planes | partial K.G | partial K3.theta | partial rs3 |
 *   |phi|^2 block partials); never smaller than stein_stream_median_workspace_bytes, so one buffer serves the median call
 *   and then the step.
 *   stein_imq_ksd_workspace_bytes = stein_imq_workspace_bytes + 4 jsplit n + 16 min(1024, ceil(n d / 1024)) (partial rd5 | the
 *   S and S_diag block partials), appended: no offset of the plain layout moves.
 * stein_imq_plan (host arithmetic): row_tiles = ceil(n / 128), col_blocks = ceil(d / 128) and
 * jsplit = clamp(floor(256 / (row_tiles col_blocks)), 1, row_tiles) with empty tails dropped: one workgroup per (row tile,
 * 128-column block, j range), stein_stream_plan's rule.  The ranges' partial sums are added in range order, no float atomics:
 * a repeated call is bit-identical.  stein_debug_stream_jsplit applies to this plan too. */
int stein_imq_workspace_bytes(int64_t n, int64_t d, int dtype, int flags, size_t* out_bytes);
int stein_imq_ksd_workspace_bytes(int64_t n, int64_t d, int dtype, int flags, size_t* out_bytes);
int stein_imq_plan(int64_t n, int64_t d, int* row_tiles, int* col_blocks, int* jsplit);
int stein_svgd_phi_imq(const void* theta, const void* score, int64_t n, int64_t d, int dtype,
                       const float* h2_in, float* phi, double* sqnorm_out,
                       void* workspace, size_t ws_bytes, int flags, void* stream);
int stein_svgd_phi_imq_ksd(const void* theta, const void* score, int64_t n, int64_t d, int dtype,
                           const float* h2_in, float* phi /* may be NULL */,
                           double* sums_out /* [3]: |phi|^2, S, S_diag */,
                           void* workspace, size_t ws_bytes, int flags, void* stream);

/* ---- Stein thinning: the m particles that best represent all n ------------------------------------------------------
 * Riabiz et al. 2022: greedily, m times and with replacement, pick the particle that most lowers the kernelized Stein
 * discrepancy of the picked set.  The reference has no counterpart (a run's particles are used whole).  With the Stein
 * kernel u_p of the chosen kernel at *h2_in (c2 = 2 h2, D = |x - y|^2, cross = (g_x - g_y).(x - y), gg = g_x.g_y):
 *   STEIN_KERNEL_IMQ  k = (1 + D / c2)^(-1/2):  u_p = k gg + k^3 cross / c2 + d k^3 / c2 - 3 k^5 D / c2^2   (as above)
 *   STEIN_KERNEL_RBF  k = exp(-D / c2):         u_p = k (gg + cross / h2 + d / h2 - D / h2^2)               (STEIN_FLAG_KSD's)
 *   obj_t[j] = u_p(j, j) / 2 + sum_{i < t} u_p(x_{s_i}, x_j),   s_t = argmin_j obj_t[j], the LOWEST index on equal value,
 *   S_t = S_{t-1} + 2 obj_t[s_t]  (t = 1 .. m; an index may repeat, so m > n is meaningful)
 *   theta, score : [n][d] float (STEIN_F32; STEIN_BF16 / STEIN_F64 return STEIN_E_UNSUPPORTED)
 *   h2_in        : DEVICE float[1], bandwidth^2, read on the device (take the median heuristic's with stein_stream_median)
 *   idx_out      : DEVICE int64[m], the picks in order
 *   ksd2_out     : DEVICE double[m] or NULL: KSD^2_V of the first t picks, S_t / t^2; idx_out is the same bits without it
 *   flags        : must be 0 (STEIN_E_BADARG).  n >= 1, d >= 1, 1 <= m <= 2^30 (STEIN_E_SHAPE); an unknown kernel id: STEIN_E_BADARG
 * One kernel (k_thin_step, stein_amd/csrc/stein_thin.hip), launched m + 1 times on `stream`: per pick ONE row of the n x n
 * Stein-kernel matrix, that of an index only the device knows, from the differences x_s - x_j, g_s - g_j in fp32 and added
 * to the objective in fp64; theta and the score are read once per pick (8 n d bytes), the matrix is never formed.  No host
 * read, no allocation, no workgroup waits for another (the launch boundary is the barrier), no atomics: a repeated call
 * is bit-identical, for any workspace contents.
 * The workspace must be 16-byte aligned (STEIN_E_BADARG); it carries nothing between calls.  It depends on n alone:
 *   stein_thin_workspace_bytes = 8 n + 2 x 1024 x 16 + 8, every term rounded up to 256 bytes
 *   (the fp64 objective, u_p(j, j) / 2 folded in by launch 0 | two alternating sets of at most 1024 per-workgroup
 *   (value, index) partials | the running S).
 * Grid: min(1024, ceil(n / rows per workgroup)) workgroups of 256 threads; a row is taken by the power-of-two group of
 * lanes that covers its 16-byte units (4-byte units where d % 4 != 0 or a base pointer is not 16-byte aligned).
 * stein_debug_thin_grid(k) (test hook, per calling thread): k > 0 launches min(k, 1024) workgroups, 0 restores the rule;
 * the picks do not depend on it. */
enum { STEIN_KERNEL_RBF = 0, STEIN_KERNEL_IMQ = 1 };
int stein_thin_workspace_bytes(int64_t n, int64_t d, int dtype, int flags, size_t* out_bytes);
int stein_thin(const void* theta, const void* score, int64_t n, int64_t d, int dtype,
               const float* h2_in, int kernel /* STEIN_KERNEL_RBF | STEIN_KERNEL_IMQ */, int64_t m,
               int64_t* idx_out /* DEVICE [m] */, double* ksd2_out /* DEVICE [m], may be NULL */,
               void* workspace, size_t ws_bytes, int flags, void* stream);
int stein_debug_thin_grid(int blocks);   /* test hook, per calling thread; 0 = default */

/* ---- KSD goodness-of-fit test: the bootstrap's quadratic forms without the n x n matrix -----------------------------
 * Chwialkowski et al. 2016, Liu et al. 2016 (Gorham & Mackey 2017 for the IMQ kernel): the V-statistic sum_ij u_p(x_i, x_j)
 * is judged against replicates sum_ij w_bi w_bj u_p(x_i, x_j) under random weights.  The reference has no counterpart.
 *   q_out[b] = sum_ij weights[b][i] weights[b][j] u_p(x_i, x_j),  b = 0 .. reps - 1   (u_p as in stein_thin, at *h2_in)
 *   diag_out = sum_i u_p(x_i, x_i) = sum_i |g_i|^2 + n d / h2 (RBF) or n d / (2 h2) (IMQ), in fp64 from the rows; may be NULL
 *   theta, score : [n][d] float (STEIN_F32; STEIN_BF16 / STEIN_F64 return STEIN_E_UNSUPPORTED)
 *   h2_in        : DEVICE float[1], bandwidth^2, read on the device
 *   weights      : DEVICE float[reps][n], row-major, any finite values (signs, centred multinomial counts, a row of ones
 *                  for the statistic itself)
 *   q_out        : DEVICE double[reps];  diag_out : DEVICE double[1] or NULL
 *   flags        : must be 0 (STEIN_E_BADARG).  n >= 2, d >= 1, reps >= 1, n <= 2^24 (STEIN_E_SHAPE); an unknown kernel id:
 *                  STEIN_E_BADARG
 * The Stein-kernel matrix is formed one 128 x 128 tile at a time from three (RBF: two) Gram products on the matrix cores
 * (fp16 hi + lo operands, fp32 accumulation), scaled by a power of two derived on the device from a bound on |u_p|, split
 * into hi + lo fp16 and contracted with all replicates' weights at once (k_ksd_boot, stein_amd/csrc/stein_boot.hip); the
 * weights are split at ONE power-of-two scale for the whole matrix.  No host read, no allocation, no atomics, no workgroup
 * waits for another: a repeated call is bit-identical, for any workspace contents; negating a row of weights leaves its
 * q_out bits unchanged (by construction: the matrix cores' sums are not sign-symmetric, so each row is contracted in the
 * sign that makes its first nonzero entry positive), and so does its position among the rows.
 * Non-finite inputs.  The host never reads theta, score or h2_in and cannot validate them, and a finite number for a sample
 * that contains a NaN would pass for a statistic, so: a NaN or an infinity ANYWHERE in theta or score, or h2 = 0 or NaN,
 * makes EVERY q_out[b] and diag_out NaN, and the call returns STEIN_OK (as the weighted predictive calls do).  So does a
 * row whose |x_i|^2, |g_i|^2, g_i.x_i or (RBF) |g_i - x_i / h2|^2 overflows fp32: these per-row sums are what the device looks
 * at (k_boot_scale), once per call and outside the j loop.  Non-finite weights are the caller's.  (A caller that counts
 * replicates >= the statistic must treat a NaN statistic itself: stein_goodness_of_fit returns a NaN p-value.)
 * The workspace must be 16-byte aligned (STEIN_E_BADARG); it carries nothing between calls.  With R = n rounded up to 128,
 * dk = d rounded up to 32, dc = d rounded up to 128, C = reps rounded up to 128 and P = reps rounded up to 32,
 *   stein_ksd_boot_workspace_bytes = 4 R + 4 (6 dc + 4) + 6 R dk + 4 n d + 4 (6 dc + 4) + 6 R dk + 4 (6 R + 4) + 6 C R
 *                                    + 4 R + 4 R + 8 R + 256 + 4 jsplit row_tiles P + 4 reps n,   every term rounded up to 256 bytes
 *   (row norms | theta's scales | theta's planes | W = G - theta / h2 (RBF) | the score-side operand's scales | its planes |
 *   the weights' scales | their planes | b_i | |m_i|^2 | |g_i|^2 (fp64) | the image's scales | the partial sums | every row of
 *   weights times the sign of its first nonzero entry: what is contracted, so that w and -w are one operand).
 * stein_ksd_boot_plan: the grid, row_tiles = ceil(n / 128) x col_groups = ceil(reps / 256) x jsplit ranges of 128-column
 * j tiles, jsplit = min(row_tiles, max(1, floor(256 / (row_tiles col_groups)))) with empty tails dropped (the streaming
 * step's rule).  stein_debug_boot_jsplit(k) (test hook, per calling thread): k > 0 asks for k ranges, 0 restores the rule;
 * it changes the workspace size with the plan. */
int stein_ksd_boot_workspace_bytes(int64_t n, int64_t d, int64_t reps, int dtype, int flags, size_t* out_bytes);
int stein_ksd_boot_plan(int64_t n, int64_t d, int64_t reps, int* row_tiles, int* col_groups, int* jsplit);
int stein_ksd_boot(const void* theta, const void* score, int64_t n, int64_t d, int dtype, const float* h2_in, int kernel,
                   const float* weights /* [reps][n], row-major */, int64_t reps,
                   double* q_out /* [reps] */, double* diag_out /* 1, may be NULL */,
                   void* workspace, size_t ws_bytes, int flags, void* stream);
int stein_debug_boot_jsplit(int jsplit);   /* test hook, per calling thread; 0 = default */

/* ---- Stein-kernel products: V U without the n x n matrix ------------------------------------------------------------
 * What stein_ksd_boot forms per workgroup and reduces away, stored: the products Stein importance weights (below) and
 * control variates are built from.  The reference has no counterpart.
 *   out[b][i] = sum_j u_p(x_i, x_j) V[b][j],  b = 0 .. reps - 1, i = 0 .. n - 1   (u_p as in stein_thin, at *h2_in)
 *   theta, score, h2_in, kernel : as stein_ksd_boot
 *   V   : DEVICE float[reps][n], row-major, any finite values;  out : DEVICE float[reps][n]
 *   flags must be 0 (STEIN_E_BADARG).  n >= 2, d >= 1, reps >= 1, n <= 2^24 (STEIN_E_SHAPE); fp32 only (STEIN_E_UNSUPPORTED)
 * The kernel is k_ksd_boot's j loop with a second tail (k_ksd_boot<Kern, true>, stein_amd/csrc/stein_boot.hip): the 128 x 32
 * accumulators of a wave are not multiplied by w_bi and reduced over the rows but stored as this j range's partial of
 * T = U V^T, one float per (j range, replicate, row < n), four consecutive rows of a lane as one 16-byte store;
 * k_boot_product_sum adds the ranges in range order in fp64, applies the out-scale and writes floats.  The plan and its test
 * hook are the bootstrap's (stein_ksd_boot_plan, stein_debug_boot_jsplit).  Every slot is written by exactly one wave, no
 * atomics: a repeated call is bit-identical, for any workspace contents; rows >= n and replicates >= reps are never written.
 * V is split as given: the sign canonicalisation of the quadratic forms is not needed here and NOT promised -- out(-V) may
 * differ from -out(V) in the last bit of a partial.
 * Non-finite inputs: as stein_ksd_boot -- a NaN or an infinity anywhere in theta or score (or a per-row sum that overflows
 * fp32), or h2 = 0 or NaN, makes every out[b][i] NaN, and the call returns STEIN_OK; nothing outside out is written.
 * The workspace must be 16-byte aligned (STEIN_E_BADARG); it carries nothing between calls.  With R, dk, dc, C, P as above it
 * is the bootstrap's layout with the partial block holding T's partials and without the canonical weights:
 *   stein_ksd_matmul_workspace_bytes = 4 R + 4 (6 dc + 4) + 6 R dk + 4 n d + 4 (6 dc + 4) + 6 R dk + 4 (6 R + 4) + 6 C R
 *                                      + 4 R + 4 R + 8 R + 256 + 4 jsplit P R,   every term rounded up to 256 bytes. */
int stein_ksd_matmul_workspace_bytes(int64_t n, int64_t d, int64_t reps, int dtype, int flags, size_t* out_bytes);
int stein_ksd_matmul(const void* theta, const void* score, int64_t n, int64_t d, int dtype,
                     const float* h2_in, int kernel,
                     const float* V /* DEVICE [reps][n] */, int64_t reps,
                     float* out /* DEVICE [reps][n] */,
                     void* workspace, size_t ws_bytes, int flags, void* stream);

/* ---- Stein importance weights ----------------------------------------------------------------------------------------
 * Black-box importance sampling (Liu & Lee 2017): the weights w on the simplex that minimise w^T U w, the KSD^2 of the
 * weighted sample; sum_i w_i f(x_i) then corrects a biased or unconverged sample (SVGD particles stopped early, MCMC
 * output, a warm start from another posterior) while keeping every particle.  The reference has no counterpart.
 * Frank-Wolfe on the simplex with an exact line search, from w = 1 / n and g = U w; for t = 1 .. iters
 *   f = sum_j w_j g_j,  s = argmin_j g_j (lowest index on equal value),  num = f - g_s,  den = f - 2 g_s + u_p(s, s)
 *   gamma = 0 if num <= 0 or den <= 0, else min(1, num / den);   w <- (1 - gamma) w + gamma e_s,  g <- (1 - gamma) g + gamma U[s, :]
 * f never increases, and f(w) - min over the simplex <= 2 (w^T g - min g): the certificate in stats_out[1].
 *   w_out     : DEVICE double[n], >= 0, sum 1
 *   stats_out : DEVICE double[3]: f(w) = w^T U w, gap = w^T g - min_i g_i (g = U w), f(uniform)
 *   idx_out   : DEVICE int64[iters] or NULL: the vertex s of every step;  gamma_out : DEVICE double[iters] or NULL: its length
 *   iters     : 0 .. 2^30 (STEIN_E_SHAPE); 0 returns the uniform weights, their gap and f(uniform) = f(w)
 *   flags must be 0 (STEIN_E_BADARG).  n >= 2, d >= 1, n <= 2^24 (STEIN_E_SHAPE); fp32 only (STEIN_E_UNSUPPORTED)
 * Launches (stein_amd/csrc/stein_weights.hip), no host read, no allocation: stein_ksd_matmul of the float row 1 / n -> g;
 * k_weights_step iters + 1 times -- per step ONE row of U, that of an index only the device knows, in fp32 from the
 * differences as stein_thin evaluates it (the device code is shared), g and w updated in fp64, u_p(s, s) summed in fp64;
 * then stein_ksd_matmul of the final weights (as floats) and a one-workgroup finish that takes stats_out[0 .. 1] from that
 * FRESH product: the certificate does not inherit the iteration's drift.  The launch boundary is the only barrier between
 * workgroups, no atomics; the per-workgroup partials (min g, index, sum w_j g_j) belong to min(1024, row batches) virtual
 * workgroups fixed by n and d, so a repeated call is bit-identical, for any workspace contents and any grid.
 * The workspace must be 16-byte aligned (STEIN_E_BADARG); it carries nothing between calls and is O(n d):
 *   stein_weights_workspace_bytes = stein_ksd_matmul_workspace_bytes(n, d, 1) + 8 n + 8 n + 4 n + 4 n + 2 x 1024 x 24,
 *   every term rounded up to 256 bytes   (the products' workspace | g | w (fp64) | w as floats | U w as floats | two
 *   alternating sets of partials); it follows stein_debug_boot_jsplit through its first term.
 * stein_debug_weights_grid(k) (test hook, per calling thread): k > 0 launches min(k, 1024) workgroups, 0 restores one per
 * virtual workgroup; no bit of the result depends on it. */
int stein_weights_workspace_bytes(int64_t n, int64_t d, int dtype, int flags, size_t* out_bytes);
int stein_weights(const void* theta, const void* score, int64_t n, int64_t d, int dtype,
                  const float* h2_in, int kernel, int64_t iters,
                  double* w_out     /* DEVICE [n] */,
                  double* stats_out /* DEVICE [3]: f(w) = w^T U w, gap = w^T g - min_i g_i (g = U w), f(uniform) */,
                  int64_t* idx_out  /* DEVICE [iters] or NULL: the vertex of every step */,
                  double* gamma_out /* DEVICE [iters] or NULL: the step length of every step */,
                  void* workspace, size_t ws_bytes, int flags, void* stream);
int stein_debug_weights_grid(int blocks);   /* test hook, per calling thread; 0 = default */

/* ---- staged path (tests, multi-rank: the host puts collectives between the stages) ------------ */

/* r_i = sum_k theta_ik^2            abstract_kernel.py:34 */
int stein_rownorms(const void* theta_all, int64_t n, int64_t d, int dtype, float* r_out, void* stream);

/* D[i][j] = r_i + r_j - 2 <theta_i, theta_j>, rows row0..row0+n_local, all n columns.
 * abstract_kernel.py:35.  dist_out is the tile-major distance image of leading dimension
 * ld_dist (>= n, multiple of 64; take it from stein_workspace_layout), rows padded to a multiple of 128.
 * hist_level0: optional (NULL to skip) pointer to the level-0 histogram int64[2][2048] (zeroed by
 * stein_median_begin): the kernel adds the level-0 counts of the entries it produces, which replaces
 * stein_median_hist_pass(level 0).  flags: 0 or STEIN_STAGE_SYMMETRIC. */
int stein_distance_block(const void* theta_all, const float* r_all, int64_t n, int64_t d,
                         int64_t row0, int64_t n_local, int dtype,
                         float* dist_out, int64_t ld_dist, void* hist_level0, const void* x3_planes, int flags,
                         void* stream);

/* Speculative median window, staged form for several ranks (stein_svgd_phi does the same inside one call; the state
 * and the idea are described there).  Every rank keeps its own SELECT and SPEC sections; they stay identical because
 * every rank sees the same medians.  Per step, on every rank:
 *   stein_spec_begin            instead of stein_median_begin: zeroes the histograms, sets the ranks and this step's window
 *   stein_distance_block_spec   stein_distance_block that also counts the weight below the window and collects the
 *                               entries inside it (and then does NOT fill hist_level0: state word `skip_l0` = 0)
 *   stein_spec_tally            entries -> table of SPEC table words (uint64): [0] weight below, [1] != 0: invalid,
 *                               [8 + k] weight of the k-th key of the window; the table is 65544 uint64 starting
 *                               2^21 uint64 into the SPEC section
 *   all-reduce(sum) of the table over the ranks (host)
 *   stein_spec_pick             both median targets from the summed table: sets h2 / median and the state word `hit`;
 *                               when `hit` stays 0 (read it back: uint32 at select_state + 64 + 28, `skip_l0` at + 52)
 *                               run the radix-select calls: stein_median_hist_pass(level 0) if skip_l0 == 0, then
 *                               all-reduce / stein_median_resolve / levels 1, 2 as usual
 *   stein_spec_update           after the median is final either way: predict the next step's window */
int stein_spec_begin(void* hist, void* select_state, void* spec_buf, int64_t total, void* stream);
int stein_distance_block_spec(const void* theta_all, const float* r_all, int64_t n, int64_t d,
                              int64_t row0, int64_t n_local, int dtype,
                              float* dist_out, int64_t ld_dist, void* hist_level0, const void* x3_planes, int flags,
                              void* select_state, void* spec_buf, void* stream);
int stein_spec_tally(void* select_state, void* spec_buf, void* stream);
int stein_spec_pick(void* select_state, void* spec_buf, int64_t n, float* h2_out, float* median_out, void* stream);
int stein_spec_update(void* select_state, void* stream);

/* Split-precision mode (STEIN_FLAG_X3), staged form: fills the PLANES section (x3_planes = workspace +
 * offsets[STEIN_WS_PLANES], planes_bytes = total - offsets[STEIN_WS_PLANES]) with the power-of-two scales and the
 * 16-bit terms (see STEIN_FLAG_X3) of every entry of theta (row-major and transposed) and of the score (transposed).
 * Passing the same pointer as `x3_planes` to stein_distance_block / stein_contract_partial / stein_kernel_contract
 * selects the 16-bit-MFMA kernels there; NULL selects the fp32-MFMA kernels.
 * dtype = STEIN_BF16 (BASELINE config 2): theta_all / score_all hold bf16 values; they are the single operand plane,
 * K is rounded to bf16 once (its rowsum uses the rounded values), every product is one bf16 MFMA with fp32
 * accumulation.  bf16 inputs always need STEIN_FLAG_X3 / the planes.
 * Either matrix may be NULL: then only the other one's scales and planes are rebuilt (theta before the distance pass,
 * the score any time before the contraction -- e.g. while its all-gather overlaps the distance pass). */
int stein_x3_prepare(const void* theta_all, const void* score_all, int64_t n, int64_t d, int dtype, void* x3_planes,
                     size_t planes_bytes, void* stream);

/* Exact median of all n*n distances by 3-level radix select on the fp32 bit pattern.
 * compute_median.py:4-16 (tf.nn.top_k of n^2//2+1 values; even count -> mean of the two middle).
 *   begin   : zero the histograms, set the two target ranks for `total` values in all
 *             (the path uses total = n*n; even -> ranks total/2-1 and total/2)
 *   hist    : add this rank's row block to level `level`'s histogram
 *   resolve : pick the digit holding each target rank (run after the histograms of all ranks
 *             have been summed); at the last level writes median and h2 = sqrt(med/ln n)^2
 *             (abstract_kernel.py:40, squared_exponential_kernel.py:22) into the select state
 *             and to h2_out.
 */
int stein_median_begin(void* hist, void* select_state, int64_t total, void* stream);
int stein_median_hist_pass(const float* dist, int64_t ld_dist, int64_t n_local, int64_t n, int level,
                           const void* select_state, void* hist, int flags, void* stream);
int stein_median_resolve(const void* hist, int level, int64_t n, void* select_state,
                         float* h2_out, float* median_out, void* stream);

/* K = exp(-D / h2 / 2)               squared_exponential_kernel.py:22 (optional output) */
int stein_kernel_matrix(const float* dist, int64_t ld_dist, int64_t n_local, int64_t n,
                        const float* h2_dev, float* K_out, int64_t ld_K, int dist_flags /* 0 or STEIN_STAGE_UPPER */,
                        void* stream);

/* phi rows of this rank:  (K.G + (rowsum(K) theta - K.theta)/h2) / n
 * squared_exponential_kernel.py:23,32 (dK) and abstract_stein_sampler.py:105 (phi).
 * Fused exp + fp32-MFMA contraction over the materialised distance block, then a finish pass. */
int stein_kernel_contract(const float* dist, int64_t ld_dist, const void* theta_all, const void* score_all,
                          int64_t n, int64_t d, int64_t row0, int64_t n_local, int dtype,
                          const float* h2_dev, float* phi_local, double* sqnorm_out, float* dK_out,
                          const void* x3_planes, void* workspace, size_t ws_bytes, int dist_flags /* 0 or STEIN_STAGE_UPPER */,
                          void* stream);

/* The two halves of stein_kernel_contract, exposed so a harness can time the MFMA kernel on its own:
 *   partial : k_phi_partial only (fills the PART_G / PART_T / PART_RS workspace sections)
 *   finish  : sums the split partials, forms phi (and dK), reduces |phi|^2 */
int stein_contract_partial(const float* dist, int64_t ld_dist, const void* theta_all, const void* score_all,
                           int64_t n, int64_t d, int64_t row0, int64_t n_local, int dtype,
                           const float* h2_dev, const void* x3_planes, void* workspace, size_t ws_bytes,
                           int dist_flags /* 0 or STEIN_STAGE_UPPER */, void* stream);
int stein_contract_finish(const void* theta_all, int64_t n, int64_t d, int64_t row0, int64_t n_local, int dtype,
                          const float* h2_dev, float* phi_local, double* sqnorm_out, float* dK_out,
                          void* workspace, size_t ws_bytes, int flags /* same STEIN_FLAG_* as the partial */,
                          void* stream);

/* ---- rank-step segments (row-sharded runs) ------------------------------------------------------------------------
 * What one rank does between two collectives, one call each: the staged calls above chained on `stream`, so that the
 * host layer issues per step only  all-gather(theta), all-gather(score) | stein_rank_begin | all-reduce | stein_rank_pick
 * (window form) or stein_rank_radix x3 with an all-reduce before each (radix form) | stein_rank_finish |
 * all-reduce(|phi|^2).  `workspace` is sized by stein_workspace_bytes(n_local, n, d, dtype, flags | STEIN_FLAG_TILED);
 * flags: STEIN_FLAG_X3, for the window form STEIN_FLAG_RANK_WINDOW, and STEIN_FLAG_KSD (every segment alike;
 * stein_rank_finish then writes double[3] to sqnorm_out: all-reduce all three).  They replace, for rank p's rows, the same
 * reference lines as stein_svgd_phi.
 *   stein_rank_begin   row norms, theta's operand planes, median set-up, the [n_local, n] distance block (level-0
 *                      histogram or window counting in its epilogue) and, window form, the tally.  Then all-reduce(sum)
 *                      the window table (65544 uint64 at 2^21 uint64 into the SPEC section) or histogram level 0.
 *   stein_rank_pick    window form: both median targets from the summed table -> h2 / median; copies the 28 bytes of
 *                      window state from `hit` to `skip_l0` (uint32 [0] = hit, [6] = skip_l0) to flags_host -- page-locked
 *                      host memory -- on the stream: wait for it (an event) and, if hit == 0, run the radix form:
 *                      stein_rank_radix(0, need_pass = !skip_l0) then all-reduce level 0, stein_rank_radix(0, 0) ...
 *   stein_rank_radix   need_pass = 1: add the local block's histogram of `level`.  need_pass = 0 (hist[level] has been
 *                      summed over the ranks): resolve `level` and, below the last level, take the local histogram of
 *                      level + 1 (all-reduce it, call again).  After level 2: h2 / median are final.
 *   stein_rank_finish  window form: predictor update; then the contraction on the local rows -> phi_local, the local part
 *                      of |phi|^2 (all-reduce it), optional dK.  The score's operand planes must have been built
 *                      (stein_x3_prepare(NULL, score_all, ...), any time after the score rows have arrived). */
int stein_rank_begin(const void* theta_all, int64_t n, int64_t d, int64_t row0, int64_t n_local, int dtype,
                     void* workspace, size_t ws_bytes, int flags, void* stream);
int stein_rank_pick(int64_t n, int64_t d, int64_t row0, int64_t n_local, int dtype, void* workspace, size_t ws_bytes,
                    int flags, float* h2_out, float* median_out, void* flags_host, void* stream);
int stein_rank_radix(int level, int need_pass, int64_t n, int64_t d, int64_t row0, int64_t n_local, int dtype,
                     void* workspace, size_t ws_bytes, int flags, float* h2_out, float* median_out, void* stream);
int stein_rank_finish(const void* theta_all, const void* score_all, int64_t n, int64_t d, int64_t row0, int64_t n_local,
                      int dtype, const float* h2_dev, float* phi_local, double* sqnorm_out, float* dK_out,
                      void* workspace, size_t ws_bytes, int flags, void* stream);

/* ---- the sharded step with the library's own RCCL communicator ("one communicator per process-rank") ----
 * The reference has no counterpart (stein_sampler.py:11-14 "does not exploit parallelism"); per rank the step replaces
 * the same reference lines as stein_svgd_phi.  RCCL is looked up at run time (the copy already loaded in the process,
 * e.g. PyTorch-ROCm's, else librccl.so.1); without it these calls return STEIN_E_RCCL.
 *   stein_comm_unique_id  one rank makes the 128-byte id; the host layer hands it to every rank (any channel).
 *   stein_comm_init       collective over the nranks processes, on the CURRENT HIP device; blocks until all have joined.
 *   stein_rank_step       one whole step for rank p's rows [p n / nranks, (p + 1) n / nranks), queued on `stream`:
 *                         all-gather(theta rows, score rows) as one group -> stein_rank_begin -> all-reduce of the window
 *                         table -> stein_rank_pick (window form, STEIN_FLAG_RANK_WINDOW; the call waits for the 4-byte hit
 *                         flag and on a miss runs the radix form) or three histogram all-reduces with stein_rank_radix
 *                         (radix form: nothing waits) -> stein_rank_finish -> all-reduce(|phi|^2).
 *                         theta_all / score_all: [n, d] gather targets; h2_out, median_out, sqnorm_out: device scalars,
 *                         identical on every rank afterwards; window_hit_out (may be NULL): 1 / 0, -1 in the radix form.
 *                         flags: STEIN_FLAG_X3, STEIN_FLAG_RANK_WINDOW, STEIN_FLAG_TIMING, STEIN_FLAG_KSD (sqnorm_out
 *                         double[3], all three all-reduced); workspace sized by
 *                         stein_workspace_bytes(n / nranks, n, d, dtype, flags | STEIN_FLAG_TILED). */
#define STEIN_COMM_ID_BYTES 128
int stein_comm_unique_id(void* id_out, size_t id_bytes);
int stein_comm_init(const void* id, size_t id_bytes, int nranks, int rank, void** comm_out);
int stein_comm_info(void* comm, int* nranks_out, int* rank_out);
int stein_comm_destroy(void* comm);
int stein_rank_step(void* comm, const void* theta_local, const void* score_local, void* theta_all, void* score_all,
                    int64_t n, int64_t d, int dtype, float* phi_local, float* h2_out, float* median_out,
                    double* sqnorm_out, float* dK_out, void* workspace, size_t ws_bytes, int flags,
                    int* window_hit_out, void* stream);

/* Stage timing of the fused call (profiling aid; the events belong to the calling thread, like the last-error string:
 * reserve, call and read from one thread).  stein_timing_reserve(calls)
 * creates the HIP events for `calls` fused calls and rewinds the cursor; each stein_svgd_phi call made with
 * STEIN_FLAG_TIMING then records an event at every stage boundary on its stream while reserved slots last.
 * stein_timing_read waits for the recorded events and returns the stage durations in milliseconds,
 * ms_out[call * STEIN_T_NSTAGES + stage]; *calls_out = calls reported (<= max_calls). */
enum {
  STEIN_T_PREPARE = 0,  /* row norms, operand scales and planes, median set-up */
  STEIN_T_DISTANCE = 1, /* distance pass (+ level-0 histogram, speculative window) */
  STEIN_T_MEDIAN = 2,   /* window selection or radix-select passes */
  STEIN_T_CONTRACT = 3, /* K.[G|theta] partial contraction */
  STEIN_T_FINISH = 4,   /* phi, |phi|^2 */
  STEIN_T_NSTAGES = 5
};
int stein_timing_reserve(int calls);
int stein_timing_read(float* ms_out, int max_calls, int* calls_out);

/* ---- optimizer apply ---------------------------------------------------------------------------
 * Fuses the norm clip  phi *= 10 / max(10, |phi|_F)  (abstract_stein_sampler.py:125), the optimizer
 * map and  theta += step  (abstract_stein_sampler.py:126).
 *   sqnorm_dev  : device double[1] holding the GLOBAL |phi|_F^2, or NULL to use clip_scale_host
 *   theta       : [count] of state_dtype, updated in place; may be NULL (state + step_out only:
 *                 this is `gd.update(phi)` on its own)
 *   step_out    : optional [count] of state_dtype, receives the step
 *   state_dtype : STEIN_F32 or STEIN_F64 for theta / optimizer state / step_out; the map is evaluated in that type
 *                 (STEIN_F64 = the reference's NumPy float64 arithmetic)
 *   phi_dtype   : STEIN_F32 (what stein_svgd_phi produces) or, with STEIN_F64 state only, STEIN_F64: `gd.update(phi)`
 *                 on a float64 array then is the reference's pure-fp64 map, phi is not rounded to fp32 first
 * Adagrad: stein/optimizers/adagrad_gradient_descent.py:37-44 (first_step -> hist = phi^2).
 * Adam   : stein/optimizers/adam_gradient_descent.py:45-58 (t = n_iters AFTER increment;
 *          t == 1 -> mu = phi, nu = phi^2); the caller multiplies lr by decay afterwards.
 */
int stein_apply_adagrad(void* theta, const void* phi, int phi_dtype, void* hist, int64_t count, int state_dtype,
                        const double* sqnorm_dev, double clip_scale_host, double clip_threshold,
                        double lr, double alpha, double eps, int first_step,
                        void* step_out, void* stream);
int stein_apply_adam(void* theta, const void* phi, int phi_dtype, void* mu, void* nu, int64_t count, int state_dtype,
                     const double* sqnorm_dev, double clip_scale_host, double clip_threshold,
                     double lr, double beta1, double beta2, double eps, int64_t t,
                     void* step_out, void* stream);

/* ---- score producers (the step before the hot path) ------------------------------
 * d log p / d theta of every particle for the generalised linear models of the reference's examples, in one launch;
 * replaces the n sequential sess.run(grad_log_p) calls of SteinSampler.train_on_batch
 * (stein/samplers/stein_sampler.py:59-68) for these models.
 *   theta [n][d] float   particle i holds the weights w at columns w_col .. w_col + n_feats and, when alpha_col >= 0,
 *                        log(alpha) at column alpha_col; any other column gets score 0
 *   X [batch][n_feats], y [batch] float (device)
 *   STEIN_GLM_LINEAR    examples/linear_regression/main.py:18-31:  log p = -1/2 sum_b (x_b.w - y_b)^2 + log prior
 *   STEIN_GLM_LOGISTIC  examples/logistic_regression/main.py:23-49: log p = scale * sum_b [y_b z_b - softplus(z_b)] + log prior,
 *                       z = X w, scale = n_train / n_batch
 *   prior: alpha_col < 0: w ~ N(0, 1 / prior_precision);  alpha_col >= 0: w ~ N(0, 1 / alpha), alpha ~ Gamma(1, gamma_rate)
 *          evaluated at alpha = exp(theta[alpha_col]) without a Jacobian term, as the reference does
 *   score [n][d] float   d/dw_c = scale * sum_b resid_b x_bc - precision * w_c;  d/dlog alpha = F/2 - alpha (sum w^2 / 2 + rate) */
enum { STEIN_GLM_LINEAR = 0, STEIN_GLM_LOGISTIC = 1 };
int stein_score_glm(const float* theta, int64_t n, int64_t d, int kind, int64_t w_col, int64_t n_feats, int64_t alpha_col,
                    const float* X, const float* y, int64_t batch, double scale, double prior_precision,
                    double gamma_rate, float* score, void* stream);

/* Bayesian neural-network regression with one hidden ReLU layer, examples/regression_neural_network/main.py:29-85:
 *   pred = relu(X w1 + b1) w2 + b2;  log p = [ (n_train / batch) sum_b log N(y_b; pred_b, 1/gamma) + log Gamma(lambda; a, b)
 *   + log Gamma(gamma; a, b) + sum over all weights of log N(.; 0, 1/lambda) ] / n_train, lambda = exp(log_lambda),
 *   gamma = exp(log_gamma), densities evaluated without a Jacobian term, as the reference does.
 *   cols[6]: first column of w1 ([n_in][n_hidden] row-major), b1 [n_hidden], w2 [n_hidden], b2, log_lambda, log_gamma in
 *   the packed particle; any other column gets score 0.  n_in <= 4, n_hidden <= 1024. */
int stein_score_bnn(const float* theta, int64_t n, int64_t d, int64_t n_in, int64_t n_hidden, const int64_t* cols,
                    const float* X, const float* y, int64_t batch, double n_train, double gamma_a, double gamma_b,
                    float* score, void* stream);

/* The same network with up to 128 input features (tabular regression sets: 6 .. 90 inputs): the arguments, the model, the
 * formulas and the output conventions of stein_score_bnn.  Domain: 1 <= n_in <= 128, n_hidden <= 1024 and
 * n_in * n_hidden <= 16384 (a particle's first layer and its gradient, 64 KB each, lie in one workgroup's LDS);
 * STEIN_E_UNSUPPORTED beyond, with a message that names the limit.  The other checks are stein_score_bnn's, in its order.
 * For n_in <= 4 the call runs stein_score_bnn itself: bit-identical.  No workspace, no atomics: a repeated call is
 * bit-identical, and the row of a particle depends on nothing but the particle (not on n, the grid or the other particles). */
int stein_score_bnn_wide(const float* theta, int64_t n, int64_t d, int64_t n_in, int64_t n_hidden, const int64_t* cols,
                         const float* X, const float* y, int64_t batch, double n_train, double gamma_a, double gamma_b,
                         float* score, void* stream);

/* Softmax (multi-class logistic) regression: the first model beyond the reference's three examples.
 *   theta [n][d] float   particle i holds W [n_feats][n_classes] row-major at w_col (W_fc at column w_col + f * n_classes + c:
 *                        how a [F, C] variable flattens) and, when alpha_col >= 0, log(alpha) at alpha_col; any other column
 *                        gets score 0.  No bias term: append a column of ones to X.
 *   X [batch][n_feats] float, labels [batch] int32 class indices (device; never read on the host)
 *   z_bc = sum_f x_bf W_fc;  log p = scale * sum_b [z_{b,y_b} - logsumexp_c z_bc] + sum_fc log N(W_fc; 0, 1/alpha)
 *          + log Gamma(alpha; 1, gamma_rate), the density at alpha = exp(theta[alpha_col]) without a Jacobian term, as
 *          STEIN_GLM_LOGISTIC; alpha_col < 0: alpha = prior_precision
 *   score [n][d] float   d/dW_fc = scale * sum_b x_bf (1[y_b = c] - p_bc) - alpha W_fc, p_b. = softmax(z_b.) evaluated with the
 *                        row maximum subtracted;  d/dlog alpha = F C / 2 - alpha (sum_fc W_fc^2 / 2 + gamma_rate)
 * Domain: 2 <= n_classes <= 32, 1 <= n_feats <= 1024, n_feats * n_classes <= 16384 (a particle's W and its gradient lie in
 * one workgroup's LDS); STEIN_E_UNSUPPORTED beyond, with a message that names the limit.  NULL pointers: STEIN_E_BADARG;
 * weights or the alpha column that do not fit d, or the alpha column inside the weights: STEIN_E_SHAPE (after the domain).
 * A label outside [0, n_classes) is no error code: the call returns STEIN_OK and every weight entry of every particle is
 * NaN (the convention of the weights of the weighted calls below).
 * One launch, no workspace, no atomics: a repeated call is bit-identical, and the row of a particle depends on nothing but
 * the particle (not on n, the grid or the other particles). */
enum { STEIN_SOFTMAX_C_MIN = 2, STEIN_SOFTMAX_C_MAX = 32, STEIN_SOFTMAX_F_MAX = 1024, STEIN_SOFTMAX_FC_MAX = 16384 };
int stein_score_softmax(const float* theta, int64_t n, int64_t d, int64_t w_col, int64_t n_feats, int64_t n_classes,
                        int64_t alpha_col, const float* X, const int32_t* labels, int64_t batch, double scale,
                        double prior_precision, double gamma_rate, float* score, void* stream);
/* test hook, per calling thread: lanes that share a row in the forward phase (a power of two up to 64; the order in which a
 * logit's F terms are summed follows it); 0 restores the rule */
int stein_debug_score_softmax_lanes(int lanes);

/* Network classifier: one hidden ReLU layer with a softmax head -- stein_score_bnn's network with stein_score_softmax's
 * likelihood, prior and scaling.
 *   theta [n][d] float   particle i packs five blocks, cols[5] gives the first column of each, in any order:
 *                        w1 [n_in][n_hidden] row-major (as stein_score_bnn), b1 [n_hidden], w2 [n_hidden][n_classes] row-major
 *                        (how an [H, C] variable flattens), b2 [n_classes], log_lambda (cols[4] < 0: lambda = prior_precision,
 *                        no entry); any other column gets score 0
 *   X [batch][n_in] float, labels [batch] int32 class indices (device; never read on the host)
 *   pre_bh = b1_h + sum_f x_bf w1_fh (f ascending), a_bh = relu(pre_bh);  z_bc = b2_c + sum_h a_bh w2_hc (h ascending),
 *   p_b. = softmax(z_b.) evaluated with the row maximum subtracted
 *   log p = scale * sum_b [z_{b,y_b} - logsumexp_c z_bc] + sum over all P = n_in H + H + H C + C entries of the four blocks of
 *           log N(. ; 0, 1/lambda) + log Gamma(lambda; 1, gamma_rate), the density at lambda = exp(theta[cols[4]]) without a
 *           Jacobian term.  The prior and the scaling are stein_score_softmax's over all four blocks; the division of
 *           everything by n_train that stein_score_bnn inherits from the reference's regression example is not taken over.
 *   score [n][d] float   with r_bc = 1[y_b = c] - p_bc, m_bh = [pre_bh > 0], delta_bh = m_bh sum_c r_bc w2_hc:
 *                        d/db2_c = scale sum_b r_bc - lambda b2_c          d/dw2_hc = scale sum_b a_bh r_bc - lambda w2_hc
 *                        d/db1_h = scale sum_b delta_bh - lambda b1_h      d/dw1_fh = scale sum_b x_bf delta_bh - lambda w1_fh
 *                        d/dlog_lambda = P / 2 - lambda (1/2 sum of squares of the P entries + gamma_rate)
 * Domain: 1 <= n_in <= 128, 2 <= n_classes <= 32, 1 <= n_hidden <= 512 and (n_in + CS) * n_hidden <= 16384 with CS =
 * n_classes rounded up to a multiple of 4 (both layers and their gradients of a particle, 128 KB at most, lie in one
 * workgroup's LDS beside a row block's activations and residuals); STEIN_E_UNSUPPORTED beyond, with a message that names the
 * limit.  Refused before the launch, in this order: NULL pointers (STEIN_E_BADARG); a bad shape (STEIN_E_SHAPE); the domain
 * (STEIN_E_UNSUPPORTED); blocks that do not fit d or overlap (STEIN_E_SHAPE).
 * A label outside [0, n_classes) is no error code: the call returns STEIN_OK and every entry of the four blocks of every
 * particle is NaN.
 * One launch, no workspace, no atomics: the launch plan follows from (n_in, n_hidden, n_classes, batch) alone, a repeated
 * call is bit-identical, and the row of a particle depends on nothing but the particle (not on n, the grid or the others). */
enum { STEIN_BNN_CLASS_NIN_MAX = 128, STEIN_BNN_CLASS_C_MIN = 2, STEIN_BNN_CLASS_C_MAX = 32, STEIN_BNN_CLASS_H_MAX = 512,
       STEIN_BNN_CLASS_W_MAX = 16384 };
int stein_score_bnn_class(const float* theta, int64_t n, int64_t d, int64_t n_in, int64_t n_hidden, int64_t n_classes,
                          const int64_t* cols, const float* X, const int32_t* labels, int64_t batch, double scale,
                          double prior_precision, double gamma_rate, float* score, void* stream);

/* ---- posterior predictive producers (the step after the update) --------------------
 * The forward pass of the same three models for every particle: what the reference's examples hand to function_posterior
 * (stein/samplers/abstract_stein_sampler.py:157-168) and then average.  One call gives any non-empty subset of
 *   pred [n][batch]  f_pb, row-major: the layout function_posterior returns
 *   mean [batch]     1/n sum_p f_pb
 *   var  [batch]     1/n sum_p (f_pb - mean_b)^2                      (np.var's default; 0 for n = 1)
 *   lpd  [batch]     log(1/n sum_p exp(l_pb)), the log predictive density of y_b; needs y
 * and the summaries never materialise [n][batch].  An output passed as NULL is not computed and nothing is written for it.
 *   z_pb = x_b . w_p (GLM) or the network output relu(X w1 + b1) w2 + b2;  f_pb = z_pb with STEIN_PRED_LINK (logits,
 *   regression mean, network output); with STEIN_PRED_MEAN f_pb = sigmoid(z_pb) for STEIN_GLM_LOGISTIC and z_pb otherwise.
 *   l_pb: linear    1/2 log tau - 1/2 tau (y_b - z_pb)^2 - 1/2 log 2 pi, tau = noise_precision (read only for this)
 *         logistic  y_b z_pb - softplus(z_pb)
 *         network   1/2 lg_p - 1/2 exp(lg_p) (y_b - z_pb)^2 - 1/2 log 2 pi, lg_p = the particle's log_gamma column
 * theta, X, y, cols as for the score producers (the same limits: n_feats <= 1024, n_in <= 4, n_hidden <= 1024:
 * STEIN_E_UNSUPPORTED); columns outside the model are not read.  n and batch are at most 2^30 each (STEIN_E_SHAPE beyond).
 * Workspace: a call that asks for mean, var or lpd needs stein_predict_workspace_bytes(n, batch) bytes: 20 bytes per row
 * and particle slice, at most 20 * min(1024 * batch, 2^19 + batch); independent of d; STEIN_E_WORKSPACE without it.  It may
 * hold anything on entry and carries nothing from call to call.  A call that only asks for pred needs none (NULL, 0).
 * Deterministic: no atomics; the particle slices are merged in slice order, so a repeated call is bit-identical.
 * Refused before any launch: all four outputs NULL, lpd without y, an unknown kind / output (STEIN_E_BADARG); columns that
 * do not fit or overlap (STEIN_E_SHAPE). */
enum { STEIN_PRED_LINK = 0, STEIN_PRED_MEAN = 1 };
int stein_predict_workspace_bytes(int64_t n, int64_t batch, size_t* out_bytes);
int stein_predict_glm(const float* theta, int64_t n, int64_t d, int kind, int output, int64_t w_col, int64_t n_feats,
                      const float* X, const float* y, int64_t batch, double noise_precision,
                      float* pred, float* mean, float* var, float* lpd,
                      void* workspace, size_t ws_bytes, void* stream);
int stein_predict_bnn(const float* theta, int64_t n, int64_t d, int64_t n_in, int64_t n_hidden, const int64_t* cols,
                      int output, const float* X, const float* y, int64_t batch,
                      float* pred, float* mean, float* var, float* lpd, void* workspace, size_t ws_bytes, void* stream);

/* Weighted summaries: the same producers under per-particle weights -- Stein importance weights (stein_weights), or the
 * counts of a thinned multiset (torch.bincount of stein_thin's indices).  weights [n]: fp64 device data, w_p >= 0, their
 * sum W > 0; they need not sum to 1.
 *   mean_b = sum_p w_p f_pb / W      var_b = sum_p w_p (f_pb - mean_b)^2 / W      lpd_b = log(sum_p w_p exp(l_pb) / W)
 *   ess [1] (fp64, device) = W^2 / sum_p w_p^2, the effective sample size of the weights
 * with f_pb and l_pb those of the unweighted calls.  pred does not depend on the weights: it is bit for bit the unweighted
 * call's and is written for every particle.  A particle of weight zero is skipped: its outputs enter no summary, even when
 * they are not finite.  The lanes hold fl32(w_p / W), the quotient taken in fp64, so a power-of-two rescaling of the
 * weights changes no bit of any output while the sums stay in fp64's normal range; a weight below 2^-126 W counts as zero.
 * The host never reads the weights: if one is negative or not finite, or W is 0 or overflows, the call returns STEIN_OK
 * and every requested summary row and ess are NaN.
 * Refusals and their order are those of the unweighted calls, with weights == NULL among the NULL pointers
 * (STEIN_E_BADARG) and ess counting as a requested output and as a summary: a call that asks for mean, var, lpd or ess
 * needs stein_predict_weighted_workspace_bytes(n, batch) bytes, 8-byte aligned -- the unweighted size plus 24 bytes per
 * particle slice and 16 more for the sums of the weights; monotone in both arguments, independent of d.  It may hold
 * anything on entry.  Deterministic: no atomics, the weights and the slices are summed in a fixed order. */
int stein_predict_weighted_workspace_bytes(int64_t n, int64_t batch, size_t* out_bytes);
int stein_predict_glm_weighted(const float* theta, int64_t n, int64_t d, int kind, int output, int64_t w_col,
                               int64_t n_feats, const float* X, const float* y, int64_t batch, double noise_precision,
                               const double* weights, float* pred, float* mean, float* var, float* lpd, double* ess,
                               void* workspace, size_t ws_bytes, void* stream);
int stein_predict_bnn_weighted(const float* theta, int64_t n, int64_t d, int64_t n_in, int64_t n_hidden,
                               const int64_t* cols, int output, const float* X, const float* y, int64_t batch,
                               const double* weights, float* pred, float* mean, float* var, float* lpd, double* ess,
                               void* workspace, size_t ws_bytes, void* stream);

/* The network with up to 128 input features: stein_predict_bnn / stein_predict_bnn_weighted with the domain of
 * stein_score_bnn_wide (1 <= n_in <= 128, n_hidden <= 1024, n_in * n_hidden <= 16384; STEIN_E_UNSUPPORTED beyond, naming the
 * limit).  Arguments, outputs, checks and their order, workspace (stein_predict_workspace_bytes /
 * stein_predict_weighted_workspace_bytes, unchanged), determinism and the conventions of the weights are the narrow calls'.
 * For n_in <= 4 the calls run the narrow calls themselves: bit-identical.  pred[p][b] depends on the particle and the row
 * alone (not on n, the slicing or the other rows), and mean, var and lpd are summaries of exactly the values pred holds.
 * Not built for n_in > 4: the order statistics and the y calls below. */
int stein_predict_bnn_wide(const float* theta, int64_t n, int64_t d, int64_t n_in, int64_t n_hidden, const int64_t* cols,
                           int output, const float* X, const float* y, int64_t batch,
                           float* pred, float* mean, float* var, float* lpd, void* workspace, size_t ws_bytes, void* stream);
int stein_predict_bnn_wide_weighted(const float* theta, int64_t n, int64_t d, int64_t n_in, int64_t n_hidden,
                                    const int64_t* cols, int output, const float* X, const float* y, int64_t batch,
                                    const double* weights, float* pred, float* mean, float* var, float* lpd, double* ess,
                                    void* workspace, size_t ws_bytes, void* stream);

/* Softmax regression (the model, theta, X, labels and the domain of stein_score_softmax; the alpha column is not read): the
 * class probabilities of every particle and their per-test-point summaries.  One call gives any non-empty subset of
 *   pred  [n][batch][n_classes]  STEIN_PRED_MEAN: p_pbc = softmax_c(z_pb.);  STEIN_PRED_LINK: the logits z_pbc
 *   prob  [batch][n_classes]     1/n sum_p p_pbc, the posterior predictive class probabilities
 *   lpd   [batch]                log(1/n sum_p p_{pb,y_b}); needs labels
 *   ent   [batch]                1/n sum_p H(p_pb.), the expected entropy, H = logsumexp(z) - sum_c p_c z_c; the mutual
 *                                information between the label and the particle is H(prob_b.) - ent_b
 *   label [batch] int32          argmax_c prob_bc, ties to the lowest class, taken of the very floats prob receives
 * and the summaries never materialise [n][batch][n_classes]; an output passed as NULL is not computed.  The summaries are
 * of the probabilities whatever `output` says.  A label outside [0, n_classes) is no error code: the call returns STEIN_OK
 * and that row's lpd is NaN, nothing else.  pred[p][b][.] depends on the particle and the row alone.
 * Workspace: a call that asks for prob, lpd, ent or label needs stein_predict_softmax_workspace_bytes(n, batch, n_classes)
 * bytes: 4 (n_classes + 2) per row and particle slice -- the slices are those of stein_predict_glm, so at most
 * 4 (n_classes + 2) * min(1024 * batch, 2^19 + batch); the slice count is not cut further, which is 71 MB + 136 bytes a
 * row at 32 classes and far less at the usual counts.  Monotone in n and batch, independent of d; it may hold anything on
 * entry.  STEIN_E_WORKSPACE without it; a call that only asks for pred needs none (NULL, 0).
 * Deterministic: no atomics; the slices are summed in slice order in fp64, so a repeated call is bit-identical.
 * Refused before any launch, in this order: theta or X NULL, all five outputs NULL, lpd without labels, an unknown output
 * (STEIN_E_BADARG); a bad shape (STEIN_E_SHAPE); the domain (STEIN_E_UNSUPPORTED, naming the limit); weights that do not
 * fit d (STEIN_E_SHAPE); the workspace (STEIN_E_WORKSPACE). */
int stein_predict_softmax_workspace_bytes(int64_t n, int64_t batch, int64_t n_classes, size_t* out_bytes);
int stein_predict_softmax(const float* theta, int64_t n, int64_t d, int output, int64_t w_col, int64_t n_feats,
                          int64_t n_classes, const float* X, const int32_t* labels, int64_t batch,
                          float* pred, float* prob, float* lpd, float* ent, int32_t* label,
                          void* workspace, size_t ws_bytes, void* stream);

/* Network classifier (the model, theta, cols, X, labels and the domain of stein_score_bnn_class; cols[4], the log_lambda
 * column, is not read): the outputs, their meaning and the workspace rule are exactly stein_predict_softmax's, with
 *   z_pbc = b2_pc + sum_h relu(b1_ph + sum_f x_bf w1_pfh) w2_phc   (f ascending, then h ascending)
 * pred [n][batch][n_classes] (probabilities with STEIN_PRED_MEAN, logits with STEIN_PRED_LINK), prob [batch][n_classes],
 * lpd [batch], ent [batch], label [batch] int32 (the lowest-index argmax of the very floats prob receives); any non-empty
 * subset, an output passed as NULL is not computed.  A label outside [0, n_classes) gives NaN in that row's lpd and nowhere
 * else.  pred[p][b][.] depends on the particle and the row alone.
 * Workspace: a call that asks for prob, lpd, ent or label needs stein_predict_bnn_class_workspace_bytes(n, batch, n_classes)
 * bytes: 4 (n_classes + 2) per row and particle slice, the slices of stein_predict_glm; it may hold anything on entry.  A
 * call that only asks for pred needs none (NULL, 0).  Deterministic: no atomics, the slices are merged in slice order in fp64.
 * Refused before any launch, in this order: theta, cols or X NULL, all five outputs NULL, lpd without labels, an unknown
 * output (STEIN_E_BADARG); a bad shape (STEIN_E_SHAPE); the domain (STEIN_E_UNSUPPORTED, naming the limit); blocks that do not
 * fit d or overlap (STEIN_E_SHAPE); the workspace (STEIN_E_WORKSPACE). */
int stein_predict_bnn_class_workspace_bytes(int64_t n, int64_t batch, int64_t n_classes, size_t* out_bytes);
int stein_predict_bnn_class(const float* theta, int64_t n, int64_t d, int output, int64_t n_in, int64_t n_hidden,
                            int64_t n_classes, const int64_t* cols, const float* X, const int32_t* labels, int64_t batch,
                            float* pred, float* prob, float* lpd, float* ent, int32_t* label,
                            void* workspace, size_t ws_bytes, void* stream);

/* Weighted class summaries: stein_predict_softmax / stein_predict_bnn_class under per-particle weights -- Stein importance
 * weights (stein_weights), or the counts of a thinned multiset (torch.bincount of stein_thin's indices).  weights [n]: fp64
 * device data, never read on the host, w_p >= 0, their sum W > 0; they need not sum to 1.
 *   prob_bc = sum_p w_p p_pbc / W      lpd_b = log(sum_p w_p p_{pb,y_b} / W)      ent_b = sum_p w_p H(p_pb.) / W
 *   label_b = the lowest-index argmax_c of the very floats prob receives
 *   ess [1] (fp64, device) = W^2 / sum_p w_p^2, the effective sample size of the weights
 * with p_pbc and H exactly those of the unweighted calls.  The conventions are those of stein_predict_glm_weighted:
 *   Lane weights: the lanes hold fl32(w_p / W), the quotient taken in fp64; a weight below 2^-126 W counts as zero.
 *   Power-of-two scaling: rescaling the weights by a power of two changes no bit of any output (while the sums stay in
 *     fp64's normal range).
 *   Zero weight: a particle of lane weight zero enters no summary, even if its probabilities are NaN.
 *   Bad weights: a negative or non-finite weight, W = 0 or an overflowing W return STEIN_OK with every requested prob / lpd /
 *     ent row and ess NaN and every label -1.
 *   Bad labels: a label outside [0, n_classes) still gives NaN in that row's lpd and nowhere else.
 *   pred does not depend on the weights: it is bit for bit the unweighted call's and is written for every particle.
 *   Deterministic: no atomics; a repeated call is bit-identical, whatever the workspace holds on entry.
 *   Summation: a slice's sums are sum_p fl32(w_p / W) q_p taken with one fmaf per term, particles ascending; the slices are
 *     added in slice order in fp64 and nothing is divided, because the lane weights already sum to 1.
 * When pred is NULL, particles of lane weight zero are not computed and staging units that hold nothing else are not read:
 * a thinned sample costs about what its distinct particles cost.  No summary bit depends on whether pred is asked for.
 * Workspace: a call that asks for prob, lpd, ent, label or ess needs stein_predict_*_weighted_workspace_bytes(n, batch,
 * n_classes) bytes, 8-byte aligned (STEIN_E_WORKSPACE otherwise) -- the unweighted size plus 24 bytes per particle slice (of
 * the bound min(ceil(n / 16), 1024)) and 16 more for the sums of the weights, which come first; monotone in n and batch,
 * independent of d.  It may hold anything on entry.  A call that only asks for pred needs none.
 * Refusals and their order are those of the unweighted calls, with weights == NULL among the NULL pointers (STEIN_E_BADARG)
 * and ess counting as a requested output and as a summary: an ess-only call is legal and needs the workspace. */
int stein_predict_softmax_weighted_workspace_bytes(int64_t n, int64_t batch, int64_t n_classes, size_t* out_bytes);
int stein_predict_softmax_weighted(const float* theta, int64_t n, int64_t d, int output, int64_t w_col, int64_t n_feats,
                                   int64_t n_classes, const float* X, const int32_t* labels, int64_t batch,
                                   const double* weights, float* pred, float* prob, float* lpd, float* ent, int32_t* label,
                                   double* ess, void* workspace, size_t ws_bytes, void* stream);
int stein_predict_bnn_class_weighted_workspace_bytes(int64_t n, int64_t batch, int64_t n_classes, size_t* out_bytes);
int stein_predict_bnn_class_weighted(const float* theta, int64_t n, int64_t d, int output, int64_t n_in, int64_t n_hidden,
                                     int64_t n_classes, const int64_t* cols, const float* X, const int32_t* labels,
                                     int64_t batch, const double* weights, float* pred, float* prob, float* lpd, float* ent,
                                     int32_t* label, double* ess, void* workspace, size_t ws_bytes, void* stream);

/* Order statistics of the outputs: credible bands and the ensemble median per test point, without pred.
 *   out [n_ranks][batch]   out[i][b] = the ranks[i]-th smallest (0-based) of the n values f_pb, p = 0 .. n-1
 * with f_pb bit for bit what stein_predict_glm / stein_predict_bnn write to pred for the same arguments (one body of device
 * code computes both).  The result is exact -- an element of the column pred would have held -- not a sketch.  The order is
 * numeric with -0 before +0; every NaN, of either sign, sorts last (as in torch.sort) and comes back as a quiet NaN.
 * ranks: a HOST array of n_ranks integers in [0, n), in any order, repeats allowed; read before the call returns.  A rank's
 * row does not depend on which other ranks share the call.  At most STEIN_PRED_RANKS_MAX ranks per call.
 * Method: a radix select over the 32-bit order-preserving keys of the outputs, 4 bits per level: the forward pass runs 8
 * times and counts digits; nothing of size n is stored.  The only values summed across workgroups are integer counts
 * (integer atomics), so a repeated call is bit-identical and the result depends neither on the grid nor on the particle
 * slices.  The host never reads device memory and never synchronises; every launch goes on `stream`.
 * Workspace: stein_predict_ranks_workspace_bytes = 76 bytes per (row, rank) -- the key prefix, the remaining rank, the rank
 * whose counts it shares, 16 counts -- so 76 * batch * n_ranks: independent of n and d, 4-byte aligned.  It may hold
 * anything on entry and carries nothing from call to call.
 * Refused before any launch, in this order: a NULL pointer (theta, X, ranks, out, cols, out_bytes) or n_ranks < 1
 * (STEIN_E_BADARG); then the output, shape, kind, column and width checks of stein_predict_* with their codes and messages;
 * n_ranks > STEIN_PRED_RANKS_MAX (STEIN_E_UNSUPPORTED); a rank outside [0, n) (STEIN_E_BADARG); no workspace, too small a
 * one or a misaligned one (STEIN_E_WORKSPACE). */
enum { STEIN_PRED_RANKS_MAX = 8 };
int stein_predict_ranks_workspace_bytes(int64_t n, int64_t batch, int64_t n_ranks, size_t* out_bytes);
int stein_predict_glm_ranks(const float* theta, int64_t n, int64_t d, int kind, int output, int64_t w_col, int64_t n_feats,
                            const float* X, int64_t batch, const int64_t* ranks /* host */, int64_t n_ranks,
                            float* out /* [n_ranks][batch] */, void* workspace, size_t ws_bytes, void* stream);
int stein_predict_bnn_ranks(const float* theta, int64_t n, int64_t d, int64_t n_in, int64_t n_hidden, const int64_t* cols,
                            int output, const float* X, int64_t batch, const int64_t* ranks, int64_t n_ranks,
                            float* out, void* workspace, size_t ws_bytes, void* stream);
/* test hook, per calling thread: the ranks calls cut the particles into `slices` slices (1 .. 1024; never less than one pass
 * of 16 particles per slice) instead of the summary calls' plan; 0 = default.  No bit of the result depends on it. */
int stein_debug_predict_ranks_slices(int slices);

/* Weighted order statistics: credible bands under per-particle weights (stein_weights) or of a thinned multiset (the counts
 * of stein_thin's indices), again without pred.  Every particle carries a mass m_p, an unsigned 32-bit integer (device
 * array masses [n]; stein_predict_rank_masses below makes them from weights).  M = sum_p m_p with 0 < M < 2^32.
 *   out [n_levels][batch]  out[i][b] = the smallest f_pb among the particles with m_p > 0 such that the mass of the
 *                          particles with m_p > 0 and key(f) <= key(f_pb) exceeds t_i = max(0, ceil(levels[i] * M) - 1)
 * t_i is computed on the device, one fp64 multiply and a ceil; the host never learns M.  This is NumPy's
 * np.quantile(f, q, weights=m, method="inverted_cdf"): with counts c it is np.sort(np.repeat(f, c))[t] exactly, with m = 1
 * the unweighted t-th order statistic bit for bit, and the level (t + 0.5) / M selects target t for every M < 2^32.  It is
 * NOT the linear interpolation that Python's quantiles() puts on top of the unweighted order statistics: no two elements
 * are ever mixed.  f_pb, the key order (-0 before +0, every NaN last, returned as a quiet NaN) and the exactness are those
 * of stein_predict_*_ranks.  A particle of mass 0 is skipped: its output may be NaN and is never returned or counted.
 * levels: a HOST array of n_levels doubles in [0, 1], in any order, repeats allowed, read before the call returns; a level's
 * row does not depend on its company.  At most STEIN_PRED_RANKS_MAX levels per call.
 * Method: the select of stein_predict_*_ranks with every output adding m_p in place of 1 to a 32-bit counter per bin; all
 * sums across workgroups are 32-bit integer atomics, so a repeated call is bit-identical and the result depends on neither
 * the grid, the particle slices nor the digit width.  A word per bin costs four times the LDS of the unweighted call's
 * bytes.  The digit width, 1 .. 4 bits a level, is the one of the least ceil(32 / bits) / min(2, workgroups whose LDS fit a
 * CU), the wider on a tie (measured: two resident workgroups run a forward pass 1.9 times faster than one, more no faster);
 * a grid of at most 256 workgroups takes the widest width that fits.  A first small launch sums the masses in 64 bits; the
 * masses are not trusted: M = 0 or M >= 2^32 gives NaN rows and STEIN_OK.
 * Workspace: stein_predict_ranks_weighted_workspace_bytes = 512 bytes + 76 per (row, level); independent of n and d,
 * 8-byte aligned; it may hold anything on entry.
 * Refused before any launch, in the order of stein_predict_*_ranks: masses == NULL and levels == NULL among the NULL
 * pointers and n_levels < 1 (STEIN_E_BADARG); the output, shape, kind, column and width checks; n_levels >
 * STEIN_PRED_RANKS_MAX (STEIN_E_UNSUPPORTED); a level outside [0, 1], NaN included (STEIN_E_BADARG); the workspace
 * (STEIN_E_WORKSPACE); a digit width forced by the hook below whose counters do not fit a CU's LDS (STEIN_E_UNSUPPORTED). */
int stein_predict_ranks_weighted_workspace_bytes(int64_t n, int64_t batch, int64_t n_levels, size_t* out_bytes);
int stein_predict_glm_ranks_weighted(const float* theta, int64_t n, int64_t d, int kind, int output, int64_t w_col,
                                     int64_t n_feats, const float* X, int64_t batch, const uint32_t* masses,
                                     const double* levels /* host */, int64_t n_levels, float* out /* [n_levels][batch] */,
                                     void* workspace, size_t ws_bytes, void* stream);
int stein_predict_bnn_ranks_weighted(const float* theta, int64_t n, int64_t d, int64_t n_in, int64_t n_hidden,
                                     const int64_t* cols, int output, const float* X, int64_t batch, const uint32_t* masses,
                                     const double* levels, int64_t n_levels, float* out, void* workspace, size_t ws_bytes,
                                     void* stream);
/* test hook, per calling thread: the digit width of the weighted ranks calls, 1 .. 4 bits a level; 0 = the rule above.  No bit
 * of the result depends on it.  The stein_debug_predict_ranks_slices hook applies to the weighted calls too. */
int stein_debug_predict_ranks_weighted_bits(int bits);

/* Masses from weights, on the device: weights [n] fp64 (device) -> masses [n] and info [2] fp64 (device).
 *   STEIN_MASS_NORMALISED  m_p = rint(w_p / W * 2^31), the quotient taken in fp64, W the fp64 sum of the weights in a fixed
 *                          order that depends on n alone.  n <= 2^30, so M <= 2^31 + n / 2 < 2^32; a weight below 2^-32 W
 *                          gets mass 0; a power-of-two rescaling of the weights changes no bit.
 *   STEIN_MASS_COUNTS      m_p = w_p exactly: every weight an integer in [0, 2^32), their sum below 2^32.
 *   info[0] = M as a double, info[1] = the number of particles with m_p > 0.
 * The host never reads the weights.  A negative or non-finite weight, W = 0, an overflow of W, or (COUNTS) a weight that is no
 * integer or a sum of 2^32 or more: the call returns STEIN_OK, every mass is 0 and info[0] is NaN, and a weighted ranks
 * call on these masses returns NaN rows.  Deterministic: no atomics; a repeated call is bit-identical.
 * Workspace: stein_predict_rank_masses_workspace_bytes(n) = 24 bytes per workgroup of 256 lanes, at most 256 of them; 8-byte
 * aligned; it may hold anything on entry.  Refused: a NULL pointer or an unknown mode (STEIN_E_BADARG), n outside
 * [1, 2^30] (STEIN_E_SHAPE), the workspace (STEIN_E_WORKSPACE). */
enum { STEIN_MASS_NORMALISED = 0, STEIN_MASS_COUNTS = 1 };
int stein_predict_rank_masses_workspace_bytes(int64_t n, size_t* out_bytes);
int stein_predict_rank_masses(const double* weights, int64_t n, int mode, uint32_t* masses, double* info /* [2] */,
                              void* workspace, size_t ws_bytes, void* stream);

/* The predictive distribution of y itself, observation noise included: the Gaussian mixture over the particles
 *   F_b(t) = sum_p w_p Phi((t - z_pb) sqrt(tau_p)) / W
 * with z_pb the linear output -- bit for bit what stein_predict_* write to pred with STEIN_PRED_LINK (the same device code) --
 * tau_p = noise_precision (STEIN_GLM_LINEAR) or exp(log_gamma_p) (the network), and w_p = 1 (weights == NULL) or the
 * caller's weights.  STEIN_GLM_LOGISTIC is refused (STEIN_E_UNSUPPORTED): y is Bernoulli there, and the predictive
 * probability is the mean of the outputs with STEIN_PRED_MEAN (output="mean").
 *
 * stein_predict_*_ycdf: out[i][b] = F_b(t[i][b]), t and out [n_pts][batch] device floats, 1 <= n_pts <=
 * STEIN_PRED_Y_POINTS_MAX.  With t = y this is the probability integral transform of the held-out rows; F_b(u) - F_b(l) is
 * the mass of an interval.  Phi(x) = erfcf(-x / sqrt 2) / 2 in fp32; every lane keeps n_pts running fp32 sums over its
 * particle slice, and a finish kernel adds the slices in slice order in fp64.
 *
 * stein_predict_*_yquantiles: out[i][b] and out_lo[i][b] (optional) bracket the levels[i]-quantile of F_b: predictive
 * intervals of y.  levels: a HOST array of n_levels <= STEIN_PRED_RANKS_MAX doubles strictly inside (0, 1), read before the
 * call returns; passes in [1, 12].  Method, passes + 1 forward passes and no host read of device memory:
 *   bracket   [lo, hi] = the least and the largest component quantile z_pb + Phi^-1(level) / sqrt(tau_p) over the particles
 *             with w_p > 0 (Phi^-1 on the host in fp64), each moved outward by 2^-21 (|z_pb| + |Phi^-1 / sqrt tau_p|) for what the
 *             fp32 evaluation can lose: below the least every component's distribution function is under the level, at the
 *             largest it has reached it, so the mixture's quantile lies between.
 *   refine    7 interior points p_j = min(fma(hi - lo, j / 8, lo), hi) per (row, level); one pass sums F at all 7 n_levels
 *             points (at most 56 running sums a lane); [lo, hi] becomes [p_(j-1), p_j] for the first j with F(p_j) >= level
 *             (p_0 = lo), or [p_7, hi] when there is none.  lo <= hi always, and no end ever moves outward.
 * The width shrinks eightfold per pass whatever the data: hi - lo <= (hi_0 - lo_0) / 8^passes plus one ulp of the bracket's
 * ends; 8 passes reach neighbouring floats from any start.  out = hi, out_lo = lo: F evaluated as above is >= level at hi
 * and < level at lo (or lo is the bracket pass's), which is the certificate.  A level's row does not depend on its company.
 *
 * Weights: as for the weighted summaries above, word for word -- fp64 device data, w >= 0, W > 0, never read on the host;
 * the lanes hold fl32(w_p / W), the quotient in fp64, so a power-of-two rescaling changes no bit; a particle of weight zero
 * is skipped even when its output is NaN; bad weights give NaN rows and STEIN_OK.  weights == NULL: every particle counts 1
 * and the finish kernel divides by n.
 * Deterministic: no atomics, the slices are merged in slice order; a repeated call is bit-identical.
 * Workspace: stein_predict_ycdf_workspace_bytes(n, batch, n_pts) / stein_predict_yquantiles_workspace_bytes(n, batch,
 * n_levels): the weight pass's header (16 bytes and 24 per particle slice), for the quantiles two floats per (row, level),
 * and the partial sums, A = n_pts or 7 n_levels floats per (slice, row).  That is up to eleven times the summaries' state,
 * so the calls cut the summaries' slice count down until the partial sums of a full call (8 points, 8 levels) fit 2^23 floats
 * (then down to whole rounds of 512 workgroups where that leaves any, or to one slice; the slices of a call do not depend on
 * how many points or levels it carries): they take at
 * most 4 A min(min(ceil(n / 16), 1024) batch, 2^19 + batch, 2^23 / A + batch) bytes.  Monotone in every argument, independent
 * of d, a multiple of 8; 8-byte aligned; it may hold anything on entry and carries nothing from call to call.
 * Refused before any launch, in this order: a NULL pointer (cols, theta, X, t / levels, out) or n_pts / n_levels < 1
 * (STEIN_E_BADARG); the shape, kind, column and width checks of stein_predict_* with their codes and messages; the logistic
 * kind (STEIN_E_UNSUPPORTED); a noise_precision that is not positive and finite (STEIN_E_BADARG); n_pts >
 * STEIN_PRED_Y_POINTS_MAX or n_levels > STEIN_PRED_RANKS_MAX (STEIN_E_UNSUPPORTED); a level outside (0, 1), NaN included, or
 * passes outside [1, 12] (STEIN_E_BADARG); no workspace, too small a one or a misaligned one (STEIN_E_WORKSPACE). */
enum { STEIN_PRED_Y_POINTS_MAX = 8, STEIN_PRED_Y_PASSES_MAX = 12 };
int stein_predict_ycdf_workspace_bytes(int64_t n, int64_t batch, int64_t n_pts, size_t* out_bytes);
int stein_predict_yquantiles_workspace_bytes(int64_t n, int64_t batch, int64_t n_levels, size_t* out_bytes);
int stein_predict_glm_ycdf(const float* theta, int64_t n, int64_t d, int kind, int64_t w_col, int64_t n_feats, const float* X,
                           int64_t batch, double noise_precision, const float* t /* device, [n_pts][batch] */, int64_t n_pts,
                           const double* weights /* device [n] or NULL */, float* out /* [n_pts][batch] */,
                           void* workspace, size_t ws_bytes, void* stream);
int stein_predict_bnn_ycdf(const float* theta, int64_t n, int64_t d, int64_t n_in, int64_t n_hidden, const int64_t* cols,
                           const float* X, int64_t batch, const float* t, int64_t n_pts, const double* weights, float* out,
                           void* workspace, size_t ws_bytes, void* stream);
int stein_predict_glm_yquantiles(const float* theta, int64_t n, int64_t d, int kind, int64_t w_col, int64_t n_feats,
                                 const float* X, int64_t batch, double noise_precision, const double* levels /* host */,
                                 int64_t n_levels, int passes, const double* weights /* device [n] or NULL */,
                                 float* out /* [n_levels][batch] */, float* out_lo /* [n_levels][batch] or NULL */,
                                 void* workspace, size_t ws_bytes, void* stream);
int stein_predict_bnn_yquantiles(const float* theta, int64_t n, int64_t d, int64_t n_in, int64_t n_hidden, const int64_t* cols,
                                 const float* X, int64_t batch, const double* levels, int64_t n_levels, int passes,
                                 const double* weights, float* out, float* out_lo, void* workspace, size_t ws_bytes,
                                 void* stream);

/* small helpers used by the host layer */
int stein_cast_f64_to_f32(const double* src, float* dst, int64_t count, void* stream);
int stein_cast_f32_to_bf16(const float* src, void* dst, int64_t count, void* stream);

/* ---- device error word -----------------------------------------------------------------------------
 * The entry points are asynchronous, so a kernel that has to give up cannot return a code.  It writes NaN into what it
 * was computing (the step's bandwidth: the reference's own failure value, compute_median.py:4-16 of identical particles)
 * and raises a per-device word in page-locked host memory; stein_svgd_phi and stein_apply_* look at that word -- a plain
 * host read, no synchronisation -- before they queue anything and return STEIN_E_HIP once, naming the kernel.  Today one
 * kernel can raise it: the one-launch radix select of the fused call (every n > 512), whose level barriers are
 * bounded although they cannot deadlock by construction.
 * stein_take_device_error: the same check on demand (0, or STEIN_E_HIP once).
 * Test hooks (per calling thread, no effect on results): stein_debug_hist_all_grid(blocks) launches that kernel with
 * `blocks` workgroups instead of one per virtual workgroup (nvb: 512 up to n = 4096, above that as many as the chip
 * holds at once; 0 = default; any grid >= 1 gives the same median: tests/test_gpu_spec.py);
 * stein_debug_raise_device_error raises the current device's word as a kernel would. */
int stein_take_device_error(void);
int stein_debug_hist_all_grid(int blocks);
int stein_debug_no_warm(int off);   /* test hook, per calling thread: 1 = the fused call's select launches without the
                                       workgroups that re-read theta and the score for the folded operand's split; 0 = default */
int stein_debug_hist_all_vblocks(int nvb);   /* tuning aid: virtual workgroups per level of that kernel (0 = default) */
int stein_debug_raise_device_error(void);

#ifdef __cplusplus
}
#endif
#endif /* STEINHIP_H */
