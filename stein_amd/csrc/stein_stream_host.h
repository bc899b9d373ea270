// stein_stream_host.h -- the host side the streaming steps share (the RBF step of stein_stream.hip, the IMQ step of
// stein_imq.hip; the streaming median works on the RBF step's layout): one shape check, one layout with its views, the size
// and plan queries, the prologue of the four step entry points and the launch that adds their block partials.
#pragma once
#include "stein_x3.h"

#include "stein_stream_tile.h"

// What tells one streaming step from the other on the host
struct StreamKind {
  const char* name;   // in the shape check's messages
  int unit;           // columns of phi one workgroup owns: the RBF step's column group of 256, the IMQ step's block of 128
  int planes;         // sets of transposed planes: W^T | theta^T, G^T
  int osets;          // sets of partial O: K.W | K.G, K3.theta
};
constexpr StreamKind STREAM_RBF{"streaming", 256, 1, 1};
constexpr StreamKind STREAM_IMQ{"IMQ", 128, 2, 2};

// r | sc | t3 | planes[0 .. np) | o[0 .. no) | rs | sq, and behind `total` what only the KSD forms use: rd | kpart.  The
// first three sections depend on n and d alone and the KSD tail is appended: a KSD buffer serves the plain step, and either
// step's buffer serves stein_stream_median (its histograms lie in planes[0], stein_stream.hip).
struct StreamLayout {
  int64_t row_tiles, col_units, cblocks, jsplit, jtiles_per, sq_blocks;
  int64_t rows, dk, dc, nk;                      // padded extents of the planes (the x3_* of SteinLayout)
  int np, no;                                    // StreamKind's planes and osets
  size_t r, sc, t3, planes[2], o[2], rs, sq, total;   // byte offsets, 256-byte aligned
  size_t rd, kpart, ksd_total;
};

static inline int stream_check_shape(const StreamKind& k, int64_t n, int64_t d, int dtype, int flags) {
  if (dtype == STEIN_BF16) return fail(STEIN_E_UNSUPPORTED, "the %s step takes fp32 inputs (STEIN_F32), not bf16", k.name);
  if (dtype != STEIN_F32) return fail(STEIN_E_UNSUPPORTED, "dtype %d", dtype);
  if (flags != 0) return fail(STEIN_E_BADARG, "the %s step takes no flags, got 0x%x", k.name, flags);
  if (n < 1 || d < 1) return fail(STEIN_E_SHAPE, "bad shape n=%lld d=%lld", (long long)n, (long long)d);
  return stein_check_size(n, d);
}

// The plan: one workgroup per (row tile, column unit, j range).  The j ranges fill the resident grid (one workgroup per CU)
// when the row tiles and column units alone do not: jsplit = floor(resident / (row_tiles col_units)), at most one range
// per 128-column j tile; ranges are whole j tiles and empty tails are dropped.  So jsplit > 1 only while
// jsplit row_tiles col_units <= resident: a set of partial sums then holds at most resident x 128 x 256 floats (32 MiB),
// whatever n and d; beyond that there is one range and they are n d floats.
static inline int stream_make_layout(const StreamKind& k, int64_t n, int64_t d, StreamLayout* L) {
  *L = StreamLayout{};
  L->row_tiles = (n + ST_ROWS - 1) / ST_ROWS;
  L->cblocks = (d + 127) / 128;
  L->col_units = (d + k.unit - 1) / k.unit;
  const int64_t jtiles = L->row_tiles;
  const int hook = stein_stream_jsplit_hook();
  int64_t want = hook > 0 ? hook : (int64_t)(RESIDENT_ONE_PER_CU / (double)(L->row_tiles * L->col_units));
  if (want < 1) want = 1;
  if (want > jtiles) want = jtiles;
  L->jtiles_per = (jtiles + want - 1) / want;
  L->jsplit = (jtiles + L->jtiles_per - 1) / L->jtiles_per;
  L->rows = L->row_tiles * ST_ROWS;
  L->nk = L->rows;
  L->dk = (int64_t)align_up((size_t)d, 32);
  L->dc = (int64_t)align_up((size_t)d, 128);
  int64_t sqb = (n * d + 1023) / 1024;
  if (sqb > 1024) sqb = 1024;
  L->sq_blocks = sqb;
  L->np = k.planes;
  L->no = k.osets;
  size_t at = 0;
  auto put = [&](size_t bytes) { const size_t o = at; at = align_up(at + bytes, 256); return o; };
  L->r = put((size_t)L->rows * 4);
  L->sc = put((size_t)(6 * L->dc + 4) * 4);
  L->t3 = put((size_t)3 * L->rows * L->dk * 2);
  for (int p = 0; p < L->np; ++p) L->planes[p] = put((size_t)3 * L->dc * L->nk * 2);
  for (int p = 0; p < L->no; ++p) L->o[p] = put((size_t)L->jsplit * n * d * 4);
  L->rs = put((size_t)L->jsplit * n * 4);
  L->sq = put((size_t)sqb * 8);
  L->total = at;
  L->rd = put((size_t)L->jsplit * n * 4);
  L->kpart = put((size_t)2 * sqb * 8);
  L->ksd_total = at;
  if (L->row_tiles * L->col_units * L->jsplit > 0x7fffffffll) return fail(STEIN_E_SHAPE, "too many tiles");
  return STEIN_OK;
}

// Every address the streaming entry points use, formed once: of a stored-D layout only the planes' extents; the planes the
// split launchers take (one set: the folded W^T in Gt3; two: theta^T, then G^T); and the step's partial sums (the j ranges'
// K.W or K.G in OG, K3.theta in OT, their row sums in RS, the |phi|^2 block partials in SQ; no K.theta: nothing here asks
// for dK, and the statistic does without it).
// The median passes StreamMedianLayout's hist / sel offsets: its histograms and select state lie where the step keeps its
// transposed planes and partial sums, which that call never touches.
static inline StepViews stream_views(const StreamLayout& L, void* workspace, size_t hist_at = 0, size_t sel_at = 0) {
  char* ws = (char*)workspace;
  StepViews v{};
  v.L.x3_rows = L.rows; v.L.x3_dk = L.dk; v.L.x3_dc = L.dc; v.L.x3_nk = L.nk;
  v.r = (float*)(ws + L.r);
  v.planes = ws;
  v.T3 = (unsigned short*)(ws + L.t3);
  if (L.np == 2) v.Tt3 = (unsigned short*)(ws + L.planes[0]);
  v.Gt3 = (unsigned short*)(ws + L.planes[L.np - 1]);
  v.sc = (float*)(ws + L.sc);
  v.cmax = (u32*)(v.sc + x3_sc_cmax(L.dc));
  v.two_s = v.sc + x3_sc_two_s(L.dc);
  v.OG = (float*)(ws + L.o[0]);
  if (L.no == 2) v.OT = (float*)(ws + L.o[1]);
  v.RS = (float*)(ws + L.rs);
  v.SQ = (double*)(ws + L.sq);
  if (sel_at) {
    v.hist = (u64*)(ws + hist_at);
    v.sel = (SelState*)(ws + sel_at);
  }
  return v;
}

// stein_{stream,imq}{,_ksd}_workspace_bytes
static inline int stream_workspace_bytes(const StreamKind& k, bool ksd, int64_t n, int64_t d, int dtype, int flags,
                                         size_t* out_bytes) {
  if (!out_bytes) return fail(STEIN_E_BADARG, "out_bytes is NULL");
  int rc = stream_check_shape(k, n, d, dtype, flags);
  if (rc) return rc;
  StreamLayout L;
  if ((rc = stream_make_layout(k, n, d, &L))) return rc;
  *out_bytes = ksd ? L.ksd_total : L.total;
  return STEIN_OK;
}

// stein_{stream,imq}_plan
static inline int stream_plan(const StreamKind& k, int64_t n, int64_t d, int* row_tiles, int* col_units, int* jsplit) {
  if (!row_tiles || !col_units || !jsplit) return fail(STEIN_E_BADARG, "NULL output");
  int rc = stream_check_shape(k, n, d, STEIN_F32, 0);
  if (rc) return rc;
  StreamLayout L;
  if ((rc = stream_make_layout(k, n, d, &L))) return rc;
  *row_tiles = (int)L.row_tiles;
  *col_units = (int)L.col_units;
  *jsplit = (int)L.jsplit;
  return STEIN_OK;
}

// The finish pass's vec word.  Bit 0: the 16-byte path, d % 4 == 0 and theta and phi aligned (a NULL phi counts as aligned),
// chosen alike in the plain and the KSD form so that |phi|^2 is summed in the same order; bit 1 (read by the KSD form only):
// the score is aligned too, which only decides how its rows are loaded on that path.
static inline int stream_vec(int64_t d, const void* theta, const void* phi, const void* score) {
  return (d % 4 == 0 && (((uintptr_t)theta | (uintptr_t)phi) & 15) == 0 ? 1 : 0) | (((uintptr_t)score & 15) == 0 ? 2 : 0);
}

// One call of a step entry point after its prologue
struct StreamCall {
  StreamLayout L;
  StepViews v;
  float* RD;        // (KSD) the j ranges' second row sum, [jsplit][n]
  double* KP;       // (KSD) the S / S_diag block partials, [2][sq_blocks]
  unsigned nblk;    // the contraction's grid
  int vec;
  hipStream_t s;
};

// The prologue of stein_svgd_phi_{stream,imq}{,_ksd}: arguments (phi may be NULL in the KSD forms only), shape, layout,
// workspace size, the device's error word, views
static inline int stream_begin(const StreamKind& k, bool ksd, const void* theta, const void* score, int64_t n, int64_t d,
                               int dtype, const float* h2_in, const float* phi, const double* out, void* workspace,
                               size_t ws_bytes, int flags, void* stream, StreamCall* c) {
  if (!theta || !score || !h2_in || (!ksd && !phi) || !out || !workspace) return fail(STEIN_E_BADARG, "NULL pointer");
  if ((uintptr_t)workspace & 15) return fail(STEIN_E_BADARG, "the workspace must be 16-byte aligned");   // (16-byte loads of its sections)
  int rc = stream_check_shape(k, n, d, dtype, flags);
  if (rc) return rc;
  if ((rc = stream_make_layout(k, n, d, &c->L))) return rc;
  const size_t need = ksd ? c->L.ksd_total : c->L.total;
  if (ws_bytes < need) return fail(STEIN_E_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, need);
  if ((rc = stein_take_device_error())) return rc;   // a kernel of an earlier call on this device gave up: say so now
  c->v = stream_views(c->L, workspace);
  c->RD = ksd ? (float*)((char*)workspace + c->L.rd) : nullptr;
  c->KP = ksd ? (double*)((char*)workspace + c->L.kpart) : nullptr;
  c->nblk = (unsigned)(c->L.row_tiles * c->L.col_units * c->L.jsplit);
  c->vec = stream_vec(d, theta, phi, score);
  c->s = (hipStream_t)stream;
  return STEIN_OK;
}

// The last launch of a step: the finish pass's block partials -> the caller's sqnorm (plain) or three sums (KSD)
static inline int stream_sum(const StreamCall& c, double* out) {
  hipLaunchKernelGGL(k_stream_sum, dim3(c.KP ? 3 : 1), dim3(256), 0, c.s, c.v.SQ, c.KP, (int)c.L.sq_blocks, out);
  LAUNCH_CHECK("k_stream_sum");
  return STEIN_OK;
}
