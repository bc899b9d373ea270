"""The case tables of the wide-network tests (more than four input features: csrc/stein_score_wide.hip, k_predict_bnn_wide
of csrc/stein_predict.hip), a Python mirror of the wide dispatch rules, and the inputs of every case -- those of
tests/score_cases.py and tests/predict_cases.py, which are generic in n_in.  Shared by tests/test_bnn_wide_cases.py (CPU:
the tables reach every instantiation and edge, the allowances hold for a correct fp32 evaluation) and the GPU tests
tests/test_gpu_score_wide.py and tests/test_gpu_predict_wide.py.

TEST INFRASTRUCTURE ONLY."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_cases as pc  # noqa: E402
import score_cases as sc  # noqa: E402

NARROW_MAX = 4                      # up to here the wide entry points run the narrow ones
NIN_MAX, H_MAX, W1_MAX = 128, 1024, 16384

# ---- score: the constants of stein_score_wide.hip (tests/test_bnn_wide_cases.py reads them back from the source) ----------
SW_R = 8                # batch rows per register block
SW_XLDS = 3584          # floats of X and y per LDS chunk
SW_WLDS = 36 * 1024     # floats of w1 and gw1 of a workgroup's particles
SW_MAX_WGS = 1024       # the grid's cap
SCORE_KERNELS = ((64, 1), (128, 1), (256, 1), (256, 2), (256, 4))     # (LH lanes per particle, KH hidden units per lane)


def score_kernel(n_in, H):
    """the instantiation stein_score_bnn_wide dispatches to: (LH, KH)"""
    lh = 64 if H <= 64 else 128 if H <= 128 else 256
    while lh < 256 and (256 // lh) * n_in * H * 2 > SW_WLDS:
        lh *= 2
    kh = 1 if lh < 256 else next(k for k in (1, 2, 4) if -(-H // 256) <= k)
    return lh, kh


def score_grid_cap(n_in, H):
    """particles one grid covers before the grid-stride loop goes round again"""
    return SW_MAX_WGS * (256 // score_kernel(n_in, H)[0])


def score_chunk_rows(n_in):
    """batch rows per LDS chunk (a multiple of the row block)"""
    return (SW_XLDS // (n_in + 1)) // SW_R * SW_R


def score_chunk_batches(n_in):
    c = score_chunk_rows(n_in)
    return (c - 1, c, c + 1, 2 * c, 3 * c + 1)


def heavy_rows(B, n_in):
    """score_cases.heavy_rows for the wide kernel's chunking: row 0, both sides of every chunk edge, and the last row"""
    c = score_chunk_rows(n_in)
    rows = {0, B - 1}
    for e in range(c, B, c):
        rows |= {e - 1, e}
    return sorted(r for r in rows if 0 <= r < B)


class _wide_chunking:
    """score_cases.bnn_args / heavy_row_shares with the heavy rows at THIS kernel's chunk edges"""
    def __enter__(self):
        self.old = sc.heavy_rows
        sc.heavy_rows = heavy_rows

    def __exit__(self, *exc):
        sc.heavy_rows = self.old


def score_args(case):
    with _wide_chunking():
        return sc.bnn_args(case)


def heavy_row_shares(case, args):
    with _wide_chunking():
        return sc.heavy_row_shares(case, args)


def _score(n_in, H, n, B, flavor="plain", seed=0):
    return sc._bnn("w%d_H%d_%s" % (n_in, H, flavor), n_in, H, n, B, flavor, seed)


# the issue's table
SCORE_TABLE = [_score(*t) for t in [
    (5, 1, 3, 7), (5, 50, 20, 20), (8, 17, 5, 12), (9, 64, 7, 9), (13, 50, 21, 32), (16, 65, 5, 8), (17, 33, 6, 10),
    (32, 128, 3, 6), (33, 129, 3, 5), (64, 100, 4, 6), (90, 100, 5, 11), (127, 16, 3, 5), (128, 128, 2, 4), (16, 1024, 2, 3)]]
# (seed: with five particles the three log precisions drawn inside (-20, 20) spanned less than score_cases.
# check_extreme_inputs asks of an extreme case -- a precondition on the inputs alone; that case was reseeded)
SCORE_FLAVOR_SEEDS = {(90, "dead"): 2}
SCORE_FLAVORS = [_score(n_in, H, n, B, fl, SCORE_FLAVOR_SEEDS.get((n_in, fl), 0))
                 for n_in, H, n, B in ((13, 50, 21, 32), (90, 100, 5, 11)) for fl in ("dead", "saturated")]
# both sides of every dispatch edge: H at 64 | 65, 128 | 129, 256 | 257, 512 | 513 (lanes per particle, hidden units per
# lane), and n_in * H at 4608 | 4609.. (four particles' w1 and gw1 fill SW_WLDS) and 9216 | 9217.. (two particles')
SCORE_EDGES = [_score(*t) for t in [
    (5, 64, 6, 9), (5, 65, 5, 9), (5, 128, 5, 7), (5, 129, 3, 7), (5, 256, 3, 5), (5, 257, 3, 5), (5, 512, 2, 5), (5, 513, 2, 4),
    (72, 64, 5, 6), (73, 64, 5, 6), (72, 128, 3, 6), (73, 128, 3, 6)]]
SCORE_EDGE_PAIRS = (((5, 64), (5, 65)), ((5, 128), (5, 129)), ((5, 256), (5, 257)), ((5, 512), (5, 513)),
                    ((72, 64), (73, 64)), ((72, 128), (73, 128)))
# batches around one, two and three LDS chunks, at the widest and the narrowest chunk
SCORE_CHUNK = [sc._bnn("w%d_H5_chunk_B%d" % (n_in, B), n_in, 5, 5, B, "chunk") for n_in in (5, 127)
               for B in score_chunk_batches(n_in)]
# n just past one grid, once per lanes-per-particle: every grid-stride loop goes round twice
SCORE_GRID = [sc._bnn("w13_H50_grid", 13, 50, 4099, 3), sc._bnn("w5_H65_grid", 5, 65, 2051, 2),
              sc._bnn("w5_H129_grid", 5, 129, 1027, 2)]
SCORE_CASES = SCORE_TABLE + SCORE_FLAVORS + SCORE_EDGES + SCORE_CHUNK + SCORE_GRID

# ---- predictive: the constants of stein_predict_fwd.h -------------------------------------------------------------------
PR_WT = 16                          # hidden units per register tile, and per staging unit
PR_WIDE_LDS = 160 * 1024 // 4 - 128  # floats of dynamic LDS at most


def predict_tile(n_in):
    """predict_wide_tile -> (ld, ps, bytes): the staged row length of X, the particles per staging unit (one tile of PR_WT
    hidden units each), the kernel's dynamic LDS"""
    ld = n_in | 1
    xt, unit = pc.PR_ROWS * ld, (n_in + 2) * PR_WT
    ps = min(pc.PR_PASS, (PR_WIDE_LDS - xt) // unit)
    return ld, ps, 4 * (xt + ps * unit)


def _pred(n_in, H, n, B, tag=""):
    return pc._case("w%d_H%d%s" % (n_in, H, tag), "bnn", n, B, n_in=n_in, H=H)


PRED_TABLE = [_pred(*t) for t in [
    (5, 1, 3, 7), (5, 50, 20, 20), (8, 3, 17, 12), (13, 50, 21, 300), (16, 65, 5, 8), (17, 64, 18, 10), (33, 129, 33, 5),
    (90, 100, 5, 257), (127, 16, 3, 5), (128, 128, 2, 4)]]
# the staging unit is one tile of PR_WT hidden units of as many of a pass's particles as fit beside the X tile: all PR_PASS
# up to n_in = 78, 15 at 79, 11 at 90, 3 at 128.  Hidden counts at one tile, one unit past it (two units), past two units
PRED_EDGES = [_pred(*t) for t in [
    (5, 64, 5, 6), (5, 65, 5, 6), (6, 15, 17, 5), (7, 16, 5, 6), (7, 17, 18, 6), (9, 32, 5, 6), (9, 33, 5, 6), (15, 16, 5, 6),
    (15, 17, 19, 6), (31, 33, 15, 4), (78, 17, 16, 5), (79, 17, 16, 5), (79, 20, 15, 4)]]
PRED_EDGE_PAIRS = (((78, 17), (79, 17)),)
# particle counts around PR_PASS, and around the particles per staging unit where that is below PR_PASS; many slices
PRED_COUNTS = [_pred(13, 10, n, 5, "_n%d" % n) for n in (1, pc.PR_PASS - 1, pc.PR_PASS, pc.PR_PASS + 1, 2 * pc.PR_PASS + 1, 600)]
PRED_COUNTS += [_pred(90, 20, n, 5, "_n%d" % n) for n in (10, 12, 23)] + [_pred(128, 20, n, 5, "_n%d" % n) for n in (3, 4, 7)] + \
               [_pred(79, 20, 31, 4, "_n31")]
# rows at PR_ROWS - 1, PR_ROWS, PR_ROWS + 1 and past two tiles
PRED_ROWS = [_pred(13, 10, 5, B, "_B%d" % B) for B in (1, pc.PR_ROWS - 1, pc.PR_ROWS, pc.PR_ROWS + 1, 2 * pc.PR_ROWS + 3)]
PRED_CASES = PRED_TABLE + PRED_EDGES + PRED_COUNTS + PRED_ROWS
PRED_SUBSET_CASE = _pred(13, 50, 37, 300, "_subsets")
PRED_WEIGHTED = [(_pred(13, 50, 70, 20, "_w"), pat) for pat in ("positive", "counts", "zero_slices")] + \
                [(_pred(90, 20, 50, 7, "_w"), "zero_slices")]


def cpu_sized(case):
    """small enough for the NumPy references and fp32 emulations (which hold [n, B, H] arrays, n_in of them in a loop)"""
    return case["n"] * case["B"] * case["H"] * (case["n_in"] + 2) <= 3_000_000
