"""Case tables of the softmax-regression calls (stein_score_softmax, stein_predict_softmax) and a Python mirror of both
dispatches: padded class count, particles per workgroup, chunk rows and lanes per row of the score; particles per pass, the X
tile and the slices of the predictive call.  TEST INFRASTRUCTURE ONLY.  tests/test_softmax_cases.py reads the constants back
from the sources and proves that the tables reach every instantiation and every edge the GPU tests promise."""
import numpy as np

import predict_cases as pc

# csrc/stein_score_softmax.hip
SM_LDS = 40448
SM_WLDS = 24576
SM_ROWS_MAX = 1024
SM_MAX_WGS = 1024
C_MIN, C_MAX, F_MAX, FC_MAX = 2, 32, 1024, 16384
PADDED = (4, 8, 16, 32)
CLASS_COUNTS = (2, 4, 5, 8, 9, 16, 17, 32)      # both ends of every padded-class instantiation


def padded(C):
    return next(cp for cp in PADDED if C <= cp)


def score_plan(F, C, B):
    """stein_score_softmax's dispatch -> dict(cp, ppw, crows, G, lds_words); from (F, C, batch) alone"""
    cs = (C + 3) & ~3
    fcs, ld = F * cs, F | 1
    ppw = 4 if 8 * fcs <= SM_WLDS else 2 if 4 * fcs <= SM_WLDS else 1
    crows = min((SM_LDS - 2 * ppw * fcs - 8) // (ld + 1 + ppw * cs), SM_ROWS_MAX, B)
    lpp, g = 256 // ppw, 1
    while g < 64 and lpp // g > crows and g < F:
        g *= 2
    return {"cp": padded(C), "ppw": ppw, "crows": crows, "G": g, "lds_words": 2 * ppw * fcs + crows * (ld + 1 + ppw * cs) + 4}


def score_chunk_rows(F, C):
    """rows of an LDS chunk when the batch does not cap it"""
    return score_plan(F, C, 1 << 30)["crows"]


def predict_plan(F, C, n, B):
    """stein_predict_softmax's dispatch -> dict(cp, pp, fc, ld, chunks, lds_words, row_tiles, slices, per)"""
    cp = padded(C)
    na = max(pc.PR_PASS, cp)
    fc = min(F, pc.PR_FC)
    ld = fc | 1
    rt, slices, per = pc.plan(n, B)
    return {"cp": cp, "pp": na // cp, "fc": fc, "ld": ld, "chunks": -(-F // fc), "lds_words": ((pc.PR_ROWS * ld + 3) & ~3) + fc * na,
            "row_tiles": rt, "slices": slices, "per": per}


def predict_workspace_bytes(n, B, C):
    return min(min(-(-n // pc.PR_PASS), pc.PR_SLICE_CAP) * B, pc.PR_TARGET_WGS * pc.PR_ROWS + B) * (C + 2) * 4


# ---- the score's cases ---------------------------------------------------------------------------------------------
def _score(name, F, C, B, n, alpha="none", lead=0, gap=0, tail=0, scale=1.0):
    """lead / gap / tail: foreign columns ahead of everything, between the alpha column and the weights, and at the end"""
    return {"name": name, "F": F, "C": C, "B": B, "n": n, "alpha": alpha, "lead": lead, "gap": gap, "tail": tail, "scale": scale}


SCORE_CLASSES = [_score("C%d" % C, 7, C, 11, 5, alpha=("after", "none", "before")[i % 3], lead=i % 2, tail=(i + 1) % 3)
                 for i, C in enumerate(CLASS_COUNTS)]
SCORE_FEATS = [_score("F1", 1, 3, 9, 6), _score("F7", 7, 3, 70, 6, alpha="after", scale=12.5), _score("F54", 54, 7, 100, 9, alpha="after"),
               _score("F512C32", 512, 32, 5, 2, alpha="before")]
_CH = score_chunk_rows(512, 32)          # 14 rows: the smallest chunk a cheap case has
SCORE_CHUNK = [_score("chunk_B%d" % B, 512, 32, B, 2) for B in (1, _CH - 1, _CH, _CH + 1, 2 * _CH - 1, 2 * _CH, 2 * _CH + 1, 3 * _CH + 1)]
# particle counts around a workgroup's, for 4, 2 and 1 particles per workgroup, and one grid plus one
SCORE_COUNTS = ([_score("ppw4_n%d" % n, 5, 3, 8, n, alpha="after") for n in (1, 3, 4, 5)]
                + [_score("ppw2_n%d" % n, 200, 16, 6, n) for n in (1, 2, 3)]
                + [_score("ppw1_n%d" % n, 400, 16, 6, n) for n in (1, 2)])
SCORE_GRID = [_score("grid_ppw4", 3, 3, 5, 4 * SM_MAX_WGS + 1, alpha="after"), _score("grid_ppw2", 200, 16, 3, 2 * SM_MAX_WGS + 1),
              _score("grid_ppw1", 400, 16, 3, SM_MAX_WGS + 1)]
# the weights' place: w_col > 0 with the alpha column before, after and absent, and foreign columns everywhere
SCORE_COLS = [_score("cols_before", 6, 5, 13, 7, alpha="before", lead=2, gap=3, tail=1),
              _score("cols_after", 6, 5, 13, 7, alpha="after", lead=2, gap=3, tail=4),
              _score("cols_none", 6, 5, 13, 7, alpha="none", lead=3, tail=2)]
# lanes per row: batches that leave 1, 2, ... 64 lanes to a row
SCORE_LANES = [_score("lanes_B%d" % B, 70, 4, B, 3) for B in (64, 32, 16, 8, 4, 2, 1)] + [_score("lanes_ppw1_B3", 400, 16, 3, 2)]
SCORE_CASES = SCORE_CLASSES + SCORE_FEATS + SCORE_CHUNK + SCORE_COUNTS + SCORE_GRID + SCORE_COLS + SCORE_LANES
SCORE_SUBSET_CASE = _score("subset", 9, 5, 20, 23, alpha="after", lead=1, tail=1)
BAD_LABEL_CASE = _score("bad_label", 6, 3, 10, 5, alpha="after", tail=1)


def _r32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def layout(case):
    """-> (w_col, alpha_col or -1, d)"""
    F, C = case["F"], case["C"]
    c = case["lead"]
    alpha_col = -1
    if case["alpha"] == "before":
        alpha_col, c = c, c + 1 + case["gap"]
    w_col = c
    c += F * C
    if case["alpha"] == "after":
        c += case["gap"]
        alpha_col, c = c, c + 1
    return w_col, alpha_col, c + case["tail"]


def score_args(case):
    """fp64 arrays of fp32-representable values; logits of order one whatever F"""
    import zlib
    rng = np.random.default_rng(zlib.crc32(("softmax:" + case["name"]).encode()))
    F, C, B, n = case["F"], case["C"], case["B"], case["n"]
    w_col, alpha_col, d = layout(case)
    theta = rng.normal(size=(n, d)) * 0.3
    theta[:, w_col:w_col + F * C] = rng.normal(size=(n, F * C)) * (1.5 / np.sqrt(F))
    if alpha_col >= 0:
        theta[:, alpha_col] = rng.uniform(-2.0, 1.0, size=n)
    X = rng.normal(size=(B, F))
    labels = rng.integers(0, C, size=B).astype(np.int32)
    return {"theta": _r32(theta), "X": _r32(X), "labels": labels, "w_col": w_col, "alpha_col": alpha_col, "d": d, "F": F, "C": C,
            "scale": case["scale"], "prior_precision": 0.75, "gamma_rate": 0.01}


def live_columns(case):
    w_col, alpha_col, d = layout(case)
    live = np.zeros(d, bool)
    live[w_col:w_col + case["F"] * case["C"]] = True
    if alpha_col >= 0:
        live[alpha_col] = True
    return live


# ---- the predictive call's cases ------------------------------------------------------------------------------------
def _pred(name, F, C, B, n, w_col=0, tail=0):
    return {"name": name, "F": F, "C": C, "B": B, "n": n, "w_col": w_col, "tail": tail}


THREE_SLICES = 40       # three slices of 14, 14 and 12 particles at a batch of one row tile
PRED_CLASSES = [_pred("C%d" % C, 9, C, 37, 19, w_col=i % 3, tail=i % 2) for i, C in enumerate(CLASS_COUNTS)]
PRED_FEATS = [_pred("F%dC%d" % (F, C), F, C, 21, 18) for F, C in ((1, 3), (58, 5), (59, 5), (117, 17), (58, 32), (59, 32))]
PRED_ROWS = [_pred("B%d" % B, 6, 3, B, 21, w_col=1) for B in (1, 255, 256, 257, 513)]
PRED_COUNTS = [_pred("n%d_C%d" % (n, C), 5, C, 7, n) for C in (3, 8, 16, 32) for n in (1, 15, 16, 17, THREE_SLICES)]
PRED_CASES = PRED_CLASSES + PRED_FEATS + PRED_ROWS + PRED_COUNTS
PRED_SUBSET_CASE = _pred("subsets", 9, 7, 300, 37, w_col=2, tail=1)


def predict_args(case):
    import zlib
    rng = np.random.default_rng(zlib.crc32(("softmax-predict:" + case["name"]).encode()))
    F, C, B, n = case["F"], case["C"], case["B"], case["n"]
    d = case["w_col"] + F * C + case["tail"]
    theta = rng.normal(size=(n, d)) * 0.3
    theta[:, case["w_col"]:case["w_col"] + F * C] = rng.normal(size=(n, F * C)) * (2.0 / np.sqrt(F))
    return {"theta": _r32(theta), "X": _r32(rng.normal(size=(B, F))), "labels": rng.integers(0, C, size=B).astype(np.int32),
            "w_col": case["w_col"], "d": d, "F": F, "C": C}
