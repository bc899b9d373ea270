"""Case tables of the network-classifier calls (stein_score_bnn_class, stein_predict_bnn_class) and a Python mirror of both
launch plans: lanes per particle, hidden units per lane, particles per workgroup and chunk rows of the score; padded class
count, staged (particle, tile) pairs, the X tile and the slices of the predictive call.  TEST INFRASTRUCTURE ONLY.
tests/test_netclass_cases.py reads the constants back from the sources and proves that the tables reach every class of the
dispatch and every edge the GPU tests promise."""
import zlib

import numpy as np

import predict_cases as pc

# csrc/stein_score_bnn_class.hip
BC_R = 8
BC_LDS = 40448
BC_PLDS = 36864
BC_ROWS_MAX = 1024
BC_MAX_WGS = 1024
NIN_MAX, C_MIN, C_MAX, H_MAX, W_MAX = 128, 2, 32, 512, 16384
# csrc/stein_predict_fwd.h
PR_WT = 16
PR_WIDE_LDS = 160 * 1024 // 4 - 128
PADDED = (4, 8, 16, 32)
CLASS_COUNTS = (2, 4, 5, 8, 9, 16, 17, 32)      # both ends of every padded-class instantiation
INSTANCES = ((64, 1), (128, 1), (256, 1), (256, 2))
BLOCKS = ("w1", "b1", "w2", "b2", "log_lambda")


def cs_of(C):
    return (C + 3) & ~3


def padded(C):
    return next(cp for cp in PADDED if C <= cp)


def in_domain(F, H, C):
    """the one formula of include/steinhip.h"""
    return 1 <= F <= NIN_MAX and C_MIN <= C <= C_MAX and 1 <= H <= H_MAX and (F + cs_of(C)) * H <= W_MAX


def particle_floats(F, H, C):
    cs = cs_of(C)
    return 2 * (((F * H + 3) & ~3) + H * cs) + BC_R * H + 2 * BC_R * cs + 2 * cs


def score_plan(F, H, C, B):
    """stein_score_bnn_class's dispatch -> dict(lh, kh, ppw, crows, lds_words); from (n_in, H, C, batch) alone"""
    pf = particle_floats(F, H, C)
    lh = 64 if H <= 64 else 128 if H <= 128 else 256
    while lh < 256 and (256 // lh) * pf > BC_PLDS:
        lh *= 2
    ppw = 256 // lh
    crows = min(((BC_LDS - ppw * pf - 8) // (F + 1)) & ~(BC_R - 1), BC_ROWS_MAX, (B + BC_R - 1) & ~(BC_R - 1))
    return {"lh": lh, "kh": -(-H // lh), "ppw": ppw, "crows": crows, "lds_words": ppw * pf + crows * (F + 1) + 4,
            "bumped": lh > (64 if H <= 64 else 128 if H <= 128 else 256)}


def score_chunk_rows(F, H, C):
    """rows of an LDS chunk when the batch does not cap it"""
    return score_plan(F, H, C, 1 << 30)["crows"]


def predict_plan(F, H, C, n, B):
    """stein_predict_bnn_class's dispatch -> dict(cp, ps, ld, tiles, lds_words, row_tiles, slices, per)"""
    ld = F | 1
    xt = (pc.PR_ROWS * ld + 3) & ~3
    iw = (F + 1 + cs_of(C)) * PR_WT + cs_of(C)
    ps = min((PR_WIDE_LDS - xt) // iw, pc.PR_PASS)
    rt, slices, per = pc.plan(n, B)
    return {"cp": padded(C), "ps": ps, "ld": ld, "tiles": -(-H // PR_WT), "lds_words": xt + ps * iw, "row_tiles": rt, "slices": slices,
            "per": per}


def predict_workspace_bytes(n, B, C):
    return min(min(-(-n // pc.PR_PASS), pc.PR_SLICE_CAP) * B, pc.PR_TARGET_WGS * pc.PR_ROWS + B) * (C + 2) * 4


# ---- layouts -----------------------------------------------------------------------------------------------------------
def layout(case):
    """-> (cols [5] with -1 for an absent log_lambda, d): the blocks in case["order"], `lead` foreign columns ahead of them,
    `gap` between any two and `tail` behind"""
    F, H, C = case["F"], case["H"], case["C"]
    size = {"w1": F * H, "b1": H, "w2": H * C, "b2": C, "log_lambda": 1}
    at, c = {}, case["lead"]
    for i, name in enumerate(case["order"]):
        if i:
            c += case["gap"]
        at[name] = c
        c += size[name]
    return [at.get(k, -1) for k in BLOCKS], c + case["tail"]


def live_columns(case):
    cols, d = layout(case)
    F, H, C = case["F"], case["H"], case["C"]
    live = np.zeros(d, bool)
    for col, size in zip(cols, (F * H, H, H * C, C, 1)):
        if col >= 0:
            live[col:col + size] = True
    return live


def block_slices(case):
    cols, _ = layout(case)
    F, H, C = case["F"], case["H"], case["C"]
    return {k: slice(col, col + size) for k, col, size in zip(BLOCKS, cols, (F * H, H, H * C, C, 1)) if col >= 0}


_ORDERS = {"after": ("w1", "b1", "w2", "b2", "log_lambda"), "none": ("w1", "b1", "w2", "b2"),
           "before": ("log_lambda", "w1", "b1", "w2", "b2"), "permuted": ("b2", "w2", "log_lambda", "b1", "w1"),
           "permuted_none": ("w2", "b1", "b2", "w1")}


def _score(name, F, H, C, B, n, order="after", lead=0, gap=0, tail=0, scale=1.0):
    return {"name": name, "F": F, "H": H, "C": C, "B": B, "n": n, "order": _ORDERS[order], "lead": lead, "gap": gap, "tail": tail,
            "scale": scale}


def _r32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _theta(rng, case, n, cols, d):
    """pre-activations and logits of order one whatever the widths"""
    F, H, C = case["F"], case["H"], case["C"]
    theta = rng.normal(size=(n, d)) * 0.3
    theta[:, cols[0]:cols[0] + F * H] = rng.normal(size=(n, F * H)) / np.sqrt(F)
    theta[:, cols[1]:cols[1] + H] = rng.normal(size=(n, H)) * 0.5
    theta[:, cols[2]:cols[2] + H * C] = rng.normal(size=(n, H * C)) * (1.5 / np.sqrt(H))
    theta[:, cols[3]:cols[3] + C] = rng.normal(size=(n, C)) * 0.3
    if cols[4] >= 0:
        theta[:, cols[4]] = rng.uniform(-2.0, 1.0, size=n)
    return _r32(theta)


def score_args(case):
    """fp64 arrays of fp32-representable values"""
    rng = np.random.default_rng(zlib.crc32(("netclass:" + case["name"]).encode()))
    cols, d = layout(case)
    theta = _theta(rng, case, case["n"], cols, d)
    X = rng.normal(size=(case["B"], case["F"]))
    labels = rng.integers(0, case["C"], size=case["B"]).astype(np.int32)
    return {"theta": theta, "X": _r32(X), "labels": labels, "cols": cols, "d": d, "F": case["F"], "H": case["H"], "C": case["C"],
            "scale": case["scale"], "prior_precision": 0.75, "gamma_rate": 0.01}


# ---- the score's cases -------------------------------------------------------------------------------------------------
SCORE_CLASSES = [_score("C%d" % C, 6, 10, C, 11, 5, order=("after", "none", "before")[i % 3], lead=i % 2, tail=(i + 1) % 3)
                 for i, C in enumerate(CLASS_COUNTS)]
# every (lanes, units per lane) instantiation, with and without the step to fewer particles per workgroup that the LDS forces
SCORE_PLANS = [_score("ppw4", 5, 16, 3, 13, 6), _score("ppw2", 6, 100, 7, 9, 3, order="none"),
               _score("ppw1", 4, 200, 3, 9, 3), _score("kh2", 8, 512, 8, 9, 2), _score("kh2_odd", 4, 300, 3, 10, 2, order="none"),
               _score("bumped_to_2", 100, 60, 5, 9, 3), _score("bumped_to_1", 128, 64, 32, 9, 2, order="none"),
               _score("covertype", 54, 100, 7, 100, 3, scale=50.0)]
SCORE_HIDDEN = [_score("H%d" % H, 3, H, 3, 10, 5, order=("after", "none")[i % 2]) for i, H in enumerate((1, 15, 16, 17, 65))]
SCORE_INPUTS = [_score("F1", 1, 12, 3, 10, 5), _score("F128", 128, 20, 4, 9, 3)]      # (5 inputs: ppw4 above)
SMALLEST_CHUNK = (116, 74, 2)            # the shape of the domain with the fewest chunk rows: 24, two particles per workgroup
_CH = score_chunk_rows(*SMALLEST_CHUNK)
SCORE_CHUNK = ([_score("chunk_B%d" % B, 116, 74, 2, B, 3, order="none") for B in (1, _CH - 1, _CH, _CH + 1, 2 * _CH + 1)]
               + [_score("lds_full", 128, 102, 32, 50, 2)])      # the largest particle: 136 KB, two chunks of 48 rows
# particle counts around a workgroup's, for 4, 2 and 1 particles per workgroup, and one grid plus one particle
SCORE_COUNTS = ([_score("ppw4_n%d" % n, 5, 16, 3, 8, n) for n in (1, 3, 4, 5)]
                + [_score("ppw2_n%d" % n, 6, 100, 7, 6, n, order="none") for n in (1, 2, 3)]
                + [_score("ppw1_n%d" % n, 4, 200, 3, 6, n) for n in (1, 2)])
SCORE_GRID = [_score("grid_ppw4", 2, 3, 2, 3, 4 * BC_MAX_WGS + 1)]
# the blocks' places: permuted, with foreign columns before, between and after; log_lambda before, after and absent
SCORE_COLS = [_score("cols_before", 5, 9, 5, 13, 7, order="before", lead=2, gap=3, tail=1),
              _score("cols_after", 5, 9, 5, 13, 7, order="after", lead=2, gap=1, tail=4),
              _score("cols_permuted", 5, 9, 5, 13, 7, order="permuted", lead=1, gap=2, tail=2),
              _score("cols_permuted_none", 5, 9, 5, 13, 7, order="permuted_none", lead=3, gap=2, tail=2)]
SCORE_CASES = SCORE_CLASSES + SCORE_PLANS + SCORE_HIDDEN + SCORE_INPUTS + SCORE_CHUNK + SCORE_COUNTS + SCORE_GRID + SCORE_COLS
SCORE_SUBSET_CASE = _score("subset", 9, 20, 5, 20, 23, order="permuted", lead=1, gap=1, tail=1)
BAD_LABEL_CASE = _score("bad_label", 6, 10, 3, 10, 5, order="after", tail=1)


# ---- the predictive call's cases ---------------------------------------------------------------------------------------
def _pred(name, F, H, C, B, n, order="none", lead=0, gap=0, tail=0):
    return {"name": name, "F": F, "H": H, "C": C, "B": B, "n": n, "order": _ORDERS[order], "lead": lead, "gap": gap, "tail": tail}


THREE_SLICES = 40       # three slices of 14, 14 and 12 particles at a batch of one row tile
PRED_CLASSES = [_pred("C%d" % C, 9, 20, C, 37, 19, order=("none", "permuted", "after")[i % 3], lead=i % 3, gap=i % 2, tail=i % 2)
                for i, C in enumerate(CLASS_COUNTS)]
PRED_HIDDEN = [_pred("H%d" % H, 4, H, 3, 21, 18) for H in (1, 15, 16, 17, 33)]
# staged pairs: the fewest the domain has (128 inputs x 32 classes), in between, and PR_PASS
PRED_STAGED = [_pred("F1", 1, 20, 3, 21, 18), _pred("F5", 5, 20, 3, 21, 18), _pred("F128C32", 128, 20, 32, 21, 5),
               _pred("F128C3", 128, 20, 3, 21, 5), _pred("F100", 100, 40, 7, 21, 5), _pred("covertype", 54, 100, 7, 50, 9)]
PRED_ROWS = [_pred("B%d" % B, 6, 10, 3, B, 21, lead=1) for B in (1, 255, 256, 257, 513)]
PRED_COUNTS = [_pred("n%d_C%d" % (n, C), 5, 20, C, 7, n) for C in (3, 32) for n in (1, 15, 16, 17, THREE_SLICES)]
PRED_CASES = PRED_CLASSES + PRED_HIDDEN + PRED_STAGED + PRED_ROWS + PRED_COUNTS
PRED_SUBSET_CASE = _pred("subsets", 9, 20, 7, 300, 37, order="permuted", lead=2, gap=1, tail=1)


def predict_args(case):
    rng = np.random.default_rng(zlib.crc32(("netclass-predict:" + case["name"]).encode()))
    cols, d = layout(case)
    theta = _theta(rng, case, case["n"], cols, d)
    return {"theta": theta, "X": _r32(rng.normal(size=(case["B"], case["F"]))),
            "labels": rng.integers(0, case["C"], size=case["B"]).astype(np.int32), "cols": cols, "d": d, "F": case["F"],
            "H": case["H"], "C": case["C"]}
