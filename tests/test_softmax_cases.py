"""CPU: the mirror of tests/softmax_cases.py holds the sources' constants and rules, every kernel's LDS fits a compute unit
over the whole domain, the tables reach every instantiation and every edge the GPU tests promise, and on every case of the
tables a correct fp32 evaluation in the kernels' summation order stays inside the references' allowances."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_cases as pc  # noqa: E402
import softmax_cases as smc  # noqa: E402
import softmax_ref as smr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stein_amd", "csrc")


def _const(text, name):
    m = re.search(r"constexpr int(?:64_t)? (?:\w+ = [^,;]+, )*%s = ([^,;]+)[,;]" % name, text)
    assert m, name
    return int(eval(m.group(1).replace("/", "//")))


def test_the_mirror_holds_the_sources_constants_and_rules():
    score = open(os.path.join(CSRC, "stein_score_softmax.hip")).read()
    for name in ("SM_LDS", "SM_WLDS", "SM_ROWS_MAX", "SM_MAX_WGS"):
        assert _const(score, name) == getattr(smc, name), name
    assert tuple(_const(score, k) for k in ("SM_C_MIN", "SM_C_MAX", "SM_F_MAX", "SM_FC_MAX")) == (smc.C_MIN, smc.C_MAX, smc.F_MAX, smc.FC_MAX)
    pred = open(os.path.join(CSRC, "stein_predict_softmax.hip")).read()
    assert tuple(_const(pred, k) for k in ("PS_C_MIN", "PS_C_MAX", "PS_FC_MAX")) == (smc.C_MIN, smc.C_MAX, smc.FC_MAX)
    fwd = open(os.path.join(CSRC, "stein_predict_fwd.h")).read()
    for name in ("PR_ROWS", "PR_PASS", "PR_FC", "PR_SLICE_CAP", "PR_TARGET_WGS"):
        assert _const(fwd, name) == getattr(pc, name), name
    assert _const(fwd, "PR_WIDTH_MAX") == smc.F_MAX
    # the launches the sources have are the mirror's instantiations
    assert tuple(int(v) for v in re.findall(r"SM_LAUNCH\((\d+), \d\);", score)) == smc.PADDED
    assert tuple(int(v) for v in re.findall(r"PS_LAUNCH\((\d+), \d\);", pred)) == smc.PADDED
    from stein_amd import _lib
    assert (_lib.SOFTMAX_C_MIN, _lib.SOFTMAX_C_MAX, _lib.SOFTMAX_F_MAX, _lib.SOFTMAX_FC_MAX) == (smc.C_MIN, smc.C_MAX, smc.F_MAX, smc.FC_MAX)


def test_the_lds_fits_over_the_whole_domain_and_a_chunk_holds_a_row():
    worst = 0
    for C in range(smc.C_MIN, smc.C_MAX + 1):
        top = min(smc.F_MAX, smc.FC_MAX // C)
        for F in sorted({1, 2, 3, 7, 54, 58, 59, 100, 255, 256, 512, top - 1, top} | set(range(1, top + 1, 37))):
            if F < 1:
                continue
            for B in (1, 3, 100, 1 << 20):
                p = smc.score_plan(F, C, B)
                assert p["crows"] >= 1 and p["ppw"] in (1, 2, 4) and p["G"] in (1, 2, 4, 8, 16, 32, 64), (F, C, B)
                assert 4 * p["lds_words"] <= 4 * smc.SM_LDS <= 158 * 1024, (F, C, B)
                assert p["ppw"] == 1 or 2 * p["ppw"] * F * ((C + 3) & ~3) <= smc.SM_WLDS
                worst = max(worst, p["lds_words"])
            q = smc.predict_plan(F, C, 100, 100)
            assert 4 * q["lds_words"] <= 80 * 1024 and q["ld"] % 2 == 1 and q["pp"] * q["cp"] in (16, 32)
    assert worst > smc.SM_LDS - 1100          # the budget is used where the weights leave little room


def test_the_score_tables_reach_every_instantiation_edge_chunk_count_and_grid():
    plans = {c["name"]: smc.score_plan(c["F"], c["C"], c["B"]) for c in smc.SCORE_CASES}
    assert len(plans) == len(smc.SCORE_CASES)                                   # names are unique
    for c in smc.SCORE_CASES + [smc.SCORE_SUBSET_CASE, smc.BAD_LABEL_CASE]:
        assert smc.C_MIN <= c["C"] <= smc.C_MAX and 1 <= c["F"] <= smc.F_MAX and c["F"] * c["C"] <= smc.FC_MAX
    assert tuple(c["C"] for c in smc.SCORE_CLASSES) == smc.CLASS_COUNTS
    for cp in smc.PADDED:       # both ends of every instantiation: its largest count, and one past the one below
        ends = {c["C"] for c in smc.SCORE_CLASSES if smc.padded(c["C"]) == cp}
        assert cp in ends and (min(ends) == 2 if cp == 4 else min(ends) == cp // 2 + 1), cp
    assert {(c["F"], c["C"]) for c in smc.SCORE_FEATS} >= {(1, 3), (7, 3), (54, 7), (512, 32)}
    assert {c["alpha"] for c in smc.SCORE_CLASSES} == {"none", "before", "after"}
    # chunks: one row, around one and two chunks, three chunks and a row
    ch = smc.score_chunk_rows(512, 32)
    assert ch == 14 and [c["B"] for c in smc.SCORE_CHUNK] == [1, ch - 1, ch, ch + 1, 2 * ch - 1, 2 * ch, 2 * ch + 1, 3 * ch + 1]
    assert all(plans[c["name"]]["crows"] == min(ch, c["B"]) for c in smc.SCORE_CHUNK)
    # particles per workgroup and the counts around them; the grid-stride loop goes round twice for each
    for ppw, counts in ((4, {1, 3, 4, 5}), (2, {1, 2, 3}), (1, {1, 2})):
        assert {c["n"] for c in smc.SCORE_COUNTS if plans[c["name"]]["ppw"] == ppw} == counts, ppw
    assert sorted((plans[c["name"]]["ppw"], c["n"]) for c in smc.SCORE_GRID) == [(p, p * smc.SM_MAX_WGS + 1) for p in (1, 2, 4)]
    assert all(c["n"] <= plans[c["name"]]["ppw"] * smc.SM_MAX_WGS for c in smc.SCORE_CASES if c not in smc.SCORE_GRID)
    # lanes per row: every power of two
    assert {plans[c["name"]]["G"] for c in smc.SCORE_LANES} == {1, 2, 4, 8, 16, 32, 64}
    assert {plans[c["name"]]["G"] for c in smc.SCORE_LANES if plans[c["name"]]["ppw"] == 1} == {64}
    # the weights' place
    lay = {c["name"]: smc.layout(c) for c in smc.SCORE_COLS}
    assert all(w > 0 for w, _, _ in lay.values())
    assert lay["cols_before"][1] < lay["cols_before"][0] and lay["cols_after"][1] > lay["cols_after"][0] and lay["cols_none"][1] == -1
    for c in smc.SCORE_COLS:
        assert (~smc.live_columns(c)).sum() >= 3                                 # foreign columns


def test_the_predictive_tables_reach_every_instantiation_chunking_row_tile_and_count():
    names = [c["name"] for c in smc.PRED_CASES]
    assert len(set(names)) == len(names)
    assert tuple(c["C"] for c in smc.PRED_CLASSES) == smc.CLASS_COUNTS
    assert {smc.predict_plan(c["F"], c["C"], c["n"], c["B"])["chunks"] for c in smc.PRED_FEATS} == {1, 2, 3}
    assert {c["F"] for c in smc.PRED_FEATS} == {1, 58, 59, 117}
    # the 32-class kernel on both sides of the 64 KB a kernel gets without asking
    big = [4 * smc.predict_plan(c["F"], c["C"], c["n"], c["B"])["lds_words"] for c in smc.PRED_FEATS if c["C"] == 32]
    assert max(big) > 64 * 1024
    assert {c["B"] for c in smc.PRED_ROWS} == {1, 255, 256, 257, 513}
    for C in (3, 8, 16, 32):
        assert {c["n"] for c in smc.PRED_COUNTS if c["C"] == C} == {1, 15, 16, 17, smc.THREE_SLICES}
    p = smc.predict_plan(5, 3, smc.THREE_SLICES, 7)
    assert p["slices"] == 3 and 0 < smc.THREE_SLICES - 2 * p["per"] < p["per"] and p["per"] % p["pp"] != 0
    assert {smc.predict_plan(5, c["C"], c["n"], c["B"])["pp"] for c in smc.PRED_COUNTS} == {4, 2, 1}
    for c in smc.PRED_CASES + [smc.PRED_SUBSET_CASE]:
        q = smc.predict_plan(c["F"], c["C"], c["n"], c["B"])
        assert q["slices"] * c["B"] * (c["C"] + 2) * 4 <= smc.predict_workspace_bytes(c["n"], c["B"], c["C"])


@pytest.mark.parametrize("case", smc.SCORE_CASES, ids=lambda c: c["name"])
def test_score_fp32_emulation_stays_inside_the_allowance(case):
    a = smc.score_args(case)
    args = (a["theta"], a["w_col"], a["F"], a["C"], a["alpha_col"], a["X"], a["labels"], a["scale"], a["prior_precision"], a["gamma_rate"])
    ref, allow = smr.score(*args)
    assert np.isfinite(ref).all() and np.isfinite(allow).all()
    live = smc.live_columns(case)
    got = smr.score_f32(*args, G=smc.score_plan(case["F"], case["C"], case["B"])["G"])
    assert (got[:, ~live] == 0).all() and (ref[:, ~live] == 0).all() and (allow[:, live] > 0).all()
    ratio = (np.abs(got.astype(np.float64) - ref)[:, live] / allow[:, live]).max()
    print("%-16s max |err| / allowance = %.3f" % (case["name"], ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize("case", smc.PRED_CASES, ids=lambda c: c["name"])
def test_predict_fp32_emulation_stays_inside_the_allowance(case):
    a = smc.predict_args(case)
    per = smc.predict_plan(case["F"], case["C"], case["n"], case["B"])["per"]
    ref = smr.predict(a["theta"], a["w_col"], a["F"], a["C"], a["X"], a["labels"], per)
    got = smr.predict_f32(a["theta"], a["w_col"], a["F"], a["C"], a["X"], a["labels"], per)
    for k in ("pred_link", "pred_mean", "prob", "lpd", "ent"):
        val, allow = ref[k]
        assert np.isfinite(val).all() and np.isfinite(allow).all() and (allow > 0).all(), k
        ratio = (np.abs(np.asarray(got[k], np.float64) - val) / allow).max()
        print("%-12s %-9s max |err| / allowance = %.3f" % (case["name"], k, ratio))
        assert ratio <= 1.0, k
    # and the tighter allowances against statistics of the emulation's own outputs
    own = smr.summaries(got["pred_link"].astype(np.float64), None, a["labels"], per, tight=True)
    own.update(smr.summaries_of_probs(got["pred_mean"].astype(np.float64), a["labels"], per))
    for k in ("prob", "lpd", "ent"):
        val, allow = own[k]
        assert (allow <= ref[k][1]).all(), k
        assert (np.abs(np.asarray(got[k], np.float64) - val) <= allow).all(), k
