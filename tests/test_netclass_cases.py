"""CPU: the mirror of tests/netclass_cases.py holds the sources' constants and rules, both kernels' LDS fits a compute unit
over the whole domain, the tables reach every class of the dispatch and every edge the GPU tests promise, no score case has
more than 2 % of its entries under an ambiguous ReLU mask, and on every case a correct fp32 evaluation in the kernels'
summation order stays inside the references' allowances."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import netclass_cases as ncc  # noqa: E402
import netclass_ref as ncr  # noqa: E402
import predict_cases as pc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stein_amd", "csrc")
SHARE_CAP = 0.02          # the cap of tests/score_ref.py's network on the entries an ambiguous mask touches


def _const(text, name):
    m = re.search(r"constexpr int(?:64_t)? (?:\w+ = [^,;]+, )*%s = ([^,;]+)[,;]" % name, text)
    assert m, name
    return int(eval(m.group(1).replace("/", "//")))


def test_the_mirror_holds_the_sources_constants_and_rules():
    score = open(os.path.join(CSRC, "stein_score_bnn_class.hip")).read()
    for name in ("BC_R", "BC_LDS", "BC_PLDS", "BC_ROWS_MAX", "BC_MAX_WGS"):
        assert _const(score, name) == getattr(ncc, name), name
    dom = (ncc.NIN_MAX, ncc.C_MIN, ncc.C_MAX, ncc.H_MAX, ncc.W_MAX)
    assert tuple(_const(score, k) for k in ("BC_NIN_MAX", "BC_C_MIN", "BC_C_MAX", "BC_H_MAX", "BC_W_MAX")) == dom
    pred = open(os.path.join(CSRC, "stein_predict_bnn_class.hip")).read()
    assert tuple(_const(pred, k) for k in ("PC_NIN_MAX", "PC_C_MIN", "PC_C_MAX", "PC_H_MAX", "PC_W_MAX")) == dom
    fwd = open(os.path.join(CSRC, "stein_predict_fwd.h")).read()
    assert _const(fwd, "PR_WT") == ncc.PR_WT and _const(fwd, "PR_WIDE_LDS") == ncc.PR_WIDE_LDS
    for name in ("PR_ROWS", "PR_PASS", "PR_SLICE_CAP", "PR_TARGET_WGS"):
        assert _const(fwd, name) == getattr(pc, name), name
    # the launches the sources have are the mirror's instantiations
    assert tuple((int(a), int(b)) for a, b in re.findall(r"BC_LAUNCH\((\d+), (\d), \d\);", score)) == ncc.INSTANCES
    assert tuple(int(v) for v in re.findall(r"PC_LAUNCH\((\d+), \d\);", pred)) == ncc.PADDED
    from stein_amd import _lib
    assert (_lib.BNN_CLASS_NIN_MAX, _lib.BNN_CLASS_C_MIN, _lib.BNN_CLASS_C_MAX, _lib.BNN_CLASS_H_MAX, _lib.BNN_CLASS_W_MAX) == dom
    head = open(os.path.join(ROOT, "include", "steinhip.h")).read()
    for k, v in zip(("NIN_MAX", "C_MIN", "C_MAX", "H_MAX", "W_MAX"), dom):
        assert "STEIN_BNN_CLASS_%s = %d" % (k, v) in head
    for F, H, C in ((54, 100, 7), (13, 50, 3), (128, 64, 32), (4, 16, 3), (8, 512, 8)):      # the shapes the domain must admit
        assert ncc.in_domain(F, H, C), (F, H, C)


def test_the_lds_fits_over_the_whole_domain_and_the_plans_stay_in_their_classes():
    worst, fewest, staged, classes = 0, 1 << 30, set(), set()
    for C in (2, 4, 5, 9, 13, 17, 21, 25, 29, 32):     # (both plans see the class count through CS alone: every CS, and both ends)
        for F in range(1, ncc.NIN_MAX + 1):
            top = min(ncc.H_MAX, ncc.W_MAX // (F + ncc.cs_of(C)))
            assert ncc.in_domain(F, top, C) and not ncc.in_domain(F, top + 1, C)
            for H in range(1, top + 1):
                for B in (1, 1 << 20) if H % 16 else (1, 9, 100, 1 << 20):
                    p = ncc.score_plan(F, H, C, B)
                    assert p["crows"] >= ncc.BC_R and p["crows"] % ncc.BC_R == 0 and (p["lh"], p["kh"]) in ncc.INSTANCES, (F, H, C, B)
                    assert p["lh"] * p["kh"] >= H and 8 * ncc.cs_of(C) <= 256
                    assert 4 * p["lds_words"] <= 4 * ncc.BC_LDS <= 158 * 1024, (F, H, C, B)
                    assert p["ppw"] == 1 or p["ppw"] * ncc.particle_floats(F, H, C) <= ncc.BC_PLDS
                    worst = max(worst, p["lds_words"])
                    classes.add((p["lh"], p["kh"], p["bumped"]))
                fewest = min(fewest, ncc.score_chunk_rows(F, H, C))
                q = ncc.predict_plan(F, H, C, 100, 100)
                assert 1 <= q["ps"] <= pc.PR_PASS and q["lds_words"] <= ncc.PR_WIDE_LDS and 4 * ncc.PR_WIDE_LDS < 160 * 1024
                assert q["ld"] % 2 == 1
                staged.add(q["ps"])
    assert worst > ncc.BC_LDS - 200           # the budget is used where the weights leave little room
    assert fewest == ncc.score_chunk_rows(*ncc.SMALLEST_CHUNK) == 24
    assert min(staged) == 2 and max(staged) == pc.PR_PASS      # the X tile of 128 inputs leaves room for two pairs, never one
    assert len(classes) == 6


def test_the_score_tables_reach_every_class_of_the_dispatch():
    plans = {c["name"]: ncc.score_plan(c["F"], c["H"], c["C"], c["B"]) for c in ncc.SCORE_CASES}
    assert len(plans) == len(ncc.SCORE_CASES)                                   # names are unique
    for c in ncc.SCORE_CASES + [ncc.SCORE_SUBSET_CASE, ncc.BAD_LABEL_CASE]:
        assert ncc.in_domain(c["F"], c["H"], c["C"]), c["name"]
    assert tuple(c["C"] for c in ncc.SCORE_CLASSES) == ncc.CLASS_COUNTS
    # every instantiation, and every one the LDS reaches by giving up particles per workgroup
    assert {(p["lh"], p["kh"], p["bumped"]) for p in plans.values()} == {(64, 1, False), (128, 1, False), (128, 1, True), (256, 1, False),
                                                                        (256, 1, True), (256, 2, False)}
    assert {c["H"] for c in ncc.SCORE_CASES} >= {1, 15, 16, 17, 65, 100, 200, 300, 512}
    assert any(c["H"] % plans[c["name"]]["lh"] for c in ncc.SCORE_CASES if plans[c["name"]]["kh"] == 2)
    assert {c["F"] for c in ncc.SCORE_CASES} >= {1, 5, 128}
    # chunks: one row, around one chunk, two chunks and a row, at the shape with the fewest rows per chunk
    ch = ncc.score_chunk_rows(*ncc.SMALLEST_CHUNK)
    edge = [c for c in ncc.SCORE_CHUNK if (c["F"], c["H"], c["C"]) == ncc.SMALLEST_CHUNK]
    assert [c["B"] for c in edge] == [1, ch - 1, ch, ch + 1, 2 * ch + 1]
    assert all(plans[c["name"]]["crows"] == min(ch, (c["B"] + 7) & ~7) for c in edge)
    assert max(p["lds_words"] for p in plans.values()) > ncc.BC_LDS - 300
    # particles per workgroup and the counts around them; the grid-strided loop goes round twice
    for ppw, counts in ((4, {1, 3, 4, 5}), (2, {1, 2, 3}), (1, {1, 2})):
        assert {c["n"] for c in ncc.SCORE_COUNTS if plans[c["name"]]["ppw"] == ppw} == counts, ppw
    g = ncc.SCORE_GRID[0]
    assert g["n"] == plans[g["name"]]["ppw"] * ncc.BC_MAX_WGS + 1 and g["F"] * g["H"] * g["C"] <= 16
    assert all(c["n"] <= 40 for c in ncc.SCORE_CASES if c not in ncc.SCORE_GRID)
    # the blocks' places
    lay = {c["name"]: ncc.layout(c)[0] for c in ncc.SCORE_COLS}
    assert lay["cols_before"][4] < min(lay["cols_before"][:4]) and lay["cols_after"][4] > max(lay["cols_after"][:4])
    assert lay["cols_permuted_none"][4] == -1 and lay["cols_permuted"][0] > lay["cols_permuted"][4] > lay["cols_permuted"][2]
    for c in ncc.SCORE_COLS:
        live = ncc.live_columns(c)
        assert not live[0] and not live[-1] and (~live).sum() >= 5 + len(c["order"])      # foreign columns before, between, after
    assert {len(c["order"]) for c in ncc.SCORE_CASES} == {4, 5}


def test_the_predictive_tables_reach_every_instantiation_unit_row_tile_and_count():
    names = [c["name"] for c in ncc.PRED_CASES]
    assert len(set(names)) == len(names)
    for c in ncc.PRED_CASES + [ncc.PRED_SUBSET_CASE]:
        assert ncc.in_domain(c["F"], c["H"], c["C"]), c["name"]
    plans = {c["name"]: ncc.predict_plan(c["F"], c["H"], c["C"], c["n"], c["B"]) for c in ncc.PRED_CASES}
    assert tuple(c["C"] for c in ncc.PRED_CLASSES) == ncc.CLASS_COUNTS
    assert {c["H"] for c in ncc.PRED_HIDDEN} == {1, 15, 16, 17, 33} and {plans[c["name"]]["tiles"] for c in ncc.PRED_HIDDEN} == {1, 2, 3}
    assert {c["F"] for c in ncc.PRED_STAGED} >= {1, 5, 128}
    staged = {plans[c["name"]]["ps"] for c in ncc.PRED_STAGED}
    assert min(staged) == 2 and max(staged) == pc.PR_PASS and len(staged) >= 4       # the domain's fewest, in between, PR_PASS
    # a unit that ends inside a particle, and one that holds several whole particles
    assert any(plans[c["name"]]["ps"] % plans[c["name"]]["tiles"] for c in ncc.PRED_STAGED)
    assert any(plans[c["name"]]["ps"] >= 2 * plans[c["name"]]["tiles"] for c in ncc.PRED_CASES)
    assert max(4 * p["lds_words"] for p in plans.values()) > 150 * 1024
    assert {c["B"] for c in ncc.PRED_ROWS} == {1, 255, 256, 257, 513}
    for C in (3, 32):
        assert {c["n"] for c in ncc.PRED_COUNTS if c["C"] == C} == {1, 15, 16, 17, ncc.THREE_SLICES}
    p = ncc.predict_plan(5, 20, 3, ncc.THREE_SLICES, 7)
    assert p["slices"] == 3 and 0 < ncc.THREE_SLICES - 2 * p["per"] < p["per"]
    for c in ncc.PRED_CASES + [ncc.PRED_SUBSET_CASE]:
        q = ncc.predict_plan(c["F"], c["H"], c["C"], c["n"], c["B"])
        assert q["slices"] * c["B"] * (c["C"] + 2) * 4 <= ncc.predict_workspace_bytes(c["n"], c["B"], c["C"])
        assert c["n"] <= 40 and c["B"] <= 513


@pytest.mark.parametrize("case", ncc.SCORE_CASES + [ncc.SCORE_SUBSET_CASE], ids=lambda c: c["name"])
def test_score_fp32_emulation_stays_inside_the_allowance_and_few_masks_are_ambiguous(case):
    a = ncc.score_args(case)
    args = (a["theta"], a["F"], a["H"], a["C"], a["cols"], a["X"], a["labels"], a["scale"], a["prior_precision"], a["gamma_rate"])
    ref, allow, share = ncr.score(*args)
    assert np.isfinite(ref).all() and np.isfinite(allow).all()
    assert share <= SHARE_CAP, share                  # a condition on the inputs: the seeds and scales of netclass_cases.py
    live = ncc.live_columns(case)
    got = ncr.score_f32(*args)
    assert (got[:, ~live] == 0).all() and (ref[:, ~live] == 0).all() and (allow[:, live] > 0).all()
    ratio = (np.abs(got.astype(np.float64) - ref)[:, live] / allow[:, live]).max()
    print("%-18s ambiguous share %.4f  max |err| / allowance = %.3f" % (case["name"], share, ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize("case", ncc.PRED_CASES, ids=lambda c: c["name"])
def test_predict_fp32_emulation_stays_inside_the_allowance(case):
    a = ncc.predict_args(case)
    per = ncc.predict_plan(case["F"], case["H"], case["C"], case["n"], case["B"])["per"]
    args = (a["theta"], a["F"], a["H"], a["C"], a["cols"], a["X"], a["labels"], per)
    ref = ncr.predict(*args)
    got = ncr.predict_f32(*args)
    for k in ("pred_link", "pred_mean", "prob", "lpd", "ent"):
        val, allow = ref[k]
        assert np.isfinite(val).all() and np.isfinite(allow).all() and (allow > 0).all(), k
        ratio = (np.abs(np.asarray(got[k], np.float64) - val) / allow).max()
        print("%-12s %-9s max |err| / allowance = %.3f" % (case["name"], k, ratio))
        assert ratio <= 1.0, k
    # and the tighter allowances against statistics of the emulation's own outputs
    own = ncr.summaries(got["pred_link"].astype(np.float64), None, a["labels"], per, tight=True)
    own.update(ncr.summaries_of_probs(got["pred_mean"].astype(np.float64), a["labels"], per))
    for k in ("prob", "lpd", "ent"):
        val, allow = own[k]
        assert (allow <= ref[k][1]).all(), k
        assert (np.abs(np.asarray(got[k], np.float64) - val) <= allow).all(), k
