"""CPU: the tables of tests/bnn_wide_cases.py reach every instantiation of the wide network kernels and both sides of every
edge of their dispatch rules; the mirror's constants are the sources'; and on the cases small enough for the CPU a correct
fp32 evaluation stays inside the references' a-priori allowances, the ambiguous-ReLU share stays under the cap the GPU test
treats as a precondition, and the heavy rows at the chunk edges cannot go unnoticed."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bnn_wide_cases as wc  # noqa: E402
import predict_cases as pc  # noqa: E402
import score_cases as sc  # noqa: E402
import score_ref as sr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stein_amd", "csrc")
MAX_AMBIGUOUS = 0.02


def _const(text, name):
    m = re.search(r"constexpr int(?:64_t)? (?:\w+ = [^,;]+, )*%s = ([^,;]+)[,;]" % name, text)
    assert m, name
    return int(eval(m.group(1).replace("/", "//")))


def test_the_mirror_holds_the_sources_constants_and_rules():
    score = open(os.path.join(CSRC, "stein_score_wide.hip")).read()
    for name in ("SW_R", "SW_XLDS", "SW_WLDS", "SW_MAX_WGS"):
        assert _const(score, name) == getattr(wc, name), name
    assert (_const(score, "SW_NIN_MAX"), _const(score, "SW_H_MAX"), _const(score, "SW_W1_MAX")) == (wc.NIN_MAX, wc.H_MAX, wc.W1_MAX)
    fwd = open(os.path.join(CSRC, "stein_predict_fwd.h")).read()
    for name in ("PR_WT", "PR_WIDE_LDS"):
        assert _const(fwd, name) == getattr(wc, name), name
    assert (_const(fwd, "PR_WIDE_NIN_MAX"), _const(fwd, "PR_WIDE_W1_MAX"), _const(fwd, "PR_NIN_MAX")) == (wc.NIN_MAX, wc.W1_MAX, wc.NARROW_MAX)
    # the launches the source has are the mirror's instantiations
    assert set(re.findall(r"SW_LAUNCH\((\d+), (\d+), \d\)", score)) == {(str(a), str(b)) for a, b in wc.SCORE_KERNELS}
    # every kernel's LDS fits a compute unit over the whole domain, and a chunk holds at least one row block
    for n_in in range(wc.NARROW_MAX + 1, wc.NIN_MAX + 1):
        assert wc.score_chunk_rows(n_in) >= wc.SW_R and wc.score_chunk_rows(n_in) % wc.SW_R == 0
        for H in {1, 16, 17, 64, 65, 128, 129, 256, 257, 1024, wc.W1_MAX // n_in} | set(range(1, 140, 7)):
            if H > wc.H_MAX or n_in * H > wc.W1_MAX:
                continue
            lh, kh = wc.score_kernel(n_in, H)
            assert (lh, kh) in wc.SCORE_KERNELS and lh * kh >= H
            words = 2 * (-(-(256 // lh) * n_in * H // 4) * 4) + wc.score_chunk_rows(n_in) * (n_in + 1) + 2 * 4 * wc.SW_R + 4
            assert 4 * words <= 160 * 1024, (n_in, H)
        ld, ps, nbytes = wc.predict_tile(n_in)
        assert ld % 2 == 1 and ld >= n_in and 1 <= ps <= pc.PR_PASS
        assert nbytes <= 4 * wc.PR_WIDE_LDS and nbytes + 256 <= 160 * 1024, n_in
        assert ps == pc.PR_PASS or nbytes + 4 * (n_in + 2) * wc.PR_WT > 4 * wc.PR_WIDE_LDS       # as many particles as fit


def test_the_tables_stay_inside_the_domain_and_names_are_unique():
    for table in (wc.SCORE_CASES, wc.PRED_CASES + [wc.PRED_SUBSET_CASE] + [wc.PRED_WEIGHTED[0][0], wc.PRED_WEIGHTED[-1][0]]):
        names = [c["name"] for c in table]
        assert len(set(names)) == len(names)
        for c in table:
            assert wc.NARROW_MAX < c["n_in"] <= wc.NIN_MAX and c["H"] <= wc.H_MAX and c["n_in"] * c["H"] <= wc.W1_MAX, c["name"]


def test_the_score_tables_reach_every_instantiation_edge_chunk_and_grid():
    assert {wc.score_kernel(c["n_in"], c["H"]) for c in wc.SCORE_CASES} == set(wc.SCORE_KERNELS)
    have = {(c["n_in"], c["H"]) for c in wc.SCORE_CASES}
    for lo, hi in wc.SCORE_EDGE_PAIRS:
        assert lo in have and hi in have and wc.score_kernel(*lo) != wc.score_kernel(*hi), (lo, hi)
    assert {wc.score_kernel(*p) for pair in wc.SCORE_EDGE_PAIRS for p in pair} == set(wc.SCORE_KERNELS)
    # the LDS edges are edges of n_in * H, not of H: the same H on both sides
    assert wc.score_kernel(72, 64) == (64, 1) and wc.score_kernel(73, 64) == (128, 1)
    assert wc.score_kernel(72, 128) == (128, 1) and wc.score_kernel(73, 128) == (256, 1)
    assert wc.score_kernel(90, 100) == (128, 1)              # the Year set's network: two particles per workgroup
    for n_in in (5, 127):       # the widest and the narrowest chunk; one, two and three chunks and one row past them
        c = wc.score_chunk_rows(n_in)
        assert {k["B"] for k in wc.SCORE_CHUNK if k["n_in"] == n_in} == {c - 1, c, c + 1, 2 * c, 3 * c + 1}
    assert (wc.score_chunk_rows(5), wc.score_chunk_rows(127), wc.score_chunk_rows(128)) == (592, 24, 24)
    # row blocks: batches below, at and past a block of SW_R rows
    assert {wc.SW_R - 1, wc.SW_R, wc.SW_R + 1} <= {c["B"] for c in wc.SCORE_CASES}
    lanes = set()
    for c in wc.SCORE_GRID:     # every grid-stride loop goes round twice, for every number of particles per workgroup
        cap = wc.score_grid_cap(c["n_in"], c["H"])
        assert cap < c["n"] <= cap + 16
        lanes.add(wc.score_kernel(c["n_in"], c["H"])[0])
    assert lanes == {64, 128, 256}
    assert all(c["n"] <= wc.score_grid_cap(c["n_in"], c["H"]) for c in wc.SCORE_CASES if c not in wc.SCORE_GRID)
    assert {c["flavor"] for c in wc.SCORE_CASES} == {"plain", "dead", "saturated", "chunk"}


def test_the_predictive_tables_reach_every_staging_unit_edge_count_and_row_tile():
    have = {(c["n_in"], c["H"]) for c in wc.PRED_CASES}
    for lo, hi in wc.PRED_EDGE_PAIRS:
        assert lo in have and hi in have
        assert wc.predict_tile(lo[0])[1] != wc.predict_tile(hi[0])[1], (lo, hi)
    assert [wc.predict_tile(n_in)[1] for n_in in (5, 13, 78, 79, 90, 127, 128)] == [16, 16, 16, 15, 11, 4, 3]
    units = set()               # hidden units: one staging unit exactly, one hidden unit past it, more than two units
    for c in wc.PRED_CASES:
        units |= {"one" if c["H"] == wc.PR_WT else "one+1" if c["H"] == wc.PR_WT + 1 else "3+" if c["H"] > 2 * wc.PR_WT else ""}
    assert {"one", "one+1", "3+"} <= units and min(c["H"] for c in wc.PRED_CASES) < wc.PR_WT
    for n_in in (79, 90, 128):  # fewer than PR_PASS particles per staging unit: counts below, at and past it, and two units
        ps = wc.predict_tile(n_in)[1]
        ns = {c["n"] for c in wc.PRED_CASES if c["n_in"] == n_in}
        assert ps < pc.PR_PASS and {ps - 1, ps, ps + 1} & ns and any(n > 2 * ps for n in ns), (n_in, ps, ns)
    ns = {c["n"] for c in wc.PRED_COUNTS}
    assert {1, pc.PR_PASS - 1, pc.PR_PASS, pc.PR_PASS + 1, 2 * pc.PR_PASS + 1} <= ns
    assert max(pc.plan(c["n"], c["B"])[1] for c in wc.PRED_COUNTS) >= 32          # many slices
    assert {1, pc.PR_ROWS - 1, pc.PR_ROWS, pc.PR_ROWS + 1, 2 * pc.PR_ROWS + 3} <= {c["B"] for c in wc.PRED_ROWS}


SCORE_CPU = [c for c in wc.SCORE_CASES if wc.cpu_sized(c)]
PRED_CPU = [c for c in wc.PRED_CASES if wc.cpu_sized(c)]


def test_most_cases_are_small_enough_for_the_cpu():
    assert len(SCORE_CPU) >= len(wc.SCORE_CASES) - 4 and len(PRED_CPU) >= len(wc.PRED_CASES) - 2


@pytest.mark.parametrize("case", SCORE_CPU, ids=lambda c: c["name"])
def test_score_fp32_emulation_stays_inside_the_allowance(case):
    a = wc.score_args(case)
    ref, allow, share = sc.reference(case, a)
    assert np.isfinite(ref).all() and np.isfinite(allow).all()
    assert share <= MAX_AMBIGUOUS, share
    got = sr.bnn_score_f32(a["theta"], a["n_in"], a["H"], a["cols"], a["X"], a["y"], a["n_train"], a["ga"], a["gb"])
    live = sc.live_columns(case, a)
    err = np.abs(got.astype(np.float64) - ref)
    assert (got[:, ~live] == 0).all() and (ref[:, ~live] == 0).all()
    ratio = (err[:, live] / allow[:, live]).max()
    print("%-24s max |err| / allowance = %.3f   ambiguous share %.5f" % (case["name"], ratio, share))
    assert ratio <= 1.0
    if case["flavor"] in ("dead", "saturated"):
        sc.check_extreme_inputs(case, a)


@pytest.mark.parametrize("case", wc.SCORE_CHUNK, ids=lambda c: c["name"])
def test_heavy_rows_at_the_chunk_edges_cannot_go_unnoticed(case):
    a = wc.score_args(case)
    rows = wc.heavy_rows(case["B"], case["n_in"])
    c = wc.score_chunk_rows(case["n_in"])
    assert 0 in rows and case["B"] - 1 in rows and all(e - 1 in rows and e in rows for e in range(c, case["B"], c))
    shares = wc.heavy_row_shares(case, a)                    # from the reference alone
    assert len(shares) == len(rows) and min(shares) >= 0.9, shares


@pytest.mark.parametrize("case", PRED_CPU, ids=lambda c: c["name"])
def test_predict_fp32_emulation_stays_inside_the_allowance(case):
    a = pc.args(case)
    ref, got = pc.reference(case, a), pc.emulate_f32(case, a)
    for k in ("pred", "mean", "var", "lpd"):
        val, allow = ref[k]
        assert np.isfinite(val).all() and np.isfinite(allow).all()
        err = np.abs(np.asarray(got[k], np.float64) - val)
        pos = allow > 0
        ratio = (err[pos] / allow[pos]).max() if pos.any() else 0.0
        print("%-16s %-4s max |err| / allowance = %.3f" % (case["name"], k, ratio))
        assert (err <= allow).all(), (k, ratio)
