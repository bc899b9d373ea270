"""CPU: tests/wquantile_cases.py is what tests/test_gpu_predict_wranks.py takes it for -- its model of the weighted select,
at every digit width, is the definition (sorted cumulative masses), which is np.sort(np.repeat(f, c))[t] for counts and
NumPy's weighted "inverted_cdf" quantile; the half-step level selects its target for every M below 2^32; the default digit
widths are the source's rule restated; the table reaches every arm the unweighted table reaches; the constants are the
source's."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_cases as pc  # noqa: E402
import quantile_cases as qc  # noqa: E402
import wquantile_cases as wq  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_are_the_sources():
    src = open(os.path.join(ROOT, "stein_amd", "csrc", "stein_predict_ranks.hip")).read()
    hdr = open(os.path.join(ROOT, "include", "steinhip.h")).read()
    assert int(re.search(r"constexpr int PQW_MPARTS = (\d+);", src).group(1)) == wq.PQW_MPARTS
    assert int(re.search(r"constexpr int PQW_CUS = (\d+);", src).group(1)) == wq.PQW_CUS
    assert int(re.search(r"constexpr int PM_BLOCKS = (\d+);", src).group(1)) == wq.PM_BLOCKS
    assert re.search(r"PQW_LDS_CU = 160 \* 1024;", src) and wq.PQW_LDS_CU == 160 * 1024
    assert "2147483648.0" in src and wq.MASS_SCALE == 2147483648
    assert "%d bytes + %d per (row, level)" % (8 * wq.PQW_MPARTS, 4 * qc.PQ_WORDS) in hdr
    assert re.search(r"enum \{ STEIN_MASS_NORMALISED = 0, STEIN_MASS_COUNTS = 1 \};", hdr)
    # the unweighted select's constants keep their text
    assert "constexpr int PQ_BITS = 4" in src and "constexpr int PQ_FLUSH = 15" in src
    assert "constexpr int PQ_WORDS = 3 + PQ_BINS;" in src and "PQ_LDS_HALF_CU = 80 * 1024;" in src
    assert re.search(r"enum \{ STEIN_PRED_RANKS_MAX = 8 \};", hdr)
    # one forward pass and one counting kernel per model: a single call site of each slice walk, whatever is counted
    assert src.count("pred_glm_slice(") == 1 and src.count("pred_bnn_pass<NIN>(") == 1
    assert "k_predict_glm_wranks" not in src and "k_predict_bnn_wranks" not in src
    assert src.count("void k_predict_glm_ranks(") == 1 and src.count("void k_predict_bnn_ranks(") == 1
    assert "template <bool MASS, class... Mass>\n__global__" in src
    assert "template <int NIN, bool MASS, class... Mass>\n__global__" in src
    # integer atomics only: no atomic on a float or a double anywhere in the file
    code = re.sub(r"//[^\n]*", "", src)
    for m in re.finditer(r"atomicAdd\(([^;]*);", code):
        assert "float" not in m.group(1) and "double" not in m.group(1)
    assert "atomicAdd" not in code[code.index("k_rank_masses_wsum"):]                      # the masses pass: none at all


def test_the_model_is_the_definition_at_every_width():
    rng = np.random.default_rng(3)
    for name, w in qc.planted():
        f = qc.planted_products(w)
        for mname, masses in wq.planted_masses(w):
            targets = wq.planted_targets(masses)
            pick = [targets[i] for i in sorted(set(rng.integers(0, len(targets), size=12)) | {0, len(targets) - 1})]
            for b in (0, 3):
                want = wq.by_definition(f[:, b], masses, pick)
                for bits in (1, 2, 3, 4):
                    got = wq.weighted_select(f[:, b], masses, pick, bits)
                    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, mname, b, bits)


def test_counts_are_np_repeat_and_numpys_inverted_cdf():
    for name, w in qc.planted():
        f = qc.planted_products(w)
        masses = dict(wq.planted_masses(w))
        for mname in ("ones", "counts", "one_hot_middle", "zero_on_nans"):
            if mname not in masses:
                continue
            c = masses[mname].astype(np.int64)
            M = int(c.sum())
            for b in range(qc.PLANT_B):
                rep = np.sort(np.repeat(f[:, b], c))                                      # NaNs last
                got = wq.weighted_select(f[:, b], c, range(M))
                assert np.array_equal(got, rep, equal_nan=True), (name, mname, b)
        # NumPy's own weighted quantile (no NaNs, no zero weights: it sorts by value and keeps zero-weight atoms)
        if not np.isnan(w).any():
            c = masses["counts"].astype(np.int64)
            live = c > 0
            M = int(c.sum())
            for q in wq.LEVELS:
                want = np.quantile(f[live, 1].astype(np.float64), q, weights=c[live], method="inverted_cdf")
                got = wq.weighted_select(f[:, 1], c, [wq.target(q, M)])[0]
                assert float(got) == float(want), (name, q)


def test_ones_are_the_unweighted_select():
    for name, w in qc.planted():
        f = qc.planted_products(w)[:, 2]
        got = wq.weighted_select(f, np.ones(qc.PLANT_N, np.uint64), range(qc.PLANT_N), bits=2)
        assert np.array_equal(got.view(np.uint32), qc.radix_select(f, range(qc.PLANT_N)).view(np.uint32)), name


def test_half_step_level_selects_its_target_for_every_total():
    rng = np.random.default_rng(17)
    top = 2 ** 32 - 1
    Ms = np.concatenate([np.arange(1, 300), 2 ** np.arange(8, 32), 2 ** np.arange(8, 33) - 1, 2 ** np.arange(8, 32) + 1,
                         rng.integers(1, top, size=4000), [top, top - 1, 2 ** 31 + 18]]).astype(np.int64)
    for M in Ms:
        M = int(M)
        ts = {0, 1, M // 2, M - 2, M - 1} | {int(t) for t in rng.integers(0, M, size=8)}
        ts |= set(range(M)) if M < 300 else set()
        for t in ts:
            if 0 <= t < M:
                assert wq.target(wq.half_step(t, M), M) == t, (t, M)
    assert wq.target(0.0, 5) == 0 and wq.target(1.0, 5) == 4 and wq.target(1.0, top) == top - 1
    assert wq.target(0.2, 5) == 0 and wq.target(0.2000001, 5) == 1 and wq.target(1e-300, top) == 0


def test_default_digit_widths_restate_the_rule():
    big = 2048                                                                           # a grid that fills the card
    # what was measured (profiles/predict_wquantile_ab.txt): the rule picks the fastest width at the large shapes ...
    assert wq.default_bits(3, wq.glm_other_bytes(54), big) == 4 and wq.default_bits(6, wq.glm_other_bytes(54), big) == 4
    assert wq.default_bits(3, wq.bnn_other_bytes(1), big) == 4 and wq.default_bits(6, wq.bnn_other_bytes(1), big) == 3
    assert wq.default_bits(3, wq.glm_other_bytes(200), big) == 4 and wq.default_bits(6, wq.glm_other_bytes(200), big) == 4
    # ... and the widest that fits where the grid is smaller than the card (the examples' own shapes: 112 and 2 workgroups)
    assert wq.default_bits(6, wq.glm_other_bytes(54), 112) == 4 and wq.default_bits(6, wq.bnn_other_bytes(1), 2) == 4
    # eight levels beside the widest tile: 4 bits do not fit a CU at all
    assert wq.glm_lds_bytes(59, 8, 4) > wq.PQW_LDS_CU and wq.default_bits(8, wq.glm_other_bytes(59), 100) == 3
    assert wq.bnn_other_bytes(4) == 24832 and wq.bnn_other_bytes(4) + wq.counters_bytes(8, 4) <= wq.PQW_LDS_CU
    for other in (wq.glm_other_bytes(1), wq.glm_other_bytes(30), wq.glm_other_bytes(58), wq.glm_other_bytes(1024),
                  wq.bnn_other_bytes(1), wq.bnn_other_bytes(4)):
        for R in range(1, 9):
            for wgs in (1, 256, 257, 2048):
                b = wq.default_bits(R, other, wgs)
                assert 1 <= b <= 4 and other + wq.counters_bytes(R, b) <= wq.PQW_LDS_CU
                if wgs <= wq.PQW_CUS:                                                     # the widest that fits
                    assert b == 4 or other + wq.counters_bytes(R, b + 1) > wq.PQW_LDS_CU
    assert wq.glm_lds_bytes(59, 2, 4) <= wq.PQW_LDS_CU                                    # two levels: every forced width fits


def test_the_table_reaches_every_arm_of_the_unweighted_table():
    assert wq.CASES is qc.CASES
    by = {c["name"]: c for c in wq.CASES}
    plans = {c["name"]: pc.plan(c["n"], c["B"]) for c in wq.CASES}
    assert any(s > 1 for _, s, _ in plans.values()) and any(c["n"] % pc.PR_PASS for c in wq.CASES)
    assert any(rt == 2 and c["B"] % pc.PR_ROWS for c, (rt, _, _) in zip(wq.CASES, plans.values()))
    assert {1, 2, 3, 4} == {c["n_in"] for c in wq.CASES if c["model"] == "bnn"}
    assert {64, 65} <= {c["H"] for c in wq.CASES if c["model"] == "bnn"}
    assert any(c["model"] != "bnn" and pc.glm_arm(c["F"]) == "chunked" for c in wq.CASES)
    assert any(c["model"] != "bnn" and pc.glm_arm(c["F"]) == "whole" for c in wq.CASES)
    assert plans["q_cap"][2] > pc.PR_PASS and by["q_cap"]["n"] == 16 * pc.PR_SLICE_CAP + 16   # the slice cap binds
    R = len(wq.LEVELS)
    assert R == wq.LEVELS_MAX and min(wq.LEVELS) == 0.0 and max(wq.LEVELS) == 1.0
    # the widths the table's cases take by default at eight levels: 4 bits, 3 where 4 do not fit beside the chunked tile, and
    # a narrower one where two workgroups on a CU pay (q_cap: 1024 workgroups)
    widths = {c["name"]: wq.case_bits(c, R) for c in wq.CASES}
    assert widths["q_chunked"] == 3 and widths["q_linear"] == 4 and widths["q_bnn_H64"] == 4 and widths["q_cap"] < 4
    assert wq.case_bits(by["q_cap"], 1) == 4
    # every weight pattern exists for some case, zero_slices among them
    import predict_weighted_cases as pwc
    assert any(pwc.applies(c, "zero_slices") for c in wq.CASES) and len(wq.PATTERNS) == 8
    # the planted mass patterns: what they promise
    for name, w in qc.planted():
        m = dict(wq.planted_masses(w))
        assert (m["ones"] == 1).all() and (m["counts"] == 0).sum() >= 9 and m["counts"].sum() > 0
        assert int(m["big"].astype(object).sum()) == 2 ** 32 - 1 and int(m["big"].max()) == 2 ** 31
        assert [int(np.flatnonzero(m[k])[0]) for k in ("one_hot_first", "one_hot_middle", "one_hot_last")] == [0, 18, 36]
        if np.isnan(w).any():
            assert ((m["zero_on_nans"] == 0) == np.isnan(w)).all() and ((m["only_on_nans"] > 0) == np.isnan(w)).all()
        else:
            assert "zero_on_nans" not in m
    sums = [int(m.astype(object).sum()) for _, m in wq.POISON]
    assert sums[0] == 0 and sums[1] > 2 ** 32 and sums[2] == 2 ** 32


def test_workspace_sizes_and_bad_inputs_are_what_they_say():
    assert wq.workspace_bytes(5, 2) == 512 + 76 * 10
    assert wq.masses_workspace_bytes(1) == 24 and wq.masses_workspace_bytes(257) == 48
    assert wq.masses_workspace_bytes(1 << 30) == 24 * 256
    for kind in wq.BAD:
        w = wq.bad_weights(40, kind)
        with np.errstate(over="ignore"):
            assert (w < 0).any() or not np.isfinite(w).all() or w.sum() == 0 or not np.isfinite(w.sum()), kind
    for kind in wq.BAD_COUNTS:
        w = wq.bad_counts(40, kind)
        ok = np.isfinite(w).all() and (w >= 0).all() and (w == np.floor(w)).all() and (w < 2.0 ** 32).all() and 0 < w.sum() < 2.0 ** 32
        assert not ok, kind


@pytest.mark.parametrize("q", (0.0, 0.3, 0.5, 1.0))
def test_fp64_quantile_function_is_the_inverted_cdf(q):
    rng = np.random.default_rng(2)
    f, w = rng.normal(size=(30, 3)), rng.exponential(size=30)
    w[::7] = 0.0
    got = wq.fp64_weighted_quantile(f, w, q)
    live = w > 0
    for b in range(3):
        assert got[b] == np.quantile(f[live, b], q, weights=w[live], method="inverted_cdf")
