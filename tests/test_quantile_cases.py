"""CPU: tests/quantile_cases.py is what tests/test_gpu_predict_ranks.py takes it for -- its constants are the source's, its
model of the digit-by-digit select agrees with np.sort on the planted multisets (ties, the last digit of the key, +-0,
+-inf, NaNs of either sign last), every planted product is exact in fp32, and the case table reaches every arm of the
counting kernels that predict_cases.plan can tell apart."""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_cases as pc  # noqa: E402
import quantile_cases as qc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_are_the_sources():
    src = open(os.path.join(ROOT, "stein_amd", "csrc", "stein_predict_ranks.hip")).read()
    hdr = open(os.path.join(ROOT, "include", "steinhip.h")).read()
    assert int(re.search(r"constexpr int PQ_BITS = (\d+)", src).group(1)) == qc.PQ_BITS
    assert int(re.search(r"constexpr int PQ_FLUSH = (\d+)", src).group(1)) == qc.PQ_FLUSH
    assert re.search(r"PQ_LDS_HALF_CU = 80 \* 1024;", src)                                 # the budget of qc.glm_bits
    assert re.search(r"constexpr int PQ_WORDS = 3 \+ PQ_BINS;", src) and qc.PQ_WORDS == 3 + (1 << qc.PQ_BITS)
    assert int(re.search(r"STEIN_PRED_RANKS_MAX = (\d+)", hdr).group(1)) == qc.RANKS_MAX
    assert "%d bytes per (row, rank)" % (4 * qc.PQ_WORDS) in hdr
    assert qc.PQ_FLUSH * pc.PR_PASS <= 255                       # a byte counter cannot overflow between two flushes
    # one forward pass, not two: the counting kernels and the summary kernels include one header and call its slice walks
    summ = open(os.path.join(ROOT, "stein_amd", "csrc", "stein_predict.hip")).read()
    fwd = open(os.path.join(ROOT, "stein_amd", "csrc", "stein_predict_fwd.h")).read()
    assert '#include "stein_predict_fwd.h"' in src and '#include "stein_predict_fwd.h"' in summ
    assert "pred_glm_slice(" in src and "pred_bnn_pass<NIN>(" in src and "pred_glm_slice(" in summ and "pred_bnn_pass<NIN>(" in summ
    assert fwd.count("void pred_glm_slice(") == 1 and fwd.count("void pred_bnn_pass(") == 1
    assert '.hip"' not in src and '.hip"' not in summ and '.hip"' not in fwd   # no source is used as a header
    assert all("STEIN_PREDICT_SHARED_ONLY" not in text for text in (src, summ, fwd))
    import __graft_entry__ as ge
    hdrs = [os.path.basename(p) for p in ge.HDRS]
    assert "stein_predict_fwd.h" in hdrs and "stein_predict.hip" not in hdrs and not any(h.endswith(".hip") for h in hdrs)
    assert "fmaf(" not in re.sub(r"//[^\n]*", "", src)             # and type no arithmetic of the forward pass again


def test_keys_are_monotone_and_invertible():
    vals = np.array([-np.inf, -3.0, -1e-30, -0.0, 0.0, 1e-30, 1.0, np.nextafter(np.float32(1.0), np.float32(2.0)), np.inf],
                    np.float32)
    keys = qc.f32_key(vals)
    assert (np.diff(keys.astype(np.int64)) > 0).all()            # numeric order, -0 before +0
    back = qc.key_f32(keys)
    assert (back.view(np.uint32) == vals.view(np.uint32)).all()
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], np.uint32).view(np.float32)
    assert (qc.f32_key(nans) == qc.NAN_KEY).all() and qc.f32_key(vals).max() < qc.NAN_KEY
    assert np.isnan(qc.key_f32(np.array([qc.NAN_KEY], np.uint32))).all()


def test_model_agrees_with_sort_on_the_planted_multisets():
    names = [name for name, _ in qc.planted()]
    assert names == ["chain", "chain_negative", "repeated", "all_equal", "zeros_infs", "one_nan", "several_nans"]
    for name, w in qc.planted():
        assert w.shape == (qc.PLANT_N,) and w.dtype == np.float32
        f = qc.planted_products(w)
        for b in range(qc.PLANT_B):
            want = np.sort(f[:, b])                              # NaNs last
            got = qc.radix_select(f[:, b], range(qc.PLANT_N))
            assert np.array_equal(got, want, equal_nan=True), (name, b)
            assert np.array_equal(qc.radix_select(f[:, b], range(qc.PLANT_N), bits=3), want, equal_nan=True), (name, b)
            zeros = want == 0
            if zeros.any():                                      # the key order is finer than ==: -0 before +0
                assert (np.diff(np.signbit(got[zeros]).astype(int)) <= 0).all()


def test_planted_sets_hold_what_they_promise():
    sets = dict(qc.planted())
    for name, sign in (("chain", 1.0), ("chain_negative", -1.0)):                         # 30 consecutive floats across 2.0
        v = np.sort((sign * sets[name]).astype(np.float32))
        at = int(np.flatnonzero(v == 2.0)[0])
        run = v[at - 15:at + 15]
        assert len(run) == 30 and (np.diff(run.view(np.uint32).astype(np.int64)) == 1).all() and run[0] < 2.0 < run[-1]
    vals, counts = np.unique(sets["repeated"], return_counts=True)
    assert counts.max() == 5
    assert len(np.unique(sets["all_equal"])) == 1
    z = sets["zeros_infs"]
    assert (z == 0).sum() == 4 and np.signbit(z[z == 0]).sum() == 2 and np.isposinf(z).sum() == 2 and np.isneginf(z).sum() == 2
    assert np.isnan(sets["one_nan"]).sum() == 1
    s = sets["several_nans"]
    assert np.isnan(s).sum() == 5 and np.signbit(s[np.isnan(s)]).sum() == 2
    tiny = np.finfo(np.float32).tiny
    for name, w in sets.items():
        f = qc.planted_products(w)
        fin = np.isfinite(f) & (f != 0)
        assert (np.abs(f[fin]) >= tiny).all(), name                                       # no subnormals


def test_every_planted_product_is_exact_in_fp32():
    x = qc.PLANT_X.astype(np.float64)
    assert (np.log2(x) == np.round(np.log2(x))).all() and (x > 0).all()                   # powers of two
    for name, w in qc.planted():
        ok = np.isfinite(w)
        exact = w[ok].astype(np.float64)[:, None] * x[None, :]                            # exact in fp64: 24 + 1 bits
        f = qc.planted_products(w)[ok]
        assert (f.astype(np.float64) == exact).all(), name


def test_the_table_reaches_every_arm():
    plans = {c["name"]: pc.plan(c["n"], c["B"]) for c in qc.CASES}
    by = {c["name"]: c for c in qc.CASES}
    assert len(by) == len(qc.CASES)
    assert pc.plan(qc.PLANT_N, qc.PLANT_B) == (1, 3, 13)                                  # the planted shape: three slices, ragged
    assert any(s > 1 for _, s, _ in plans.values())                                       # more than one particle slice
    assert any(c["n"] % pc.PR_PASS for c in qc.CASES) and qc.PLANT_N % pc.PR_PASS         # a ragged last pass
    assert any(rt == 2 and c["B"] % pc.PR_ROWS for c, (rt, _, _) in zip(qc.CASES, plans.values()))   # two row tiles, a tail
    cap = by["q_cap"]
    assert cap["n"] == 16 * 1024 + 16 and cap["B"] == 3
    rt = -(-cap["B"] // pc.PR_ROWS)
    assert min(-(-pc.PR_TARGET_WGS // rt), -(-cap["n"] // pc.PR_PASS)) > pc.PR_SLICE_CAP  # the cap is what binds
    assert plans["q_cap"][2] > pc.PR_PASS                                                 # and a slice walks two passes
    assert any(c["model"] != "bnn" and pc.glm_arm(c["F"]) == "chunked" and c["F"] == 59 for c in qc.CASES)
    assert any(c["model"] != "bnn" and pc.glm_arm(c["F"]) == "whole" for c in qc.CASES)
    assert {64, 65} <= {c["H"] for c in qc.CASES if c["model"] == "bnn"}                  # both sides of a hidden chunk edge
    assert {1, 2, 3, 4} == {c["n_in"] for c in qc.CASES if c["model"] == "bnn"}           # the four network instantiations
    assert any(c["model"] == "logistic" and c["output"] == "mean" for c in qc.CASES)
    # both digit widths of the GLM call, and a rank alone (4 bits) against the same rank in company (3)
    assert {qc.glm_bits(c["F"], len(qc.ranks_of(c["n"]))) for c in qc.CASES if c["model"] != "bnn"} == {3, 4}
    assert qc.glm_bits(by["q_chunked"]["F"], 7) == 3 and qc.glm_bits(by["q_chunked"]["F"], 1) == 4
    assert all(qc.glm_bits(F, R) == 4 for F in (1, 54, 59, 1024) for R in (1, 2, 3, 4))
    assert -(-by["q_flush"]["n"] // pc.PR_PASS) > qc.PQ_FLUSH                             # one slice of it flushes mid-way
    for c in qc.CASES:
        r = qc.ranks_of(c["n"])
        assert len(r) <= qc.RANKS_MAX and min(r) == 0 and max(r) == c["n"] - 1 and len(set(r)) == len(r)
    groups = qc.rank_groups(qc.PLANT_N)
    assert sum(groups, []) == list(range(qc.PLANT_N)) and max(map(len, groups)) == qc.RANKS_MAX
