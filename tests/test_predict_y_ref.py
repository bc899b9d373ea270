"""CPU: the proof of the inputs of tests/test_gpu_predict_ycdf.py and tests/test_gpu_predict_yquantiles.py.

(a) the constants tests/predict_y_ref.py and tests/predict_y_cases.py mirror are the ones in csrc/stein_predict_y.hip and
    include/steinhip.h, and the plan and the workspace size are the library's (host arithmetic: no GPU);
(b) the tables reach every arm: both GLM tile arms, the four network instantiations, one slice / several / the slice cap, the
    cut-down slice count of the 56-sum pass and the plain one, every weight pattern and none, every count with and without weights;
(c) a NumPy float32 emulation of the kernel's arithmetic stays inside the allowance a_F on these very inputs (rows are
    independent, so a few rows per case do);
(d) the initial bracket of every (case, pattern, level) contains the fp64 quantile: F(lo0) <= level <= F(hi0) in fp64;
(e) the emulated 8-ary search keeps lo <= hi, the width contract and the bracket contract [Q(q - a_F), Q(q + a_F)] on the
    small cases and on every planted mixture, where the closed-form quantile lies inside the bracket up to that uncertainty.
"""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_cases as pc  # noqa: E402
import predict_weighted_cases as pwc  # noqa: E402
import predict_y_cases as yc  # noqa: E402
import predict_y_ref as yr  # noqa: E402

ROWS_KEPT = 6


def _rows(B):
    return np.unique(np.r_[0:min(B, ROWS_KEPT // 2), max(0, B - ROWS_KEPT // 2):B])


def test_constants_plan_and_workspace_mirror_the_source():
    src = open(os.path.join(ROOT, "stein_amd", "csrc", "stein_predict_y.hip")).read()
    hdr = open(os.path.join(ROOT, "include", "steinhip.h")).read()
    assert int(re.search(r"constexpr int PY_K = (\d+);", src).group(1)) == yr.K
    assert "PY_PART_FLOATS = (int64_t)1 << 23;" in src and yr.PART_FLOATS == 1 << 23
    assert int(re.search(r"constexpr int PY_ROUND_WGS = (\d+);", src).group(1)) == yr.ROUND_WGS
    assert float(re.search(r"PY_WIDEN = ([0-9.e+-]+)f;", src).group(1)) == yr.WIDEN
    assert int(re.search(r"STEIN_PRED_Y_POINTS_MAX = (\d+)", hdr).group(1)) == yr.POINTS_MAX
    assert int(re.search(r"STEIN_PRED_Y_PASSES_MAX = (\d+)", hdr).group(1)) == yr.PASSES_MAX
    assert "pred_glm_slice(" in src and "pred_bnn_pass<NIN>(" in src and "predict_weight_pass(" in src
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomic" not in code and "k_predict_wsum" not in code          # no atomics; the weight pass is not copied
    from stein_amd import _lib
    assert (_lib.PRED_Y_POINTS_MAX, _lib.PRED_Y_PASSES_MAX) == (yr.POINTS_MAX, yr.PASSES_MAX)
    ns, Bs = (1, 15, 16, 17, 4000, 17403, 1 << 20, 1 << 30), (1, 5, 255, 256, 257, 2049, 100000, 1 << 30)
    for count in (1, 3, 8):
        tc = [[_lib.predict_ycdf_workspace_bytes(n, B, count) for B in Bs] for n in ns]
        tq = [[_lib.predict_yquantiles_workspace_bytes(n, B, count) for B in Bs] for n in ns]
        for i, n in enumerate(ns):
            for j, B in enumerate(Bs):
                assert tc[i][j] == yc.workspace_bytes(n, B, count, 0) and tq[i][j] == yc.workspace_bytes(n, B, yr.K * count, count)
                assert tc[i][j] % 8 == 0 and tq[i][j] % 8 == 0
                if i:
                    assert tc[i][j] >= tc[i - 1][j] and tq[i][j] >= tq[i - 1][j]
                if j:
                    assert tc[i][j] >= tc[i][j - 1] and tq[i][j] >= tq[i][j - 1]
                if count > 1:
                    assert tc[i][j] >= _lib.predict_ycdf_workspace_bytes(n, B, count - 1)
                # the size covers what the plan of the call writes
                for acc, lv, got in ((count, 0, tc[i][j]), (yr.K * count, count, tq[i][j])):
                    _, slices, _ = yc.y_plan(n, B, lv > 0)
                    assert 8 * (pwc.PW_HEAD + 3 * slices) + 4 * (2 * lv * B + slices * B * acc) <= got
    with pytest.raises(ValueError, match="more than 8 points"):
        _lib.predict_ycdf_workspace_bytes(4, 4, 9)
    with pytest.raises(ValueError, match="n_levels 0"):
        _lib.predict_yquantiles_workspace_bytes(4, 4, 0)


def test_tables_reach_every_arm():
    cases = {c["name"]: c for c, _, _ in yc.CROSSED}.values()
    assert all(c["model"] in ("linear", "bnn") for c in cases)
    assert {pc.glm_arm(c["F"]) for c in cases if c["model"] == "linear"} == {"whole", "chunked"}
    assert {c["n_in"] for c in cases if c["model"] == "bnn"} == {1, 2, 3, 4}
    for lo, hi in pc.BNN_EDGES:
        assert {lo, hi} <= {c["H"] for c in cases if c["model"] == "bnn"}
    slices = {pc.plan(c["n"], c["B"])[1] for c in cases}
    assert 1 in slices and pc.PR_SLICE_CAP in slices and any(1 < s < pc.PR_SLICE_CAP for s in slices)
    assert {c["n"] for c in cases} >= {1, pc.PR_PASS - 1, pc.PR_PASS, pc.PR_PASS + 1, 17403}
    assert {c["B"] for c in cases} >= {1, pc.PR_ROWS - 1, pc.PR_ROWS, pc.PR_ROWS + 1, 2 * pc.PR_ROWS + 3}
    cut = [yc.y_plan(c["n"], c["B"], True)[1] < pc.plan(c["n"], c["B"])[1] for c, _, k in yc.CROSSED]
    assert any(cut) and not all(cut)                      # the quantiles' plan with its slices cut down, and the plain plan
    assert {p for _, p, _ in yc.CROSSED} == set(pwc.PATTERNS) | {None}
    assert {(p is None, k) for _, p, k in yc.CROSSED} == {(a, k) for a in (True, False) for k in yc.COUNT_CHOICES}
    for k in yc.COUNT_CHOICES:
        assert len(yc.levels(k)) == k and all(0.0 < q < 1.0 for q in yc.levels(k))
    assert 1e-6 in yc.levels(3) and 0.5 in yc.levels(1) and 0.5 in yc.levels(3) and 0.5 in yc.levels(8)
    names = [p[0] for p in yc.planted()]
    assert names == ["identical", "single", "symmetric", "far_modes", "nan_dead", "collapse"]


def _parts(case, a, pattern):
    """the case cut down to a few rows (rows are independent) -> its args, weights and the emulated and fp64 parts"""
    rows = _rows(case["B"])
    w = yc.weights(case, pattern, a)
    a = dict(a, X=a["X"][rows], y=a["y"][rows])
    z32, s32, rs32 = yc.emulated_parts(case, a)
    _, _, s64 = yc.model_parts(case, a)
    w32 = None if w is None else yr.norm_weights_f32(w)
    return a, w, w32, z32, s32, rs32, z32.astype(np.float64), np.asarray(s64, np.float64)


def _emulable(case, pattern):
    return case["n"] <= 4000 or pattern in (None, "positive", "zero_slices", "wide")   # (the long loops: four patterns do)


@pytest.mark.parametrize("tr", [t for t in yc.CROSSED if _emulable(t[0], t[1])], ids=yc.triple_id)
def test_emulated_cdf_stays_inside_the_allowance(tr):
    case, pattern, count = tr
    a = pc.args(case)
    a, w, w32, z32, s32, _, z64, s64 = _parts(case, a, pattern)
    _, slices, per = yc.y_plan(case["n"], case["B"], False)
    t = yc.points(case, a, np.asarray(yc.model_parts(case, a)[0]), s64, w, count)
    got = yr.cdf_f32(t, z32, s32, w32, per).astype(np.float32).astype(np.float64)
    ref, allow = yr.cdf(t.astype(np.float64), z64, 0.0 * z64, s64, w, case["model"], per, slices)
    err = np.abs(got - ref)
    assert np.isfinite(ref).all() and np.isfinite(allow).all()
    assert (err <= allow).all(), float((err / allow).max())
    assert (allow < 1e-4).all()                            # an allowance that allowed anything would prove nothing
    assert ref.min() < 0.2 and ref.max() > 0.8 or count == 1   # the points reach both sides of the mixture


@pytest.mark.parametrize("tr", yc.CROSSED, ids=yc.triple_id)
def test_initial_bracket_contains_the_fp64_quantile(tr):
    case, pattern, count = tr
    a = pc.args(case)
    a, w, w32, z32, s32, rs32, z64, s64 = _parts(case, a, pattern)
    zero = 0.0 * z64
    for q in yc.levels(count):
        lo0, hi0 = yr.bracket_f32(z32, s32, rs32, w32, np.float32(yr.ndtri(q)))
        assert np.isfinite(lo0).all() and np.isfinite(hi0).all() and (lo0 <= hi0).all()
        F = yr.cdf(np.stack([lo0, hi0]).astype(np.float64), z64, zero, s64, w, case["model"], 1, 1)[0]
        assert (F[0] <= q).all() and (F[1] >= q).all(), (q, F)


def _check_search(case, w, w32, z32, s32, rs32, z64, s64, levels, passes, per, slices):
    """the emulated call against the contract -> the brackets and, per level, Q64(q - a_F) and Q64(q + a_F)"""
    lo, hi, lo0, hi0 = yr.yquantiles_f32(levels, passes, z32, s32, rs32, w32, per)
    lo1, hi1, _, _ = yr.yquantiles_f32(levels, 1, z32, s32, rs32, w32, per)
    assert (lo <= hi).all() and (lo0 <= lo).all() and (hi <= hi0).all()
    width = hi.astype(np.float64) - lo.astype(np.float64)
    bound = yr.width_bound(lo1, hi1, passes)
    assert (width <= bound).all(), float((width / bound).max())
    zero = 0.0 * z64
    q_minus, q_plus = [], []
    for i, q in enumerate(levels):
        a_hi = yr.cdf(hi[i:i + 1].astype(np.float64), z64, zero, s64, w, case["model"], per, slices)[1][0]
        a_lo = yr.cdf(lo[i:i + 1].astype(np.float64), z64, zero, s64, w, case["model"], per, slices)[1][0]
        q_minus.append(yr.quantile64(q - a_hi, z64, s64, w)[0])
        q_plus.append(yr.quantile64(q + a_lo, z64, s64, w)[1])
        assert (hi[i] >= q_minus[i]).all() and (lo[i] <= q_plus[i]).all(), q
    return lo, hi, q_minus, q_plus, bound


SEARCHED = [t for t in yc.CROSSED if t[0]["n"] <= 100]


@pytest.mark.parametrize("tr", SEARCHED, ids=yc.triple_id)
def test_emulated_search_keeps_the_contract(tr):
    case, pattern, count = tr
    a = pc.args(case)
    a, w, w32, z32, s32, rs32, z64, s64 = _parts(case, a, pattern)
    _, slices, per = yc.y_plan(case["n"], case["B"], True)
    _check_search(case, w, w32, z32, s32, rs32, z64, s64, yc.levels(count), 8, per, slices)


@pytest.mark.parametrize("plant", yc.planted(), ids=lambda p: p[0])
def test_emulated_search_finds_the_planted_quantiles(plant):
    name, case, a, w, levels, expect, passes = plant
    z32 = np.repeat(a["theta"][:, a["w_col"]].astype(np.float32)[:, None], case["B"], axis=1)   # X = 1: z_pb = w_p
    s32, rs32 = yr.s_f32("linear", tau=case["tau"])
    s32, rs32 = np.full(case["n"], s32, np.float32), np.full(case["n"], rs32, np.float32)
    w32 = None if w is None else yr.norm_weights_f32(w)
    z64, s64 = z32.astype(np.float64), np.full(case["n"], np.sqrt(case["tau"]))
    _, slices, per = yc.y_plan(case["n"], case["B"], True)
    lo, hi, q_minus, q_plus, bound = _check_search(case, w, w32, z32, s32, rs32, z64, s64, levels, passes, per, slices)
    for i, q in enumerate(levels):
        if np.isnan(expect[i]):
            continue
        # the closed form lies between the bisection's Q(q - a_F) and Q(q + a_F), and so does the result up to its width
        assert (q_minus[i] <= expect[i]).all() and (expect[i] <= q_plus[i]).all(), (name, q)
        assert (hi[i] >= q_minus[i]).all() and (hi[i] <= q_plus[i] + bound[i]).all(), (name, q, hi[i], expect[i])
    if name == "collapse":                                   # the bracket is down to neighbouring floats well before pass 12
        early = yr.yquantiles_f32(levels, 9, z32, s32, rs32, w32, per)
        assert (np.abs(early[1] - early[0]) <= np.spacing(np.abs(early[1]))).all()
