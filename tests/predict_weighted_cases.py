"""The case tables of tests/test_gpu_predict_weighted_matrix.py: the cases of tests/predict_cases.py (dispatch arms,
particle counts, row counts, conditioning) crossed with weight patterns, and the weights of every (case, pattern), NumPy and
seeded.  Shared with tests/test_predict_weighted_ref.py, which checks on the CPU that the tables reach every weighted path
of csrc/stein_predict.hip and that a correct fp32 evaluation stays inside the allowance on these very inputs.

TEST INFRASTRUCTURE ONLY.

Patterns (w [n] in fp64):
    positive     exponential draws; on lpd_range the heaviest weight (50 times the largest draw) sits on the least likely particle
    counts       bincount of ceil(n / 4) draws with replacement: integer weights, many zeros
    one_hot_first | one_hot_last | one_hot_ragged     a single 1: particle 0, particle n - 1, and one inside the last pass of
                 the last slice (the ragged one when the slice length is no multiple of PR_PASS)
    zero_slices  exponential draws with whole slices at zero -- slice 0, the last slice and every third between -- and the
                 first particle of every other slice at zero: the finish kernel skips slices at both ends and inside a
                 group, and a live slice's state is set by a particle that is not its first.  Needs a live slice that is
                 neither the first nor the last and has a second particle: slices >= 3 and per >= 2.
    wide         2^(-150 (1 - p / (n - 1))): rising from 2^-150 to 1, so the leading weights fall under the flush (2^-126 W),
                 whole leading slices with them, and the first live particle lies inside a slice
    uniform      the constant 3.7

The dispatch-arm and row-count cases take one pattern each, in rotation (their business is the forward pass and the row
tiles, which the weights do not touch); the particle-count and conditioning cases take every pattern that exists for them.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_cases as pc  # noqa: E402
import predict_ref as pr  # noqa: E402
import predict_weighted_ref as pwr  # noqa: E402

PW_HEAD = 2            # doubles ahead of the per-slice sums in the weighted workspace (stein_predict.hip)
PATTERNS = ("positive", "counts", "one_hot_first", "one_hot_last", "one_hot_ragged", "zero_slices", "wide", "uniform")


def workspace_bytes(n, B):
    """predict_wws_bytes: the weight pass's header (W, sum w^2, three doubles per slice of the bound) ahead of the states"""
    return 8 * (PW_HEAD + 3 * min(-(-n // pc.PR_PASS), pc.PR_SLICE_CAP)) + pc.workspace_bytes(n, B)


def used_bytes(n, B):
    """what a call's plan writes: the header of its own slice count, then slices * B states"""
    _, slices, _ = pc.plan(n, B)
    return 8 * (PW_HEAD + 3 * slices), slices * pc.PR_STATE * 4 * B


def applies(case, pattern):
    _, slices, per = pc.plan(case["n"], case["B"])
    if pattern == "zero_slices":
        return slices >= 3 and per >= 2
    return True


def ragged_index(case):
    """a particle inside the last pass of the last slice"""
    n = case["n"]
    _, slices, per = pc.plan(n, case["B"])
    begin = (slices - 1) * per
    L = n - begin
    p0 = (L - 1) // pc.PR_PASS * pc.PR_PASS
    return begin + p0 + (L - p0) // 2


def dead_slices(case):
    """the slices zero_slices puts to zero"""
    _, slices, _ = pc.plan(case["n"], case["B"])
    return sorted({0, slices - 1} | set(range(3, slices - 1, 3)))


def weights(case, pattern, a=None):
    """-> w [n] float64; `a` (the case's args) is needed on lpd_range only"""
    n = case["n"]
    rng = np.random.default_rng([sum(map(ord, case["name"] + pattern)), n, case["B"], 11])
    _, slices, per = pc.plan(n, case["B"])
    if pattern == "positive":
        w = rng.exponential(size=n)
        if case["flavor"] == "lpd_range":
            a = pc.args(case) if a is None else a
            worst = int(np.argmax(np.abs(a["y"][0] - a["theta"][:, a["w_col"]])))   # X = 1: l falls with |y - theta|
            w[worst] = 50.0 * w.max()
        return w
    if pattern == "counts":
        return np.bincount(rng.integers(0, n, size=-(-n // 4)), minlength=n).astype(np.float64)
    if pattern.startswith("one_hot"):
        w = np.zeros(n)
        w[{"one_hot_first": 0, "one_hot_last": n - 1, "one_hot_ragged": ragged_index(case)}[pattern]] = 1.0
        return w
    if pattern == "zero_slices":
        assert applies(case, pattern)
        w = rng.exponential(size=n) + 0.01
        w[::per] = 0.0                                     # the first particle of every slice
        for s in dead_slices(case):
            w[s * per:(s + 1) * per] = 0.0
        return w
    if pattern == "wide":
        return 2.0 ** (-150.0 * (1.0 - np.arange(n) / max(n - 1, 1))) if n > 1 else np.ones(1)
    if pattern == "uniform":
        return np.full(n, 3.7)
    raise ValueError(pattern)


def _crossed():
    out = []
    single = pc.ARMS + pc.ROWS
    for i, case in enumerate(single):
        pat = PATTERNS[i % len(PATTERNS)]
        out.append((case, pat if applies(case, pat) else "positive"))
    for case in pc.COUNTS + pc.COND:
        out += [(case, pat) for pat in PATTERNS if applies(case, pat)]
    return out


CROSSED = _crossed()                     # [(case, pattern)]
SUBSET = (pc.SUBSET_CASE, "counts")
BAD = ("negative", "nan", "inf", "all_zero")


def bad_weights(n, kind):
    w = np.random.default_rng(5).exponential(size=n)
    if kind == "all_zero":
        return np.zeros(n)
    w[n // 2] = {"negative": -1e-3, "nan": float("nan"), "inf": float("inf")}[kind]
    return w


def pair_id(pair):
    return "%s-%s" % (pair[0]["name"], pair[1])


def reference(case, a, w, to=lambda v: v, z=None, f=None):
    """predict_cases.reference under the weights w -> dict(pred, mean, var, lpd -> (value, allowance), ess -> (value, allowance))"""
    th, X, y, w = to(a["theta"]), to(a["X"]), to(a["y"]), to(w)
    _, slices, per = pc.plan(case["n"], case["B"])
    lg = None
    if case["model"] == "bnn":
        zz, dz, lg = pwr.bnn_link(th, case["n_in"], case["H"], a["cols"], X)
    else:
        zz, dz = pwr.glm_link(th, a["w_col"], case["F"], X)
    if z is not None:
        zz, dz = z, 0.0 * dz
    fv, df = pwr.outputs(zz, dz, case["model"] == "logistic" and case["output"] == "mean")
    if f is not None:
        fv, df = f, 0.0 * df
    l, dl = pwr.loglik(case["model"], zz, dz, y, case["tau"], lg)
    mean, a_mean, var, a_var = pwr.mean_var(fv, df, w, per, slices)
    val, a_lpd = pwr.lpd(l, dl, w, per, slices)
    return dict(pred=(fv, df), mean=(mean, a_mean), var=(var, a_var), lpd=(val, a_lpd), ess=pwr.ess(w), l=l)


def emulate_f32(case, a, w):
    """the kernel's arithmetic in NumPy float32 -> dict(pred, mean, var, lpd, l)"""
    got = pc.emulate_f32(case, a)
    _, _, per = pc.plan(case["n"], case["B"])
    with np.errstate(over="ignore", under="ignore"):
        mean, var, lpd = pwr.summaries_f32(got["pred"], got["l"], w, per)
    return dict(pred=got["pred"], mean=mean, var=var, lpd=lpd, l=got["l"])
