"""The case tables of tests/test_gpu_predict_matrix.py and the inputs of every case (NumPy, seeded), shared with
tests/test_predict_ref.py, which checks on the CPU that the tables reach every instantiation and dispatch arm of
csrc/stein_predict.hip and that a correct fp32 evaluation stays inside the allowance on these very inputs.

TEST INFRASTRUCTURE ONLY."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_ref as pr  # noqa: E402
import score_cases as sc  # noqa: E402
import score_ref as sr  # noqa: E402

# the constants of stein_predict.hip (tests/test_predict_ref.py reads them back from the source)
PR_ROWS = 256          # rows of X per workgroup
PR_PASS = 16           # particles per pass of a slice
PR_SLICE_CAP = 1024
PR_TARGET_WGS = 2048
PR_FC = 58             # GLM: features per LDS chunk of the X tile and of the staged weights
PR_HC = 64             # network: hidden units per LDS chunk of the staged weights
PR_STATE = 5           # workspace floats per (slice, row)


def plan(n, B):
    """predict_plan of stein_predict.hip -> (row_tiles, slices, per)"""
    rt = -(-B // PR_ROWS)
    s = min(-(-PR_TARGET_WGS // rt), PR_SLICE_CAP, -(-n // PR_PASS))
    per = -(-n // s)
    return rt, -(-n // per), per


def workspace_bytes(n, B):
    """predict_ws_bytes: a monotone upper bound of slices * B states"""
    return min(min(-(-n // PR_PASS), PR_SLICE_CAP) * B, PR_TARGET_WGS * PR_ROWS + B) * PR_STATE * 4


def glm_arm(F):
    """the arm of k_predict_glm F features take: the X tile staged once, or chunk by chunk inside every pass"""
    return "whole" if F <= PR_FC else "chunked"


def _case(name, model, n, B, F=None, n_in=None, H=None, output="link", alpha=None, flavor="plain", tau=1.0):
    return dict(name=name, model=model, n=n, B=B, F=F, n_in=n_in, H=H, output=output, alpha=alpha, flavor=flavor, tau=tau)


# ---- dispatch arms: both sides of the X / weight chunk edge of the GLM kernel (F = PR_FC | PR_FC + 1), two and three
# chunks and one feature past them, both parities of the staged row length, the four network instantiations, the hidden
# chunk edges, hidden counts that are no multiple of 4; three models, both outputs, model columns before / between / after
# spare columns
GLM_EDGES = ((PR_FC, PR_FC + 1), (2 * PR_FC, 2 * PR_FC + 1), (3 * PR_FC, 3 * PR_FC + 1))
BNN_EDGES = ((PR_HC, PR_HC + 1), (2 * PR_HC, 2 * PR_HC + 1), (3 * PR_HC, 3 * PR_HC + 1))
ARMS = [_case("glmF%d" % F, kind, n, B, F=F, output=out, alpha=alpha, tau=tau) for F, kind, out, alpha, n, B, tau in [
    (1, "linear", "link", None, 5, 40, 1.0), (2, "logistic", "mean", "before", 19, 33, 1.0),
    (57, "logistic", "link", "after", 21, 70, 1.0), (58, "linear", "mean", "last", 18, 30, 0.25),
    (59, "logistic", "mean", None, 17, 41, 1.0), (116, "linear", "link", "before", 9, 25, 3.0),
    (117, "logistic", "link", "last", 20, 12, 1.0), (174, "logistic", "mean", "after", 7, 9, 1.0),
    (175, "linear", "link", None, 6, 10, 1.0), (1024, "logistic", "link", "before", 3, 6, 1.0)]]
ARMS += [_case("bnnH%d_in%d" % (H, n_in), "bnn", n, B, n_in=n_in, H=H) for H, n_in, n, B in [
    (1, 1, 1, 7), (3, 2, 17, 20), (63, 3, 5, 12), (64, 4, 18, 9), (65, 1, 19, 30), (128, 2, 7, 16), (129, 3, 5, 10),
    (192, 4, 6, 8), (193, 1, 5, 25), (1024, 4, 2, 6), (100, 1, 20, 20)]]

# ---- particle counts: 1, around one pass of a slice, and just past cap * pass at the cap's own slice count (every slice
# walks two passes); with 2049 rows the plan asks for 228 slices, below the cap and below the passes there are
COUNTS = [_case("n%d_%s" % (n, m), m, n, 5, F=3, n_in=2, H=5, alpha="after") for m in ("logistic", "bnn")
          for n in (1, PR_PASS - 1, PR_PASS, PR_PASS + 1, 2 * PR_PASS + 1, 17403)]
COUNTS += [_case("want228", "linear", 4000, 2049, F=3, alpha="before")]

# ---- row counts: 1 and around one row tile
ROWS = [_case("B%d_%s" % (B, m), m, 21, B, F=9, n_in=1, H=6) for m in ("linear", "bnn")
        for B in (1, PR_ROWS - 1, PR_ROWS, PR_ROWS + 1, 2 * PR_ROWS + 3)]

# ---- conditioning
COND = [_case("var_offset", "linear", 100, 7, F=2, flavor="var_offset"),
        _case("var_offset_bnn", "bnn", 100, 7, n_in=1, H=8, flavor="var_offset"),
        _case("lpd_range", "linear", 120, 5, F=1, flavor="lpd_range"),
        _case("logit_sat", "logistic", 45, 40, F=6, output="mean", flavor="logit_sat")]
SUBSET_CASE = _case("subsets", "logistic", 37, 70, F=9, output="mean", alpha="after")
CASES = ARMS + COUNTS + ROWS + COND


def _r32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def args(case):
    """-> dict(theta, X, y [fp64 holding fp32 values], d, and the model's layout: w_col | cols)"""
    rng = np.random.default_rng([sum(map(ord, case["name"])), case["n"], case["B"], 7])
    n, B, flavor = case["n"], case["B"], case["flavor"]
    if case["model"] == "bnn":
        n_in, H = case["n_in"], case["H"]
        cols, d = sc.bnn_layout(n_in, H, sc.BNN_BLOCK_ORDERS[(H + n_in) % 3])
        c = dict(zip(sr.BNN_ORDER, cols))
        th = rng.normal(size=(n, d)) * 0.7
        X, y = rng.uniform(size=(B, n_in)), rng.normal(size=B)
        if flavor == "var_offset":            # a common output offset of 10^3 through b2, a spread of 10^-2 across particles
            th[:, c["w2"]:c["w2"] + H] *= 0.01
            th[:, c["b2"]] = 1000.0 + 0.01 * rng.normal(size=n)
            y = 1000.0 + rng.normal(size=B)
        return dict(theta=_r32(th), X=_r32(X), y=_r32(y), d=d, cols=cols)
    F = case["F"]
    w_col, _, d = sc.glm_layout(F, case["alpha"])
    th = rng.normal(size=(n, d)) * 0.5
    X = rng.normal(size=(B, F))
    y = rng.normal(size=B) if case["model"] == "linear" else (rng.uniform(size=B) < 0.5).astype(np.float64)
    w = slice(w_col, w_col + F)
    if flavor == "var_offset":                # feature 0 is the constant 1; its weight carries the offset
        X[:, 0] = 1.0
        th[:, w] = 0.01 * rng.normal(size=(n, F))
        th[:, w_col] += 1000.0
        y = 1000.0 + rng.normal(size=B)
    if flavor == "lpd_range":                 # residuals over [45, 50]: l from -1013 down to -1251
        X[:] = 1.0
        th[:, w_col] = rng.permutation(np.linspace(-2.5, 2.5, n))
        y[:] = 47.5
    if flavor == "logit_sat":                 # |z| up to 90 on both sides
        th[:, w] *= 90.0 / np.abs(X @ th[:, w].T).max()
    return dict(theta=_r32(th), X=_r32(X), y=_r32(y), d=d, w_col=w_col)


def reference(case, a, to=lambda v: v, z=None, f=None):
    """-> dict(pred, mean, var, lpd -> (value, allowance)) from a case's args; `to` moves an array to where the reference
    runs.  z (fp64, [n, B]): take these linear outputs as exact instead -- the allowance then holds the reduction terms and
    the roundings of f and l alone (the summaries are of the values pred holds).  f (fp64, [n, B]): take these reported
    outputs as exact for the mean and the variance -- their allowance then holds the reduction terms alone, the sigmoid's
    roundings too being the forward pass's business."""
    th, X, y = to(a["theta"]), to(a["X"]), to(a["y"])
    _, slices, per = plan(case["n"], case["B"])
    lg = None
    if case["model"] == "bnn":
        zz, dz, lg = pr.bnn_link(th, case["n_in"], case["H"], a["cols"], X)
    else:
        zz, dz = pr.glm_link(th, a["w_col"], case["F"], X)
    if z is not None:
        zz, dz = z, 0.0 * dz
    fv, df = pr.outputs(zz, dz, case["model"] == "logistic" and case["output"] == "mean")
    if f is not None:
        fv, df = f, 0.0 * df
    l, dl = pr.loglik(case["model"], zz, dz, y, case["tau"], lg)
    mean, a_mean, var, a_var = pr.mean_var(fv, df, per, slices)
    val, a_lpd = pr.lpd(l, dl, per, slices)
    return dict(pred=(fv, df), mean=(mean, a_mean), var=(var, a_var), lpd=(val, a_lpd), l=l)


def emulate_f32(case, a):
    """the kernel's arithmetic in NumPy float32 -> dict(pred, mean, var, lpd)"""
    _, _, per = plan(case["n"], case["B"])
    model = case["model"]
    if model == "bnn":
        z = pr.link_f32(model, a["theta"], a["X"], n_in=case["n_in"], H=case["H"], cols=a["cols"])
        lg = a["theta"][:, dict(zip(sr.BNN_ORDER, a["cols"]))["log_gamma"]]
    else:
        z = pr.link_f32(model, a["theta"], a["X"], w_col=a["w_col"], F=case["F"])
        lg = None
    with np.errstate(over="ignore", under="ignore"):
        f = pr.outputs_f32(z, model == "logistic" and case["output"] == "mean")
        l = pr.loglik_f32(model, z, a["y"], case["tau"], lg)
        mean, var, lpd = pr.summaries_f32(f, l, per)
    return dict(pred=f, mean=mean, var=var, lpd=lpd, l=l)


def cpu_sized(case):
    width = case["F"] if case["model"] != "bnn" else case["H"] * (case["n_in"] + 2)
    return case["n"] * case["B"] * width <= 3_000_000


def check_conditioning_inputs(case, a, ref):
    """assert from the inputs and the reference alone that a conditioning case is what its flavor promises"""
    f = np.asarray(ref["pred"][0])
    if case["flavor"] == "var_offset":
        assert np.abs(f.mean(0) - 1000.0).max() < 5.0 and 2e-3 < f.std(0).min() and f.std(0).max() < 5e-2
    if case["flavor"] == "lpd_range":
        l = np.asarray(ref["l"])
        assert l.max() < -1000.0 and (l.max(0) - l.min(0)).min() > 200.0
    if case["flavor"] == "logit_sat":
        z = a["X"] @ a["theta"][:, a["w_col"]:a["w_col"] + case["F"]].T
        assert 85.0 <= z.max() <= 90.5 or 85.0 <= -z.min() <= 90.5
        assert z.max() > 60.0 and z.min() < -60.0
