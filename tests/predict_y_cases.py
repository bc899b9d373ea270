"""The case tables of tests/test_gpu_predict_ycdf.py and tests/test_gpu_predict_yquantiles.py: the regression rows (linear and
network) of tests/predict_cases.py -- dispatch arms, particle counts, row counts, the two var_offset cases -- crossed with the
weight patterns of tests/predict_weighted_cases.py and with weights=None, the points and levels of every case, and planted
mixtures with closed-form quantiles.  Shared with tests/test_predict_y_ref.py, which proves the inputs on the CPU.

The calls through the C ABI that the two GPU files share are at the end.

TEST INFRASTRUCTURE ONLY."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_cases as pc  # noqa: E402
import predict_ref as pr  # noqa: E402
import predict_weighted_cases as pwc  # noqa: E402
import predict_y_ref as yr  # noqa: E402
import score_cases as sc  # noqa: E402
import score_ref as sr  # noqa: E402

COUNT_CHOICES = (1, 3, 8)                    # n_pts and n_levels
LEVEL_SETS = {1: (0.5,), 3: (1e-6, 0.5, 0.95), 8: (1e-6, 0.025, 0.05, 0.25, 0.5, 0.75, 0.95, 0.975)}


def regression(cases):
    return [c for c in cases if c["model"] in ("linear", "bnn")]


SINGLE = regression(pc.ARMS) + regression(pc.ROWS)                     # one pattern each, in rotation, and None
EVERY = regression(pc.COUNTS) + [c for c in regression(pc.COND) if c["flavor"] == "var_offset"]   # every pattern, and None


def y_plan(n, B, quantiles):
    """predict_y_plan of stein_predict_y.hip -> (row_tiles, slices, per): the summaries' plan, its slices cut down until the
    partial sums of a full call of this kind (8 floats per (slice, row of a whole row tile) for the distribution function, 56
    for the quantiles) fit PY_PART_FLOATS -- whatever the call's own count of points or levels"""
    acc = yr.K * yr.LEVELS_MAX if quantiles else yr.POINTS_MAX
    rt, slices, per = pc.plan(n, B)
    s = max(1, yr.PART_FLOATS // (rt * pc.PR_ROWS * acc))
    if slices > s:
        if s * rt >= yr.ROUND_WGS:                      # whole rounds of the card
            s = max(1, s * rt // yr.ROUND_WGS * yr.ROUND_WGS // rt)
        per = -(-n // s)
        slices = -(-n // per)
    return rt, slices, per


def workspace_bytes(n, B, acc, levels):
    """predict_y_ws_bytes"""
    s = min(-(-n // pc.PR_PASS), pc.PR_SLICE_CAP)
    floats = min(s * B * acc, (pc.PR_TARGET_WGS * pc.PR_ROWS + B) * acc, yr.PART_FLOATS + B * acc)
    return (8 * (pwc.PW_HEAD + 3 * s) + 4 * (2 * levels * B + floats) + 7) // 8 * 8


def _crossed():
    """[(case, pattern or None, count)]: count in COUNT_CHOICES by rotation over the whole table, so every arm, every particle
    count regime and every pattern meets every count somewhere"""
    pairs = []
    for i, case in enumerate(SINGLE):
        pat = pwc.PATTERNS[i % len(pwc.PATTERNS)]
        pairs += [(case, pat if pwc.applies(case, pat) else "positive"), (case, None)]
    for case in EVERY:
        pairs += [(case, pat) for pat in pwc.PATTERNS if pwc.applies(case, pat)] + [(case, None)]
    return [(case, pat, COUNT_CHOICES[k % 3]) for k, (case, pat) in enumerate(pairs)]


CROSSED = _crossed()


def triple_id(tr):
    return "%s-%s-%d" % (tr[0]["name"], tr[1] or "none", tr[2])


def weights(case, pattern, a=None):
    return None if pattern is None else pwc.weights(case, pattern, a)


def model_parts(case, a, to=lambda v: v):
    """-> (z, dz, s) in fp64: the reference's linear outputs with their allowance, and sqrt(tau) per particle"""
    th, X = to(a["theta"]), to(a["X"])
    if case["model"] == "bnn":
        z, dz, lg = pr.bnn_link(th, case["n_in"], case["H"], a["cols"], X)
        s = (0.5 * lg).exp() if sr._xp(lg) is not np else np.exp(0.5 * lg)
    else:
        z, dz = pr.glm_link(th, a["w_col"], case["F"], X)
        s = to(np.full(case["n"], np.sqrt(np.float64(case["tau"]))))
    return z, dz, s


def emulated_parts(case, a):
    """-> (z f32 [n, B], s f32, 1 / s f32) as the kernels compute them"""
    if case["model"] == "bnn":
        z = pr.link_f32("bnn", a["theta"], a["X"], n_in=case["n_in"], H=case["H"], cols=a["cols"])
        lg = a["theta"][:, dict(zip(sr.BNN_ORDER, a["cols"]))["log_gamma"]]
        s, rs = yr.s_f32("bnn", lg=lg)
    else:
        z = pr.link_f32(case["model"], a["theta"], a["X"], w_col=a["w_col"], F=case["F"])
        s, rs = yr.s_f32("linear", tau=case["tau"])
        s, rs = np.full(case["n"], s, np.float32), np.full(case["n"], rs, np.float32)
    return np.asarray(z, np.float32), s, rs


def points(case, a, z, s, w, count):
    """t [count, B] float32: y itself first (the PIT), then points spread over the mixture's bulk and both tails, from the
    reference's own centre and spread per row (NumPy fp64 z [n, B], s [n])"""
    rng = np.random.default_rng([sum(map(ord, case["name"])), count, 13])
    wn = np.full(z.shape[0], 1.0 / z.shape[0]) if w is None else w / w.sum()
    live = wn > 0
    zl, sl, wl = z[live], s[live], wn[live]
    centre = (wl[:, None] * zl).sum(0)
    spread = np.sqrt((wl[:, None] * ((zl - centre) ** 2 + 1.0 / sl[:, None] ** 2)).sum(0))
    offs = np.array([0.0, -1.0, 1.0, -3.0, 0.3, 2.0, -6.0, 8.0])[:count]
    t = centre[None, :] + offs[:, None] * spread[None, :] * rng.uniform(0.8, 1.2, size=(count, z.shape[1]))
    t[0] = a["y"]
    return np.asarray(t, np.float32)


def levels(count):
    return LEVEL_SETS[count]


# ---- planted mixtures ------------------------------------------------------------------------------------------------------
# A linear model with one feature and X = 1 has z_pb = w_p for every row, so the particles' outputs are planted exactly.
def _planted_case(name, n, B=3, tau=1.0):
    return pc._case("planted_" + name, "linear", n, B, F=1, tau=tau)


def planted():
    """-> [(name, case, args, w or None, levels, expected [L] float64, passes)]: the quantiles in closed form (NaN: a level
    with no closed form, held to the bracket contract alone)"""
    out = []

    def add(name, zvals, tau, w, lv, expect, passes=8, B=3):
        n = len(zvals)
        case = _planted_case(name, n, B, tau)
        w_col, _, d = sc.glm_layout(1, None)
        th = np.zeros((n, d))
        th[:, w_col] = zvals
        a = dict(theta=np.asarray(th, np.float32).astype(np.float64), X=np.ones((B, 1)), y=np.zeros(B), d=d, w_col=w_col)
        out.append((name, case, a, w, tuple(lv), expect, passes))
    q3 = (0.025, 0.5, 0.975)
    # identical particles: Q = z + Phi^-1(q) / sqrt(tau)
    add("identical", np.full(40, 3.25), 4.0, None, q3, 3.25 + yr.ndtri(np.array(q3)) / 2.0)
    # one particle
    add("single", np.array([-1.5]), 0.25, None, q3, -1.5 + yr.ndtri(np.array(q3)) * 2.0)
    # two components at +-a, equal weights: the median is 0
    add("symmetric", np.array([-2.0, 2.0]), 1.0, None, (0.5,), np.array([0.0]))
    # +-40 with sigma = 0.1: no density between the modes; levels inside either mode, in closed form from that mode alone
    # (the median is any point of the plateau between them)
    add("far_modes", np.array([-40.0, 40.0]), 100.0, None, (0.25, 0.5, 0.75), np.array([-40.0, np.nan, 40.0]))
    # a particle of weight 0 whose output is NaN beside identical live ones
    z = np.full(20, -7.0)
    z[3] = np.nan
    w = np.ones(20)
    w[3] = 0.0
    add("nan_dead", z, 1.0, w, q3, -7.0 + yr.ndtri(np.array(q3)))
    # a bracket that collapses before the last pass: identical particles, 12 passes
    add("collapse", np.full(17, 0.5), 1.0, None, q3, 0.5 + yr.ndtri(np.array(q3)), passes=12)
    return out


# ---- the calls through the C ABI (GPU tests only: torch and the library are imported where they are used) ---------------------
def device_inputs(a, dev):
    import torch
    return tuple(torch.tensor(a[k], dtype=torch.float32, device=dev) for k in ("theta", "X"))


def _model_args(case, a, th, X):
    """-> (entry-point stem, the arguments up to and including batch [, noise_precision])"""
    import ctypes
    from stein_amd import _lib
    n, B = th.shape[0], X.shape[0]
    if case["model"] == "bnn":
        return "bnn", [th.data_ptr(), n, a["d"], case["n_in"], case["H"], (ctypes.c_int64 * 6)(*a["cols"]), X.data_ptr(), B]
    kind = _lib.GLM_LINEAR if case["model"] == "linear" else _lib.GLM_LOGISTIC
    return "glm", [th.data_ptr(), n, a["d"], kind, a["w_col"], case["F"], X.data_ptr(), B, float(case["tau"])]


def _weights_tensor(w, dev):
    import torch
    return None if w is None else torch.as_tensor(np.asarray(w, np.float64), device=dev)


def call_pred(case, a, dev, tensors=None):
    """the library's own linear outputs z [n, B] (pred with STEIN_PRED_LINK)"""
    import ctypes
    import torch
    from stein_amd import _lib
    th, X = tensors or device_inputs(a, dev)
    n, B = th.shape[0], X.shape[0]
    pred = torch.empty(n, B, dtype=torch.float32, device=dev)
    tail = [pred.data_ptr(), None, None, None, None, 0, torch.cuda.current_stream(dev).cuda_stream]
    if case["model"] == "bnn":
        _lib.call("stein_predict_bnn", th.data_ptr(), n, a["d"], case["n_in"], case["H"], (ctypes.c_int64 * 6)(*a["cols"]),
                  _lib.PRED_LINK, X.data_ptr(), None, B, *tail)
    else:
        _lib.call("stein_predict_glm", th.data_ptr(), n, a["d"], _lib.GLM_LINEAR, _lib.PRED_LINK, a["w_col"], case["F"],
                  X.data_ptr(), None, B, float(case["tau"]), *tail)
    return pred


def call_ycdf(case, a, t, w, dev, ws_fill=float("nan"), tensors=None, fill=float("nan")):
    """stein_predict_*_ycdf -> (out [A, B] float32, workspace as float32 words); t: a float32 device tensor [A, B]"""
    import torch
    from stein_amd import _lib
    th, X = tensors or device_inputs(a, dev)
    n, B, A = th.shape[0], X.shape[0], t.shape[0]
    out = torch.full((A, B), fill, dtype=torch.float32, device=dev)
    ws = torch.full((_lib.predict_ycdf_workspace_bytes(n, B, A) // 4,), ws_fill, dtype=torch.float32, device=dev)
    assert ws.data_ptr() % 8 == 0
    wd = _weights_tensor(w, dev)
    stem, args = _model_args(case, a, th, X)
    _lib.call("stein_predict_%s_ycdf" % stem, *args, t.data_ptr(), A, None if wd is None else wd.data_ptr(), out.data_ptr(),
              ws.data_ptr(), ws.numel() * 4, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return out, ws


def call_yquantiles(case, a, lv, passes, w, dev, ws_fill=float("nan"), tensors=None, want_lo=True):
    """stein_predict_*_yquantiles -> (lo or None, hi) [L, B] float32"""
    import ctypes
    import torch
    from stein_amd import _lib
    th, X = tensors or device_inputs(a, dev)
    n, B, L = th.shape[0], X.shape[0], len(lv)
    hi = torch.full((L, B), float("nan"), dtype=torch.float32, device=dev)
    lo = torch.full((L, B), float("nan"), dtype=torch.float32, device=dev) if want_lo else None
    ws = torch.full((_lib.predict_yquantiles_workspace_bytes(n, B, L) // 4,), ws_fill, dtype=torch.float32, device=dev)
    assert ws.data_ptr() % 8 == 0
    wd = _weights_tensor(w, dev)
    stem, args = _model_args(case, a, th, X)
    _lib.call("stein_predict_%s_yquantiles" % stem, *args, (ctypes.c_double * L)(*lv), L, passes,
              None if wd is None else wd.data_ptr(), hi.data_ptr(), None if lo is None else lo.data_ptr(), ws.data_ptr(),
              ws.numel() * 4, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return lo, hi


def same_bits(a, b):
    import torch
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))
