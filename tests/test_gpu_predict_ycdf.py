"""GPU: the predictive distribution function of y (csrc/stein_predict_y.hip, stein_predict_*_ycdf) through the C ABI across
the table of tests/predict_y_cases.py -- the regression cases of tests/predict_cases.py crossed with the weight patterns and
weights=None, 1, 3 or 8 points -- against the fp64 reference of tests/predict_y_ref.py evaluated in torch fp64 on the device,
inside that reference's a-priori allowance a_F (a derivation; tests/test_predict_y_ref.py checks it on the CPU).

Every (case, pattern, count) prefills the output and the workspace with NaN and asserts: every output finite and inside a_F
against the mixture built from the library's OWN pred (z taken as exact: the new code alone) and end to end against the fp64
forward pass with its error dz folded in; a second call and a call on a zero-filled workspace bit-identical; the weights
times 2^40 and 2^-40 bit-identical; NaN / inf in the particles of weight zero change no bit; monotone in t up to the two
allowances; weights=None against all-ones weights within the two allowances.  Then: the device's Phi itself (n = 1, z = 0,
tau = 1) against scipy's ndtr; bad weights give NaN rows with STEIN_OK; the refusals in the header's order.
Each prints max |err| / allowance (run with -s)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from stein_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_cases as pc  # noqa: E402
import predict_weighted_cases as pwc  # noqa: E402
import predict_y_cases as yc  # noqa: E402
import predict_y_ref as yr  # noqa: E402

pytestmark = pytest.mark.gpu


def _ratio(err, allow):
    return float((err / allow).max())


def _inside(tag, what, got, ref, allow):
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(allow).all())
    assert bool(torch.isfinite(got).all()), "%s: non-finite outputs (or outputs never written)" % tag
    err = (got.double() - ref).abs()
    print("%-34s F %s max |err| / allowance = %.3f" % (tag, what, _ratio(err, allow)))
    assert bool((err <= allow).all()), "%s outside the allowance (%s): ratio %.3g" % (tag, what, _ratio(err, allow))


@pytest.mark.parametrize("tr", yc.CROSSED, ids=yc.triple_id)
def test_every_case_pattern_and_count(cuda, tr):
    case, pattern, count = tr
    dev, tag = cuda, yc.triple_id(tr)
    a = pc.args(case)
    w = yc.weights(case, pattern, a)
    to = lambda v: torch.tensor(v, dtype=torch.float64, device=dev)   # noqa: E731
    wt = None if w is None else to(w)
    tensors = yc.device_inputs(a, dev)
    _, slices, per = yc.y_plan(case["n"], case["B"], False)
    z_ref, dz, s = yc.model_parts(case, a, to=to)
    z_own = yc.call_pred(case, a, dev, tensors).double()
    t = torch.tensor(yc.points(case, a, z_own.cpu().numpy(), s.cpu().numpy(), w, count), device=dev)
    got, _ = yc.call_ycdf(case, a, t, w, dev, tensors=tensors)
    # the new code alone: the mixture of the values pred holds; then end to end, the forward pass's error folded in
    ref_own, a_own = yr.cdf(t.double(), z_own, 0.0 * dz, s, wt, case["model"], per, slices)
    _inside(tag, "vs own pred ", got, ref_own, a_own)
    ref, allow = yr.cdf(t.double(), z_ref, dz, s, wt, case["model"], per, slices)
    _inside(tag, "vs reference", got, ref, allow)
    assert bool((got >= 0).all()) and bool((got.double() <= 1 + a_own).all())   # (the fp32 weights may sum to 1 + n u)
    again, _ = yc.call_ycdf(case, a, t, w, dev, tensors=tensors)
    zero, _ = yc.call_ycdf(case, a, t, w, dev, tensors=tensors, ws_fill=0.0)
    assert yc.same_bits(got, again), "a second call differs"
    assert yc.same_bits(got, zero), "the result depends on what the workspace held"
    # monotone in t up to the two allowances
    for i in range(count):
        for j in range(count):
            up = t[i] <= t[j]
            assert bool((got[i].double()[up] <= (got[j].double() + a_own[i] + a_own[j])[up]).all()), (i, j)
    if w is None:
        ones, _ = yc.call_ycdf(case, a, t, np.ones(case["n"]), dev, tensors=tensors)
        a_ones = yr.cdf(t.double(), z_own, 0.0 * dz, s, to(np.ones(case["n"])), case["model"], per, slices)[1]
        assert bool(((got.double() - ones.double()).abs() <= a_own + a_ones).all()), "weights=None against all-ones weights"
        return
    for scale in (2.0 ** 40, 2.0 ** -40):
        scaled, _ = yc.call_ycdf(case, a, t, w * scale, dev, tensors=tensors)
        assert yc.same_bits(got, scaled), "a power-of-two rescaling of the weights changes the result"
    if (w == 0).any():
        th = tensors[0].clone()
        dead = torch.tensor(np.flatnonzero(w == 0), device=dev)
        th[dead[0::2]] = float("nan")
        th[dead[1::2]] = float("inf")
        hurt, _ = yc.call_ycdf(case, a, t, w, dev, tensors=(th, tensors[1]))
        assert yc.same_bits(got, hurt), "a particle of weight zero is read"


def test_the_devices_phi_against_ndtr(cuda):
    """n = 1, z = 0, tau = 1: y_cdf returns the device's Phi(t) = erfcf(-t / sqrt 2) / 2 itself.  8 x 4096 points over [-9, 9]."""
    from scipy.special import ndtr
    B = 4096
    case = pc._case("phi_itself", "linear", 1, B, F=1, tau=1.0)
    w_col, _, d = yc.sc.glm_layout(1, None)
    a = dict(theta=np.zeros((1, d)), X=np.ones((B, 1)), y=np.zeros(B), d=d, w_col=w_col)
    grid = np.linspace(-9.0, 9.0, 8 * B).astype(np.float32).reshape(8, B)
    got, _ = yc.call_ycdf(case, a, torch.tensor(grid, device=cuda), None, cuda)
    got = got.cpu().numpy().astype(np.float64)
    ref = ndtr(grid.astype(np.float64))
    allow = yr.cdf(grid.astype(np.float64), np.zeros((1, B)), np.zeros((1, B)), np.ones(1), None, "linear", 1, 1)[1]
    err = np.abs(got - ref)
    rel = err[ref > 0] / ref[ref > 0]
    print("device Phi vs ndtr over [-9, 9]: largest |err| = %.3f ulp of 1 (2^-23), largest relative error = %.3g u, "
          "|err| / allowance = %.3f; charged: erfcf %d u of the %.1f u allowed" %
          (err.max() / 2.0 ** -23, rel.max() / yr.U, (err / allow).max(), yr.ERFC_U, allow.min() / yr.U))
    assert (err <= allow).all(), float((err / allow).max())
    assert err.max() <= yr.ERFC_U * yr.U, "the device's erfcf errs by more than the 16 ulp it is charged"


@pytest.mark.parametrize("kind", pwc.BAD)
@pytest.mark.parametrize("case", [yc.EVERY[4], yc.SINGLE[1]], ids=lambda c: c["name"])
def test_bad_weights_give_nan_rows_and_ok(cuda, case, kind):
    a = pc.args(case)
    t = torch.zeros(3, case["B"], dtype=torch.float32, device=cuda)
    got, _ = yc.call_ycdf(case, a, t, pwc.bad_weights(case["n"], kind), cuda, fill=-5.0)   # raises unless STEIN_OK
    assert bool(torch.isnan(got).all()), kind


def test_refusals_in_order(cuda):
    case = yc.SINGLE[0]
    assert case["model"] == "linear"
    a = pc.args(case)
    th, X = yc.device_inputs(a, cuda)
    n, B, d, F = case["n"], case["B"], a["d"], case["F"]
    t = torch.zeros(2, B, dtype=torch.float32, device=cuda)
    out = torch.full((2, B), -5.0, dtype=torch.float32, device=cuda)
    nbytes = _lib.predict_ycdf_workspace_bytes(n, B, 2)
    ws = torch.zeros(nbytes // 4 + 2, dtype=torch.float32, device=cuda)
    stream = torch.cuda.current_stream(cuda).cuda_stream
    good = dict(theta=th.data_ptr(), n=n, d=d, kind=_lib.GLM_LINEAR, w_col=a["w_col"], F=F, X=X.data_ptr(), B=B, tau=1.0,
                t=t.data_ptr(), n_pts=2, w=None, out=out.data_ptr(), ws=ws.data_ptr(), ws_bytes=nbytes)

    def call(**over):
        g = dict(good, **over)
        rc = _lib.load().stein_predict_glm_ycdf(g["theta"], g["n"], g["d"], g["kind"], g["w_col"], g["F"], g["X"], g["B"],
                                                g["tau"], g["t"], g["n_pts"], g["w"], g["out"], g["ws"], g["ws_bytes"], stream)
        return rc, _lib.load().stein_last_error().decode()
    assert call()[0] == _lib.OK
    bad_everything = dict(theta=None, n_pts=0, n=0, kind=7, w_col=d, F=F, tau=-1.0, ws=None)
    # each refusal with every later one still present: the order is the header's
    steps = [("theta", _lib.E_BADARG, "NULL"), ("n_pts", _lib.E_BADARG, "n_pts 0"), ("n", _lib.E_SHAPE, "bad shape"),
             ("kind", _lib.E_BADARG, "kind 7"), ("w_col", _lib.E_SHAPE, "do not fit"), ("tau", _lib.E_BADARG, "noise_precision"),
             ("ws", _lib.E_WORKSPACE, "workspace")]
    over = dict(bad_everything)
    over.pop("F")
    for key, code, text in steps:
        rc, msg = call(**over)
        assert rc == code and text in msg, (key, rc, msg)
        over.pop(key)
    assert call(**over)[0] == _lib.OK
    for ptr in ("theta", "X", "t", "out"):
        assert call(**{ptr: None})[0] == _lib.E_BADARG
    rc, msg = call(kind=_lib.GLM_LOGISTIC, tau=-1.0, n_pts=9)
    assert rc == _lib.E_UNSUPPORTED and 'output="mean"' in msg            # ahead of noise_precision and of the point count
    rc, msg = call(tau=float("nan"), n_pts=9)
    assert rc == _lib.E_BADARG and "noise_precision" in msg
    rc, msg = call(n_pts=9, ws=None)
    assert rc == _lib.E_UNSUPPORTED and "more than 8 points" in msg
    assert call(ws_bytes=nbytes - 8)[0] == _lib.E_WORKSPACE and call(ws=ws.data_ptr() + 4)[0] == _lib.E_WORKSPACE
    assert call(F=1025, w_col=0, d=2000)[0] in (_lib.E_UNSUPPORTED, _lib.E_SHAPE)
    # the quantiles: a level outside (0, 1) and the passes, behind the level count and ahead of the workspace
    hi = torch.empty(8, B, dtype=torch.float32, device=cuda)

    def callq(levels, passes, ws_ptr=ws.data_ptr(), kind=_lib.GLM_LINEAR):
        L = len(levels)
        rc = _lib.load().stein_predict_glm_yquantiles(th.data_ptr(), n, d, kind, a["w_col"], F, X.data_ptr(), B, 1.0,
                                                      (ctypes.c_double * max(L, 1))(*levels), L, passes, None, hi.data_ptr(), None,
                                                      ws_ptr, _lib.predict_yquantiles_workspace_bytes(n, B, max(1, min(L, 8))),
                                                      stream)
        return rc, _lib.load().stein_last_error().decode()
    big = torch.zeros(_lib.predict_yquantiles_workspace_bytes(n, B, 8) // 4, dtype=torch.float32, device=cuda)
    assert callq([0.5], 8, big.data_ptr())[0] == _lib.OK
    assert callq([], 8, big.data_ptr())[0] == _lib.E_BADARG
    assert callq([0.5] * 9, 0, None)[0] == _lib.E_UNSUPPORTED
    for bad in (0.0, 1.0, float("nan"), -0.1, 1.5):
        rc, msg = callq([0.5, bad], 0, None)
        assert rc == _lib.E_BADARG and "level" in msg, bad
    for passes in (0, 13):
        rc, msg = callq([0.5], passes, None)
        assert rc == _lib.E_BADARG and "passes" in msg
    assert callq([0.5], 8, None)[0] == _lib.E_WORKSPACE
    assert callq([0.5], 8, big.data_ptr(), kind=_lib.GLM_LOGISTIC)[0] == _lib.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out[:, 0] != -5.0).all())            # (the good calls wrote; the refused ones launched nothing)
