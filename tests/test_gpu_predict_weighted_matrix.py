"""GPU: the weighted predictive summaries (csrc/stein_predict.hip, stein_predict_*_weighted) through the C ABI across the
cases of tests/predict_cases.py crossed with the weight patterns of tests/predict_weighted_cases.py, element by element of
mean, var, lpd and ess against the fp64 references of tests/predict_weighted_ref.py, evaluated in torch fp64 on the device,
inside that reference's a-priori allowance (a derivation; tests/test_predict_weighted_ref.py checks it on the CPU).

Every (case, pattern) prefills the outputs and the workspace with NaN and asserts: all finite; |got - ref| <= allowance
elementwise; the same against weighted fp64 statistics of the kernel's OWN pred, where the allowance holds the reduction
terms only; pred bit-identical to the unweighted call's; a second call bit-identical; the weights times 2^200 and 2^-200
bit-identical; and, by pattern,
  one_hot      mean bit-equal to pred[p], var == 0 exactly, ess == 1
  uniform      within the sum of the two allowances of the unweighted call's results
  counts       within the sum of the two allowances of the unweighted call on theta.repeat_interleave(counts)
  any zeros    NaN / inf in the theta rows of the zero-weight particles leaves every summary bit-identical
Then: bad weight vectors give NaN everywhere with STEIN_OK; every output subset matches the full call and touches nothing
else; the result does not depend on what the workspace held and no word past the plan is written.
Each prints max |err| / allowance (run with -s)."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest
import torch

from stein_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_cases as pc  # noqa: E402
import predict_weighted_cases as pwc  # noqa: E402

pytestmark = pytest.mark.gpu
OUTPUTS = ("pred", "mean", "var", "lpd", "ess")
SUMMARIES = ("mean", "var", "lpd")
GUARD = -12345.5


def _inputs(a, dev):
    return tuple(torch.tensor(a[k], dtype=torch.float32, device=dev) for k in ("theta", "X", "y"))


def _call(case, a, w, dev, want=OUTPUTS, ws_fill=float("nan"), fill=float("nan"), theta=None):
    """one weighted call through the C ABI (w = None: the unweighted entry point) -> ({name: tensor}, workspace as float32 words)"""
    th, X, y = _inputs(a, dev)
    if theta is not None:
        th = theta
    n, B = th.shape[0], case["B"]
    bufs = dict(pred=torch.full((n, B), fill, dtype=torch.float32, device=dev))
    for k in SUMMARIES:
        bufs[k] = torch.full((B,), fill, dtype=torch.float32, device=dev)
    bufs["ess"] = torch.full((1,), fill, dtype=torch.float64, device=dev)
    weighted = w is not None
    nbytes = _lib.predict_weighted_workspace_bytes(n, B) if weighted else _lib.predict_workspace_bytes(n, B)
    ws = torch.full((nbytes // 4,), ws_fill, dtype=torch.float32, device=dev)
    assert ws.data_ptr() % 8 == 0
    ptr = {k: bufs[k].data_ptr() if k in want else None for k in OUTPUTS}
    summary = any(k in want for k in (SUMMARIES + ("ess",) if weighted else SUMMARIES))
    tail = [ws.data_ptr() if summary else None, ws.numel() * 4 if summary else 0, torch.cuda.current_stream(dev).cuda_stream]
    yp = y.data_ptr() if "lpd" in want else None
    out = _lib.PRED_MEAN if case["output"] == "mean" else _lib.PRED_LINK
    wd = torch.as_tensor(np.asarray(w, np.float64), device=dev) if weighted else None
    wp, ep = ([wd.data_ptr()], [ptr["ess"]]) if weighted else ([], [])
    outs = [ptr["pred"], ptr["mean"], ptr["var"], ptr["lpd"]]
    suffix = "_weighted" if weighted else ""
    if case["model"] == "bnn":
        _lib.call("stein_predict_bnn" + suffix, th.data_ptr(), n, a["d"], case["n_in"], case["H"], (ctypes.c_int64 * 6)(*a["cols"]),
                  out, X.data_ptr(), yp, B, *wp, *outs, *ep, *tail)
    else:
        kind = _lib.GLM_LINEAR if case["model"] == "linear" else _lib.GLM_LOGISTIC
        _lib.call("stein_predict_glm" + suffix, th.data_ptr(), n, a["d"], kind, out, a["w_col"], case["F"], X.data_ptr(), yp, B,
                  float(case["tau"]), *wp, *outs, *ep, *tail)
    torch.cuda.synchronize()
    return bufs, ws


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _ratio(err, allow):
    pos = allow > 0
    return float((err[pos] / allow[pos]).max()) if bool(pos.any()) else 0.0


def _inside(tag, got, ref, what, keys):
    for k in keys:
        val, allow = ref[k]
        val, allow = torch.as_tensor(val), torch.as_tensor(allow)
        assert bool(torch.isfinite(val).all()) and bool(torch.isfinite(allow).all()), k
        assert bool(torch.isfinite(got[k]).all()), "%s: non-finite entries (or entries never written)" % k
        err = (got[k].double() - val.to(got[k].device)).abs()
        allow = allow.to(got[k].device)
        print("%-30s %-4s %s max |err| / allowance = %.3f" % (tag, k, what, _ratio(err.reshape(-1), allow.reshape(-1))))
        assert bool((err <= allow).all()), "%s outside the allowance (%s): ratio %.3g" % (k, what, _ratio(err.reshape(-1), allow.reshape(-1)))


def _close(tag, what, got, other, allow_a, allow_b, keys=SUMMARIES):
    """two computed results of one exact value: apart by at most the sum of their allowances"""
    for k in keys:
        err = (got[k].double() - other[k].double()).abs()
        allow = torch.as_tensor(allow_a[k][1]).to(err.device) + torch.as_tensor(allow_b[k][1]).to(err.device)
        print("%-30s %-4s %s max |diff| / (sum of allowances) = %.3f" % (tag, k, what, _ratio(err, allow)))
        assert bool((err <= allow).all()), (k, what, _ratio(err, allow))


@pytest.mark.parametrize("pair", pwc.CROSSED, ids=pwc.pair_id)
def test_every_case_under_every_weight_pattern(cuda, pair):
    case, pat = pair
    dev, tag = cuda, pwc.pair_id(pair)
    a = pc.args(case)
    w = pwc.weights(case, pat, a)
    to = lambda v: torch.tensor(v, dtype=torch.float64, device=dev)   # noqa: E731
    got, _ = _call(case, a, w, dev)
    again, _ = _call(case, a, w, dev)
    ref = pwc.reference(case, a, w, to=to)
    _inside(tag, got, ref, "vs reference", OUTPUTS)
    for k in OUTPUTS:
        assert _same(got[k], again[k]), "%s: a second call differs" % k
    plain, _ = _call(case, a, None, dev)
    assert _same(got["pred"], plain["pred"]), "pred depends on the weights"
    # the summaries are of the values pred holds (tests/test_gpu_predict_matrix.py): reduction terms only
    z = got["pred"] if case["output"] == "link" else _call(dict(case, output="link"), a, None, dev)[0]["pred"]
    _inside(tag, got, pwc.reference(case, a, w, to=to, z=z.double(), f=got["pred"].double()), "vs own pred", SUMMARIES)
    for scale in (2.0 ** 200, 2.0 ** -200):
        scaled, _ = _call(case, a, w * scale, dev)
        for k in OUTPUTS:
            assert _same(got[k], scaled[k]), "%s changes under a power-of-two rescaling of the weights" % k
    if pat.startswith("one_hot"):
        p = int(np.argmax(w))
        assert _same(got["mean"], got["pred"][p]) and bool((got["var"] == 0).all()) and float(got["ess"]) == 1.0
    if pat == "uniform":
        assert float(got["ess"]) == pytest.approx(case["n"], rel=1e-12)
        _close(tag, "vs unweighted", got, plain, ref, pc.reference(case, a, to=to))
    if pat == "counts":
        counts = torch.tensor(w, dtype=torch.int64, device=dev)
        th = _inputs(a, dev)[0]
        rep_case = dict(case, n=int(counts.sum()))
        rep_a = dict(a, theta=np.repeat(a["theta"], np.asarray(w, np.int64), axis=0))
        rep, _ = _call(rep_case, rep_a, None, dev, theta=th.repeat_interleave(counts, dim=0).contiguous())
        _close(tag, "vs unweighted on the repeated sample", got, rep, ref, pc.reference(rep_case, rep_a, to=to))
    if (w == 0).any():
        th = _inputs(a, dev)[0].clone()
        dead = torch.tensor(np.flatnonzero(w == 0), device=dev)
        th[dead[0::2]] = float("nan")
        th[dead[1::2]] = float("inf")
        hurt, _ = _call(case, a, w, dev, theta=th)
        for k in SUMMARIES + ("ess",):
            assert _same(got[k], hurt[k]), "%s reads a particle of weight zero" % k
        live = torch.tensor(np.flatnonzero(w > 0), device=dev)
        assert _same(got["pred"][live], hurt["pred"][live])


@pytest.mark.parametrize("kind", pwc.BAD)
@pytest.mark.parametrize("case", [pc.COUNTS[4], pc.COUNTS[11], pc.ARMS[5]], ids=lambda c: c["name"])
def test_bad_weights_give_nan_and_ok(cuda, case, kind):
    a = pc.args(case)
    w = pwc.bad_weights(case["n"], kind)
    got, _ = _call(case, a, w, cuda, fill=GUARD)           # _lib.call raises unless the code is STEIN_OK
    for k in SUMMARIES + ("ess",):
        assert bool(torch.isnan(got[k]).all()), (k, kind)
    plain, _ = _call(case, a, None, cuda)
    assert _same(got["pred"], plain["pred"])               # pred does not depend on the weights, bad ones included
    only_ess, _ = _call(case, a, w, cuda, want=("ess",), fill=GUARD)
    assert bool(torch.isnan(only_ess["ess"]).all())


def test_every_output_subset_matches_the_full_call_and_touches_nothing_else(cuda):
    case, pat = pwc.SUBSET
    a = pc.args(case)
    w = pwc.weights(case, pat, a)
    full, _ = _call(case, a, w, cuda)
    assert all(bool(torch.isfinite(full[k]).all()) for k in OUTPUTS)
    subsets = [s for r in range(1, 6) for s in itertools.combinations(OUTPUTS, r)]
    assert len(subsets) == 31
    for want in subsets:
        got, _ = _call(case, a, w, cuda, want=want, fill=GUARD)
        for k in OUTPUTS:
            if k in want:
                assert _same(got[k], full[k]), (want, k)
            else:
                assert bool((got[k] == GUARD).all()), "%s was not asked for in %s but was written" % (k, want)


@pytest.mark.parametrize("pair", [(pc.COUNTS[5], "zero_slices"), (pc.COUNTS[11], "wide"), (pc.ARMS[5], "positive"),
                                  (pc.COUNTS[12], "counts")], ids=pwc.pair_id)
def test_result_does_not_depend_on_what_the_workspace_held(cuda, pair):
    case, pat = pair
    a = pc.args(case)
    w = pwc.weights(case, pat, a)
    nan1, ws1 = _call(case, a, w, cuda, ws_fill=float("nan"))
    nan2, _ = _call(case, a, w, cuda, ws_fill=float("nan"))
    zero, _ = _call(case, a, w, cuda, ws_fill=0.0)
    junk, _ = _call(case, a, w, cuda, ws_fill=3.0e38)
    for k in OUTPUTS:
        assert bool(torch.isfinite(nan1[k]).all()), k
        assert _same(nan1[k], nan2[k]) and _same(nan1[k], zero[k]) and _same(nan1[k], junk[k]), k
    head, states = pwc.used_bytes(case["n"], case["B"])
    assert head + states <= ws1.numel() * 4
    assert bool(torch.isfinite(ws1[:head // 4].view(torch.float64)).all())
    assert bool(torch.isfinite(ws1[head // 4:(head + states) // 4]).all())
    assert bool(torch.isnan(ws1[(head + states) // 4:]).all())         # and it writes no word past its plan
