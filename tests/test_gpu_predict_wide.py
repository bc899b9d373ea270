"""GPU: the network's predictive producers for more than four input features (k_predict_bnn_wide of csrc/stein_predict.hip:
stein_predict_bnn_wide and stein_predict_bnn_wide_weighted through the C ABI), element by element of pred, mean, var and lpd
against the fp64 references of tests/predict_ref.py, evaluated in torch fp64 on the device, inside that reference's a-priori
fp32 allowance (a derivation; no tolerance relative to the largest entry).

The cases (tests/bnn_wide_cases.py; tests/test_bnn_wide_cases.py checks on the CPU that they reach every edge of the staging
unit): the issue's table; hidden units at one staging unit of 16, one past it and more than two units; 16 | 15 | 11 | 3
particles per staging unit; particle counts around PR_PASS and around a staging unit; rows around a row tile.

Every case runs on a NaN-filled workspace and NaN-filled outputs and asserts: all finite, |got - ref| <= allowance
elementwise, a second call bit-identical, and the summaries against fp64 statistics of the call's OWN pred (reduction terms
only).  Then: pred is bit-identical for subsets of the particles and of the rows; the weighted form stays inside
tests/predict_weighted_cases.reference on three weight patterns; three inputs through the wide entry points give the narrow
entry points' bits; and the order-statistic and y methods of BnnPredict raise for a wide producer.
Each prints max |err| / allowance (run with -s)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from stein_amd import _lib
from stein_amd.predict import BnnPredict

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bnn_wide_cases as wc  # noqa: E402
import predict_cases as pc  # noqa: E402
import predict_weighted_cases as pwc  # noqa: E402

pytestmark = pytest.mark.gpu
OUTPUTS = ("pred", "mean", "var", "lpd")
GUARD = -12345.5


def _call(case, a, dev, want=OUTPUTS, ws_fill=float("nan"), fill=float("nan"), w=None, theta=None, X=None, y=None, wide=True):
    """one call through the C ABI (w: the weighted entry point) -> {name: tensor}"""
    th = torch.tensor(a["theta"], dtype=torch.float32, device=dev) if theta is None else theta
    X = torch.tensor(a["X"], dtype=torch.float32, device=dev) if X is None else X
    y = torch.tensor(a["y"], dtype=torch.float32, device=dev) if y is None else y
    n, B = th.shape[0], X.shape[0]
    bufs = dict(pred=torch.full((n, B), fill, dtype=torch.float32, device=dev))
    for k in OUTPUTS[1:]:
        bufs[k] = torch.full((B,), fill, dtype=torch.float32, device=dev)
    bufs["ess"] = torch.full((1,), fill, dtype=torch.float64, device=dev)
    weighted = w is not None
    nbytes = _lib.predict_weighted_workspace_bytes(n, B) if weighted else _lib.predict_workspace_bytes(n, B)
    ws = torch.full((nbytes // 4,), ws_fill, dtype=torch.float32, device=dev)
    ptr = [bufs[k].data_ptr() if k in want else None for k in OUTPUTS]
    summary = weighted or any(k in want for k in OUTPUTS[1:])
    tail = [ws.data_ptr() if summary else None, ws.numel() * 4 if summary else 0, torch.cuda.current_stream(dev).cuda_stream]
    yp = y.data_ptr() if "lpd" in want else None
    wd = torch.as_tensor(np.asarray(w, np.float64), device=dev) if weighted else None
    wp, ep = ([wd.data_ptr()], [bufs["ess"].data_ptr()]) if weighted else ([], [])
    name = "stein_predict_bnn" + ("_wide" if wide else "") + ("_weighted" if weighted else "")
    _lib.call(name, th.data_ptr(), n, a["d"], case["n_in"], case["H"], (ctypes.c_int64 * 6)(*a["cols"]), _lib.PRED_LINK,
              X.data_ptr(), yp, B, *wp, *ptr, *ep, *tail)
    torch.cuda.synchronize()
    return bufs


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _inside(tag, got, ref, what, keys):
    for k in keys:
        val, allow = (torch.as_tensor(v).to(got[k].device) for v in ref[k])
        assert bool(torch.isfinite(val).all()) and bool(torch.isfinite(allow).all()), k
        assert bool(torch.isfinite(got[k]).all()), "%s: non-finite entries (or entries never written)" % k
        err = (got[k].double() - val).abs().reshape(-1)
        allow = allow.reshape(-1)
        pos = allow > 0                                      # (n = 1: the variance and its allowance are exactly 0)
        ratio = float((err[pos] / allow[pos]).max()) if bool(pos.any()) else 0.0
        print("%-18s %-4s %s max |err| / allowance = %.3f" % (tag, k, what, ratio))
        assert bool((err <= allow).all()), "%s outside the allowance (%s): ratio %.3g" % (k, what, ratio)


@pytest.mark.parametrize("case", wc.PRED_CASES, ids=lambda c: c["name"])
def test_every_case_inside_the_allowance_and_repeatable(cuda, case):
    a = pc.args(case)
    to = lambda v: torch.tensor(v, dtype=torch.float64, device=cuda)   # noqa: E731
    got = _call(case, a, cuda)
    again = _call(case, a, cuda, ws_fill=0.0)
    _inside(case["name"], got, pc.reference(case, a, to=to), "vs reference", OUTPUTS)
    for k in OUTPUTS:
        assert _same(got[k], again[k]), "%s: a second call (on another workspace) differs" % k
    if case["n"] == 1:
        assert bool((got["var"] == 0).all())
    # the summaries are of the values pred holds: reduction terms only
    own = got["pred"].double()
    _inside(case["name"], got, pc.reference(case, a, to=to, z=own, f=own), "vs own pred", OUTPUTS[1:])


def test_pred_does_not_depend_on_the_other_particles_or_rows(cuda):
    case = wc.PRED_SUBSET_CASE
    a = pc.args(case)
    th, X, y = (torch.tensor(a[k], dtype=torch.float32, device=cuda) for k in ("theta", "X", "y"))
    full = _call(case, a, cuda)
    assert bool(torch.isfinite(full["pred"]).all())
    n, B = case["n"], case["B"]
    assert n > 2 * pc.PR_PASS and B > pc.PR_ROWS             # the full call walks several passes and two row tiles
    for ps in (slice(0, 1), slice(5, 6), slice(n - 1, n), slice(3, 3 + pc.PR_PASS + 1), slice(0, n, 2)):
        part = _call(case, a, cuda, want=("pred",), theta=th[ps].contiguous())
        assert _same(part["pred"], full["pred"][ps]), "pred of the particles %s alone differs" % (ps,)
    for rs in (slice(0, 1), slice(B - 1, B), slice(pc.PR_ROWS - 3, pc.PR_ROWS + 2), slice(1, B, 3)):
        part = _call(case, a, cuda, want=("pred",), X=X[rs].contiguous(), y=y[rs].contiguous())
        assert _same(part["pred"], full["pred"][:, rs]), "pred of the rows %s alone differs" % (rs,)
    only = _call(case, a, cuda, want=("pred",), fill=GUARD)  # pred alone needs no workspace and touches nothing else
    assert _same(only["pred"], full["pred"]) and all(bool((only[k] == GUARD).all()) for k in OUTPUTS[1:])
    summaries = _call(case, a, cuda, want=OUTPUTS[1:], fill=GUARD)
    assert all(_same(summaries[k], full[k]) for k in OUTPUTS[1:]) and bool((summaries["pred"] == GUARD).all())


@pytest.mark.parametrize("pair", wc.PRED_WEIGHTED, ids=pwc.pair_id)
def test_the_weighted_form(cuda, pair):
    case, pat = pair
    a = pc.args(case)
    assert pwc.applies(case, pat)
    w = pwc.weights(case, pat, a)
    to = lambda v: torch.tensor(v, dtype=torch.float64, device=cuda)   # noqa: E731
    keys = OUTPUTS + ("ess",)
    got = _call(case, a, cuda, w=w)
    again = _call(case, a, cuda, w=w, ws_fill=3.0e38)
    tag = pwc.pair_id(pair)
    _inside(tag, got, pwc.reference(case, a, w, to=to), "vs reference", keys)
    for k in keys:
        assert _same(got[k], again[k]), "%s: a second call differs" % k
    plain = _call(case, a, cuda)
    assert _same(got["pred"], plain["pred"]), "pred depends on the weights"
    own = got["pred"].double()
    _inside(tag, got, pwc.reference(case, a, w, to=to, z=own, f=own), "vs own pred", OUTPUTS[1:])
    if (w == 0).any():                                       # a particle of weight zero is skipped
        th = torch.tensor(a["theta"], dtype=torch.float32, device=cuda)
        dead = torch.tensor(np.flatnonzero(w == 0), device=cuda)
        th[dead[0::2]] = float("nan")
        th[dead[1::2]] = float("inf")
        hurt = _call(case, a, cuda, w=w, theta=th)
        for k in OUTPUTS[1:] + ("ess",):
            assert _same(got[k], hurt[k]), "%s reads a particle of weight zero" % k
    bad = np.array(w)
    bad[len(bad) // 2] = -1e-3                               # bad weights: NaN rows with STEIN_OK (_lib.call raises otherwise)
    poisoned = _call(case, a, cuda, w=bad)
    assert all(bool(torch.isnan(poisoned[k]).all()) for k in OUTPUTS[1:] + ("ess",)) and _same(poisoned["pred"], plain["pred"])


def test_three_inputs_through_the_wide_entry_points_are_the_narrow_entry_points_bits(cuda):
    case = pc._case("narrow_through_wide", "bnn", 37, 300, n_in=3, H=65)
    a = pc.args(case)
    w = pwc.weights(case, "positive", a)
    for weights in (None, w):
        narrow = _call(case, a, cuda, w=weights, wide=False)
        wide = _call(case, a, cuda, w=weights, wide=True)
        for k in OUTPUTS + (("ess",) if weights is not None else ()):
            assert bool(torch.isfinite(narrow[k]).all()) and _same(narrow[k], wide[k]), k


def test_the_rank_and_y_methods_raise_for_a_wide_producer(cuda):
    case = wc.PRED_TABLE[1]
    a = pc.args(case)
    th, X, y = (torch.tensor(a[k], dtype=torch.float32, device=cuda) for k in ("theta", "X", "y"))
    prod = BnnPredict(case["n_in"], case["H"], a["cols"])
    feed = {"X": X, "y": y}
    w = torch.ones(case["n"], dtype=torch.float64, device=cuda)
    calls = dict(quantiles=lambda: prod.quantiles(th, feed, (0.5,)), order_statistics=lambda: prod.order_statistics(th, feed, (0,)),
                 weighted_quantiles=lambda: prod.weighted_quantiles(th, feed, w, (0.5,)), y_cdf=lambda: prod.y_cdf(th, feed),
                 y_quantiles=lambda: prod.y_quantiles(th, feed, (0.5,)))
    for name, call in calls.items():
        with pytest.raises(ValueError) as info:
            call()
        msg = str(info.value)
        assert name in msg and "n_in <= 4" in msg and "function_posterior" in msg, msg
    # what runs through the summary launch works, and is the C ABI's result
    got = _call(case, a, cuda)
    mean, var, lpd = prod.summary(th, feed)
    assert _same(prod(th, feed), got["pred"]) and _same(mean, got["mean"]) and _same(var, got["var"]) and _same(lpd, got["lpd"])
    wm, wv, wl, ess = prod.weighted_summary(th, feed, w)
    assert all(bool(torch.isfinite(t).all()) for t in (wm, wv, wl, ess)) and float(ess) == pytest.approx(case["n"])
