"""GPU: the predictive producers (csrc/stein_predict.hip) through the C ABI across their whole dispatch domain, element by
element of pred, mean, var and lpd against the fp64 references of tests/predict_ref.py, evaluated in torch fp64 on the
device, inside that reference's a-priori fp32 allowance (a derivation; no tolerance relative to the largest entry).

The cases (tests/predict_cases.py; tests/test_predict_ref.py checks on the CPU that they reach every instantiation and arm):
  arms      both sides of every feature / hidden chunk edge, the four network instantiations, three models, both outputs,
            model columns before / between / after spare columns
  counts    n = 1, around one pass of a slice, and just past cap * pass (1024 slices of two passes); 223 slices at 2049 rows
  rows      batch = 1 and around one row tile
  cond      a common output offset of 10^3 with a spread of 10^-2; log likelihoods below -10^3 spread over 200 nats;
            logits up to 90 on both sides read out as probabilities

Every case prefills the outputs and the workspace with NaN and asserts: all finite, |got - ref| <= allowance elementwise, a
second call bit-identical.  Then the summaries are checked against fp64 statistics of the kernel's OWN pred, where the
allowance holds the reduction terms only.  Each prints max |err| / allowance (run with -s)."""
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

pytestmark = pytest.mark.gpu
OUTPUTS = ("pred", "mean", "var", "lpd")
GUARD = -12345.5


def _call(case, a, dev, want=OUTPUTS, ws_fill=float("nan"), fill=float("nan")):
    """one call through the C ABI -> ({name: tensor} for all four buffers, workspace)"""
    th, X, y = (torch.tensor(a[k], dtype=torch.float32, device=dev) for k in ("theta", "X", "y"))
    n, B = case["n"], case["B"]
    bufs = dict(pred=torch.full((n, B), fill, dtype=torch.float32, device=dev))
    for k in OUTPUTS[1:]:
        bufs[k] = torch.full((B,), fill, dtype=torch.float32, device=dev)
    ws = torch.full((_lib.predict_workspace_bytes(n, B) // 4,), ws_fill, dtype=torch.float32, device=dev)
    ptr = [bufs[k].data_ptr() if k in want else None for k in OUTPUTS]
    summary = any(k in want for k in OUTPUTS[1:])
    tail = [ws.data_ptr() if summary else None, ws.numel() * 4 if summary else 0, torch.cuda.current_stream(dev).cuda_stream]
    yp = y.data_ptr() if "lpd" in want else None
    out = _lib.PRED_MEAN if case["output"] == "mean" else _lib.PRED_LINK
    if case["model"] == "bnn":
        _lib.call("stein_predict_bnn", th.data_ptr(), n, a["d"], case["n_in"], case["H"], (ctypes.c_int64 * 6)(*a["cols"]), out,
                  X.data_ptr(), yp, B, *ptr, *tail)
    else:
        kind = _lib.GLM_LINEAR if case["model"] == "linear" else _lib.GLM_LOGISTIC
        _lib.call("stein_predict_glm", th.data_ptr(), n, a["d"], kind, out, a["w_col"], case["F"], X.data_ptr(), yp, B,
                  float(case["tau"]), *ptr, *tail)
    torch.cuda.synchronize()
    return bufs, ws


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _inside(case, got, ref, tag, keys=OUTPUTS):
    for k in keys:
        val, allow = ref[k]
        assert bool(torch.isfinite(val).all()) and bool(torch.isfinite(allow).all()), k
        assert bool(torch.isfinite(got[k]).all()), "%s: non-finite entries (or entries never written)" % k
        err = (got[k].double() - val).abs()
        pos = allow > 0                                      # (n = 1: the variance and its allowance are exactly 0)
        ratio = float((err[pos] / allow[pos]).max()) if bool(pos.any()) else 0.0
        print("%-16s %-4s %s max |err| / allowance = %.3f" % (case["name"], k, tag, ratio))
        assert bool((err <= allow).all()), "%s outside the allowance (%s): ratio %.3g" % (k, tag, ratio)


def _check(case, dev):
    a = pc.args(case)
    to = lambda v: torch.tensor(v, dtype=torch.float64, device=dev)   # noqa: E731
    got, _ = _call(case, a, dev)
    again, _ = _call(case, a, dev)
    _inside(case, got, pc.reference(case, a, to=to), "vs reference")
    for k in OUTPUTS:
        assert _same(got[k], again[k]), "%s: a second call differs" % k
    if case["n"] == 1:
        assert bool((got["var"] == 0).all())
    # the summaries are of the values pred holds: mean and var against fp64 statistics of this call's own pred (for
    # output = "mean" the sigmoid's outputs, as the kernel reduced them), lpd against the z the kernel holds -- pred itself
    # with output = "link", else the pred of a link call on the same inputs (the same arithmetic up to z).  Reduction terms only.
    z = got["pred"] if case["output"] == "link" else _call(dict(case, output="link"), a, dev)[0]["pred"]
    _inside(case, got, pc.reference(case, a, to=to, z=z.double(), f=got["pred"].double()), "vs own pred", OUTPUTS[1:])
    return a, got


def _id(case):
    return case["name"]


@pytest.mark.parametrize("case", pc.ARMS, ids=_id)
def test_every_instantiation_and_dispatch_arm(cuda, case):
    _check(case, cuda)


@pytest.mark.parametrize("case", pc.COUNTS, ids=_id)
def test_particle_counts_around_a_pass_and_past_the_slice_cap(cuda, case):
    _check(case, cuda)


@pytest.mark.parametrize("case", pc.ROWS, ids=_id)
def test_row_counts_around_a_row_tile(cuda, case):
    _check(case, cuda)


@pytest.mark.parametrize("case", pc.COND, ids=_id)
def test_conditioning(cuda, case):
    a, got = _check(case, cuda)
    ref = pc.reference(case, a)
    pc.check_conditioning_inputs(case, a, ref)               # preconditions, from the inputs and the reference alone
    if case["flavor"] == "logit_sat":
        assert bool((got["pred"] >= 0).all()) and bool((got["pred"] <= 1).all())
        assert bool((got["mean"] >= 0).all()) and bool((got["mean"] <= 1).all())
    if case["flavor"] == "var_offset":
        assert bool((torch.tensor(ref["var"][1]) < 0.5 * torch.tensor(ref["var"][0])).all())   # the allowance resolves the variance


def test_every_output_subset_matches_the_full_call_and_touches_nothing_else(cuda):
    case = pc.SUBSET_CASE
    a = pc.args(case)
    full, _ = _call(case, a, cuda)
    subsets = [s for r in range(1, 5) for s in itertools.combinations(OUTPUTS, r)]
    assert len(subsets) == 15
    for want in subsets:
        got, _ = _call(case, a, cuda, want=want, fill=GUARD)
        for k in OUTPUTS:
            if k in want:
                assert _same(got[k], full[k]), (want, k)
            else:
                assert bool((got[k] == GUARD).all()), "%s was not asked for in %s but was written" % (k, want)


@pytest.mark.parametrize("case", [pc.COUNTS[5], pc.COUNTS[11], pc.ARMS[5]], ids=_id)
def test_result_does_not_depend_on_what_the_workspace_held(cuda, case):
    a = pc.args(case)
    nan1, ws1 = _call(case, a, cuda, ws_fill=float("nan"))
    nan2, _ = _call(case, a, cuda, ws_fill=float("nan"))
    zero, _ = _call(case, a, cuda, ws_fill=0.0)
    for k in OUTPUTS:
        assert bool(torch.isfinite(nan1[k]).all()), k
        assert _same(nan1[k], nan2[k]) and _same(nan1[k], zero[k]), k
    _, slices, _ = pc.plan(case["n"], case["B"])
    used = slices * pc.PR_STATE * case["B"]
    assert bool(torch.isfinite(ws1[:used]).all()) and bool(torch.isnan(ws1[used:]).all())   # and it writes no word past its plan
