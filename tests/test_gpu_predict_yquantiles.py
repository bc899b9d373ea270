"""GPU: the quantiles of the predictive distribution of y (csrc/stein_predict_y.hip, stein_predict_*_yquantiles) through the C
ABI across the table of tests/predict_y_cases.py, 1, 3 or 8 levels (10^-6 and 0.5 among them), against the contract of
include/steinhip.h.  For every (case, pattern, count) and level, with the call's bracket [lo, hi] after 8 passes:
  lo <= hi;
  hi - lo <= (hi0 - lo0) / 8^passes + ulp, hi0 - lo0 taken as eight times the width a passes=1 call returns
  (predict_y_ref.width_bound);
  lo <= Q64(q + a_F) and hi >= Q64(q - a_F): Q64 an fp64 bisection of the reference mixture on the device, built from the
  library's OWN pred (z exact), a_F the allowance of F-hat at the end in question (tests/predict_y_ref.py).  A level below
  a_F makes the lower condition vacuous; every case carries the level 0.5, for which both bind (asserted);
  the same end to end: the mixture from the fp64 forward pass, its error dz folded into a_F as |dz| s phi_max;
  the 8-pass bracket lies inside the 1-pass bracket; a second call and a zero-filled workspace change no bit; a level's rows
  do not depend on which other levels share the call.
Then the planted mixtures with closed-form quantiles (identical particles, n = 1, a symmetric pair, modes at +-40 with
sigma = 0.1, a NaN particle of weight zero, a bracket that collapses before the last of 12 passes), and bad weights.
Each prints the largest width in ulp and how close the ends come to the contract (run with -s)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_cases as pc  # noqa: E402
import predict_weighted_cases as pwc  # noqa: E402
import predict_y_cases as yc  # noqa: E402
import predict_y_ref as yr  # noqa: E402

pytestmark = pytest.mark.gpu
PASSES = 8


def _contract(tag, what, case, lo, hi, levels, z, dz, s, wt, per, slices):
    """lo <= Q64(q + a_F(lo)) and hi >= Q64(q - a_F(hi)) per level; -> whether both conditions bound at the level 0.5"""
    bound_both = False
    for i, q in enumerate(levels):
        a_hi = yr.cdf(hi[i:i + 1].double(), z, dz, s, wt, case["model"], per, slices)[1][0]
        a_lo = yr.cdf(lo[i:i + 1].double(), z, dz, s, wt, case["model"], per, slices)[1][0]
        q_minus = yr.quantile64(q - a_hi, z, s, wt)[0]
        q_plus = yr.quantile64(q + a_lo, z, s, wt)[1]
        assert bool((hi[i].double() >= q_minus).all()), "%s %s: hi < Q64(q - a_F) at level %g" % (tag, what, q)
        assert bool((lo[i].double() <= q_plus).all()), "%s %s: lo > Q64(q + a_F) at level %g" % (tag, what, q)
        if q == 0.5:
            bound_both = bool(torch.isfinite(q_minus).all()) and bool(torch.isfinite(q_plus).all())
    return bound_both


def _width_ok(tag, lo, hi, lo1, hi1, passes):
    width = hi.double().cpu().numpy() - lo.double().cpu().numpy()
    bound = yr.width_bound(lo1.cpu().numpy(), hi1.cpu().numpy(), passes)
    ulps = width / np.spacing(np.maximum(np.abs(hi.cpu().numpy()), np.float32(1e-30)))
    print("%-34s largest hi - lo = %.1f ulp of hi; (hi - lo) / bound = %.3f" % (tag, ulps.max(), (width / bound).max()))
    assert (width <= bound).all(), "%s: width / bound = %.4g" % (tag, (width / bound).max())


@pytest.mark.parametrize("tr", yc.CROSSED, ids=yc.triple_id)
def test_every_case_pattern_and_count(cuda, tr):
    case, pattern, count = tr
    dev, tag = cuda, yc.triple_id(tr)
    a = pc.args(case)
    w = yc.weights(case, pattern, a)
    levels = yc.levels(count)
    to = lambda v: torch.tensor(v, dtype=torch.float64, device=dev)   # noqa: E731
    wt = None if w is None else to(w)
    tensors = yc.device_inputs(a, dev)
    _, slices, per = yc.y_plan(case["n"], case["B"], True)
    lo, hi = yc.call_yquantiles(case, a, levels, PASSES, w, dev, tensors=tensors)
    lo1, hi1 = yc.call_yquantiles(case, a, levels, 1, w, dev, tensors=tensors)
    assert bool(torch.isfinite(lo).all()) and bool(torch.isfinite(hi).all()), "non-finite ends (or ends never written)"
    assert bool((lo <= hi).all())
    assert bool((lo1 <= lo).all()) and bool((hi <= hi1).all()), "an end moved outward after the first pass"
    _width_ok(tag, lo, hi, lo1, hi1, PASSES)
    z_ref, dz, s = yc.model_parts(case, a, to=to)
    z_own = yc.call_pred(case, a, dev, tensors).double()
    assert _contract(tag, "vs own pred", case, lo, hi, levels, z_own, 0.0 * dz, s, wt, per, slices), "no level binds both ends"
    _contract(tag, "vs reference", case, lo, hi, levels, z_ref, dz, s, wt, per, slices)
    again = yc.call_yquantiles(case, a, levels, PASSES, w, dev, tensors=tensors)
    zero = yc.call_yquantiles(case, a, levels, PASSES, w, dev, tensors=tensors, ws_fill=0.0)
    only_hi = yc.call_yquantiles(case, a, levels, PASSES, w, dev, tensors=tensors, want_lo=False)[1]
    for got in (again, zero):
        assert yc.same_bits(lo, got[0]) and yc.same_bits(hi, got[1]), "a repeat or the workspace's content changes the result"
    assert yc.same_bits(hi, only_hi)
    if count > 1:                                           # a level's rows do not depend on its company
        alone = yc.call_yquantiles(case, a, levels[1:2], PASSES, w, dev, tensors=tensors)
        rev = yc.call_yquantiles(case, a, levels[::-1], PASSES, w, dev, tensors=tensors)
        assert yc.same_bits(lo[1], alone[0][0]) and yc.same_bits(hi[1], alone[1][0])
        assert yc.same_bits(lo, rev[0].flip(0)) and yc.same_bits(hi, rev[1].flip(0))
    if w is not None and (w == 0).any():
        th = tensors[0].clone()
        th[torch.tensor(np.flatnonzero(w == 0), device=dev)] = float("nan")
        hurt = yc.call_yquantiles(case, a, levels, PASSES, w, dev, tensors=(th, tensors[1]))
        assert yc.same_bits(lo, hurt[0]) and yc.same_bits(hi, hurt[1]), "a particle of weight zero is read"


@pytest.mark.parametrize("plant", yc.planted(), ids=lambda p: p[0])
def test_planted_mixtures(cuda, plant):
    name, case, a, w, levels, expect, passes = plant
    dev = cuda
    to = lambda v: torch.tensor(v, dtype=torch.float64, device=dev)   # noqa: E731
    wt = None if w is None else to(w)
    _, slices, per = yc.y_plan(case["n"], case["B"], True)
    lo, hi = yc.call_yquantiles(case, a, levels, passes, w, dev)
    lo1, hi1 = yc.call_yquantiles(case, a, levels, 1, w, dev)
    assert bool(torch.isfinite(lo).all()) and bool(torch.isfinite(hi).all()) and bool((lo <= hi).all())
    _width_ok("planted " + name, lo, hi, lo1, hi1, passes)
    z = to(np.repeat(a["theta"][:, a["w_col"]][:, None], case["B"], axis=1))          # X = 1: z_pb = w_p, exactly
    s = to(np.full(case["n"], np.sqrt(case["tau"])))
    zero = torch.zeros_like(z)
    _contract("planted " + name, "closed form", case, lo, hi, levels, z, zero, s, wt, per, slices)
    bound = yr.width_bound(lo1.cpu().numpy(), hi1.cpu().numpy(), passes)
    for i, q in enumerate(levels):
        if np.isnan(expect[i]):
            continue
        # the closed form lies in [Q64(q - a_F), Q64(q + a_F)], and the result with it up to the bracket's width
        a_f = yr.cdf(hi[i:i + 1].double(), z, zero, s, wt, case["model"], per, slices)[1][0]
        q_minus = yr.quantile64(q - a_f, z, s, wt)[0].cpu().numpy()
        q_plus = yr.quantile64(q + a_f, z, s, wt)[1].cpu().numpy()
        got = hi[i].double().cpu().numpy()
        assert (q_minus <= expect[i]).all() and (expect[i] <= q_plus).all(), (name, q)
        print("planted %-10s level %-6g result - closed form = %+.3g (uncertainty %.3g)" %
              (name, q, float((got - expect[i]).max()), float((q_plus - q_minus).max() + bound[i].max())))
        assert (got >= q_minus).all() and (got <= q_plus + bound[i]).all(), (name, q, got, expect[i])
    if name == "collapse":                                   # neighbouring floats well before the last pass, and no end moves
        early = yc.call_yquantiles(case, a, levels, 9, w, dev)
        assert bool(((early[1] - early[0]).abs() <= torch.tensor(np.spacing(np.abs(early[1].cpu().numpy())), device=dev)).all())
        assert bool((early[0] <= lo).all()) and bool((hi <= early[1]).all())


@pytest.mark.parametrize("kind", pwc.BAD)
def test_bad_weights_give_nan_rows_and_ok(cuda, kind):
    case = yc.EVERY[4]
    a = pc.args(case)
    lo, hi = yc.call_yquantiles(case, a, (0.05, 0.95), PASSES, pwc.bad_weights(case["n"], kind), cuda)   # raises unless STEIN_OK
    assert bool(torch.isnan(lo).all()) and bool(torch.isnan(hi).all()), kind
