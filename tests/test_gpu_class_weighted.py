"""GPU: the weighted class summaries through the C ABI (stein_predict_softmax_weighted, stein_predict_bnn_class_weighted) on
every (case, pattern) of tests/class_weighted_cases.py, on a NaN-filled workspace with NaN-prefilled outputs, against the
fp64 reference of tests/class_weighted_ref.py evaluated in torch fp64 on the device.

Each (case, pattern) asserts: prob, ent, lpd and ess inside the a-priori allowance; inside the tighter allowance against
weighted fp64 statistics of the call's own pred; label exactly the lowest-index argmax of the returned prob; pred bit-identical
to the unweighted call's; a repeat, another workspace content, summaries with and without pred (the dead-unit skip) and weights
times 2^10 and 2^-20 bit-identical; a one-hot weight returns that particle's pred bit for bit with ess == 1.  Further down:
constant weights at n = 16 and 32 against the unweighted call, a NaN-filled particle of weight zero, the bad weights and a bad
label under weights."""
import os
import sys

import numpy as np
import pytest
import torch

from stein_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import class_weighted_cases as cwc  # noqa: E402
import class_weighted_ref as cwr  # noqa: E402
import netclass_cases as ncc  # noqa: E402
import softmax_cases as smc  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("prob", "lpd", "ent", "label")
NAN = float("nan")
RATIOS = {}


def _same(a, b):
    a, b = a.contiguous(), b.contiguous()
    if a.dtype == torch.float64:
        return torch.equal(a.view(torch.int64), b.view(torch.int64))
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _device(a, cuda):
    th, X = (torch.tensor(a[k], dtype=torch.float32, device=cuda) for k in ("theta", "X"))
    return th, X, torch.tensor(a["labels"], device=cuda)


def _raw(model, a, th, X, y, w, cuda, output="mean", want_pred=False, fill=NAN):
    """one call of the C ABI -> (pred or None, {prob, lpd, ent, label, ess}); w None: the unweighted call.  fill: what the
    workspace holds on entry; every output is prefilled with NaN (label: -7)"""
    import ctypes
    n, B, C = th.shape[0], X.shape[0], a["C"]
    pred = torch.full((n, B, C), NAN, device=cuda) if want_pred else None
    out = {"prob": torch.full((B, C), NAN, device=cuda), "lpd": torch.full((B,), NAN, device=cuda),
           "ent": torch.full((B,), NAN, device=cuda), "label": torch.full((B,), -7, dtype=torch.int32, device=cuda)}
    stem = "softmax" if model == "softmax" else "bnn_class"
    size = getattr(_lib, "predict_%s_%sworkspace_bytes" % (stem, "" if w is None else "weighted_"))(n, B, C)
    ws = torch.empty(size, dtype=torch.uint8, device=cuda)
    ws.view(torch.float32).fill_(fill)
    head = (th.data_ptr(), n, a["d"], _lib.PRED_LINK if output == "link" else _lib.PRED_MEAN)
    model_args = (a["w_col"], a["F"], C) if model == "softmax" else (a["F"], a["H"], C, (ctypes.c_int64 * 5)(*a["cols"]))
    wargs, eargs = (), ()
    if w is not None:
        out["ess"] = torch.full((1,), NAN, dtype=torch.float64, device=cuda)
        wargs, eargs = (w.data_ptr(),), (out["ess"].data_ptr(),)
    _lib.call("stein_predict_%s%s" % (stem, "" if w is None else "_weighted"), *head, *model_args, X.data_ptr(), y.data_ptr(), B,
              *wargs, None if pred is None else pred.data_ptr(), out["prob"].data_ptr(), out["lpd"].data_ptr(),
              out["ent"].data_ptr(), out["label"].data_ptr(), *eargs, ws.data_ptr(), ws.numel(),
              torch.cuda.current_stream(cuda).cuda_stream)
    torch.cuda.synchronize()
    return pred, out


def _inside(name, what, got, val, allow):
    err = (got.double() - val).abs()
    ratio = float((err / allow).max())
    print("%-40s %-16s max |err| / allowance = %.3f" % (name, what, ratio))
    RATIOS[what] = max(RATIOS.get(what, 0.0), ratio)
    assert bool(torch.isfinite(val).all()) and bool((allow > 0).all()), what
    assert bool((err <= allow).all()), "%s outside the allowance: ratio %.3g" % (what, ratio)


def _to(cuda):
    def to(v):
        v = np.asarray(v)
        return torch.tensor(v, device=cuda, dtype=torch.float64 if v.dtype.kind == "f" else None)
    return to


@pytest.mark.parametrize("triple", cwc.ALL, ids=cwc.triple_id)
def test_every_case_under_every_pattern(cuda, triple):
    model, case, pat = triple
    name = cwc.triple_id(triple)
    a = cwc.args(model, case)
    w_np = cwc.weights(case, pat)
    th, X, y = _device(a, cuda)
    w = torch.tensor(w_np, dtype=torch.float64, device=cuda)
    per = cwc.plan(model, case)["per"]
    _, base = _raw(model, a, th, X, y, w, cuda)            # no pred: dead units are skipped
    # inside the allowance against fp64
    ref = cwc.reference(model, case, a, w_np, to=_to(cuda))
    for k in ("prob", "ent", "lpd"):
        _inside(name, k, base[k], *ref[k])
    _inside(name, "ess", base["ess"], *[torch.as_tensor(v, device=cuda).reshape(1) for v in ref["ess"]])
    # pred: bit for bit the unweighted call's, and the summaries with it are the summaries without it
    mean_u, _ = _raw(model, a, th, X, y, None, cuda, "mean", True)
    link_u, _ = _raw(model, a, th, X, y, None, cuda, "link", True)
    for output, want in (("mean", mean_u), ("link", link_u)):
        pred, out = _raw(model, a, th, X, y, w, cuda, output, True, fill=3.0e38)
        assert _same(pred, want), output
        for k in KEYS + ("ess",):
            assert _same(out[k], base[k]), (k, output)
    # the tighter allowances: weighted fp64 statistics of the call's own pred
    own = cwc.reference(model, case, a, w_np, to=_to(cuda), z=link_u.double(), tight=True)
    own.update(cwr.summaries_of_probs(mean_u.double(), y, w, per))
    for k in ("prob", "lpd", "ent"):
        assert bool((own[k][1] <= ref[k][1]).all()), k
        _inside(name, k + " (own pred)", base[k], *own[k])
    # the label: the lowest-index argmax of the floats prob received
    top = base["prob"].max(-1, keepdim=True).values
    cls = torch.arange(a["C"], device=cuda).expand_as(base["prob"])
    assert torch.equal(base["label"].long(), torch.where(base["prob"] == top, cls, torch.full_like(cls, a["C"])).min(-1).values)
    # a repeat on another workspace content, and the weights rescaled by powers of two
    for ww, fill in ((w, 0.0), (w * 2.0 ** 10, NAN), (w * 2.0 ** -20, -1.0)):
        _, out = _raw(model, a, th, X, y, ww, cuda, fill=fill)
        for k in KEYS + ("ess",):
            assert _same(out[k], base[k]), (k, fill)
    if pat.startswith("one_hot"):
        p = int(np.argmax(w_np))
        assert _same(base["prob"], mean_u[p]) and float(base["ess"]) == 1.0


def test_the_largest_error_per_output(cuda):
    """the record of the run above (printed with -s); empty when this test runs alone"""
    for what, ratio in sorted(RATIOS.items()):
        print("largest |err| / allowance  %-16s %.3f" % (what, ratio))
        assert ratio <= 1.0


def _uniform_cases(model):
    mod = smc if model == "softmax" else ncc
    sixteen = [c for c in mod.PRED_COUNTS if c["n"] == 16]
    if model == "softmax":
        return sixteen + [smc._pred("n32_C%d" % C, 5, C, 7, 32) for C in (3, 32)]
    return sixteen + [ncc._pred("n32_C%d" % C, 5, 20, C, 7, 32) for C in (3, 32)]


@pytest.mark.parametrize("model", cwc.MODELS)
def test_constant_weights_at_a_power_of_two_n_are_the_unweighted_call(cuda, model):
    """the lane weight is 2^-k exactly, so every slice sum is 2^-k times the unweighted one and the fp64 merge divides nothing"""
    for case in _uniform_cases(model):
        a = cwc.args(model, case)
        th, X, y = _device(a, cuda)
        _, plain = _raw(model, a, th, X, y, None, cuda)
        for c in (1.0, 3.7):
            w = torch.full((case["n"],), c, dtype=torch.float64, device=cuda)
            _, out = _raw(model, a, th, X, y, w, cuda)
            for k in KEYS:
                assert _same(out[k], plain[k]), (case["name"], c, k)
            assert float(out["ess"]) == float(case["n"])


@pytest.mark.parametrize("model", cwc.MODELS)
def test_a_nan_particle_of_weight_zero_enters_nothing(cuda, model):
    mod = smc if model == "softmax" else ncc
    for case, pat in ((mod.PRED_COUNTS[4], "counts"), (mod.PRED_COUNTS[4], "zero_slices"), (mod.PRED_COUNTS[3], "one_hot_ragged")):
        a = cwc.args(model, case)
        w_np = cwc.weights(case, pat)
        th, X, y = _device(a, cuda)
        w = torch.tensor(w_np, dtype=torch.float64, device=cuda)
        _, clean = _raw(model, a, th, X, y, w, cuda)
        th2 = th.clone()
        th2[torch.tensor(w_np == 0, device=cuda)] = NAN
        assert bool((w_np == 0).any())
        for want_pred in (False, True):
            pred, out = _raw(model, a, th2, X, y, w, cuda, "mean", want_pred)
            for k in KEYS + ("ess",):
                assert bool(torch.isfinite(out[k].double()).all()), (k, want_pred)
                assert _same(out[k], clean[k]), (k, want_pred)
            if pred is not None:
                assert bool(torch.isfinite(pred[torch.tensor(w_np > 0, device=cuda)]).all())


@pytest.mark.parametrize("model", cwc.MODELS)
@pytest.mark.parametrize("kind", cwc.BAD)
def test_bad_weights_give_nan_rows_nan_ess_and_the_label_minus_one(cuda, model, kind):
    mod = smc if model == "softmax" else ncc
    case = mod.PRED_COUNTS[4]
    a = cwc.args(model, case)
    th, X, y = _device(a, cuda)
    w = torch.tensor(cwc.bad_weights(case["n"], kind), dtype=torch.float64, device=cuda)
    mean_u, _ = _raw(model, a, th, X, y, None, cuda, "mean", True)
    for want_pred in (False, True):
        pred, out = _raw(model, a, th, X, y, w, cuda, "mean", want_pred)      # returns: STEIN_OK
        for k in ("prob", "lpd", "ent", "ess"):
            assert bool(torch.isnan(out[k]).all()), (k, kind)
        assert bool((out["label"] == -1).all())
        if pred is not None:
            assert _same(pred, mean_u)


@pytest.mark.parametrize("model", cwc.MODELS)
@pytest.mark.parametrize("bad", [-1, "C"], ids=["minus_one", "C"])
def test_a_bad_label_under_weights_is_nan_in_that_rows_lpd_alone(cuda, model, bad):
    mod = smc if model == "softmax" else ncc
    case = mod.PRED_CLASSES[2]
    a = cwc.args(model, case)
    th, X, y = _device(a, cuda)
    w = torch.tensor(cwc.weights(case, "positive"), dtype=torch.float64, device=cuda)
    _, good = _raw(model, a, th, X, y, w, cuda)
    y2 = y.clone()
    y2[5] = case["C"] if bad == "C" else -1
    _, out = _raw(model, a, th, X, y2, w, cuda)            # returns: STEIN_OK
    assert bool(torch.isnan(out["lpd"][5]))
    keep = torch.ones(case["B"], dtype=torch.bool, device=cuda)
    keep[5] = False
    assert _same(out["lpd"][keep], good["lpd"][keep])
    for k in ("prob", "ent", "label", "ess"):
        assert _same(out[k], good[k]), k
