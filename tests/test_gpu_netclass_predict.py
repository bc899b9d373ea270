"""GPU: the predictive call of the network classifier (csrc/stein_predict_bnn_class.hip, stein_predict_bnn_class through
BnnClassPredict) against the fp64 reference of tests/netclass_ref.py evaluated in torch fp64 on the device: pred (both
outputs), prob, lpd and ent element by element inside the reference's a-priori fp32 allowances, and prob, lpd and ent
inside the second, tighter allowances against fp64 statistics of the call's own pred.

The cases (tests/netclass_cases.py; tests/test_netclass_cases.py proves on the CPU what they reach):
  classes   C in {2, 4, 5, 8, 9, 16, 17, 32}, the blocks in three orders with foreign columns
  hidden    H in {1, 15, 16, 17, 33}: one, two and three tiles of 16 hidden units
  staged    2 (128 inputs x 32 classes: the fewest the domain has), 3, 8 and 16 (particle, tile) pairs per unit; 54 x 100 x 7
  rows      batches of 1, 255, 256, 257 and 513 rows
  counts    n in {1, 15, 16, 17, 40}: 40 particles are three slices with a ragged last one; 3 and 32 classes

Each case also asserts: label is the lowest-index argmax of the returned prob, exactly; every prob row sums to 1 within its
summed allowance; a repeat, a NaN-filled workspace and summaries asked for with and without pred are bit-identical.  One
planted case ties every output to SoftmaxPredict's."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from stein_amd import _lib
from stein_amd.predict import BnnClassPredict, SoftmaxPredict

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import netclass_cases as ncc  # noqa: E402
import netclass_ref as ncr  # noqa: E402
import softmax_ref as smr  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("prob", "lpd", "ent", "label")


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _device(a, cuda):
    th, X = (torch.tensor(a[k], dtype=torch.float32, device=cuda) for k in ("theta", "X"))
    return th, X, torch.tensor(a["labels"], device=cuda)


def _raw(a, th, X, y, cuda, output, want_pred, fill=None):
    """one call of the C ABI -> (pred or None, {prob, lpd, ent, label}); fill: what the workspace holds on entry"""
    n, B, C = th.shape[0], X.shape[0], a["C"]
    pred = torch.full((n, B, C), float("nan"), device=cuda) if want_pred else None
    out = {"prob": torch.full((B, C), float("nan"), device=cuda), "lpd": torch.full((B,), float("nan"), device=cuda),
           "ent": torch.full((B,), float("nan"), device=cuda), "label": torch.full((B,), -7, dtype=torch.int32, device=cuda)}
    ws = torch.empty(_lib.predict_bnn_class_workspace_bytes(n, B, C), dtype=torch.uint8, device=cuda)
    if fill is not None:
        ws.view(torch.float32).fill_(fill)
    cols = (ctypes.c_int64 * 5)(*a["cols"])
    _lib.call("stein_predict_bnn_class", th.data_ptr(), n, a["d"], _lib.PRED_LINK if output == "link" else _lib.PRED_MEAN, a["F"],
              a["H"], C, cols, X.data_ptr(), y.data_ptr(), B, None if pred is None else pred.data_ptr(), out["prob"].data_ptr(),
              out["lpd"].data_ptr(), out["ent"].data_ptr(), out["label"].data_ptr(), ws.data_ptr(), ws.numel(),
              torch.cuda.current_stream(cuda).cuda_stream)
    torch.cuda.synchronize()
    return pred, out


def _inside(name, what, got, val, allow):
    err = (got.double() - val).abs()
    ratio = float((err / allow).max())
    print("%-12s %-14s max |err| / allowance = %.3f" % (name, what, ratio))
    assert bool(torch.isfinite(val).all()) and bool((allow > 0).all()), what
    assert bool((err <= allow).all()), "%s outside the allowance: ratio %.3g" % (what, ratio)
    return ratio


def _check(case, cuda):
    a = ncc.predict_args(case)
    th, X, y = _device(a, cuda)
    per = ncc.predict_plan(case["F"], case["H"], case["C"], case["n"], case["B"])["per"]
    ref = ncr.predict(th.double(), a["F"], a["H"], a["C"], a["cols"], X.double(), y, per)
    prod = {o: BnnClassPredict(a["F"], a["H"], a["C"], a["cols"], output=o) for o in ("link", "mean")}
    n, B, C = case["n"], case["B"], case["C"]
    link = prod["link"](th, {"X": X}, out=torch.full((n, B, C), float("nan"), device=cuda))
    mean = prod["mean"](th, {"X": X}, out=torch.full((n, B, C), float("nan"), device=cuda))
    _inside(case["name"], "pred (link)", link, *ref["pred_link"])
    _inside(case["name"], "pred (mean)", mean, *ref["pred_mean"])
    s = prod["mean"].summary(th, {"X": X, "y": y})
    torch.cuda.synchronize()
    assert set(s) == set(KEYS) and s["label"].dtype == torch.int32
    for k in ("prob", "lpd", "ent"):
        _inside(case["name"], k, s[k], *ref[k])
    # the tighter allowances: statistics of the call's own outputs
    own = ncr.summaries(link.double(), None, y, per, tight=True)
    own.update(ncr.summaries_of_probs(mean.double(), y, per))
    for k in ("prob", "lpd", "ent"):
        assert bool((own[k][1] <= ref[k][1]).all()), k
        _inside(case["name"], k + " (own pred)", s[k], *own[k])
    # the label: the lowest-index argmax of the floats prob received
    top = s["prob"].max(-1, keepdim=True).values
    cls = torch.arange(C, device=cuda).expand_as(s["prob"])
    first = torch.where(s["prob"] == top, cls, torch.full_like(cls, C)).min(-1).values
    assert torch.equal(s["label"].long(), first)
    # a prob row sums to 1 within the sum of its allowances
    assert bool(((s["prob"].double().sum(-1) - 1.0).abs() <= ref["prob"][1].sum(-1)).all())
    # bit-identical: a repeat, a workspace full of NaN, and with pred in the same call (either output)
    base_pred, base = _raw(a, th, X, y, cuda, "mean", True, fill=0.0)
    for k in KEYS:
        assert _same(base[k], s[k]), k
    assert _same(base_pred, mean)
    for output, want_pred, fill in (("mean", True, float("nan")), ("mean", False, float("nan")), ("link", True, 3.0e38), ("link", False, None)):
        pred, out = _raw(a, th, X, y, cuda, output, want_pred, fill)
        for k in KEYS:
            assert _same(out[k], base[k]), (k, output, want_pred, fill)
        if pred is not None:
            assert _same(pred, mean if output == "mean" else link)


def _id(case):
    return case["name"]


@pytest.mark.parametrize("case", ncc.PRED_CLASSES, ids=_id)
def test_every_padded_class_instantiation_at_both_ends(cuda, case):
    _check(case, cuda)


@pytest.mark.parametrize("case", ncc.PRED_HIDDEN + ncc.PRED_STAGED, ids=_id)
def test_the_hidden_tiles_and_every_size_of_the_staging_unit(cuda, case):
    _check(case, cuda)


@pytest.mark.parametrize("case", ncc.PRED_ROWS, ids=_id)
def test_batches_around_a_row_tile(cuda, case):
    _check(case, cuda)


@pytest.mark.parametrize("case", ncc.PRED_COUNTS, ids=_id)
def test_particle_counts_around_a_pass_and_three_ragged_slices(cuda, case):
    _check(case, cuda)


def test_row_and_particle_subsets_of_pred_are_bit_identical(cuda):
    case = ncc.PRED_SUBSET_CASE
    a = ncc.predict_args(case)
    th, X, y = _device(a, cuda)
    for output in ("mean", "link"):
        prod = BnnClassPredict(a["F"], a["H"], a["C"], a["cols"], output=output)
        full = prod(th, {"X": X})
        assert bool(torch.isfinite(full).all())
        for lo, hi in ((0, 1), (5, 21), (16, 37), (36, 37)):
            assert _same(prod(th[lo:hi].contiguous(), {"X": X}), full[lo:hi]), ("particles", lo, hi)
        for lo, hi in ((0, 1), (3, 259), (255, 257), (299, 300)):
            assert _same(prod(th, {"X": X[lo:hi].contiguous()}), full[:, lo:hi]), ("rows", lo, hi)


@pytest.mark.parametrize("bad", [-1, "C"], ids=["minus_one", "C"])
def test_a_label_outside_the_classes_is_nan_in_that_rows_lpd_alone(cuda, bad):
    case = ncc.PRED_CLASSES[2]
    a = ncc.predict_args(case)
    th, X, y = _device(a, cuda)
    _, good = _raw(a, th, X, y, cuda, "mean", False)
    y2 = y.clone()
    y2[5] = case["C"] if bad == "C" else -1
    _, out = _raw(a, th, X, y2, cuda, "mean", False)       # returns: STEIN_OK
    assert bool(torch.isnan(out["lpd"][5]))
    keep = torch.ones(case["B"], dtype=torch.bool, device=cuda)
    keep[5] = False
    assert _same(out["lpd"][keep], good["lpd"][keep])
    for k in ("prob", "ent", "label"):
        assert _same(out[k], good[k]), k


def test_planted_identity_first_layer_gives_the_softmax_models_outputs(cuda):
    """n_in = H, w1 the identity, b1 = b2 = 0, X >= 0: the hidden layer reproduces X exactly, so pred, prob, ent and lpd agree
    with SoftmaxPredict on W = w2 inside the sum of both allowances"""
    rng = np.random.default_rng(21)
    n, H, C, B = 19, 20, 5, 37
    case = ncc._pred("planted", H, H, C, B, n, order="none", lead=1, tail=1)
    cols, d = ncc.layout(case)
    theta = np.zeros((n, d))
    theta[:, cols[0]:cols[0] + H * H] = np.eye(H).reshape(-1)
    W = ncc._r32(rng.normal(size=(n, H * C)) * (1.5 / np.sqrt(H)))
    theta[:, cols[2]:cols[2] + H * C] = W
    th = torch.tensor(theta, dtype=torch.float32, device=cuda)
    Wd = torch.tensor(W, dtype=torch.float32, device=cuda)
    X = torch.tensor(np.abs(rng.normal(size=(B, H))), dtype=torch.float32, device=cuda)
    y = torch.tensor(rng.integers(0, C, size=B).astype(np.int32), device=cuda)
    per = ncc.predict_plan(H, H, C, n, B)["per"]
    a_net = ncr.predict(th.double(), H, H, C, cols, X.double(), y, per)
    a_soft = smr.predict(Wd.double(), 0, H, C, X.double(), y, per)
    for output, key in (("link", "pred_link"), ("mean", "pred_mean")):
        net = BnnClassPredict(H, H, C, cols, output=output)(th, {"X": X})
        soft = SoftmaxPredict(H, C, output=output)(Wd, {"X": X})
        assert bool(((net.double() - soft.double()).abs() <= a_net[key][1] + a_soft[key][1]).all()), key
    s_net = BnnClassPredict(H, H, C, cols).summary(th, {"X": X, "y": y})
    s_soft = SoftmaxPredict(H, C).summary(Wd, {"X": X, "y": y})
    torch.cuda.synchronize()
    for k in ("prob", "ent", "lpd"):
        err = (s_net[k].double() - s_soft[k].double()).abs()
        both = a_net[k][1] + a_soft[k][1]
        print("planted %-5s max |difference| / (sum of allowances) = %.3f" % (k, float((err / both).max())))
        assert bool((err <= both).all()), k
