"""GPU: the score of softmax regression (csrc/stein_score_softmax.hip, stein_score_softmax through SoftmaxScore) against the
fp64 reference of tests/softmax_ref.py evaluated in torch fp64 on the device, element by element inside that reference's
a-priori fp32 allowance (a derivation; no tolerance relative to the largest entry).

The cases (tests/softmax_cases.py; tests/test_softmax_cases.py proves on the CPU what they reach):
  classes   C in {2, 4, 5, 8, 9, 16, 17, 32}: both ends of the four padded-class instantiations
  features  F in {1, 7, 54} and 512 x 32
  chunk     512 x 32 (14 rows per LDS chunk): batches of 1, 13, 14, 15, 27, 28, 29 and 43 rows
  counts    n around 4, 2 and 1 particles per workgroup, and one grid plus one for each
  columns   w_col > 0, the alpha column before / after the weights / absent, foreign columns
  lanes     1, 2, ... 64 lanes per row in the forward phase

Every case prefills the output with NaN and asserts: all entries finite, foreign columns exactly 0, |got - ref| <= allowance
elementwise, a second call bit-identical, and single particles alone bit-identical to their rows of the full call.  Each
prints max |err| / allowance (run with -s)."""
import os
import sys

import pytest
import torch

from stein_amd.scores import SoftmaxScore

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import softmax_cases as smc  # noqa: E402
import softmax_ref as smr  # noqa: E402

pytestmark = pytest.mark.gpu


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _producer(a):
    return SoftmaxScore(a["F"], a["C"], w_col=a["w_col"], alpha_col=None if a["alpha_col"] < 0 else a["alpha_col"],
                        n_train=a["scale"] * a["X"].shape[0], prior_precision=a["prior_precision"], gamma_rate=a["gamma_rate"])


def _device(a, cuda):
    th, X = (torch.tensor(a[k], dtype=torch.float32, device=cuda) for k in ("theta", "X"))
    return th, X, torch.tensor(a["labels"], device=cuda)


def _check(case, cuda):
    a = smc.score_args(case)
    th, X, y = _device(a, cuda)
    ref, allow = smr.score(th.double(), a["w_col"], a["F"], a["C"], a["alpha_col"], X.double(), y, a["scale"],
                           a["prior_precision"], a["gamma_rate"])
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(allow).all())
    prod = _producer(a)
    feed = {"X": X, "y": y}
    got = prod(th, feed, out=torch.full_like(th, float("nan")))
    again = prod(th, feed, out=torch.full_like(th, float("nan")))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got).all()), "non-finite entries (or entries never written)"
    live = torch.tensor(smc.live_columns(case), device=cuda)
    assert bool((got[:, ~live] == 0).all()), "a foreign column is not exactly 0"
    err = (got.double() - ref).abs()
    ratio = float((err[:, live] / allow[:, live]).max())
    print("%-16s %s max |err| / allowance = %.3f" % (case["name"], smc.score_plan(case["F"], case["C"], case["B"]), ratio))
    bad = (err > allow).nonzero()
    assert bad.numel() == 0, "outside the allowance at (particle, column) %s ...: ratio %.3g" % (bad[:4].tolist(), ratio)
    assert _same(got, again), "a second call differs"
    n = case["n"]
    for p in sorted({0, 1 % n, n // 2, n - 1}):       # a particle's row depends on nothing but the particle
        alone = prod(th[p:p + 1].contiguous(), feed, out=torch.full((1, th.shape[1]), float("nan"), device=cuda))
        assert _same(alone[0], got[p]), "particle %d alone differs from its row of the full call" % p


def _id(case):
    return case["name"]


@pytest.mark.parametrize("case", smc.SCORE_CLASSES + smc.SCORE_FEATS, ids=_id)
def test_every_padded_class_instantiation_at_both_ends_and_the_feature_counts(cuda, case):
    _check(case, cuda)


@pytest.mark.parametrize("case", smc.SCORE_CHUNK, ids=_id)
def test_batches_around_the_lds_chunk_edges(cuda, case):
    _check(case, cuda)


@pytest.mark.parametrize("case", smc.SCORE_COUNTS + smc.SCORE_GRID, ids=_id)
def test_particle_counts_around_a_workgroup_and_one_grid_plus_one(cuda, case):
    _check(case, cuda)


@pytest.mark.parametrize("case", smc.SCORE_COLS, ids=_id)
def test_the_weights_place_and_foreign_columns(cuda, case):
    _check(case, cuda)


@pytest.mark.parametrize("case", smc.SCORE_LANES, ids=_id)
def test_every_number_of_lanes_per_row(cuda, case):
    _check(case, cuda)


def test_a_particle_subset_is_bit_identical_to_its_rows(cuda):
    a = smc.score_args(smc.SCORE_SUBSET_CASE)
    th, X, y = _device(a, cuda)
    prod, feed = _producer(a), {"X": X, "y": y}
    full = prod(th, feed)
    for lo, hi in ((0, 1), (3, 10), (5, 9), (20, 23)):
        part = prod(th[lo:hi].contiguous(), feed)
        assert _same(part, full[lo:hi]), (lo, hi)
    assert bool(torch.isfinite(full).all())


@pytest.mark.parametrize("bad", [-1, "C"], ids=["minus_one", "C"])
def test_one_label_outside_the_classes_makes_every_weight_entry_nan(cuda, bad):
    case = smc.BAD_LABEL_CASE
    a = smc.score_args(case)
    th, X, y = _device(a, cuda)
    y = y.clone()
    y[4] = case["C"] if bad == "C" else -1
    got = _producer(a)(th, {"X": X, "y": y}, out=torch.full_like(th, 7.0))     # returns: STEIN_OK
    torch.cuda.synchronize()
    w = slice(a["w_col"], a["w_col"] + a["F"] * a["C"])
    assert bool(torch.isnan(got[:, w]).all()), "a weight entry is not NaN"
    ref, allow = smr.score(th.double(), a["w_col"], a["F"], a["C"], a["alpha_col"], X.double(), y, a["scale"],
                           a["prior_precision"], a["gamma_rate"])
    assert bool(torch.isnan(ref[:, w]).all())
    rest = torch.tensor(smc.live_columns(case), device=cuda)
    rest[w] = False
    assert bool(((got.double() - ref).abs()[:, rest] <= allow[:, rest]).all())   # the alpha entry does not read the labels
    assert bool((got[:, ~torch.tensor(smc.live_columns(case), device=cuda)] == 0).all())
