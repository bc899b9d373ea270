"""GPU: the score of the network classifier (csrc/stein_score_bnn_class.hip, stein_score_bnn_class through BnnClassScore)
against the fp64 reference of tests/netclass_ref.py evaluated in torch fp64 on the device, element by element inside that
reference's a-priori fp32 allowance (a derivation; no tolerance relative to the largest entry).

The cases (tests/netclass_cases.py; tests/test_netclass_cases.py proves on the CPU what they reach):
  classes   C in {2, 4, 5, 8, 9, 16, 17, 32}
  plans     every (lanes, units per lane) instantiation, reached by the hidden units and by the LDS; 54 x 100 x 7
  hidden    H in {1, 15, 16, 17, 65}, 300 on 256 lanes;  inputs  n_in in {1, 5, 128}
  chunk     116 x 74 x 2 (24 rows per LDS chunk): batches of 1, 23, 24, 25 and 49 rows; 128 x 102 x 32, the fullest LDS
  counts    n around 4, 2 and 1 particles per workgroup, and one grid plus one particle
  columns   the blocks permuted, foreign columns before, between and after, log_lambda before / after / absent

Every case prefills the output with NaN and asserts: the share of entries under an ambiguous ReLU mask is at most 2 % (so
an allowance can never swallow a case), all entries finite, foreign columns exactly 0, |got - ref| <= allowance elementwise,
a second call bit-identical, and single particles alone bit-identical to their rows of the full call.  Each prints
max |err| / allowance per block (run with -s).  One planted case ties the w2 block to SoftmaxScore's W block."""
import os
import sys

import numpy as np
import pytest
import torch

from stein_amd.scores import BnnClassScore, SoftmaxScore

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import netclass_cases as ncc  # noqa: E402
import netclass_ref as ncr  # noqa: E402
import softmax_ref as smr  # noqa: E402

pytestmark = pytest.mark.gpu
SHARE_CAP = 0.02


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _producer(a):
    cols = [None if c < 0 else c for c in a["cols"]]
    return BnnClassScore(a["F"], a["H"], a["C"], cols, n_train=a["scale"] * a["X"].shape[0], prior_precision=a["prior_precision"],
                         gamma_rate=a["gamma_rate"])


def _device(a, cuda):
    th, X = (torch.tensor(a[k], dtype=torch.float32, device=cuda) for k in ("theta", "X"))
    return th, X, torch.tensor(a["labels"], device=cuda)


def _check(case, cuda):
    a = ncc.score_args(case)
    th, X, y = _device(a, cuda)
    ref, allow, share = ncr.score(th.double(), a["F"], a["H"], a["C"], a["cols"], X.double(), y, a["scale"], a["prior_precision"],
                                  a["gamma_rate"])
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(allow).all())
    assert share <= SHARE_CAP, "ambiguous ReLU masks touch %.3f of the entries" % share
    prod = _producer(a)
    feed = {"X": X, "y": y}
    got = prod(th, feed, out=torch.full_like(th, float("nan")))
    again = prod(th, feed, out=torch.full_like(th, float("nan")))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got).all()), "non-finite entries (or entries never written)"
    live = torch.tensor(ncc.live_columns(case), device=cuda)
    assert bool((got[:, ~live] == 0).all()), "a foreign column is not exactly 0"
    assert bool((allow[:, live] > 0).all())
    err = (got.double() - ref).abs()
    ratios = {k: float((err[:, sl] / allow[:, sl]).max()) for k, sl in ncc.block_slices(case).items()}
    print("%-18s %s share %.4f max |err| / allowance: %s" % (case["name"], ncc.score_plan(case["F"], case["H"], case["C"], case["B"]),
                                                              share, " ".join("%s %.3f" % kv for kv in ratios.items())))
    bad = (err > allow).nonzero()
    assert bad.numel() == 0, "outside the allowance at (particle, column) %s ...: ratios %s" % (bad[:4].tolist(), ratios)
    assert _same(got, again), "a second call differs"
    n = case["n"]
    for p in sorted({0, 1 % n, n // 2, n - 1}):       # a particle's row depends on nothing but the particle
        alone = prod(th[p:p + 1].contiguous(), feed, out=torch.full((1, th.shape[1]), float("nan"), device=cuda))
        assert _same(alone[0], got[p]), "particle %d alone differs from its row of the full call" % p


def _id(case):
    return case["name"]


@pytest.mark.parametrize("case", ncc.SCORE_CLASSES, ids=_id)
def test_the_class_counts_at_both_ends_of_every_padding(cuda, case):
    _check(case, cuda)


@pytest.mark.parametrize("case", ncc.SCORE_PLANS + ncc.SCORE_HIDDEN + ncc.SCORE_INPUTS, ids=_id)
def test_every_instantiation_and_the_hidden_and_input_widths(cuda, case):
    _check(case, cuda)


@pytest.mark.parametrize("case", ncc.SCORE_CHUNK, ids=_id)
def test_batches_around_the_lds_chunk_edges(cuda, case):
    _check(case, cuda)


@pytest.mark.parametrize("case", ncc.SCORE_COUNTS + ncc.SCORE_GRID, ids=_id)
def test_particle_counts_around_a_workgroup_and_one_grid_plus_one(cuda, case):
    _check(case, cuda)


@pytest.mark.parametrize("case", ncc.SCORE_COLS, ids=_id)
def test_the_blocks_places_and_foreign_columns(cuda, case):
    _check(case, cuda)


def test_a_particle_subset_is_bit_identical_to_its_rows(cuda):
    a = ncc.score_args(ncc.SCORE_SUBSET_CASE)
    th, X, y = _device(a, cuda)
    prod, feed = _producer(a), {"X": X, "y": y}
    full = prod(th, feed)
    for lo, hi in ((0, 1), (3, 10), (5, 9), (20, 23)):
        part = prod(th[lo:hi].contiguous(), feed)
        assert _same(part, full[lo:hi]), (lo, hi)
    assert bool(torch.isfinite(full).all())


@pytest.mark.parametrize("bad", [-1, "C"], ids=["minus_one", "C"])
def test_one_label_outside_the_classes_makes_every_entry_of_the_four_blocks_nan(cuda, bad):
    case = ncc.BAD_LABEL_CASE
    a = ncc.score_args(case)
    th, X, y = _device(a, cuda)
    y = y.clone()
    y[4] = case["C"] if bad == "C" else -1
    got = _producer(a)(th, {"X": X, "y": y}, out=torch.full_like(th, 7.0))     # returns: STEIN_OK
    torch.cuda.synchronize()
    live = torch.tensor(ncc.live_columns(case), device=cuda)
    four = live.clone()
    four[a["cols"][4]] = False
    assert bool(torch.isnan(got[:, four]).all()), "an entry of the four blocks is not NaN"
    ref, allow, _ = ncr.score(th.double(), a["F"], a["H"], a["C"], a["cols"], X.double(), y, a["scale"], a["prior_precision"],
                              a["gamma_rate"])
    assert bool(torch.isnan(ref[:, four]).all())
    ll = a["cols"][4]
    assert bool(((got.double() - ref).abs()[:, ll] <= allow[:, ll]).all())      # the log_lambda entry does not read the labels
    assert bool((got[:, ~live] == 0).all())


def test_planted_identity_first_layer_gives_the_softmax_models_w_block(cuda):
    """n_in = H, w1 the identity, b1 = b2 = 0, X >= 0: the hidden layer reproduces X exactly, so the w2 block of the score is
    SoftmaxScore's W block at the same precision, inside the sum of both allowances"""
    rng = np.random.default_rng(20)
    n, H, C, B = 6, 12, 5, 40
    case = ncc._score("planted", H, H, C, B, n, order="none", lead=1, tail=1)
    cols, d = ncc.layout(case)
    theta = np.zeros((n, d))
    theta[:, cols[0]:cols[0] + H * H] = np.eye(H).reshape(-1)
    W = ncc._r32(rng.normal(size=(n, H * C)) * (1.5 / np.sqrt(H)))
    theta[:, cols[2]:cols[2] + H * C] = W
    X = ncc._r32(np.abs(rng.normal(size=(B, H))))
    labels = rng.integers(0, C, size=B).astype(np.int32)
    th, Xd, y = torch.tensor(theta, dtype=torch.float32, device=cuda), torch.tensor(X, dtype=torch.float32, device=cuda), torch.tensor(labels, device=cuda)
    scale, prec = 3.0, 0.75
    net = BnnClassScore(H, H, C, cols[:4] + [None], n_train=scale * B, prior_precision=prec)(th, {"X": Xd, "y": y})
    Wd = torch.tensor(W, dtype=torch.float32, device=cuda)
    soft = SoftmaxScore(H, C, n_train=scale * B, prior_precision=prec)(Wd, {"X": Xd, "y": y})
    torch.cuda.synchronize()
    _, a_net, share = ncr.score(th.double(), H, H, C, cols, Xd.double(), y, scale, prec, 0.01)
    _, a_soft = smr.score(Wd.double(), 0, H, C, -1, Xd.double(), y, scale, prec, 0.01)
    both = a_net[:, cols[2]:cols[2] + H * C] + a_soft
    err = (net[:, cols[2]:cols[2] + H * C].double() - soft.double()).abs()
    print("planted: max |w2 block - W block| / (sum of allowances) = %.3f" % float((err / both).max()))
    assert bool((err <= both).all())
