"""GPU: how the folded contraction (k_phi_x3fs<2, true>, csrc/stein_x3.hip) is fed -- its producers request a D tile two k
tiles ahead (PD = 2; the unfolded kernel four), in visit order, across stage boundaries, mirrored and permuted stages.

Only when a load is issued and waited for differs from the four-tile lead, so every result is what it was; what can go
wrong is a wait that counts the wrong number of younger loads, or a request that takes the source kind (natural /
mirrored) or the stage (permuted order) of the wrong pipeline stage.  The shapes are the smallest that put each of these
in front of the two-tile lead:

  ranges of 1, 2, 3 k tiles        fewer tiles than the lead, as many, one more (the prologue's requests, the drain waits)
  5, 6, 7 k tiles                  a partial last stage of 1, 2, 3 tiles: slots 2, 3 of the full stage request into it
  640 x 130, one range             mirrored stages, then natural ones, in every row tile but the first: the requests of
                                   slots 2, 3 take the NEXT stage's source, those of slots 0, 1 this stage's
  1024 x 300, two ranges           a range that starts behind the diagonal for some row tiles, with the theta half
  8192 x 132, one range            the permuted stage order at the smallest n that takes it (group = 32 row tiles, 64
                                   stages): the stage behind stage v is not v + 1
  8224 x 132, one range            just outside it (65 stages: no power of two), last stage of one tile, the theta half

Driver, checks and bounds are test_gpu_contract_matrix.py's _run_fold (imported, not restated): forced fold, the path
asserted first, poisoned workspace and outputs, phi (and dK) over ALL rows and columns against the fp64 formulae of
contract_cases.reference -- 128 x 128 tiles within 2 TOL, elementwise and per column within TOL = 1e-5 --, row sums, a second
call bit-identical, phi with and without dK bit-identical.  The same shapes run unfolded (lead 4) as the case outside
the changed branch.  Run with -s to see every figure."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contract_cases as cc  # noqa: E402
import test_gpu_contract_matrix as tm  # noqa: E402

pytestmark = pytest.mark.gpu


def _fold(n, d, k, dk):
    return cc.Case("fold", n, d, n, 0, k, dk)


# (case, what the plan must say about it: ntile of every W range, permuted?, theta half?)
FEED = [
    (_fold(32, 130, 1, False), [1], False),
    (_fold(40, 130, 1, True), [2], False),
    (_fold(96, 130, 1, False), [3], False),
    (_fold(160, 130, 1, True), [5], False),
    (_fold(192, 257, 1, False), [6], False),
    (_fold(223, 130, 1, True), [7], False),
    (_fold(640, 130, 1, True), [20], False),
    (_fold(1024, 300, 2, True), [16, 16], False),
    (_fold(8192, 132, 1, False), [256], True),
    (_fold(8224, 132, 1, True), [257], False),
]
IDS = [cc.case_id(c) for c, _, _ in FEED]


@pytest.mark.parametrize("case,ntiles,permuted", FEED, ids=IDS)
def test_folded_feed(cuda, case, ntiles, permuted):
    m = cc.classify_case(case)
    tag = "feed " + cc.case_id(case)
    assert m["fold"] and [r["ntile"] for r in m["ranges"]] == ntiles, (tag, [r["ntile"] for r in m["ranges"]])
    assert [r["permute"] for r in m["ranges"]] == [permuted] * len(ntiles), tag
    assert (m["theta_range"] is not None) == case.dk, tag
    if case.n == 640:       # both kinds of stage in one range, for every row tile but the first
        assert all(0 < t < m["ranges"][0]["nstage"] for t in m["ranges"][0]["ntr"][1:]), tag
    if case.n == 8224:      # a last stage of one tile
        assert m["ranges"][0]["tile_tail"] == 1 and m["theta_range"]["tile_tail"] == 1, tag
    if permuted:            # the order is not the natural one for the row tiles behind the first group
        assert any(m["ranges"][0]["xmask"]), tag
    tm._run_fold(case, m, cuda, tag)


@pytest.mark.parametrize("n,d,dk", [(223, 130, True), (640, 130, True), (8224, 132, False)])
def test_unfolded_beside_it(cuda, n, d, dk):
    """the same shapes on the unfolded kernel, whose lead stays at four tiles"""
    case = cc.Case("unfolded", n, d, n, 0, 0, dk)
    m = cc.classify_case(case)
    assert not m["fold"]
    tm._run_upper(case, m, cuda, "feed " + cc.case_id(case))
