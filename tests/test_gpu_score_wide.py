"""GPU: the network's score for more than four input features (csrc/stein_score_wide.hip, stein_score_bnn_wide through
BnnScore) against the vectorised fp64 reference of tests/score_ref.py, evaluated in torch fp64 on the device, element by
element inside that reference's a-priori fp32 allowance (a derivation; no tolerance relative to the largest entry).

The cases (tests/bnn_wide_cases.py; tests/test_bnn_wide_cases.py checks on the CPU that they reach the five instantiations,
both sides of every dispatch edge, the chunk edges and the three grid-stride caps):
  table     5 .. 128 inputs, 1 .. 1024 hidden units, up to n_in * n_hidden = 16384
  flavors   dead hidden units, saturated pre-activations, log precisions over [-20, 20]
  edges     H at 64 | 65, 128 | 129, 256 | 257, 512 | 513; n_in * H at 4608 | 4672 and 9216 | 9344
  chunk     batches around one, two and three LDS chunks, with heavy rows at the chunk edges
  grid      n just above what one grid covers

Every case prefills the output with NaN and asserts: the ambiguous-ReLU share of the reference <= 2 % (a precondition), all
entries finite, spare columns exactly 0, |got - ref| <= allowance elementwise, a second call bit-identical, and the call on
one particle alone bit-identical to its row of the full call.  Each prints max |err| / allowance (run with -s)."""
import ctypes
import os
import sys

import pytest
import torch

from stein_amd import _lib
from stein_amd.scores import BnnScore

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bnn_wide_cases as wc  # noqa: E402
import score_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu
MAX_AMBIGUOUS = 0.02


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check(case, cuda):
    a = wc.score_args(case)
    to = lambda v: torch.tensor(v, dtype=torch.float64, device=cuda)   # noqa: E731
    ref, allow, share = sc.reference(case, a, to=to)
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(allow).all())
    assert share <= MAX_AMBIGUOUS, share                     # precondition, from the reference alone
    th, X, y = (torch.tensor(a[k], dtype=torch.float32, device=cuda) for k in ("theta", "X", "y"))
    assert a["n_in"] > wc.NARROW_MAX
    prod = BnnScore(a["n_in"], a["H"], a["cols"], n_train=a["n_train"], gamma_a=a["ga"], gamma_b=a["gb"])
    feed = {"X": X, "y": y}
    got = prod(th, feed, out=torch.full_like(th, float("nan")))
    again = prod(th, feed, out=torch.full_like(th, float("nan")))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got).all()), "non-finite entries (or entries never written)"
    live = torch.tensor(sc.live_columns(case, a), device=cuda)
    assert bool((got[:, ~live] == 0).all()), "a spare column is not exactly 0"
    err = (got.double() - ref).abs()
    ratio = float((err[:, live] / allow[:, live]).max())
    print("%-24s %s max |err| / allowance = %.3f   ambiguous share %.5f" % (case["name"], wc.score_kernel(a["n_in"], a["H"]), ratio, share))
    bad = (err > allow).nonzero()
    assert bad.numel() == 0, "outside the allowance at (particle, column) %s ...: ratio %.3g" % (bad[:4].tolist(), ratio)
    assert _same(got, again), "a second call differs"
    # a particle's row depends on nothing but the particle: not on n, the grid, or its place in a workgroup
    n = case["n"]
    for p in sorted({0, 1 % n, n // 2, n - 1}):
        alone = prod(th[p:p + 1].contiguous(), feed, out=torch.full((1, th.shape[1]), float("nan"), device=cuda))
        assert _same(alone[0], got[p]), "particle %d alone differs from its row of the full call" % p
    return a


def _id(case):
    return case["name"]


@pytest.mark.parametrize("case", wc.SCORE_TABLE + wc.SCORE_EDGES, ids=_id)
def test_every_instantiation_and_both_sides_of_every_dispatch_edge(cuda, case):
    _check(case, cuda)


@pytest.mark.parametrize("case", wc.SCORE_FLAVORS, ids=_id)
def test_dead_and_saturated_units_stay_finite_and_inside_the_allowance(cuda, case):
    a = _check(case, cuda)
    sc.check_extreme_inputs(case, a)


@pytest.mark.parametrize("case", wc.SCORE_CHUNK, ids=_id)
def test_batches_around_the_lds_chunk_edges(cuda, case):
    """(SW_XLDS // (n_in + 1)) rounded down to whole row blocks fit the chunk: batches of one row less, exactly, one more,
    two chunks, and three chunks and a row"""
    a = _check(case, cuda)
    shares = wc.heavy_row_shares(case, a)                    # precondition: the heavy rows at the edges cannot go unnoticed
    assert min(shares) >= 0.9, shares


@pytest.mark.parametrize("case", wc.SCORE_GRID, ids=_id)
def test_grid_stride_loops_go_round_twice(cuda, case):
    _check(case, cuda)


def test_three_inputs_through_the_wide_entry_point_are_the_narrow_entry_points_bits(cuda):
    case = sc._bnn("narrow_through_wide", 3, 65, 19, 10)
    a = sc.bnn_args(case)
    th, X, y = (torch.tensor(a[k], dtype=torch.float32, device=cuda) for k in ("theta", "X", "y"))
    outs = {}
    for name in ("stein_score_bnn", "stein_score_bnn_wide"):
        out = torch.full_like(th, float("nan"))
        _lib.call(name, th.data_ptr(), case["n"], a["d"], 3, 65, (ctypes.c_int64 * 6)(*a["cols"]), X.data_ptr(), y.data_ptr(),
                  case["B"], a["n_train"], a["ga"], a["gb"], out.data_ptr(), torch.cuda.current_stream(cuda).cuda_stream)
        torch.cuda.synchronize()
        outs[name] = out
    assert bool(torch.isfinite(outs["stein_score_bnn"]).all())
    assert _same(outs["stein_score_bnn"], outs["stein_score_bnn_wide"])
