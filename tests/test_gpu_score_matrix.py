"""GPU: every instantiation and every loop of the score kernels (csrc/stein_score.hip) against the vectorised fp64
reference of tests/score_ref.py, evaluated in torch fp64 on the device, element by element inside that reference's
a-priori fp32 allowance (a derivation, see score_ref.py; no tolerance relative to the largest entry).

The cases (tests/score_cases.py; tests/test_score_ref.py checks on the CPU that they reach every SC_LAUNCH / BNN_LAUNCH
pair, k_score_glm_few, both sides of every dispatch edge, the chunk edges and the five grid-stride caps):
  inst      one case per dispatch edge value of F / H, both GLM kinds, log alpha at varied columns, BNN blocks unsorted
  chunk     batches around one, two and three LDS chunks, with heavy rows at the chunk edges: a row dropped or staged
            twice there moves >= 90 % of the entries by >= 4 allowances (asserted from the reference alone)
  grid      n just above what one grid covers, so that every grid-stride loop goes round twice
  extreme   saturated logits, fractional labels, log precisions over [-20, 20], dead hidden units, targets of 1e4

Every case prefills the output with NaN and asserts: all finite, spare columns exactly 0, |got - ref| <= allowance
elementwise, a second call bit-identical.  Each prints max |err| / allowance (run with -s)."""
import os
import sys

import numpy as np
import pytest
import torch

from stein_amd.scores import BnnScore, GlmScore

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu
MAX_AMBIGUOUS = 0.02


def _run(case, a, cuda):
    th, X, y = (torch.tensor(a[k], dtype=torch.float32, device=cuda) for k in ("theta", "X", "y"))
    assert all(torch.equal(t.double().cpu(), torch.tensor(a[k])) for t, k in ((th, "theta"), (X, "X"), (y, "y")))
    if case["model"] == "glm":
        prod = GlmScore(a["kind"], a["F"], w_col=a["w_col"], alpha_col=None if a["alpha_col"] < 0 else a["alpha_col"],
                        n_train=a["n_train"], prior_precision=a["prior_precision"], gamma_rate=a["gamma_rate"])
        assert float(prod.n_train) / case["B"] == a["scale"]
    else:
        prod = BnnScore(a["n_in"], a["H"], a["cols"], n_train=a["n_train"], gamma_a=a["ga"], gamma_b=a["gb"])
    outs = []
    for _ in range(2):
        out = torch.full_like(th, float("nan"))
        prod(th, {"X": X, "y": y}, out=out)
        torch.cuda.synchronize()
        outs.append(out)
    return outs


def _check(case, cuda):
    a = sc.glm_args(case) if case["model"] == "glm" else sc.bnn_args(case)
    to = lambda v: torch.tensor(v, dtype=torch.float64, device=cuda)   # noqa: E731
    ref, allow, share = sc.reference(case, a, to=to)
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(allow).all())
    assert share <= MAX_AMBIGUOUS, share                     # precondition, from the reference alone
    got, again = _run(case, a, cuda)
    assert bool(torch.isfinite(got).all()), "non-finite entries (or entries never written)"
    live = torch.tensor(sc.live_columns(case, a), device=cuda)
    assert bool((got[:, ~live] == 0).all()), "a spare column is not exactly 0"
    err = (got.double() - ref).abs()
    ratio = float((err[:, live] / allow[:, live]).max())
    print("%s %-18s max |err| / allowance = %.3f   ambiguous share %.5f" % (case["model"], case["name"], ratio, share))
    bad = (err > allow).nonzero()
    assert bad.numel() == 0, "outside the allowance at (particle, column) %s ...: ratio %.3g" % (bad[:4].tolist(), ratio)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "a second call differs"
    return a


def _id(case):
    return case["name"]


@pytest.mark.parametrize("case", sc.GLM_INST, ids=_id)
def test_glm_every_instantiation(cuda, case):
    _check(case, cuda)


@pytest.mark.parametrize("case", sc.BNN_INST, ids=_id)
def test_bnn_every_instantiation(cuda, case):
    _check(case, cuda)


@pytest.mark.parametrize("case", sc.GLM_CHUNK + sc.BNN_CHUNK, ids=lambda c: c["model"] + "-" + c["name"])
def test_batches_around_the_lds_chunk_edges(cuda, case):
    """chunk_rows = SC_MAXLDS // (F + 1) rows of X (GLM; n_in + 1 for the BNN) fit the LDS of a workgroup: batches of
    chunk_rows - 1, chunk_rows, chunk_rows + 1, 2 chunk_rows and 3 chunk_rows + 1 rows."""
    a = _check(case, cuda)
    shares = sc.heavy_row_shares(case, a)                    # precondition: the heavy rows at the edges cannot go unnoticed
    assert min(shares) >= 0.9, shares


@pytest.mark.parametrize("case", sc.GLM_GRID + sc.BNN_GRID, ids=lambda c: c["model"] + "-" + c["name"])
def test_grid_stride_loops_go_round_twice(cuda, case):
    _check(case, cuda)


@pytest.mark.parametrize("case", sc.GLM_EXTREME + sc.BNN_EXTREME, ids=lambda c: c["model"] + "-" + c["name"])
def test_extreme_inputs_stay_finite_and_inside_the_allowance(cuda, case):
    a = _check(case, cuda)
    sc.check_extreme_inputs(case, a)                         # |z| near 200, dead units, log precisions at -20 and 20, ...
