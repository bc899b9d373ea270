"""GPU: the order statistics of the predictive outputs (stein_predict_glm_ranks / stein_predict_bnn_ranks of
csrc/stein_predict_ranks.hip) through the C ABI, always on a workspace filled with 0xFF bytes.

  planted     f_pb = x_b * w_p exactly (tests/quantile_cases.py): every rank 0 .. n-1, eight per call, equals np.sort of the
              products entry by entry -- the last digit of the key, ties, +-0, +-inf, NaNs last
  own pred    for every case of the table the ranks {0, 1, k, k+1, n/2, n-2, n-1} equal torch.sort of the pred that
              stein_predict_* writes for the same arguments, exactly
  fp64        an order statistic moves by at most the largest perturbation of any element, so
              |out[i][b] - sort64(f64[:, b])[r_i]| <= max_p df_pb with f64, df of tests/predict_ref.py: no new tolerance
  independence  a repeat, a zeroed workspace, permuted and repeated ranks, a rank alone or in company (for q_chunked that is
              also 4 against 3 bits a level), any particle slicing (the slices hook; one slice of 19 passes flushes its
              byte counters mid-way): the same bits
Each fp64 case prints max |err| / allowance (run with -s)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from stein_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_cases as pc  # noqa: E402
import quantile_cases as qc  # noqa: E402

pytestmark = pytest.mark.gpu


def _model_args(case, a):
    out = _lib.PRED_MEAN if case["output"] == "mean" else _lib.PRED_LINK
    if case["model"] == "bnn":
        return "bnn", lambda th, n: [th.data_ptr(), n, a["d"], case["n_in"], case["H"], (ctypes.c_int64 * 6)(*a["cols"]), out]
    kind = _lib.GLM_LINEAR if case["model"] == "linear" else _lib.GLM_LOGISTIC
    return "glm", lambda th, n: [th.data_ptr(), n, a["d"], kind, out, a["w_col"], case["F"]]


def _device(a, dev):
    return tuple(torch.tensor(a[k], dtype=torch.float32, device=dev) for k in ("theta", "X"))


def _ranks(case, a, ranks, dev, ws_byte=0xFF, tensors=None):
    """one ranks call -> out [len(ranks), B]"""
    th, X = tensors or _device(a, dev)
    n, B, R = th.shape[0], case["B"], len(ranks)
    out = torch.full((R, B), -12345.5, dtype=torch.float32, device=dev)
    ws = torch.full((_lib.predict_ranks_workspace_bytes(n, B, R),), ws_byte, dtype=torch.uint8, device=dev)
    which, head = _model_args(case, a)
    _lib.call("stein_predict_%s_ranks" % which, *head(th, n), X.data_ptr(), B, (ctypes.c_int64 * R)(*ranks), R, out.data_ptr(),
              ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return out


def _pred(case, a, dev, tensors=None):
    th, X = tensors or _device(a, dev)
    n, B = th.shape[0], case["B"]
    pred = torch.full((n, B), float("nan"), dtype=torch.float32, device=dev)
    which, head = _model_args(case, a)
    tau = [1.0] if which == "glm" else []
    _lib.call("stein_predict_%s" % which, *head(th, n), X.data_ptr(), None, B, *tau, pred.data_ptr(), None, None, None, None, 0,
              torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return pred


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


_SHARED = {}


def _case_data(case, dev):
    """inputs, device tensors and the library's own pred of a case: computed once, shared, never changed"""
    if case["name"] not in _SHARED:
        a = pc.args(case)
        tensors = _device(a, dev)
        _SHARED[case["name"]] = (a, tensors, _pred(case, a, dev, tensors))
    return _SHARED[case["name"]]


PLANT_CASE = pc._case("planted", "linear", qc.PLANT_N, qc.PLANT_B, F=1)


def _planted_args(w):
    return dict(theta=w[:, None].astype(np.float32), X=qc.PLANT_X[:, None], d=1, w_col=0)


@pytest.mark.parametrize("name", [name for name, _ in qc.planted()])
def test_planted_outputs_exact(cuda, name):
    w = dict(qc.planted())[name]
    a = _planted_args(w)
    want = np.sort(qc.planted_products(w), axis=0)                       # NaNs last
    got = np.concatenate([_ranks(PLANT_CASE, a, g, cuda).cpu().numpy() for g in qc.rank_groups(qc.PLANT_N)], axis=0)
    assert got.shape == want.shape
    for r in range(qc.PLANT_N):
        assert np.array_equal(got[r], want[r], equal_nan=True), "rank %d: %s, np.sort has %s" % (r, got[r], want[r])
    zeros = want[:, 0] == 0
    if zeros.any():                                                     # the key order: every -0 before every +0
        assert (np.diff(np.signbit(got[zeros, 0]).astype(int)) <= 0).all()
    nans = np.isnan(got)
    if nans.any():                                                      # quiet NaNs come back
        assert ((got[nans].view(np.uint32) & 0x7FC00000) == 0x7FC00000).all()


@pytest.mark.parametrize("case", qc.CASES, ids=lambda c: c["name"])
def test_against_the_librarys_own_pred_exact(cuda, case):
    a, tensors, pred = _case_data(case, cuda)
    assert bool(torch.isfinite(pred).all())
    ranks = qc.ranks_of(case["n"])
    got = _ranks(case, a, ranks, cuda, tensors=tensors)
    want = torch.sort(pred, dim=0).values[torch.tensor(ranks, device=cuda)]
    assert torch.equal(got, want), "ranks %s: %d entries differ from torch.sort of pred" % (ranks, int((got != want).sum()))


@pytest.mark.parametrize("case", [c for c in qc.CASES if pc.cpu_sized(c) or c["name"] == "q_cap"], ids=lambda c: c["name"])
def test_against_fp64_inside_the_largest_perturbation(cuda, case):
    a, tensors, _ = _case_data(case, cuda)
    to = lambda v: torch.tensor(v, dtype=torch.float64, device=cuda)   # noqa: E731
    f64, df = pc.reference(case, a, to=to)["pred"]
    ranks = qc.ranks_of(case["n"])
    got = _ranks(case, a, ranks, cuda, tensors=tensors).double()
    want = torch.sort(f64, dim=0).values[torch.tensor(ranks, device=cuda)]
    allow = df.max(0).values[None, :].expand_as(want)
    err = (got - want).abs()
    print("%-14s max |err| / allowance = %.3f" % (case["name"], float((err / allow).max())))
    assert bool((err <= allow).all()), float((err / allow).max())


def test_repeat_workspace_and_rank_sets_change_no_bit(cuda):
    for case in (qc.CASES[1], qc.CASES[2], qc.CASES[4]):   # q_chunked: 3 bits a level with seven ranks, 4 with one
        a, tensors, _ = _case_data(case, cuda)
        n = case["n"]
        ranks = qc.ranks_of(n)
        first = _ranks(case, a, ranks, cuda, tensors=tensors)
        assert _same(first, _ranks(case, a, ranks, cuda, tensors=tensors)), "a second call differs"
        assert _same(first, _ranks(case, a, ranks, cuda, ws_byte=0, tensors=tensors)), "the workspace's contents matter"
        assert _same(first, _ranks(case, a, ranks, cuda, ws_byte=0x5A, tensors=tensors))
        perm = [3, 0, 6, 6, 2, 5, 0, 1]                                # permuted, with repeats; rank 4 left out
        mixed = _ranks(case, a, [ranks[i] for i in perm], cuda, tensors=tensors)
        for row, i in enumerate(perm):
            assert _same(mixed[row], first[i]), "rank %d changes with its company" % ranks[i]
        for i, r in enumerate(ranks):                                  # alone
            assert _same(_ranks(case, a, [r], cuda, tensors=tensors)[0], first[i]), "rank %d alone differs" % r


@pytest.mark.parametrize("case", [qc.CASES[7], qc.CASES[5], PLANT_CASE], ids=lambda c: c["name"])
def test_any_particle_slicing_gives_the_same_bits(cuda, case):
    if case is PLANT_CASE:
        a = _planted_args(dict(qc.planted())["repeated"])
        tensors = _device(a, cuda)
    else:
        a, tensors, _ = _case_data(case, cuda)
    ranks = qc.ranks_of(case["n"])
    first = _ranks(case, a, ranks, cuda, tensors=tensors)
    try:
        for slices in (1, 2, 7, 1024):                                 # 1: q_flush walks 19 passes in one slice
            _lib.debug_predict_ranks_slices(slices)
            assert _same(first, _ranks(case, a, ranks, cuda, tensors=tensors)), "%d slices differ" % slices
    finally:
        _lib.debug_predict_ranks_slices(0)
